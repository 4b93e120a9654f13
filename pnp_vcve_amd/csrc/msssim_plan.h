// The plan of one MS-SSIM plane (include/pnpvcve.h, pnp_msssim_*): the dimensions of the five levels, the blocks of the level kernel
// and where a level sits in a plane's slot of the fp32 pyramid.  ONE copy of these rules, used by the entries that answer the sizing
// queries, by the launcher and inside both kernels of msssim.hip; and the step of the 2 x 2 mean pyramid that reads 8-bit planes
// through plane_load.h.  Host and device code: tests/host/msssim_stub.cpp drives the very same functions over heap blocks under
// AddressSanitizer (-DPNP_HOST_STUB: no HIP header is needed).
#pragma once
#include "plane_load.h"

#define PNP_MSSSIM_LEVELS 5
#define PNP_MSSSIM_MIN_SIZE 176     /* 11 << 4: level 4 must hold one 11 x 11 window */

struct PnpMsLevel {
    int rows, cols;         // the level's plane
    int oh, ow;             // its valid map: rows - 10, cols - 10
    int tiles_x, blocks;    // 16 x 32 tiles of the valid map
    int blk0;               // first block of the level among the plane's blocks
    int64_t ws_off;         // floats from the start of the plane's pyramid slot (levels 1..4; -1 for level 0, which is the source)
};

struct PnpMsPlan {
    PnpMsLevel lv[PNP_MSSSIM_LEVELS];
    int blocks;             // all levels
    int ok;                 // 0: the plane cannot be scored (every other field is 0 then)
    int64_t ws_floats;      // floats of one plane's pyramid slot: levels 1..4, each rounded up to a multiple of 4 floats
};

// rows x cols: the plane before the crop; crop: the samples cut from each of its sides at level 0
PNP_PLANE_HD PnpMsPlan pnp_ms_plan(int rows, int cols, int crop) {
    PnpMsPlan p;
    p.blocks = 0, p.ok = 0, p.ws_floats = 0;
    for (int s = 0; s < PNP_MSSSIM_LEVELS; ++s) {
        PnpMsLevel& l = p.lv[s];
        l.rows = l.cols = l.oh = l.ow = l.tiles_x = l.blocks = l.blk0 = 0;
        l.ws_off = -1;
    }
    if (rows < 1 || cols < 1 || crop < 0 || crop >= rows || crop >= cols) return p;
    int r = (int)((int64_t)rows - 2 * (int64_t)crop), c = (int)((int64_t)cols - 2 * (int64_t)crop);
    if (r < PNP_MSSSIM_MIN_SIZE || c < PNP_MSSSIM_MIN_SIZE) return p;
    for (int s = 0; s < PNP_MSSSIM_LEVELS; ++s) {
        PnpMsLevel& l = p.lv[s];
        l.rows = r, l.cols = c;
        l.oh = r - 10, l.ow = c - 10;
        l.tiles_x = (l.ow + 31) / 32;
        l.blocks = ((l.oh + 15) / 16) * l.tiles_x;
        l.blk0 = p.blocks;
        p.blocks += l.blocks;
        if (s) {
            l.ws_off = p.ws_floats;
            p.ws_floats += ((int64_t)r * c + 3) & ~(int64_t)3;
        }
        r /= 2, c /= 2;         // an odd last row or column is dropped
    }
    p.ok = 1;
    return p;
}

// One sample of the next level: the mean of a 2 x 2 square, formed in fp64 and stored as fp32.  Exact for integer samples of up to 22
// bits (no rounding at all); for fp32 samples this expression IS the definition.
PNP_PLANE_HD float pnp_ms_mean4(float x00, float x01, float x10, float x11) {
    return (float)((((double)x00 + (double)x01) + ((double)x10 + (double)x11)) * 0.25);
}

// Level 1 from an 8-bit plane: samples 2 gx and 2 gx + 1 (ncol = 1 | 2 of them) of row r of level 1 of frame f, read as ONE group of
// 2 ncol samples from each of the rows crop + 2 r and crop + 2 r + 1 of the plane, at column crop + 4 gx, through pnp_plane_load4 (so
// the reading rule of the 4:2:0 boundary holds: dwords where they lie inside the plane's rows, bytes elsewhere).  sel: the plane is
// the second of an interleaved pair.  -> how many of the two fetches were dword fetches.
PNP_PLANE_HD int pnp_ms_down_plane8(const PnpPlaneSrc& s, int sel, int64_t f, int crop, int r, int gx, int ncol, float out[2]) {
    unsigned w0[2], w1[2];
    const int f0 = pnp_plane_load4(s, f, crop + 2 * r, crop + 4 * gx, 2 * ncol, w0);
    const int f1 = pnp_plane_load4(s, f, crop + 2 * r + 1, crop + 4 * gx, 2 * ncol, w1);
    const unsigned t = sel ? w0[1] : w0[0], b = sel ? w1[1] : w1[0];
    out[0] = pnp_ms_mean4((float)(t & 255u), (float)((t >> 8) & 255u), (float)(b & 255u), (float)((b >> 8) & 255u));
    out[1] = ncol > 1 ? pnp_ms_mean4((float)((t >> 16) & 255u), (float)(t >> 24), (float)((b >> 16) & 255u), (float)(b >> 24)) : 0.f;
    return f0 + f1;
}
