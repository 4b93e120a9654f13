// The per-frame fold table of the Winograd front halves (conv_wino.hip, fold-only body): one 8-byte record per 8x8 quadrant of a frame,
// made by one small launch (conv_persist.hip: launch_par_fold_table) in front of a branch run and read a tile ahead by the run's 16
// front halves, instead of each of them deriving it again, tile by tile, from the partition planes.
//
// A record says which plane the fold-only body folds into the weights of the quadrant and with which factor, exactly as that body
// derived both itself from the quadrant's first pixel: plane = the lowest j with par_j(first pixel) != 0, or -1 when all three are
// zero or the quadrant lies outside the frame (a quadrant cut by the frame's edge has its first pixel inside: it counts with the
// pixels it has, like bit 6 of the tile flags); factor = 0.25f * par_plane(first pixel), one fp32 product, 0 for plane -1.  The
// record means something to the kernels only on a frame that passed the gate (bit 3 of the frame's partition word: every quadrant
// all zero or one constant plane); on any other frame it still holds what this rule gives.
//
// Layout: tile-major, the four quadrants of a 16x16 tile side by side in wave order (wave w of the tile kernel owns quadrant
// (w >> 1, w & 1)), so a block reads its tile's records from one block-uniform address.  Tiles cover the frame rounded up to 16: the
// quadrants beyond it are there and empty.  Host and device code, no HIP needed: the host tests restate the rule against this file.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(PNP_HOST_STUB)
#define PNP_FOLD_HD __host__ __device__
#else
#define PNP_FOLD_HD
#endif

struct PnpFoldRec {
    int plane;               // 0..2, or -1: nothing to fold
    unsigned factor_bits;    // the bits of the fp32 factor 0.25f * value
};

// records (8 bytes each) of one frame
static inline PNP_FOLD_HD long pnp_fold_records(int H, int W) { return 4L * ((W + 15) / 16) * ((H + 15) / 16); }

// the record of quadrant (qy, qx) = pixels [8 qy, 8 qy + 8) x [8 qx, 8 qx + 8); tiles_x = (W + 15) / 16
static inline PNP_FOLD_HD long pnp_fold_index(int qy, int qx, int tiles_x) {
    return ((long)(qy >> 1) * tiles_x + (qx >> 1)) * 4 + (qy & 1) * 2 + (qx & 1);
}

// from the three plane values of the quadrant's first pixel (zeros for a quadrant outside the frame)
static inline PNP_FOLD_HD PnpFoldRec pnp_fold_record(float v0, float v1, float v2) {
    PnpFoldRec r;
    r.plane = -1;
    float f = 0.f;
    if (v2 != 0.f) { r.plane = 2; f = 0.25f * v2; }
    if (v1 != 0.f) { r.plane = 1; f = 0.25f * v1; }
    if (v0 != 0.f) { r.plane = 0; f = 0.25f * v0; }
#if defined(__HIP_DEVICE_COMPILE__)
    r.factor_bits = __float_as_uint(f);
#else
    memcpy(&r.factor_bits, &f, 4);
#endif
    return r;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// the whole table of one frame on the host (what the kernel writes; tests and tools): par = 3 planes of H x W floats, `plane` floats apart
static inline void pnp_fold_table_host(const float* par, long plane, int H, int W, PnpFoldRec* tab) {
    const int tiles_x = (W + 15) / 16, qrows = 2 * ((H + 15) / 16), qcols = 2 * tiles_x;
    for (int qy = 0; qy < qrows; ++qy)
        for (int qx = 0; qx < qcols; ++qx) {
            const bool in = 8 * qy < H && 8 * qx < W;
            const long px = (long)8 * qy * W + 8 * qx;
            tab[pnp_fold_index(qy, qx, tiles_x)] = in ? pnp_fold_record(par[px], par[plane + px], par[2 * plane + px]) : pnp_fold_record(0.f, 0.f, 0.f);
        }
}
#endif
