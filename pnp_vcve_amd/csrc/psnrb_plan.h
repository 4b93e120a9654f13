// The plan of PSNR-B (include/pnpvcve.h, pnp_psnrb_*): the region of one plane after the crop, which neighbour pairs are block-boundary
// pairs, how many pairs of each kind exist, and the tiles the kernel of psnrb.hip cuts the region into.  ONE copy of these rules, used by
// the entries that answer the queries, by the launcher and inside the kernel, so that they cannot disagree.  Integers only.  Host and
// device code: tests/host/psnrb_stub.cpp drives the very same functions under AddressSanitizer / UBSan (-DPNP_HOST_STUB: no HIP header
// is needed).
#pragma once
#include "plane_load.h"

// A thread block of psnrb_kernel owns one tile of the region: PNP_PB_TILE_W columns (a wave of 64 lanes, four samples a lane) by
// PNP_PB_TILE_H rows (the block's four waves, PNP_PB_WAVE_ROWS rows each), anchored at the region's first sample.
#define PNP_PB_TILE_W 256
#define PNP_PB_WAVE_ROWS 8
#define PNP_PB_TILE_H (4 * PNP_PB_WAVE_ROWS)

struct PnpPbPlane {
    int rows, cols;         // the plane before the crop: the block grid is anchored at ITS origin
    int bp;                 // block size of the plane: a power of two
    int y0, y1, x0, x1;     // the region: rows [y0, y1), columns [x0, x1)
    int tiles_x, tiles_y;   // tiles of the region
    int ok;                 // 0: nothing can be scored (every other field is 0 then)
};

PNP_PLANE_HD int pnp_pb_block_ok(int bp, int lo, int hi) { return bp >= lo && bp <= hi && (bp & (bp - 1)) == 0; }

// a plane of rows x cols samples cropped by `crop` on every side, blocks of bp x bp (2 .. 64, a power of two); needs min(h, w) >= bp
PNP_PLANE_HD PnpPbPlane pnp_pb_plane(int rows, int cols, int crop, int bp) {
    PnpPbPlane p;
    p.rows = p.cols = p.bp = p.y0 = p.y1 = p.x0 = p.x1 = p.tiles_x = p.tiles_y = p.ok = 0;
    if (rows < 1 || cols < 1 || crop < 0 || 2 * (int64_t)crop >= rows || 2 * (int64_t)crop >= cols || !pnp_pb_block_ok(bp, 2, 64)) return p;
    const int h = rows - 2 * crop, w = cols - 2 * crop;
    if (h < bp || w < bp) return p;
    p.rows = rows, p.cols = cols, p.bp = bp;
    p.y0 = crop, p.y1 = rows - crop, p.x0 = crop, p.x1 = cols - crop;
    p.tiles_x = (w + PNP_PB_TILE_W - 1) / PNP_PB_TILE_W;
    p.tiles_y = (h + PNP_PB_TILE_H - 1) / PNP_PB_TILE_H;
    p.ok = 1;
    return p;
}

// The pair (i, i + 1) along one axis -- (y, x), (y, x + 1) or (y, x), (y + 1, x) -- is a block-boundary pair iff i + 1 is a multiple of bp.
PNP_PLANE_HD int pnp_pb_boundary(int i, int bp) { return ((i + 1) & (bp - 1)) == 0; }

// boundary pairs along an axis whose samples [lo, hi) are in the region: the multiples of bp in [lo + 1, hi - 1]
PNP_PLANE_HD int pnp_pb_crossings(int lo, int hi, int bp) { return (hi - 1) / bp - lo / bp; }

// counts[4] = NBh, NNh, NBv, NNv: the horizontal boundary / other and the vertical boundary / other pairs that exist in the region
PNP_PLANE_HD void pnp_pb_counts(const PnpPbPlane& p, int64_t counts[4]) {
    const int64_t h = p.y1 - p.y0, w = p.x1 - p.x0;
    const int64_t kx = pnp_pb_crossings(p.x0, p.x1, p.bp), ky = pnp_pb_crossings(p.y0, p.y1, p.bp);
    counts[0] = h * kx;
    counts[1] = h * (w - 1 - kx);
    counts[2] = w * ky;
    counts[3] = w * (h - 1 - ky);
}

// The rows wave `wave` (0 .. 3) of tile row ty owns, [r0, r1) (empty when r1 <= r0); it also READS row r1 of the test clip when
// r1 < y1: the vertical pair (r1 - 1, r1) belongs to its top sample.
PNP_PLANE_HD void pnp_pb_wave_rows(const PnpPbPlane& p, int ty, int wave, int& r0, int& r1) {
    r0 = p.y0 + ty * PNP_PB_TILE_H + wave * PNP_PB_WAVE_ROWS;
    r1 = r0 + PNP_PB_WAVE_ROWS < p.y1 ? r0 + PNP_PB_WAVE_ROWS : p.y1;
}

// The group of four samples lane `lane` (0 .. 63) of tile column tx owns in every row: its first column and how many of the four lie
// in the region (<= 0: none).  The lane also needs sample col + 4 of the test clip when that lies in the region: the horizontal pair
// (col + 3, col + 4) belongs to its left sample.
PNP_PLANE_HD void pnp_pb_lane_cols(const PnpPbPlane& p, int tx, int lane, int& col, int& n) {
    col = p.x0 + tx * PNP_PB_TILE_W + 4 * lane;
    n = p.x1 - col < 4 ? p.x1 - col : 4;
}
