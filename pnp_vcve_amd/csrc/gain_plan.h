// The plan of the enhancement gain (include/pnpvcve.h, pnp_gain_*): the region of one plane after the crop, the grid of gain cells, which
// cell a sample belongs to, how many samples of a cell lie in the region, and the tiles the kernel of gain.hip cuts a plane into.  ONE
// copy of these rules, used by the entries that answer the queries, by the launcher and inside the kernel, so that they cannot disagree.
// Integers only.  Host and device code: tests/host/gain_stub.cpp drives the very same functions under AddressSanitizer / UBSan
// (-DPNP_HOST_STUB: no HIP header is needed).
#pragma once
#include "plane_load.h"

// A thread block of gain_kernel owns one tile: PNP_GAIN_TILE_W columns (a wave of 64 lanes, four samples a lane) of ONE row of cells,
// anchored at the UNCROPPED plane's origin as the cells are.  A cell is a multiple of four samples wide in every plane (8 at the least:
// the chroma of block 16), so a lane's four samples share a cell and a tile holds whole cells only: every cell belongs to one tile.
#define PNP_GAIN_TILE_W 256
#define PNP_GAIN_MAX_CELLS (PNP_GAIN_TILE_W / 8)    // cells of a tile at the most

struct PnpGainPlane {
    int rows, cols;         // the plane before the crop: the cell grid is anchored at ITS origin
    int bh, bw;             // a cell of this plane: block / sy rows, block / sx columns
    int y0, y1, x0, x1;     // the region: rows [y0, y1), columns [x0, x1)
    int grows, gcols;       // the grid: ceil(rows / bh) x ceil(cols / bw), the same for every plane of a format
    int tiles_x;            // tiles across; there are grows rows of them
    int ok;                 // 0: nothing can be scored (every other field is 0 then)
};

PNP_PLANE_HD int pnp_gain_block_ok(int block) { return block == 16 || block == 32 || block == 64 || block == 128; }

// the grid of h x w frames: ceil(h / block) rows, ceil(w / block) columns
PNP_PLANE_HD void pnp_gain_grid_of(int h, int w, int block, int& grows, int& gcols) {
    grows = (h + block - 1) / block;
    gcols = (w + block - 1) / block;
}

// The plane of an h x w frame that the factors (sx, sy) subsample (1, 1 for Y and for frames of pixels), cropped by crop / sy down and
// crop / sx across; sx divides w and sy divides h.
PNP_PLANE_HD PnpGainPlane pnp_gain_plane(int h, int w, int crop, int block, int sx, int sy) {
    PnpGainPlane p;
    p.rows = p.cols = p.bh = p.bw = p.y0 = p.y1 = p.x0 = p.x1 = p.grows = p.gcols = p.tiles_x = p.ok = 0;
    if (h < 1 || w < 1 || crop < 0 || 2 * (int64_t)crop >= h || 2 * (int64_t)crop >= w || !pnp_gain_block_ok(block)) return p;
    if (sx < 1 || sx > 2 || sy < 1 || sy > 2 || h % sy || w % sx) return p;
    const int rows = h / sy, cols = w / sx, cy = crop / sy, cx = crop / sx;
    if (2 * cy >= rows || 2 * cx >= cols) return p;
    p.rows = rows, p.cols = cols, p.bh = block / sy, p.bw = block / sx;
    p.y0 = cy, p.y1 = rows - cy, p.x0 = cx, p.x1 = cols - cx;
    pnp_gain_grid_of(h, w, block, p.grows, p.gcols);
    p.tiles_x = (cols + PNP_GAIN_TILE_W - 1) / PNP_GAIN_TILE_W;
    p.ok = 1;
    return p;
}

// the cell of sample (y, x) of the plane: row i, column j of the grid
PNP_PLANE_HD void pnp_gain_cell_of(const PnpGainPlane& p, int y, int x, int& i, int& j) {
    i = y / p.bh;
    j = x / p.bw;
}

// samples of [k * b, (k + 1) * b) inside [lo, hi): 0 when the cell's extent lies in the crop (or beyond the plane)
PNP_PLANE_HD int pnp_gain_overlap(int k, int b, int lo, int hi) {
    const int a = k * b > lo ? k * b : lo, e = (k + 1) * b < hi ? (k + 1) * b : hi;
    return e > a ? e - a : 0;
}

// samples of cell (i, j) inside the region, in closed form
PNP_PLANE_HD int64_t pnp_gain_cell_samples(const PnpGainPlane& p, int i, int j) {
    return (int64_t)pnp_gain_overlap(i, p.bh, p.y0, p.y1) * pnp_gain_overlap(j, p.bw, p.x0, p.x1);
}

PNP_PLANE_HD int pnp_gain_tiles(const PnpGainPlane& p) { return p.tiles_x * p.grows; }

// Tile `tile` (0 .. pnp_gain_tiles - 1) is tile column tx of cell row ti.  Its rows inside the region are [r0, r1) (empty when
// r1 <= r0: the cell row lies in the crop); its first cell is column j0 of the grid and it holds ncell of them.
PNP_PLANE_HD void pnp_gain_tile(const PnpGainPlane& p, int tile, int& ti, int& tx, int& r0, int& r1, int& j0, int& ncell) {
    ti = tile / p.tiles_x;
    tx = tile - ti * p.tiles_x;
    r0 = ti * p.bh > p.y0 ? ti * p.bh : p.y0;
    r1 = (ti + 1) * p.bh < p.y1 ? (ti + 1) * p.bh : p.y1;
    j0 = tx * (PNP_GAIN_TILE_W / p.bw);
    ncell = p.gcols - j0 < PNP_GAIN_TILE_W / p.bw ? p.gcols - j0 : PNP_GAIN_TILE_W / p.bw;
}

// Lane `lane` (0 .. 63) of tile column tx owns the samples [col, col + n) of every row of the tile (n <= 0: none): what is left of its
// four columns inside the region.  They lie in cell `cell` of the tile (0 .. ncell - 1 wherever n > 0); the lanes of a cell are
// p.bw / 4 consecutive ones.
PNP_PLANE_HD void pnp_gain_lane_cols(const PnpGainPlane& p, int tx, int lane, int& col, int& n, int& cell) {
    const int c0 = tx * PNP_GAIN_TILE_W + 4 * lane;
    col = c0 > p.x0 ? c0 : p.x0;
    n = (c0 + 4 < p.x1 ? c0 + 4 : p.x1) - col;
    cell = 4 * lane / p.bw;
}
