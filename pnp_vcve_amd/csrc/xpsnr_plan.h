// The plan of XPSNR (include/pnpvcve.h, pnp_xpsnr_*): the block size N, the block grid of the cropped luma plane, a block's bounds, its
// chroma block, its activity region and the border b that chooses the spatial filter.  ONE copy of these rules, used by the entries that
// answer the queries, by the launcher and inside the kernel of xpsnr.hip.  Everything is integer arithmetic (no sqrt: the rounding of
// N is decided by comparing squares), so host and device cannot disagree.  Host and device code: tests/host/xpsnr_stub.cpp drives the
// very same functions under AddressSanitizer / UBSan (-DPNP_HOST_STUB: no HIP header is needed).
#pragma once
#include "plane_load.h"

struct PnpXpPlan {
    int H, W;               // the cropped luma plane
    int crop;               // samples cut from each side of the luma plane (even; half of it on chroma)
    int N;                  // block size: a multiple of 4, >= 4
    int rows, cols;         // blocks: ceil(H / N) x ceil(W / N)
    int b;                  // border of the activity filters: 1 (3 x 3 filter, every sample) | 2 (6 x 6 filter, every second sample)
    int ok;                 // 0: nothing can be scored (every other field is 0 then)
};

// [y0, y1) x [x0, x1): a block of the luma plane, or its activity region (which may be empty: y1 <= y0 or x1 <= x0)
struct PnpXpRect {
    int y0, y1, x0, x1;
};

// N = max(4, 4 * floor(32 * sqrt(W H / (3840 * 2160)) + 0.5)) for a cropped plane of H x W samples.  floor(32 sqrt(q) + 0.5) is the
// largest k with (k - 0.5)^2 <= 1024 q, i.e. (2k - 1)^2 * 3840 * 2160 <= 4096 * W * H: decided in 64-bit integers.
PNP_PLANE_HD int pnp_xp_block_size(int H, int W) {
    const uint64_t area = (uint64_t)H * (uint64_t)W;       // H, W < 2^31 / ... : the entries refuse planes whose 4096 * area leaves 64 bits
    uint64_t k = 0;
    while ((2 * k + 1) * (2 * k + 1) * 8294400ull <= 4096ull * area) ++k;
    return k < 1 ? 4 : (int)(4 * k);
}

// h x w: the luma plane before the crop
PNP_PLANE_HD PnpXpPlan pnp_xp_plan(int h, int w, int crop) {
    PnpXpPlan p;
    p.H = p.W = p.crop = p.N = p.rows = p.cols = p.b = p.ok = 0;
    if (h < 2 || w < 2 || (h & 1) || (w & 1) || crop < 0 || (crop & 1) || 2 * (int64_t)crop >= h || 2 * (int64_t)crop >= w) return p;
    if (h > (1 << 24) || w > (1 << 24)) return p;           // 4096 * H * W stays far inside 64 bits
    p.H = h - 2 * crop, p.W = w - 2 * crop, p.crop = crop;
    p.N = pnp_xp_block_size(p.H, p.W);
    p.rows = (p.H + p.N - 1) / p.N;
    p.cols = (p.W + p.N - 1) / p.N;
    p.b = (int64_t)p.W * p.H > 2048 * 1152 ? 2 : 1;
    p.ok = 1;
    return p;
}

// block k = by * cols + bx of the cropped luma plane, clipped at the plane's edge; every bound is even
PNP_PLANE_HD PnpXpRect pnp_xp_block(const PnpXpPlan& p, int by, int bx) {
    PnpXpRect r;
    r.y0 = by * p.N, r.x0 = bx * p.N;
    r.y1 = r.y0 + p.N < p.H ? r.y0 + p.N : p.H;
    r.x1 = r.x0 + p.N < p.W ? r.x0 + p.N : p.W;
    return r;
}

// the chroma block of a luma block: exact halves
PNP_PLANE_HD PnpXpRect pnp_xp_chroma(const PnpXpRect& k) {
    PnpXpRect r;
    r.y0 = k.y0 / 2, r.y1 = k.y1 / 2, r.x0 = k.x0 / 2, r.x1 = k.x1 / 2;
    return r;
}

// The activity region of block k of an H x W plane with border b: the block without the b samples next to the PICTURE's edge.  The
// filters read across block edges (b samples before the region, b -- 3 x 3 -- or 3 -- 6 x 6, from an even position -- behind its last
// position) but never across the picture's edge.
PNP_PLANE_HD PnpXpRect pnp_xp_region(const PnpXpRect& k, int H, int W, int b) {
    PnpXpRect r;
    r.y0 = k.y0 > 0 ? k.y0 : b;
    r.y1 = k.y1 < H ? k.y1 : H - b;
    r.x0 = k.x0 > 0 ? k.x0 : b;
    r.x1 = k.x1 < W ? k.x1 : W - b;
    return r;
}

PNP_PLANE_HD int pnp_xp_empty(const PnpXpRect& r) { return r.y1 <= r.y0 || r.x1 <= r.x0; }

// rows * cols of a region, 0 when it is empty
PNP_PLANE_HD int64_t pnp_xp_area(const PnpXpRect& r) { return pnp_xp_empty(r) ? 0 : (int64_t)(r.y1 - r.y0) * (r.x1 - r.x0); }

// The rows (or columns) the filter at position `pos` of a region reads: [pos - b, pos + (b == 1 ? 1 : 3)].  The stub checks these
// against the plane for every position the kernel visits.
PNP_PLANE_HD int pnp_xp_read_lo(int pos, int b) { return pos - b; }
PNP_PLANE_HD int pnp_xp_read_hi(int pos, int b) { return pos + (b == 1 ? 1 : 3); }

// The lanes that share one block: 4, 16, 64 or the whole thread block of 256, the smallest of them that is no less than the N * N / 4
// groups of four luma samples of a full block -- so that N = 4 puts 64 blocks into a thread block and N = 8 sixteen.
PNP_PLANE_HD int pnp_xp_lanes(int N) {
    const int groups = N * N / 4;
    return groups <= 4 ? 4 : (groups <= 16 ? 16 : (groups <= 64 ? 64 : 256));
}
