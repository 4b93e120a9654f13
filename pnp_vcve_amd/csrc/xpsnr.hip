// XPSNR of 4:2:0 clips at 8 to 12 bit (include/pnpvcve.h, pnp_xpsnr_*): per frame and block of the data-dependent block grid, the exact
// integer squared error of the Y, Cb and Cr planes and the spatial and temporal activity of the ORIGINAL's luma.  Integers only: the
// weights, the sums over blocks and the logarithm are the host's (fp64, written once), so the device and a restatement cannot differ
// in rounding.  One launch covers all frames and blocks; frames t - 1 and t - 2 of the original are read again by the block that needs
// them, there is no workspace.  xpsnr_plan.h holds the grid, the regions and the chroma mapping; metric_src.h fetches the samples.
#include "metric_src.h"
#include "xpsnr_plan.h"

namespace {

// metric_src.h::plane_load4 (samples (row, col ..) of frame f, 0 beyond n) for 1 <= n <= 8
template <bool S16>
__device__ __forceinline__ void xp_load8(const PlaneSamp& s, long f, int row, int col, int n, int v[8]) {
    plane_load4<S16>(s, f, row, col, n < 4 ? n : 4, v);
    if (n > 4) {
        plane_load4<S16>(s, f, row, col + 4, n - 4, v + 4);
    } else {
#pragma unroll
        for (int j = 4; j < 8; ++j) v[j] = 0;
    }
}

struct XpArgs {
    PlaneSamp a[3], b[3];           // the test clip and the original: Y, Cb, Cr (clip_planes)
    PnpXpPlan plan;
    int mask, fps;
    int lanes, lanes_log2;          // pnp_xp_lanes(N): the lanes that share one block
    unsigned long long* sums;       // [frames][rows * cols][5]: sse_y, sse_u, sse_v, sa, ta
};

// the squared error of two planes over rect k (coordinates of the cropped plane), a group of four samples of a row per lane and step
template <bool S16>
__device__ __forceinline__ unsigned long long xp_sse(const PlaneSamp& a, const PlaneSamp& b, long f, const PnpXpRect& k, int crop, int lane, int lanes) {
    const int g = (k.x1 - k.x0 + 3) / 4, items = (k.y1 - k.y0) * g;
    unsigned long long acc = 0;
    for (int i = lane; i < items; i += lanes) {
        const int r = i / g, x = k.x0 + 4 * (i - r * g);
        const int n = k.x1 - x < 4 ? k.x1 - x : 4;
        int va[4], vb[4];
        plane_load4<S16>(a, f, crop + k.y0 + r, crop + x, n, va);
        plane_load4<S16>(b, f, crop + k.y0 + r, crop + x, n, vb);
#pragma unroll
        for (int j = 0; j < 4; ++j) {                       // absent samples are 0 in both
            const int d = va[j] - vb[j];
            acc += (unsigned)(d * d);
        }
    }
    return acc;
}

// b = 1: every sample of region R is a position; the 3 x 3 filter 12 / -2 / -1; s_t is the sample.  A lane takes four positions of a
// row: the six samples around them from three rows, and the four of the one or two frames before.
template <bool S16>
__device__ __forceinline__ void xp_activity1(const PlaneSamp& o, long f, const PnpXpRect& R, int crop, int order, int lane, int lanes,
                                             unsigned long long& sa, unsigned long long& ta) {
    const int g = (R.x1 - R.x0 + 3) / 4, items = (R.y1 - R.y0) * g;
    for (int i = lane; i < items; i += lanes) {
        const int r = i / g, y = R.y0 + r, x = R.x0 + 4 * (i - r * g);
        const int np = R.x1 - x < 4 ? R.x1 - x : 4;
        int v[3][8];
#pragma unroll
        for (int q = 0; q < 3; ++q) xp_load8<S16>(o, f, crop + y - 1 + q, crop + x - 1, np + 2, v[q]);
        int p1[4] = {0, 0, 0, 0}, p2[4] = {0, 0, 0, 0};
        if (order >= 1) plane_load4<S16>(o, f - 1, crop + y, crop + x, np, p1);
        if (order == 2) plane_load4<S16>(o, f - 2, crop + y, crop + x, np, p2);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j < np) {
                const int c = v[1][j + 1];
                const int e = 12 * c - 2 * (v[1][j] + v[1][j + 2] + v[0][j + 1] + v[2][j + 1]) - (v[0][j] + v[0][j + 2] + v[2][j] + v[2][j + 2]);
                sa += (unsigned)(e < 0 ? -e : e);
                const int d = order == 2 ? c - 2 * p1[j] + p2[j] : (order == 1 ? c - p1[j] : 0);
                ta += (unsigned)(d < 0 ? -d : d);
            }
        }
    }
}

// b = 2: every second row and column of region R, from its first, is a position; the 6 x 6 zero-sum filter over rows and columns
// -2 .. +3; s_t is the sum of the 2 x 2 samples at the position.  A lane takes two neighbouring positions: eight samples of six rows.
template <bool S16>
__device__ __forceinline__ void xp_activity2(const PlaneSamp& o, long f, const PnpXpRect& R, int crop, int order, int lane, int lanes,
                                             unsigned long long& sa, unsigned long long& ta) {
    constexpr int K6[6][6] = {{0, -1, -1, -1, -1, 0}, {-1, -2, -3, -3, -2, -1}, {-1, -3, 12, 12, -3, -1},
                              {-1, -3, 12, 12, -3, -1}, {-1, -2, -3, -3, -2, -1}, {0, -1, -1, -1, -1, 0}};
    const int prow = (R.y1 - R.y0 + 1) / 2, pcol = (R.x1 - R.x0 + 1) / 2;
    const int g = (pcol + 1) / 2, items = prow * g;
    for (int i = lane; i < items; i += lanes) {
        const int r = i / g, gx = i - r * g;
        const int y = R.y0 + 2 * r, x = R.x0 + 4 * gx;
        const int np = pcol - 2 * gx < 2 ? 1 : 2;
        int v[6][8];
#pragma unroll
        for (int q = 0; q < 6; ++q) xp_load8<S16>(o, f, crop + y - 2 + q, crop + x - 2, 4 + 2 * np, v[q]);
        int p1[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}}, p2[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            if (order >= 1) plane_load4<S16>(o, f - 1, crop + y + q, crop + x, 2 * np, p1[q]);
            if (order == 2) plane_load4<S16>(o, f - 2, crop + y + q, crop + x, 2 * np, p2[q]);
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (j < np) {
                int e = 0;
#pragma unroll
                for (int q = 0; q < 6; ++q)
#pragma unroll
                    for (int c = 0; c < 6; ++c) e += K6[q][c] * v[q][2 * j + c];
                sa += (unsigned)(e < 0 ? -e : e);
                const int s0 = v[2][2 * j + 2] + v[2][2 * j + 3] + v[3][2 * j + 2] + v[3][2 * j + 3];
                const int s1 = p1[0][2 * j] + p1[0][2 * j + 1] + p1[1][2 * j] + p1[1][2 * j + 1];
                const int s2 = p2[0][2 * j] + p2[0][2 * j + 1] + p2[1][2 * j] + p2[1][2 * j + 1];
                const int d = order == 2 ? s0 - 2 * s1 + s2 : (order == 1 ? s0 - s1 : 0);
                ta += (unsigned)(d < 0 ? -d : d);
            }
        }
    }
}

// A thread block of 256 owns 256 / lanes whole XPSNR blocks, `lanes` consecutive threads each (64 blocks when N = 4, 16 when N = 8,
// one from N = 20 on), so a wave is busy whatever N.  Sums go registers -> shuffles within the block's lanes, or (a block shared by
// four waves) metric_src.h::block_sums -> plain stores of the five totals.  No atomics: every slot has one writer and every slot is written, the planes
// outside the mask as 0.
template <bool S16>
__global__ __launch_bounds__(256) void xpsnr_kernel(const XpArgs s) {
    __shared__ unsigned long long red[4][5];
    const PnpXpPlan& p = s.plan;
    const int lanes = s.lanes, sub = threadIdx.x >> s.lanes_log2, lane = threadIdx.x & (lanes - 1);
    const long frame = blockIdx.y;
    const int nblk = p.rows * p.cols;
    const int kb = (int)blockIdx.x * (256 >> s.lanes_log2) + sub;
    unsigned long long acc[5] = {0, 0, 0, 0, 0};
    if (kb < nblk) {
        const int by = kb / p.cols, bx = kb - by * p.cols;
        const PnpXpRect k = pnp_xp_block(p, by, bx);
        if (s.mask & PNP_PLANE_Y) acc[0] = xp_sse<S16>(s.a[0], s.b[0], frame, k, p.crop, lane, lanes);
        const PnpXpRect kc = pnp_xp_chroma(k);
        if (s.mask & PNP_PLANE_CB) acc[1] = xp_sse<S16>(s.a[1], s.b[1], frame, kc, p.crop >> 1, lane, lanes);
        if (s.mask & PNP_PLANE_CR) acc[2] = xp_sse<S16>(s.a[2], s.b[2], frame, kc, p.crop >> 1, lane, lanes);
        const PnpXpRect R = pnp_xp_region(k, p.H, p.W, p.b);
        const int order = frame == 0 ? 0 : (s.fps >= 32 && frame >= 2 ? 2 : 1);
        if (!pnp_xp_empty(R)) {
            if (p.b == 1) xp_activity1<S16>(s.b[0], frame, R, p.crop, order, lane, lanes, acc[3], acc[4]);
            else xp_activity2<S16>(s.b[0], frame, R, p.crop, order, lane, lanes, acc[3], acc[4]);
        }
    }
    unsigned long long* out = s.sums + ((long)frame * nblk + kb) * 5;
    if (lanes <= 64) {                                          // (the same for the whole thread block)
#pragma unroll
        for (int q = 0; q < 5; ++q)
            for (int off = lanes >> 1; off > 0; off >>= 1) acc[q] += __shfl_down(acc[q], off, lanes);
        if (kb < nblk && lane == 0) {
#pragma unroll
            for (int q = 0; q < 5; ++q) out[q] = acc[q];
        }
        return;
    }
    const unsigned long long v = block_sums(acc, red);
    if (kb < nblk && threadIdx.x < 5) out[threadIdx.x] = v;
}

template <bool S16>
int launch(XpArgs& s, int mask, int fps, unsigned long long* sums, int frames, hipStream_t st) {
    s.mask = mask, s.fps = fps, s.sums = sums;
    s.lanes = pnp_xp_lanes(s.plan.N);
    s.lanes_log2 = 0;
    while ((1 << s.lanes_log2) < s.lanes) ++s.lanes_log2;
    const int per = 256 / s.lanes, nblk = s.plan.rows * s.plan.cols;
    hipLaunchKernelGGL(xpsnr_kernel<S16>, dim3((unsigned)((nblk + per - 1) / per), (unsigned)frames), dim3(256), 0, st, s);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" int pnp_xpsnr_block_size(int h, int w, int crop_border) { return pnp_xp_plan(h, w, crop_border).N; }

extern "C" int pnp_xpsnr_grid(int h, int w, int crop_border, int* rows, int* cols) {
    const PnpXpPlan p = pnp_xp_plan(h, w, crop_border);
    if (!p.ok || !rows || !cols) return PNP_ERR_BAD_ARG;
    *rows = p.rows;
    *cols = p.cols;
    return PNP_OK;
}

extern "C" int pnp_xpsnr_sums_yuv420(const pnp_yuv420_planes* a, const pnp_yuv420_planes* b, int plane_mask, unsigned long long* sums,
                                     int frames, int h, int w, int crop_border, int fps, void* stream) {
    if (!planes_args_ok(a, b, sums, frames, h, w, crop_border) || !plane_mask_ok(plane_mask) || fps < 1) return PNP_ERR_BAD_ARG;
    XpArgs s;
    s.plan = pnp_xp_plan(h, w, crop_border);
    if (!s.plan.ok) return PNP_ERR_BAD_ARG;
    clip_planes(*a, h, w, PNP_YUV_FORMAT_420, s.a);
    clip_planes(*b, h, w, PNP_YUV_FORMAT_420, s.b);
    return launch<false>(s, plane_mask, fps, sums, frames, (hipStream_t)stream);
}

extern "C" int pnp_xpsnr_sums_yuv420p16(const pnp_yuv420_planes16* a, const pnp_yuv420_planes16* b, int plane_mask, unsigned long long* sums,
                                        int frames, int h, int w, int crop_border, int fps, void* stream) {
    if (!planes16_args_ok(a, b, sums, frames, h, w, crop_border) || !plane_mask_ok(plane_mask) || fps < 1) return PNP_ERR_BAD_ARG;
    XpArgs s;
    s.plan = pnp_xp_plan(h, w, crop_border);
    if (!s.plan.ok) return PNP_ERR_BAD_ARG;
    clip_planes(*a, s.a);
    clip_planes(*b, s.b);
    return launch<true>(s, plane_mask, fps, sums, frames, (hipStream_t)stream);
}
