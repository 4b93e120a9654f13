// PSNR-B (include/pnpvcve.h, pnp_psnrb_*): per frame and plane the five sums behind the blocking-aware PSNR of Yim and Bovik -- the
// squared error against the reference and the squared steps of the TEST clip across block-boundary and ordinary neighbour pairs, to
// the right and below.  Integers only on every boundary that scores bytes or d-bit samples (exact 64-bit sums, integer atomics, the
// same bits every run); fp64 partials, one per thread block, for the fp32 Y of PNP_COLOR_Y.  The value is the host's (fp64, written
// once in metrics.psnrb_values), so the device and a restatement cannot differ in rounding.  psnrb_plan.h holds the region, the
// boundary rule, the counts and the tiling; metric_src.h fetches the samples.
//
// One kernel launch covers all frames and planes.  A thread block owns a tile of 256 x 32 samples: a wave walks DOWN eight rows of 256
// columns, a lane keeping its four samples of the row above in registers -- the vertical pairs -- and taking the sample right of its
// four from the next lane by a shuffle -- the horizontal pair between two lanes.  What is left is read again through the cache: the
// first row of the wave below (1/8 of the test clip) and, by lane 63 only, the first sample of the tile to the right.  A pair belongs
// to its left / top sample, so a pair across a seam is counted once, by the tile that holds that sample.  The reference is read once.
#include "metric_src.h"
#include "psnrb_plan.h"

namespace {

enum { PB_RGB, PB_Y, PB_F32, PB_P8, PB_P16 };

// One clip on any of the five sample paths.  NOT metric_src.h's ClipSrc / plane_load4: with them psnrb_kernel<PB_P8> / <PB_P16> took
// 28.3 / 36.1 us a call against 26.8 / 35.0 (tools/bench_psnrb.py, profiles/metric_src_refactor.txt), at the same registers and within
// 12 instructions of the same listing; with this struct and the loader below the time is the parent's.  The host side fills it from
// clip_planes like every other plane entry, and the sums leave through block_sums.
struct PbSrc {
    FrameSrc fs;            // PB_RGB, PB_Y: frames of either format; PB_F32: (frames, C, h, w) fp32 planes
    int C;
    PnpPlaneSrc p8[3];      // PB_P8: Y, Cb, Cr
    int sel[3];             //        the plane is the second of an interleaved pair
    Plane16 p16[3];         // PB_P16
};

struct PbArgs {
    PbSrc a, b;
    int has_b;
    PnpPbPlane geo[3];      // PB_P8 / PB_P16: the planes (ok = 0: not in the mask); else geo[0] serves every channel
    int W;                  // PB_RGB / PB_Y / PB_F32: the frame's width, hw = h * w
    long hw;
    int slots;              // planes of a frame in `sums`
    unsigned long long* sums;       // [frames][slots][5], zeroed by the launcher
    double* partial;        // PB_Y: [frames][tiles][5]
};

template <int MODE>
struct PbTraits {
    typedef int T;
    typedef unsigned Acc;               // a thread adds at most 36 squares below 2^24
    typedef unsigned long long Wide;
    static constexpr int NCH = MODE == PB_RGB ? 3 : 1;
};
template <>
struct PbTraits<PB_Y> {
    typedef float T;
    typedef double Acc;
    typedef double Wide;
    static constexpr int NCH = 1;
};

__device__ __forceinline__ unsigned pb_sq(int d) { return (unsigned)(d * d); }
__device__ __forceinline__ double pb_sq(float d) { return (double)d * (double)d; }

// v[c][j] = sample (row, col + j) of frame f for j < n, 0 for n <= j < 4 -- on the luma path too, where an absent sample is 0 and not
// the luma of a black pixel: absent samples only ever meet absent samples; 1 <= n <= 4
template <int MODE>
__device__ __forceinline__ void pb_load4(const PbSrc& s, const PbArgs& g, const double* lt, long f, int plane, int row, int col, int n,
                                         typename PbTraits<MODE>::T v[][4]) {
    if (MODE == PB_RGB || MODE == PB_Y) {
        unsigned px[4];
        load_px4(s.fs, f, g.hw, (long)row * g.W + col, n, px);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (MODE == PB_Y) {
                v[0][j] = j < n ? luma_of(lt, px[j]) : 0;
            } else {
#pragma unroll
                for (int c = 0; c < PbTraits<MODE>::NCH; ++c) v[c][j] = (int)((px[j] >> (8 * c)) & 255u);
            }
        }
    } else if (MODE == PB_F32) {
        float x[4];
        f32_load4(static_cast<const float*>(s.fs.p) + (f * s.C + plane) * g.hw + (long)row * g.W + col, n, x);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[0][j] = to_u8(x[j]);         // (to_u8(0.f) = 0)
    } else if (MODE == PB_P8) {
        unsigned w[2];
        pnp_plane_load4(s.p8[plane], f, row, col, n, w);
        const unsigned x = s.sel[plane] ? w[1] : w[0];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[0][j] = (int)((x >> (8 * j)) & 255u);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[0][j] = j < n ? (int)load16(s.p16[plane], f, row, col + j) : 0;
    }
}

// grid = (tiles of the largest plane, frames, planes); a block past its plane's tiles, or of a plane outside the mask, has nothing to do
template <int MODE>
__global__ __launch_bounds__(256) void psnrb_kernel(const PbArgs s) {
    typedef typename PbTraits<MODE>::T T;
    typedef typename PbTraits<MODE>::Acc Acc;
    typedef typename PbTraits<MODE>::Wide Wide;
    constexpr int NCH = PbTraits<MODE>::NCH;
    __shared__ double lt[MODE == PB_Y ? 768 : 1];
    __shared__ Wide red[4][NCH * 5];
    Acc acc[NCH * 5];                                               // [channel][sum]
    const int plane = blockIdx.z;
    const PnpPbPlane g = s.geo[(MODE == PB_P8 || MODE == PB_P16) ? plane : 0];
    const int ntiles = g.tiles_x * g.tiles_y;
    if (!g.ok || (int)blockIdx.x >= ntiles) return;                 // the whole block
    if (MODE == PB_Y) stage_luma_table(lt);
    const long frame = blockIdx.y;
    const int ty = (int)blockIdx.x / g.tiles_x, tx = (int)blockIdx.x - ty * g.tiles_x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int r0, r1, col, n;
    pnp_pb_wave_rows(g, ty, wave, r0, r1);
    pnp_pb_lane_cols(g, tx, lane, col, n);
    const bool right = n == 4 && col + 4 < g.x1;                    // the pair (col + 3, col + 4) exists
    const int rend = r1 > r0 && r1 < g.y1 ? r1 + 1 : r1;            // row r1 is read for the pairs (r1 - 1, r1) only
    T prev[NCH][4];
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
#pragma unroll
        for (int q = 0; q < 5; ++q) acc[c * 5 + q] = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) prev[c][j] = 0;
    }
    for (int row = r0; row < rend; ++row) {                         // the same rows for every lane of the wave
        T cur[NCH][4];
#pragma unroll
        for (int c = 0; c < NCH; ++c)
#pragma unroll
            for (int j = 0; j < 4; ++j) cur[c][j] = 0;
        if (n > 0) pb_load4<MODE>(s.a, s, lt, frame, plane, row, col, n, cur);
        if (row < r1) {
            T nxt[NCH];
#pragma unroll
            for (int c = 0; c < NCH; ++c) nxt[c] = __shfl_down(cur[c][0], 1, 64);
            if (lane == 63 && right) {                              // the next tile's first sample
                T one[NCH][4];
                pb_load4<MODE>(s.a, s, lt, frame, plane, row, col + 4, 1, one);
#pragma unroll
                for (int c = 0; c < NCH; ++c) nxt[c] = one[c][0];
            }
            if (s.has_b && n > 0) {
                T ref[NCH][4];
                pb_load4<MODE>(s.b, s, lt, frame, plane, row, col, n, ref);
#pragma unroll
                for (int c = 0; c < NCH; ++c)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[c * 5] += pb_sq(cur[c][j] - ref[c][j]);      // absent samples are 0 in both
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool exists = j < 3 ? j + 1 < n : right;
                const bool bnd = pnp_pb_boundary(col + j, g.bp);
#pragma unroll
                for (int c = 0; c < NCH; ++c) {
                    const T nb = j < 3 ? cur[c][(j + 1) & 3] : nxt[c];
                    const Acc e = exists ? (Acc)pb_sq(cur[c][j] - nb) : (Acc)0;
                    acc[c * 5 + 1] += bnd ? e : (Acc)0;
                    acc[c * 5 + 2] += bnd ? (Acc)0 : e;
                }
            }
        }
        if (row > r0) {
            const int q = pnp_pb_boundary(row - 1, g.bp) ? 3 : 4;   // the same for the whole wave
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                Acc e = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) e += pb_sq(prev[c][j] - cur[c][j]);                 // absent samples are 0 in both rows
                if (q == 3) acc[c * 5 + 3] += e;
                else acc[c * 5 + 4] += e;
            }
        }
#pragma unroll
        for (int c = 0; c < NCH; ++c)
#pragma unroll
            for (int j = 0; j < 4; ++j) prev[c][j] = cur[c][j];
    }
    // registers -> the block's sums (metric_src.h::block_sums) -> one integer atomic per block and sum, or (Y) the block's own five
    // partials, added in a fixed order
    const Wide v = block_sums(acc, red);
    const int t = threadIdx.x;
    if (t < NCH * 5) {
        if (MODE == PB_Y) {
            s.partial[(frame * ntiles + blockIdx.x) * 5 + t] = (double)v;
        } else if (v != 0) {
            atomicAdd(&s.sums[(frame * s.slots + (long)plane * NCH) * 5 + t], (unsigned long long)v);
        }
    }
}

inline bool block_ok(int block) { return block == 4 || block == 8 || block == 16 || block == 32 || block == 64; }

template <int MODE>
int launch(PbArgs& s, int frames, int planes, hipStream_t st) {
    int tiles = 0;
    for (int k = 0; k < 3; ++k)
        if (s.geo[k].ok && s.geo[k].tiles_x * s.geo[k].tiles_y > tiles) tiles = s.geo[k].tiles_x * s.geo[k].tiles_y;
    if (MODE != PB_Y) {
        const int ze = launch_zero_words(s.sums, 2L * frames * s.slots * 5, st);      // a kernel, not a memset node (prep.h)
        if (ze != PNP_OK) return ze;
    }
    hipLaunchKernelGGL(psnrb_kernel<MODE>, dim3((unsigned)tiles, (unsigned)frames, (unsigned)planes), dim3(256), 0, st, s);
    return (int)hipGetLastError();
}

// the planes of a 4:2:0 clip that the mask names: Y with `block`, Cb / Cr with half of it and half the crop.  (gain.hip has a loop of
// the same shape; the two are not shared: the plans are different structs made from different arguments, and a template over both
// would need a functor per unit that is as long as the loop.)
bool plan_planes(PbArgs& s, int mask, int h, int w, int crop, int block) {
    for (int k = 0; k < 3; ++k) {
        s.geo[k] = pnp_pb_plane(0, 0, 0, 0);
        if (!(mask & (1 << k))) continue;
        s.geo[k] = k == 0 ? pnp_pb_plane(h, w, crop, block) : pnp_pb_plane(h / 2, w / 2, crop / 2, block / 2);
        if (!s.geo[k].ok) return false;
    }
    return true;
}

// the launch of the two plane entries: pa, pb = the planes of the two clips (clip_planes; pb: nullptr without a reference)
template <int MODE>
int launch_planes(PbArgs& s, const PlaneSamp* pa, const PlaneSamp* pb, unsigned long long* sums, int frames, void* stream) {
    for (int k = 0; k < 3; ++k) {
        s.a.p8[k] = pa[k].p8, s.a.sel[k] = pa[k].sel, s.a.p16[k] = pa[k].p16;
        if (pb) s.b.p8[k] = pb[k].p8, s.b.sel[k] = pb[k].sel, s.b.p16[k] = pb[k].p16;
    }
    s.has_b = pb != nullptr;
    s.slots = 3;
    s.sums = sums;
    return launch<MODE>(s, frames, 3, (hipStream_t)stream);
}

}  // namespace

extern "C" int pnp_psnrb_counts(int rows, int cols, int crop, int plane_block, int64_t counts[4]) {
    const PnpPbPlane p = pnp_pb_plane(rows, cols, crop, plane_block);
    if (!p.ok || !counts) return PNP_ERR_BAD_ARG;
    pnp_pb_counts(p, counts);
    return PNP_OK;
}

extern "C" int pnp_psnrb_luma_blocks(int h, int w, int crop_border) {
    const PnpPbPlane p = pnp_pb_plane(h, w, crop_border, 2);        // the tiling does not depend on the block size
    return p.ok ? p.tiles_x * p.tiles_y : 0;
}

extern "C" int pnp_psnrb_sums_io(const void* a, int a_format, const void* b, int b_format, int color, void* out, int frames, int c, int h,
                                 int w, int crop_border, int block, void* stream) {
    if (!io_args_ok(a, a_format, b ? b : a, b ? b_format : a_format, color, out, frames, c, h, w, crop_border) || !block_ok(block))
        return PNP_ERR_BAD_ARG;
    PbArgs s = {};
    s.geo[0] = pnp_pb_plane(h, w, crop_border, block);
    if (!s.geo[0].ok) return PNP_ERR_BAD_ARG;
    s.geo[1] = s.geo[2] = pnp_pb_plane(0, 0, 0, 0);
    s.a.fs = frame_src(a, a_format, frames, h, w);
    s.b.fs = frame_src(b ? b : a, b ? b_format : a_format, frames, h, w);
    s.a.C = s.b.C = c;
    s.has_b = b != nullptr;
    s.W = w;
    s.hw = (long)h * w;
    s.slots = c;
    hipStream_t st = (hipStream_t)stream;
    if (color == PNP_COLOR_Y) {
        s.partial = static_cast<double*>(out);
        return launch<PB_Y>(s, frames, 1, st);
    }
    s.sums = static_cast<unsigned long long*>(out);
    if (c == 3) return launch<PB_RGB>(s, frames, 1, st);
    return launch<PB_F32>(s, frames, c, st);                        // io_args_ok: fp32 planes on both sides
}

extern "C" int pnp_psnrb_sums_yuv420(const pnp_yuv420_planes* a, const pnp_yuv420_planes* b, int plane_mask, unsigned long long* sums,
                                     int frames, int h, int w, int crop_border, int block, void* stream) {
    if (!planes_args_ok(a, b ? b : a, sums, frames, h, w, crop_border) || !plane_mask_ok(plane_mask) || !block_ok(block)) return PNP_ERR_BAD_ARG;
    PbArgs s = {};
    if (!plan_planes(s, plane_mask, h, w, crop_border, block)) return PNP_ERR_BAD_ARG;
    PlaneSamp pa[3], pb[3];
    clip_planes(*a, h, w, PNP_YUV_FORMAT_420, pa);
    if (b) clip_planes(*b, h, w, PNP_YUV_FORMAT_420, pb);
    return launch_planes<PB_P8>(s, pa, b ? pb : nullptr, sums, frames, stream);
}

extern "C" int pnp_psnrb_sums_yuv420p16(const pnp_yuv420_planes16* a, const pnp_yuv420_planes16* b, int plane_mask, unsigned long long* sums,
                                        int frames, int h, int w, int crop_border, int block, void* stream) {
    if (!planes16_args_ok(a, b ? b : a, sums, frames, h, w, crop_border) || !plane_mask_ok(plane_mask) || !block_ok(block)) return PNP_ERR_BAD_ARG;
    PbArgs s = {};
    if (!plan_planes(s, plane_mask, h, w, crop_border, block)) return PNP_ERR_BAD_ARG;
    PlaneSamp pa[3], pb[3];
    clip_planes(*a, pa);
    if (b) clip_planes(*b, pb);
    return launch_planes<PB_P16>(s, pa, b ? pb : nullptr, sums, frames, stream);
}
