// Self-ensemble side kernels (include/pnpvcve.h, "Self-ensemble"): the oriented copy of a variant's inputs and the oriented running
// sum of its output.  Both are one gather: an OUTPUT plane of oh x ow elements reads a SOURCE plane of sh x sw,
//     out[r][c] = src[ T ? Fr(c) : Fr(r) ][ T ? Fc(r) : Fc(c) ],   Fr(k) = flip_r ? sh-1-k : k,  Fc(k) = flip_c ? sw-1-k : k,
// with (oh, ow) = (sw, sh) when T (transposed) and (sh, sw) otherwise.
//   view, variant v:        src = the original, out = the view;  flip_r = bit 1, flip_c = bit 0, T = bit 2.
//   accumulate, variant v:  src = the variant's output, out = acc (original orientation); the inverse applies bit 2, then bit 1, then
//                           bit 0, which as a gather is flip_r = bit 1, flip_c = bit 0 without T and flip_r = bit 0, flip_c = bit 1
//                           with T (the source's rows are the original's columns).
// T clear: a block copies a 16 x 64 tile row by row; a wave reads and writes 256 contiguous bytes (a flipped row is read backwards:
// the same lines).  T set: a 32 x 32 tile goes through LDS with a pitch of 33 dwords -- rows are written with consecutive addresses
// and read with stride 33, conflict-free on the 32 banks a 4-byte LDS access sees per 32-lane half -- so that the global reads and the
// global writes are both row-contiguous.  uint8 HWC frames move as 3-byte pixels, byte by byte (no row is assumed dword-aligned: w or h
// odd puts rows at odd addresses); their tile has a pitch of 99 bytes (24.75 dwords: a half-wave's 11 pixels of a column land on 11
// different banks).  The frames are 3 of the 40 B per pixel a view moves.  Every element offset is 64-bit.
#include "common.h"

namespace {
constexpr int kThreads = 256;
constexpr int kT = 32;                   // transposed tile: kT x kT
constexpr int kRowW = 64, kRowH = 16;    // row-wise tile
constexpr int kPitchF = kT + 1;          // dwords
constexpr int kPitchB = 3 * kT + 3;      // bytes: 99

struct Orient {
    int transposed, flip_r, flip_c;
};

__device__ __forceinline__ int flip(int k, int n, int on) { return on ? n - 1 - k : k; }

// one fp32 plane tile; op(dst element, source value)
template <class Op>
__device__ __forceinline__ void plane_tile(const float* __restrict__ src, int sh, int sw, float* __restrict__ dst, int tile_r, int tile_c,
                                           Orient o, float* lds, Op op) {
    const int tid = threadIdx.x;
    if (!o.transposed) {
        const int c = tile_c * kRowW + (tid & 63);
        if (c >= sw) return;
        const int sc = flip(c, sw, o.flip_c);
#pragma unroll
        for (int k = 0; k < kRowH / 4; ++k) {
            const int r = tile_r * kRowH + (tid >> 6) + 4 * k;
            if (r < sh) op(dst + (int64_t)r * sw + c, src[(int64_t)flip(r, sh, o.flip_r) * sw + sc]);
        }
        return;
    }
    const int oh = sw, ow = sh;
    const int tx = tid & 31, ty = tid >> 5;
    const int r_in = tile_r * kT + tx;       // output row whose source column this lane loads
#pragma unroll
    for (int k = 0; k < kT / 8; ++k) {
        const int j = ty + 8 * k, c = tile_c * kT + j;
        if (c < ow && r_in < oh) lds[j * kPitchF + tx] = src[(int64_t)flip(c, sh, o.flip_r) * sw + flip(r_in, sw, o.flip_c)];
    }
    __syncthreads();
    const int c_out = tile_c * kT + tx;
#pragma unroll
    for (int k = 0; k < kT / 8; ++k) {
        const int j = ty + 8 * k, r = tile_r * kT + j;
        if (r < oh && c_out < ow) op(dst + (int64_t)r * ow + c_out, lds[tx * kPitchF + j]);
    }
}

// one tile of a uint8 HWC frame: the same gather on 3-byte pixels
__device__ __forceinline__ void frame_tile_u8(const unsigned char* __restrict__ src, int sh, int sw, unsigned char* __restrict__ dst,
                                              int tile_r, int tile_c, Orient o, unsigned char* lds) {
    const int tid = threadIdx.x;
    if (!o.transposed) {
        const int lane = tid & 63;
#pragma unroll
        for (int k = 0; k < kRowH / 4; ++k) {
            const int r = tile_r * kRowH + (tid >> 6) + 4 * k;
            if (r >= sh) continue;
            const unsigned char* s = src + (int64_t)flip(r, sh, o.flip_r) * sw * 3;
            unsigned char* d = dst + (int64_t)r * sw * 3;
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const int e = lane + 64 * q, p = e / 3, ch = e - 3 * p, c = tile_c * kRowW + p;
                if (c < sw) d[(int64_t)c * 3 + ch] = s[(int64_t)flip(c, sw, o.flip_c) * 3 + ch];
            }
        }
        return;
    }
    const int oh = sw, ow = sh;
    const int tx = tid & 31, ty = tid >> 5;
#pragma unroll
    for (int k = 0; k < kT / 8; ++k) {
        const int j = ty + 8 * k, c = tile_c * kT + j;
        if (c >= ow) continue;
        const unsigned char* s = src + (int64_t)flip(c, sh, o.flip_r) * sw * 3;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const int e = tx + 32 * q, p = e / 3, ch = e - 3 * p, r = tile_r * kT + p;
            if (r < oh) lds[j * kPitchB + e] = s[(int64_t)flip(r, sw, o.flip_c) * 3 + ch];
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kT / 8; ++k) {
        const int j = ty + 8 * k, r = tile_r * kT + j;
        if (r >= oh) continue;
        unsigned char* d = dst + (int64_t)r * ow * 3;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const int e = tx + 32 * q, p = e / 3, ch = e - 3 * p, c = tile_c * kT + p;
            if (c < ow) d[(int64_t)c * 3 + ch] = lds[p * kPitchB + j * 3 + ch];
        }
    }
}

struct ViewArgs {
    const void* lq;
    const float* mvs;
    const float* par;
    void* lq_out;
    float* mvs_out;
    float* par_out;
    int u8, t, h, w, variant;
    int units_lq, units_mvs;      // units (planes, or uint8 frames) of lq and of mvs; the rest are par's
    int tiles_r, tiles_c;         // tiles of one unit, over the OUTPUT grid
};

struct CopySigned {
    int negate;
    __device__ __forceinline__ void operator()(float* d, float v) const { *d = negate ? -v : v; }
};

// grid.x = units * tiles_r * tiles_c; a block is one tile of one plane (or of one uint8 frame)
template <bool U8>
__global__ __launch_bounds__(kThreads) void ensemble_view_kernel(ViewArgs a) {
    __shared__ float lds[kT * kPitchF];
    const int per = a.tiles_r * a.tiles_c;
    const int unit = blockIdx.x / per, tile = blockIdx.x - unit * per;
    const int tile_r = tile / a.tiles_c, tile_c = tile - tile_r * a.tiles_c;
    const Orient o = {(a.variant >> 2) & 1, (a.variant >> 1) & 1, a.variant & 1};
    const int rev = (a.variant >> 3) & 1;
    const int64_t hw = (int64_t)a.h * a.w;
    if (U8 && unit < a.units_lq) {
        const int fo = unit, fi = flip(fo, a.t, rev);
        frame_tile_u8((const unsigned char*)a.lq + fi * hw * 3, a.h, a.w, (unsigned char*)a.lq_out + fo * hw * 3, tile_r, tile_c, o,
                      (unsigned char*)lds);
        return;
    }
    const float* src;
    float* dst;
    int C, u, is_mv = 0;
    if (unit < a.units_lq) {
        src = (const float*)a.lq, dst = (float*)a.lq_out, C = 3, u = unit;
    } else if (unit < a.units_lq + a.units_mvs) {
        src = a.mvs, dst = a.mvs_out, C = 4, u = unit - a.units_lq, is_mv = 1;
    } else {
        src = a.par, dst = a.par_out, C = 3, u = unit - a.units_lq - a.units_mvs;
    }
    const int fo = u / C, co = u - fo * C, fi = flip(fo, a.t, rev);
    int ci = co, negate = 0;
    if (is_mv) {      // out channel co holds source channel ci: undo bit 3's pair swap, then bit 2's x / y swap; x is negated by bit 0, y by bit 1
        ci = co ^ (rev ? 2 : 0) ^ (o.transposed ? 1 : 0);
        negate = (ci & 1) ? o.flip_r : o.flip_c;
    }
    plane_tile(src + ((int64_t)fi * C + ci) * hw, a.h, a.w, dst + ((int64_t)fo * C + co) * hw, tile_r, tile_c, o, lds, CopySigned{negate});
}

struct Accumulate {
    int first;
    float scale;
    __device__ __forceinline__ void operator()(float* d, float v) const {
        const float s = first ? v : *d + v;
        *d = scale == 1.f ? s : s * scale;
    }
};

// x (t,c,H',W') -> acc (t,c,H,W); grid.x = t*c * tiles_r * tiles_c over acc's grid
__global__ __launch_bounds__(kThreads) void ensemble_accumulate_kernel(const float* __restrict__ x, float* __restrict__ acc, int t, int c, int H,
                                                                       int W, int variant, int first, float scale, int tiles_r,
                                                                       int tiles_c) {
    __shared__ float lds[kT * kPitchF];
    const int per = tiles_r * tiles_c;
    const int unit = blockIdx.x / per, tile = blockIdx.x - unit * per;
    const int tile_r = tile / tiles_c, tile_c = tile - tile_r * tiles_c;
    const int tr = (variant >> 2) & 1, b1 = (variant >> 1) & 1, b0 = variant & 1;
    const Orient o = {tr, tr ? b0 : b1, tr ? b1 : b0};
    const int fo = unit / c, ch = unit - fo * c, fi = flip(fo, t, (variant >> 3) & 1);
    const int64_t hw = (int64_t)H * W;
    const int sh = tr ? W : H, sw = tr ? H : W;
    plane_tile(x + ((int64_t)fi * c + ch) * hw, sh, sw, acc + ((int64_t)fo * c + ch) * hw, tile_r, tile_c, o, lds, Accumulate{first, scale});
}

// tiles of an oh x ow output grid
inline void tile_grid(int oh, int ow, int transposed, int* tiles_r, int* tiles_c) {
    *tiles_r = transposed ? (oh + kT - 1) / kT : (oh + kRowH - 1) / kRowH;
    *tiles_c = transposed ? (ow + kT - 1) / kT : (ow + kRowW - 1) / kRowW;
}
}  // namespace

static int launch_ensemble_view(const void* lq, const float* mvs, const float* par, void* lq_out, float* mvs_out, float* par_out, int u8, int t,
                         int h, int w, int variant, hipStream_t stream) {
    ViewArgs a = {lq, mvs, par, lq_out, mvs_out, par_out, u8, t, h, w, variant, 0, 0, 0, 0};
    a.units_lq = lq ? (u8 ? t : 3 * t) : 0;
    a.units_mvs = mvs ? 4 * t : 0;
    const int64_t units = (int64_t)a.units_lq + a.units_mvs + (par ? 3 * (int64_t)t : 0);
    if (units == 0) return PNP_OK;
    const int tr = (variant >> 2) & 1;
    tile_grid(tr ? w : h, tr ? h : w, tr, &a.tiles_r, &a.tiles_c);
    const int64_t blocks = units * a.tiles_r * a.tiles_c;
    if (blocks > 0x7fffffffLL) return PNP_ERR_UNSUPPORTED;
    if (u8 && lq)
        hipLaunchKernelGGL(ensemble_view_kernel<true>, dim3((unsigned)blocks), dim3(kThreads), 0, stream, a);
    else
        hipLaunchKernelGGL(ensemble_view_kernel<false>, dim3((unsigned)blocks), dim3(kThreads), 0, stream, a);
    return (int)hipGetLastError();
}

static int launch_ensemble_accumulate(const float* x, float* acc, int t, int c, int H, int W, int variant, int first, float scale,
                               hipStream_t stream) {
    int tiles_r, tiles_c;
    tile_grid(H, W, (variant >> 2) & 1, &tiles_r, &tiles_c);
    const int64_t blocks = (int64_t)t * c * tiles_r * tiles_c;
    if (blocks > 0x7fffffffLL) return PNP_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(ensemble_accumulate_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, stream, x, acc, t, c, H, W, variant, first, scale,
                       tiles_r, tiles_c);
    return (int)hipGetLastError();
}

extern "C" int pnp_ensemble_view(const void* lq, const float* mvs, const float* par, void* lq_out, float* mvs_out, float* par_out,
                                 int frames_format, int t, int h, int w, int variant, void* stream) {
    if (!lq != !lq_out || !mvs != !mvs_out || !par != !par_out) return PNP_ERR_BAD_ARG;
    if (variant < 0 || variant > 15 || t < 1 || h < 1 || w < 1) return PNP_ERR_BAD_ARG;
    if (frames_format != PNP_FRAMES_F32_NCHW && frames_format != PNP_FRAMES_U8_HWC) return PNP_ERR_BAD_ARG;
    if ((lq && lq == lq_out) || (mvs && mvs == mvs_out) || (par && par == par_out)) return PNP_ERR_BAD_ARG;
    return launch_ensemble_view(lq, mvs, par, lq_out, mvs_out, par_out, frames_format == PNP_FRAMES_U8_HWC, t, h, w, variant,
                                (hipStream_t)stream);
}

extern "C" int pnp_ensemble_accumulate_f32(const float* x, float* acc, int t, int c, int H, int W, int variant, int first, float scale,
                                           void* stream) {
    if (!x || !acc || x == acc) return PNP_ERR_BAD_ARG;
    if (variant < 0 || variant > 15 || t < 1 || c < 1 || H < 1 || W < 1) return PNP_ERR_BAD_ARG;
    if (!(scale > 0.f) || scale > 3.402823466e+38f) return PNP_ERR_BAD_ARG;      // NaN, <= 0 and +inf
    return launch_ensemble_accumulate(x, acc, t, c, H, W, variant, first != 0, scale, (hipStream_t)stream);
}
