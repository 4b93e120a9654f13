// The front ends of the device metrics: how a clip is named and how its samples are fetched.  Included by all six metric units --
// metrics.hip (PSNR / SSIM of frames), plane_metrics.hip (PSNR / SSIM of Y'CbCr planes), msssim.hip, xpsnr.hip, psnrb.hip and gain.hip
// (the SSIM ones through ssim_tile.h).  What lives here:
//   - the byte of an fp32 sample (to_u8), the luma step (luma_of and its table), the pixel-group loader of frames (FrameSrc, load_px4);
//   - one clip on any sample path (ClipSrc; its planes are plane_src.h's PlaneSamp, filled by clip_planes) and the two group loaders
//     the kernels read through: plane_load4<S16> (8-bit planes through plane_load.h, 16-bit words through load16) and f32_load4.
//     ONE exception: psnrb_kernel's plane arms keep a private struct and loader (psnrb.hip::PbSrc, pb_load4 -- the shared ones cost
//     that kernel 5 % / 3 % of a call; profiles/metric_src_refactor.txt), filled on the host from clip_planes all the same;
//   - the block reduction every deterministic sum leaves through (block_sums);
//   - what the entries refuse before they look at their statistic, and SSIM's window.
// The loaders return integers or raw floats, 0 where a group ends: luma_of, to_u8, the channels of a pixel and what an ABSENT sample is
// worth are the calling kernel's.  Everything is internal to the unit that includes it (anonymous namespace); nothing here launches
// a kernel.
#pragma once
#include "plane_src.h"
#include "prep.h"
#include <cmath>

namespace {

__device__ __forceinline__ int to_u8(float v) {
    v = fminf(fmaxf(v, 0.f), 1.f);
    return (int)rintf(v * 255.0f);
}

// Luma: the reference's mmcv.bgr2ycbcr(img / 255., y_only=True) * 255. on the uint8 BGR image.  mmcv is not available to this build:
// the arithmetic is restated from its published source (mmcv/image/colorspace.py: np.dot(img, [24.966, 128.553, 65.481]) + 16.0 in
// float64, / 255., back to float32), as SSIM's cv2.filter2D is in metrics.hip.  With x_c = (float)byte_c / 255.0f (PnpU8Table):
//     Y = (float)((((double)x_B * 24.966 + (double)x_G * 128.553) + (double)x_R * 65.481 + 16.0) / 255.0) * 255.0f
// The 3 x 256 fp64 products are evaluated by the compiler (each rounded once, IEEE) and staged in LDS; what is left on the device is
// three fp64 additions, an fp64 division, the rounding to fp32 and one fp32 multiply, compiled with contraction off.
struct PnpLumaTable {
    double v[3][256];       // [R, G, B of the RGB frames = channels 2, 1, 0 of the reference's BGR image][byte]
    constexpr PnpLumaTable() : v() {
        for (int i = 0; i < 256; ++i) {
            const float x = (float)i / 255.0f;
            v[0][i] = (double)x * 65.481;
            v[1][i] = (double)x * 128.553;
            v[2][i] = (double)x * 24.966;
        }
    }
};
__device__ const PnpLumaTable k_luma_table = PnpLumaTable();

// lt: 768 doubles of LDS; blocks of 256 threads
__device__ __forceinline__ void stage_luma_table(double* lt) {
    const double* src = &k_luma_table.v[0][0];
    for (int i = threadIdx.x; i < 768; i += 256) lt[i] = src[i];
    __syncthreads();
}

// px = R | G << 8 | B << 16.  Contraction is off in here: the closing fp32 product must be rounded before a caller subtracts two of
// these (d = Y_a - Y_b would otherwise become fma(y_a, 255, -Y_b), which is not what the reference subtracts).
__device__ __forceinline__ float luma_of(const double* lt, unsigned px) {
#pragma clang fp contract(off)
    const double y64 = (((lt[512 + (px >> 16)] + lt[256 + ((px >> 8) & 255u)]) + lt[px & 255u]) + 16.0) / 255.0;
    return (float)y64 * 255.0f;
}

__device__ __forceinline__ unsigned px_of_f32(float r, float g, float b) {
    return (unsigned)to_u8(r) | ((unsigned)to_u8(g) << 8) | ((unsigned)to_u8(b) << 16);
}

// v[j] = p[j] for j < n, 0.f for n <= j < 4: ONE aligned 16-byte load where n == 4 and the address allows it, one by one elsewhere
__device__ __forceinline__ void f32_load4(const float* p, int n, float v[4]) {
    if (n == 4 && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = t[j];
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = j < n ? p[j] : 0.f;
    }
}

// One input of a metric: the clip's first frame and, for a byte clip, the bytes [lo, hi) that may be read.
struct FrameSrc {
    const void* p;
    const unsigned char *lo, *hi;
    int fmt;
};

// px[j] = the packed bytes of pixels p0 + j (j < npix <= 4; px[j] = 0 beyond) of `frame`; hw = h * w.
// A byte frame: the 12 bytes of four pixels sit at ANY address (frames and cropped rows start anywhere), so they are read as the
// aligned dwords that cover them and shifted into place -- 3 loads, 4 when the address is not a multiple of 4 -- where those dwords lie
// inside the clip; the groups where they do not (the first of a misaligned clip, the last) and the short group at the end of a row
// are read byte by byte (the head / body / tail split of pack_lr_u8_any_kernel, decided per group).
__device__ __forceinline__ void load_px4(const FrameSrc& s, long frame, long hw, long p0, int npix, unsigned px[4]) {
    if (s.fmt == PNP_FRAMES_U8_HWC) {
        const unsigned char* q = static_cast<const unsigned char*>(s.p) + (frame * hw + p0) * 3;
        const unsigned sh = (unsigned)(reinterpret_cast<uintptr_t>(q) & 3);
        const unsigned char* q0 = q - sh;
        if (npix == 4 && q0 >= s.lo && q0 + (sh ? 16 : 12) <= s.hi) {
            const unsigned* d = reinterpret_cast<const unsigned*>(q0);
            unsigned d0 = d[0], d1 = d[1], d2 = d[2];
            if (sh) {
                const unsigned d3 = d[3];
                d0 = __builtin_amdgcn_alignbyte(d1, d0, sh);      // ({hi, lo} >> 8 sh), low dword
                d1 = __builtin_amdgcn_alignbyte(d2, d1, sh);
                d2 = __builtin_amdgcn_alignbyte(d3, d2, sh);
            }
            // little-endian bytes: d0 = r0 g0 b0 r1, d1 = g1 b1 r2 g2, d2 = b2 r3 g3 b3
            px[0] = d0 & 0xffffffu;
            px[1] = (d0 >> 24) | ((d1 & 0xffffu) << 8);
            px[2] = (d1 >> 16) | ((d2 & 0xffu) << 16);
            px[3] = d2 >> 8;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                px[j] = 0;
                if (j < npix) px[j] = (unsigned)q[3 * j] | ((unsigned)q[3 * j + 1] << 8) | ((unsigned)q[3 * j + 2] << 16);
            }
        }
        return;
    }
    const float* f = static_cast<const float*>(s.p) + frame * 3 * hw + p0;
    float v[3][4];
#pragma unroll
    for (int c = 0; c < 3; ++c) f32_load4(f + c * hw, npix, v[c]);
#pragma unroll
    for (int j = 0; j < 4; ++j) px[j] = j < npix ? px_of_f32(v[0][j], v[1][j], v[2][j]) : 0u;
}

inline bool known_format(int f) { return f == PNP_FRAMES_F32_NCHW || f == PNP_FRAMES_U8_HWC; }

inline FrameSrc frame_src(const void* p, int fmt, int frames, int h, int w) {
    FrameSrc s;
    s.p = p;
    s.fmt = fmt;
    s.lo = static_cast<const unsigned char*>(p);
    s.hi = s.lo + (fmt == PNP_FRAMES_U8_HWC ? (long)frames * h * w * 3 : 0);
    return s;
}

// what every io entry refuses before it looks at its statistic
inline bool io_args_ok(const void* a, int fa, const void* b, int fb, int color, const void* out, int frames, int c, int h, int w, int crop) {
    if (!a || !b || !out || !known_format(fa) || !known_format(fb) || (color != PNP_COLOR_NONE && color != PNP_COLOR_Y)) return false;
    if (frames < 1 || c < 1 || h < 1 || w < 1 || crop < 0 || 2 * crop >= h || 2 * crop >= w) return false;
    const bool planes_only = fa == PNP_FRAMES_F32_NCHW && fb == PNP_FRAMES_F32_NCHW && color == PNP_COLOR_NONE;
    return c == 3 || planes_only;
}

// sample (row, col) of frame f of a plane of 16-bit words (plane_src.h)
__device__ __forceinline__ unsigned load16(const Plane16& s, long f, int row, int col) {
    const unsigned short* q = reinterpret_cast<const unsigned short*>(reinterpret_cast<const char*>(s.p) + f * s.frame + (long)row * s.pitch);
    return ((unsigned)q[(long)col * s.step] >> s.shift) & s.mask;
}

// One clip on any sample path; only the members of the kernel instance's kind are read.
struct ClipSrc {
    FrameSrc fs;            // frames of either format; or (frames, C, h, w) fp32 planes at fs.p
    int C;
    PlaneSamp pl[3];        // the Y, Cb and Cr planes of a plane clip (clip_planes)
};

// v[j] = sample (row, col + j) of frame f of the plane for j < n, 0 for n <= j < 4; 1 <= n <= 4.  S16: 16-bit words, one load each;
// otherwise bytes, a group through the plane loader.  T: the integer (or float) type the caller computes in.
template <bool S16, class T>
__device__ __forceinline__ void plane_load4(const PlaneSamp& s, long f, int row, int col, int n, T v[4]) {
    if (S16) {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = j < n ? (T)load16(s.p16, f, row, col + j) : (T)0;
    } else {
        unsigned w[2];
        pnp_plane_load4(s.p8, f, row, col, n, w);           // bytes >= n are 0
        const unsigned x = s.sel ? w[1] : w[0];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (T)((x >> (8 * j)) & 255u);
    }
}

// The block reduction of every deterministic sum (blocks of 256 threads, red: Wide[4][N] of LDS).  wave_sums: sum n of a wave by
// shuffles (32, 16, .. 1) into red[wave][n].  waves_sum, behind a barrier: the four waves added in wave order.  block_sums: both; the
// block's sum n is returned to thread n < N, which stores it, keeps it as an fp64 partial or adds it with `if (v) atomicAdd`.
// The chains of one or two sums (the SSIM / MS-SSIM kernels: one tile a block, so the tail's latency shows -- MS-SSIM on fp32 planes
// took 2 % longer with its two chains one after the other) run side by side; more sums go one after the other, so that only one
// widened sum is live at a time (PSNR-B has up to 15, the gain's classes 24).  Either way a sum's own chain and order are the same.
template <int N, class Wide, class Acc>
__device__ __forceinline__ void wave_sums(const Acc (&acc)[N], Wide (*red)[N]) {
    constexpr int G = N <= 2 ? N : 1;
#pragma unroll
    for (int n0 = 0; n0 < N; n0 += G) {
        Wide v[G];
#pragma unroll
        for (int g = 0; g < G; ++g) v[g] = acc[n0 + g];
        for (int off = 32; off > 0; off >>= 1)
#pragma unroll
            for (int g = 0; g < G; ++g) v[g] += __shfl_down(v[g], off, 64);
        if ((threadIdx.x & 63) == 0)
#pragma unroll
            for (int g = 0; g < G; ++g) red[threadIdx.x >> 6][n0 + g] = v[g];
    }
}
template <int N, class Wide>
__device__ __forceinline__ Wide waves_sum(Wide (*red)[N], int n) {
    return ((red[0][n] + red[1][n]) + red[2][n]) + red[3][n];
}
template <int N, class Wide, class Acc>
__device__ __forceinline__ Wide block_sums(const Acc (&acc)[N], Wide (*red)[N]) {
    wave_sums(acc, red);
    __syncthreads();
    return (int)threadIdx.x < N ? waves_sum(red, (int)threadIdx.x) : Wide(0);
}

// the crop rule of a format: crop_border even where an axis is subsampled (4:2:0, 4:2:2), any value >= 0 at 4:4:4
inline bool plane_crop_ok(int format, int h, int w, int crop) {
    return crop >= 0 && !(yuv_sx(format) == 2 && (crop & 1)) && 2 * crop < h && 2 * crop < w;
}

// what the plane entries refuse before they look at their statistic
inline bool planes_args_ok(const pnp_yuv420_planes* a, const pnp_yuv420_planes* b, const void* out, int frames, int h, int w, int crop,
                           int format = PNP_YUV_FORMAT_420) {
    if (!a || !b || !out || !yuv_frame_ok(format, frames, h, w) || !plane_crop_ok(format, h, w, crop)) return false;
    return yuv_planes_ok(*a, w, format) && yuv_planes_ok(*b, w, format);
}

inline bool planes16_args_ok(const pnp_yuv420_planes16* a, const pnp_yuv420_planes16* b, const void* out, int frames, int h, int w, int crop,
                             int format = PNP_YUV_FORMAT_420) {
    if (!a || !b || !out || !yuv_frame_ok(format, frames, h, w) || !plane_crop_ok(format, h, w, crop)) return false;
    return yuv_planes_ok(*a, w, format) && yuv_planes_ok(*b, w, format) && a->bit_depth == b->bit_depth;
}

inline void ssim_window(double* g) {                     // cv2.getGaussianKernel(11, 1.5)
    double sum = 0;
    for (int i = 0; i < 11; ++i) {
        g[i] = exp(-((i - 5.0) * (i - 5.0)) / (2 * 1.5 * 1.5));
        sum += g[i];
    }
    for (int i = 0; i < 11; ++i) g[i] /= sum;
}

}  // namespace
