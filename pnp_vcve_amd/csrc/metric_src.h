// The front ends of the device metrics, shared by metrics.hip (PSNR / SSIM of frames), plane_metrics.hip (PSNR / SSIM of 4:2:0
// planes) and msssim.hip (MS-SSIM on every boundary): how a sample of a clip is fetched -- fp32 planes rounded to the byte, uint8 RGB
// frames, the optional luma step, 8-bit planes through plane_load.h, 16-bit words -- and what the entries refuse before they look at
// their statistic.  Everything is internal to the unit that includes it (anonymous namespace); nothing here launches a kernel.
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
    for (int c = 0; c < 3; ++c) {
        const float* fc = f + c * hw;
        if (npix == 4 && (reinterpret_cast<uintptr_t>(fc) & 15) == 0) {
            const f32x4 t = *reinterpret_cast<const f32x4*>(fc);
#pragma unroll
            for (int j = 0; j < 4; ++j) v[c][j] = t[j];
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[c][j] = j < npix ? fc[j] : 0.f;
        }
    }
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

// One plane of a 10 / 12-bit clip (pnp_yuv420_planes16): 2-byte loads, sample (row, col) of frame f is the word at
// p + f * frame + row * pitch (bytes) + col * step (samples), read as (word >> shift) & mask.
struct Plane16 {
    const unsigned short* p;
    long pitch, frame;
    int step;
    unsigned shift, mask;
};
__device__ __forceinline__ unsigned load16(const Plane16& s, long f, int row, int col) {
    const unsigned short* q = reinterpret_cast<const unsigned short*>(reinterpret_cast<const char*>(s.p) + f * s.frame + (long)row * s.pitch);
    return ((unsigned)q[(long)col * s.step] >> s.shift) & s.mask;
}
inline Plane16 plane16(const pnp_yuv420_planes16& p, int plane) {      // plane: 0 Y | 1 Cb | 2 Cr
    const unsigned shift = p.msb_aligned ? 16u - (unsigned)p.bit_depth : 0u, mask = (1u << p.bit_depth) - 1u;
    if (plane == 0) return Plane16{p.y, p.y_pitch, p.y_frame, 1, shift, mask};
    return Plane16{plane == 1 ? p.cb : p.cr, p.c_pitch, p.c_frame, p.c_step, shift, mask};
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
