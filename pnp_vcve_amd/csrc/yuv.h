// Y'CbCr boundary (yuv.hip): NV12 / NV21 / I420 planes at 8 bit, P010 / P012 / yuv420p10le / yuv420p12le planes at 10 and 12
// bit <-> fp32 RGB, and the 4:2:2 and 4:4:4 planes of the same containers (the chroma format: bits 12..13 of the code).  The
// arithmetic is stated ONCE, in include/pnpvcve.h (pnp_frames_from_yuv420 / pnp_frames_to_yuv420, pnp_yuv420_planes16, "Chroma
// formats"); tests/yuv_ref.py and tests/yuv16_ref.py restate it in numpy and the kernels are bit-equal to those.  The two
// public descriptors become ONE internal one at the extern "C" edge (YuvPlanes); everything behind it is written once, in terms of
// the sample's size.
#pragma once
#include "common.h"

// Every constant of a standard at depth d: evaluated in double from Kr, Kb and rounded to fp32 once (yuv_coef), on the host.  The
// container beside them: a sample reads as (word >> shift) & vmask and is written as value << shift (8 bit: shift 0, the whole byte).
struct YuvCoef {
    float cy, crv, cbu, cgu, cgv;       // samples -> RGB
    float kr, kg, kb, sy, sc, ipb, ipr; // RGB -> samples: luma weights, scales, 0.5 / (1 - Kb), 0.5 / (1 - Kr)
    int yoff;                           // 16 << (d - 8), or 0 (full range)
    int cmid;                           // 2^(d-1)
    float vmax;                         // 2^d - 1
    unsigned shift;                     // 0 (low-aligned) | 16 - d (high-aligned)
    unsigned vmask;                     // 2^d - 1
    int chroma;                         // PNP_YUV_CHROMA_*: the siting and filters of both directions (bits 8..11 of the code)
    int format;                         // PNP_YUV_FORMAT_*: the chroma planes' geometry (bits 12..13 of the code)
};
// A chroma format is its two subsampling factors: the chroma planes are (h / sy) x (w / sx)
static inline bool yuv_format_ok(int format) { return format >= PNP_YUV_FORMAT_420 && format <= PNP_YUV_FORMAT_444; }
static inline int yuv_sx(int format) { return format == PNP_YUV_FORMAT_444 ? 1 : 2; }
static inline int yuv_sy(int format) { return format == PNP_YUV_FORMAT_420 ? 2 : 1; }
// n frames of h x w in a format: sx divides w and sy divides h (4:2:0 keeps its lower bound of 2 x 2)
static inline bool yuv_frame_ok(int format, int n, int h, int w) {
    return yuv_format_ok(format) && n >= 1 && h >= yuv_sy(format) && w >= yuv_sx(format) && !(h % yuv_sy(format)) && !(w % yuv_sx(format));
}
// depth 8 (low-aligned only: the sample is the byte), or 10 | 12 in a 16-bit word, low- or high-aligned
static inline bool yuv_depth_ok(int bit_depth, int msb_aligned) {
    return bit_depth == 8 ? msb_aligned == 0 : (bit_depth == 10 || bit_depth == 12) && (msb_aligned == 0 || msb_aligned == 1);
}
// `code` is what every entry takes as yuv_standard: PNP_YUV_CODE3(standard, chroma, format), the standard 0..3 in bits 0..7, the chroma
// mode 0..3 in bits 8..11 and the chroma format 0..2 in bits 12..13; any other bit set (a mode above 3, a low byte above 3, format 3,
// bits from 14 up, a negative value) is refused
static inline bool yuv_coef(int code, int bit_depth, int msb_aligned, YuvCoef* k) {
    if ((code & ~0x3303) || !yuv_format_ok((code >> 12) & 3) || !yuv_depth_ok(bit_depth, msb_aligned)) return false;
    const int standard = code & 0xff;
    k->chroma = (code >> 8) & 0xf;
    k->format = (code >> 12) & 3;
    const bool bt709 = standard >= PNP_YUV_BT709_LIMITED, full = (standard & 1) != 0;
    const double Kr = bt709 ? 0.2126 : 0.299, Kb = bt709 ? 0.0722 : 0.114, Kg = 1.0 - Kr - Kb;
    const double s = (double)(1 << (bit_depth - 8)), top = (double)((1 << bit_depth) - 1);
    const double sy = full ? top : 219.0 * s, sc = full ? top : 224.0 * s;
    k->cy = (float)(1.0 / sy);
    k->crv = (float)(2.0 * (1.0 - Kr) / sc);
    k->cbu = (float)(2.0 * (1.0 - Kb) / sc);
    k->cgu = (float)(2.0 * Kb * (1.0 - Kb) / (Kg * sc));
    k->cgv = (float)(2.0 * Kr * (1.0 - Kr) / (Kg * sc));
    k->kr = (float)Kr, k->kg = (float)Kg, k->kb = (float)Kb;
    k->sy = (float)sy, k->sc = (float)sc;
    k->ipb = (float)(0.5 / (1.0 - Kb)), k->ipr = (float)(0.5 / (1.0 - Kr));
    k->yoff = full ? 0 : 16 << (bit_depth - 8);
    k->cmid = 1 << (bit_depth - 1);
    k->vmax = (float)top;
    k->shift = msb_aligned ? 16u - (unsigned)bit_depth : 0u;
    k->vmask = (1u << bit_depth) - 1u;
    return true;
}

// The planes of a clip, whichever public descriptor named them: byte pointers, pitches and frame strides in bytes, c_step in samples.
struct YuvPlanes {
    unsigned char *y, *cb, *cr;
    int64_t y_pitch, c_pitch, y_frame, c_frame;
    int c_step;
    int sample_bytes;                   // 1 | 2
    int bit_depth, msb_aligned;         // the container (yuv_coef): 8, 0 for sample_bytes 1
};
static inline YuvPlanes yuv_planes(const pnp_yuv420_planes& p) {
    return YuvPlanes{p.y, p.cb, p.cr, p.y_pitch, p.c_pitch, p.y_frame, p.c_frame, p.c_step, 1, 8, 0};
}
static inline YuvPlanes yuv_planes(const pnp_yuv420_planes16& p) {
    return YuvPlanes{reinterpret_cast<unsigned char*>(p.y), reinterpret_cast<unsigned char*>(p.cb), reinterpret_cast<unsigned char*>(p.cr),
                     p.y_pitch, p.c_pitch, p.y_frame, p.c_frame, p.c_step, 2, p.bit_depth, p.msb_aligned};
}
static inline bool yuv_coef(int code, const YuvPlanes& p, YuvCoef* k) { return yuv_coef(code, p.bit_depth, p.msb_aligned, k); }

// What a descriptor must satisfy for h x w frames of a format (yuv_frame_ok): planes present, a depth and container of its sample
// size, c_step 1 | 2, pitches that hold a row (chroma: c_step * w / sx samples); with 2-byte samples even pointers, pitches and
// strides (bytes: any address and pitch, odd ones too).  Without a format: 4:2:0.
static inline bool yuv_planes_ok(const YuvPlanes& p, int w, int format) {
    const int64_t S = p.sample_bytes;
    if ((S != 1 && S != 2) || (S == 1) != (p.bit_depth == 8) || !yuv_depth_ok(p.bit_depth, p.msb_aligned)) return false;
    if (!p.y || !p.cb || !p.cr || (p.c_step != 1 && p.c_step != 2)) return false;
    const uintptr_t bits = reinterpret_cast<uintptr_t>(p.y) | reinterpret_cast<uintptr_t>(p.cb) | reinterpret_cast<uintptr_t>(p.cr) |
                           (uintptr_t)p.y_pitch | (uintptr_t)p.c_pitch | (uintptr_t)p.y_frame | (uintptr_t)p.c_frame;
    return yuv_format_ok(format) && !(bits & (uintptr_t)(S - 1)) && p.y_pitch >= S * w && p.c_pitch >= S * p.c_step * (w / yuv_sx(format));
}
static inline bool yuv_planes_ok(const YuvPlanes& p, int w) { return yuv_planes_ok(p, w, PNP_YUV_FORMAT_420); }
static inline bool yuv_planes_ok(const pnp_yuv420_planes& p, int w) { return yuv_planes_ok(yuv_planes(p), w); }
static inline bool yuv_planes_ok(const pnp_yuv420_planes16& p, int w) { return yuv_planes_ok(yuv_planes(p), w); }
static inline bool yuv_planes_ok(const pnp_yuv420_planes& p, int w, int format) { return yuv_planes_ok(yuv_planes(p), w, format); }
static inline bool yuv_planes_ok(const pnp_yuv420_planes16& p, int w, int format) { return yuv_planes_ok(yuv_planes(p), w, format); }
// the aligned fast form of the pack kernel applies: four-sample loads (a dword | 8 bytes) of two Y rows and of the interleaved chroma
// row (c_step 2: the planes one sample apart; two-sample loads of each chroma plane with c_step 1), four pixels of two rows per thread.
// 4:2:2 loads what 4:2:0 loads, a row at a time, under the same conditions; 4:4:4 loads four samples of each chroma plane (c_step 1)
// or two four-sample loads of the pair (c_step 2), so its planar chroma needs the four-sample alignment too.  Without a format: 4:2:0.
static inline bool yuv_planes_fast(const YuvPlanes& p, int w, int format) {
    const uintptr_t S = (uintptr_t)p.sample_bytes, four = 4 * S - 1, two = format == PNP_YUV_FORMAT_444 ? four : 2 * S - 1;
    if ((w & 3) || ((reinterpret_cast<uintptr_t>(p.y) | (uintptr_t)p.y_pitch | (uintptr_t)p.y_frame) & four)) return false;
    const uintptr_t cb = reinterpret_cast<uintptr_t>(p.cb), cr = reinterpret_cast<uintptr_t>(p.cr);
    if (p.c_step == 2) {
        const uintptr_t lo = cb < cr ? cb : cr, hi = cb < cr ? cr : cb;
        return hi - lo == S && !((lo | (uintptr_t)p.c_pitch | (uintptr_t)p.c_frame) & four);
    }
    return !((cb | cr | (uintptr_t)p.c_pitch | (uintptr_t)p.c_frame) & two);
}
static inline bool yuv_planes_fast(const YuvPlanes& p, int w) { return yuv_planes_fast(p, w, PNP_YUV_FORMAT_420); }

// frame i of a clip's planes
static inline YuvPlanes yuv_frame(const YuvPlanes& p, int64_t i) {
    YuvPlanes q = p;
    q.y += i * p.y_frame, q.cb += i * p.c_frame, q.cr += i * p.c_frame;
    return q;
}

// T frames of planes -> the (T,H,W,4) RGB0 conv source (clamped fp32 RGB, 4th channel zero).  1.5 samples (4:2:2: 2, 4:4:4: 3) read +
// 16 B written per pixel.  k.format is the planes' chroma format in all three launchers (the `420` in their names is historical).
// force_general: the single-sample-load form even where the aligned one applies (same values; tests).  k.chroma selects the kernels
// here and in the two launchers below: PNP_YUV_CHROMA_REPLICATE the replicate / box ones, every other mode the sited ones
int launch_pack_lr_yuv420(const YuvPlanes& in, const YuvCoef& k, float* lr4, int T, int H, int W, bool force_general, hipStream_t stream);
// n frames of planes <-> (n,3,H,W) fp32 planes; any address and pitch yuv_planes_ok admits, bytes beyond a row's width are neither
// read nor written
int launch_frames_from_yuv420(const YuvPlanes& in, const YuvCoef& k, float* out, int nframes, int H, int W, hipStream_t stream);
int launch_frames_to_yuv420(const float* in, const YuvPlanes& out, const YuvCoef& k, int nframes, int H, int W, hipStream_t stream);
