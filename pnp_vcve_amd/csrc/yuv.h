// Y'CbCr 4:2:0 boundary (yuv.hip): NV12 / NV21 / I420 planes at 8 bit, P010 / P012 / yuv420p10le / yuv420p12le planes at 10 and 12
// bit <-> fp32 RGB.  The arithmetic is stated ONCE, in include/pnpvcve.h (pnp_frames_from_yuv420 / pnp_frames_to_yuv420,
// pnp_yuv420_planes16); tests/yuv_ref.py and tests/yuv16_ref.py restate it in numpy and the kernels are bit-equal to those.  The two
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
};
// depth 8 (low-aligned only: the sample is the byte), or 10 | 12 in a 16-bit word, low- or high-aligned
static inline bool yuv_depth_ok(int bit_depth, int msb_aligned) {
    return bit_depth == 8 ? msb_aligned == 0 : (bit_depth == 10 || bit_depth == 12) && (msb_aligned == 0 || msb_aligned == 1);
}
// `code` is what every entry takes as yuv_standard: PNP_YUV_CODE(standard, chroma), the standard 0..3 in bits 0..7 and the chroma mode
// 0..3 in bits 8..11; any other bit set (a mode above 3, a low byte above 3, bits from 12 up, a negative value) is refused
static inline bool yuv_coef(int code, int bit_depth, int msb_aligned, YuvCoef* k) {
    if ((code & ~0x303) || !yuv_depth_ok(bit_depth, msb_aligned)) return false;
    const int standard = code & 0xff;
    k->chroma = (code >> 8) & 0xf;
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

// What a descriptor must satisfy for h x w frames (h, w even): planes present, a depth and container of its sample size, c_step
// 1 | 2, pitches that hold a row; with 2-byte samples even pointers, pitches and strides (bytes: any address and pitch, odd ones too).
static inline bool yuv_planes_ok(const YuvPlanes& p, int w) {
    const int64_t S = p.sample_bytes;
    if ((S != 1 && S != 2) || (S == 1) != (p.bit_depth == 8) || !yuv_depth_ok(p.bit_depth, p.msb_aligned)) return false;
    if (!p.y || !p.cb || !p.cr || (p.c_step != 1 && p.c_step != 2)) return false;
    const uintptr_t bits = reinterpret_cast<uintptr_t>(p.y) | reinterpret_cast<uintptr_t>(p.cb) | reinterpret_cast<uintptr_t>(p.cr) |
                           (uintptr_t)p.y_pitch | (uintptr_t)p.c_pitch | (uintptr_t)p.y_frame | (uintptr_t)p.c_frame;
    return !(bits & (uintptr_t)(S - 1)) && p.y_pitch >= S * w && p.c_pitch >= S * p.c_step * (w / 2);
}
static inline bool yuv_planes_ok(const pnp_yuv420_planes& p, int w) { return yuv_planes_ok(yuv_planes(p), w); }
static inline bool yuv_planes_ok(const pnp_yuv420_planes16& p, int w) { return yuv_planes_ok(yuv_planes(p), w); }
// the aligned fast form of the pack kernel applies: four-sample loads (a dword | 8 bytes) of two Y rows and of the interleaved chroma
// row (c_step 2: the planes one sample apart; two-sample loads of each chroma plane with c_step 1), four pixels of two rows per thread
static inline bool yuv_planes_fast(const YuvPlanes& p, int w) {
    const uintptr_t S = (uintptr_t)p.sample_bytes, four = 4 * S - 1, two = 2 * S - 1;
    if ((w & 3) || ((reinterpret_cast<uintptr_t>(p.y) | (uintptr_t)p.y_pitch | (uintptr_t)p.y_frame) & four)) return false;
    const uintptr_t cb = reinterpret_cast<uintptr_t>(p.cb), cr = reinterpret_cast<uintptr_t>(p.cr);
    if (p.c_step == 2) {
        const uintptr_t lo = cb < cr ? cb : cr, hi = cb < cr ? cr : cb;
        return hi - lo == S && !((lo | (uintptr_t)p.c_pitch | (uintptr_t)p.c_frame) & four);
    }
    return !((cb | cr | (uintptr_t)p.c_pitch | (uintptr_t)p.c_frame) & two);
}

// frame i of a clip's planes
static inline YuvPlanes yuv_frame(const YuvPlanes& p, int64_t i) {
    YuvPlanes q = p;
    q.y += i * p.y_frame, q.cb += i * p.c_frame, q.cr += i * p.c_frame;
    return q;
}

// T frames of planes -> the (T,H,W,4) RGB0 conv source (clamped fp32 RGB, 4th channel zero).  1.5 samples read + 16 B written per
// pixel.  force_general: the single-sample-load form even where the aligned one applies (same values; tests).  k.chroma selects the
// kernels here and in the two launchers below: PNP_YUV_CHROMA_REPLICATE the replicate / box ones, every other mode the sited ones
int launch_pack_lr_yuv420(const YuvPlanes& in, const YuvCoef& k, float* lr4, int T, int H, int W, bool force_general, hipStream_t stream);
// n frames of planes <-> (n,3,H,W) fp32 planes; any address and pitch yuv_planes_ok admits, bytes beyond a row's width are neither
// read nor written
int launch_frames_from_yuv420(const YuvPlanes& in, const YuvCoef& k, float* out, int nframes, int H, int W, hipStream_t stream);
int launch_frames_to_yuv420(const float* in, const YuvPlanes& out, const YuvCoef& k, int nframes, int H, int W, hipStream_t stream);
