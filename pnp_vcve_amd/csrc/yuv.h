// Y'CbCr 4:2:0 boundary (yuv.hip): NV12 / NV21 / I420 planes <-> fp32 RGB.  The arithmetic is stated ONCE, in include/pnpvcve.h
// (pnp_frames_from_yuv420 / pnp_frames_to_yuv420); tests/yuv_ref.py restates it in numpy and the kernels are bit-equal to that.
#pragma once
#include "common.h"

// Every constant of a standard: evaluated in double from Kr, Kb and rounded to fp32 once (yuv_coef), on the host.
struct YuvCoef {
    float cy, crv, cbu, cgu, cgv;       // bytes -> RGB
    float kr, kg, kb, sy, sc, ipb, ipr; // RGB -> bytes: luma weights, scales, 0.5 / (1 - Kb), 0.5 / (1 - Kr)
    int yoff;
};
static inline bool yuv_coef(int standard, YuvCoef* k) {
    if (standard < PNP_YUV_BT601_LIMITED || standard > PNP_YUV_BT709_FULL) return false;
    const bool bt709 = standard >= PNP_YUV_BT709_LIMITED, full = (standard & 1) != 0;
    const double Kr = bt709 ? 0.2126 : 0.299, Kb = bt709 ? 0.0722 : 0.114, Kg = 1.0 - Kr - Kb;
    const double sy = full ? 255.0 : 219.0, sc = full ? 255.0 : 224.0;
    k->cy = (float)(1.0 / sy);
    k->crv = (float)(2.0 * (1.0 - Kr) / sc);
    k->cbu = (float)(2.0 * (1.0 - Kb) / sc);
    k->cgu = (float)(2.0 * Kb * (1.0 - Kb) / (Kg * sc));
    k->cgv = (float)(2.0 * Kr * (1.0 - Kr) / (Kg * sc));
    k->kr = (float)Kr, k->kg = (float)Kg, k->kb = (float)Kb;
    k->sy = (float)sy, k->sc = (float)sc;
    k->ipb = (float)(0.5 / (1.0 - Kb)), k->ipr = (float)(0.5 / (1.0 - Kr));
    k->yoff = full ? 0 : 16;
    return true;
}

// What a descriptor must satisfy for h x w frames (h, w even): planes present, c_step 1 | 2, pitches that hold a row.
static inline bool yuv_planes_ok(const pnp_yuv420_planes& p, int w) {
    return p.y && p.cb && p.cr && (p.c_step == 1 || p.c_step == 2) && p.y_pitch >= w && p.c_pitch >= (int64_t)p.c_step * (w / 2);
}
// the aligned fast form of the pack kernel applies: dword loads of two Y rows and of the interleaved chroma row (c_step 2; 16-bit
// loads of each chroma plane with c_step 1), four pixels of two rows per thread
static inline bool yuv_planes_fast(const pnp_yuv420_planes& p, int w) {
    if ((w & 3) || ((reinterpret_cast<uintptr_t>(p.y) | (uintptr_t)p.y_pitch | (uintptr_t)p.y_frame) & 3)) return false;
    const uintptr_t cb = reinterpret_cast<uintptr_t>(p.cb), cr = reinterpret_cast<uintptr_t>(p.cr);
    if (p.c_step == 2) {
        const uintptr_t lo = cb < cr ? cb : cr, hi = cb < cr ? cr : cb;
        return hi - lo == 1 && !((lo | (uintptr_t)p.c_pitch | (uintptr_t)p.c_frame) & 3);
    }
    return !((cb | cr | (uintptr_t)p.c_pitch | (uintptr_t)p.c_frame) & 1);
}

// frame i of a clip's planes
static inline pnp_yuv420_planes yuv_frame(const pnp_yuv420_planes& p, int64_t i) {
    pnp_yuv420_planes q = p;
    q.y += i * p.y_frame, q.cb += i * p.c_frame, q.cr += i * p.c_frame;
    return q;
}

// T frames of planes -> the (T,H,W,4) RGB0 conv source (clamped fp32 RGB, 4th channel zero).  1.5 B read + 16 B written per pixel.
// force_general: the byte-load form even where the aligned one applies (same values; tests)
int launch_pack_lr_yuv420(const pnp_yuv420_planes& in, const YuvCoef& k, float* lr4, int T, int H, int W, bool force_general, hipStream_t stream);
// n frames of planes <-> (n,3,H,W) fp32 planes; any address and pitch, bytes beyond a row's width are neither read nor written
int launch_frames_from_yuv420(const pnp_yuv420_planes& in, const YuvCoef& k, float* out, int nframes, int H, int W, hipStream_t stream);
int launch_frames_to_yuv420(const float* in, const pnp_yuv420_planes& out, const YuvCoef& k, int nframes, int H, int W, hipStream_t stream);
