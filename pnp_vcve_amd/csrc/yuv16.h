// 10 / 12-bit Y'CbCr 4:2:0 boundary (yuv16.hip): P010 / P012 / yuv420p10le / yuv420p12le planes <-> fp32 RGB.  The arithmetic is
// stated ONCE, in include/pnpvcve.h (pnp_yuv420_planes16); tests/yuv16_ref.py restates it in numpy and the kernels are bit-equal to
// that.  The formulas are yuv.h's with the constants of the depth; only the sample container is new.
#pragma once
#include "yuv.h"

// The constants of a standard at depth d (yuv.h's YuvCoef, the chroma midpoint and the top code beside it) and the container: a word
// reads as (word >> shift) & vmask and is written as value << shift.
struct YuvCoef16 {
    YuvCoef k;
    int cmid;           // 2^(d-1)
    float vmax;         // 2^d - 1
    unsigned shift;     // 0 (low-aligned) | 16 - d (high-aligned)
    unsigned vmask;     // 2^d - 1
};
static inline bool yuv_depth_ok(int bit_depth, int msb_aligned) { return (bit_depth == 10 || bit_depth == 12) && (msb_aligned == 0 || msb_aligned == 1); }
static inline bool yuv_coef16(int standard, int bit_depth, int msb_aligned, YuvCoef16* c) {
    if (standard < PNP_YUV_BT601_LIMITED || standard > PNP_YUV_BT709_FULL || !yuv_depth_ok(bit_depth, msb_aligned)) return false;
    const bool bt709 = standard >= PNP_YUV_BT709_LIMITED, full = (standard & 1) != 0;
    const double Kr = bt709 ? 0.2126 : 0.299, Kb = bt709 ? 0.0722 : 0.114, Kg = 1.0 - Kr - Kb;
    const double s = (double)(1 << (bit_depth - 8)), top = (double)((1 << bit_depth) - 1);
    const double sy = full ? top : 219.0 * s, sc = full ? top : 224.0 * s;
    YuvCoef* k = &c->k;
    k->cy = (float)(1.0 / sy);
    k->crv = (float)(2.0 * (1.0 - Kr) / sc);
    k->cbu = (float)(2.0 * (1.0 - Kb) / sc);
    k->cgu = (float)(2.0 * Kb * (1.0 - Kb) / (Kg * sc));
    k->cgv = (float)(2.0 * Kr * (1.0 - Kr) / (Kg * sc));
    k->kr = (float)Kr, k->kg = (float)Kg, k->kb = (float)Kb;
    k->sy = (float)sy, k->sc = (float)sc;
    k->ipb = (float)(0.5 / (1.0 - Kb)), k->ipr = (float)(0.5 / (1.0 - Kr));
    k->yoff = full ? 0 : 16 << (bit_depth - 8);
    c->cmid = 1 << (bit_depth - 1);
    c->vmax = (float)top;
    c->shift = msb_aligned ? 16u - (unsigned)bit_depth : 0u;
    c->vmask = (1u << bit_depth) - 1u;
    return true;
}

// What a descriptor must satisfy for h x w frames (h, w even): planes present, depth and container known, c_step 1 | 2, even pointers,
// pitches and strides, pitches that hold a row.
static inline bool yuv16_planes_ok(const pnp_yuv420_planes16& p, int w) {
    if (!p.y || !p.cb || !p.cr || !yuv_depth_ok(p.bit_depth, p.msb_aligned) || (p.c_step != 1 && p.c_step != 2)) return false;
    const uintptr_t bits = reinterpret_cast<uintptr_t>(p.y) | reinterpret_cast<uintptr_t>(p.cb) | reinterpret_cast<uintptr_t>(p.cr) |
                           (uintptr_t)p.y_pitch | (uintptr_t)p.c_pitch | (uintptr_t)p.y_frame | (uintptr_t)p.c_frame;
    return !(bits & 1) && p.y_pitch >= 2 * (int64_t)w && p.c_pitch >= 2 * (int64_t)p.c_step * (w / 2);
}
// the aligned fast form of the pack kernel applies: 8-byte loads of two Y rows and of the interleaved chroma row (c_step 2; 4-byte
// loads of each chroma plane with c_step 1), four pixels of two rows per thread
static inline bool yuv16_planes_fast(const pnp_yuv420_planes16& p, int w) {
    if ((w & 3) || ((reinterpret_cast<uintptr_t>(p.y) | (uintptr_t)p.y_pitch | (uintptr_t)p.y_frame) & 7)) return false;
    const uintptr_t cb = reinterpret_cast<uintptr_t>(p.cb), cr = reinterpret_cast<uintptr_t>(p.cr);
    if (p.c_step == 2) {
        const uintptr_t lo = cb < cr ? cb : cr, hi = cb < cr ? cr : cb;
        return hi - lo == 2 && !((lo | (uintptr_t)p.c_pitch | (uintptr_t)p.c_frame) & 7);
    }
    return !((cb | cr | (uintptr_t)p.c_pitch | (uintptr_t)p.c_frame) & 3);
}

// frame i of a clip's planes (strides are bytes)
static inline pnp_yuv420_planes16 yuv16_frame(const pnp_yuv420_planes16& p, int64_t i) {
    pnp_yuv420_planes16 q = p;
    q.y = reinterpret_cast<unsigned short*>(reinterpret_cast<char*>(p.y) + i * p.y_frame);
    q.cb = reinterpret_cast<unsigned short*>(reinterpret_cast<char*>(p.cb) + i * p.c_frame);
    q.cr = reinterpret_cast<unsigned short*>(reinterpret_cast<char*>(p.cr) + i * p.c_frame);
    return q;
}

// yuv.h's three launchers on 16-bit planes.  3 B read + 16 B written per pixel for the pack launch.
int launch_pack_lr_yuv420p16(const pnp_yuv420_planes16& in, const YuvCoef16& k, float* lr4, int T, int H, int W, bool force_general, hipStream_t stream);
int launch_frames_from_yuv420p16(const pnp_yuv420_planes16& in, const YuvCoef16& k, float* out, int nframes, int H, int W, hipStream_t stream);
int launch_frames_to_yuv420p16(const float* in, const pnp_yuv420_planes16& out, const YuvCoef16& k, int nframes, int H, int W, hipStream_t stream);
