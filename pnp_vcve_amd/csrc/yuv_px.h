// The pieces of the Y'CbCr boundary's kernels (yuv.hip), each written ONCE: what a pixel, a chroma pair and a thread index go through on
// the way in (planes -> RGB) and on the way out (RGB -> planes).  No kernel and no launch here.  The arithmetic is the one
// include/pnpvcve.h states; every product and sum is an fp32 operation rounded on its own, so every function that computes carries
// `#pragma clang fp contract(off)` -- once, here, and the bit-exactness of the boundary rests on these lines alone.  Everything is a
// template on the sample type S (unsigned char | unsigned short); pitches and frame strides are bytes, c_step is samples, and only the
// loads, the extraction of a sample from a load and the store know S.
#pragma once
#include <type_traits>

#include "yuv.h"

namespace {

// The chroma mode as a template argument is PNP_YUV_CHROMA_* itself; its co-sited axes (CENTER: none; LEFT: x; TOPLEFT: both)
constexpr bool cm_xco(int CM) { return CM == PNP_YUV_CHROMA_LEFT || CM == PNP_YUV_CHROMA_TOPLEFT; }
constexpr bool cm_yco(int CM) { return CM == PNP_YUV_CHROMA_TOPLEFT; }

template <class S>
__device__ __forceinline__ const S* at(const unsigned char* p, long bytes) { return reinterpret_cast<const S*>(p + bytes); }
template <class S>
__device__ __forceinline__ S* at(unsigned char* p, long bytes) { return reinterpret_cast<S*>(p + bytes); }

// the value of a stored sample: a byte is its value, a word holds it in the container's bits
template <class S>
__device__ __forceinline__ unsigned val(const YuvCoef& k, unsigned word) {
    if constexpr (sizeof(S) == 1) return word;
    else return (word >> k.shift) & k.vmask;
}

// Four consecutive samples / two consecutive samples, loaded at once (a dword / 16 bits of bytes, 8 / 4 bytes of words), and sample j
// of such a load as it is stored
template <class S> struct Load;
template <> struct Load<unsigned char> {
    using Four = unsigned;
    using Two = unsigned short;
    static __device__ __forceinline__ unsigned get(unsigned q, int j) { return j == 3 ? q >> 24 : (q >> (8 * j)) & 255u; }
    static __device__ __forceinline__ unsigned get2(unsigned q, int j) { return j ? q >> 8 : q & 255u; }
};
template <> struct Load<unsigned short> {
    using Four = uint2;
    using Two = unsigned;
    static __device__ __forceinline__ unsigned get(uint2 q, int j) { const unsigned w = j & 2 ? q.y : q.x; return j & 1 ? w >> 16 : w & 0xffffu; }
    static __device__ __forceinline__ unsigned get2(unsigned q, int j) { return j ? q >> 16 : q & 0xffffu; }
};

// The linear thread index i over frames x nrow x ncol (columns fastest): 2x2 blocks, four-pixel groups or the chroma samples of a row
struct Idx { long f; int row, col; };
__device__ __forceinline__ Idx split(long i, int nrow, int ncol) {
    const int col = (int)(i % ncol);
    const long r = i / ncol;
    return Idx{r / nrow, (int)(r % nrow), col};
}

// ---- the way in
// the chroma terms of a chroma sample, shared by the pixels that replicate it
struct ChromaTerms { float rv, gu, gv, bu; };
__device__ __forceinline__ ChromaTerms chroma_terms(const YuvCoef& k, unsigned cb, unsigned cr) {
#pragma clang fp contract(off)
    const float u = (float)((int)cb - k.cmid), v = (float)((int)cr - k.cmid);
    return ChromaTerms{k.crv * v, k.cgu * u, k.cgv * v, k.cbu * u};
}
// the chroma terms of ONE pixel from its weighted sums of 16 (exact in fp32: below 2^16 at 12 bit)
__device__ __forceinline__ ChromaTerms chroma_terms16(const YuvCoef& k, int cb16, int cr16) {
#pragma clang fp contract(off)
    const float u = (float)(cb16 - 16 * k.cmid) * 0.0625f, v = (float)(cr16 - 16 * k.cmid) * 0.0625f;
    return ChromaTerms{k.crv * v, k.cgu * u, k.cgv * v, k.cbu * u};
}
__device__ __forceinline__ f32x4 rgb0_of(const YuvCoef& k, unsigned Y, const ChromaTerms& c) {
#pragma clang fp contract(off)
    const float y = k.cy * (float)((int)Y - k.yoff);
    const float r = y + c.rv, g = (y - c.gu) - c.gv, b = y + c.bu;
    const f32x4 o = {fminf(fmaxf(r, 0.f), 1.f), fminf(fmaxf(g, 0.f), 1.f), fminf(fmaxf(b, 0.f), 1.f), 0.f};
    return o;
}

// Sited chroma (PNP_YUV_CHROMA_CENTER | _LEFT | _TOPLEFT).  One axis, weights in quarters: the even and the odd luma index of chroma
// index i, from the samples m, c, p at max(i - 1, 0), i, min(i + 1, n - 1).  CO: the axis is co-sited (even: c alone; odd: halfway to
// p), else midway (3 : 1 towards the nearer neighbour).  Both axes together weigh 16 and the sum is an integer.
template <bool CO> __device__ __forceinline__ int tap_even(int m, int c) { return CO ? 4 * c : 3 * c + m; }
template <bool CO> __device__ __forceinline__ int tap_odd(int c, int p) { return CO ? 2 * c + 2 * p : 3 * c + p; }

// The aligned forms' chroma of the columns 2 gx and 2 gx + 1 of the chroma row at byte offset co: one four-sample load of the
// interleaved pair (STEP 2: samples a0 b0 a1 b1 of the plane that starts first; cr_first says which one that is) or one two-sample
// load of each plane (STEP 1).  As stored: val<S> has not been applied.
template <class S, int STEP>
__device__ __forceinline__ void load_pairs(const YuvPlanes& p, long co, int gx, int cr_first, unsigned (&cb)[2], unsigned (&cr)[2]) {
    using L = Load<S>;
    if constexpr (STEP == 2) {
        const typename L::Four q = *at<typename L::Four>(cr_first ? p.cr : p.cb, co + (long)sizeof(S) * (4 * gx));
        const unsigned a0 = L::get(q, 0), b0 = L::get(q, 1), a1 = L::get(q, 2), b1 = L::get(q, 3);
        cb[0] = cr_first ? b0 : a0, cr[0] = cr_first ? a0 : b0;
        cb[1] = cr_first ? b1 : a1, cr[1] = cr_first ? a1 : b1;
    } else {
        const long cx = co + (long)sizeof(S) * (2 * gx);
        const unsigned qb = *at<typename L::Two>(p.cb, cx), qr = *at<typename L::Two>(p.cr, cx);
        cb[0] = L::get2(qb, 0), cb[1] = L::get2(qb, 1), cr[0] = L::get2(qr, 0), cr[1] = L::get2(qr, 1);
    }
}

// The chroma terms of the four pixels (00, 01, 10, 11) of the 2x2 block (by, bx) of frame f at 4:2:0 in mode CM, from single-sample
// loads at any address, pitch and c_step.  REPLICATE: the block's own pair.  Sited: the clamped 3x3 neighbourhood, rows across first (a
// co-sited axis has no tap at index - 1: its loads fold into the centre's).
template <class S, int CM>
__device__ __forceinline__ void block_terms(const YuvPlanes& p, const YuvCoef& k, long f, int by, int bx, int bh, int bw, ChromaTerms (&c)[4]) {
    if constexpr (CM == PNP_YUV_CHROMA_REPLICATE) {
        const long co = f * p.c_frame + (long)by * p.c_pitch;
        const long cx = (long)bx * p.c_step;
        c[0] = c[1] = c[2] = c[3] = chroma_terms(k, val<S>(k, at<S>(p.cb, co)[cx]), val<S>(k, at<S>(p.cr, co)[cx]));
    } else {
        constexpr bool XCO = cm_xco(CM), YCO = cm_yco(CM);
        const int rows[3] = {YCO ? by : max(by - 1, 0), by, min(by + 1, bh - 1)};
        const long cols[3] = {(long)(XCO ? bx : max(bx - 1, 0)) * p.c_step, (long)bx * p.c_step, (long)min(bx + 1, bw - 1) * p.c_step};
        int be[3], bo[3], re[3], ro[3];     // each row across: the even and the odd column, cb and cr
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const long co = f * p.c_frame + (long)rows[r] * p.c_pitch;
            const S *b = at<S>(p.cb, co), *q = at<S>(p.cr, co);
            const int bm = (int)val<S>(k, b[cols[0]]), bc = (int)val<S>(k, b[cols[1]]), bp = (int)val<S>(k, b[cols[2]]);
            const int rm = (int)val<S>(k, q[cols[0]]), rc = (int)val<S>(k, q[cols[1]]), rp = (int)val<S>(k, q[cols[2]]);
            be[r] = tap_even<XCO>(bm, bc), bo[r] = tap_odd<XCO>(bc, bp);
            re[r] = tap_even<XCO>(rm, rc), ro[r] = tap_odd<XCO>(rc, rp);
        }
        c[0] = chroma_terms16(k, tap_even<YCO>(be[0], be[1]), tap_even<YCO>(re[0], re[1]));
        c[1] = chroma_terms16(k, tap_even<YCO>(bo[0], bo[1]), tap_even<YCO>(ro[0], ro[1]));
        c[2] = chroma_terms16(k, tap_odd<YCO>(be[1], be[2]), tap_odd<YCO>(re[1], re[2]));
        c[3] = chroma_terms16(k, tap_odd<YCO>(bo[1], bo[2]), tap_odd<YCO>(ro[1], ro[2]));
    }
}

// 4:2:2 and 4:4:4: chroma rows are luma rows, so no vertical tap; SX is the horizontal factor, 2 | 1.  XM is what the x axis does with
// the mode:
//   XM_PLAIN   replication on the way in, (p0 + p1) * 0.5 on the way out -- and everything at SX = 1, where every mode is the pixel's
//              own sample both ways (the sited sum is 16 (C - mid), and float(16 n) * 0.0625f = float(n) exactly)
//   XM_MIDWAY  planes -> RGB with the midway taps (CENTER); its way out is XM_PLAIN's
//   XM_COSITED the co-sited taps both ways (LEFT and TOPLEFT: the same function with no vertical axis to tell them apart)
// The y axis weighs 4 in the sums of 16.
enum { XM_PLAIN = 0, XM_MIDWAY = 1, XM_COSITED = 2 };

// the chroma terms of the SX pixels of chroma sample bx from the samples (bm, rm) left of it, its own (bc, rc) and (bp, rp) right of it
template <int SX, int XM>
__device__ __forceinline__ void row_terms(const YuvCoef& k, int bm, int bc, int bp, int rm, int rc, int rp, ChromaTerms (&c)[SX]) {
    if constexpr (XM == XM_PLAIN) {
        c[0] = chroma_terms(k, (unsigned)bc, (unsigned)rc);
        if constexpr (SX == 2) c[1] = c[0];
    } else {
        constexpr bool XCO = XM == XM_COSITED;
        c[0] = chroma_terms16(k, 4 * tap_even<XCO>(bm, bc), 4 * tap_even<XCO>(rm, rc));
        c[1] = chroma_terms16(k, 4 * tap_odd<XCO>(bc, bp), 4 * tap_odd<XCO>(rc, rp));
    }
}

// Where pixel (y, x) of frame f lies in the (T,H,W,4) RGB0 conv source (PLANAR false) or in (n,3,H,W) fp32 planes (PLANAR true: its R,
// with G and B H * W floats apart), and the store of the pixel dy rows and dx columns further on
template <bool PLANAR>
__device__ __forceinline__ float* px_at(float* out, long f, int H, int W, int y, int x) {
    if constexpr (PLANAR) return out + f * 3 * ((long)H * W) + (long)y * W + x;
    else return out + 4 * ((f * H + y) * W + x);
}
template <bool PLANAR>
__device__ __forceinline__ void store_px(float* d, int H, int W, int dy, int dx, const f32x4& v) {
    if constexpr (PLANAR) {
        const long hw = (long)H * W;
        float* q = d + dy * W + dx;
        q[0] = v[0];
        q[hw] = v[1];
        q[2 * hw] = v[2];
    } else {
        reinterpret_cast<f32x4*>(d)[dy * W + dx] = v;
    }
}
// the aligned forms' four pixels of a row: four 16-byte stores, 64 contiguous bytes
__device__ __forceinline__ void store_group(float* d, const f32x4 (&t)[4]) {
    f32x4* q = reinterpret_cast<f32x4*>(d);
    q[0] = t[0];
    q[1] = t[1];
    q[2] = t[2];
    q[3] = t[3];
}

// ---- the way out
// clamp(rint(x), 0, 2^d - 1), rint rounding half to even, as it is stored: a byte, or a word with the bits outside the value zero
template <class S>
__device__ __forceinline__ S sample_of(const YuvCoef& k, float x) {
    const float v = fminf(fmaxf(rintf(x), 0.f), k.vmax);
    if constexpr (sizeof(S) == 1) return (S)v;
    else return (S)((unsigned)v << k.shift);
}

// One pixel of (n,3,H,W) fp32 planes, q its R with G and B hw floats apart: clamp, luma, the colour differences; its Y sample goes to
// *y where `store` says so (a thread evaluates the pixels beside the ones it owns without storing them)
struct PbPr { float yl, pb, pr; };
template <class S>
__device__ __forceinline__ PbPr px_out(const YuvCoef& k, const float* q, long hw, S* y, bool store) {
#pragma clang fp contract(off)
    const float rr = fminf(fmaxf(q[0], 0.f), 1.f), gg = fminf(fmaxf(q[hw], 0.f), 1.f), bb = fminf(fmaxf(q[2 * hw], 0.f), 1.f);
    const float yl = (k.kr * rr + k.kg * gg) + k.kb * bb;
    if (store) *y = sample_of<S>(k, (float)k.yoff + k.sy * yl);
    return PbPr{yl, (bb - yl) * k.ipb, (rr - yl) * k.ipr};
}
// [1 2 1] / 4 of a co-sited axis
__device__ __forceinline__ float tap121(float l, float c, float r) {
#pragma clang fp contract(off)
    return ((l + r) + (c + c)) * 0.25f;
}
// the chroma pair (mean pb, mean pr) of chroma sample cx of the chroma row at byte offset co
template <class S>
__device__ __forceinline__ void store_chroma(const YuvPlanes& p, const YuvCoef& k, long co, long cx, float mb, float mr) {
#pragma clang fp contract(off)
    at<S>(p.cb, co)[cx] = sample_of<S>(k, (float)k.cmid + k.sc * mb);
    at<S>(p.cr, co)[cx] = sample_of<S>(k, (float)k.cmid + k.sc * mr);
}

}  // namespace
