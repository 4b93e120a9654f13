// Y'CbCr boundary (the 4:2:0 kernels first; the 4:2:2 and 4:4:4 ones, which own pixels of one row, behind them).
// 4:2:0: the decoder's planes straight into the conv source, and fp32 RGB planes out as planes an encoder or a display
// takes -- NV12 / NV21 / I420 bytes, or the 16-bit words a Main10 / VVC decoder writes (P010 / P012: the value in the high bits;
// yuv420p10le / yuv420p12le: in the low bits).  The arithmetic is the one include/pnpvcve.h states (pnp_frames_from_yuv420 /
// pnp_frames_to_yuv420, pnp_yuv420_planes16): constants of the depth rounded to fp32 once on the host (yuv.h), every product and sum
// after that an fp32 operation rounded on its own -- contraction is off in every function that computes.  Chroma is replicated on the
// way in (pixel (y, x) reads sample (y >> 1, x >> 1)) and box-averaged on the way out, so a thread owns whole 2x2 blocks and reads
// each chroma pair once.  The other chroma modes of the header (PNP_YUV_CHROMA_CENTER / _LEFT / _TOPLEFT: bilinear chroma at its true
// position on the way in, [1 2 1] / 4 on the co-sited axes on the way out) have kernels of their own below (the *_sited_* ones): a
// thread still owns whole 2x2 blocks and reads the clamped neighbours it needs beside them.  Every kernel is a template on the sample
// type S (unsigned char | unsigned short); pitches and frame strides are bytes, c_step is samples, and only the loads, the extraction
// of a sample from a load and the store know S.
#include <type_traits>

#include "yuv.h"

namespace {

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

// the chroma terms of a 2x2 block, shared by its four pixels
struct ChromaTerms { float rv, gu, gv, bu; };
__device__ __forceinline__ ChromaTerms chroma_terms(const YuvCoef& k, unsigned cb, unsigned cr) {
#pragma clang fp contract(off)
    const float u = (float)((int)cb - k.cmid), v = (float)((int)cr - k.cmid);
    return ChromaTerms{k.crv * v, k.cgu * u, k.cgv * v, k.cbu * u};
}
__device__ __forceinline__ f32x4 rgb0_of(const YuvCoef& k, unsigned Y, const ChromaTerms& c) {
#pragma clang fp contract(off)
    const float y = k.cy * (float)((int)Y - k.yoff);
    const float r = y + c.rv, g = (y - c.gu) - c.gv, b = y + c.bu;
    const f32x4 o = {fminf(fmaxf(r, 0.f), 1.f), fminf(fmaxf(g, 0.f), 1.f), fminf(fmaxf(b, 0.f), 1.f), 0.f};
    return o;
}

// General form: one thread = one 2x2 block, single-sample loads at any address and pitch yuv_planes_ok admits.
// i over T * (H/2) * (W/2).
template <class S>
__global__ __launch_bounds__(256) void pack_lr_yuv420_kernel(const YuvPlanes p, const YuvCoef k, float* __restrict__ lr4, int H, int W, long total) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int bw = W >> 1, bh = H >> 1;
    const int bx = (int)(i % bw);
    const long r = i / bw;
    const int by = (int)(r % bh);
    const long f = r / bh;
    const S* y0 = at<S>(p.y, f * p.y_frame + (long)(2 * by) * p.y_pitch) + 2 * bx;
    const S* y1 = at<S>(reinterpret_cast<const unsigned char*>(y0), p.y_pitch);
    const long co = f * p.c_frame + (long)by * p.c_pitch;
    const long cx = (long)bx * p.c_step;
    const ChromaTerms c = chroma_terms(k, val<S>(k, at<S>(p.cb, co)[cx]), val<S>(k, at<S>(p.cr, co)[cx]));
    f32x4* d = reinterpret_cast<f32x4*>(lr4) + (f * H + 2 * by) * W + 2 * bx;
    const unsigned y00 = y0[0], y01 = y0[1], y10 = y1[0], y11 = y1[1];
    d[0] = rgb0_of(k, val<S>(k, y00), c);
    d[1] = rgb0_of(k, val<S>(k, y01), c);
    d[W] = rgb0_of(k, val<S>(k, y10), c);
    d[W + 1] = rgb0_of(k, val<S>(k, y11), c);
}

// Aligned fast form (yuv_planes_fast): one thread = two rows of four pixels = two four-sample loads of Y, one four-sample load of the
// interleaved chroma row (STEP 2: samples a0 b0 a1 b1 of the plane that starts first; cr_first says which one that is) or one
// two-sample load of each chroma plane (STEP 1), and eight 16-byte stores, 64 contiguous bytes per row.  W is a multiple of 4.
// i over T * (H/2) * (W/4).
template <class S, int STEP>
__global__ __launch_bounds__(256) void pack_lr_yuv420_fast_kernel(const YuvPlanes p, const YuvCoef k, float* __restrict__ lr4, int H, int W, int cr_first,
                                                                  long total) {
    using L = Load<S>;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int gw = W >> 2, bh = H >> 1;
    const int gx = (int)(i % gw);
    const long r = i / gw;
    const int by = (int)(r % bh);
    const long f = r / bh;
    const unsigned char* yp = p.y + f * p.y_frame + (long)(2 * by) * p.y_pitch + (long)sizeof(S) * (4 * gx);
    const typename L::Four ya = *at<typename L::Four>(yp, 0), yb = *at<typename L::Four>(yp, p.y_pitch);
    unsigned cb0, cr0, cb1, cr1;
    const long co = f * p.c_frame + (long)by * p.c_pitch;
    if (STEP == 2) {
        const typename L::Four q = *at<typename L::Four>(cr_first ? p.cr : p.cb, co + (long)sizeof(S) * (4 * gx));
        const unsigned a0 = L::get(q, 0), b0 = L::get(q, 1), a1 = L::get(q, 2), b1 = L::get(q, 3);
        cb0 = cr_first ? b0 : a0, cr0 = cr_first ? a0 : b0;
        cb1 = cr_first ? b1 : a1, cr1 = cr_first ? a1 : b1;
    } else {
        const long cx = co + (long)sizeof(S) * (2 * gx);
        const unsigned qb = *at<typename L::Two>(p.cb, cx), qr = *at<typename L::Two>(p.cr, cx);
        cb0 = L::get2(qb, 0), cb1 = L::get2(qb, 1), cr0 = L::get2(qr, 0), cr1 = L::get2(qr, 1);
    }
    const ChromaTerms c0 = chroma_terms(k, val<S>(k, cb0), val<S>(k, cr0)), c1 = chroma_terms(k, val<S>(k, cb1), val<S>(k, cr1));
    f32x4* d = reinterpret_cast<f32x4*>(lr4) + (f * H + 2 * by) * W + 4 * gx;
    const f32x4 t0 = rgb0_of(k, val<S>(k, L::get(ya, 0)), c0), t1 = rgb0_of(k, val<S>(k, L::get(ya, 1)), c0);
    const f32x4 t2 = rgb0_of(k, val<S>(k, L::get(ya, 2)), c1), t3 = rgb0_of(k, val<S>(k, L::get(ya, 3)), c1);
    const f32x4 u0 = rgb0_of(k, val<S>(k, L::get(yb, 0)), c0), u1 = rgb0_of(k, val<S>(k, L::get(yb, 1)), c0);
    const f32x4 u2 = rgb0_of(k, val<S>(k, L::get(yb, 2)), c1), u3 = rgb0_of(k, val<S>(k, L::get(yb, 3)), c1);
    d[0] = t0;
    d[1] = t1;
    d[2] = t2;
    d[3] = t3;
    d[W] = u0;
    d[W + 1] = u1;
    d[W + 2] = u2;
    d[W + 3] = u3;
}

// planes -> (n,3,H,W) fp32 planes: the general form's loads, the same values
template <class S>
__global__ __launch_bounds__(256) void frames_from_yuv420_kernel(const YuvPlanes p, const YuvCoef k, float* __restrict__ out, int H, int W, long total) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int bw = W >> 1, bh = H >> 1;
    const int bx = (int)(i % bw);
    const long r = i / bw;
    const int by = (int)(r % bh);
    const long f = r / bh;
    const long yo = f * p.y_frame + (long)(2 * by) * p.y_pitch;
    const long co = f * p.c_frame + (long)by * p.c_pitch;
    const long cx = (long)bx * p.c_step;
    const ChromaTerms c = chroma_terms(k, val<S>(k, at<S>(p.cb, co)[cx]), val<S>(k, at<S>(p.cr, co)[cx]));
    const long hw = (long)H * W;
    float* d = out + f * 3 * hw + (long)(2 * by) * W + 2 * bx;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int dy = j >> 1, dx = j & 1;
        const f32x4 v = rgb0_of(k, val<S>(k, at<S>(p.y, yo + dy * p.y_pitch)[2 * bx + dx]), c);
        float* q = d + dy * W + dx;
        q[0] = v[0];
        q[hw] = v[1];
        q[2 * hw] = v[2];
    }
}

// ---- sited chroma on the way in (PNP_YUV_CHROMA_CENTER | _LEFT | _TOPLEFT).  One axis, weights in quarters: the even and the odd
// luma index of chroma index i, from the samples m, c, p at max(i - 1, 0), i, min(i + 1, n - 1).  CO: the axis is co-sited (even: c
// alone; odd: halfway to p), else midway (3 : 1 towards the nearer neighbour).  Both axes together weigh 16 and the sum is an integer.
template <bool CO> __device__ __forceinline__ int tap_even(int m, int c) { return CO ? 4 * c : 3 * c + m; }
template <bool CO> __device__ __forceinline__ int tap_odd(int c, int p) { return CO ? 2 * c + 2 * p : 3 * c + p; }

// the chroma terms of ONE pixel from its weighted sums of 16 (exact in fp32: below 2^16 at 12 bit)
__device__ __forceinline__ ChromaTerms chroma_terms16(const YuvCoef& k, int cb16, int cr16) {
#pragma clang fp contract(off)
    const float u = (float)(cb16 - 16 * k.cmid) * 0.0625f, v = (float)(cr16 - 16 * k.cmid) * 0.0625f;
    return ChromaTerms{k.crv * v, k.cgu * u, k.cgv * v, k.cbu * u};
}

// The chroma terms of the four pixels (00, 01, 10, 11) of block (by, bx) of frame f: single-sample loads of the clamped 3x3
// neighbourhood (a co-sited axis has no tap at index - 1: its loads fold into the centre's), at any address, pitch and c_step.
template <class S, bool XCO, bool YCO>
__device__ __forceinline__ void sited_terms(const YuvPlanes& p, const YuvCoef& k, long f, int by, int bx, int bh, int bw, ChromaTerms (&c)[4]) {
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

// General sited form: pack_lr_yuv420_kernel's thread, loads of Y and stores, with sited_terms' chroma
template <class S, bool XCO, bool YCO>
__global__ __launch_bounds__(256) void pack_lr_yuv420_sited_kernel(const YuvPlanes p, const YuvCoef k, float* __restrict__ lr4, int H, int W, long total) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int bw = W >> 1, bh = H >> 1;
    const int bx = (int)(i % bw);
    const long r = i / bw;
    const int by = (int)(r % bh);
    const long f = r / bh;
    const S* y0 = at<S>(p.y, f * p.y_frame + (long)(2 * by) * p.y_pitch) + 2 * bx;
    const S* y1 = at<S>(reinterpret_cast<const unsigned char*>(y0), p.y_pitch);
    ChromaTerms c[4];
    sited_terms<S, XCO, YCO>(p, k, f, by, bx, bh, bw, c);
    f32x4* d = reinterpret_cast<f32x4*>(lr4) + (f * H + 2 * by) * W + 2 * bx;
    const unsigned y00 = y0[0], y01 = y0[1], y10 = y1[0], y11 = y1[1];
    d[0] = rgb0_of(k, val<S>(k, y00), c[0]);
    d[1] = rgb0_of(k, val<S>(k, y01), c[1]);
    d[W] = rgb0_of(k, val<S>(k, y10), c[2]);
    d[W + 1] = rgb0_of(k, val<S>(k, y11), c[3]);
}

// Aligned sited form (yuv_planes_fast): pack_lr_yuv420_fast_kernel's thread -- two four-sample loads of Y, eight 16-byte stores, 64
// contiguous bytes per row -- with the chroma of its two columns loaded as there, once per row of the clamped rows by - 1, by, by + 1
// (a pitch that is aligned keeps every row's load aligned), and the clamped columns 2 gx - 1 and 2 gx + 2 beside them as single
// samples.  The same integers as the general form, so the same values.
template <class S, int STEP, bool XCO, bool YCO>
__global__ __launch_bounds__(256) void pack_lr_yuv420_sited_fast_kernel(const YuvPlanes p, const YuvCoef k, float* __restrict__ lr4, int H, int W,
                                                                        int cr_first, long total) {
    using L = Load<S>;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int gw = W >> 2, bh = H >> 1, bw = W >> 1;
    const int gx = (int)(i % gw);
    const long r = i / gw;
    const int by = (int)(r % bh);
    const long f = r / bh;
    const unsigned char* yp = p.y + f * p.y_frame + (long)(2 * by) * p.y_pitch + (long)sizeof(S) * (4 * gx);
    const typename L::Four ya = *at<typename L::Four>(yp, 0), yb = *at<typename L::Four>(yp, p.y_pitch);
    const int rows[3] = {YCO ? by : max(by - 1, 0), by, min(by + 1, bh - 1)};
    const long xl = (long)(XCO ? 2 * gx : max(2 * gx - 1, 0)) * STEP, xr = (long)min(2 * gx + 2, bw - 1) * STEP;
    int hb[3][4], hr[3][4];             // each row across: the thread's four columns, cb and cr
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const long co = f * p.c_frame + (long)rows[j] * p.c_pitch;
        unsigned cb0, cr0, cb1, cr1;
        if (STEP == 2) {
            const typename L::Four q = *at<typename L::Four>(cr_first ? p.cr : p.cb, co + (long)sizeof(S) * (4 * gx));
            const unsigned a0 = L::get(q, 0), b0 = L::get(q, 1), a1 = L::get(q, 2), b1 = L::get(q, 3);
            cb0 = cr_first ? b0 : a0, cr0 = cr_first ? a0 : b0;
            cb1 = cr_first ? b1 : a1, cr1 = cr_first ? a1 : b1;
        } else {
            const long cx = co + (long)sizeof(S) * (2 * gx);
            const unsigned qb = *at<typename L::Two>(p.cb, cx), qr = *at<typename L::Two>(p.cr, cx);
            cb0 = L::get2(qb, 0), cb1 = L::get2(qb, 1), cr0 = L::get2(qr, 0), cr1 = L::get2(qr, 1);
        }
        const S *b = at<S>(p.cb, co), *q = at<S>(p.cr, co);
        const int bA = (int)val<S>(k, cb0), bB = (int)val<S>(k, cb1), rA = (int)val<S>(k, cr0), rB = (int)val<S>(k, cr1);
        const int bL = XCO ? bA : (int)val<S>(k, b[xl]), rL = XCO ? rA : (int)val<S>(k, q[xl]);
        const int bR = (int)val<S>(k, b[xr]), rR = (int)val<S>(k, q[xr]);
        hb[j][0] = tap_even<XCO>(bL, bA), hb[j][1] = tap_odd<XCO>(bA, bB), hb[j][2] = tap_even<XCO>(bA, bB), hb[j][3] = tap_odd<XCO>(bB, bR);
        hr[j][0] = tap_even<XCO>(rL, rA), hr[j][1] = tap_odd<XCO>(rA, rB), hr[j][2] = tap_even<XCO>(rA, rB), hr[j][3] = tap_odd<XCO>(rB, rR);
    }
    f32x4* d = reinterpret_cast<f32x4*>(lr4) + (f * H + 2 * by) * W + 4 * gx;
    f32x4 t[4], u[4];
#pragma unroll
    for (int x = 0; x < 4; ++x) {
        t[x] = rgb0_of(k, val<S>(k, L::get(ya, x)), chroma_terms16(k, tap_even<YCO>(hb[0][x], hb[1][x]), tap_even<YCO>(hr[0][x], hr[1][x])));
        u[x] = rgb0_of(k, val<S>(k, L::get(yb, x)), chroma_terms16(k, tap_odd<YCO>(hb[1][x], hb[2][x]), tap_odd<YCO>(hr[1][x], hr[2][x])));
    }
    d[0] = t[0];
    d[1] = t[1];
    d[2] = t[2];
    d[3] = t[3];
    d[W] = u[0];
    d[W + 1] = u[1];
    d[W + 2] = u[2];
    d[W + 3] = u[3];
}

// planes -> (n,3,H,W) fp32 planes with sited chroma: frames_from_yuv420_kernel's thread and stores, the general sited form's values
template <class S, bool XCO, bool YCO>
__global__ __launch_bounds__(256) void frames_from_yuv420_sited_kernel(const YuvPlanes p, const YuvCoef k, float* __restrict__ out, int H, int W, long total) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int bw = W >> 1, bh = H >> 1;
    const int bx = (int)(i % bw);
    const long r = i / bw;
    const int by = (int)(r % bh);
    const long f = r / bh;
    const long yo = f * p.y_frame + (long)(2 * by) * p.y_pitch;
    ChromaTerms c[4];
    sited_terms<S, XCO, YCO>(p, k, f, by, bx, bh, bw, c);
    const long hw = (long)H * W;
    float* d = out + f * 3 * hw + (long)(2 * by) * W + 2 * bx;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int dy = j >> 1, dx = j & 1;
        const f32x4 v = rgb0_of(k, val<S>(k, at<S>(p.y, yo + dy * p.y_pitch)[2 * bx + dx]), c[j]);
        float* q = d + dy * W + dx;
        q[0] = v[0];
        q[hw] = v[1];
        q[2 * hw] = v[2];
    }
}

// clamp(rint(x), 0, 2^d - 1), rint rounding half to even, as it is stored: a byte, or a word with the bits outside the value zero
template <class S>
__device__ __forceinline__ S sample_of(const YuvCoef& k, float x) {
    const float v = fminf(fmaxf(rintf(x), 0.f), k.vmax);
    if constexpr (sizeof(S) == 1) return (S)v;
    else return (S)((unsigned)v << k.shift);
}

// (n,3,H,W) fp32 planes -> planes: one thread = one 2x2 block = four Y samples and one chroma pair, single-sample stores; nothing
// beyond a row's width is written
template <class S>
__global__ __launch_bounds__(256) void frames_to_yuv420_kernel(const float* __restrict__ in, const YuvPlanes p, const YuvCoef k, int H, int W, long total) {
#pragma clang fp contract(off)
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int bw = W >> 1, bh = H >> 1;
    const int bx = (int)(i % bw);
    const long r = i / bw;
    const int by = (int)(r % bh);
    const long f = r / bh;
    const long hw = (long)H * W;
    const float* s = in + f * 3 * hw + (long)(2 * by) * W + 2 * bx;
    const long yo = f * p.y_frame + (long)(2 * by) * p.y_pitch;
    float pb[4], pr[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {       // 00, 01, 10, 11: rows top then bottom, columns left then right
        const int dy = j >> 1, dx = j & 1;
        const float* q = s + dy * W + dx;
        const float rr = fminf(fmaxf(q[0], 0.f), 1.f), gg = fminf(fmaxf(q[hw], 0.f), 1.f), bb = fminf(fmaxf(q[2 * hw], 0.f), 1.f);
        const float yl = (k.kr * rr + k.kg * gg) + k.kb * bb;
        at<S>(p.y, yo + dy * p.y_pitch)[2 * bx + dx] = sample_of<S>(k, (float)k.yoff + k.sy * yl);
        pb[j] = (bb - yl) * k.ipb;
        pr[j] = (rr - yl) * k.ipr;
    }
    const float mb = ((pb[0] + pb[1]) + (pb[2] + pb[3])) * 0.25f, mr = ((pr[0] + pr[1]) + (pr[2] + pr[3])) * 0.25f;
    const long co = f * p.c_frame + (long)by * p.c_pitch;
    const long cx = (long)bx * p.c_step;
    at<S>(p.cb, co)[cx] = sample_of<S>(k, (float)k.cmid + k.sc * mb);
    at<S>(p.cr, co)[cx] = sample_of<S>(k, (float)k.cmid + k.sc * mr);
}

// (n,3,H,W) fp32 planes -> planes with chroma co-sited with the even luma columns (PNP_YUV_CHROMA_LEFT; YCO: and with the even luma
// rows, PNP_YUV_CHROMA_TOPLEFT).  frames_to_yuv420_kernel's thread and stores; the chroma sample takes pb, pr of the columns
// max(2 bx - 1, 0), 2 bx, 2 bx + 1 as ((pL + pR) + (pC + pC)) * 0.25 in each of its rows -- 2 by and 2 by + 1, combined as
// (a0 + a1) * 0.5, or max(2 by - 1, 0), 2 by, 2 by + 1, combined with the three-tap form -- so a thread evaluates the pixels beside
// its block once more (the same fp32 operations: the same values) and reads nothing outside the frame.
template <class S, bool YCO>
__global__ __launch_bounds__(256) void frames_to_yuv420_sited_kernel(const float* __restrict__ in, const YuvPlanes p, const YuvCoef k, int H, int W, long total) {
#pragma clang fp contract(off)
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int bw = W >> 1, bh = H >> 1;
    const int bx = (int)(i % bw);
    const long r = i / bw;
    const int by = (int)(r % bh);
    const long f = r / bh;
    const long hw = (long)H * W;
    const float* s = in + f * 3 * hw;
    constexpr int NR = YCO ? 3 : 2;
    const int cols[3] = {max(2 * bx - 1, 0), 2 * bx, 2 * bx + 1};
    float ab[NR], ar[NR];               // each row across
#pragma unroll
    for (int j = 0; j < NR; ++j) {
        const int dy = YCO ? j - 1 : j;                 // the row's place in the block: -1 (above it), 0, 1
        const int row = max(2 * by + dy, 0);
        float pb[3], pr[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float* q = s + (long)row * W + cols[c];
            const float rr = fminf(fmaxf(q[0], 0.f), 1.f), gg = fminf(fmaxf(q[hw], 0.f), 1.f), bb = fminf(fmaxf(q[2 * hw], 0.f), 1.f);
            const float yl = (k.kr * rr + k.kg * gg) + k.kb * bb;
            if (dy >= 0 && c >= 1) at<S>(p.y, f * p.y_frame + (long)row * p.y_pitch)[cols[c]] = sample_of<S>(k, (float)k.yoff + k.sy * yl);
            pb[c] = (bb - yl) * k.ipb;
            pr[c] = (rr - yl) * k.ipr;
        }
        ab[j] = ((pb[0] + pb[2]) + (pb[1] + pb[1])) * 0.25f;
        ar[j] = ((pr[0] + pr[2]) + (pr[1] + pr[1])) * 0.25f;
    }
    float mb, mr;
    if constexpr (YCO) mb = ((ab[0] + ab[2]) + (ab[1] + ab[1])) * 0.25f, mr = ((ar[0] + ar[2]) + (ar[1] + ar[1])) * 0.25f;
    else mb = (ab[0] + ab[1]) * 0.5f, mr = (ar[0] + ar[1]) * 0.5f;
    const long co = f * p.c_frame + (long)by * p.c_pitch;
    const long cx = (long)bx * p.c_step;
    at<S>(p.cb, co)[cx] = sample_of<S>(k, (float)k.cmid + k.sc * mb);
    at<S>(p.cr, co)[cx] = sample_of<S>(k, (float)k.cmid + k.sc * mr);
}

// ---- 4:2:2 and 4:4:4 (include/pnpvcve.h, "Chroma formats"): chroma rows are luma rows (sy = 1), so a thread owns pixels of ONE row and
// no kernel has a vertical tap.  SX is the horizontal factor: 2 (4:2:2) | 1 (4:4:4).  XM is what the x axis does with the mode:
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

// General form, planes -> RGB0 (PLANAR false: the (T,H,W,4) conv source) or -> (n,3,H,W) fp32 planes (PLANAR true): one thread = one
// chroma sample = SX pixels of a row, single-sample loads at any address, pitch and c_step.  i over T * H * (W / SX).
template <class S, int SX, int XM, bool PLANAR>
__global__ __launch_bounds__(256) void yuv_rows_in_kernel(const YuvPlanes p, const YuvCoef k, float* __restrict__ out, int H, int W, long total) {
    static_assert(SX == 2 || XM == XM_PLAIN, "4:4:4 has one form");
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int bw = W / SX;
    const int bx = (int)(i % bw);
    const long r = i / bw;
    const int y = (int)(r % H);
    const long f = r / H;
    const S* yr = at<S>(p.y, f * p.y_frame + (long)y * p.y_pitch) + SX * bx;
    const long co = f * p.c_frame + (long)y * p.c_pitch;
    const S *b = at<S>(p.cb, co), *q = at<S>(p.cr, co);
    const long xc = (long)bx * p.c_step;
    const int bc = (int)val<S>(k, b[xc]), rc = (int)val<S>(k, q[xc]);
    int bm = bc, rm = rc, bp = bc, rp = rc;
    if constexpr (XM != XM_PLAIN) {
        const long xp = (long)min(bx + 1, bw - 1) * p.c_step;
        bp = (int)val<S>(k, b[xp]), rp = (int)val<S>(k, q[xp]);
        if constexpr (XM == XM_MIDWAY) {
            const long xm = (long)max(bx - 1, 0) * p.c_step;
            bm = (int)val<S>(k, b[xm]), rm = (int)val<S>(k, q[xm]);
        }
    }
    ChromaTerms c[SX];
    row_terms<SX, XM>(k, bm, bc, bp, rm, rc, rp, c);
    const long hw = (long)H * W;
#pragma unroll
    for (int j = 0; j < SX; ++j) {
        const f32x4 v = rgb0_of(k, val<S>(k, yr[j]), c[j]);
        if constexpr (PLANAR) {
            float* d = out + f * 3 * hw + (long)y * W + SX * bx + j;
            d[0] = v[0];
            d[hw] = v[1];
            d[2 * hw] = v[2];
        } else {
            reinterpret_cast<f32x4*>(out)[(f * H + y) * W + SX * bx + j] = v;
        }
    }
}

// Aligned fast form (yuv_planes_fast with the format): one thread = four pixels of a row = one four-sample load of Y and four 16-byte
// stores, 64 contiguous bytes.  Chroma of its columns: 4:2:2 one four-sample load of the interleaved pair (STEP 2: a0 b0 a1 b1;
// cr_first says which plane starts) or a two-sample load of each plane (STEP 1), with the clamped columns beside them as single
// samples where the mode has taps; 4:4:4 two four-sample loads of the pair or one of each plane.  W is a multiple of 4.  The same
// integers as the general form, so the same values.  i over T * H * (W / 4).
template <class S, int SX, int STEP, int XM>
__global__ __launch_bounds__(256) void pack_lr_rows_fast_kernel(const YuvPlanes p, const YuvCoef k, float* __restrict__ lr4, int H, int W, int cr_first,
                                                                long total) {
    static_assert(SX == 2 || XM == XM_PLAIN, "4:4:4 has one form");
    using L = Load<S>;
    using Four = typename L::Four;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int gw = W >> 2;
    const int gx = (int)(i % gw);
    const long r = i / gw;
    const int y = (int)(r % H);
    const long f = r / H;
    const Four ya = *at<Four>(p.y, f * p.y_frame + (long)y * p.y_pitch + (long)sizeof(S) * (4 * gx));
    const long co = f * p.c_frame + (long)y * p.c_pitch;
    constexpr int NC = 4 / SX;          // chroma samples of the thread's four pixels
    unsigned cb[NC], cr[NC];
    if constexpr (SX == 2) {
        if (STEP == 2) {
            const Four q = *at<Four>(cr_first ? p.cr : p.cb, co + (long)sizeof(S) * (4 * gx));
            const unsigned a0 = L::get(q, 0), b0 = L::get(q, 1), a1 = L::get(q, 2), b1 = L::get(q, 3);
            cb[0] = cr_first ? b0 : a0, cr[0] = cr_first ? a0 : b0;
            cb[1] = cr_first ? b1 : a1, cr[1] = cr_first ? a1 : b1;
        } else {
            const long cx = co + (long)sizeof(S) * (2 * gx);
            const unsigned qb = *at<typename L::Two>(p.cb, cx), qr = *at<typename L::Two>(p.cr, cx);
            cb[0] = L::get2(qb, 0), cb[1] = L::get2(qb, 1), cr[0] = L::get2(qr, 0), cr[1] = L::get2(qr, 1);
        }
    } else {
        if (STEP == 2) {
            const long cx = co + (long)sizeof(S) * (8 * gx);
            const Four q0 = *at<Four>(cr_first ? p.cr : p.cb, cx), q1 = *at<Four>(cr_first ? p.cr : p.cb, cx + 4 * (long)sizeof(S));
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const unsigned a = L::get(j < 2 ? q0 : q1, 2 * (j & 1)), b = L::get(j < 2 ? q0 : q1, 2 * (j & 1) + 1);
                cb[j] = cr_first ? b : a, cr[j] = cr_first ? a : b;
            }
        } else {
            const long cx = co + (long)sizeof(S) * (4 * gx);
            const Four qb = *at<Four>(p.cb, cx), qr = *at<Four>(p.cr, cx);
#pragma unroll
            for (int j = 0; j < 4; ++j) cb[j] = L::get(qb, j), cr[j] = L::get(qr, j);
        }
    }
    f32x4 t[4];
    if constexpr (SX == 2) {
        const int bw = W >> 1;
        const int bA = (int)val<S>(k, cb[0]), bB = (int)val<S>(k, cb[1]), rA = (int)val<S>(k, cr[0]), rB = (int)val<S>(k, cr[1]);
        int bL = bA, rL = rA, bR = bB, rR = rB;
        if constexpr (XM != XM_PLAIN) {
            const S *b = at<S>(p.cb, co), *q = at<S>(p.cr, co);
            const long xr = (long)min(2 * gx + 2, bw - 1) * STEP;
            bR = (int)val<S>(k, b[xr]), rR = (int)val<S>(k, q[xr]);
            if constexpr (XM == XM_MIDWAY) {
                const long xl = (long)max(2 * gx - 1, 0) * STEP;
                bL = (int)val<S>(k, b[xl]), rL = (int)val<S>(k, q[xl]);
            }
        }
        ChromaTerms c0[2], c1[2];
        row_terms<2, XM>(k, bL, bA, bB, rL, rA, rB, c0);
        row_terms<2, XM>(k, bA, bB, bR, rA, rB, rR, c1);
        t[0] = rgb0_of(k, val<S>(k, L::get(ya, 0)), c0[0]);
        t[1] = rgb0_of(k, val<S>(k, L::get(ya, 1)), c0[1]);
        t[2] = rgb0_of(k, val<S>(k, L::get(ya, 2)), c1[0]);
        t[3] = rgb0_of(k, val<S>(k, L::get(ya, 3)), c1[1]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) t[j] = rgb0_of(k, val<S>(k, L::get(ya, j)), chroma_terms(k, val<S>(k, cb[j]), val<S>(k, cr[j])));
    }
    f32x4* d = reinterpret_cast<f32x4*>(lr4) + (f * H + y) * W + 4 * gx;
    d[0] = t[0];
    d[1] = t[1];
    d[2] = t[2];
    d[3] = t[3];
}

// (n,3,H,W) fp32 planes -> planes: one thread = one chroma sample = SX pixels of a row, single-sample stores; nothing beyond a row's
// width is written.  XM_PLAIN: the pixel's own pb, pr (SX 1) or (p0 + p1) * 0.5 (SX 2); XM_COSITED (SX 2): the taps max(2 bx - 1, 0),
// 2 bx, 2 bx + 1 as ((pL + pR) + (pC + pC)) * 0.25 -- one left neighbour, evaluated once more (the same fp32 operations: the same
// values), nothing outside the frame read.  i over n * H * (W / SX).
template <class S, int SX, int XM>
__global__ __launch_bounds__(256) void yuv_rows_out_kernel(const float* __restrict__ in, const YuvPlanes p, const YuvCoef k, int H, int W, long total) {
#pragma clang fp contract(off)
    static_assert(XM == XM_PLAIN || (SX == 2 && XM == XM_COSITED), "the forms of the way out");
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int bw = W / SX;
    const int bx = (int)(i % bw);
    const long r = i / bw;
    const int y = (int)(r % H);
    const long f = r / H;
    const long hw = (long)H * W;
    const float* s = in + f * 3 * hw + (long)y * W;
    S* yo = at<S>(p.y, f * p.y_frame + (long)y * p.y_pitch);
    constexpr int N = XM == XM_COSITED ? 3 : SX;
    const int x0 = XM == XM_COSITED ? 2 * bx - 1 : SX * bx;     // the first tap before it is clamped
    float pb[N], pr[N];
#pragma unroll
    for (int c = 0; c < N; ++c) {
        const int x = max(x0 + c, 0);
        const float* q = s + x;
        const float rr = fminf(fmaxf(q[0], 0.f), 1.f), gg = fminf(fmaxf(q[hw], 0.f), 1.f), bb = fminf(fmaxf(q[2 * hw], 0.f), 1.f);
        const float yl = (k.kr * rr + k.kg * gg) + k.kb * bb;
        if (XM != XM_COSITED || c >= 1) yo[x] = sample_of<S>(k, (float)k.yoff + k.sy * yl);
        pb[c] = (bb - yl) * k.ipb;
        pr[c] = (rr - yl) * k.ipr;
    }
    float mb, mr;
    if constexpr (XM == XM_COSITED) mb = ((pb[0] + pb[2]) + (pb[1] + pb[1])) * 0.25f, mr = ((pr[0] + pr[2]) + (pr[1] + pr[1])) * 0.25f;
    else if constexpr (SX == 2) mb = (pb[0] + pb[1]) * 0.5f, mr = (pr[0] + pr[1]) * 0.5f;
    else mb = pb[0], mr = pr[0];
    const long co = f * p.c_frame + (long)y * p.c_pitch;
    const long cx = (long)bx * p.c_step;
    at<S>(p.cb, co)[cx] = sample_of<S>(k, (float)k.cmid + k.sc * mb);
    at<S>(p.cr, co)[cx] = sample_of<S>(k, (float)k.cmid + k.sc * mr);
}

unsigned blocks_of(long total) { return (unsigned)((total + 255) / 256); }

// the x-axis form of a mode on the way in, for a format other than 4:2:0
int xm_in(const YuvCoef& k) {
    if (k.format == PNP_YUV_FORMAT_444 || k.chroma == PNP_YUV_CHROMA_REPLICATE) return XM_PLAIN;
    return k.chroma == PNP_YUV_CHROMA_CENTER ? XM_MIDWAY : XM_COSITED;
}

// f<S, SX, XM>(args...) for the sample size, the format (4:2:2 | 4:4:4) and the x-axis form
#define YUV_ROWS_S(f, S, fmt, xm, ...)                                                                  \
    ((fmt) == PNP_YUV_FORMAT_444 ? f<S, 1, XM_PLAIN>(__VA_ARGS__)                                      \
     : (xm) == XM_PLAIN          ? f<S, 2, XM_PLAIN>(__VA_ARGS__)                                      \
     : (xm) == XM_MIDWAY         ? f<S, 2, XM_MIDWAY>(__VA_ARGS__)                                     \
                                 : f<S, 2, XM_COSITED>(__VA_ARGS__))
#define YUV_ROWS(f, bytes, fmt, xm, ...) \
    ((bytes) == 1 ? YUV_ROWS_S(f, unsigned char, fmt, xm, __VA_ARGS__) : YUV_ROWS_S(f, unsigned short, fmt, xm, __VA_ARGS__))

template <class S, int SX, int XM>
int rows_in(const YuvPlanes& in, const YuvCoef& k, float* out, int n, int H, int W, bool planar, bool fast, hipStream_t stream) {
    if (fast) {         // (the pack alone)
        const long total = (long)n * H * (W / 4);
        const int cr_first = in.cr < in.cb ? 1 : 0;
        if (in.c_step == 2) hipLaunchKernelGGL((pack_lr_rows_fast_kernel<S, SX, 2, XM>), dim3(blocks_of(total)), dim3(256), 0, stream, in, k, out, H, W, cr_first, total);
        else hipLaunchKernelGGL((pack_lr_rows_fast_kernel<S, SX, 1, XM>), dim3(blocks_of(total)), dim3(256), 0, stream, in, k, out, H, W, cr_first, total);
        return (int)hipGetLastError();
    }
    const long total = (long)n * H * (W / SX);
    if (planar) hipLaunchKernelGGL((yuv_rows_in_kernel<S, SX, XM, true>), dim3(blocks_of(total)), dim3(256), 0, stream, in, k, out, H, W, total);
    else hipLaunchKernelGGL((yuv_rows_in_kernel<S, SX, XM, false>), dim3(blocks_of(total)), dim3(256), 0, stream, in, k, out, H, W, total);
    return (int)hipGetLastError();
}
template <class S, int SX, int XM>
int rows_out(const float* in, const YuvPlanes& out, const YuvCoef& k, int n, int H, int W, hipStream_t stream) {
    const long total = (long)n * H * (W / SX);
    if constexpr (XM == XM_MIDWAY) return rows_out<S, SX, XM_PLAIN>(in, out, k, n, H, W, stream);
    else {
        hipLaunchKernelGGL((yuv_rows_out_kernel<S, SX, XM>), dim3(blocks_of(total)), dim3(256), 0, stream, in, out, k, H, W, total);
        return (int)hipGetLastError();
    }
}

template <class S>
int pack_lr(const YuvPlanes& in, const YuvCoef& k, float* lr4, int T, int H, int W, bool fast, hipStream_t stream) {
    if (fast) {
        const long total = (long)T * (H / 2) * (W / 4);
        const int cr_first = in.cr < in.cb ? 1 : 0;
        if (in.c_step == 2) hipLaunchKernelGGL((pack_lr_yuv420_fast_kernel<S, 2>), dim3(blocks_of(total)), dim3(256), 0, stream, in, k, lr4, H, W, cr_first, total);
        else hipLaunchKernelGGL((pack_lr_yuv420_fast_kernel<S, 1>), dim3(blocks_of(total)), dim3(256), 0, stream, in, k, lr4, H, W, cr_first, total);
        return (int)hipGetLastError();
    }
    const long total = (long)T * (H / 2) * (W / 2);
    hipLaunchKernelGGL(pack_lr_yuv420_kernel<S>, dim3(blocks_of(total)), dim3(256), 0, stream, in, k, lr4, H, W, total);
    return (int)hipGetLastError();
}

// the sited forms: XCO, YCO are the co-sited axes of k.chroma (CENTER: none; LEFT: x; TOPLEFT: both)
template <class S, bool XCO, bool YCO>
int pack_lr_sited(const YuvPlanes& in, const YuvCoef& k, float* lr4, int T, int H, int W, bool fast, hipStream_t stream) {
    if (fast) {
        const long total = (long)T * (H / 2) * (W / 4);
        const int cr_first = in.cr < in.cb ? 1 : 0;
        if (in.c_step == 2)
            hipLaunchKernelGGL((pack_lr_yuv420_sited_fast_kernel<S, 2, XCO, YCO>), dim3(blocks_of(total)), dim3(256), 0, stream, in, k, lr4, H, W, cr_first, total);
        else
            hipLaunchKernelGGL((pack_lr_yuv420_sited_fast_kernel<S, 1, XCO, YCO>), dim3(blocks_of(total)), dim3(256), 0, stream, in, k, lr4, H, W, cr_first, total);
        return (int)hipGetLastError();
    }
    const long total = (long)T * (H / 2) * (W / 2);
    hipLaunchKernelGGL((pack_lr_yuv420_sited_kernel<S, XCO, YCO>), dim3(blocks_of(total)), dim3(256), 0, stream, in, k, lr4, H, W, total);
    return (int)hipGetLastError();
}
template <class S, bool XCO, bool YCO>
int frames_from_sited(const YuvPlanes& in, const YuvCoef& k, float* out, int H, int W, long total, hipStream_t stream) {
    hipLaunchKernelGGL((frames_from_yuv420_sited_kernel<S, XCO, YCO>), dim3(blocks_of(total)), dim3(256), 0, stream, in, k, out, H, W, total);
    return (int)hipGetLastError();
}
template <class S, bool YCO>
int frames_to_sited(const float* in, const YuvPlanes& out, const YuvCoef& k, int H, int W, long total, hipStream_t stream) {
    hipLaunchKernelGGL((frames_to_yuv420_sited_kernel<S, YCO>), dim3(blocks_of(total)), dim3(256), 0, stream, in, out, k, H, W, total);
    return (int)hipGetLastError();
}

// f<S, XCO, YCO>(args...) for the sample size and the sited mode (CENTER | LEFT | TOPLEFT)
#define YUV_SITED(f, bytes, mode, ...)                                                                                  \
    ((bytes) == 1 ? ((mode) == PNP_YUV_CHROMA_CENTER ? f<unsigned char, false, false>(__VA_ARGS__)                      \
                     : (mode) == PNP_YUV_CHROMA_LEFT ? f<unsigned char, true, false>(__VA_ARGS__)                       \
                                                     : f<unsigned char, true, true>(__VA_ARGS__))                       \
                  : ((mode) == PNP_YUV_CHROMA_CENTER ? f<unsigned short, false, false>(__VA_ARGS__)                     \
                     : (mode) == PNP_YUV_CHROMA_LEFT ? f<unsigned short, true, false>(__VA_ARGS__)                      \
                                                     : f<unsigned short, true, true>(__VA_ARGS__)))

}  // namespace

int launch_pack_lr_yuv420(const YuvPlanes& in, const YuvCoef& k, float* lr4, int T, int H, int W, bool force_general, hipStream_t stream) {
    if (!yuv_frame_ok(k.format, T, H, W) || !lr4 || !yuv_planes_ok(in, W, k.format)) return PNP_ERR_BAD_ARG;
    const bool fast = !force_general && yuv_planes_fast(in, W, k.format);
    if (k.format != PNP_YUV_FORMAT_420) return YUV_ROWS(rows_in, in.sample_bytes, k.format, xm_in(k), in, k, lr4, T, H, W, false, fast, stream);
    if (k.chroma != PNP_YUV_CHROMA_REPLICATE) return YUV_SITED(pack_lr_sited, in.sample_bytes, k.chroma, in, k, lr4, T, H, W, fast, stream);
    return in.sample_bytes == 1 ? pack_lr<unsigned char>(in, k, lr4, T, H, W, fast, stream) : pack_lr<unsigned short>(in, k, lr4, T, H, W, fast, stream);
}

int launch_frames_from_yuv420(const YuvPlanes& in, const YuvCoef& k, float* out, int nframes, int H, int W, hipStream_t stream) {
    if (!yuv_frame_ok(k.format, nframes, H, W) || !out || !yuv_planes_ok(in, W, k.format)) return PNP_ERR_BAD_ARG;
    if (k.format != PNP_YUV_FORMAT_420) return YUV_ROWS(rows_in, in.sample_bytes, k.format, xm_in(k), in, k, out, nframes, H, W, true, false, stream);
    const long total = (long)nframes * (H / 2) * (W / 2);
    if (k.chroma != PNP_YUV_CHROMA_REPLICATE) return YUV_SITED(frames_from_sited, in.sample_bytes, k.chroma, in, k, out, H, W, total, stream);
    if (in.sample_bytes == 1) hipLaunchKernelGGL(frames_from_yuv420_kernel<unsigned char>, dim3(blocks_of(total)), dim3(256), 0, stream, in, k, out, H, W, total);
    else hipLaunchKernelGGL(frames_from_yuv420_kernel<unsigned short>, dim3(blocks_of(total)), dim3(256), 0, stream, in, k, out, H, W, total);
    return (int)hipGetLastError();
}

int launch_frames_to_yuv420(const float* in, const YuvPlanes& out, const YuvCoef& k, int nframes, int H, int W, hipStream_t stream) {
    if (!yuv_frame_ok(k.format, nframes, H, W) || !in || !yuv_planes_ok(out, W, k.format)) return PNP_ERR_BAD_ARG;
    if (k.format != PNP_YUV_FORMAT_420)         // (CENTER writes what REPLICATE writes, as at 4:2:0)
        return YUV_ROWS(rows_out, out.sample_bytes, k.format, xm_in(k), in, out, k, nframes, H, W, stream);
    const long total = (long)nframes * (H / 2) * (W / 2);
    if (k.chroma == PNP_YUV_CHROMA_LEFT || k.chroma == PNP_YUV_CHROMA_TOPLEFT) {        // (CENTER writes the box mean, as REPLICATE)
        const bool yco = k.chroma == PNP_YUV_CHROMA_TOPLEFT;
        if (out.sample_bytes == 1) return yco ? frames_to_sited<unsigned char, true>(in, out, k, H, W, total, stream) : frames_to_sited<unsigned char, false>(in, out, k, H, W, total, stream);
        return yco ? frames_to_sited<unsigned short, true>(in, out, k, H, W, total, stream) : frames_to_sited<unsigned short, false>(in, out, k, H, W, total, stream);
    }
    if (out.sample_bytes == 1) hipLaunchKernelGGL(frames_to_yuv420_kernel<unsigned char>, dim3(blocks_of(total)), dim3(256), 0, stream, in, out, k, H, W, total);
    else hipLaunchKernelGGL(frames_to_yuv420_kernel<unsigned short>, dim3(blocks_of(total)), dim3(256), 0, stream, in, out, k, H, W, total);
    return (int)hipGetLastError();
}

namespace {

// the bodies of the public entries, once for both descriptors (P: pnp_yuv420_planes | pnp_yuv420_planes16)
template <class P>
int frames_from(const P* in, int yuv_standard, float* out_planes, int n, int h, int w, void* stream) {
    YuvCoef k;
    if (!in || !out_planes) return PNP_ERR_BAD_ARG;
    const YuvPlanes p = yuv_planes(*in);
    if (!yuv_coef(yuv_standard, p, &k) || !yuv_frame_ok(k.format, n, h, w) || !yuv_planes_ok(p, w, k.format)) return PNP_ERR_BAD_ARG;
    return launch_frames_from_yuv420(p, k, out_planes, n, h, w, (hipStream_t)stream);
}
template <class P>
int frames_to(const float* planes, const P* out, int yuv_standard, int n, int h, int w, void* stream) {
    YuvCoef k;
    if (!out || !planes) return PNP_ERR_BAD_ARG;
    const YuvPlanes p = yuv_planes(*out);
    if (!yuv_coef(yuv_standard, p, &k) || !yuv_frame_ok(k.format, n, h, w) || !yuv_planes_ok(p, w, k.format)) return PNP_ERR_BAD_ARG;
    return launch_frames_to_yuv420(planes, p, k, n, h, w, (hipStream_t)stream);
}
template <class P>
int debug_pack(const P* in, int yuv_standard, float* lr4, int t, int h, int w, int general, void* stream) {
    YuvCoef k;
    if (!in || !lr4 || !yuv_coef(yuv_standard, yuv_planes(*in), &k)) return PNP_ERR_BAD_ARG;
    return launch_pack_lr_yuv420(yuv_planes(*in), k, lr4, t, h, w, general != 0, (hipStream_t)stream);
}

}  // namespace

extern "C" {

int pnp_frames_from_yuv420(const pnp_yuv420_planes* in, int yuv_standard, float* out_planes, int n, int h, int w, void* stream) {
    return frames_from(in, yuv_standard, out_planes, n, h, w, stream);
}
int pnp_frames_from_yuv420p16(const pnp_yuv420_planes16* in, int yuv_standard, float* out_planes, int n, int h, int w, void* stream) {
    return frames_from(in, yuv_standard, out_planes, n, h, w, stream);
}

int pnp_frames_to_yuv420(const float* planes, const pnp_yuv420_planes* out, int yuv_standard, int n, int h, int w, void* stream) {
    return frames_to(planes, out, yuv_standard, n, h, w, stream);
}
int pnp_frames_to_yuv420p16(const float* planes, const pnp_yuv420_planes16* out, int yuv_standard, int n, int h, int w, void* stream) {
    return frames_to(planes, out, yuv_standard, n, h, w, stream);
}

int pnp_debug_pack_lr_yuv420(const pnp_yuv420_planes* in, int yuv_standard, float* lr4, int t, int h, int w, int general, void* stream) {
    return debug_pack(in, yuv_standard, lr4, t, h, w, general, stream);
}
int pnp_debug_pack_lr_yuv420p16(const pnp_yuv420_planes16* in, int yuv_standard, float* lr4, int t, int h, int w, int general, void* stream) {
    return debug_pack(in, yuv_standard, lr4, t, h, w, general, stream);
}

}  // extern "C"
