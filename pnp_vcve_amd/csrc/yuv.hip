// Y'CbCr boundary: the decoder's planes straight into the conv source, and fp32 RGB planes out as planes an encoder or a display
// takes -- NV12 / NV21 / I420 bytes, or the 16-bit words a Main10 / VVC decoder writes (P010 / P012: the value in the high bits;
// yuv420p10le / yuv420p12le: in the low bits), at 4:2:0, 4:2:2 and 4:4:4.  The arithmetic is the one include/pnpvcve.h states
// (pnp_frames_from_yuv420 / pnp_frames_to_yuv420, pnp_yuv420_planes16, "Chroma modes", "Chroma formats"): constants of the depth
// rounded to fp32 once on the host (yuv.h), every product and sum after that an fp32 operation rounded on its own.  What a pixel goes
// through is written once, in yuv_px.h; this file holds who owns which pixels -- three kernels per family -- and the host side.
//   4:2:0: a thread owns whole 2x2 blocks (the aligned pack: two of them side by side) and reads each chroma pair once, with the
//          clamped neighbours a sited mode needs beside them.  CM is the chroma mode, PNP_YUV_CHROMA_* itself.
//   4:2:2 and 4:4:4: chroma rows are luma rows, so a thread owns pixels of ONE row and no kernel has a vertical tap.  SX is the
//          horizontal factor and XM the x-axis form of the mode (yuv_px.h).
// Every kernel is a template on the sample type S (unsigned char | unsigned short).
#include "yuv_px.h"

namespace {

// General form at 4:2:0, planes -> RGB0 (PLANAR false: the (T,H,W,4) conv source) or -> (n,3,H,W) fp32 planes (PLANAR true): one thread
// = one 2x2 block, single-sample loads at any address and pitch yuv_planes_ok admits.  i over T * (H/2) * (W/2).
template <class S, int CM, bool PLANAR>
__global__ __launch_bounds__(256) void yuv420_in_kernel(const YuvPlanes p, const YuvCoef k, float* __restrict__ out, int H, int W, long total) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int bw = W >> 1, bh = H >> 1;
    const Idx t = split(i, bh, bw);
    const int by = t.row, bx = t.col;
    ChromaTerms c[4];
    block_terms<S, CM>(p, k, t.f, by, bx, bh, bw, c);
    const long yo = t.f * p.y_frame + (long)(2 * by) * p.y_pitch;
    float* d = px_at<PLANAR>(out, t.f, H, W, 2 * by, 2 * bx);
#pragma unroll
    for (int j = 0; j < 4; ++j)         // 00, 01, 10, 11: rows top then bottom, columns left then right
        store_px<PLANAR>(d, H, W, j >> 1, j & 1, rgb0_of(k, val<S>(k, at<S>(p.y, yo + (j >> 1) * p.y_pitch)[2 * bx + (j & 1)]), c[j]));
}

// Aligned fast form at 4:2:0 (yuv_planes_fast): one thread = two rows of four pixels = two four-sample loads of Y, eight 16-byte stores,
// 64 contiguous bytes per row, and load_pairs' chroma of its two columns -- once (REPLICATE), or once per row of the clamped rows by - 1,
// by, by + 1 (a pitch that is aligned keeps every row's load aligned) with the clamped columns 2 gx - 1 and 2 gx + 2 beside them as
// single samples.  The same integers as the general form, so the same values.  W is a multiple of 4.  i over T * (H/2) * (W/4).
template <class S, int STEP, int CM>
__global__ __launch_bounds__(256) void pack_lr_yuv420_fast_kernel(const YuvPlanes p, const YuvCoef k, float* __restrict__ lr4, int H, int W, int cr_first,
                                                                  long total) {
    using L = Load<S>;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int gw = W >> 2, bh = H >> 1, bw = W >> 1;
    const Idx g = split(i, bh, gw);
    const int by = g.row, gx = g.col;
    const unsigned char* yp = p.y + g.f * p.y_frame + (long)(2 * by) * p.y_pitch + (long)sizeof(S) * (4 * gx);
    const typename L::Four ya = *at<typename L::Four>(yp, 0), yb = *at<typename L::Four>(yp, p.y_pitch);
    float* d = px_at<false>(lr4, g.f, H, W, 2 * by, 4 * gx);
    f32x4 t[4], u[4];
    if constexpr (CM == PNP_YUV_CHROMA_REPLICATE) {
        unsigned cb[2], cr[2];
        load_pairs<S, STEP>(p, g.f * p.c_frame + (long)by * p.c_pitch, gx, cr_first, cb, cr);
        const ChromaTerms c[2] = {chroma_terms(k, val<S>(k, cb[0]), val<S>(k, cr[0])), chroma_terms(k, val<S>(k, cb[1]), val<S>(k, cr[1]))};
#pragma unroll
        for (int x = 0; x < 4; ++x) t[x] = rgb0_of(k, val<S>(k, L::get(ya, x)), c[x >> 1]), u[x] = rgb0_of(k, val<S>(k, L::get(yb, x)), c[x >> 1]);
    } else {
        constexpr bool XCO = cm_xco(CM), YCO = cm_yco(CM);
        const int rows[3] = {YCO ? by : max(by - 1, 0), by, min(by + 1, bh - 1)};
        const long xl = (long)(XCO ? 2 * gx : max(2 * gx - 1, 0)) * STEP, xr = (long)min(2 * gx + 2, bw - 1) * STEP;
        int hb[3][4], hr[3][4];             // each row across: the thread's four columns, cb and cr
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const long co = g.f * p.c_frame + (long)rows[j] * p.c_pitch;
            unsigned cb[2], cr[2];
            load_pairs<S, STEP>(p, co, gx, cr_first, cb, cr);
            const S *b = at<S>(p.cb, co), *q = at<S>(p.cr, co);
            const int bA = (int)val<S>(k, cb[0]), bB = (int)val<S>(k, cb[1]), rA = (int)val<S>(k, cr[0]), rB = (int)val<S>(k, cr[1]);
            const int bL = XCO ? bA : (int)val<S>(k, b[xl]), rL = XCO ? rA : (int)val<S>(k, q[xl]);
            const int bR = (int)val<S>(k, b[xr]), rR = (int)val<S>(k, q[xr]);
            hb[j][0] = tap_even<XCO>(bL, bA), hb[j][1] = tap_odd<XCO>(bA, bB), hb[j][2] = tap_even<XCO>(bA, bB), hb[j][3] = tap_odd<XCO>(bB, bR);
            hr[j][0] = tap_even<XCO>(rL, rA), hr[j][1] = tap_odd<XCO>(rA, rB), hr[j][2] = tap_even<XCO>(rA, rB), hr[j][3] = tap_odd<XCO>(rB, rR);
        }
#pragma unroll
        for (int x = 0; x < 4; ++x) {
            t[x] = rgb0_of(k, val<S>(k, L::get(ya, x)), chroma_terms16(k, tap_even<YCO>(hb[0][x], hb[1][x]), tap_even<YCO>(hr[0][x], hr[1][x])));
            u[x] = rgb0_of(k, val<S>(k, L::get(yb, x)), chroma_terms16(k, tap_odd<YCO>(hb[1][x], hb[2][x]), tap_odd<YCO>(hr[1][x], hr[2][x])));
        }
    }
    store_group(d, t);
    store_group(d + 4 * (long)W, u);
}

// (n,3,H,W) fp32 planes -> planes at 4:2:0: one thread = one 2x2 block = four Y samples and one chroma pair, single-sample stores;
// nothing beyond a row's width is written.  OM is the mode that decides the chroma sample: REPLICATE (and CENTER, which the host maps
// to it) the box mean; LEFT, co-sited with the even luma columns, takes pb, pr of the columns max(2 bx - 1, 0), 2 bx, 2 bx + 1 as
// [1 2 1] / 4 in each of its rows 2 by and 2 by + 1, combined as (a0 + a1) * 0.5; TOPLEFT, co-sited with the even luma rows too, the
// rows max(2 by - 1, 0), 2 by, 2 by + 1 combined with the three-tap form.  So a co-sited thread evaluates the pixels beside its block
// once more (the same fp32 operations: the same values) and reads nothing outside the frame.  i over n * (H/2) * (W/2).
template <class S, int OM>
__global__ __launch_bounds__(256) void yuv420_out_kernel(const float* __restrict__ in, const YuvPlanes p, const YuvCoef k, int H, int W, long total) {
#pragma clang fp contract(off)
    static_assert(OM != PNP_YUV_CHROMA_CENTER, "CENTER writes the box mean");
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const Idx t = split(i, H >> 1, W >> 1);
    const int by = t.row, bx = t.col;
    const long hw = (long)H * W;
    const float* s = in + t.f * 3 * hw + (long)(2 * by) * W + 2 * bx;           // the block's pixel 00 and its Y sample
    S* yo = at<S>(p.y, t.f * p.y_frame + (long)(2 * by) * p.y_pitch) + 2 * bx;
    constexpr bool XCO = cm_xco(OM), YCO = cm_yco(OM);
    constexpr int NR = YCO ? 3 : 2, NC = XCO ? 3 : 2;       // the rows and columns evaluated; the block is the last two of each
    float ab[NR], ar[NR];                                   // each row across
#pragma unroll
    for (int j = 0; j < NR; ++j) {
        const int dy = YCO ? max(j - 1, -2 * by) : j;   // from the block's first row: -1 (above it, clamped to the frame), 0, 1
        PbPr v[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const int dx = XCO ? max(c - 1, -2 * bx) : c;
            v[c] = px_out<S>(k, s + dy * W + dx, hw, at<S>(reinterpret_cast<unsigned char*>(yo), dy * p.y_pitch) + dx, j >= NR - 2 && c >= NC - 2);
        }
        if constexpr (XCO) ab[j] = tap121(v[0].pb, v[1].pb, v[2].pb), ar[j] = tap121(v[0].pr, v[1].pr, v[2].pr);
        else ab[j] = v[0].pb + v[1].pb, ar[j] = v[0].pr + v[1].pr;
    }
    float mb, mr;
    if constexpr (YCO) mb = tap121(ab[0], ab[1], ab[2]), mr = tap121(ar[0], ar[1], ar[2]);
    else mb = (ab[0] + ab[1]) * (XCO ? 0.5f : 0.25f), mr = (ar[0] + ar[1]) * (XCO ? 0.5f : 0.25f);
    store_chroma<S>(p, k, t.f * p.c_frame + (long)by * p.c_pitch, (long)bx * p.c_step, mb, mr);
}

// General form at 4:2:2 | 4:4:4, planes -> RGB0 or -> fp32 planes (PLANAR): one thread = one chroma sample = SX pixels of a row,
// single-sample loads at any address, pitch and c_step.  i over T * H * (W / SX).
template <class S, int SX, int XM, bool PLANAR>
__global__ __launch_bounds__(256) void yuv_rows_in_kernel(const YuvPlanes p, const YuvCoef k, float* __restrict__ out, int H, int W, long total) {
    static_assert(SX == 2 || XM == XM_PLAIN, "4:4:4 has one form");
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int bw = W / SX;
    const Idx t = split(i, H, bw);
    const int y = t.row, bx = t.col;
    const S* yr = at<S>(p.y, t.f * p.y_frame + (long)y * p.y_pitch) + SX * bx;
    const long co = t.f * p.c_frame + (long)y * p.c_pitch;
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
    float* d = px_at<PLANAR>(out, t.f, H, W, y, SX * bx);
#pragma unroll
    for (int j = 0; j < SX; ++j) store_px<PLANAR>(d, H, W, 0, j, rgb0_of(k, val<S>(k, yr[j]), c[j]));
}

// Aligned fast form at 4:2:2 | 4:4:4 (yuv_planes_fast with the format): one thread = four pixels of a row = one four-sample load of Y
// and four 16-byte stores, 64 contiguous bytes.  Chroma of its columns: 4:2:2 load_pairs', with the clamped columns beside them as
// single samples where the mode has taps; 4:4:4 two four-sample loads of the interleaved pair (STEP 2) or one of each plane (STEP 1).
// W is a multiple of 4.  The same integers as the general form, so the same values.  i over T * H * (W / 4).
template <class S, int SX, int STEP, int XM>
__global__ __launch_bounds__(256) void pack_lr_rows_fast_kernel(const YuvPlanes p, const YuvCoef k, float* __restrict__ lr4, int H, int W, int cr_first,
                                                                long total) {
    static_assert(SX == 2 || XM == XM_PLAIN, "4:4:4 has one form");
    using L = Load<S>;
    using Four = typename L::Four;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const Idx g = split(i, H, W >> 2);
    const int y = g.row, gx = g.col;
    const Four ya = *at<Four>(p.y, g.f * p.y_frame + (long)y * p.y_pitch + (long)sizeof(S) * (4 * gx));
    const long co = g.f * p.c_frame + (long)y * p.c_pitch;
    float* d = px_at<false>(lr4, g.f, H, W, y, 4 * gx);
    f32x4 t[4];
    if constexpr (SX == 2) {
        unsigned cb[2], cr[2];
        load_pairs<S, STEP>(p, co, gx, cr_first, cb, cr);
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
        unsigned cb[4], cr[4];
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
#pragma unroll
        for (int j = 0; j < 4; ++j) t[j] = rgb0_of(k, val<S>(k, L::get(ya, j)), chroma_terms(k, val<S>(k, cb[j]), val<S>(k, cr[j])));
    }
    store_group(d, t);
}

// (n,3,H,W) fp32 planes -> planes at 4:2:2 | 4:4:4: one thread = one chroma sample = SX pixels of a row, single-sample stores; nothing
// beyond a row's width is written.  XM_PLAIN: the pixel's own pb, pr (SX 1) or (p0 + p1) * 0.5 (SX 2); XM_COSITED (SX 2): the taps
// max(2 bx - 1, 0), 2 bx, 2 bx + 1 as [1 2 1] / 4 -- one left neighbour, evaluated once more (the same fp32 operations: the same
// values), nothing outside the frame read.  i over n * H * (W / SX).
template <class S, int SX, int XM>
__global__ __launch_bounds__(256) void yuv_rows_out_kernel(const float* __restrict__ in, const YuvPlanes p, const YuvCoef k, int H, int W, long total) {
#pragma clang fp contract(off)
    static_assert(XM == XM_PLAIN || (SX == 2 && XM == XM_COSITED), "the forms of the way out");
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const Idx t = split(i, H, W / SX);
    const int y = t.row, bx = t.col;
    const long hw = (long)H * W;
    const float* s = in + t.f * 3 * hw + (long)y * W;
    S* yo = at<S>(p.y, t.f * p.y_frame + (long)y * p.y_pitch);
    constexpr int N = XM == XM_COSITED ? 3 : SX;
    const int x0 = XM == XM_COSITED ? 2 * bx - 1 : SX * bx;     // the first tap before it is clamped
    PbPr v[N];
#pragma unroll
    for (int c = 0; c < N; ++c) {
        const int x = max(x0 + c, 0);
        v[c] = px_out<S>(k, s + x, hw, yo + x, XM != XM_COSITED || c >= 1);
    }
    float mb, mr;
    if constexpr (XM == XM_COSITED) mb = tap121(v[0].pb, v[1].pb, v[2].pb), mr = tap121(v[0].pr, v[1].pr, v[2].pr);
    else if constexpr (SX == 2) mb = (v[0].pb + v[1].pb) * 0.5f, mr = (v[0].pr + v[1].pr) * 0.5f;
    else mb = v[0].pb, mr = v[0].pr;
    store_chroma<S>(p, k, t.f * p.c_frame + (long)y * p.c_pitch, (long)bx * p.c_step, mb, mr);
}

// ---- the host side.  A geometry is what the kernels of a family are templates on beside S: Blocks<CM> at 4:2:0, Rows<SX, XM> otherwise;
// sx, sy are the format's factors (a thread of the general forms owns sx x sy pixels).
template <int CM> struct Blocks { static constexpr int sx = 2, sy = 2; };
template <int SX, int XM> struct Rows { static constexpr int sx = SX, sy = 1; };

// the kernel of a form for a geometry.  On the way out CENTER writes what REPLICATE writes, in every format
template <class S, bool PLANAR, int CM> constexpr auto in_kernel(Blocks<CM>) { return yuv420_in_kernel<S, CM, PLANAR>; }
template <class S, bool PLANAR, int SX, int XM> constexpr auto in_kernel(Rows<SX, XM>) { return yuv_rows_in_kernel<S, SX, XM, PLANAR>; }
template <class S, int STEP, int CM> constexpr auto fast_kernel(Blocks<CM>) { return pack_lr_yuv420_fast_kernel<S, STEP, CM>; }
template <class S, int STEP, int SX, int XM> constexpr auto fast_kernel(Rows<SX, XM>) { return pack_lr_rows_fast_kernel<S, SX, STEP, XM>; }
template <class S, int CM> constexpr auto out_kernel(Blocks<CM>) { return yuv420_out_kernel<S, CM == PNP_YUV_CHROMA_CENTER ? PNP_YUV_CHROMA_REPLICATE : CM>; }
template <class S, int SX, int XM> constexpr auto out_kernel(Rows<SX, XM>) { return yuv_rows_out_kernel<S, SX, XM == XM_MIDWAY ? XM_PLAIN : XM>; }

// f(S(), geometry) for the sample size, the format and the mode: THE dispatch of all three launchers
template <class S, class F>
int dispatch_geometry(const YuvCoef& k, F&& f) {
    if (k.format == PNP_YUV_FORMAT_444) return f(S(), Rows<1, XM_PLAIN>());
    if (k.format == PNP_YUV_FORMAT_422) {
        if (k.chroma == PNP_YUV_CHROMA_REPLICATE) return f(S(), Rows<2, XM_PLAIN>());
        return k.chroma == PNP_YUV_CHROMA_CENTER ? f(S(), Rows<2, XM_MIDWAY>()) : f(S(), Rows<2, XM_COSITED>());
    }
    if (k.chroma == PNP_YUV_CHROMA_REPLICATE) return f(S(), Blocks<PNP_YUV_CHROMA_REPLICATE>());
    if (k.chroma == PNP_YUV_CHROMA_CENTER) return f(S(), Blocks<PNP_YUV_CHROMA_CENTER>());
    return k.chroma == PNP_YUV_CHROMA_LEFT ? f(S(), Blocks<PNP_YUV_CHROMA_LEFT>()) : f(S(), Blocks<PNP_YUV_CHROMA_TOPLEFT>());
}
template <class F>
int yuv_dispatch(const YuvPlanes& p, const YuvCoef& k, F&& f) {
    return p.sample_bytes == 1 ? dispatch_geometry<unsigned char>(k, f) : dispatch_geometry<unsigned short>(k, f);
}

// one thread per index below `total`, in blocks of 256; `total` is every kernel's last argument
template <class K, class... A>
int launch(K kernel, hipStream_t stream, long total, A... args) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, args..., total);
    return (int)hipGetLastError();
}

}  // namespace

int launch_pack_lr_yuv420(const YuvPlanes& in, const YuvCoef& k, float* lr4, int T, int H, int W, bool force_general, hipStream_t stream) {
    if (!yuv_frame_ok(k.format, T, H, W) || !lr4 || !yuv_planes_ok(in, W, k.format)) return PNP_ERR_BAD_ARG;
    const bool fast = !force_general && yuv_planes_fast(in, W, k.format);
    return yuv_dispatch(in, k, [&](auto s, auto g) {
        using S = decltype(s);
        using G = decltype(g);
        if (!fast) return launch(in_kernel<S, false>(g), stream, (long)T * (H / G::sy) * (W / G::sx), in, k, lr4, H, W);
        const long total = (long)T * (H / G::sy) * (W / 4);
        const int cr_first = in.cr < in.cb ? 1 : 0;
        return in.c_step == 2 ? launch(fast_kernel<S, 2>(g), stream, total, in, k, lr4, H, W, cr_first)
                              : launch(fast_kernel<S, 1>(g), stream, total, in, k, lr4, H, W, cr_first);
    });
}

int launch_frames_from_yuv420(const YuvPlanes& in, const YuvCoef& k, float* out, int nframes, int H, int W, hipStream_t stream) {
    if (!yuv_frame_ok(k.format, nframes, H, W) || !out || !yuv_planes_ok(in, W, k.format)) return PNP_ERR_BAD_ARG;
    return yuv_dispatch(in, k, [&](auto s, auto g) {
        using G = decltype(g);
        return launch(in_kernel<decltype(s), true>(g), stream, (long)nframes * (H / G::sy) * (W / G::sx), in, k, out, H, W);
    });
}

int launch_frames_to_yuv420(const float* in, const YuvPlanes& out, const YuvCoef& k, int nframes, int H, int W, hipStream_t stream) {
    if (!yuv_frame_ok(k.format, nframes, H, W) || !in || !yuv_planes_ok(out, W, k.format)) return PNP_ERR_BAD_ARG;
    return yuv_dispatch(out, k, [&](auto s, auto g) {
        using G = decltype(g);
        return launch(out_kernel<decltype(s)>(g), stream, (long)nframes * (H / G::sy) * (W / G::sx), in, out, k, H, W);
    });
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
