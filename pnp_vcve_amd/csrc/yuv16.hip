// 10 / 12-bit Y'CbCr 4:2:0 boundary: the planes a Main10 / VVC decoder writes (P010 / P012: the value in the high bits of a 16-bit
// word; yuv420p10le / yuv420p12le: in the low bits) straight into the conv source, and fp32 RGB planes out as such planes.  The
// arithmetic is the one include/pnpvcve.h states (pnp_yuv420_planes16): yuv.hip's formulas with the constants of the depth, rounded
// to fp32 once on the host (yuv16.h), every product and sum after that an fp32 operation rounded on its own -- contraction is off in
// every function that computes.  A thread owns whole 2x2 blocks and reads each chroma pair once.  Pitches and frame strides are
// bytes, c_step is samples; every address is even (yuv16_planes_ok).
#include "yuv16.h"

namespace {

__device__ __forceinline__ const unsigned short* at(const unsigned short* p, long bytes) {
    return reinterpret_cast<const unsigned short*>(reinterpret_cast<const char*>(p) + bytes);
}
__device__ __forceinline__ unsigned short* at(unsigned short* p, long bytes) {
    return reinterpret_cast<unsigned short*>(reinterpret_cast<char*>(p) + bytes);
}
__device__ __forceinline__ unsigned val(const YuvCoef16& c, unsigned word) { return (word >> c.shift) & c.vmask; }

// the chroma terms of a 2x2 block, shared by its four pixels
struct ChromaTerms16 { float rv, gu, gv, bu; };
__device__ __forceinline__ ChromaTerms16 chroma_terms(const YuvCoef16& c, unsigned cb, unsigned cr) {
#pragma clang fp contract(off)
    const float u = (float)((int)cb - c.cmid), v = (float)((int)cr - c.cmid);
    return ChromaTerms16{c.k.crv * v, c.k.cgu * u, c.k.cgv * v, c.k.cbu * u};
}
__device__ __forceinline__ f32x4 rgb0_of(const YuvCoef16& c, unsigned Y, const ChromaTerms16& t) {
#pragma clang fp contract(off)
    const float y = c.k.cy * (float)((int)Y - c.k.yoff);
    const float r = y + t.rv, g = (y - t.gu) - t.gv, b = y + t.bu;
    const f32x4 o = {fminf(fmaxf(r, 0.f), 1.f), fminf(fmaxf(g, 0.f), 1.f), fminf(fmaxf(b, 0.f), 1.f), 0.f};
    return o;
}

// General form: one thread = one 2x2 block, 2-byte loads at any even address and pitch.  i over T * (H/2) * (W/2).
__global__ __launch_bounds__(256) void pack_lr_yuv420p16_kernel(const pnp_yuv420_planes16 p, const YuvCoef16 k, float* __restrict__ lr4, int H, int W,
                                                                long total) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int bw = W >> 1, bh = H >> 1;
    const int bx = (int)(i % bw);
    const long r = i / bw;
    const int by = (int)(r % bh);
    const long f = r / bh;
    const unsigned short* y0 = at(p.y, f * p.y_frame + (long)(2 * by) * p.y_pitch) + 2 * bx;
    const unsigned short* y1 = at(y0, p.y_pitch);
    const long co = f * p.c_frame + (long)by * p.c_pitch;
    const long cx = (long)bx * p.c_step;
    const ChromaTerms16 c = chroma_terms(k, val(k, at(p.cb, co)[cx]), val(k, at(p.cr, co)[cx]));
    f32x4* d = reinterpret_cast<f32x4*>(lr4) + (f * H + 2 * by) * W + 2 * bx;
    const unsigned y00 = y0[0], y01 = y0[1], y10 = y1[0], y11 = y1[1];
    d[0] = rgb0_of(k, val(k, y00), c);
    d[1] = rgb0_of(k, val(k, y01), c);
    d[W] = rgb0_of(k, val(k, y10), c);
    d[W + 1] = rgb0_of(k, val(k, y11), c);
}

// Aligned fast form (yuv16_planes_fast): one thread = two rows of four pixels = two 8-byte loads of Y, one 8-byte load of the
// interleaved chroma row (STEP 2: words a0 b0 a1 b1 of the plane that starts first; cr_first says which one that is) or one 4-byte
// load of each chroma plane (STEP 1), and eight 16-byte stores, 64 contiguous bytes per row.  W is a multiple of 4.
// i over T * (H/2) * (W/4).
template <int STEP>
__global__ __launch_bounds__(256) void pack_lr_yuv420p16_fast_kernel(const pnp_yuv420_planes16 p, const YuvCoef16 k, float* __restrict__ lr4, int H,
                                                                     int W, int cr_first, long total) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int gw = W >> 2, bh = H >> 1;
    const int gx = (int)(i % gw);
    const long r = i / gw;
    const int by = (int)(r % bh);
    const long f = r / bh;
    const unsigned short* yp = at(p.y, f * p.y_frame + (long)(2 * by) * p.y_pitch) + 4 * gx;
    const uint2 ya = *reinterpret_cast<const uint2*>(yp), yb = *reinterpret_cast<const uint2*>(at(yp, p.y_pitch));
    unsigned cb0, cr0, cb1, cr1;
    const long co = f * p.c_frame + (long)by * p.c_pitch;
    if (STEP == 2) {
        const uint2 q = *reinterpret_cast<const uint2*>(at(cr_first ? p.cr : p.cb, co) + 4 * gx);
        const unsigned a0 = q.x & 0xffffu, b0 = q.x >> 16, a1 = q.y & 0xffffu, b1 = q.y >> 16;
        cb0 = cr_first ? b0 : a0, cr0 = cr_first ? a0 : b0;
        cb1 = cr_first ? b1 : a1, cr1 = cr_first ? a1 : b1;
    } else {
        const unsigned qb = *reinterpret_cast<const unsigned*>(at(p.cb, co) + 2 * gx), qr = *reinterpret_cast<const unsigned*>(at(p.cr, co) + 2 * gx);
        cb0 = qb & 0xffffu, cb1 = qb >> 16, cr0 = qr & 0xffffu, cr1 = qr >> 16;
    }
    const ChromaTerms16 c0 = chroma_terms(k, val(k, cb0), val(k, cr0)), c1 = chroma_terms(k, val(k, cb1), val(k, cr1));
    f32x4* d = reinterpret_cast<f32x4*>(lr4) + (f * H + 2 * by) * W + 4 * gx;
    const f32x4 t0 = rgb0_of(k, val(k, ya.x & 0xffffu), c0), t1 = rgb0_of(k, val(k, ya.x >> 16), c0);
    const f32x4 t2 = rgb0_of(k, val(k, ya.y & 0xffffu), c1), t3 = rgb0_of(k, val(k, ya.y >> 16), c1);
    const f32x4 u0 = rgb0_of(k, val(k, yb.x & 0xffffu), c0), u1 = rgb0_of(k, val(k, yb.x >> 16), c0);
    const f32x4 u2 = rgb0_of(k, val(k, yb.y & 0xffffu), c1), u3 = rgb0_of(k, val(k, yb.y >> 16), c1);
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
__global__ __launch_bounds__(256) void frames_from_yuv420p16_kernel(const pnp_yuv420_planes16 p, const YuvCoef16 k, float* __restrict__ out, int H,
                                                                    int W, long total) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int bw = W >> 1, bh = H >> 1;
    const int bx = (int)(i % bw);
    const long r = i / bw;
    const int by = (int)(r % bh);
    const long f = r / bh;
    const unsigned short* yp = at(p.y, f * p.y_frame + (long)(2 * by) * p.y_pitch) + 2 * bx;
    const long co = f * p.c_frame + (long)by * p.c_pitch;
    const long cx = (long)bx * p.c_step;
    const ChromaTerms16 c = chroma_terms(k, val(k, at(p.cb, co)[cx]), val(k, at(p.cr, co)[cx]));
    const long hw = (long)H * W;
    float* d = out + f * 3 * hw + (long)(2 * by) * W + 2 * bx;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int dy = j >> 1, dx = j & 1;
        const f32x4 v = rgb0_of(k, val(k, at(yp, dy * p.y_pitch)[dx]), c);
        float* q = d + dy * W + dx;
        q[0] = v[0];
        q[hw] = v[1];
        q[2 * hw] = v[2];
    }
}

// clamp(rint(x), 0, 2^d - 1), rint rounding half to even, in the container: the bits outside the value are zero
__device__ __forceinline__ unsigned short word_of(const YuvCoef16& c, float x) {
    return (unsigned short)((unsigned)fminf(fmaxf(rintf(x), 0.f), c.vmax) << c.shift);
}

// (n,3,H,W) fp32 planes -> planes: one thread = one 2x2 block = four Y words and one chroma pair, 2-byte stores at any even address;
// nothing beyond a row's width is written
__global__ __launch_bounds__(256) void frames_to_yuv420p16_kernel(const float* __restrict__ in, const pnp_yuv420_planes16 p, const YuvCoef16 c, int H,
                                                                  int W, long total) {
#pragma clang fp contract(off)
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const YuvCoef& k = c.k;
    const int bw = W >> 1, bh = H >> 1;
    const int bx = (int)(i % bw);
    const long r = i / bw;
    const int by = (int)(r % bh);
    const long f = r / bh;
    const long hw = (long)H * W;
    const float* s = in + f * 3 * hw + (long)(2 * by) * W + 2 * bx;
    unsigned short* yp = at(p.y, f * p.y_frame + (long)(2 * by) * p.y_pitch) + 2 * bx;
    float pb[4], pr[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {       // 00, 01, 10, 11: rows top then bottom, columns left then right
        const int dy = j >> 1, dx = j & 1;
        const float* q = s + dy * W + dx;
        const float rr = fminf(fmaxf(q[0], 0.f), 1.f), gg = fminf(fmaxf(q[hw], 0.f), 1.f), bb = fminf(fmaxf(q[2 * hw], 0.f), 1.f);
        const float yl = (k.kr * rr + k.kg * gg) + k.kb * bb;
        at(yp, dy * p.y_pitch)[dx] = word_of(c, (float)k.yoff + k.sy * yl);
        pb[j] = (bb - yl) * k.ipb;
        pr[j] = (rr - yl) * k.ipr;
    }
    const float mb = ((pb[0] + pb[1]) + (pb[2] + pb[3])) * 0.25f, mr = ((pr[0] + pr[1]) + (pr[2] + pr[3])) * 0.25f;
    const long co = f * p.c_frame + (long)by * p.c_pitch;
    const long cx = (long)bx * p.c_step;
    at(p.cb, co)[cx] = word_of(c, (float)c.cmid + k.sc * mb);
    at(p.cr, co)[cx] = word_of(c, (float)c.cmid + k.sc * mr);
}

unsigned blocks_of(long total) { return (unsigned)((total + 255) / 256); }

bool frame_ok(int n, int H, int W) { return n >= 1 && H >= 2 && W >= 2 && !(H & 1) && !(W & 1); }

}  // namespace

int launch_pack_lr_yuv420p16(const pnp_yuv420_planes16& in, const YuvCoef16& k, float* lr4, int T, int H, int W, bool force_general, hipStream_t stream) {
    if (!frame_ok(T, H, W) || !lr4 || !yuv16_planes_ok(in, W)) return PNP_ERR_BAD_ARG;
    if (!force_general && yuv16_planes_fast(in, W)) {
        const long total = (long)T * (H / 2) * (W / 4);
        const int cr_first = in.cr < in.cb ? 1 : 0;
        if (in.c_step == 2) hipLaunchKernelGGL(pack_lr_yuv420p16_fast_kernel<2>, dim3(blocks_of(total)), dim3(256), 0, stream, in, k, lr4, H, W, cr_first, total);
        else hipLaunchKernelGGL(pack_lr_yuv420p16_fast_kernel<1>, dim3(blocks_of(total)), dim3(256), 0, stream, in, k, lr4, H, W, cr_first, total);
        return (int)hipGetLastError();
    }
    const long total = (long)T * (H / 2) * (W / 2);
    hipLaunchKernelGGL(pack_lr_yuv420p16_kernel, dim3(blocks_of(total)), dim3(256), 0, stream, in, k, lr4, H, W, total);
    return (int)hipGetLastError();
}

int launch_frames_from_yuv420p16(const pnp_yuv420_planes16& in, const YuvCoef16& k, float* out, int nframes, int H, int W, hipStream_t stream) {
    if (!frame_ok(nframes, H, W) || !out || !yuv16_planes_ok(in, W)) return PNP_ERR_BAD_ARG;
    const long total = (long)nframes * (H / 2) * (W / 2);
    hipLaunchKernelGGL(frames_from_yuv420p16_kernel, dim3(blocks_of(total)), dim3(256), 0, stream, in, k, out, H, W, total);
    return (int)hipGetLastError();
}

int launch_frames_to_yuv420p16(const float* in, const pnp_yuv420_planes16& out, const YuvCoef16& k, int nframes, int H, int W, hipStream_t stream) {
    if (!frame_ok(nframes, H, W) || !in || !yuv16_planes_ok(out, W)) return PNP_ERR_BAD_ARG;
    const long total = (long)nframes * (H / 2) * (W / 2);
    hipLaunchKernelGGL(frames_to_yuv420p16_kernel, dim3(blocks_of(total)), dim3(256), 0, stream, in, out, k, H, W, total);
    return (int)hipGetLastError();
}

extern "C" {

int pnp_frames_from_yuv420p16(const pnp_yuv420_planes16* in, int yuv_standard, float* out_planes, int n, int h, int w, void* stream) {
    YuvCoef16 k;
    if (!in || !out_planes || !frame_ok(n, h, w) || !yuv_coef16(yuv_standard, in->bit_depth, in->msb_aligned, &k) || !yuv16_planes_ok(*in, w))
        return PNP_ERR_BAD_ARG;
    return launch_frames_from_yuv420p16(*in, k, out_planes, n, h, w, (hipStream_t)stream);
}

int pnp_frames_to_yuv420p16(const float* planes, const pnp_yuv420_planes16* out, int yuv_standard, int n, int h, int w, void* stream) {
    YuvCoef16 k;
    if (!out || !planes || !frame_ok(n, h, w) || !yuv_coef16(yuv_standard, out->bit_depth, out->msb_aligned, &k) || !yuv16_planes_ok(*out, w))
        return PNP_ERR_BAD_ARG;
    return launch_frames_to_yuv420p16(planes, *out, k, n, h, w, (hipStream_t)stream);
}

int pnp_debug_pack_lr_yuv420p16(const pnp_yuv420_planes16* in, int yuv_standard, float* lr4, int t, int h, int w, int general, void* stream) {
    YuvCoef16 k;
    if (!in || !lr4 || !yuv_coef16(yuv_standard, in->bit_depth, in->msb_aligned, &k)) return PNP_ERR_BAD_ARG;
    return launch_pack_lr_yuv420p16(*in, k, lr4, t, h, w, general != 0, (hipStream_t)stream);
}

}  // extern "C"
