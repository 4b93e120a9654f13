// Y'CbCr 4:2:0 boundary: the decoder's planes (NV12 / NV21 / I420, 8 bit) straight into the conv source, and fp32 RGB planes out as
// planes an encoder or a display takes.  The arithmetic is the one include/pnpvcve.h states (pnp_frames_from_yuv420 /
// pnp_frames_to_yuv420): constants rounded to fp32 once on the host (yuv.h), every product and sum after that an fp32 operation
// rounded on its own -- contraction is off in every function that computes.  Chroma is replicated on the way in (pixel (y, x) reads
// sample (y >> 1, x >> 1)) and box-averaged on the way out, so a thread owns whole 2x2 blocks and reads each chroma pair once.
#include "yuv.h"

namespace {

// the chroma terms of a 2x2 block, shared by its four pixels
struct ChromaTerms { float rv, gu, gv, bu; };
__device__ __forceinline__ ChromaTerms chroma_terms(const YuvCoef& k, unsigned cb, unsigned cr) {
#pragma clang fp contract(off)
    const float u = (float)((int)cb - 128), v = (float)((int)cr - 128);
    return ChromaTerms{k.crv * v, k.cgu * u, k.cgv * v, k.cbu * u};
}
__device__ __forceinline__ f32x4 rgb0_of(const YuvCoef& k, unsigned Y, const ChromaTerms& c) {
#pragma clang fp contract(off)
    const float y = k.cy * (float)((int)Y - k.yoff);
    const float r = y + c.rv, g = (y - c.gu) - c.gv, b = y + c.bu;
    const f32x4 o = {fminf(fmaxf(r, 0.f), 1.f), fminf(fmaxf(g, 0.f), 1.f), fminf(fmaxf(b, 0.f), 1.f), 0.f};
    return o;
}

// General form: one thread = one 2x2 block, byte loads at any address and pitch.  i over T * (H/2) * (W/2).
__global__ __launch_bounds__(256) void pack_lr_yuv420_kernel(const pnp_yuv420_planes p, const YuvCoef k, float* __restrict__ lr4, int H, int W,
                                                             long total) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int bw = W >> 1, bh = H >> 1;
    const int bx = (int)(i % bw);
    const long r = i / bw;
    const int by = (int)(r % bh);
    const long f = r / bh;
    const unsigned char* yp = p.y + f * p.y_frame + (long)(2 * by) * p.y_pitch + 2 * bx;
    const long co = f * p.c_frame + (long)by * p.c_pitch + (long)bx * p.c_step;
    const ChromaTerms c = chroma_terms(k, p.cb[co], p.cr[co]);
    f32x4* d = reinterpret_cast<f32x4*>(lr4) + (f * H + 2 * by) * W + 2 * bx;
    const unsigned y00 = yp[0], y01 = yp[1], y10 = yp[p.y_pitch], y11 = yp[p.y_pitch + 1];
    d[0] = rgb0_of(k, y00, c);
    d[1] = rgb0_of(k, y01, c);
    d[W] = rgb0_of(k, y10, c);
    d[W + 1] = rgb0_of(k, y11, c);
}

// Aligned fast form (yuv_planes_fast): one thread = two rows of four pixels = two dword loads of Y, one dword of the interleaved
// chroma row (STEP 2: bytes a0 b0 a1 b1 of the plane that starts first; cr_first says which one that is) or one 16-bit load of each
// chroma plane (STEP 1), and eight 16-byte stores, 64 contiguous bytes per row.  W is a multiple of 4.  i over T * (H/2) * (W/4).
template <int STEP>
__global__ __launch_bounds__(256) void pack_lr_yuv420_fast_kernel(const pnp_yuv420_planes p, const YuvCoef k, float* __restrict__ lr4, int H, int W,
                                                                  int cr_first, long total) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int gw = W >> 2, bh = H >> 1;
    const int gx = (int)(i % gw);
    const long r = i / gw;
    const int by = (int)(r % bh);
    const long f = r / bh;
    const unsigned char* yp = p.y + f * p.y_frame + (long)(2 * by) * p.y_pitch + 4 * gx;
    const unsigned ya = *reinterpret_cast<const unsigned*>(yp), yb = *reinterpret_cast<const unsigned*>(yp + p.y_pitch);
    unsigned cb0, cr0, cb1, cr1;
    if (STEP == 2) {
        const unsigned char* lo = cr_first ? p.cr : p.cb;
        const unsigned q = *reinterpret_cast<const unsigned*>(lo + f * p.c_frame + (long)by * p.c_pitch + 4 * gx);
        const unsigned a0 = q & 255u, b0 = (q >> 8) & 255u, a1 = (q >> 16) & 255u, b1 = q >> 24;
        cb0 = cr_first ? b0 : a0, cr0 = cr_first ? a0 : b0;
        cb1 = cr_first ? b1 : a1, cr1 = cr_first ? a1 : b1;
    } else {
        const long co = f * p.c_frame + (long)by * p.c_pitch + 2 * gx;
        const unsigned qb = *reinterpret_cast<const unsigned short*>(p.cb + co), qr = *reinterpret_cast<const unsigned short*>(p.cr + co);
        cb0 = qb & 255u, cb1 = qb >> 8, cr0 = qr & 255u, cr1 = qr >> 8;
    }
    const ChromaTerms c0 = chroma_terms(k, cb0, cr0), c1 = chroma_terms(k, cb1, cr1);
    f32x4* d = reinterpret_cast<f32x4*>(lr4) + (f * H + 2 * by) * W + 4 * gx;
    const f32x4 t0 = rgb0_of(k, ya & 255u, c0), t1 = rgb0_of(k, (ya >> 8) & 255u, c0), t2 = rgb0_of(k, (ya >> 16) & 255u, c1), t3 = rgb0_of(k, ya >> 24, c1);
    const f32x4 u0 = rgb0_of(k, yb & 255u, c0), u1 = rgb0_of(k, (yb >> 8) & 255u, c0), u2 = rgb0_of(k, (yb >> 16) & 255u, c1), u3 = rgb0_of(k, yb >> 24, c1);
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
__global__ __launch_bounds__(256) void frames_from_yuv420_kernel(const pnp_yuv420_planes p, const YuvCoef k, float* __restrict__ out, int H, int W,
                                                                 long total) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int bw = W >> 1, bh = H >> 1;
    const int bx = (int)(i % bw);
    const long r = i / bw;
    const int by = (int)(r % bh);
    const long f = r / bh;
    const unsigned char* yp = p.y + f * p.y_frame + (long)(2 * by) * p.y_pitch + 2 * bx;
    const long co = f * p.c_frame + (long)by * p.c_pitch + (long)bx * p.c_step;
    const ChromaTerms c = chroma_terms(k, p.cb[co], p.cr[co]);
    const long hw = (long)H * W;
    float* d = out + f * 3 * hw + (long)(2 * by) * W + 2 * bx;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int dy = j >> 1, dx = j & 1;
        const f32x4 v = rgb0_of(k, yp[dy * p.y_pitch + dx], c);
        float* q = d + dy * W + dx;
        q[0] = v[0];
        q[hw] = v[1];
        q[2 * hw] = v[2];
    }
}

__device__ __forceinline__ unsigned char byte_of(float x) {      // clamp(rint(x), 0, 255), rint rounding half to even
    return (unsigned char)fminf(fmaxf(rintf(x), 0.f), 255.f);
}

// (n,3,H,W) fp32 planes -> planes: one thread = one 2x2 block = four Y bytes and one chroma pair, byte stores at any address; nothing
// beyond a row's width is written
__global__ __launch_bounds__(256) void frames_to_yuv420_kernel(const float* __restrict__ in, const pnp_yuv420_planes p, const YuvCoef k, int H, int W,
                                                               long total) {
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
    unsigned char* yp = p.y + f * p.y_frame + (long)(2 * by) * p.y_pitch + 2 * bx;
    float pb[4], pr[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {       // 00, 01, 10, 11: rows top then bottom, columns left then right
        const int dy = j >> 1, dx = j & 1;
        const float* q = s + dy * W + dx;
        const float rr = fminf(fmaxf(q[0], 0.f), 1.f), gg = fminf(fmaxf(q[hw], 0.f), 1.f), bb = fminf(fmaxf(q[2 * hw], 0.f), 1.f);
        const float yl = (k.kr * rr + k.kg * gg) + k.kb * bb;
        yp[dy * p.y_pitch + dx] = byte_of((float)k.yoff + k.sy * yl);
        pb[j] = (bb - yl) * k.ipb;
        pr[j] = (rr - yl) * k.ipr;
    }
    const float mb = ((pb[0] + pb[1]) + (pb[2] + pb[3])) * 0.25f, mr = ((pr[0] + pr[1]) + (pr[2] + pr[3])) * 0.25f;
    const long co = f * p.c_frame + (long)by * p.c_pitch + (long)bx * p.c_step;
    p.cb[co] = byte_of(128.0f + k.sc * mb);
    p.cr[co] = byte_of(128.0f + k.sc * mr);
}

unsigned blocks_of(long total) { return (unsigned)((total + 255) / 256); }

}  // namespace

int launch_pack_lr_yuv420(const pnp_yuv420_planes& in, const YuvCoef& k, float* lr4, int T, int H, int W, bool force_general, hipStream_t stream) {
    if (T < 1 || H < 2 || W < 2 || (H & 1) || (W & 1) || !lr4 || !yuv_planes_ok(in, W)) return PNP_ERR_BAD_ARG;
    if (!force_general && yuv_planes_fast(in, W)) {
        const long total = (long)T * (H / 2) * (W / 4);
        const int cr_first = in.cr < in.cb ? 1 : 0;
        if (in.c_step == 2) hipLaunchKernelGGL(pack_lr_yuv420_fast_kernel<2>, dim3(blocks_of(total)), dim3(256), 0, stream, in, k, lr4, H, W, cr_first, total);
        else hipLaunchKernelGGL(pack_lr_yuv420_fast_kernel<1>, dim3(blocks_of(total)), dim3(256), 0, stream, in, k, lr4, H, W, cr_first, total);
        return (int)hipGetLastError();
    }
    const long total = (long)T * (H / 2) * (W / 2);
    hipLaunchKernelGGL(pack_lr_yuv420_kernel, dim3(blocks_of(total)), dim3(256), 0, stream, in, k, lr4, H, W, total);
    return (int)hipGetLastError();
}

int launch_frames_from_yuv420(const pnp_yuv420_planes& in, const YuvCoef& k, float* out, int nframes, int H, int W, hipStream_t stream) {
    if (nframes < 1 || H < 2 || W < 2 || (H & 1) || (W & 1) || !out || !yuv_planes_ok(in, W)) return PNP_ERR_BAD_ARG;
    const long total = (long)nframes * (H / 2) * (W / 2);
    hipLaunchKernelGGL(frames_from_yuv420_kernel, dim3(blocks_of(total)), dim3(256), 0, stream, in, k, out, H, W, total);
    return (int)hipGetLastError();
}

int launch_frames_to_yuv420(const float* in, const pnp_yuv420_planes& out, const YuvCoef& k, int nframes, int H, int W, hipStream_t stream) {
    if (nframes < 1 || H < 2 || W < 2 || (H & 1) || (W & 1) || !in || !yuv_planes_ok(out, W)) return PNP_ERR_BAD_ARG;
    const long total = (long)nframes * (H / 2) * (W / 2);
    hipLaunchKernelGGL(frames_to_yuv420_kernel, dim3(blocks_of(total)), dim3(256), 0, stream, in, out, k, H, W, total);
    return (int)hipGetLastError();
}

extern "C" {

int pnp_frames_from_yuv420(const pnp_yuv420_planes* in, int yuv_standard, float* out_planes, int n, int h, int w, void* stream) {
    YuvCoef k;
    if (!in || !out_planes || n < 1 || h < 2 || w < 2 || (h & 1) || (w & 1) || !yuv_coef(yuv_standard, &k) || !yuv_planes_ok(*in, w)) return PNP_ERR_BAD_ARG;
    return launch_frames_from_yuv420(*in, k, out_planes, n, h, w, (hipStream_t)stream);
}

int pnp_frames_to_yuv420(const float* planes, const pnp_yuv420_planes* out, int yuv_standard, int n, int h, int w, void* stream) {
    YuvCoef k;
    if (!out || !planes || n < 1 || h < 2 || w < 2 || (h & 1) || (w & 1) || !yuv_coef(yuv_standard, &k) || !yuv_planes_ok(*out, w)) return PNP_ERR_BAD_ARG;
    return launch_frames_to_yuv420(planes, *out, k, n, h, w, (hipStream_t)stream);
}

int pnp_debug_pack_lr_yuv420(const pnp_yuv420_planes* in, int yuv_standard, float* lr4, int t, int h, int w, int general, void* stream) {
    YuvCoef k;
    if (!in || !lr4 || !yuv_coef(yuv_standard, &k)) return PNP_ERR_BAD_ARG;
    return launch_pack_lr_yuv420(*in, k, lr4, t, h, w, general != 0, (hipStream_t)stream);
}

}  // extern "C"
