// On-device PSNR statistic (the step right after the hot path).
//
// Reference: BasicVSR.evaluate (mmedit/models/restorers/basicvsr.py:119-153) moves every frame
// to the host, tensor2img (mmedit/core/misc.py:51-71: clamp to [0,1], *255, round -> uint8) and
// psnr (mmedit/core/evaluation/metrics.py:200-215: mean squared uint8 difference).
// Here: one pass over the two frames in HBM, rounding exactly as numpy does (half to even), the
// squared differences summed as 64-bit INTEGERS (exact, order-independent, deterministic), so the
// host only sees 8 bytes per frame instead of 2 x 3*H*W*4.  HBM-bound: 8 B per element.
#include "metric_src.h"
#include <cmath>

namespace {

// a, b: (frames, C, H, W) fp32; sse: (frames) u64, zeroed by the launcher
__global__ __launch_bounds__(256) void psnr_sse_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                       unsigned long long* __restrict__ sse, int C, int H, int W,
                                                       int crop) {
    const int frame = blockIdx.y;
    const long plane = (long)H * W, per = plane * C;
    const float* fa = a + frame * per;
    const float* fb = b + frame * per;
    unsigned long long acc = 0;
    if (crop == 0 && (per & 3) == 0) {
        const f32x4* a4 = reinterpret_cast<const f32x4*>(fa);
        const f32x4* b4 = reinterpret_cast<const f32x4*>(fb);
        for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < per / 4; i += (long)gridDim.x * blockDim.x) {
            const f32x4 x = a4[i], y = b4[i];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int d = to_u8(x[k]) - to_u8(y[k]);
                acc += (unsigned)(d * d);
            }
        }
    } else {
        for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < per; i += (long)gridDim.x * blockDim.x) {
            const long p = i % plane;
            const int yy = (int)(p / W), xx = (int)(p - (long)yy * W);
            if (yy < crop || yy >= H - crop || xx < crop || xx >= W - crop) continue;
            const int d = to_u8(fa[i]) - to_u8(fb[i]);
            acc += (unsigned)(d * d);
        }
    }
    // wave reduction, then one atomic per wave
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((threadIdx.x & 63) == 0 && acc) atomicAdd(&sse[frame], acc);
}

// ---------------------------------------------------------------------------------------------
// SSIM (mmedit/core/evaluation/metrics.py:266-355): per channel, 11x11 Gaussian (sigma 1.5) 'valid' window
// over the uint8-rounded frames, in fp64 like the reference.  The reference filters with cv2.filter2D
// (absent here -> parity unpinned; checked against the numpy restatement in pnp_vcve_amd/metrics.py).
// One block = a 16x32 tile of the valid map of one (frame, channel): the two u8 tiles (26x42) go to LDS,
// a horizontal pass leaves the five windowed moments of 26x32 positions in LDS, the vertical pass finishes
// them and forms the SSIM ratio; each block writes ONE partial sum (deterministic; the host adds them).
struct SsimArgs {
    double g[11];
    const float* a;
    const float* b;
    double* partial;       // [frames*C][blocks_per_plane]
    int H, W, crop, oh, ow, tiles_x, blocks_per_plane;
};

__global__ __launch_bounds__(256) void ssim_kernel(const SsimArgs s) {
    __shared__ float ta[26 * 42], tb[26 * 42];
    __shared__ double hm[5][26 * 32];
    __shared__ double red[4];
    const int plane = blockIdx.y, blk = blockIdx.x, t = threadIdx.x;
    const int ty0 = (blk / s.tiles_x) * 16, tx0 = (blk % s.tiles_x) * 32;        // in valid-map coordinates
    const float* pa = s.a + (long)plane * s.H * s.W;
    const float* pb = s.b + (long)plane * s.H * s.W;
    for (int i = t; i < 26 * 42; i += 256) {
        const int r = i / 42, c = i - r * 42;
        const int y = s.crop + ty0 + r, x = s.crop + tx0 + c;
        float va = 0.f, vb = 0.f;
        if (y < s.H - s.crop && x < s.W - s.crop) {
            va = (float)to_u8(pa[(long)y * s.W + x]);
            vb = (float)to_u8(pb[(long)y * s.W + x]);
        }
        ta[i] = va;
        tb[i] = vb;
    }
    __syncthreads();
    for (int i = t; i < 26 * 32; i += 256) {
        const int r = i >> 5, c = i & 31;
        double m1 = 0, m2 = 0, s11 = 0, s22 = 0, s12 = 0;
#pragma unroll
        for (int k = 0; k < 11; ++k) {
            const double x = ta[r * 42 + c + k], y = tb[r * 42 + c + k], gk = s.g[k];
            m1 += gk * x;
            m2 += gk * y;
            s11 += gk * x * x;
            s22 += gk * y * y;
            s12 += gk * x * y;
        }
        hm[0][i] = m1;
        hm[1][i] = m2;
        hm[2][i] = s11;
        hm[3][i] = s22;
        hm[4][i] = s12;
    }
    __syncthreads();
    const double C1 = (0.01 * 255) * (0.01 * 255), C2 = (0.03 * 255) * (0.03 * 255);
    double acc = 0;
    for (int i = t; i < 16 * 32; i += 256) {
        const int r = i >> 5, c = i & 31;
        if (ty0 + r >= s.oh || tx0 + c >= s.ow) continue;
        double v[5] = {0, 0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < 11; ++k)
#pragma unroll
            for (int q = 0; q < 5; ++q) v[q] += s.g[k] * hm[q][(r + k) * 32 + c];
        const double mu1 = v[0], mu2 = v[1];
        const double sg1 = v[2] - mu1 * mu1, sg2 = v[3] - mu2 * mu2, sg12 = v[4] - mu1 * mu2;
        acc += ((2 * mu1 * mu2 + C1) * (2 * sg12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (sg1 + sg2 + C2));
    }
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((t & 63) == 0) red[t >> 6] = acc;
    __syncthreads();
    if (t == 0) s.partial[(long)plane * s.blocks_per_plane + blk] = red[0] + red[1] + red[2] + red[3];
}

}  // namespace

extern "C" int pnp_ssim_blocks(int h, int w, int crop_border) {
    const int oh = h - 2 * crop_border - 10, ow = w - 2 * crop_border - 10;
    if (oh < 1 || ow < 1) return 0;
    return ((oh + 15) / 16) * ((ow + 31) / 32);
}

extern "C" int pnp_ssim_partials_f32(const float* a, const float* b, double* partials, int frames, int c, int h, int w,
                                     int crop_border, void* stream) {
    const int nb = pnp_ssim_blocks(h, w, crop_border);
    if (frames < 1 || c < 1 || nb < 1 || crop_border < 0) return PNP_ERR_BAD_ARG;
    SsimArgs s;
    double sum = 0;
    for (int i = 0; i < 11; ++i) {                       // cv2.getGaussianKernel(11, 1.5)
        s.g[i] = exp(-((i - 5.0) * (i - 5.0)) / (2 * 1.5 * 1.5));
        sum += s.g[i];
    }
    for (int i = 0; i < 11; ++i) s.g[i] /= sum;
    s.a = a;
    s.b = b;
    s.partial = partials;
    s.H = h;
    s.W = w;
    s.crop = crop_border;
    s.oh = h - 2 * crop_border - 10;
    s.ow = w - 2 * crop_border - 10;
    s.tiles_x = (s.ow + 31) / 32;
    s.blocks_per_plane = nb;
    hipLaunchKernelGGL(ssim_kernel, dim3(nb, frames * c), dim3(256), 0, (hipStream_t)stream, s);
    return (int)hipGetLastError();
}

extern "C" int pnp_psnr_sse_f32(const float* a, const float* b, unsigned long long* sse, int frames, int c, int h,
                                int w, int crop_border, void* stream) {
    if (frames < 1 || c < 1 || h < 1 || w < 1 || crop_border < 0 || 2 * crop_border >= h || 2 * crop_border >= w)
        return PNP_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    const int ze = launch_zero_words(sse, 2L * frames, st);      // a kernel, not a memset node (prep.h)
    if (ze != PNP_OK) return ze;
    const long per = (long)c * h * w;
    long bx = (per / 4 + 255) / 256;
    if (bx > 1024) bx = 1024;
    if (bx < 1) bx = 1;
    hipLaunchKernelGGL(psnr_sse_kernel, dim3((unsigned)bx, frames), dim3(256), 0, st, a, b, sse, c, h, w, crop_border);
    return (int)hipGetLastError();
}

// tensor2img for the write-back (mmedit/core/misc.py:51-71 + mmcv.imwrite, basicvsr.py:205-231): (frames,3,h,w) fp32
// planes -> (frames,h,w,3) uint8 RGB, clamp to [0,1], * 255, round half to even -- a quarter of the D2H bytes.
namespace {
__global__ __launch_bounds__(256) void frames_to_rgb8_kernel(const float* __restrict__ x, unsigned char* __restrict__ out,
                                                             long hw, long total) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;       // over frames * hw pixels
    if (i >= total) return;
    const long f = i / hw, p = i - f * hw;
    const float* s = x + f * 3 * hw + p;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float v = fminf(fmaxf(s[c * hw], 0.f), 1.f) * 255.0f;
        out[i * 3 + c] = (unsigned char)rintf(v);
    }
}

// The inverse layout: (frames,h,w,3) uint8 RGB -> (frames,3,h,w) fp32 planes, byte v -> float(v) / 255.0f through the table of
// prep.h (what the loader's RescaleToZeroOne + HWC->CHW make of a decoded frame, bit for bit).
__device__ const PnpU8Table k_u8_table = PnpU8Table();

__global__ __launch_bounds__(256) void frames_from_rgb8_kernel(const unsigned char* __restrict__ in, float* __restrict__ out,
                                                               long hw, long total) {
    __shared__ float tab[256];
    tab[threadIdx.x] = k_u8_table.v[threadIdx.x];
    __syncthreads();
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;       // over frames * hw pixels
    if (i >= total) return;
    const long f = i / hw, p = i - f * hw;
    float* d = out + f * 3 * hw + p;
#pragma unroll
    for (int c = 0; c < 3; ++c) d[c * hw] = tab[in[i * 3 + c]];
}
}  // namespace

int launch_frames_to_rgb8(const float* frames, unsigned char* out, int nframes, int h, int w, hipStream_t stream) {
    const long hw = (long)h * w, total = hw * nframes;
    hipLaunchKernelGGL(frames_to_rgb8_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, frames, out, hw, total);
    return (int)hipGetLastError();
}

int launch_frames_from_rgb8(const unsigned char* in, float* out, int nframes, int h, int w, hipStream_t stream) {
    const long hw = (long)h * w, total = hw * nframes;
    hipLaunchKernelGGL(frames_from_rgb8_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, in, out, hw, total);
    return (int)hipGetLastError();
}

extern "C" int pnp_frames_to_rgb8(const float* frames, unsigned char* out, int nframes, int h, int w, void* stream) {
    if (nframes < 1 || h < 1 || w < 1 || !frames || !out) return PNP_ERR_BAD_ARG;
    return launch_frames_to_rgb8(frames, out, nframes, h, w, (hipStream_t)stream);
}

extern "C" int pnp_frames_from_rgb8(const unsigned char* in, float* out, int nframes, int h, int w, void* stream) {
    if (nframes < 1 || h < 1 || w < 1 || !in || !out) return PNP_ERR_BAD_ARG;
    return launch_frames_from_rgb8(in, out, nframes, h, w, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------
// The same statistics behind a front end that does not care how a frame is stored -- (frames,3,h,w) fp32 planes, rounded by to_u8, or
// (frames,h,w,3) uint8 RGB, the byte as it is, each input on its own -- with an optional luma step between the byte and the statistic
// (test_cfg.convert_to = 'y': basicvsr.py:132-150 -> metrics.py:200-206, 338-346).  The metric of two byte clips reads 6 B per pixel.
// The loaders and the luma step are metric_src.h's (msssim.hip reads through them too).
namespace {

// The pixels of a frame inside the crop as `rows` runs of `roww` consecutive pixels (crop 0: ONE run of h*w), each cut into groups of
// four: group g -> its first pixel and how many of the four exist.
struct PixelRuns {
    long hw, roww, gpr, groups;     // gpr: groups per run
    int W, crop, rows;
    __host__ PixelRuns(int h, int w, int c) : hw((long)h * w), W(w), crop(c) {
        rows = c ? h - 2 * c : 1;
        roww = c ? w - 2 * c : hw;
        gpr = (roww + 3) / 4;
        groups = gpr * rows;
    }
    __device__ __forceinline__ long first(long g, int& npix) const {
        const long r = rows == 1 ? 0 : g / gpr, gx = g - r * gpr;
        const long left = roww - 4 * gx;
        npix = left < 4 ? (int)left : 4;
        return (crop + r) * W + crop + 4 * gx;
    }
};

struct PsnrIoArgs {
    FrameSrc a, b;
    PixelRuns runs;
    unsigned long long* sse;    // !Y: (frames), zeroed by the launcher
    double* partial;            //  Y: [frames][gridDim.x]
};

// !Y: the exact integer SSE of the three channels, one integer atomic per wave like psnr_sse_kernel.  Y: d = Y_a - Y_b in fp32 as the
// reference subtracts, (double)d * d (exact: 48 bits) summed in fp64 in a fixed order -- a thread's groups in index order, the wave
// by shuffles, the block's four waves through four doubles of LDS -- and ONE partial per block, which the host adds in index order.
template <bool Y>
__global__ __launch_bounds__(256) void psnr_io_kernel(const PsnrIoArgs s) {
    __shared__ double lt[Y ? 768 : 1];
    __shared__ double red[4];
    if (Y) stage_luma_table(lt);
    const long frame = blockIdx.y;
    unsigned long long acc = 0;
    double accd = 0;
    for (long g = (long)blockIdx.x * 256 + threadIdx.x; g < s.runs.groups; g += (long)gridDim.x * 256) {
        int npix;
        const long p0 = s.runs.first(g, npix);
        unsigned pa[4], pb[4];
        load_px4(s.a, frame, s.runs.hw, p0, npix, pa);
        load_px4(s.b, frame, s.runs.hw, p0, npix, pb);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j >= npix) continue;
            if (Y) {
                const float d = luma_of(lt, pa[j]) - luma_of(lt, pb[j]);
                accd += (double)d * (double)d;
            } else {
                unsigned e = 0;
#pragma unroll
                for (int k = 0; k < 24; k += 8) {
                    const int d = (int)((pa[j] >> k) & 255u) - (int)((pb[j] >> k) & 255u);
                    e += (unsigned)(d * d);
                }
                acc += e;
            }
        }
    }
    if (Y) {
        for (int off = 32; off > 0; off >>= 1) accd += __shfl_down(accd, off, 64);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = accd;
        __syncthreads();
        if (threadIdx.x == 0) s.partial[frame * gridDim.x + blockIdx.x] = red[0] + red[1] + red[2] + red[3];
    } else {
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
        if ((threadIdx.x & 63) == 0 && acc) atomicAdd(&s.sse[frame], acc);
    }
}

// frames of either format -> (frames, h, w) fp32 Y; four pixels per thread, one 16-byte store where the address allows
__global__ __launch_bounds__(256) void luma_kernel(const FrameSrc src, float* __restrict__ out, long hw, long groups) {
    __shared__ double lt[768];
    stage_luma_table(lt);
    const long frame = blockIdx.y;
    for (long g = (long)blockIdx.x * 256 + threadIdx.x; g < groups; g += (long)gridDim.x * 256) {
        const long p0 = 4 * g, left = hw - p0;
        const int npix = left < 4 ? (int)left : 4;
        unsigned px[4];
        load_px4(src, frame, hw, p0, npix, px);
        float* o = out + frame * hw + p0;
        if (npix == 4 && (reinterpret_cast<uintptr_t>(o) & 15) == 0) {
            const f32x4 y = {luma_of(lt, px[0]), luma_of(lt, px[1]), luma_of(lt, px[2]), luma_of(lt, px[3])};
            *reinterpret_cast<f32x4*>(o) = y;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < npix) o[j] = luma_of(lt, px[j]);
        }
    }
}

// ssim_kernel with a loader in front: the value of (plane, y, x) comes from either format and, with Y, through the luma step (one
// plane per frame, the window runs over the fp32 Y).  Tiling, LDS layout and both passes are ssim_kernel's, statement for statement,
// so a byte frame gives the partials of its fp32 planes bit for bit.
struct SsimIoArgs {
    double g[11];
    FrameSrc a, b;
    double* partial;       // [planes][blocks_per_plane]
    int H, W, crop, oh, ow, tiles_x, blocks_per_plane;
};

template <bool Y>
__device__ __forceinline__ float ssim_value(const FrameSrc& s, long frame, int ch, long hw, long pix, const double* lt) {
    if (s.fmt == PNP_FRAMES_U8_HWC) {
        const unsigned char* q = static_cast<const unsigned char*>(s.p) + (frame * hw + pix) * 3;
        if (!Y) return (float)q[ch];
        return luma_of(lt, (unsigned)q[0] | ((unsigned)q[1] << 8) | ((unsigned)q[2] << 16));
    }
    const float* f = static_cast<const float*>(s.p) + frame * 3 * hw + pix;
    if (!Y) return (float)to_u8(f[ch * hw]);
    return luma_of(lt, px_of_f32(f[0], f[hw], f[2 * hw]));
}

template <bool Y>
__global__ __launch_bounds__(256) void ssim_io_kernel(const SsimIoArgs s) {
    __shared__ float ta[26 * 42], tb[26 * 42];
    __shared__ double hm[5][26 * 32];
    __shared__ double red[4];
    __shared__ double lt[Y ? 768 : 1];
    if (Y) stage_luma_table(lt);
    const int plane = blockIdx.y, blk = blockIdx.x, t = threadIdx.x;
    const int ty0 = (blk / s.tiles_x) * 16, tx0 = (blk % s.tiles_x) * 32;        // in valid-map coordinates
    const long frame = Y ? plane : plane / 3, hw = (long)s.H * s.W;
    const int ch = Y ? 0 : plane % 3;
    for (int i = t; i < 26 * 42; i += 256) {
        const int r = i / 42, c = i - r * 42;
        const int y = s.crop + ty0 + r, x = s.crop + tx0 + c;
        float va = 0.f, vb = 0.f;
        if (y < s.H - s.crop && x < s.W - s.crop) {
            va = ssim_value<Y>(s.a, frame, ch, hw, (long)y * s.W + x, lt);
            vb = ssim_value<Y>(s.b, frame, ch, hw, (long)y * s.W + x, lt);
        }
        ta[i] = va;
        tb[i] = vb;
    }
    __syncthreads();
    for (int i = t; i < 26 * 32; i += 256) {
        const int r = i >> 5, c = i & 31;
        double m1 = 0, m2 = 0, s11 = 0, s22 = 0, s12 = 0;
#pragma unroll
        for (int k = 0; k < 11; ++k) {
            const double x = ta[r * 42 + c + k], y = tb[r * 42 + c + k], gk = s.g[k];
            m1 += gk * x;
            m2 += gk * y;
            s11 += gk * x * x;
            s22 += gk * y * y;
            s12 += gk * x * y;
        }
        hm[0][i] = m1;
        hm[1][i] = m2;
        hm[2][i] = s11;
        hm[3][i] = s22;
        hm[4][i] = s12;
    }
    __syncthreads();
    const double C1 = (0.01 * 255) * (0.01 * 255), C2 = (0.03 * 255) * (0.03 * 255);
    double acc = 0;
    for (int i = t; i < 16 * 32; i += 256) {
        const int r = i >> 5, c = i & 31;
        if (ty0 + r >= s.oh || tx0 + c >= s.ow) continue;
        double v[5] = {0, 0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < 11; ++k)
#pragma unroll
            for (int q = 0; q < 5; ++q) v[q] += s.g[k] * hm[q][(r + k) * 32 + c];
        const double mu1 = v[0], mu2 = v[1];
        const double sg1 = v[2] - mu1 * mu1, sg2 = v[3] - mu2 * mu2, sg12 = v[4] - mu1 * mu2;
        acc += ((2 * mu1 * mu2 + C1) * (2 * sg12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (sg1 + sg2 + C2));
    }
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((t & 63) == 0) red[t >> 6] = acc;
    __syncthreads();
    if (t == 0) s.partial[(long)plane * s.blocks_per_plane + blk] = red[0] + red[1] + red[2] + red[3];
}

// blocks per frame of the pixel-group kernels: about four groups (16 pixels) a thread, so that staging the table is paid seldom
int pixel_group_blocks(long groups) {
    long bx = (groups + 1023) / 1024;
    return (int)(bx < 1 ? 1 : (bx > 512 ? 512 : bx));
}

}  // namespace

extern "C" int pnp_psnr_luma_blocks(int h, int w, int crop_border) {
    if (h < 1 || w < 1 || crop_border < 0 || 2 * crop_border >= h || 2 * crop_border >= w) return 0;
    return pixel_group_blocks(PixelRuns(h, w, crop_border).groups);
}

extern "C" int pnp_psnr_stat_io(const void* a, int a_format, const void* b, int b_format, int color, void* stat, int frames, int c,
                                int h, int w, int crop_border, void* stream) {
    if (!io_args_ok(a, a_format, b, b_format, color, stat, frames, c, h, w, crop_border)) return PNP_ERR_BAD_ARG;
    if (a_format == PNP_FRAMES_F32_NCHW && b_format == PNP_FRAMES_F32_NCHW && color == PNP_COLOR_NONE)
        return pnp_psnr_sse_f32(static_cast<const float*>(a), static_cast<const float*>(b), static_cast<unsigned long long*>(stat), frames, c,
                                h, w, crop_border, stream);
    hipStream_t st = (hipStream_t)stream;
    PsnrIoArgs s = {frame_src(a, a_format, frames, h, w), frame_src(b, b_format, frames, h, w), PixelRuns(h, w, crop_border), nullptr, nullptr};
    const int bx = pixel_group_blocks(s.runs.groups);
    if (color == PNP_COLOR_Y) {
        s.partial = static_cast<double*>(stat);
        hipLaunchKernelGGL((psnr_io_kernel<true>), dim3(bx, frames), dim3(256), 0, st, s);
    } else {
        s.sse = static_cast<unsigned long long*>(stat);
        const int ze = launch_zero_words(s.sse, 2L * frames, st);
        if (ze != PNP_OK) return ze;
        hipLaunchKernelGGL((psnr_io_kernel<false>), dim3(bx, frames), dim3(256), 0, st, s);
    }
    return (int)hipGetLastError();
}

extern "C" int pnp_ssim_partials_io(const void* a, int a_format, const void* b, int b_format, int color, double* partials, int frames,
                                    int c, int h, int w, int crop_border, void* stream) {
    if (!io_args_ok(a, a_format, b, b_format, color, partials, frames, c, h, w, crop_border)) return PNP_ERR_BAD_ARG;
    const int nb = pnp_ssim_blocks(h, w, crop_border);
    if (nb < 1) return PNP_ERR_BAD_ARG;
    if (a_format == PNP_FRAMES_F32_NCHW && b_format == PNP_FRAMES_F32_NCHW && color == PNP_COLOR_NONE)
        return pnp_ssim_partials_f32(static_cast<const float*>(a), static_cast<const float*>(b), partials, frames, c, h, w, crop_border, stream);
    SsimIoArgs s;
    double sum = 0;
    for (int i = 0; i < 11; ++i) {                       // cv2.getGaussianKernel(11, 1.5)
        s.g[i] = exp(-((i - 5.0) * (i - 5.0)) / (2 * 1.5 * 1.5));
        sum += s.g[i];
    }
    for (int i = 0; i < 11; ++i) s.g[i] /= sum;
    s.a = frame_src(a, a_format, frames, h, w);
    s.b = frame_src(b, b_format, frames, h, w);
    s.partial = partials;
    s.H = h;
    s.W = w;
    s.crop = crop_border;
    s.oh = h - 2 * crop_border - 10;
    s.ow = w - 2 * crop_border - 10;
    s.tiles_x = (s.ow + 31) / 32;
    s.blocks_per_plane = nb;
    if (color == PNP_COLOR_Y)
        hipLaunchKernelGGL((ssim_io_kernel<true>), dim3(nb, frames), dim3(256), 0, (hipStream_t)stream, s);
    else
        hipLaunchKernelGGL((ssim_io_kernel<false>), dim3(nb, frames * 3), dim3(256), 0, (hipStream_t)stream, s);
    return (int)hipGetLastError();
}

extern "C" int pnp_luma_from_frames(const void* frames_dev, int format, float* out, int nframes, int h, int w, void* stream) {
    if (!frames_dev || !out || !known_format(format) || nframes < 1 || h < 1 || w < 1) return PNP_ERR_BAD_ARG;
    const long hw = (long)h * w, groups = (hw + 3) / 4;
    hipLaunchKernelGGL(luma_kernel, dim3(pixel_group_blocks(groups), nframes), dim3(256), 0, (hipStream_t)stream,
                       frame_src(frames_dev, format, nframes, h, w), out, hw, groups);
    return (int)hipGetLastError();
}
