// On-device PSNR statistic (the step right after the hot path).
//
// Reference: BasicVSR.evaluate (mmedit/models/restorers/basicvsr.py:119-153) moves every frame
// to the host, tensor2img (mmedit/core/misc.py:51-71: clamp to [0,1], *255, round -> uint8) and
// psnr (mmedit/core/evaluation/metrics.py:200-215: mean squared uint8 difference).
// Here: one pass over the two frames in HBM, rounding exactly as numpy does (half to even), the
// squared differences summed as 64-bit INTEGERS (exact, order-independent, deterministic), so the
// host only sees 8 bytes per frame instead of 2 x 3*H*W*4.  HBM-bound: 8 B per element.
#include "ssim_tile.h"

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
// SSIM (mmedit/core/evaluation/metrics.py:266-355): per channel, 11x11 Gaussian (sigma 1.5) 'valid' window over the uint8-rounded
// frames, in fp64 like the reference.  The reference filters with cv2.filter2D (absent here -> parity unpinned; checked against the
// numpy restatement in pnp_vcve_amd/metrics.py).  One block = a 16x32 tile of the valid map of one plane; the tile body -- LDS tiles,
// both passes, the block's sum -- is ssim_tile.h's, which every SSIM and MS-SSIM kernel runs, so a byte frame, a luma plane or a
// decoder's plane gives the partials of its fp32 planes bit for bit.  Each block writes ONE partial sum.
struct SsimArgs {
    double g[11];
    FrameSrc a, b;         // ssim_kernel: fp32 planes at a.p / b.p
    double* partial;       // [planes][blocks_per_plane]
    int H, W, crop, oh, ow, tiles_x, blocks_per_plane;
};

// what follows a kernel's tile fill: both passes, SSIM's closing expression at the 8-bit peak, the block's partial
__device__ __forceinline__ void ssim_tile_partial(const SsimArgs& s, const float* ta, const float* tb, double (*hm)[SSIM_HM], double (*red)[1],
                                                  int ty0, int tx0) {
    __syncthreads();
    ssim_rows_pass(ta, tb, hm, s.g);
    __syncthreads();
    const SsimConsts k(255.0);
    double acc[1] = {0};
    ssim_cols_pass(hm, s.g, ty0, tx0, s.oh, s.ow,
                   [&](double mu1, double mu2, double sg1, double sg2, double sg12) { acc[0] += ssim_index(k, mu1, mu2, sg1, sg2, sg12); });
    ssim_block_sums(acc, red, s.partial + (long)blockIdx.y * s.blocks_per_plane + blockIdx.x);
}

// (frames, C, H, W) fp32 planes, rounded by to_u8: a plane per y of the grid
__global__ __launch_bounds__(256) void ssim_kernel(const SsimArgs s) {
    __shared__ float ta[SSIM_TILE], tb[SSIM_TILE];
    __shared__ double hm[5][SSIM_HM];
    __shared__ double red[4][1];
    const int plane = blockIdx.y, blk = blockIdx.x;
    const int ty0 = (blk / s.tiles_x) * SSIM_OUT_R, tx0 = (blk % s.tiles_x) * SSIM_OUT_C;        // in valid-map coordinates
    ssim_fill_f32(ta, tb, static_cast<const float*>(s.a.p) + (long)plane * s.H * s.W, static_cast<const float*>(s.b.p) + (long)plane * s.H * s.W,
                  s.H, s.W, s.crop, ty0, tx0);
    ssim_tile_partial(s, ta, tb, hm, red, ty0, tx0);
}

SsimArgs ssim_args(const void* a, int a_format, const void* b, int b_format, double* partials, int frames, int h, int w, int crop, int nb) {
    SsimArgs s;
    ssim_window(s.g);
    s.a = frame_src(a, a_format, frames, h, w);
    s.b = frame_src(b, b_format, frames, h, w);
    s.partial = partials;
    s.H = h;
    s.W = w;
    s.crop = crop;
    s.oh = h - 2 * crop - 10;
    s.ow = w - 2 * crop - 10;
    s.tiles_x = (s.ow + 31) / 32;
    s.blocks_per_plane = nb;
    return s;
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
    const SsimArgs s = ssim_args(a, PNP_FRAMES_F32_NCHW, b, PNP_FRAMES_F32_NCHW, partials, frames, h, w, crop_border, nb);
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
// reference subtracts, (double)d * d (exact: 48 bits) summed in fp64 in a fixed order -- a thread's groups in index order, then
// metric_src.h::block_sums -- and ONE partial per block, which the host adds in index order.
template <bool Y>
__global__ __launch_bounds__(256) void psnr_io_kernel(const PsnrIoArgs s) {
    __shared__ double lt[Y ? 768 : 1];
    __shared__ double red[4][1];
    if (Y) stage_luma_table(lt);
    const long frame = blockIdx.y;
    unsigned long long acc = 0;
    double accd[1] = {0};
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
                accd[0] += (double)d * (double)d;
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
        const double v = block_sums(accd, red);
        if (threadIdx.x == 0) s.partial[frame * gridDim.x + blockIdx.x] = v;
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
// plane per frame, the window runs over the fp32 Y).
template <bool Y>
__global__ __launch_bounds__(256) void ssim_io_kernel(const SsimArgs s) {
    __shared__ float ta[SSIM_TILE], tb[SSIM_TILE];
    __shared__ double hm[5][SSIM_HM];
    __shared__ double red[4][1];
    __shared__ double lt[Y ? 768 : 1];
    if (Y) stage_luma_table(lt);
    const int plane = blockIdx.y, blk = blockIdx.x;
    const int ty0 = (blk / s.tiles_x) * SSIM_OUT_R, tx0 = (blk % s.tiles_x) * SSIM_OUT_C;        // in valid-map coordinates
    ssim_fill_frames<Y>(ta, tb, s.a, s.b, Y ? plane : plane / 3, Y ? 0 : plane % 3, s.H, s.W, s.crop, ty0, tx0, lt);
    ssim_tile_partial(s, ta, tb, hm, red, ty0, tx0);
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
    const SsimArgs s = ssim_args(a, a_format, b, b_format, partials, frames, h, w, crop_border, nb);
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
