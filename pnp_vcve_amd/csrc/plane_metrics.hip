// Plane PSNR / SSIM of Y'CbCr clips (include/pnpvcve.h, pnp_psnr_sse_yuv / pnp_ssim_partials_yuv; the _yuv420 entries are those at
// PNP_YUV_FORMAT_420; a format gives the chroma planes their true rows, columns and a crop per axis): the statistics of
// metrics.hip read from the decoder's planes where they lie -- NV12 / NV21 / I420, any address and pitch, each of the two clips
// described on its own -- 1.5 B per pixel and clip, no RGB and no fp32 copy in between.  What a codec-enhancement result is scored by:
// Y, Cb and Cr on their own (and the 6:1:1 mean the host forms).  plane_load.h fetches; the statistics are metrics.hip's.
#include "ssim_tile.h"

namespace {

// sum over the four bytes of (x_j - y_j)^2; absent samples are 0 in both words
__device__ __forceinline__ unsigned sq4(unsigned x, unsigned y) {
    unsigned e = 0;
#pragma unroll
    for (int k = 0; k < 32; k += 8) {
        const int d = (int)((x >> k) & 255u) - (int)((y >> k) & 255u);
        e += (unsigned)(d * d);
    }
    return e;
}

__device__ __forceinline__ void load_chroma4(const ChromaSrc& s, long f, int row, int col, int npix, unsigned& cb, unsigned& cr) {
    unsigned o[2];
    if (s.paired) {
        pnp_plane_load4(s.c[0], f, row, col, npix, o);
        cb = s.cr_first ? o[1] : o[0];
        cr = s.cr_first ? o[0] : o[1];
    } else {
        pnp_plane_load4(s.c[0], f, row, col, npix, o);
        cb = o[0];
        pnp_plane_load4(s.c[1], f, row, col, npix, o);
        cr = o[0];
    }
}

struct PsnrYuvArgs {
    PnpPlaneSrc ay, by;
    ChromaSrc ac, bc;
    PnpPlaneRuns ry, rc;            // the cropped Y plane; the cropped chroma planes (one group = four Cb and four Cr samples)
    unsigned long long* sse;        // (frames, 3), zeroed by the launcher
};

// The exact integer SSE of the three planes in ONE launch.  A block is 64 x 4 threads: a wave walks the groups of one row (64 groups =
// 256 contiguous bytes a step), the block's four waves and the grid's x walk the rows -- first the Y plane's, then the chroma planes'
// -- so a wave never diverges and nothing is divided.  Integer sums and one integer atomic per block and plane: psnr_sse_kernel's
// scheme, order-independent and deterministic.
__global__ __launch_bounds__(256) void psnr_yuv420_kernel(const PsnrYuvArgs s) {
    const long frame = blockIdx.y;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    unsigned long long acc[3] = {0, 0, 0};
    const int total = s.ry.rows + s.rc.rows;
    for (int r = blockIdx.x * 4 + ty; r < total; r += gridDim.x * 4) {
        int row, col, npix;
        if (r < s.ry.rows) {
#pragma unroll 4
            for (int gx = tx; gx < s.ry.gpr; gx += 64) {
                pnp_plane_group(s.ry, r, gx, row, col, npix);
                unsigned a[2], b[2];
                pnp_plane_load4(s.ay, frame, row, col, npix, a);
                pnp_plane_load4(s.by, frame, row, col, npix, b);
                acc[0] += sq4(a[0], b[0]);
            }
        } else {
#pragma unroll 2
            for (int gx = tx; gx < s.rc.gpr; gx += 64) {
                pnp_plane_group(s.rc, r - s.ry.rows, gx, row, col, npix);
                unsigned acb, acr, bcb, bcr;
                load_chroma4(s.ac, frame, row, col, npix, acb, acr);
                load_chroma4(s.bc, frame, row, col, npix, bcb, bcr);
                acc[1] += sq4(acb, bcb);
                acc[2] += sq4(acr, bcr);
            }
        }
    }
    // the block's three sums (metric_src.h::block_sums), then one atomic per block and plane
    __shared__ unsigned long long red[4][3];
    const unsigned long long v = block_sums(acc, red);
    if (threadIdx.x < 3 && v) atomicAdd(&s.sse[frame * 3 + threadIdx.x], v);
}

// ssim_kernel (metrics.hip) with the plane loader in front: the tile body is ssim_tile.h's, as it is ssim_kernel's, so a plane gives the
// partials of its (frames,1,rows,cols) fp32 plane byte / 255.0f bit for bit (to_u8 of that value is the byte).  One launch serves
// every plane of the mask: blocks [blk0, blk0 + blocks) of the grid's x are plane k's.
struct SsimPlane {
    PlaneSamp a, b;         // the plane of the two clips (clip_planes)
    int H, W, cropy, cropx, oh, ow, tiles_x, blocks, blk0;      // (a crop per axis: 4:2:2 chroma is cropped by c down, c / 2 across)
    long out0;              // first partial of this plane
};
struct SsimYuvArgs {
    double g[11];
    SsimPlane pl[3];
    int nplanes;
    double* partial;
    double L;               // the 16-bit sample path's peak 2^d - 1 (the 8-bit path's is the constant 255)
};

// S16: the samples are the values of 16-bit words (Plane16), fetched one by one; otherwise bytes through the plane loader.  Only the
// tile fill and the peak differ.
template <bool S16>
__global__ __launch_bounds__(256) void ssim_yuv420_kernel(const SsimYuvArgs s) {
    __shared__ float ta[SSIM_TILE], tb[SSIM_TILE];
    __shared__ double hm[5][SSIM_HM];
    __shared__ double red[4][1];
    SsimPlane p = s.pl[0];
    if (s.nplanes > 1 && (int)blockIdx.x >= s.pl[1].blk0) p = s.pl[1];
    if (s.nplanes > 2 && (int)blockIdx.x >= s.pl[2].blk0) p = s.pl[2];
    const int blk = blockIdx.x - p.blk0;
    const long frame = blockIdx.y;
    const int ty0 = (blk / p.tiles_x) * SSIM_OUT_R, tx0 = (blk % p.tiles_x) * SSIM_OUT_C;        // in valid-map coordinates
    if (S16) ssim_fill_plane16(ta, tb, p.a, p.b, frame, p.H, p.W, p.cropy, p.cropx, ty0, tx0);
    else ssim_fill_plane8(ta, tb, p.a, p.b, frame, p.H, p.W, p.cropy, p.cropx, ty0, tx0);
    __syncthreads();
    ssim_rows_pass(ta, tb, hm, s.g);
    __syncthreads();
    const SsimConsts k(S16 ? s.L : 255.0);
    double acc[1] = {0};
    ssim_cols_pass(hm, s.g, ty0, tx0, p.oh, p.ow,
                   [&](double mu1, double mu2, double sg1, double sg2, double sg12) { acc[0] += ssim_index(k, mu1, mu2, sg1, sg2, sg12); });
    ssim_block_sums(acc, red, s.partial + p.out0 + frame * p.blocks + blk);
}

// The exact integer SSE of the three planes of two 16-bit clips in one launch: psnr_yuv420_kernel's walk (a wave a row, first the Y
// plane's rows, then the chroma planes') with one 2-byte load per sample.  A squared difference reaches 2^24: 64-bit sums throughout.
struct Psnr16Args {
    Plane16 a[3], b[3];
    int crop, ccy, ccx, ry, wy, rc, wc;     // crop of the Y plane; of the chroma planes down and across; rows and columns of the cropped planes
    unsigned long long* sse;        // (frames, 3), zeroed by the launcher
};
__global__ __launch_bounds__(256) void psnr_yuv420p16_kernel(const Psnr16Args s) {
    const long frame = blockIdx.y;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    unsigned long long acc[3] = {0, 0, 0};
    const int total = s.ry + s.rc;
    for (int r = blockIdx.x * 4 + ty; r < total; r += gridDim.x * 4) {
        if (r < s.ry) {
            for (int x = tx; x < s.wy; x += 64) {
                const long d = (long)load16(s.a[0], frame, s.crop + r, s.crop + x) - (long)load16(s.b[0], frame, s.crop + r, s.crop + x);
                acc[0] += (unsigned long long)(d * d);
            }
        } else {
            const int row = s.ccy + r - s.ry;
            for (int x = tx; x < s.wc; x += 64) {
                const long db = (long)load16(s.a[1], frame, row, s.ccx + x) - (long)load16(s.b[1], frame, row, s.ccx + x);
                const long dr = (long)load16(s.a[2], frame, row, s.ccx + x) - (long)load16(s.b[2], frame, row, s.ccx + x);
                acc[1] += (unsigned long long)(db * db);
                acc[2] += (unsigned long long)(dr * dr);
            }
        }
    }
    __shared__ unsigned long long red[4][3];
    const unsigned long long v = block_sums(acc, red);
    if (threadIdx.x < 3 && v) atomicAdd(&s.sse[frame * 3 + threadIdx.x], v);
}

}  // namespace

namespace {

// the planes of the mask, in the order Y, Cb, Cr, laid out in one grid and one partials array, and the window; a, b: the two clips'
// planes (clip_planes); false: a cropped plane below 11x11
bool ssim_planes(SsimYuvArgs& s, const PlaneSamp (&a)[3], const PlaneSamp (&b)[3], int plane_mask, int frames, int h, int w, int crop, int format,
                 int& blk0) {
    s.nplanes = 0;
    blk0 = 0;
    long out0 = 0;
    for (int k = 0; k < 3; ++k) {
        const int bit = 1 << k;
        if (!(plane_mask & bit)) continue;
        const int nb = pnp_ssim_blocks_yuv(h, w, crop, bit, format);
        if (nb < 1) return false;
        SsimPlane& p = s.pl[s.nplanes++];
        p.a = a[k], p.b = b[k];
        const PlaneGeom g = plane_geom(h, w, crop, bit, format);
        p.H = g.H, p.W = g.W, p.cropy = g.cropy, p.cropx = g.cropx;
        p.oh = p.H - 2 * p.cropy - 10;
        p.ow = p.W - 2 * p.cropx - 10;
        p.tiles_x = (p.ow + 31) / 32;
        p.blocks = nb;
        p.blk0 = blk0;
        p.out0 = out0;
        blk0 += nb;
        out0 += (long)frames * nb;
    }
    for (int k = s.nplanes; k < 3; ++k) s.pl[k] = s.pl[0];
    ssim_window(s.g);
    return true;
}

}  // namespace

extern "C" int pnp_psnr_sse_yuv(const pnp_yuv420_planes* a, const pnp_yuv420_planes* b, unsigned long long* sse, int frames, int h, int w,
                                int crop_border, int chroma_format, void* stream) {
    if (!yuv_format_ok(chroma_format) || !planes_args_ok(a, b, sse, frames, h, w, crop_border, chroma_format)) return PNP_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    const int ze = launch_zero_words(sse, 2L * 3 * frames, st);      // a kernel, not a memset node (prep.h)
    if (ze != PNP_OK) return ze;
    PsnrYuvArgs s;
    s.ay = luma_src(*a, h, w);
    s.by = luma_src(*b, h, w);
    s.ac = chroma_src(*a, h, w, chroma_format);
    s.bc = chroma_src(*b, h, w, chroma_format);
    s.ry = pnp_plane_runs(h, w, crop_border);
    const PlaneGeom g = plane_geom(h, w, crop_border, PNP_PLANE_CB, chroma_format);
    s.rc = pnp_plane_runs(g.H, g.W, g.cropy, g.cropx);
    s.sse = sse;
    int bx = (s.ry.rows + s.rc.rows + 3) / 4;                        // a row a wave, up to 4096 rows in flight per frame
    bx = bx > 1024 ? 1024 : bx;
    hipLaunchKernelGGL(psnr_yuv420_kernel, dim3(bx, frames), dim3(256), 0, st, s);
    return (int)hipGetLastError();
}

extern "C" int pnp_psnr_sse_yuv420(const pnp_yuv420_planes* a, const pnp_yuv420_planes* b, unsigned long long* sse, int frames, int h,
                                   int w, int crop_border, void* stream) {
    return pnp_psnr_sse_yuv(a, b, sse, frames, h, w, crop_border, PNP_YUV_FORMAT_420, stream);
}

extern "C" int pnp_ssim_blocks_yuv(int h, int w, int crop_border, int plane, int chroma_format) {
    if (!yuv_frame_ok(chroma_format, 1, h, w) || crop_border < 0 || (yuv_sx(chroma_format) == 2 && (crop_border & 1))) return 0;
    if (plane != PNP_PLANE_Y && plane != PNP_PLANE_CB && plane != PNP_PLANE_CR) return 0;
    const PlaneGeom g = plane_geom(h, w, crop_border, plane, chroma_format);
    return pnp_ssim_blocks(g.H - 2 * g.cropy, g.W - 2 * g.cropx, 0);      // (pnp_ssim_blocks(rows, cols, crop) where the crops are equal)
}

extern "C" int pnp_ssim_blocks_yuv420(int h, int w, int crop_border, int plane) {
    return pnp_ssim_blocks_yuv(h, w, crop_border, plane, PNP_YUV_FORMAT_420);
}

extern "C" int pnp_ssim_partials_yuv(const pnp_yuv420_planes* a, const pnp_yuv420_planes* b, int plane_mask, double* partials, int frames,
                                     int h, int w, int crop_border, int chroma_format, void* stream) {
    if (!yuv_format_ok(chroma_format) || !planes_args_ok(a, b, partials, frames, h, w, crop_border, chroma_format) || !plane_mask_ok(plane_mask))
        return PNP_ERR_BAD_ARG;
    SsimYuvArgs s;
    s.partial = partials;
    s.L = 255.0;
    PlaneSamp pa[3], pb[3];
    clip_planes(*a, h, w, chroma_format, pa);
    clip_planes(*b, h, w, chroma_format, pb);
    int blk0 = 0;
    if (!ssim_planes(s, pa, pb, plane_mask, frames, h, w, crop_border, chroma_format, blk0)) return PNP_ERR_BAD_ARG;      // a cropped plane of the mask below 11x11
    hipLaunchKernelGGL(ssim_yuv420_kernel<false>, dim3(blk0, frames), dim3(256), 0, (hipStream_t)stream, s);
    return (int)hipGetLastError();
}

extern "C" int pnp_ssim_partials_yuv420(const pnp_yuv420_planes* a, const pnp_yuv420_planes* b, int plane_mask, double* partials,
                                        int frames, int h, int w, int crop_border, void* stream) {
    return pnp_ssim_partials_yuv(a, b, plane_mask, partials, frames, h, w, crop_border, PNP_YUV_FORMAT_420, stream);
}

extern "C" int pnp_psnr_sse_yuvp16(const pnp_yuv420_planes16* a, const pnp_yuv420_planes16* b, unsigned long long* sse, int frames, int h,
                                   int w, int crop_border, int chroma_format, void* stream) {
    if (!yuv_format_ok(chroma_format) || !planes16_args_ok(a, b, sse, frames, h, w, crop_border, chroma_format)) return PNP_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    const int ze = launch_zero_words(sse, 2L * 3 * frames, st);      // a kernel, not a memset node (prep.h)
    if (ze != PNP_OK) return ze;
    Psnr16Args s;
    for (int k = 0; k < 3; ++k) s.a[k] = plane16(*a, k), s.b[k] = plane16(*b, k);
    const PlaneGeom g = plane_geom(h, w, crop_border, PNP_PLANE_CB, chroma_format);
    s.crop = crop_border, s.ccy = g.cropy, s.ccx = g.cropx;
    s.ry = h - 2 * crop_border, s.wy = w - 2 * crop_border;
    s.rc = g.H - 2 * g.cropy, s.wc = g.W - 2 * g.cropx;
    s.sse = sse;
    int bx = (s.ry + s.rc + 3) / 4;
    bx = bx > 1024 ? 1024 : bx;
    hipLaunchKernelGGL(psnr_yuv420p16_kernel, dim3(bx, frames), dim3(256), 0, st, s);
    return (int)hipGetLastError();
}

extern "C" int pnp_psnr_sse_yuv420p16(const pnp_yuv420_planes16* a, const pnp_yuv420_planes16* b, unsigned long long* sse, int frames, int h,
                                      int w, int crop_border, void* stream) {
    return pnp_psnr_sse_yuvp16(a, b, sse, frames, h, w, crop_border, PNP_YUV_FORMAT_420, stream);
}

extern "C" int pnp_ssim_partials_yuvp16(const pnp_yuv420_planes16* a, const pnp_yuv420_planes16* b, int plane_mask, double* partials,
                                        int frames, int h, int w, int crop_border, int chroma_format, void* stream) {
    if (!yuv_format_ok(chroma_format) || !planes16_args_ok(a, b, partials, frames, h, w, crop_border, chroma_format) || !plane_mask_ok(plane_mask))
        return PNP_ERR_BAD_ARG;
    SsimYuvArgs s;
    s.partial = partials;
    s.L = (double)((1 << a->bit_depth) - 1);
    PlaneSamp pa[3], pb[3];
    clip_planes(*a, pa);
    clip_planes(*b, pb);
    int blk0 = 0;
    if (!ssim_planes(s, pa, pb, plane_mask, frames, h, w, crop_border, chroma_format, blk0)) return PNP_ERR_BAD_ARG;      // a cropped plane of the mask below 11x11
    hipLaunchKernelGGL(ssim_yuv420_kernel<true>, dim3(blk0, frames), dim3(256), 0, (hipStream_t)stream, s);
    return (int)hipGetLastError();
}

extern "C" int pnp_ssim_partials_yuv420p16(const pnp_yuv420_planes16* a, const pnp_yuv420_planes16* b, int plane_mask, double* partials,
                                           int frames, int h, int w, int crop_border, void* stream) {
    return pnp_ssim_partials_yuvp16(a, b, plane_mask, partials, frames, h, w, crop_border, PNP_YUV_FORMAT_420, stream);
}
