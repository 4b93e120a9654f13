// Multi-scale SSIM on the device (include/pnpvcve.h, pnp_msssim_*: the ONE statement of the definition): Wang, Simoncelli and Bovik
// 2003, five scales, per plane, on every boundary SSIM is computed on -- fp32 planes, uint8 RGB frames, the reference's Y, 8-bit and
// 10 / 12-bit 4:2:0 planes.  The definition is this project's own: the reference has no MS-SSIM and no external tool was at hand to
// compare digits with; it is pinned by two restatements (pnp_vcve_amd/metrics.py::msssim, tests/msssim_ref.py).
//
// Two kernels.  msssim_down_kernel makes level s + 1 of BOTH clips from level s: at s = 0 it reads through the boundary's loaders
// (metric_src.h, plane_load.h), from s = 1 on it reads the fp32 pyramid; a thread makes two neighbouring output samples of one row
// from a group of four input samples on two rows, whole samples only, so nothing is divided or accumulated across threads.
// msssim_level_kernel runs the SSIM tile body of ssim_tile.h, as ssim_kernel (metrics.hip) does -- a 16 x 32 tile of the valid map per
// block, two 26 x 42 input tiles in LDS, a horizontal pass that leaves five windowed moments of 26 x 32 positions in LDS, a vertical
// pass -- and closes it with cs = (2 s_ab + C2) / (s_a^2 + s_b^2 + C2) and l * cs, the block's TWO partial sums.  ONE launch covers every level of
// every plane: a plane's blocks are the concatenation of its levels' blocks (msssim_plan.h), the planes of a mask follow each
// other along the grid's x, so the 1 x 1 valid map of level 4 costs one block and no empty tile is launched.  Four launches of
// the first kernel and one of the second per call; the host adds a level's partials in index order (deterministic).
// The library owns no device memory: the pyramid (levels 1..4 of both clips, fp32) lives in the caller's workspace.
#include "ssim_tile.h"
#include "msssim_plan.h"

namespace {

enum { K_RGB = 0, K_Y = 1, K_P8 = 2, K_P16 = 3, K_LEVEL = 4 };      // what a kernel instance reads at level 0 (K_LEVEL: the pyramid only)

// Planes of one size and source: the channels of RGB frames, the Y of frames, or one plane of a 4:2:0 mask.  A `unit` (the grid's y)
// is one plane of one frame: frame * planes + channel (K_RGB), the frame otherwise.
struct MsClass {
    int plane;              // K_P8 / K_P16: which of the clips' planes (MsArgs::a.pl, b.pl) the class is
    PnpMsPlan plan;
    int H, W, crop;         // the plane before its crop
    int blk0;               // first block of the class along the level kernel's x
    long part0;             // first double of the class among the partials
    float *wa, *wb;         // pyramid slots of unit 0 of the two clips
};

struct MsArgs {
    double g[11];
    ClipSrc a, b;           // the two clips: fs (K_RGB, K_Y) or pl (K_P8, K_P16)
    MsClass cl[3];
    int nclass;
    long slot;              // floats between two units' pyramid slots
    double* partial;        // [class][unit][level][block][2]
    double L;               // the peak
};

// v[i][j]: sample crop + 4 gx + j (j < npix = 2 | 4) of row crop + 2 r + i of the unit's level-0 plane
template <int KIND>
__device__ __forceinline__ void fetch_2x4(const ClipSrc& s, const MsClass& c, long unit, int r, int gx, int npix, const double* lt,
                                          float v[2][4]) {
    const int y0 = c.crop + 2 * r, x0 = c.crop + 4 * gx;
    const long hw = (long)c.H * c.W;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const long p0 = (long)(y0 + i) * c.W + x0;
        if (KIND == K_P16) {
            plane_load4<true>(s.pl[c.plane], unit, y0 + i, x0, npix, v[i]);
        } else if (KIND == K_Y) {
            unsigned px[4];
            load_px4(s.fs, unit, hw, p0, npix, px);
#pragma unroll
            for (int j = 0; j < 4; ++j) v[i][j] = j < npix ? luma_of(lt, px[j]) : 0.f;
        } else if (s.fs.fmt == PNP_FRAMES_U8_HWC) {                                // K_RGB, bytes: the pixel group, this unit's channel of it
            const long frame = unit / 3;
            const unsigned sh = 8u * (unsigned)(unit - frame * 3);
            unsigned px[4];
            load_px4(s.fs, frame, hw, p0, npix, px);
#pragma unroll
            for (int j = 0; j < 4; ++j) v[i][j] = (float)((px[j] >> sh) & 255u);
        } else {                                                                    // K_RGB, fp32 planes (any number of them a frame)
            float x[4];
            f32_load4(static_cast<const float*>(s.fs.p) + unit * hw + p0, npix, x);
#pragma unroll
            for (int j = 0; j < 4; ++j) v[i][j] = j < npix ? (float)to_u8(x[j]) : 0.f;
        }
    }
}

// Level `level` + 1 of both clips from level `level`; KIND: what level 0 is read from (K_LEVEL: level >= 1, the fp32 pyramid).
// grid (x: groups, y: units, z: classes)
template <int KIND>
__global__ __launch_bounds__(256) void msssim_down_kernel(const MsArgs s, const int level) {
    __shared__ double lt[KIND == K_Y ? 768 : 1];
    if (KIND == K_Y) stage_luma_table(lt);
    const MsClass& c = s.cl[blockIdx.z];                                // (read where it lies, in the kernel's argument segment)
    const long unit = blockIdx.y;
    const PnpMsLevel &src = c.plan.lv[level], &dst = c.plan.lv[level + 1];
    const int gpr = (dst.cols + 1) / 2;                                 // groups per output row: two samples each
    const long groups = (long)dst.rows * gpr;
    float* oa = c.wa + unit * s.slot + dst.ws_off;
    float* ob = c.wb + unit * s.slot + dst.ws_off;
    const float* ia = c.wa + unit * s.slot + src.ws_off;               // (used from level 1 on)
    const float* ib = c.wb + unit * s.slot + src.ws_off;
    for (long g = (long)blockIdx.x * 256 + threadIdx.x; g < groups; g += (long)gridDim.x * 256) {
        const int r = (int)(g / gpr), gx = (int)(g - (long)r * gpr);
        const int ncol = dst.cols - 2 * gx < 2 ? 1 : 2;
        float ra[2], rb[2];
        if constexpr (KIND == K_P8) {
            pnp_ms_down_plane8(s.a.pl[c.plane].p8, s.a.pl[c.plane].sel, unit, c.crop, r, gx, ncol, ra);
            pnp_ms_down_plane8(s.b.pl[c.plane].p8, s.b.pl[c.plane].sel, unit, c.crop, r, gx, ncol, rb);
        } else {
            float va[2][4], vb[2][4];
            if constexpr (KIND == K_LEVEL) {
                const long p0 = (long)(2 * r) * src.cols + 4 * gx;
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const bool in = j < 2 * ncol;
                        va[i][j] = in ? ia[p0 + (long)i * src.cols + j] : 0.f;
                        vb[i][j] = in ? ib[p0 + (long)i * src.cols + j] : 0.f;
                    }
            } else {
                fetch_2x4<KIND>(s.a, c, unit, r, gx, 2 * ncol, lt, va);
                fetch_2x4<KIND>(s.b, c, unit, r, gx, 2 * ncol, lt, vb);
            }
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                ra[j] = pnp_ms_mean4(va[0][2 * j], va[0][2 * j + 1], va[1][2 * j], va[1][2 * j + 1]);
                rb[j] = pnp_ms_mean4(vb[0][2 * j], vb[0][2 * j + 1], vb[1][2 * j], vb[1][2 * j + 1]);
            }
        }
        const long o = (long)r * dst.cols + 2 * gx;
        oa[o] = ra[0];
        ob[o] = rb[0];
        if (ncol > 1) {
            oa[o + 1] = ra[1];
            ob[o + 1] = rb[1];
        }
    }
}

// The SSIM tile body (ssim_tile.h) on one 16 x 32 tile of the valid map of one level of one unit; the block's place along x names the
// class, the level and the tile.  Level 0 is filled through the loaders of the instance's kind, levels 1..4 from the fp32 pyramid;
// the closing expression is MS-SSIM's own: cs and l by a division each, TWO sums a block.
template <int KIND>
__global__ __launch_bounds__(256) void msssim_level_kernel(const MsArgs s) {
    __shared__ float ta[SSIM_TILE], tb[SSIM_TILE];
    __shared__ double hm[5][SSIM_HM];
    __shared__ double red[4][2];
    __shared__ double lt[KIND == K_Y ? 768 : 1];
    if (KIND == K_Y) stage_luma_table(lt);
    int ci = 0;
    if (s.nclass > 1 && (int)blockIdx.x >= s.cl[1].blk0) ci = 1;
    if (s.nclass > 2 && (int)blockIdx.x >= s.cl[2].blk0) ci = 2;
    const MsClass& c = s.cl[ci];                                        // (read where it lies, in the kernel's argument segment)
    const int blk = blockIdx.x - c.blk0;
    const long unit = blockIdx.y;
    int level = 0;
#pragma unroll
    for (int k = 1; k < PNP_MSSSIM_LEVELS; ++k)
        if (blk >= c.plan.lv[k].blk0) level = k;
    const PnpMsLevel& lv = c.plan.lv[level];
    const int b = blk - lv.blk0;
    const int ty0 = (b / lv.tiles_x) * SSIM_OUT_R, tx0 = (b % lv.tiles_x) * SSIM_OUT_C;            // in valid-map coordinates
    if (level > 0) {
        ssim_fill_level(ta, tb, c.wa + unit * s.slot + lv.ws_off, c.wb + unit * s.slot + lv.ws_off, lv.rows, lv.cols, ty0, tx0);
    } else if (KIND == K_P8) {
        ssim_fill_plane8(ta, tb, s.a.pl[c.plane], s.b.pl[c.plane], unit, c.H, c.W, c.crop, c.crop, ty0, tx0);
    } else if (KIND == K_P16) {
        ssim_fill_plane16(ta, tb, s.a.pl[c.plane], s.b.pl[c.plane], unit, c.H, c.W, c.crop, c.crop, ty0, tx0);
    } else {                                                            // a unit of K_RGB is frame * 3 + channel
        const long frame = KIND == K_Y ? unit : unit / 3;
        ssim_fill_frames<KIND == K_Y>(ta, tb, s.a.fs, s.b.fs, frame, (int)(unit - frame * 3), c.H, c.W, c.crop, ty0, tx0, lt);
    }
    __syncthreads();
    ssim_rows_pass(ta, tb, hm, s.g);
    __syncthreads();
    const SsimConsts k(s.L);
    double acc[2] = {0, 0};                                             // cs, l * cs
    ssim_cols_pass(hm, s.g, ty0, tx0, lv.oh, lv.ow, [&](double mu1, double mu2, double sg1, double sg2, double sg12) {
        const double cs = (2 * sg12 + k.C2) / (sg1 + sg2 + k.C2);
        const double l = (2 * mu1 * mu2 + k.C1) / (mu1 * mu1 + mu2 * mu2 + k.C1);
        acc[0] += cs;
        acc[1] += l * cs;
    });
    ssim_block_sums(acc, red, s.partial + c.part0 + (unit * c.plan.blocks + blk) * 2);
}

// the five launches of one call: level 1 from the source, levels 2..4 from the pyramid, then every level's statistics
template <int KIND>
int launch_all(const MsArgs& s, int units, hipStream_t st) {
    int blocks = 0;
    for (int k = 0; k < s.nclass; ++k) blocks += s.cl[k].plan.blocks;
    for (int level = 0; level + 1 < PNP_MSSSIM_LEVELS; ++level) {
        long groups = 0;                                                            // of the largest class
        for (int k = 0; k < s.nclass; ++k) {
            const PnpMsLevel& d = s.cl[k].plan.lv[level + 1];
            const long g = (long)d.rows * ((d.cols + 1) / 2);
            groups = g > groups ? g : groups;
        }
        long bx = (groups + 255) / 256;
        bx = bx < 1 ? 1 : (bx > 4096 ? 4096 : bx);
        const dim3 grid((unsigned)bx, (unsigned)units, (unsigned)s.nclass);
        if (level == 0) hipLaunchKernelGGL((msssim_down_kernel<KIND>), grid, dim3(256), 0, st, s, level);
        else hipLaunchKernelGGL((msssim_down_kernel<K_LEVEL>), grid, dim3(256), 0, st, s, level);
        const int e = (int)hipGetLastError();
        if (e) return e;
    }
    hipLaunchKernelGGL((msssim_level_kernel<KIND>), dim3((unsigned)blocks, (unsigned)units), dim3(256), 0, st, s);
    return (int)hipGetLastError();
}

// the classes' places along the level kernel's x, among the partials and in the workspace: class k's slots follow class k - 1's,
// clip b's follow clip a's
void place_classes(MsArgs& s, float* ws, long units_per_class) {
    int blk0 = 0;
    long part0 = 0;
    for (int k = 0; k < s.nclass; ++k) {
        MsClass& c = s.cl[k];
        c.blk0 = blk0;
        c.part0 = part0;
        c.wa = ws + (long)k * units_per_class * s.slot;
        c.wb = ws + ((long)s.nclass + k) * units_per_class * s.slot;
        blk0 += c.plan.blocks;
        part0 += units_per_class * c.plan.blocks * 2;
    }
    for (int k = s.nclass; k < 3; ++k) s.cl[k] = s.cl[0];
}

// The classes of a plane mask over h x w 4:2:0 frames cropped by `crop` on the Y plane (the clips' planes are in s.a.pl, s.b.pl), then
// what both plane entries set and their launches
template <int KIND>
int launch_planes(MsArgs& s, int plane_mask, double* partials, void* workspace, int frames, int h, int w, int crop, double L, void* stream) {
    s.nclass = 0;
    for (int p = 0; p < 3; ++p) {
        if (!(plane_mask & (1 << p))) continue;
        MsClass& k = s.cl[s.nclass++];
        k.plane = p;
        if (p == 0) k.H = h, k.W = w, k.crop = crop;
        else k.H = h / 2, k.W = w / 2, k.crop = crop / 2;
        k.plan = pnp_ms_plan(k.H, k.W, k.crop);
        if (!k.plan.ok) return PNP_ERR_BAD_ARG;                                     // a cropped plane of the mask below 176
    }
    s.slot = pnp_ms_plan(h, w, crop).ws_floats;
    s.partial = partials;
    s.L = L;
    ssim_window(s.g);
    place_classes(s, static_cast<float*>(workspace), frames);
    return launch_all<KIND>(s, frames, (hipStream_t)stream);
}

}  // namespace

extern "C" int pnp_msssim_min_size(void) { return PNP_MSSSIM_MIN_SIZE; }

extern "C" int pnp_msssim_level_dims(int h, int w, int crop_border, int level, int* rows, int* cols) {
    const PnpMsPlan p = pnp_ms_plan(h, w, crop_border);
    if (!p.ok || level < 0 || level >= PNP_MSSSIM_LEVELS || !rows || !cols) return PNP_ERR_BAD_ARG;
    *rows = p.lv[level].rows;
    *cols = p.lv[level].cols;
    return PNP_OK;
}

extern "C" int pnp_msssim_blocks(int h, int w, int crop_border, int level) {
    const PnpMsPlan p = pnp_ms_plan(h, w, crop_border);
    if (!p.ok || level < 0 || level >= PNP_MSSSIM_LEVELS) return 0;
    return p.lv[level].blocks;
}

extern "C" int64_t pnp_msssim_workspace_bytes(int frames, int planes, int h, int w, int crop_border) {
    const PnpMsPlan p = pnp_ms_plan(h, w, crop_border);
    if (!p.ok || frames < 1 || planes < 1) return 0;
    return 2 * (int64_t)frames * planes * p.ws_floats * (int64_t)sizeof(float);
}

extern "C" int pnp_msssim_partials_io(const void* a, int a_format, const void* b, int b_format, int color, double* partials,
                                      void* workspace, int frames, int c, int h, int w, int crop_border, void* stream) {
    if (!io_args_ok(a, a_format, b, b_format, color, partials, frames, c, h, w, crop_border) || !workspace) return PNP_ERR_BAD_ARG;
    MsArgs s;
    MsClass& k = s.cl[0];
    k.plan = pnp_ms_plan(h, w, crop_border);
    if (!k.plan.ok) return PNP_ERR_BAD_ARG;
    s.a = s.b = ClipSrc{};
    s.a.fs = frame_src(a, a_format, frames, h, w);
    s.b.fs = frame_src(b, b_format, frames, h, w);
    k.plane = 0;
    k.H = h, k.W = w, k.crop = crop_border;
    const int planes = color == PNP_COLOR_Y ? 1 : c;
    s.nclass = 1;
    s.slot = k.plan.ws_floats;
    s.partial = partials;
    s.L = 255.0;
    ssim_window(s.g);
    place_classes(s, static_cast<float*>(workspace), (long)frames * planes);
    if (color == PNP_COLOR_Y) return launch_all<K_Y>(s, frames, (hipStream_t)stream);
    return launch_all<K_RGB>(s, frames * planes, (hipStream_t)stream);
}

extern "C" int pnp_msssim_partials_yuv420(const pnp_yuv420_planes* a, const pnp_yuv420_planes* b, int plane_mask, double* partials,
                                          void* workspace, int frames, int h, int w, int crop_border, void* stream) {
    if (!planes_args_ok(a, b, partials, frames, h, w, crop_border) || !workspace || !plane_mask_ok(plane_mask)) return PNP_ERR_BAD_ARG;
    MsArgs s;
    s.a = s.b = ClipSrc{};
    clip_planes(*a, h, w, PNP_YUV_FORMAT_420, s.a.pl);
    clip_planes(*b, h, w, PNP_YUV_FORMAT_420, s.b.pl);
    return launch_planes<K_P8>(s, plane_mask, partials, workspace, frames, h, w, crop_border, 255.0, stream);
}

extern "C" int pnp_msssim_partials_yuv420p16(const pnp_yuv420_planes16* a, const pnp_yuv420_planes16* b, int plane_mask, double* partials,
                                             void* workspace, int frames, int h, int w, int crop_border, void* stream) {
    if (!planes16_args_ok(a, b, partials, frames, h, w, crop_border) || !workspace || !plane_mask_ok(plane_mask)) return PNP_ERR_BAD_ARG;
    MsArgs s;
    s.a = s.b = ClipSrc{};
    clip_planes(*a, s.a.pl);
    clip_planes(*b, s.b.pl);
    return launch_planes<K_P16>(s, plane_mask, partials, workspace, frames, h, w, crop_border, (double)((1 << a->bit_depth) - 1), stream);
}
