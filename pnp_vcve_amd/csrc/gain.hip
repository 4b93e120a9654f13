// Enhancement gain (include/pnpvcve.h, pnp_gain_*): what the test clip a gained over the compressed input l, both measured against the
// original g.  Per frame, plane and gain cell the two squared-error sums E_a = sum (a - g)^2 and E_l = sum (l - g)^2, and -- with a
// partition map -- per frame and partition class the pixel count and the same two sums.  ONE launch reads a, l and g once each (two
// PSNR launches read g twice) and par when it is given.  Integers only on every boundary that scores bytes or d-bit samples; fp64 for
// the fp32 Y of PNP_COLOR_Y.  The values are the host's (metrics.gain_values).  gain_plan.h holds the region, the cells and the tiling;
// metric_src.h fetches the samples.
//
// A thread block owns one tile (gain_plan.h): 256 columns of one row of cells.  A wave takes every fourth row of the tile, a lane four
// samples of it, all of one cell.  A cell's sums: the lane's registers -> the cell's lanes by shuffles -> the block's four waves through
// LDS, added in wave order -> ONE plain store by the cell's only owner.  No atomic touches the grid, integer or not, and every run
// gives the same bits.  The class sums of a block leave through one integer atomic per class and sum, or (Y) as the tile's own 24
// partials, which the host adds in index order.
#include "metric_src.h"
#include "gain_plan.h"

namespace {

enum { GN_RGB, GN_Y, GN_P8, GN_P16 };

struct GnArgs {
    ClipSrc a, l, g;        // GN_RGB, GN_Y: fs; GN_P8 / GN_P16: pl
    PnpGainPlane geo[3];    // GN_P8 / GN_P16: the planes (ok = 0: not in the mask); else geo[0] is the frame of pixels
    int W;                  // GN_RGB / GN_Y: the frame's width, hw = h * w
    long hw;
    int slots;              // planes of a frame in `grid`
    const float* par;       // (frames, 3, h, w) or nullptr
    void* grid;             // [frames][slots][grows][gcols][2] uint64 (GN_Y: double), zeroed by the launcher
    void* cls;              // [frames][8][3] uint64, zeroed by the launcher; GN_Y: [frames][tiles][8][3] double
};

template <int MODE>
struct GnTraits {
    typedef unsigned T;                 // GN_RGB: R | G << 8 | B << 16; else the sample
    typedef unsigned Acc;               // a thread adds at most 32 rows x 4 samples x 3 x 255^2 < 2^25
    typedef unsigned long long Wide;
};
template <>
struct GnTraits<GN_P16> {
    typedef unsigned T;
    typedef unsigned long long Acc;     // a squared difference reaches 2^24
    typedef unsigned long long Wide;
};
template <>
struct GnTraits<GN_Y> {
    typedef float T;
    typedef double Acc;
    typedef double Wide;
};

template <int MODE>
__device__ __forceinline__ typename GnTraits<MODE>::Acc gn_err(typename GnTraits<MODE>::T x, typename GnTraits<MODE>::T y) {
    if constexpr (MODE == GN_Y) {
        const float d = x - y;                                      // one fp32 subtraction, as pnp_psnr_stat_io forms it
        return (double)d * (double)d;
    } else if constexpr (MODE == GN_RGB) {
        unsigned e = 0;
#pragma unroll
        for (int k = 0; k < 24; k += 8) {
            const int d = (int)((x >> k) & 255u) - (int)((y >> k) & 255u);
            e += (unsigned)(d * d);
        }
        return e;
    } else {
        const int d = (int)x - (int)y;
        return (typename GnTraits<MODE>::Acc)(unsigned)(d * d);
    }
}

// v[j] = sample (row, col + j) of frame f for j < n, the value of an all-zero sample for n <= j < 4 -- on the luma path the luma of a
// black pixel, the same in all three clips, so an absent sample adds 0 to both sums; 1 <= n <= 4
template <int MODE>
__device__ __forceinline__ void gn_load4(const ClipSrc& s, const GnArgs& g, const double* lt, long f, int plane, int row, int col, int n,
                                         typename GnTraits<MODE>::T v[4]) {
    if constexpr (MODE == GN_RGB || MODE == GN_Y) {
        unsigned px[4];
        load_px4(s.fs, f, g.hw, (long)row * g.W + col, n, px);      // px[j] = 0 beyond n
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if constexpr (MODE == GN_Y) v[j] = luma_of(lt, px[j]);
            else v[j] = px[j];
        }
    } else {
        plane_load4<MODE == GN_P16>(s.pl[plane], f, row, col, n, v);
    }
}

// k[j] = the 3-bit class of pixel (row, col + j) for j < n: (par0 != 0) | (par1 != 0) << 1 | (par2 != 0) << 2
__device__ __forceinline__ void gn_class4(const float* par, long f, long hw, int W, int row, int col, int n, int k[4]) {
    float v[3][4];                                                  // (the three loads first: 2 - 6 VGPRs fewer than a load and an OR per channel)
#pragma unroll
    for (int c = 0; c < 3; ++c) f32_load4(par + (f * 3 + c) * hw + (long)row * W + col, n, v[c]);
#pragma unroll
    for (int j = 0; j < 4; ++j) k[j] = (v[0][j] != 0.f ? 1 : 0) | (v[1][j] != 0.f ? 2 : 0) | (v[2][j] != 0.f ? 4 : 0);
}

// grid = (tiles of the largest plane, frames, planes); a block past its plane's tiles, or of a plane outside the mask, has nothing to do
template <int MODE, bool CLS>
__global__ __launch_bounds__(256) void gain_kernel(const GnArgs s) {
    typedef typename GnTraits<MODE>::T T;
    typedef typename GnTraits<MODE>::Acc Acc;
    typedef typename GnTraits<MODE>::Wide Wide;
    __shared__ double lt[MODE == GN_Y ? 768 : 1];
    __shared__ Wide red[4][PNP_GAIN_MAX_CELLS][2];
    __shared__ Wide redc[4][CLS ? 24 : 1];
    const int plane = blockIdx.z;
    const PnpGainPlane g = s.geo[(MODE == GN_P8 || MODE == GN_P16) ? plane : 0];
    const int ntiles = pnp_gain_tiles(g);
    if (!g.ok || (int)blockIdx.x >= ntiles) return;                 // the whole block
    if (MODE == GN_Y) stage_luma_table(lt);
    const long frame = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int ti, tx, r0, r1, j0, ncell, col, n, cell;
    pnp_gain_tile(g, (int)blockIdx.x, ti, tx, r0, r1, j0, ncell);
    pnp_gain_lane_cols(g, tx, lane, col, n, cell);
    const bool classes = CLS && plane == 0;                         // kept on the Y plane / the pixels only
    Acc ea = 0, el = 0;
    Acc cs[CLS ? 24 : 1];                                           // [class][N, E_a, E_l]
#pragma unroll
    for (int c = 0; c < (CLS ? 24 : 1); ++c) cs[c] = 0;
    if (n > 0) {
        for (int row = r0 + wave; row < r1; row += 4) {
            T va[4], vl[4], vg[4];
            gn_load4<MODE>(s.a, s, lt, frame, plane, row, col, n, va);
            gn_load4<MODE>(s.l, s, lt, frame, plane, row, col, n, vl);
            gn_load4<MODE>(s.g, s, lt, frame, plane, row, col, n, vg);
            int k[4] = {0, 0, 0, 0};
            if (classes) gn_class4(s.par, frame, (long)g.rows * g.cols, g.cols, row, col, n, k);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const Acc xa = gn_err<MODE>(va[j], vg[j]), xl = gn_err<MODE>(vl[j], vg[j]);     // absent samples: 0 in all three clips
                ea += xa;
                el += xl;
                if (CLS) {
                    const bool in = classes && j < n;
#pragma unroll
                    for (int c = 0; c < 8; ++c) {
                        const bool m = in && k[j] == c;
                        cs[3 * c] += m ? (Acc)1 : (Acc)0;
                        cs[3 * c + 1] += m ? xa : (Acc)0;
                        cs[3 * c + 2] += m ? xl : (Acc)0;
                    }
                }
            }
        }
    }
    // a cell's lanes are g.bw / 4 consecutive ones (2 .. 32, the same for the whole block): a butterfly among them, in one fixed order
    const int per = g.bw >> 2;
    Wide wa = ea, wl = el;
#pragma unroll
    for (int off = 1; off < 32; off <<= 1) {
        if (off < per) {
            wa += __shfl_xor(wa, off, 64);
            wl += __shfl_xor(wl, off, 64);
        }
    }
    if ((lane & (per - 1)) == 0) {
        red[wave][cell][0] = wa;
        red[wave][cell][1] = wl;
    }
    if (CLS && classes) wave_sums(cs, redc);                        // (block_sums' two halves around the one barrier of both reductions)
    __syncthreads();
    const int t = threadIdx.x;
    if (t < 2 * ncell) {                                            // the only writer of this cell's two sums
        const int ce = t >> 1, q = t & 1;
        const Wide v = ((red[0][ce][q] + red[1][ce][q]) + red[2][ce][q]) + red[3][ce][q];
        Wide* out = static_cast<Wide*>(s.grid);
        out[((((frame * s.slots + plane) * g.grows + ti) * g.gcols) + j0 + ce) * 2 + q] = v;
    }
    if (CLS && classes && t < 24) {
        const Wide v = waves_sum(redc, t);
        if constexpr (MODE == GN_Y) {
            static_cast<double*>(s.cls)[(frame * ntiles + blockIdx.x) * 24 + t] = v;
        } else if (v != 0) {
            atomicAdd(static_cast<unsigned long long*>(s.cls) + frame * 24 + t, (unsigned long long)v);
        }
    }
}

template <int MODE>
int launch(GnArgs& s, int frames, int planes, hipStream_t st) {
    int tiles = 0;
    for (int k = 0; k < 3; ++k)
        if (s.geo[k].ok && pnp_gain_tiles(s.geo[k]) > tiles) tiles = pnp_gain_tiles(s.geo[k]);
    const PnpGainPlane& g0 = s.geo[0].ok ? s.geo[0] : (s.geo[1].ok ? s.geo[1] : s.geo[2]);
    int ze = launch_zero_words(s.grid, 2L * 2 * frames * s.slots * g0.grows * g0.gcols, st);      // a kernel, not a memset node (prep.h)
    if (ze == PNP_OK && s.cls && MODE != GN_Y) ze = launch_zero_words(s.cls, 2L * 24 * frames, st);
    if (ze != PNP_OK) return ze;
    const dim3 grid((unsigned)tiles, (unsigned)frames, (unsigned)planes);
    if (s.par) hipLaunchKernelGGL((gain_kernel<MODE, true>), grid, dim3(256), 0, st, s);
    else hipLaunchKernelGGL((gain_kernel<MODE, false>), grid, dim3(256), 0, st, s);
    return (int)hipGetLastError();
}

// the planes of a clip of a format that the mask names (psnrb.hip has a loop of the same shape; why the two are not shared is said there)
bool plan_planes(GnArgs& s, int mask, int h, int w, int crop, int block, int format) {
    for (int k = 0; k < 3; ++k) {
        s.geo[k] = pnp_gain_plane(0, 0, 0, 0, 1, 1);
        if (!(mask & (1 << k))) continue;
        s.geo[k] = k == 0 ? pnp_gain_plane(h, w, crop, block, 1, 1) : pnp_gain_plane(h, w, crop, block, yuv_sx(format), yuv_sy(format));
        if (!s.geo[k].ok) return false;
    }
    return true;
}

// the launch of the two plane entries, their sources filled
template <int MODE>
int launch_planes(GnArgs& s, const float* par, void* grid, void* cls, int frames, void* stream) {
    s.slots = 3;
    s.par = par;
    s.grid = grid;
    s.cls = cls;
    return launch<MODE>(s, frames, 3, (hipStream_t)stream);
}

// par and the class sums come together, and classes are kept on Y
inline bool class_args_ok(const void* par, const void* cls, int mask) { return (par != nullptr) == (cls != nullptr) && (!par || (mask & PNP_PLANE_Y)); }

}  // namespace

extern "C" int pnp_gain_grid(int h, int w, int block, int* rows, int* cols) {
    if (h < 1 || w < 1 || !pnp_gain_block_ok(block) || !rows || !cols) return PNP_ERR_BAD_ARG;
    pnp_gain_grid_of(h, w, block, *rows, *cols);
    return PNP_OK;
}

extern "C" int pnp_gain_cell_count(int h, int w, int crop_border, int block, int plane, int chroma_format, int row, int col, int64_t* count) {
    if (!count || !yuv_format_ok(chroma_format) || (plane != PNP_PLANE_Y && plane != PNP_PLANE_CB && plane != PNP_PLANE_CR)) return PNP_ERR_BAD_ARG;
    const bool luma = plane == PNP_PLANE_Y;
    if (!luma && !plane_crop_ok(chroma_format, h, w, crop_border)) return PNP_ERR_BAD_ARG;
    const PnpGainPlane p = pnp_gain_plane(h, w, crop_border, block, luma ? 1 : yuv_sx(chroma_format), luma ? 1 : yuv_sy(chroma_format));
    if (!p.ok || row < 0 || row >= p.grows || col < 0 || col >= p.gcols) return PNP_ERR_BAD_ARG;
    *count = pnp_gain_cell_samples(p, row, col);
    return PNP_OK;
}

extern "C" int pnp_gain_luma_tiles(int h, int w, int crop_border, int block) {
    const PnpGainPlane p = pnp_gain_plane(h, w, crop_border, block, 1, 1);
    return p.ok ? pnp_gain_tiles(p) : 0;
}

extern "C" int pnp_gain_sums_io(const void* a, int a_format, const void* l, int l_format, const void* g, int g_format, int color,
                                const float* par, void* grid, void* cls, int frames, int c, int h, int w, int crop_border, int block,
                                void* stream) {
    if (!io_args_ok(a, a_format, g, g_format, color, grid, frames, c, h, w, crop_border) || !l || !known_format(l_format) || c != 3 ||
        !pnp_gain_block_ok(block) || !class_args_ok(par, cls, PNP_PLANE_Y))
        return PNP_ERR_BAD_ARG;
    GnArgs s = {};
    s.geo[0] = pnp_gain_plane(h, w, crop_border, block, 1, 1);
    if (!s.geo[0].ok) return PNP_ERR_BAD_ARG;
    s.geo[1] = s.geo[2] = pnp_gain_plane(0, 0, 0, 0, 1, 1);
    s.a.fs = frame_src(a, a_format, frames, h, w);
    s.l.fs = frame_src(l, l_format, frames, h, w);
    s.g.fs = frame_src(g, g_format, frames, h, w);
    s.W = w;
    s.hw = (long)h * w;
    s.slots = 1;
    s.par = par;
    s.grid = grid;
    s.cls = cls;
    hipStream_t st = (hipStream_t)stream;
    return color == PNP_COLOR_Y ? launch<GN_Y>(s, frames, 1, st) : launch<GN_RGB>(s, frames, 1, st);
}

extern "C" int pnp_gain_sums_yuv(const pnp_yuv420_planes* a, const pnp_yuv420_planes* l, const pnp_yuv420_planes* g, int plane_mask,
                                 const float* par, unsigned long long* grid, unsigned long long* cls, int frames, int h, int w,
                                 int crop_border, int block, int chroma_format, void* stream) {
    if (!yuv_format_ok(chroma_format) || !planes_args_ok(a, g, grid, frames, h, w, crop_border, chroma_format) ||
        !planes_args_ok(l, g, grid, frames, h, w, crop_border, chroma_format) || !plane_mask_ok(plane_mask) || !pnp_gain_block_ok(block) ||
        !class_args_ok(par, cls, plane_mask))
        return PNP_ERR_BAD_ARG;
    GnArgs s = {};
    if (!plan_planes(s, plane_mask, h, w, crop_border, block, chroma_format)) return PNP_ERR_BAD_ARG;
    clip_planes(*a, h, w, chroma_format, s.a.pl);
    clip_planes(*l, h, w, chroma_format, s.l.pl);
    clip_planes(*g, h, w, chroma_format, s.g.pl);
    return launch_planes<GN_P8>(s, par, grid, cls, frames, stream);
}

extern "C" int pnp_gain_sums_yuvp16(const pnp_yuv420_planes16* a, const pnp_yuv420_planes16* l, const pnp_yuv420_planes16* g, int plane_mask,
                                    const float* par, unsigned long long* grid, unsigned long long* cls, int frames, int h, int w,
                                    int crop_border, int block, int chroma_format, void* stream) {
    if (!yuv_format_ok(chroma_format) || !planes16_args_ok(a, g, grid, frames, h, w, crop_border, chroma_format) ||
        !planes16_args_ok(l, g, grid, frames, h, w, crop_border, chroma_format) || !plane_mask_ok(plane_mask) || !pnp_gain_block_ok(block) ||
        !class_args_ok(par, cls, plane_mask))
        return PNP_ERR_BAD_ARG;
    GnArgs s = {};
    if (!plan_planes(s, plane_mask, h, w, crop_border, block, chroma_format)) return PNP_ERR_BAD_ARG;
    clip_planes(*a, s.a.pl);
    clip_planes(*l, s.l.pl);
    clip_planes(*g, s.g.pl);
    return launch_planes<GN_P16>(s, par, grid, cls, frames, stream);
}
