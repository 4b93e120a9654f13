// The ONE statement of the SSIM tile body, behind every SSIM and MS-SSIM kernel (metrics.hip, plane_metrics.hip, msssim.hip).
// SSIM (mmedit/core/evaluation/metrics.py:266-355): an 11x11 Gaussian (sigma 1.5) 'valid' window over the samples, in fp64 like the
// reference.  One block of 256 threads = a 16 x 32 tile of the valid map of one plane: the two 26 x 42 input tiles go to LDS as fp32
// (a fill below), the horizontal pass leaves the five windowed moments of 26 x 32 positions in LDS, the vertical pass finishes them
// and hands mu1, mu2, sg1, sg2, sg12 to the caller's closing expression; the block's sums go through wave shuffles and four doubles
// of LDS per sum (metric_src.h::block_sums) to ONE partial each (deterministic; the host adds them).  Every kernel that uses the body declares
//     __shared__ float ta[SSIM_TILE], tb[SSIM_TILE];  __shared__ double hm[5][SSIM_HM];  __shared__ double red[4][N];
// The kernels agree to the bit because they run these statements; nothing here is a kernel or launches one.
#pragma once
#include "metric_src.h"

namespace {

enum {
    SSIM_TAPS = 11,
    SSIM_OUT_R = 16, SSIM_OUT_C = 32,                                       // a block's tile of the valid map
    SSIM_IN_R = SSIM_OUT_R + SSIM_TAPS - 1, SSIM_IN_C = SSIM_OUT_C + SSIM_TAPS - 1,       // 26 x 42: the samples under it
    SSIM_TILE = SSIM_IN_R * SSIM_IN_C,
    SSIM_HM = SSIM_IN_R * SSIM_OUT_C,                                       // positions the horizontal pass leaves
    SSIM_GROUPS = (SSIM_IN_C + 3) / 4                                       // a tile row = 10 groups of four and one of two
};

// ---- the tile fills: ta / tb = the samples of rows cropy + ty0 .., columns cropx + tx0 .. of an H x W plane of the two clips, 0 in
// both tiles where the cropped plane ends.  load(y, x, va, vb) fetches one sample of each clip.
template <class Load>
__device__ __forceinline__ void ssim_fill(float* ta, float* tb, int H, int W, int cropy, int cropx, int ty0, int tx0, Load load) {
    for (int i = threadIdx.x; i < SSIM_TILE; i += 256) {
        const int r = i / SSIM_IN_C, c = i - r * SSIM_IN_C;
        const int y = cropy + ty0 + r, x = cropx + tx0 + c;
        float va = 0.f, vb = 0.f;
        if (y < H - cropy && x < W - cropx) load(y, x, va, vb);
        ta[i] = va;
        tb[i] = vb;
    }
}

// fp32 planes, rounded to the byte
__device__ __forceinline__ void ssim_fill_f32(float* ta, float* tb, const float* pa, const float* pb, int H, int W, int crop, int ty0, int tx0) {
    ssim_fill(ta, tb, H, W, crop, crop, ty0, tx0, [&](int y, int x, float& va, float& vb) {
        va = (float)to_u8(pa[(long)y * W + x]);
        vb = (float)to_u8(pb[(long)y * W + x]);
    });
}

// sample `pix` (= y * W + x) of channel `ch` of frame `frame` of a clip of frames: the byte SSIM reads, or (Y) the fp32 luma of the
// pixel.  (fp32 planes, !Y: plane 3 * frame + ch of the clip, whatever the number of planes a frame)
template <bool Y>
__device__ __forceinline__ float ssim_frame_value(const FrameSrc& s, long frame, int ch, long hw, long pix, const double* lt) {
    if (s.fmt == PNP_FRAMES_U8_HWC) {
        const unsigned char* q = static_cast<const unsigned char*>(s.p) + (frame * hw + pix) * 3;
        if (!Y) return (float)q[ch];
        return luma_of(lt, (unsigned)q[0] | ((unsigned)q[1] << 8) | ((unsigned)q[2] << 16));
    }
    const float* f = static_cast<const float*>(s.p) + frame * 3 * hw + pix;
    if (!Y) return (float)to_u8(f[ch * hw]);
    return luma_of(lt, px_of_f32(f[0], f[hw], f[2 * hw]));
}

// frames of either format, each input on its own; lt: the staged luma table (Y)
template <bool Y>
__device__ __forceinline__ void ssim_fill_frames(float* ta, float* tb, const FrameSrc& a, const FrameSrc& b, long frame, int ch, int H, int W,
                                                 int crop, int ty0, int tx0, const double* lt) {
    const long hw = (long)H * W;
    ssim_fill(ta, tb, H, W, crop, crop, ty0, tx0, [&](int y, int x, float& va, float& vb) {
        va = ssim_frame_value<Y>(a, frame, ch, hw, (long)y * W + x, lt);
        vb = ssim_frame_value<Y>(b, frame, ch, hw, (long)y * W + x, lt);
    });
}

// 16-bit words, fetched one by one
__device__ __forceinline__ void ssim_fill_plane16(float* ta, float* tb, const PlaneSamp& a, const PlaneSamp& b, long frame, int H, int W, int cropy,
                                                  int cropx, int ty0, int tx0) {
    ssim_fill(ta, tb, H, W, cropy, cropx, ty0, tx0, [&](int y, int x, float& va, float& vb) {
        va = (float)load16(a.p16, frame, y, x);
        vb = (float)load16(b.p16, frame, y, x);
    });
}

// a level of the fp32 pyramid of MS-SSIM: rows x cols floats, no crop, the values as they are
__device__ __forceinline__ void ssim_fill_level(float* ta, float* tb, const float* pa, const float* pb, int rows, int cols, int ty0, int tx0) {
    ssim_fill(ta, tb, rows, cols, 0, 0, ty0, tx0, [&](int y, int x, float& va, float& vb) {
        va = pa[(long)y * cols + x];
        vb = pb[(long)y * cols + x];
    });
}

// 8-bit planes through the plane loader (metric_src.h::plane_load4), a group of four bytes a thread and step
__device__ __forceinline__ void ssim_fill_plane8(float* ta, float* tb, const PlaneSamp& a, const PlaneSamp& b, long frame, int H, int W, int cropy,
                                                 int cropx, int ty0, int tx0) {
    for (int i = threadIdx.x; i < SSIM_IN_R * SSIM_GROUPS; i += 256) {
        const int r = i / SSIM_GROUPS, gc = i - r * SSIM_GROUPS;
        const int y = cropy + ty0 + r, x = cropx + tx0 + 4 * gc;
        int npix = SSIM_IN_C - 4 * gc < 4 ? SSIM_IN_C - 4 * gc : 4;
        if (W - cropx - x < npix) npix = W - cropx - x;
        float va[4] = {0.f, 0.f, 0.f, 0.f}, vb[4] = {0.f, 0.f, 0.f, 0.f};
        if (y < H - cropy && npix > 0) {
            plane_load4<false>(a, frame, y, x, npix, va);
            plane_load4<false>(b, frame, y, x, npix, vb);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (4 * gc + j < SSIM_IN_C) {
                ta[r * SSIM_IN_C + 4 * gc + j] = va[j];
                tb[r * SSIM_IN_C + 4 * gc + j] = vb[j];
            }
        }
    }
}

// ---- the two passes.  g: the window (metric_src.h::ssim_window), read where it lies in the kernel's argument segment.
__device__ __forceinline__ void ssim_rows_pass(const float* ta, const float* tb, double (*hm)[SSIM_HM], const double* g) {
    for (int i = threadIdx.x; i < SSIM_HM; i += 256) {
        const int r = i >> 5, c = i & 31;
        double m1 = 0, m2 = 0, s11 = 0, s22 = 0, s12 = 0;
#pragma unroll
        for (int k = 0; k < SSIM_TAPS; ++k) {
            const double x = ta[r * SSIM_IN_C + c + k], y = tb[r * SSIM_IN_C + c + k], gk = g[k];
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
}

// close(mu1, mu2, sg1, sg2, sg12) at every position of the block's tile inside the oh x ow valid map, a thread's positions in index
// order.  The closing expression is the metric's own: SSIM forms one quotient (ssim_index), MS-SSIM cs and l with two divisions.
template <class Close>
__device__ __forceinline__ void ssim_cols_pass(const double (*hm)[SSIM_HM], const double* g, int ty0, int tx0, int oh, int ow, Close close) {
    for (int i = threadIdx.x; i < SSIM_OUT_R * SSIM_OUT_C; i += 256) {
        const int r = i >> 5, c = i & 31;
        if (ty0 + r >= oh || tx0 + c >= ow) continue;
        double v[5] = {0, 0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < SSIM_TAPS; ++k)
#pragma unroll
            for (int q = 0; q < 5; ++q) v[q] += g[k] * hm[q][(r + k) * SSIM_OUT_C + c];
        const double mu1 = v[0], mu2 = v[1];
        const double sg1 = v[2] - mu1 * mu1, sg2 = v[3] - mu2 * mu2, sg12 = v[4] - mu1 * mu2;
        close(mu1, mu2, sg1, sg2, sg12);
    }
}

// the stabilisers of a peak L (the 8-bit kernels pass the literal 255.0: they fold when the kernel is compiled)
struct SsimConsts {
    double C1, C2;
    __device__ __forceinline__ explicit SsimConsts(double L) : C1((0.01 * L) * (0.01 * L)), C2((0.03 * L) * (0.03 * L)) {}
};

// SSIM's closing expression
__device__ __forceinline__ double ssim_index(const SsimConsts& k, double mu1, double mu2, double sg1, double sg2, double sg12) {
    return ((2 * mu1 * mu2 + k.C1) * (2 * sg12 + k.C2)) / ((mu1 * mu1 + mu2 * mu2 + k.C1) * (sg1 + sg2 + k.C2));
}

// out[n] = the block's sum of acc[n], n < N (metric_src.h::block_sums)
template <int N>
__device__ __forceinline__ void ssim_block_sums(const double (&acc)[N], double (*red)[N], double* out) {
    const double v = block_sums(acc, red);
    if ((int)threadIdx.x < N) out[threadIdx.x] = v;
}

}  // namespace
