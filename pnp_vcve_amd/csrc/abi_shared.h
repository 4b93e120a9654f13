// What the two host-side units of the C ABI share: generator.hip (layout, packer, clip scheduler) and ops_abi.hip (the
// stand-alone op entry points).  Internal: not installed, not part of include/.
#pragma once
#include <cstring>

#include "../../include/pnpvcve.h"
#include "prep.h"

constexpr int64_t IMG_WIDE = 9 * 4096;   // floats: 9 chunks, 64 output channels
constexpr int64_t IMG_CHUNK = 4096;      // 1 chunk, 64 output channels
constexpr int64_t IMG_RGB = 9 * 2048;    // conv_last: 9 chunks, 32 (3 valid) output channels

// The two small kernels of generator.hip, for both units.
// dst[0 .. n) = v, n <= 64: one small block.  A KERNEL, not hipMemsetAsync, because the call can end up inside a captured graph
// (see launch_zero_words in prep.h); the split-fp16 tile queue is zeroed with it.
int launch_fill(float* dst, float v, int n, hipStream_t stream);
// dst[0 .. n_total) from src: zero-padded copy of n_valid floats | pixel-shuffle bias permutation dst[sub*64 + c] = src[c*4 + sub]
// (256 floats) | DCN offset/mask channel order of prep.h (src: the 432 reference channels)
enum { PNP_COPY_PAD = 0, PNP_COPY_PIXEL_SHUFFLE_BIAS = 1, PNP_COPY_DCN_CHANNELS = 2 };
int launch_small_copy(const float* src, float* dst, int n_valid, int n_total, int mode, hipStream_t stream);

// op-level entry points: the conv kernels address an NHWC64 fp32 map with 32-bit byte offsets
inline bool op_map_fits(int h, int w) { return h >= 1 && w >= 1 && (int64_t)h * w * 256 < ((int64_t)1 << 32); }

inline PackArgs plain_pack(const float* w, int cin_total, int ktaps, int kind, int cbase, int ntb, int n_valid, float* dst) {
    PackArgs a;
    memset(&a, 0, sizeof(a));
    a.w = w;
    a.ew = nullptr;
    a.E = 1;
    a.e_stride = 0;
    a.cin_total = cin_total;
    a.ktaps = ktaps;
    a.co_mul = 1;
    a.co_add = 0;
    a.n_valid = n_valid;
    a.co_mode = 0;
    a.cvalid = 3;
    a.kind = kind;
    a.cbase = cbase;
    a.ntb = ntb;
    a.scale = 1.f;
    a.dst = dst;
    return a;
}

// How one packed weight image is made from one tensor of the flat parameter buffer: plain_pack's arguments and the overrides in
// use.  build_layout records one per image while it lays the parameter out; pnp_generator_pack replays them.
struct WeightImage {
    int64_t src, dst;         // flat offset of the tensor, packed offset of the image
    int cin_total, ktaps, kind, cbase, ntb, n_valid;
    int group_cin = 0;        // PackArgs fields that differ from plain_pack's in some image
    float scale = 1.f;
    int cvalid = 3, co_mul = 1, co_add = 0, co_mode = 0;
    int grid_y = 1;           // images made by the one launch, dst_ystride floats apart (all from the same tensor)
    int64_t dst_ystride = 0;
    bool sum01 = false;       // the sum of the tensor's first two 64-channel input ranges from cbase on (BranchPk::in_wide01)
    int64_t wino = -1;        // packed offset of the image's Winograd image (fp32 path), -1 = none
};

// ones2: two floats 1.0 on the device, read by a sum01 image (nullptr if there is none)
inline int pack_weight_image(const WeightImage& r, const float* flat, float* packed, const float* ones2, hipStream_t st) {
    PackArgs a = plain_pack(flat + r.src, r.cin_total, r.ktaps, r.kind, r.cbase, r.ntb, r.n_valid, packed + r.dst);
    a.group_cin = r.group_cin;
    a.scale = r.scale;
    a.cvalid = r.cvalid;
    a.co_mul = r.co_mul;
    a.co_add = r.co_add;
    a.co_mode = r.co_mode;
    a.dst_ystride = r.dst_ystride;
    if (r.sum01) {       // the "expert" mechanism with weights (1, 1) over the two 64-channel input ranges
        a.ew = ones2;
        a.E = 2;
        a.e_stride = 64 * 9;
    }
    return launch_pack_weights(a, r.grid_y, st);
}

// PixelShufflePack's conv3x3 64 -> 256 (weight at flat offset src) as 4 sub-pixel images from packed offset dst on, IMG_WIDE apart
inline void pixel_shuffle_images(int64_t src, int64_t dst, WeightImage out[4]) {
    for (int sub = 0; sub < 4; ++sub) {
        out[sub] = WeightImage{src, dst + sub * IMG_WIDE, 64, 9, PACK_WIDE, 0, 2, 64};
        out[sub].co_mul = 4;      // F.pixel_shuffle(2): conv channel c*4 + (dy*2+dx) -> pixel (2y+dy, 2x+dx), channel c
        out[sub].co_add = sub;
    }
}
