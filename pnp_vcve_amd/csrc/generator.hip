// Host-side clip scheduler + C ABI for the BAE/CAA forward hot path.
//
// Restates generator.forward (mmedit/models/backbones/sr_backbones/iconvsr_ipb_par.py:44-149):
// CAA prediction, key-frame selection from slice types, the backward and forward recurrent
// sweeps with MV-guided alignment of the nearest key frame, and the reconstruction / x4
// heads -- as one asynchronous stream of HIP kernel launches per clip.  Design differences
// from the reference (results identical up to fp32 rounding):
//   * feature maps live pixel-major (H,W,64) in a caller-provided workspace; `cat` is never
//     materialised (the input conv reads its 2-4 sources directly);
//   * the expert mixture mm(w, W) (sr_backbone_utils.py:198-202) is hoisted from
//     16 blocks x 2 sweeps x T frames to once per distinct base-QP value per clip;
//   * the three 1x1 partition branches and the SE gain are fused into the 3x3 MFMA kernel;
//   * samples of a batch are processed one after another (they never interact);
//   * mirror-extension detection (iconvsr.py:396-410) is skipped: for this class it only
//     switches compute_flow (iconvsr_ipb.py:33-46) to an indexing that selects the same MV
//     maps (flows_backward[-i] == mvs[:, i, 0:2]), so the output does not depend on it.
#include <deque>
#include <string>
#include <vector>
#include <cstring>
#include <cstdlib>

#include "../../include/pnpvcve.h"
#include "../../include/pnpvcve_debug.h"
#include "abi_shared.h"
#include "conv_mfma.h"
#include "prep.h"
#include "warp.h"
#include "dcn.h"
#include "yuv.h"
#ifdef PNP_HOST_STUB
#include "host_stub/io_stub.h"   // recording stand-ins for the byte-frame launchers (prep.h, conv_mfma.h) of the host-only scheduler tests
#include "host_stub/yuv_stub.h"  // ... and for the 4:2:0 launchers (yuv.h)
#include "host_stub/fold_stub.h" // ... and for the fold table's launcher (conv_mfma.h)
#endif

namespace {

struct ParamInfo {
    std::string name;
    std::vector<int64_t> shape;
    int64_t offset = 0, numel = 0;
};

struct BlockPk {
    int64_t conv1_img = -1;       // packed, static conv1 (one_layer)
    int64_t conv1_bias = -1;      // flat
    int64_t conv2_img = -1;       // packed, static conv2 (blocktype 'drt_woqp': a plain nn.Conv2d too, sr_backbone_utils.py:343-344)
    int64_t conv2_bias = -1;      // flat
    int64_t w1x1 = -1;            // packed, 3 chunks + 3 chunks scaled by PNP_PAR_UNIT (split-fp16 fast path on binary partition maps)
    int dyn_conv2 = -1, dyn_conv1 = -1;
    int64_t conv1_wino = -1, conv2_wino = -1, w1x1_wino = -1;   // packed: Winograd images of the static convs / the 1x1 branches (conv_wino.hip)
};

struct BranchPk {
    int64_t in_lr = -1;           // packed, 1 chunk
    int64_t in_wide[3] = {-1, -1, -1};
    int64_t in_wide01 = -1;       // packed: in_wide[0] + in_wide[1] (align_key with an adjacent key frame: both are the
                                  // same warped tensor, conv(x, W0) + conv(x, W1) = conv(x, W0 + W1))
    int n_wide = 0;
    int64_t in_lr_wino = -1, in_wide_wino[3] = {-1, -1, -1}, in_wide01_wino = -1;   // packed: their Winograd images (conv_wino.hip, MS form)
    int64_t in_bias = -1;         // flat
    std::vector<BlockPk> blocks;
};

}  // namespace

struct ProfRec {
    hipEvent_t a, b;
    int kind;
    double work;
};

struct pnp_generator {
    pnp_generator_cfg cfg;
    int prec = PNP_PREC_F32;          // pnp_generator_set_precision
    int opt[PNP_OPT_COUNT] = {1, 1, 1, 1, 1, 1, 1, 0, 1, 1};   // pnp_generator_set_option (defaults: everything on but the chain mirrors; Winograd on large frames)
    int max_resident = 0;             // pnp_generator_set_max_resident: bound on the frame feature maps held across steps (0 = one per frame)
    // optional per-launch HIP-event timing (pnp_generator_profile*): off by default
    mutable bool prof_on = false;
    mutable std::vector<hipEvent_t> prof_pool;
    mutable size_t prof_used = 0;
    mutable std::vector<ProfRec> prof_recs;
    mutable hipEvent_t prof_last = nullptr;          // end event of the latest timed launch (ProfScope), reusable as a start
    mutable hipStream_t prof_last_stream = nullptr;
    // side streams / events for batch-level concurrency (pnp_generator_forward with a multi-context workspace)
    mutable std::vector<hipStream_t> side_streams;
    mutable std::vector<hipEvent_t> join_events;
    mutable hipEvent_t fork_event = nullptr;
    // row-band chains (pnp_generator_set_band_split): chain B's stream, one `ready` event per conv of a chain and the join event;
    // made the first time a frame qualifies
    int band_split = 1;
    int any_size = 0;                 // pnp_generator_set_any_size: frames whose height / width is no multiple of 4 run too
    mutable hipStream_t band_stream = nullptr;
    mutable std::vector<hipEvent_t> band_events;
    mutable std::deque<ConvBandSplit> band_recs;     // the split of every chained conv of the latest forward (ConvArgs::band points here: the
                                                     // recording launchers of the host-only scheduler tests read it back after the call)
    std::vector<ParamInfo> params;
    int64_t flat_floats = 0, packed_floats = 0;
    int ndyn = 0;
    int64_t dyn_w = 0, dyn_b = 0;     // flat offsets of the dynamic conv banks
    BranchPk br[2];                   // 0 backward, 1 forward
    int64_t hr_img = -1, hr_bias = -1, last_img = -1, last_bias = -1;       // last_bias packed (32)
    int64_t hr_wino = -1;                                                   // packed: Winograd image of conv_hr
    int64_t ones2 = -1;                                                     // packed: {1, 1}
    int64_t last_valu = -1;                                                 // packed: conv_last weights [9][64][4]
    int64_t up_img[2] = {-1, -1}, up_bias[2] = {-1, -1};                    // packed
    // deform = 'basic' | 'fvc' (iconvsr_mv.py:21-84): flat offsets of the aligner's parameters, packed images
    int64_t f_dcn_b = -1, f_off0_b = -1, f_off2_b = -1;
    int64_t dcn_img = -1, off0_flow_img = -1, off0_feat_img = -1, off2_img = -1, off2_bias = -1;
    int64_t p_w1 = -1, p_b1 = -1, p_w2 = -1, p_b2 = -1, p_v1 = -1, p_v2 = -1;  // flat
    // what pack() makes: every packed weight image with its flat tensor (build_layout), and the flat offsets of the few tensors
    // it copies by hand
    std::vector<WeightImage> images;
    int64_t f_last_w = -1, f_last_b = -1, f_up_b[2] = {-1, -1};

    int64_t add_param(const std::string& name, std::vector<int64_t> shape) {
        ParamInfo p;
        p.name = name;
        p.shape = shape;
        p.numel = 1;
        for (auto d : shape) p.numel *= d;
        p.offset = flat_floats;
        flat_floats += (p.numel + 3) & ~int64_t(3);   // keep every tensor 16-byte aligned
        params.push_back(p);
        return p.offset;
    }
    int64_t add_packed(int64_t n) {
        const int64_t o = packed_floats;
        packed_floats += (n + 4095) & ~int64_t(4095);   // whole chunks: the fp16 mirror is made chunk by chunk
        return o;
    }
};

namespace {

int build_layout(pnp_generator* g) {
    const auto& c = g->cfg;
    if (c.mid_channels != 64) return PNP_ERR_UNSUPPORTED;
    if (c.num_blocks < 1 || c.num_experts < 1 || c.num_experts > 64) return PNP_ERR_BAD_ARG;
    if (c.with_se && !c.with_bias) return PNP_ERR_BAD_ARG;   // reference: gamma is None -> crash
    if (c.with_bias && !c.use_base_qp) return PNP_ERR_BAD_ARG;   // iconvsr_ipb_par.py:27 assert
    if (c.deform < 0 || c.deform > 2) return PNP_ERR_BAD_ARG;
    if (c.flow_inter < 0 || c.flow_inter > 1 || c.blocktype < 0 || c.blocktype > 1) return PNP_ERR_BAD_ARG;
    if (c.num_group < 1 || c.num_group > 64 || 64 % c.num_group) return PNP_ERR_BAD_ARG;    // nn.Conv2d: channels % groups != 0 -> ValueError
    // 'drt_woqp' calls both 3x3 convs on the bare map (sr_backbone_utils.py:376-377,379,384), which a Dynamic_conv2d_se indexes with
    // 'x': it runs only with one_layer=True.  sparse_val multiplies the (64, 64/groups) 1x1 weight with 64-channel columns (:295).
    if (c.blocktype == 1 && !c.one_layer) return PNP_ERR_UNSUPPORTED;
    if (c.sparse_val && c.num_group != 1) return PNP_ERR_UNSUPPORTED;
    const int nb = c.num_blocks, E = c.num_experts;
    const int gc = 64 / c.num_group;                 // input channels per group of every conv of a block (:285-289)
    const bool woqp = c.blocktype == 1;
    const int dpb = woqp ? 0 : (c.one_layer ? 1 : 2);   // expert-mixed convs per block
    g->ndyn = 2 * nb * dpb;
    static const char* brn[2] = {"backward_resblocks", "forward_resblocks"};
    // 1) dynamic conv banks first, with uniform strides (batched expert mixing indexes them by blockIdx.y)
    g->dyn_w = g->flat_floats;
    for (int b = 0; b < 2; ++b) {
        g->br[b].blocks.resize(nb);
        for (int i = 0; i < nb; ++i) {
            const std::string p = std::string(brn[b]) + ".main." + std::to_string(i) + ".";
            if (woqp) continue;
            g->br[b].blocks[i].dyn_conv2 = (b * nb + i) * dpb;
            g->add_param(p + "conv2.weight", {E, 64, gc, 3, 3});
            if (!c.one_layer) {
                g->br[b].blocks[i].dyn_conv1 = (b * nb + i) * dpb + 1;
                g->add_param(p + "conv1.weight", {E, 64, gc, 3, 3});
            }
        }
    }
    g->dyn_b = g->flat_floats;
    for (int b = 0; b < 2; ++b)
        for (int i = 0; i < nb; ++i) {
            const std::string p = std::string(brn[b]) + ".main." + std::to_string(i) + ".";
            if (woqp) continue;
            g->add_param(p + "conv2.bias", {E, 64});
            if (!c.one_layer) g->add_param(p + "conv1.bias", {E, 64});
        }
    // 2) everything else.  A parameter that has packed images is recorded in g->images with how each one is made, here and nowhere
    // else: pnp_generator_pack replays the records.
    auto image = [&](int64_t src, int64_t dst, int cin_total, int ktaps, int kind, int cbase, int ntb = 2, int n_valid = 64) -> WeightImage& {
        g->images.push_back(WeightImage{src, dst, cin_total, ktaps, kind, cbase, ntb, n_valid});
        return g->images.back();
    };
    // grouped convs (num_group > 1) are packed as the dense conv they equal: zeros outside the diagonal blocks
    const int gcin = c.num_group > 1 ? gc : 0;
    g->p_w1 = g->add_param("BasePredictor.BaseNet.0.weight", {64, 1});
    g->p_b1 = g->add_param("BasePredictor.BaseNet.0.bias", {64});
    g->p_w2 = g->add_param("BasePredictor.BaseNet.2.weight", {E, 64});
    g->p_b2 = g->add_param("BasePredictor.BaseNet.2.bias", {E});
    if (c.with_bias) {
        if (c.with_se) {
            g->p_v1 = g->add_param("BiasePredictor.fc.0.weight", {4, 1});
            g->p_v2 = g->add_param("BiasePredictor.fc.2.weight", {64, 4});
        } else {   // Bias_Predictor: parameters exist but do not reach the drt block's output
            g->add_param("BiasePredictor.qf_embed.0.weight", {64, 1});
            g->add_param("BiasePredictor.qf_embed.0.bias", {64});
            g->add_param("BiasePredictor.to_gamma.0.weight", {64, 64});
            g->add_param("BiasePredictor.to_gamma.0.bias", {64});
            g->add_param("BiasePredictor.to_beta.0.weight", {64, 64});
            g->add_param("BiasePredictor.to_beta.0.bias", {64});
        }
    }
    for (int b = 0; b < 2; ++b) {
        BranchPk& B = g->br[b];
        B.n_wide = (b == 0) ? (c.with_cat ? 2 : 1) : (c.with_cat ? 3 : 2);
        const int cin = 3 + 64 * B.n_wide;
        const int64_t in_w = g->add_param(std::string(brn[b]) + ".input_conv.0.weight", {64, cin, 3, 3});
        B.in_bias = g->add_param(std::string(brn[b]) + ".input_conv.0.bias", {64});
        B.in_lr = g->add_packed(IMG_CHUNK);
        image(in_w, B.in_lr, cin, 9, PACK_RGB4, 0);
        for (int s = 0; s < B.n_wide; ++s) {
            B.in_wide[s] = g->add_packed(IMG_WIDE);
            image(in_w, B.in_wide[s], cin, 9, PACK_WIDE, 3 + 64 * s);
        }
        if (c.with_cat && c.align_key) {
            B.in_wide01 = g->add_packed(IMG_WIDE);
            image(in_w, B.in_wide01, cin, 9, PACK_WIDE, 3).sum01 = true;
        }
        for (int i = 0; i < nb; ++i) {
            const std::string p = std::string(brn[b]) + ".main." + std::to_string(i) + ".";
            BlockPk& K = B.blocks[i];
            if (c.one_layer) {
                const int64_t w1 = g->add_param(p + "conv1.weight", {64, gc, 3, 3});
                K.conv1_bias = g->add_param(p + "conv1.bias", {64});
                K.conv1_img = g->add_packed(IMG_WIDE);
                image(w1, K.conv1_img, 64, 9, PACK_WIDE, 0).group_cin = gcin;
            }
            if (woqp) {
                const int64_t w2 = g->add_param(p + "conv2.weight", {64, gc, 3, 3});
                K.conv2_bias = g->add_param(p + "conv2.bias", {64});
                K.conv2_img = g->add_packed(IMG_WIDE);
                image(w2, K.conv2_img, 64, 9, PACK_WIDE, 0).group_cin = gcin;
            }
            static const char* k1[3] = {"conv16x16", "conv16x8", "conv8x8"};
            int64_t w1x1[3];
            for (int j = 0; j < 3; ++j) w1x1[j] = g->add_param(p + k1[j] + ".weight", {64, gc, 1, 1});
            K.w1x1 = g->add_packed(6 * IMG_CHUNK);      // conv16x16 / conv16x8 / conv8x8, then the same three x PNP_PAR_UNIT
            for (int j = 0; j < 6; ++j) {
                WeightImage& r = image(w1x1[j % 3], K.w1x1 + j * IMG_CHUNK, 64, 1, PACK_1X1, 0);
                r.group_cin = gcin;
                if (j >= 3) r.scale = PNP_PAR_UNIT;
            }
        }
    }
    if (c.deform != 0) {
        const int64_t dcn_w = g->add_param("deform_align.weight", {64, 64, 3, 3});
        g->f_dcn_b = g->add_param("deform_align.bias", {64});
        const int64_t off0_w = g->add_param("deform_align.conv_offset.0.weight", {64, 66, 3, 3});
        g->f_off0_b = g->add_param("deform_align.conv_offset.0.bias", {64});
        const int64_t off2_w = g->add_param("deform_align.conv_offset.2.weight", {432, 64, 3, 3});
        g->f_off2_b = g->add_param("deform_align.conv_offset.2.bias", {432});
        g->dcn_img = g->add_packed(IMG_WIDE);
        g->off0_flow_img = g->add_packed(IMG_CHUNK);
        g->off0_feat_img = g->add_packed(IMG_WIDE);
        g->off2_img = g->add_packed(7 * IMG_WIDE);
        g->off2_bias = g->add_packed(448);
        image(dcn_w, g->dcn_img, 64, 9, PACK_WIDE, 0);
        // conv_offset[0] over cat([ref, flow]) (iconvsr_mv.py:33,70): the 2 flow channels are concat channels 64,65
        image(off0_w, g->off0_flow_img, 66, 9, PACK_RGB4, 64).cvalid = 2;
        image(off0_w, g->off0_feat_img, 66, 9, PACK_WIDE, 0);
        WeightImage& po = image(off2_w, g->off2_img, 64, 9, PACK_WIDE, 0);
        po.co_mode = 1;            // 7 blocks of 64 permuted output channels (432 valid)
        po.grid_y = 7;
        po.dst_ystride = IMG_WIDE;
    }
    g->ones2 = g->add_packed(64);
    const int64_t hr_w = g->add_param("conv_hr.weight", {64, 64, 3, 3});
    g->hr_bias = g->add_param("conv_hr.bias", {64});
    g->hr_img = g->add_packed(IMG_WIDE);
    image(hr_w, g->hr_img, 64, 9, PACK_WIDE, 0);
    g->f_last_w = g->add_param("conv_last.weight", {3, 64, 3, 3});
    g->f_last_b = g->add_param("conv_last.bias", {3});
    g->last_img = g->add_packed(IMG_RGB);
    image(g->f_last_w, g->last_img, 64, 9, PACK_WIDE, 0, 1, 3);
    g->last_bias = g->add_packed(32);
    g->last_valu = g->add_packed(9 * 64 * 4);
    if (c.vsr) {
        for (int u = 0; u < 2; ++u) {
            const std::string p = "upsample" + std::to_string(u + 1) + ".upsample_conv.";
            const int64_t up_w = g->add_param(p + "weight", {256, 64, 3, 3});
            g->f_up_b[u] = g->add_param(p + "bias", {256});
            g->up_img[u] = g->add_packed(4 * IMG_WIDE);
            g->up_bias[u] = g->add_packed(256);
            WeightImage sub[4];
            pixel_shuffle_images(up_w, g->up_img[u], sub);
            g->images.insert(g->images.end(), sub, sub + 4);
        }
    }
    // Winograd images of the static 64 -> 64 convs and of the 1x1 branches (PNP_OPT_WINOGRAD; conv_wino.hip).  Appended last: no
    // earlier offset moves.  The dynamic convs get theirs per frame in the workspace (their channel gain is folded in).
    auto wino_of = [&](int64_t img) {      // reserves the Winograd image of the 64 -> 64 image at packed offset img, in its record too
        for (WeightImage& r : g->images)
            if (r.dst == img) return r.wino = g->add_packed(PNP_WINO_IMG_FLOATS);
        return int64_t(-1);
    };
    for (int b = 0; b < 2; ++b) {
        BranchPk& B = g->br[b];
        B.in_lr_wino = g->add_packed(PNP_WINO_RGB_FLOATS);
        for (int s = 0; s < B.n_wide; ++s) B.in_wide_wino[s] = wino_of(B.in_wide[s]);
        if (B.in_wide01 >= 0) B.in_wide01_wino = wino_of(B.in_wide01);
    }
    for (int b = 0; b < 2; ++b)
        for (auto& K : g->br[b].blocks) {
            if (K.conv1_img >= 0) K.conv1_wino = wino_of(K.conv1_img);
            if (K.conv2_img >= 0) K.conv2_wino = wino_of(K.conv2_img);
            K.w1x1_wino = g->add_packed(PNP_WINO_PAR_FLOATS);
        }
    g->hr_wino = wino_of(g->hr_img);
    return PNP_OK;
}

__global__ void fill_kernel(float* dst, float v, int n) {
    if ((int)threadIdx.x < n) dst[threadIdx.x] = v;
}

__global__ void small_copy_kernel(const float* __restrict__ src, float* __restrict__ dst, int n_valid, int n_total,
                                  int mode) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_total) return;
    if (mode == 0) {            // zero-padded copy
        dst[i] = i < n_valid ? src[i] : 0.f;
    } else if (mode == 1) {     // pixel-shuffle bias permutation: dst[sub*64 + c] = src[c*4 + sub]
        dst[i] = src[(i & 63) * 4 + (i >> 6)];
    } else {                    // DCN offset/mask channel order (prep.h)
        const int r = pnp_dcn_ref_channel_impl(i);
        dst[i] = r >= 0 ? src[r] : 0.f;
    }
}

struct ProfScope {
    const pnp_generator* g;
    hipStream_t st;
    bool on;
    hipEvent_t b;
    ProfScope(const pnp_generator* g_, hipStream_t st_, int kind, double work) : g(g_), st(st_), on(g_->prof_on) {
        if (!on) return;
        while (g->prof_pool.size() < g->prof_used + 2) {
            hipEvent_t e;
            if (hipEventCreate(&e) != hipSuccess) {
                on = false;
                return;
            }
            g->prof_pool.push_back(e);
        }
        // Back-to-back timed launches on one stream share an event: the end of one is the start of the next (its
        // duration then includes the ~1.5 us dispatch gap in front of it).  Halves the events in the timed region.
        hipEvent_t a;
        if (g->prof_last && g->prof_last_stream == st) {
            a = g->prof_last;
        } else {
            a = g->prof_pool[g->prof_used++];
            (void)hipEventRecord(a, st);
        }
        b = g->prof_pool[g->prof_used++];
        g->prof_recs.push_back(ProfRec{a, b, kind, work});
    }
    ~ProfScope() {
        if (!on) return;
        (void)hipEventRecord(b, st);
        g->prof_last = b;
        g->prof_last_stream = st;
    }
};

// One fused-conv launch of the scheduler, spelled as a chain of named setters instead of 20 positional arguments.
struct ConvCall {
    int nsrc = 0;
    const float* src[4] = {nullptr, nullptr, nullptr, nullptr};
    int sc[4] = {0, 0, 0, 0};
    const float* w[4] = {nullptr, nullptr, nullptr, nullptr};
    const float *bias_ = nullptr, *gamma_ = nullptr, *wpar_ = nullptr, *par_ = nullptr, *residual_ = nullptr, *lr_ = nullptr;
    float* dst = nullptr;
    long lr_plane_ = 0, w_ystride_ = 0;
    int bias_ystride_ = 0, act_ = 0, H, W, mode_ = 0, cfg_, gy_ = 1, io16_ = 0;

    ConvCall(int h, int w, int cfg) : H(h), W(w), cfg_(cfg) {}
    const float* wsrc_wino_[4] = {nullptr, nullptr, nullptr, nullptr};
    // next member of the virtual concat; wino: the Winograd image of wimg (input conv on conv_wino.hip's multi-source form) or nullptr
    ConvCall& source(const float* s, int channels, const float* wimg, const float* wino = nullptr) {
        src[nsrc] = s;
        sc[nsrc] = channels;
        wsrc_wino_[nsrc] = wino;
        w[nsrc++] = wimg;
        return *this;
    }
    ConvCall& bias(const float* b, int ystride = 0) { bias_ = b; bias_ystride_ = ystride; return *this; }
    ConvCall& gamma(const float* g) { gamma_ = g; return *this; }
    const int* par_flags_ = nullptr;
    const int* par_any_ = nullptr;
    const PnpFoldRec* fold_tab_ = nullptr;
    // see ConvArgs::par_any, ConvArgs::fold_tab
    ConvCall& gate(const int* frame_any, const PnpFoldRec* fold_tab = nullptr) { par_any_ = frame_any; fold_tab_ = fold_tab; return *this; }
    ConvCall& partition(const float* w1x1, const float* par, const int* tile_flags = nullptr) {
        wpar_ = w1x1;
        par_ = par;
        par_flags_ = tile_flags;
        return *this;
    }
    ConvCall& residual(const float* r) { residual_ = r; return *this; }
    // Winograd images of the (single) source's weights and of the branch weights; nullptr = the direct kernels
    const float *wino_ = nullptr, *wino_par_ = nullptr;
    ConvCall& wino(const float* u, const float* upar = nullptr) { wino_ = u; wino_par_ = upar; return *this; }
    int units_ = 0;
    ConvCall& units(bool on) { units_ = on ? 1 : 0; return *this; }      // with wino(): one block per 8x8 quadrant unit (small frames)
    ConvCall& act(int a) { act_ = a; return *this; }                      // 0 none, 1 relu, 2 leaky-relu(0.1)
    ConvCall& to(float* d) { dst = d; return *this; }
    // out_mode of conv_mfma.h with `gy` weight images `w_ystride` floats apart (pixel shuffle: 4, DCN offsets: 7)
    ConvCall& mode(int m, int gy = 1, long w_ystride = 0) { mode_ = m; gy_ = gy; w_ystride_ = w_ystride; return *this; }
    const float* wvalu_ = nullptr;
    // conv_last: the frame to add (3 NCHW planes) and the weights in the vector-ALU kernel's layout
    ConvCall& rgb(const float* lr, long plane, const float* wvalu = nullptr) {
        lr_ = lr;
        lr_plane_ = plane;
        wvalu_ = wvalu;
        return *this;
    }
    // conv_last at a byte boundary (ConvArgs::lr_u8 / out_u8): the frame as (h,w,3) bytes instead of rgb()'s planes, the output as
    // (H,W,3) bytes next to (or, with to(nullptr), instead of) the fp32 planes
    const unsigned char* lr8_ = nullptr;
    unsigned char* out8_ = nullptr;
    ConvCall& rgb8(const unsigned char* lr8, unsigned char* out8) { lr8_ = lr8; out8_ = out8; return *this; }
    // conv_last behind a 4:2:0 clip (ConvArgs::lr_rgb0): the frame as the (h,w,4) RGB0 conv source in the workspace
    const float* lr0_ = nullptr;
    ConvCall& rgb0(const float* lr0) { lr0_ = lr0; return *this; }
    // fp16 path: 1 = the output is an fp16 map, 2 = the (single) source is one
    ConvCall& f16_map(int io16) { io16_ = io16; return *this; }
    // fp16 path with mirrors (PNP_OPT_F16_MIRRORS): the fp16 copy its producer wrote of the source added last (read INSTEAD of
    // the fp32 map), and an fp16 copy to write of this conv's fp32 output.  nullptr = none.
    const void* src16_[4] = {nullptr, nullptr, nullptr, nullptr};
    void* out16_ = nullptr;
    ConvCall& mirror16(const void* m) { src16_[nsrc - 1] = m; return *this; }
    ConvCall& also16(void* m) { out16_ = m; return *this; }
};

struct Workspace {
    float *lr4, *slots, *kw, *tmp0, *tmp1, *u1, *u2, *u3, *ew, *gamma, *mixw, *mixb, *flow4, *om, *parbin;
    float* mixh;      // PNP_PREC_F16: fp16 mirror of mixw (same element count); PNP_PREC_F16X3: its split image (twice the halfs)
    // PNP_PREC_F16 + mirrors: fp16 NHWC64 copies of the running map of a branch (x16) and of every frame's slot (slots16);
    // the MV-aligned key frame is then fp16 only and lives in kw
    uint16_t *x16, *slots16;
    int* parany;      // per frame: OR of its tile flags (ConvArgs::par_any)
    int* parflags;    // per frame, per 8x16 tile: which partition planes are nonzero there (ConvArgs::par_flags)
    PnpFoldRec* foldtab;   // PNP_PREC_F32: two fold tables (ConvArgs::fold_tab), one per branch run in flight like the image buffers of `wino`
    float* wino;      // PNP_PREC_F32: Winograd images of one branch's dynamic convs for the frame in flight (2 per block; gain folded in)
    int* queue;       // PNP_PREC_F16X3: the split kernel's tile queue (ConvArgs::tile_queue), 16 ints, zero between launches
    // byte frames on a last conv that keeps its fp32 interface (io_staged): ONE frame of fp32 planes each way, converted per frame
    float *lr1, *out1;
    int64_t bytes;
};

int64_t align_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }

// 8x16 tiles of a frame: one partition flag word each (Workspace::parflags, ConvArgs::par_flags)
int64_t par_flag_tiles(int h, int w) { return (int64_t)((w + 15) / 16) * ((h + 7) / 8); }

// Largest per-LR-pixel byte extent any kernel of the clip addresses with 32-bit offsets: a 64-channel fp32 map is
// 256 B/pixel (x16 pixels behind the x4 heads); the DCN aligners' offset/mask map is 448 channels = 1792 B/pixel.
int64_t pnp_addr32_bytes_per_lr_pixel(int vsr, int deform) {
    int64_t b = 256 * (vsr ? 16 : 1);
    if (deform != 0 && b < 1792) b = 1792;
    return b;
}

// ---- bounded-memory schedule (pnp_generator_set_max_resident)
// With a bound k on the 64-channel frame maps held across branch runs (0 < k < t), the backward sweep runs once as a checkpoint
// pass that keeps the first R frames' features (produced last, consumed first) and, at every boundary b of the segments
// [R, R+L), [R+L, R+2L), ..., [.., t), the two maps the recompute of the segment ending at b reads: B[b] (with_cat) and B[first key >= b].
// The forward sweep recomputes each segment's backward features from its checkpoint just before it consumes them.  Recomputed
// frames: t - R.  Upper bound of the maps alive at any step (c = 2 with_cat, 1 without; nC = checkpoint boundaries):
//   head of the checkpoint pass R + c*nC + 1, a segment of it c*nC + c + 1, a recomputed segment L + c + c*nC.
int plan_need(int t, int with_cat, int R, int L) {
    if (R >= t) return t;
    const int c = with_cat ? 2 : 1;
    const int nc = (t - R + L - 1) / L - 1;
    int need = c * nc + c + 1;
    if (R > 0 && R + c * nc + 1 > need) need = R + c * nc + 1;
    if (L + c + c * nc > need) need = L + c + c * nc;
    return need;
}

// the most resident frames (fewest recomputed) a bound of k maps allows: false if k is below the minimum.  k <= 0 or k >= t: R = t.
bool plan_pick(int t, int with_cat, int k, int* R, int* L) {
    if (k <= 0 || k >= t) {
        *R = t;
        *L = 0;
        return true;
    }
    for (int r = k < t - 1 ? k : t - 1; r >= 0; --r)       // plan_need >= R + 1 and >= L + 1: both stay below k
        for (int l = 1; l <= k && l <= t - r; ++l)
            if (plan_need(t, with_cat, r, l) <= k) {
                *R = r;
                *L = l;
                return true;
            }
    return false;
}

int plan_min_resident(int t, int with_cat) {
    int R, L, k = 1;
    while (!plan_pick(t, with_cat, k, &R, &L)) ++k;
    return k;
}

bool bounded_mode(const pnp_generator* g, int t) { return g->max_resident > 0 && g->max_resident < t; }

// ---- row-band chains (pnp_generator_set_band_split)
// A chain of nconv 3x3 convs c_0 .. c_(nconv-1), each reading the previous one's output, on a frame of `rows` 16-pixel tile rows, run as
// two chains with the boundary a_n = a_0 - n:  A (the caller's stream) computes tile rows [0, a_n) of c_n, B (the side stream) rows
// [a_n, rows).  A 3x3 conv's output on pixel rows [p, q) reads pixel rows [p - 1, q + 1) of its input, and its residual / partition
// planes at its own pixels.  With tile row r = pixel rows [16 r, 16 r + 16):
//   * A's c_n reads input pixel rows <= 16 a_n, i.e. tile rows <= a_n = a_(n-1) - 1 < a_(n-1): all written by A's c_(n-1).  A never waits.
//   * B's c_n reads input pixel rows >= 16 a_n - 1, i.e. tile rows >= a_n - 1: rows a_n - 1 and a_n are A's c_(n-1) (both < a_(n-1)), the
//     rest B's own c_(n-1) (rows >= a_(n-1) = a_n + 1).  So B's c_n is enqueued behind an event recorded in front of A's c_n: it then
//     follows A's c_(n-1) and all earlier ones, and B's c_(n-1) by stream order.
//   * what runs unordered against B's c_n is A's c_m for m >= n.  Writes: A's c_m writes tile rows < a_m <= a_n, B's c_n rows >= a_n:
//     disjoint, whichever buffers they are (the branch ping-pongs tmp0 -> tmp1 -> tmp0 and a back half writes over its own residual).
//     A's writes against B's reads, m > n: A writes tile rows <= a_m - 1 <= a_n - 2, B reads tile rows >= a_n - 1.  m = n: the same conv,
//     whose output is not its input.  B's writes against A's reads, m > n: A's c_m reads tile rows <= a_m <= a_n - 1, B's c_n writes
//     rows >= a_n.  m = n: A reads the input, B writes the output.
//   * B's c_n against A's c_m, m < n, is ordered by the event; the chain ends with A's stream waiting for B's.
// Both regions non-empty over the whole chain: 1 <= a_(nconv-1) and a_0 <= rows - 1.  The centred trapezoid a_0 = (rows + nconv - 1) / 2
// gives both chains the same number of tiles (+- a row); `a0` > 0 names another first boundary.
bool band_plan(int rows, int nconv, int a0, int* first) {
    if (rows < 1 || nconv < 1 || a0 < 0) return false;
    const int a = a0 > 0 ? a0 : (rows + nconv - 1) / 2;
    if (a - (nconv - 1) < 1 || a > rows - 1) return false;
    *first = a;
    return true;
}

// One branch run of the clip schedule: the backward (sweep 0) or forward (sweep 1) branch of `frame`, and where its maps live.
// out / key / nb / own: index of a 64-channel frame map in W.slots (and W.slots16); -1 = not read.  key_frame: the key frame it aligns.
struct Step {
    int sweep, frame, key_frame;
    int out, key, nb, own;      // written map; aligned key-frame map; neighbour (with_cat: B[i+1] | F[i-1]); own backward feature (forward)
};

// The clip's branch runs in launch order.  Unbounded (k = 0 or k >= t): today's schedule, frame i in slot i.  Bounded: checkpoint
// pass + recomputed segments, every map placed by a liveness scan on a free list of k slots.  Returns false if the scan ever needs
// more than k slots (plan_need is an upper bound, so this does not happen; kept as a guard against a write past the workspace).
bool make_schedule(const pnp_generator* g, int t, const std::vector<char>& key, std::vector<Step>& steps, int* recomputed) {
    const int cat = g->cfg.with_cat;
    steps.clear();
    *recomputed = 0;
    auto nk = [&](int i) { int k = i + 1; while (!key[k]) ++k; return k; };
    auto pk = [&](int i) { int k = i - 1; while (!key[k]) --k; return k; };
    if (!bounded_mode(g, t)) {
        for (int i = t - 1; i >= 0; --i)
            steps.push_back({0, i, i < t - 1 ? nk(i) : -1, i, i < t - 1 ? nk(i) : -1, (cat && i < t - 1) ? i + 1 : -1, -1});
        for (int i = 0; i < t; ++i)
            steps.push_back({1, i, i > 0 ? pk(i) : -1, i, i > 0 ? pk(i) : -1, (cat && i > 0) ? i - 1 : -1, i});
        return true;
    }
    int R, L;
    if (!plan_pick(t, cat, g->max_resident, &R, &L)) return false;
    // 1) the steps with the INSTANCE (= producing step) each one reads
    std::vector<int> bc(t, -1), br(t, -1), fw(t, -1);
    for (int i = t - 1; i >= 0; --i) {
        const int s = (int)steps.size();
        steps.push_back({0, i, i < t - 1 ? nk(i) : -1, s, i < t - 1 ? bc[nk(i)] : -1, (cat && i < t - 1) ? bc[i + 1] : -1, -1});
        bc[i] = s;
    }
    for (int i = 0; i < t; ++i) {
        if (i >= R && (i - R) % L == 0) {          // entering segment [i, b): recompute b-1 .. i from the checkpoint of b
            const int b = i + L < t ? i + L : t;
            for (int j = b - 1; j >= i; --j) {
                const int s = (int)steps.size();
                const int kj = j < t - 1 ? nk(j) : -1;
                steps.push_back({0, j, kj, s, kj < 0 ? -1 : (kj < b ? br[kj] : bc[kj]),
                                 (cat && j < t - 1) ? (j + 1 < b ? br[j + 1] : bc[b]) : -1, -1});
                br[j] = s;
                ++*recomputed;
            }
        }
        const int s = (int)steps.size();
        steps.push_back({1, i, i > 0 ? pk(i) : -1, s, i > 0 ? fw[pk(i)] : -1, (cat && i > 0) ? fw[i - 1] : -1, i < R ? bc[i] : br[i]});
        fw[i] = s;
    }
    // 2) last reader of every instance, 3) slots: a step frees what it read for the last time BEFORE its output takes a slot (every
    // read of a step -- the alignment and the input conv -- is done before its last block writes the output)
    const int ns = (int)steps.size();
    std::vector<int> last(ns);
    for (int s = 0; s < ns; ++s) {
        last[s] = s;
        for (int r : {steps[s].key, steps[s].nb, steps[s].own})
            if (r >= 0 && s > last[r]) last[r] = s;
    }
    std::vector<int> slot(ns, -1), free_slots;
    for (int k = g->max_resident - 1; k >= 0; --k) free_slots.push_back(k);
    for (int s = 0; s < ns; ++s) {
        Step& st = steps[s];
        int* rd[3] = {&st.key, &st.nb, &st.own};
        const int inst[3] = {st.key, st.nb, st.own};
        for (int j = 0; j < 3; ++j) {
            if (inst[j] < 0) continue;
            if (slot[inst[j]] < 0) return false;
            *rd[j] = slot[inst[j]];
        }
        for (int j = 0; j < 3; ++j)
            if (inst[j] >= 0 && last[inst[j]] == s && slot[inst[j]] >= 0) {
                free_slots.push_back(slot[inst[j]]);
                slot[inst[j]] = -1;       // (read twice by one step: freed once)
            }
        if (free_slots.empty()) return false;
        slot[s] = free_slots.back();
        free_slots.pop_back();
        st.out = slot[s];
        if (last[s] == s) {
            free_slots.push_back(slot[s]);
            slot[s] = -1;
        }
    }
    return true;
}

// Byte frames: conv_last's vector-ALU kernel reads and writes bytes itself (launch_conv_last_io).  The two other kernels that add the
// frame -- the fp16 path's RGB body and the matrix-core conv under PNP_OPT_CONV_LAST_VALU = 0 -- keep their fp32 interface behind a
// one-frame fp32 copy of the frame and / or of the output in the workspace.
bool io_staged(const pnp_generator* g) { return g->prec == PNP_PREC_F16 || !g->opt[PNP_OPT_CONV_LAST_VALU]; }

// 4:2:0 frames (pnp_generator_forward_clips_yuv): a frame format of the scheduler only -- the public entry for formats refuses it -- and
// one more bit of the output mask.  The unpacked frame in the workspace is what conv_last adds (ConvArgs::lr_rgb0); the kernels with an
// fp32 interface get the one-frame planes of the byte boundary.  Output planes are made per frame from the fp32 output frame: the
// caller's where PNP_OUT_F32 is asked for, the one-frame buffer otherwise.
constexpr int FRAMES_YUV420 = 2;

Workspace carve(const pnp_generator* g, char* base, int t, int h, int w, int lq_format = PNP_FRAMES_F32_NCHW, int out_mask = PNP_OUT_F32) {
    Workspace W;
    int64_t off = 0;
    const int64_t hw = (int64_t)h * w;
    auto take = [&](int64_t floats) {
        float* p = base ? reinterpret_cast<float*>(base + off) : nullptr;
        off = align_up(off + floats * 4, 256);
        return p;
    };
    // frame maps: one per frame, or the bound's k (bounded schedule); the bounded schedule also binarises a sparse_val partition map
    // per frame just before its branch runs instead of once per clip
    const bool bounded = bounded_mode(g, t);
    const int64_t nslots = bounded ? g->max_resident : t;
    W.lr4 = take(hw * 4 * t);
    W.slots = take(hw * 64 * nslots);
    W.kw = take(hw * 64);
    W.tmp0 = take(hw * 64);
    W.tmp1 = take(hw * 64);
    if (g->cfg.vsr) {
        W.u1 = take(hw * 4 * 64);
        W.u2 = take(hw * 16 * 64);
        W.u3 = take(hw * 16 * 64);
    } else {
        W.u1 = W.u2 = W.u3 = nullptr;
    }
    if (g->cfg.deform != 0) {
        W.flow4 = take(hw * 4);
        W.om = take(hw * 448);
    } else {
        W.flow4 = W.om = nullptr;
    }
    W.parbin = g->cfg.sparse_val ? take(hw * 3 * (bounded ? 1 : t)) : nullptr;
    W.ew = take((int64_t)t * g->cfg.num_experts);
    W.gamma = take((int64_t)t * 64);
    W.mixw = take((int64_t)t * g->ndyn * IMG_WIDE);
    W.mixb = take((int64_t)t * g->ndyn * 64);
    W.mixh = g->prec != PNP_PREC_F32 ? take((int64_t)t * g->ndyn * IMG_WIDE / (g->prec == PNP_PREC_F16X3 ? 1 : 2)) : nullptr;
    // (not the last region: the flags behind it are written by every forward, which is what the sanitizer harness's shrunken-workspace self-test trips over)
    W.wino = (g->prec == PNP_PREC_F32 && g->ndyn > 0) ? take((int64_t)2 * 2 * g->cfg.num_blocks * PNP_WINO_IMG_FLOATS) : nullptr;      // two buffers: run s + 1's images are made while run s reads its own
    const bool mir = g->prec == PNP_PREC_F16 && g->cfg.deform == 0;      // sized whether or not PNP_OPT_F16_MIRRORS is on
    W.x16 = mir ? reinterpret_cast<uint16_t*>(take(hw * 32)) : nullptr;
    W.slots16 = mir ? reinterpret_cast<uint16_t*>(take(hw * 32 * nslots)) : nullptr;
    // (a record is 8 bytes = two floats; sized by the frame, not by the clip: what the workspace grows by per frame stays what it was)
    W.foldtab = g->prec == PNP_PREC_F32 ? reinterpret_cast<PnpFoldRec*>(take(2 * 2 * pnp_fold_records(h, w))) : nullptr;
    W.parany = reinterpret_cast<int*>(take(t));        // (not last: the harness shrinks the workspace and expects the last region to be touched)
    W.parflags = reinterpret_cast<int*>(take(t * par_flag_tiles(h, w)));
    W.queue = g->prec == PNP_PREC_F16X3 ? reinterpret_cast<int*>(take(16)) : nullptr;
    // (behind everything else and only in the modes that need them: the fp32 boundary's layout and size are what they were)
    const bool staged = io_staged(g);
    W.lr1 = (staged && (lq_format == PNP_FRAMES_U8_HWC || lq_format == FRAMES_YUV420)) ? take(hw * 3) : nullptr;
    const bool out1 = !(out_mask & PNP_OUT_F32) && ((staged && (out_mask & PNP_OUT_U8)) || (out_mask & PNP_OUT_YUV420));
    W.out1 = out1 ? take(hw * 3 * (g->cfg.vsr ? 16 : 1)) : nullptr;
    W.bytes = off;
    return W;
}

}  // namespace

int launch_fill(float* dst, float v, int n, hipStream_t stream) {
    if (n < 0 || n > 64) return PNP_ERR_BAD_ARG;
    hipLaunchKernelGGL(fill_kernel, dim3(1), dim3(64), 0, stream, dst, v, n);
    return (int)hipGetLastError();
}

int launch_small_copy(const float* src, float* dst, int n_valid, int n_total, int mode, hipStream_t stream) {
    if (n_total < 1 || mode < PNP_COPY_PAD || mode > PNP_COPY_DCN_CHANNELS) return PNP_ERR_BAD_ARG;
    const int threads = n_total < 256 ? 64 : 256;
    hipLaunchKernelGGL(small_copy_kernel, dim3((n_total + threads - 1) / threads), dim3(threads), 0, stream, src, dst, n_valid, n_total, mode);
    return (int)hipGetLastError();
}

extern "C" {

int pnp_abi_version(void) { return 5; }

int pnp_generator_create(const pnp_generator_cfg* cfg, pnp_generator** out) {
    if (!cfg || !out) return PNP_ERR_BAD_ARG;
    pnp_generator* g = new pnp_generator();
    g->cfg = *cfg;
    if (g->cfg.num_group == 0) g->cfg.num_group = 1;      // a zeroed field is the reference's default (num_group=1)
    const int rc = build_layout(g);
    if (rc != PNP_OK) {
        delete g;
        return rc;
    }
    *out = g;
    return PNP_OK;
}

void pnp_generator_destroy(pnp_generator* g) {
    if (!g) return;
    for (hipEvent_t e : g->prof_pool) (void)hipEventDestroy(e);
    for (hipEvent_t e : g->join_events) (void)hipEventDestroy(e);
    for (hipStream_t s : g->side_streams) (void)hipStreamDestroy(s);
    if (g->fork_event) (void)hipEventDestroy(g->fork_event);
    for (hipEvent_t e : g->band_events) (void)hipEventDestroy(e);
    if (g->band_stream) (void)hipStreamDestroy(g->band_stream);
    delete g;
}

int pnp_generator_num_params(const pnp_generator* g) { return (int)g->params.size(); }
const char* pnp_generator_param_name(const pnp_generator* g, int i) { return g->params[i].name.c_str(); }
int pnp_generator_param_ndim(const pnp_generator* g, int i) { return (int)g->params[i].shape.size(); }
int64_t pnp_generator_param_dim(const pnp_generator* g, int i, int d) { return g->params[i].shape[d]; }
int64_t pnp_generator_param_offset(const pnp_generator* g, int i) { return g->params[i].offset; }
int64_t pnp_generator_flat_floats(const pnp_generator* g) { return g->flat_floats; }
// fp32 images, then (PNP_PREC_F16) their fp16 mirror: element i of the mirror region is element i of the images; or
// (PNP_PREC_F16X3) their split images: the 16 KiB at halfs 2 * i.. belong to the 64-deep chunk at float i
int64_t pnp_generator_packed_floats(const pnp_generator* g) {
    const int halves = g->prec == PNP_PREC_F16 ? 1 : (g->prec == PNP_PREC_F16X3 ? 2 : 0);
    return g->packed_floats + halves * (g->packed_floats / 2);
}

int pnp_generator_set_precision(pnp_generator* g, int precision) {
    if (!g || (precision != PNP_PREC_F32 && precision != PNP_PREC_F16 && precision != PNP_PREC_F16X3)) return PNP_ERR_BAD_ARG;
    g->prec = precision;
    return PNP_OK;
}
int pnp_generator_get_precision(const pnp_generator* g) { return g ? g->prec : -1; }

int pnp_generator_set_option(pnp_generator* g, int option, int value) {
    if (!g || option < 0 || option >= PNP_OPT_COUNT) return PNP_ERR_BAD_ARG;
    g->opt[option] = option == PNP_OPT_WINOGRAD ? (value < 0 ? 0 : (value > 2 ? 2 : value)) : (value != 0);
    return PNP_OK;
}
int pnp_generator_get_option(const pnp_generator* g, int option) {
    return (g && option >= 0 && option < PNP_OPT_COUNT) ? g->opt[option] : -1;
}

int pnp_generator_pack(const pnp_generator* g, const float* flat, float* packed, void* stream_) {
    hipStream_t st = (hipStream_t)stream_;
    const auto& c = g->cfg;
    int rc;
    // Regions are padded to whole chunks and the fp16 mirror below converts the buffer wholesale: define the padding instead of
    // asking the caller for a zeroed buffer (found by the host-only sanitizer build, tests/test_host_scheduler.py).
    {
        const hipError_t e = hipMemsetAsync(packed, 0, (size_t)g->packed_floats * sizeof(float), st);
        if (e != hipSuccess) return (int)e;
    }
    for (const WeightImage& r : g->images) {
        if (r.sum01) {       // the two "expert" weights (1, 1) its mixture reads
            rc = launch_fill(packed + g->ones2, 1.0f, 2, st);
            if (rc) return rc;
        }
        rc = pack_weight_image(r, flat, packed, packed + g->ones2, st);
        if (rc) return rc;
    }
    // what is not a weight image made by launch_pack_weights: three small bias copies and conv_last's vector-ALU layout
    if (c.deform != 0) {
        rc = launch_small_copy(flat + g->f_off2_b, packed + g->off2_bias, 432, 448, PNP_COPY_DCN_CHANNELS, st);
        if (rc) return rc;
    }
    rc = launch_small_copy(flat + g->f_last_b, packed + g->last_bias, 3, 32, PNP_COPY_PAD, st);
    if (rc) return rc;
    rc = launch_pack_last_valu(flat + g->f_last_w, packed + g->last_valu, st);
    if (rc) return rc;
    for (int u = 0; c.vsr && u < 2; ++u) {
        rc = launch_small_copy(flat + g->f_up_b[u], packed + g->up_bias[u], 256, 256, PNP_COPY_PIXEL_SHUFFLE_BIAS, st);
        if (rc) return rc;
    }
    if (g->prec == PNP_PREC_F32) {   // Winograd images (only the fp32 path has a Winograd kernel)
        for (int b = 0; b < 2; ++b) {
            const BranchPk& B = g->br[b];
            rc = launch_wino_rgb_image(packed + B.in_lr, packed + B.in_lr_wino, st);
            if (rc) return rc;
            for (const BlockPk& K : B.blocks) {
                rc = launch_wino_par_image(packed + K.w1x1, packed + K.w1x1_wino, st);
                if (rc) return rc;
            }
        }
        std::vector<const float*> ws;
        std::vector<float*> wd;
        for (const WeightImage& r : g->images)
            if (r.wino >= 0) { ws.push_back(packed + r.dst); wd.push_back(packed + r.wino); }
        for (size_t i = 0; i < ws.size(); i += 16) {
            const int n = (int)(ws.size() - i < 16 ? ws.size() - i : 16);
            rc = launch_wino_images(ws.data() + i, wd.data() + i, n, nullptr, st);
            if (rc) return rc;
        }
    }
    if (g->prec == PNP_PREC_F16) {   // every region is whole 64-output-channel chunks (the others are never read as fp16)
        rc = launch_f16_image(packed, packed + g->packed_floats, (int)(g->packed_floats / IMG_CHUNK), 2, st);
        if (rc) return rc;
        // conv_last's image has ONE 32-channel N tile per k-step: its chunks are half as long
        rc = launch_f16_image(packed + g->last_img, reinterpret_cast<uint16_t*>(packed + g->packed_floats) + g->last_img, 9, 1, st);
        if (rc) return rc;
        if (c.deform != 0) {      // the DCN contraction consumes k in the order its lanes gather it (dcn.hip)
            rc = launch_dcn_f16_image(packed + g->dcn_img, reinterpret_cast<uint16_t*>(packed + g->packed_floats) + g->dcn_img, st);
            if (rc) return rc;
        }
    }
    if (g->prec == PNP_PREC_F16X3) {     // split image of every region; only the NHWC64 64-channel convs read theirs
        rc = launch_f16x3_image(packed, packed + g->packed_floats, (int)(g->packed_floats / IMG_CHUNK), st);
        if (rc) return rc;
    }
    return (int)hipGetLastError();
}

int64_t pnp_generator_workspace_bytes(const pnp_generator* g, int t, int h, int w) {
    int R, L;
    if (bounded_mode(g, t) && !plan_pick(t, g->cfg.with_cat, g->max_resident, &R, &L)) return -1;    // bound below the minimum
    return carve(g, nullptr, t, h, w).bytes;
}

int pnp_generator_set_max_resident(pnp_generator* g, int k) {
    if (!g || k < 0) return PNP_ERR_BAD_ARG;
    g->max_resident = k;
    return PNP_OK;
}
int pnp_generator_get_max_resident(const pnp_generator* g) { return g ? g->max_resident : -1; }
int pnp_generator_set_band_split(pnp_generator* g, int on) {
    if (!g || on < 0) return PNP_ERR_BAD_ARG;
    g->band_split = on;
    return PNP_OK;
}
int pnp_generator_get_band_split(const pnp_generator* g) { return g ? g->band_split : -1; }
int pnp_generator_set_any_size(pnp_generator* g, int on) {
    if (!g || on < 0) return PNP_ERR_BAD_ARG;
    g->any_size = on != 0;
    return PNP_OK;
}
int pnp_generator_get_any_size(const pnp_generator* g) { return g ? g->any_size : -1; }
int pnp_band_plan(int rows, int nconv, int a0, int* bounds) {
    int first;
    if (!bounds || nconv > 4096 || !band_plan(rows, nconv, a0, &first)) return 0;
    for (int n = 0; n < nconv; ++n) bounds[n] = first - n;
    return 1;
}
int pnp_generator_min_resident(const pnp_generator* g, int t) {
    if (!g || t < 1) return -1;
    return plan_min_resident(t, g->cfg.with_cat);
}

}  // extern "C"

namespace {

// An untimed launch (or a wait) was issued: it sits between two timed ones, whose shared event (ProfScope) would time it too.
void untimed(const pnp_generator* g) { g->prof_last = nullptr; }

// A row-band chain in flight (band_plan): ClipRun::step opens one per branch run, ClipRun::conv attaches every conv of the run.
// The destructor joins: the caller's stream waits for chain B also on the way out of an error.
struct BandChain {
    const pnp_generator* g;
    hipStream_t st;           // the caller's stream (chain A)
    bool enabled;             // the clip qualifies at all (ClipRun's band_mode)
    int rows;                 // 16-pixel tile rows of the frame
    bool is_open = false, forked = false;
    int left = 0, n = 0, row = 0;       // convs still to come; convs split so far; the next conv's boundary row

    BandChain(const pnp_generator* g_, hipStream_t st_, bool enabled_, int h) : g(g_), st(st_), enabled(enabled_), rows((h + 15) / 16) {}
    BandChain(const BandChain&) = delete;
    ~BandChain() { (void)close(); }
    int first_row() const { return g->band_split >= 2 ? g->band_split : 0; }      // pnp_generator_set_band_split: >= 2 names the first boundary
    int open(int nconv) {
        if (!enabled) return PNP_OK;
        // (the stream and the events are made the first time a frame qualifies: with the chain's first conv on another kernel it is
        //  one conv shorter)
        int first;
        if (!band_plan(rows, nconv, first_row(), &first) && !band_plan(rows, nconv - 1, first_row(), &first)) return PNP_OK;
        if (!g->band_stream) {
            const hipError_t e = hipStreamCreateWithFlags(&g->band_stream, hipStreamNonBlocking);
            if (e != hipSuccess) return (int)e;
        }
        while ((int)g->band_events.size() < nconv + 1) {
            hipEvent_t e;
            const hipError_t err = hipEventCreateWithFlags(&e, hipEventDisableTiming);
            if (err != hipSuccess) return (int)err;
            g->band_events.push_back(e);
        }
        is_open = true, forked = false;
        left = nconv, n = 0;
        return PNP_OK;
    }
    // The next conv of the open chain.  tiles: it runs on the Winograd tile kernels at the frame's size, which take a conv of the chain as
    // two launches.  A conv on another kernel can only be the chain's first (the RGB-only input conv of a clip's last frame): it runs
    // whole on the caller's stream in front of the first `ready` event, and the numbering starts behind it
    int attach(ConvArgs& a, bool tiles) {
        if (!tiles && n > 0) return PNP_ERR_UNSUPPORTED;
        if (tiles && n == 0 && !band_plan(rows, left, first_row(), &row)) is_open = false;          // too few tile rows for this chain: one launch per conv
        --left;
        if (!tiles || !is_open) return PNP_OK;
        g->band_recs.emplace_back();
        ConvBandSplit& band = g->band_recs.back();
        memset(&band, 0, sizeof(band));
        band.side = g->band_stream;
        band.ready = g->band_events[n++];
        band.row = row--;
        a.band = &band;
        forked = true;
        return PNP_OK;
    }
    // the caller's stream waits for chain B: in front of whatever reads a whole map next
    int close() {
        const bool join = is_open && forked;
        is_open = forked = false;
        if (!join) return PNP_OK;
        hipError_t e = hipEventRecord(g->band_events.back(), g->band_stream);
        if (e == hipSuccess) e = hipStreamWaitEvent(st, g->band_events.back(), 0);
        untimed(g);
        return (int)e;
    }
};

// A 4:2:0 clip of either public kind (pnp_clip_yuv | pnp_clip_yuv16): its planes in and out, and the pointers the two kinds share
struct YuvClip {
    YuvPlanes lq, out;
    const float *mvs_dev, *par_dev;
    float* out_f32_dev;
    unsigned char* out_u8_dev;
};

// One sample (clip) of the batch on one stream with one workspace context: what the run needs to know, and its launches phase by phase.
struct ClipRun {
    const pnp_generator* const g;
    const pnp_generator_cfg& c;
    const float *const flat, *const packed;
    const Workspace W;
    const int t, h, w;
    const hipStream_t st;
    // the clip's tensors: the frames as fp32 planes or as bytes, the output as fp32 planes and / or bytes
    const float* const lr_b; const unsigned char* const lq8;
    float* const out_b; unsigned char* const out8;
    const float *const mv_b, *const par_in, *const sl, *const qp, *const bq;
    // ... or the frames and / or one more output as 4:2:0 planes of either sample size (nullptr: not), with the standard's constants
    // at the input's depth and container, and at the output's
    const YuvPlanes *const lqy, *const outy;
    YuvCoef yk_in{}, yk_out{};
    const bool staged, alone;      // alone: the only workspace context in flight
    const int64_t hw = (int64_t)h * w, fm = hw * 64;
    const int E = c.num_experts, cfg_lr = conv_pick_cfg(h, w), os = c.vsr ? 4 : 1;
    const bool f16_maps = g->prec == PNP_PREC_F16 && g->opt[PNP_OPT_F16_MAPS], par_skip = g->opt[PNP_OPT_PAR_SKIP] != 0;
    // Winograd form of the single-source 64 -> 64 convs (fp32 path only): 1 = frames that fill the chip with 16x16 tiles, 2 = always
    const int wopt = g->prec == PNP_PREC_F32 ? g->opt[PNP_OPT_WINOGRAD] : 0;
    const bool wino_on = wopt != 0;
    // every 64-channel map that is only read as an MFMA A operand gets an fp16 copy from its producer
    const bool mirrors = f16_maps && g->opt[PNP_OPT_F16_MIRRORS] && c.deform == 0 && W.x16 != nullptr;
    // ... and, optionally, the running map x INSIDE a branch too (input conv and every block write x16 next to x, every front
    // half reads it).  Measured at 720p inside the pipeline (profiles/r03_fp16_*): the front half gains what the back half loses
    // to the extra 128 B per pixel it writes -- off by default, the frame slots keep their mirrors.
    const bool chain16 = mirrors && g->opt[PNP_OPT_F16_CHAIN_MIRRORS];
    // row-band chains: not with several clips on several streams, which fill each other's launch tails already
    const bool band_mode = alone && g->band_split != 0 && wopt != 0 && !wino_units(h, w);
    BandChain chain{g, st, band_mode, h};
    // what the prologue leaves for the sweeps: the mixture of every frame, the key frames, the partition planes the block convs read
    std::vector<int> uidx;
    std::vector<char> key;
    const float* par_b = par_in;
    bool sparse_per_frame = false;

    ClipRun(const pnp_generator* g_, const float* flat_, const float* packed_, const pnp_clip_io& io, int lq_format, int out_mask,
            const float* sl_, const float* qp_, const float* bq_, const Workspace& W_, int t_, int h_, int w_, hipStream_t st_, bool alone_,
            const YuvClip* yuv = nullptr, int yuv_standard = 0)
        : g(g_), c(g_->cfg), flat(flat_), packed(packed_), W(W_), t(t_), h(h_), w(w_), st(st_),
          lr_b(lq_format == PNP_FRAMES_F32_NCHW ? static_cast<const float*>(io.lq_dev) : nullptr),
          lq8(lq_format == PNP_FRAMES_U8_HWC ? static_cast<const unsigned char*>(io.lq_dev) : nullptr),
          out_b((out_mask & PNP_OUT_F32) ? io.out_f32_dev : nullptr), out8((out_mask & PNP_OUT_U8) ? io.out_u8_dev : nullptr),
          mv_b(io.mvs_dev), par_in(io.par_dev), sl(sl_), qp(qp_), bq(bq_), lqy(yuv ? &yuv->lq : nullptr),
          outy((yuv && (out_mask & PNP_OUT_YUV420)) ? &yuv->out : nullptr), staged((lq8 || out8 || lqy) && io_staged(g_)), alone(alone_) {
        if (lqy) (void)yuv_coef(yuv_standard, *lqy, &yk_in);
        if (outy) (void)yuv_coef(yuv_standard, *outy, &yk_out);
    }

    // fp16 mirror of a weight image that lives in `packed` or in the per-clip expert mixtures
    const void* twin(const float* p) const {
        if (g->prec == PNP_PREC_F32 || !p) return nullptr;
        const int64_t halfs = g->prec == PNP_PREC_F16X3 ? 2 : 1;       // halfs of the twin per float of the image
        if (p >= packed && p < packed + g->packed_floats)
            return reinterpret_cast<const uint16_t*>(packed + g->packed_floats) + halfs * (p - packed);
        if (p >= W.mixw && p < W.mixw + (int64_t)t * g->ndyn * IMG_WIDE) return reinterpret_cast<const uint16_t*>(W.mixh) + halfs * (p - W.mixw);
        return nullptr;
    }
    // wopt 1: a frame of N 16x16 tiles takes the quadrant-unit kernel up to N = 128 (4 N blocks; 128x128: 12 us per conv against the direct
    // kernel's 15 and the tile kernel's 26 on 64 of 256 CUs) and the persistent tile kernel above (240 tiles: 31 us against 48 direct);
    // the input convs over wide sources likewise (180x320, 240 tiles, fp32: 561 frames/s direct, 707 with the direct input convs kept,
    // 712 with the multi-source tile kernel).  2 = the tile kernels at every size (tests)
    static int64_t ntiles16(int hh, int ww) { return (int64_t)((hh + 15) / 16) * ((ww + 15) / 16); }
    bool wino_units(int hh, int ww) const { return wopt == 1 && ntiles16(hh, ww) <= PNP_WINO_UNITS_MAX_TILES; }
    const float* wi(int64_t off) const { return wino_on ? packed + off : nullptr; }      // a Winograd image in `packed`
    // image buffer `buf` of W.wino: a branch run's Winograd images of its expert-mixed convs (branch_images)
    float* wino_buf(int buf) const { return W.wino + (int64_t)buf * 2 * c.num_blocks * PNP_WINO_IMG_FLOATS; }
    // expert-mixed conv `dyn` of mixture u: its weight image and its bias
    float* mix_w(int u, int dyn) const { return W.mixw + ((int64_t)u * g->ndyn + dyn) * IMG_WIDE; }
    float* mix_b(int u, int dyn) const { return W.mixb + ((int64_t)u * g->ndyn + dyn) * 64; }
    const float* gam(int i) const { return (c.with_bias && c.with_se) ? W.gamma + (int64_t)i * 64 : nullptr; }      // frame i's channel gain
    const float* routing() const { return c.use_base_qp ? bq : qp; }
    float* slot_of(int s) const { return W.slots + (int64_t)s * fm; }
    // fp16 mirror of a frame slot (sources of an input conv, conv_hr)
    const void* s16of(int s) const { return mirrors ? (const void*)(W.slots16 + (int64_t)s * fm) : nullptr; }
    // bounded schedule: frame i's sparse-equivalent partition map into the one-frame buffer
    int sparse_frame(int i) const { return launch_par_sparse(par_in + (int64_t)i * 3 * hw, W.parbin, 1, h, w, st); }

    // ConvCall -> ConvArgs: no side effect, no chain state
    ConvArgs conv_args(const ConvCall& q) const {
        ConvArgs a;
        memset(&a, 0, sizeof(a));
        a.nsrc = q.nsrc;
        a.prec = g->prec;                 // PNP_PREC_* are ConvArgs::prec's values
        for (int s = 0; s < q.nsrc; ++s) {
            a.src[s] = q.src[s], a.src_c[s] = q.sc[s];
            a.wsrc[s] = q.w[s], a.wsrc_h[s] = twin(q.w[s]);
        }
        a.wpar = q.wpar_, a.wwino = q.wino_, a.wwino_par = q.wino_par_;
        if (q.nsrc >= 2 && q.sc[0] == 4 && q.wsrc_wino_[0]) {      // input conv with Winograd images on every member
            a.wwino_rgb = q.wsrc_wino_[0];
            for (int s = 1; s < q.nsrc; ++s) a.wwino_src[s] = q.wsrc_wino_[s];
        }
        a.wino_units = (q.wino_ || a.wwino_rgb) ? q.units_ : 0;
        a.par_any = (q.wino_ && q.wpar_) ? q.par_any_ : nullptr;       // (tile kernels and quadrant-unit kernels alike: one gated launch)
        a.fold_tab = a.par_any ? q.fold_tab_ : nullptr;
        a.wpar_h = twin(q.wpar_);
        a.wpar_h_scaled = (g->prec == PNP_PREC_F16X3 && a.wpar_h) ? 1 : 0;     // the packed buffer holds 3 + 3 branch images (build_layout)
        a.par = q.par_, a.par_flags = q.par_flags_;
        a.tile_queue = (g->prec == PNP_PREC_F16X3 && g->opt[PNP_OPT_TILE_QUEUE]) ? W.queue : nullptr;
        a.par_plane = (long)q.H * q.W;
        a.bias = q.bias_, a.gamma = q.gamma_, a.residual = q.residual_, a.out = q.dst;
        a.lr = q.lr_, a.lr_plane = q.lr_plane_;
        a.wvalu = g->opt[PNP_OPT_CONV_LAST_VALU] ? q.wvalu_ : nullptr;
        a.no_persist = g->opt[PNP_OPT_PERSIST] ? 0 : 1, a.no_small16 = g->opt[PNP_OPT_SMALL_F16] ? 0 : 1;
        a.w_ystride = q.w_ystride_, a.bias_ystride = q.bias_ystride_;
        a.H = q.H, a.W = q.W, a.act = q.act_;
        a.out_mode = q.mode_, a.out_cstride = 448;
        a.lr_u8 = q.lr8_, a.out_u8 = q.out8_;
        a.lr_rgb0 = q.lr0_;
        a.out_f16 = q.io16_ & 1;          // io16: bit 0 the output is an fp16 map, bit 1 source 0 is one
        a.src_f16 = (q.io16_ & 2) ? 1 : 0;
        if (mirrors) {
            for (int s = 0; s < q.nsrc; ++s)
                if (q.src16_[s]) {
                    a.src[s] = reinterpret_cast<const float*>(q.src16_[s]);
                    a.src_f16 |= 1 << s;
                }
            a.out16 = q.out16_;
        }
        return a;
    }
    // what ProfScope books a launch under: its kind, and its algorithmic FLOPs (reference channel counts, not padded ones)
    static int conv_kind(const ConvCall& q) {
        return (q.mode_ != 0) ? PNP_PROF_CONV_HEAD : (q.nsrc > 1 || q.sc[0] != 64) ? PNP_PROF_CONV_INPUT : PNP_PROF_CONV_BLOCK;
    }
    static double conv_work(const ConvCall& q) {
        double kreal = 0;
        for (int s = 0; s < q.nsrc; ++s) kreal += 9.0 * (q.sc[s] == 64 ? 64 : 3);
        if (q.wpar_) kreal += 3 * 64;
        const double nreal = (q.mode_ == 2 || q.mode_ == 3) ? 3 : 64;   // RGB heads; mode 4 (DCN offsets) is 64 per blockIdx.y
        return 2.0 * kreal * nreal * (double)q.H * q.W * q.gy_;
    }
    int conv(const ConvCall& q) {
        ConvArgs a = conv_args(q);
        // (a conv of a row-band chain is timed like any other, on the caller's stream: back to back with its neighbours that is the
        //  chain's time per conv.  Its part on the side stream shares the chip with the next conv's part A: timed as well and added,
        //  a kind's total would exceed wall time, which bench.py's rooflines -- executed work over launch time -- rule out)
        ProfScope ps(g, st, conv_kind(q), conv_work(q));
        if (chain.is_open) {
            const bool tiles = !a.wino_units && q.H == h && q.W == w && (conv_wino_eligible(a, q.cfg_, q.gy_) || conv_wino_ms_eligible(a, q.cfg_, q.gy_));
            const int rc = chain.attach(a, tiles);
            if (rc) return rc;
        }
        if (a.lr_u8 || a.out_u8 || a.lr_rgb0) return launch_conv_last_io(a, st);      // (conv_last only, outside every chain)
        return launch_conv3x3(a, q.cfg_, q.gy_, st);
    }

    int fill_and_pack() {
        untimed(g);           // untimed launches follow
        if (W.queue) {
            // the last block of every launch leaves the queue zeroed; once per clip for a fresh workspace or a launch that was cut short.
            // A KERNEL, not hipMemsetAsync: as a memset node of a captured graph (generator.use_graphs) the 64 bytes came back as
            // pointer-like garbage from the second replay on (ROCm 7.2; tools/repro/graph_memset_node.py), i.e. endless ticket loops
            const int rc = launch_fill(reinterpret_cast<float*>(W.queue), 0.0f, 16, st);
            if (rc) return rc;
        }
        if (lqy) return launch_pack_lr_yuv420(*lqy, yk_in, W.lr4, t, h, w, false, st);
        if (!lq8) return launch_pack_lr(lr_b, W.lr4, t, h, w, st);
        // any_size: a clip that is not whole 12-byte groups on a 4-aligned address takes the kernel with a head and a tail; every
        // other clip the one it always took
        const bool ragged = (((int64_t)t * hw) & 3) || (reinterpret_cast<uintptr_t>(lq8) & 3);
        return (g->any_size && ragged) ? launch_pack_lr_u8_any(lq8, W.lr4, t, h, w, st) : launch_pack_lr_u8(lq8, W.lr4, t, h, w, st);
    }
    int partition_maps() {
        // the reference's (eval-mode) sparse evaluation as a dense map (prep.hip): for the whole clip at once, or (bounded schedule)
        // one frame at a time into a one-frame buffer, just before each branch run that reads it
        const bool sparse_now = c.sparse_val && g->opt[PNP_OPT_SPARSE_EVAL];
        sparse_per_frame = sparse_now && bounded_mode(g, t);
        int rc = PNP_OK;
        if (sparse_now && !sparse_per_frame) {
            rc = launch_par_sparse(par_in, W.parbin, t, h, w, st);
            if (rc) return rc;
            par_b = W.parbin;
        }
        // which 1x1 partition branches each 8x16 tile of each frame needs at all (32 front-half launches per frame use it)
        if (!par_skip) return PNP_OK;
        for (int i = 0; sparse_per_frame && i < t && !rc; ++i) {
            rc = sparse_frame(i);
            if (!rc) rc = launch_par_tile_flags(W.parbin, hw, W.parflags + i * par_flag_tiles(h, w), 1, h, w, st);
        }
        if (!sparse_per_frame) rc = launch_par_tile_flags(par_b, hw, W.parflags, t, h, w, st);
        if (rc) return rc;
        if (wopt >= 1) rc = launch_par_frame_any(W.parflags, W.parany, t, h, w, st);      // (for the I frames' gated front halves)
        return rc;
    }
    // CAA hyper-network (iconvsr_ipb_par.py:45-48)
    int caa() {
        for (int t0 = 0; t0 < t; t0 += 32) {
            CaaArgs a;
            memset(&a, 0, sizeof(a));
            a.count = (t - t0 < 32) ? t - t0 : 32;
            for (int i = 0; i < a.count; ++i) {
                a.q_ew[i] = routing()[t0 + i];
                a.q_g[i] = qp[t0 + i];
            }
            a.t0 = t0, a.E = E, a.softmax = c.expert_softmax;
            a.with_se = (c.with_bias && c.with_se) ? 1 : 0;
            a.w1 = flat + g->p_w1, a.b1 = flat + g->p_b1;
            a.w2 = flat + g->p_w2, a.b2 = flat + g->p_b2;
            a.v1 = a.with_se ? flat + g->p_v1 : nullptr;
            a.v2 = a.with_se ? flat + g->p_v2 : nullptr;
            a.ew = W.ew, a.gamma = W.gamma;
            const int rc = launch_caa_predict(a, st);
            if (rc) return rc;
        }
        return PNP_OK;
    }
    // mixture u of every expert-mixed conv, from frame i's expert attention (+ its fp16 twin)
    int mix(int i, int u) {
        const int gcm = 64 / c.num_group;
        PackArgs a = plain_pack(flat + g->dyn_w, 64, 9, PACK_WIDE, 0, 2, 64, mix_w(u, 0));
        a.ew = W.ew + (int64_t)i * E;
        a.E = E;
        a.e_stride = 64 * gcm * 9;
        a.group_cin = c.num_group > 1 ? gcm : 0;
        a.w_ystride = (int64_t)E * 64 * gcm * 9;
        a.dst_ystride = IMG_WIDE;
        int rc = launch_pack_weights(a, g->ndyn, st);
        if (rc) return rc;
        rc = launch_mix_bias(flat + g->dyn_b, a.ew, mix_b(u, 0), E, 64, g->ndyn, st);
        if (rc) return rc;
        uint16_t* const mixh = reinterpret_cast<uint16_t*>(W.mixh);
        if (g->prec == PNP_PREC_F16) rc = launch_f16_image(a.dst, mixh + (a.dst - W.mixw), g->ndyn * 9, 2, st);
        if (g->prec == PNP_PREC_F16X3) rc = launch_f16x3_image(a.dst, mixh + (a.dst - W.mixw) * 2, g->ndyn * 9, st);
        return rc;
    }
    // expert mixing, once per distinct routing input
    int mix_experts() {
        const float* qe = routing();
        uidx.resize(t);
        std::vector<int> ufirst;
        for (int i = 0; i < t; ++i) {
            int u = 0;
            while (u < (int)ufirst.size() && memcmp(&qe[ufirst[u]], &qe[i], sizeof(float)) != 0) ++u;
            if (u == (int)ufirst.size()) {
                ufirst.push_back(i);
                const int rc = g->ndyn > 0 ? mix(i, u) : PNP_OK;      // ('drt_woqp': no expert-mixed conv at all)
                if (rc) return rc;
            }
            uidx[i] = u;
        }
        return PNP_OK;
    }

    // deform_align(feat, flow) -> W.kw  (iconvsr_ipb.py:19-24 dispatch; iconvsr_mv.py:12-84)
    int align(const float* feat, const float* fxp, const float* fyp) {
        int r;
        if (c.deform == 0 || c.deform == 1) {   // 'vos', and the pre-warp of 'basic' (:69)
            ProfScope ps(g, st, PNP_PROF_WARP, (mirrors ? 392.0 : 520.0) * (double)hw);     // 8 flow + 256 gather + 256 | 128 write
            r = launch_mv_warp_nhwc(feat, fxp, fyp, c.deform == 0 ? W.kw : W.tmp0, h, w, 64, st, mirrors, c.flow_inter == 1);   // mirrors: kw is fp16
            if (r || c.deform == 0) return r;
        }
        r = launch_pack_flow4(fxp, fyp, W.flow4, h, w, st);
        untimed(g);
        if (r) return r;
        // conv_offset[0] + LeakyReLU over cat([ref_warped | ref_unwarped, flow])
        r = conv(ConvCall(h, w, cfg_lr).source(W.flow4, 4, packed + g->off0_flow_img)
                     .source(c.deform == 1 ? W.tmp0 : feat, 64, packed + g->off0_feat_img)
                     .bias(flat + g->f_off0_b).act(2).to(W.tmp1));
        if (r) return r;
        // conv_offset[2]: 64 -> 432 (7 blocks of 64 permuted channels), no activation
        r = conv(ConvCall(h, w, cfg_lr).source(W.tmp1, 64, packed + g->off2_img).bias(packed + g->off2_bias, 64)
                     .mode(4, 7, IMG_WIDE).to(W.om));
        if (r) return r;
        DcnArgs d;
        d.dbg = nullptr;
        d.x = feat, d.om = W.om, d.out = W.kw;
        d.fx = c.deform == 1 ? fxp : nullptr;
        d.fy = c.deform == 1 ? fyp : nullptr;
        d.w = packed + g->dcn_img;
        d.w16 = g->prec == PNP_PREC_F16 ? twin(packed + g->dcn_img) : nullptr;
        d.bias = flat + g->f_dcn_b;
        d.H = h, d.W = w;
        ProfScope ps(g, st, PNP_PROF_DCN, 2240.0 * (double)hw);
        return launch_dcn(d, st);
    }

    // A branch run's Winograd images of its expert-mixed convs, this frame's channel gain folded in, into image buffer `buf` of W.wino.
    // They depend on the clip prologue only (mixtures, gamma), not on any feature map, so the step loop issues run s + 1's in front
    // of run s's chain (the first run's in front of the loop) into the buffer run s does not read: inside run_branch, between the
    // input conv and the first block conv, the launch waited for CUs behind chain B's input-conv part and held chain A back.
    // Buffer s & 1 is rewritten (for run s + 2) in front of run s + 1's chain, i.e. behind run s's join on the caller's stream.
    int branch_images(int brid, int i, int buf) {
        if (!(wino_on && g->ndyn > 0)) return 0;
        float* wb = wino_buf(buf);
        std::vector<const float*> ws;
        std::vector<float*> wd;
        for (int k = 0; k < c.num_blocks; ++k) {
            const BlockPk& K = g->br[brid].blocks[k];
            if (K.dyn_conv2 >= 0) { ws.push_back(mix_w(uidx[i], K.dyn_conv2)); wd.push_back(wb + (int64_t)(2 * k) * PNP_WINO_IMG_FLOATS); }
            if (K.dyn_conv1 >= 0) { ws.push_back(mix_w(uidx[i], K.dyn_conv1)); wd.push_back(wb + (int64_t)(2 * k + 1) * PNP_WINO_IMG_FLOATS); }
        }
        for (size_t j = 0; j < ws.size(); j += 16) {
            const int n = (int)(ws.size() - j < 16 ? ws.size() - j : 16);
            const int r = launch_wino_images(ws.data() + j, wd.data() + j, n, gam(i), st);
            if (r) return r;
        }
        untimed(g);
        return 0;
    }

    // Frame i's fold table (fold_table.h) into table buffer `buf`, in front of the branch run that reads it: plane and factor of every
    // 8x8 quadrant, which each of the run's gated front halves would otherwise derive again per tile from the partition planes.  One
    // small launch on the caller's stream, in plain stream order behind the frame's partition map (bounded schedule: its one-frame
    // buffer) and in front of both chains of the run; two buffers, used like the image buffers of W.wino (run s writes s & 1, which
    // run s - 2 read last).  Per run and not per clip: a table per frame of the clip would be workspace that grows with the clip.
    bool fold_on() const { return W.foldtab && wino_on && par_skip && !wino_units(h, w); }
    PnpFoldRec* fold_buf(int buf) const { return W.foldtab + (int64_t)buf * pnp_fold_records(h, w); }
    const float* par_of(int i) const { return sparse_per_frame ? W.parbin : par_b + (int64_t)i * 3 * hw; }
    int fold_table(int i, int buf) {
        if (!fold_on()) return 0;
        const int rc = launch_par_fold_table(par_of(i), hw, fold_buf(buf), 1, h, w, st);
        untimed(g);
        return rc;
    }

    // input conv over the virtual concat `in` (sources already added), then the BAE blocks
    // (out: the frame map its last block writes, Step::out)
    int run_branch(int brid, int i, int out, int buf, ConvCall in) {
        const BranchPk& B = g->br[brid];
        const float* wbuf = W.wino ? wino_buf(buf) : nullptr;
        const float* parp = par_of(i);
        const PnpFoldRec* ftab = fold_on() ? fold_buf(buf) : nullptr;
        const int* pflags = par_skip ? W.parflags + (int64_t)i * par_flag_tiles(h, w) : nullptr;
        // the frame's partition word (launch_par_frame_any) gates the front halves on the device: fold-only kernel / branch kernel
        // (launch_conv3x3_wino); an I frame usually carries no record at all (its word is then 8: all quadrants zero)
        // (any frame size: a quadrant cut by the frame's edge -- 180x320 has a last row of them 4 pixels high -- counts with the pixels
        //  it has, in the flags and in the kernels alike)
        const int* pany = (par_skip && wopt >= 1) ? W.parany + i : nullptr;
        const int u = uidx[i];
        const bool un = wino_units(h, w);
        // fp16 mirrors: the input conv writes x16 next to x when it runs on the fp16 kernels at all (an RGB-only one does not)
        const void* x16 = (chain16 && in.nsrc > 1) ? W.x16 : nullptr;
        int r = conv(in.bias(flat + B.in_bias).act(2).units(un).to(W.tmp0).also16(const_cast<void*>(x16)));
        if (r) return r;
        const float* x = W.tmp0;
        const bool woqp = c.blocktype == 1;      // conv2 a plain conv as well: no expert mix, no gain (sr_backbone_utils.py:366-384)
        // the map between the two halves is read only as an MFMA A operand: an fp16 map on the fp16 path
        const int o16 = f16_maps ? 1 : 0, s16 = f16_maps ? 2 : 0;
        for (int k = 0; k < c.num_blocks; ++k) {
            const BlockPk& K = B.blocks[k];
            const bool last = k == c.num_blocks - 1;
            float* dst = last ? slot_of(out) : W.tmp0;
            void* dst16 = !mirrors ? nullptr : last ? (void*)(W.slots16 + (int64_t)out * fm) : (chain16 ? (void*)W.x16 : nullptr);
            const float* w2 = woqp ? packed + K.conv2_img : mix_w(u, K.dyn_conv2);
            const float* b2 = woqp ? flat + K.conv2_bias : mix_b(u, K.dyn_conv2);
            const float* g2 = woqp ? nullptr : gam(i);
            const float* w1 = c.one_layer ? packed + K.conv1_img : mix_w(u, K.dyn_conv1);
            const float* b1 = c.one_layer ? flat + K.conv1_bias : mix_b(u, K.dyn_conv1);
            const float* g1 = c.one_layer ? nullptr : gam(i);
            const float* u2 = !wino_on ? nullptr : (woqp ? packed + K.conv2_wino : wbuf + (int64_t)(2 * k) * PNP_WINO_IMG_FLOATS);
            const float* u1 = !wino_on ? nullptr : (c.one_layer ? packed + K.conv1_wino : wbuf + (int64_t)(2 * k + 1) * PNP_WINO_IMG_FLOATS);
            if (c.channel_first) {   // sr_backbone_utils.py:305-313
                r = conv(ConvCall(h, w, cfg_lr).source(x, 64, w2).mirror16(x16).bias(b2).gamma(g2)
                             .partition(packed + K.w1x1, parp, pflags).gate(pany, ftab).wino(u2, wi(K.w1x1_wino)).units(un).act(1).to(W.tmp1).f16_map(o16));
                if (!r)
                    r = conv(ConvCall(h, w, cfg_lr).source(W.tmp1, 64, w1).bias(b1).gamma(g1).wino(u1).units(un).residual(x).to(dst)
                                 .f16_map(s16).also16(dst16));
            } else {                 // sr_backbone_utils.py:314-327
                r = conv(ConvCall(h, w, cfg_lr).source(x, 64, w1).mirror16(x16).bias(b1).gamma(g1).wino(u1).units(un).act(1).to(W.tmp1)
                             .f16_map(o16));
                if (!r)
                    r = conv(ConvCall(h, w, cfg_lr).source(W.tmp1, 64, w2).bias(b2).gamma(g2)
                                 .partition(packed + K.w1x1, parp, pflags).gate(pany, ftab).wino(u2, wi(K.w1x1_wino)).units(un).residual(x).to(dst).f16_map(s16).also16(dst16));
            }
            if (r) return r;
            x = dst;
            x16 = chain16 ? dst16 : nullptr;
        }
        return 0;
    }

    // reconstruction of a forward step's frame (iconvsr_ipb_par.py:135-146): [two PixelShufflePack(2) convs, 4 sub-pixel weight images
    // each,] conv_hr, then conv_last + the (x4 bilinear) frame
    int head(const Step& sp) {
        const int i = sp.frame, H = h * os, Wd = w * os;
        // every map of the head is read by exactly one conv, as an MFMA A operand: fp16 maps all the way on the fp16 path
        // (the 720p map between the second pixel shuffle and conv_hr alone is 236 MB written + read per frame in fp32)
        const int o16 = f16_maps ? 1 : 0, s16 = f16_maps ? 2 : 0;
        const float* x = slot_of(sp.out);
        const void* x16 = s16of(sp.out);
        int rc = PNP_OK;
        if (c.vsr) {
            rc = conv(ConvCall(h, w, cfg_lr).source(x, 64, packed + g->up_img[0]).bias(packed + g->up_bias[0], 64)
                          .act(2).mode(1, 4, IMG_WIDE).to(W.u1).f16_map(o16));
            if (!rc)
                rc = conv(ConvCall(2 * h, 2 * w, conv_pick_cfg(2 * h, 2 * w)).source(W.u1, 64, packed + g->up_img[1])
                              .bias(packed + g->up_bias[1], 64).act(2).mode(1, 4, IMG_WIDE).to(W.u2).f16_map(o16 | s16));
            if (rc) return rc;
            x = W.u2;
            x16 = nullptr;
        }
        float* const top = c.vsr ? W.u3 : W.tmp1;
        rc = conv(ConvCall(H, Wd, conv_pick_cfg(H, Wd)).source(x, 64, packed + g->hr_img).mirror16(x16).bias(flat + g->hr_bias)
                      .wino(wi(g->hr_wino)).units(wino_units(H, Wd)).act(2).to(top).f16_map(c.vsr ? o16 | s16 : o16));
        if (!rc) rc = chain.close();      // (conv_hr at the frame's size is the last conv of a forward branch's chain)
        if (rc) return rc;
        const float* lr_i = lr_b ? lr_b + (int64_t)i * 3 * hw : nullptr;
        float* out_i = out_b ? out_b + (int64_t)i * 3 * hw * os * os : nullptr;
        const unsigned char* lr8_i = lq8 ? lq8 + (int64_t)i * 3 * hw : nullptr;
        unsigned char* const out8_i = out8 ? out8 + (int64_t)i * 3 * hw * os * os : nullptr;
        // a last conv with an fp32 interface: this frame's bytes to planes in front of it, its planes to bytes behind it (untimed, like pack_lr)
        if (staged && lr8_i) {
            rc = launch_frames_from_rgb8(lr8_i, W.lr1, 1, h, w, st);
            untimed(g);
            if (rc) return rc;
            lr_i = W.lr1;
            lr8_i = nullptr;
        }
        // a 4:2:0 clip: the frame conv_last adds is the RGB0 frame the pack launch left in the workspace, or (fp32 interface) its planes
        const float* lr0_i = nullptr;
        if (lqy && staged) {
            rc = launch_frames_from_yuv420(yuv_frame(*lqy, i), yk_in, W.lr1, 1, h, w, st);
            untimed(g);
            if (rc) return rc;
            lr_i = W.lr1;
        } else if (lqy) {
            lr0_i = W.lr4 + (int64_t)i * hw * 4;
        }
        if (((staged && out8_i) || outy) && !out_i) out_i = W.out1;
        rc = conv(ConvCall(H, Wd, CONV_CFG_RGB).source(top, 64, packed + g->last_img).bias(packed + g->last_bias)
                      .mode(c.vsr ? 3 : 2).rgb(lr_i, hw, packed + g->last_valu).rgb8(lr8_i, staged ? nullptr : out8_i).rgb0(lr0_i).to(out_i).f16_map(s16));
        if (rc) return rc;
        if (staged && out8_i) {
            untimed(g);
            rc = launch_frames_to_rgb8(out_i, out8_i, 1, H, Wd, st);
            if (rc) return rc;
        }
        if (!outy) return rc;
        untimed(g);
        return launch_frames_to_yuv420(out_i, yuv_frame(*outy, i), yk_out, 1, H, Wd, st);
    }

    // one branch run of the schedule (recomputed runs of the bounded schedule are steps like any other) and, forward, the frame's head
    int step(const std::vector<Step>& steps, size_t si) {
        const Step& sp = steps[si];
        const int i = sp.frame;
        const BranchPk& B = g->br[sp.sweep];
        ConvCall in(h, w, cfg_lr);
        in.source(W.lr4 + (int64_t)i * hw * 4, 4, packed + B.in_lr, wi(B.in_lr_wino));
        int rc;
        if (sp.key >= 0) {      // backward: the nearest key frame after i (flow planes 2, 3); forward: before i (planes 0, 1)
            const int fp = sp.sweep == 0 ? 2 : 0;
            rc = align(slot_of(sp.key), mv_b + ((int64_t)i * 4 + fp) * hw, mv_b + ((int64_t)i * 4 + fp + 1) * hw);
            if (rc) return rc;
            // fp16 mirrors of the sources: the aligned key frame (fp16 ONLY in this mode, written by the warp) and the neighbouring / own slots
            const void* kw16 = mirrors ? (const void*)W.kw : nullptr;
            if (c.with_cat && c.align_key && sp.key_frame == (sp.sweep == 0 ? i + 1 : i - 1)) {     // neighbour == key frame: one source, summed weights
                in.source(W.kw, 64, packed + B.in_wide01, wi(B.in_wide01_wino)).mirror16(kw16);
            } else {
                in.source(W.kw, 64, packed + B.in_wide[0], wi(B.in_wide_wino[0])).mirror16(kw16);
                if (c.with_cat) in.source(slot_of(sp.nb), 64, packed + B.in_wide[1], wi(B.in_wide_wino[1])).mirror16(s16of(sp.nb));
            }
        }
        if (sp.sweep == 1)      // backward feature of this frame
            in.source(slot_of(sp.own), 64, packed + B.in_wide[B.n_wide - 1], wi(B.in_wide_wino[B.n_wide - 1])).mirror16(s16of(sp.own));
        if (sparse_per_frame) {
            rc = sparse_frame(i);
            untimed(g);
            if (rc) return rc;
        }
        // the branch's convs as a row-band chain: input conv + two per block (+ conv_hr behind a forward branch at the frame's size)
        const bool hr_in_chain = sp.sweep == 1 && !c.vsr;
        // the next run's images first: off this run's chains
        if (si + 1 < steps.size()) {
            rc = branch_images(steps[si + 1].sweep, steps[si + 1].frame, (int)((si + 1) & 1));
            if (rc) return rc;
        }
        rc = fold_table(i, (int)(si & 1));
        if (rc) return rc;
        rc = chain.open(1 + 2 * c.num_blocks + (hr_in_chain ? 1 : 0));
        if (rc) return rc;
        rc = run_branch(sp.sweep, i, sp.out, (int)(si & 1), in);
        if (!rc && !hr_in_chain) rc = chain.close();
        if (rc || sp.sweep == 0) return rc;
        return head(sp);
    }

    int run() {
        int rc = fill_and_pack();
        if (!rc) rc = partition_maps();
        if (!rc) rc = caa();
        if (!rc) rc = mix_experts();
        if (rc) return rc;
        // key frames (iconvsr_ipb_par.py:60-62)
        key.resize(t);
        for (int i = 0; i < t; ++i) key[i] = (sl[i] == 73.0f) || (sl[i] == 80.0f);
        key[0] = key[t - 1] = 1;
        // backward sweep (iconvsr_ipb_par.py:71-100), forward sweep + heads (:103-147); bounded: with recomputed segments
        std::vector<Step> steps;
        int recomputed = 0;
        if (!make_schedule(g, t, key, steps, &recomputed)) return PNP_ERR_BAD_ARG;
        if (!steps.empty()) rc = branch_images(steps[0].sweep, steps[0].frame, 0);
        for (size_t si = 0; si < steps.size() && !rc; ++si) rc = step(steps, si);
        return rc;
    }
};

bool io_args_ok(int lq_format, int out_mask) {
    return (lq_format == PNP_FRAMES_F32_NCHW || lq_format == PNP_FRAMES_U8_HWC) && out_mask >= 1 && out_mask <= (PNP_OUT_F32 | PNP_OUT_U8);
}

// What a forward refuses before it looks at a clip: batch and frame size, the bound, the workspace.  PNP_OK or the error.
int forward_check(const pnp_generator* g, int n, int t, int h, int w, int lq_format, int out_mask, const void* workspace,
                  int64_t workspace_bytes) {
    if (n < 1 || t < 1) return PNP_ERR_BAD_ARG;
    if (g->cfg.sparse_val && g->opt[PNP_OPT_SPARSE_EVAL] && n != 1) return PNP_ERR_UNSUPPORTED;   // sparse_conv reads feature[0] only (sr_backbone_utils.py:262-275)
    if (h < 64 || w < 64) return PNP_ERR_SIZE_ASSERT;
    if (!g->any_size && ((h % 4) || (w % 4))) return PNP_ERR_SIZE_VALUE;
    if (g->any_size && g->cfg.deform != 0) return PNP_ERR_UNSUPPORTED;      // the DCN aligners have never run on a frame that is no multiple of 4
    // the kernels address a feature map with 32-bit byte offsets: the largest one (x16 pixels with the x4 heads) must
    // stay below 4 GiB (2160p, or 720p -> 2880p with vsr, still fit)
    if (pnp_addr32_bytes_per_lr_pixel(g->cfg.vsr, g->cfg.deform) * (int64_t)h * w >= (int64_t)1 << 32)
        return PNP_ERR_UNSUPPORTED;
    int plan_r, plan_l;
    if (bounded_mode(g, t) && !plan_pick(t, g->cfg.with_cat, g->max_resident, &plan_r, &plan_l)) return PNP_ERR_BAD_ARG;
    const int64_t ctx_bytes = carve(g, nullptr, t, h, w, lq_format, out_mask).bytes;
    if (workspace_bytes < ctx_bytes || (reinterpret_cast<uintptr_t>(workspace) & 255)) return PNP_ERR_WORKSPACE;
    return PNP_OK;
}

// The batch loop behind both entry points: n clips, each named by a descriptor, `lq_format` / `out_mask` for all of them.
int forward_batch(const pnp_generator* g, const float* flat, const float* packed, const pnp_clip_io* clips, int n, int lq_format,
                  int out_mask, const float* slices, const float* qps, const float* base_qps, void* workspace, int64_t workspace_bytes,
                  int t, int h, int w, hipStream_t st, const YuvClip* yclips = nullptr, int yuv_standard = 0) {
    const int bad = forward_check(g, n, t, h, w, lq_format, out_mask, workspace, workspace_bytes);
    if (bad) return bad;
    const int64_t ctx_bytes = carve(g, nullptr, t, h, w, lq_format, out_mask).bytes;
    // Samples of a batch never interact.  With a workspace of k contexts they run k at a time on the library's side
    // streams (forked from / joined to the caller's stream with events): small frames leave most of the chip idle.
    int nctx = (int)(workspace_bytes / ctx_bytes);
    nctx = nctx > PNP_MAX_CONTEXTS ? PNP_MAX_CONTEXTS : nctx;
    nctx = nctx > n ? n : nctx;
    if (nctx > 1) {
        while ((int)g->side_streams.size() < nctx) {
            hipStream_t s;
            hipEvent_t e;
            hipError_t err = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
            if (err != hipSuccess) return (int)err;
            err = hipEventCreateWithFlags(&e, hipEventDisableTiming);
            if (err != hipSuccess) return (int)err;
            g->side_streams.push_back(s);
            g->join_events.push_back(e);
        }
        if (!g->fork_event) {
            const hipError_t err = hipEventCreateWithFlags(&g->fork_event, hipEventDisableTiming);
            if (err != hipSuccess) return (int)err;
        }
        hipError_t err = hipEventRecord(g->fork_event, st);
        for (int k = 0; k < nctx && err == hipSuccess; ++k) err = hipStreamWaitEvent(g->side_streams[k], g->fork_event, 0);
        if (err != hipSuccess) return (int)err;
    }
    int rc = PNP_OK;
    g->band_recs.clear();
    for (int b = 0; b < n && rc == PNP_OK; ++b) {
        const int k = b % nctx;
        const Workspace W = carve(g, (char*)workspace + (int64_t)k * ctx_bytes, t, h, w, lq_format, out_mask);
        // (a 4:2:0 batch comes as its own descriptors: the pointers the two kinds share, then the planes)
        const pnp_clip_io io = yclips ? pnp_clip_io{nullptr, yclips[b].mvs_dev, yclips[b].par_dev, yclips[b].out_f32_dev, yclips[b].out_u8_dev} : clips[b];
        rc = ClipRun(g, flat, packed, io, lq_format, out_mask, slices + (int64_t)b * t, qps + (int64_t)b * t, base_qps + (int64_t)b * t,
                     W, t, h, w, nctx > 1 ? g->side_streams[k] : st, nctx == 1, yclips ? yclips + b : nullptr, yuv_standard).run();
    }
    if (nctx > 1) {      // join even after an error: the caller's stream must not run ahead of what was launched
        for (int k = 0; k < nctx; ++k) {
            hipError_t err = hipEventRecord(g->join_events[k], g->side_streams[k]);
            if (err == hipSuccess) err = hipStreamWaitEvent(st, g->join_events[k], 0);
            if (err != hipSuccess && rc == PNP_OK) rc = (int)err;
        }
    }
    return rc;
}

// The body behind the two 4:2:0 entries (the scheduler's 4:2:0 frame format: the workspace holds fp32 frames only, so its layout does
// not know the sample size): what only these entries can get wrong, in front of everything else (no HIP call has been made).
int forward_clips_yuv(const pnp_generator* g, const float* flat, const float* packed, const std::vector<YuvClip>& clips, int yuv_standard,
                      int out_mask, const float* slices, const float* qps, const float* base_qps, void* workspace, int64_t workspace_bytes, int t,
                      int h, int w, hipStream_t st) {
    YuvCoef k;
    if (!g || !yuv_coef(yuv_standard, 8, 0, &k) || out_mask < 1 || out_mask > (PNP_OUT_F32 | PNP_OUT_U8 | PNP_OUT_YUV420)) return PNP_ERR_BAD_ARG;
    if (!yuv_frame_ok(k.format, 1, h, w)) return PNP_ERR_BAD_ARG;      // (the format's parity rules: sx divides w, sy divides h)
    const int os = g->cfg.vsr ? 4 : 1;
    for (const YuvClip& c : clips) {
        if (!yuv_planes_ok(c.lq, w, k.format) || !c.mvs_dev || !c.par_dev) return PNP_ERR_BAD_ARG;
        if ((out_mask & PNP_OUT_F32) && !c.out_f32_dev) return PNP_ERR_BAD_ARG;
        const uintptr_t amask = g->any_size ? 0 : 3;      // (the byte output's rule of pnp_generator_forward_clips)
        if ((out_mask & PNP_OUT_U8) && (!c.out_u8_dev || (reinterpret_cast<uintptr_t>(c.out_u8_dev) & amask))) return PNP_ERR_BAD_ARG;
        if ((out_mask & PNP_OUT_YUV420) && !yuv_planes_ok(c.out, w * os, k.format)) return PNP_ERR_BAD_ARG;
    }
    return forward_batch(g, flat, packed, nullptr, (int)clips.size(), FRAMES_YUV420, out_mask, slices, qps, base_qps, workspace, workspace_bytes, t, h,
                         w, st, clips.data(), yuv_standard);
}

}  // namespace

extern "C" {

int64_t pnp_generator_workspace_bytes_io(const pnp_generator* g, int t, int h, int w, int lq_format, int out_mask) {
    if (!g || !io_args_ok(lq_format, out_mask)) return -1;
    int R, L;
    if (bounded_mode(g, t) && !plan_pick(t, g->cfg.with_cat, g->max_resident, &R, &L)) return -1;
    return carve(g, nullptr, t, h, w, lq_format, out_mask).bytes;
}

int pnp_generator_forward(const pnp_generator* g, const float* flat, const float* packed, const float* lrs,
                          const float* mvs, const float* par, const float* slices, const float* qps,
                          const float* base_qps, float* out, void* workspace, int64_t workspace_bytes, int n, int t,
                          int h, int w, void* stream_) {
    // (its own errors first, as ever: they are decided before a pointer of the batch is touched, and callers probe them with null buffers)
    const int bad = forward_check(g, n, t, h, w, PNP_FRAMES_F32_NCHW, PNP_OUT_F32, workspace, workspace_bytes);
    if (bad) return bad;
    // n descriptors from the strides: sample b of every tensor
    const int64_t hw = (int64_t)h * w, os = g->cfg.vsr ? 4 : 1;
    std::vector<pnp_clip_io> clips(n);
    for (int b = 0; b < n; ++b)
        clips[b] = pnp_clip_io{lrs + (int64_t)b * t * 3 * hw, mvs + (int64_t)b * t * 4 * hw, par + (int64_t)b * t * 3 * hw,
                               out + (int64_t)b * t * 3 * hw * os * os, nullptr};
    return forward_batch(g, flat, packed, clips.data(), n, PNP_FRAMES_F32_NCHW, PNP_OUT_F32, slices, qps, base_qps, workspace, workspace_bytes,
                         t, h, w, (hipStream_t)stream_);
}

int pnp_generator_forward_clips(const pnp_generator* g, const float* flat, const float* packed, const pnp_clip_io* clips, int n,
                                int lq_format, int out_mask, const float* slices, const float* qps, const float* base_qps,
                                void* workspace, int64_t workspace_bytes, int t, int h, int w, void* stream_) {
    // what only this entry can get wrong, in front of everything else (no HIP call has been made)
    if (!g || !clips || n < 1 || !io_args_ok(lq_format, out_mask)) return PNP_ERR_BAD_ARG;
    for (int b = 0; b < n; ++b) {
        const pnp_clip_io& c = clips[b];
        if (!c.lq_dev || !c.mvs_dev || !c.par_dev) return PNP_ERR_BAD_ARG;
        if ((out_mask & PNP_OUT_F32) && !c.out_f32_dev) return PNP_ERR_BAD_ARG;
        // (any_size: a clip of t*h*w*3 bytes inside a batch starts at any byte address; the kernels then read and write bytes there)
        const uintptr_t amask = g->any_size ? 0 : 3;
        if ((out_mask & PNP_OUT_U8) && (!c.out_u8_dev || (reinterpret_cast<uintptr_t>(c.out_u8_dev) & amask))) return PNP_ERR_BAD_ARG;
        if (lq_format == PNP_FRAMES_U8_HWC && (reinterpret_cast<uintptr_t>(c.lq_dev) & amask)) return PNP_ERR_BAD_ARG;
    }
    return forward_batch(g, flat, packed, clips, n, lq_format, out_mask, slices, qps, base_qps, workspace, workspace_bytes, t, h, w,
                         (hipStream_t)stream_);
}

int64_t pnp_generator_workspace_bytes_yuv(const pnp_generator* g, int t, int h, int w, int out_mask) {
    if (!g || out_mask < 1 || out_mask > (PNP_OUT_F32 | PNP_OUT_U8 | PNP_OUT_YUV420)) return -1;
    int R, L;
    if (bounded_mode(g, t) && !plan_pick(t, g->cfg.with_cat, g->max_resident, &R, &L)) return -1;
    return carve(g, nullptr, t, h, w, FRAMES_YUV420, out_mask).bytes;
}

int pnp_generator_forward_clips_yuv(const pnp_generator* g, const float* flat, const float* packed, const pnp_clip_yuv* clips, int n,
                                    int yuv_standard, int out_mask, const float* slices, const float* qps, const float* base_qps,
                                    void* workspace, int64_t workspace_bytes, int t, int h, int w, void* stream_) {
    if (!clips || n < 1) return PNP_ERR_BAD_ARG;      // (what the conversion itself needs; everything else is forward_clips_yuv's to refuse)
    std::vector<YuvClip> y(n);
    for (int b = 0; b < n; ++b) {
        const pnp_clip_yuv& c = clips[b];
        y[b] = YuvClip{yuv_planes(c.lq), yuv_planes(c.out_yuv), c.mvs_dev, c.par_dev, c.out_f32_dev, c.out_u8_dev};
    }
    return forward_clips_yuv(g, flat, packed, y, yuv_standard, out_mask, slices, qps, base_qps, workspace, workspace_bytes, t, h, w, (hipStream_t)stream_);
}

int pnp_generator_forward_clips_yuv16(const pnp_generator* g, const float* flat, const float* packed, const pnp_clip_yuv16* clips, int n,
                                      int yuv_standard, int out_mask, const float* slices, const float* qps, const float* base_qps,
                                      void* workspace, int64_t workspace_bytes, int t, int h, int w, void* stream_) {
    if (!clips || n < 1) return PNP_ERR_BAD_ARG;      // (what the conversion itself needs; everything else is forward_clips_yuv's to refuse)
    std::vector<YuvClip> y(n);
    for (int b = 0; b < n; ++b) {
        const pnp_clip_yuv16& c = clips[b];
        y[b] = YuvClip{yuv_planes(c.lq), yuv_planes(c.out_yuv16), c.mvs_dev, c.par_dev, c.out_f32_dev, c.out_u8_dev};
    }
    return forward_clips_yuv(g, flat, packed, y, yuv_standard, out_mask, slices, qps, base_qps, workspace, workspace_bytes, t, h, w, (hipStream_t)stream_);
}

int pnp_generator_profile(pnp_generator* g, int enable) {
    if (!g) return PNP_ERR_BAD_ARG;
    g->prof_on = enable != 0;
    g->prof_used = 0;
    g->prof_recs.clear();
    g->prof_last = nullptr;
    return PNP_OK;
}

int pnp_generator_profile_read(pnp_generator* g, int kind, double* total_ms, int64_t* launches, double* work) {
    if (!g || !total_ms || !launches || !work) return PNP_ERR_BAD_ARG;
    double ms = 0, wk = 0;
    int64_t n = 0;
    for (const ProfRec& r : g->prof_recs) {
        if (r.kind != kind) continue;
        hipError_t e = hipEventSynchronize(r.b);
        if (e != hipSuccess) return (int)e;
        float f = 0.f;
        e = hipEventElapsedTime(&f, r.a, r.b);
        if (e != hipSuccess) return (int)e;
        ms += f;
        wk += r.work;
        ++n;
    }
    *total_ms = ms;
    *launches = n;
    *work = wk;
    return PNP_OK;
}

}  // extern "C"
