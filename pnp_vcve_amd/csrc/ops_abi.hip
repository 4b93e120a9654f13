// Stand-alone op entry points of the C ABI (include/pnpvcve.h, pnpvcve_debug.h): one kernel family each, addressed directly
// by the op-level tests, benches and the PyTorch glue.  Independent of pnp_generator (generator.hip).
#include <cstring>

#include "../../include/pnpvcve.h"
#include "../../include/pnpvcve_debug.h"
#include "abi_shared.h"
#include "conv_mfma.h"
#include "warp.h"
#include "dcn.h"

namespace {

// What the stand-alone conv ops fill alike: the sources of the virtual concat, the partition planes, the epilogue and the frame.
// Each op adds the weight images of its kernel family and its own switches.
ConvArgs op_conv_args(int nsrc, const float* const* srcs, const int* src_channels, const float* bias, const float* gamma, const float* par,
                      const int* par_flags, const float* residual, int act, float* out, int h, int w, void* trace) {
    ConvArgs a;
    memset(&a, 0, sizeof(a));
    a.nsrc = nsrc;
    for (int s = 0; s < nsrc; ++s) {
        a.src[s] = srcs[s];
        a.src_c[s] = src_channels[s];
    }
    a.par = par;
    a.par_flags = par_flags;
    a.par_plane = (long)h * w;
    a.bias = bias;
    a.gamma = gamma;
    a.residual = residual;
    a.out = out;
    a.H = h;
    a.W = w;
    a.act = act;
    a.dbg = (unsigned long long*)trace;
    return a;
}

}  // namespace

extern "C" {

// the clip scheduler's byte-frame unpacking alone: any_size 0 = the aligned, whole-group form with its refusals, 1 = any address and count
int pnp_debug_pack_lr_u8(const unsigned char* lq, float* lr4, int t, int h, int w, int any_size, void* st) {
    if (!lq || !lr4 || t < 1 || h < 1 || w < 1) return PNP_ERR_BAD_ARG;
    return any_size ? launch_pack_lr_u8_any(lq, lr4, t, h, w, (hipStream_t)st) : launch_pack_lr_u8(lq, lr4, t, h, w, (hipStream_t)st);
}

int pnp_flow_warp_nchw_f32(const float* x, const float* flow, float* out, int n, int c, int h, int w, void* st) {
    if (n < 1 || c < 1 || h < 1 || w < 1) return PNP_ERR_BAD_ARG;
    return launch_flow_warp_nchw(x, flow, out, n, c, h, w, (hipStream_t)st);
}

int pnp_flow_warp_nchw_mode_f32(const float* x, const float* flow, float* out, int n, int c, int h, int w, int mode, void* st) {
    if (n < 1 || c < 1 || h < 1 || w < 1 || mode < 0 || mode > 1) return PNP_ERR_BAD_ARG;
    return launch_flow_warp_nchw(x, flow, out, n, c, h, w, (hipStream_t)st, mode == 1);
}

int pnp_mv_warp_nhwc_mode_f32(const float* feat, const float* fx, const float* fy, float* out, int h, int w, int c, int mode,
                              void* st) {
    if (h < 1 || w < 1 || c < 4 || mode < 0 || mode > 1) return PNP_ERR_BAD_ARG;
    return launch_mv_warp_nhwc(feat, fx, fy, out, h, w, c, (hipStream_t)st, false, mode == 1);
}

int pnp_mv_warp_nhwc_f32(const float* feat, const float* fx, const float* fy, float* out, int h, int w, int c,
                         void* st) {
    if (h < 1 || w < 1 || c < 4) return PNP_ERR_BAD_ARG;
    return launch_mv_warp_nhwc(feat, fx, fy, out, h, w, c, (hipStream_t)st);
}

int pnp_nchw_to_nhwc_f32(const float* in, float* out, int n, int c, int h, int w, void* st) {
    return launch_nchw_to_nhwc(in, out, n, c, h, w, (hipStream_t)st);
}

int pnp_nhwc_to_nchw_f32(const float* in, float* out, int n, int c, int h, int w, void* st) {
    return launch_nhwc_to_nchw(in, out, n, c, h, w, (hipStream_t)st);
}

int pnp_caa_predict_f32(const float* q_ew, const float* q_g, int count, int E, int softmax, const float* w1,
                        const float* b1, const float* w2, const float* b2, const float* v1, const float* v2,
                        float* ew, float* gamma, void* st) {
    for (int t0 = 0; t0 < count; t0 += 32) {
        CaaArgs a;
        memset(&a, 0, sizeof(a));
        a.count = (count - t0 < 32) ? count - t0 : 32;
        for (int i = 0; i < a.count; ++i) {
            a.q_ew[i] = q_ew[t0 + i];
            a.q_g[i] = q_g[t0 + i];
        }
        a.t0 = t0;
        a.E = E;
        a.softmax = softmax;
        a.with_se = (v1 && v2) ? 1 : 0;
        a.w1 = w1;
        a.b1 = b1;
        a.w2 = w2;
        a.b2 = b2;
        a.v1 = v1;
        a.v2 = v2;
        a.ew = ew;
        a.gamma = gamma;
        const int rc = launch_caa_predict(a, (hipStream_t)st);
        if (rc) return rc;
    }
    return PNP_OK;
}

int pnp_dcn_nhwc_f32(const float* x, const float* om, const float* fx, const float* fy, const float* w_packed,
                     const float* bias, float* out, int h, int w, void* st) {
    return pnp_dcn_nhwc_f32_ex(x, om, fx, fy, w_packed, bias, out, h, w, nullptr, st);
}

int pnp_dcn_f16_image_from_f32(const float* w_packed, void* dst, void* st) {
    if (!w_packed || !dst) return PNP_ERR_BAD_ARG;
    return launch_dcn_f16_image(w_packed, dst, (hipStream_t)st);
}

int pnp_dcn_nhwc_f16(const float* x, const float* om, const float* fx, const float* fy, const void* w_f16,
                     const float* bias, float* out, int h, int w, void* st) {
    if (h < 1 || w < 1 || !w_f16) return PNP_ERR_BAD_ARG;
    DcnArgs d;
    d.dbg = nullptr;
    d.x = x;
    d.om = om;
    d.fx = fx;
    d.fy = fy;
    d.w = nullptr;
    d.w16 = w_f16;
    d.bias = bias;
    d.out = out;
    d.H = h;
    d.W = w;
    return launch_dcn(d, (hipStream_t)st);
}

int pnp_dcn_nhwc_f32_ex(const float* x, const float* om, const float* fx, const float* fy, const float* w_packed,
                        const float* bias, float* out, int h, int w, void* trace, void* st) {
    if (h < 1 || w < 1) return PNP_ERR_BAD_ARG;
    DcnArgs d;
    d.w16 = nullptr;
    d.dbg = (unsigned long long*)trace;
    d.x = x;
    d.om = om;
    d.fx = fx;
    d.fy = fy;
    d.w = w_packed;
    d.bias = bias;
    d.out = out;
    d.H = h;
    d.W = w;
    return launch_dcn(d, (hipStream_t)st);
}

int pnp_dcn_ref_channel(int packed_channel) { return pnp_dcn_ref_channel_impl(packed_channel); }

int pnp_dcn_trace_u64s(void) { return dcn_trace_u64s(); }

int64_t pnp_packed_conv_floats(int csrc) { return csrc == 64 ? IMG_WIDE : IMG_CHUNK; }

int pnp_pack_conv3x3_f32(const float* w, const float* ew, int E, int cout, int cin_total, int cbase, int csrc,
                         float* dst, void* st) {
    if (cout > 64 || (csrc != 64 && csrc != 3) || E < 1) return PNP_ERR_BAD_ARG;
    PackArgs a = plain_pack(w, cin_total, 9, csrc == 64 ? PACK_WIDE : PACK_RGB4, cbase, 2, cout, dst);
    a.E = E;
    a.ew = ew;
    a.e_stride = (long)cout * cin_total * 9;
    if (E > 1 && !ew) return PNP_ERR_BAD_ARG;
    return launch_pack_weights(a, 1, (hipStream_t)st);
}

int pnp_pack_conv1x1_f32(const float* w, float* dst, void* st) {
    return launch_pack_weights(plain_pack(w, 64, 1, PACK_1X1, 0, 2, 64, dst), 1, (hipStream_t)st);
}

int64_t pnp_wino_image_floats(void) { return PNP_WINO_IMG_FLOATS; }
int64_t pnp_wino_par_image_floats(void) { return PNP_WINO_PAR_FLOATS; }

int64_t pnp_wino_rgb_image_floats(void) { return PNP_WINO_RGB_FLOATS; }

int pnp_wino_rgb_image_from_packed_f32(const float* packed_rgb_chunk, float* dst, void* st) {
    return launch_wino_rgb_image(packed_rgb_chunk, dst, (hipStream_t)st);
}

static int wino_ms_op(int nsrc, const float* const* srcs, const float* const* wino_w, const float* bias, int act, float* out,
                      int h, int w, int units, void* st);

static int g_debug_wino_row0 = 0, g_debug_wino_rows = 0;
static void* g_debug_wino_ms_trace = nullptr;
int pnp_debug_wino_ms_trace(void* trace_dev) {
    g_debug_wino_ms_trace = trace_dev;
    return 0;
}
int pnp_debug_wino_tile_rows(int row0, int nrows) {
    if (row0 < 0 || nrows < 0) return PNP_ERR_BAD_ARG;
    g_debug_wino_row0 = row0;
    g_debug_wino_rows = nrows;
    return 0;
}

int pnp_conv3x3_wino_ms_f32(int nsrc, const float* const* srcs, const float* const* wino_w, const float* bias, int act, float* out,
                            int h, int w, void* st) {
    return wino_ms_op(nsrc, srcs, wino_w, bias, act, out, h, w, 0, st);
}

int pnp_conv3x3_wino_ms_units_f32(int nsrc, const float* const* srcs, const float* const* wino_w, const float* bias, int act,
                                  float* out, int h, int w, void* st) {
    return wino_ms_op(nsrc, srcs, wino_w, bias, act, out, h, w, 1, st);
}

static int wino_ms_op(int nsrc, const float* const* srcs, const float* const* wino_w, const float* bias, int act, float* out,
                      int h, int w, int units, void* st) {
    if (nsrc < 2 || nsrc > 4 || !srcs || !wino_w || !out || act < 0 || act > 2) return PNP_ERR_BAD_ARG;
    if (!op_map_fits(h, w)) return PNP_ERR_UNSUPPORTED;
    static const int channels[4] = {4, 64, 64, 64};
    ConvArgs a = op_conv_args(nsrc, srcs, channels, bias, nullptr, nullptr, nullptr, nullptr, act, out, h, w, units ? nullptr : g_debug_wino_ms_trace);
    for (int s = 0; s < nsrc; ++s) {
        if (!srcs[s] || !wino_w[s]) return PNP_ERR_BAD_ARG;
        a.wwino_src[s] = wino_w[s];
    }
    a.wwino_rgb = wino_w[0];
    a.wino_units = units;
    if (!units) {
        a.tile_row0 = g_debug_wino_row0;
        a.tile_rows = g_debug_wino_rows;
    }
    if (!conv_wino_ms_eligible(a, CONV_CFG_BIG, 1)) return PNP_ERR_UNSUPPORTED;
    return launch_conv3x3_wino(a, (hipStream_t)st);
}

int pnp_wino_image_from_packed_f32(const float* packed_w, const float* gamma, float* dst, void* st) {
    return launch_wino_images(&packed_w, &dst, 1, gamma, (hipStream_t)st);
}

int pnp_wino_par_image_from_packed_f32(const float* packed_w1x1, float* dst, void* st) {
    return launch_wino_par_image(packed_w1x1, dst, (hipStream_t)st);
}

int pnp_conv3x3_wino_f32(const float* src, const float* wino_w, const float* bias, const float* gamma, const float* wino_w1x1,
                         const float* par, const int* par_flags, const float* residual, int act, float* out, int h, int w,
                         void* st) {
    return pnp_conv3x3_wino_f32_ex(src, wino_w, bias, gamma, wino_w1x1, par, par_flags, residual, act, out, h, w, nullptr, st);
}

int pnp_conv3x3_wino_units_f32(const float* src, const float* wino_w, const float* bias, const float* gamma, const float* wino_w1x1,
                               const float* par, const int* par_flags, const float* residual, int act, float* out, int h, int w,
                               void* st) {
    // (trace = this function's own address: the marker pnp_conv3x3_wino_f32_ex reads as "quadrant-unit kernel, no timeline")
    return pnp_conv3x3_wino_f32_ex(src, wino_w, bias, gamma, wino_w1x1, par, par_flags, residual, act, out, h, w,
                                   (void*)&pnp_conv3x3_wino_units_f32, st);
}

static const int* g_debug_wino_gate_word = nullptr;
int pnp_debug_wino_gate_word(const int* gate_word_dev) {
    g_debug_wino_gate_word = gate_word_dev;
    return 0;
}

int pnp_debug_par_fold_table(const float* par, void* table, int h, int w, void* st) {
    if (!par || !table || h < 1 || w < 1) return PNP_ERR_BAD_ARG;
    return launch_par_fold_table(par, (long)h * w, static_cast<PnpFoldRec*>(table), 1, h, w, (hipStream_t)st);
}

// The fold-only body of the gated launch reads the frame's fold table (ConvArgs::fold_tab), which the clip scheduler makes in its
// workspace in front of every branch run.  This stand-alone entry reaches the gated launch under the test hook above only and has no
// workspace: it keeps one table per device, grown on demand, and makes it again on every such call, on the call's stream in front of
// the conv.  Like the hook itself this is process-wide and for one stream at a time.
static int debug_fold_table(const float* par, int h, int w, hipStream_t st, const PnpFoldRec** out) {
    static std::mutex mu;
    static PnpFoldRec* tab[PnpPerDevice::MAXDEV] = {};
    static long cap[PnpPerDevice::MAXDEV] = {};
    int dev = 0;
    PNP_CHECK(hipGetDevice(&dev));
    if (dev < 0 || dev >= PnpPerDevice::MAXDEV) return PNP_ERR_UNSUPPORTED;
    std::lock_guard<std::mutex> lock(mu);
    const long need = pnp_fold_records(h, w);
    if (cap[dev] < need) {
        if (tab[dev]) PNP_CHECK(hipFree(tab[dev]));       // (waits for the device: no launch still reads the old table)
        tab[dev] = nullptr, cap[dev] = 0;
        PNP_CHECK(hipMalloc(reinterpret_cast<void**>(&tab[dev]), (size_t)need * sizeof(PnpFoldRec)));
        cap[dev] = need;
    }
    *out = tab[dev];
    return launch_par_fold_table(par, (long)h * w, tab[dev], 1, h, w, st);
}

int pnp_conv3x3_wino_f32_ex(const float* src, const float* wino_w, const float* bias, const float* gamma, const float* wino_w1x1,
                            const float* par, const int* par_flags, const float* residual, int act, float* out, int h, int w,
                            void* trace, void* st) {
    if (!src || !wino_w || !out || act < 0 || act > 2 || (wino_w1x1 && !par)) return PNP_ERR_BAD_ARG;
    if (!op_map_fits(h, w)) return PNP_ERR_UNSUPPORTED;
    const int channels = 64;
    const bool units = trace == (void*)&pnp_conv3x3_wino_units_f32;
    ConvArgs a = op_conv_args(1, &src, &channels, bias, gamma, wino_w1x1 ? par : nullptr, wino_w1x1 ? par_flags : nullptr, residual, act,
                              out, h, w, units ? nullptr : trace);
    a.wwino = wino_w;
    a.wwino_par = wino_w1x1;
    a.wpar = wino_w1x1;              // "has branches"; the direct-form image itself is not read on this path
    a.par_any = (wino_w1x1 && par_flags) ? g_debug_wino_gate_word : nullptr;
    a.wino_units = units ? 1 : 0;
    if (!units) {
        a.tile_row0 = g_debug_wino_row0;
        a.tile_rows = g_debug_wino_rows;
    }
    if (!conv_wino_eligible(a, CONV_CFG_BIG, 1)) return PNP_ERR_UNSUPPORTED;
    if (a.par_any && !units) {
        const int rc = debug_fold_table(par, h, w, (hipStream_t)st, &a.fold_tab);
        if (rc) return rc;
    }
    return launch_conv3x3_wino(a, (hipStream_t)st);
}

int pnp_conv3x3_f32(int nsrc, const float* const* srcs, const int* src_channels, const float* const* packed_w,
                    const float* bias, const float* gamma, const float* packed_w1x1, const float* par,
                    const float* residual, int act, float* out, int h, int w, void* st) {
    return pnp_conv3x3_f32_ex(nsrc, srcs, src_channels, packed_w, bias, gamma, packed_w1x1, par, residual, act, out, h, w,
                              PNP_CONV_AUTO, nullptr, nullptr, st);
}

int pnp_conv3x3_f32_ex(int nsrc, const float* const* srcs, const int* src_channels, const float* const* packed_w,
                       const float* bias, const float* gamma, const float* packed_w1x1, const float* par,
                       const float* residual, int act, float* out, int h, int w, int variant, const int* par_flags,
                       void* trace, void* st) {
    if (nsrc < 1 || nsrc > 4) return PNP_ERR_BAD_ARG;
    if (!op_map_fits(h, w)) return PNP_ERR_UNSUPPORTED;      // 32-bit byte offsets into a map
    if (variant != PNP_CONV_AUTO && variant != PNP_CONV_TILE && variant != PNP_CONV_TILE_BIG) return PNP_ERR_BAD_ARG;
    ConvArgs a = op_conv_args(nsrc, srcs, src_channels, bias, gamma, par, par_flags, residual, act, out, h, w, trace);
    for (int s = 0; s < nsrc; ++s) a.wsrc[s] = packed_w[s];
    a.wpar = packed_w1x1;
    a.no_persist = variant != PNP_CONV_AUTO;
    return launch_conv3x3(a, variant == PNP_CONV_TILE_BIG ? CONV_CFG_BIG : conv_pick_cfg(h, w), 1, (hipStream_t)st);
}

// ResidualBlockNoBNDynamic_drt.forward, channel_first / one_layer branch (sr_backbone_utils.py:305-313,329): two fused-conv
// launches with the intermediate in caller scratch.
int pnp_bae_block_f32(const float* x, const float* w2_packed, const float* b2, const float* gamma, const float* w1x1_packed,
                      const float* par, const float* w1_packed, const float* b1, float* scratch, float* out, int h, int w,
                      void* st) {
    if (!x || !w2_packed || !w1_packed || !scratch || !out || h < 1 || w < 1) return PNP_ERR_BAD_ARG;
    if ((w1x1_packed == nullptr) != (par == nullptr)) return PNP_ERR_BAD_ARG;
    const float* src[1] = {x};
    const int sc[1] = {64};
    const float* wp[1] = {w2_packed};
    int rc = pnp_conv3x3_f32(1, src, sc, wp, b2, gamma, w1x1_packed, par, nullptr, 1, scratch, h, w, st);
    if (rc) return rc;
    src[0] = scratch;
    wp[0] = w1_packed;
    return pnp_conv3x3_f32(1, src, sc, wp, b1, nullptr, nullptr, nullptr, x, 0, out, h, w, st);
}

// PixelShufflePack (common/upsample.py:40-51): conv3x3 64 -> 256 + F.pixel_shuffle(2), as 4 sub-pixel convs whose
// output-channel order is permuted at pack time so that every sub-pixel is a contiguous 64-channel pixel row.
int64_t pnp_packed_pixel_shuffle_floats(void) { return 4 * IMG_WIDE + 256; }

int pnp_pack_pixel_shuffle_f32(const float* w, const float* b, float* dst, void* st_) {
    hipStream_t st = (hipStream_t)st_;
    if (!w || !b || !dst) return PNP_ERR_BAD_ARG;
    WeightImage sub[4];
    pixel_shuffle_images(0, 0, sub);
    for (const WeightImage& r : sub) {
        const int rc = pack_weight_image(r, w, dst, nullptr, st);
        if (rc) return rc;
    }
    return launch_small_copy(b, dst + 4 * IMG_WIDE, 256, 256, PNP_COPY_PIXEL_SHUFFLE_BIAS, st);
}

int pnp_pixel_shuffle_conv_f32(const float* x, const float* packed, int act, float* out, int h, int w, void* st) {
    if (!x || !packed || !out || h < 1 || w < 1 || act < 0 || act > 2) return PNP_ERR_BAD_ARG;
    if ((int64_t)h * w * 4 * 256 >= (int64_t)1 << 32) return PNP_ERR_UNSUPPORTED;
    const int channels = 64;
    ConvArgs a = op_conv_args(1, &x, &channels, packed + 4 * IMG_WIDE, nullptr, nullptr, nullptr, nullptr, act, out, h, w, nullptr);
    a.wsrc[0] = packed;
    a.w_ystride = IMG_WIDE;
    a.bias_ystride = 64;
    a.out_mode = 1;
    return launch_conv3x3(a, conv_pick_cfg(h, w), 4, (hipStream_t)st);
}

// pnpvcve_debug.h: the reconstruction head's two conv forms alone (generator.hip head()), ConvArgs filled as Clip::conv_args fills
// them for those calls, handed to the launch_* functions Clip::conv hands them to.  An explicit route runs iff the project's own
// predicate selects it for exactly these arguments; nothing is rerouted.

// the pixel-shuffle conv: ConvCall(h, w, cfg).source(x, 64, up_img).bias(up_bias, 64).act(act).mode(1, 4, IMG_WIDE).to(out).f16_map(..)
int pnp_debug_pixel_shuffle_conv(const void* x, int x_f16, const float* packed, const void* twin, int twin_kind, int act, void* out,
                                 int out_f16, int h, int w, int route, int* tile_queue, void* st) {
    if (!x || !packed || !out || h < 1 || w < 1 || act < 0 || act > 2) return PNP_ERR_BAD_ARG;
    if (twin_kind < 0 || twin_kind > 2 || (twin_kind != 0) != (twin != nullptr)) return PNP_ERR_BAD_ARG;
    if (route != PNP_HEAD_AUTO && route != PNP_HEAD_F32 && route != PNP_HEAD_F16 && route != PNP_HEAD_F16X3) return PNP_ERR_BAD_ARG;
    if ((int64_t)h * w * 4 * 256 >= (int64_t)1 << 32) return PNP_ERR_UNSUPPORTED;      // 32-bit byte offsets into the (2h, 2w, 64) map
    const int channels = 64, cfg = conv_pick_cfg(h, w);
    const float* src = reinterpret_cast<const float*>(x);
    ConvArgs a = op_conv_args(1, &src, &channels, packed + 4 * IMG_WIDE, nullptr, nullptr, nullptr, nullptr, act, reinterpret_cast<float*>(out), h, w,
                              nullptr);
    a.wsrc[0] = packed;
    a.wsrc_h[0] = twin;
    a.w_ystride = IMG_WIDE;
    a.bias_ystride = 64;
    a.out_mode = 1;
    a.out_cstride = 448;
    a.src_f16 = x_f16 ? 1 : 0;
    a.out_f16 = out_f16 ? 1 : 0;
    a.tile_queue = twin_kind == 2 ? tile_queue : nullptr;
    a.prec = route == PNP_HEAD_F32 ? 0 : twin_kind;      // (the generator's precision is the kind of twin its packed buffer carries)
    if (a.tile_queue) {      // as pnp_conv3x3_f16x3_ex: a queue that is not all zero would end the blocks' walk early
        const int rc = launch_fill(reinterpret_cast<float*>(a.tile_queue), 0.0f, 16, (hipStream_t)st);
        if (rc) return rc;
    }
    switch (route) {
        case PNP_HEAD_AUTO: return launch_conv3x3(a, cfg, 4, (hipStream_t)st);
        case PNP_HEAD_F32:       // (launch_conv3x3's order: no other fp32 kernel may claim the launch in front of the tile kernel)
            if (a.src_f16 || a.out_f16 || conv_wino_eligible(a, cfg, 4) || conv_wino_ms_eligible(a, cfg, 4) || conv_last_valu_eligible(a, cfg, 4) ||
                conv_persist_eligible(a, cfg, 4))
                return PNP_ERR_UNSUPPORTED;
            return launch_conv3x3(a, cfg, 4, (hipStream_t)st);
        case PNP_HEAD_F16:
            if (twin_kind != 1 || !conv_f16_eligible(a, cfg, 4)) return PNP_ERR_UNSUPPORTED;
            return launch_conv3x3_f16(a, 4, (hipStream_t)st);
        default:
            if (twin_kind != 2 || !conv_f16x3_eligible(a, cfg, 4)) return PNP_ERR_UNSUPPORTED;
            return launch_conv3x3_f16x3(a, cfg, (hipStream_t)st);
    }
}

// conv_last's weights as pnp_generator_pack lays them out: [IMG_RGB image | 32-float bias | [9][64][4] vector-ALU layout | fp16 twin]
static constexpr int64_t LAST_BIAS = IMG_RGB, LAST_VALU = LAST_BIAS + 32, LAST_TWIN = LAST_VALU + 9 * 64 * 4;
int64_t pnp_debug_conv_last_packed_floats(void) { return LAST_TWIN + IMG_RGB / 2; }

int pnp_debug_pack_conv_last(const float* w, const float* b, float* dst, void* st_) {
    hipStream_t st = (hipStream_t)st_;
    if (!w || !b || !dst) return PNP_ERR_BAD_ARG;
    int rc = pack_weight_image(WeightImage{0, 0, 64, 9, PACK_WIDE, 0, 1, 3}, w, dst, nullptr, st);     // ONE 32-channel N tile per k-step, 3 valid
    if (!rc) rc = launch_small_copy(b, dst + LAST_BIAS, 3, 32, PNP_COPY_PAD, st);
    if (!rc) rc = launch_pack_last_valu(w, dst + LAST_VALU, st);
    if (!rc) rc = launch_f16_image(dst, dst + LAST_TWIN, 9, 1, st);
    return rc;
}

// conv_last: ConvCall(H, W, CONV_CFG_RGB).source(src, 64, last_img).bias(last_bias).mode(2 | 3).rgb(lr, plane, last_valu)
//                .rgb8(lr8, out8).rgb0(lr0).to(out).f16_map(..)
int pnp_debug_conv_last(const void* src, int src_f16, const float* packed, int prec, int act, int out_mode, const void* frame,
                        int frame_form, float* out, unsigned char* out_u8, int H, int W, int route, void* st) {
    if (!src || !packed || !frame || (!out && !out_u8) || H < 1 || W < 1 || act < 0 || act > 2) return PNP_ERR_BAD_ARG;
    if ((out_mode != 2 && out_mode != 3) || prec < 0 || prec > 2) return PNP_ERR_BAD_ARG;
    if (out_mode == 3 && ((H | W) & 3)) return PNP_ERR_BAD_ARG;      // the x4 heads: the frame is (H / 4, W / 4)
    if (frame_form != PNP_HEAD_FRAME_PLANES && frame_form != PNP_HEAD_FRAME_U8 && frame_form != PNP_HEAD_FRAME_RGB0) return PNP_ERR_BAD_ARG;
    if (route != PNP_HEAD_AUTO && route != PNP_HEAD_F32 && route != PNP_HEAD_F16 && route != PNP_HEAD_VALU) return PNP_ERR_BAD_ARG;
    if (!op_map_fits(H, W)) return PNP_ERR_UNSUPPORTED;      // 32-bit byte offsets into the source map
    const int channels = 64;
    const float* s = reinterpret_cast<const float*>(src);
    ConvArgs a = op_conv_args(1, &s, &channels, packed + LAST_BIAS, nullptr, nullptr, nullptr, nullptr, act, out, H, W, nullptr);
    a.wsrc[0] = packed;
    a.out_mode = out_mode;
    a.out_cstride = 448;
    a.src_f16 = src_f16 ? 1 : 0;
    a.lr_plane = out_mode == 3 ? (long)(H >> 2) * (W >> 2) : (long)H * W;
    if (frame_form == PNP_HEAD_FRAME_PLANES) a.lr = reinterpret_cast<const float*>(frame);
    if (frame_form == PNP_HEAD_FRAME_U8) a.lr_u8 = reinterpret_cast<const unsigned char*>(frame);
    if (frame_form == PNP_HEAD_FRAME_RGB0) a.lr_rgb0 = reinterpret_cast<const float*>(frame);
    a.out_u8 = out_u8;
    const bool io = a.lr_u8 || a.out_u8 || a.lr_rgb0;      // Clip::conv: the byte boundary goes to launch_conv_last_io
    a.prec = route == PNP_HEAD_AUTO ? prec : (route == PNP_HEAD_F16 ? 1 : 0);
    a.wsrc_h[0] = a.prec == 1 ? (const void*)(packed + LAST_TWIN) : nullptr;
    a.wvalu = route == PNP_HEAD_F32 ? nullptr : packed + LAST_VALU;
    switch (route) {
        case PNP_HEAD_AUTO:
            if (io && prec == 1) return PNP_ERR_UNSUPPORTED;      // io_staged: the fp16 path keeps conv_last's fp32 interface
            return io ? launch_conv_last_io(a, (hipStream_t)st) : launch_conv3x3(a, CONV_CFG_RGB, 1, (hipStream_t)st);
        case PNP_HEAD_VALU:
            if (io) return launch_conv_last_io(a, (hipStream_t)st);      // (refuses by conv_last_valu_shape itself)
            if (!conv_last_valu_eligible(a, CONV_CFG_RGB, 1)) return PNP_ERR_UNSUPPORTED;
            return launch_conv_last_valu(a, (hipStream_t)st);
        case PNP_HEAD_F32:       // the fp32 MFMA RGB configuration: fp32 planes in and out only
            if (io || a.src_f16) return PNP_ERR_UNSUPPORTED;
            return launch_conv3x3(a, CONV_CFG_RGB, 1, (hipStream_t)st);
        default:
            if (io || !conv_f16_eligible(a, CONV_CFG_RGB, 1)) return PNP_ERR_UNSUPPORTED;
            return launch_conv3x3_f16(a, 1, (hipStream_t)st);
    }
}

int pnp_par_tile_flags_f32(const float* par, int* flags, int h, int w, void* st) {
    if (!par || !flags || h < 1 || w < 1) return PNP_ERR_BAD_ARG;
    return launch_par_tile_flags(par, (long)h * w, flags, 1, h, w, (hipStream_t)st);
}

int pnp_f16_image_from_f32(const float* packed_w, void* dst, int nchunks, void* st) {
    if (!packed_w || !dst) return PNP_ERR_BAD_ARG;
    return launch_f16_image(packed_w, dst, nchunks, 2, (hipStream_t)st);
}

int pnp_conv3x3_f16(int nsrc, const float* const* srcs, const int* src_channels, const void* const* packed_w_f16,
                    const float* bias, const float* gamma, const void* packed_w1x1_f16, const float* par,
                    const float* residual, int act, float* out, int h, int w, void* st) {
    return pnp_conv3x3_f16_ex(nsrc, srcs, src_channels, packed_w_f16, bias, gamma, packed_w1x1_f16, par, residual, act, out,
                              h, w, nullptr, st);
}

int pnp_conv3x3_f16_ex(int nsrc, const float* const* srcs, const int* src_channels, const void* const* packed_w_f16,
                       const float* bias, const float* gamma, const void* packed_w1x1_f16, const float* par,
                       const float* residual, int act, float* out, int h, int w, void* trace, void* st) {
    if (nsrc < 1 || nsrc > 4) return PNP_ERR_BAD_ARG;
    if (!op_map_fits(h, w)) return PNP_ERR_UNSUPPORTED;      // 32-bit byte offsets into a map
    ConvArgs a = op_conv_args(nsrc, srcs, src_channels, bias, gamma, par, nullptr, residual, act, out, h, w, trace);
    a.prec = 1;
    for (int s = 0; s < nsrc; ++s) a.wsrc_h[s] = packed_w_f16[s];
    a.wpar_h = packed_w1x1_f16;
    if (a.wpar_h && (nsrc != 1 || !par)) return PNP_ERR_BAD_ARG;
    if (!conv_f16_eligible(a, CONV_CFG_BIG, 1)) return PNP_ERR_UNSUPPORTED;
    return launch_conv3x3_f16(a, 1, (hipStream_t)st);
}

int pnp_f16x3_image_from_f32(const float* packed_w, void* dst, int nchunks, void* st) {
    if (!packed_w || !dst) return PNP_ERR_BAD_ARG;
    return launch_f16x3_image(packed_w, dst, nchunks, (hipStream_t)st);
}

int pnp_conv3x3_f16x3(int nsrc, const float* const* srcs, const int* src_channels, const float* const* packed_w_f32,
                      const void* const* packed_w_x3, const float* bias, const float* gamma, const void* packed_w1x1_x3,
                      const float* par, const int* par_flags, const float* residual, int act, float* out, int h, int w, void* st) {
    return pnp_conv3x3_f16x3_ex(nsrc, srcs, src_channels, packed_w_f32, packed_w_x3, bias, gamma, packed_w1x1_x3, par, par_flags,
                                residual, act, out, h, w, 0, nullptr, nullptr, st);
}

int pnp_conv3x3_f16x3_ex(int nsrc, const float* const* srcs, const int* src_channels, const float* const* packed_w_f32,
                         const void* const* packed_w_x3, const float* bias, const float* gamma, const void* packed_w1x1_x3,
                         const float* par, const int* par_flags, const float* residual, int act, float* out, int h, int w,
                         int w1x1_scaled, int* tile_queue, void* trace, void* st) {
    if (nsrc < 1 || nsrc > 4 || !srcs || !src_channels || !packed_w_x3 || !out) return PNP_ERR_BAD_ARG;
    if (!op_map_fits(h, w)) return PNP_ERR_UNSUPPORTED;      // 32-bit byte offsets into a map
    ConvArgs a = op_conv_args(nsrc, srcs, src_channels, bias, gamma, par, par_flags, residual, act, out, h, w, trace);
    a.prec = 2;
    for (int s = 0; s < nsrc; ++s) {
        a.wsrc[s] = packed_w_f32 ? packed_w_f32[s] : nullptr;
        a.wsrc_h[s] = packed_w_x3[s];
        if (src_channels[s] == 4 && (s != 0 || !a.wsrc[s])) return PNP_ERR_BAD_ARG;    // the RGB frame: source 0, fp32 image
    }
    a.wpar_h = packed_w1x1_x3;
    a.wpar_h_scaled = (packed_w1x1_x3 && w1x1_scaled) ? 1 : 0;
    a.tile_queue = tile_queue;
    // A queue that is not all zero on entry ends the blocks' walk early (tiles left unwritten, no error): zero it here instead of
    // trusting the caller -- a launch aborted in mid-clip would leave it dirty for this entry point
    if (tile_queue) {
        const int rc = launch_fill(reinterpret_cast<float*>(tile_queue), 0.0f, 16, (hipStream_t)st);
        if (rc) return rc;
    }
    if (a.wpar_h && (nsrc != 1 || !par)) return PNP_ERR_BAD_ARG;
    if (!conv_f16x3_eligible(a, CONV_CFG_BIG, 1)) return PNP_ERR_UNSUPPORTED;
    return launch_conv3x3_f16x3(a, conv_pick_cfg(h, w), (hipStream_t)st);
}

// pnpvcve_debug.h: the fp16-operand conv with explicit fp16 maps -- what pnp_generator_forward uses between its launches under
// PNP_OPT_F16_MAPS / PNP_OPT_F16_MIRRORS -- so that tests can address every kernel variant through the ABI.
int pnp_conv3x3_f16_maps(int nsrc, const void* const* srcs, const int* src_channels, int src_f16_mask,
                         const void* const* packed_w_f16, const float* bias, const float* gamma, const void* packed_w1x1_f16,
                         const float* par, const int* par_flags, const float* residual, int act, void* out, int out_f16,
                         void* out16, int h, int w, int chain, void* trace, void* st) {
    if (nsrc < 1 || nsrc > 4) return PNP_ERR_BAD_ARG;
    if (!op_map_fits(h, w)) return PNP_ERR_UNSUPPORTED;      // 32-bit byte offsets into a map
    ConvArgs a = op_conv_args(nsrc, reinterpret_cast<const float* const*>(srcs), src_channels, bias, gamma, par, par_flags, residual, act,
                              reinterpret_cast<float*>(out), h, w, trace);
    a.prec = 1;
    for (int s = 0; s < nsrc; ++s) a.wsrc_h[s] = packed_w_f16[s];
    a.src_f16 = src_f16_mask;
    a.out_f16 = out_f16 ? 1 : 0;
    a.out16 = out16;
    a.no_multi16 = chain ? 1 : 0;
    a.wpar_h = packed_w1x1_f16;
    if (a.wpar_h && (nsrc != 1 || !par)) return PNP_ERR_BAD_ARG;
    if (!conv_f16_eligible(a, CONV_CFG_BIG, 1)) return PNP_ERR_UNSUPPORTED;
    return launch_conv3x3_f16(a, 1, (hipStream_t)st);
}

int pnp_mv_warp_nhwc_f16out(const float* feat, const float* fx, const float* fy, void* out16, int h, int w, int c, void* st) {
    if (h < 1 || w < 1 || c < 4) return PNP_ERR_BAD_ARG;
    return launch_mv_warp_nhwc(feat, fx, fy, out16, h, w, c, (hipStream_t)st, true);
}

int pnp_mv_warp_nhwc_f16out_mode(const float* feat, const float* fx, const float* fy, void* out16, int h, int w, int c, int mode,
                                 void* st) {
    if (h < 1 || w < 1 || c < 4 || mode < 0 || mode > 1) return PNP_ERR_BAD_ARG;
    return launch_mv_warp_nhwc(feat, fx, fy, out16, h, w, c, (hipStream_t)st, true, mode == 1);
}

}  // extern "C"
