// Host-only run of the byte-frame boundary of the clip scheduler (pnp_generator_forward_clips) under AddressSanitizer / UBSan.
//
// TEST INFRASTRUCTURE.  Built by tests/test_byte_frames_host.py with a plain host compiler:
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -DPNP_HOST_STUB -Dmain=sched_stub_main
//         -x c++ tests/host/byte_frames_stub.cpp
// It reuses tests/host/sched_stub.cpp unchanged (recording launchers over csrc/generator.hip; its driver is renamed away).  The four
// launchers of the byte boundary are recorded by csrc/host_stub/io_stub.h; the hook below gives them the same range bookkeeping the
// other launchers have.  Two kinds of scenario, one JSON object each:
//   * "same": an fp32 batch through pnp_generator_forward, then the same batch as descriptors through pnp_generator_forward_clips with
//     (PNP_FRAMES_F32_NCHW, PNP_OUT_F32): the two ordered traces (sched_stub.cpp: every HIP call and launch with every argument) must be
//     identical, line for line;
//   * "io": clips in separately allocated buffers of exactly the sizes the ABI names (ASan's red zones are the poisoned gaps between
//     them), a format and an output mask: every read and write lies inside the owning clip's buffers, the pack launch reads exactly
//     t*h*w*3 bytes, the last conv writes exactly H*W*3 bytes per frame, only the requested outputs are written and no launch is handed
//     fp32 planes of a clip in byte mode.
#include "sched_stub.cpp"

namespace {

using namespace stub;

int n_pack = 0, n_from = 0, n_to = 0, n_last_io = 0;

void io_hook(const PnpStubIoLaunch& r) {
    trace_io(r);
    note_launch(r.stream);
    const size_t px = (size_t)r.frames * r.h * r.w;
    switch (r.kind) {
        case PNP_STUB_IO_PACK_LR_U8:
            cur = "launch_pack_lr_u8";
            ++n_pack;
            RD("the byte frames", r.in, px * 3);
            WR("the packed RGB0 frames", r.out, px * 16);
            break;
        case PNP_STUB_IO_FROM_RGB8:
            cur = "launch_frames_from_rgb8";
            ++n_from;
            RD("a byte frame", r.in, px * 3);
            WR("a frame of fp32 planes", r.out, px * 12);
            break;
        case PNP_STUB_IO_TO_RGB8:
            cur = "launch_frames_to_rgb8";
            ++n_to;
            RD("a frame of fp32 planes", r.in, px * 12);
            WR("a byte frame", r.out, px * 3);
            break;
        default: {
            cur = "launch_conv_last_io";
            ++n_last_io;
            const ConvArgs& a = r.conv;
            const size_t hw = (size_t)a.H * a.W, lhw = a.out_mode == 2 ? hw : hw / 16;
            RD("conv_last's source", a.src[0], hw * 256);
            RD("the vector-ALU conv_last weights", a.wvalu, 9 * 64 * 4 * 4);
            RD("the bias", a.bias, 3 * 4);
            if (a.lr_u8) RD("the low-quality frame's bytes", a.lr_u8, lhw * 3);
            else RD("the low-quality frame", a.lr, (size_t)(2 * a.lr_plane + lhw) * 4);
            if (a.out) WR("the output frame", a.out, hw * 12);
            if (a.out_u8) WR("the output frame's bytes", a.out_u8, hw * 3);
        }
    }
}

void reset() {
    errors.clear();
    written.clear();
    waits.clear();
    records.clear();
    launch_streams.clear();
    warps.clear();
    convs.clear();
    mixes.clear();
    pnp_stub_io_log.clear();
    dcn_calls = 0;
    n_pack = n_from = n_to = n_last_io = 0;
}

struct IoScenario {
    std::string name, kind;      // kind: "same" | "io"
    pnp_generator_cfg cfg;
    int prec, n, t, h, w, contexts, lq_format, out_mask, wino, last_valu, max_resident;
};

bool any_written(const void* p, size_t n) {
    const uintptr_t lo = (uintptr_t)p, hi = lo + n;
    for (const auto& iv : written)
        if (iv.first < hi && iv.second > lo) return true;
    return false;
}

void side_info(int n, int t, std::vector<float>& slices, std::vector<float>& qps, std::vector<float>& bqs) {
    for (int b = 0; b < n; ++b) {
        const std::vector<float> sl = pattern("IBBBP", t);
        for (int i = 0; i < t; ++i) {
            slices.push_back(sl[i]);
            qps.push_back((20.f + (float)((i * 7 + b) % 20)) / 255.f);
            bqs.push_back((b ? 35.f : 25.f) / 255.f);
        }
    }
}

int run_io(IoScenario sc) {
    reset();
    regions.clear();
    trace.clear();
    pnp_generator* g = nullptr;
    if (pnp_generator_create(&sc.cfg, &g)) return 2;
    pnp_generator_set_precision(g, sc.prec);
    pnp_generator_set_option(g, PNP_OPT_WINOGRAD, sc.wino);
    pnp_generator_set_option(g, PNP_OPT_CONV_LAST_VALU, sc.last_valu);
    if (sc.max_resident < 0) sc.max_resident = pnp_generator_min_resident(g, sc.t);
    pnp_generator_set_max_resident(g, sc.max_resident);
    const int t = sc.t, n = sc.n;
    const bool u8_in = sc.lq_format == PNP_FRAMES_U8_HWC;
    const int64_t flat_n = pnp_generator_flat_floats(g), packed_n = pnp_generator_packed_floats(g);
    const int64_t plain_bytes = pnp_generator_workspace_bytes(g, t, sc.h, sc.w);
    const int64_t ctx_bytes = pnp_generator_workspace_bytes_io(g, t, sc.h, sc.w, sc.lq_format, sc.out_mask);
    const int64_t ws_bytes = ctx_bytes * sc.contexts;
    const size_t hw = (size_t)sc.h * sc.w, os = sc.cfg.vsr ? 4 : 1;
    float* flat = (float*)malloc((size_t)flat_n * 4);
    float* packed = (float*)malloc((size_t)packed_n * 4);
    char* ws = nullptr;
    if (ws_bytes <= 0 || posix_memalign((void**)&ws, 256, (size_t)ws_bytes)) return 2;
    mark(flat, (size_t)flat_n * 4);
    region("flat", flat, (size_t)flat_n * 4);
    region("packed", packed, (size_t)packed_n * 4);
    region("ws", ws, (size_t)ws_bytes);
    std::vector<float> slices, qps, bqs;
    side_info(n, t, slices, qps, bqs);
    pnp_stub_stream caller{0};
    const int prc = pnp_generator_pack(g, flat, packed, &caller);
    pnp_stub_io_hook = io_hook;
    int frc = 0, same = -1;
    size_t first_diff = 0, list_len = 0;
    std::vector<pnp_clip_io> clips(n);
    std::vector<void*> owned;
    const size_t lq_bytes = (size_t)t * 3 * hw * (u8_in ? 1 : 4), out_px = (size_t)t * 3 * hw * os * os;
    if (sc.kind == "same") {
        // one contiguous batch, as pnp_generator_forward takes it; then descriptors of its samples
        float* lrs = (float*)malloc((size_t)n * t * 3 * hw * 4);
        float* mvs = (float*)malloc((size_t)n * t * 4 * hw * 4);
        float* par = (float*)malloc((size_t)n * t * 3 * hw * 4);
        float* out = (float*)malloc((size_t)n * out_px * 4);
        owned = {lrs, mvs, par, out};
        mark(lrs, (size_t)n * t * 3 * hw * 4);
        mark(mvs, (size_t)n * t * 4 * hw * 4);
        mark(par, (size_t)n * t * 3 * hw * 4);
        region("lrs", lrs, (size_t)n * t * 3 * hw * 4);
        region("mvs", mvs, (size_t)n * t * 4 * hw * 4);
        region("par", par, (size_t)n * t * 3 * hw * 4);
        region("out", out, (size_t)n * out_px * 4);
        const auto before = written;
        // (a first forward makes the handle's streams and events as it goes, and a chain's join event is "the last one made so far": the
        //  two forwards compared both run on a handle that has them all)
        frc = pnp_generator_forward(g, flat, packed, lrs, mvs, par, slices.data(), qps.data(), bqs.data(), out, ws, ws_bytes, n, t, sc.h, sc.w, &caller);
        const std::vector<std::string> errs0 = errors;
        reset();
        errors = errs0;
        written = before;
        const size_t ref_begin = trace.size();
        frc = pnp_generator_forward(g, flat, packed, lrs, mvs, par, slices.data(), qps.data(), bqs.data(), out, ws, ws_bytes, n, t, sc.h, sc.w, &caller);
        if (frc == 0 && !covered(out, (size_t)n * out_px * 4)) fail("pnp_generator_forward left part of the output unwritten");
        const std::vector<std::string> ref(trace.begin() + ref_begin, trace.end());
        const std::vector<std::string> errs = errors;
        reset();
        errors = errs;
        written = before;
        for (int b = 0; b < n; ++b)
            clips[b] = pnp_clip_io{lrs + (size_t)b * t * 3 * hw, mvs + (size_t)b * t * 4 * hw, par + (size_t)b * t * 3 * hw, out + (size_t)b * out_px, nullptr};
        const int crc = pnp_generator_forward_clips(g, flat, packed, clips.data(), n, PNP_FRAMES_F32_NCHW, PNP_OUT_F32, slices.data(), qps.data(),
                                                    bqs.data(), ws, ws_bytes, t, sc.h, sc.w, &caller);
        if (crc != frc) fail("the two entry points return different codes");
        if (crc == 0 && !covered(out, (size_t)n * out_px * 4)) fail("pnp_generator_forward_clips left part of the output unwritten");
        const std::vector<std::string> got(trace.begin() + ref_begin + ref.size(), trace.end());
        list_len = ref.size();
        same = ref.size() == got.size() ? 1 : 0;
        for (size_t i = 0; same == 1 && i < ref.size(); ++i)
            if (ref[i] != got[i]) {
                same = 0;
                first_diff = i;
                if (getenv("PNP_STUB_SHOW_DIFF")) fprintf(stderr, "line %zu: [%s] against [%s]\n", i, ref[i].c_str(), got[i].c_str());
            }
    } else {
        // every tensor of every clip its own heap block of exactly the size the ABI names; both output buffers exist whatever the mask asks for
        for (int b = 0; b < n; ++b) {
            void* lq = malloc(lq_bytes);
            float* mv = (float*)malloc((size_t)t * 4 * hw * 4);
            float* pr = (float*)malloc((size_t)t * 3 * hw * 4);
            float* of = (float*)malloc(out_px * 4);
            unsigned char* o8 = (unsigned char*)malloc(out_px);
            for (void* p : {lq, (void*)mv, (void*)pr, (void*)of, (void*)o8}) owned.push_back(p);
            mark(lq, lq_bytes);
            mark(mv, (size_t)t * 4 * hw * 4);
            mark(pr, (size_t)t * 3 * hw * 4);
            const std::string cb = std::to_string(b);
            region("lq" + cb, lq, lq_bytes);
            region("mvs" + cb, mv, (size_t)t * 4 * hw * 4);
            region("par" + cb, pr, (size_t)t * 3 * hw * 4);
            region("out_f32_" + cb, of, out_px * 4);
            region("out_u8_" + cb, o8, out_px);
            clips[b] = pnp_clip_io{lq, mv, pr, of, o8};
        }
        frc = pnp_generator_forward_clips(g, flat, packed, clips.data(), n, sc.lq_format, sc.out_mask, slices.data(), qps.data(), bqs.data(), ws,
                                          ws_bytes, t, sc.h, sc.w, &caller);
        for (int b = 0; b < n && frc == 0; ++b) {
            const bool f_w = covered(clips[b].out_f32_dev, out_px * 4), u_w = covered(clips[b].out_u8_dev, out_px);
            if ((sc.out_mask & PNP_OUT_F32) ? !f_w : any_written(clips[b].out_f32_dev, out_px * 4)) fail("the fp32 output is not what the mask asks for");
            if ((sc.out_mask & PNP_OUT_U8) ? !u_w : any_written(clips[b].out_u8_dev, out_px)) fail("the uint8 output is not what the mask asks for");
        }
        const bool staged = io_staged(g);
        // the pack launches: one per clip, reading the clip's bytes from its first to its last
        for (const PnpStubIoLaunch& r : pnp_stub_io_log) {
            if (r.kind == PNP_STUB_IO_PACK_LR_U8) {
                bool own = false;
                for (int b = 0; b < n; ++b) own = own || r.in == clips[b].lq_dev;
                if (!own || r.frames != t || r.h != sc.h || r.w != sc.w) fail("a pack launch does not read one clip's t*h*w*3 bytes");
            }
            if (r.kind == PNP_STUB_IO_CONV_LAST) {
                const ConvArgs& a = r.conv;
                if (u8_in && a.lr) fail("the last conv was handed fp32 planes of the frame in byte mode");
                if (a.out_u8) {
                    bool own = false;
                    for (int b = 0; b < n; ++b) {
                        const ptrdiff_t d = a.out_u8 - clips[b].out_u8_dev;
                        own = own || (d >= 0 && (size_t)d < out_px && (size_t)d % (3 * hw * os * os) == 0);
                    }
                    if (!own || (size_t)a.H * a.W != hw * os * os) fail("the last conv's byte output is not one frame of a clip's output");
                }
            }
            if (r.kind == PNP_STUB_IO_FROM_RGB8 && (r.frames != 1 || !staged)) fail("a staging conversion of more than one frame");
            if (r.kind == PNP_STUB_IO_TO_RGB8 && (r.frames != 1 || !staged)) fail("a staging conversion of more than one frame");
        }
        // a conv that adds the frame through the fp32 interface reads the one-frame staging buffer in byte mode, never a clip
        for (const ConvRec& c : convs)
            if ((c.a.out_mode == 2 || c.a.out_mode == 3) && u8_in) {
                bool in_ws = (const char*)c.a.lr >= ws && (const char*)c.a.lr < ws + ws_bytes;
                if (!in_ws) fail("a conv read fp32 planes of the frame from outside the workspace in byte mode");
            }
    }
    pnp_stub_io_hook = nullptr;
    int rgb_heads = 0;
    for (const ConvRec& c : convs) rgb_heads += (c.a.out_mode == 2 || c.a.out_mode == 3) ? 1 : 0;
    int banded = 0;
    for (const ConvRec& c : convs) banded += c.a.band ? 1 : 0;
    std::vector<int> streams_used = launch_streams;
    std::sort(streams_used.begin(), streams_used.end());
    streams_used.erase(std::unique(streams_used.begin(), streams_used.end()), streams_used.end());
    printf("{\"name\": \"%s\", \"kind\": \"%s\", \"pack_rc\": %d, \"forward_rc\": %d, \"same\": %d, \"first_diff\": %zu, \"records\": %zu, "
           "\"plain_bytes\": %lld, \"ctx_bytes\": %lld, \"frame_bytes\": %lld, \"out_frame_bytes\": %lld, \"staged\": %d, "
           "\"n_pack\": %d, \"n_from\": %d, \"n_to\": %d, \"n_last_io\": %d, \"rgb_heads_fp32_interface\": %d, \"banded\": %d, \"frames\": %d, ",
           sc.name.c_str(), sc.kind.c_str(), prc, frc, same, first_diff, list_len, (long long)plain_bytes, (long long)ctx_bytes,
           (long long)(hw * 12), (long long)(hw * 12 * os * os), io_staged(g) ? 1 : 0, n_pack, n_from, n_to, n_last_io, rgb_heads, banded, n * t);
    json_ints("streams_used", streams_used);
    pnp_generator_destroy(g);
    trace_dump(sc.name);
    printf("\"errors\": [");
    for (size_t i = 0; i < errors.size(); ++i) printf("%s\"%s\"", i ? ", " : "", errors[i].c_str());
    printf("]}\n");
    fflush(stdout);
    free(flat);
    free(packed);
    free(ws);
    for (void* p : owned) free(p);
    return errors.empty() ? 0 : 1;
}

}  // namespace

#undef main
int main(int argc, char** argv) {
    const pnp_generator_cfg d = default_cfg();
    pnp_generator_cfg vsr = d, sparse = d;
    vsr.vsr = 1;
    sparse.sparse_val = 1;
    const int F = PNP_FRAMES_F32_NCHW, U = PNP_FRAMES_U8_HWC;
    //   name                 kind    cfg  prec n  t   h    w   ctx fmt mask wino valu k
    const std::vector<IoScenario> all = {
        {"same_128_n3_ctx3", "same", d, 0, 3, 3, 128, 128, 3, F, 1, 1, 1, 0},
        {"same_720_band", "same", d, 0, 1, 3, 720, 1280, 1, F, 1, 1, 1, 0},
        {"same_128_bounded", "same", d, 0, 1, 9, 128, 128, 1, F, 1, 1, 1, -1},
        {"same_128_f16", "same", d, 1, 2, 3, 128, 128, 2, F, 1, 1, 1, 0},
        {"u8_128_n2_mask1", "io", d, 0, 2, 3, 128, 128, 2, U, 1, 1, 1, 0},
        {"u8_128_n2_mask2", "io", d, 0, 2, 3, 128, 128, 2, U, 2, 1, 1, 0},
        {"u8_128_n2_mask3", "io", d, 0, 2, 3, 128, 128, 2, U, 3, 1, 1, 0},
        {"f32_128_n2_mask2", "io", d, 0, 2, 3, 128, 128, 2, F, 2, 1, 1, 0},
        {"f32_128_n2_mask3", "io", d, 0, 2, 3, 128, 128, 1, F, 3, 1, 1, 0},
        {"u8_720_band_n2_mask2", "io", d, 0, 2, 2, 720, 1280, 1, U, 2, 1, 1, 0},
        {"u8_128_bounded_mask2", "io", d, 0, 1, 9, 128, 128, 1, U, 2, 1, 1, -1},
        {"u8_vsr_mask3", "io", vsr, 0, 2, 2, 64, 96, 2, U, 3, 1, 1, 0},
        {"u8_sparse_mask2", "io", sparse, 0, 1, 3, 128, 128, 1, U, 2, 1, 1, 0},
        {"u8_x3_mask2", "io", d, 2, 2, 3, 128, 128, 2, U, 2, 1, 1, 0},
        {"u8_f16_mask2", "io", d, 1, 2, 3, 128, 128, 2, U, 2, 1, 1, 0},
        {"u8_f16_mask3", "io", d, 1, 2, 3, 128, 128, 2, U, 3, 1, 1, 0},
        {"u8_f16_vsr_mask2", "io", vsr, 1, 1, 2, 64, 96, 1, U, 2, 1, 1, 0},
        {"u8_mfma_last_mask2", "io", d, 0, 2, 3, 128, 128, 2, U, 2, 1, 0, 0},
        {"f32_mfma_last_mask2", "io", d, 0, 1, 3, 128, 128, 1, F, 2, 1, 0, 0},
        {"u8_direct_convs_mask1", "io", d, 0, 1, 3, 128, 128, 1, U, 1, 0, 1, 0},
    };
    int bad = 0;
    for (const IoScenario& s : all) {
        bool want = argc < 2;
        for (int i = 1; i < argc; ++i) want = want || s.name == argv[i];
        if (want) bad += run_io(s);
    }
    return bad ? 1 : 0;
}
