// Host-only run of the Y'CbCr 4:2:0 boundary of the clip scheduler (pnp_generator_forward_clips_yuv) under AddressSanitizer / UBSan.
//
// TEST INFRASTRUCTURE.  Built by tests/test_yuv_frames_host.py with a plain host compiler:
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -DPNP_HOST_STUB -Dmain=sched_stub_main
//         -x c++ tests/host/yuv_stub.cpp
// It reuses tests/host/sched_stub.cpp unchanged (recording launchers over csrc/generator.hip; its driver is renamed away).  The three
// launchers of the 4:2:0 boundary are recorded by csrc/host_stub/yuv_stub.h; the hooks below give them, and conv_last's launch behind
// a 4:2:0 clip, the range bookkeeping the other launchers have.  One JSON object per scenario:
//   * every plane of every clip is a heap block of its own that ends with the last sample of its last row (ASan's red zone behind
//     it) and starts 9 bytes into the block behind 8 poisoned bytes: odd addresses, odd pitches.  Only the samples inside a row's
//     width count as written, so a launch that reads a row's padding, or anything outside its plane's rows, is an error;
//   * every sample of every requested output plane is written exactly once and no other byte of those blocks at all; the fp32 and
//     uint8 outputs are written iff the mask asks for them;
//   * the same clips run as fp32 planes through pnp_generator_forward_clips first: apart from the pack launch, conv_last's
//     arguments and the converters, the two ordered traces (every HIP call and launch with every argument) are identical.
#include <unordered_map>

#include "sched_stub.cpp"
#include "yuv_common.h"      // each_row, Block, any_written

namespace {

using namespace stub;

int n_pack = 0, n_pack_fast = 0, n_from = 0, n_to = 0, n_to8 = 0, n_last_io = 0, n_last_rgb0 = 0;
std::unordered_map<uintptr_t, int> out_writes;      // byte address -> times a 4:2:0 output launch wrote it

void trace_yuv(const PnpStubYuvLaunch& r) {
    static const char* const names[3] = {"launch_pack_lr_yuv420", "launch_frames_from_yuv420", "launch_frames_to_yuv420"};
    Tr(names[r.kind], r.stream).p("y", r.planes.y).p("cb", r.planes.cb).p("cr", r.planes.cr).p("in", r.in).p("out", r.out).i("frames", r.frames)
        .i("H", r.h).i("W", r.w);
}

void yuv_hook(const PnpStubYuvLaunch& r) {
    trace_yuv(r);
    note_launch(r.stream);
    const size_t px = (size_t)r.frames * r.h * r.w;
    auto rd = [](const char* what, const unsigned char* p, size_t n) { RD(what, p, n); };
    auto wr = [](const char* what, unsigned char* p, size_t n) {
        WR(what, p, n);
        for (size_t j = 0; j < n; ++j) ++out_writes[(uintptr_t)p + j];
    };
    switch (r.kind) {
        case PNP_STUB_YUV_PACK:
            cur = "launch_pack_lr_yuv420";
            ++n_pack;
            n_pack_fast += r.fast ? 1 : 0;
            each_row(r.planes, r.frames, r.h, r.w, rd);
            WR("the packed RGB0 frames", r.out, px * 16);
            break;
        case PNP_STUB_YUV_FROM:
            cur = "launch_frames_from_yuv420";
            ++n_from;
            each_row(r.planes, r.frames, r.h, r.w, rd);
            WR("a frame of fp32 planes", r.out, px * 12);
            break;
        default:
            cur = "launch_frames_to_yuv420";
            ++n_to;
            RD("a frame of fp32 planes", r.in, px * 12);
            each_row(r.planes, r.frames, r.h, r.w, wr);
    }
}

void io_hook(const PnpStubIoLaunch& r) {
    trace_io(r);
    note_launch(r.stream);
    cur = "launch_conv_last_io";
    if (r.kind == PNP_STUB_IO_TO_RGB8) {      // the uint8 output behind a last conv with an fp32 interface: one frame of planes to bytes
        cur = "launch_frames_to_rgb8";
        ++n_to8;
        if (r.frames != 1) fail("a staging conversion of more than one frame");
        RD("a frame of fp32 planes", r.in, (size_t)r.h * r.w * 12);
        return WR("a byte frame", r.out, (size_t)r.h * r.w * 3);
    }
    if (r.kind != PNP_STUB_IO_CONV_LAST) return fail("a launcher that reads byte frames ran at the 4:2:0 boundary");
    ++n_last_io;
    const ConvArgs& a = r.conv;
    const size_t hw = (size_t)a.H * a.W, lhw = a.out_mode == 2 ? hw : hw / 16;
    RD("conv_last's source", a.src[0], hw * 256);
    RD("the vector-ALU conv_last weights", a.wvalu, 9 * 64 * 4 * 4);
    RD("the bias", a.bias, 3 * 4);
    if (a.lr_rgb0) {
        ++n_last_rgb0;
        RD("the frame's RGB0 pixels", a.lr_rgb0, lhw * 16);
        if (a.lr || a.lr_u8) fail("conv_last was handed the frame twice");
    } else {
        fail("conv_last behind a 4:2:0 clip does not read the RGB0 frame");
    }
    if (a.out) WR("the output frame", a.out, hw * 12);
    if (a.out_u8) WR("the output frame's bytes", a.out_u8, hw * 3);
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
    pnp_stub_yuv_log.clear();
    out_writes.clear();
    dcn_calls = 0;
    n_pack = n_pack_fast = n_from = n_to = n_to8 = n_last_io = n_last_rgb0 = 0;
}

struct ClipPlanes {
    Block y, c0, c1;
    pnp_yuv420_planes d;
    // planes 9 bytes into their blocks; layout 0 nv12 | 1 nv21 | 2 i420; pitches odd: w + 7 for Y, for chroma w + 5 (interleaved) or w/2 + 3
    void make(const std::string& name, int layout, int t, int h, int w) {
        const int64_t yp = w + 7, cp = layout == 2 ? w / 2 + 3 : w + 5;
        const int64_t yf = yp * h + 3, cf = cp * (h / 2) + 5;
        y.make(t, h, yp, yf, w, 9);
        region(name + ".y", y.p, y.bytes);
        if (layout == 2) {
            c0.make(t, h / 2, cp, cf, w / 2, 9);
            c1.make(t, h / 2, cp, cf, w / 2, 9);
            region(name + ".cb", c0.p, c0.bytes);
            region(name + ".cr", c1.p, c1.bytes);
            d = pnp_yuv420_planes{y.p, c0.p, c1.p, yp, cp, yf, cf, 1};
        } else {
            c0.make(t, h / 2, cp, cf, w, 9);
            region(name + ".c", c0.p, c0.bytes);
            d = pnp_yuv420_planes{y.p, layout == 0 ? c0.p : c0.p + 1, layout == 0 ? c0.p + 1 : c0.p, yp, cp, yf, cf, 2};
        }
    }
    void release() { y.release(), c0.release(), c1.release(); }
};

struct YuvScenario {
    std::string name;
    pnp_generator_cfg cfg;
    int prec, n, t, h, w, contexts, layout, out_mask, last_valu, max_resident, any_size;
};

// what the comparison of the two traces leaves out: the pack launch and the converters go, a conv_last launch becomes one token
std::vector<std::string> comparable(const std::vector<std::string>& tr) {
    std::vector<std::string> out;
    for (const std::string& ln : tr) {
        if (ln.rfind("launch_pack_lr", 0) == 0 || ln.rfind("launch_frames_", 0) == 0) continue;
        const bool head = ln.find(" out_mode=2 ") != std::string::npos || ln.find(" out_mode=3 ") != std::string::npos;
        out.push_back(head ? "conv_last" : ln);
    }
    return out;
}

int run_yuv(YuvScenario sc) {
    reset();
    regions.clear();
    trace.clear();
    pnp_generator* g = nullptr;
    if (pnp_generator_create(&sc.cfg, &g)) return 2;
    pnp_generator_set_precision(g, sc.prec);
    pnp_generator_set_option(g, PNP_OPT_CONV_LAST_VALU, sc.last_valu);
    pnp_generator_set_any_size(g, sc.any_size);
    if (sc.max_resident < 0) sc.max_resident = pnp_generator_min_resident(g, sc.t);
    pnp_generator_set_max_resident(g, sc.max_resident);
    const int t = sc.t, n = sc.n, os = sc.cfg.vsr ? 4 : 1, H = sc.h * os, W = sc.w * os;
    const int64_t flat_n = pnp_generator_flat_floats(g), packed_n = pnp_generator_packed_floats(g);
    const int64_t plain_bytes = pnp_generator_workspace_bytes(g, t, sc.h, sc.w);
    const int64_t ctx_bytes = pnp_generator_workspace_bytes_yuv(g, t, sc.h, sc.w, sc.out_mask);
    const int64_t ws_bytes = ctx_bytes * sc.contexts;
    const size_t hw = (size_t)sc.h * sc.w, out_px = (size_t)t * 3 * H * W;
    float* flat = (float*)malloc((size_t)flat_n * 4);
    float* packed = (float*)malloc((size_t)packed_n * 4);
    char* ws = nullptr;
    if (plain_bytes <= 0 || ws_bytes <= 0 || posix_memalign((void**)&ws, 256, (size_t)ws_bytes)) return 2;
    mark(flat, (size_t)flat_n * 4);
    region("flat", flat, (size_t)flat_n * 4);
    region("packed", packed, (size_t)packed_n * 4);
    region("ws", ws, (size_t)ws_bytes);
    std::vector<float> slices, qps, bqs;
    for (int b = 0; b < n; ++b) {
        const std::vector<float> sl = pattern("IBBBP", t);
        for (int i = 0; i < t; ++i) {
            slices.push_back(sl[i]);
            qps.push_back((20.f + (float)((i * 7 + b) % 20)) / 255.f);
            bqs.push_back((b ? 35.f : 25.f) / 255.f);
        }
    }
    pnp_stub_stream caller{0};
    const int prc = pnp_generator_pack(g, flat, packed, &caller);
    pnp_stub_io_hook = io_hook;
    pnp_stub_yuv_hook = yuv_hook;
    std::vector<pnp_clip_io> fclips(n);
    std::vector<pnp_clip_yuv> yclips(n);
    std::vector<ClipPlanes> in(n), out(n);
    std::vector<void*> owned;
    for (int b = 0; b < n; ++b) {
        const std::string cb = std::to_string(b);
        float* lr = (float*)malloc((size_t)t * 3 * hw * 4);
        float* mv = (float*)malloc((size_t)t * 4 * hw * 4);
        float* pr = (float*)malloc((size_t)t * 3 * hw * 4);
        float* of = (float*)malloc(out_px * 4);
        unsigned char* o8 = (unsigned char*)malloc(out_px);
        for (void* p : {(void*)lr, (void*)mv, (void*)pr, (void*)of, (void*)o8}) owned.push_back(p);
        region("lrs" + cb, lr, (size_t)t * 3 * hw * 4);
        region("mvs" + cb, mv, (size_t)t * 4 * hw * 4);
        region("par" + cb, pr, (size_t)t * 3 * hw * 4);
        region("out_f32_" + cb, of, out_px * 4);
        region("out_u8_" + cb, o8, out_px);
        in[b].make("lq" + cb, sc.layout, t, sc.h, sc.w);
        out[b].make("out_yuv" + cb, sc.layout, t, H, W);
        fclips[b] = pnp_clip_io{lr, mv, pr, of, nullptr};
        yclips[b] = pnp_clip_yuv{in[b].d, mv, pr, of, o8, out[b].d};
    }
    auto inputs_written = [&]() {
        for (int b = 0; b < n; ++b) {
            mark(fclips[b].lq_dev, (size_t)t * 3 * hw * 4);
            mark(fclips[b].mvs_dev, (size_t)t * 4 * hw * 4);
            mark(fclips[b].par_dev, (size_t)t * 3 * hw * 4);
            each_row(yuv_planes(in[b].d), t, sc.h, sc.w, [](const char*, const unsigned char* p, size_t k) { mark(p, k); });      // (a row's samples, not its padding)
        }
    };
    // the fp32 boundary on the same handle: once to make its streams and events, once for the trace
    const int64_t ref_ws_bytes = plain_bytes * sc.contexts;
    int frc = 0;
    std::vector<std::string> ref;
    for (int pass = 0; pass < 2; ++pass) {
        const auto before = written;
        const std::vector<std::string> errs = errors;
        reset();
        errors = errs;
        written = before;
        inputs_written();
        const size_t begin = trace.size();
        frc = pnp_generator_forward_clips(g, flat, packed, fclips.data(), n, PNP_FRAMES_F32_NCHW, PNP_OUT_F32, slices.data(), qps.data(), bqs.data(), ws,
                                          ref_ws_bytes, t, sc.h, sc.w, &caller);
        ref.assign(trace.begin() + begin, trace.end());
        written = before;
    }
    if (n_pack || n_from || n_to || n_to8 || n_last_io) fail("a launcher of a byte or 4:2:0 boundary ran at the fp32 boundary");
    {
        const std::vector<std::string> errs = errors;
        reset();
        errors = errs;
    }
    mark(flat, (size_t)flat_n * 4);
    mark(packed, (size_t)packed_n * 4);
    inputs_written();
    const size_t begin = trace.size();
    const int yrc = pnp_generator_forward_clips_yuv(g, flat, packed, yclips.data(), n, PNP_YUV_BT709_LIMITED, sc.out_mask, slices.data(), qps.data(),
                                                    bqs.data(), ws, ws_bytes, t, sc.h, sc.w, &caller);
    if (yrc != frc) fail("the two entry points return different codes");
    const std::vector<std::string> got(trace.begin() + begin, trace.end());
    const std::vector<std::string> a = comparable(ref), c = comparable(got);
    int same = a.size() == c.size() ? 1 : 0;
    size_t first_diff = 0;
    for (size_t i = 0; same == 1 && i < a.size(); ++i)
        if (a[i] != c[i]) {
            same = 0;
            first_diff = i;
            if (getenv("PNP_STUB_SHOW_DIFF")) fprintf(stderr, "line %zu: [%s] against [%s]\n", i, a[i].c_str(), c[i].c_str());
        }
    // outputs: what the mask asks for, completely; the 4:2:0 planes sample by sample exactly once and nothing else of their blocks
    size_t expect_writes = 0;
    for (int b = 0; b < n && yrc == 0; ++b) {
        const bool f_w = covered(yclips[b].out_f32_dev, out_px * 4), u_w = covered(yclips[b].out_u8_dev, out_px);
        if ((sc.out_mask & PNP_OUT_F32) ? !f_w : any_written(yclips[b].out_f32_dev, out_px * 4)) fail("the fp32 output is not what the mask asks for");
        if ((sc.out_mask & PNP_OUT_U8) ? !u_w : any_written(yclips[b].out_u8_dev, out_px)) fail("the uint8 output is not what the mask asks for");
        if (sc.out_mask & PNP_OUT_YUV420)
            each_row(yuv_planes(out[b].d), t, H, W, [&](const char* what, const unsigned char* p, size_t k) {
                for (size_t j = 0; j < k; ++j) {
                    const auto it = out_writes.find((uintptr_t)p + j);
                    if (it == out_writes.end() || it->second != 1) return fail(std::string("a sample of ") + what + " of the output was not written exactly once");
                }
                expect_writes += k;
            });
    }
    if (yrc == 0 && out_writes.size() != expect_writes) fail("a 4:2:0 output launch wrote bytes that are no sample of a requested output plane");
    // the launches: one pack per clip over the clip's own planes, one frame per converter, the frame conv_last adds from the workspace
    const bool staged = io_staged(g);
    for (const PnpStubYuvLaunch& r : pnp_stub_yuv_log) {
        if (r.kind == PNP_STUB_YUV_PACK) {
            bool own = false;
            for (int b = 0; b < n; ++b) own = own || r.planes.y == in[b].d.y;
            if (!own || r.frames != t || r.h != sc.h || r.w != sc.w) fail("a pack launch does not read one clip's t frames");
            if (r.fast) fail("planes at odd addresses took the aligned form of the pack launch");
        } else if (r.frames != 1) {
            fail("a conversion of more than one frame");
        }
        if (r.kind == PNP_STUB_YUV_FROM && !staged) fail("a frame was converted to fp32 planes in front of a last conv that reads RGB0");
        if (r.planes.sample_bytes != 1 || r.planes.bit_depth != 8 || r.planes.msb_aligned) fail("a launch at the 8-bit boundary does not name bytes");
    }
    int rgb_heads = 0;
    for (const ConvRec& cr : convs)
        if (cr.a.out_mode == 2 || cr.a.out_mode == 3) {
            ++rgb_heads;
            if (!((const char*)cr.a.lr >= ws && (const char*)cr.a.lr < ws + ws_bytes)) fail("a conv read fp32 planes of the frame from outside the workspace");
        }
    pnp_stub_io_hook = nullptr;
    pnp_stub_yuv_hook = nullptr;
    std::vector<int> streams_used = launch_streams;
    std::sort(streams_used.begin(), streams_used.end());
    streams_used.erase(std::unique(streams_used.begin(), streams_used.end()), streams_used.end());
    printf("{\"name\": \"%s\", \"pack_rc\": %d, \"forward_rc\": %d, \"same\": %d, \"first_diff\": %zu, \"records\": %zu, \"plain_bytes\": %lld, "
           "\"ctx_bytes\": %lld, \"frame_bytes\": %lld, \"out_frame_bytes\": %lld, \"staged\": %d, \"n_pack\": %d, \"n_from\": %d, \"n_to\": %d, "
           "\"n_to8\": %d, \"n_last_io\": %d, \"n_last_rgb0\": %d, \"rgb_heads_fp32_interface\": %d, \"frames\": %d, \"out_samples\": %zu, ",
           sc.name.c_str(), prc, yrc, same, first_diff, a.size(), (long long)plain_bytes, (long long)ctx_bytes, (long long)(hw * 12),
           (long long)(hw * 12 * os * os), staged ? 1 : 0, n_pack, n_from, n_to, n_to8, n_last_io, n_last_rgb0, rgb_heads, n * t, expect_writes);
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
    for (int b = 0; b < n; ++b) in[b].release(), out[b].release();
    return errors.empty() ? 0 : 1;
}

}  // namespace

#undef main
int main(int argc, char** argv) {
    const pnp_generator_cfg d = default_cfg();
    pnp_generator_cfg vsr = d;
    vsr.vsr = 1;
    //   name               cfg prec n  t   h    w  ctx layout mask valu k any_size
    const std::vector<YuvScenario> all = {
        {"plain_nv12_mask7", d, 0, 1, 3, 128, 128, 1, 0, 7, 1, 0, 0},
        {"plain_nv21_mask4", d, 0, 1, 3, 64, 96, 1, 1, 4, 1, 0, 0},
        {"vsr_i420_mask4", vsr, 0, 1, 2, 64, 96, 1, 2, 4, 1, 0, 0},
        {"f16_nv21_mask6", d, 1, 1, 3, 128, 128, 1, 1, 6, 1, 0, 0},
        {"f16_vsr_nv12_mask5", vsr, 1, 1, 2, 64, 96, 1, 0, 5, 1, 0, 0},
        {"x3_nv12_mask5", d, 2, 1, 3, 128, 128, 1, 0, 5, 1, 0, 0},
        {"mfma_last_i420_mask2", d, 0, 1, 3, 64, 96, 1, 2, 2, 0, 0, 0},
        {"bounded_i420_mask4", d, 0, 1, 9, 64, 96, 1, 2, 4, 1, -1, 0},
        {"two_clips_nv12_mask7", d, 0, 2, 3, 128, 128, 2, 0, 7, 1, 0, 0},
        {"any_size_66x70_nv12_mask7", d, 0, 1, 3, 66, 70, 1, 0, 7, 1, 0, 1},
    };
    int bad = 0;
    for (const YuvScenario& s : all) {
        bool want = argc < 2;
        for (int i = 1; i < argc; ++i) want = want || s.name == argv[i];
        if (want) bad += run_yuv(s);
    }
    return bad ? 1 : 0;
}
