// Host-only run of the 10 / 12-bit 4:2:0 boundary of the clip scheduler (pnp_generator_forward_clips_yuv16) under AddressSanitizer / UBSan.
//
// TEST INFRASTRUCTURE.  Built by tests/test_yuv16_host.py with a plain host compiler:
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -DPNP_HOST_STUB -Dmain=sched_stub_main
//         -x c++ tests/host/yuv16_stub.cpp
// It reuses tests/host/sched_stub.cpp unchanged (recording launchers over csrc/generator.hip; its driver is renamed away).  The
// launchers of the 4:2:0 boundary are recorded by csrc/host_stub/yuv_stub.h, one record type whose sample_bytes tells the 8-bit run
// from the 16-bit one; the hooks below give them, and conv_last's launch behind a 4:2:0 clip, the range bookkeeping the other
// launchers have.  One JSON object per scenario:
//   * every plane of every 16-bit clip is a heap block of its own that ends with the last sample of its last row (ASan's red zone
//     behind it) and starts 10 bytes into the block behind 8 poisoned bytes: even addresses that are not 4-byte aligned, pitches of
//     a row plus 2 or 6 bytes.  Only the samples inside a row's width count as written, so a launch that reads a row's padding, or
//     anything outside its plane's rows, is an error; one scenario has 8-byte aligned planes and pitches, where the aligned form runs;
//   * every sample (two bytes) of every requested output plane is written exactly once and no other byte of those blocks at all; the
//     fp32 and uint8 outputs are written iff the mask asks for them;
//   * the same clips run as 8-bit planes through pnp_generator_forward_clips_yuv first, with the same workspace and outputs: apart
//     from the pack launch, the staged conversion and the output conversion, the two ordered traces (every HIP call and launch with
//     every argument) are identical, and the two workspace sizes are one query.
#include <unordered_map>

#include "sched_stub.cpp"
#include "yuv_common.h"      // each_row, Block, any_written

namespace {

using namespace stub;

int n_pack = 0, n_pack_fast = 0, n_from = 0, n_to = 0, n_to8 = 0, n_last_io = 0, n8 = 0;
bool count_writes = false;
std::unordered_map<uintptr_t, int> out_writes;      // byte address -> times a 16-bit output launch wrote it

// (the 8- and the 16-bit run go through the same three launchers)
const char* const names[3] = {"launch_pack_lr_yuv420", "launch_frames_from_yuv420", "launch_frames_to_yuv420"};

void yuv_launch(const PnpStubYuvLaunch& r) {
    Tr(names[r.kind], r.stream).p("y", r.planes.y).p("cb", r.planes.cb).p("cr", r.planes.cr).p("in", r.in).p("out", r.out).i("frames", r.frames)
        .i("H", r.h).i("W", r.w);
    note_launch(r.stream);
    cur = names[r.kind];
    const size_t px = (size_t)r.frames * r.h * r.w;
    auto rd = [](const char* what, const unsigned char* p, size_t n) { RD(what, p, n); };
    auto wr = [](const char* what, unsigned char* p, size_t n) {
        WR(what, p, n);
        for (size_t j = 0; count_writes && j < n; ++j) ++out_writes[(uintptr_t)p + j];
    };
    switch (r.kind) {
        case PNP_STUB_YUV_PACK:
            each_row(r.planes, r.frames, r.h, r.w, rd);
            WR("the packed RGB0 frames", r.out, px * 16);
            break;
        case PNP_STUB_YUV_FROM:
            if (r.frames != 1) fail("a staged conversion of more than one frame");
            each_row(r.planes, r.frames, r.h, r.w, rd);
            WR("a frame of fp32 planes", r.out, px * 12);
            break;
        default:
            if (r.frames != 1) fail("an output conversion of more than one frame");
            RD("a frame of fp32 planes", r.in, px * 12);
            each_row(r.planes, r.frames, r.h, r.w, wr);
    }
}

void yuv_hook(const PnpStubYuvLaunch& r) {
    if (r.planes.sample_bytes == 1) {
        ++n8;
    } else {
        n_pack += r.kind == PNP_STUB_YUV_PACK;
        n_pack_fast += r.kind == PNP_STUB_YUV_PACK && r.fast;
        n_from += r.kind == PNP_STUB_YUV_FROM;
        n_to += r.kind == PNP_STUB_YUV_TO;
    }
    yuv_launch(r);
}

void io_hook(const PnpStubIoLaunch& r) {
    trace_io(r);
    note_launch(r.stream);
    cur = "launch_conv_last_io";
    if (r.kind == PNP_STUB_IO_TO_RGB8) {      // the uint8 output behind a last conv with an fp32 interface: one frame of planes to bytes
        cur = "launch_frames_to_rgb8";
        ++n_to8;
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
    if (a.lr_rgb0) RD("the frame's RGB0 pixels", a.lr_rgb0, lhw * 16);
    else fail("conv_last behind a 4:2:0 clip does not read the RGB0 frame");
    if (a.lr || a.lr_u8) fail("conv_last was handed the frame twice");
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
    n_pack = n_pack_fast = n_from = n_to = n_to8 = n_last_io = n8 = 0;
}

// S = 1: pnp_yuv420_planes (D), bytes; S = 2: pnp_yuv420_planes16, 16-bit words.  layout 0: Y + interleaved Cb Cr | 1: Cr Cb | 2: planar.
// ragged: planes 10 bytes into their blocks, pitches of a row plus 2 (Y) or 6 (chroma) bytes; otherwise 16 bytes in, pitches rounded
// up to 8 bytes: where the aligned form of the pack launch applies (w a multiple of 4)
template <int S>
struct ClipPlanes {
    Block y, c0, c1;
    int64_t yp, cp, yf, cf;
    int c_step;
    unsigned char *py, *pcb, *pcr;
    void make(const std::string& name, int layout, int t, int h, int w, bool ragged) {
        const int lead = ragged ? 10 : 16;
        const int64_t yrow = (int64_t)w * S, crow = layout == 2 ? (int64_t)w / 2 * S : (int64_t)w * S;
        yp = ragged ? yrow + 2 : (yrow + 7) / 8 * 8;
        cp = ragged ? crow + 6 : (crow + 7) / 8 * 8;
        yf = yp * h + (ragged ? 2 : 8), cf = cp * (h / 2) + (ragged ? 6 : 8);
        c_step = layout == 2 ? 1 : 2;
        y.make(t, h, yp, yf, yrow, lead);
        region(name + ".y", y.p, y.bytes);
        py = y.p;
        c0.make(t, h / 2, cp, cf, crow, lead);
        if (layout == 2) {
            c1.make(t, h / 2, cp, cf, crow, lead);
            region(name + ".cb", c0.p, c0.bytes);
            region(name + ".cr", c1.p, c1.bytes);
            pcb = c0.p, pcr = c1.p;
        } else {
            region(name + ".c", c0.p, c0.bytes);
            pcb = layout == 0 ? c0.p : c0.p + S, pcr = layout == 0 ? c0.p + S : c0.p;
        }
    }
    pnp_yuv420_planes d8() const { return pnp_yuv420_planes{py, pcb, pcr, yp, cp, yf, cf, c_step}; }
    pnp_yuv420_planes16 d16(int depth, int msb) const {
        return pnp_yuv420_planes16{(unsigned short*)py, (unsigned short*)pcb, (unsigned short*)pcr, yp, cp, yf, cf, c_step, depth, msb};
    }
    void release() { y.release(), c0.release(), c1.release(); }
};

struct Scenario16 {
    std::string name;
    pnp_generator_cfg cfg;
    int prec, n, t, h, w, contexts, layout, depth, msb, out_depth, out_msb, out_mask, last_valu, any_size, ragged;
};

// what the comparison of the two traces leaves out: the pack launch, the staged conversion and the output conversion
std::vector<std::string> comparable(const std::vector<std::string>& tr) {
    std::vector<std::string> out;
    for (const std::string& ln : tr)
        if (ln.rfind("launch_pack_lr_yuv420", 0) != 0 && ln.rfind("launch_frames_from_yuv420", 0) != 0 && ln.rfind("launch_frames_to_yuv420", 0) != 0)
            out.push_back(ln);
    return out;
}

int run(const Scenario16& sc) {
    reset();
    regions.clear();
    trace.clear();
    pnp_generator* g = nullptr;
    pnp_generator_cfg cfg = sc.cfg;
    if (pnp_generator_create(&cfg, &g)) return 2;
    pnp_generator_set_precision(g, sc.prec);
    pnp_generator_set_option(g, PNP_OPT_CONV_LAST_VALU, sc.last_valu);
    pnp_generator_set_any_size(g, sc.any_size);
    const int t = sc.t, n = sc.n, os = sc.cfg.vsr ? 4 : 1, H = sc.h * os, W = sc.w * os;
    const int64_t flat_n = pnp_generator_flat_floats(g), packed_n = pnp_generator_packed_floats(g);
    const int64_t ctx_bytes = pnp_generator_workspace_bytes_yuv(g, t, sc.h, sc.w, sc.out_mask);      // ONE query for both boundaries
    const int64_t ws_bytes = ctx_bytes * sc.contexts;
    const size_t hw = (size_t)sc.h * sc.w, out_px = (size_t)t * 3 * H * W;
    float* flat = (float*)malloc((size_t)flat_n * 4);
    float* packed = (float*)malloc((size_t)packed_n * 4);
    char* ws = nullptr;
    if (ws_bytes <= 0 || posix_memalign((void**)&ws, 256, (size_t)ws_bytes)) return 2;
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
    std::vector<pnp_clip_yuv> clips8(n);
    std::vector<pnp_clip_yuv16> clips16(n);
    std::vector<ClipPlanes<1>> in8(n), out8(n);
    std::vector<ClipPlanes<2>> in16(n), out16(n);
    std::vector<void*> owned;
    for (int b = 0; b < n; ++b) {
        const std::string cb = std::to_string(b);
        float* mv = (float*)malloc((size_t)t * 4 * hw * 4);
        float* pr = (float*)malloc((size_t)t * 3 * hw * 4);
        float* of = (float*)malloc(out_px * 4);
        unsigned char* o8 = (unsigned char*)malloc(out_px);
        for (void* p : {(void*)mv, (void*)pr, (void*)of, (void*)o8}) owned.push_back(p);
        region("mvs" + cb, mv, (size_t)t * 4 * hw * 4);
        region("par" + cb, pr, (size_t)t * 3 * hw * 4);
        region("out_f32_" + cb, of, out_px * 4);
        region("out_u8_" + cb, o8, out_px);
        in8[b].make("lq8_" + cb, sc.layout, t, sc.h, sc.w, sc.ragged);
        out8[b].make("out_yuv8_" + cb, sc.layout, t, H, W, sc.ragged);
        in16[b].make("lq16_" + cb, sc.layout, t, sc.h, sc.w, sc.ragged);
        out16[b].make("out_yuv16_" + cb, sc.layout, t, H, W, sc.ragged);
        clips8[b] = pnp_clip_yuv{in8[b].d8(), mv, pr, of, o8, out8[b].d8()};
        clips16[b] = pnp_clip_yuv16{in16[b].d16(sc.depth, sc.msb), mv, pr, of, o8, out16[b].d16(sc.out_depth, sc.out_msb)};
    }
    auto inputs_written = [&]() {
        mark(flat, (size_t)flat_n * 4);
        mark(packed, (size_t)packed_n * 4);
        for (int b = 0; b < n; ++b) {
            mark(clips8[b].mvs_dev, (size_t)t * 4 * hw * 4);
            mark(clips8[b].par_dev, (size_t)t * 3 * hw * 4);
            auto mk = [](const char*, const unsigned char* p, size_t k) { mark(p, k); };      // (a row's samples, not its padding)
            each_row(yuv_planes(clips8[b].lq), t, sc.h, sc.w, mk);
            each_row(yuv_planes(clips16[b].lq), t, sc.h, sc.w, mk);
        }
    };
    // the 8-bit 4:2:0 boundary on the same handle, workspace and outputs: once to make its streams and events, once for the trace
    int rc8 = 0;
    std::vector<std::string> ref;
    for (int pass = 0; pass < 2; ++pass) {
        const auto before = written;
        const std::vector<std::string> errs = errors;
        reset();
        errors = errs;
        written = before;
        inputs_written();
        const size_t begin = trace.size();
        rc8 = pnp_generator_forward_clips_yuv(g, flat, packed, clips8.data(), n, PNP_YUV_BT709_LIMITED, sc.out_mask, slices.data(), qps.data(), bqs.data(),
                                              ws, ws_bytes, t, sc.h, sc.w, &caller);
        ref.assign(trace.begin() + begin, trace.end());
        written = before;
    }
    if (n_pack || n_from || n_to) fail("a 16-bit launcher ran at the 8-bit boundary");
    {
        const std::vector<std::string> errs = errors;
        reset();
        errors = errs;
    }
    inputs_written();
    count_writes = true;
    const size_t begin = trace.size();
    const int rc16 = pnp_generator_forward_clips_yuv16(g, flat, packed, clips16.data(), n, PNP_YUV_BT709_LIMITED, sc.out_mask, slices.data(), qps.data(),
                                                       bqs.data(), ws, ws_bytes, t, sc.h, sc.w, &caller);
    count_writes = false;
    if (rc16 != rc8) fail("the two entry points return different codes");
    const std::vector<std::string> got(trace.begin() + begin, trace.end());
    const std::vector<std::string> a = comparable(ref), c = comparable(got);
    int same = a.size() == c.size() && ref.size() == got.size() ? 1 : 0;
    size_t first_diff = 0;
    for (size_t i = 0; same == 1 && i < a.size(); ++i)
        if (a[i] != c[i]) {
            same = 0;
            first_diff = i;
            if (getenv("PNP_STUB_SHOW_DIFF")) fprintf(stderr, "line %zu: [%s] against [%s]\n", i, a[i].c_str(), c[i].c_str());
        }
    // outputs: what the mask asks for, completely; the planes sample by sample exactly once and nothing else of their blocks
    size_t expect_writes = 0;
    for (int b = 0; b < n && rc16 == 0; ++b) {
        const bool f_w = covered(clips16[b].out_f32_dev, out_px * 4), u_w = covered(clips16[b].out_u8_dev, out_px);
        if ((sc.out_mask & PNP_OUT_F32) ? !f_w : any_written(clips16[b].out_f32_dev, out_px * 4)) fail("the fp32 output is not what the mask asks for");
        if ((sc.out_mask & PNP_OUT_U8) ? !u_w : any_written(clips16[b].out_u8_dev, out_px)) fail("the uint8 output is not what the mask asks for");
        if (sc.out_mask & PNP_OUT_YUV420)
            each_row(yuv_planes(clips16[b].out_yuv16), t, H, W, [&](const char* what, const unsigned char* p, size_t k) {
                for (size_t j = 0; j < k; ++j) {
                    const auto it = out_writes.find((uintptr_t)p + j);
                    if (it == out_writes.end() || it->second != 1) return fail(std::string("a sample of ") + what + " of the output was not written exactly once");
                }
                expect_writes += k;
            });
    }
    if (rc16 == 0 && out_writes.size() != expect_writes) fail("a 16-bit output launch wrote bytes that are no sample of a requested output plane");
    const bool staged = io_staged(g);
    for (const PnpStubYuvLaunch& r : pnp_stub_yuv_log) {      // (the log was reset behind the 8-bit run)
        if (r.planes.sample_bytes != 2) {
            fail("a launch at the 16-bit boundary does not name 16-bit words");
            continue;
        }
        if (r.kind == PNP_STUB_YUV_PACK) {
            bool own = false;
            for (int b = 0; b < n; ++b) own = own || r.planes.y == (unsigned char*)clips16[b].lq.y;
            if (!own || r.frames != t || r.h != sc.h || r.w != sc.w) fail("a pack launch does not read one clip's t frames");
            if (r.fast != !sc.ragged) fail("the pack launch's form does not follow the planes' alignment");
        }
        if (r.kind == PNP_STUB_YUV_FROM && !staged) fail("a frame was converted to fp32 planes in front of a last conv that reads RGB0");
        if (r.kind == PNP_STUB_YUV_TO && (r.planes.bit_depth != sc.out_depth || r.planes.msb_aligned != sc.out_msb)) fail("the output conversion does not write the output's container");
        if (r.kind != PNP_STUB_YUV_TO && (r.planes.bit_depth != sc.depth || r.planes.msb_aligned != sc.msb)) fail("a conversion does not read the input's container");
    }
    pnp_stub_io_hook = nullptr;
    pnp_stub_yuv_hook = nullptr;
    std::vector<int> streams_used = launch_streams;
    std::sort(streams_used.begin(), streams_used.end());
    streams_used.erase(std::unique(streams_used.begin(), streams_used.end()), streams_used.end());
    printf("{\"name\": \"%s\", \"pack_rc\": %d, \"forward_rc\": %d, \"same\": %d, \"first_diff\": %zu, \"records\": %zu, \"ctx_bytes\": %lld, "
           "\"ctx_bytes_8bit_run\": %lld, \"staged\": %d, \"n_pack\": %d, \"n_pack_fast\": %d, \"n_from\": %d, \"n_to\": %d, \"n_to8\": %d, \"n_last_io\": %d, "
           "\"n8\": %d, \"frames\": %d, \"out_samples\": %zu, ",
           sc.name.c_str(), prc, rc16, same, first_diff, a.size(), (long long)ctx_bytes, (long long)(ws_bytes / sc.contexts), staged ? 1 : 0, n_pack,
           n_pack_fast, n_from, n_to, n_to8, n_last_io, n8, n * t, expect_writes / 2);
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
    for (int b = 0; b < n; ++b) in8[b].release(), out8[b].release(), in16[b].release(), out16[b].release();
    return errors.empty() ? 0 : 1;
}

}  // namespace

#undef main
int main(int argc, char** argv) {
    const pnp_generator_cfg d = default_cfg();
    pnp_generator_cfg vsr = d;
    vsr.vsr = 1;
    //   name                                 cfg prec n  t   h    w  ctx layout depth msb out: depth msb mask valu any_size ragged
    const std::vector<Scenario16> all = {
        {"plain_p010_mask7", d, 0, 1, 3, 128, 128, 1, 0, 10, 1, 10, 1, 7, 1, 0, 1},
        {"aligned_p010_mask5", d, 0, 1, 3, 128, 128, 1, 0, 10, 1, 12, 0, 5, 1, 0, 0},
        {"vsr_yuv420p12le_mask4", vsr, 0, 1, 2, 64, 96, 1, 2, 12, 0, 12, 0, 4, 1, 0, 1},
        {"f16_p010_mask6", d, 1, 1, 3, 128, 128, 1, 1, 10, 1, 10, 0, 6, 1, 0, 1},
        {"mfma_last_p012_mask2", d, 0, 1, 3, 64, 96, 1, 0, 12, 1, 12, 1, 2, 0, 0, 1},
        {"two_clips_p010_mask7", d, 0, 2, 3, 128, 128, 2, 0, 10, 1, 10, 1, 7, 1, 0, 1},
        {"any_size_66x70_yuv420p10le_mask7", d, 0, 1, 3, 66, 70, 1, 2, 10, 0, 10, 0, 7, 1, 1, 1},
    };
    int bad = 0;
    for (const Scenario16& s : all) {
        bool want = argc < 2;
        for (int i = 1; i < argc; ++i) want = want || s.name == argv[i];
        if (want) bad += run(s);
    }
    return bad ? 1 : 0;
}
