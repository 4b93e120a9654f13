// Host-only run of the clip scheduler with pnp_generator_set_any_size on, under AddressSanitizer / UBSan: frames whose height and
// width are no multiple of 4 (nor of the 16-pixel tile, the 8x8 quadrant or the 8x16 flag tile).
//
// TEST INFRASTRUCTURE.  Built by tests/test_any_size_host.py with a plain host compiler:
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -DPNP_HOST_STUB -Dmain=sched_stub_main
//         -x c++ tests/host/any_size_stub.cpp
// It reuses tests/host/sched_stub.cpp unchanged: recording launchers over csrc/generator.hip that check every byte range a kernel
// would touch against ASan's shadow and against what has been written so far.  Every tensor of every clip is its own heap block of
// exactly the size the ABI names.  A byte clip starts at a deliberately odd offset inside its block, and the bytes in front of it are
// poisoned: a launcher that reads or writes one byte outside [clip, clip + t*h*w*3) lands in poison.  One JSON object per scenario:
//   * "plain": fp32 planes through pnp_generator_forward;
//   * "bounded": the same under the bounded schedule at its minimum k;
//   * "clips": two clips by pointer, bytes in and both outputs, at odd addresses;
//   * "heads": the x4 heads (4h x 4w outputs).
// Every scenario must return PNP_OK, leave no range error, and write every output frame exactly once.
#include "sched_stub.cpp"

namespace {

using namespace stub;

int n_pack = 0, n_last_io = 0;
std::vector<std::pair<uintptr_t, uintptr_t>> out_writes;      // [lo, hi) of every write of an output frame (fp32 planes or bytes)

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
            RD("a byte frame", r.in, px * 3);
            WR("a frame of fp32 planes", r.out, px * 12);
            break;
        case PNP_STUB_IO_TO_RGB8:
            cur = "launch_frames_to_rgb8";
            RD("a frame of fp32 planes", r.in, px * 12);
            WR("a byte frame", r.out, px * 3);
            out_writes.push_back({(uintptr_t)r.out, (uintptr_t)r.out + px * 3});
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
            if (a.out) {
                WR("the output frame", a.out, hw * 12);
                out_writes.push_back({(uintptr_t)a.out, (uintptr_t)a.out + hw * 12});
            }
            if (a.out_u8) {
                WR("the output frame's bytes", a.out_u8, hw * 3);
                out_writes.push_back({(uintptr_t)a.out_u8, (uintptr_t)a.out_u8 + hw * 3});
            }
        }
    }
}

struct AnyScenario {
    std::string name, kind;      // kind: "plain" | "bounded" | "clips" | "heads"
    int t, h, w;
};

// a block of `bytes` usable bytes that starts `odd` bytes into its heap block, the bytes in front poisoned
struct OddBlock {
    char* base = nullptr;
    size_t odd = 0;
    void* ptr() const { return base + odd; }
    void make(size_t bytes, size_t odd_) {
        odd = odd_;
        base = (char*)malloc(bytes + odd);
#if PNP_HAVE_ASAN
        if (odd) ASAN_POISON_MEMORY_REGION(base, odd);
#endif
    }
    void release() {
#if PNP_HAVE_ASAN
        if (odd) ASAN_UNPOISON_MEMORY_REGION(base, odd);
#endif
        free(base);
    }
};

// every byte of [p, p + n) is covered by exactly one of the recorded output writes
bool written_once(const void* p, size_t n, std::string* why) {
    const uintptr_t lo = (uintptr_t)p, hi = lo + n;
    std::vector<std::pair<uintptr_t, uintptr_t>> in;
    for (const auto& iv : out_writes)
        if (iv.first < hi && iv.second > lo) in.push_back(iv);
    std::sort(in.begin(), in.end());
    uintptr_t at = lo;
    for (const auto& iv : in) {
        if (iv.first < at) { *why = "an output range is written twice"; return false; }
        if (iv.first > at) { *why = "an output range is never written"; return false; }
        at = iv.second;
    }
    if (at != hi) { *why = at < hi ? "the end of an output is never written" : "a write runs past the end of an output"; return false; }
    return true;
}

int run_any(const AnyScenario& sc) {
    errors.clear();
    written.clear();
    waits.clear();
    records.clear();
    launch_streams.clear();
    warps.clear();
    convs.clear();
    mixes.clear();
    pnp_stub_io_log.clear();
    out_writes.clear();
    regions.clear();
    trace.clear();
    n_pack = n_last_io = 0;
    pnp_generator_cfg cfg = default_cfg();
    cfg.num_blocks = 2;
    cfg.vsr = sc.kind == "heads" ? 1 : 0;
    pnp_generator* g = nullptr;
    if (pnp_generator_create(&cfg, &g)) return 2;
    const bool clips_mode = sc.kind == "clips";
    const int t = sc.t, n = clips_mode ? 2 : 1, h = sc.h, w = sc.w;
    const int64_t off_bytes = pnp_generator_workspace_bytes(g, t, h, w);
    // the refusals of the switch's off state, then the switch
    const float one_side[1] = {73.f};
    const int rc_off = pnp_generator_forward(g, nullptr, nullptr, nullptr, nullptr, nullptr, one_side, one_side, one_side, nullptr, nullptr, 0, 1, 1, h, w, nullptr);
    if (((h % 4) || (w % 4)) && rc_off != PNP_ERR_SIZE_VALUE) fail("with any_size off the frame is not refused with PNP_ERR_SIZE_VALUE");
    if (pnp_generator_set_any_size(g, 1) != PNP_OK || pnp_generator_get_any_size(g) != 1) fail("pnp_generator_set_any_size");
    if (sc.kind == "bounded") pnp_generator_set_max_resident(g, pnp_generator_min_resident(g, t));
    const int fmt = clips_mode ? PNP_FRAMES_U8_HWC : PNP_FRAMES_F32_NCHW, mask = clips_mode ? (PNP_OUT_F32 | PNP_OUT_U8) : PNP_OUT_F32;
    const int64_t flat_n = pnp_generator_flat_floats(g), packed_n = pnp_generator_packed_floats(g);
    const int64_t ctx_bytes = pnp_generator_workspace_bytes_io(g, t, h, w, fmt, mask);
    if (sc.kind == "plain" && ctx_bytes != off_bytes) fail("the switch changes the workspace size");
    // (two workspace contexts, except at 1078x1918: one, so that the two clips run one after the other with row-band chains)
    const int64_t ws_bytes = ctx_bytes * (h >= 1000 ? 1 : n);
    const size_t hw = (size_t)h * w, os = cfg.vsr ? 4 : 1;
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
        const std::vector<float> sl = pattern(b ? "IPBBPBBPB" : "IBBBPBBBP", t);
        for (int i = 0; i < t; ++i) {
            slices.push_back(sl[i]);
            qps.push_back((20.f + (float)((i * 7 + b) % 20)) / 255.f);
            bqs.push_back((b ? 35.f : 25.f) / 255.f);
        }
    }
    pnp_stub_stream caller{0};
    const int prc = pnp_generator_pack(g, flat, packed, &caller);
    pnp_stub_io_hook = io_hook;
    const size_t lq_bytes = (size_t)t * 3 * hw * (clips_mode ? 1 : 4), out_px = (size_t)t * 3 * hw * os * os;
    std::vector<pnp_clip_io> clips(n);
    std::vector<OddBlock> blocks;
    for (int b = 0; b < n; ++b) {
        // byte tensors at offsets 1 and 3 (clip 0), 2 and 1 (clip 1); fp32 tensors where malloc puts them
        OddBlock lq, mv, pr, of, o8;
        lq.make(lq_bytes, clips_mode ? (b ? 2 : 1) : 0);
        mv.make((size_t)t * 4 * hw * 4, 0);
        pr.make((size_t)t * 3 * hw * 4, 0);
        of.make(out_px * 4, 0);
        o8.make(out_px, b ? 1 : 3);
        for (const OddBlock& k : {lq, mv, pr, of, o8}) blocks.push_back(k);
        mark(lq.ptr(), lq_bytes);
        mark(mv.ptr(), (size_t)t * 4 * hw * 4);
        mark(pr.ptr(), (size_t)t * 3 * hw * 4);
        const std::string cb = std::to_string(b);
        region("lq" + cb, lq.ptr(), lq_bytes);
        region("mvs" + cb, mv.ptr(), (size_t)t * 4 * hw * 4);
        region("par" + cb, pr.ptr(), (size_t)t * 3 * hw * 4);
        region("out_f32_" + cb, of.ptr(), out_px * 4);
        region("out_u8_" + cb, o8.ptr(), out_px);
        clips[b] = pnp_clip_io{lq.ptr(), (const float*)mv.ptr(), (const float*)pr.ptr(), (float*)of.ptr(), (unsigned char*)o8.ptr()};
    }
    int frc;
    if (clips_mode) {
        frc = pnp_generator_forward_clips(g, flat, packed, clips.data(), n, fmt, mask, slices.data(), qps.data(), bqs.data(), ws, ws_bytes, t, h, w, &caller);
    } else {
        frc = pnp_generator_forward(g, flat, packed, (const float*)clips[0].lq_dev, clips[0].mvs_dev, clips[0].par_dev, slices.data(), qps.data(),
                                    bqs.data(), clips[0].out_f32_dev, ws, ws_bytes, 1, t, h, w, &caller);
    }
    pnp_stub_io_hook = nullptr;
    // the fp32 heads that went through launch_conv3x3 (the fp32 boundary): their output frames
    for (const ConvRec& c : convs)
        if (c.a.out_mode == 2 || c.a.out_mode == 3) out_writes.push_back({(uintptr_t)c.a.out, (uintptr_t)c.a.out + (size_t)c.a.H * c.a.W * 12});
    std::string why;
    for (int b = 0; b < n && frc == 0; ++b) {
        if (!written_once(clips[b].out_f32_dev, out_px * 4, &why)) fail("fp32 output of clip " + std::to_string(b) + ": " + why);
        if (clips_mode && !written_once(clips[b].out_u8_dev, out_px, &why)) fail("uint8 output of clip " + std::to_string(b) + ": " + why);
        if (!clips_mode && any_of(out_writes.begin(), out_writes.end(), [&](const std::pair<uintptr_t, uintptr_t>& iv) {
                return iv.first < (uintptr_t)clips[b].out_u8_dev + out_px && iv.second > (uintptr_t)clips[b].out_u8_dev; }))
            fail("the uint8 output was written although the mask does not ask for it");
    }
    int banded = 0, tiles = 0, units = 0;
    for (const ConvRec& c : convs) {
        banded += c.a.band ? 1 : 0;
        const bool wino = c.path == 0 && (conv_wino_eligible(c.a, c.cfg, c.gy) || conv_wino_ms_eligible(c.a, c.cfg, c.gy));
        tiles += (wino && !c.a.wino_units) ? 1 : 0;
        units += (wino && c.a.wino_units) ? 1 : 0;
        if (c.a.band && (c.a.band->row < 1 || c.a.band->row >= (h + 15) / 16)) fail("a band boundary outside the frame's tile rows");
    }
    printf("{\"name\": \"%s\", \"kind\": \"%s\", \"pack_rc\": %d, \"forward_rc\": %d, \"rc_off\": %d, \"ctx_bytes\": %lld, \"n_pack\": %d, "
           "\"n_last_io\": %d, \"convs\": %zu, \"banded\": %d, \"wino_tiles\": %d, \"wino_units\": %d, \"frames\": %d, ",
           sc.name.c_str(), sc.kind.c_str(), prc, frc, rc_off, (long long)ctx_bytes, n_pack, n_last_io, convs.size(), banded, tiles, units, n * t);
    pnp_generator_destroy(g);
    trace_dump(sc.name);
    printf("\"errors\": [");
    for (size_t i = 0; i < errors.size(); ++i) printf("%s\"%s\"", i ? ", " : "", errors[i].c_str());
    printf("]}\n");
    fflush(stdout);
    free(flat);
    free(packed);
    free(ws);
    for (OddBlock& k : blocks) k.release();
    return errors.empty() ? 0 : 1;
}

}  // namespace

#undef main
int main(int argc, char** argv) {
    std::vector<AnyScenario> all;
    const int sizes[6][2] = {{65, 65}, {66, 79}, {73, 67}, {177, 193}, {480, 854}, {1078, 1918}};
    for (const auto& s : sizes) {
        const std::string sz = std::to_string(s[0]) + "x" + std::to_string(s[1]);
        const bool big = s[0] >= 1000;      // (a 1078x1918 map is 529 MB: fewer frames)
        all.push_back({"plain_" + sz, "plain", big ? 2 : 3, s[0], s[1]});
        all.push_back({"bounded_" + sz, "bounded", big ? 5 : 9, s[0], s[1]});
        all.push_back({"clips_" + sz, "clips", big ? 2 : 3, s[0], s[1]});
        // the x4 heads: up to where the 16x maps still fit 32-bit offsets (480x854 -> 1920x3416)
        if (!big) all.push_back({"heads_" + sz, "heads", 2, s[0], s[1]});
    }
    int bad = 0;
    for (const AnyScenario& s : all) {
        bool want = argc < 2;
        for (int i = 1; i < argc; ++i) want = want || s.name == argv[i];
        if (want) bad += run_any(s);
    }
    return bad ? 1 : 0;
}
