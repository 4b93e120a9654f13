// Host-only check of the prefetched per-frame Winograd images (pnp_vcve_amd/csrc/generator.hip: branch_images, the two buffers of
// Workspace::wino).  TEST INFRASTRUCTURE, built by tests/test_host_wino_prefetch.py like sched_stub.cpp, which this file #includes
// whole (HIP stand-ins, recording launchers, the scheduler itself); only its driver is replaced.
//
// The recording launchers keep the convs in launch order but not the image launches.  The scheduler hands launch_wino_images the
// `data()` of two vectors -- `const float**` and `float**` -- so an overload with exactly these parameter types, declared before the
// scheduler is compiled, is the better match: it notes where in the conv sequence the launch sits, what it writes and how many stream
// waits were made before it, then calls the recording launcher.
//
// Checked per scenario (one JSON object each):
//   * every conv that reads an image of W.wino reads what the launch made FOR ITS RUN wrote (launch number r <-> branch run number r),
//     and that launch was issued before the run's input conv: written before read, and off the run's chains;
//   * no image launch sits between a run's input conv and its last conv and writes what that run reads: not rewritten while a chain
//     that reads it is open;
//   * when an image launch is issued, every run of its stream up to the last reader of the
//     buffer it writes (run r - 2) that ran as row-band chains (ConvArgs::band: a conv's second
//     launch goes to the chain's side stream) has been joined to that stream.
#include <vector>

#include "../../pnp_vcve_amd/csrc/conv_mfma.h"

int launch_wino_images(const float** src, float** dst, int n, const float* gamma, hipStream_t s);

#define main sched_stub_main
#include "sched_stub.cpp"
#undef main

namespace {

struct ImgEv {
    size_t conv_index, nwaits;
    int stream;
    std::vector<const float*> dst;
};
std::vector<ImgEv> img_events;

}  // namespace

int launch_wino_images(const float** src, float** dst, int n, const float* gamma, hipStream_t s) {
    if (!stub::mixes.empty()) {      // (the pack's static images come before any expert mixture: not recorded)
        ImgEv e{stub::convs.size(), stub::waits.size(), stub::sid(s), {}};
        for (int i = 0; i < n; ++i) e.dst.push_back(dst[i]);
        img_events.push_back(e);
    }
    return launch_wino_images(static_cast<const float* const*>(src), static_cast<float* const*>(dst), n, gamma, s);
}

namespace {

struct Case {
    const char* name;
    pnp_generator_cfg cfg;
    int n, t, h, w, contexts, wino, bound;      // bound: 0 = every frame resident, -1 = the smallest bound
    const char* pat;
};

int run_case(const Case& cs) {
    using namespace stub;
    errors.clear();
    written.clear();
    waits.clear();
    records.clear();
    launch_streams.clear();
    warps.clear();
    convs.clear();
    mixes.clear();
    img_events.clear();
    regions.clear();
    trace.clear();
    pnp_stub_io_hook = trace_io;
    pnp_generator* g = nullptr;
    if (pnp_generator_create(&cs.cfg, &g)) return 2;
    pnp_generator_set_precision(g, PNP_PREC_F32);
    pnp_generator_set_option(g, PNP_OPT_WINOGRAD, cs.wino);
    int bound_rc = 0;
    if (cs.bound) bound_rc = pnp_generator_set_max_resident(g, pnp_generator_min_resident(g, cs.t));
    const int64_t flat_n = pnp_generator_flat_floats(g), packed_n = pnp_generator_packed_floats(g);
    const int64_t ctx_bytes = pnp_generator_workspace_bytes(g, cs.t, cs.h, cs.w), ws_bytes = ctx_bytes * cs.contexts;
    const size_t hw = (size_t)cs.h * cs.w, nt = (size_t)cs.n * cs.t;
    float* flat = (float*)malloc((size_t)flat_n * 4);
    float* packed = (float*)malloc((size_t)packed_n * 4);
    char* ws = nullptr;
    if (posix_memalign((void**)&ws, 256, (size_t)ws_bytes)) return 2;
    float* lrs = (float*)malloc(nt * 3 * hw * 4);
    float* mvs = (float*)malloc(nt * 4 * hw * 4);
    float* par = (float*)malloc(nt * 3 * hw * 4);
    float* out = (float*)malloc(nt * 3 * hw * 4);
    mark(flat, (size_t)flat_n * 4);
    mark(lrs, nt * 3 * hw * 4);
    mark(mvs, nt * 4 * hw * 4);
    mark(par, nt * 3 * hw * 4);
    region("flat", flat, (size_t)flat_n * 4);
    region("packed", packed, (size_t)packed_n * 4);
    region("ws", ws, (size_t)ws_bytes);
    region("lrs", lrs, nt * 3 * hw * 4);
    region("mvs", mvs, nt * 4 * hw * 4);
    region("par", par, nt * 3 * hw * 4);
    region("out", out, nt * 3 * hw * 4);
    std::vector<float> sl, qp, bq;
    for (int b = 0; b < cs.n; ++b) {
        const std::vector<float> p = pattern(cs.pat, cs.t);
        for (int i = 0; i < cs.t; ++i) {
            sl.push_back(p[i]);
            qp.push_back((20.f + (float)((i * 7 + b) % 20)) / 255.f);
            bq.push_back(25.f / 255.f);
        }
    }
    pnp_stub_stream caller{0};
    const int prc = pnp_generator_pack(g, flat, packed, &caller);
    const int frc = pnp_generator_forward(g, flat, packed, lrs, mvs, par, sl.data(), qp.data(), bq.data(), out, ws, ws_bytes, cs.n, cs.t,
                                          cs.h, cs.w, &caller);
    // ---- the records
    auto in_wino = [&](const float* p) {      // inside some context's image buffers
        for (int k = 0; k < cs.contexts; ++k) {
            const Workspace W = carve(g, ws + (int64_t)k * ctx_bytes, cs.t, cs.h, cs.w);
            if (W.wino && p >= W.wino && p < W.wino + (int64_t)4 * cs.cfg.num_blocks * PNP_WINO_IMG_FLOATS) return true;
        }
        return false;
    };
    std::vector<size_t> run_start;            // conv index of every branch run's input conv (its first source is the RGB frame)
    for (size_t i = 0; i < convs.size(); ++i)
        if (convs[i].a.src_c[0] == 4) run_start.push_back(i);
    if (run_start.size() != img_events.size())
        fail("image launches " + std::to_string(img_events.size()) + " != branch runs " + std::to_string(run_start.size()));
    int reads = 0, side_convs = 0, buffers_seen[2] = {0, 0};
    for (size_t r = 0; r < run_start.size() && r < img_events.size(); ++r) {
        const size_t rs = run_start[r], re = r + 1 < run_start.size() ? run_start[r + 1] : convs.size();
        const ImgEv& mine = img_events[r];
        if (mine.conv_index > rs) fail("run " + std::to_string(r) + ": its images are launched behind its input conv (inside its chains)");
        for (const float* d : mine.dst)
            if (!in_wino(d)) fail("run " + std::to_string(r) + ": an image is written outside Workspace::wino");
        for (size_t i = rs; i < re; ++i) {
            const ConvArgs& a = convs[i].a;
            if (a.band) ++side_convs;      // (a conv of a row-band chain: its second launch goes to the chain's side stream)
            if (!a.wwino || !in_wino(a.wwino)) continue;
            ++reads;
            // the last launch in front of this conv that wrote the image it reads must be the run's own
            int writer = -1;
            for (size_t e = 0; e < img_events.size(); ++e)
                if (img_events[e].conv_index <= i && std::find(img_events[e].dst.begin(), img_events[e].dst.end(), a.wwino) != img_events[e].dst.end())
                    writer = (int)e;
            if (writer != (int)r)
                fail("run " + std::to_string(r) + " conv " + std::to_string(i) + " reads an image last written by launch " + std::to_string(writer));
            // ... and no launch inside the run writes it
            for (const ImgEv& e : img_events)
                if (e.conv_index > rs && e.conv_index < re && std::find(e.dst.begin(), e.dst.end(), a.wwino) != e.dst.end())
                    fail("run " + std::to_string(r) + ": an image it reads is rewritten while the run is open");
        }
        for (int k = 0; k < cs.contexts; ++k) {
            const Workspace W = carve(g, ws + (int64_t)k * ctx_bytes, cs.t, cs.h, cs.w);
            if (W.wino && !mine.dst.empty() && mine.dst[0] >= W.wino && mine.dst[0] < W.wino + (int64_t)4 * cs.cfg.num_blocks * PNP_WINO_IMG_FLOATS)
                ++buffers_seen[(mine.dst[0] - W.wino) / ((int64_t)2 * cs.cfg.num_blocks * PNP_WINO_IMG_FLOATS)];
        }
        // every earlier run of this stream that forked a side chain has been joined when the launch is issued
        int forked = 0, joins = 0;
        for (size_t q = 0; q + 1 < r; ++q) {      // (run r - 1 comes behind this launch; run r - 2 was the last to read this buffer)
            bool side = false;
            for (size_t i = run_start[q]; i < run_start[q + 1]; ++i) side = side || convs[i].a.band != nullptr;
            if (side && convs[run_start[q]].stream == mine.stream) ++forked;
        }
        for (size_t k = 0; k < mine.nwaits && k < waits.size(); ++k)
            if (waits[k].stream == mine.stream && waits[k].event_recorded_on != mine.stream) ++joins;
        if (joins < forked) fail("run " + std::to_string(r) + ": its images are launched with " + std::to_string(forked - joins) + " chain(s) not joined");
    }
    pnp_generator_destroy(g);
    trace_dump(cs.name);
    printf("{\"name\": \"%s\", \"pack_rc\": %d, \"forward_rc\": %d, \"bound_rc\": %d, \"runs\": %zu, \"image_launches\": %zu, \"image_reads\": %d, "
           "\"side_stream_convs\": %d, \"launches_into_buffer\": [%d, %d], \"errors\": [",
           cs.name, prc, frc, bound_rc, run_start.size(), img_events.size(), reads, side_convs, buffers_seen[0], buffers_seen[1]);
    for (size_t i = 0; i < errors.size(); ++i) printf("%s\"%s\"", i ? ", " : "", errors[i].c_str());
    printf("]}\n");
    free(flat);
    free(packed);
    free(ws);
    free(lrs);
    free(mvs);
    free(par);
    free(out);
    return errors.empty() ? 0 : 1;
}

}  // namespace

int main() {
    const pnp_generator_cfg d = default_cfg();
    pnp_generator_cfg chlast = d;
    chlast.channel_first = 0;
    chlast.one_layer = 0;
    const Case cases[] = {
        {"plain_p720_t3", d, 1, 3, 720, 1280, 1, 1, 0, "IBBBP"},                // row-band chains: a side stream per run
        {"plain_two_layer_t4", chlast, 1, 4, 64, 64, 1, 2, 0, "IBBBP"},         // 16 images per run, quadrant units
        {"bounded_t12", d, 1, 12, 64, 96, 1, 2, -1, "IBBBP"},                   // the smallest bound: recomputed runs
        {"two_contexts_n2_t3", d, 2, 3, 64, 64, 2, 2, 0, "IBBBP"},
    };
    int bad = 0;
    for (const Case& c : cases) bad += run_case(c);
    return bad ? 1 : 0;
}
