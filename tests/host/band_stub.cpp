// Host-only run of the row-band chains of the clip scheduler (pnp_generator_set_band_split) under AddressSanitizer / UBSan.
//
// TEST INFRASTRUCTURE.  Built by tests/test_band_split_host.py with a plain host compiler:
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -DPNP_HOST_STUB -Dmain=sched_stub_main
//         -x c++ tests/host/band_stub.cpp
// It reuses tests/host/sched_stub.cpp unchanged (recording launchers over csrc/generator.hip; its driver is renamed away).  The
// recording launch_conv3x3 treats every conv as a whole-frame launch -- a valid over-approximation for its range bookkeeping -- and
// keeps the ConvArgs; the split the scheduler attached to a conv (ConvArgs::band) stays readable in the handle until the next forward,
// so this driver reports, per conv in launch order: its boundary row, its `ready` event and the side stream; and the joins (the caller's stream waiting for an event recorded on the side stream).  One JSON object per scenario.
#include "sched_stub.cpp"

namespace {

struct BandScenario {
    std::string name;
    pnp_generator_cfg cfg;
    int prec, n, t, h, w, contexts, band, profile, wino, forwards, max_resident;
};

int run_band(const BandScenario& sc) {
    using namespace stub;
    errors.clear();
    written.clear();
    waits.clear();
    records.clear();
    launch_streams.clear();
    warps.clear();
    convs.clear();
    mixes.clear();
    dcn_calls = 0;
    streams_created = events_created = 0;
    regions.clear();
    trace.clear();
    pnp_stub_io_hook = trace_io;
    pnp_generator* g = nullptr;
    if (pnp_generator_create(&sc.cfg, &g)) return 2;
    pnp_generator_set_precision(g, sc.prec);
    pnp_generator_set_option(g, PNP_OPT_WINOGRAD, sc.wino);
    const int default_band = pnp_generator_get_band_split(g);
    if (sc.band >= 0) pnp_generator_set_band_split(g, sc.band);
    pnp_generator_set_max_resident(g, sc.max_resident);
    const int t = sc.t;
    const int64_t flat_n = pnp_generator_flat_floats(g), packed_n = pnp_generator_packed_floats(g);
    const int64_t ctx_bytes = pnp_generator_workspace_bytes(g, t, sc.h, sc.w);
    const int64_t ws_bytes = ctx_bytes * sc.contexts;
    const size_t hw = (size_t)sc.h * sc.w, os = sc.cfg.vsr ? 4 : 1, nt = (size_t)sc.n * t;
    float* flat = (float*)malloc((size_t)flat_n * 4);
    float* packed = (float*)malloc((size_t)packed_n * 4);
    char* ws = nullptr;
    if (ws_bytes <= 0 || posix_memalign((void**)&ws, 256, (size_t)ws_bytes)) return 2;
    float* lrs = (float*)malloc(nt * 3 * hw * 4);
    float* mvs = (float*)malloc(nt * 4 * hw * 4);
    float* par = (float*)malloc(nt * 3 * hw * 4);
    float* out = (float*)malloc(nt * 3 * hw * os * os * 4);
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
    region("out", out, nt * 3 * hw * os * os * 4);
    std::vector<float> slices, qps, bqs;
    for (int b = 0; b < sc.n; ++b) {
        const std::vector<float> sl = pattern("IBBBP", t);
        for (int i = 0; i < t; ++i) {
            slices.push_back(sl[i]);
            qps.push_back((20.f + (float)((i * 7 + b) % 20)) / 255.f);
            bqs.push_back(25.f / 255.f);
        }
    }
    pnp_stub_stream caller{0};
    const int prc = pnp_generator_pack(g, flat, packed, &caller);
    int frc = 0;
    std::vector<int> streams_after, events_after;
    for (int f = 0; f < sc.forwards && frc == 0; ++f) {
        convs.clear();
        waits.clear();
        records.clear();
        if (sc.profile) pnp_generator_profile(g, 1);
        frc = pnp_generator_forward(g, flat, packed, lrs, mvs, par, slices.data(), qps.data(), bqs.data(), out, ws, ws_bytes, sc.n, t,
                                    sc.h, sc.w, &caller);
        streams_after.push_back(streams_created);
        events_after.push_back(events_created - (int)g->prof_pool.size());
    }
    if (frc == 0 && !covered(out, nt * 3 * hw * os * os * 4)) fail("the output clip is not completely written");
    std::vector<int> row, ready, side, c0, nsrc, mode, tile, hh, stream;
    for (const ConvRec& c : convs) {
        const ConvBandSplit* b = c.a.band;
        row.push_back(b ? b->row : -1);
        ready.push_back(b && b->ready ? b->ready->id : -1);
        side.push_back(b && b->side ? b->side->id : -1);
        c0.push_back(c.a.src_c[0]);
        nsrc.push_back(c.a.nsrc);
        mode.push_back(c.a.out_mode);
        hh.push_back(c.a.H);
        stream.push_back(c.stream);
        tile.push_back((c.path == 0 && !c.a.wino_units && (conv_wino_eligible(c.a, c.cfg, c.gy) || conv_wino_ms_eligible(c.a, c.cfg, c.gy))) ? 1 : 0);
        if (c.a.tile_rows != 0 || c.a.tile_row0 != 0) fail("the scheduler restricted a conv to a row range (an op-level hook only)");
    }
    // joins: the caller's stream waits for an event recorded on another stream; for each, how many convs had been issued is not
    // known here -- the order of records is: the count of joins and that every one of them names the side stream
    std::vector<int> join_on;
    for (const Wait& wv : waits)
        if (wv.stream == 0) join_on.push_back(wv.event_recorded_on);
    double ms = 0, wk = 0;
    int64_t nl = -1;
    if (sc.profile) pnp_generator_profile_read(g, PNP_PROF_CONV_BLOCK, &ms, &nl, &wk);
    printf("{\"name\": \"%s\", \"pack_rc\": %d, \"forward_rc\": %d, \"default_band\": %d, \"rows\": %d, \"block_launches\": %lld, \"block_ms\": %.1f, ",
           sc.name.c_str(), prc, frc, default_band, (sc.h + 15) / 16, (long long)nl, ms);
    json_ints("row", row);
    json_ints("ready", ready);
    json_ints("side", side);
    json_ints("c0", c0);
    json_ints("nsrc", nsrc);
    json_ints("mode", mode);
    json_ints("conv_h", hh);
    json_ints("conv_stream", stream);
    json_ints("tile", tile);
    json_ints("join_on", join_on);
    json_ints("streams_created_after_forward", streams_after);
    json_ints("band_events_created_after_forward", events_after);
    pnp_generator_destroy(g);
    trace_dump(sc.name);
    printf("\"live_events_after_destroy\": %d, \"live_streams_after_destroy\": %d, \"errors\": [", live_events, live_streams);
    for (size_t i = 0; i < errors.size(); ++i) printf("%s\"%s\"", i ? ", " : "", errors[i].c_str());
    printf("]}\n");
    fflush(stdout);
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

#undef main
int main(int argc, char** argv) {
    const pnp_generator_cfg d = default_cfg();
    pnp_generator_cfg vsr = d, chlast = d;
    vsr.vsr = 1;
    chlast.channel_first = 0;
    chlast.one_layer = 0;
    //                                name              cfg   prec n  t   h    w   ctx band prof wino fwd k
    const std::vector<BandScenario> all = {
        {"p720_t3", d, 0, 1, 3, 720, 1280, 1, -1, 0, 1, 2, 0},
        {"p720_t3_off", d, 0, 1, 3, 720, 1280, 1, 0, 0, 1, 1, 0},
        {"p720_t3_a38", d, 0, 1, 3, 720, 1280, 1, 38, 0, 1, 1, 0},
        {"p720_t3_a45", d, 0, 1, 3, 720, 1280, 1, 45, 0, 1, 1, 0},
        {"p720_t3_profiled", d, 0, 1, 3, 720, 1280, 1, -1, 1, 1, 2, 0},
        {"p720_n2_ctx2", d, 0, 2, 2, 720, 1280, 2, -1, 0, 1, 1, 0},
        {"p720_n2_ctx1", d, 0, 2, 2, 720, 1280, 1, -1, 0, 1, 1, 0},
        {"p720_t2_f16", d, 1, 1, 2, 720, 1280, 1, -1, 0, 1, 1, 0},
        {"p720_t2_x3", d, 2, 1, 2, 720, 1280, 1, -1, 0, 1, 1, 0},
        {"p720_t2_direct", d, 0, 1, 2, 720, 1280, 1, -1, 0, 0, 1, 0},
        {"p720_t2_channel_last", chlast, 0, 1, 2, 720, 1280, 1, -1, 0, 1, 1, 0},
        {"p720_t9_bounded", d, 0, 1, 9, 720, 1280, 1, -1, 0, 1, 1, -1},
        {"rows19_t3", d, 0, 1, 3, 304, 128, 1, -1, 0, 1, 1, 0},
        {"rows18_t3", d, 0, 1, 3, 288, 144, 1, -1, 0, 1, 1, 0},
        {"rows17_t3", d, 0, 1, 3, 272, 160, 1, -1, 0, 1, 1, 0},
        {"rows16_t3", d, 0, 1, 3, 256, 160, 1, -1, 0, 1, 1, 0},
        {"vsr_rows19_t2", vsr, 0, 1, 2, 304, 128, 1, -1, 0, 1, 1, 0},
        {"small_wino2_t3", d, 0, 1, 3, 64, 64, 1, -1, 0, 2, 1, 0},
        {"small_units_t3", d, 0, 1, 3, 128, 128, 1, -1, 0, 1, 1, 0},
    };
    int bad = 0;
    for (BandScenario s : all) {
        bool want = argc < 2;
        for (int i = 1; i < argc; ++i) want = want || s.name == argv[i];
        if (!want) continue;
        if (s.max_resident < 0) {
            pnp_generator* g = nullptr;
            if (pnp_generator_create(&s.cfg, &g) == 0) {
                s.max_resident = pnp_generator_min_resident(g, s.t);
                pnp_generator_destroy(g);
            }
        }
        bad += run_band(s);
    }
    return bad ? 1 : 0;
}
