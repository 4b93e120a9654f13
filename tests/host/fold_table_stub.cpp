// Host-only checks of the Winograd front halves' fold table (csrc/fold_table.h) under AddressSanitizer / UBSan.
//
// TEST INFRASTRUCTURE.  Built by tests/test_fold_table_host.py with a plain host compiler:
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -DPNP_HOST_STUB -Dmain=sched_stub_main
//         -x c++ tests/host/fold_table_stub.cpp
// Two modes.
//   fold_table_stub table H W in.f32 out.i32   the table of one (3, H, W) map by csrc/fold_table.h's own host loop (the rule and the
//       index function the kernel uses), from and into exact-size heap blocks; the Python test compares it with its numpy restatement
//   fold_table_stub [scenario ...]             the clip scheduler (csrc/generator.hip) over tests/host/sched_stub.cpp, unchanged: the
//       table's launcher is recorded by csrc/host_stub/fold_stub.h; the hook below gives it the range bookkeeping the other launchers
//       get (the planes it reads must have been written, the table it writes must lie inside the workspace) and notes how many
//       convs had been issued before it.  Afterwards every conv that carries a table (ConvArgs::fold_tab) is checked against the
//       launches in issue order: the LATEST launch that wrote its table before it must exist, must have read this conv's own partition
//       planes (so the table is the frame's, written before its first reader and not rewritten for another frame while the run
//       that reads it is open) and must have been issued on the stream of the run's chain A, in front of the run's first conv.
#include "sched_stub.cpp"

#include "../../pnp_vcve_amd/csrc/fold_table.h"

namespace {

struct FoldRec {
    PnpStubFoldLaunch l;
    size_t convs_before;
    int stream;
};
std::vector<FoldRec> fold_launches;

void fold_hook(const PnpStubFoldLaunch& r) {
    using namespace stub;
    cur = "launch_par_fold_table";
    const size_t hw = (size_t)r.h * r.w;
    for (int f = 0; f < r.frames; ++f) RD("the partition planes", r.par + (size_t)f * 3 * r.plane, (size_t)(2 * r.plane + hw) * 4);
    WR("the fold table", r.tab, (size_t)r.frames * pnp_fold_records(r.h, r.w) * sizeof(PnpFoldRec));
    fold_launches.push_back({r, convs.size(), sid(r.stream)});
}

struct FoldScenario {
    std::string name;
    pnp_generator_cfg cfg;
    int prec, n, t, h, w, contexts, wino, par_skip, max_resident;      // max_resident < 0: the clip's minimum (bounded schedule)
};

int run_fold(FoldScenario sc) {
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
    fold_launches.clear();
    pnp_stub_fold_log.clear();
    pnp_stub_io_hook = trace_io;
    pnp_stub_fold_hook = fold_hook;
    pnp_generator* g = nullptr;
    if (pnp_generator_create(&sc.cfg, &g)) return 2;
    pnp_generator_set_precision(g, sc.prec);
    pnp_generator_set_option(g, PNP_OPT_WINOGRAD, sc.wino);
    pnp_generator_set_option(g, PNP_OPT_PAR_SKIP, sc.par_skip);
    if (sc.max_resident < 0) sc.max_resident = pnp_generator_min_resident(g, sc.t);
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
    const int frc = pnp_generator_forward(g, flat, packed, lrs, mvs, par, slices.data(), qps.data(), bqs.data(), out, ws, ws_bytes, sc.n, t,
                                          sc.h, sc.w, &caller);
    if (frc == 0 && !covered(out, nt * 3 * hw * os * os * 4)) fail("the output clip is not completely written");
    // ---- every conv with a table against the launches, in issue order
    const size_t tab_bytes = (size_t)pnp_fold_records(sc.h, sc.w) * sizeof(PnpFoldRec);
    int readers = 0, gated_without = 0, table_without_gate = 0, units_with = 0;
    std::vector<int> readers_of(fold_launches.size(), 0), launch_stream, launch_in_ws, first_reader_after;
    for (size_t k = 0; k < convs.size(); ++k) {
        const ConvArgs& a = convs[k].a;
        const bool tile = convs[k].path == 0 && !a.wino_units && conv_wino_eligible(a, convs[k].cfg, convs[k].gy);
        if (a.fold_tab && !a.par_any) ++table_without_gate;
        if (a.fold_tab && !tile) ++units_with;
        if (a.par_any && tile && !a.fold_tab) ++gated_without;
        if (!a.fold_tab) continue;
        ++readers;
        cur = "a gated front half";
        RD("the frame's fold table", a.fold_tab, tab_bytes);
        int latest = -1;
        for (size_t j = 0; j < fold_launches.size(); ++j)
            if (fold_launches[j].convs_before <= k && fold_launches[j].l.tab == a.fold_tab) latest = (int)j;
        if (latest < 0) {
            fail("conv " + std::to_string(k) + " reads a fold table no launch wrote before it");
            continue;
        }
        const FoldRec& fr = fold_launches[latest];
        if (fr.l.par != a.par) fail("conv " + std::to_string(k) + " reads a fold table made from another frame's planes (rewritten while its run was open?)");
        if (fr.l.h != a.H || fr.l.w != a.W || fr.l.plane != a.par_plane || fr.l.frames != 1) fail("conv " + std::to_string(k) + ": the table's launch had another shape");
        ++readers_of[latest];
    }
    for (size_t j = 0; j < fold_launches.size(); ++j) {
        const FoldRec& fr = fold_launches[j];
        launch_stream.push_back(fr.stream);
        launch_in_ws.push_back((const char*)fr.l.tab >= ws && (const char*)fr.l.tab + tab_bytes <= ws + ws_bytes ? 1 : 0);
        // the first conv issued behind the launch is the run's input conv, on the launch's stream (chain A; chain B waits for an event
        // recorded on that stream behind the launch)
        int ok = 0;
        if (fr.convs_before < convs.size()) ok = convs[fr.convs_before].stream == fr.stream && convs[fr.convs_before].a.src_c[0] == 4;
        first_reader_after.push_back(ok);
    }
    printf("{\"name\": \"%s\", \"pack_rc\": %d, \"forward_rc\": %d, \"convs\": %zu, \"launches\": %zu, \"readers\": %d, \"gated_tile_convs_without_table\": %d, "
           "\"tables_without_gate\": %d, \"tables_on_other_kernels\": %d, \"context_bytes\": %lld, ",
           sc.name.c_str(), prc, frc, convs.size(), fold_launches.size(), readers, gated_without, table_without_gate, units_with, (long long)ctx_bytes);
    json_ints("readers_of_launch", readers_of);
    json_ints("launch_stream", launch_stream);
    json_ints("launch_in_workspace", launch_in_ws);
    json_ints("input_conv_follows_on_the_same_stream", first_reader_after);
    pnp_generator_destroy(g);
    trace_dump(sc.name);
    printf("\"errors\": [");
    for (size_t i = 0; i < errors.size(); ++i) printf("%s\"%s\"", i ? ", " : "", errors[i].c_str());
    printf("]}\n");
    fflush(stdout);
    pnp_stub_fold_hook = nullptr;
    free(flat);
    free(packed);
    free(ws);
    free(lrs);
    free(mvs);
    free(par);
    free(out);
    return errors.empty() ? 0 : 1;
}

int table_mode(int argc, char** argv) {
    if (argc != 6) return 2;
    const int h = atoi(argv[2]), w = atoi(argv[3]);
    if (h < 1 || w < 1) return 2;
    const size_t hw = (size_t)h * w, nrec = (size_t)pnp_fold_records(h, w);
    float* par = (float*)malloc(3 * hw * 4);
    PnpFoldRec* tab = (PnpFoldRec*)malloc(nrec * sizeof(PnpFoldRec));
    FILE* fi = fopen(argv[4], "rb");
    if (!fi || fread(par, 4, 3 * hw, fi) != 3 * hw) return 3;
    fclose(fi);
    memset(tab, 0xAB, nrec * sizeof(PnpFoldRec));      // (every record must be written)
    pnp_fold_table_host(par, (long)hw, h, w, tab);
    FILE* fo = fopen(argv[5], "wb");
    if (!fo || fwrite(tab, sizeof(PnpFoldRec), nrec, fo) != nrec) return 3;
    fclose(fo);
    free(par);
    free(tab);
    return 0;
}

}  // namespace

#undef main
int main(int argc, char** argv) {
    static_assert(sizeof(PnpFoldRec) == 8, "a record is two 32-bit words");
    if (argc >= 2 && std::string(argv[1]) == "table") return table_mode(argc, argv);
    const pnp_generator_cfg d = default_cfg();
    pnp_generator_cfg chlast = d, sparse = d;
    chlast.channel_first = 0;
    chlast.one_layer = 0;
    sparse.sparse_val = 1;
    //                            name                   cfg   prec n  t   h    w   ctx wino skip k
    const std::vector<FoldScenario> all = {
        {"plain_wino2_t3", d, 0, 1, 3, 64, 64, 1, 2, 1, 0},
        {"plain_ragged_t3", d, 0, 1, 3, 100, 132, 1, 2, 1, 0},
        {"channel_last_t3", chlast, 0, 1, 3, 64, 64, 1, 2, 1, 0},
        {"p720_t2", d, 0, 1, 2, 720, 1280, 1, 1, 1, 0},
        {"bounded_t9", d, 0, 1, 9, 64, 64, 1, 2, 1, -1},
        {"bounded_sparse_t9", sparse, 0, 1, 9, 64, 64, 1, 2, 1, -1},
        {"sparse_t3", sparse, 0, 1, 3, 64, 64, 1, 2, 1, 0},
        {"two_contexts_n2", d, 0, 2, 3, 64, 64, 2, 2, 1, 0},
        {"one_context_n2", d, 0, 2, 3, 64, 64, 1, 2, 1, 0},
        {"p720_two_contexts_n3", d, 0, 3, 2, 720, 1280, 2, 1, 1, 0},
        {"units_128_t3", d, 0, 1, 3, 128, 128, 1, 1, 1, 0},
        {"no_skip_t3", d, 0, 1, 3, 64, 64, 1, 2, 0, 0},
        {"direct_t3", d, 0, 1, 3, 64, 64, 1, 0, 1, 0},
        {"f16_t3", d, 1, 1, 3, 64, 64, 1, 2, 1, 0},
    };
    int bad = 0;
    for (const FoldScenario& s : all) {
        bool want = argc < 2;
        for (int i = 1; i < argc; ++i) want = want || s.name == argv[i];
        if (want) bad += run_fold(s);
    }
    return bad ? 1 : 0;
}
