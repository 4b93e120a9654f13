// Host-only run of the bounded-memory clip schedule (pnp_generator_set_max_resident) under AddressSanitizer / UBSan.
//
// TEST INFRASTRUCTURE.  Built by tests/test_long_clip_host.py with a plain host compiler:
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -DPNP_HOST_STUB -Dmain=sched_stub_main
//         -x c++ tests/host/long_clip_stub.cpp
// It reuses tests/host/sched_stub.cpp unchanged (recording launchers over csrc/generator.hip; its own driver is renamed away by
// -Dmain=...): every byte range a kernel would touch must lie inside the buffer the C ABI sized, and nothing may be read before
// something wrote it.  On top of that this driver follows every frame map LOGICALLY: the map written by the last block of a branch
// run is tagged with (sample, sweep, frame), and each alignment source, neighbour, own backward feature and head input is looked up
// by its address.  A bounded run must read, at every step, the same logical frames as the unbounded run of the same clip -- a map
// that was overwritten too early shows up as the wrong tag even though its bytes were "written".  One JSON object per scenario.
#include <tuple>

#include "sched_stub.cpp"

namespace {

struct LcScenario {
    std::string name;
    pnp_generator_cfg cfg;
    int prec, n, t, h, w, contexts, k, mirrors, wino;
    std::string pattern;
};

// a branch run as the records show it: which logical maps it read (-1 = none), encoded (sample * 2 + sweep) * 100000 + frame
struct StepRec {
    int sample, sweep, frame;
    int key, nb, own, warp_plane;
    bool operator==(const StepRec& o) const {
        return sample == o.sample && sweep == o.sweep && frame == o.frame && key == o.key && nb == o.nb && own == o.own &&
               warp_plane == o.warp_plane;
    }
};

int enc(int sample, int sweep, int frame) { return (sample * 2 + sweep) * 100000 + frame; }

struct LcResult {
    int create_rc = 0, pack_rc = 0, forward_rc = 0, ws_rc = 0;
    int64_t ctx_bytes = 0;
    int input_convs = 0, head_reads = 0, plan_r = -1, plan_l = -1;
    std::vector<StepRec> steps;
    std::vector<std::string> errors;
};

LcResult run_lc(const LcScenario& sc, int k) {
    using namespace stub;
    LcResult res;
    errors.clear();
    written.clear();
    waits.clear();
    records.clear();
    launch_streams.clear();
    warps.clear();
    convs.clear();
    mixes.clear();
    dcn_calls = 0;
    regions.clear();
    trace.clear();
    pnp_stub_io_hook = trace_io;
    pnp_generator* g = nullptr;
    res.create_rc = pnp_generator_create(&sc.cfg, &g);
    if (res.create_rc) return res;
    pnp_generator_set_precision(g, sc.prec);
    pnp_generator_set_option(g, PNP_OPT_F16_MIRRORS, sc.mirrors >= 1);
    pnp_generator_set_option(g, PNP_OPT_F16_CHAIN_MIRRORS, sc.mirrors >= 2);
    pnp_generator_set_option(g, PNP_OPT_WINOGRAD, sc.wino);
    res.ws_rc = pnp_generator_set_max_resident(g, k);
    plan_pick(sc.t, sc.cfg.with_cat, k, &res.plan_r, &res.plan_l);
    const int t = sc.t;
    const int64_t flat_n = pnp_generator_flat_floats(g), packed_n = pnp_generator_packed_floats(g);
    res.ctx_bytes = pnp_generator_workspace_bytes(g, t, sc.h, sc.w);
    const int64_t ws_bytes = res.ctx_bytes * sc.contexts;
    const size_t hw = (size_t)sc.h * sc.w, os = sc.cfg.vsr ? 4 : 1, fm = hw * 64;
    // exact-size heap blocks: ASan's red zones start at the first byte past what the ABI asked for
    float* flat = (float*)malloc((size_t)flat_n * 4);
    float* packed = (float*)malloc((size_t)packed_n * 4);
    char* ws = nullptr;
    if (ws_bytes <= 0 || posix_memalign((void**)&ws, 256, (size_t)ws_bytes)) {
        res.errors.push_back("no workspace");
        pnp_generator_destroy(g);
        free(flat);
        free(packed);
        return res;
    }
    const size_t nt = (size_t)sc.n * t;
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
        const std::vector<float> sl = pattern(sc.pattern, t);
        for (int i = 0; i < t; ++i) {
            slices.push_back(sl[i]);
            qps.push_back((20.f + (float)((i * 7 + b) % 20)) / 255.f);
            bqs.push_back((15.f + 10.f * (float)(b % 3)) / 255.f);
        }
    }
    pnp_stub_stream caller{0};
    res.pack_rc = pnp_generator_pack(g, flat, packed, &caller);
    res.forward_rc = pnp_generator_forward(g, flat, packed, lrs, mvs, par, slices.data(), qps.data(), bqs.data(), out, ws, ws_bytes,
                                           sc.n, t, sc.h, sc.w, &caller);
    if (res.forward_rc == 0 && !covered(out, nt * 3 * hw * os * os * 4)) fail("the output clip is not completely written");

    // ---- follow the frame maps through the recorded launches
    std::vector<Workspace> Ws;
    for (int c = 0; c < sc.contexts; ++c) Ws.push_back(carve(g, ws + (int64_t)c * res.ctx_bytes, t, sc.h, sc.w));
    const int64_t nslots = bounded_mode(g, t) ? g->max_resident : t;
    auto in_slots = [&](const void* p) {
        for (const Workspace& W : Ws) {
            if ((const char*)p >= (const char*)W.slots && (const char*)p < (const char*)(W.slots + nslots * fm)) return true;
            if (W.slots16 && (const char*)p >= (const char*)W.slots16 && (const char*)p < (const char*)(W.slots16 + nslots * fm)) return true;
        }
        return false;
    };
    std::map<const void*, int> tag;
    auto lookup = [&](const void* p, const char* what) {
        auto it = tag.find(p);
        if (it == tag.end()) {
            fail(std::string("a branch run reads ") + what + " from a map no branch run wrote");
            return -2;
        }
        return it->second;
    };
    size_t wj = 0;
    int sample = 0, in_branch = -1, cur_sweep = 0, cur_frame = 0;
    bool last_fwd_done = false;
    const int nconv_branch = 2 * sc.cfg.num_blocks;
    for (const ConvRec& cr : convs) {
        const ConvArgs& a = cr.a;
        int sweep = -1;
        for (int b = 0; b < 2; ++b)
            if (a.nsrc >= 1 && a.src_c[0] == 4 && a.wsrc[0] == packed + g->br[b].in_lr) sweep = b;
        if (sweep >= 0) {                       // input conv: a branch run starts
            if (in_branch >= 0) fail("an input conv inside a branch run");
            if (last_fwd_done) {
                ++sample;
                last_fwd_done = false;
            }
            int ctx = -1, frame = -1;
            for (int c = 0; c < sc.contexts; ++c)
                if (a.src[0] >= Ws[c].lr4 && a.src[0] < Ws[c].lr4 + (size_t)t * hw * 4) {
                    ctx = c;
                    frame = (int)((a.src[0] - Ws[c].lr4) / (hw * 4));
                }
            if (ctx != sample % sc.contexts) fail("a branch run in the wrong workspace context");
            const BranchPk& B = g->br[sweep];
            StepRec r{sample, sweep, frame, -1, -1, -1, -1};
            for (int s = 1; s < a.nsrc; ++s) {
                const float* w = a.wsrc[s];
                const bool is_own = sweep == 1 && w == packed + B.in_wide[B.n_wide - 1];
                const bool is_kw = w == packed + B.in_wide[0] || (B.in_wide01 >= 0 && w == packed + B.in_wide01);
                if (is_kw) {
                    if ((const void*)a.src[s] != (const void*)Ws[ctx < 0 ? 0 : ctx].kw) fail("the aligned key frame is not read from kw");
                    if (wj >= warps.size()) {
                        fail("an aligned source without an alignment");
                        continue;
                    }
                    const WarpRec& wr = warps[wj++];
                    if (!in_slots(wr.feat)) fail("an alignment reads outside the frame maps");
                    r.key = lookup(wr.feat, "the key frame");
                    const size_t plane = (size_t)((const float*)wr.fx - mvs) / hw;
                    r.warp_plane = (int)plane;
                    if ((int)(plane / 4) != sample * t + frame || (int)(plane % 4) != (sweep == 0 ? 2 : 0))
                        fail("an alignment uses another frame's motion vectors");
                } else {
                    if (!in_slots(a.src[s])) fail("an input conv reads a 64-channel source outside the frame maps");
                    (is_own ? r.own : r.nb) = lookup(a.src[s], is_own ? "its own backward feature" : "the neighbour");
                }
            }
            res.steps.push_back(r);
            ++res.input_convs;
            in_branch = 0;
            cur_sweep = sweep;
            cur_frame = frame;
            continue;
        }
        if (in_branch >= 0) {
            if (++in_branch == nconv_branch) {           // the branch's last conv writes the frame map
                if (!in_slots(a.out)) fail("a branch run writes its frame map outside the frame maps");
                tag[a.out] = enc(sample, cur_sweep, cur_frame);
                if (a.out16) tag[a.out16] = enc(sample, cur_sweep, cur_frame);
                in_branch = -1;
                if (cur_sweep == 1 && cur_frame == t - 1) last_fwd_done = true;
            }
            continue;
        }
        // heads (and DCN offset convs): a conv that reads a frame map must read this frame's forward feature
        for (int s = 0; s < a.nsrc; ++s)
            if (in_slots(a.src[s])) {
                ++res.head_reads;
                if (lookup(a.src[s], "a head input") != enc(sample, 1, cur_frame) || cur_sweep != 1)
                    fail("a head reads another map than its frame's forward feature");
            }
    }
    // (deform = basic: the DCN offset convs run between an alignment and its input conv, outside any branch run, and read no frame map)
    if (wj != warps.size()) fail("an alignment whose result no input conv read");
    pnp_generator_destroy(g);
    trace_dump(sc.name + "/k=" + std::to_string(k));
    res.errors = errors;
    free(flat);
    free(packed);
    free(ws);
    free(lrs);
    free(mvs);
    free(par);
    free(out);
    return res;
}

void json_steps(const char* key, const std::vector<StepRec>& v) {
    printf("\"%s\": [", key);
    for (size_t i = 0; i < v.size(); ++i)
        printf("%s[%d, %d, %d, %d, %d, %d, %d]", i ? ", " : "", v[i].sample, v[i].sweep, v[i].frame, v[i].key, v[i].nb, v[i].own,
               v[i].warp_plane);
    printf("], ");
}

int report(const LcScenario& sc) {
    const LcResult b = run_lc(sc, sc.k), u = run_lc(sc, 0);
    // every branch run of the bounded schedule reads what the unbounded run of the same (sample, sweep, frame) read
    std::map<std::tuple<int, int, int>, StepRec> ref;
    for (const StepRec& r : u.steps) ref[std::make_tuple(r.sample, r.sweep, r.frame)] = r;
    int mismatches = 0;
    std::vector<StepRec> fwd_b, fwd_u;
    for (const StepRec& r : b.steps) {
        auto it = ref.find(std::make_tuple(r.sample, r.sweep, r.frame));
        if (it == ref.end() || !(it->second == r)) ++mismatches;
        if (r.sweep == 1) fwd_b.push_back(r);
    }
    for (const StepRec& r : u.steps)
        if (r.sweep == 1) fwd_u.push_back(r);
    printf("{\"name\": \"%s\", \"k\": %d, \"t\": %d, \"n\": %d, \"create_rc\": %d, \"set_rc\": %d, \"pack_rc\": %d, \"forward_rc\": %d, "
           "\"unbounded_forward_rc\": %d, \"context_bytes\": %lld, \"unbounded_context_bytes\": %lld, \"plan_r\": %d, \"plan_l\": %d, "
           "\"input_convs\": %d, \"unbounded_input_convs\": %d, \"head_reads\": %d, \"unbounded_head_reads\": %d, "
           "\"mismatches\": %d, \"forward_order_equal\": %d, ",
           sc.name.c_str(), sc.k, sc.t, sc.n, b.create_rc, b.ws_rc, b.pack_rc, b.forward_rc, u.forward_rc, (long long)b.ctx_bytes,
           (long long)u.ctx_bytes, b.plan_r, b.plan_l, b.input_convs, u.input_convs, b.head_reads, u.head_reads, mismatches,
           fwd_b == fwd_u ? 1 : 0);
    json_steps("steps", b.steps);
    json_steps("unbounded_steps", u.steps);
    printf("\"errors\": [");
    size_t i = 0;
    for (const auto& e : b.errors) printf("%s\"%s\"", i++ ? ", " : "", e.c_str());
    for (const auto& e : u.errors) printf("%s\"unbounded: %s\"", i++ ? ", " : "", e.c_str());
    printf("]}\n");
    fflush(stdout);
    return (b.errors.empty() && u.errors.empty()) ? 0 : 1;
}

}  // namespace

#undef main
int main(int argc, char** argv) {
    std::vector<LcScenario> all;
    auto add = [&](const std::string& name, pnp_generator_cfg c, int prec, int n, int t, int h, int w, int contexts, const char* pat,
                   int k, int mirrors = 1, int wino = 0) {
        pnp_generator* g = nullptr;
        if (pnp_generator_create(&c, &g) == 0) {
            if (k < 0) k = pnp_generator_min_resident(g, t) - k - 1;      // -1 = the minimum, -4 = the minimum + 3
            pnp_generator_destroy(g);
        }
        all.push_back(LcScenario{name, c, prec, n, t, h, w, contexts, k, mirrors, wino, pat});
    };
    const pnp_generator_cfg d = default_cfg();
    pnp_generator_cfg vsr = d, basic = d, nocat = d, noalign = d, sparse = d, chlast = d;
    vsr.vsr = 1;
    basic.deform = 1;
    nocat.with_cat = 0;
    noalign.align_key = 0;
    sparse.sparse_val = 1;
    chlast.channel_first = 0;
    chlast.one_layer = 0;
    add("ibbbp_t23_kmin", d, 0, 1, 23, 64, 64, 1, "IBBBP", -1);
    add("ibbbp_t23_kmin3", d, 0, 1, 23, 64, 64, 1, "IBBBP", -4);
    add("ibbbp_t23_k22", d, 0, 1, 23, 64, 64, 1, "IBBBP", 22);
    add("ibbbp_t23_k23", d, 0, 1, 23, 64, 64, 1, "IBBBP", 23);
    add("allB_t17", d, 0, 1, 17, 64, 64, 1, "allB", -1);
    add("allP_t9", d, 0, 1, 9, 64, 64, 1, "allP", -1);
    add("two_keys_t24", d, 0, 1, 24, 64, 64, 1, "IBBBBBBBBBBBPBBBBBBBBBBB", -1);
    add("n3_ctx2_t11", d, 0, 3, 11, 64, 64, 2, "IBBBP", -1);
    add("vsr_t9", vsr, 0, 1, 9, 64, 64, 1, "IBBBP", -1);
    add("basic_t9", basic, 0, 1, 9, 64, 64, 1, "IBBBP", -1);
    add("nocat_t19", nocat, 0, 1, 19, 64, 64, 1, "IBBBP", -1);
    add("noalign_t13", noalign, 0, 1, 13, 64, 64, 1, "allP", -1);
    add("sparse_val_t11", sparse, 0, 1, 11, 64, 64, 1, "IBBBP", -1);
    add("channel_last_t10", chlast, 0, 1, 10, 64, 64, 1, "IBBBP", -1);
    add("f16_mirrors_t13", d, 1, 1, 13, 64, 64, 1, "IBBBP", -1);
    add("f16_chain_t13", d, 1, 1, 13, 64, 64, 1, "IBBBP", -1, 2);
    add("f16_nomirrors_t13", d, 1, 1, 13, 64, 64, 1, "IBBBP", -1, 0);
    add("x3_t13", d, 2, 1, 13, 64, 64, 1, "IBBBP", -1);
    add("x3_n2_ctx2_t9", d, 2, 2, 9, 64, 64, 2, "allB", -1);
    add("wino0_t13", d, 0, 1, 13, 64, 64, 1, "IBBBP", -1, 1, 0);
    add("wino1_t13", d, 0, 1, 13, 64, 64, 1, "IBBBP", -1, 1, 1);
    add("wino2_t13", d, 0, 1, 13, 64, 64, 1, "IBBBP", -1, 1, 2);
    add("wino2_sparse_t9", sparse, 0, 1, 9, 64, 64, 1, "allB", -1, 1, 2);
    int bad = 0;
    for (const LcScenario& s : all) {
        bool want = argc < 2;
        for (int i = 1; i < argc; ++i) want = want || s.name == argv[i];
        if (want) bad += report(s);
    }
    return bad ? 1 : 0;
}
