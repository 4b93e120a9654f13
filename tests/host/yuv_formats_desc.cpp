// Host-only check of the chroma formats' descriptor rules (csrc/yuv.h) and of the chroma plane sources of the plane metrics
// (csrc/plane_src.h) under AddressSanitizer / UBSan.
//
// TEST INFRASTRUCTURE.  Built by tests/test_yuv_formats_host.py with a plain host compiler:
//     g++ -std=c++17 -O2 -g -fsanitize=address,undefined -fno-sanitize-recover=all -DPNP_HOST_STUB -x c++ tests/host/yuv_formats_desc.cpp
// 1. yuv_planes_ok(p, w, format) / yuv_planes_fast(p, w, format) against predicates written here on their own, format by format, from
//    the rules of include/pnpvcve.h (a chroma row holds c_step * w / sx samples; the aligned pack loads four Y samples, and of the
//    chroma 4:2:2 a pair of pairs or two samples of each plane, 4:4:4 two four-sample loads of the pairs or four samples of each
//    plane), over a sweep of pointers, pitches, steps and widths at both sample sizes.  No address is dereferenced.  The two-argument
//    forms must be the 4:2:0 ones.
// 2. chroma_src(p, h, w, format) of 8-bit planes that are heap blocks of EXACTLY the bytes the reading rule allows (the last row ends
//    with its last sample; ASan's red zone sits right behind it), walked through pnp_plane_load4 with pnp_plane_runs of the plane's true
//    rows, columns and per-axis crop, the way the PSNR kernel walks them: every sample inside the crop is fetched exactly once with its
//    value, none outside it.  clip_planes(p, h, w, format, ...) -- what the metric entries fill their kernel arguments with -- must name
//    the same planes: every group is fetched again through its Cb and Cr sources and their `sel` and must be the same word.
// 3. The pack launcher's choice of its form, through the host-only stand-in of the launcher (csrc/host_stub/yuv_stub.h, which records
//    what the scheduler build would launch): tightly packed aligned planes of nv16 / yuv422p / nv24 / yuv444p and their 16-bit
//    siblings must record the aligned form, the same planes 2 samples further on and a forced general launch must not, and a frame
//    the format refuses (4:2:2 with an odd width) must be PNP_ERR_BAD_ARG with nothing recorded.
// One JSON line per part; the exit status is 0 when all is well.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../pnp_vcve_amd/csrc/host_stub/yuv_stub.h"
#include "../../pnp_vcve_amd/csrc/plane_src.h"

namespace {

// ---------------------------------------------------------------------------------------------- 1. the predicates
bool aligned(uintptr_t v, uintptr_t a) { return v % a == 0; }

bool ref_ok(const YuvPlanes& p, int w, int format) {
    const int64_t S = p.sample_bytes;
    if (format < 0 || format > 2) return false;
    if (S == 1 && !(p.bit_depth == 8 && p.msb_aligned == 0)) return false;
    if (S == 2 && !((p.bit_depth == 10 || p.bit_depth == 12) && (p.msb_aligned == 0 || p.msb_aligned == 1))) return false;
    if (S != 1 && S != 2) return false;
    if (!p.y || !p.cb || !p.cr) return false;
    if (p.c_step != 1 && p.c_step != 2) return false;
    for (uintptr_t v : {(uintptr_t)p.y, (uintptr_t)p.cb, (uintptr_t)p.cr, (uintptr_t)p.y_pitch, (uintptr_t)p.c_pitch, (uintptr_t)p.y_frame, (uintptr_t)p.c_frame})
        if (!aligned(v, (uintptr_t)S)) return false;
    const int64_t chroma_samples = format == 0 ? w / 2 : format == 1 ? w / 2 : w;
    return p.y_pitch >= S * w && p.c_pitch >= S * p.c_step * chroma_samples;
}

bool ref_fast(const YuvPlanes& p, int w, int format) {
    const uintptr_t S = (uintptr_t)p.sample_bytes;
    if (w % 4) return false;
    if (!aligned((uintptr_t)p.y, 4 * S) || !aligned((uintptr_t)p.y_pitch, 4 * S) || !aligned((uintptr_t)p.y_frame, 4 * S)) return false;
    const uintptr_t cb = (uintptr_t)p.cb, cr = (uintptr_t)p.cr;
    if (p.c_step == 2) {        // pairs: the planes one sample apart, four-sample loads from the first of them
        const uintptr_t first = cb < cr ? cb : cr, second = cb < cr ? cr : cb;
        return second - first == S && aligned(first, 4 * S) && aligned((uintptr_t)p.c_pitch, 4 * S) && aligned((uintptr_t)p.c_frame, 4 * S);
    }
    const uintptr_t load = format == 2 ? 4 * S : 2 * S;       // planar: four samples of each plane at 4:4:4, two otherwise
    return aligned(cb, load) && aligned(cr, load) && aligned((uintptr_t)p.c_pitch, load) && aligned((uintptr_t)p.c_frame, load);
}

struct Tally {
    long long tuples = 0, ok = 0, fast = 0, wrong = 0;
    char first[200] = "";
};

template <int S>
void sweep(Tally& T) {
    const uintptr_t Y_BASE = 0x100000, C_BASE = 0x200000;
    for (int format = -1; format <= 3; ++format)
    for (int w : {2, 3, 4, 6, 8})
    for (int c_step = 0; c_step <= 3; ++c_step)
    for (int ay : {0, 1, 2, 4, 8})
    for (int ab : {0, 1, 2, 4, 8})
    for (int dr : {-2, -1, 0, 1, 2, 64, 66, 72})
    for (int py : {-1, 0, 1, 3, 8})
    for (int pc = -2 * S; pc <= 9; ++pc)
    for (int64_t cf : {0, 1, 2, 4, 8, 1004, 1008}) {
        const uintptr_t y = Y_BASE + ay, cb = C_BASE + ab, cr = cb + dr;
        // chroma pitches around every format's row: w / 2, w and 2 w samples times the step
        for (int row : {w / 2, w, 2 * w}) {
            const int64_t y_pitch = (int64_t)w * S + py, c_pitch = (int64_t)row * S + pc;
            YuvPlanes p{(unsigned char*)y, (unsigned char*)cb, (unsigned char*)cr, y_pitch, c_pitch, (int64_t)(4 * (ay & 1)), cf, c_step, S, S == 1 ? 8 : 10, 0};
            const bool ok_ref = ref_ok(p, w, format), ok_new = yuv_planes_ok(p, w, format);
            const bool in = format >= 0 && format <= 2;
            const bool fast_ref = in && ref_fast(p, w, format), fast_new = in && yuv_planes_fast(p, w, format);
            bool same = ok_ref == ok_new && fast_ref == fast_new;
            if (format == 0) same = same && yuv_planes_ok(p, w) == ok_new && yuv_planes_fast(p, w) == fast_new;
            ++T.tuples, T.ok += ok_new, T.fast += fast_new;
            if (!same && !T.wrong++)
                snprintf(T.first, sizeof T.first, "S=%d format=%d w=%d y=%p cb=%p cr=%p pitches %lld %lld c_frame %lld c_step=%d: ok %d/%d fast %d/%d", S,
                         format, w, (void*)y, (void*)cb, (void*)cr, (long long)y_pitch, (long long)c_pitch, (long long)cf, c_step, ok_ref, ok_new, fast_ref,
                         fast_new);
        }
    }
}

// ---------------------------------------------------------------------------------------------- 2. the chroma plane sources
unsigned char value_of(int plane, int f, int r, int c) { return (unsigned char)(37 * plane + 101 * f + 7 * r + 13 * c + (r * c) % 5); }

int nerrors = 0;
char first_error[200] = "";
void fail(const char* what, int format, int step, int off, int extra, int crop, int r, int c) {
    if (!nerrors++) snprintf(first_error, sizeof first_error, "%s: format %d step %d off %d pitch+%d crop %d row %d col %d", what, format, step, off, extra, crop, r, c);
}

// a block of exactly `off` bytes and then what the reading rule allows of a plane: (rows - 1) * pitch + rowbytes
unsigned char* block_of(int off, int rows, int64_t pitch, int rowbytes) {
    const size_t n = (size_t)off + (size_t)(rows - 1) * pitch + rowbytes;
    unsigned char* b = (unsigned char*)malloc(n);
    memset(b, 0xA5, n);
    return b;
}

long walk_case(int format, int step, bool paired, bool cr_first, int off, int extra, int h, int w, int crop) {
    const int rows = h / yuv_sy(format), cols = w / yuv_sx(format);
    const int64_t pitch = (int64_t)step * cols + extra;
    std::vector<unsigned char*> blocks;
    pnp_yuv420_planes p{};
    p.c_pitch = pitch, p.c_frame = 0, p.c_step = step, p.y_pitch = w, p.y_frame = 0;
    unsigned char* plane_at[2];     // where plane 0 (Cb) and plane 1 (Cr) start
    if (paired) {
        unsigned char* b = block_of(off, rows, pitch, 2 * cols);
        blocks.push_back(b);
        plane_at[cr_first ? 1 : 0] = b + off, plane_at[cr_first ? 0 : 1] = b + off + 1;
    } else {
        for (int k = 0; k < 2; ++k) {
            blocks.push_back(block_of(off, rows, pitch, step * (cols - 1) + 1));
            plane_at[k] = blocks.back() + off;
        }
    }
    for (int k = 0; k < 2; ++k)
        for (int r = 0; r < rows; ++r)
            for (int c = 0; c < cols; ++c) plane_at[k][r * pitch + (int64_t)c * step] = value_of(k, 0, r, c);
    p.cb = plane_at[0], p.cr = plane_at[1];
    p.y = plane_at[0];              // (never read here)
    const ChromaSrc s = chroma_src(p, h, w, format);
    if (s.paired != (paired ? 1 : 0) || (paired && s.cr_first != (cr_first ? 1 : 0))) fail("pairing", format, step, off, extra, crop, 0, 0);
    PlaneSamp pl[3];
    clip_planes(p, h, w, format, pl);
    const PlaneGeom g = plane_geom(h, w, crop, PNP_PLANE_CB, format);
    if (g.H != rows || g.W != cols) fail("geometry", format, step, off, extra, crop, g.H, g.W);
    const PnpPlaneRuns runs = pnp_plane_runs(g.H, g.W, g.cropy, g.cropx);
    std::vector<int> seen((size_t)2 * rows * cols, 0);
    long loads = 0;
    for (int rr = 0; rr < runs.rows; ++rr)
        for (int gx = 0; gx < runs.gpr; ++gx) {
            int row, col, npix;
            pnp_plane_group(runs, rr, gx, row, col, npix);
            unsigned v[2];          // [0]: Cb's four samples, [1]: Cr's (plane_metrics.hip's load_chroma4)
            unsigned o[2];
            if (s.paired) {
                pnp_plane_load4(s.c[0], 0, row, col, npix, o);
                v[0] = s.cr_first ? o[1] : o[0], v[1] = s.cr_first ? o[0] : o[1];
                ++loads;
            } else {
                pnp_plane_load4(s.c[0], 0, row, col, npix, o);
                v[0] = o[0];
                pnp_plane_load4(s.c[1], 0, row, col, npix, o);
                v[1] = o[0];
                loads += 2;
            }
            for (int k = 0; k < 2; ++k) {       // the plane as a metric kernel reads it (metric_src.h::plane_load4's 8-bit arm)
                pnp_plane_load4(pl[1 + k].p8, 0, row, col, npix, o);
                if ((pl[1 + k].sel ? o[1] : o[0]) != v[k]) fail("clip_planes names another plane", format, step, off, extra, crop, row, col);
            }
            for (int k = 0; k < 2; ++k)
                for (int j = 0; j < 4; ++j) {
                    const unsigned got = (v[k] >> (8 * j)) & 255u;
                    if (j >= npix) {
                        if (got) fail("a byte beyond npix is not zero", format, step, off, extra, crop, row, col + j);
                        continue;
                    }
                    if (row < 0 || row >= rows || col + j >= cols) {
                        fail("a group outside the plane", format, step, off, extra, crop, row, col + j);
                        continue;
                    }
                    ++seen[((size_t)k * rows + row) * cols + col + j];
                    if (got != value_of(k, 0, row, col + j)) fail("wrong value", format, step, off, extra, crop, row, col + j);
                }
        }
    for (int k = 0; k < 2; ++k)
        for (int r = 0; r < rows; ++r)
            for (int c = 0; c < cols; ++c) {
                const bool in = r >= g.cropy && r < rows - g.cropy && c >= g.cropx && c < cols - g.cropx;
                if (seen[((size_t)k * rows + r) * cols + c] != (in ? 1 : 0)) fail("a sample fetched other than once", format, step, off, extra, crop, r, c);
            }
    for (unsigned char* b : blocks) free(b);
    return loads;
}

// ---------------------------------------------------------------------------------------------- 3. the form the pack launch takes
int form_errors = 0;
char first_form[200] = "";

// planes of t frames of h x w at "device address" base (never dereferenced), tightly packed in the layout: Y, then chroma
YuvPlanes packed_planes(uintptr_t base, int S, int format, int step, int h, int w) {
    const int64_t cw = w / yuv_sx(format), ch = h / yuv_sy(format);
    const int64_t y_pitch = (int64_t)S * w, c_pitch = (int64_t)S * step * cw;
    const int64_t frame = h * y_pitch + ch * c_pitch * (step == 2 ? 1 : 2);
    unsigned char* y = (unsigned char*)base;
    unsigned char* cb = y + h * y_pitch;
    unsigned char* cr = step == 2 ? cb + S : cb + ch * c_pitch;
    return YuvPlanes{y, cb, cr, y_pitch, c_pitch, frame, frame, step, S, S == 1 ? 8 : 10, 0};
}

void expect_form(const char* what, int S, int format, int step, const YuvPlanes& p, int w, bool force_general, bool want_fast) {
    YuvCoef k;
    const size_t before = pnp_stub_yuv_log.size();
    const bool coded = yuv_coef(PNP_YUV_CODE3(PNP_YUV_BT709_LIMITED, PNP_YUV_CHROMA_LEFT, format), p, &k);
    float* lr4 = (float*)(uintptr_t)0x4000000;
    const int rc = coded ? launch_pack_lr_yuv420(p, k, lr4, 2, 64, w, force_general, nullptr) : -1;
    const bool recorded = pnp_stub_yuv_log.size() == before + 1;
    const bool good = rc == 0 && recorded && pnp_stub_yuv_log.back().kind == PNP_STUB_YUV_PACK && pnp_stub_yuv_log.back().fast == want_fast;
    if (!good && !form_errors++)
        snprintf(first_form, sizeof first_form, "%s: S=%d format=%d step=%d w=%d general=%d: rc %d recorded %d fast %d, want fast %d", what, S, format, step, w,
                 (int)force_general, rc, (int)recorded, recorded ? (int)pnp_stub_yuv_log.back().fast : -1, (int)want_fast);
}

long forms() {
    long n = 0;
    for (int S : {1, 2})
        for (int format : {PNP_YUV_FORMAT_422, PNP_YUV_FORMAT_444})
            for (int step : {1, 2}) {      // planar (yuv422p / yuv444p and their 16-bit forms), pairs (nv16 / nv24, P210 / P410)
                const uintptr_t base = 0x1000000;
                const YuvPlanes p = packed_planes(base, S, format, step, 64, 96);
                expect_form("tight and aligned", S, format, step, p, 96, false, true);
                expect_form("forced general", S, format, step, p, 96, true, false);
                expect_form("2 samples further on", S, format, step, packed_planes(base + 2 * S, S, format, step, 64, 96), 96, false, false);
                expect_form("no multiple of 4", S, format, step, packed_planes(base, S, format, step, 64, 98), 98, false, false);
                n += 4;
                if (format == PNP_YUV_FORMAT_422) {     // an odd width is refused, and nothing is recorded
                    YuvCoef k;
                    const size_t before = pnp_stub_yuv_log.size();
                    const YuvPlanes q = packed_planes(base, S, PNP_YUV_FORMAT_444, step, 64, 97);
                    const bool refused = yuv_coef(PNP_YUV_CODE3(0, 0, format), q, &k) &&
                                         launch_pack_lr_yuv420(q, k, (float*)(uintptr_t)0x4000000, 2, 64, 97, false, nullptr) == PNP_ERR_BAD_ARG &&
                                         pnp_stub_yuv_log.size() == before;
                    if (!refused && !form_errors++) snprintf(first_form, sizeof first_form, "4:2:2 with 97 columns was not refused (S=%d step=%d)", S, step);
                    ++n;
                }
            }
    return n;
}

}  // namespace

int main() {
    Tally t8, t16;
    sweep<1>(t8);
    sweep<2>(t16);
    printf("{\"sweep\": 1, \"tuples8\": %lld, \"ok8\": %lld, \"fast8\": %lld, \"wrong8\": %lld, \"first8\": \"%s\", \"tuples16\": %lld, \"ok16\": %lld, "
           "\"fast16\": %lld, \"wrong16\": %lld, \"first16\": \"%s\"}\n",
           t8.tuples, t8.ok, t8.fast, t8.wrong, t8.first, t16.tuples, t16.ok, t16.fast, t16.wrong, t16.first);
    long cases = 0, loads = 0;
    const int h = 14, w = 38;       // 4:4:4: 38 columns (a short group ends every row); 4:2:2 and 4:2:0: 19
    for (int format = 0; format <= 2; ++format)
        for (int off = 0; off < 4; ++off)
            for (int extra : {0, 3, 6})
                for (int crop : {0, 2, 3}) {
                    if (crop == 3 && format != 2) continue;     // an odd crop is 4:4:4's alone
                    loads += walk_case(format, 1, false, false, off, extra, h, w, crop);      // planar
                    loads += walk_case(format, 2, false, false, off, extra, h, w, crop);      // a step of 2, planes of their own
                    loads += walk_case(format, 2, true, false, off, extra, h, w, crop);       // pairs, Cb first
                    loads += walk_case(format, 2, true, true, off, extra, h, w, crop);        // pairs, Cr first
                    cases += 4;
                }
    printf("{\"walk\": 1, \"cases\": %ld, \"loads\": %ld, \"errors\": %d, \"first\": \"%s\"}\n", cases, loads, nerrors, first_error);
    const long nforms = forms();
    printf("{\"forms\": 1, \"cases\": %ld, \"errors\": %d, \"first\": \"%s\"}\n", nforms, form_errors, first_form);
    return (t8.wrong || t16.wrong || nerrors || form_errors) ? 1 : 0;
}
