// Host-only run of the MS-SSIM plan and of the level-0 step of its pyramid on 8-bit planes (pnp_vcve_amd/csrc/msssim_plan.h) under
// AddressSanitizer / UBSan.
//
// TEST INFRASTRUCTURE.  Built by tests/test_msssim_ref.py with a plain host compiler:
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -DPNP_HOST_STUB tests/host/msssim_stub.cpp
// msssim_down_kernel (csrc/msssim.hip) makes level 1 of an 8-bit plane through pnp_ms_down_plane8, one call per two output samples,
// and msssim_level_kernel fills its level-0 tiles through pnp_plane_load4, eleven groups a tile row, over the tiles pnp_ms_plan
// counts; this program drives those very functions the way the two kernels do, over planes that are heap blocks which END AT THE
// LAST SAMPLE OF THE LAST ROW (ASan's red zone sits right behind it) behind a base offset of 0..3, with pitches of the row's bytes,
// + 5 and + 7 (odd), steps 1 and 2 (interleaved pairs: either plane of the pair), at 176 x 176 and 178 x 216 (crop 0 and 1).
// Level 1 is compared with a plain loop over the bytes; every tile sample must carry the right value; the plan is compared with
// the rules restated here.  One JSON line per case, "errors" empty when all is well.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../pnp_vcve_amd/csrc/msssim_plan.h"

namespace {

std::vector<std::string> errors;
void fail(const std::string& s) {
    if (errors.size() < 8) errors.push_back(s);
}

unsigned char value_of(int plane, int f, int r, int c) { return (unsigned char)(41 * plane + 97 * f + 11 * r + 5 * c + (r * c) % 7); }

struct Case {
    int off, pitch_extra, step, rows, cols, crop;
};

void check_plan(int rows, int cols, int crop) {
    const PnpMsPlan p = pnp_ms_plan(rows, cols, crop);
    int r = rows - 2 * crop, c = cols - 2 * crop;
    const bool ok = crop >= 0 && r >= 176 && c >= 176;
    if ((p.ok != 0) != ok) return fail("plan: ok is wrong");
    if (!ok) {
        if (p.blocks || p.ws_floats) fail("plan: a refused plane has blocks or floats");
        return;
    }
    int blocks = 0;
    int64_t floats = 0;
    for (int s = 0; s < 5; ++s) {
        const PnpMsLevel& l = p.lv[s];
        const int nb = ((r - 10 + 15) / 16) * ((c - 10 + 31) / 32);
        if (l.rows != r || l.cols != c || l.oh != r - 10 || l.ow != c - 10 || l.blocks != nb || l.blk0 != blocks || l.tiles_x != (c - 10 + 31) / 32)
            fail("plan: a level's dimensions or blocks are wrong");
        if (l.ws_off != (s ? floats : -1)) fail("plan: a level's place in the slot is wrong");
        blocks += nb;
        if (s) floats += ((int64_t)r * c + 3) / 4 * 4;
        r /= 2, c /= 2;
    }
    if (p.blocks != blocks || p.ws_floats != floats) fail("plan: totals are wrong");
    if (p.lv[4].rows < 11 || p.lv[4].cols < 11) fail("plan: level 4 holds no window");
}

void run(const Case& k) {
    errors.clear();
    const int rowbytes = k.step * k.cols;
    const int64_t pitch = rowbytes + k.pitch_extra;
    const int frames = 2;
    // the block of a frame ends with the last sample of its last row
    std::vector<unsigned char*> blocks;
    for (int f = 0; f < frames; ++f) {
        const size_t n = (size_t)k.off + (size_t)(k.rows - 1) * pitch + rowbytes;
        unsigned char* b = (unsigned char*)malloc(n);
        for (size_t i = 0; i < n; ++i) b[i] = 0xA5;
        for (int r = 0; r < k.rows; ++r)
            for (int c = 0; c < k.cols; ++c)
                for (int p = 0; p < k.step; ++p) b[k.off + r * pitch + c * k.step + p] = value_of(p, f, r, c);
        blocks.push_back(b);
    }
    const PnpPlaneSrc src{blocks[0] + k.off, pitch, (int64_t)((intptr_t)blocks[1] - (intptr_t)blocks[0]), k.step, k.rows, rowbytes};
    check_plan(k.rows, k.cols, k.crop);
    const PnpMsPlan plan = pnp_ms_plan(k.rows, k.cols, k.crop);
    long dwords = 0, fetches = 0;
    if (plan.ok) {
        const PnpMsLevel& d = plan.lv[1];
        for (int f = 0; f < frames; ++f)
            for (int sel = 0; sel < k.step; ++sel) {
                // msssim_down_kernel's walk: groups of two output samples along the rows of level 1
                std::vector<float> got((size_t)d.rows * d.cols, -1.f);
                const int gpr = (d.cols + 1) / 2;
                for (long g = 0; g < (long)d.rows * gpr; ++g) {
                    const int r = (int)(g / gpr), gx = (int)(g - (long)r * gpr);
                    const int ncol = d.cols - 2 * gx < 2 ? 1 : 2;
                    float out[2] = {-7.f, -7.f};
                    dwords += pnp_ms_down_plane8(src, sel, f, k.crop, r, gx, ncol, out);
                    fetches += 2;
                    for (int j = 0; j < ncol; ++j) got[(size_t)r * d.cols + 2 * gx + j] = out[j];
                }
                // the plain loop
                for (int r = 0; r < d.rows; ++r)
                    for (int c = 0; c < d.cols; ++c) {
                        const int y = k.crop + 2 * r, x = k.crop + 2 * c;
                        const double want = (((double)value_of(sel, f, y, x) + value_of(sel, f, y, x + 1)) +
                                             ((double)value_of(sel, f, y + 1, x) + value_of(sel, f, y + 1, x + 1))) * 0.25;
                        if ((double)got[(size_t)r * d.cols + c] != want) {
                            char msg[160];
                            snprintf(msg, sizeof msg, "level 1: frame %d plane %d row %d col %d: got %.4f want %.4f", f, sel, r, c,
                                     (double)got[(size_t)r * d.cols + c], want);
                            fail(msg);
                        }
                    }
                // msssim_level_kernel's level-0 tile fill: 26 x 42 tiles, 16 x 32 apart, eleven groups a row
                const PnpMsLevel& l0 = plan.lv[0];
                for (int b = 0; b < l0.blocks; ++b) {
                    const int ty0 = (b / l0.tiles_x) * 16, tx0 = (b % l0.tiles_x) * 32;
                    for (int i = 0; i < 26 * 11; ++i) {
                        const int r = i / 11, gc = i - r * 11;
                        const int y = k.crop + ty0 + r, x = k.crop + tx0 + 4 * gc;
                        int npix = 42 - 4 * gc < 4 ? 42 - 4 * gc : 4;
                        if (k.cols - k.crop - x < npix) npix = k.cols - k.crop - x;
                        if (y >= k.rows - k.crop || npix <= 0) continue;
                        unsigned w[2] = {0xdeadbeefu, 0xdeadbeefu};
                        dwords += pnp_plane_load4(src, f, y, x, npix, w);
                        fetches += 1;
                        const unsigned v = sel ? w[1] : w[0];
                        for (int j = 0; j < 4; ++j) {
                            const unsigned want = j < npix ? value_of(sel, f, y, x + j) : 0u;
                            if (((v >> (8 * j)) & 255u) != want) fail("tile: a wrong sample");
                        }
                    }
                }
            }
    } else {
        fail("the case's plane cannot be scored");
    }
    if (!dwords) fail("the dword form was never used");
    if (dwords == fetches && k.off) fail("a misaligned plane was read without a single byte fetch");
    printf("{\"off\": %d, \"pitch_extra\": %d, \"step\": %d, \"rows\": %d, \"cols\": %d, \"crop\": %d, \"dwords\": %ld, \"fetches\": %ld, \"errors\": [",
           k.off, k.pitch_extra, k.step, k.rows, k.cols, k.crop, dwords, fetches);
    for (size_t i = 0; i < errors.size(); ++i) printf("%s\"%s\"", i ? ", " : "", errors[i].c_str());
    printf("]}\n");
    for (unsigned char* b : blocks) free(b);
}

}  // namespace

int main() {
    // the plan alone, around its thresholds
    errors.clear();
    for (int rows : {175, 176, 177, 191, 192, 215, 352, 720})
        for (int cols : {175, 176, 178, 215, 300, 1280})
            for (int crop : {0, 1, 4, 6}) check_plan(rows, cols, crop);
    check_plan(176, 176, -1);
    check_plan(0, 0, 0);
    printf("{\"plan\": true, \"errors\": [");
    for (size_t i = 0; i < errors.size(); ++i) printf("%s\"%s\"", i ? ", " : "", errors[i].c_str());
    printf("]}\n");
    int ncases = 0;
    for (int off = 0; off < 4; ++off)
        for (int extra : {0, 5, 7})
            for (int step : {1, 2}) {
                run(Case{off, extra, step, 176, 176, 0});
                run(Case{off, extra, step, 178, 216, 0});
                run(Case{off, extra, step, 178, 216, 1});
                ncases += 3;
            }
    printf("{\"cases\": %d}\n", ncases);
    return 0;
}
