// Host-only run of the plane loader of the plane metrics (pnp_vcve_amd/csrc/plane_load.h) under AddressSanitizer / UBSan.
//
// TEST INFRASTRUCTURE.  Built by tests/test_yuv_metrics_host.py with a plain host compiler:
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -DPNP_HOST_STUB tests/host/plane_metrics_stub.cpp
// The kernels of csrc/plane_metrics.hip fetch every sample through pnp_plane_load4 and walk a cropped plane with pnp_plane_runs /
// pnp_plane_group; this program drives those very functions the way the two kernels do -- the PSNR kernel's runs of groups of four (run by run, group by group),
// the SSIM kernel's 26 x 42 tiles of eleven groups a row -- over planes that are heap blocks of EXACTLY rows * pitch bytes behind a
// base offset of 0..3 (every alignment of a row start occurs; ASan's red zone sits right behind the last row), every frame of a clip
// a block of its own, with pitches w, w + 6 and w + 7, steps 1 and 2 (interleaved pairs: both planes from one fetch), widths 36, 38
// and 70 and crops 0, 1, 2.  Every sample of the cropped plane must be fetched exactly once with the right value; the form of every
// fetch is checked against the rule restated here (dwords exactly where the covering aligned dwords lie inside the frame's rows, so
// never in front of a misaligned plane's first sample and never behind the last sample of the last row); ASan must stay silent.
// One JSON line per case, "errors" empty when all is well.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../pnp_vcve_amd/csrc/plane_load.h"

namespace {

std::vector<std::string> errors;
void fail(const std::string& s) {
    if (errors.size() < 8) errors.push_back(s);
}

unsigned char value_of(int plane, int f, int r, int c) { return (unsigned char)(37 * plane + 101 * f + 7 * r + 13 * c + (r * c) % 5); }

struct Case {
    int off, pitch_extra, step, cols, rows, crop, frames;
};

// a clip of `frames` frames, each frame a block of its own of exactly off + rows * pitch bytes whose plane starts `off` bytes in: the
// frame stride is whatever the allocator gave (any value, negative ones too)
struct Clip {
    std::vector<unsigned char*> blocks;
    PnpPlaneSrc src;
    int64_t pitch;
    Clip(const Case& k) {
        const int rowbytes = k.step * k.cols;
        pitch = rowbytes + k.pitch_extra;
        // rows * pitch bytes hold the plane; the block ends with the last row's padding, as the planes of a decoder's frame do
        for (int f = 0; f < k.frames; ++f) {
            unsigned char* b = (unsigned char*)malloc((size_t)k.off + (size_t)k.rows * pitch);
            for (int64_t i = 0; i < k.off + (int64_t)k.rows * pitch; ++i) b[i] = 0xA5;
            for (int r = 0; r < k.rows; ++r)
                for (int c = 0; c < k.cols; ++c)
                    for (int p = 0; p < k.step; ++p) b[k.off + r * pitch + c * k.step + p] = value_of(p, f, r, c);
            blocks.push_back(b);
        }
        // frames of one clip are `frame` bytes apart: use two blocks only when their distance can be expressed (always, on a flat heap)
        src = PnpPlaneSrc{blocks[0] + k.off, pitch, k.frames > 1 ? (int64_t)((intptr_t)blocks[1] - (intptr_t)blocks[0]) : 0, k.step, k.rows, rowbytes};
    }
    ~Clip() {
        for (unsigned char* b : blocks) free(b);
    }
};

struct Tally {
    std::vector<int> seen;      // per (plane, row, col) of one frame
    int rows, cols, step;
    long dwords = 0, bytes = 0;
    Tally(int rows_, int cols_, int step_) : seen((size_t)rows_ * cols_ * step_, 0), rows(rows_), cols(cols_), step(step_) {}
    void take(const PnpPlaneSrc& s, int f, int row, int col, int npix, const unsigned out[2], int form) {
        (form == PNP_PLANE_LOAD_DWORDS ? dwords : bytes) += 1;
        // the form, decided here on its own: dwords exactly where the aligned dwords that cover a whole group lie inside the frame's rows
        const uintptr_t lo = (uintptr_t)s.p + (uintptr_t)((int64_t)f * s.frame), hi = lo + (uintptr_t)((int64_t)(s.rows - 1) * s.pitch + s.rowbytes);
        const uintptr_t q = lo + (uintptr_t)((int64_t)row * s.pitch + (int64_t)col * s.step), q0 = q & ~(uintptr_t)3;
        const bool inside = npix == 4 && q0 >= lo && q0 + 4 * s.step + (q != q0 ? 4 : 0) <= hi;
        if (inside != (form == PNP_PLANE_LOAD_DWORDS)) fail(inside ? "byte loads where the dwords lie inside the plane" : "dword loads that leave the plane's rows");
        for (int p = 0; p < step; ++p)
            for (int j = 0; j < 4; ++j) {
                const unsigned v = (out[p] >> (8 * j)) & 255u;
                if (j >= npix) {
                    if (v) fail("a byte beyond npix is not zero");
                    continue;
                }
                if (row < 0 || row >= rows || col + j >= cols) {
                    fail("a group outside the plane");
                    continue;
                }
                ++seen[((size_t)p * rows + row) * cols + col + j];
                if (v != value_of(p, f, row, col + j)) {
                    char msg[160];
                    snprintf(msg, sizeof msg, "wrong value: plane %d frame %d row %d col %d: got %u want %u (form %d)", p, f, row, col + j, v,
                             (unsigned)value_of(p, f, row, col + j), form);
                    fail(msg);
                }
            }
        if (step == 1 && out[1]) fail("step 1 filled the second word");
    }
    // every sample inside the crop exactly `want` times, none outside it
    void check(int crop, int want, const char* what) {
        for (int p = 0; p < step; ++p)
            for (int r = 0; r < rows; ++r)
                for (int c = 0; c < cols; ++c) {
                    const bool in = r >= crop && r < rows - crop && c >= crop && c < cols - crop;
                    const int n = seen[((size_t)p * rows + r) * cols + c];
                    if (n != (in ? want : 0)) {
                        char msg[160];
                        snprintf(msg, sizeof msg, "%s: plane %d row %d col %d fetched %d times, want %d", what, p, r, c, n, in ? want : 0);
                        fail(msg);
                    }
                }
    }
};

void run(const Case& k) {
    errors.clear();
    Clip clip(k);
    long dwords = 0, bytes = 0;
    // the PSNR kernel's walk: groups of four along the cropped rows
    const PnpPlaneRuns runs = pnp_plane_runs(k.rows, k.cols, k.crop);
    for (int f = 0; f < k.frames; ++f) {
        Tally t(k.rows, k.cols, k.step);
        for (int rr = 0; rr < runs.rows; ++rr)
            for (int gx = 0; gx < runs.gpr; ++gx) {
                int row, col, npix;
                pnp_plane_group(runs, rr, gx, row, col, npix);
                unsigned out[2] = {0xdeadbeefu, 0xdeadbeefu};
                const int form = pnp_plane_load4(clip.src, f, row, col, npix, out);
                t.take(clip.src, f, row, col, npix, out, form);
            }
        t.check(k.crop, 1, "runs");
        dwords += t.dwords, bytes += t.bytes;
    }
    // the SSIM kernel's walk: 26 x 42 tiles, 16 x 32 apart, eleven groups a row; a sample is fetched once per tile that holds it
    const int oh = k.rows - 2 * k.crop - 10, ow = k.cols - 2 * k.crop - 10;
    if (oh >= 1 && ow >= 1) {
        const int tiles_y = (oh + 15) / 16, tiles_x = (ow + 31) / 32;
        for (int ty = 0; ty < tiles_y; ++ty)
            for (int tx = 0; tx < tiles_x; ++tx) {
                Tally t(k.rows, k.cols, k.step);
                for (int i = 0; i < 26 * 11; ++i) {
                    const int r = i / 11, gc = i - r * 11;
                    const int y = k.crop + ty * 16 + r, x = k.crop + tx * 32 + 4 * gc;
                    int npix = 42 - 4 * gc < 4 ? 42 - 4 * gc : 4;
                    if (k.cols - k.crop - x < npix) npix = k.cols - k.crop - x;
                    if (y < k.rows - k.crop && npix > 0) {
                        unsigned out[2] = {0xdeadbeefu, 0xdeadbeefu};
                        const int form = pnp_plane_load4(clip.src, 0, y, x, npix, out);
                        t.take(clip.src, 0, y, x, npix, out, form);
                    }
                }
                for (int r = 0; r < k.rows; ++r)
                    for (int c = 0; c < k.cols; ++c) {
                        const bool in = r >= k.crop + ty * 16 && r < k.crop + ty * 16 + 26 && r < k.rows - k.crop && c >= k.crop + tx * 32 &&
                                        c < k.crop + tx * 32 + 42 && c < k.cols - k.crop;
                        for (int p = 0; p < k.step; ++p)
                            if (t.seen[((size_t)p * k.rows + r) * k.cols + c] != (in ? 1 : 0)) fail("tile: a sample fetched other than once");
                    }
                dwords += t.dwords, bytes += t.bytes;
            }
    }
    if (!dwords) fail("the dword form was never used");
    if (!bytes && (k.cols - 2 * k.crop) % 4) fail("the byte form was never used");      // (a short group ends every row)
    printf("{\"off\": %d, \"pitch_extra\": %d, \"step\": %d, \"cols\": %d, \"rows\": %d, \"crop\": %d, \"frames\": %d, \"dwords\": %ld, \"bytes\": %ld, \"errors\": [",
           k.off, k.pitch_extra, k.step, k.cols, k.rows, k.crop, k.frames, dwords, bytes);
    for (size_t i = 0; i < errors.size(); ++i) printf("%s\"%s\"", i ? ", " : "", errors[i].c_str());
    printf("]}\n");
}

}  // namespace

int main() {
    // the alignbyte stand-in against its definition
    for (unsigned sh = 0; sh < 4; ++sh) {
        const unsigned got = pnp_plane_alignbyte(0x77665544u, 0x33221100u, sh);
        const unsigned want[4] = {0x33221100u, 0x44332211u, 0x55443322u, 0x66554433u};
        if (got != want[sh]) {
            printf("{\"errors\": [\"alignbyte stand-in: shift %u gives %08x\"]}\n", sh, got);
            return 1;
        }
    }
    int ncases = 0;
    for (int off = 0; off < 4; ++off)
        for (int extra : {0, 6, 7})
            for (int step : {1, 2})
                for (int cols : {36, 38, 70})
                    for (int crop : {0, 1, 2}) {
                        run(Case{off, extra, step, cols, 30, crop, 2});
                        ++ncases;
                    }
    printf("{\"cases\": %d}\n", ncases);
    return 0;
}
