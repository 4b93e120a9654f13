// Host-only walk of the XPSNR plan (pnp_vcve_amd/csrc/xpsnr_plan.h) under AddressSanitizer / UBSan.
//
// TEST INFRASTRUCTURE.  Built by tests/test_xpsnr_ref.py with a plain host compiler:
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -DPNP_HOST_STUB tests/host/xpsnr_stub.cpp
// xpsnr_kernel (csrc/xpsnr.hip) takes its block size, grid, block bounds, chroma blocks, activity regions and lane groups from the
// functions of that header; this program calls those very functions over ragged sizes, both borders b, crops and a forced empty
// region, and checks with rules restated here that
//   * the blocks tile the cropped plane exactly once, the chroma blocks the chroma plane, and every bound is even;
//   * every region lies inside its block and keeps b samples from the PICTURE's edge, and the regions together are the picture without
//     that border;
//   * for every position the kernel visits (every sample with b = 1, every second row and column from the region's first with b = 2)
//     the filter's footprint -- rows and columns [pos - b, pos + 1] or [pos - 2, pos + 3], and the 2 x 2 square of the temporal term --
//     stays inside the plane: the footprint is marked in a heap block of exactly H x W bytes, so a step outside is ASan's to report;
//   * an empty region has area 0.
// One JSON line per case, "errors" empty when all is well.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../pnp_vcve_amd/csrc/xpsnr_plan.h"

namespace {

std::vector<std::string> errors;
void fail(const std::string& s) {
    if (errors.size() < 8) errors.push_back(s);
}

// the plan's N against the published formula in floating point
int block_size_fp(int H, int W) {
    const int k = (int)std::floor(32.0 * std::sqrt((double)W * H / (3840.0 * 2160.0)) + 0.5);
    return 4 * k > 4 ? 4 * k : 4;
}

// walks one plan with border b (the plan's own, or a forced one); -> positions visited
long walk(const PnpXpPlan& p, int b, long* empty_regions) {
    const int H = p.H, W = p.W;
    std::vector<unsigned char> luma((size_t)H * W, 0), chroma((size_t)(H / 2) * (W / 2), 0);
    unsigned char* touched = (unsigned char*)malloc((size_t)H * W);      // exactly the plane: a footprint outside it is a heap overflow
    for (size_t i = 0; i < (size_t)H * W; ++i) touched[i] = 0;
    std::vector<unsigned char> in_region((size_t)H * W, 0);
    long positions = 0;
    if (p.rows != (H + p.N - 1) / p.N || p.cols != (W + p.N - 1) / p.N) fail("grid: rows or cols are wrong");
    if (p.N % 4 || p.N < 4) fail("N is no multiple of 4 or below 4");
    const int lanes = pnp_xp_lanes(p.N);
    if ((lanes != 4 && lanes != 16 && lanes != 64 && lanes != 256) || (lanes < 256 && lanes < p.N * p.N / 4) || 256 % lanes) fail("lanes are wrong");
    for (int by = 0; by < p.rows; ++by)
        for (int bx = 0; bx < p.cols; ++bx) {
            const PnpXpRect k = pnp_xp_block(p, by, bx);
            if ((k.y0 | k.y1 | k.x0 | k.x1) & 1) fail("a block bound is odd");
            if (k.y0 < 0 || k.x0 < 0 || k.y1 > H || k.x1 > W || k.y1 <= k.y0 || k.x1 <= k.x0) fail("a block leaves the plane or is empty");
            for (int y = k.y0; y < k.y1; ++y)
                for (int x = k.x0; x < k.x1; ++x) luma[(size_t)y * W + x]++;
            const PnpXpRect c = pnp_xp_chroma(k);
            if (2 * c.y0 != k.y0 || 2 * c.y1 != k.y1 || 2 * c.x0 != k.x0 || 2 * c.x1 != k.x1) fail("a chroma block is not the half of its luma block");
            for (int y = c.y0; y < c.y1; ++y)
                for (int x = c.x0; x < c.x1; ++x) chroma[(size_t)y * (W / 2) + x]++;
            const PnpXpRect R = pnp_xp_region(k, H, W, b);
            if (pnp_xp_empty(R)) {
                ++*empty_regions;
                if (pnp_xp_area(R) != 0) fail("an empty region has an area");
                continue;
            }
            if (pnp_xp_area(R) != (int64_t)(R.y1 - R.y0) * (R.x1 - R.x0)) fail("a region's area is wrong");
            if (R.y0 < k.y0 || R.y1 > k.y1 || R.x0 < k.x0 || R.x1 > k.x1) fail("a region leaves its block");
            if (R.y0 < b || R.x0 < b || R.y1 > H - b || R.x1 > W - b) fail("a region touches the picture's border");
            for (int y = R.y0; y < R.y1; ++y)
                for (int x = R.x0; x < R.x1; ++x) in_region[(size_t)y * W + x]++;
            for (int y = R.y0; y < R.y1; y += b)
                for (int x = R.x0; x < R.x1; x += b) {
                    ++positions;
                    for (int yy = pnp_xp_read_lo(y, b); yy <= pnp_xp_read_hi(y, b); ++yy)
                        for (int xx = pnp_xp_read_lo(x, b); xx <= pnp_xp_read_hi(x, b); ++xx) {
                            if (yy < 0 || yy >= H || xx < 0 || xx >= W) {
                                fail("a filter footprint leaves the plane");
                                continue;
                            }
                            touched[(size_t)yy * W + xx] = 1;
                        }
                    for (int q = 0; q < b * b; ++q) {      // the temporal term's samples: the position, or its 2 x 2 square
                        const int yy = y + q / b, xx = x + q % b;
                        if (yy >= H || xx >= W) fail("the temporal term leaves the plane");
                    }
                }
        }
    for (size_t i = 0; i < luma.size(); ++i)
        if (luma[i] != 1) {
            fail("the blocks do not tile the luma plane exactly once");
            break;
        }
    for (size_t i = 0; i < chroma.size(); ++i)
        if (chroma[i] != 1) {
            fail("the chroma blocks do not tile the chroma plane exactly once");
            break;
        }
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const int want = y >= b && y < H - b && x >= b && x < W - b;
            if (in_region[(size_t)y * W + x] != want) {
                fail("the regions are not the picture without its border");
                y = H;
                break;
            }
        }
    free(touched);
    return positions;
}

void run(int h, int w, int crop, int force_b) {
    errors.clear();
    const PnpXpPlan p = pnp_xp_plan(h, w, crop);
    long empty = 0, positions = 0;
    if (!p.ok) {
        fail("the case's plane cannot be scored");
    } else {
        if (p.H != h - 2 * crop || p.W != w - 2 * crop || p.crop != crop) fail("plan: the cropped size is wrong");
        if (p.N != block_size_fp(p.H, p.W)) fail("plan: N differs from the published formula");
        if (p.b != ((int64_t)p.H * p.W > 2048 * 1152 ? 2 : 1)) fail("plan: b is wrong");
        positions = walk(p, force_b ? force_b : p.b, &empty);
    }
    printf("{\"h\": %d, \"w\": %d, \"crop\": %d, \"N\": %d, \"b\": %d, \"rows\": %d, \"cols\": %d, \"positions\": %ld, \"empty\": %ld, \"errors\": [", h, w,
           crop, p.N, force_b ? force_b : p.b, p.rows, p.cols, positions, empty);
    for (size_t i = 0; i < errors.size(); ++i) printf("%s\"%s\"", i ? ", " : "", errors[i].c_str());
    printf("]}\n");
}

}  // namespace

int main() {
    // refusals of the plan
    errors.clear();
    const int bad[][3] = {{0, 0, 0}, {1, 8, 0}, {8, 7, 0}, {8, 8, 1}, {8, 8, -2}, {8, 8, 4}, {8, 12, 6}, {(1 << 24) + 2, 8, 0}};
    for (const auto& k : bad) {
        const PnpXpPlan p = pnp_xp_plan(k[0], k[1], k[2]);
        if (p.ok || p.N || p.rows || p.cols) fail("a refused plane has a plan");
    }
    printf("{\"refusals\": true, \"errors\": [");
    for (size_t i = 0; i < errors.size(); ++i) printf("%s\"%s\"", i ? ", " : "", errors[i].c_str());
    printf("]}\n");
    int ncases = 0;
    const int sizes[][2] = {{54, 70}, {122, 204}, {182, 316}, {720, 1280}, {1080, 1920}, {1146, 2064}, {2160, 3840}, {1154, 2050}, {1152, 2048}};
    for (const auto& s : sizes)
        for (int crop : {0, 2, 6}) {
            run(s[0], s[1], crop, 0);
            ++ncases;
        }
    // both borders on ragged small planes, whatever the plan's own b would be
    const int small[][2] = {{54, 70}, {122, 204}, {30, 46}, {8, 8}, {6, 10}};
    for (int b : {1, 2})
        for (const auto& s : small) {
            run(s[0], s[1], 0, b);
            ++ncases;
        }
    // forced empty regions: a plane of two rows (b = 1), and planes of two and four rows or columns with b = 2
    run(2, 16, 0, 1), run(16, 2, 0, 1), run(2, 2, 0, 1), run(6, 6, 2, 1);
    run(4, 16, 0, 2), run(16, 4, 0, 2), run(2, 8, 0, 2), run(4, 4, 0, 2);
    ncases += 8;
    printf("{\"cases\": %d}\n", ncases);
    return 0;
}
