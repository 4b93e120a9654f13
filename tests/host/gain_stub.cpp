// Host stub for csrc/gain_plan.h, built with -DPNP_HOST_STUB -fsanitize=address,undefined and run by tests/test_gain_ref.py.
//
// gain_kernel (csrc/gain.hip) takes its region, its cells, its tiles, a tile's rows and a lane's columns from the functions of that
// header.  This program walks every tile, wave and lane the launcher would start, exactly as the kernel does, over a heap block of
// exactly rows * cols bytes -- so a sample fetched outside the plane is an AddressSanitizer report -- and checks that
//   * every sample of the region is owned by exactly one lane of exactly one tile, and no sample outside it is touched;
//   * the cell the kernel adds a sample to (the lane's cell of the tile) is the cell pnp_gain_cell_of gives that sample, lies among the
//     tile's cells, and is written by that tile alone;
//   * every cell of the grid is written by exactly one tile (the cells in the crop too: they hold zeros);
//   * the samples a cell received are pnp_gain_cell_samples' closed form, and they sum to the region's size.
// One JSON line per case with the cells' counts; the test compares them with its own enumeration.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../pnp_vcve_amd/csrc/gain_plan.h"

static int run_case(int h, int w, int crop, int block, int sx, int sy) {
    std::string err;
    auto fail = [&](const std::string& what) {
        if (err.empty()) err = "\"" + what + "\"";
    };
    const PnpGainPlane p = pnp_gain_plane(h, w, crop, block, sx, sy);
    if (!p.ok) {
        printf("{\"h\": %d, \"w\": %d, \"crop\": %d, \"block\": %d, \"sx\": %d, \"sy\": %d, \"errors\": [\"refused\"]}\n", h, w, crop, block, sx, sy);
        return 1;
    }
    int gr, gc;
    pnp_gain_grid_of(h, w, block, gr, gc);
    if (gr != p.grows || gc != p.gcols) fail("grid");
    unsigned char* owned = static_cast<unsigned char*>(calloc((size_t)p.rows * p.cols, 1));       // exactly the plane
    std::vector<int64_t> got((size_t)gr * gc, 0);
    std::vector<int> writers((size_t)gr * gc, 0);
    const int tiles = pnp_gain_tiles(p);
    for (int tile = 0; tile < tiles; ++tile) {
        int ti, tx, r0, r1, j0, ncell;
        pnp_gain_tile(p, tile, ti, tx, r0, r1, j0, ncell);
        if (ti < 0 || ti >= gr || ncell < 1 || ncell > PNP_GAIN_MAX_CELLS || j0 < 0 || j0 + ncell > gc) fail("tile " + std::to_string(tile));
        for (int ce = 0; ce < ncell; ++ce) ++writers[(size_t)ti * gc + j0 + ce];                  // the block's stores
        for (int wave = 0; wave < 4; ++wave)
            for (int lane = 0; lane < 64; ++lane) {
                int col, n, cell;
                pnp_gain_lane_cols(p, tx, lane, col, n, cell);
                if (cell < 0 || cell >= PNP_GAIN_MAX_CELLS) fail("lane cell");                    // it indexes the block's LDS
                if (n <= 0) continue;
                if (cell >= ncell) fail("a sample in a cell the tile does not write");
                for (int row = r0 + wave; row < r1; row += 4)
                    for (int j = 0; j < n; ++j) {
                        ++owned[(size_t)row * p.cols + col + j];
                        int ci, cj;
                        pnp_gain_cell_of(p, row, col + j, ci, cj);
                        if (ci != ti || cj != j0 + cell) fail("cell of " + std::to_string(row) + "," + std::to_string(col + j));
                        else ++got[(size_t)ci * gc + cj];
                    }
            }
    }
    int64_t total = 0;
    for (int y = 0; y < p.rows; ++y)
        for (int x = 0; x < p.cols; ++x) {
            const bool in = y >= p.y0 && y < p.y1 && x >= p.x0 && x < p.x1;
            if (owned[(size_t)y * p.cols + x] != (in ? 1 : 0)) fail("ownership at " + std::to_string(y) + "," + std::to_string(x));
        }
    std::string counts;
    for (int i = 0; i < gr; ++i)
        for (int j = 0; j < gc; ++j) {
            const int64_t v = got[(size_t)i * gc + j];
            if (v != pnp_gain_cell_samples(p, i, j)) fail("closed form of cell " + std::to_string(i) + "," + std::to_string(j));
            if (writers[(size_t)i * gc + j] != 1) fail("writers of cell " + std::to_string(i) + "," + std::to_string(j));
            total += v;
            counts += (counts.empty() ? "" : ", ") + std::to_string((long long)v);
        }
    if (total != (int64_t)(p.y1 - p.y0) * (p.x1 - p.x0)) fail("total");
    printf("{\"h\": %d, \"w\": %d, \"crop\": %d, \"block\": %d, \"sx\": %d, \"sy\": %d, \"grows\": %d, \"gcols\": %d, \"tiles\": %d, \"tiles_x\": %d, "
           "\"counts\": [%s], \"errors\": [%s]}\n",
           h, w, crop, block, sx, sy, gr, gc, tiles, p.tiles_x, counts.c_str(), err.c_str());
    free(owned);
    return err.empty() ? 0 : 1;
}

int main() {
    const int sizes[][2] = {{64, 80}, {66, 78}, {130, 70}, {16, 16}, {34, 530}, {18, 258}, {2, 2}};
    const int crops[] = {0, 2, 6};
    const int blocks[] = {16, 32, 64, 128};
    const int factors[][2] = {{1, 1}, {2, 2}, {2, 1}};
    int cases = 0, bad = 0;
    for (const auto& s : sizes)
        for (int crop : crops)
            for (int block : blocks)
                for (const auto& f : factors) {
                    if (2 * crop >= s[0] || 2 * crop >= s[1]) continue;
                    ++cases;
                    bad += run_case(s[0], s[1], crop, block, f[0], f[1]);
                }
    bad += run_case(67, 79, 3, 16, 1, 1);                             // odd sizes and an odd crop: frames of pixels, 4:4:4
    ++cases;
    // refusals
    const int refused[][6] = {{0, 8, 0, 16, 1, 1}, {8, 8, 4, 16, 1, 1}, {8, 8, -1, 16, 1, 1}, {16, 16, 0, 8, 1, 1}, {16, 16, 0, 48, 1, 1},
                              {16, 16, 0, 256, 1, 1}, {17, 16, 0, 16, 2, 2}, {16, 17, 0, 16, 2, 1}, {16, 16, 0, 16, 3, 1}};
    for (const auto& r : refused)
        if (pnp_gain_plane(r[0], r[1], r[2], r[3], r[4], r[5]).ok) {
            printf("{\"refusal_missed\": [%d, %d, %d, %d, %d, %d]}\n", r[0], r[1], r[2], r[3], r[4], r[5]);
            ++bad;
        }
    printf("{\"cases\": %d}\n", cases);
    return bad ? 1 : 0;
}
