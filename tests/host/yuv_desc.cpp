// Host-only check of csrc/yuv.h: the one set of descriptor predicates against the two sets it replaced, and the constants as bits.
//
// TEST INFRASTRUCTURE.  Built by tests/test_yuv_desc_host.py with a plain host compiler:
//     g++ -std=c++17 -O2 -g -fsanitize=address,undefined -fno-sanitize-recover=all -DPNP_HOST_STUB -pthread -x c++ tests/host/yuv_desc.cpp
// Until the two sample sizes shared one implementation there were four predicates: yuv_planes_ok / yuv_planes_fast on
// pnp_yuv420_planes and yuv16_planes_ok / yuv16_planes_fast on pnp_yuv420_planes16.  They are restated below, word for word, as the
// reference (ref8_*, ref16_*), and yuv.h's predicates -- reached the way the library reaches them, through yuv_planes() -- must agree
// with them on every tuple of a grid around every rule: widths, chroma steps, plane addresses of every alignment, chroma planes next
// to each other and far apart, pitches around a row's bytes, frame strides of every alignment, known and unknown depths and
// containers.  No address is dereferenced.  One JSON line for the grid, then one per (standard, depth, container) with every field of
// yuv_coef as its 32-bit pattern.
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

#include "../../pnp_vcve_amd/csrc/yuv.h"

namespace {

bool ref8_ok(const pnp_yuv420_planes& p, int w) {
    return p.y && p.cb && p.cr && (p.c_step == 1 || p.c_step == 2) && p.y_pitch >= w && p.c_pitch >= (int64_t)p.c_step * (w / 2);
}
bool ref8_fast(const pnp_yuv420_planes& p, int w) {
    if ((w & 3) || ((reinterpret_cast<uintptr_t>(p.y) | (uintptr_t)p.y_pitch | (uintptr_t)p.y_frame) & 3)) return false;
    const uintptr_t cb = reinterpret_cast<uintptr_t>(p.cb), cr = reinterpret_cast<uintptr_t>(p.cr);
    if (p.c_step == 2) {
        const uintptr_t lo = cb < cr ? cb : cr, hi = cb < cr ? cr : cb;
        return hi - lo == 1 && !((lo | (uintptr_t)p.c_pitch | (uintptr_t)p.c_frame) & 3);
    }
    return !((cb | cr | (uintptr_t)p.c_pitch | (uintptr_t)p.c_frame) & 1);
}
bool ref16_depth_ok(int bit_depth, int msb_aligned) { return (bit_depth == 10 || bit_depth == 12) && (msb_aligned == 0 || msb_aligned == 1); }
bool ref16_ok(const pnp_yuv420_planes16& p, int w) {
    if (!p.y || !p.cb || !p.cr || !ref16_depth_ok(p.bit_depth, p.msb_aligned) || (p.c_step != 1 && p.c_step != 2)) return false;
    const uintptr_t bits = reinterpret_cast<uintptr_t>(p.y) | reinterpret_cast<uintptr_t>(p.cb) | reinterpret_cast<uintptr_t>(p.cr) |
                           (uintptr_t)p.y_pitch | (uintptr_t)p.c_pitch | (uintptr_t)p.y_frame | (uintptr_t)p.c_frame;
    return !(bits & 1) && p.y_pitch >= 2 * (int64_t)w && p.c_pitch >= 2 * (int64_t)p.c_step * (w / 2);
}
bool ref16_fast(const pnp_yuv420_planes16& p, int w) {
    if ((w & 3) || ((reinterpret_cast<uintptr_t>(p.y) | (uintptr_t)p.y_pitch | (uintptr_t)p.y_frame) & 7)) return false;
    const uintptr_t cb = reinterpret_cast<uintptr_t>(p.cb), cr = reinterpret_cast<uintptr_t>(p.cr);
    if (p.c_step == 2) {
        const uintptr_t lo = cb < cr ? cb : cr, hi = cb < cr ? cr : cb;
        return hi - lo == 2 && !((lo | (uintptr_t)p.c_pitch | (uintptr_t)p.c_frame) & 7);
    }
    return !((cb | cr | (uintptr_t)p.c_pitch | (uintptr_t)p.c_frame) & 3);
}

struct Tally {
    long long tuples = 0, ok = 0, fast = 0, wrong = 0;
    char first[256] = "";
    void add(const Tally& o) {
        tuples += o.tuples, ok += o.ok, fast += o.fast;
        if (o.wrong && !wrong) memcpy(first, o.first, sizeof first);
        wrong += o.wrong;
    }
    void note(bool ok_ref, bool ok_new, bool fast_ref, bool fast_new, const char* what, int w, const YuvPlanes& p) {
        ++tuples;
        ok += ok_new;
        fast += fast_new;
        if (ok_ref == ok_new && fast_ref == fast_new) return;
        if (!wrong++)
            snprintf(first, sizeof first, "%s w=%d y=%p cb=%p cr=%p pitches %lld %lld strides %lld %lld c_step=%d depth=%d msb=%d: ok %d/%d fast %d/%d", what,
                     w, (void*)p.y, (void*)p.cb, (void*)p.cr, (long long)p.y_pitch, (long long)p.c_pitch, (long long)p.y_frame, (long long)p.c_frame,
                     p.c_step, p.bit_depth, p.msb_aligned, ok_ref, ok_new, fast_ref, fast_new);
    }
};

// "device addresses" that are never dereferenced: the Y plane and the chroma planes around two 64-byte aligned bases
const uintptr_t Y_BASE = 0x100000, C_BASE = 0x200000;
const int CR_FROM_CB[8] = {-2, -1, 0, 1, 2, 64, 65, 66};
const int64_t STRIDES[9] = {0, 1, 2, 4, 8, 1001, 1002, 1004, 1008};
const int DEPTHS[4] = {8, 9, 10, 12}, MSBS[3] = {0, 1, 2};

// the grid's tuples of one width (a thread each: 1.6e9 tuples in all)
template <int S>
void grid(Tally& T, int w) {
    for (int c_step = 0; c_step <= 3; ++c_step)
    for (int ay = 0; ay < 10; ++ay)
    for (int ab = 0; ab < 10; ++ab)
    for (int dr : CR_FROM_CB)
    for (int py = -1; py <= 9; ++py)
    for (int pc = -1; pc <= 9; ++pc)
    for (int64_t yf : STRIDES)
    for (int64_t cf : STRIDES) {
        const uintptr_t y = Y_BASE + ay, cb = C_BASE + ab, cr = cb + dr;
        const int64_t y_pitch = (int64_t)w * S + py, c_pitch = (int64_t)w * S + pc;
        if (S == 1) {
            const pnp_yuv420_planes p{(unsigned char*)y, (unsigned char*)cb, (unsigned char*)cr, y_pitch, c_pitch, yf, cf, c_step};
            const YuvPlanes q = yuv_planes(p);
            T.note(ref8_ok(p, w), yuv_planes_ok(p, w), ref8_fast(p, w), yuv_planes_fast(q, w), "8 bit", w, q);
        } else {
            for (int depth : DEPTHS)
                for (int msb : MSBS) {
                    const pnp_yuv420_planes16 p{(unsigned short*)y, (unsigned short*)cb, (unsigned short*)cr, y_pitch, c_pitch, yf, cf, c_step, depth, msb};
                    const YuvPlanes q = yuv_planes(p);
                    T.note(ref16_ok(p, w), yuv_planes_ok(p, w), ref16_fast(p, w), yuv_planes_fast(q, w), "16 bit", w, q);
                }
        }
    }
}

unsigned bits(float f) {
    unsigned u;
    memcpy(&u, &f, 4);
    return u;
}

}  // namespace

int main() {
    Tally part8[4], part16[4], t8, t16;
    std::vector<std::thread> pool;
    for (int j = 0; j < 4; ++j) pool.emplace_back([&, j] { grid<1>(part8[j], 2 + 2 * j), grid<2>(part16[j], 2 + 2 * j); });
    for (std::thread& th : pool) th.join();
    for (int j = 0; j < 4; ++j) t8.add(part8[j]), t16.add(part16[j]);
    printf("{\"grid\": 1, \"tuples8\": %lld, \"ok8\": %lld, \"fast8\": %lld, \"wrong8\": %lld, \"first8\": \"%s\", \"tuples16\": %lld, \"ok16\": %lld, "
           "\"fast16\": %lld, \"wrong16\": %lld, \"first16\": \"%s\"}\n",
           t8.tuples, t8.ok, t8.fast, t8.wrong, t8.first, t16.tuples, t16.ok, t16.fast, t16.wrong, t16.first);
    int refused = 0;
    for (int standard = 0; standard < 4; ++standard)
        for (int depth : {8, 10, 12})
            for (int msb = 0; msb <= (depth == 8 ? 0 : 1); ++msb) {
                YuvCoef k;
                if (!yuv_coef(standard, depth, msb, &k)) {
                    ++refused;
                    continue;
                }
                printf("{\"standard\": %d, \"depth\": %d, \"msb\": %d, \"cy\": %u, \"crv\": %u, \"cbu\": %u, \"cgu\": %u, \"cgv\": %u, \"kr\": %u, \"kg\": %u, "
                       "\"kb\": %u, \"sy\": %u, \"sc\": %u, \"ipb\": %u, \"ipr\": %u, \"yoff\": %d, \"cmid\": %d, \"vmax\": %u, \"shift\": %u, \"vmask\": %u}\n",
                       standard, depth, msb, bits(k.cy), bits(k.crv), bits(k.cbu), bits(k.cgu), bits(k.cgv), bits(k.kr), bits(k.kg), bits(k.kb), bits(k.sy),
                       bits(k.sc), bits(k.ipb), bits(k.ipr), k.yoff, k.cmid, bits(k.vmax), k.shift, k.vmask);
            }
    // what yuv_coef refuses: an unknown standard, a depth with no container here, a high-aligned byte
    YuvCoef k;
    const bool refusals = !yuv_coef(4, 8, 0, &k) && !yuv_coef(-1, 10, 0, &k) && !yuv_coef(0, 8, 1, &k) && !yuv_coef(0, 9, 0, &k) && !yuv_coef(0, 16, 0, &k) &&
                          !yuv_coef(0, 10, 2, &k);
    printf("{\"refusals\": %d}\n", refusals ? 1 : 0);
    return (t8.wrong || t16.wrong || refused || !refusals) ? 1 : 0;
}
