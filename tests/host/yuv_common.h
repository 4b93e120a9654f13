// What tests/host/yuv_stub.cpp and tests/host/yuv16_stub.cpp share: the rows a 4:2:0 launch touches, the heap block of a plane and
// the question whether a range was written at all.  TEST INFRASTRUCTURE; included behind sched_stub.cpp, whose bookkeeping it uses.
#pragma once

namespace {

using namespace stub;

// the bytes of `frames` frames of h x w a launch touches: each row's samples, nothing of the padding.  Pitches and frame strides are
// bytes, c_step is samples, sample_bytes the size of one
template <class F>
void each_row(const YuvPlanes& p, int frames, int h, int w, F f) {
    const size_t S = (size_t)p.sample_bytes;
    for (int i = 0; i < frames; ++i) {
        for (int r = 0; r < h; ++r) f("a row of the Y plane", p.y + (int64_t)i * p.y_frame + (int64_t)r * p.y_pitch, (size_t)w * S);
        for (int r = 0; r < h / 2; ++r) {
            const int64_t o = (int64_t)i * p.c_frame + (int64_t)r * p.c_pitch;
            if (p.c_step == 2) {
                f("a row of interleaved chroma", (p.cb < p.cr ? p.cb : p.cr) + o, (size_t)w * S);
            } else {
                f("a row of the Cb plane", p.cb + o, (size_t)w / 2 * S);
                f("a row of the Cr plane", p.cr + o, (size_t)w / 2 * S);
            }
        }
    }
}

// One plane (or one interleaved chroma pair) of a clip: a heap block whose first 8 bytes are poisoned, the plane `lead` bytes in, the
// block ending with the last sample of the last row.
struct Block {
    unsigned char *base = nullptr, *p = nullptr;
    size_t bytes = 0;
    void make(int t, int rows, int64_t pitch, int64_t frame, int64_t row_bytes, int lead) {
        bytes = (size_t)((t - 1) * frame + (rows - 1) * pitch + row_bytes);
        base = (unsigned char*)malloc(lead + bytes);      // (malloc: 16-byte aligned)
        p = base + lead;
#if PNP_HAVE_ASAN
        ASAN_POISON_MEMORY_REGION(base, 8);
#endif
    }
    void release() {
#if PNP_HAVE_ASAN
        if (base) ASAN_UNPOISON_MEMORY_REGION(base, 8);
#endif
        free(base);
        base = p = nullptr;
    }
};

bool any_written(const void* p, size_t n) {
    const uintptr_t lo = (uintptr_t)p, hi = lo + n;
    for (const auto& iv : written)
        if (iv.first < hi && iv.second > lo) return true;
    return false;
}

}  // namespace
