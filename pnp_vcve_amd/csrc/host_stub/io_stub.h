// Host-only stand-ins (-DPNP_HOST_STUB) for the launchers of the byte-frame boundary that the clip scheduler (csrc/generator.hip)
// calls: launch_pack_lr_u8 (and its any_size form), launch_frames_from_rgb8, launch_frames_to_rgb8 (prep.h) and launch_conv_last_io (conv_mfma.h).
//
// The recording launchers of the scheduler's other kernels live in tests/host/sched_stub.cpp, which the earlier host tests include
// unchanged; these four are defined here so that those tests keep compiling without knowing them (a forward at the fp32 boundary
// never reaches one).  A launch is a record, as in hip_stub.h: it is appended to pnp_stub_io_log and handed to pnp_stub_io_hook,
// where the test that drives the byte boundary (tests/host/byte_frames_stub.cpp) does its range bookkeeping at launch time -- the
// conv source the pack launch writes must count as written before the first input conv reads it.  Nothing here is used by the
// product build.
#pragma once
#include <vector>

#include "../conv_mfma.h"
#include "../prep.h"

enum { PNP_STUB_IO_PACK_LR_U8 = 0, PNP_STUB_IO_FROM_RGB8 = 1, PNP_STUB_IO_TO_RGB8 = 2, PNP_STUB_IO_CONV_LAST = 3 };

struct PnpStubIoLaunch {
    int kind;              // PNP_STUB_IO_*
    hipStream_t stream;
    const void* in;        // the bytes (pack, from) or the fp32 planes (to) read; nullptr for the conv (see `conv`)
    void* out;             // what is written: RGB0 frames, fp32 planes, bytes
    int frames, h, w;      // h, w: of the frames converted
    ConvArgs conv;         // PNP_STUB_IO_CONV_LAST: the launch's arguments (lr / lr_u8, out / out_u8 say what it touches)
};

inline std::vector<PnpStubIoLaunch> pnp_stub_io_log;
inline void (*pnp_stub_io_hook)(const PnpStubIoLaunch&) = nullptr;

inline int pnp_stub_io_record(const PnpStubIoLaunch& r) {
    pnp_stub_io_log.push_back(r);
    if (pnp_stub_io_hook) pnp_stub_io_hook(r);
    return 0;
}

inline int launch_pack_lr_u8(const unsigned char* lq, float* lr4, int T, int H, int W, hipStream_t stream) {
    if (T < 1 || (((long)H * W * T) & 3) || (reinterpret_cast<uintptr_t>(lq) & 3)) return PNP_ERR_BAD_ARG;       // prep.hip's own checks
    PnpStubIoLaunch r{PNP_STUB_IO_PACK_LR_U8, stream, lq, lr4, T, H, W, {}};
    return pnp_stub_io_record(r);
}

inline int launch_pack_lr_u8_any(const unsigned char* lq, float* lr4, int T, int H, int W, hipStream_t stream) {
    if (T < 1 || H < 1 || W < 1 || !lq || !lr4) return PNP_ERR_BAD_ARG;
    PnpStubIoLaunch r{PNP_STUB_IO_PACK_LR_U8, stream, lq, lr4, T, H, W, {}};      // (the same ranges: t*h*w*3 bytes read, 16 B per pixel written)
    return pnp_stub_io_record(r);
}

inline int launch_frames_from_rgb8(const unsigned char* in, float* out, int nframes, int H, int W, hipStream_t stream) {
    PnpStubIoLaunch r{PNP_STUB_IO_FROM_RGB8, stream, in, out, nframes, H, W, {}};
    return pnp_stub_io_record(r);
}

inline int launch_frames_to_rgb8(const float* in, unsigned char* out, int nframes, int H, int W, hipStream_t stream) {
    PnpStubIoLaunch r{PNP_STUB_IO_TO_RGB8, stream, in, out, nframes, H, W, {}};
    return pnp_stub_io_record(r);
}

inline int launch_conv_last_io(const ConvArgs& a, hipStream_t stream) {
    if (!conv_last_valu_shape(a, CONV_CFG_RGB, 1, a.lr || a.lr_u8 || a.lr_rgb0) || (!a.out && !a.out_u8)) return PNP_ERR_UNSUPPORTED;      // conv_last.hip's rule
    PnpStubIoLaunch r{PNP_STUB_IO_CONV_LAST, stream, nullptr, nullptr, 1, a.H, a.W, a};
    return pnp_stub_io_record(r);
}
