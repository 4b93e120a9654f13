// Host-only stand-ins (-DPNP_HOST_STUB) for the launchers of the 10 / 12-bit 4:2:0 boundary that the clip scheduler
// (csrc/generator.hip) calls: launch_pack_lr_yuv420p16, launch_frames_from_yuv420p16 and launch_frames_to_yuv420p16 (yuv16.h).  As in
// yuv_stub.h a launch is a record, appended to pnp_stub_yuv16_log and handed to pnp_stub_yuv16_hook, where tests/host/yuv16_stub.cpp
// does its range bookkeeping at launch time; the earlier host tests never reach one and compile without knowing them.  Nothing
// here is used by the product build.
#pragma once
#include <vector>

#include "../yuv16.h"
#include "yuv_stub.h"      // the record kinds (PNP_STUB_YUV_*)

struct PnpStubYuv16Launch {
    int kind;                    // PNP_STUB_YUV_*
    hipStream_t stream;
    pnp_yuv420_planes16 planes;  // read (pack, from) or written (to)
    const float* in;             // PNP_STUB_YUV_TO: the fp32 planes read
    float* out;                  // pack: RGB0 frames; from: fp32 planes
    int frames, h, w;
    bool fast;                   // pack: the aligned form would run (8-byte / 4-byte loads)
};

inline std::vector<PnpStubYuv16Launch> pnp_stub_yuv16_log;
inline void (*pnp_stub_yuv16_hook)(const PnpStubYuv16Launch&) = nullptr;

inline int pnp_stub_yuv16_record(const PnpStubYuv16Launch& r) {
    pnp_stub_yuv16_log.push_back(r);
    if (pnp_stub_yuv16_hook) pnp_stub_yuv16_hook(r);
    return 0;
}

inline bool pnp_stub_yuv16_args_ok(const pnp_yuv420_planes16& p, int n, int H, int W) {      // yuv16.hip's own checks
    return n >= 1 && H >= 2 && W >= 2 && !(H & 1) && !(W & 1) && yuv16_planes_ok(p, W);
}

inline int launch_pack_lr_yuv420p16(const pnp_yuv420_planes16& in, const YuvCoef16&, float* lr4, int T, int H, int W, bool force_general,
                                    hipStream_t stream) {
    if (!lr4 || !pnp_stub_yuv16_args_ok(in, T, H, W)) return PNP_ERR_BAD_ARG;
    return pnp_stub_yuv16_record(PnpStubYuv16Launch{PNP_STUB_YUV_PACK, stream, in, nullptr, lr4, T, H, W, !force_general && yuv16_planes_fast(in, W)});
}

inline int launch_frames_from_yuv420p16(const pnp_yuv420_planes16& in, const YuvCoef16&, float* out, int nframes, int H, int W, hipStream_t stream) {
    if (!out || !pnp_stub_yuv16_args_ok(in, nframes, H, W)) return PNP_ERR_BAD_ARG;
    return pnp_stub_yuv16_record(PnpStubYuv16Launch{PNP_STUB_YUV_FROM, stream, in, nullptr, out, nframes, H, W, false});
}

inline int launch_frames_to_yuv420p16(const float* in, const pnp_yuv420_planes16& out, const YuvCoef16&, int nframes, int H, int W, hipStream_t stream) {
    if (!in || !pnp_stub_yuv16_args_ok(out, nframes, H, W)) return PNP_ERR_BAD_ARG;
    return pnp_stub_yuv16_record(PnpStubYuv16Launch{PNP_STUB_YUV_TO, stream, out, in, nullptr, nframes, H, W, false});
}
