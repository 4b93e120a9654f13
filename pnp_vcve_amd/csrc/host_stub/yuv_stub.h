// Host-only stand-ins (-DPNP_HOST_STUB) for the launchers of the 4:2:0 boundary that the clip scheduler (csrc/generator.hip) calls:
// launch_pack_lr_yuv420, launch_frames_from_yuv420 and launch_frames_to_yuv420 (yuv.h), for planes of either sample size.  As in
// io_stub.h a launch is a record, appended to pnp_stub_yuv_log and handed to pnp_stub_yuv_hook, where tests/host/yuv_stub.cpp and
// tests/host/yuv16_stub.cpp do their range bookkeeping at launch time; the earlier host tests never reach one and compile without
// knowing them.  conv_last's launch behind a 4:2:0 clip is io_stub.h's PNP_STUB_IO_CONV_LAST record (ConvArgs::lr_rgb0 says what it
// reads).  Nothing here is used by the product build.
#pragma once
#include <vector>

#include "../yuv.h"

enum { PNP_STUB_YUV_PACK = 0, PNP_STUB_YUV_FROM = 1, PNP_STUB_YUV_TO = 2 };

struct PnpStubYuvLaunch {
    int kind;                  // PNP_STUB_YUV_*
    hipStream_t stream;
    YuvPlanes planes;          // read (pack, from) or written (to); sample_bytes, bit_depth and msb_aligned tell the container
    const float* in;           // PNP_STUB_YUV_TO: the fp32 planes read
    float* out;                // pack: RGB0 frames; from: fp32 planes
    int frames, h, w;
    bool fast;                 // pack: the aligned form would run (four- / two-sample loads)
};

inline std::vector<PnpStubYuvLaunch> pnp_stub_yuv_log;
inline void (*pnp_stub_yuv_hook)(const PnpStubYuvLaunch&) = nullptr;

inline int pnp_stub_yuv_record(const PnpStubYuvLaunch& r) {
    pnp_stub_yuv_log.push_back(r);
    if (pnp_stub_yuv_hook) pnp_stub_yuv_hook(r);
    return 0;
}

inline bool pnp_stub_yuv_args_ok(const YuvPlanes& p, const YuvCoef& k, int n, int H, int W) {      // yuv.hip's own checks
    return yuv_frame_ok(k.format, n, H, W) && yuv_planes_ok(p, W, k.format);
}

inline int launch_pack_lr_yuv420(const YuvPlanes& in, const YuvCoef& k, float* lr4, int T, int H, int W, bool force_general, hipStream_t stream) {
    if (!lr4 || !pnp_stub_yuv_args_ok(in, k, T, H, W)) return PNP_ERR_BAD_ARG;
    return pnp_stub_yuv_record(PnpStubYuvLaunch{PNP_STUB_YUV_PACK, stream, in, nullptr, lr4, T, H, W, !force_general && yuv_planes_fast(in, W, k.format)});
}

inline int launch_frames_from_yuv420(const YuvPlanes& in, const YuvCoef& k, float* out, int nframes, int H, int W, hipStream_t stream) {
    if (!out || !pnp_stub_yuv_args_ok(in, k, nframes, H, W)) return PNP_ERR_BAD_ARG;
    return pnp_stub_yuv_record(PnpStubYuvLaunch{PNP_STUB_YUV_FROM, stream, in, nullptr, out, nframes, H, W, false});
}

inline int launch_frames_to_yuv420(const float* in, const YuvPlanes& out, const YuvCoef& k, int nframes, int H, int W, hipStream_t stream) {
    if (!in || !pnp_stub_yuv_args_ok(out, k, nframes, H, W)) return PNP_ERR_BAD_ARG;
    return pnp_stub_yuv_record(PnpStubYuvLaunch{PNP_STUB_YUV_TO, stream, out, in, nullptr, nframes, H, W, false});
}
