// Host-only stand-in (-DPNP_HOST_STUB) for launch_par_fold_table (conv_mfma.h, conv_persist.hip), which the clip scheduler
// (csrc/generator.hip) calls in front of a branch run.  As in io_stub.h: the recording launchers of the scheduler's other kernels live
// in tests/host/sched_stub.cpp, which the earlier host tests include unchanged, so this one is defined here and they keep compiling
// without knowing it (and their ordered traces stay what they were).  A launch is a record, appended to pnp_stub_fold_log and handed
// to pnp_stub_fold_hook, where the test that checks the table's order against the front halves (tests/host/fold_table_stub.cpp)
// does its range bookkeeping at launch time.  Nothing here is used by the product build.
#pragma once
#include <vector>

#include "../conv_mfma.h"

struct PnpStubFoldLaunch {
    hipStream_t stream;
    const float* par;      // 3 planes per frame, `plane` floats apart
    long plane;
    PnpFoldRec* tab;       // frames * pnp_fold_records(h, w) records written
    int frames, h, w;
};

inline std::vector<PnpStubFoldLaunch> pnp_stub_fold_log;
inline void (*pnp_stub_fold_hook)(const PnpStubFoldLaunch&) = nullptr;

inline int launch_par_fold_table(const float* par, long par_plane, PnpFoldRec* tab, int frames, int H, int W, hipStream_t stream) {
    if (!par || !tab || frames < 1 || H < 1 || W < 1) return PNP_ERR_BAD_ARG;       // conv_persist.hip's own checks
    const PnpStubFoldLaunch r{stream, par, par_plane, tab, frames, H, W};
    pnp_stub_fold_log.push_back(r);
    if (pnp_stub_fold_hook) pnp_stub_fold_hook(r);
    return 0;
}
