// Loader of 8-bit planes for the plane metrics (plane_metrics.hip): four consecutive samples of a row of a plane that sits at ANY byte
// address with ANY pitch, as the aligned dwords that cover them where those dwords lie inside the plane, byte by byte elsewhere (the
// first group of a misaligned plane, the last of its last row, the short group at the end of a cropped row).  The rule is the 4:2:0
// boundary's (include/pnpvcve.h): no byte outside the plane's rows is read -- here the last row counts up to its last sample, an
// allocation may end there.  Host and device code: tests/host/plane_metrics_stub.cpp drives the very same functions over heap blocks
// under AddressSanitizer (-DPNP_HOST_STUB: no HIP header is needed).
#pragma once
#include <stdint.h>
#include <string.h>

#ifdef PNP_HOST_STUB
#define PNP_PLANE_HD inline
#else
#include <hip/hip_runtime.h>
#define PNP_PLANE_HD __host__ __device__ __forceinline__
#endif

// One plane of a clip, or the two interleaved chroma planes of NV12 / NV21 read as one (step 2, p the one at the lower address).
struct PnpPlaneSrc {
    const unsigned char* p;     // first sample of frame 0
    int64_t pitch, frame;       // bytes between rows / between frames
    int step;                   // bytes between samples of a row: 1 | 2
    int rows;                   // rows of a frame
    int rowbytes;               // bytes of a row that exist: frame f may be read in [p + f * frame, p + f * frame + (rows - 1) * pitch + rowbytes)
};

#define PNP_PLANE_LOAD_BYTES 0
#define PNP_PLANE_LOAD_DWORDS 1

// ({hi, lo} >> 8 sh), low dword: v_alignbyte_b32 on the device, plain C++ on the host
PNP_PLANE_HD unsigned pnp_plane_alignbyte(unsigned hi, unsigned lo, unsigned sh) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbyte(hi, lo, sh);
#else
    return (unsigned)(((((unsigned long long)hi) << 32) | lo) >> (8 * sh));
#endif
}

// q is 4-byte aligned
PNP_PLANE_HD unsigned pnp_plane_ld32(const unsigned char* q) {
#if defined(__HIP_DEVICE_COMPILE__)
    return *reinterpret_cast<const unsigned*>(q);
#else
    unsigned v;
    memcpy(&v, q, 4);
    return v;
#endif
}

// The group of npix <= 4 samples that starts at column col of row `row` of frame f.
//   out[0]: sample j of the plane at s.p in byte j;  out[1] (step 2): sample j of the plane one byte behind it; bytes >= npix are 0.
// -> the form that applied: a whole group (npix == 4) whose covering aligned dwords -- 1 or 2 of them with step 1, 2 or 3 with step 2
// -- lie inside the frame's rows is fetched as those dwords and shifted into place; every other group byte by byte.
PNP_PLANE_HD int pnp_plane_load4(const PnpPlaneSrc& s, int64_t f, int row, int col, int npix, unsigned out[2]) {
    const uintptr_t lo = reinterpret_cast<uintptr_t>(s.p) + (uintptr_t)(f * s.frame);
    const uintptr_t hi = lo + (uintptr_t)((int64_t)(s.rows - 1) * s.pitch + s.rowbytes);
    const uintptr_t q = lo + (uintptr_t)((int64_t)row * s.pitch + (int64_t)col * s.step);
    const unsigned sh = (unsigned)(q & 3);
    const uintptr_t q0 = q - sh;
    if (npix == 4 && q0 >= lo && q0 + 4 * s.step + (sh ? 4 : 0) <= hi) {
        const unsigned char* d = reinterpret_cast<const unsigned char*>(q0);
        unsigned d0 = pnp_plane_ld32(d);
        if (s.step == 1) {
            if (sh) d0 = pnp_plane_alignbyte(pnp_plane_ld32(d + 4), d0, sh);
            out[0] = d0;
            out[1] = 0;
        } else {
            unsigned d1 = pnp_plane_ld32(d + 4);
            if (sh) {
                const unsigned d2 = pnp_plane_ld32(d + 8);
                d0 = pnp_plane_alignbyte(d1, d0, sh);
                d1 = pnp_plane_alignbyte(d2, d1, sh);
            }
            // little-endian bytes: d0 = a0 b0 a1 b1, d1 = a2 b2 a3 b3
            out[0] = (d0 & 0xffu) | ((d0 >> 8) & 0xff00u) | ((d1 & 0xffu) << 16) | ((d1 << 8) & 0xff000000u);
            out[1] = ((d0 >> 8) & 0xffu) | ((d0 >> 16) & 0xff00u) | ((d1 << 8) & 0xff0000u) | (d1 & 0xff000000u);
        }
        return PNP_PLANE_LOAD_DWORDS;
    }
    const unsigned char* b = reinterpret_cast<const unsigned char*>(q);
    unsigned v0 = 0, v1 = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (j < npix) {
            v0 |= (unsigned)b[(int64_t)j * s.step] << (8 * j);
            if (s.step == 2 && (int64_t)j * 2 + 1 < s.rowbytes - (int64_t)col * 2) v1 |= (unsigned)b[j * 2 + 1] << (8 * j);
        }
    }
    out[0] = v0;
    out[1] = v1;
    return PNP_PLANE_LOAD_BYTES;
}

// The samples of a plane inside its crop as `rows` runs of `roww` samples, each cut into `gpr` groups of four: group gx of run rr -> its
// row, its first column and how many of the four exist.  (Runs and groups are walked as two indices: no division on the device.)
// The crop is one per axis (crop: rows at the top and the bottom; cropx: columns left and right): the chroma planes of 4:2:2 are cropped
// by crop_border down and crop_border / 2 across.
struct PnpPlaneRuns {
    int crop, rows, roww, gpr, cropx;
};
PNP_PLANE_HD PnpPlaneRuns pnp_plane_runs(int prows, int pcols, int cropy, int cropx) {
    PnpPlaneRuns r;
    r.crop = cropy;
    r.cropx = cropx;
    r.rows = prows - 2 * cropy;
    r.roww = pcols - 2 * cropx;
    r.gpr = (r.roww + 3) / 4;
    return r;
}
PNP_PLANE_HD PnpPlaneRuns pnp_plane_runs(int prows, int pcols, int crop) { return pnp_plane_runs(prows, pcols, crop, crop); }
PNP_PLANE_HD void pnp_plane_group(const PnpPlaneRuns& r, int rr, int gx, int& row, int& col, int& npix) {
    const int left = r.roww - 4 * gx;
    npix = left < 4 ? left : 4;
    row = r.crop + rr;
    col = r.cropx + 4 * gx;
}
