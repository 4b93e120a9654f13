// The planes of a Y'CbCr clip as sources of the plane loader (plane_load.h): the Y plane, and the chroma planes with the rows and
// columns their chroma format gives them (yuv.h: (h / sy) x (w / sx)), the geometry and crop of a plane of a format, and -- what every
// plane entry of the device metrics fills its kernel arguments with -- the three planes of a clip on either sample path (PlaneSamp,
// clip_planes).  Host code only, shared by the metric units through metric_src.h; tests/host/yuv_formats_desc.cpp walks these very
// sources through pnp_plane_load4 over exactly-sized heap blocks under AddressSanitizer (-DPNP_HOST_STUB).
#pragma once
#include "plane_load.h"
#include "yuv.h"

// The chroma of one clip: paired (NV12 / NV21: one load gives both planes; c[0] is the pair at the lower address and cr_first says
// which plane that is) or two planes of their own (I420; c[0] = Cb, c[1] = Cr).
struct ChromaSrc {
    PnpPlaneSrc c[2];
    int paired, cr_first;
};

static inline PnpPlaneSrc luma_src(const pnp_yuv420_planes& p, int h, int w) { return PnpPlaneSrc{p.y, p.y_pitch, p.y_frame, 1, h, w}; }

// (format: PNP_YUV_FORMAT_*, the chroma planes' true rows and columns; 4:4:4 planar chroma has rowbytes c_step * (w - 1) + 1)
static inline ChromaSrc chroma_src(const pnp_yuv420_planes& p, int h, int w, int format = PNP_YUV_FORMAT_420) {
    ChromaSrc s;
    const int rows = h / yuv_sy(format), cols = w / yuv_sx(format);
    const uintptr_t cb = reinterpret_cast<uintptr_t>(p.cb), cr = reinterpret_cast<uintptr_t>(p.cr);
    s.paired = p.c_step == 2 && (cb > cr ? cb - cr : cr - cb) == 1;
    s.cr_first = cr < cb;
    if (s.paired) {
        s.c[0] = s.c[1] = PnpPlaneSrc{s.cr_first ? p.cr : p.cb, p.c_pitch, p.c_frame, 2, rows, 2 * cols};
    } else {
        const int rowbytes = p.c_step * (cols - 1) + 1;
        s.c[0] = PnpPlaneSrc{p.cb, p.c_pitch, p.c_frame, p.c_step, rows, rowbytes};
        s.c[1] = PnpPlaneSrc{p.cr, p.c_pitch, p.c_frame, p.c_step, rows, rowbytes};
    }
    return s;
}

// The geometry of one plane (PNP_PLANE_*) of h x w frames in a format under crop_border = crop: rows, columns, and the crop down and
// across -- the Y plane is cropped by crop on every side, the chroma planes by crop / sy down and crop / sx across.
struct PlaneGeom { int H, W, cropy, cropx; };
static inline PlaneGeom plane_geom(int h, int w, int crop, int plane, int format) {
    if (plane == PNP_PLANE_Y) return PlaneGeom{h, w, crop, crop};
    const int sx = yuv_sx(format), sy = yuv_sy(format);
    return PlaneGeom{h / sy, w / sx, crop / sy, crop / sx};
}

// One plane of a 10 / 12-bit clip (pnp_yuv420_planes16): 2-byte loads, sample (row, col) of frame f is the word at
// p + f * frame + row * pitch (bytes) + col * step (samples), read as (word >> shift) & mask (metric_src.h::load16).
struct Plane16 {
    const unsigned short* p;
    long pitch, frame;
    int step;
    unsigned shift, mask;
};
static inline Plane16 plane16(const pnp_yuv420_planes16& p, int plane) {      // plane: 0 Y | 1 Cb | 2 Cr
    const unsigned shift = p.msb_aligned ? 16u - (unsigned)p.bit_depth : 0u, mask = (1u << p.bit_depth) - 1u;
    if (plane == 0) return Plane16{p.y, p.y_pitch, p.y_frame, 1, shift, mask};
    return Plane16{plane == 1 ? p.cb : p.cr, p.c_pitch, p.c_frame, p.c_step, shift, mask};
}

// One plane of one clip on either sample path; only the members of the kernel instance's kind are read.
struct PlaneSamp {
    PnpPlaneSrc p8;         // 8-bit: the plane, or the interleaved pair it is one of, as pnp_plane_load4 reads it
    int sel;                //        the plane is the second word of the loader's pair
    Plane16 p16;            // 16-bit words
};

// out = the Y, Cb and Cr planes of a clip of h x w frames of a chroma format (PNP_YUV_FORMAT_*) / of a 16-bit clip
static inline void clip_planes(const pnp_yuv420_planes& p, int h, int w, int format, PlaneSamp out[3]) {
    const ChromaSrc cs = chroma_src(p, h, w, format);
    out[0] = PlaneSamp{luma_src(p, h, w), 0, Plane16{}};
    for (int cr = 0; cr < 2; ++cr)
        out[1 + cr] = PlaneSamp{cs.c[cr], cs.paired && cr != cs.cr_first, Plane16{}};      // sel: the plane one byte behind the pair's first
}
static inline void clip_planes(const pnp_yuv420_planes16& p, PlaneSamp out[3]) {
    for (int k = 0; k < 3; ++k) out[k] = PlaneSamp{PnpPlaneSrc{}, 0, plane16(p, k)};
}

// a plane mask names at least one of PNP_PLANE_Y | PNP_PLANE_CB | PNP_PLANE_CR and nothing else
static inline bool plane_mask_ok(int mask) { return mask >= 1 && mask <= 7; }
