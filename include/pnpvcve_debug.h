/* libpnpvcve_hip.so -- diagnostic entry points (kernel-variant selection and in-kernel timelines).
 *
 * Declared separately from pnpvcve.h because nothing in the reference corresponds to them: they exist so that
 * tests can compare two kernels of this build bit for bit and so that tools/trace_*.py can read shader-clock
 * timelines.  Same conventions as pnpvcve.h (device pointers, void* stream, int return); no global state -- the
 * variant and the trace buffer are arguments of the call.
 */
#ifndef PNPVCVE_DEBUG_H
#define PNPVCVE_DEBUG_H
#include "pnpvcve.h"
#ifdef __cplusplus
extern "C" {
#endif

#define PNP_CONV_AUTO 0     /* what pnp_conv3x3_f32 does: persistent strips from 1024 tiles, else tile per block */
#define PNP_CONV_TILE 1     /* tile-per-block kernel, tile size picked from the frame size */
#define PNP_CONV_TILE_BIG 2 /* tile-per-block kernel, 8x16 tiles */

/* The fused conv of pnpvcve.h (sr_backbone_utils.py:304-333 halves, basicvsr_net.py:484, iconvsr.py:365) with an explicit kernel
 * variant, optional per-tile partition flags (pnp_par_tile_flags_f32; NULL = no branch skipped) and an optional
 * timeline buffer (8-16 u64 per block, device memory, NULL = none). */
int pnp_conv3x3_f32_ex(int nsrc, const float* const* srcs_dev, const int* src_channels,
                       const float* const* packed_w_dev, const float* bias_dev, const float* gamma_dev,
                       const float* packed_w1x1_dev, const float* par_dev, const float* residual_dev,
                       int act, float* out_dev, int h, int w, int variant, const int* par_flags_dev,
                       void* trace_dev, void* stream);

/* pnp_conv3x3_wino_f32 of pnpvcve.h with a timeline buffer (16 u64 per block: [0] start tick, [1] K-loop ticks, [2] epilogue ticks,
 * [3] end tick, [7] tiles walked, [13] / [14] the 100 MHz counter at start / end; NULL = none). */
int pnp_conv3x3_wino_f32_ex(const float* src_dev, const float* wino_w_dev, const float* bias_dev, const float* gamma_dev,
                            const float* wino_w1x1_dev, const float* par_dev, const int* par_flags_dev,
                            const float* residual_dev, int act, float* out_dev, int h, int w, void* trace_dev, void* stream);
/* The frame's partition word (pnp_generator_forward computes it per frame: bit 3 = every 8x8 quadrant is all zero or one constant
 * plane) for the NEXT pnp_conv3x3_wino_f32_ex calls with branches: they then take the one gated launch the generator uses (fold-only
 * body when bit 3 is set).  A device int; NULL = back to the ungated branch kernel.  Process-wide, not thread-safe: a tracing hook. */
int pnp_debug_wino_gate_word(const int* gate_word_dev);
/* The frame's fold table, which the fold-only body reads instead of the partition planes (pnp_generator_forward makes it in front of
 * every branch run; a gated pnp_conv3x3_wino_f32_ex call makes its own): for a (3, h, w) partition map, 4 * ceil(h / 16) * ceil(w / 16)
 * records of two 32-bit words -- the plane to fold (0..2, or -1) and the bits of the fp32 factor 0.25f * value -- one per 8x8
 * quadrant, in the order record((tile_y * tiles_x + tile_x) * 4 + 2 * (qy & 1) + (qx & 1)) with tile = quadrant >> 1; from the
 * quadrant's first pixel: the lowest plane that is nonzero there, -1 and 0 if none is or the quadrant lies outside the frame. */
int pnp_debug_par_fold_table(const float* par_dev, void* table_dev, int h, int w, void* stream);

/* The NEXT pnp_conv3x3_wino_f32 / _ex / pnp_conv3x3_wino_ms_f32 calls (tile kernels, not the quadrant-unit forms) compute the 16-pixel
 * tile rows [row0, row0 + nrows) of the frame only and leave the rest of out_dev untouched -- one part of a row-band chain
 * (pnp_generator_set_band_split).  nrows = 0: back to whole frames.  A range beyond the frame's ceil(h / 16) rows: the conv returns
 * PNP_ERR_BAD_ARG.  Process-wide, not thread-safe: a test hook. */
int pnp_debug_wino_tile_rows(int row0, int nrows);

/* A timeline buffer (the 16 u64 per block of pnp_conv3x3_wino_f32_ex; [1] sums the frame's chunks and every source segment of a tile)
 * for the NEXT pnp_conv3x3_wino_ms_f32 calls (tile kernel only).  NULL = none.  Process-wide, not thread-safe: a tracing hook. */
int pnp_debug_wino_ms_trace(void* trace_dev);

/* The byte-frame unpacking in front of pnp_generator_forward_clips' convs, alone: lq_dev (t,h,w,3) uint8 -> lr4_dev (t,h,w,4) fp32
 * RGB0, every byte through the table of pnp_frames_from_rgb8.  any_size = 0: the form for whole 12-byte groups on a 4-aligned address
 * (PNP_ERR_BAD_ARG otherwise, before any launch); 1: the form pnp_generator_set_any_size adds, any address and any t*h*w. */
int pnp_debug_pack_lr_u8(const unsigned char* lq_dev, float* lr4_dev, int t, int h, int w, int any_size, void* stream);

/* The 4:2:0 unpacking in front of pnp_generator_forward_clips_yuv's convs, alone: t frames of planes -> lr4_dev (t,h,w,4) fp32 RGB0,
 * the values of pnp_frames_from_yuv420.  general = 0: the form the forward picks (the aligned one where planes and pitches are 4-byte
 * aligned and w is a multiple of 4); 1: the byte-load form whatever the alignment.  Same values either way.  yuv_standard takes
 * PNP_YUV_CODE(standard, chroma) as every 4:2:0 entry does: a chroma mode other than 0 runs the sited forms of the two kernels. */
int pnp_debug_pack_lr_yuv420(const pnp_yuv420_planes* in_host_desc, int yuv_standard, float* lr4_dev, int t, int h, int w,
                             int general, void* stream);
/* The same for 10 / 12-bit planes (pnp_generator_forward_clips_yuv16): the values of pnp_frames_from_yuv420p16.  general = 0: the
 * aligned form where planes, pitches and strides are 8-byte aligned and w is a multiple of 4; 1: the 2-byte-load form. */
int pnp_debug_pack_lr_yuv420p16(const pnp_yuv420_planes16* in_host_desc, int yuv_standard, float* lr4_dev, int t, int h, int w,
                                int general, void* stream);

/* The row-band plan of pnp_generator_set_band_split as a pure function: for a chain of nconv convs on a frame of `rows` tile rows,
 * writes the boundary row a_n of each conv (chain A: tile rows [0, a_n), chain B: [a_n, rows); a_n = a_0 - n) to bounds[0 .. nconv)
 * and returns 1, or returns 0 (bounds untouched) when the frame has too few rows for both regions to stay non-empty: no split.
 * a0 = 0: the centred trapezoid a_0 = (rows + nconv - 1) / 2; a0 > 0: that first boundary. */
int pnp_band_plan(int rows, int nconv, int a0, int* bounds);

/* The fp16-operand conv of pnpvcve.h with an optional timeline buffer (16 u64 per 4-wave group). */
int pnp_conv3x3_f16_ex(int nsrc, const float* const* srcs_dev, const int* src_channels,
                       const void* const* packed_w_f16_dev, const float* bias_dev, const float* gamma_dev,
                       const void* packed_w1x1_f16_dev, const float* par_dev, const float* residual_dev,
                       int act, float* out_dev, int h, int w, void* trace_dev, void* stream);

/* The modulated deformable conv of pnpvcve.h with an optional timeline buffer: 8 u64 per wave (8 waves per block,
 * one block per CU): shader-clock sums of window fill, prologue, gather, MFMA, barrier + weight hand-over, epilogue,
 * total, tiles.  The buffer must hold pnp_dcn_trace_u64s() elements (the launch has one block per CU of the current device). */
int pnp_dcn_trace_u64s(void);
int pnp_dcn_nhwc_f32_ex(const float* x_dev, const float* om_dev, const float* flow_x_dev, const float* flow_y_dev,
                        const float* w_packed_dev, const float* bias_dev, float* out_dev, int h, int w, void* trace_dev,
                        void* stream);

/* The fp16-operand conv with explicit fp16 maps, as pnp_generator_forward chains its launches under PNP_OPT_F16_MAPS /
 * PNP_OPT_F16_MIRRORS.  Bit s of src_f16_mask: srcs_dev[s] IS an fp16 NHWC64 map (else fp32); out_f16: out_dev is an fp16 map
 * (single source, no residual); out16_dev (optional, only with an fp32 out_dev): an fp16 copy of the output written in the same
 * pass; par_flags_dev: pnp_par_tile_flags_f32 output or NULL.  Several 64-channel sources run as ONE launch when all of them are
 * fp16 maps (chain = 0), or -- fp32 sources only -- as the chain of single-source launches through fp32 partial sums (chain = 1;
 * bit-identical). */
int pnp_conv3x3_f16_maps(int nsrc, const void* const* srcs_dev, const int* src_channels, int src_f16_mask,
                         const void* const* packed_w_f16_dev, const float* bias_dev, const float* gamma_dev,
                         const void* packed_w1x1_f16_dev, const float* par_dev, const int* par_flags_dev,
                         const float* residual_dev, int act, void* out_dev, int out_f16, void* out16_dev, int h, int w,
                         int chain, void* trace_dev, void* stream);

/* pnp_conv3x3_f16x3 with the in-kernel timeline: trace_dev = 8 u64 per persistent block (512 at most): s_memtime at kernel
 * start; cycles spent waiting for / splitting the halo into the A tiles; cycles in the K loops; s_memtime at the end; cycles in the
 * epilogues; tiles done; block lifetime in 100 MHz s_memrealtime ticks; HW_REG_LDS_ALLOC (low byte 0: the first block on its CU). */
int pnp_conv3x3_f16x3_ex(int nsrc, const float* const* srcs_dev, const int* src_channels,
                         const float* const* packed_w_f32_dev, const void* const* packed_w_x3_dev, const float* bias_dev,
                         const float* gamma_dev, const void* packed_w1x1_x3_dev, const float* par_dev,
                         const int* par_flags_dev, const float* residual_dev, int act, float* out_dev, int h, int w,
                         int w1x1_scaled, int* tile_queue_dev, void* trace_dev, void* stream);
/* tile_queue_dev: NULL (every block walks a static share of the tiles) or 16 ints, zero on entry and zero again when the launch
 * has finished: the blocks draw their tiles per XCD from it, as pnp_generator_forward's launches do from its workspace
 * (PNP_OPT_TILE_QUEUE).
 * w1x1_scaled != 0: packed_w1x1_x3_dev holds 12 split chunks -- the three branch images and then the same three scaled by 1/255
 * (what pnp_generator_pack lays out) -- and tiles whose partition values are all 0 or exactly 1/255 (par_flags bits 3..5) contract
 * the branches with the scaled images and a masked A operand instead of re-splitting par_j(pixel) * x.  trace_dev may be NULL. */

/* pnp_mv_warp_nhwc_f32 writing its result as an fp16 (h,w,c) map (saturating round-to-nearest-even of the fp32 value). */
int pnp_mv_warp_nhwc_f16out(const float* feat_dev, const float* flow_x_dev, const float* flow_y_dev, void* out16_dev, int h,
                            int w, int c, void* stream);
/* ... with pnp_mv_warp_nhwc_mode_f32's `mode` (0 'bilinear', 1 'nearest'): the fp16-output instantiations of both modes. */
int pnp_mv_warp_nhwc_f16out_mode(const float* feat_dev, const float* flow_x_dev, const float* flow_y_dev, void* out16_dev, int h,
                                 int w, int c, int mode, void* stream);

/* ---- The reconstruction head's two conv forms alone (iconvsr_ipb_par.py:135-146), each with an explicit kernel route, so that a test
 * knows which kernel it ran.  Arguments only, no process-wide state; the launch is the one the clip scheduler makes for the head.  A
 * route that the project's own eligibility rule does not select for exactly these arguments is PNP_ERR_UNSUPPORTED: nothing is rerouted.
 * NULL pointers, act outside 0..2, h or w below 1 and unknown routes / modes / forms are PNP_ERR_BAD_ARG, a map beyond 32-bit byte
 * offsets is PNP_ERR_UNSUPPORTED, all before any launch. */
#define PNP_HEAD_AUTO 0    /* what the clip scheduler launches at the given precision */
#define PNP_HEAD_F32 1     /* the fp32 matrix-core tile kernel (pixel shuffle: 4x16 or 8x16 tiles by frame size; conv_last: the RGB configuration) */
#define PNP_HEAD_F16 2     /* the fp16-operand kernel (pixel shuffle: any mix of fp32 / fp16 maps; conv_last: its RGB body) */
#define PNP_HEAD_F16X3 3   /* pixel shuffle only: the split-fp16 kernel, four launches */
#define PNP_HEAD_VALU 4    /* conv_last only: the vector-ALU kernel, with or without a byte / RGB0 boundary */

/* PixelShufflePack (common/upsample.py:40-51): x_dev (h,w,64) fp32, or fp16 when x_f16 -> out_dev (2h,2w,64) fp32, or fp16 when
 * out_f16.  packed_dev: the image of pnp_pack_pixel_shuffle_f32.  twin_dev / twin_kind: that image's first 36 chunks as
 * pnp_f16_image_from_f32 makes them (kind 1) or as pnp_f16x3_image_from_f32 does (kind 2), or NULL / 0; the kind is the precision
 * PNP_HEAD_AUTO routes for.
 * tile_queue_dev (kind 2 only): NULL or the 16 ints of pnp_conv3x3_f16x3_ex. */
int pnp_debug_pixel_shuffle_conv(const void* x_dev, int x_f16, const float* packed_dev, const void* twin_dev, int twin_kind, int act,
                                 void* out_dev, int out_f16, int h, int w, int route, int* tile_queue_dev, void* stream);

/* conv_last's weights as pnp_generator_pack lays them out, from conv_last.weight (3,64,3,3) and conv_last.bias (3): the matrix-core
 * image (9 chunks of one 32-channel N tile, 3 channels valid), the bias padded to 32 floats, the [9][64][4] vector-ALU layout and the
 * fp16 twin of the image, in that order; the second function is the size of dst_dev in floats. */
int pnp_debug_pack_conv_last(const float* w_dev, const float* b_dev, float* dst_dev, void* stream);
int64_t pnp_debug_conv_last_packed_floats(void);

#define PNP_HEAD_FRAME_PLANES 0   /* the frame to add as 3 fp32 planes */
#define PNP_HEAD_FRAME_U8 1       /* as (h,w,3) bytes, read through the table of pnp_frames_from_rgb8 */
#define PNP_HEAD_FRAME_RGB0 2     /* as (h,w,4) fp32 RGB0, what a 4:2:0 clip is unpacked into */

/* out = act(conv_last(src)) + frame (out_mode 2; the frame is H x W) or + bilinear x4 of the frame (out_mode 3; the frame is
 * H/4 x W/4, H and W multiples of 4).  src_dev (H,W,64) fp32, or fp16 when src_f16.  packed_dev: pnp_debug_pack_conv_last's buffer.
 * prec: the PNP_PREC_* that PNP_HEAD_AUTO routes for (ignored by the explicit routes).  out_dev: 3 fp32 planes (H,W) and / or
 * out_u8_dev: (H,W,3) bytes, round-half-even of clamp(x, 0, 1) * 255 of the fp32 sum x; either may be NULL, not both.  Byte output
 * and the two frame forms other than planes exist on the vector-ALU kernel only. */
int pnp_debug_conv_last(const void* src_dev, int src_f16, const float* packed_dev, int prec, int act, int out_mode,
                        const void* frame_dev, int frame_form, float* out_dev, unsigned char* out_u8_dev, int H, int W, int route,
                        void* stream);

#ifdef __cplusplus
}
#endif
#endif
