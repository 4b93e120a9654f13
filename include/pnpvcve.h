/* libpnpvcve_hip.so -- C ABI of the MI355X-native PnP-VCVE BAE/CAA forward hot path.
 *
 * The reference (ZeldaM1/PnP-VCVE) is pure Python on PyTorch/mmcv and has no FFI of its own;
 * each entry point below names the reference function it replaces (paths relative to
 * /root/reference).  All pointers named *_dev are device (HBM) addresses owned by the
 * caller; the library allocates no device memory, launches asynchronously on the supplied
 * stream (a hipStream_t passed as void*) and returns 0 on success, a hipError_t value, or
 * one of the PNP_ERR_* codes.  fp32 throughout unless PNP_PREC_F16 is selected.
 * State: all mutable state lives in the pnp_generator handle (precision, options, profiling events, side streams);
 * a handle must not be used from two threads at once.  The only process-wide state is a per-DEVICE cache of one-time
 * kernel attributes (dynamic-LDS opt-in, CU count), keyed by the current device and mutex-protected, so one process may
 * drive several GPUs.  No environment variables are read.
 */
#ifndef PNPVCVE_H
#define PNPVCVE_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define PNP_ERR_BAD_ARG 1001
#define PNP_ERR_UNSUPPORTED 1002
#define PNP_ERR_WORKSPACE 1003
#define PNP_ERR_SIZE_ASSERT 1004 /* reference: AssertionError, h/w < 64 (iconvsr_ipb_par.py:51) */
#define PNP_ERR_SIZE_VALUE 1005  /* reference: ValueError from flow_warp.py:27-29 (h/w % 4 != 0) */
/* any_size (this is the ONE statement of the rule).  0 (default): a frame whose height or width is no multiple of 4 is refused with
 * PNP_ERR_SIZE_VALUE, as the reference refuses it (its spatial_padding pads lrs alone, iconvsr.py:371-394, and flow_warp.py:27-29 then
 * raises).  1: such frames run -- the same formulas on the h x w grid as given, no padding and no crop: every conv zero-pads at the
 * true frame edge, warps and partition planes are indexed on h x w, the output is (n,t,3,h,w) or (n,t,3,4h,4w) with cfg.vsr.  For h and
 * w multiples of 4 the forward is the one of any_size = 0, launch for launch.  h, w >= 64 (PNP_ERR_SIZE_ASSERT) holds in both modes.
 * With the switch on a byte clip (PNP_FRAMES_U8_HWC / PNP_OUT_U8) may start at any byte address -- clip b of a (n,t,h,w,3) batch
 * does when t*h*w*3 is no multiple of 4 -- and cfg.deform = 'basic' | 'fvc' is refused with PNP_ERR_UNSUPPORTED at every size (the
 * DCN aligners have not run on such frames).  Honoured by pnp_generator_forward, pnp_generator_forward_clips and the two workspace
 * queries (which size any h x w; the refusals are the forward's).  The reference has no output at these sizes: the mode is pinned
 * to the oracle's blocks (tests/any_size_ref.py).  Negative `on`: PNP_ERR_BAD_ARG; get: 0 / 1, -1 for NULL. */
typedef struct pnp_generator pnp_generator; /* (pnp_generator_create below) */
int pnp_generator_set_any_size(pnp_generator* g, int on);
int pnp_generator_get_any_size(const pnp_generator* g);

int pnp_abi_version(void); /* 5: PNP_OPT_WINOGRAD, pnp_wino_* / pnp_conv3x3_wino_f32.  4: pnp_generator_cfg grew num_group / flow_inter / blocktype (3: the never-implemented fused-block option / query of v2
                              removed, PNP_OPT_* renumbered, PNP_OPT_SPARSE_EVAL, PNP_OPT_F16_MIRRORS) */

/* ------------------------------------------------------------------ generator (a1/a2)
 * Constructor kwargs of IconVSR_restore_wo_refill_mv_ipb_fast_domain_dynamic_with_par
 * (mmedit/models/backbones/sr_backbones/iconvsr_ipb_par.py:18-41 and parents
 *  iconvsr_ipb.py:16-31, iconvsr.py:346-369).  Booleans are 0/1. */
typedef struct pnp_generator_cfg {
    int mid_channels; /* only 64 */
    int num_blocks;
    int num_experts;
    int with_cat, use_base_qp, expert_softmax, with_bias, with_se;
    int one_layer, channel_first, align_key, vsr;
    int deform; /* 0 'vos' (MV bilinear warp, iconvsr_mv.py:12-18); 1 'basic' (:52-84), 2 'fvc' (:21-41):
                   flow-guided modulated deformable conv, deform_groups 16 (mmcv semantics restated) */
    int sparse_val; /* eval-time sparse evaluation of the 1x1 partition branches (basicvsr_net.py:456-476,511-514,
                       sr_backbone_utils.py:262-302): branch j where plane j != 0, later planes overwrite, result / 255.
                       Identical to the dense path for one-hot maps in {0, 1/255}; one clip at a time (n == 1): the
                       reference indexes sample 0 only */
    int num_group;  /* groups of every conv of a BAE block (sr_backbone_utils.py:285-289): a divisor of 64 (0 = 1); packed as the dense
                       conv it equals.  Not with sparse_val (the reference's sparse_conv multiplies a (64, 64/groups) weight
                       with 64-channel columns and raises) */
    int flow_inter; /* 0 'bilinear', 1 'nearest' (flow_warp.py:8,47 -> F.grid_sample mode): the MV alignment and the warp inside
                       the 'basic' aligner */
    int blocktype;  /* 0 'drt'; 1 'drt_woqp' (ResidualBlockNoBNDynamic_drt_wo_qp, sr_backbone_utils.py:336-384): both 3x3 convs
                       are plain convs, no expert mix and no gain; needs one_layer = 1 (with Dynamic_conv2d_se convs the
                       reference indexes a tensor with 'x' and raises) */
} pnp_generator_cfg;

int pnp_generator_create(const pnp_generator_cfg* cfg, pnp_generator** out);
void pnp_generator_destroy(pnp_generator* g);

/* Parameter schema = the reference state-dict: name, shape and the
 * float offset of each tensor inside the flat parameter buffer the caller fills. */
int pnp_generator_num_params(const pnp_generator* g);
const char* pnp_generator_param_name(const pnp_generator* g, int i);
int pnp_generator_param_ndim(const pnp_generator* g, int i);
int64_t pnp_generator_param_dim(const pnp_generator* g, int i, int d);
int64_t pnp_generator_param_offset(const pnp_generator* g, int i);
int64_t pnp_generator_flat_floats(const pnp_generator* g);
int64_t pnp_generator_packed_floats(const pnp_generator* g);

/* Arithmetic of the 64-channel convs (BASELINE configs[4]; mmcv's wrap_fp16_model / fp16_enabled switch,
 * mmedit/models/restorers/basic_restorer.py:64 @auto_fp16).  PNP_PREC_F32 (default): exact fp32 MFMA.
 * PNP_PREC_F16: activations and weights rounded to fp16 as MFMA operands, fp32 accumulation, fp32 feature
 * maps in HBM; conv_last and an RGB-only input conv stay fp32.
 * PNP_PREC_F16X3: split fp16 -- every activation and weight of the NHWC64 64-channel convs is carried as
 * hi + lo/2048 (two fp16 numbers, 22 significand bits) and each product is three fp16 MFMAs with fp32
 * accumulation; results agree with PNP_PREC_F32 to ~1e-6 relative per conv (inside north_star's 1e-3 gate,
 * which PNP_PREC_F16 is not) at about a third of the fp16 matrix rate.  Feature maps stay fp32; the RGB
 * frame, the RGB head (conv_last) and the deformable alignment stay on the exact fp32 kernels.  Range: the high
 * parts are fp16, so activations and weights beyond +-65504 saturate (the exact fp32 path has no such limit).
 * Set it BEFORE sizing/packing: it changes pnp_generator_packed_floats and pnp_generator_workspace_bytes. */
#define PNP_PREC_F32 0
#define PNP_PREC_F16 1
#define PNP_PREC_F16X3 2
int pnp_generator_set_precision(pnp_generator* g, int precision);
int pnp_generator_get_precision(const pnp_generator* g);

/* Per-generator execution switches (A/B and diagnostic; results are bit-identical either way unless stated).
 * value 0/1 (PNP_OPT_WINOGRAD: 0/1/2); all default to 1 except PNP_OPT_F16_CHAIN_MIRRORS.  State lives in the handle. */
#define PNP_OPT_F16_MAPS 0       /* PNP_PREC_F16: the map between the two halves of a BAE block / behind conv_hr is stored fp16 */
#define PNP_OPT_PAR_SKIP 1       /* skip 1x1 partition branches whose plane is all zero on a tile (exact zeros); on frames whose every 8x8
                                    quadrant is zero or one constant plane on its pixels inside the image (any frame size) also launch the
                                    front halves in a cheaper form behind a device-side gate on the frame's partition word (bit-identical
                                    results) */
#define PNP_OPT_CONV_LAST_VALU 2 /* conv_last on the vector ALUs (<= 2e-6 from the MFMA kernel: other summation order) */
#define PNP_OPT_PERSIST 3        /* persistent strip kernel for the 64->64 convs on frames with >= 1024 tiles */
#define PNP_OPT_SMALL_F16 4      /* PNP_PREC_F16: tile-per-block fp16 kernel for the 64->64 convs on frames with < 1024 tiles */
#define PNP_OPT_SPARSE_EVAL 5    /* cfg.sparse_val only: 1 = eval mode (sparse semantics), 0 = training mode -- the reference takes the
                                    sparse branch only when `self.sparse_val and not self.training` (sr_backbone_utils.py:308,322,
                                    basicvsr_net.py:511) and the dense par * conv1x1 formula otherwise (NOT bit-identical: the two
                                    differ on non-one-hot maps) */
#define PNP_OPT_F16_MIRRORS 6    /* PNP_PREC_F16 (with PNP_OPT_F16_MAPS, deform 'vos'): every 64-channel map that is only read as an MFMA A
                                    operand (the running map of a branch, the frame slots, the MV-aligned key frame) gets an fp16 copy
                                    from its producer, and the input conv of a branch runs as ONE launch over those copies instead of
                                    a chain of single-source launches through fp32 partial sums.  Bit-identical: same rounding points */
#define PNP_OPT_F16_CHAIN_MIRRORS 7 /* with PNP_OPT_F16_MIRRORS: also mirror the running map x inside a branch (default 0: measured
                                    neutral at 720p -- the back half writes 128 B per pixel more for what the front half reads less) */
#define PNP_OPT_TILE_QUEUE 8     /* PNP_PREC_F16X3: the split conv kernel's blocks draw their tiles from a per-XCD queue in the workspace instead of
                                    walking a static share (tiles differ in cost and the two blocks of a CU in speed); results identical */
#define PNP_OPT_WINOGRAD 9       /* PNP_PREC_F32: the single-source 64 -> 64 convs (both halves of a BAE block, conv_hr) and the input convs over wide sources in
                                    Winograd F(2x2,3x3) form (conv_wino.hip): 2.25x fewer matrix FLOPs, still fp32 products and sums, NOT bit-identical
                                    to the direct kernels (summation order + the +-1 input transform: ~1e-6 per conv on unit-scale maps; whole-clip
                                    gates in tests/test_gpu_wino.py).  0 off | 1 (default): frames of up to PNP_WINO_UNITS_MAX_TILES 16x16 tiles
                                    one block per 8x8 quadrant unit, larger ones the persistent tile kernels (same values bit for bit) |
                                    2: the tile kernels at every frame size.  This is the ONE statement of the rule */
#define PNP_WINO_UNITS_MAX_TILES 128   /* ceil(h/16) * ceil(w/16) up to which PNP_OPT_WINOGRAD = 1 takes the quadrant-unit kernels */
#define PNP_OPT_COUNT 10
int pnp_generator_set_option(pnp_generator* g, int option, int value);
int pnp_generator_get_option(const pnp_generator* g, int option);

/* flat (reference layouts) -> packed (MFMA B images); replaces nothing in the reference,
 * it is the checkpoint-load-time half of mmcv load_checkpoint (iconvsr.py:510-523). */
int pnp_generator_pack(const pnp_generator* g, const float* flat_dev, float* packed_dev, void* stream);

/* Bytes of ONE workspace context (one clip in flight).  pnp_generator_forward accepts a workspace of k such
 * contexts (k <= PNP_MAX_CONTEXTS) and then runs up to k samples of the batch concurrently on internal streams
 * forked from / joined to the caller's stream -- worth it for small frames, which cannot fill 256 CUs alone. */
#define PNP_MAX_CONTEXTS 8
int64_t pnp_generator_workspace_bytes(const pnp_generator* g, int t, int h, int w);

/* Bounded-memory forward for long clips.  k bounds the 64-channel frame feature maps the two recurrent sweeps hold across branch
 * runs (the per-frame slots of the workspace and their fp16 mirrors; per-launch scratch does not count).  0 (default) = unbounded:
 * one map per frame, the schedule of earlier versions launch for launch; k >= t gives that schedule too.  0 < k < t: the backward
 * sweep runs once as a checkpoint pass and the forward sweep recomputes each segment of backward features from its checkpoint
 * just before it reads them -- the same kernels on the same values, so the output is bit-identical to the unbounded schedule.
 * The workspace then holds k maps instead of t (the 16 B/pixel/frame RGB0 frames and the per-frame regions that do not scale with
 * h*w stay per frame: DESIGN.md section 4).  The profiling counters count what runs, recomputed branch runs included.
 * Set k BEFORE sizing: pnp_generator_workspace_bytes follows it and returns -1 when 0 < k < pnp_generator_min_resident(g, t),
 * where pnp_generator_forward returns PNP_ERR_BAD_ARG.  pnp_generator_min_resident: the smallest k the scheme accepts for t
 * frames with this configuration (about 2 * sqrt(2t); fewer without with_cat), -1 for t < 1.  Negative k: PNP_ERR_BAD_ARG. */
int pnp_generator_set_max_resident(pnp_generator* g, int k);
int pnp_generator_get_max_resident(const pnp_generator* g);
int pnp_generator_min_resident(const pnp_generator* g, int t);

/* Row-band chains.  A branch is a chain of 3x3 convs, each reading the previous one's whole output, and every
 * launch of the persistent tile kernels ends with a partial round and a drain during which most of the chip idles.  With the switch
 * on, a chain runs as two: chain A on the caller's stream computes tile rows [0, a_n) of conv n, chain B on an internal stream rows
 * [a_n, rows), with a_n = a_0 - n -- a region that shrinks by one tile row per conv never reads outside what its own chain wrote, and
 * B's conv n waits (an event) only for A's conv n - 1.  The device then always holds a ready kernel that does not depend on the one
 * whose tail is running.  Same kernels, same arithmetic per tile: the output is bit-identical to the one-launch schedule.
 * This is the ONE statement of the rule: 0 = one launch per conv; 1 (default) = band chains where ALL of these hold -- PNP_PREC_F32,
 * the Winograd tile kernels (PNP_OPT_WINOGRAD, a frame above PNP_WINO_UNITS_MAX_TILES tiles), one workspace context in flight
 * (several clips on several streams fill each other's tails already), and enough tile rows that both regions stay non-empty
 * over the whole chain (rows >= convs of the chain + 1: 720p and up); k >= 2 = as 1 with the first boundary a_0 = k instead of the
 * centred (rows + convs - 1) / 2 (a tuning aid; a chain it leaves a region empty in takes one launch per conv).  Negative:
 * PNP_ERR_BAD_ARG.  Stays on under pnp_generator_profile: a split conv counts as one launch, timed on the caller's stream
 * (back to back with its neighbours: the chain's time per conv; the part on the internal stream overlaps the next conv and is not
 * added, so a kind's total stays within wall time). */
int pnp_generator_set_band_split(pnp_generator* g, int on);
int pnp_generator_get_band_split(const pnp_generator* g);

/* generator.forward(lrs, QPs, slices, mvs, base_QPs, par_map)  iconvsr_ipb_par.py:44-149.
 *   lrs_dev (n,t,3,h,w)  mvs_dev (n,t,4,h,w)  par_dev (n,t,3,h,w)      NCHW, contiguous
 *   slices/qps/base_qps: HOST arrays of n*t floats (the (n,t,1,1,1) tensors, flattened);
 *   the reference reads the same values host-side (int(torch.where(...)), :81,:116).
 *   out_dev (n,t,3,h,w), or (n,t,3,4h,4w) when cfg.vsr. */
int pnp_generator_forward(const pnp_generator* g, const float* flat_dev, const float* packed_dev,
                          const float* lrs_dev, const float* mvs_dev, const float* par_dev,
                          const float* slices_host, const float* qps_host, const float* base_qps_host,
                          float* out_dev, void* workspace_dev, int64_t workspace_bytes,
                          int n, int t, int h, int w, void* stream);

/* Byte frames and clips by pointer.  The same forward at the boundary a video pipeline has: the frames as the
 * decoder's bytes, the output as display bytes, a batch as a HOST array of n clip descriptors (the clips live wherever they live:
 * nothing is concatenated).  One lq_format and one out_mask per call.
 *   PNP_FRAMES_U8_HWC: lq_dev (t,h,w,3) uint8 RGB; byte v stands for the fp32 value (float)v / 255.0f (IEEE division, one 256-entry
 *   table), so the result is bit-identical to the fp32 forward on pnp_frames_from_rgb8 of the same bytes.
 *   PNP_OUT_U8: out_u8_dev (t,H,W,3) = round_half_even(clamp(x,0,1) * 255) of the very fp32 value PNP_OUT_F32 stores, the arithmetic
 *   of pnp_frames_to_rgb8; both bits: both buffers are written.  (H, W = h, w, or 4h, 4w with cfg.vsr.)
 * No fp32 copy of a byte clip is made: the frames are unpacked straight into the conv source, and conv_last's vector-ALU kernel reads
 * and writes the bytes itself; the kernels that keep an fp32 interface (PNP_PREC_F16, PNP_OPT_CONV_LAST_VALU = 0) go through ONE
 * frame of fp32 planes in the workspace.  mvs_dev / par_dev as in pnp_generator_forward; slices / qps / base_qps: n*t host floats.
 * Errors: those of pnp_generator_forward, and PNP_ERR_BAD_ARG for an unknown format, an out_mask of 0 or with bits beyond 3, a NULL
 * pointer the format or mask requires, or a uint8 pointer that is not 4-byte aligned.  pnp_generator_forward is this call with
 * descriptors made from its strides, PNP_FRAMES_F32_NCHW and PNP_OUT_F32: the same launches.
 * pnp_generator_workspace_bytes_io: bytes of one context for that boundary (-1: unknown format / mask, or a bound below the minimum);
 * with PNP_FRAMES_F32_NCHW and PNP_OUT_F32 it equals pnp_generator_workspace_bytes, otherwise it adds at most the one-frame buffers. */
#define PNP_FRAMES_F32_NCHW 0 /* (t,3,h,w) fp32 */
#define PNP_FRAMES_U8_HWC 1   /* (t,h,w,3) uint8 RGB */
#define PNP_OUT_F32 1
#define PNP_OUT_U8 2
typedef struct pnp_clip_io {
    const void* lq_dev;
    const float* mvs_dev;
    const float* par_dev;
    float* out_f32_dev;        /* may be NULL when PNP_OUT_F32 is not in out_mask */
    unsigned char* out_u8_dev; /* may be NULL when PNP_OUT_U8 is not in out_mask */
} pnp_clip_io;
int pnp_generator_forward_clips(const pnp_generator* g, const float* flat_dev, const float* packed_dev,
                                const pnp_clip_io* clips_host, int n, int lq_format, int out_mask,
                                const float* slices_host, const float* qps_host, const float* base_qps_host,
                                void* workspace_dev, int64_t workspace_bytes, int t, int h, int w, void* stream);
int64_t pnp_generator_workspace_bytes_io(const pnp_generator* g, int t, int h, int w, int lq_format, int out_mask);

/* Y'CbCr 4:2:0 boundary: the same forward on the planes a decoder writes (NV12 / NV21 / I420, 8 bit) and, on
 * request, writing planes an encoder or a display takes -- 1.5 B per pixel and frame each way, no RGB bytes and no fp32 copy of a clip
 * in between, ONE rounding (on the way out).  The reference has no such path (its loaders read PNGs): the mode is pinned to the
 * arithmetic below, which tests/yuv_ref.py restates in numpy.  This is the ONE statement of it.
 *   Standards: Kr, Kb = 0.299, 0.114 (BT.601) | 0.2126, 0.0722 (BT.709), Kg = 1 - Kr - Kb; limited range sy = 219, sc = 224,
 *   yoff = 16; full range sy = sc = 255, yoff = 0.  Every constant named below is evaluated in double from Kr and Kb and rounded to
 *   fp32 ONCE; every product and sum after that is an fp32 operation rounded on its own (no fused multiply-add).
 *   Bytes -> RGB (fp32, not rounded to 8 bits): y = cy * float(Y - yoff), u = float(Cb - 128), v = float(Cr - 128) with cy = 1 / sy,
 *   crv = 2 (1 - Kr) / sc, cbu = 2 (1 - Kb) / sc, cgu = 2 Kb (1 - Kb) / (Kg sc), cgv = 2 Kr (1 - Kr) / (Kg sc);
 *       R = y + crv * v,   G = (y - cgu * u) - cgv * v,   B = y + cbu * u,   each then min(max(x, 0), 1).
 *   Chroma is REPLICATED: pixel (yy, xx) reads the chroma sample (yy >> 1, xx >> 1).
 *   RGB -> bytes: r, g, b clamped to [0, 1]; yl = (Kr * r + Kg * g) + Kb * b; Y = clamp(rint(float(yoff) + sy * yl), 0, 255), rint
 *   rounding half to even; per pixel pb = (b - yl) * (0.5 / (1 - Kb)), pr = (r - yl) * (0.5 / (1 - Kr)); the chroma sample of a 2x2
 *   block is the BOX MEAN ((p00 + p01) + (p10 + p11)) * 0.25 (rows top then bottom, columns left then right) and
 *   Cb = clamp(rint(128 + sc * mean_pb), 0, 255), Cr likewise.  Box-down and replicate-up are consistent (centre siting) and are the
 *   DEFAULT chroma mode; the other modes are stated below, and so are the 4:2:2 and 4:4:4 chroma formats (10 and 12 bit:
 *   pnp_yuv420_planes16 below).  Limited-range white (235,128,128) gives 0.99999994, not 1.
 * Chroma modes (siting and filters; opt-in, at every depth; tests/yuv_chroma_ref.py restates them in numpy).  This is the ONE statement
 * of them; like the rest of this boundary, and like MS-SSIM's and XPSNR's arithmetic below, the definition is the project's own: no
 * external tool's digits are pinned.  Every entry that takes yuv_standard takes PNP_YUV_CODE(standard, chroma): the standard 0..3 in
 * bits 0..7, the mode in bits 8..11, so a bare standard is mode 0 and what it always was.  A mode selects BOTH directions:
 *     mode                          chroma sample (j, i) lies at luma (row, column)   planes -> RGB   RGB -> planes
 *     0 PNP_YUV_CHROMA_REPLICATE    (2j + 1/2, 2i + 1/2)                              replication     box mean       (the default, above)
 *     1 PNP_YUV_CHROMA_CENTER       (2j + 1/2, 2i + 1/2)                              bilinear        box mean
 *     2 PNP_YUV_CHROMA_LEFT         (2j + 1/2, 2i)     H.264 / HEVC / VVC type 0      bilinear        [1 2 1] / 4 across, box down
 *     3 PNP_YUV_CHROMA_TOPLEFT      (2j,       2i)     BT.2020 / UHD type 2           bilinear        [1 2 1] / 4 both ways
 *   An axis is CO-SITED where chroma lies on the even luma indices (x for LEFT; x and y for TOPLEFT) and MIDWAY otherwise.
 *   Planes -> RGB, modes 1..3: per axis, luma index k with i = k >> 1 takes two chroma indices with weights in quarters, n the chroma
 *   plane's extent on that axis:
 *       co-sited axis:  even k: (i: 4)                        odd k: (i: 2, min(i + 1, n - 1): 2)
 *       midway axis:    even k: (i: 3, max(i - 1, 0): 1)      odd k: (i: 3, min(i + 1, n - 1): 1)
 *   Indices clamp; nothing outside the plane is read.  The interpolated chroma is an exact integer, u16 = sum of wy * wx * (Cb[a][b] -
 *   mid) over the two rows a and the two columns b (the weights sum to 16; mid = 128, or 2^(d-1)), and u = float(u16) * 0.0625f, v
 *   likewise from Cr.  |u16| < 2^16 at 12 bit, so the fp32 value is exact and there is no summation order to pin.  From u, v on, the
 *   formulas, constants, clamp and the rule of no contraction are the ones above, word for word; Y is untouched.  The limited-range
 *   identity of the 16-bit statement carries over: u16 scales by s exactly.
 *   RGB -> planes, modes 2 and 3: pb, pr per pixel are the ones above; every operation below is one fp32 operation rounded on its own.
 *   On a co-sited axis the sample at 2i takes the taps L = max(2i - 1, 0), C = 2i, R = 2i + 1 as ((pL + pR) + (pC + pC)) * 0.25; on a
 *   midway axis it takes (p0 + p1) * 0.5 of 2i and 2i + 1.  LEFT: each of the rows 2j and 2j + 1 is filtered across first, then the two
 *   are combined.  TOPLEFT: the rows max(2j - 1, 0), 2j, 2j + 1 are filtered across, then combined with the three-tap form.  Modes 0
 *   and 1 keep the box mean's expression.  Rounding and clamping to samples are unchanged; so is Y.
 *   A chroma ramp C[i] = a + b i therefore upsamples to a + b (x - off) / 2 exactly away from the clamped edges, off = 0 on a
 *   co-sited axis and 1/2 on a midway one.  A mode above 3 and a low byte above 3 are PNP_ERR_BAD_ARG.
 * Chroma formats (4:2:2 and 4:4:4; at every depth, in every container and chroma mode; tests/yuv_formats_ref.py restates them in
 * numpy).  This is the ONE statement of them; the definition is the project's own and no external tool's digits are pinned.  A chroma
 * format is a pair of subsampling factors (sx, sy): PNP_YUV_FORMAT_420 (2, 2), what is stated above; PNP_YUV_FORMAT_422 (2, 1);
 * PNP_YUV_FORMAT_444 (1, 1).  The chroma planes are (h / sy) x (w / sx); sx must divide w and sy must divide h, so 4:2:2 needs an even
 * w only and 4:4:4 puts no parity condition on h or w.  The format rides in bits 12..13 of the integer every entry takes as
 * yuv_standard, PNP_YUV_CODE3(standard, chroma, format): a code with format 0 is every code there was and does what it did; format
 * value 3 and any bit from 14 up are PNP_ERR_BAD_ARG.  The entries, descriptors and PNP_OUT_YUV420 keep their names: the `420` in
 * them is historical, and every one of them (the forwards, pnp_frames_from_yuv420 / _to_yuv420 and their p16 forms, the debug pack)
 * takes every format on the same descriptors, with c_pitch >= c_step * w / sx samples.  A clip's output planes have the input's
 * format: one code serves both directions.  Standards, depths, containers, constants, rounding and the rule of no contraction are
 * those of the 4:2:0 statement, word for word; only the chroma geometry changes:
 *   Planes -> RGB.  PNP_YUV_CHROMA_REPLICATE: pixel (yy, xx) reads chroma sample (yy / sy, xx / sx).  The other modes: the per-axis
 *   tap table above applies on every axis whose factor is 2; on an axis whose factor is 1, luma index k takes chroma index k with
 *   weight 4.  The weights still sum to 16; u16, u = float(u16) * 0.0625f and everything after are the expressions above.  So in 4:2:2
 *   LEFT and TOPLEFT are the same function, in 4:4:4 all four modes are the same function, and no mode is refused for any format.
 *   RGB -> planes.  Y, pb and pr per pixel are as above.  On an axis with factor 2 the mode's filter of the 4:2:0 statement applies
 *   on that axis (midway: (p0 + p1) * 0.5; co-sited: ((pL + pR) + (pC + pC)) * 0.25 with the clamped left tap); on an axis with factor
 *   1 the sample is the pixel's own value, with no operation.  Modes 0 and 1 at 4:2:2 are therefore (p0 + p1) * 0.5 across, and at
 *   4:4:4 every mode rounds pb and pr of the pixel itself.  Each operation is one fp32 operation rounded on its own.
 *   The reading and writing rule below carries over with the chroma planes' true rows and columns.
 *   BT.2020 constants, a conversion between the input's and the output's format, packed formats (YUY2, v210, AYUV) and MS-SSIM,
 *   XPSNR and PSNR-B on 4:2:2 or 4:4:4 planes are not offered.
 * A plane pointer may sit at ANY byte address and a pitch may be any value that holds a row, odd ones too.  No byte outside
 * [plane, plane + rows * pitch) of a plane is read or written, and inside it the bytes of a row beyond the frame's width are never
 * written.  Planes and pitches that are 4-byte aligned take a faster form of the unpacking (same values).
 * pnp_generator_forward_clips_yuv: pnp_generator_forward_clips with the frames as planes; out_mask is any non-empty set of
 * PNP_OUT_F32 | PNP_OUT_U8 | PNP_OUT_YUV420, each output the one its own call would write: the result is bit-identical to the fp32
 * forward on pnp_frames_from_yuv420 of the planes, and the PNP_OUT_YUV420 bytes are pnp_frames_to_yuv420 of the fp32 output.
 * Errors, decided on the host before any HIP call: PNP_ERR_BAD_ARG for an unknown standard, a mask of 0 or beyond 7, a NULL plane or
 * output the mask needs, c_step not 1 or 2, a pitch below the row's bytes, or odd h or w (4:2:2: odd w; 4:4:4: neither); then the
 * forward's own, in their order (with pnp_generator_set_any_size every even h, w >= 64 runs; 4:2:2: every h >= 64 with an even
 * w >= 64; 4:4:4: every h, w >= 64).
 * pnp_generator_workspace_bytes_yuv: bytes of one context (-1: mask, or a bound below the minimum): pnp_generator_workspace_bytes
 * plus ONE frame of fp32 planes (12 h w bytes, 256-aligned) in front of a last conv that keeps its fp32 interface (PNP_PREC_F16,
 * PNP_OPT_CONV_LAST_VALU = 0), plus ONE output frame of fp32 planes (12 H W) where bytes or planes are made of an fp32 frame the
 * caller did not ask for (PNP_OUT_YUV420 without PNP_OUT_F32; PNP_OUT_U8 without it on such a last conv). */
#define PNP_YUV_BT601_LIMITED 0
#define PNP_YUV_BT601_FULL 1
#define PNP_YUV_BT709_LIMITED 2
#define PNP_YUV_BT709_FULL 3
#define PNP_YUV_CHROMA_REPLICATE 0
#define PNP_YUV_CHROMA_CENTER 1
#define PNP_YUV_CHROMA_LEFT 2
#define PNP_YUV_CHROMA_TOPLEFT 3
#define PNP_YUV_CODE(standard, chroma) ((standard) | ((chroma) << 8))
#define PNP_YUV_FORMAT_420 0
#define PNP_YUV_FORMAT_422 1
#define PNP_YUV_FORMAT_444 2
#define PNP_YUV_CODE3(standard, chroma, format) ((standard) | ((chroma) << 8) | ((format) << 12))
#define PNP_OUT_YUV420 4
typedef struct pnp_yuv420_planes {      /* t frames of h x w, 8 bit, 4:2:0 */
    unsigned char *y, *cb, *cr;         /* first frame's planes; NV12: cr == cb + 1, c_step 2; NV21: cb == cr + 1; I420: c_step 1 */
    int64_t y_pitch, c_pitch;           /* bytes between rows (>= w, >= c_step * w/2); any value, odd ones too */
    int64_t y_frame, c_frame;           /* bytes between frames of the Y plane / of the chroma planes */
    int c_step;                         /* 1 | 2: bytes between chroma samples of a row */
} pnp_yuv420_planes;
typedef struct pnp_clip_yuv {
    pnp_yuv420_planes lq;               /* read only */
    const float *mvs_dev, *par_dev;     /* as in pnp_clip_io */
    float* out_f32_dev;                 /* PNP_OUT_F32 */
    unsigned char* out_u8_dev;          /* PNP_OUT_U8 */
    pnp_yuv420_planes out_yuv;          /* PNP_OUT_YUV420: H x W = h x w, or 4h x 4w with cfg.vsr */
} pnp_clip_yuv;
int pnp_generator_forward_clips_yuv(const pnp_generator* g, const float* flat_dev, const float* packed_dev,
                                    const pnp_clip_yuv* clips_host, int n, int yuv_standard, int out_mask,
                                    const float* slices_host, const float* qps_host, const float* base_qps_host,
                                    void* workspace_dev, int64_t workspace_bytes, int t, int h, int w, void* stream);
int64_t pnp_generator_workspace_bytes_yuv(const pnp_generator* g, int t, int h, int w, int out_mask);
/* The two conversions alone, n frames: in_host_desc / out_host_desc are HOST structs of device addresses; planes_dev (n,3,h,w) fp32. */
int pnp_frames_from_yuv420(const pnp_yuv420_planes* in_host_desc, int yuv_standard, float* out_planes_dev, int n, int h, int w,
                           void* stream);
int pnp_frames_to_yuv420(const float* planes_dev, const pnp_yuv420_planes* out_host_desc, int yuv_standard, int n, int h, int w,
                         void* stream);

/* Plane metrics of two 4:2:0 clips (plane_metrics.hip): what a codec-enhancement result is scored by -- PSNR / SSIM of the Y, the Cb
 * and the Cr plane, each on its own, read from the 8-bit planes where they lie (1.5 B per pixel and clip; no RGB, no second rounding).
 * The reference has no such path; the statistics are the ones of pnp_psnr_sse_f32 / pnp_ssim_partials_f32 below, per plane.  This is
 * the ONE statement of the arithmetic.
 *   a_host_desc, b_host_desc: HOST structs of device addresses, `frames` frames of h x w each (h, w even), described each on its own
 *   (the generator's NV12 output against an I420 ground truth): any byte address, any pitch that holds a row, any frame stride,
 *   c_step 1 | 2.  The reading rule is the one above: no byte outside [plane, plane + rows * pitch) of a plane is read; aligned
 *   dword loads where the dwords lie inside the plane's rows, byte loads at heads, tails and misaligned rows (the same values).
 *   crop_border (even): the Y plane is cropped by crop_border on every side, the chroma planes by crop_border / 2.
 * PSNR: sse_dev (frames, 3) uint64 = the exact sum of squared byte differences of the cropped Y, Cb and Cr plane of each frame
 *   (integer: order-independent, deterministic).  The host forms PSNR_p = 10 log10(255^2 N_p / SSE_p) with N_Y = (h - 2c)(w - 2c),
 *   N_C = (h/2 - c/2)(w/2 - c/2), c = crop_border; infinite where SSE_p = 0; PSNR_YUV = (6 PSNR_Y + PSNR_Cb + PSNR_Cr) / 8.
 * SSIM: pnp_ssim_partials_f32's window, tiling and summation order on the bytes as they are: the partials of a plane are, bit for
 *   bit, those of pnp_ssim_partials_f32 on the (frames,1,rows,cols) fp32 plane (float)byte / 255.0f with the plane's crop.
 *   pnp_ssim_blocks_yuv420: the blocks of one plane (plane = PNP_PLANE_Y | PNP_PLANE_CB | PNP_PLANE_CR): pnp_ssim_blocks(h, w, crop)
 *   for Y, pnp_ssim_blocks(h/2, w/2, crop/2) for Cb / Cr; 0 when it cannot run.  partials_dev: for each plane of plane_mask in the
 *   order Y, Cb, Cr, [frames][blocks of that plane] doubles, one plane after the other; SSIM_p(frame) = sum of its partials in index
 *   order / ((rows - 2 crop_p - 10)(cols - 2 crop_p - 10)).
 * PNP_ERR_BAD_ARG, decided on the host before any HIP call: a NULL descriptor, plane or output; frames < 1; odd or < 2 h / w; a
 * negative or odd crop_border; 2 crop >= h or w; c_step not 1 or 2; a pitch below the row's bytes; plane_mask 0 or beyond 7; for
 * SSIM a cropped plane of the mask smaller than 11x11. */
#define PNP_PLANE_Y 1
#define PNP_PLANE_CB 2
#define PNP_PLANE_CR 4
int pnp_psnr_sse_yuv420(const pnp_yuv420_planes* a_host_desc, const pnp_yuv420_planes* b_host_desc,
                        unsigned long long* sse_dev, int frames, int h, int w, int crop_border, void* stream);
int pnp_ssim_blocks_yuv420(int h, int w, int crop_border, int plane);
int pnp_ssim_partials_yuv420(const pnp_yuv420_planes* a_host_desc, const pnp_yuv420_planes* b_host_desc, int plane_mask,
                             double* partials_dev, int frames, int h, int w, int crop_border, void* stream);
/* The plane metrics of every chroma format ("Chroma formats" above): these entries take chroma_format = PNP_YUV_FORMAT_*, and the
 * _yuv420 / _yuv420p16 entries are calls of them with PNP_YUV_FORMAT_420, returning what they returned.  Everything above holds with
 * the chroma planes' true geometry: they are (h / sy) x (w / sx) and are cropped by crop_border / sx across and crop_border / sy down
 * (the Y plane by crop_border on every side).  crop_border must be even for 4:2:0 and 4:2:2; for 4:4:4 any value >= 0 is accepted.
 * N_C = (h/sy - 2c/sy)(w/sx - 2c/sx), c = crop_border.  PSNR_YUV keeps the project's 6:1:1 definition (6 PSNR_Y + PSNR_Cb + PSNR_Cr) / 8
 * for every format, 4:4:4 included, where the three planes have equal sizes: it is a score of this project, not a sample-weighted
 * mean.  pnp_ssim_blocks_yuv: pnp_ssim_blocks of the cropped plane; with equal crops on both axes the partials are today's, bit for
 * bit.  PNP_ERR_BAD_ARG (pnp_ssim_blocks_yuv: 0) for a chroma_format outside 0..2, an h or w the format refuses, an odd crop_border at
 * 4:2:0 or 4:2:2, and whatever the entries above refuse.  The p16 entries: as pnp_psnr_sse_yuv420p16 / pnp_ssim_partials_yuv420p16. */
int pnp_psnr_sse_yuv(const pnp_yuv420_planes* a_host_desc, const pnp_yuv420_planes* b_host_desc, unsigned long long* sse_dev, int frames,
                     int h, int w, int crop_border, int chroma_format, void* stream);
int pnp_ssim_blocks_yuv(int h, int w, int crop_border, int plane, int chroma_format);
int pnp_ssim_partials_yuv(const pnp_yuv420_planes* a_host_desc, const pnp_yuv420_planes* b_host_desc, int plane_mask,
                          double* partials_dev, int frames, int h, int w, int crop_border, int chroma_format, void* stream);

/* 10 / 12-bit 4:2:0 boundary (yuv.hip): the same boundary on the planes HEVC Main10 / VVC decoders and reference software write.
 * The reference has no such path; tests/yuv16_ref.py restates the arithmetic below in numpy.  This is the ONE statement of it.
 *   Containers: bit depth d = 10 | 12, a sample in a 16-bit little-endian word; LOW-aligned (yuv420p10le / yuv420p12le: the value in
 *   the low d bits, msb_aligned = 0) or HIGH-aligned (P010 / P012: the value in the high d bits, msb_aligned = 1).  Reading is total
 *   and deterministic: a low-aligned word is taken & (2^d - 1), a high-aligned word >> (16 - d).  Writing sets the bits outside the
 *   value to zero.
 *   Range constants, with s = 2^(d-8): limited range yoff = 16 s, sy = 219 s, sc = 224 s; full range yoff = 0, sy = sc = 2^d - 1; the
 *   chroma midpoint is 2^(d-1) in both (it takes the place of 128).
 *   Kr, Kb, the formulas, the clamp to [0, 1], replicated chroma on the way in and the box mean on the way out (and the other chroma
 *   modes, PNP_YUV_CODE) are those of the 8-bit statement above, word for word, with these constants; rounding is rint, half to even, clamped to [0, 2^d - 1].  Every constant
 *   is evaluated in double and rounded to fp32 ONCE; every later product and sum is an fp32 operation of its own, no contraction.
 *   The limited-range identity: in limited range every constant is the 8-bit one times an exact power of two (cy, crv, ... divided by
 *   s; yoff, sy, sc and the midpoint times s), and float(s Y - 16 s) = s float(Y - 16) exactly.  So planes whose samples are s
 *   times an 8-bit clip's samples convert to the SAME fp32 RGB as that clip, bit for bit (tests/test_yuv16_ref.py and the GPU
 *   suite rest on this: it ties this path to the pinned 8-bit one).  Full range has no such identity: 2^d - 1 is no multiple of 255.
 *   Limited-range white (235 s, 128 s, 128 s) therefore gives 0.99999994 here too.
 * pnp_yuv420_planes16: pointers, pitches and frame strides must be EVEN (pitches and strides are in BYTES, c_step in SAMPLES);
 * beyond that any address and any pitch that holds a row.  The 8-bit rule carries over: no byte outside [plane, plane + rows *
 * pitch) of a plane is read or written, and inside it no byte of a row beyond the frame's width is written.  Planes, pitches and
 * strides that are 8-byte aligned (w a multiple of 4; interleaved chroma: the pair's first plane) take a faster form of the
 * unpacking (same values).
 * pnp_generator_forward_clips_yuv16: pnp_generator_forward_clips_yuv on such planes.  out_mask as there; PNP_OUT_YUV420 selects
 * out_yuv16, whose depth and container may differ from the input's.  The workspace is exactly that of
 * pnp_generator_workspace_bytes_yuv (every staged frame is fp32).  The fp32 output is bit-identical to the fp32 forward on
 * pnp_frames_from_yuv420p16 of the planes, and the planes written are pnp_frames_to_yuv420p16 of the fp32 output.
 * Plane metrics: pnp_psnr_sse_yuv420p16 is pnp_psnr_sse_yuv420 on the sample values (exact uint64; a squared difference reaches
 * 2^24, sums are 64-bit from the start); the host applies the peak (2^d - 1)^2.  pnp_ssim_partials_yuv420p16: the window, tiling,
 * block counts (pnp_ssim_blocks_yuv420 as is) and summation order of pnp_ssim_partials_yuv420 on the sample values as floats, with
 * C1 = (0.01 L)^2, C2 = (0.03 L)^2, L = 2^d - 1.  The two clips are described each on its own (layout, pitch, container), but their
 * bit_depth must agree.
 * Errors, decided on the host before any HIP call: PNP_ERR_BAD_ARG for what the 8-bit entries refuse (standard, mask, NULL plane or
 * output the mask needs, c_step not 1 or 2, odd h or w, frames / crop / plane_mask of the metrics) and for a bit_depth that is not 10
 * or 12, msb_aligned not 0 or 1, an odd pointer, pitch or frame stride, a pitch below 2 w (Y) or 2 c_step w/2 (chroma) bytes, and
 * differing depths in a metric call; then the forward's own, in their order. */
typedef struct pnp_yuv420_planes16 {    /* t frames of h x w, 10 or 12 bit in 16-bit words, 4:2:0 */
    unsigned short *y, *cb, *cr;        /* first frame's planes; P010: cr == cb + 1, c_step 2; yuv420p10le: c_step 1 */
    int64_t y_pitch, c_pitch;           /* BYTES between rows (>= 2 w, >= 2 c_step w/2), even */
    int64_t y_frame, c_frame;           /* BYTES between frames of the Y plane / of the chroma planes, even */
    int c_step;                         /* 1 | 2: SAMPLES between chroma samples of a row */
    int bit_depth;                      /* 10 | 12 */
    int msb_aligned;                    /* 0: value in the low bits; 1: in the high bits (P010 / P012) */
} pnp_yuv420_planes16;
typedef struct pnp_clip_yuv16 {
    pnp_yuv420_planes16 lq;             /* read only */
    const float *mvs_dev, *par_dev;     /* as in pnp_clip_io */
    float* out_f32_dev;                 /* PNP_OUT_F32 */
    unsigned char* out_u8_dev;          /* PNP_OUT_U8 */
    pnp_yuv420_planes16 out_yuv16;      /* PNP_OUT_YUV420: H x W = h x w, or 4h x 4w with cfg.vsr */
} pnp_clip_yuv16;
int pnp_generator_forward_clips_yuv16(const pnp_generator* g, const float* flat_dev, const float* packed_dev,
                                      const pnp_clip_yuv16* clips_host, int n, int yuv_standard, int out_mask,
                                      const float* slices_host, const float* qps_host, const float* base_qps_host,
                                      void* workspace_dev, int64_t workspace_bytes, int t, int h, int w, void* stream);
int pnp_frames_from_yuv420p16(const pnp_yuv420_planes16* in_host_desc, int yuv_standard, float* out_planes_dev, int n, int h, int w,
                              void* stream);
int pnp_frames_to_yuv420p16(const float* planes_dev, const pnp_yuv420_planes16* out_host_desc, int yuv_standard, int n, int h, int w,
                            void* stream);
int pnp_psnr_sse_yuv420p16(const pnp_yuv420_planes16* a_host_desc, const pnp_yuv420_planes16* b_host_desc,
                           unsigned long long* sse_dev, int frames, int h, int w, int crop_border, void* stream);
int pnp_ssim_partials_yuv420p16(const pnp_yuv420_planes16* a_host_desc, const pnp_yuv420_planes16* b_host_desc, int plane_mask,
                                double* partials_dev, int frames, int h, int w, int crop_border, void* stream);
int pnp_psnr_sse_yuvp16(const pnp_yuv420_planes16* a_host_desc, const pnp_yuv420_planes16* b_host_desc, unsigned long long* sse_dev,
                        int frames, int h, int w, int crop_border, int chroma_format, void* stream);
int pnp_ssim_partials_yuvp16(const pnp_yuv420_planes16* a_host_desc, const pnp_yuv420_planes16* b_host_desc, int plane_mask,
                             double* partials_dev, int frames, int h, int w, int crop_border, int chroma_format, void* stream);

/* Optional per-launch timing with HIP events recorded on the caller's stream around every
 * kernel of pnp_generator_forward (measurement aid for bench.py; replaces the reference's
 * wall-clock print, mmedit/models/restorers/basicvsr.py:176-182).  Enable, run forwards,
 * then read per kind: total device ms, launch count and algorithmic work (FLOPs for the
 * conv kinds, bytes for PNP_PROF_WARP).  Reading waits for the recorded events. */
#define PNP_PROF_CONV_BLOCK 0 /* the 64->64 BAE convs (K = 576 or 768) */
#define PNP_PROF_CONV_INPUT 1 /* input convs over the virtual concat */
#define PNP_PROF_CONV_HEAD 2  /* conv_hr is BLOCK-shaped but conv_last / upsample convs land here */
#define PNP_PROF_WARP 3       /* MV-guided bilinear alignment, 520 B per pixel */
#define PNP_PROF_DCN 4        /* modulated deformable alignment (deform = basic|fvc), 2240 B per pixel */
int pnp_generator_profile(pnp_generator* g, int enable);
int pnp_generator_profile_read(pnp_generator* g, int kind, double* total_ms, int64_t* launches, double* work);

/* ------------------------------------------------------------------ single ops
 * flow_warp(x, flow, 'bilinear', 'zeros', align_corners=True)  mmedit/models/common/flow_warp.py:6-50
 *   x (n,c,h,w) NCHW ; flow (n,h,w,2) pixels (dx,dy) ; out (n,c,h,w). */
int pnp_flow_warp_nchw_f32(const float* x_dev, const float* flow_dev, float* out_dev,
                           int n, int c, int h, int w, void* stream);
/* The same gather in the pixel-major layout the fused path uses (VOSAlignment.forward,
 * iconvsr_mv.py:17-18): feat/out (h,w,c) ; flow_x/flow_y (h,w) planes. */
int pnp_mv_warp_nhwc_f32(const float* feat_dev, const float* flow_x_dev, const float* flow_y_dev,
                         float* out_dev, int h, int w, int c, void* stream);
/* Both with flow_warp's `interpolation` argument (flow_warp.py:8,47 -> F.grid_sample mode): mode 0 'bilinear', 1 'nearest' (the
 * pixel at nearbyint of the sampling position, ties to even, 0 outside the image -- ATen's grid_sampler_2d). */
int pnp_flow_warp_nchw_mode_f32(const float* x_dev, const float* flow_dev, float* out_dev, int n, int c, int h, int w, int mode,
                                void* stream);
int pnp_mv_warp_nhwc_mode_f32(const float* feat_dev, const float* flow_x_dev, const float* flow_y_dev, float* out_dev, int h,
                              int w, int c, int mode, void* stream);

int pnp_nchw_to_nhwc_f32(const float* in_dev, float* out_dev, int n, int c, int h, int w, void* stream);
int pnp_nhwc_to_nchw_f32(const float* in_dev, float* out_dev, int n, int c, int h, int w, void* stream);

/* Base_Predictor / SEModule  (domain_aware.py:172-183, 210-222); host QP values in,
 * ew_dev (count, E) and gamma_dev (count, 64) out.  v1/v2 may be NULL (gamma = 1). */
int pnp_caa_predict_f32(const float* q_ew_host, const float* q_gamma_host, int count, int num_experts,
                        int softmax, const float* w1_dev, const float* b1_dev, const float* w2_dev,
                        const float* b2_dev, const float* v1_dev, const float* v2_dev,
                        float* ew_dev, float* gamma_dev, void* stream);

/* Weight packing for pnp_conv3x3_f32: OIHW (cout, cin_total, 3, 3) -> B image of input
 * channels [cbase, cbase+csrc) (csrc = 64 -> 9 chunks, csrc = 3 -> 1 chunk); with
 * num_experts > 1, w is (E, cout, cin_total, 3, 3) and ew_dev (E) mixes the experts first
 * (Dynamic_conv2d_se.forward, sr_backbone_utils.py:198-199).  cout <= 64. */
int64_t pnp_packed_conv_floats(int csrc);
int pnp_pack_conv3x3_f32(const float* w_dev, const float* ew_dev, int num_experts, int cout, int cin_total,
                         int cbase, int csrc, float* dst_dev, void* stream);
/* 1x1 (64,64,1,1) -> 1 chunk */
int pnp_pack_conv1x1_f32(const float* w_dev, float* dst_dev, void* stream);

/* Generic fused 3x3 conv over a virtual concat of up to 4 pixel-major sources
 * (64 channels each, or the 4-channel RGB0 frame):
 *   v = conv3x3(cat(srcs)) ; v = (v + bias) * gamma ; v += sum_j par_j * conv1x1_j(src0)
 *   v = act(v) ; v += residual ; out (h,w,64)
 * This one op covers input_conv+LeakyReLU (basicvsr_net.py:484,515), both halves of
 * ResidualBlockNoBNDynamic_drt.forward (sr_backbone_utils.py:304-333) and conv_hr
 * (iconvsr.py:365).  NULL for unused bias/gamma/par/w1x1/residual.  act: 0 none, 1 relu,
 * 2 leaky-relu(0.1).  par_dev: 3 NCHW planes (3,h,w). */
int pnp_conv3x3_f32(int nsrc, const float* const* srcs_dev, const int* src_channels,
                    const float* const* packed_w_dev, const float* bias_dev, const float* gamma_dev,
                    const float* packed_w1x1_dev, const float* par_dev, const float* residual_dev,
                    int act, float* out_dev, int h, int w, void* stream);

/* One BAE block, ResidualBlockNoBNDynamic_drt.forward in the shipped layout (channel_first, one_layer;
 * sr_backbone_utils.py:305-313,329):  out = x + conv1(relu(gamma * (conv2_mix(x) + b2) + sum_j par_j * conv1x1_j(x))) + b1.
 * w2_packed: the expert-mixed dynamic conv (pnp_pack_conv3x3_f32 with num_experts > 1 = Dynamic_conv2d_se's
 * mm(attention, weight), :198-199); w1_packed: the static conv1; w1x1_packed / par may both be NULL.
 * scratch_dev: h*w*64 floats for the intermediate; out_dev may alias x_dev. */
int pnp_bae_block_f32(const float* x_dev, const float* w2_packed_dev, const float* b2_dev, const float* gamma_dev,
                      const float* w1x1_packed_dev, const float* par_dev, const float* w1_packed_dev,
                      const float* b1_dev, float* scratch_dev, float* out_dev, int h, int w, void* stream);

/* PixelShufflePack (mmedit/models/common/upsample.py:8-51): conv3x3 64 -> 256 followed by F.pixel_shuffle(2).
 * w (256,64,3,3), b (256) -> packed image (pnp_packed_pixel_shuffle_floats floats); x (h,w,64) -> out (2h,2w,64),
 * act as in pnp_conv3x3_f32 (the x4 head applies leaky-relu, iconvsr_ipb_par.py:136-137). */
int64_t pnp_packed_pixel_shuffle_floats(void);
int pnp_pack_pixel_shuffle_f32(const float* w_dev, const float* b_dev, float* dst_dev, void* stream);
int pnp_pixel_shuffle_conv_f32(const float* x_dev, const float* packed_dev, int act, float* out_dev, int h, int w,
                               void* stream);

/* The single-source 64 -> 64 form of pnp_conv3x3_f32 as Winograd F(2x2,3x3) (sr_backbone_utils.py:304-333 block halves,
 * iconvsr_ipb_par.py:144 conv_hr): act(gamma * (conv3x3(x; W) + bias) + Sum_j par_j * conv1x1_j(x)) + residual with
 * x (h,w,64).  wino_w_dev = pnp_wino_image_from_packed_f32 of the packed direct-conv image WITH the same gamma: the gain of the conv
 * term lives in the transformed weights, and gamma_dev HERE SCALES ONLY THE BIAS -- an image built without it (or with another one)
 * gives gamma * bias + conv instead of gamma * (conv + bias), silently; the C ABI cannot tell (the Python op checks the pairing);
 * wino_w1x1_dev = pnp_wino_par_image_from_packed_f32 of the
 * packed 1x1 images or NULL (then par_dev / par_flags_dev are ignored); par_flags_dev as pnp_par_tile_flags_f32 writes
 * them, or NULL.  fp32 arithmetic; differs from pnp_conv3x3_f32 by summation order (~1e-6 on unit-scale maps).  With residual_dev the
 * tile form takes act = 0 only (what the reference's blocks do; PNP_ERR_UNSUPPORTED otherwise), the unit form any act. */
int64_t pnp_wino_image_floats(void);
int64_t pnp_wino_par_image_floats(void);
int pnp_wino_image_from_packed_f32(const float* packed_w_dev, const float* gamma_dev, float* dst_dev, void* stream);
int pnp_wino_par_image_from_packed_f32(const float* packed_w1x1_dev, float* dst_dev, void* stream);
/* The input conv (basicvsr_net.py:484 over the virtual concat of iconvsr_ipb_par.py:90,125) in the same form: srcs_dev[0] the frame
 * as (h,w,4) RGB0, srcs_dev[1..nsrc-1] one to three (h,w,64) maps; wino_w_dev[0] = pnp_wino_rgb_image_from_packed_f32 of the frame's
 * packed chunk (pnp_pack_conv3x3_f32 with csrc 3), wino_w_dev[s] = pnp_wino_image_from_packed_f32 (no gamma) of source s's image.
 * The images of the 64-channel sources must lie within 4 GiB of each other.  out = act(sum_s conv3x3(src_s) + bias). */
int64_t pnp_wino_rgb_image_floats(void);
int pnp_wino_rgb_image_from_packed_f32(const float* packed_rgb_chunk_dev, float* dst_dev, void* stream);
int pnp_conv3x3_wino_ms_f32(int nsrc, const float* const* srcs_dev, const float* const* wino_w_dev, const float* bias_dev,
                            int act, float* out_dev, int h, int w, void* stream);
int pnp_conv3x3_wino_ms_units_f32(int nsrc, const float* const* srcs_dev, const float* const* wino_w_dev, const float* bias_dev,
                                  int act, float* out_dev, int h, int w, void* stream);   /* one block per quadrant unit (small frames) */
int pnp_conv3x3_wino_f32(const float* src_dev, const float* wino_w_dev, const float* bias_dev, const float* gamma_dev,
                         const float* wino_w1x1_dev, const float* par_dev, const int* par_flags_dev,
                         const float* residual_dev, int act, float* out_dev, int h, int w, void* stream);
/* The same conv with one block per 8x8 QUADRANT of a 16x16 tile (four waves = four 16-channel slices of the output): what
 * pnp_generator_forward uses on frames too small to fill the chip with whole tiles (<= PNP_WINO_UNITS_MAX_TILES of them; PNP_OPT_WINOGRAD = 1).  Same
 * arguments, same values bit for bit. */
int pnp_conv3x3_wino_units_f32(const float* src_dev, const float* wino_w_dev, const float* bias_dev, const float* gamma_dev,
                               const float* wino_w1x1_dev, const float* par_dev, const int* par_flags_dev,
                               const float* residual_dev, int act, float* out_dev, int h, int w, void* stream);

/* Which of the three 1x1 partition branches (sr_backbone_utils.py:310-311, Sum_j par_j * conv1x1_j(x)) an 8x16 pixel tile
 * needs at all: par_dev (3,h,w) -> flags_dev[((w+15)/16) * ((h+7)/8)] ints, bit j set iff plane j is nonzero somewhere in
 * the tile.  pnp_generator_forward computes these once per frame; its persistent conv kernel skips a branch on tiles
 * where the plane is zero (exact zeros: bit-identical result).  Codec partition maps are one-hot per >= 8x8 block.
 * Bit 3 + j: every value of plane j in the tile is 0 or exactly 1/255 (what loading_ipb.py writes: uint8 one-hot / 255.) -- the
 * split-fp16 kernel then contracts a masked operand with weights scaled at pack time; consumers of bits 0..2 mask with 7. */
int pnp_par_tile_flags_f32(const float* par_dev, int* flags_dev, int h, int w, void* stream);

/* The same op with fp16 MFMA operands (fp32 sources, accumulation and output): packed_w_f16 are fp16 images
 * made by pnp_f16_image_from_f32 from the fp32 images above (nchunks = 9 per 64-channel source, 1 per RGB0
 * source, 3 for the 1x1 branches; same element count, so nchunks * 8192 bytes).  At least one source must
 * have 64 channels; several 64-channel sources exclude gamma / residual; otherwise PNP_ERR_UNSUPPORTED. */
int pnp_f16_image_from_f32(const float* packed_w_dev, void* dst_dev, int nchunks, void* stream);
int pnp_conv3x3_f16(int nsrc, const float* const* srcs_dev, const int* src_channels,
                    const void* const* packed_w_f16_dev, const float* bias_dev, const float* gamma_dev,
                    const void* packed_w1x1_f16_dev, const float* par_dev, const float* residual_dev,
                    int act, float* out_dev, int h, int w, void* stream);

/* The same op in split fp16 (PNP_PREC_F16X3): every activation x and weight w is carried as hi + lo/2048 with
 * hi = fp16(x), lo = fp16((x - hi) * 2048), a product is three fp16 MFMAs (hi*hi, lo*hi, hi*lo) accumulated in
 * fp32 -- fp32-level results (~1e-6 relative to pnp_conv3x3_f32) from the fp16 matrix pipe.  fp32 sources and
 * output.  packed_w_f32 are the fp32 images (read only for a 4-channel RGB0 source, which runs on the exact fp32
 * kernel; may be NULL for 64-channel sources); packed_w_x3 = pnp_f16x3_image_from_f32 of the same fp32 images
 * (64-channel sources and the 1x1 branches; hi and lo halves interleaved: nchunks * 16384 bytes, nchunks as for
 * pnp_f16_image_from_f32).  par_flags_dev: optional pnp_par_tile_flags_f32 output.  Restrictions as for
 * pnp_conv3x3_f16. */
int pnp_f16x3_image_from_f32(const float* packed_w_dev, void* dst_dev, int nchunks, void* stream);
int pnp_conv3x3_f16x3(int nsrc, const float* const* srcs_dev, const int* src_channels,
                      const float* const* packed_w_f32_dev, const void* const* packed_w_x3_dev,
                      const float* bias_dev, const float* gamma_dev, const void* packed_w1x1_x3_dev,
                      const float* par_dev, const int* par_flags_dev, const float* residual_dev, int act,
                      float* out_dev, int h, int w, void* stream);

/* Per-frame sum of squared differences of the uint8-rounded frames (the statistic behind
 * psnr(tensor2img(a), tensor2img(b)), mmedit/core/misc.py:51-71 + core/evaluation/metrics.py:200-215):
 * a, b (frames, c, h, w) fp32 in HBM -> sse_dev (frames) uint64, exact.  PSNR = 20 log10(255 / sqrt(sse / N)),
 * N = c * (h - 2 crop) * (w - 2 crop). */
int pnp_psnr_sse_f32(const float* a_dev, const float* b_dev, unsigned long long* sse_dev, int frames,
                     int c, int h, int w, int crop_border, void* stream);

/* tensor2img for the PNG write-back (mmedit/core/misc.py:51-71, basicvsr.py:205-231): frames (n,3,h,w) fp32 ->
 * out (n,h,w,3) uint8 RGB = round_half_even(clamp(x,0,1) * 255); a quarter of the D2H bytes of the fp32 frames. */
int pnp_frames_to_rgb8(const float* frames_dev, unsigned char* out_dev, int nframes, int h, int w, void* stream);
/* The inverse layout (RescaleToZeroOne + HWC -> CHW of a decoded frame): in (n,h,w,3) uint8 RGB -> out (n,3,h,w) fp32 planes, byte v
 * -> (float)v / 255.0f by IEEE division (the table PNP_FRAMES_U8_HWC reads). */
int pnp_frames_from_rgb8(const unsigned char* in_dev, float* out_dev, int nframes, int h, int w, void* stream);

/* SSIM statistic (mmedit/core/evaluation/metrics.py:266-355: per channel, 11x11 Gaussian sigma 1.5, 'valid'
 * window, fp64, on the uint8-rounded frames).  Writes one partial sum of the SSIM map per 16x32 tile:
 * partials_dev [frames*c][pnp_ssim_blocks(h,w,crop)] doubles; SSIM(frame) = mean over channels of
 * sum(partials) / ((h-2crop-10)(w-2crop-10)). */
int pnp_ssim_blocks(int h, int w, int crop_border);
int pnp_ssim_partials_f32(const float* a_dev, const float* b_dev, double* partials_dev, int frames, int c, int h,
                          int w, int crop_border, void* stream);

/* The same two statistics with a front end that does not care how a frame is stored, and an optional luma step (what
 * BasicVSR.evaluate forwards as test_cfg.convert_to, mmedit/models/restorers/basicvsr.py:132-150, to psnr / ssim,
 * mmedit/core/evaluation/metrics.py:200-206, 338-346).
 *   a_format, b_format, each on its own: PNP_FRAMES_F32_NCHW, (frames,3,h,w) fp32, rounded to the byte tensor2img makes of it, or
 *   PNP_FRAMES_U8_HWC, (frames,h,w,3) uint8 RGB, the byte as it is.  A byte clip may start at any byte address and h*w*3 need not
 *   be a multiple of 4; no byte outside [p, p + frames*h*w*3) is read.  A U8_HWC clip gives, bit for bit, the statistic of
 *   pnp_frames_from_rgb8 of it; with both formats F32_NCHW and PNP_COLOR_NONE the calls ARE pnp_psnr_sse_f32 / pnp_ssim_partials_f32.
 *   color: PNP_COLOR_NONE, the three channels; PNP_COLOR_Y, the reference's mmcv.bgr2ycbcr(img / 255., y_only=True) * 255. of the
 *   uint8 BGR image (arithmetic restated from mmcv's published source, mmcv/image/colorspace.py; mmcv is not vendored and parity
 *   with an installed mmcv is unpinned): with x_c = (float)byte_c / 255.0f,
 *       Y = (float)((((double)x_B * 24.966 + (double)x_G * 128.553) + (double)x_R * 65.481 + 16.0) / 255.0) * 255.0f,
 *   every product and sum rounded on its own.  pnp_luma_from_frames writes that plane: frames of either format -> (frames,h,w) fp32.
 * pnp_psnr_stat_io: PNP_COLOR_NONE: stat_dev (frames) uint64, the exact SSE over the 3 channels inside the crop, as
 *   pnp_psnr_sse_f32.  PNP_COLOR_Y: stat_dev [frames][pnp_psnr_luma_blocks(h,w,crop)] doubles, one partial sum per block of
 *   (double)d * d, d = Y_a - Y_b in fp32; the caller adds a frame's partials in index order (no floating-point atomics: the same
 *   bits every run) and PSNR = 20 log10(255 / sqrt(sum / ((h - 2 crop)(w - 2 crop)))).
 * pnp_ssim_partials_io: pnp_ssim_partials_f32's tiling, pnp_ssim_blocks and summation order; partials_dev [planes][blocks] with
 *   planes = frames * 3 (PNP_COLOR_NONE) or frames (PNP_COLOR_Y, the window runs over the fp32 Y).
 * PNP_ERR_BAD_ARG: c != 3 with a byte format or with PNP_COLOR_Y; an unknown format or color; 2 crop >= h or w; for SSIM a cropped
 * frame smaller than 11x11; frames < 1, a negative crop or a NULL pointer. */
#define PNP_COLOR_NONE 0
#define PNP_COLOR_Y 1
int pnp_psnr_luma_blocks(int h, int w, int crop_border);
int pnp_psnr_stat_io(const void* a_dev, int a_format, const void* b_dev, int b_format, int color, void* stat_dev,
                     int frames, int c, int h, int w, int crop_border, void* stream);
int pnp_ssim_partials_io(const void* a_dev, int a_format, const void* b_dev, int b_format, int color,
                         double* partials_dev, int frames, int c, int h, int w, int crop_border, void* stream);
int pnp_luma_from_frames(const void* frames_dev, int format, float* out_dev, int nframes, int h, int w, void* stream);

/* Multi-scale SSIM (msssim.hip) on every boundary SSIM is computed on.  This is a definition of the project's OWN: the reference has no
 * MS-SSIM, and no HM / VTM / libvmaf binary was at hand to compare digits with, so agreement with a particular external tool is
 * unpinned.  It is pinned by two independent numpy restatements (pnp_vcve_amd/metrics.py::msssim, tests/msssim_ref.py).  This is the
 * ONE statement of it: Wang, Simoncelli and Bovik 2003, five scales, on one plane of samples (a, b) with peak P.
 *   Samples and peak: the samples SSIM reads on the same boundary.  pnp_msssim_partials_io: PNP_COLOR_NONE, the byte of every channel
 *   (to_u8 of an fp32 plane, the byte of a U8_HWC frame as it is), P = 255; PNP_COLOR_Y, the fp32 Y of pnp_luma_from_frames, P = 255.
 *   pnp_msssim_partials_yuv420: the byte, P = 255.  pnp_msssim_partials_yuv420p16: the word's value as pnp_yuv420_planes16 is read,
 *   P = 2^d - 1.
 *   Crop: once, at level 0, as SSIM's: crop_border on RGB / Y planes, half of it on chroma planes, even for 4:2:0.
 *   Pyramid: level 0 is the cropped plane, h0 x w0.  Level s+1 is floor(h_s / 2) x floor(w_s / 2); its sample (r, c) is
 *       (float)((((double)x[2r][2c] + x[2r][2c+1]) + ((double)x[2r+1][2c] + x[2r+1][2c+1])) * 0.25), stored as fp32.
 *   An odd last row or column of a level is dropped.  For integer samples of up to 12 bits every level is exact in fp32 (12 + 8 bits),
 *   so the fp32 storage IS the fp64 pyramid; for the fp32 Y the expression above is the definition, rounding included.
 *   Statistics at every level: SSIM's window -- 11 taps, sigma 1.5, normalised, separable, 'valid', fp64.  With C1 = (0.01 P)^2,
 *   C2 = (0.03 P)^2:  cs = (2 s_ab + C2) / (s_a^2 + s_b^2 + C2),  l = (2 mu_a mu_b + C1) / (mu_a^2 + mu_b^2 + C1).  The device leaves,
 *   per frame, plane and level, the partial sums of cs and of l * cs over the valid map, one pair per block (16 x 32 tiles of the
 *   valid map, as pnp_ssim_partials_*); the host adds them in index order (deterministic) and divides by the valid map's size
 *   (rows_s - 10)(cols_s - 10): the means are CS_s and S_s.
 *   Value: MS-SSIM = prod_{s=0..3} max(CS_s, 0)^{w_s} * max(S_4, 0)^{w_4}, w = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333) as published
 *   (sum 1.0001, not renormalised), formed by the host in fp64.  A plane pair whose structure is anticorrelated at some scale scores
 *   0, not NaN.  Several planes (RGB, PNP_COLOR_NONE) give the mean of the planes' values, with or without a crop (the reference's
 *   crop quirk belongs to its ssim; it is not carried over to a metric the reference does not have).
 *   Smallest frame: level 4 must hold one window: min(h0, w0) >= pnp_msssim_min_size() = 176 after the crop, for every plane asked
 *   for; chroma planes therefore need a 352-line frame.
 * Sizing (host only, msssim_plan.h), for ONE plane of h x w samples cropped by crop_border on each side (a chroma plane of H x W
 * frames: h = H/2, w = W/2, crop_border = crop/2): pnp_msssim_level_dims gives the level's rows and columns, pnp_msssim_blocks its
 * blocks (0 when the plane cannot be scored or the level is not 0..4).  pnp_msssim_workspace_bytes: the fp32 pyramid, levels 1..4 of
 * both clips, of `planes` such planes a frame (0 when it cannot run); the library owns no device memory, workspace_dev is the
 * caller's, 4-byte aligned.  The 4:2:0 entries take pnp_msssim_workspace_bytes(frames, planes of the mask, h, w, crop_border) of the
 * FRAME: every plane of the mask gets a slot of the Y plane's size.
 * Partials: pnp_msssim_partials_io: partials_dev [frames][planes][B][2] doubles, planes = c (PNP_COLOR_NONE) or 1 (PNP_COLOR_Y), B =
 * sum over the five levels of pnp_msssim_blocks, level after level; [..][0] the block's sum of cs, [..][1] of l * cs.  The 4:2:0 entries:
 * for each plane of plane_mask in the order Y, Cb, Cr, [frames][B of that plane][2], one plane after the other.
 * PNP_ERR_BAD_ARG, decided on the host before any HIP call: whatever pnp_ssim_partials_io / _yuv420 / _yuv420p16 refuse (formats,
 * colors, descriptors, masks, odd crops, differing depths), a NULL workspace, and a cropped plane asked for below 176 x 176. */
int pnp_msssim_min_size(void);
int pnp_msssim_level_dims(int h, int w, int crop_border, int level, int* rows, int* cols);
int pnp_msssim_blocks(int h, int w, int crop_border, int level);
int64_t pnp_msssim_workspace_bytes(int frames, int planes, int h, int w, int crop_border);
int pnp_msssim_partials_io(const void* a_dev, int a_format, const void* b_dev, int b_format, int color, double* partials_dev,
                           void* workspace_dev, int frames, int c, int h, int w, int crop_border, void* stream);
int pnp_msssim_partials_yuv420(const pnp_yuv420_planes* a_host_desc, const pnp_yuv420_planes* b_host_desc, int plane_mask,
                               double* partials_dev, void* workspace_dev, int frames, int h, int w, int crop_border, void* stream);
int pnp_msssim_partials_yuv420p16(const pnp_yuv420_planes16* a_host_desc, const pnp_yuv420_planes16* b_host_desc, int plane_mask,
                                  double* partials_dev, void* workspace_dev, int frames, int h, int w, int crop_border, void* stream);

/* XPSNR (xpsnr.hip): a PSNR whose squared error is weighted block by block with the inverse of the ORIGINAL's spatio-temporal activity
 * (Helmrich et al., ICASSP 2020; ITU-T HSTP-VID-WPOM), of 4:2:0 planes at 8, 10 or 12 bit.  No ffmpeg, VTM or vvenc build was at hand
 * to compare digits with, so agreement with a particular external tool is UNPINNED; the definition follows the published scheme as
 * closely as it could be stated without one, and a deviation found later against a real tool is a bug in THIS statement, the one
 * statement of it.  It is pinned by two independent numpy restatements (pnp_vcve_amd/metrics.py::xpsnr, tests/xpsnr_ref.py).
 *   Inputs: the original clip o (b: the ground truth, whose activity sets the weights) and the test clip r (a), 4:2:0 planes of one bit
 *   depth d in {8, 10, 12}, T frames, luma h x w (even); an integer fps >= 1.  The crop (even; half of it on chroma) is applied first:
 *   H, W and the block grid below refer to the cropped planes and no sample outside the crop is used (16-bit samples are fetched one
 *   by one; bytes as the aligned dwords that cover a group of four where those lie inside the plane's rows -- the reading rule of
 *   the other plane metrics).  Samples are the integers the other plane metrics read (the byte; the word's value as
 *   pnp_yuv420_planes16 is read).  P = 2^d - 1.
 *   Block grid: N = max(4, 4 * floor(32 * sqrt(W H / (3840 * 2160)) + 0.5)) -- 44 at 1280 x 720, 64 at 1920 x 1080, 128 at 3840 x 2160, 4
 *   on small frames (the library decides the rounding in integers: the largest k with (2k - 1)^2 * 3840 * 2160 <= 4096 W H).  Luma
 *   blocks k are the ceil(H / N) x ceil(W / N) tiles [y0, y1) x [x0, x1), clipped at the plane's edge, in row-major order; the chroma
 *   block of k is [y0/2, y1/2) x [x0/2, x1/2) of the chroma plane (all bounds are even).
 *   Activity region of block k (luma of o, frame t): border b = 2 if W H > 2048 * 1152, else 1.  R_k is rows [y0 > 0 ? y0 : b,
 *   y1 < H ? y1 : H - b) and columns likewise: the filters read across block edges, never across the picture's edge.  area_k = rows *
 *   columns of R_k; if R_k is empty, sa = ta = 0 and the activity is the floor.
 *   Spatial activity, b = 1: sa_k = sum over (y, x) in R_k of |12 o[y][x] - 2 (o[y][x-1] + o[y][x+1] + o[y-1][x] + o[y+1][x]) - (the four
 *   diagonal neighbours)|.  b = 2: the positions are every second row and column of R_k starting at its first; at each, |sum of
 *   K6 * o[y-2 .. y+3][x-2 .. x+3]| with the zero-sum kernel K6, rows -2 .. +3:
 *        0 -1 -1 -1 -1  0 / -1 -2 -3 -3 -2 -1 / -1 -3 12 12 -3 -1 / -1 -3 12 12 -3 -1 / -1 -2 -3 -3 -2 -1 / 0 -1 -1 -1 -1  0
 *   (reads stay inside the plane for every block: positions are even and below H - 2, W - 2).
 *   Temporal activity, same positions: s_t is the sample (b = 1) or the sum of the 2 x 2 samples at the position (b = 2).  Second order
 *   when fps >= 32 and t >= 2: ta_k = sum |s_t - 2 s_{t-1} + s_{t-2}|, factor f = 1.  First order otherwise (fps < 32, or t = 1): ta_k =
 *   sum |s_t - s_{t-1}|, f = 2.  At t = 0: ta_k = 0.
 *   Weights (host, fp64): act_k = max((sa_k + f ta_k) / area_k, 2^(d-6)); a_k = act_k^2; minimum smoothing a^_k = max(a_k, min of a_j over
 *   the existing 8 neighbour blocks) (a block with no neighbour keeps a_k); A = sqrt(16 * 2^(2d-9) * sqrt(3840 * 2160 / (W H)));
 *   w_k = A / sqrt(a^_k).
 *   Error: sse_{p,k}, the exact integer squared error of plane p in {Y, U, V} over block k (chroma: over its chroma block).
 *   Value: wsse_p(t) = sum_k w_k sse_{p,k}, added in block index order.  Per frame XPSNR_p(t) = 10 log10(P^2 H_p W_p / wsse_p(t)); per
 *   clip -- the metric's own convention, the log of the mean, not the mean of the logs -- XPSNR_p = 10 log10(P^2 H_p W_p T / sum_t
 *   wsse_p(t)); +inf when the sum is 0.
 * The device part is integers only.  pnp_xpsnr_block_size: N of h x w frames cropped by crop_border (0 when they cannot be scored);
 * pnp_xpsnr_grid: the rows and columns of the block grid (host only, xpsnr_plan.h).  pnp_xpsnr_sums_yuv420 / _yuv420p16: a is the test
 * clip, b the original, each described on its own (any pitch and address, interleaved or planar chroma, low- or high-aligned words);
 * sums_dev [frames][rows * cols][5] uint64 = sse_y, sse_u, sse_v, sa, ta of every frame and block, all of it written by ONE launch,
 * without atomics, the same bits on every run.  plane_mask (PNP_PLANE_*) selects the planes whose error is formed -- only they are read,
 * the others' sums are 0 -- and the Y plane of b, the activity's source, is read whatever the mask.  sa and ta are the raw sums: f is
 * applied by the host.
 * PNP_ERR_BAD_ARG, decided on the host before any HIP call: NULL descriptors, planes (b's Y among them) or sums, frames < 1, odd or
 * too small frames, odd, negative or too large crops, bad descriptors, differing depths (as pnp_ssim_partials_yuv420 / _yuv420p16), a
 * mask outside 1..7, fps < 1. */
int pnp_xpsnr_block_size(int h, int w, int crop_border);
int pnp_xpsnr_grid(int h, int w, int crop_border, int* rows, int* cols);
int pnp_xpsnr_sums_yuv420(const pnp_yuv420_planes* a_host_desc, const pnp_yuv420_planes* b_host_desc, int plane_mask,
                          unsigned long long* sums_dev, int frames, int h, int w, int crop_border, int fps, void* stream);
int pnp_xpsnr_sums_yuv420p16(const pnp_yuv420_planes16* a_host_desc, const pnp_yuv420_planes16* b_host_desc, int plane_mask,
                             unsigned long long* sums_dev, int frames, int h, int w, int crop_border, int fps, void* stream);

/* PSNR-B (psnrb.hip): PSNR with a blocking effect factor (BEF) added to the mean squared error (Yim and Bovik, "Quality assessment of
 * deblocked images", IEEE TIP 2011), the artifact-specific score of the compression-artifact-reduction literature, on every boundary
 * PSNR is served on.  No external tool's digits could be compared, so agreement with a particular public port is UNPINNED; this is the
 * ONE statement of the definition and it is pinned by two independent numpy restatements (pnp_vcve_amd/metrics.py::psnrb, which slices,
 * and tests/psnrb_ref.py, which enumerates pairs).  Two points are stated on purpose: the BEF is taken from the TEST clip a (the
 * enhanced frames), as in the paper -- some public ports take it from their first argument, whichever that is -- and the pair counts
 * are the pairs that really exist -- the popular ports assume sizes that are multiples of the block.
 * For one plane of the test clip a and of the reference b:
 *   Dimensions and crop: the plane has rows x cols samples and peak P; the crop is c (crop_border; crop_border / 2 on the chroma planes
 *   of 4:2:0, crop_border even there).
 *   Block size: Bp = block on RGB channels, on the Y of RGB clips and on the Y plane; block / 2 on Cb / Cr of 4:2:0 (coded chroma blocks
 *   are half size).  block is one of 4, 8, 16, 32, 64; the default of every caller is 8.
 *   Region: rows [y0, y1) = [c, rows - c), columns [x0, x1) = [c, cols - c), h = y1 - y0, w = x1 - x0; every plane asked for needs
 *   min(h, w) >= Bp.  The block grid is anchored at the UNCROPPED plane's origin, which is the coded picture's: a crop does not move it.
 *   Pairs: a horizontal pair is (y, x), (y, x + 1) with both samples in the region; it is a BOUNDARY pair iff (x + 1) mod Bp == 0.  A
 *   vertical pair is (y, x), (y + 1, x); it is a boundary pair iff (y + 1) mod Bp == 0.
 *   Sums, five per frame and plane: sse = sum (a - b)^2 over the region; sbh, snh = sum of (a[y][x] - a[y][x+1])^2 over the boundary /
 *   the other horizontal pairs; sbv, snv likewise over the vertical pairs.  Only a enters the four pair sums.
 *   Counts (host, closed form): kx = floor((x1 - 1) / Bp) - floor(x0 / Bp), ky likewise; NBh = h kx, NNh = h (w - 1 - kx), NBv = w ky,
 *   NNv = w (h - 1 - ky).
 *   Value (host, fp64): D_B = (sbh + sbv) / (NBh + NBv), 0 when there is no boundary pair; D_N = (snh + snv) / (NNh + NNv);
 *   eta = log2(Bp) / log2(min(h, w)); BEF = eta (D_B - D_N) if D_B > D_N, else 0; MSE = sse / (h w);
 *   PSNR-B = 10 log10(P^2 / (MSE + BEF)), +inf when the denominator is 0.
 *   Aggregation: a clip's value is aggregated over frames exactly as PSNR's is on the same boundary; three RGB channels give the mean of
 *   the three channels' values per frame (MS-SSIM's convention here for several planes).
 *   Samples and peaks are those PSNR reads on the same boundary: to_u8 of an fp32 channel or the byte of a U8_HWC frame, P = 255; the
 *   byte of 8-bit planes; the word's value as pnp_yuv420_planes16 is read, P = 2^d - 1; PNP_COLOR_Y: the fp32 Y of pnp_luma_from_frames,
 *   P = 255, where every difference is one fp32 subtraction, squared as (double)d * d.
 *   Magnitudes: a squared difference reaches 2^24 at 12 bit; every sum of a 3840 x 2160 plane stays below 2^63.
 * pnp_psnrb_counts: counts[4] = NBh, NNh, NBv, NNv of a plane of rows x cols samples cropped by `crop` with blocks of plane_block (Bp: a
 * power of two, 2 .. 64); pnp_psnrb_luma_blocks: the partials per frame of PNP_COLOR_Y below, 0 when nothing can be scored.  Both host only
 * (psnrb_plan.h, the one copy of the rules the launcher and the kernel use too).
 * pnp_psnrb_sums_io: frames as pnp_psnr_stat_io takes them, each input in its own format.  PNP_COLOR_NONE: out_dev [frames][c][5] uint64 =
 * sse, sbh, snh, sbv, snv of every frame and channel, exact, the same bits on every run (integer atomics into a buffer the entry
 * zeroes).  PNP_COLOR_Y: out_dev [frames][pnp_psnrb_luma_blocks(h, w, crop_border)][5] doubles, one partial of the five sums per thread
 * block, each written by one thread; the host adds them in index order (no floating-point atomics).
 * pnp_psnrb_sums_yuv420 / _yuv420p16: the planes as pnp_psnr_sse_yuv420 / _yuv420p16 take them, each clip described on its own (any
 * address, any pitch that holds a row, interleaved or planar chroma, low- or high-aligned words; no byte outside [plane, plane + rows *
 * pitch) is read); sums_dev [frames][3][5] uint64 in the order Y, Cb, Cr.  plane_mask (PNP_PLANE_*) selects the planes: only they are
 * read, the others' sums are written as 0.
 * The no-reference form: b (b_dev / the b descriptor) may be NULL; sse is then 0 and nothing of b is read (b_format is ignored) -- the
 * four pair sums are the blockiness of a alone.
 * PNP_ERR_BAD_ARG, decided on the host before any HIP call: whatever pnp_psnr_stat_io / pnp_psnr_sse_yuv420 / _yuv420p16 refuse (with
 * a in b's place when b is NULL), a mask outside 1..7, a block outside the five values, a plane asked for with min(h, w) < Bp, a NULL
 * a or output. */
int pnp_psnrb_counts(int rows, int cols, int crop, int plane_block, int64_t counts[4]);
int pnp_psnrb_luma_blocks(int h, int w, int crop_border);
int pnp_psnrb_sums_io(const void* a_dev, int a_format, const void* b_dev, int b_format, int color, void* out_dev, int frames, int c, int h,
                      int w, int crop_border, int block, void* stream);
int pnp_psnrb_sums_yuv420(const pnp_yuv420_planes* a_host_desc, const pnp_yuv420_planes* b_host_desc, int plane_mask,
                          unsigned long long* sums_dev, int frames, int h, int w, int crop_border, int block, void* stream);
int pnp_psnrb_sums_yuv420p16(const pnp_yuv420_planes16* a_host_desc, const pnp_yuv420_planes16* b_host_desc, int plane_mask,
                             unsigned long long* sums_dev, int frames, int h, int w, int crop_border, int block, void* stream);

/* Enhancement gain (gain.hip): what the enhancement gained over the compressed input -- the dPSNR / dSSIM of the compression-artifact-
 * reduction literature, per frame, per cell of the picture and per partition class.  Nothing here is pinned to an external tool; this
 * is the ONE statement of the definition, pinned by two independent numpy restatements (pnp_vcve_amd/metrics.py::gain_sums, which
 * reshapes, and tests/gain_ref.py, which loops over cells and pixels).
 * Three clips of one size, one chroma format and one bit depth: a, the test clip (the generator's output); l, the compressed input the
 * generator was given; g, the original.
 *   Region: what PSNR scores.  Frames of pixels and the Y plane are cropped by c = crop_border on every side, a chroma plane by c / sy
 *   down and c / sx across (crop_border even where an axis is subsampled).
 *   Cells: a gain block B is 16, 32, 64 or 128 luma samples (64: the CTU of HEVC, every caller's default; 128: VVC's).  The grid is
 *   anchored at the UNCROPPED frame's origin, as PSNR-B's is, and has ceil(h / B) rows and ceil(w / B) columns for every plane of every
 *   format.  A chroma cell is B / sy x B / sx samples, so cell (i, j) covers the same picture area in every plane: sample (y, x) of a
 *   plane lies in cell (floor(y / (B / sy)), floor(x / (B / sx))).  A cell's sums run over its samples inside the region; a cell wholly
 *   inside the crop holds zeros.
 *   Sums, two per frame, plane and cell: E_a = sum (a - g)^2 and E_l = sum (l - g)^2.  On planes they are exact integers over the
 *   samples pnp_psnr_sse_yuv / _yuvp16 compare.  On frames with PNP_COLOR_NONE they are exact integers over the very samples
 *   pnp_psnr_stat_io compares -- to_u8 of an fp32 channel or the byte of a U8_HWC frame, each of the three inputs in its own format
 *   -- the three channels of a pixel added.  With PNP_COLOR_Y they are fp64 sums of (double)d * d, d the one fp32 subtraction of two
 *   Y of pnp_luma_from_frames, as pnp_psnr_stat_io forms it.  A cell is owned by one thread block, reduced in a fixed order and stored
 *   once: no atomic, integer or floating-point, touches the grid, and every run gives the same bits.
 *   Partition classes (only with a partition map par (frames, 3, h, w) fp32, as the generator takes it): the class of a pixel is the
 *   3-bit mask (par0 != 0) | (par1 != 0) << 1 | (par2 != 0) << 2; class 0 is "no block painted", overlapping planes give the mixed
 *   classes.  Per frame and class three numbers N (pixels of the class in the region), E_a and E_l, kept on the Y plane of planes clips
 *   and on the pixels of frames (a pixel's error: the sum over its channels), never on chroma planes.
 *   Values (host, fp64, one function for the device path and the numpy path), with peak P = 255 or 2^d - 1 and N the samples of the
 *   region (frames with PNP_COLOR_NONE: 3 per pixel):
 *     PSNR_t(x) = 10 log10(P^2 N / E_x,t), +inf for E = 0;   dPSNR_t = 10 log10(E_l,t / E_a,t): 0 for 0 / 0, +inf for E_a = 0 < E_l,
 *     -inf for E_l = 0 < E_a.  A clip's dPSNR is the mean over frames; PSNR_SD is the population standard deviation (ddof 0) of
 *     PSNR_t over the frames; dPSNR_YUV_t = (6 dY + dU + dV) / 8.  The SSIM halves are the existing SSIM entries called twice.
 * pnp_gain_grid: rows, cols of the grid of h x w frames.  pnp_gain_cell_count: the samples of cell (row, col) of `plane` (PNP_PLANE_*;
 * PNP_PLANE_Y with any format for frames of pixels, where it counts pixels) inside the region, in closed form.  pnp_gain_luma_tiles:
 * the thread blocks per frame that PNP_COLOR_Y leaves class partials of, 0 when nothing can be scored.  All three host only
 * (gain_plan.h, the one copy of the geometry the launcher and the kernel use too).
 * pnp_gain_sums_io: frames as pnp_psnr_stat_io takes them, c == 3, each of a, l, g in its own format.  grid_dev
 * [frames][rows][cols][2] = E_a, E_l: uint64 with PNP_COLOR_NONE, doubles with PNP_COLOR_Y.  class_dev, with par_dev: PNP_COLOR_NONE
 * [frames][8][3] uint64 = N, E_a, E_l (integer atomics, one per thread block, class and sum, into a buffer the entry zeroes);
 * PNP_COLOR_Y [frames][pnp_gain_luma_tiles(h, w, crop_border, block)][8][3] doubles, a thread block's own partials, which the host adds
 * in index order.
 * pnp_gain_sums_yuv / _yuvp16: the planes as pnp_psnr_sse_yuv / _yuvp16 take them, each of the three clips described on its own (any
 * address, any pitch that holds a row, interleaved or planar chroma, low- or high-aligned words; no byte outside [plane, plane + rows *
 * pitch) is read).  grid_dev [frames][3][rows][cols][2] uint64 in the order Y, Cb, Cr; plane_mask (PNP_PLANE_*) selects the planes:
 * only they are read, the others' cells are written as 0.  class_dev [frames][8][3] uint64 with par_dev, classes of the Y plane.
 * The grid and the integer class sums are zeroed by the entry (a kernel, not a memset node), the class partials of PNP_COLOR_Y are written
 * whole by their tiles, and ONE kernel launch follows per call.
 * PNP_ERR_BAD_ARG, decided on the host before any HIP call: whatever pnp_psnr_stat_io / pnp_psnr_sse_yuv / _yuvp16 refuse for (a, g)
 * or (l, g), c != 3, a NULL input or grid, a block outside the four values, a crop that leaves nothing, a mask outside 1..7, class_dev
 * without par_dev or par_dev without class_dev, par_dev with a mask that lacks PNP_PLANE_Y. */
int pnp_gain_grid(int h, int w, int block, int* rows, int* cols);
int pnp_gain_cell_count(int h, int w, int crop_border, int block, int plane, int chroma_format, int row, int col, int64_t* count);
int pnp_gain_luma_tiles(int h, int w, int crop_border, int block);
int pnp_gain_sums_io(const void* a_dev, int a_format, const void* l_dev, int l_format, const void* g_dev, int g_format, int color,
                     const float* par_dev, void* grid_dev, void* class_dev, int frames, int c, int h, int w, int crop_border, int block,
                     void* stream);
int pnp_gain_sums_yuv(const pnp_yuv420_planes* a_host_desc, const pnp_yuv420_planes* l_host_desc, const pnp_yuv420_planes* g_host_desc,
                      int plane_mask, const float* par_dev, unsigned long long* grid_dev, unsigned long long* class_dev, int frames, int h,
                      int w, int crop_border, int block, int chroma_format, void* stream);
int pnp_gain_sums_yuvp16(const pnp_yuv420_planes16* a_host_desc, const pnp_yuv420_planes16* l_host_desc,
                         const pnp_yuv420_planes16* g_host_desc, int plane_mask, const float* par_dev, unsigned long long* grid_dev,
                         unsigned long long* class_dev, int frames, int h, int w, int crop_border, int block, int chroma_format,
                         void* stream);

/* Modulated deformable 3x3 conv, 64 -> 64 channels, deform_groups 16 (mmcv.ops.modulated_deform_conv2d as
 * called at mmedit/models/backbones/sr_backbones/iconvsr_mv.py:38-41,81-84; semantics restated, mmcv is not
 * vendored).  x_dev (h,w,64) pixel-major; om_dev (h,w,448): conv_offset[2] output (pre-sigmoid masks) in the
 * channel order given by pnp_dcn_ref_channel (packed channel -> reference channel of the 432, -1 = padding);
 * flow_x/flow_y (h,w) planes added to every (dx, dy) offset or NULL; w_packed = pnp_pack_conv3x3_f32 image. */
int pnp_dcn_nhwc_f32(const float* x_dev, const float* om_dev, const float* flow_x_dev, const float* flow_y_dev,
                     const float* w_packed_dev, const float* bias_dev, float* out_dev, int h, int w, void* stream);
int pnp_dcn_ref_channel(int packed_channel);
/* The same op with fp16 MFMA operands (PNP_PREC_F16: samples and weights rounded to fp16, fp32 accumulation):
 * w_f16_dev = pnp_dcn_f16_image_from_f32(w_packed) (9 * 4096 halfs = 73,728 bytes). */
int pnp_dcn_f16_image_from_f32(const float* w_packed_dev, void* dst_dev, void* stream);
int pnp_dcn_nhwc_f16(const float* x_dev, const float* om_dev, const float* flow_x_dev, const float* flow_y_dev,
                     const void* w_f16_dev, const float* bias_dev, float* out_dev, int h, int w, void* stream);

/* MV / partition records -> dense maps: the inner loop of LoadImageFromFileList_ipb.__call__
 * (mmedit/datasets/pipelines/loading_ipb.py:328-369) + RescaleToZeroOne(partitions) + HWC->CHW.
 *   records_dev (R,10) fp32 rows (direction, w, h, x_w, y_w, x, y, motion_x, motion_y, scale) in file
 *   order over the whole clip; rec_frame_dev (R) int32 frame of each row; slices_host (t) = ord('I'|'P'|'B').
 *   mvs_dev (t,4,h,w) and par_dev (t,3,h,w) are fully written; scratch_dev = t*2*h*w int32.  t <= 256. */
int pnp_rasterise_side_info_f32(const float* records_dev, const int* rec_frame_dev, long num_records,
                                const float* slices_host, int t, int h, int w, float* mvs_dev, float* par_dev,
                                int* scratch_dev, void* stream);

/* Self-ensemble over the 8 flips / transposes of a frame and, optionally, time reversal -- the reference's SpatialTemporalEnsemble
 * (mmedit/models/common/ensemble.py) with the side information transformed together with the frames, which the reference does not do
 * (it calls the model with the frames only and cannot run this generator).
 * A variant is 4 bits v: bit 0 = 'vertical' in the reference's naming, a flip of the WIDTH axis; bit 1 = 'horizontal', a flip of the
 * HEIGHT axis; bit 2 = transpose; bit 3 = time reversal.  Input views apply bit 0, then bit 1, then bit 2 (the reference's img_list
 * order); the output inverse applies bit 2, then bit 1, then bit 0; time reversal commutes with all three.  For an original plane X
 * of h x w, with (h', w') = (w, h) if bit 2 else (h, w) and frame i' = t-1-i if bit 3 else i:
 *     X'[i', y', x'] = X[i, y, x],  (a, b) = (x', y') if bit 2 else (y', x');  y = h-1-a if bit 1 else a;  x = w-1-b if bit 0 else b.
 *   Frames (lq: fp32 (t,3,h,w) or uint8 (t,h,w,3)) and partition planes (t,3,h,w) are moved and nothing else: partition classes are
 *   areas (256, 128 or 64 px), so 16x8 and 8x16 already share a plane.
 *   Motion vectors (t,4,h,w), channels (fwd x, fwd y, bwd x, bwd y), are moved and then changed in this order: bit 0 negates channels
 *   0 and 2; bit 1 negates 1 and 3; bit 2 swaps 0 <-> 1 and 2 <-> 3; bit 3 swaps (0,1) <-> (2,3).  A negated zero is -0.0.
 *   slices, QPs, base_QPs (t) are reversed in time under bit 3 and untouched otherwise (host data: no entry here).
 * The ensemble's output over the variants V = 0..7 (spatial) or 0..15 (with time reversal) is a sequential fp32 sum in ascending v,
 * acc = inv_0(G(view_0)); acc = acc + inv_v(G(view_v)) for v = 1, 2, ...; out = acc * (1/|V|), one exact power-of-two scaling.
 * pnp_ensemble_view: one launch writes variant v's lq', mvs' and par' from the originals.  Each in / out pair may be NULL together.
 *   No row of a uint8 frame is assumed dword-aligned (w or h odd); all element offsets are 64-bit.
 * pnp_ensemble_accumulate_f32: x_dev (t,c,H',W') is variant v's output, acc_dev (t,c,H,W) lies in the original orientation and frame
 *   order; per element s = first ? x : acc + x, then acc = s if scale == 1 else s * scale (plain fp32, no fused operation).
 * PNP_ERR_BAD_ARG, decided on the host before any HIP call: one side of a pair NULL; variant outside 0..15; t, h, w, c < 1 (H, W
 *   alike); an unknown format; in == out; scale not finite or <= 0.  PNP_ERR_UNSUPPORTED: more than 2^31 - 1 tiles in one call. */
int pnp_ensemble_view(const void* lq_dev, const float* mvs_dev, const float* par_dev, void* lq_out_dev, float* mvs_out_dev,
                      float* par_out_dev, int frames_format, int t, int h, int w, int variant, void* stream);
int pnp_ensemble_accumulate_f32(const float* x_dev, float* acc_dev, int t, int c, int H, int W, int variant, int first, float scale,
                                void* stream);

#ifdef __cplusplus
}
#endif
#endif
