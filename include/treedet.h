/*
 * treedet.h — C ABI of libtreedet_hip.so, the MI355X (gfx950) tile-inference engine that
 * stands behind the reference's model seam:
 *
 *     batch_predictions = self.model(batch_tensors)      TreeDetection/prediction.py:182-183
 *
 * (a Python call into detectron2's GeneralizedRCNN configured by TreeDetection/config.py:25-66;
 * the reference itself has no FFI — this header is the FFI a maintainer would bind instead, see
 * INTEGRATION.md). Plain pointers and sizes only; no C++ or torch types cross this boundary.
 *
 * Conventions
 *   - every function returns td_status: 0 = ok, < 0 = error; the message is td_last_error().
 *   - "dev" pointers are device (HBM) addresses on the engine's GPU; "host" pointers are host.
 *   - activations are NHWC float32 (or float16 when precision = 1) inside the engine.
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).
 *   - the engine is NOT thread-safe; one engine per device and stream.
 */
#ifndef TREEDET_H
#define TREEDET_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int td_status;
typedef struct td_engine td_engine;

enum {
    TD_OK = 0,
    TD_ERR_INVALID = -1,   /* bad argument / shape */
    TD_ERR_HIP = -2,       /* a HIP runtime call failed */
    TD_ERR_WEIGHTS = -3,   /* missing or mis-shaped tensor in load_weights */
    TD_ERR_CAPACITY = -4,  /* forward() exceeds what reserve() sized */
    TD_ERR_STATE = -5,     /* call order (forward before load/reserve) */
    TD_ERR_UNSUPPORTED = -6 /* a well-formed input this library does not decode (td_jpeg_decode: progressive, 12-bit, ...) */
};

enum { TD_PRECISION_FP32 = 0, TD_PRECISION_FP16 = 1 };
enum { TD_INPUT_F32_CHW = 0,  /* float32 [B,3,Hp,Wp], BGR 0..255 — what prediction.py:170 builds   */
       TD_INPUT_U8_HWC = 1 }; /* uint8   [B,Hp,Wp,3],  BGR        — the same values before astype() */

/* Model hyper-parameters. Defaults (td_model_desc_default) = detectron2 defaults + the overrides
 * of TreeDetection/config.py:35,59-61 (NUM_CLASSES=1, SCORE_THRESH_TEST=0.3, NMS_THRESH_TEST=0.5). */
typedef struct td_model_desc {
    int32_t num_classes;           /* 1 */
    int32_t precision;             /* TD_PRECISION_* */
    int32_t pre_nms_topk;          /* 1000 per FPN level */
    int32_t post_nms_topk;         /* 1000 per image */
    int32_t detections_per_image;  /* 100 */
    float rpn_nms_thresh;          /* 0.7 */
    float score_thresh;            /* 0.3 (strict >) */
    float nms_thresh;              /* 0.5 */
    float mask_thresh;             /* 0.5 (>=) */
} td_model_desc;

/* One named fp32 host tensor; names are detectron2 state-dict keys
 * (e.g. "backbone.bottom_up.res2.0.conv1.norm.running_var"). */
typedef struct td_tensor_desc {
    const char* name;
    const float* data;   /* host, contiguous, torch layout ([Cout,Cin,kh,kw] / [out,in]) */
    int32_t ndim;
    int64_t shape[4];
} td_tensor_desc;

#define TD_MASK_SIDE 28

/* Caller-allocated device output of one forward(). D = detections_per_image.
 * Fields may be NULL to skip that output (mask_bits == NULL skips the paste). */
typedef struct td_detections {
    float* boxes;          /* dev [B, D, 4]  x1,y1,x2,y2 in OUTPUT (pre-resize tile) pixels, score-descending */
    float* scores;         /* dev [B, D] */
    int32_t* classes;      /* dev [B, D] */
    int32_t* count;        /* dev [B]    number of valid rows */
    float* mask_probs;     /* dev [B, D, 28, 28] sigmoid probabilities */
    int32_t* mask_region;  /* dev [B, D, 4] x0,y0,x1,y1: the integer region the CPU paste evaluates */
    int64_t* mask_offset;  /* dev [B, D]   offset (in 32-bit words) of detection's bit rows from mask_bits of image b */
    uint32_t* mask_bits;   /* dev [B, mask_words_per_image]; row r of a region starts at offset + r*ceil((x1-x0)/32);
                              bit (x-x0)&31 of word (x-x0)>>5 = pasted mask >= mask_thresh */
    int64_t mask_words_per_image;
} td_detections;

/* ---- engine life cycle ------------------------------------------------------------------- */
void td_model_desc_default(td_model_desc* desc);
td_status td_engine_create(const td_model_desc* desc, int device, td_engine** out);
td_status td_engine_load_weights(td_engine* e, const td_tensor_desc* tensors, size_t n);
/* Size the workspace for forward() calls of up to max_batch images of padded size max_hp x max_wp
 * (multiples of 32). May be called again to grow. */
td_status td_engine_reserve(td_engine* e, int max_batch, int max_hp, int max_wp);
/* images: dev, format per `input_format`, B images padded to Hp x Wp (multiples of 32);
 * hw_valid: host int32 [B,2] un-padded (H', W') of each image (detectron2 image_sizes);
 * hw_out:   host int32 [B,2] output (height, width) = the tile's pre-resize size (prediction.py:168,182).
 * Asynchronous on `stream`; results are complete once the stream has drained. */
td_status td_engine_forward(td_engine* e, const void* images, int input_format, const int32_t* hw_valid,
                            const int32_t* hw_out, int B, int Hp, int Wp, void* stream, td_detections* out);
/* The same forward cut into six phases for cross-batch software pipelining (three engines, a main stream and one
 * side stream per engine):
 *   0 trunk (stem .. RPN heads)   1 RPN top-k / NMS / merge + RoIAlign 7x7   2 box-head FCs + predictors
 *   3 detections + RoIAlign 14x14 4 mask-head convolutions                   5 mask predictor, scatter, paste
 * Even phases are dense contractions, odd phases low-occupancy selection work: enqueue the even phases of successive
 * batches back to back on a main stream and each batch's odd phases on its own side stream, and the selection work of
 * one batch overlaps the contractions of the next (bench.py: per tick trunk(t), mask convs(t-2), FCs(t-1)). Phase 0 takes the arguments of td_engine_forward and stores them; phases 1-5
 * ignore everything but `e`, `phase` and `stream`. Each phase waits (hipStreamWaitEvent) for the previous phase of the
 * same batch; phase 0 waits for phases 0-4 of the engine's previous batch (the trunk rewrites what they read, the
 * Winograd workspace of the fp32 mask-head convolutions included) and phase 3 for the previous batch's phase 5 (whose
 * predictor / paste read the mask buffers and row count that phases 3-4 rewrite), so any stream assignment is correct.
 * Optional pre-phase TD_PHASE_STEM (6): stem convolution + max-pool of the NEXT batch (VALU / HBM work, no matrix
 * cores) with the arguments of phase 0; the following phase 0 (images may be NULL) then starts at res2. Run it on a side
 * stream while the previous batch's contractions hold the main stream. "stem" and "pool" of td_engine_tensor are
 * available after it. */
#define TD_PHASE_STEM 6
td_status td_engine_forward_phase(td_engine* e, int phase, const void* images, int input_format, const int32_t* hw_valid,
                                  const int32_t* hw_out, int B, int Hp, int Wp, void* stream, td_detections* out);
/* Expose an internal buffer of the last forward() for stage-wise parity tests. The names, extents and element types are the
 * public rows of the engine's workspace plan (csrc/workspace.cpp; td_workspace_plan below lists them for any shape). B, Hp, Wp are
 * those of the batch in hand, h x w a pyramid level's map (Hp >> 2 .. Hp >> 5; p6 = (p5 - 1) / 2 + 1), P = post_nms_topk,
 * D = detections_per_image, C the model's widths; "act" = float16 in the fp16 engine, else float32. A name exists once its phase
 * of td_engine_forward_phase has run in this forward, and until the next phase 0 or a td_engine_reserve that grows the workspace.
 *   stem pre-phase or phase 0: "stem" [B,Hp/2,Wp/2,C] act, "pool" [B,Hp/4,Wp/4,C] act
 *   phase 0: "res2".."res5" [B,h,w,C] act, "p2".."p6" [B,h,w,C] act, "rpn_head2".."rpn_head6" [B,h,w,15] float32 in both
 *            precisions (3 logits, then 12 deltas per position)
 *   phase 1: "rpn_cand_boxes" [B,5,1024,4] float32, "rpn_cand_scores" [B,5,1024] float32, "rpn_cand_valid" / "rpn_cand_idx" /
 *            "rpn_keep" [B,5,1024] int32, "rpn_keep_count" [B,5] int32, "proposals" [B,P,4] float32, "proposal_scores" [B,P]
 *            float32, "proposal_count" [B] int32, "pooled7" [B*P,7,7,C] act
 *   phase 2: "box_pred" [B*P,6] float32 in both precisions (two logits, foreground first, then four deltas)
 *   phase 3: "det_all_boxes" [B,P,4] / "det_all_scores" [B,P] float32, "det_flags" [B,P] int32, "det_sorted_boxes" [B,P,4] /
 *            "det_sorted_scores" [B,P] float32 (the flagged rows by score descending, index ascending) with "det_sorted_count" [B]
 *            int32, "det_keep" [B,D] int32 (positions in the sorted list) with "det_keep_count" [B] int32, "det_boxes_net" [B,D,4]
 *            float32, "pooled14" [B*D,14,14,C] act
 *   phase 4: "mask_total_rows" [1] int32 (the device row count the mask head reads), "mask_fcn3" / "mask_fcn4" [B*D,14,14,C] act,
 *            "mask_deconv" [B*D,28,28,C] act
 *   phase 5: "mask_logits" / "mask_probs_compact" [B*D,28,28] float32 (the first total = sum of counts rows are live)
 * The "rpn_head*" pointers may be overwritten between phase 0 and phase 1 of
 * td_engine_forward_phase (after phase 0 has completed on its stream): stage tests feed crafted heads that way. The same way,
 * "proposals", "proposal_count" (int32, every entry within [0, P]) and "box_pred" may be overwritten between phase 2
 * and phase 3, and "mask_deconv" between phase 4 and phase 5, each after the earlier phase has completed on its
 * stream: the later phases then run on the crafted values. No other buffer may be written.
 * dims is filled with up to 4 extents (0-padded); *elem_size with the element size in bytes. */
td_status td_engine_tensor(td_engine* e, const char* name, void** dev_ptr, int64_t dims[4], int* elem_size);
/* Copy that activation into a caller-owned device buffer of `bytes` bytes (asynchronous on `stream`). */
td_status td_engine_read_tensor(td_engine* e, const char* name, void* dst_dev, int64_t bytes, void* stream);
/* Per-category device timing of forward(): when enabled, every kernel launch is bracketed by HIP events on the
 * forward's stream. Categories: 0 conv_igemm (all MFMA contractions), 1 stem, 2 pool/subsample, 3 rpn_select
 * (top-k, decode, NMS, merge), 4 roi_align, 5 detect (decode/sort/NMS/finalize), 6 mask_tail (predictor, scatter,
 * paste), 7 mask-head contractions (row count lives on the device: flops/bytes are left 0 for the caller to fill),
 * 8 "executed": no time of its own — flops[8] = multiply-adds x 2 the category-0 launches really issued (the Winograd
 * path of the fp32 engine runs 4/9 of a 3x3 layer's algorithmic FLOPs; its two transform kernels are timed inside
 * category 0, the conv family), launches[8] = layers that took the Winograd path. td_engine_profile_read synchronises the recorded events and ACCUMULATES since the last reset:
 * ms[c] device milliseconds, launches[c], flops[c] algorithmic FLOPs (2*M*N*K, conv only), bytes[c] algorithmic
 * HBM bytes (inputs read once + outputs written once). Arrays hold TD_PROF_CATEGORIES entries. */
#define TD_PROF_CATEGORIES 9
/* enable: 0 off, 1 one event pair per category group, 2 "detail": additionally one event pair per launch of the
 * contraction family for td_engine_profile_classes (perturbs the forward: use it on a region of its own). */
td_status td_engine_profile_enable(td_engine* e, int enable);
td_status td_engine_profile_read(td_engine* e, double* ms, int64_t* launches, double* flops, double* bytes, int reset);
/* Speed-of-light accounting of the contraction family by class. Per class since the last reset: launches; the FLOPs the
 * launches really EXECUTE (a Winograd layer's plane products, not the direct convolution's multiplies); the bytes the
 * chosen algorithm moves through HBM when every tensor is read / written once (V / M planes of the Winograd layers
 * included); tmin_ms = sum over launches of max(executed FLOPs / MFMA peak of the engine's precision, bytes /
 * achievable HBM rate) with the constants below (MI355X_MICROARCH.md); ms = measured time (detail mode only, else 0).
 * Class 5 (mask head) has a device-side row count: only its time is reported. Arrays hold TD_PROF_CLASSES entries. */
#define TD_PROF_CLASSES 7
#define TD_CLS_WINO_GEMM 0   /* Winograd plane contractions (fp32 engine) */
#define TD_CLS_WINO_XFORM 1  /* Winograd input / output transform kernels */
#define TD_CLS_CONV1X1 2     /* 1x1 convolutions: bottleneck conv1 / conv3 / shortcut, FPN laterals, RPN heads */
#define TD_CLS_CONV3X3 3     /* direct 3x3 convolutions (fp16 engine: all of them; fp32: the 64-channel res2 layers) */
#define TD_CLS_FC 4          /* box head: fc1, fc2, predictors */
#define TD_CLS_MASK_HEAD 5   /* mask-head contractions and transforms (rows = live detections, known on the device only) */
#define TD_CLS_TAIL 6        /* fused bottleneck tail: 3x3 (mid -> mid) + 1x1 (mid -> 4 mid) + shortcut in one launch (res2; fp16: res3 too) */
#define TD_PEAK_F32_MFMA_TFLOPS 157.3   /* v_mfma_f32_32x32x2_f32, dense (a split-bf16 launch enters the accounting with 6/16 of its FLOPs, SPLIT_PIPE_FACTOR of csrc/launch_cost.cpp: its MFMA pipe time at this rate) */
#define TD_PEAK_F16_MFMA_TFLOPS 2500.0  /* v_mfma_f32_32x32x16_f16, dense */
#define TD_HBM_ACHIEVABLE_TBS 6.3       /* measured streaming rate (8.0 TB/s spec) */
td_status td_engine_profile_classes(td_engine* e, double* ms, int64_t* launches, double* exec_flops, double* bytes, double* tmin_ms, int reset);
const char* td_last_error(void);
void td_engine_destroy(td_engine* e);

/* ---- tile preprocessing (reference Predictor._process_tile, prediction.py:159-176) ---------- */
/* Pillow-exact 8-bit bilinear resize (two fixed-point passes) of one tile, fused with the
 * band pick (2,1,0)=BGR of prediction.py:166: src dev uint8 [h, w, C] (pixel-interleaved, C >= 3),
 * dst dev uint8 [dst_pitch_rows.., 3] written at dst[(y*dst_pitch_px + x)*3 + c] for y<out_h, x<out_w. */
td_status td_resize_tile_u8(const uint8_t* src, int h, int w, int c, uint8_t* dst, int out_h, int out_w,
                            int dst_pitch_px, void* tmp_dev /* >= h*out_w*3 bytes */, void* stream);
/* The same for n tiles of one common size in two launches: src_tiles = HOST array of n device pointers; tile i is
 * written to dst + i*dst_image_stride_bytes; tmp_dev >= n*h*out_w*3 bytes. */
td_status td_resize_batch_u8(const uint8_t* const* src_tiles, int n, int h, int w, int c, uint8_t* dst, int out_h,
                             int out_w, int dst_pitch_px, int64_t dst_image_stride_bytes, void* tmp_dev, void* stream);
/* The float branch of the same step (prediction.py:167-169): a tile that is not uint8 (16-bit imagery rescaled by
 * 255 * x / 65535, float rasters) goes through detectron2's ResizeTransform → torch.nn.functional.interpolate(mode="bilinear",
 * align_corners=False) and is then cast to float32. src dev float64 [c, h, w] (planar, BGR already picked); dst dev float32,
 * written at dst[ch * dst_plane_stride + y * dst_pitch_px + x] for y < out_h, x < out_w (the caller zero-fills the padding).
 * Arithmetic in float64 in torch's own order (half-pixel centres, source index clamped at 0, border neighbours clamped),
 * rounded to float32 once. */
td_status td_resize_bilinear_f64(const double* src, int c, int h, int w, float* dst, int out_h, int out_w, int dst_pitch_px,
                                 int64_t dst_plane_stride, void* stream);
/* The same step for 16-bit rasters that lie decoded in HBM (td_tiff_blocks_to_image_u16_dev, or uploaded whole): the rule of
 * prediction.py:166-169 and the float resize in two launches per batch, no float64 tile crossing PCIe. raster: DEVICE uint16
 * [height, width, c] (pixel-interleaved, c >= 3). windows: HOST int32 [n][8], one row per tile window of ONE common size (n <=
 * 64) = {r0, c0, h, w, vy0, vy1, vx0, vx1}: the window's first row / column in the raster, its size, and the rows [vy0, vy1) /
 * columns [vx0, vx1) of the window whose pixel centres lie inside the tile's bounds (rasterio.mask; everything else reads 0).
 * Launch 1 writes band1_max[i] (DEVICE int32 [n]) = the maximum of file band 1 over the masked window; launch 2 picks bands
 * (2, 1, 0), turns every tap x into 255 * x / 65535 in float64 (one multiplication, one IEEE division) where band1_max[i] > 255
 * and into (double)x elsewhere, then interpolates exactly as td_resize_bilinear_f64 does. dst: DEVICE float32, written at
 * dst[i * dst_image_stride + ch * dst_plane_stride + y * dst_pitch_px + x] for y < out_h, x < out_w (the caller zero-fills the
 * padding). Bit-identical to td_resize_bilinear_f64 fed with numpy's `255.0 * bgr / 65535.0`. Asynchronous on `stream`. */
td_status td_windows_u16_to_input(const uint16_t* raster, int height, int width, int c, const int32_t* windows, int n, int32_t* band1_max,
                                  float* dst, int out_h, int out_w, int dst_pitch_px, int64_t dst_plane_stride, int64_t dst_image_stride,
                                  void* stream);
/* ResizeShortestEdge(800, 1333) output shape for an h x w tile (Appendix A item 2). */
void td_resize_shape(int h, int w, int short_edge, int max_size, int* out_h, int* out_w);

/* ---- op-level entry points (parity tests; each is the kernel the engine itself launches) ---- */
/* Fused tail of a bottleneck block (detectron2 BottleneckBlock: conv2 3x3 + FrozenBN + ReLU, conv3 1x1 + FrozenBN, + shortcut,
 * ReLU) in one launch: x [B,H,W,mid], w2 [mid,3,3,mid], w3 [cout,mid], scale / bias per layer (NULL = 1 / 0),
 * shortcut and y [B,H,W,cout]; cout = 4 mid; mid = 64 (fp32, fp16) or 128 (fp16). precision: TD_PRECISION_*.
 * Bit-identical to td_conv2d_nhwc(3x3, relu) followed by td_conv2d_nhwc(1x1, residual, relu). */
td_status td_bottleneck_tail_nhwc(const void* x, const void* w2, const float* scale2, const float* bias2, const void* w3,
                                  const float* scale3, const float* bias3, const void* shortcut, void* y, int B, int H, int W,
                                  int mid, int cout, int precision, void* stream);
/* The split form of the float32 tail (mid = 64, cout = 256; what the fp32 engine runs in res2 by default): the 3x3 contracts on
 * the bf16 matrix cores with both operands as three bf16 pieces (w2 is split here, the engine splits once at load), the 1x1 and
 * its epilogue are td_bottleneck_tail_nhwc's. Same tensors; another rounding of the 3x3 than the fp32 form (inside the same
 * float64 bound). mid_out NULL: the fused launch, y is written. mid_out [B,H,W,mid] (DEVICE float32): the unfused twin — the
 * launch stops behind conv2 + FrozenBN + ReLU and stores that tensor; w3 / scale3 / bias3 / shortcut / y are ignored (may be
 * NULL). The fused y is bit-identical to the mid_out launch followed by td_conv2d_nhwc(1x1, residual, relu) on a float32 tile. */
td_status td_bottleneck_tail_split_nhwc(const void* x, const void* w2, const float* scale2, const float* bias2, const void* w3,
                                        const float* scale3, const float* bias3, const void* shortcut, void* y, void* mid_out,
                                        int B, int H, int W, int mid, int cout, void* stream);
/* Host only: the split-bf16 filter bank of conv_split.hip / the split tail from float32 filters w [cout][taps][cin] (taps = 1:
 * a 1x1 / FC bank; 9: a 3x3 bank), cin a multiple of 32: [ceil(cout/32)][taps * cin/32 k-chunks, channel chunk outer, tap
 * inner][2 slices][3 pieces][64 lanes][8 bf16]; lane l = (r = l & 31, h = l >> 5) of (tile t, chunk cc * taps + tap, slice s, piece
 * p) holds piece p of w[32 t + r][tap][32 cc + 16 s + 4 h .. + 3] and [.. + 8 + 4 h .. + 3]. Returns the bank's size in bytes
 * (what `out` must hold; nothing is written when out is NULL or out_bytes is smaller), < 0 on bad arguments. */
int64_t td_conv_split_pack(const float* w, int cout, int cin, int taps, uint8_t* out, int64_t out_bytes);
/* NHWC convolution: y = act(conv(x, w) * scale + bias [+ residual]).
 * x [B,H,W,Cin], w [Cout,KH,KW,Cin], scale/bias [Cout] (NULL = 1 / 0), residual [B,Ho>>rs,Wo>>rs,Cout]
 * (rs = res_shift: 1 = nearest-2x upsampled add, the FPN top-down path), y [B,Ho,Wo,Cout].
 * Cin must be a multiple of 32. precision selects float32 or float16 tensors (weights follow); bits 8..15 of
 * `precision` may carry (block-tile id + 1) to force one kernel variant (parity tests of every variant; 0 = the
 * library chooses); bit 16 with float16 tensors: y is float32 (how the engine runs the RPN / box-predictor heads).
 * Bit 17 (0x20000, strict tile selection; tests only, the engine never sets it): a forced tile id (bits 8..15, or the
 * TD_CONV_CFG diagnostic) that cannot run this launch — an fp16-only tile on float32 tensors, a plane-contraction tile
 * (18-20) off a plain fp32 1x1 / stride-1 layer, the filter-stationary tile (33) where conv_bs_ok fails, a filter-direct
 * tile where conv_bd_ok fails — returns TD_ERR_INVALID with a message naming the id and the condition, instead of running
 * the heuristic tile in its place.
 * Tile ids 34-37 (float32 tensors, 1x1 without padding, Cin a multiple of 32 only) contract on the bf16 matrix cores with both
 * operands written as three bf16 pieces (six piece products per 16 k into the float32 accumulator, conv_split.hip): float32 in
 * and out, another rounding than ids 0-33 (inside the same float64 bound), bit-identical to each other. */
td_status td_conv2d_nhwc(const void* x, const void* w, const float* scale, const float* bias,
                         const void* residual, int res_shift, void* y, int B, int H, int W, int Cin,
                         int Cout, int KH, int KW, int stride, int pad, int relu, int precision,
                         void* stream);
/* td_conv2d_nhwc at stride 1 without residual, with the two launch properties only the mask head uses (tests only: the op-level
 * door to what phase 4 of the forward launches). out_mode 0: y [B,Ho,Wo,Cout]. out_mode 1 (the 2x2 / stride 2 deconvolution
 * written as a 1x1 layer with a pixel-shuffle store; Cout a multiple of 32): y [B,2Ho,2Wo,Cq], Cq = Cout/4, filter row
 * n = (dy*2+dx)*Cq + co lands at y[b, 2h+dy, 2w+dx, co], and scale / bias hold Cq entries indexed by co = n % Cq.
 * rows_dyn (DEVICE int32 scalar, or NULL): the kernels read it and compute only the first min(B*Ho*Wo, *rows_dyn * rows_mul)
 * output rows (rows_mul = Ho*Wo turns an image count into rows); nothing past them is written and no input row at or past
 * them contributes to a row below them. `precision` carries the same bits as in td_conv2d_nhwc (forced tile id, strict
 * selection, float16 tensors with float32 y); strict selection refuses a tile that cannot run the out_mode or a device row
 * count (the fp16 ping-pong tile and the filter-direct tiles: out_mode 0 only; the filter-stationary tile: no device count). */
td_status td_conv2d_rows_nhwc(const void* x, const void* w, const float* scale, const float* bias, void* y, int B, int H, int W,
                              int Cin, int Cout, int KH, int KW, int pad, int relu, int out_mode, const int32_t* rows_dyn,
                              int rows_mul, int precision, void* stream);
/* A 256-channel float16 convolution (stride 1, + bias, ReLU) whose output feeds ONLY a 1x1 head (reference: detectron2's
 * StandardRPNHead behind prediction.py:183 — conv3x3 + ReLU, then the objectness / anchor-delta 1x1 layers, SURVEY.md
 * Appendix A item 5): the head is contracted from the finished tile inside the same launch and only
 * head_y [B*Ho*Wo][head_n] (float32) = conv_out . head_w^T + head_b is written. head_w [head_n <= 32][256] float16.
 * bits 8..15 of `precision` must carry (tile id + 1) of a block tile that owns all 256 output channels and stages them as one float16 tile
 * (9, 10, 12, 13, 17, 23, 27). Bit-identical to td_conv2d_nhwc(relu) followed by a 1x1 td_conv2d_nhwc with float32 output. */
td_status td_conv2d_head_nhwc(const void* x, const void* w, const float* bias, const void* head_w, const float* head_b,
                              float* head_y, int B, int H, int W, int Cin, int KH, int KW, int pad, int head_n, int precision,
                              void* stream);
/* The same 3x3 / stride 1 / pad 1 convolution (float32) through the Winograd F(2x2,3x3) path the fp32 engine uses where it
 * measures faster (input transform, 16 batched plane contractions on the MFMA kernel, output transform): x [B,H,W,Cin],
 * w [Cout,3,3,Cin], y [B,H,W,Cout] = act(conv * scale + bias), all DEVICE pointers; Cin % 32 == 0, Cout % 4 == 0.
 * Synchronous (allocates its own scratch): parity tests only. Test switches of the environment: TD_WINO_TILE=4 the F(4x4,3x3) form,
 * TD_WINO_FOLD=1 its folded launch, TD_WINO_SPLIT=1 the 36 planes of the unfolded F(4x4) form on the split-bf16 tiles (the twin bank
 * is packed in scratch; also read by td_conv2d_winograd_head_nhwc), TD_CONV_CFG the block tile of the plane contraction. */
td_status td_conv2d_winograd_nhwc(const float* x, const float* w, const float* scale, const float* bias, float* y, int B,
                                  int H, int W, int Cin, int Cout, int relu, void* stream);
/* F(4x4,3x3) form of td_conv2d_head_nhwc for float32 tensors (how the fp32 engine runs the RPN, reference StandardRPNHead behind
 * prediction.py:183): 3x3 / stride 1 / pad 1 conv to 256 channels + bias + ReLU, whose output feeds only the 1x1 head
 * head_w [head_n <= 32][256]; the head is contracted inside the output transform and only head_y [B*H*W][head_n] is written.
 * Bit-identical to td_conv2d_winograd_nhwc (TD_WINO_TILE=4) followed by a 1x1 td_conv2d_nhwc. */
td_status td_conv2d_winograd_head_nhwc(const float* x, const float* w, const float* bias, const float* head_w, const float* head_b,
                                       float* head_y, int B, int H, int W, int Cin, int head_n, void* stream);
/* Diagnostic (tests, tools; host only, needs no engine and no GPU): which form the engine gives one convolution of the forward —
 * the one rule its every contraction asks. The forms differ in rounding, so the answer depends on the layer's own shape and the
 * rules only, never on the batch or a timing.
 *   rules[8]  = precision, winograd, wino_fused, wino_minc, wino43_min, wino_fold, wino_slab, fuse_head (the engine's defaults for
 *               TD_PRECISION_FP32: 0, 1, 1, 128, 12, 39, 0, 1); a negative entry after the precision = what an engine created
 *               now would use, its default or the TD_* diagnostic switch of the environment. wino_elems = floats in each
 *               Winograd workspace plane (td_engine_reserve: 16 x the largest [tiles of 2x2 outputs] x [channels] of the 3x3
 *               layers, which never runs short for the engine's own layers; 0 for the fp16 engine)
 *   layer[9]  = cout, cin, kh, kw, has a scale, writes float32, and which banks it has: F(2x2) filters, F(4x4) filters, split-bf16
 *               (of a 3x3 layer with F(4x4) filters: the split-bf16 twin of that bank — form 3 then contracts its 36 planes on the
 *               split-bf16 tiles where the rows are static, and its tune key carries flag 128 on top of 64)
 *   call[10]  = B, H, W, stride, pad, relu, has a residual, out_mode, device-side row count, rows_mul
 *   head[9]   = the same facts of a 1x1 layer that is this layer's only consumer, or NULL
 *   out[10]   = form (0 direct, 1 split-bf16, 2 Winograd F(2x2), 3 F(4x4) in three launches, 4 F(4x4) folded),
 *               head (0 a launch of its own, 1 inside the F(4x4) output transform, 2 inside the direct launch if the measured tile
 *               owns all 256 output channels), 1 if a block tile is measured for the form, the five fields of its tune key
 *               (TD_TUNE_CACHE lines: cout, cin, kh*16+kw, rows, flags), tiles per F(2x2) slab, images per fold group */
td_status td_conv_path(const int32_t* rules, int64_t wino_elems, const int32_t* layer, const int32_t* call, const int32_t* head,
                       int32_t* out);
/* Diagnostic (tests; host only, needs no engine and no GPU): the workspace plan of an engine — every device buffer td_engine_reserve
 * would allocate for (B, Hp, Wp), one row each, from the table the engine itself walks (csrc/workspace.cpp). widths[16] = what the
 * loader reads off the weights: stem channels; cout of conv1, of conv2 and of conv3 in the first block of res2 .. res5 (4 + 4 + 4);
 * FPN channels; box-head FC width; mask deconv output channels. winograd: the TD_WINOGRAD switch (fp32 engine: 1 by default).
 * Fills min(cap, *n_rows) rows; TD_ERR_CAPACITY when cap is short (*n_rows still says how many there are). */
typedef struct td_workspace_row {
    char name[32];         /* the engine's buffer; "res[2]" for a member of an indexed family */
    char public_name[32];  /* td_engine_tensor's name for it, or "" */
    int32_t kind;          /* 0 activation (engine precision), 1 float32, 2 int32, 3 uint32, 4 uint64 */
    int32_t elem_size;     /* bytes */
    int32_t phase;         /* the public name exists after this phase (6: after the stem pre-phase or phase 0); -1 without one */
    int32_t pad_;
    int64_t dims[4];       /* extents at (B, Hp, Wp), 0-padded: what td_engine_tensor reports after a forward of that shape */
    int64_t alloc_bytes;   /* size of the allocation */
} td_workspace_row;
td_status td_workspace_plan(int precision, int winograd, int post_nms_topk, int detections_per_image, const int32_t* widths, int B,
                            int Hp, int Wp, td_workspace_row* rows, int cap, int* n_rows);
/* Greedy NMS of n boxes (dev [n,4], scores dev [n]); keep_idx dev int32 [n] receives the kept
 * indices in descending-score order (ties: lower index first), *keep_count (dev) their number. */
td_status td_nms(const float* boxes, const float* scores, int n, float iou_thresh, int32_t* keep_idx,
                 int32_t* keep_count, void* stream);
/* RoIAlign (aligned, adaptive sampling) over one NHWC level: feat [H,W,C], rois dev [R,4],
 * out [R,pooled,pooled,C]. */
td_status td_roi_align(const void* feat, int H, int W, int C, const float* rois, int R, float spatial_scale,
                       int pooled, void* out, int precision, void* stream);
/* Paste N 28x28 probability masks into out_h x out_w at `boxes` (output units): fills
 * mask_region/mask_offset/mask_bits exactly like forward() does for one image. */
td_status td_paste_masks(const float* mask_probs, const float* boxes, int n, int out_h, int out_w,
                         float thresh, int32_t* mask_region, int64_t* mask_offset, uint32_t* mask_bits,
                         int64_t mask_words_cap, void* stream);

/* Same for a batch of images, asynchronously on `stream` (no host synchronisation): mask_probs [batch][D][28*28],
 * boxes [batch][D][4], counts [batch] — all DEVICE pointers; out_hw = host array of (height, width) per image.
 * Outputs as in td_detections: mask_region [batch][D][4], mask_offset [batch][D], mask_bits
 * [batch][mask_words_per_image]. This is how rank 0 pastes the detections gathered from the other ranks. */
td_status td_paste_masks_batch(const float* mask_probs, const float* boxes, const int32_t* counts, const int32_t* out_hw,
                               int batch, int dets_per_image, float thresh, int32_t* mask_region, int64_t* mask_offset,
                               uint32_t* mask_bits, int64_t mask_words_per_image, void* stream);

/* Border following ON THE DEVICE for the packed masks of a batch (same contours, order and points as
 * td_find_contours on each detection's region; prediction.py:232-236). Inputs: the mask_region / mask_offset /
 * mask_bits / count arrays of td_detections (device). Outputs (device, caller-allocated):
 *   points        int16 [batch][points_cap][2]   (x, y) in tile pixels
 *   image_points  int32 [batch]                  points allocated per image (may exceed points_cap: see status 4)
 *   det_info      int32 [batch][D][4]            status, contour count, first point, total points of the detection
 *   contour_info  int32 [batch][D][TD_CONTOUR_MAX][2]   per contour in RETR_TREE order: (point offset inside the
 *                                                detection's block, number of points)
 * status: 0 traced; 1 region larger than the on-chip label image; 2 more than TD_CONTOUR_MAX contours; 4 point
 * buffer full — such detections are left to td_find_contours on the host. Asynchronous on `stream`. */
#define TD_CONTOUR_MAX 256
td_status td_trace_contours_dev(const int32_t* mask_region, const int64_t* mask_offset, const uint32_t* mask_bits,
                                int64_t mask_words_per_image, const int32_t* counts, int batch, int dets_per_image,
                                int16_t* points, int points_cap, int32_t* image_points, int32_t* det_info,
                                int32_t* contour_info, void* stream);

/* ---- host-side epilogue (reference prediction.py:232-245, utilities.py:182-207) ------------- */
/* Border following on a binary image (row-major uint8, non-zero = foreground) equivalent to
 * cv2.findContours(RETR_TREE / RETR_LIST ordering, CHAIN_APPROX_SIMPLE): writes contour points as
 * int32 (x,y) pairs into `points` (capacity max_points pairs) and contour start offsets into
 * `starts` (capacity max_contours+1). Returns the number of contours, or < 0 on overflow/error. */
int td_find_contours(const uint8_t* img, int h, int w, int32_t* points, int max_points, int32_t* starts,
                     int max_contours);
/* Whole host epilogue of one tile (reference prediction.py:229-261, Predictor._process_and_save_single):
 * the n detections' packed masks (mask_region / mask_offset / mask_bits of td_detections for ONE image, copied
 * to host memory; mask_words = capacity of mask_bits in 32-bit words) → border following → contours with >= 4
 * points, ring closed → pixel-corner coordinates through `transform` (rasterio order a,b,c,d,e,f; float64) →
 * the JSON array the reference writes to Prediction_<tile>.json, one entry per contour:
 *   {"image_id": <image_id>, "category_id": <class>, "score": <score>, "polygon_coords": [[[x, y], ...]]}
 * byte-identical to Python's json.dumps of that list. Writes the text (no terminator) to buf if it fits in
 * cap bytes; *needed always receives its length. Returns the number of entries, TD_ERR_CAPACITY when cap is
 * too small (call again with *needed bytes), or another negative status. Thread-safe; host code only. */
int td_tile_polygons_json(const int32_t* mask_region, const int64_t* mask_offset, const uint32_t* mask_bits,
                          int64_t mask_words, const float* scores, const int32_t* classes, int n,
                          const double* transform, const char* image_id, char* buf, int64_t cap, int64_t* needed);

/* The same epilogue for a tile whose packed rows are still on the device (reference prediction.py:197-265 end to end for
 * one tile: the masks leave the GPU, become polygons and are written to Prediction_<tile>.json): mask_region / mask_offset /
 * scores / classes are the host copies of the image's small records, mask_bits_dev the DEVICE pointer of its bit rows
 * (td_detections.mask_bits + b * mask_words_per_image) and rows_host a pinned host buffer of mask_words words. Only the
 * words the paste wrote (mask_offset[n-1] + size of the last region; 0.1-5 MB against a 12.8 MB capacity at 1000 x 1000)
 * cross PCIe: copied on one of the library's own copy streams of `device`, waited for by this thread alone. Then
 * td_tile_polygons_json's text is written to `path` (created / truncated). *bytes_written receives the file size.
 * Returns the number of entries or a negative status. Thread-safe; the caller has made sure the forward that produced
 * the rows has completed (the host copies it passes were read after that event). */
int td_tile_prediction_file(int device, const int32_t* mask_region, const int64_t* mask_offset, const uint32_t* mask_bits_dev,
                            uint32_t* rows_host, int64_t mask_words, const float* scores, const int32_t* classes, int n,
                            const double* transform, const char* image_id, const char* path, int64_t* bytes_written);

/* The tile files of a whole batch in ONE call: tile i reads its records at mask_region + i * D * 4, mask_offset + i * D, scores /
 * classes + i * D (D = dets_per_image), counts[i] detections (count < 0: the tile is skipped, as a dropped tile is), its device rows
 * at mask_bits_dev + i * bits_stride_words, uses the pinned rows_host + i * bits_stride_words, the affine at transforms + 6 * i and
 * writes paths[i]; status[i] / bytes_written[i] receive td_tile_prediction_file's result per tile. The tiles are spread over
 * `threads` host threads. Returns TD_OK or the first failing tile's status (the other tiles are still written). */
int td_batch_prediction_files(int device, int n_tiles, int dets_per_image, const int32_t* mask_region, const int64_t* mask_offset,
                              const uint32_t* mask_bits_dev, uint32_t* rows_host, int64_t bits_stride_words, const float* scores,
                              const int32_t* classes, const int32_t* counts, const double* transforms, const char* image_id,
                              const char* const* paths, int threads, int32_t* status, int64_t* bytes_written);

/* ---- raster input (reference prediction.py:61,164: rasterio.open / rasterio.mask.mask → GDAL → libtiff) ---- */
/* Decompress one TIFF strip or tile: LZW (compression 5) and PackBits (32773) per TIFF 6.0; DEFLATE strips go
 * through zlib on the host side. Return the number of bytes written to dst (capacity cap), or a negative status
 * (TD_ERR_CAPACITY when the stream decodes to more than cap bytes, TD_ERR_INVALID for a corrupt stream). */
int64_t td_tiff_lzw_decode(const uint8_t* src, int64_t n, uint8_t* dst, int64_t cap);
int64_t td_tiff_packbits_decode(const uint8_t* src, int64_t n, uint8_t* dst, int64_t cap);
/* The writer's side of td_tiff_lzw_decode (test rasters, the bench's LZW fixture): one strip or tile → a TIFF 6.0 LZW stream
 * (ClearCode first, EOI last) that libtiff / GDAL / td_tiff_lzw_decode read back. Returns the compressed size or a negative status. */
int64_t td_tiff_lzw_encode(const uint8_t* src, int64_t n, uint8_t* dst, int64_t cap);
/* ---- compressed rasters decoded on the GPU (tiffdecode.hip). The reference decodes every tile window on the
 * host (prediction.py:164 → GDAL → libtiff); here the compressed blocks of a raster cross PCIe once and are decoded by one wave
 * each. comp: DEVICE copy of the file's compressed bytes (padded by >= 8 bytes); block_off / block_nbytes: DEVICE int64
 * [nblocks], position and size of every LZW strip / tile in comp; blocks_out: DEVICE [nblocks][block_cap] bytes, block b decoded
 * at b * block_cap (block_cap = bytes of a full block); decoded: DEVICE int64 [nblocks], status: DEVICE int32 [2 * nblocks + 1] (the
 * first nblocks entries are the blocks' status; behind them lies the wide-pass list, which stays readable after the launch: status[nblocks] =
 * how many blocks the first pass left to the second one (an epoch's output outgrew the 16-bit table: a table-adding code arrived more
 * than 65535 - 4096 bytes into it), then their block numbers in no particular order; the entries behind those are not written) — bytes produced (low 32 bits; the high 32
 * bits count the strings that were copied through memory instead of the LDS ring: a diagnostic), and 0 = ok,
 * 1 = corrupt stream, 2 = more than block_cap bytes (the rules of td_tiff_lzw_decode). Asynchronous on `stream`, whose device must be
 * the calling thread's current one. The decoder waves share workgroups (6 - 12 each, one workgroup per CU at most) and take their blocks
 * from a per-launch counter, so a raster that decodes while forwards run on other streams leaves whole CUs to them. */
td_status td_tiff_lzw_decode_dev(const uint8_t* comp, const int64_t* block_off, const int64_t* block_nbytes, int nblocks,
                                 uint8_t* blocks_out, int64_t block_cap, int64_t* decoded, int32_t* status, void* stream);
/* The same for DEFLATE blocks (TIFF compression 8 / 32946: zlib streams; inflate_core.h): status int32 [nblocks], decoded int64
 * [nblocks]; the decoder stops at the end of the last DEFLATE block: the Adler-32 trailer is not checked (td_tiff_inflate_verified_dev
 * checks it). */
td_status td_tiff_inflate_dev(const uint8_t* comp, const int64_t* block_off, const int64_t* block_nbytes, int nblocks,
                              uint8_t* blocks_out, int64_t block_cap, int64_t* decoded, int32_t* status, void* stream);
/* td_tiff_inflate_dev followed, on the same stream, by the check zlib ends with: every block that decoded with status 0 is summed
 * (Adler-32 over its decoded[b] bytes in blocks_out, before any predictor is undone) and compared with the big-endian trailer that
 * follows its last DEFLATE block in comp. status: 0 / 1 / 2 as above, 3 = the sums differ or the stream ends before its trailer. The
 * decoder also applies zlib's rules where td_tiff_inflate_dev is laxer (window size in the header, incomplete code sets), so that a
 * block has status 0 exactly when zlib accepts its stream and it fits block_cap. end_off: DEVICE int64 [nblocks] scratch — where each
 * block's trailer begins, from the start of its stream (not block_nbytes - 4: a byte count may include padding). */
td_status td_tiff_inflate_verified_dev(const uint8_t* comp, const int64_t* block_off, const int64_t* block_nbytes, int nblocks,
                                       uint8_t* blocks_out, int64_t block_cap, int64_t* decoded, int32_t* status, int64_t* end_off,
                                       void* stream);
/* The second launch of td_tiff_inflate_verified_dev alone (measurements: tools/raster_decode_bench.py): one workgroup per block sums
 * blocks[b * block_cap .. + decoded[b]) of the blocks whose status is 0 and writes status 3 where the trailer at
 * comp[block_off[b] + end_off[b]] differs or would lie beyond block_nbytes[b]. */
td_status td_tiff_adler32_blocks_dev(const uint8_t* blocks, int64_t block_cap, const int64_t* decoded, const uint8_t* comp,
                                     const int64_t* block_off, const int64_t* block_nbytes, const int64_t* end_off, int nblocks,
                                     int32_t* status, void* stream);
/* The same kernel over one DEVICE buffer of n < 2^31 bytes: its Adler-32 (zlib.adler32's value) → out_dev[0]. Asynchronous on `stream`. */
td_status td_adler32_dev(const uint8_t* data_dev, int64_t n, uint32_t* out_dev, void* stream);
/* The decoder td_tiff_inflate_dev runs, instantiated for one lane on the host (parity tests against zlib without a GPU): one zlib
 * stream → dst; returns the bytes produced or a negative status (TD_ERR_INVALID corrupt stream, TD_ERR_CAPACITY). */
int64_t td_tiff_inflate(const uint8_t* src, int64_t n, uint8_t* dst, int64_t cap);
/* The decoder and the rules of td_tiff_inflate_verified_dev on the host: zlib's header and code-set rules, then the Adler-32 trailer
 * after the last DEFLATE block (bytes behind it are ignored, as zlib leaves them unused). Accepts exactly the streams zlib's inflate
 * accepts; TD_ERR_INVALID for a corrupt stream, a wrong checksum or a missing trailer, TD_ERR_CAPACITY. */
int64_t td_tiff_inflate_verified(const uint8_t* src, int64_t n, uint8_t* dst, int64_t cap);
/* Zstandard (RFC 8878; TIFF compression 50000, GDAL's COMPRESS=ZSTD; zstd_core.h). One strip or tile → dst: every frame of the stream
 * in turn, skippable frames skipped, a content checksum (XXH64, low 32 bits) verified. Returns the bytes produced, TD_ERR_INVALID for a
 * corrupt stream, a dictionary id, a wrong checksum or bytes that begin no frame, TD_ERR_CAPACITY when the stream regenerates more
 * than cap bytes. The tile reader's block decoder; libzstd is used nowhere on the reading side. */
int64_t td_tiff_zstd_decode(const uint8_t* src, int64_t n, uint8_t* dst, int64_t cap);
/* What a Zstandard stream is made of (fixture generator, coverage test): counters int64 [TD_ZSTD_STATS], in this order — frames,
 * block_raw, block_rle, block_comp, max_blocks_per_frame, lit_raw, lit_rle, lit_huff, lit_treeless, lit_streams_1, lit_streams_4,
 * hufw_direct, hufw_fse, seq0, LL_predef, LL_rle, LL_fse, LL_repeat, OF_predef, OF_rle, OF_fse, OF_repeat, ML_predef, ML_rle, ML_fse,
 * ML_repeat, window_desc, single_segment, checksum, seq_long (3-byte sequence count), seq_2byte, skippable. Returns the bytes the stream
 * decodes to or a negative status. */
#define TD_ZSTD_STATS 32
int64_t td_zstd_stream_stats(const uint8_t* src, int64_t n, int64_t* counters);
/* Zstandard blocks on the GPU, one wave per block (zstddecode.hip): arguments and launch shape as td_tiff_inflate_dev (comp padded by
 * >= 8 bytes, waves share workgroups, one workgroup per CU at most, blocks by a per-launch counter, asynchronous on `stream`). status
 * int32 [nblocks]: 0 ok, 1 corrupt, 2 more than block_cap bytes (decoded[b] then says how far the decoder got, the bytes that fit are
 * right), 4 declined — a content checksum, a second frame or a skippable frame in the block: the host reader takes such a raster.
 * scratch: DEVICE memory of td_tiff_zstd_scratch_bytes(nblocks) bytes (the literal buffers of the resident decoder waves), to be kept
 * until the launch has ended. */
td_status td_tiff_zstd_decode_dev(const uint8_t* comp, const int64_t* block_off, const int64_t* block_nbytes, int nblocks,
                                  uint8_t* blocks_out, int64_t block_cap, int64_t* decoded, int32_t* status, uint8_t* scratch,
                                  int64_t scratch_bytes, void* stream);
int64_t td_tiff_zstd_scratch_bytes(int nblocks);
/* Decoded blocks (strips: block_w = width; tiles: full padded tiles, row-major grid blocks_across x blocks_down) → the raster
 * image [height][width][spp] uint8 (DEVICE), predictor 2 undone per block row on the way (td_tiff_unpredict's arithmetic).
 * spp <= 4. Asynchronous on `stream`. */
td_status td_tiff_blocks_to_image_dev(const uint8_t* blocks, int64_t block_cap, int block_w, int block_h, int blocks_across,
                                      int blocks_down, int spp, int predictor, uint8_t* image, int width, int height, void* stream);
/* The same for two-byte samples: blocks hold little-endian uint16 (block_cap still counts BYTES), image is [height][width][spp]
 * uint16 (DEVICE), and predictor 2 is undone per whole sample modulo 65536 (TIFF 6.0 section 14). spp <= 4. Asynchronous on `stream`. */
td_status td_tiff_blocks_to_image_u16_dev(const uint8_t* blocks, int64_t block_cap, int block_w, int block_h, int blocks_across,
                                          int blocks_down, int spp, int predictor, uint16_t* image, int width, int height, void* stream);
/* The same for float32 samples (height rasters): blocks hold the bytes as the block decoders left them, image is [height][width][spp]
 * float (DEVICE). predictor 1: little-endian floats, copied; 2: horizontal differencing of the samples viewed as uint32, modulo 2^32;
 * 3: the floating-point predictor (TIFF Technical Note 3, td_tiff_unpredict_float's rule), undone per block row. spp <= 4.
 * Asynchronous on `stream`. */
td_status td_tiff_blocks_to_image_f32_dev(const uint8_t* blocks, int64_t block_cap, int block_w, int block_h, int blocks_across,
                                          int blocks_down, int spp, int predictor, float* image, int width, int height, void* stream);
/* The same three for band-separate files (PlanarConfiguration = 2): `blocks` holds the decoded blocks of the SELECTED bands only (bit p
 * of plane_mask: band p), bands ascending, within a band the file's own order (blocks_across x blocks_down, row-major), each block at
 * a multiple of block_cap BYTES. A block row is block_w consecutive samples of one band: predictor 2 is a stride-1 running sum per
 * block row modulo 2^8 / 2^16 / 2^32; predictor 3 (float32 only) is TIFF Technical Note 3 with one sample per pixel (four byte planes
 * of block_w bytes, most significant first, differenced byte-wise over all 4 * block_w bytes: td_tiff_unpredict_float's rule). image
 * is [height][width][spp] as above; the channels of bands that are not selected are written as 0. 1 <= spp <= 4, plane_mask non-zero
 * and below 1 << spp. One launch, asynchronous on `stream`. */
td_status td_tiff_planes_to_image_dev(const uint8_t* blocks, int64_t block_cap, int block_w, int block_h, int blocks_across,
                                      int blocks_down, int spp, int plane_mask, int predictor, uint8_t* image, int width, int height,
                                      void* stream);
td_status td_tiff_planes_to_image_u16_dev(const uint8_t* blocks, int64_t block_cap, int block_w, int block_h, int blocks_across,
                                          int blocks_down, int spp, int plane_mask, int predictor, uint16_t* image, int width, int height,
                                          void* stream);
td_status td_tiff_planes_to_image_f32_dev(const uint8_t* blocks, int64_t block_cap, int block_w, int block_h, int blocks_across,
                                          int blocks_down, int spp, int plane_mask, int predictor, float* image, int width, int height,
                                          void* stream);
/* ---- JPEG-in-TIFF (compression 7; jpeg_core.h, jpegcodec.cpp, jpegdecode.hip): sequential Huffman, 8-bit, grey, three components
 * (Y 1x1 / 2x1 / 2x2, chroma 1x1) or four (all 1x1, stored as they decode: RGB + an extra sample, separated), restart intervals; the
 * output equals the host reader's (Pillow's libjpeg: accurate integer IDCT, fancy
 * upsampling, its YCbCr → RGB) byte for byte. Everything else is unsupported and stays with the host reader. */
/* Host plan of a raster, once per image: the JPEGTables tag (tables, tables_len; 0 = none) is parsed once, then every block's headers
 * (data + block_off[b], block_nbytes[b] bytes; host memory) as the host reader's stream sees them (an Adobe segment saying
 * photometric == 6 first when bands == 3 and the block has no JFIF; nothing is added for bands == 4, whose blocks must hold four
 * components sampled 1x1 and no Adobe segment naming a transform — YCCK is unsupported). bands: 1, 3 or 4. block_rows[b]: the rows the block must hold; its SOF width must be
 * block_w. Per block, block_info int64 [nblocks][8] = {0 decodable / 1 unsupported, table set, sampling mode (0 grey, 1 4:4:4, 2 4:2:2,
 * 3 4:2:0, 4 four components as stored), 1 = YCbCr → RGB (never in mode 4), SOF width, SOF height, first coefficient (int16 elements), restart interval}. segs int64 [seg_cap][4]: one
 * entropy-coded segment per block, or one per restart interval = {offset in data, bytes, block, first MCU | MCU count << 32}.
 * tabsets: [tabset_cap] deduplicated table sets of TD_JPEG_TABSET_BYTES each (quantisation tables in natural order, Huffman lookup
 * tables). totals int64 [4] = {segments, table sets, coefficients, unsupported blocks}. Returns TD_OK, TD_ERR_CAPACITY (totals say how
 * much is needed) or TD_ERR_INVALID. Host code, thread-safe. */
#define TD_JPEG_TABSET_BYTES 11904
td_status td_tiff_jpeg_plan(const uint8_t* tables, int64_t tables_len, const uint8_t* data, const int64_t* block_off,
                            const int64_t* block_nbytes, int nblocks, int photometric, int bands, int block_w, const int32_t* block_rows,
                            int64_t* block_info, int64_t* segs, int64_t seg_cap, void* tabsets, int64_t tabset_cap, int64_t* totals);
/* Decode a planned raster on the GPU: comp = DEVICE copy of `data` (same offsets), block_info / segs / tabsets = DEVICE copies of the
 * plan's arrays (nseg segments); coef: DEVICE int16 [totals[2]] scratch (zeroed here), planes: DEVICE uint8 [totals[2]] scratch;
 * image: DEVICE [height][width][bands] uint8, blocks block_w x block_h (strips: block_w = width) in a grid blocks_across wide, each
 * cropped to the raster. status: DEVICE int32 [nblocks], 0 = ok, 1 = corrupt entropy-coded data. One lane decodes one segment, the
 * waves take 64 segments at a time from a per-launch counter; then the IDCT and the upsampling / colour kernels. bands == 4 (every block
 * of mode 4, as the plan for four bands gives them): image must be 4-byte aligned, each pixel is written as one dword. Asynchronous on
 * `stream`, whose device must be the calling thread's current one. */
td_status td_tiff_jpeg_decode_dev(const uint8_t* comp, const int64_t* block_info, int nblocks, const int64_t* segs, int nseg,
                                  const void* tabsets, int16_t* coef, uint8_t* planes, int64_t coef_count, int32_t* status, uint8_t* image,
                                  int width, int height, int bands, int block_w, int block_h, int blocks_across, void* stream);
/* The same decoder on one host thread, one complete stream (src, n bytes) → dst [height][width][components] (cap bytes); shape int32 [3]
 * receives (height, width, components). Returns the bytes written, TD_ERR_UNSUPPORTED, TD_ERR_INVALID (corrupt stream) or
 * TD_ERR_CAPACITY. */
int64_t td_jpeg_decode(const uint8_t* src, int64_t n, uint8_t* dst, int64_t cap, int32_t* shape);
/* td_tiff_jpeg_decode_dev for rasters with entropy-coded segments too long for one lane (blocks without restart markers). The plan's
 * segments come as two lists (DEVICE int64 [n][4], either may be empty): segs_short goes through the lane-per-segment kernel as
 * above; each segment of segs_long is decoded by the 64 lanes of one wave (self-synchronising Huffman decoding, jpeg_core.h: the
 * bytes are cut into subsequences of subseq_bytes (4 .. 1 << 20) raw bytes, 64 of them form a window, the lanes walk them from
 * guessed states and again from their predecessor's exit state until the states agree, at most 64 rounds a window; then they write
 * the coefficients, and a second kernel turns the DC differences into DC values, one wave per (segment, component)). Same
 * coefficients, same status as one lane gives, then the same IDCT and pixel kernels. stats: DEVICE int64 [4], zeroed here, then
 * {walk rounds summed over the windows, windows, the most rounds one window took, windows that took one round} of the long segments.
 * nshort + nlong >= nblocks. Asynchronous on `stream`, whose device must be the calling thread's current one. */
td_status td_tiff_jpeg_decode_long_dev(const uint8_t* comp, const int64_t* block_info, int nblocks, const int64_t* segs_short, int nshort,
                                       const int64_t* segs_long, int nlong, int subseq_bytes, const void* tabsets, int16_t* coef,
                                       uint8_t* planes, int64_t coef_count, int32_t* status, int64_t* stats, uint8_t* image, int width,
                                       int height, int bands, int block_w, int block_h, int blocks_across, void* stream);
/* td_jpeg_decode with every entropy-coded segment decoded by that window procedure on one host thread, `lanes` (1 .. 64) emulated
 * lanes walking subsequences of subseq_bytes bytes: the same bytes and the same errors as td_jpeg_decode. stats (int64 [4], may be
 * NULL) receives what td_tiff_jpeg_decode_long_dev counts. */
int64_t td_jpeg_decode_sync(const uint8_t* src, int64_t n, uint8_t* dst, int64_t cap, int32_t* shape, int subseq_bytes, int lanes,
                            int64_t* stats);
/* Window of an uncompressed pixel-interleaved raster with contiguous strips (the tile windows of reference
 * prediction.py:164, rasterio.mask.mask(..., crop=True)): `rows` pieces of `row_bytes` bytes lying `row_stride` bytes apart
 * from `file_off` on, read with pread(2) into the dense buffer dst (e.g. pinned staging memory). Returns the bytes read or
 * TD_ERR_INVALID (bad argument, read error, file shorter than the window). Thread-safe (no file position is used). */
int64_t td_read_window(int fd, int64_t file_off, int64_t row_stride, int64_t row_bytes, int64_t rows, uint8_t* dst);
/* The windows of a whole batch in one call: window i = rows[i] pieces of row_bytes[i] bytes lying row_stride apart from file_off[i],
 * read into dst + dst_off[i]; the windows are cut into row bands and spread over `threads` host threads. Returns the bytes read or
 * TD_ERR_INVALID. */
int64_t td_read_windows(int fd, int n, const int64_t* file_off, int64_t row_stride, const int64_t* row_bytes, const int64_t* rows,
                        uint8_t* dst, const int64_t* dst_off, int threads);
/* Undo TIFF predictor 2 (horizontal differencing) in place on one decoded block of rows x cols pixels with
 * `samples` interleaved samples of 1, 2 or 4 bytes (host byte order). */
int td_tiff_unpredict(void* data, int64_t rows, int64_t cols, int samples, int bytes_per_sample);
/* Undo TIFF predictor 3 (floating-point predictor, TIFF Technical Note 3; libtiff's fpAcc) in place on one decoded block of
 * rows x cols pixels with `samples` interleaved samples of bytes_per_sample == 4 bytes. A row of n = cols * samples floats is
 * stored as 4n bytes: a byte-wise running sum modulo 256 with stride `samples` runs over ALL of them (across the plane
 * boundaries), then the bytes are four planes of n, most significant first — in every file, whatever its byte order. The
 * result is floats in host byte order. TD_ERR_INVALID for a null pointer or another sample size. */
int td_tiff_unpredict_float(void* data, int64_t rows, int64_t cols, int samples, int bytes_per_sample);

/* The same file text from contours traced on the device: points / det_info / contour_info are ONE image's slices of the
 * td_trace_contours_dev outputs, copied to the host. Detections the device left to the host (status != 0) are traced
 * from mask_bits as above; when such a detection exists and mask_bits is NULL the call returns TD_ERR_STATE and the
 * caller repeats it with the image's mask rows. Byte-identical to td_tile_polygons_json on the same masks. */
int td_tile_polygons_json_dev(const int16_t* points, int64_t points_cap, const int32_t* det_info, const int32_t* contour_info,
                              const int32_t* mask_region, const int64_t* mask_offset, const uint32_t* mask_bits,
                              int64_t mask_words, const float* scores, const int32_t* classes, int n,
                              const double* transform, const char* image_id, char* buf, int64_t cap, int64_t* needed);

/* ---- stitching consumer of the prediction files (reference helpers.py:419-476) -------------- */
/* `geometry.simplify(tolerance, preserve_topology=True)` (helpers.py:464-465) for one closed shell ring:
 * topology-preserving Douglas-Peucker as GEOS' TopologyPreservingSimplifier performs it. xy = n (x,y) pairs,
 * first == last for a ring; writes the kept vertices (a subsequence, closed again) to out_xy (capacity out_cap
 * pairs) and returns their number (>= 4 for a ring of >= 4 points), or a negative status. Host code only. */
int td_simplify_ring(const double* xy, int n, double tolerance, double* out_xy, int out_cap);

/* OGC validity of one closed polygon shell (n points, first == last) as GEOS decides it: 1 valid, 0 invalid (self-touching,
 * self-crossing, spikes, fewer than three distinct points, non-finite coordinates), < 0 error. Replaces `geom.is_valid` on the
 * fused crowns, reference TreeDetection/helpers.py:816,819. Host code. */
int td_ring_is_valid(const double* xy, int n);
/* One tile's prediction file → the features it contributes to the image's layer (helpers.py:436-470,
 * process_prediction_file_sync): parse the JSON array the predictor wrote (`json` / `len`, UTF-8 text), take
 * "score" and "polygon_coords" of every entry (coordinates flattened and paired like reshape(-1, 2); fewer than 4
 * points or a missing key fail the whole file, as the reference's exception path does), simplify the ring
 * (tolerance > 0), keep it when it lies `within` box = (minx, miny, maxx, maxy), and encode it as a GeoPackage
 * geometry blob (header with envelope + `srs_id`, little-endian WKB polygon). Feature i = blobs[blob_offsets[i] ..
 * blob_offsets[i+1]) with scores[i]. Returns the feature count; TD_ERR_CAPACITY (needed_bytes / needed_features
 * say how much) when a buffer is too small; TD_ERR_INVALID for malformed input. Host code only, thread-safe. */
int td_stitch_tile_json(const char* json, int64_t len, const double* box, double tolerance, int32_t srs_id,
                        uint8_t* blobs, int64_t blob_cap, int64_t* blob_offsets, double* scores, int max_features,
                        int64_t* needed_bytes, int* needed_features);

/* The same for a whole image in ONE call (reference helpers.py:524-554 process_folder_sync: every tile file of the image's
 * prediction folder): file i = the NUL-terminated path at paths + path_offsets[i] with its own box (boxes[4 i ..]) and
 * srs_ids[i]; the files are read, parsed, simplified, filtered and encoded on `threads` host threads and the features come
 * back concatenated in FILE order (feature numbering as in td_stitch_tile_json, blob_offsets has total + 1 entries).
 * file_status[i] = features of file i, or the negative status that file failed with — such a file is left out, as the
 * reference's per-file try / except leaves it out (helpers.py:419-476). Returns the total feature count; TD_ERR_CAPACITY
 * (needed_bytes / needed_features) when a buffer is too small. Host code only. */
int td_stitch_tile_files(const char* paths, const int64_t* path_offsets, int n_files, const double* boxes, double tolerance,
                         const int32_t* srs_ids, int threads, uint8_t* blobs, int64_t blob_cap, int64_t* blob_offsets,
                         double* scores, int max_features, int32_t* file_status, int64_t* needed_bytes, int* needed_features);

/* ---- outline predicates (reference helpers.py:703-834 fuse_predictions; preprocessing.py:70-95 tile flags) ---- */
/* Relates query rings to a region given as polygons with holes (the outline file's geometries, NOT unioned):
 * ring r = ring_xy[ring_start[r] .. ring_start[r+1]) (x,y pairs, closed), ring_poly[r] = polygon it belongs to,
 * rings of one polygon consecutive with the shell first. For each closed query ring q:
 *   flags[q] bit 0 = query.intersects(union of the polygons), bit 1 = query.within(union of the polygons)
 * (shapely/GEOS semantics for a simple query ring; exact-sign arithmetic). Host code only. */
int td_region_relate(const double* ring_xy, const int64_t* ring_start, const int32_t* ring_poly, int n_rings,
                     const double* query_xy, const int64_t* query_start, int n_queries, uint8_t* flags);

/* The same predicates on the device (csrc/regionrelate.hip; the arithmetic of csrc/geom_predicates.h on both sides, so flags[q] equals
 * td_region_relate's for every query it decides). Every pointer is DEVICE memory; ring_xy and query_xy 16-byte aligned.
 *   region: ring_xy / ring_start / ring_poly as above (n_vertices = ring_start[n_rings] < 2^31 - 1, ring_poly not decreasing) and
 *   edge_ring int32 [n_vertices], the ring of each vertex. Edge id = index of the edge's first vertex.
 *   index: the y-bins of td_region_relate — bin b = floor((y - ymin) * inv_h) clamped to [0, n_bins) — as bin_start int32
 *   [n_bins + 1] into bin_edges int32 [n_bin_edges]: the ids of the edges whose y-range touches the bin, ascending; ymin / ymax the
 *   region's y-range.
 *   queries: closed rings, query_start int64 [n_queries + 1] into query_xy (n_query_vertices points).
 * Out: flags uint8 [n_queries] (bit 0 intersects, bit 1 within, as above), status int32 [n_queries]:
 *   0 decided; 1 NOT decided (flag 0) because a fixed capacity of the kernel was exceeded — more than TD_RELATE_QUERY_CAP points in
 *   the ring, more than TD_RELATE_MEET_CAP meetings of ONE query edge with region edges, or more than TD_RELATE_RING_CAP distinct
 *   region rings met by the query — td_region_relate decides such a query; 2 refused (flag 0): fewer than 4 points, not closed, a
 *   non-finite coordinate, a start outside query_xy.
 * One wave per query, one launch for any n_queries, asynchronous on `stream`; no query is half-decided. The kernel checks every id it
 * takes from the index against n_vertices / n_rings / n_bin_edges before it addresses anything, so no index content makes it read
 * outside the arrays; the ANSWERS need a consistent index. With check_index != 0 the call first verifies that on the device
 * (bin_start rising within bin_edges, every edge id inside the edge array and inside the ring edge_ring names, ids ascending per
 * bin, ring_poly not decreasing), waits for the verdict and returns TD_ERR_INVALID without launching the predicates when it fails:
 * pass it once per uploaded index. TD_ERR_INVALID (before anything runs) for a null pointer, a bad count, a non-finite y-range or a
 * misaligned xy; n_queries = 0 returns TD_OK and launches nothing. */
#define TD_RELATE_QUERY_CAP 256   /* points of a query ring, the closing one included */
#define TD_RELATE_MEET_CAP 254    /* meeting parameters of one query edge (a collinear overlap counts two) */
#define TD_RELATE_RING_CAP 64     /* distinct region rings one query meets */
td_status td_region_relate_dev(const double* ring_xy, const int64_t* ring_start, const int32_t* ring_poly, int n_rings, int64_t n_vertices,
                               const int32_t* edge_ring, const int32_t* bin_start, const int32_t* bin_edges, int n_bins,
                               int64_t n_bin_edges, double ymin, double ymax, double inv_h, const double* query_xy,
                               const int64_t* query_start, int n_queries, int64_t n_query_vertices, uint8_t* flags, int32_t* status,
                               int check_index, void* stream);

/* ---- crown post-processing (reference postprocessing.py:25-347) ----------------------------- */
/* Raster statistics inside each crown's bounding circle. raster: device float32 [rows][cols]; transform: host
 * (a,b,c,d,e,f) of the raster; window: host (row_lo, col_lo, row_hi, col_hi) = the reference's subset of the raster
 * (its whole extent when the bounds passed are the raster's own); circles: device float32 [n][3] (centre x, y of
 * the crown's bounding box and the largest vertex distance from it, computed from the float32 vertex arrays).
 * mode 0 (get_height_within_polygon): out [n][3] = max value, x, y of its first occurrence (float64 membership test);
 * mode 1 (get_ndvi_within_polygon / NDVI half of get_metadata_within_polygon with radius_scale 0.5): out [n][4] =
 * min, max, mean, population variance (float32 membership test). -1 everywhere for a circle without pixels.
 * Asynchronous on `stream`. */
td_status td_crown_stats(const float* raster, int rows, int cols, const double* transform, const int32_t* window,
                         const float* circles, int n, int mode, float radius_scale, float* out, void* stream);

/* Zonal statistics: the same per-crown statistics over the pixels inside the crown's OUTLINE instead of its bounding circle
 * (config crown_statistics: polygon; csrc/crown_zonal.h is the rule, shared by both functions). raster: float32 [rows][cols], the
 * whole raster, fewer than 2^31 pixels; transform: HOST (a,b,c,d,e,f), finite. Rings arrive open (without the repeated closing
 * vertex), concatenated, as for td_ring_pairs_area: xy = n_xy (x, y) pairs, start int64 [n + 1] with crown q in
 * [start[q], start[q + 1]). Exterior rings only, either winding.
 * Pixel (row, col) has the centre P.x = (a*(col+0.5) + b*(row+0.5)) + c, P.y = (d*(col+0.5) + e*(row+0.5)) + f in float64, every
 * operation rounded on its own, and belongs to the crown iff P lies inside the closed ring or on it: even-odd over all edges (a
 * ring that crosses itself is not an error), half-open in y, every sign exact (csrc/geom_predicates.h).
 * Out, per crown: out float32 [n][4] = min, max, mean, population variance of the pixels inside (float64 sums, the variance in a
 * second pass about the float64 mean, each rounded once); pos int32 [n][3] = their count, raster row and column of the maximum.
 * A NaN inside makes min, max, mean and variance NaN and the position that of the FIRST NaN in row-major order; among numbers the
 * first occurrence of the maximum is reported and the minimum carries the sign of the first of equal zeros (numpy's order, as
 * td_crown_stats).
 * status int32 [n]: 0 computed — a crown with no pixel centre inside has count 0, out -1 in all four fields, both positions -1.
 * 1 (device only): more than TD_ZONAL_RING_CAP vertices, the wave's LDS region — not computed (out NaN, pos -1); td_crown_zonal
 * computes such a crown. 2 refused (out NaN, pos -1): fewer than 3 vertices, a non-finite coordinate, start[q] < 0,
 * start[q + 1] < start[q] or start[q + 1] > n_xy (checked in the kernel before any vertex is read).
 * td_crown_zonal_dev: raster, xy, start, out, pos, status are DEVICE memory, xy 16-byte aligned; one wave per crown, a bounded grid
 * with a grid-stride loop (any n is one launch); asynchronous on `stream`. td_crown_zonal: HOST memory, host code, no vertex cap;
 * status, count, min, max and position equal the device's bit for bit, mean and variance are sums in another order. Both return
 * TD_ERR_INVALID (with a message, before anything runs) for a null pointer, n < 0 or n_xy < 0, rows or cols < 1 or 2^31 pixels and
 * more, a non-finite transform or a misaligned xy; n = 0 returns TD_OK and launches nothing. */
#define TD_ZONAL_RING_CAP 512    /* vertices of an open ring the kernel holds */
td_status td_crown_zonal_dev(const float* raster, int rows, int cols, const double* transform, const double* xy, int64_t n_xy,
                             const int64_t* start, int n, float* out, int32_t* pos, int32_t* status, void* stream);
td_status td_crown_zonal(const float* raster, int rows, int cols, const double* transform, const double* xy, int64_t n_xy,
                         const int64_t* start, int n, float* out, int32_t* pos, int32_t* status);

/* Crown label raster: the inverse question — which crown owns this pixel. The grid (rows, cols, HOST transform), the rings (xy,
 * n_xy, start, n) and pixel membership are td_crown_zonal's above, unchanged (csrc/crown_zonal.h: pixel_centre, point_in_query,
 * pixel_box as the search box). value: uint32 [n], one per ring; labels: uint32 [rows][cols]. The rule:
 *   labels[r][c] = max( labels_before[r][c], max{ value[q] : status[q] == 0 and the centre of (r, c) belongs to ring q } )
 * The call does NOT clear labels — the caller does —, so several calls, and the host function after the device one, composite
 * into one raster. The maximum is unsigned and does not depend on the order of the rings or of the waves that draw them: the
 * raster is reproducible bit for bit and the same from both functions for any values, equal ones and values >= 2^31 included. A
 * value of 0 changes nothing.
 * status int32 [n]: 0 drawn (a crown with no pixel centre inside draws nothing). 1 (device only): more than TD_ZONAL_RING_CAP
 * vertices — nothing drawn; td_crown_labels draws such a crown. 2 refused, nothing drawn: fewer than 3 vertices, a non-finite
 * coordinate, start[q] < 0, start[q + 1] < start[q] or start[q + 1] > n_xy (checked in the kernel before any vertex is read).
 * td_crown_labels_dev: xy, start, value, labels, status are DEVICE memory, xy 16-byte aligned; one wave per crown, a bounded grid
 * with a grid-stride loop, one relaxed agent-scope atomic maximum per pixel inside (csrc/crownzonal.hip); asynchronous on `stream`.
 * td_crown_labels: HOST memory, host code, no vertex cap. Both return TD_ERR_INVALID (with a message, before anything runs) for a
 * null pointer, n < 0 or n_xy < 0, rows or cols < 1 or 2^31 pixels and more, a non-finite transform or a misaligned xy; n = 0
 * returns TD_OK and launches nothing. */
td_status td_crown_labels_dev(int rows, int cols, const double* transform, const double* xy, int64_t n_xy, const int64_t* start,
                              const uint32_t* value, int n, uint32_t* labels, int32_t* status, void* stream);
td_status td_crown_labels(int rows, int cols, const double* transform, const double* xy, int64_t n_xy, const int64_t* start,
                          const uint32_t* value, int n, uint32_t* labels, int32_t* status);

/* Treetops in a height raster (reference supplementary/pretraining_generate_voronoi.py:32-74, 294-320: gaussian_filter, then the
 * local maxima of a maximum_filter above a height; csrc/treetops.h is the rule, shared by both functions). raster: float32
 * [rows][cols], fewer than 2^31 pixels. weights: HOST float64 [2 * radius + 1], the normalised 1-D Gaussian as scipy builds it, built
 * by the caller (no exp of the C library or the device enters the result); finite and symmetric. radius = 0 with weights = [1.0]:
 * no smoothing. window: odd k >= 1, h = k / 2. floor: float32, not NaN.
 * Smoothing: two 1-D passes, axis 0 first, then axis 1, each output rounded to float32 once; an index outside [0, n) is reflected
 * (d c b a | a b c d | d c b a: p = 2n, i = i mod p, i = p - 1 - i if i >= n; any n). One output, in float64, multiply and add
 * rounded separately:  t = in[l] * w[r];  for ii = -r .. -1: t = t + (in[l+ii] + in[l-ii]) * w[r+ii];  out[l] = (float)t  —
 * scipy.ndimage.gaussian_filter (float32 in and out) bit for bit.
 * Treetop: with s the smoothed raster, pixel (row, col) is one iff s > floor and s >= s' for every non-NaN s' among the in-range
 * pixels of the k x k window centred on it; a NaN s never is; every pixel of a plateau that equals its window maximum is. With
 * NaN-free s this is argwhere((s == maximum_filter(s, size=k)) & (s > floor)). The reference applies maximum_filter to a copy with
 * NaN where s <= 2.5 instead, which differs only where a NaN enters a window and there depends on scipy's comparison order.
 * Out: marks uint8 [rows][cols] = 1 / 0, every pixel written; smoothed float32 [rows][cols] when non-null (a NaN is a NaN: its
 * sign and payload are not part of the rule); counts int32 [rows] when non-null = the marks of each row.
 * td_treetops_dev: raster, marks, smoothed, counts are DEVICE memory; one launch, a workgroup per output tile (64 x 64, or 32 x 32
 * when radius + h > 13), the raw tile with its halo of radius + h staged in LDS, both passes and the separable maximum there — no
 * smoothed raster travels through memory between the passes; counts is zeroed on `stream` by the call and receives one atomic add
 * per tile row that holds a treetop; radius <= TD_TREETOP_RADIUS_CAP and window <= TD_TREETOP_WINDOW_CAP (at most 64 KB of LDS);
 * asynchronous on `stream`. td_treetops: HOST memory, host code, any radius and window; marks and smoothed equal the device's bit
 * for bit. Both return TD_ERR_INVALID (with a message, before anything runs) for a null raster, weights or marks, rows or cols < 1
 * or 2^31 pixels and more, an even window or window < 1, radius < 0, a non-finite or asymmetric weight table, a NaN floor and, on
 * the device, a parameter over its cap. */
#define TD_TREETOP_RADIUS_CAP 8
#define TD_TREETOP_WINDOW_CAP 15
td_status td_treetops_dev(const float* raster, int rows, int cols, const double* weights, int radius, int window, float floor,
                          uint8_t* marks, float* smoothed, int32_t* counts, void* stream);
td_status td_treetops(const float* raster, int rows, int cols, const double* weights, int radius, int window, float floor,
                      uint8_t* marks, float* smoothed, int32_t* counts);

/* GDAL's separable triangle-filter resampling (src.read(out_shape=..., resampling=bilinear), reference postprocessing.py:781-797)
 * of a raster that lies in device memory, with the NDVI rule of helpers.ndvi_array_from_rgbi (880-895) fused into the second pass.
 * src: DEVICE uint8 [height][width][c] pixel-interleaved (TD_SAMPLE_U8, c <= 4) or DEVICE float32 [height][width] (TD_SAMPLE_F32,
 * c = 1). bands: HOST list of n_bands <= 4 band indices < c — only these are computed. The filter taps are the caller's, one table
 * per axis in DEVICE memory: output j of the axis is the sum over k < count[j] of sample[start[j] + k] * weights[offset[j] + k],
 * accumulated in float32 in ascending k, multiply and add rounded separately; start / count / offset int32 [n_dst] (n_dst = out_w
 * for the x tables, out_h for the y tables), weights float32 [n_weights]. The caller guarantees start >= 0, count >= 1,
 * start + count <= the source size of the axis and offset + count <= n_weights (device memory is not read by the checks of this
 * call; the kernels ignore what lies outside). tmp: DEVICE float32 [n_bands][height][out_w], the first pass's result.
 * dst by mode: TD_RESAMPLE_F32 float32 [n_bands][out_h][out_w]; TD_RESAMPLE_U8 uint8 [n_bands][out_h][out_w] =
 * clip(floor(v + 0.5), 0, 255); TD_RESAMPLE_NDVI (exactly two bands: red, near-infrared) float32 [out_h][out_w] = both rounded to
 * uint8 as in mode u8, then (nir / 255 - red / 255) / (nir / 255 + red / 255 + 1e-10) in float64, rounded once. Modes u8 and ndvi
 * take uint8 sources only. Returns TD_ERR_INVALID (with a message, before any launch) for a null pointer, a bad shape, sample type
 * or mode, a band index >= c, or a mode / band count / sample type combination outside the above. Asynchronous on `stream`. */
enum { TD_SAMPLE_U8 = 0, TD_SAMPLE_F32 = 1, TD_SAMPLE_U16 = 2 };    /* (U16: td_seam_first_dev only) */
enum { TD_RESAMPLE_F32 = 0, TD_RESAMPLE_U8 = 1, TD_RESAMPLE_NDVI = 2 };
td_status td_resample_gdal_dev(const void* src, int sample_type, int height, int width, int c, const int32_t* bands, int n_bands,
                               const int32_t* x_start, const int32_t* x_count, const int32_t* x_offset, const float* x_weights,
                               int out_w, int64_t x_n_weights, const int32_t* y_start, const int32_t* y_count,
                               const int32_t* y_offset, const float* y_weights, int out_h, int64_t y_n_weights, float* tmp,
                               void* dst, int mode, void* stream);

/* ---- the crown stage's box-pair filters (reference postprocessing.py:349-476) without their N x N matrices ----
 * boxes: DEVICE float32 [n][4] (x1, y1, x2, y2), 16-byte aligned; areas_f16: DEVICE float16 [n], the polygon areas. All arithmetic is
 * the reference's, each operation rounded on its own: connected(i, j) = iou > iou_threshold in float32 (inter / ((area_i + area_j) -
 * inter), IEEE division) AND |a_i - a_j| / max(a_i, a_j) < area_threshold_f16 on the float16 areas, rounded to half after every
 * operation as numpy does (thresholds: a float32 and a float16 bit pattern); containment ratio[i][j] = inter / area_j in float32,
 * compared >= containment_threshold. Pairs of disjoint boxes are skipped, which changes nothing when every coordinate is finite,
 * every float32 box area finite and positive, iou_threshold >= 0 and containment_threshold > 0 — the CALLER's preconditions, not
 * checked here (device memory is not read by the checks of these calls).
 * td_crown_pairs_count: counts int32 [n] = connected j != i per row (NULL: containment only; needs areas_f16 otherwise);
 * num_contained int32 [n] = j != i with ratio[i][j] >= threshold and is_contained int32 [n] = 0 / 1, any i' != i with
 * ratio[i'][i] >= threshold (both NULL: de-duplication only). The outputs are zeroed on `stream` by the call.
 * td_crown_pairs_fill: row_start DEVICE int64 [n + 1] = exclusive prefix sum of counts; cols int32 [row_start[n]] receives the
 * connected column indices of row i in [row_start[i], row_start[i + 1]), in no particular order; cursor: int32 [n] of scratch.
 * Same boxes, areas and thresholds as the count pass, which ran the same pair test.
 * Both return TD_ERR_INVALID (with a message, before any launch) for a null pointer, a misaligned boxes pointer, n < 1 or
 * n > 67 107 840 (65 535 column chunks of 1 024 crowns, the launch grid's second dimension).
 * Asynchronous on `stream`. */
td_status td_crown_pairs_count(const float* boxes, const uint16_t* areas_f16, int n, float iou_threshold, uint16_t area_threshold_f16,
                               int32_t* counts, float containment_threshold, int32_t* num_contained, int32_t* is_contained,
                               void* stream);
td_status td_crown_pairs_fill(const float* boxes, const uint16_t* areas_f16, int n, float iou_threshold, uint16_t area_threshold_f16,
                              const int64_t* row_start, int32_t* cursor, int32_t* cols, void* stream);
/* The greedy pass of the de-duplication over those rows (HOST memory throughout, host code, O(n + edges)): rows in index order; a
 * removed row is skipped; of a row's members and the row itself the one with the highest float16 confidence (conf_f16: bit
 * patterns, no NaN) stays and every other one is marked in removed uint8 [n] (removed members still vote in later groups). Ties
 * go as the reference's argmax over "ascending members, then the row itself" does: the smallest index among the members; the row
 * itself takes part at its own index when the mask's diagonal holds for it (self_connected uint8 [n]; NULL = it holds for every
 * row; a row that lists itself in cols says the same) and otherwise wins only when strictly higher. The order inside a row does
 * not matter. TD_ERR_INVALID for a null pointer, n < 0, a decreasing row_start or a column outside [0, n). */
int td_crown_pairs_greedy(const int64_t* row_start, const int32_t* cols, const uint16_t* conf_f16, const uint8_t* self_connected,
                          int n, uint8_t* removed);

/* ---- polygon IoU of crown pairs (clean_crowns: reference helpers.py:602-701, utilities.calc_iou 209-212) ----
 * For every pair (pairs int32 [n_pairs][2]: a ring index into set A, one into set B) the area of the intersection of the two
 * simple rings and the two ring areas: out float64 [n_pairs][3] = inter, |area_A|, |area_B|; status int32 [n_pairs]. Rings arrive
 * open (without the repeated closing vertex), concatenated: xy = (x, y) pairs, start int64 [n + 1] with ring r in
 * [start[r], start[r + 1]) — non-decreasing from >= 0 and inside xy: the CALLER's guarantee. Exterior rings only, either winding.
 * Arithmetic (csrc/ring_clip.h, float64, every operation rounded on its own, IEEE division): the fan decomposition about
 * O = the centre of the intersection of the two rings' float64 bounding boxes — inter = sigma_A sigma_B sum_i sum_j sgn(s_i)
 * sgn(t_j) area(tri(O, a_i, a_i+1) n tri(O, b_j, b_j+1)) on the vertices v - O, each term a triangle clipped by three half-planes;
 * term t = i * n_b_vertices + j is added by lane t mod 64 in ascending t and the 64 partial sums meet in a butterfly over xor 32,
 * 16, 8, 4, 2, 1; the ring areas are the shoelace sums on v - O in the same lane order. A box intersection of non-positive width
 * or height gives inter = +0 without a clip; inter is clamped to [0, min(|area_A|, |area_B|)].
 * status 0: computed. status 1 (device only): the two rings together have more than 1 024 vertices, the wave's LDS region — not
 * computed, out is NaN; td_ring_pairs_area computes such a pair. status 2: refused, out is NaN — a pair index outside [0, n_a) /
 * [0, n_b) (checked in the kernel: no ring memory is touched), a ring of fewer than 3 vertices, a non-finite coordinate.
 * td_ring_pairs_area_dev: every pointer is DEVICE memory, xy_a / xy_b 16-byte aligned; one wave per pair, a bounded grid with a
 * grid-stride loop (any n_pairs is one launch); asynchronous on `stream`. td_ring_pairs_area: HOST memory, host code, the wave's
 * lanes emulated — its results equal the device's bit for bit; no vertex cap. Both return TD_ERR_INVALID (with a message, before
 * anything runs) for a null pointer, a negative count or a misaligned xy; n_pairs = 0 returns TD_OK and launches nothing. */
td_status td_ring_pairs_area_dev(const double* xy_a, const int64_t* start_a, int n_a, const double* xy_b, const int64_t* start_b,
                                 int n_b, const int32_t* pairs, int64_t n_pairs, double* out, int32_t* status, void* stream);
td_status td_ring_pairs_area(const double* xy_a, const int64_t* start_a, int n_a, const double* xy_b, const int64_t* start_b, int n_b,
                             const int32_t* pairs, int64_t n_pairs, double* out, int32_t* status);

/* ---- evaluation against annotated crowns (reference supplementary/evaluation_compute_scores.py) ----
 * Candidate pairs between TWO box sets A and B (csrc/boxpairs_ab.hip, boxpairs_ab_host.cpp). Boxes are float64 [n][4] =
 * (x1, y1, x2, y2). THE PAIR RULE: (i, j), i in A and j in B, is a pair iff
 *     min(x2_i, x2_j) > max(x1_i, x1_j)  and  min(y2_i, y2_j) > max(y1_i, y1_j)
 * — an overlap of positive area — decided by comparisons alone: every upper coordinate of the two boxes exceeds every lower one
 * of the same axis (x2_i > x1_i, x2_j > x1_j, x2_i > x1_j, x2_j > x1_i, likewise y). Nothing is rounded; a NaN coordinate fails
 * every comparison, so its box pairs with nothing; touching boxes and boxes of zero width or height pair with nothing. The
 * device calls and the host call give the same set for any input.
 * td_box_pairs_ab_count: boxes_a, boxes_b, counts are DEVICE memory, the boxes 16-byte aligned; counts int32 [n_a] = pairs of row
 * i, zeroed on `stream` by the call. td_box_pairs_ab_fill: row_start DEVICE int64 [n_a + 1] = exclusive prefix sum of counts; cols
 * int32 [row_start[n_a]] receives the column indices of row i in [row_start[i], row_start[i + 1]), in no particular order; cursor:
 * int32 [n_a] of scratch, zeroed on `stream` by the call. Same boxes as the count pass, which ran the same test. 256 rows of A per
 * workgroup against chunks of 1 024 boxes of B in LDS. Both return TD_ERR_INVALID (with a message, before any launch) for a null
 * pointer, misaligned boxes, n_a < 1 or n_b < 1, or more than 67 107 840 boxes on a side (65 535 column chunks, the launch
 * grid's second dimension). Asynchronous on `stream`.
 * td_box_pairs_ab: HOST memory, host code (a sweep over B sorted by x1); counts int32 [n_a]; when cols is non-null the column
 * indices of row i follow those of row i - 1 in cols, ASCENDING within the row; TD_ERR_CAPACITY when they exceed cols_cap
 * entries (call once with cols = NULL for the counts). n_a = 0 or n_b = 0 is served. TD_ERR_INVALID for a null pointer or a
 * negative count. */
td_status td_box_pairs_ab_count(const double* boxes_a, int n_a, const double* boxes_b, int n_b, int32_t* counts, void* stream);
td_status td_box_pairs_ab_fill(const double* boxes_a, int n_a, const double* boxes_b, int n_b, const int64_t* row_start,
                               int32_t* cursor, int32_t* cols, void* stream);
td_status td_box_pairs_ab(const double* boxes_a, int n_a, const double* boxes_b, int n_b, int32_t* counts, int32_t* cols,
                          int64_t cols_cap);
/* The matching loop of the reference's calculate_iou over a sparse IoU matrix (HOST memory throughout, host code, O(m + entries)):
 * CSR rows over the m predictions — row_start int64 [m + 1] from 0, cols int32 = annotation indices in [0, n), iou float64, no
 * NaN. Predictions are walked in index order; a prediction with selected[i] == 0 is passed over; a selected one takes, of its
 * entries whose annotation is still unmatched, the one with the largest IoU (the lowest annotation index among equal IoUs,
 * whatever order the row is stored in) when that IoU is >= t, and stays unmatched otherwise. Out: match_of_pred int32 [m] = the
 * annotation index or -1, match_iou float64 [m] (0 where unmatched), ann_matched uint8 [n]. TD_ERR_INVALID for a null pointer, a
 * negative count, row_start[0] != 0, a decreasing row_start, a column outside [0, n), a NaN IoU or t outside (0, 1]. */
int td_match_greedy(const int64_t* row_start, const int32_t* cols, const double* iou, const uint8_t* selected, int m, int n, double t,
                    int32_t* match_of_pred, double* match_iou, uint8_t* ann_matched);

/* ---- seam strips (reference helpers.py merge_images 1023-1051 + crop_image 1053-1085; csrc/seam.hip) ----
 * The strip [rows][cols][spp] (DEVICE, dense, aligned to its samples; TD_SAMPLE_U8, TD_SAMPLE_U16 or TD_SAMPLE_F32, 1 <= spp <= 4)
 * that the centre crop of rasterio.merge's "first" mosaic of two rasters holds, from up to two source buffers in one launch, without
 * the mosaic. Per SAMPLE: d = fill; then for `first`, then `second`: where the pixel lies in the source's rectangle, equals(d, fill)
 * and not (has_own and equals(s, own)), d = s. equals: exact for the integer types; float32: isnan(a) when the value is NaN, else
 * (|a - (float)v| <= (float)(1e-8 + 1e-5 |v|) and isfinite(v)) or a == (float)v, subtraction and comparisons in float32, float32
 * subnormals kept — numpy.isclose(float32 array, python float) as treedetection_amd.merging._equals calls it.
 * A source: `data` DEVICE samples of the strip's type, pixel-interleaved, `rows` buffer rows of `pitch` PIXELS; (row0, col0) = the
 * strip coordinates of its pixel (0, 0), negative where the buffer begins above / left of the strip; rows r_lo..r_hi and columns
 * c_lo..c_hi (half-open, inside the strip AND inside the buffer) = the rectangle it may fill — the caller clips it as merge_images
 * clips the footprint; has_own / own = its own nodata. A NULL source, NULL data or an empty rectangle contributes nothing.
 * fill and own are given as doubles; for the integer types they must be values of the type. Lanes store 16 bytes at aligned
 * addresses and load 16 bytes, dwords or single samples as the source address of the row allows. Returns TD_ERR_INVALID (with a
 * message, before the launch) for a null or misaligned pointer, a bad shape or sample type, or a rectangle that leaves the strip or
 * its buffer. Asynchronous on `stream`. */
typedef struct td_seam_source {
    const void* data;
    int64_t pitch;
    int32_t rows;
    int32_t row0, col0;
    int32_t r_lo, c_lo, r_hi, c_hi;
    int32_t has_own;
    double own;
} td_seam_source;
td_status td_seam_first_dev(void* strip, int rows, int cols, int spp, int sample_type, double fill, const td_seam_source* first,
                            const td_seam_source* second, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TREEDET_H */
