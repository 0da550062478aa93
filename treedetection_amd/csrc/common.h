// Shared declarations of libtreedet_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <cstdint>
#include <cstddef>
#include "../../include/treedet.h"
#include "conv_path.h"
#include "launch_cost.h"
#include <string>
#include <vector>

void td_set_error(const char* fmt, ...);

// epilogue.cpp: the text of one tile's prediction file from its packed rows on the host; returns the entry count or < 0
int td_polygons_json_text(const int32_t* mask_region, const int64_t* mask_offset, const uint32_t* mask_bits, int64_t mask_words,
                          const float* scores, const int32_t* classes, int n, const double* transform, const char* image_id,
                          std::string& out, const char* who);

#define TD_HIP_CHECK(expr)                                                                         \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess) {                                                                    \
            td_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            return TD_ERR_HIP;                                                                     \
        }                                                                                          \
    } while (0)

#define TD_REQUIRE(cond, ...)            \
    do {                                 \
        if (!(cond)) {                   \
            td_set_error(__VA_ARGS__);   \
            return TD_ERR_INVALID;       \
        }                                \
    } while (0)

#define TD_KERNEL_CHECK() TD_HIP_CHECK(hipGetLastError())

// tiffdecode.hip: a zeroed work counter for one raster-decode launch on `s` (taken by whole waves) and the device's CU count
td_status td_decode_ticket(hipStream_t s, int** ticket, int* cus);

static inline int td_cdiv(int a, int b) { return (a + b - 1) / b; }
inline bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }     // for pointers read as float4 / double2

// ---- convolution (conv_igemm.hip) -------------------------------------------------------------
struct ConvArgs {
    const void* x;        // NHWC [B,H,W,Cin]
    const void* w;        // [Cout][KH][KW][Cin]
    const float* scale;   // [Cout] or nullptr
    const float* bias;    // [Cout] or nullptr
    const void* res;      // residual or nullptr
    void* y;              // NHWC [B,Ho,Wo,Cout] (out_mode 0) / [B,2Ho,2Wo,Cout/4] (out_mode 1)
    int B, H, W, Cin, Cout, KH, KW, stride, pad, Ho, Wo;
    int res_shift;        // 0: residual same size; 1: residual at half resolution (nearest 2x upsample)
    int relu;
    int out_mode;         // 0 plain, 1 deconv2x2 pixel shuffle: n = (dy*2+dx)*Cq + co, Cq = Cout/4
    int M;                // B*Ho*Wo
    const int* m_dyn;     // optional device scalar: effective rows = min(M, *m_dyn * m_mul - m_off)
    int m_mul;
    int m_off;            // rows of the dynamic count that belong to earlier launches (Winograd slabs); 0 otherwise
    int out_f32;          // fp16 path only: write y as float32 (RPN / box-predictor heads feed the fp32 selection kernels)
    // batched launch (blockIdx.y = 0 .. batch_count-1): per-batch element offsets of x / w / y. Used by the Winograd path,
    // whose 16 transform planes are 16 independent 1x1 contractions (winograd.hip). 0 / 1 = a plain launch.
    int batch_count;
    long long x_bs, w_bs, y_bs;
    const void* w_frag;   // the same filters in MFMA fragment order (the tiles with ConvTile::frag), or nullptr
    const void* w_split;  // fp32 1x1 / FC filters as three bf16 pieces per weight in fragment order (conv_split_pack; the TILE_SPLIT ids), or nullptr
                          // (batched: the planes' banks concatenated, and w_bs counts BYTES of one plane's bank — conv_split_bank_bytes)
    int tile_cfg;         // -1 = heuristic; else an id of TD_CONV_TILES (engine autotunes)
    int tile_strict;      // 1: a forced tile_cfg this launch cannot run is an error, not a silent switch to the heuristic tile (tests)
    // fused 1x1 head (fp16 engine, block tiles that own all 256 output channels: ConvTile::head): the finished fp16
    // tile — this layer's output — is contracted with head_w [head_n <= 32][Cout = 256] straight from its LDS staging and
    // only head_y [M][head_n] (fp32, + head_b) is written; y is NOT written. The RPN's 3x3 conv + its 15-row head.
    const void* head_w;
    const float* head_b;
    float* head_y;
    int head_n;
    // grouped launch over pyramid levels (conv_pp8_grouped_launch; fp16, 3x3 / stride 1 / pad 1, 256 -> 256): ONE grid whose tiles
    // walk nlev independent problems of the same layer shape on different maps — the FPN's four output convs (own filters per
    // level) or the RPN conv + head on p2..p6 (shared filters). Per level: input, filters, bias, output (or head output), map size.
    int nlev;
    struct Level {
        const void* x;
        const void* w;
        const float* bias;
        void* y;
        float* head_y;
        int H, W, M, tile0;       // M = B*H*W rows; tile0 = index of the level's first 256-row tile in the grid
    } lev[5];
    int ntiles;                   // tiles of all levels
};
// ---- block tiles (ConvArgs::tile_cfg): one row per id. Tune-cache files, tests and profiles/ name tiles by these ids, so an
// id keeps its number and a retired one keeps its row. Adding a tile: a row here and a case in its family's launcher.
// Families: conv_igemm_kernel (conv_igemm.hip:dispatch); conv_pp8_kernel (8 waves, ping-pong phases, DMA 1.5 k-chunks ahead);
// plane_gemm_kernel (persistent walk over the fp32 Winograd planes); conv_bd_kernel (conv_bdirect.hip: filter fragments from the
// fragment-ordered copy straight into registers); conv_bs_kernel (conv_bstat.hip: filter-stationary 1x1, one block per CU);
// conv_split_kernel (conv_split.hip: fp32 1x1 / FC on the bf16 matrix cores, operands as three bf16 pieces — its own rounding: a
// launch runs these ids if and only if it carries ConvArgs::w_split, which the engine sets by a fixed rule on the layer).
enum ConvFamily : unsigned char { TILE_IGEMM, TILE_PP8, TILE_PLANE, TILE_BD, TILE_BS, TILE_RETIRED, TILE_SPLIT };
enum : unsigned char { TILE_F32 = 1 << TD_PRECISION_FP32, TILE_F16 = 1 << TD_PRECISION_FP16, TILE_ANY = TILE_F32 | TILE_F16 };
struct ConvTile {
    ConvFamily family;
    unsigned char variant;      // TILE_BD: conv_bd_launch's variant
    unsigned char prec;         // TILE_F32 / TILE_F16: the precisions it runs
    bool head;                  // owns all 256 output channels as one fp16 tile: a fused head (ConvArgs::head_w) applies
    bool frag;                  // reads the fragment-ordered filter copy (ConvArgs::w_frag)
    signed char tune_rank;      // position in the tuner's order, -1 = never timed
    unsigned char max_ksteps;   // tuner only: at most this many k-steps (KH * KW * Cin / k-chunk), 0 = any
    short min_cout, max_cout;   // tuner only: output channels, 0 = no limit
};
// Tuning order (tune_rank): from the tile that moves the fewest bytes per FLOP to the one that moves the most; a later candidate
// replaces the best so far only when it is more than TD_TUNE_HYST percent faster (default 2): among tiles that tie within the
// measurement noise the one with the larger footprint wins, which keeps the choice (and with it the HBM / L2 traffic the PMC
// passes report) from flipping between runs — fc1 was seen on the 128 x 128 tile in one run and on a 64 x 128 tile (+2 GB of filter
// re-reads per step, same time) in the next.
inline constexpr ConvTile TD_CONV_TILES[] = {
    //  family        var  prec      head   frag  rank kstp cout>=  <=      id: block tile
    {TILE_IGEMM,   0, TILE_ANY, false, false,  5, 0,   0,  0},     //  0: 128x128, 4 waves, 2 LDS stages
    {TILE_IGEMM,   0, TILE_ANY, false, false, 10, 0,   0,  0},     //  1: 128x64
    {TILE_IGEMM,   0, TILE_ANY, false, false, 11, 0,   0,  0},     //  2: 64x128
    {TILE_IGEMM,   0, TILE_ANY, false, false, 16, 0,   0,  0},     //  3: 64x64
    {TILE_IGEMM,   0, TILE_ANY, false, false, -1, 0,   0,  0},     //  4..7: 0..3 with 3 LDS stages (measured no better)
    {TILE_IGEMM,   0, TILE_ANY, false, false, -1, 0,   0,  0},
    {TILE_IGEMM,   0, TILE_ANY, false, false, -1, 0,   0,  0},
    {TILE_IGEMM,   0, TILE_ANY, false, false, -1, 0,   0,  0},
    {TILE_IGEMM,   0, TILE_ANY, false, false, -1, 0,   0,  0},     //  8: 256x128, 8 waves
    {TILE_IGEMM,   0, TILE_ANY, true,  false, -1, 0,   0,  0},     //  9: 128x256, 8 waves
    {TILE_IGEMM,   0, TILE_ANY, true,  false,  1, 0,   0,  0},     // 10: 256x256, 16 waves
    {TILE_IGEMM,   0, TILE_ANY, false, false, -1, 0,   0,  0},     // 11..13: 256x256 with larger per-wave tiles
    {TILE_IGEMM,   0, TILE_ANY, true,  false, -1, 0,   0,  0},
    {TILE_IGEMM,   0, TILE_ANY, true,  false, -1, 0,   0,  0},
    {TILE_IGEMM,   0, TILE_ANY, false, false, -1, 4,   0,  0},     // 14..16: one LDS stage, 256x256 / 128x128 / 128x256 (thin 1x1 layers;
    {TILE_IGEMM,   0, TILE_ANY, false, false,  6, 4,   0,  0},     //   14 / 16 stage their output as fp32 wave-rows: no fused head)
    {TILE_IGEMM,   0, TILE_ANY, false, false,  4, 4,   0,  0},
    {TILE_PP8,     0, TILE_F16, true,  false,  2, 0, 128,  0},     // 17: conv_pp8_kernel 256x256
    {TILE_PLANE,   0, TILE_F32, false, false, 18, 0,   0,  0},     // 18: plane_gemm_kernel 64x128
    {TILE_PLANE,   0, TILE_F32, false, false, 19, 0,   0,  0},     // 19: 128x128
    {TILE_PLANE,   0, TILE_F32, false, false, 20, 0,   0,  0},     // 20: 64x64
    {TILE_RETIRED, 0, 0,        false, false, -1, 0,   0,  0},     // 21, 22: stream-K (retired: measured slower, deleted)
    {TILE_RETIRED, 0, 0,        false, false, -1, 0,   0,  0},
    {TILE_BD,      0, TILE_ANY, true,  true,   8, 0,   0,  0},     // 23: conv_bd_kernel 64x256
    {TILE_BD,      1, TILE_ANY, false, true,  12, 0,   0,  0},     // 24: 64x128
    {TILE_BD,      2, TILE_ANY, false, true,  13, 0,   0,  0},     // 25: 64x128, two k-chunks per barrier
    {TILE_BD,      3, TILE_ANY, false, true,  14, 0,   0,  0},     // 26: 64x128, three k-steps of loads in flight
    {TILE_BD,      4, TILE_ANY, true,  true,   9, 0,   0,  0},     // 27: 64x256, two k-steps in flight
    {TILE_RETIRED, 0, 0,        false, false, -1, 0,   0,  0},     // 28: the 4-wave 256x256 tile
    {TILE_BD,      5, TILE_ANY, true,  true,   3, 0,   0,  0},     // 29: 128x256, three k-steps in flight (half the filter re-reads)
    {TILE_BD,      6, TILE_ANY, false, true,   7, 0,   0,  0},     // 30: 128x128, three k-steps in flight
    {TILE_IGEMM,   0, TILE_ANY, false, false, 15, 0,   0, 32},     // 31: 256x32, 4 x 1 waves (the thin heads)
    {TILE_IGEMM,   0, TILE_ANY, false, false, 17, 0,   0, 32},     // 32: 128x32
    {TILE_BS,      0, TILE_ANY, false, true,   0, 4, 128,  0},     // 33: conv_bs_kernel (its other tuning rules: conv_bs_ok)
    {TILE_SPLIT,   0, TILE_F32, false, false, 21, 0,   0,  0},     // 34: conv_split_kernel 128x256, 1 x 4 waves of 128x64 (ranks 21 - 24: timed for launches with w_split only,
    {TILE_SPLIT,   1, TILE_F32, false, false, 22, 0,   0,  0},     // 35: 128x128               and then nothing else is — tuned_cfg filters by family)
    {TILE_SPLIT,   2, TILE_F32, false, false, 23, 0,   0,  0},     // 36: 64x256
    {TILE_SPLIT,   3, TILE_F32, false, false, 24, 0,   0,  0},     // 37: 64x128, 2 waves (the M = 5 000 layers: twice the blocks of 35)
    // 34 - 37 also run batched launches of plain planes (batch_count > 1, static rows, no residual, w_bs = bytes of one plane's split
    // bank: the unfolded F(4x4) layers' 36 planes); a batched launch with w_split runs no other family (conv_tile_refusal)
};
static inline const ConvTile* conv_tile(int id) { return id >= 0 && id < (int)(sizeof TD_CONV_TILES / sizeof *TD_CONV_TILES) ? &TD_CONV_TILES[id] : nullptr; }
static inline bool conv_head_capable(int id, int precision) { return precision == TD_PRECISION_FP16 && conv_tile(id) && conv_tile(id)->head; }
// nullptr when tile `id` can run this launch, else why not (-1, the heuristic tile, runs every launch)
const char* conv_tile_refusal(int id, const ConvArgs& a, int precision);
td_status conv2d_launch(const ConvArgs& a, int precision, hipStream_t stream);
// a.nlev levels (x / w / bias / y / head_y / H / W filled in; M, tile0, ntiles are computed here) in one conv_pp8_kernel grid;
// everything else (B, Cin, Cout = 256, KH = KW = 3, relu, head_w / head_b / head_n) from the common fields. Bit-identical to one
// conv2d_launch per level on any tile.
td_status conv_pp8_grouped_launch(ConvArgs a, hipStream_t stream);
// filter-direct form (conv_bdirect.hip)
void conv_bd_pack(const void* w_ohwi, int elem_bytes, int cout, int kh, int kw, int cin, std::vector<unsigned char>& out);
bool conv_bd_ok(const ConvArgs& a, int precision);
td_status conv_bd_launch(const ConvArgs& a, int precision, int variant, hipStream_t stream);
// filter-stationary form (conv_bstat.hip, tile id 33)
bool conv_bs_ok(const ConvArgs& a, int precision);
td_status conv_bs_launch(const ConvArgs& a, int precision, hipStream_t stream);
// split-bf16 form (conv_split.hip, tile ids 34 - 37): w [cout][cin] fp32 → the three-piece fragment bank (6 bytes per weight)
// (taps = 9 with w [cout][3][3][cin]: the 3x3 bank of the split bottleneck tail, k-chunks channel chunk outer / tap inner)
void conv_split_pack(const float* w, int cout, int cin, std::vector<unsigned char>& out, int taps = 1);
// bytes of the split bank of one [cout][cin] plane; a batched launch (batch_count > 1: the 36 planes of an F(4x4) layer, each packed
// on its own and concatenated — conv_split_pack_planes) carries it as w_bs
size_t conv_split_bank_bytes(int cout, int cin);
void conv_split_pack_planes(const float* u, int planes, int cout, int cin, std::vector<unsigned char>& out);
bool conv_split_ok(const ConvArgs& a, int precision);
td_status conv_split_launch(const ConvArgs& a, int variant, hipStream_t stream);
td_status wino_gemm_launch(const ConvArgs& a, hipStream_t stream);     // Winograd plane contractions, input transform fused (fp32)

// ---- fused bottleneck tail (bottleneck.hip): 3x3 (mid -> mid) + BN + ReLU, then 1x1 (mid -> 4 mid) + BN + shortcut + ReLU ----
struct TailArgs {
    const void* x;        // NHWC [B,H,W,MID]: output of the block's first 1x1
    const void* w2;       // [MID][3][3][MID]
    const float* scale2;  // [MID] FrozenBN fold of conv2 (nullptr = 1 / 0)
    const float* bias2;
    const void* w3;       // [COUT][MID]
    const float* scale3;  // [COUT]
    const float* bias3;
    const void* res;      // NHWC [B,H,W,COUT]: the block's shortcut (same size)
    void* y;              // NHWC [B,H,W,COUT]
    int B, H, W, MID, COUT, M;
    // the split form (fp32, MID 64): conv2's bank as three bf16 pieces per weight (conv_split_pack with taps = 9); the 3x3 then runs
    // on the bf16 matrix cores, the 1x1 as before. mid_out set = the unfused twin: the launch stops behind phase 2 and stores the
    // mid tile as the [M][MID] fp32 tensor (w3 / scale3 / bias3 / res / y unused).
    const void* w2_split;
    float* mid_out;
};
bool bottleneck_tail_ok(int precision, int mid, int cout);          // shapes the fused kernel is built for
bool bottleneck_tail_split_ok(int precision, int mid, int cout, long long M);      // ... and its split form (TailArgs::w2_split)
td_status bottleneck_tail_launch(const TailArgs& a, int precision, hipStream_t stream);

// ---- Winograd F(2x2,3x3) transforms (winograd.hip; fp32 engine) ---------------------------------
// tiles [t0, t0 + Ts) of the layer ("slab"): V / Mb hold 16 planes of [Ts][C]
td_status wino_input_launch(const float* x, int B, int H, int W, int C, float* V, const int* m_dyn, int m_mul, long long t0, int Ts,
                            hipStream_t s);
td_status wino_output_launch(const float* Mb, int B, int H, int W, int N, const float* scale, const float* bias, int relu,
                             float* y, const int* m_dyn, int m_mul, long long t0, int Ts, hipStream_t s);
void wino_filter_transform(const float* w_ohwi, int N, int C, float* U);     // host: U [16][N][C]
// F(4x4,3x3): whole layers only; V / Mb hold 36 planes of [T][C], T = B * ceil(H/4) * ceil(W/4)
// (m_dyn: optional device-side image count <= B, the mask head's live RoIs)
td_status wino43_input_launch(const float* x, int B, int H, int W, int C, float* V, const int* m_dyn, hipStream_t s);
// F(4x4,3x3) contraction + output transform in ONE launch (wino_fused.hip): V [36][T][C] x U [36][N][C] → y, the M planes never
// reach memory. Another association of the transform sums than wino43_output_launch: a fixed rule picks the layers (conv_path.h,
// which also declares wino43_fused_ok, the shapes it runs).
td_status wino43_fused_launch(const float* V, const float* U, int B, int H, int W, int C, int N, const float* scale, const float* bias,
                              int relu, float* y, const int* m_dyn, hipStream_t s);
td_status wino43_output_launch(const float* Mb, int B, int H, int W, int N, const float* scale, const float* bias, int relu,
                               float* y, const int* m_dyn, hipStream_t s);
// the same for a 256-channel layer whose only consumer is a 1x1 head [head_n <= 32][256]: head_y [B*H*W][head_n] = y . head_w^T + head_b,
// y itself is not written (bit-identical to wino43_output_launch followed by the head as a conv2d_launch of its own)
td_status wino43_output_head_launch(const float* Mb, int B, int H, int W, int N, const float* scale, const float* bias, int relu,
                                    const float* head_w, const float* head_b, float* head_y, int head_n, hipStream_t s);
void wino43_filter_transform(const float* w_ohwi, int N, int C, float* U);   // host: U [36][N][C]
// ---- the Winograd launch sequences of one layer (wino_seq.cpp), each written once over the entries above: F(2x2) with the input
// transform fused into the contraction or per slab, F(4x4) in three launches, with the head in its output transform, or folded
struct WinoRun {
    int form;                  // CONV_WINO22 / CONV_WINO43 / CONV_WINO43_FOLD (conv_path.h)
    bool fused_input;          // F(2x2): wino_gemm_kernel transforms the input in its A staging, V never exists in memory
    int slab_tiles;            // F(2x2): tiles per slab
    int fold_group;            // folded F(4x4): images per launch pair
    const float *x, *U, *scale, *bias;      // U: the layer's filter bank of the form, [16] or [36][cout][cin]
    const void* U_split;       // F(4x4) in three launches only: the split-bf16 twin of U (conv_split_pack_planes) — the 36 plane
                               // contractions then run on the TILE_SPLIT ids (another rounding: a fixed rule of the caller's), or nullptr
    float* y;
    int B, H, W, cin, cout, relu;
    float *V, *M;              // workspace planes
    const int* m_dyn;          // optional device-side count (rows for F(2x2) with m_mul rows per image, images for F(4x4))
    int m_mul;
    int gemm_cfg;              // block tile of the batched plane contraction (-1 = heuristic)
    const float *head_w, *head_b;           // F(4x4) in three launches only: the 1x1 head in the output transform, y is not written
    float* head_y;
    int head_n;
};
ConvArgs wino_plane_args(const WinoRun& r, int n, long long t0);      // what the tuner times: the launch shapes of the plane contractions
ConvArgs wino43_plane_args(const WinoRun& r);
// Optional books of a caller around every launch (the engine's profiling): n = tiles of the slab (F(2x2)) or images of the launch
// (F(4x4)); the steps: WINO_STEP_* (launch_cost.h). A null hook costs a null check per launch.
struct WinoHook {
    void* ctx;
    void (*begin)(void* ctx, int step, long long n);
    void (*end)(void* ctx);
};
td_status wino_run(const WinoRun& r, hipStream_t s, const WinoHook* hook = nullptr);

// ---- stem / pooling / resize (stem.hip) ---------------------------------------------------------
struct ImgSizes {           // per-image valid sizes, passed by value (B <= TD_MAX_BATCH)
    int h[64];
    int w[64];
};
#define TD_MAX_BATCH 64
// w16 / bias16 (optional, from stem_mfma_prepare): the fp16 engine's uint8 inputs with 64 channels take the MFMA stem
td_status stem_launch(const void* images, int input_format, const ImgSizes& valid, int B, int Hp, int Wp,
                      const float* w_kc /*[147][cout]*/, const float* scale, const float* bias, void* y,
                      int cout, int precision, hipStream_t stream, const void* w16 = nullptr, const float* bias16 = nullptr);
void stem_mfma_prepare(const float* w_kc, const float* scale, const float* bias, int cout, std::vector<unsigned short>& w16_bits,
                       std::vector<float>& bias16);       // w16_bits: IEEE half bit patterns (this header is also compiled by g++)
td_status maxpool3x3s2_launch(const void* x, void* y, int B, int H, int W, int C, int precision, hipStream_t stream);
td_status subsample2_launch(const void* x, void* y, int B, int H, int W, int C, int precision, hipStream_t stream);
td_status resize_batch_u8_launch(const uint8_t* const* srcs, int n, int h, int w, int c, uint8_t* dst, int out_h,
                                 int out_w, int dst_pitch_px, size_t dst_img_bytes, void* tmp, hipStream_t stream);
td_status resize_bilinear_f64_launch(const double* src, int c, int h, int w, float* dst, int out_h, int out_w, int dst_pitch,
                                     long long dst_plane, hipStream_t stream);
td_status windows_u16_to_input_launch(const uint16_t* raster, int H, int W, int C, const int32_t* windows, int n, int* band1_max, float* dst,
                                      int out_h, int out_w, int dst_pitch, long long dst_plane, long long dst_image, hipStream_t stream);
td_status resize_tile_u8_launch(const uint8_t* src, int h, int w, int c, uint8_t* dst, int out_h, int out_w,
                                int dst_pitch_px, void* tmp, hipStream_t stream);
