// td_engine: weights, workspace plan and the forward schedule of the Mask R-CNN R50/R101-FPN tile predictor.
//
// Stands behind `self.model(batch_tensors)` (TreeDetection/prediction.py:182-183) with the model that
// TreeDetection/config.py:25-66 configures. Layer order and hyper-parameters follow SURVEY.md Appendix A; every
// contraction runs through conv2d_launch (MFMA implicit GEMM), everything else through the kernels of
// stem.hip / rpn.hip / roi.hip. The whole forward is asynchronous on one HIP stream: dynamic counts
// (proposals, detections) stay on the device and bound the later kernels, so there is no host sync inside.
#include "common.h"
#include "detect.h"
#include "workspace.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <functional>
#include <map>
#include <optional>
#include <string>
#include <tuple>
#include <vector>

namespace {

struct HostTensor {
    const float* data = nullptr;
    std::vector<int64_t> shape;
    int64_t numel() const {
        int64_t n = 1;
        for (auto s : shape) n *= s;
        return n;
    }
};

enum { SPLIT_FC = 1, SPLIT_LATERAL = 2, SPLIT_CONV1 = 4, SPLIT_CONV3 = 8, SPLIT_SHORTCUT = 16,
       SPLIT_DEFAULT = SPLIT_FC | SPLIT_LATERAL | SPLIT_CONV1 | SPLIT_SHORTCUT };
// layer classes of td_engine::f32_split_wino (the split twin of the F(4x4) filter bank)
enum { WINO_SPLIT_RES = 1, WINO_SPLIT_FPN = 2, WINO_SPLIT_RPN = 4, WINO_SPLIT_DEFAULT = WINO_SPLIT_RES | WINO_SPLIT_FPN | WINO_SPLIT_RPN };

struct ConvLayer {
    int cout = 0, cin = 0, kh = 1, kw = 1;
    void* w = nullptr;        // [cout][kh][kw][cin], float32 or float16 (engine precision)
    float* scale = nullptr;   // [cout] or null
    float* bias = nullptr;    // [cout] or null
    bool out_f32 = false;     // fp16 engine: this layer still writes float32 (feeds the fp32 selection kernels)
    void* w_frag = nullptr;   // fp16 engine: the filters in MFMA fragment order (conv_bdirect.hip), layers with cin % 64 == 0
    void* w_split = nullptr;  // fp32 engine, the layers of the split rule (td_engine::f32_split): three bf16 pieces per weight in fragment
                              // order (conv_split.hip); a layer that has it runs the TILE_SPLIT ids and nothing else
    void* w_tail_split = nullptr;   // fp32 engine, conv2 of the res2 blocks (td_engine::f32_split_tail): the 3x3 bank as three bf16 pieces per weight
                              // in the split tail's fragment order (bottleneck.hip). Not w_split: the layer is no conv_path SPLIT layer
    float* wino_u = nullptr;  // fp32 engine, 3x3 layers: Winograd-transformed filters U [16][cout][cin] (winograd.hip)
    float* wino_u43 = nullptr;  // the same for F(4x4,3x3): U [36][cout][cin] (layers with >= 128 channels on both sides)
    void* wino_u43_split = nullptr;   // fp32 engine, the layer classes of td_engine::f32_split_wino: the 36 planes of wino_u43 as split-bf16
                              // banks (conv_split_pack per plane, concatenated); the unfolded F(4x4) form then contracts on the TILE_SPLIT ids
};

struct Block {
    ConvLayer c1, c2, c3, sc;
    bool has_sc = false;
    int stride = 1;
};

struct NamedTensor { void* p; WsDims dims; int elem; };     // what td_engine_tensor answers

}  // namespace

struct td_engine : Workspace {          // (the workspace pointers: workspace.h)
    td_model_desc desc{};
    int device = 0;
    bool loaded = false;
    std::vector<void*> weight_allocs;
    std::vector<void*> ws_allocs;

    // weights
    float* stem_w = nullptr;  // [147][stem_c]
    float* stem_scale = nullptr;
    float* stem_bias = nullptr;
    unsigned short* stem_w16 = nullptr;   // fp16 engine: filter image (half bit patterns) of the MFMA stem [64][192] (stem.hip stem_mfma_kernel)
    float* stem_bias16 = nullptr;   //              bias with the mean subtraction folded in
    int stem_c = 64;
    std::vector<Block> stages[4];
    ConvLayer lateral[4], fpn_out[4];
    ConvLayer rpn_conv, rpn_head;   // head: fused 3 + 12 rows
    ConvLayer fc1, fc2, pred;       // pred: fused 2 + 4 rows
    ConvLayer mask_fcn[4], deconv;  // deconv packed [4*C][C]
    float* mask_pred_w = nullptr;
    float mask_pred_b = 0.f;
    int fpn_c = 256, fc_dim = 1024;

    int rB = 0, rHp = 0, rWp = 0;          // what the workspace is sized for (td_engine_reserve)
    std::map<std::string, NamedTensor> named;

    int backbone_subbatch = 0;    // 0 = whole batch; else images per backbone pass (TD_BACKBONE_SUBBATCH)
    // measured block-tile choice per launch shape, filled lazily by the first forward of a shape; key (ConvPath::key): (cout, cin,
    // kh*16+kw, rows, stride*4 + out_mode*2 + has_residual + flag) — layers of identical shape share it
    std::map<std::tuple<int, int, int, int, int>, int> tuned;
    // winograd, wino_fused, wino_slab, wino_minc, wino43_min, wino_fold and fuse_head below, with the precision and wino_elems, are
    // the rules of conv_path (conv_path.h): which form a layer takes is that function's answer and nothing else's.
    bool winograd = true;         // TD_WINOGRAD=0 disables the Winograd path (diagnostics)
    size_t wino_elems = 0;
    bool group_levels = true;     // TD_GROUP_LEVELS=0: the FPN output convs / the RPN conv + head as one launch per pyramid level (fp16 engine)
    bool fuse_head = true;        // TD_FUSE_HEAD=0: the RPN's 1x1 head as a launch of its own at every level (diagnostics, tests)
    bool fuse_tail = true;        // TD_FUSE_TAIL=0: conv2 / conv3 of res2 as two launches (diagnostics, tests); 2: fuse the fp16 engine's res3 too
    bool fuse_tail_fp16 = false;
    bool wino_fused = true;       // TD_WINO_FUSED=0: separate input-transform kernel + batched conv_igemm launch (diagnostics)
    // TD_WINO_SLAB: tiles per F(2x2) slab (diagnostics). A layer can be walked in slabs of tiles whose V and M planes would stay inside
    // the 256 MiB Infinity Cache; measured on the bench (round 2, fp32, 3 batches in flight): 4096-tile slabs 425 tiles/s, 8192 441,
    // whole layers 456 — the shorter launches lose more to their tails and boundaries than the on-die hand-over of V / M saves, so
    // the default (0) is one slab = the whole layer.
    int wino_slab = 0;
    int wino_minc = 128;          // fewest channels (both sides) of a 3x3 layer on the Winograd path (TD_WINO_MINC: experiments)
    int wino43_min = 12;          // maps at least this large on both sides take F(4x4,3x3) (TD_WINO43_MIN; 0 = never)
    // F(4x4) layers whose plane contractions and output transform run as ONE launch (wino43_fused_kernel: the M planes never reach
    // memory). A FIXED rule on the layer's own shape — per-image map size and channels, never the batch and never a timing: the
    // fold associates the transform sums differently from the three-launch form, and a batch of 8 must equal eight batches of 1
    // bit for bit. Measured (profiles/r04_wino_fold.txt, batch 8): 256 -> 256 on the 200 x 200 maps 1 007 -> 895 us, 128 -> 128
    // on 100 x 100 (res3 conv2) 103 -> 95 us; it loses where its 64-tile x 64-channel blocks cannot fill the chip (res4 / res5,
    // p3 - p6: 88 - 316 blocks on 256 CUs) and on the RPN layers, whose head rides in the three-launch form's output transform.
    // TD_WINO_FOLD (bit mask): 1 = 256 channels from 160 x 160 and 128 channels from 80 x 80 (isolated winners), 2 = the mask head
    // (device-side RoI count), 4 = 256-channel maps from 80 x 80 (FPN output 3): with three forwards in flight the fold also pays
    // where its isolated time ties, it frees HBM bandwidth for the other streams (bench, fp32 tiles/s: 0 → 638, 1 → 650, 3 → 655,
    // 7 → 656) —, 8 = every map from 40 x 40 and 16 = every layer the kernel can run: 660 - 661 under the stream schedule but
    // 574 → 545 one forward at a time (88-block launches on 256 CUs), not taken.
    // 32 = the RPN conv on the 160 x 160+ maps folds too (its head becomes a launch of its own). The default is 39 = 1 + 2 + 4 + 32.
    int wino_fold = 39;
    // fp32 engine: the 1x1 / FC layers that run on the bf16 matrix cores with both operands as three bf16 pieces (conv_split.hip:
    // its own rounding, so a FIXED rule on the layer — its place in the network and K >= 256 —, never a timing). Bit mask of layer
    // classes (TD_F32_SPLIT; 0 = none, for an A/B on one build): SPLIT_FC the box head's fc1 / fc2, SPLIT_LATERAL the four FPN
    // laterals, SPLIT_CONV1 / SPLIT_CONV3 / SPLIT_SHORTCUT the 1x1 layers of res3 - res5. Never through this rule: layers that also
    // exist inside a fused kernel or have a bit-identity twin (the RPN head, the box and mask predictors; res2: its 3x3 has a rule of
    // its own, f32_split_tail below), K < 256, the fp16 engine.
    // The default is the box head, the FPN laterals, conv1 and the shortcuts (23): the classes whose gain on the headline was
    // measured (profiles/f32_split.txt, profiles/f32_split_backbone.txt). conv3 stays off: res4 ties or loses in the per-layer table.
    // Cost: the split banks, 6 B per weight, about 48 MB per fp32 engine beside the fp32 filters.
    int f32_split = SPLIT_DEFAULT;
    // fp32 engine: conv2 (3x3, 64 -> 64) of the res2 blocks on the bf16 matrix cores the same way, inside the fused tail
    // (bottleneck.hip, the split form; the 1x1 behind it stays on the fp32 MFMA: it is memory-bound). A switch of its own
    // (TD_F32_SPLIT_TAIL, default 1; 0 = the fp32 tail), not a bit of f32_split, and like it a FIXED rule on the layer, never a timing:
    // no tile is chosen, nothing is written to the tune cache. The bit-identity twin of the fused launch is kept by construction:
    // with TD_FUSE_TAIL=0 conv2 runs as the SAME kernel's mid-store launch (it stops behind phase 2 and writes t2) and conv3 as the
    // fp32 1x1 launch it always was, which the fused kernel's phase 3 equals bit for bit. Cost: 221 KB per block, +0.66 MB per engine.
    bool f32_split_tail = true;
    // fp32 engine: the 36 plane contractions of the F(4x4,3x3) layers that do NOT fold (CONV_WINO43, three launches) on the bf16 matrix
    // cores the same way: each plane is a plain 1x1 contraction V[p] [T x C] . U[p]^T, one batched launch of conv_split_kernel. A FIXED
    // rule on the layer (TD_F32_SPLIT_WINO, bit mask of layer classes; 0 = fp32 planes, for an A/B on one build), never a timing:
    // WINO_SPLIT_RES conv2 of res4 / res5, WINO_SPLIT_FPN the FPN outputs, WINO_SPLIT_RPN the RPN conv. A layer of a class has the
    // twin bank; conv_path takes it where the layer runs the unfolded form with static rows (the folded layers and the mask head never do).
    // The default is all three classes (7): in the layer table (batch 8, 800 x 800) the contractions of res4 conv2 go 67 - 74 -> 60 - 63 us,
    // res5 conv2 76 - 77 -> 71 - 72, fpn_output4 67 -> 61, rpn p3 / p4 220 / 69 -> 164 / 60; the 7 x 7 and 4 x 4 maps of 256 channels
    // (fpn_output5, rpn p5 / p6: 25 / 26 / 15 us) lose 2 - 3 us each and keep their class's rule. Headline 758.5 - 764.4 -> 773.1 - 779.0
    // tiles/s on one box, alternated (profiles/f32_split_wino.txt).
    // Cost: 36 N C 6 B per layer (14 MB at 256 x 256, 57 MB at 512 x 512); measured per R50 engine 958 -> 1 288 MB of device memory
    // (+ 329 MB: 256 / 58 / 14 MB for the three classes) and 0.80 - 0.86 -> 1.04 s of load time.
    int f32_split_wino = WINO_SPLIT_DEFAULT;
    std::string tune_cache;       // TD_TUNE_CACHE: load / append measured choices (keeps profiled runs free of tuning launches)
    // The tuner times every candidate tile with the L2 (8 x 4 MB) emptied before each launch (a fill of this scratch on the same
    // stream): in the forward a layer's filters and most of its input are NOT in L2 — 50-odd other launches ran since — and a loop of
    // back-to-back launches of one layer otherwise favours tiles that re-read their filters (res5 conv2, fp16: the hot loop picked
    // a tile that runs 57 us in the forward against 45 us for the cold loop's choice). TD_TUNE_EVICT=0 restores the hot loop.
    void* tune_evict = nullptr;
    size_t tune_evict_bytes = 0;

    // forward context (kept between the phases of td_engine_forward_phase) and the per-phase completion events
    struct FwdCtx {
        const void* images = nullptr;
        int input_format = 0, B = 0, Hp = 0, Wp = 0;
        ImgSizes valid{}, outsz{};
        td_detections out{};
        bool valid_ctx = false;
    } ctx;
    hipEvent_t phase_ev[7] = {};           // [6] = the optional stem pre-phase (TD_PHASE_STEM)
    bool phase_ev_recorded[7] = {};
    hipEvent_t prev5_ev = nullptr;         // phase-5 event of the previous batch (the next batch's phase 3 waits for it)
    bool prev5_recorded = false;
    bool stem_done = false;                // stem + pool of the current batch already ran in the pre-phase

    // optional per-category device timing (td_engine_profile_*)
    bool prof = false;
    bool prof_group_open = false;
    struct ProfRec { hipEvent_t a, b; int id; };      // a recorded event pair of category / class id
    std::vector<ProfRec> prof_recs;
    std::vector<hipEvent_t> prof_free;
    double prof_ms[TD_PROF_CATEGORIES] = {};
    int64_t prof_launches[TD_PROF_CATEGORIES] = {};
    double prof_flops[TD_PROF_CATEGORIES] = {};
    double prof_bytes[TD_PROF_CATEGORIES] = {};
    // per-class speed-of-light accounting of the contraction family (td_engine_profile_classes): what each launch EXECUTES
    // (Winograd planes: the plane products, not the direct convolution's multiplies) and the bytes its algorithm moves
    // (V / M planes included), with t_min = max(executed FLOPs / MFMA peak, bytes / achievable HBM rate) per launch;
    // measured time per class only in detail mode (td_engine_profile_enable(e, 2): an event pair per launch)
    bool prof_detail = false;
    double cls_ms[TD_PROF_CLASSES] = {};
    int64_t cls_launches[TD_PROF_CLASSES] = {};
    double cls_flops[TD_PROF_CLASSES] = {};
    double cls_bytes[TD_PROF_CLASSES] = {};
    double cls_tmin_ms[TD_PROF_CLASSES] = {};
    std::vector<ProfRec> cls_recs;
};

namespace {

td_status dev_alloc(std::vector<void*>& pool, void** p, size_t bytes) {
    if (bytes == 0) bytes = 16;
    TD_HIP_CHECK(hipMalloc(p, bytes));
    pool.push_back(*p);
    return TD_OK;
}

template <typename T>
td_status upload(td_engine* e, const std::vector<T>& h, T** d) {
    void* p = nullptr;
    td_status st = dev_alloc(e->weight_allocs, &p, h.size() * sizeof(T));
    if (st < 0) return st;
    TD_HIP_CHECK(hipMemcpy(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    *d = static_cast<T*>(p);
    return TD_OK;
}

// conv / fc weight matrix in the engine's precision (float16: round-to-nearest-even on the host)
td_status upload_w(td_engine* e, const std::vector<float>& h, void** d) {
    if (e->desc.precision == TD_PRECISION_FP16) {
        std::vector<_Float16> hh(h.size());
        for (size_t i = 0; i < h.size(); ++i) hh[i] = (_Float16)h[i];
        _Float16* p = nullptr;
        td_status st = upload(e, hh, &p);
        *d = p;
        return st;
    }
    float* p = nullptr;
    td_status st = upload(e, h, &p);
    *d = p;
    return st;
}

// second copy of a filter bank in MFMA fragment order for the tiles with ConvTile::frag, both precisions
td_status upload_frag(td_engine* e, const std::vector<float>& h, ConvLayer& L) {
    L.w_frag = nullptr;
    static const bool off = getenv("TD_BDIRECT") && atoi(getenv("TD_BDIRECT")) == 0;
    const bool f16 = e->desc.precision == TD_PRECISION_FP16;
    const int ke = f16 ? 64 : 32;
    if (off || L.cin % ke != 0 || L.kh * L.kw > 32 || (size_t)L.cout * L.kh * L.kw * L.cin != h.size()) return TD_OK;
    std::vector<unsigned char> packed;
    if (f16) {
        std::vector<unsigned short> bits(h.size());
        for (size_t i = 0; i < h.size(); ++i) bits[i] = __builtin_bit_cast(unsigned short, (_Float16)h[i]);
        conv_bd_pack(bits.data(), 2, L.cout, L.kh, L.kw, L.cin, packed);
    } else {
        conv_bd_pack(h.data(), 4, L.cout, L.kh, L.kw, L.cin, packed);
    }
    unsigned char* d = nullptr;
    td_status st = upload(e, packed, &d);
    L.w_frag = d;
    return st;
}

// the split-bf16 bank of a layer of class `cls` (SPLIT_*) when the rule takes that class: fp32 engine, 1x1, K >= 256
td_status upload_split(td_engine* e, const std::vector<float>& h, ConvLayer& L, int cls) {
    L.w_split = nullptr;
    if (e->desc.precision != TD_PRECISION_FP32 || !(e->f32_split & cls) || L.kh != 1 || L.kw != 1 || L.cin < 256 || L.cin % 32 != 0 ||
        (size_t)L.cout * L.cin != h.size())
        return TD_OK;
    std::vector<unsigned char> packed;
    conv_split_pack(h.data(), L.cout, L.cin, packed);
    unsigned char* d = nullptr;
    td_status st = upload(e, packed, &d);
    L.w_split = d;
    return st;
}

// the split tail's bank of a res2 conv2 (3x3, 64 -> 64 in front of a 64 -> 256 conv3) when the rule is on: fp32 engine only
td_status upload_tail_split(td_engine* e, const std::vector<float>& w_ohwi, ConvLayer& L, int cout3) {
    L.w_tail_split = nullptr;
    if (!e->f32_split_tail || L.kh != 3 || L.kw != 3 || L.cin != L.cout || !bottleneck_tail_split_ok(e->desc.precision, L.cout, cout3, 1) ||
        (size_t)L.cout * 9 * L.cin != w_ohwi.size())
        return TD_OK;
    std::vector<unsigned char> packed;
    conv_split_pack(w_ohwi.data(), L.cout, L.cin, packed, 9);
    unsigned char* d = nullptr;
    td_status st = upload(e, packed, &d);
    L.w_tail_split = d;
    return st;
}

using TensorMap = std::map<std::string, HostTensor>;

td_status need(const TensorMap& tm, const std::string& name, int ndim, const HostTensor** out) {
    auto it = tm.find(name);
    if (it == tm.end()) {
        td_set_error("load_weights: tensor '%s' missing", name.c_str());
        return TD_ERR_WEIGHTS;
    }
    if ((int)it->second.shape.size() != ndim) {
        td_set_error("load_weights: tensor '%s' has %d dims, expected %d", name.c_str(), (int)it->second.shape.size(), ndim);
        return TD_ERR_WEIGHTS;
    }
    *out = &it->second;
    return TD_OK;
}

// [Cout,Cin,KH,KW] → [Cout][KH][KW][Cin]
std::vector<float> pack_ohwi(const HostTensor& t) {
    const int co = (int)t.shape[0], ci = (int)t.shape[1], kh = (int)t.shape[2], kw = (int)t.shape[3];
    std::vector<float> out((size_t)co * ci * kh * kw);
    for (int o = 0; o < co; ++o)
        for (int c = 0; c < ci; ++c)
            for (int y = 0; y < kh; ++y)
                for (int x = 0; x < kw; ++x)
                    out[(((size_t)o * kh + y) * kw + x) * ci + c] = t.data[(((size_t)o * ci + c) * kh + y) * kw + x];
    return out;
}

// FrozenBN fold: scale = gamma * (1/sqrt(var + eps)), bias = beta - mean * scale (float32, like the oracle)
td_status bn_fold(const TensorMap& tm, const std::string& p, int c, std::vector<float>& scale, std::vector<float>& bias) {
    const HostTensor *g, *b, *m, *v;
    td_status st;
    if ((st = need(tm, p + ".norm.weight", 1, &g)) < 0) return st;
    if ((st = need(tm, p + ".norm.bias", 1, &b)) < 0) return st;
    if ((st = need(tm, p + ".norm.running_mean", 1, &m)) < 0) return st;
    if ((st = need(tm, p + ".norm.running_var", 1, &v)) < 0) return st;
    if (g->shape[0] != c || b->shape[0] != c || m->shape[0] != c || v->shape[0] != c) {
        td_set_error("load_weights: norm tensors of '%s' do not have %d channels", p.c_str(), c);
        return TD_ERR_WEIGHTS;
    }
    scale.resize(c);
    bias.resize(c);
    for (int i = 0; i < c; ++i) {
        const float r = 1.0f / std::sqrt(v->data[i] + 1e-5f);
        const float s = g->data[i] * r;
        const float ms = m->data[i] * s;
        scale[i] = s;
        bias[i] = b->data[i] - ms;
    }
    return TD_OK;
}

// fp32 engine: the Winograd filter banks of a 3x3 layer (which form uses them where: conv_path)
// wino_cls (WINO_SPLIT_*): the layer's class under td_engine::f32_split_wino — the F(4x4) bank then gets its split-bf16 twin
td_status upload_wino(td_engine* e, const std::vector<float>& w_ohwi, ConvLayer& L, int wino_cls) {
    L.wino_u = nullptr;
    L.wino_u43_split = nullptr;
    if (e->desc.precision != TD_PRECISION_FP32 || !e->winograd || L.kh != 3 || L.kw != 3 || L.cin % 32 != 0 || L.cout % 4 != 0)
        return TD_OK;
    std::vector<float> u((size_t)16 * L.cout * L.cin);
    wino_filter_transform(w_ohwi.data(), L.cout, L.cin, u.data());
    td_status st = upload(e, u, &L.wino_u);
    if (st < 0 || e->wino43_min <= 0 || L.cin < e->wino_minc || L.cout < e->wino_minc) return st;
    std::vector<float> u43((size_t)36 * L.cout * L.cin);
    wino43_filter_transform(w_ohwi.data(), L.cout, L.cin, u43.data());
    if ((st = upload(e, u43, &L.wino_u43)) < 0 || !(e->f32_split_wino & wino_cls)) return st;
    std::vector<unsigned char> packed;
    conv_split_pack_planes(u43.data(), 36, L.cout, L.cin, packed);
    unsigned char* d = nullptr;
    st = upload(e, packed, &d);
    L.wino_u43_split = d;
    return st;
}

td_status load_conv_bn(td_engine* e, const TensorMap& tm, const std::string& p, ConvLayer& L, int split_cls = 0, int wino_cls = 0) {
    const HostTensor* w;
    td_status st = need(tm, p + ".weight", 4, &w);
    if (st < 0) return st;
    L.cout = (int)w->shape[0];
    L.cin = (int)w->shape[1];
    L.kh = (int)w->shape[2];
    L.kw = (int)w->shape[3];
    const std::vector<float> packed = pack_ohwi(*w);
    if ((st = upload_w(e, packed, &L.w)) < 0) return st;
    if ((st = upload_frag(e, packed, L)) < 0) return st;
    if ((st = upload_split(e, packed, L, split_cls)) < 0) return st;
    if ((st = upload_wino(e, packed, L, wino_cls)) < 0) return st;
    std::vector<float> s, b;
    if ((st = bn_fold(tm, p, L.cout, s, b)) < 0) return st;
    if ((st = upload(e, s, &L.scale)) < 0) return st;
    return upload(e, b, &L.bias);
}

td_status load_conv_bias(td_engine* e, const TensorMap& tm, const std::string& p, ConvLayer& L, int split_cls = 0, int wino_cls = 0) {
    const HostTensor *w, *b;
    td_status st = need(tm, p + ".weight", 4, &w);
    if (st < 0) return st;
    if ((st = need(tm, p + ".bias", 1, &b)) < 0) return st;
    L.cout = (int)w->shape[0];
    L.cin = (int)w->shape[1];
    L.kh = (int)w->shape[2];
    L.kw = (int)w->shape[3];
    if (b->shape[0] != L.cout) {
        td_set_error("load_weights: bias of '%s' has wrong length", p.c_str());
        return TD_ERR_WEIGHTS;
    }
    const std::vector<float> packed = pack_ohwi(*w);
    if ((st = upload_w(e, packed, &L.w)) < 0) return st;
    if ((st = upload_frag(e, packed, L)) < 0) return st;
    if ((st = upload_split(e, packed, L, split_cls)) < 0) return st;
    if ((st = upload_wino(e, packed, L, wino_cls)) < 0) return st;
    L.scale = nullptr;
    return upload(e, std::vector<float>(b->data, b->data + L.cout), &L.bias);
}

// The geometry of the workspace plan (workspace.h) for this engine's model at one batch shape
WsGeom engine_geom(const td_engine* e, int B, int Hp, int Wp) {
    int32_t c[WS_WIDTHS] = {e->stem_c};
    for (int s = 0; s < 4; ++s) { c[1 + s] = e->stages[s][0].c1.cout; c[5 + s] = e->stages[s][0].c2.cout; c[9 + s] = e->stages[s][0].c3.cout; }
    c[13] = e->fpn_c; c[14] = e->fc_dim; c[15] = e->deconv.cout / 4;
    return ws_geom(e->desc.precision, e->winograd, e->desc.post_nms_topk, e->desc.detections_per_image, c, B, Hp, Wp);
}

// td_engine_tensor's names of the rows a finished phase fills, at the geometry of the batch in hand (phase 0 brings the stem
// pre-phase's two along: it runs the stem itself when nobody ran the pre-phase)
void publish(td_engine* e, const WsGeom& g, int phase) {
    for (const WsRow& r : ws_rows())
        for (int i = 0; r.pub && (r.phase == phase || (phase == 0 && r.phase == TD_PHASE_STEM)) && i < r.count; ++i) {
            char name[32];
            snprintf(name, sizeof name, r.pub, i + 2);
            e->named[name] = NamedTensor{*ws_slot(e, r, i), r.dims(g, i), (int)ws_elem_bytes(r, g)};
        }
}

// an event of the engine's pool, recorded on s
hipEvent_t prof_event(td_engine* e, hipStream_t s) {
    hipEvent_t ev = nullptr;
    if (!e->prof_free.empty()) {
        ev = e->prof_free.back();
        e->prof_free.pop_back();
    } else {
        (void)hipEventCreate(&ev);
    }
    (void)hipEventRecord(ev, s);
    return ev;
}

// the finished event pairs of one book: their times into ms[id], the events back to the pool
td_status drain_recs(td_engine* e, std::vector<td_engine::ProfRec>& recs, double* ms) {
    for (auto& r : recs) {
        TD_HIP_CHECK(hipEventSynchronize(r.b));
        float t = 0.f;
        TD_HIP_CHECK(hipEventElapsedTime(&t, r.a, r.b));
        ms[r.id] += t;
        e->prof_free.push_back(r.a);
        e->prof_free.push_back(r.b);
    }
    recs.clear();
    return TD_OK;
}

// THE booking bracket (RAII) of one launch, or (cat or cls none, launch_cost.h) of a sequence / of one step of it: adds what the launch
// costs to both books and records start on construction and stop on destruction (only when profiling is on). The category side: a
// GROUP scope brackets a run of back-to-back launches of one category with ONE event pair (an event per launch costs ≈3 % of the
// fp32 step and ≈10 % of the fp16 step in extra kernel boundaries); launches inside it only add their counts. The class side: always
// the model (executed FLOPs, bytes the chosen algorithm moves, t_min); in detail mode also an event pair of its own, inside the other.
struct ProfScope {
    td_engine* e;
    hipStream_t s;
    hipEvent_t a = nullptr, cls_a = nullptr;
    int cat, cls;
    bool group;
    ProfScope(td_engine* e_, hipStream_t s_, int cat_, bool group_ = false) : ProfScope(e_, s_, LaunchCost{cat_}, group_) {}
    ProfScope(td_engine* e_, hipStream_t s_, const LaunchCost& c, bool group_ = false) : e(e_), s(s_), cat(c.cat), cls(c.cls), group(group_) {
        if (!e->prof) return;
        if (cat >= 0 && !group) {
            e->prof_flops[cat] += c.flops;
            e->prof_bytes[cat] += c.bytes;
            e->prof_launches[cat] += c.layers;
            e->prof_flops[8] += c.exec_flops;
            e->prof_launches[8] += c.wino ? 1 : 0;
        }
        if (cat >= 0 && !e->prof_group_open) {         // (else counted; the enclosing group owns the events: groups do not nest)
            a = prof_event(e, s);
            if (group) e->prof_group_open = true;
        }
        if (cls < 0) return;
        const double peak = (e->desc.precision == TD_PRECISION_FP16 ? TD_PEAK_F16_MFMA_TFLOPS : TD_PEAK_F32_MFMA_TFLOPS) * 1e12;
        e->cls_launches[cls] += 1;
        e->cls_flops[cls] += c.exec_flops;
        e->cls_bytes[cls] += c.cls_bytes;
        e->cls_tmin_ms[cls] += 1e3 * std::max(c.exec_flops / peak, c.cls_bytes / (TD_HBM_ACHIEVABLE_TBS * 1e12));
        if (e->prof_detail) cls_a = prof_event(e, s);
    }
    ~ProfScope() {
        if (cls_a) e->cls_recs.push_back({cls_a, prof_event(e, s), cls});
        if (!a) return;
        e->prof_recs.push_back({a, prof_event(e, s), cat});
        if (group) e->prof_group_open = false;
    }
};

// Measured block-tile choices shared between engines (and runs) through the TD_TUNE_CACHE file: read at creation and
// again whenever a layer shape is missing, so engines created together pick up what the first one measured.
void load_tune_cache(td_engine* e) {
    if (e->tune_cache.empty()) return;
    if (FILE* f = fopen(e->tune_cache.c_str(), "r")) {
        int pr, a0, a1, a2, a3, a4, cfg;
        while (fscanf(f, "%d %d %d %d %d %d %d", &pr, &a0, &a1, &a2, &a3, &a4, &cfg) == 7) {
            if (pr == e->desc.precision && conv_tile(cfg)) e->tuned[std::make_tuple(a0, a1, a2, a3, a4)] = cfg;
        }
        fclose(f);
    }
}

void free_pool(std::vector<void*>& pool) {
    for (void* p : pool) (void)hipFree(p);
    pool.clear();
}

// The diagnostic switches on the rules of conv_path (an engine reads them once, at creation)
void read_rule_switches(td_engine* e) {
    if (const char* wg = getenv("TD_WINOGRAD")) e->winograd = atoi(wg) != 0;
    if (const char* ws = getenv("TD_WINO_SLAB")) e->wino_slab = atoi(ws);
    if (const char* wf = getenv("TD_WINO_FUSED")) e->wino_fused = atoi(wf) != 0;
    if (const char* fh = getenv("TD_FUSE_HEAD")) e->fuse_head = atoi(fh) != 0;
    if (const char* w4 = getenv("TD_WINO43_MIN")) e->wino43_min = atoi(w4);
    if (const char* wf2 = getenv("TD_WINO_FOLD")) e->wino_fold = atoi(wf2);
    if (const char* wc = getenv("TD_WINO_MINC")) e->wino_minc = atoi(wc);
}

ConvRules conv_rules(const td_engine* e) {
    return {e->desc.precision, e->winograd, e->wino_fused, e->wino_minc, e->wino43_min, e->wino_fold, e->wino_slab, e->fuse_head, e->wino_elems};
}

}  // namespace

extern "C" {

td_status td_engine_create(const td_model_desc* desc, int device, td_engine** out) {
    TD_REQUIRE(out, "td_engine_create: out is NULL");
    td_model_desc d;
    if (desc) d = *desc; else td_model_desc_default(&d);
    TD_REQUIRE(d.num_classes == 1, "td_engine_create: num_classes=%d (the reference configures exactly 1, config.py:35)", d.num_classes);
    TD_REQUIRE(d.precision == TD_PRECISION_FP32 || d.precision == TD_PRECISION_FP16, "td_engine_create: bad precision %d", d.precision);
    TD_REQUIRE(d.pre_nms_topk >= 1 && d.pre_nms_topk <= RPN_CAND, "td_engine_create: pre_nms_topk must be in [1,%d]", RPN_CAND);
    TD_REQUIRE(d.post_nms_topk >= 1 && d.post_nms_topk <= 1024, "td_engine_create: post_nms_topk must be in [1,1024]");
    TD_REQUIRE(d.detections_per_image >= 1 && d.detections_per_image <= 1024, "td_engine_create: detections_per_image must be in [1,1024]");
    int ndev = 0;
    TD_HIP_CHECK(hipGetDeviceCount(&ndev));
    TD_REQUIRE(device >= 0 && device < ndev, "td_engine_create: device %d of %d", device, ndev);
    TD_HIP_CHECK(hipSetDevice(device));
    td_engine* e = new td_engine();
    if (const char* sbenv = getenv("TD_BACKBONE_SUBBATCH")) e->backbone_subbatch = atoi(sbenv);
    if (const char* tc = getenv("TD_TUNE_CACHE")) e->tune_cache = tc;
    if (const char* gl = getenv("TD_GROUP_LEVELS")) e->group_levels = atoi(gl) != 0;
    if (const char* ft = getenv("TD_FUSE_TAIL")) { e->fuse_tail = atoi(ft) != 0; e->fuse_tail_fp16 = atoi(ft) == 2; }
    if (const char* sp = getenv("TD_F32_SPLIT")) e->f32_split = atoi(sp);
    if (const char* spt = getenv("TD_F32_SPLIT_TAIL")) e->f32_split_tail = atoi(spt) != 0;
    if (const char* spw = getenv("TD_F32_SPLIT_WINO")) e->f32_split_wino = atoi(spw);
    e->desc = d;
    read_rule_switches(e);
    load_tune_cache(e);
    e->device = device;
    *out = e;
    return TD_OK;
}

void td_engine_destroy(td_engine* e) {
    if (!e) return;
    (void)hipSetDevice(e->device);
    free_pool(e->weight_allocs);
    free_pool(e->ws_allocs);
    if (e->tune_evict) (void)hipFree(e->tune_evict);
    for (auto& r : e->prof_recs) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
    for (auto& r : e->cls_recs) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
    for (auto ev : e->prof_free) (void)hipEventDestroy(ev);
    for (auto ev : e->phase_ev) if (ev) (void)hipEventDestroy(ev);
    if (e->prev5_ev) (void)hipEventDestroy(e->prev5_ev);
    delete e;
}

td_status td_conv_path(const int32_t* rules, int64_t wino_elems, const int32_t* layer, const int32_t* call, const int32_t* head, int32_t* out) {
    TD_REQUIRE(rules && layer && call && out && wino_elems >= 0, "td_conv_path: bad argument");
    TD_REQUIRE(call[0] >= 1 && call[1] >= 1 && call[2] >= 1 && call[3] >= 1 && layer[2] >= 1 && layer[3] >= 1, "td_conv_path: bad geometry");
    td_engine fresh;              // (a plain object: nothing of it touches the GPU) — the rules an engine created now would run by
    fresh.desc.precision = rules[0];
    fresh.wino_elems = (size_t)wino_elems;
    read_rule_switches(&fresh);
    ConvRules r = conv_rules(&fresh);
    if (rules[1] >= 0) r.winograd = rules[1] != 0;
    if (rules[2] >= 0) r.wino_fused = rules[2] != 0;
    if (rules[3] >= 0) r.wino_minc = rules[3];
    if (rules[4] >= 0) r.wino43_min = rules[4];
    if (rules[5] >= 0) r.wino_fold = rules[5];
    if (rules[6] >= 0) r.wino_slab = rules[6];
    if (rules[7] >= 0) r.fuse_head = rules[7] != 0;
    auto facts = [](const int32_t* f) { return ConvLayerFacts{f[0], f[1], f[2], f[3], f[4] != 0, f[5] != 0, f[6] != 0, f[7] != 0, f[8] != 0}; };
    const ConvSite s{facts(layer), call[0], call[1], call[2], call[3], call[4], call[5] != 0, call[6] != 0, call[7], call[8] != 0, call[9],
                     head != nullptr, head ? facts(head) : ConvLayerFacts{}};
    const ConvPath p = conv_path(r, s);
    out[0] = p.form; out[1] = p.head; out[2] = p.tune ? 1 : 0;
    for (int i = 0; i < 5; ++i) out[3 + i] = p.tune ? p.key[i] : 0;
    out[8] = p.slab_tiles; out[9] = p.fold_group;
    return TD_OK;
}

td_status td_engine_load_weights(td_engine* e, const td_tensor_desc* tensors, size_t n) {
    TD_REQUIRE(e && tensors, "td_engine_load_weights: null argument");
    TD_HIP_CHECK(hipSetDevice(e->device));
    TensorMap tm;
    for (size_t i = 0; i < n; ++i) {
        TD_REQUIRE(tensors[i].name && tensors[i].data && tensors[i].ndim >= 1 && tensors[i].ndim <= 4,
                   "td_engine_load_weights: bad tensor descriptor %zu", i);
        HostTensor t;
        t.data = tensors[i].data;
        t.shape.assign(tensors[i].shape, tensors[i].shape + tensors[i].ndim);
        tm[tensors[i].name] = t;
    }
    free_pool(e->weight_allocs);
    e->loaded = false;
    td_status st;
    // stem: [C,3,7,7] → [k = (ky*7+kx)*3 + c][C]
    {
        const HostTensor* w;
        if ((st = need(tm, "backbone.bottom_up.stem.conv1.weight", 4, &w)) < 0) return st;
        if (w->shape[1] != 3 || w->shape[2] != 7 || w->shape[3] != 7) {
            td_set_error("load_weights: stem conv must be [C,3,7,7] (RGB+nDSM tiles still feed 3 channels, prediction.py:166)");
            return TD_ERR_WEIGHTS;
        }
        e->stem_c = (int)w->shape[0];
        std::vector<float> p((size_t)147 * e->stem_c);
        for (int co = 0; co < e->stem_c; ++co)
            for (int c = 0; c < 3; ++c)
                for (int ky = 0; ky < 7; ++ky)
                    for (int kx = 0; kx < 7; ++kx)
                        p[(size_t)((ky * 7 + kx) * 3 + c) * e->stem_c + co] = w->data[(((size_t)co * 3 + c) * 7 + ky) * 7 + kx];
        if ((st = upload(e, p, &e->stem_w)) < 0) return st;
        std::vector<float> s, b;
        if ((st = bn_fold(tm, "backbone.bottom_up.stem.conv1", e->stem_c, s, b)) < 0) return st;
        if ((st = upload(e, s, &e->stem_scale)) < 0) return st;
        if ((st = upload(e, b, &e->stem_bias)) < 0) return st;
        const char* mfma_stem = getenv("TD_STEM_MFMA");              // 0 = the VALU stem for uint8 inputs too (diagnostics, tests)
        if (e->desc.precision == TD_PRECISION_FP16 && e->stem_c == 64 && !(mfma_stem && atoi(mfma_stem) == 0)) {
            std::vector<unsigned short> w16;
            std::vector<float> b16;
            stem_mfma_prepare(p.data(), s.data(), b.data(), e->stem_c, w16, b16);
            if ((st = upload(e, w16, &e->stem_w16)) < 0) return st;
            if ((st = upload(e, b16, &e->stem_bias16)) < 0) return st;
        }
    }
    for (int si = 0; si < 4; ++si) {
        e->stages[si].clear();
        for (int bi = 0;; ++bi) {
            const std::string p = "backbone.bottom_up.res" + std::to_string(si + 2) + "." + std::to_string(bi);
            if (tm.find(p + ".conv1.weight") == tm.end()) break;
            Block blk;
            blk.stride = (bi == 0 && si > 0) ? 2 : 1;
            // (the split rule: res3 - res5 only — conv2 / conv3 of res2 also exist inside bottleneck_tail_kernel; its conv2 takes the
            // split tail's bank below)
            if ((st = load_conv_bn(e, tm, p + ".conv1", blk.c1, si > 0 ? SPLIT_CONV1 : 0)) < 0) return st;
            if ((st = load_conv_bn(e, tm, p + ".conv2", blk.c2, 0, si >= 2 ? WINO_SPLIT_RES : 0)) < 0) return st;
            if ((st = load_conv_bn(e, tm, p + ".conv3", blk.c3, si > 0 ? SPLIT_CONV3 : 0)) < 0) return st;
            if (si == 0 && (st = upload_tail_split(e, pack_ohwi(tm.at(p + ".conv2.weight")), blk.c2, blk.c3.cout)) < 0) return st;
            blk.has_sc = tm.find(p + ".shortcut.weight") != tm.end();
            if (blk.has_sc && (st = load_conv_bn(e, tm, p + ".shortcut", blk.sc, si > 0 ? SPLIT_SHORTCUT : 0)) < 0) return st;
            e->stages[si].push_back(blk);
        }
        if (e->stages[si].empty()) {
            td_set_error("load_weights: no blocks found for res%d", si + 2);
            return TD_ERR_WEIGHTS;
        }
    }
    for (int l = 0; l < 4; ++l) {
        if ((st = load_conv_bias(e, tm, "backbone.fpn_lateral" + std::to_string(l + 2), e->lateral[l], SPLIT_LATERAL)) < 0) return st;
        if ((st = load_conv_bias(e, tm, "backbone.fpn_output" + std::to_string(l + 2), e->fpn_out[l], 0, WINO_SPLIT_FPN)) < 0) return st;
    }
    e->fpn_c = e->lateral[0].cout;
    if ((st = load_conv_bias(e, tm, "proposal_generator.rpn_head.conv", e->rpn_conv, 0, WINO_SPLIT_RPN)) < 0) return st;
    {
        const HostTensor *wo, *bo, *wd, *bd;
        if ((st = need(tm, "proposal_generator.rpn_head.objectness_logits.weight", 4, &wo)) < 0) return st;
        if ((st = need(tm, "proposal_generator.rpn_head.objectness_logits.bias", 1, &bo)) < 0) return st;
        if ((st = need(tm, "proposal_generator.rpn_head.anchor_deltas.weight", 4, &wd)) < 0) return st;
        if ((st = need(tm, "proposal_generator.rpn_head.anchor_deltas.bias", 1, &bd)) < 0) return st;
        if (wo->shape[0] != RPN_A || wd->shape[0] != 4 * RPN_A || wo->shape[1] != e->fpn_c || wd->shape[1] != e->fpn_c) {
            td_set_error("load_weights: RPN head must have %d anchors per position", RPN_A);
            return TD_ERR_WEIGHTS;
        }
        const int c = e->fpn_c;
        std::vector<float> w((size_t)RPN_HEAD_C * c), b(RPN_HEAD_C);
        std::memcpy(w.data(), wo->data, sizeof(float) * RPN_A * c);
        std::memcpy(w.data() + (size_t)RPN_A * c, wd->data, sizeof(float) * 4 * RPN_A * c);
        std::memcpy(b.data(), bo->data, sizeof(float) * RPN_A);
        std::memcpy(b.data() + RPN_A, bd->data, sizeof(float) * 4 * RPN_A);
        e->rpn_head.cout = RPN_HEAD_C; e->rpn_head.cin = c; e->rpn_head.kh = e->rpn_head.kw = 1;
        e->rpn_head.out_f32 = true;
        if ((st = upload_w(e, w, &e->rpn_head.w)) < 0) return st;
        if ((st = upload_frag(e, w, e->rpn_head)) < 0) return st;
        if ((st = upload(e, b, &e->rpn_head.bias)) < 0) return st;
    }
    {   // fc1: input index c*49 + y*7 + x → (y*7 + x)*C + c (RoIAlign writes NHWC rows)
        const HostTensor *w, *b;
        if ((st = need(tm, "roi_heads.box_head.fc1.weight", 2, &w)) < 0) return st;
        if ((st = need(tm, "roi_heads.box_head.fc1.bias", 1, &b)) < 0) return st;
        const int c = e->fpn_c, o = (int)w->shape[0];
        if (w->shape[1] != (int64_t)c * 49) {
            td_set_error("load_weights: fc1 expects %d inputs", c * 49);
            return TD_ERR_WEIGHTS;
        }
        std::vector<float> p((size_t)o * c * 49);
        for (int r = 0; r < o; ++r)
            for (int ch = 0; ch < c; ++ch)
                for (int q = 0; q < 49; ++q) p[(size_t)r * c * 49 + (size_t)q * c + ch] = w->data[(size_t)r * c * 49 + (size_t)ch * 49 + q];
        e->fc1.cout = o; e->fc1.cin = c * 49; e->fc1.kh = e->fc1.kw = 1;
        e->fc_dim = o;
        if ((st = upload_w(e, p, &e->fc1.w)) < 0) return st;
        if ((st = upload_frag(e, p, e->fc1)) < 0) return st;
        if ((st = upload_split(e, p, e->fc1, SPLIT_FC)) < 0) return st;
        if ((st = upload(e, std::vector<float>(b->data, b->data + o), &e->fc1.bias)) < 0) return st;
    }
    {
        const HostTensor *w, *b;
        if ((st = need(tm, "roi_heads.box_head.fc2.weight", 2, &w)) < 0) return st;
        if ((st = need(tm, "roi_heads.box_head.fc2.bias", 1, &b)) < 0) return st;
        e->fc2.cout = (int)w->shape[0]; e->fc2.cin = (int)w->shape[1]; e->fc2.kh = e->fc2.kw = 1;
        const std::vector<float> w2v(w->data, w->data + w->numel());
        if ((st = upload_w(e, w2v, &e->fc2.w)) < 0) return st;
        if ((st = upload_frag(e, w2v, e->fc2)) < 0) return st;
        if ((st = upload_split(e, w2v, e->fc2, SPLIT_FC)) < 0) return st;
        if ((st = upload(e, std::vector<float>(b->data, b->data + e->fc2.cout), &e->fc2.bias)) < 0) return st;
    }
    {
        const HostTensor *wc, *bc, *wr, *br;
        if ((st = need(tm, "roi_heads.box_predictor.cls_score.weight", 2, &wc)) < 0) return st;
        if ((st = need(tm, "roi_heads.box_predictor.cls_score.bias", 1, &bc)) < 0) return st;
        if ((st = need(tm, "roi_heads.box_predictor.bbox_pred.weight", 2, &wr)) < 0) return st;
        if ((st = need(tm, "roi_heads.box_predictor.bbox_pred.bias", 1, &br)) < 0) return st;
        if (wc->shape[0] != 2 || wr->shape[0] != 4) {
            td_set_error("load_weights: box predictor must be 1 class (+background), got cls %lld / reg %lld rows",
                         (long long)wc->shape[0], (long long)wr->shape[0]);
            return TD_ERR_WEIGHTS;
        }
        const int k = (int)wc->shape[1];
        std::vector<float> w((size_t)6 * k), b(6);
        std::memcpy(w.data(), wc->data, sizeof(float) * 2 * k);
        std::memcpy(w.data() + (size_t)2 * k, wr->data, sizeof(float) * 4 * k);
        std::memcpy(b.data(), bc->data, sizeof(float) * 2);
        std::memcpy(b.data() + 2, br->data, sizeof(float) * 4);
        e->pred.cout = 6; e->pred.cin = k; e->pred.kh = e->pred.kw = 1;
        e->pred.out_f32 = true;
        if ((st = upload_w(e, w, &e->pred.w)) < 0) return st;
        if ((st = upload_frag(e, w, e->pred)) < 0) return st;
        if ((st = upload(e, b, &e->pred.bias)) < 0) return st;
    }
    for (int i = 0; i < 4; ++i)
        if ((st = load_conv_bias(e, tm, "roi_heads.mask_head.mask_fcn" + std::to_string(i + 1), e->mask_fcn[i])) < 0) return st;
    {   // ConvTranspose2d weight [Cin,Cout,2,2] → rows n = (dy*2+dx)*Cout + co over Cin
        const HostTensor *w, *b;
        if ((st = need(tm, "roi_heads.mask_head.deconv.weight", 4, &w)) < 0) return st;
        if ((st = need(tm, "roi_heads.mask_head.deconv.bias", 1, &b)) < 0) return st;
        const int ci = (int)w->shape[0], co = (int)w->shape[1];
        if (w->shape[2] != 2 || w->shape[3] != 2) {
            td_set_error("load_weights: mask deconv must be 2x2");
            return TD_ERR_WEIGHTS;
        }
        std::vector<float> p((size_t)4 * co * ci);
        for (int i = 0; i < ci; ++i)
            for (int o = 0; o < co; ++o)
                for (int q = 0; q < 4; ++q) p[((size_t)q * co + o) * ci + i] = w->data[((size_t)i * co + o) * 4 + q];
        e->deconv.cout = 4 * co; e->deconv.cin = ci; e->deconv.kh = e->deconv.kw = 1;
        if ((st = upload_w(e, p, &e->deconv.w)) < 0) return st;
        if ((st = upload(e, std::vector<float>(b->data, b->data + co), &e->deconv.bias)) < 0) return st;
    }
    {
        const HostTensor *w, *b;
        if ((st = need(tm, "roi_heads.mask_head.predictor.weight", 4, &w)) < 0) return st;
        if ((st = need(tm, "roi_heads.mask_head.predictor.bias", 1, &b)) < 0) return st;
        if (w->shape[0] != 1) {
            td_set_error("load_weights: mask predictor must have 1 output channel");
            return TD_ERR_WEIGHTS;
        }
        if ((st = upload(e, std::vector<float>(w->data, w->data + w->shape[1]), &e->mask_pred_w)) < 0) return st;
        e->mask_pred_b = b->data[0];
    }
    e->loaded = true;
    return TD_OK;
}

td_status td_engine_reserve(td_engine* e, int B, int Hp, int Wp) {
    TD_REQUIRE(e, "td_engine_reserve: null engine");
    TD_REQUIRE(e->loaded, "td_engine_reserve: load weights first");
    TD_REQUIRE(B >= 1 && B <= TD_MAX_BATCH, "td_engine_reserve: batch %d not in [1,%d]", B, TD_MAX_BATCH);
    TD_REQUIRE(Hp >= 64 && Wp >= 64 && Hp % 32 == 0 && Wp % 32 == 0, "td_engine_reserve: padded size %dx%d must be multiples of 32 (>= 64)", Hp, Wp);
    if (B <= e->rB && Hp <= e->rHp && Wp <= e->rWp) return TD_OK;   // current plan already covers it
    B = B > e->rB ? B : e->rB;
    Hp = Hp > e->rHp ? Hp : e->rHp;
    Wp = Wp > e->rWp ? Wp : e->rWp;
    TD_HIP_CHECK(hipSetDevice(e->device));
    free_pool(e->ws_allocs);
    e->named.clear();           // the names of the last forward point into what was just freed
    e->rB = e->rHp = e->rWp = 0;
    const WsGeom g = engine_geom(e, B, Hp, Wp);
    e->wino_v = e->wino_m = nullptr;
    for (size_t k = 0; k < ws_row_count(g); ++k)
        for (int i = 0; i < ws_rows()[k].count; ++i)
            if (td_status st = dev_alloc(e->ws_allocs, ws_slot(e, ws_rows()[k], i), ws_alloc_bytes(ws_rows()[k], g, i)); st < 0) return st;
    e->wino_elems = ws_wino_elems(g);
    e->rB = B;
    e->rHp = Hp;
    e->rWp = Wp;
    return TD_OK;
}

}  // extern "C"

namespace {

// Times `launch` on the live buffers (idempotent: same inputs, same outputs); launches shorter than ~100 us are timed again
// over a longer run (event granularity and clock ramps otherwise pick the wrong tile for them).
td_status time_launch(td_engine* e, hipStream_t s, hipEvent_t ea, hipEvent_t eb, const std::function<td_status()>& launch, float* ms_out) {
    td_status st = launch();
    if (st < 0) return st;
    static const bool evict = !(getenv("TD_TUNE_EVICT") && atoi(getenv("TD_TUNE_EVICT")) == 0);
    if (evict && !e->tune_evict) {      // one launch per timed interval, L2 emptied before it; the fastest of five
        e->tune_evict_bytes = (size_t)64 << 20;
        if (hipMalloc(&e->tune_evict, e->tune_evict_bytes) != hipSuccess) {      // no room for the scratch: time the hot loop instead
            (void)hipGetLastError();
            e->tune_evict = nullptr;
            e->tune_evict_bytes = 0;
        }
    }
    const bool cold = evict && e->tune_evict;       // cold: five rounds of one launch; hot: 2 launches, then 8 when under 0.1 ms
    float ms = 1e30f;
    for (int round = 0, reps = cold ? 1 : 2; round < (cold ? 5 : 2); ++round, reps = cold ? 1 : 8) {
        if (cold) TD_HIP_CHECK(hipMemsetAsync(e->tune_evict, round, e->tune_evict_bytes, s));
        TD_HIP_CHECK(hipEventRecord(ea, s));
        for (int rep = 0; rep < reps; ++rep)
            if ((st = launch()) < 0) return st;
        TD_HIP_CHECK(hipEventRecord(eb, s));
        TD_HIP_CHECK(hipEventSynchronize(eb));
        float t = 0.f;
        TD_HIP_CHECK(hipEventElapsedTime(&t, ea, eb));
        t /= (float)reps;
        if (t < ms) ms = t;
        if (!cold && ms > 0.1f) break;
    }
    *ms_out = ms;
    return TD_OK;
}

// Measured block tile of one launch shape (cached per engine, shared through the TD_TUNE_CACHE file). The candidates are the
// tiles of TD_CONV_TILES with a tuning rank, in rank order, within their tuning limits and able to run `a` — the ConvArgs the
// timed launch carries — so the id recorded is the tile that ran. launch_cfg(id) runs the launch on tile id.
td_status tuned_cfg(td_engine* e, const std::tuple<int, int, int, int, int>& key, int prec, const ConvArgs& a, hipStream_t s,
                    const std::function<td_status(int)>& launch_cfg, int* cfg_out) {
    const int ksteps = a.KH * a.KW * a.Cin / (prec == TD_PRECISION_FP16 ? 64 : 32);
    auto candidate = [&](int id) {
        const ConvTile* t = conv_tile(id);
        // a launch with the split bank is one of the split rule's layers: it times the TILE_SPLIT ids and nothing else, every other
        // launch never times one (conv_tile_refusal: no bank) — which rounding a layer gets is the rule's decision, not a timing's
        return t && (t->family == TILE_SPLIT) == (a.w_split != nullptr) && (!t->max_ksteps || ksteps <= t->max_ksteps) && a.Cout >= t->min_cout && (!t->max_cout || a.Cout <= t->max_cout) &&
               !conv_tile_refusal(id, a, prec);
    };
    static const int forced = getenv("TD_FORCE_CFG") ? atoi(getenv("TD_FORCE_CFG")) : -1;      // diagnostics: one block tile everywhere it applies
    if (candidate(forced)) {
        *cfg_out = forced;
        return TD_OK;
    }
    auto it = e->tuned.find(key);
    if (it == e->tuned.end()) {
        load_tune_cache(e);                   // another engine of this process may have measured it meanwhile
        it = e->tuned.find(key);
    }
    if (it != e->tuned.end()) {
        *cfg_out = it->second;
        return TD_OK;
    }
    std::vector<int> order;
    for (const ConvTile& t : TD_CONV_TILES)
        if (t.tune_rank >= 0 && candidate((int)(&t - TD_CONV_TILES))) order.push_back((int)(&t - TD_CONV_TILES));
    std::sort(order.begin(), order.end(), [](int x, int y) { return TD_CONV_TILES[x].tune_rank < TD_CONV_TILES[y].tune_rank; });
    float best = 1e30f;
    int best_cfg = -1;
    hipEvent_t ea, eb;
    TD_HIP_CHECK(hipEventCreate(&ea));
    TD_HIP_CHECK(hipEventCreate(&eb));
    td_status st = TD_OK;
    for (int c : order) {
        float ms = 1e30f;
        if ((st = time_launch(e, s, ea, eb, [&]() { return launch_cfg(c); }, &ms)) < 0) break;
        static const float hyst = 1.f - 0.01f * (getenv("TD_TUNE_HYST") ? (float)atof(getenv("TD_TUNE_HYST")) : 2.f);
        if (best_cfg < 0 || ms < best * hyst) { best = ms; best_cfg = c; }
    }
    (void)hipEventDestroy(ea);
    (void)hipEventDestroy(eb);
    if (st < 0) return st;
    e->tuned.emplace(key, best_cfg);
    if (FILE* f = e->tune_cache.empty() ? nullptr : fopen(e->tune_cache.c_str(), "a")) {
        fprintf(f, "%d %d %d %d %d %d %d\n", prec, std::get<0>(key), std::get<1>(key), std::get<2>(key), std::get<3>(key), std::get<4>(key), best_cfg);
        fclose(f);
    }
    *cfg_out = best_cfg;
    return TD_OK;
}

// The engine's books of every launch of a Winograd sequence (wino_run's hook): a class bracket per step, priced by launch_cost.h
struct WinoBooks {
    td_engine* e;
    hipStream_t s;
    const ConvSite& site;
    const ConvPath& path;
    bool head_fused;
    std::optional<ProfScope> ps;
    static void begin(void* ctx, int step, long long n) {
        WinoBooks& k = *static_cast<WinoBooks*>(ctx);
        k.ps.emplace(k.e, k.s, wino_step_cost(k.site, k.path, k.e->wino_fused, k.head_fused, step, n));
    }
    static void end(void* ctx) { static_cast<WinoBooks*>(ctx)->ps.reset(); }
};

ConvLayerFacts layer_facts(const ConvLayer& L) {
    return {L.cout, L.cin, L.kh, L.kw, L.scale != nullptr, L.out_f32, L.wino_u != nullptr, L.wino_u43 != nullptr, L.w_split != nullptr || L.wino_u43_split != nullptr};
}

// One contraction of the forward: ask conv_path which form the layer takes, measure the block tile of the launch shape it names
// (tuning launches enter no books), book the launch (launch_cost.h), launch. head (optional): the 1x1 layer that is this layer's
// only consumer — *head_fused tells the caller whether it rode along (head_y written, y_ not) or still needs a launch of its own.
td_status run_conv(td_engine* e, const ConvLayer& L, const void* x_, int B_, int H_, int W_, int stride, int pad, bool relu, void* y_,
                   const void* res_, int res_shift, hipStream_t s_, const int* m_dyn = nullptr, int m_mul = 1, int out_mode = 0,
                   const ConvLayer* head = nullptr, float* head_y = nullptr, bool* head_fused = nullptr) {
    const int prec_ = e->desc.precision;
    const ConvSite site{layer_facts(L), B_, H_, W_, stride, pad, relu, res_ != nullptr, out_mode, m_dyn != nullptr, m_mul,
                        head != nullptr, head ? layer_facts(*head) : ConvLayerFacts{}};
    const ConvPath path = conv_path(conv_rules(e), site);
    const bool use_wino = path.form >= CONV_WINO22, use_43 = path.form >= CONV_WINO43;
    const int Ho = (H_ + 2 * pad - L.kh) / stride + 1, Wo = (W_ + 2 * pad - L.kw) / stride + 1;
    td_status st2;
    ConvArgs ca{};          // the direct launch (tuned tile, fused head below)
    ca.x = x_; ca.w = L.w; ca.w_frag = L.w_frag; ca.w_split = path.form == CONV_SPLIT ? L.w_split : nullptr; ca.scale = L.scale; ca.bias = L.bias; ca.res = res_; ca.y = y_;
    ca.B = B_; ca.H = H_; ca.W = W_; ca.Cin = L.cin; ca.Cout = L.cout; ca.KH = L.kh; ca.KW = L.kw;
    ca.stride = stride; ca.pad = pad; ca.Ho = Ho; ca.Wo = Wo;
    ca.res_shift = res_shift; ca.relu = relu ? 1 : 0; ca.out_mode = out_mode;
    ca.M = B_ * Ho * Wo; ca.m_dyn = m_dyn; ca.m_mul = m_mul; ca.tile_cfg = -1; ca.out_f32 = L.out_f32 ? 1 : 0;
    WinoRun wr{};           // the Winograd sequence (wino_seq.cpp)
    if (use_wino) {
        wr.form = path.form; wr.fused_input = e->wino_fused; wr.slab_tiles = path.slab_tiles; wr.fold_group = path.fold_group;
        wr.x = static_cast<const float*>(x_); wr.U = use_43 ? L.wino_u43 : L.wino_u; wr.scale = L.scale; wr.bias = L.bias; wr.y = static_cast<float*>(y_);
        wr.B = B_; wr.H = H_; wr.W = W_; wr.cin = L.cin; wr.cout = L.cout; wr.relu = relu ? 1 : 0;
        wr.V = e->wino_v; wr.M = e->wino_m; wr.m_dyn = m_dyn; wr.m_mul = m_mul; wr.gemm_cfg = -1;
        wr.U_split = path.split_planes ? L.wino_u43_split : nullptr;
    }
    if (path.tune) {
        const auto key = std::make_tuple(path.key[0], path.key[1], path.key[2], path.key[3], path.key[4]);
        if (use_wino) {     // the batched plane contraction is a launch shape of its own; timed inside the whole sequence, head apart
            auto wino = [&](int c) { WinoRun q = wr; q.gemm_cfg = c; return wino_run(q, s_); };
            st2 = tuned_cfg(e, key, prec_, use_43 ? wino43_plane_args(wr) : wino_plane_args(wr, path.key[3], 0), s_, wino, &wr.gemm_cfg);
        } else {
            auto direct = [&](int c) { ConvArgs a = ca; a.tile_cfg = c; return conv2d_launch(a, prec_, s_); };
            st2 = tuned_cfg(e, key, prec_, ca, s_, direct, &ca.tile_cfg);
        }
        if (st2 < 0) return st2;
    }
    // the head rides along: by the rule, or (bit-identical either way) when the measured tile owns all 256 output channels
    const bool fuse_head = path.head == HEAD_IN_TRANSFORM || (path.head == HEAD_IF_TILE_OWNS_256 && conv_head_capable(ca.tile_cfg, prec_));
    if (head_fused) *head_fused = fuse_head;
    ProfScope ps(e, s_, conv_cost(prec_, site, path, fuse_head));        // a Winograd layer: the sequence; its steps book their classes
    if (use_wino) {
        if (fuse_head) { wr.head_w = static_cast<const float*>(head->w); wr.head_b = head->bias; wr.head_y = head_y; wr.head_n = head->cout; }
        WinoBooks books{e, s_, site, path, fuse_head, std::nullopt};
        const WinoHook hook{&books, WinoBooks::begin, WinoBooks::end};
        return wino_run(wr, s_, e->prof ? &hook : nullptr);
    }
    if (fuse_head) { ca.head_w = head->w; ca.head_b = head->bias; ca.head_y = head_y; ca.head_n = head->cout; }
    return conv2d_launch(ca, prec_, s_);
}

// The forward in six phases. Contractions (0 trunk: stem..RPN heads, 2 box-head FCs, 4 mask-head convs) and the
// low-occupancy selection work (1 RPN top-k/NMS/merge + RoIAlign 7x7, 3 detections + RoIAlign 14x14, 5 mask
// predictor/scatter/paste) alternate, so a caller can keep three batches in flight: contraction phases of successive
// batches back to back on a main stream, selection phases on a side stream where they overlap the next contractions.
td_status forward_impl(td_engine* e, unsigned phase_mask, hipStream_t s) {
    const td_engine::FwdCtx& c = e->ctx;
    const void* images = c.images;
    const int input_format = c.input_format, B = c.B, Hp = c.Hp, Wp = c.Wp;
    const ImgSizes& valid = c.valid;
    const ImgSizes& outsz = c.outsz;
    const td_detections* out = &c.out;
    const int prec = e->desc.precision;
    auto PH = [&](int k) { return (phase_mask >> k) & 1u; };
    if (PH(0)) e->named.clear();
    td_status st;
    // The same 3x3 layer shape on several pyramid levels as ONE launch (conv_pp8_grouped_launch, fp16 engine): the FPN's output
    // convs, the RPN conv with its head. The small levels (p4-p6: 79 / 20 / 6 tiles of 256 rows) cannot fill 256 CUs on their own;
    // in one grid their tiles run beside the big levels' last wave. A fixed rule (layer shapes only); bit-identical per level.
    auto groupable = [&](const ConvLayer& L) {
        return L.kh == 3 && L.kw == 3 && L.cout == 256 && L.cin % 64 == 0 && !L.scale && L.bias && !L.out_f32;
    };
    auto run_grouped = [&](const ConvLayer* const* Ls, const void* const* xs, void* const* ys, float* const* head_ys, int nl, const int* Hs,
                           const int* Ws, bool relu, const ConvLayer* head, hipStream_t s_) -> td_status {
        ConvArgs a{};
        a.B = B; a.Cin = Ls[0]->cin; a.Cout = 256; a.KH = a.KW = 3; a.stride = 1; a.pad = 1; a.relu = relu ? 1 : 0; a.m_mul = 1; a.nlev = nl;
        a.tile_cfg = 17;
        for (int l = 0; l < nl; ++l) {
            a.lev[l].x = xs[l]; a.lev[l].w = Ls[l]->w; a.lev[l].bias = Ls[l]->bias;
            a.lev[l].y = ys ? ys[l] : nullptr; a.lev[l].head_y = head_ys ? head_ys[l] : nullptr;
            a.lev[l].H = Hs[l]; a.lev[l].W = Ws[l];
        }
        if (head) { a.head_w = head->w; a.head_b = head->bias; a.head_n = head->cout; }
        ProfScope ps(e, s_, grouped_cost(B, a.Cin, Hs, Ws, nl, head ? head->cout : 0));
        return conv_pp8_grouped_launch(a, s_);
    };
    // conv2 (3x3) → conv3 (1x1) + shortcut + ReLU of a bottleneck block as one launch (bottleneck_tail_kernel)
    // split_ (the res2 blocks of the fp32 engine under f32_split_tail): the 3x3 on the bf16 matrix cores. mid_out_ set: that kernel's
    // mid-store launch, the unfused twin's conv2 (t2 written, no conv3)
    auto run_tail = [&](const Block& blk, const void* t1_, int B_, int H_, int W_, void* y_, const void* shortcut_, hipStream_t s_,
                        bool split_ = false, void* mid_out_ = nullptr) -> td_status {
        TailArgs a{};
        a.x = t1_; a.w2 = blk.c2.w; a.scale2 = blk.c2.scale; a.bias2 = blk.c2.bias;
        a.w3 = blk.c3.w; a.scale3 = blk.c3.scale; a.bias3 = blk.c3.bias; a.res = shortcut_; a.y = y_;
        a.B = B_; a.H = H_; a.W = W_; a.MID = blk.c2.cout; a.COUT = blk.c3.cout; a.M = B_ * H_ * W_;
        if (split_) a.w2_split = blk.c2.w_tail_split;
        if (mid_out_) {
            a.mid_out = static_cast<float*>(mid_out_);
            a.w3 = nullptr; a.scale3 = nullptr; a.bias3 = nullptr; a.res = nullptr; a.y = nullptr;
        }
        ProfScope ps(e, s_, tail_cost(prec, a.M, a.MID, a.COUT, split_, mid_out_ != nullptr));
        return bottleneck_tail_launch(a, prec, s_);
    };
    // ---- backbone ------------------------------------------------------------------------------------------
    // Runs in sub-batches of `sb` images (stem → res5 per sub-batch): the stage-2/3 activations of a sub-batch
    // (≈ 80 MB per 256-channel tensor and image at fp32) then hand over from layer to layer through the 256 MiB
    // Infinity Cache instead of HBM. sb comes from TD_BACKBONE_SUBBATCH (default: the whole batch at once).
    const WsGeom g = engine_geom(e, B, Hp, Wp);
    const int *hs = g.h, *wsz = g.w;
    auto off = [&](void* p, size_t elems) -> void* { return static_cast<char*>(p) + elems * g.es; };
    int sb = e->backbone_subbatch > 0 ? e->backbone_subbatch : B;
    if (sb > B) sb = B;
    const bool do_stem = PH(6) || (PH(0) && !e->stem_done);
    // ONE event pair around the whole trunk (backbone, FPN, RPN convs): every hipEventRecord is a kernel boundary with a
    // signal on the main stream, and the fp16 trunk is short enough to notice each of them (un-profiled 4.87 ms per step,
    // 5.11 ms with a pair per section). The p6 subsample (5 us) falls inside the bracket and is timed with the convs.
    std::optional<ProfScope> trunk_group;
    for (int b0 = 0; (PH(0) || PH(6)) && b0 < B; b0 += sb) {
        const int nb_img = (B - b0) < sb ? (B - b0) : sb;
        ImgSizes vsub{};
        for (int i = 0; i < nb_img; ++i) {
            vsub.h[i] = valid.h[b0 + i];
            vsub.w[i] = valid.w[b0 + i];
        }
        const size_t in_img = input_format == TD_INPUT_U8_HWC ? (size_t)Hp * Wp * 3 : (size_t)Hp * Wp * 3 * 4;
        const void* img_sub = static_cast<const char*>(images) + (size_t)b0 * in_img;
        void* stem_sub = off(e->stem_out, (size_t)b0 * (Hp / 2) * (Wp / 2) * e->stem_c);
        void* pool_sub = off(e->pool_out, (size_t)b0 * hs[0] * wsz[0] * e->stem_c);
        if (do_stem) {
            { ProfScope ps(e, s, 1);
            if ((st = stem_launch(img_sub, input_format, vsub, nb_img, Hp, Wp, e->stem_w, e->stem_scale, e->stem_bias, stem_sub,
                                  e->stem_c, prec, s, e->stem_w16, e->stem_bias16)) < 0) return st; }
            { ProfScope ps(e, s, 2);
            if ((st = maxpool3x3s2_launch(stem_sub, pool_sub, nb_img, Hp / 2, Wp / 2, e->stem_c, prec, s)) < 0) return st; }
        }
        if (!PH(0)) continue;
        if (!trunk_group && sb >= B) trunk_group.emplace(e, s, 0, true);
        const void* x = pool_sub;
        int xh = hs[0], xw = wsz[0];
        ProfScope backbone_group(e, s, 0, true);
        for (int si = 0; si < 4; ++si) {
            const int nb = (int)e->stages[si].size();
            const int oh = hs[si], ow = wsz[si];
            const size_t px = (size_t)b0 * oh * ow;
            const int mid = e->stages[si][0].c1.cout, co = e->stages[si][0].c3.cout;
            void* t1 = off(e->t1[si], px * mid);
            void* t2 = off(e->t2[si], px * mid);
            void* scb = off(e->scb[si], px * co);
            void* resb = off(e->res[si], px * co);
            void* xtmp = off(e->xtmp[si], px * co);
            for (int bi = 0; bi < nb; ++bi) {
                const Block& blk = e->stages[si][bi];
                // the last block must land in res[si]: alternate so that block nb-1 writes res
                void* y = ((nb - 1 - bi) % 2 == 0) ? resb : xtmp;
                const void* shortcut = x;
                if (blk.has_sc) {
                    if ((st = run_conv(e, blk.sc, x, nb_img, xh, xw, blk.stride, 0, false, scb, nullptr, 0, s)) < 0) return st;
                    shortcut = scb;
                }
                if ((st = run_conv(e, blk.c1, x, nb_img, xh, xw, blk.stride, 0, true, t1, nullptr, 0, s)) < 0) return st;
                // Measured (round 3, plain loop, batch 8, 64-row blocks): fp32 res2 345 us fused against 215 + 185 us as two launches;
                // fp16 res2 130 us against 54 + 87; fp16 res3 111 us against 41 + 47 — slower (a fused block is a chain of short
                // latency-bound steps, and with 128 mid channels only two blocks fit a CU), so res3 fuses only on request
                // (TD_FUSE_TAIL=2). Either way the result is bit-identical, so this IS allowed to follow a measurement.
                // The split tail (f32_split_tail: fp32 engine, res2): a fixed rule on the layer — it has the bank — and the launch's
                // size; fused or not, conv2 is bottleneck_tail_kernel's split form (the mid-store launch below is the fused launch's
                // phases 1 and 2), so the two stay bit-identical here too.
                const bool tail_shape = blk.c2.kh == 3 && blk.c2.kw == 3 && blk.c2.cin == blk.c2.cout && blk.c3.cin == blk.c2.cout &&
                                        bottleneck_tail_ok(prec, blk.c2.cout, blk.c3.cout);
                const bool split_tail = tail_shape && blk.c2.w_tail_split &&
                                        bottleneck_tail_split_ok(prec, blk.c2.cout, blk.c3.cout, (long long)nb_img * oh * ow);
                if (e->fuse_tail && (blk.c2.cout == 64 || e->fuse_tail_fp16) && tail_shape) {
                    // conv2 + conv3 + shortcut add in one launch, bit-identical to the two launches below (bottleneck.hip); the mid
                    // tensor t2 never reaches HBM
                    if ((st = run_tail(blk, t1, nb_img, oh, ow, y, shortcut, s, split_tail)) < 0) return st;
                } else if (split_tail) {
                    if ((st = run_tail(blk, t1, nb_img, oh, ow, nullptr, nullptr, s, true, t2)) < 0) return st;
                    if ((st = run_conv(e, blk.c3, t2, nb_img, oh, ow, 1, 0, true, y, shortcut, 0, s)) < 0) return st;
                } else {
                    if ((st = run_conv(e, blk.c2, t1, nb_img, oh, ow, 1, 1, true, t2, nullptr, 0, s)) < 0) return st;
                    if ((st = run_conv(e, blk.c3, t2, nb_img, oh, ow, 1, 0, true, y, shortcut, 0, s)) < 0) return st;
                }
                x = y;
                xh = oh;
                xw = ow;
            }
        }
    }
    if (PH(0)) {
    // ---- FPN (top-down; the nearest-2x upsampled add rides in the lateral conv's epilogue) ---------------------
    {
    ProfScope fpn_group(e, s, 0, true);
    // fp16: the four output convs do not depend on each other (only the lateral sums chain top-down), so the laterals run first
    // and the outputs follow as one grouped launch
    const bool group_fpn = prec == TD_PRECISION_FP16 && e->group_levels && groupable(e->fpn_out[0]) && groupable(e->fpn_out[1]) &&
                           groupable(e->fpn_out[2]) && groupable(e->fpn_out[3]);
    for (int l = 3; l >= 0; --l) {
        const void* td_res = l == 3 ? nullptr : e->inner[l + 1];
        if ((st = run_conv(e, e->lateral[l], e->res[l], B, hs[l], wsz[l], 1, 0, false, e->inner[l], td_res, td_res ? 1 : 0, s)) < 0) return st;
        if (!group_fpn && (st = run_conv(e, e->fpn_out[l], e->inner[l], B, hs[l], wsz[l], 1, 1, false, e->pfeat[l], nullptr, 0, s)) < 0) return st;
    }
    if (group_fpn) {
        const ConvLayer* Ls[4] = {&e->fpn_out[0], &e->fpn_out[1], &e->fpn_out[2], &e->fpn_out[3]};
        const void* xs[4] = {e->inner[0], e->inner[1], e->inner[2], e->inner[3]};
        void* ys[4] = {e->pfeat[0], e->pfeat[1], e->pfeat[2], e->pfeat[3]};
        if ((st = run_grouped(Ls, xs, ys, nullptr, 4, hs, wsz, false, nullptr, s)) < 0) return st;
    }
    }
    { ProfScope ps(e, s, 2);
    if ((st = subsample2_launch(e->pfeat[3], e->pfeat[4], B, hs[3], wsz[3], e->fpn_c, prec, s)) < 0) return st; }
    // ---- RPN -----------------------------------------------------------------------------------------------------
    {
        ProfScope rpn_group(e, s, 0, true);
        const bool group_rpn = prec == TD_PRECISION_FP16 && e->group_levels && e->fuse_head && groupable(e->rpn_conv) && e->rpn_head.cin == 256 &&
                               e->rpn_head.kh == 1 && e->rpn_head.kw == 1 && e->rpn_head.cout <= 32 && e->rpn_head.out_f32 && !e->rpn_head.scale;
        if (group_rpn) {
            const ConvLayer* Ls[5] = {&e->rpn_conv, &e->rpn_conv, &e->rpn_conv, &e->rpn_conv, &e->rpn_conv};
            const void* xs[5] = {e->pfeat[0], e->pfeat[1], e->pfeat[2], e->pfeat[3], e->pfeat[4]};
            float* hy[5] = {e->rpn_headbuf[0], e->rpn_headbuf[1], e->rpn_headbuf[2], e->rpn_headbuf[3], e->rpn_headbuf[4]};
            if ((st = run_grouped(Ls, xs, nullptr, hy, 5, hs, wsz, true, &e->rpn_head, s)) < 0) return st;
        }
        for (int l = 0; l < 5 && !group_rpn; ++l) {
            bool fused = false;
            if ((st = run_conv(e, e->rpn_conv, e->pfeat[l], B, hs[l], wsz[l], 1, 1, true, e->rpn_t, nullptr, 0, s, nullptr, 1, 0,
                               &e->rpn_head, e->rpn_headbuf[l], &fused)) < 0) return st;
            if (!fused && (st = run_conv(e, e->rpn_head, e->rpn_t, B, hs[l], wsz[l], 1, 0, false, e->rpn_headbuf[l], nullptr, 0, s)) < 0) return st;
        }
    }
    trunk_group.reset();
    }   // phase 0
    RpnLevels lv{};
    {
        static const int sizes[5] = {32, 64, 128, 256, 512};
        static const double ratios[3] = {0.5, 1.0, 2.0};
        int off = 0;
        for (int l = 0; l < 5; ++l) {
            lv.head[l] = e->rpn_headbuf[l];
            lv.h[l] = hs[l];
            lv.w[l] = wsz[l];
            lv.stride[l] = 4 << l;
            lv.anchor_off[l] = off;
            off += hs[l] * wsz[l] * RPN_A;
            const double area = (double)sizes[l] * sizes[l];
            for (int a = 0; a < 3; ++a) {
                const double w = std::sqrt(area / ratios[a]);
                const double h = ratios[a] * w;
                lv.base[l][a][0] = (float)(-w / 2.0);
                lv.base[l][a][1] = (float)(-h / 2.0);
                lv.base[l][a][2] = (float)(w / 2.0);
                lv.base[l][a][3] = (float)(h / 2.0);
            }
        }
        lv.total_anchors = off;
    }
    const int P = g.P, D = g.D, mrows = g.mrows;
    FeatLevels fl{};
    for (int l = 0; l < 4; ++l) {
        fl.feat[l] = e->pfeat[l];
        fl.h[l] = hs[l];
        fl.w[l] = wsz[l];
        fl.scale[l] = 1.0f / (float)(4 << l);
    }
    fl.C = e->fpn_c;
    float* o_boxes = out->boxes ? out->boxes : e->o_boxes;
    float* o_scores = out->scores ? out->scores : e->o_scores;
    int* o_classes = out->classes ? out->classes : e->o_classes;
    int* o_count = out->count ? out->count : e->o_count;
    float* o_probs = out->mask_probs ? out->mask_probs : e->o_mask_probs;
    if (PH(1)) {
    { ProfScope ps(e, s, 3);
    if ((st = rpn_topk_decode_launch(lv, valid, B, e->desc.pre_nms_topk, e->key_ws, e->cand_boxes, e->cand_scores,
                                     e->cand_valid, e->cand_idx, s)) < 0) return st; }
    { ProfScope ps(e, s, 3);
    if ((st = nms_launch(e->cand_boxes, nullptr, e->cand_valid, B * RPN_LEVELS, RPN_CAND, e->desc.rpn_nms_thresh,
                         e->nms_mask, e->rpn_keep, e->rpn_keep_count, RPN_CAND, s)) < 0) return st; }
    { ProfScope ps(e, s, 3);
    if ((st = rpn_merge_launch(e->cand_boxes, e->cand_scores, e->rpn_keep, e->rpn_keep_count, B, P, e->props,
                               e->prop_scores, e->prop_count, P, s)) < 0) return st; }
    // ---- box head -----------------------------------------------------------------------------------------------
    { ProfScope ps(e, s, 4);
    if ((st = roi_align_launch(fl, e->props, e->prop_count, B, P, 7, 0, e->pooled7, nullptr, prec, s)) < 0) return st; }
    }   // phase 1
    if (PH(2)) {
    {
    ProfScope box_group(e, s, 0, true);
    if ((st = run_conv(e, e->fc1, e->pooled7, B * P, 1, 1, 1, 0, true, e->fc1_out, nullptr, 0, s)) < 0) return st;
    if ((st = run_conv(e, e->fc2, e->fc1_out, B * P, 1, 1, 1, 0, true, e->fc2_out, nullptr, 0, s)) < 0) return st;
    if ((st = run_conv(e, e->pred, e->fc2_out, B * P, 1, 1, 1, 0, false, e->pred_out, nullptr, 0, s)) < 0) return st;
    }
    }   // phase 2
    if (PH(3)) {
    { ProfScope ps(e, s, 5);
    if ((st = det_decode_launch(e->pred_out, 6, e->props, e->prop_count, valid, B, P, e->desc.score_thresh, e->dboxes,
                                e->dscores, e->dflags, s)) < 0) return st; }
    { ProfScope ps(e, s, 5);
    if ((st = sort_boxes_launch(e->dboxes, e->dscores, e->dflags, e->prop_count, B, P, e->sboxes, e->sscores, e->sidx,
                                e->scount, s)) < 0) return st; }
    { ProfScope ps(e, s, 5);
    if ((st = nms_launch(e->sboxes, e->scount, nullptr, B, P, e->desc.nms_thresh, e->nms_mask, e->det_keep,
                         e->det_keep_count, D, s)) < 0) return st; }
    { ProfScope ps(e, s, 5);
    if ((st = det_finalize_launch(e->sboxes, e->sscores, e->det_keep, e->det_keep_count, valid, outsz, B, P, D,
                                  e->det_boxes_net, o_boxes, o_scores, o_classes, o_count, s)) < 0) return st; }
    // ---- mask head (compact rows: only live detections are computed) ------------------------------------------
    { ProfScope ps(e, s, 4);
    if ((st = roi_align_launch(fl, e->det_boxes_net, o_count, B, D, 14, 1, e->pooled14, e->total_rows, prec, s)) < 0) return st; }
    }   // phase 3
    if (PH(4)) {
    const void* mx = e->pooled14;
    void* mbuf[2] = {e->mbuf0, e->mbuf1};
    {
    ProfScope mask_group(e, s, 7, true);
    for (int i = 0; i < 4; ++i) {
        if ((st = run_conv(e, e->mask_fcn[i], mx, mrows, 14, 14, 1, 1, true, mbuf[i & 1], nullptr, 0, s, e->total_rows, 196)) < 0) return st;
        mx = mbuf[i & 1];
    }
    if ((st = run_conv(e, e->deconv, mx, mrows, 14, 14, 1, 0, true, e->deconv_out, nullptr, 0, s, e->total_rows, 196, 1)) < 0) return st;
    }
    }   // phase 4
    if (PH(5)) {
    { ProfScope ps(e, s, 6);
    if ((st = mask_predict_launch(e->deconv_out, e->mask_pred_w, e->mask_pred_b, e->deconv.cout / 4, mrows * 784,
                                  e->total_rows, 784, e->mask_logits, e->mask_probs_compact, prec, s)) < 0) return st; }
    { ProfScope ps(e, s, 6);
    if ((st = mask_scatter_launch(e->mask_probs_compact, o_count, B, D, o_probs, s)) < 0) return st; }
    if (out->mask_bits) {
        { ProfScope ps(e, s, 6);
        if ((st = paste_masks_launch(o_probs, o_boxes, o_count, outsz, B, D, e->desc.mask_thresh, out->mask_region,
                                     reinterpret_cast<long long*>(out->mask_offset), out->mask_bits,
                                     out->mask_words_per_image, s)) < 0) return st; }
    }
    }   // phase 5
    // every phase asked for has run: its names exist now (the stem pre-phase publishes its two too: a stage test may stop after it)
    for (int k = 0; k <= TD_PHASE_STEM; ++k) if (PH(k)) publish(e, g, k);
    return TD_OK;
}

td_status set_forward_ctx(td_engine* e, const void* images, int input_format, const int32_t* hw_valid,
                          const int32_t* hw_out, int B, int Hp, int Wp, const td_detections* out) {
    TD_REQUIRE(e && images && hw_valid && hw_out && out, "td_engine_forward: null argument");
    TD_REQUIRE(e->loaded, "td_engine_forward: load weights first");
    TD_REQUIRE(input_format == TD_INPUT_F32_CHW || input_format == TD_INPUT_U8_HWC, "td_engine_forward: bad input format %d", input_format);
    TD_REQUIRE(B >= 1 && Hp % 32 == 0 && Wp % 32 == 0 && Hp >= 64 && Wp >= 64, "td_engine_forward: bad batch geometry B=%d %dx%d", B, Hp, Wp);
    if (B > e->rB || Hp > e->rHp || Wp > e->rWp) {
        td_set_error("td_engine_forward: B=%d %dx%d exceeds the reserved B=%d %dx%d", B, Hp, Wp, e->rB, e->rHp, e->rWp);
        return TD_ERR_CAPACITY;
    }
    td_engine::FwdCtx& c = e->ctx;
    c.valid_ctx = false;
    for (int i = 0; i < B; ++i) {
        c.valid.h[i] = hw_valid[2 * i];
        c.valid.w[i] = hw_valid[2 * i + 1];
        c.outsz.h[i] = hw_out[2 * i];
        c.outsz.w[i] = hw_out[2 * i + 1];
        TD_REQUIRE(c.valid.h[i] >= 1 && c.valid.h[i] <= Hp && c.valid.w[i] >= 1 && c.valid.w[i] <= Wp, "td_engine_forward: image %d valid size %dx%d outside %dx%d", i, c.valid.h[i], c.valid.w[i], Hp, Wp);
        TD_REQUIRE(c.outsz.h[i] >= 1 && c.outsz.w[i] >= 1, "td_engine_forward: image %d has an empty output size", i);
    }
    if (out->mask_bits)
        TD_REQUIRE(out->mask_region && out->mask_offset && out->mask_words_per_image > 0, "td_engine_forward: mask_bits needs mask_region, mask_offset and mask_words_per_image");
    c.images = images;
    c.input_format = input_format;
    c.B = B;
    c.Hp = Hp;
    c.Wp = Wp;
    c.out = *out;
    c.valid_ctx = true;
    return TD_OK;
}

}  // namespace

extern "C" {

td_status td_engine_forward(td_engine* e, const void* images, int input_format, const int32_t* hw_valid,
                            const int32_t* hw_out, int B, int Hp, int Wp, void* stream_v, td_detections* out) {
    td_status st = set_forward_ctx(e, images, input_format, hw_valid, hw_out, B, Hp, Wp, out);
    if (st < 0) return st;
    e->stem_done = false;
    return forward_impl(e, 0x3fu, static_cast<hipStream_t>(stream_v));
}

td_status td_engine_forward_phase(td_engine* e, int phase, const void* images, int input_format, const int32_t* hw_valid,
                                  const int32_t* hw_out, int B, int Hp, int Wp, void* stream_v, td_detections* out) {
    TD_REQUIRE(e && phase >= 0 && phase <= TD_PHASE_STEM, "td_engine_forward_phase: bad phase %d", phase);
    hipStream_t s = static_cast<hipStream_t>(stream_v);
    td_status st;
    if (phase == TD_PHASE_STEM) {
        // pre-phase of the NEXT batch: needs the engine's stem / pool buffers, which the previous batch's trunk read
        if ((st = set_forward_ctx(e, images, input_format, hw_valid, hw_out, B, Hp, Wp, out)) < 0) return st;
        // (the previous batch's LATER phases do not touch stem_out / pool_out: waiting for its phase 5 here put the
        // pre-phase behind the whole selection tail and stalled the next trunk 0.8 ms per fp16 step)
        if (e->phase_ev_recorded[0]) TD_HIP_CHECK(hipStreamWaitEvent(s, e->phase_ev[0], 0));
        e->stem_done = false;
    } else if (phase == 0) {
        if (e->stem_done) {
            TD_REQUIRE(e->ctx.valid_ctx && (!images || images == e->ctx.images),
                       "td_engine_forward_phase: phase 0 after the stem pre-phase must continue the same batch");
            TD_HIP_CHECK(hipStreamWaitEvent(s, e->phase_ev[TD_PHASE_STEM], 0));
        } else if ((st = set_forward_ctx(e, images, input_format, hw_valid, hw_out, B, Hp, Wp, out)) < 0) {
            return st;
        }
        // The engine's previous batch must have left the buffers the trunk writes. The FPN levels and RPN head maps are
        // read last by RoIAlign 14x14 in phase 3, but phase 4 (the mask-head 3x3 convs) goes through run_conv like any
        // other layer: in the fp32 engine its Winograd transforms use e->wino_v / e->wino_m, the workspace the next
        // trunk's Winograd layers write. So the trunk waits for the previous batch's phase 4 (which implies 0-3). Its
        // phase 5 (predictor, scatter, paste) only reads deconv_out / total_rows / the mask buffers, which the next
        // batch rewrites in phases 3 and 4: that dependency is kept in its own slot (prev5_ev) and taken by the next
        // batch's phase 3 — waiting for phase 5 HERE chained every trunk behind the previous-but-two batch's mask tail
        // (0.5-0.8 ms of idle main stream per fp16 step, rocprof trace of round 2). With the even phases on one
        // stream, as the Predictor and bench.py enqueue them, the phase-4 wait is already satisfied by stream order.
        for (int k = 4; k >= 0; --k)
            if (e->phase_ev_recorded[k]) {
                TD_HIP_CHECK(hipStreamWaitEvent(s, e->phase_ev[k], 0));
                break;
            }
        if (e->phase_ev_recorded[5]) {            // hand the previous batch's phase-5 event to the slot phase 3 waits on
            std::swap(e->phase_ev[5], e->prev5_ev);
            e->prev5_recorded = true;
        }
    } else {
        TD_REQUIRE(e->ctx.valid_ctx, "td_engine_forward_phase: phase %d before phase 0", phase);
        TD_REQUIRE(e->phase_ev_recorded[phase - 1], "td_engine_forward_phase: phase %d before phase %d", phase, phase - 1);
        TD_HIP_CHECK(hipStreamWaitEvent(s, e->phase_ev[phase - 1], 0));
        if (phase == 3 && e->prev5_recorded) {    // the previous batch's predictor / paste still read what phases 3-4 rewrite
            TD_HIP_CHECK(hipStreamWaitEvent(s, e->prev5_ev, 0));
            e->prev5_recorded = false;
        }
    }
    if ((st = forward_impl(e, 1u << phase, s)) < 0) return st;
    if (!e->phase_ev[phase]) TD_HIP_CHECK(hipEventCreateWithFlags(&e->phase_ev[phase], hipEventDisableTiming));
    TD_HIP_CHECK(hipEventRecord(e->phase_ev[phase], s));
    e->phase_ev_recorded[phase] = true;
    if (phase == TD_PHASE_STEM) e->stem_done = true;
    if (phase == 0) {
        e->stem_done = false;
        for (int k = 1; k < 6; ++k) e->phase_ev_recorded[k] = false;
    }
    return TD_OK;
}

td_status td_engine_tensor(td_engine* e, const char* name, void** dev_ptr, int64_t dims[4], int* elem_size) {
    TD_REQUIRE(e && name && dev_ptr && dims, "td_engine_tensor: null argument");
    auto it = e->named.find(name);
    if (it == e->named.end()) {
        td_set_error("td_engine_tensor: no tensor named '%s' (run forward first)", name);
        return TD_ERR_INVALID;
    }
    *dev_ptr = it->second.p;
    for (int i = 0; i < 4; ++i) dims[i] = it->second.dims.d[i];
    if (elem_size) *elem_size = it->second.elem;
    return TD_OK;
}

td_status td_engine_profile_enable(td_engine* e, int enable) {
    TD_REQUIRE(e, "td_engine_profile_enable: null engine");
    e->prof = enable != 0;
    e->prof_detail = enable == 2;
    return TD_OK;
}

td_status td_engine_profile_classes(td_engine* e, double* ms, int64_t* launches, double* exec_flops, double* bytes, double* tmin_ms, int reset) {
    TD_REQUIRE(e, "td_engine_profile_classes: null engine");
    if (td_status st = drain_recs(e, e->cls_recs, e->cls_ms); st < 0) return st;
    for (int c = 0; c < TD_PROF_CLASSES; ++c) {
        if (ms) ms[c] = e->cls_ms[c];
        if (launches) launches[c] = e->cls_launches[c];
        if (exec_flops) exec_flops[c] = e->cls_flops[c];
        if (bytes) bytes[c] = e->cls_bytes[c];
        if (tmin_ms) tmin_ms[c] = e->cls_tmin_ms[c];
        if (reset) {
            e->cls_ms[c] = 0.0;
            e->cls_launches[c] = 0;
            e->cls_flops[c] = e->cls_bytes[c] = e->cls_tmin_ms[c] = 0.0;
        }
    }
    return TD_OK;
}

td_status td_engine_profile_read(td_engine* e, double* ms, int64_t* launches, double* flops, double* bytes, int reset) {
    TD_REQUIRE(e, "td_engine_profile_read: null engine");
    if (td_status st = drain_recs(e, e->prof_recs, e->prof_ms); st < 0) return st;
    for (int c = 0; c < TD_PROF_CATEGORIES; ++c) {
        if (ms) ms[c] = e->prof_ms[c];
        if (launches) launches[c] = e->prof_launches[c];
        if (flops) flops[c] = e->prof_flops[c];
        if (bytes) bytes[c] = e->prof_bytes[c];
        if (reset) {
            e->prof_ms[c] = 0.0;
            e->prof_launches[c] = 0;
            e->prof_flops[c] = 0.0;
            e->prof_bytes[c] = 0.0;
        }
    }
    return TD_OK;
}

td_status td_engine_read_tensor(td_engine* e, const char* name, void* dst_dev, int64_t bytes, void* stream) {
    TD_REQUIRE(e && name && dst_dev, "td_engine_read_tensor: null argument");
    auto it = e->named.find(name);
    if (it == e->named.end()) {
        td_set_error("td_engine_read_tensor: no tensor named '%s' (run forward first)", name);
        return TD_ERR_INVALID;
    }
    int64_t n = it->second.elem;
    for (int i = 0; i < 4; ++i)
        if (it->second.dims.d[i] > 0) n *= it->second.dims.d[i];
    TD_REQUIRE(bytes == n, "td_engine_read_tensor: '%s' is %lld bytes, caller passed %lld", name, (long long)n, (long long)bytes);
    TD_HIP_CHECK(hipMemcpyAsync(dst_dev, it->second.p, (size_t)n, hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream)));
    return TD_OK;
}

}  // extern "C"
