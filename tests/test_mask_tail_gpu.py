"""The mask tail (roi.hip: mask_predict_kernel, mask_scatter_kernel, paste_plan_kernel, paste_fill_kernel) on a crafted
``mask_deconv``, in the fp32 and the fp16 engine. The detections come from the crafted selections of tests/det_cases.py
(disjoint boxes, one score, counts [7, 0, 100] and [0, 3, 0]: the image without detections sits between two live ones, and
the live one between two empty ones); tests/det_stage.py overwrites ``mask_deconv`` between phases 4 and 5 and poisons
every buffer the tail writes. The predictor of the synthetic network gets bias 0.375 and weight -0.75 on channel 5, so a
pixel whose only non-zero input is 0.5 on that channel has a logit of exactly 0.

  * mask_logits: the float64 dot of the stored ``mask_deconv`` row (float32 or float16, as read back) with the float32
    predictor weights, plus the bias, within (C / 64 + 6 + 2) * 2^-24 * sum|x_i w_i| + 1 ulp of the result: C / 64 fused
    multiply-adds per lane, a 6-level pairwise reduction over the 64 lanes, the bias add and the final rounding. Detection
    rows cycle through: random values; channels and whole pixels that are zero (logit = bias exactly); two huge channels
    that cancel; constant logit exactly 0; large logits of both signs. Rows >= total_rows * 784 keep
    their NaN poison although their inputs are finite (zeros: a kernel without the row limit would write the bias there);
  * mask_probs_compact: within (2 * EXPF_ULP + 2) * 2^-24 relative of the float64 sigmoid of the engine's own logit
    (expf within EXPF_ULP = 1 ulp = 2 * 2^-24 relative — the HIP math API's documented bound, assumed as in
    tests/det_cases.py —, one add, one divide), plus 2^-149; a logit of exactly 0 gives exactly 0.5;
  * out["mask_probs"][b, d] bit-equal to compact row prefix(b) + d for d < count[b], exactly 0 beyond;
  * region / offset / bits: region equal to R.paste_region per detection and zero beyond the count, offsets consecutive
    and non-overlapping, ``unpack_masks`` bit-equal to R.paste_masks on the engine's own probabilities and boxes (a
    constant-0.5 mask tests >= at the threshold; boxes on all four borders, a box under one pixel, a region 144 px wide),
    unused high bits of a row's last word 0, words beyond the last region untouched (poison survives).
"""
import numpy as np
import pytest
import torch

from oracle import ops_ref as R
from tests import det_cases as dc
from tests.det_stage import make_engine, run_stage
from treedetection_amd.engine import unpack_masks
from treedetection_amd.weights import make_synthetic_state_dict

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
BIAS, C0, W0 = 0.375, 5, -0.75
PX = 784


def state_dict(precision):
    """The half-width synthetic network for the fp32 engine; the fp16 engine needs the full width (its k-chunks are 64
    channels). Predictor bias and one weight replaced as the module docstring says."""
    sd = dict(make_synthetic_state_dict(50, seed=3, width_div=2 if precision == "fp32" else 1))
    w = np.array(sd["roi_heads.mask_head.predictor.weight"], dtype=np.float32, copy=True)
    w[0, C0, 0, 0] = W0
    sd["roi_heads.mask_head.predictor.weight"] = w
    sd["roi_heads.mask_head.predictor.bias"] = np.array([BIAS], np.float32)
    return sd


@pytest.fixture(scope="module")
def engines():
    """precision -> (engine, predictor weights [C]); built on first use, closed at teardown."""
    made = {}

    def get(precision):
        if precision not in made:
            sd = state_dict(precision)
            made[precision] = (make_engine("default", precision, sd),
                               sd["roi_heads.mask_head.predictor.weight"].reshape(-1).astype(np.float32))
        return made[precision]
    yield get
    for e, _ in made.values():
        e.close()


def pattern(r):
    """Input pattern of compact detection row r: row 0 (the whole-image box where there is one) is the constant-0.5 mask."""
    return (r + 3) % 5


def crafted_deconv(w):
    """deconv_fn of run_stage: detection row r takes pattern(r); rows beyond total_rows are zero (finite)."""
    def fn(total, shape, dtype):
        rows, _, _, C = shape
        assert shape[1:3] == (28, 28) and C == w.size and total <= rows
        rng = np.random.default_rng(77)
        unit = 1.0 / float(np.linalg.norm(w))                  # input scale at which the logit has unit deviation
        x = np.zeros((rows, PX, C), dtype=np.float32)          # dead rows: zeros, so a kernel that computed them would write
                                                               # the bias and its sigmoid over the NaN poison of its outputs
        aw = np.abs(w)
        aw[C0] = 0.0
        c1, c2 = int(np.argmax(aw[:64])), 64 + int(np.argmax(aw[64:128]))  # heavy channels 64 apart: two lanes of the wave
        for r in range(total):
            k = pattern(r)
            if k == 0:
                v = rng.normal(0.0, 2.0 * unit, (PX, C))
            elif k == 1:                                       # half the channels zero, every third pixel zero altogether
                v = rng.normal(0.0, 2.0 * unit, (PX, C))
                v[:, rng.random(C) < 0.5] = 0.0
                v[::3] = 0.0
            elif k == 2:                                       # two huge products of opposite sign that all but cancel
                v = rng.normal(0.0, 0.05, (PX, C))
                v[:, c1] = 1000.0
                v[:, c2] = np.clip(-1000.0 * w[c1] / w[c2], -60000.0, 60000.0)
            elif k == 3:                                       # 0.5 * -0.75 + 0.375 = 0 exactly: a constant-0.5 mask
                v = np.zeros((PX, C))
                v[:, C0] = 0.5
            else:                                              # logits of deviation 12: saturated both ways, |logit| stays below
                v = rng.normal(0.0, 12.0 * unit, (PX, C))      # 88, where expf(-logit) would leave the float32 range
            x[r] = v
        return torch.from_numpy(x.reshape(shape)).to(dtype)
    return fn


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
@pytest.mark.parametrize("name", dc.MASK_CASE_NAMES)
def test_mask_tail_on_crafted_deconv(name, precision, engines):
    eng, w = engines(precision)
    case = dc.make_case(name)
    got = run_stage(eng, case, crafted_deconv(w))
    D = dc.D
    counts = got["count"].astype(np.int64)
    assert counts.tolist() == [e["count"] for e in case["expect"]], (name, counts)
    total = int(counts.sum())
    C = w.size
    assert got["deconv"].dtype == (np.float32 if precision == "fp32" else np.float16)
    x = got["deconv"].reshape(3 * D, PX, C)[:total].astype(np.float64)
    # ---- logits
    prod = x * w.astype(np.float64)[None, None, :]
    ref = prod.sum(axis=2) + BIAS
    bound = (C / 64 + 6 + 2) * U * np.abs(prod).sum(axis=2) + np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    logits = got["mask_logits"].reshape(3 * D, PX)
    err = np.abs(logits[:total].astype(np.float64) - ref)
    print(f"{name} {precision}: {total} rows; logit error / bound max {float((err / bound).max()):.3f}")
    assert (err <= bound).all(), (name, precision, np.argwhere(err > bound)[:5])
    assert np.isnan(logits[total:]).all() and np.isnan(got["mask_probs_compact"].reshape(3 * D, PX)[total:]).all()   # untouched
    zero_rows = [r for r in range(total) if pattern(r) == 3]
    assert zero_rows and (logits[zero_rows] == 0).all(), (name, precision)           # the true logit is exactly 0, and so is the engine's
    dead = [r for r in range(total) if pattern(r) == 1]
    assert (logits[dead][:, ::3] == np.float32(BIAS)).all()                          # all-zero pixels: the bias alone
    # ---- probabilities: sigmoid of the engine's own logit
    probs = got["mask_probs_compact"].reshape(3 * D, PX)[:total]
    p64 = 1.0 / (1.0 + np.exp(-logits[:total].astype(np.float64)))
    tol = (2 * dc.EXPF_ULP + 2) * U * p64 + 2.0 ** -149
    perr = np.abs(probs.astype(np.float64) - p64)
    print(f"{name} {precision}: probability error / bound max {float((perr / tol).max()):.3f}")
    assert (perr <= tol).all()
    assert (probs[zero_rows] == np.float32(0.5)).all()
    # ---- scatter
    prefix = np.concatenate([[0], np.cumsum(counts)])
    mp = got["mask_probs"].reshape(3, D, PX)
    for b in range(3):
        c = int(counts[b])
        assert np.array_equal(mp[b, :c].view(np.uint32), probs[prefix[b]: prefix[b] + c].view(np.uint32)), (name, b, "scatter")
        assert (mp[b, c:].view(np.uint32) == 0).all(), (name, b, "beyond the count")
    # ---- paste
    thr = 0.5
    for b in range(3):
        c = int(counts[b])
        oh, ow = case["hw_out"][b]
        region, offset = got["mask_region"][b], got["mask_offset"][b]
        words = got["mask_bits"][b].view(np.uint32)
        assert (region[c:] == 0).all() and (offset[c:] == 0).all(), (name, b)
        boxes = got["boxes"][b, :c]
        off = 0
        for d in range(c):
            x0, y0, x1, y1 = R.paste_region(boxes[d], oh, ow)
            assert region[d].tolist() == [x0, y0, x1, y1] and x1 > x0 and y1 > y0, (name, b, d, region[d])
            assert int(offset[d]) == off, (name, b, d)                                 # consecutive, non-overlapping
            wpr = (x1 - x0 + 31) // 32
            rows = words[off: off + wpr * (y1 - y0)].reshape(y1 - y0, wpr)
            spare = wpr * 32 - (x1 - x0)
            if spare:
                assert (rows[:, -1] >> np.uint32(32 - spare) == 0).all(), (name, b, d, "unused high bits")
            off += wpr * (y1 - y0)
        assert (words[off:] == 0xFFFFFFFF).all(), (name, b, "words beyond the last region")
        masks = unpack_masks(region, offset, got["mask_bits"][b], c, oh, ow)
        ref_masks = R.paste_masks(mp[b, :c].reshape(c, 28, 28), boxes, oh, ow, thr)
        assert np.array_equal(masks, ref_masks), (name, b, int((masks != ref_masks).sum()))
        for d in range(c):
            if pattern(prefix[b] + d) == 3:                                                # the constant-0.5 mask: >= keeps the interior
                vals, (x0, y0, x1, y1) = R.paste_mask_values(mp[b, d].reshape(28, 28), boxes[d], oh, ow)
                at_thr = vals == np.float32(0.5)
                print(f"{name} {precision} image {b} detection {d}: {int(at_thr.sum())} pixels exactly at the threshold")
                assert masks[d, y0:y1, x0:x1][at_thr].all()
    b0 = int(np.nonzero(counts)[0][0])                  # compact row 0: the whole-image box with the constant-0.5 mask
    vals, _ = R.paste_mask_values(mp[b0, 0].reshape(28, 28), got["boxes"][b0, 0], *case["hw_out"][b0])
    assert (vals == np.float32(0.5)).sum() > 100        # the >= is really exercised: many pasted values are exactly 0.5
