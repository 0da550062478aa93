"""Mutation controls for tests/roi_ref.py (CPU only): RoIAlign outputs computed deliberately wrong — in the ways a subtly
broken RoIAlign kernel goes wrong — must be rejected by the same checker the GPU tests use, and the oracle's own output
must pass. Also pins the checker's vectorised float32 reference to oracle/ops_ref.py roi_align bit for bit."""
import numpy as np
import pytest
import torch

from oracle import ops_ref as R
from tests import roi_ref as rr

H, W, C, POOLED = 13, 11, 8, 3


def _case(fp16=False, poison=False, seed=0):
    rng = np.random.default_rng(seed)
    feat = rng.standard_normal((H, W, C), dtype=np.float32)
    if fp16:
        feat = feat.astype(np.float16).astype(np.float32)
    if poison:
        feat[0, 0, 0::3] = np.nan
        feat[0, 0, 1::3] = np.inf
        feat[0, 0, 2::3] = -np.inf
    rois = np.concatenate([rr.edge_rois(H, W, POOLED), rr.random_rois(rng, 8, H, W, 1.0, 8.0)])
    return feat, rois


def _oracle(feat, rois, pooled=POOLED, scale=1.0):
    """ops_ref.roi_align in the kernel's layout [R * pooled^2, C]."""
    o = R.roi_align(feat.transpose(2, 0, 1), rois, scale, pooled)
    return np.ascontiguousarray(o.transpose(0, 2, 3, 1)).reshape(-1, feat.shape[2])


@pytest.mark.parametrize("fp16,poison,pooled,scale", [(False, False, 3, 1.0), (True, False, 3, 1.0), (False, True, 3, 1.0),
                                                      (True, True, 2, 1.0), (False, False, 7, 0.25), (False, False, 1, 1.0)])
def test_vectorised_float32_reference_is_the_oracle_bit_for_bit(fp16, poison, pooled, scale):
    feat, rois = _case(fp16, poison, seed=pooled)
    t = rr.taps(rois, H, W, scale, pooled)
    got = rr.ref32(t, rr.hwc_gather(feat), C)
    want = _oracle(feat, rois, pooled, scale)
    assert rr._same_bits(got, want).all()
    assert np.array_equal(np.isnan(got), np.isnan(want))
    if poison:
        assert np.isnan(want).any() and np.isfinite(want).any()


def _emit(ref, fp16, mutant=None, values=None):
    """A guarded CPU output holding `values` (default: the oracle's), with one write defect."""
    r32 = ref.r32 if values is None else values
    out = rr.new_output(r32.shape[0], r32.shape[1], fp16, "cpu")
    if fp16:
        v = r32.astype(np.float16)
        if mutant == "fp16_truncated":                       # round toward zero instead of to nearest
            v = _truncate_to_fp16(r32)
    else:
        v = r32
    t = torch.from_numpy(np.ascontiguousarray(v))
    if mutant == "bin_unwritten":
        out.t[:4] = t[:4]
        out.t[5:] = t[5:]
    else:
        out.t.copy_(t)
    if mutant == "write_past_end":
        out.buf[out.g + out.n] = out.t.reshape(-1)[-1]
    return out


def _truncate_to_fp16(x):
    """float32 → fp16 rounding toward zero: the nearest fp16, stepped one ulp back toward 0 where it rounded away."""
    y = x.astype(np.float16)
    away = np.abs(y.astype(np.float32)) > np.abs(x)
    return np.where(away, np.nextafter(y, np.float16(0)), y)


def _mutated_values(feat, rois, mutant):
    t = rr.taps(rois, H, W, 1.0, POOLED)
    g = rr.hwc_gather(feat)
    if mutant == "corner_weights_swapped":                   # w1 and w2 of every sample exchanged
        t.w = t.w[:, [1, 0, 2, 3]].copy()
    elif mutant == "sample_dropped":                         # one sample of one bin never accumulated
        k = len(t.bin) // 2
        keep = np.ones(len(t.bin), bool)
        keep[k] = False
        for f in ("bin", "slot", "yl", "yh", "xl", "xh", "w"):
            setattr(t, f, getattr(t, f)[keep])
    elif mutant == "divisor_off_by_one":
        t.count = t.count + 1
    v = rr.ref32(t, g, C)
    if mutant == "neighbour_bin":                            # the half-wave pairing error: bin b takes bin b + 1's value
        b = int(np.flatnonzero((v[:-1] != v[1:]).any(axis=1))[0])
        v = v.copy()
        v[b] = v[b + 1]
    return v


MUTANTS = ["corner_weights_swapped", "sample_dropped", "divisor_off_by_one", "neighbour_bin", "bin_unwritten", "write_past_end",
           "fp16_truncated"]


@pytest.mark.parametrize("mutant", MUTANTS)
def test_checker_rejects_mutant(mutant):
    fp16 = mutant == "fp16_truncated"
    feat, rois = _case(fp16)
    ref = rr.reference(rr.taps(rois, H, W, 1.0, POOLED), rr.hwc_gather(feat), C)
    values = None
    if mutant in ("corner_weights_swapped", "sample_dropped", "divisor_off_by_one", "neighbour_bin"):
        values = _mutated_values(feat, rois, mutant)
    v = rr.check(_emit(ref, fp16, mutant, values), ref)
    assert v.failures, mutant
    want = {"bin_unwritten": "(c)", "write_past_end": "(c)"}.get(mutant, "(a)")
    assert any(f.startswith(want) for f in v.failures), v.failures


def test_fp16_truncation_mutant_really_truncates():
    x = np.array([1.0 + 3 * 2.0 ** -12, -(1.0 + 3 * 2.0 ** -12), 0.1, 2.0 ** -30, 1.0], np.float32)
    t = _truncate_to_fp16(x).astype(np.float32)
    assert (np.abs(t) <= np.abs(x)).all()
    assert list(t != x.astype(np.float16).astype(np.float32)) == [True, True, False, False, False]


def test_bound_rejects_an_error_of_a_few_ulp_on_large_sums():
    feat, rois = _case()
    ref = rr.reference(rr.taps(rois, H, W, 1.0, POOLED), rr.hwc_gather(feat), C)
    v = ref.r32.copy()
    k = np.unravel_index(np.argmax(np.abs(ref.r64) / np.maximum(ref.mag * ref.ghw[:, None], 1e-30)), v.shape)
    v[k] = np.float32(ref.r64[k] + (4 * ref.ghw[k[0]] + 3) * 2.0 ** -24 * ref.mag[k] * 4)
    out = _emit(ref, False, values=v)
    assert any(f.startswith("(b)") for f in rr.check(out, ref).failures)


@pytest.mark.parametrize("fp16,poison", [(False, False), (True, False), (False, True), (True, True)])
def test_checker_accepts_the_oracle(fp16, poison):
    feat, rois = _case(fp16, poison)
    ref = rr.reference(rr.taps(rois, H, W, 1.0, POOLED), rr.hwc_gather(feat), C)
    want = _oracle(feat, rois)
    v = rr.check(_emit(ref, fp16, values=want), ref)
    assert not v.failures, v.failures
    assert v.exact == 1.0 and v.worst <= 1.0
    if not poison:
        assert v.worst > 0.0           # (the bound is exercised, not vacuous)


def test_edge_rois_put_samples_exactly_on_the_map_edges():
    t = rr.taps(rr.edge_rois(H, W, POOLED), H, W, 1.0, POOLED)
    assert t.samples > 0
    # samples at exactly -1 and exactly H / W are kept (clamped to the border pixel with weight 1 on it)
    assert ((t.yl == 0) & (t.yh == 1) & (t.w[:, 0] + t.w[:, 1] == 1)).any()
    assert ((t.yl == H - 1) & (t.yh == H - 1)).any() and ((t.xl == W - 1) & (t.xh == W - 1)).any()
