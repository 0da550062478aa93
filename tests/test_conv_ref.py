"""Mutation controls for tests/conv_ref.py (CPU only): outputs computed deliberately wrong — in the ways a subtly broken
conv tile goes wrong — must be rejected by the same checker the GPU sweep uses, and the exactly rounded result must pass."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import conv_ref as cr

SHAPES = {
    # (layer, fp16, batch): M = 312 / 300 / 288 rows, so each has a ragged last 256-row tile
    "fp32_3x3": (cr.Conv("m32", 64, 64, 3, 1, 1, 12, 13), False, 2),
    "fp16_3x3_k2304": (cr.Conv("m16", 256, 64, 3, 1, 1, 10, 10), True, 3),
    "fp32_1x1_up2": (cr.Conv("lat32", 64, 64, 1, 1, 0, 12, 12, scale=False, res=2, relu=False), False, 2),
    "fp16_1x1_up2": (cr.Conv("lat16", 128, 128, 1, 1, 0, 12, 12, scale=False, res=2, relu=False), True, 2),
}


def _nchw(t):
    return t.permute(0, 3, 1, 2).double()


def emulate(L, inp, mutant=None):
    """The convolution on the CPU in float64, rounded once to the output dtype, with one deliberate defect."""
    x, w = _nchw(inp["x"].t), _nchw(inp["w"])
    ke = 64 if inp["fp16"] else 32
    if mutant == "dropped_k_chunk":                 # one k-chunk (ke input channels of one tap) never accumulated
        w = w.clone()
        w[:, ke:2 * ke, L.k // 2, L.k // 2] = 0
    if mutant == "padding_shifted":                 # the padded window one pixel off to the left
        y = F.conv2d(F.pad(x, (L.pad + 1, L.pad - 1, L.pad, L.pad)), w, stride=L.stride)
    elif mutant == "fp16_accumulation":             # the accumulator held in fp16 between 16-product MFMA steps
        P = cr._patches(L, inp["x"].t, torch.arange(inp["B"] * L.Ho * L.Wo)).double()
        Wm = inp["w"].reshape(L.Cout, -1).double()
        acc = torch.zeros(P.shape[0], L.Cout, dtype=torch.float64)
        for c in range(0, L.K, 16):
            acc = (acc + P[:, c:c + 16] @ Wm[:, c:c + 16].T).half().double()
        y = acc.reshape(inp["B"], L.Ho, L.Wo, L.Cout).permute(0, 3, 1, 2)
    else:
        y = F.conv2d(x, w, stride=L.stride, padding=L.pad)
    sc = inp["scale"].double()[None, :, None, None] if inp["scale"] is not None else 1.0
    bi = inp["bias"].double()[None, :, None, None] if inp["bias"] is not None else 0.0
    y = (y + bi) * sc if mutant == "bias_before_scale" else y * sc + bi
    if inp["res"] is not None:
        r = _nchw(inp["res"].t)
        if L.res == 2:
            r = F.interpolate(r, scale_factor=2.0, mode="nearest")
            if mutant == "residual_row_off_by_one":     # row oh reads source row (oh + 1) >> 1
                r = torch.cat([r[:, :, 1:], r[:, :, -1:]], dim=2)
        y = y + r
    if L.relu:
        y = y.clamp_min(0)
    out = cr.new_output(L, inp)
    vals = y.permute(0, 2, 3, 1).to(out.t.dtype)
    if mutant == "last_tile_unwritten":
        M = out.t.numel() // L.Cout
        keep = (M - 1) // cr.BLOCK_ROWS * cr.BLOCK_ROWS
        out.t.reshape(-1, L.Cout)[:keep] = vals.reshape(-1, L.Cout)[:keep]
    else:
        out.t.copy_(vals)
    if mutant == "write_past_end":                  # one row written past the end of y
        out.buf[out.g + out.n:out.g + out.n + L.Cout] = 0.5
    return out


MUTANTS = ["dropped_k_chunk", "padding_shifted", "last_tile_unwritten", "fp16_accumulation", "residual_row_off_by_one",
           "bias_before_scale", "write_past_end"]


def _setup(key):
    L, fp16, B = SHAPES[key]
    inp = cr.make_inputs(L, fp16, B, "cpu", seed=11)
    ref = cr.reference(L, inp, cr.sample_rows(L, B, seed=5))
    return L, inp, ref


@pytest.mark.parametrize("key", list(SHAPES))
def test_exact_result_passes(key):
    L, inp, ref = _setup(key)
    v = cr.check(L, emulate(L, inp), ref)
    print(f"\n[exact {key}] err/bound {v.err_over_bound:.3g}, RMS {v.rms:.3g}")
    assert v.ok, v.why


@pytest.mark.parametrize("key,mutant", [(k, m) for k in SHAPES for m in MUTANTS
                                         if not (m == "residual_row_off_by_one" and SHAPES[k][0].res != 2)
                                         and not (m == "fp16_accumulation" and not SHAPES[k][1])
                                         and not (m == "padding_shifted" and SHAPES[k][0].pad == 0)
                                         and not (m == "bias_before_scale" and not SHAPES[k][0].scale)])
def test_mutant_is_rejected(key, mutant):
    L, inp, ref = _setup(key)
    v = cr.check(L, emulate(L, inp, mutant), ref)
    print(f"\n[mutant {mutant} on {key}] rejected (RMS {v.rms:.3g}): {v.why}")
    assert not v.ok, f"{mutant} passed the checker (err/bound {v.err_over_bound:.3g}, RMS {v.rms:.3g})"


def test_sample_covers_corners_block_edges_and_the_ragged_tile():
    L = cr.Conv("s", 64, 64, 3, 1, 1, 50, 37)
    B = 3
    rows = set(cr.sample_rows(L, B, seed=1).tolist())
    HW, M = L.Ho * L.Wo, B * L.Ho * L.Wo
    for b in range(B):
        assert {b * HW, b * HW + L.Wo - 1, b * HW + HW - L.Wo, b * HW + HW - 1} <= rows
    assert set(range((M - 1) // 256 * 256, M)) <= rows
    assert {0, 255, 256, 511} <= rows
    assert len(rows) >= 2048


def test_tile_predicates_match_the_library_rules():
    """Spot checks of the mirrored conv2d_launch / tuned_cfg rules on the shapes the vacuous tests used to hit."""
    c3 = cr.Conv("c3", 256, 256, 3, 1, 1, 50, 50)
    s2 = cr.Conv("s2", 256, 128, 1, 2, 0, 40, 40)
    k3 = cr.Conv("k3", 192, 300, 1, 1, 0, 23, 19)
    up = cr.Conv("up", 512, 256, 1, 1, 0, 16, 16, res=2)
    assert not cr.tile_runs(33, c3, True, 1) and not cr.tile_runs(33, s2, True, 1) and not cr.tile_runs(33, k3, True, 2)
    assert cr.tile_runs(33, cr.Conv("t", 128, 256, 1, 1, 0, 20, 20), True, 1)
    assert not cr.tile_runs(17, c3, False, 1) and cr.tile_runs(17, c3, True, 1)
    assert not cr.tile_runs(18, up, False, 1) and not cr.tile_runs(19, c3, False, 1) and not cr.tile_runs(20, k3, True, 1)
    assert cr.tile_runs(20, k3, False, 1)
    for c in (21, 22, 28):
        assert not cr.tile_runs(c, c3, True, 1)
    assert 33 not in cr.tuner_ids(c3, True, 1) and 17 in cr.tuner_ids(c3, True, 1) and 15 not in cr.tuner_ids(c3, True, 1)
    assert set(cr.tuner_ids(cr.Conv("h", 256, 15, 1, 1, 0, 60, 60, out_f32=True), True, 1)) >= {31, 32, 15, 16}


def test_fp16_accumulation_is_caught_by_the_rms_criterion_alone():
    """At K = 2304 the per-element bound is loose by ~sqrt(K); the RMS criterion is what separates a tile that keeps its
    accumulator in fp16 from one that accumulates in fp32 (exact: R ~ 0.43, the fp16 output rounding)."""
    L, inp, ref = _setup("fp16_3x3_k2304")
    exact, bad = cr.check(L, emulate(L, inp), ref), cr.check(L, emulate(L, inp, "fp16_accumulation"), ref)
    assert exact.rms <= cr.RMS_MAX[torch.float16] / 3
    assert bad.rms > 1.4 * cr.RMS_MAX[torch.float16], bad.rms


# ---- launches with a device row count and the pixel-shuffle store (td_conv2d_rows_nhwc; the mask head's phase 4) ----
ROWS_SHAPES = {
    # (layer, fp16): B = 4 reserved RoIs of 14 x 14, 3 live: 588 live rows end inside the 256-row block 512..767
    "fp32_conv": (cr.Conv("mc32", 64, 64, 3, 1, 1, 14, 14, scale=False), False),
    "fp16_conv": (cr.Conv("mc16", 64, 64, 3, 1, 1, 14, 14, scale=False), True),
    "fp32_deconv": (cr.Conv("md32", 64, 128, 1, 1, 0, 14, 14, scale=False, out_mode=1), False),
    "fp16_deconv": (cr.Conv("md16", 64, 128, 1, 1, 0, 14, 14, out_mode=1), True),
}
ROWS_B, ROWS_COUNT = 4, 3
ROWS_MUTANTS = ["shuffle_dy_dx_swapped", "bias_at_n", "last_live_roi_unwritten", "row_past_count", "halo_from_next_roi"]


def emulate_rows(L, inp, count, mutant=None):
    """The first `count` RoIs in float64, rounded once, stored as the launch stores them; everything else keeps the sentinel."""
    HW, Cq = L.Ho * L.Wo, L.Cy
    x, w = _nchw(inp["x"].t[:count]), _nchw(inp["w"])
    y = F.conv2d(x, w, padding=L.pad)                                           # [count, Cout, Ho, Wo]
    if mutant == "halo_from_next_roi":          # one pixel of RoI 0's last row: the taps below it read RoI 1's first row, not padding
        ow = 5
        patch = torch.zeros(x.shape[1], 3, 3, dtype=torch.float64)
        patch[:, :2] = x[0, :, L.H - 2:, ow - 1:ow + 2]
        patch[:, 2] = x[1, :, 0, ow - 1:ow + 2]
        y[0, :, L.Ho - 1, ow] = (w * patch[None]).sum((1, 2, 3))
    sc = inp["scale"].double() if inp["scale"] is not None else torch.ones(Cq, dtype=torch.float64)
    bi = inp["bias"].double() if inp["bias"] is not None else torch.zeros(Cq, dtype=torch.float64)
    if L.out_mode == 1:
        sc = sc.repeat(4)
        bi = torch.cat([bi, torch.zeros(3 * Cq, dtype=torch.float64)]) if mutant == "bias_at_n" else bi.repeat(4)
    y = (y * sc[None, :, None, None] + bi[None, :, None, None]).clamp_min(0).permute(0, 2, 3, 1)     # [count, Ho, Wo, Cout]
    out = cr.new_output(L, inp)
    if L.out_mode == 1:
        y = y.reshape(count, L.Ho, L.Wo, 2, 2, Cq)                              # [.., dy, dx, co]
        if mutant == "shuffle_dy_dx_swapped":
            y = y.transpose(3, 4)
        y = y.permute(0, 1, 3, 2, 4, 5).reshape(count, 2 * L.Ho, 2 * L.Wo, Cq)
    n = count - 1 if mutant == "last_live_roi_unwritten" else count
    out.t[:n] = y[:n].to(out.t.dtype)
    if mutant == "row_past_count":              # conv row count * HW (the first dead one, inside the last live 256-row block)
        assert (count * HW) % cr.BLOCK_ROWS != 0
        px = cr.stored_rows(L, torch.tensor([count * HW])).reshape(-1)[0]
        out.t.reshape(-1, Cq)[px] = 0.5
    return out


def _rows_setup(key):
    L, fp16 = ROWS_SHAPES[key]
    inp = cr.make_inputs(L, fp16, ROWS_B, "cpu", seed=17)
    ref = cr.reference(L, inp, torch.arange(ROWS_B * L.Ho * L.Wo))            # every row of every reserved RoI, once
    qi, qv = cr.QNAN[inp["x"].t.dtype]
    inp["x"].t[ROWS_COUNT:].view(qi).fill_(qv)                                 # dead RoIs: quiet NaN
    return L, inp, ref


@pytest.mark.parametrize("key", list(ROWS_SHAPES))
def test_exact_live_rows_pass_and_the_reference_shuffles(key):
    L, inp, ref = _rows_setup(key)
    live = ROWS_COUNT * L.Ho * L.Wo
    v = cr.check(L, emulate_rows(L, inp, ROWS_COUNT), ref, live_rows=live)
    print(f"\n[exact rows {key}] err/bound {v.err_over_bound:.3g}, RMS {v.rms:.3g}")
    assert v.ok, v.why
    assert cr.check(L, cr.new_output(L, inp), ref, live_rows=0).ok               # count 0: an untouched y is right
    assert not cr.check(L, emulate_rows(L, inp, ROWS_COUNT), ref, live_rows=live - 1).ok     # and the count is exact
    assert not cr.check(L, emulate_rows(L, inp, ROWS_COUNT), ref).ok             # a static launch leaves no sentinel
    if L.out_mode == 1:                                                        # the stated layout, element by element
        px = cr.stored_rows(L, torch.tensor([L.Wo + 2]))                        # RoI 0, h = 1, w = 2
        assert px.tolist() == [[2 * 28 + 4, 2 * 28 + 5, 3 * 28 + 4, 3 * 28 + 5]]
        assert torch.equal(cr.conv_row_of_pixel(L, px.reshape(-1)), torch.full((4,), L.Wo + 2))


@pytest.mark.parametrize("key,mutant", [(k, m) for k in ROWS_SHAPES for m in ROWS_MUTANTS
                                         if not (m in ("shuffle_dy_dx_swapped", "bias_at_n") and ROWS_SHAPES[k][0].out_mode == 0)
                                         and not (m == "halo_from_next_roi" and ROWS_SHAPES[k][0].k == 1)])
def test_rows_mutant_is_rejected(key, mutant):
    L, inp, ref = _rows_setup(key)
    v = cr.check(L, emulate_rows(L, inp, ROWS_COUNT, mutant), ref, live_rows=ROWS_COUNT * L.Ho * L.Wo)
    print(f"\n[rows mutant {mutant} on {key}] rejected: {v.why}")
    assert not v.ok, f"{mutant} passed the checker (err/bound {v.err_over_bound:.3g}, RMS {v.rms:.3g})"


def test_rows_predicates_match_the_library_rules():
    """conv_tile_refusal on out_mode and a device count: PP8 and the filter-direct family refuse the shuffle, the
    filter-stationary tile refuses both, the plain igemm tiles take everything."""
    conv = cr.Conv("mask.conv", 256, 256, 3, 1, 1, 14, 14, scale=False)
    dec = cr.Conv("mask.deconv", 256, 1024, 1, 1, 0, 14, 14, scale=False, out_mode=1)
    one = cr.Conv("one", 128, 1024, 1, 1, 0, 14, 14, scale=False)
    for fp16 in (False, True):
        assert all(cr.tile_runs(c, dec, fp16, 8, dyn) == (c <= 16 or c in (31, 32)) for c in cr.SWEEP_IDS for dyn in (False, True))
        assert cr.tile_runs(33, one, fp16, 8) and not cr.tile_runs(33, one, fp16, 8, dyn=True)
        assert cr.tile_runs(23, conv, fp16, 8, dyn=True) and cr.tile_runs(17, conv, fp16, 8, dyn=True) == fp16
        assert not {17, 23, 24, 25, 26, 27, 29, 30, 33} & set(cr.tuner_ids(dec, fp16, 8, dyn=True))
        assert 33 in cr.tuner_ids(one, fp16, 8) and 33 not in cr.tuner_ids(one, fp16, 8, dyn=True)
        assert set(cr.tuner_ids(dec, fp16, 8, dyn=True)) <= {c for c in cr.SWEEP_IDS if cr.tile_runs(c, dec, fp16, 8, True)}
