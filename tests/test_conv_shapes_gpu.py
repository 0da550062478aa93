"""Every conv tile the library can run, at the network's own layer shapes (SURVEY.md Appendix B, 800 x 800 input), against
a sampled float64 reference with guarded buffers (tests/conv_ref.py).

For each layer x (precision, batch) every tile id 0-33 except the retired 21 / 22 / 28 is forced in strict mode: the ids
the launch accepts must be exactly the ones conv2d_launch's rules allow, they must include every id the engine's tuner
would time for that shape, and every accepted run must pass the guards, the per-element fp64 bound and the RMS
criterion. Filter-direct / filter-stationary tiles (23-27, 29, 30, 33) and the fp16 ping-pong tile (17) keep tile 0's k
order and epilogue: their whole output must equal tile 0's bit for bit."""
import dataclasses
import math
import os
import time
import zlib

import pytest
import torch

from tests import conv_ref as cr

pytestmark = pytest.mark.gpu

C = cr.Conv
# (layer, images per network image: RoIs for the box / mask heads)
LAYERS = [
    (C("res2.conv1.first", 64, 64, 1, 1, 0, 200, 200), 1),
    (C("res2.conv1", 256, 64, 1, 1, 0, 200, 200), 1),
    (C("res2.conv2", 64, 64, 3, 1, 1, 200, 200), 1),
    (C("res2.conv3", 64, 256, 1, 1, 0, 200, 200, res=1), 1),
    (C("res2.shortcut", 64, 256, 1, 1, 0, 200, 200, relu=False), 1),
    (C("res3.conv1.s2", 256, 128, 1, 2, 0, 200, 200), 1),                   # STRIDE_IN_1X1
    (C("res3.conv1", 512, 128, 1, 1, 0, 100, 100), 1),
    (C("res3.conv2", 128, 128, 3, 1, 1, 100, 100), 1),
    (C("res3.conv3", 128, 512, 1, 1, 0, 100, 100, res=1), 1),
    (C("res3.shortcut.s2", 256, 512, 1, 2, 0, 200, 200, relu=False), 1),
    (C("res4.conv1.s2", 512, 256, 1, 2, 0, 100, 100), 1),
    (C("res4.conv1", 1024, 256, 1, 1, 0, 50, 50), 1),
    (C("res4.conv2", 256, 256, 3, 1, 1, 50, 50), 1),
    (C("res4.conv3", 256, 1024, 1, 1, 0, 50, 50, res=1), 1),
    (C("res4.shortcut.s2", 512, 1024, 1, 2, 0, 100, 100, relu=False), 1),
    (C("res5.conv1.s2", 1024, 512, 1, 2, 0, 50, 50), 1),
    (C("res5.conv1", 2048, 512, 1, 1, 0, 25, 25), 1),
    (C("res5.conv2", 512, 512, 3, 1, 1, 25, 25), 1),                         # K = 4608
    (C("res5.conv3", 512, 2048, 1, 1, 0, 25, 25, res=1), 1),
    (C("res5.shortcut.s2", 1024, 2048, 1, 2, 0, 50, 50, relu=False), 1),
    (C("fpn.lateral2", 256, 256, 1, 1, 0, 200, 200, scale=False, res=2, relu=False), 1),     # + nearest-2x of the level above
    (C("fpn.lateral3", 512, 256, 1, 1, 0, 100, 100, scale=False, res=2, relu=False), 1),
    (C("fpn.lateral4", 1024, 256, 1, 1, 0, 50, 50, scale=False, res=2, relu=False), 1),
    (C("fpn.lateral5", 2048, 256, 1, 1, 0, 25, 25, scale=False, relu=False), 1),
    (C("fpn.output2", 256, 256, 3, 1, 1, 200, 200, scale=False, relu=False), 1),
    (C("fpn.output4", 256, 256, 3, 1, 1, 50, 50, scale=False, relu=False), 1),
    (C("fpn.output5", 256, 256, 3, 1, 1, 25, 25, scale=False, relu=False), 1),
    (C("rpn.conv.p3", 256, 256, 3, 1, 1, 100, 100, scale=False), 1),
    (C("rpn.conv.p6", 256, 256, 3, 1, 1, 13, 13, scale=False), 1),
    (C("rpn.head.p3", 256, 15, 1, 1, 0, 100, 100, scale=False, relu=False, out_f32=True), 1),
    (C("box.fc1", 12544, 1024, 1, 1, 0, 1, 1, scale=False), 1000),          # 1x1 over the 7 x 7 x 256 RoI features
    (C("box.fc2", 1024, 1024, 1, 1, 0, 1, 1, scale=False), 1000),
    (C("box.predictor", 1024, 6, 1, 1, 0, 1, 1, scale=False, relu=False, out_f32=True), 1000),
    (C("mask.conv", 256, 256, 3, 1, 1, 14, 14, scale=False), 100),
    (C("res2.conv2.200x336", 64, 64, 3, 1, 1, 200, 336), 1),                # 800 x 1333 input: W not a multiple of a tile
]
CONFIGS = [(False, 1), (False, 8), (True, 8), (True, 32)]                   # (fp16, batch); fp16 batch 32 = configs[4]
BIT_IDENTICAL_TO_0 = {17, 23, 24, 25, 26, 27, 29, 30, 33}
STATS = {}          # (family, output dtype) -> [worst err/bound, worst RMS]


def _family(cfg):
    return "filter-direct" if cfg in BIT_IDENTICAL_TO_0 - {17} else ("pp8" if cfg == 17 else ("plane" if 18 <= cfg <= 20 else "igemm"))


def _note(fam, dt, v):
    s = STATS.setdefault((fam, str(dt).replace("torch.", "")), [0.0, 0.0])
    s[0], s[1] = max(s[0], v.err_over_bound), max(s[1], v.rms)


def sweep(L, fp16, B, seed, tail=0, n_random=2048):
    """Run every sweep id on one launch shape; returns (accepted ids, failure messages, inputs)."""
    inp = cr.make_inputs(L, fp16, B, "cuda", seed)
    ref = cr.reference(L, inp, cr.sample_rows(L, B, seed, n_random=n_random, tail=tail))
    accepted, fails, y0 = [], [], None
    dt = cr.out_dtype(L, fp16)
    for cfg in cr.SWEEP_IDS:
        y = cr.new_output(L, inp)
        try:
            cr.launch(L, inp, y, cfg, strict=True)
        except Exception as e:                                          # a refusal must name the id and say why
            if not (f"tile_cfg {cfg} cannot run" in str(e)):
                fails.append(f"tile {cfg}: unexpected error {e}")
            continue
        accepted.append(cfg)
        v = cr.check(L, y, ref)
        _note(_family(cfg), dt, v)
        print(f"  tile {cfg:2d}: err/bound {v.err_over_bound:.3g}  RMS {v.rms:.3g}{'' if v.ok else '  FAIL ' + v.why}")
        if not v.ok:
            fails.append(f"tile {cfg}: {v.why}")
        if cfg == 0:
            y0 = y
        elif cfg in BIT_IDENTICAL_TO_0 and y0 is not None and not torch.equal(y.t.view(y.ity), y0.t.view(y0.ity)):
            n = int((y.t.view(y.ity) != y0.t.view(y0.ity)).sum())
            fails.append(f"tile {cfg}: {n} outputs differ from tile 0 (stated bit-identical)")
    return accepted, fails, inp


@pytest.mark.parametrize("fp16,batch", CONFIGS, ids=[f"{'fp16' if h else 'fp32'}-B{b}" for h, b in CONFIGS])
@pytest.mark.parametrize("layer,mult", LAYERS, ids=[L.name for L, _ in LAYERS])
def test_every_tile_at_the_layer_shape(layer, mult, fp16, batch):
    L = layer if fp16 else dataclasses.replace(layer, out_f32=False)
    B = batch * mult
    t0 = time.time()
    print(f"\n[{L.name} {'fp16' if fp16 else 'fp32'} B={batch}] M={B * L.Ho * L.Wo} K={L.K} N={L.Cout}")
    accepted, fails, _ = sweep(L, fp16, B, seed=zlib.crc32(f"{L.name} {fp16} {batch}".encode()))
    tuned = cr.tuner_ids(L, fp16, B)
    print(f"  ids run: {accepted}; tuner candidates: {sorted(tuned)}; {time.time() - t0:.1f} s")
    assert not fails, "\n".join(fails)
    assert accepted == [c for c in cr.SWEEP_IDS if cr.tile_runs(c, L, fp16, B)]
    assert set(tuned) <= set(accepted), f"the tuner would time {sorted(set(tuned) - set(accepted))}, which this launch refuses"


# ---- the 4 GB limit: inputs just under 0xfffffff0 - 1 MB bytes (32-bit buffer offsets; padding reads rely on OOB = 0xfffffff0) ----
LIM = 0xFFFFFFF0 - (1 << 20)
BIG = [   # (layer, fp16): B = 1, H * W * Cin * es just below LIM
    (C("4gb.fp16", 256, 256, 3, 1, 1, 1513, 5543, scale=False), True),      # 496 bytes below
    (C("4gb.fp32", 256, 256, 3, 1, 1, 1023, 4099, scale=False), False),     # 3 056 bytes below
]


@pytest.mark.parametrize("layer,fp16", BIG, ids=[L.name for L, _ in BIG])
def test_every_tile_just_under_the_4gb_input_limit(layer, fp16):
    L = layer
    es = 2 if fp16 else 4
    nbytes = L.H * L.W * L.Cin * es
    assert LIM - 4096 < nbytes < LIM
    print(f"\n[{L.name}] input {nbytes} bytes = LIM - {LIM - nbytes}")
    accepted, fails, inp = sweep(L, fp16, 1, seed=7, tail=L.Wo * 8, n_random=4096)     # random rows in the last 8 output rows
    print(f"  ids run: {accepted}")
    assert not fails, "\n".join(fails)
    assert accepted == [c for c in cr.SWEEP_IDS if cr.tile_runs(c, L, fp16, 1)]
    # one pixel more (B = 1, H = 1: the smallest step over the limit at Cin = 256) is refused before any launch; the buffers
    # passed are the ones above, and the pixels past their end stay inside the 64 KB guards
    px = L.H * L.W + (1 if fp16 else 3)
    assert px * L.Cin * es >= LIM and (px - L.H * L.W) * L.Cin * es <= cr.GUARD_BYTES
    y = cr.new_output(L, inp)
    with pytest.raises(Exception, match="4 GB"):
        cr.launch(dataclasses.replace(L, H=1, W=px), inp, y, -1, strict=True)
    assert y.guards_intact() and y.pattern_count() == y.n


# ---- Winograd (fp32 engine) and the fused bottleneck tail at the same shapes ----
# |y - y64| <= C_W * 2^-24 * A   (A = |scale| S (1 + gamma_K) + |bias|, conv_ref.Reference.A): the transforms amplify rounding
# error, so the direct conv's gamma_K does not apply. C_W per form, fitted on an MI355X with a margin of 4x or more over the
# worst ratio measured at these shapes (WINO_WORST: F(2x2) on the mask head, both F(4x4) forms on the FPN output at p2).
C_W = {"F2x2": 16.0, "F4x4": 256.0, "F4x4-fold": 256.0}
WINO_WORST = {"F2x2": 3.6, "F4x4": 56.3, "F4x4-fold": 47.5}
WINO_LAYERS = [L for L, m in LAYERS if L.k == 3 and L.Cin >= 128 and m == 1] + [LAYERS[[L.name for L, _ in LAYERS].index("mask.conv")][0]]
WINO_FORMS = {"F2x2": {}, "F4x4": {"TD_WINO_TILE": "4", "TD_WINO_FOLD": "0"}, "F4x4-fold": {"TD_WINO_TILE": "4", "TD_WINO_FOLD": "1"}}


@pytest.mark.parametrize("layer", WINO_LAYERS, ids=[L.name for L in WINO_LAYERS])
def test_winograd_forms_at_the_layer_shapes(layer):
    from treedetection_amd import _lib
    lib = _lib.load()
    L = layer
    B = 8 * (100 if L.name == "mask.conv" else 1)
    inp = cr.make_inputs(L, False, B, "cuda", seed=zlib.crc32(L.name.encode()))
    ref = cr.reference(L, inp, cr.sample_rows(L, B, seed=3))
    p = lambda t: t.data_ptr() if t is not None else None      # noqa: E731
    fails = []
    for form, env in WINO_FORMS.items():
        y = cr.new_output(L, inp)
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            _lib.check(lib.td_conv2d_winograd_nhwc(p(inp["x"]), p(inp["w"]), p(inp["scale"]), p(inp["bias"]), p(y), B, L.H, L.W, L.Cin,
                                                   L.Cout, int(L.relu), _lib.stream_ptr()), "td_conv2d_winograd_nhwc")
        finally:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k)
                else:
                    os.environ[k] = v
        if not y.guards_intact() or y.pattern_count() or not bool(torch.isfinite(y.t).all()):
            fails.append(f"{form}: guard / unwritten / non-finite")
            continue
        got = y.t.reshape(-1, L.Cout)[ref.rows.cuda()].cpu().double()
        ratio = float(((got - ref.y64).abs() / (cr.U32 * ref.A)).max())
        s = STATS.setdefault((f"winograd {form}", "float32"), [0.0, 0.0])
        s[0] = max(s[0], ratio / C_W[form])
        print(f"\n[{L.name} {form}] max |err| / (2^-24 A) = {ratio:.1f} (C_W = {C_W[form]:g})")
        if ratio > C_W[form]:
            fails.append(f"{form}: |err| / (2^-24 A) = {ratio:.1f} > C_W")
    assert not fails, "\n".join(fails)


TAIL_SHAPES = [  # (fp16, B, H, W, mid): res2 (mid 64) and res3 (mid 128, fp16 only) at production map sizes
    (False, 8, 200, 200, 64), (False, 8, 200, 336, 64), (True, 8, 200, 200, 64), (True, 32, 200, 200, 64),
    (True, 8, 100, 100, 128), (True, 32, 100, 100, 128), (True, 8, 100, 168, 128),
]


@pytest.mark.parametrize("case", TAIL_SHAPES)
def test_bottleneck_tail_equals_the_two_launches_at_production_maps(case):
    from treedetection_amd import _lib
    lib = _lib.load()
    fp16, B, H, W, mid = case
    cout = 4 * mid
    L2 = C("conv2", mid, mid, 3, 1, 1, H, W)
    L3 = C("conv3", mid, cout, 1, 1, 0, H, W, res=1)
    a = cr.make_inputs(L2, fp16, B, "cuda", seed=B + H + mid)
    b = cr.make_inputs(L3, fp16, B, "cuda", seed=B + W + mid)
    t = cr.new_output(L2, a)
    cr.launch(L2, a, t, -1, strict=False)
    b["x"] = t
    two = cr.new_output(L3, b)
    cr.launch(L3, b, two, -1, strict=False)
    y = cr.new_output(L3, b)
    p = lambda v: v.data_ptr() if v is not None else None      # noqa: E731
    _lib.check(lib.td_bottleneck_tail_nhwc(p(a["x"]), p(a["w"]), p(a["scale"]), p(a["bias"]), p(b["w"]), p(b["scale"]), p(b["bias"]),
                                           p(b["res"]), p(y), B, H, W, mid, cout, 1 if fp16 else 0, _lib.stream_ptr()), "td_bottleneck_tail_nhwc")
    assert y.guards_intact() and y.pattern_count() == 0 and two.pattern_count() == 0
    assert bool(torch.isfinite(y.t).all())
    assert torch.equal(y.t.view(y.ity), two.t.view(two.ity)), int((y.t != two.t).sum())


def test_print_the_measured_table():
    """(runs last in this file) the worst err/bound and RMS per kernel family and output dtype, for the record."""
    for (fam, dt), (eb, rms) in sorted(STATS.items()):
        print(f"\n[table] {fam:20s} {dt:8s} worst err/bound {eb:.3g}  worst RMS {rms:.3g}")
    assert math.isfinite(sum(v[0] for v in STATS.values()))
