"""The path rule of the forward's contractions (csrc/conv_path.h) through its diagnostic entry td_conv_path: which form every R50
site takes under the default rules, what each rule flag moves, that the answer never depends on the batch, what a short workspace
does, and the literal tune keys (tune-cache files written before the rule became one function must still apply). Host only."""
import pytest

from treedetection_amd import _lib

DIRECT, SPLIT, F22, F43, FOLD = _lib.CONV_FORMS
OWN, IN_XFORM, IF_TILE = _lib.CONV_HEADS
FP32, FP16 = 0, 1
RULES = dict(precision=FP32, winograd=1, wino_fused=1, wino_minc=128, wino43_min=12, wino_fold=39, wino_slab=0, fuse_head=1)
SIDES = (200, 100, 50, 25, 13)          # p2 .. p6 of an 800 x 800 input
D = 100                                 # detections per image: the mask head reserves B * D RoIs


def reserve_elems(B):
    """td_engine_reserve's Winograd workspace at 800 x 800 (R50): 16 planes of the largest [2x2-output tiles] x [channels]."""
    t = lambda h: ((h + 1) // 2) ** 2
    need = max([B * t(h) * 256 for h in SIDES] + [B * t(h) * c for h, c in zip(SIDES, (64, 128, 256, 512))] + [B * D * t(14) * 256])
    return 16 * need


def test_reserve_elems_is_the_plans_winograd_allocation():
    """The restatement above against the engine's own workspace plan (td_workspace_plan): B = 8 at 800 x 800, R50 widths."""
    mid = [64, 128, 256, 512]
    rows = _lib.workspace_plan(FP32, 1, 1000, D, [64] + mid + mid + [4 * m for m in mid] + [256, 1024, 256], 8, 800, 800)
    assert {r["name"]: r["alloc_bytes"] for r in rows}["wino_v"] == 4 * reserve_elems(8)


def layer(cout, cin, k, scale=0, out_f32=0, banks=""):
    """banks: "2" F(2x2) filters, "4" F(4x4) filters, "s" split-bf16 (what the loader gives the layer under the default rules)"""
    return [cout, cin, k, k, scale, out_f32, "2" in banks, "4" in banks, "s" in banks]


def site(lay, side, B=8, stride=1, pad=None, relu=1, res=0, out_mode=0, dyn=0, mul=1, head=None):
    return dict(layer=lay, call=[B, side, side, stride, (lay[2] // 2 if pad is None else pad), relu, res, out_mode, dyn, mul], head=head)


def ask(s, wino_elems=None, **flags):
    r = dict(RULES, **flags)
    if wino_elems is None:
        wino_elems = reserve_elems(8)                      # every site of the table is a batch of 8
    return _lib.conv_path([r[k] for k in RULES], wino_elems, s["layer"], s["call"], s["head"])


RPN_HEAD = layer(15, 256, 1, out_f32=1)
conv2 = lambda c, side: site(layer(c, c, 3, scale=1, banks="24" if c >= 128 else "2"), side)
fpn_out = lambda side: site(layer(256, 256, 3, banks="24"), side, relu=0)
rpn = lambda side: site(layer(256, 256, 3, banks="24"), side, head=RPN_HEAD)
mask_fcn = lambda side: site(layer(256, 256, 3, banks="24"), side, B=8 * D, dyn=1, mul=side * side)
lateral = lambda **kw: site(layer(256, 1024, 1, banks="s"), 50, relu=0, **kw)
FC1 = site(layer(1024, 12544, 1, banks="s"), 1, B=8000)

# site -> (form, head placement) under the default rules of the fp32 engine, batch 8
TABLE = {
    "res2 conv2": (conv2(64, 200), DIRECT, OWN),
    "res3 conv2": (conv2(128, 100), FOLD, OWN),
    "res4 conv2": (conv2(256, 50), F43, OWN),
    "res5 conv2": (conv2(512, 25), F43, OWN),
    "fpn_output p2": (fpn_out(200), FOLD, OWN),
    "fpn_output p3": (fpn_out(100), FOLD, OWN),
    "fpn_output p4": (fpn_out(50), F43, OWN),
    "fpn_output p5": (fpn_out(25), F43, OWN),
    "rpn p2": (rpn(200), FOLD, OWN),
    "rpn p3": (rpn(100), F43, IN_XFORM),
    "rpn p4": (rpn(50), F43, IN_XFORM),
    "rpn p5": (rpn(25), F43, IN_XFORM),
    "rpn p6": (rpn(13), F43, IN_XFORM),
    "mask_fcn 14": (mask_fcn(14), FOLD, OWN),
    "mask_fcn 7 (odd side, device count)": (mask_fcn(7), DIRECT, OWN),
    "3x3 on 8x8": (site(layer(256, 256, 3, banks="24"), 8), F22, OWN),
    "mask deconv": (site(layer(1024, 256, 1), 14, B=8 * D, out_mode=1, dyn=1, mul=196), DIRECT, OWN),
    "fpn_lateral4": (lateral(), SPLIT, OWN),
    "fpn_lateral4 + half-resolution residual": (lateral(res=1), SPLIT, OWN),
    "fc1": (FC1, SPLIT, OWN),
    "conv3 + shortcut": (site(layer(1024, 256, 1, scale=1), 50, res=1), DIRECT, OWN),
}
STATIC = [n for n, (s, _, _) in TABLE.items() if not s["call"][8]]


@pytest.mark.parametrize("name", sorted(TABLE))
def test_default_rules_table(name):
    s, form, head = TABLE[name]
    got = ask(s)
    assert (got["form"], got["head"]) == (form, head)
    if name == "mask_fcn 14":
        assert got["fold_group"] == 8 * D                  # a device-side count: all reserved RoIs are one group
    if name == "3x3 on 8x8":
        assert got["key"] is None                          # wino_fused: F(2x2) has no tile to measure
    if name == "res4 conv2":
        assert got["key"][4] == 4 + 64


def test_split_layer_with_device_count_is_direct():
    """The split rule asks for static rows (the split kernels read no device row count): the bank alone does not make the form."""
    assert ask(lateral(B=8 * D, dyn=1, mul=2500))["form"] == DIRECT


@pytest.mark.parametrize("name", sorted(TABLE))
def test_fp16_engine_is_direct(name):
    s, _, _ = TABLE[name]
    got = ask(s, wino_elems=0, precision=FP16)
    assert got["form"] == DIRECT
    assert got["head"] == (IF_TILE if s["head"] else OWN)


def forms(**flags):
    got = {n: ask(s, **flags) for n, (s, _, _) in TABLE.items()}
    return {n: (g["form"], g["head"]) for n, g in got.items()}


DEFAULT = {n: (f, h) for n, (_, f, h) in TABLE.items()}


def test_flag_wino_fold_0():
    want = {n: ((F43, IN_XFORM if n == "rpn p2" else h) if f == FOLD else (f, h)) for n, (f, h) in DEFAULT.items()}
    assert forms(wino_fold=0) == want


def test_flag_wino_fold_7():
    assert forms(wino_fold=7) == dict(DEFAULT, **{"rpn p2": (F43, IN_XFORM)})


def test_flag_wino43_min_0():
    assert forms(wino43_min=0) == {n: ((F22, OWN) if f in (F22, F43, FOLD) else (f, h)) for n, (f, h) in DEFAULT.items()}


def test_flag_winograd_off():
    assert forms(winograd=0) == {n: ((DIRECT, OWN) if f in (F22, F43, FOLD) else (f, h)) for n, (f, h) in DEFAULT.items()}


def test_flag_fuse_head_off():
    assert forms(fuse_head=0) == {n: (f, OWN) for n, (f, h) in DEFAULT.items()}
    assert all(ask(s, wino_elems=0, precision=FP16, fuse_head=0)["head"] == OWN for s, _, _ in TABLE.values())


def test_flag_wino_minc_64():
    """res2 conv2 joins the Winograd path (the loader then gives it the F(4x4) bank; the fold kernel does not run 64 channels)"""
    s = site(layer(64, 64, 3, scale=1, banks="24"), 200)
    assert ask(s, wino_minc=64)["form"] == F43 and ask(s)["form"] == DIRECT
    got = forms(wino_minc=64)
    assert got.pop("res2 conv2") == (F22, OWN)             # (with the F(2x2) bank alone)
    assert got == {n: v for n, v in DEFAULT.items() if n != "res2 conv2"}      # nobody else moves


@pytest.mark.parametrize("name", STATIC)
def test_batch_invariance(name):
    s = TABLE[name][0]
    per_image = s["call"][0] // 8                          # fc1: 1000 rows per image
    at = lambda B: ask(dict(s, call=[B * per_image] + s["call"][1:]), wino_elems=reserve_elems(B))
    one = at(1)
    for B in range(1, 17):
        got = at(B)
        assert (got["form"], got["head"]) == (one["form"], one["head"]), B


def test_capacity():
    """res4 conv2, batch 8: F(4x4) needs 36 planes of the whole layer's 8 * 13 * 13 tiles, F(2x2) 16 planes of one slab's (with
    whole-layer slabs F(2x2) is the hungrier form on every map F(4x4) takes, so the steps show with 1024-tile slabs)."""
    s = TABLE["res4 conv2"][0]
    n43, n22 = 36 * 8 * 13 * 13 * 256, 16 * 1024 * 256
    assert ask(s, wino_elems=n43, wino_slab=1024)["form"] == F43
    assert ask(s, wino_elems=n43 - 1, wino_slab=1024)["form"] == F22
    assert ask(s, wino_elems=n22, wino_slab=1024)["form"] == F22
    assert ask(s, wino_elems=n22 - 1, wino_slab=1024)["form"] == DIRECT
    assert ask(s, wino_elems=16 * 8 * 25 * 25 * 256 - 1)["form"] == DIRECT        # whole-layer slabs: F(2x2) does not fit, nothing does


def test_tune_keys():
    """(cout, cin, kh*16+kw, rows, stride*4 + out_mode*2 + has_residual + flag): flag 64 the batched F(4x4) planes, 32 the F(2x2)
    planes of a slab, 128 a split layer."""
    s = TABLE["res4 conv2"][0]
    assert ask(s)["key"] == (256, 256, 17, 8 * 13 * 13, 68)
    assert ask(s, wino43_min=0, wino_fused=0)["key"] == (256, 256, 17, 8 * 25 * 25, 36)
    assert ask(s, wino43_min=0, wino_fused=0, wino_slab=4096)["key"] == (256, 256, 17, 4096, 36)
    assert ask(s, winograd=0)["key"] == (256, 256, 51, 8 * 50 * 50, 4)
    assert ask(FC1)["key"] == (1024, 12544, 17, 8000, 132)
    assert ask(dict(FC1, layer=layer(1024, 12544, 1)))["key"] == (1024, 12544, 17, 8000, 4)
    assert ask(lateral(res=1))["key"] == (256, 1024, 17, 8 * 50 * 50, 133)
    assert ask(TABLE["mask deconv"][0])["key"] == (1024, 256, 17, 800 * 196, 6)


def test_refuses_bad_arguments():
    lib = _lib.load()
    assert lib.td_conv_path(None, 0, None, None, None, None) == _lib.ERR_INVALID
