"""td_roi_align against float64 in both precisions, on every kernel path (tests/roi_ref.py holds the checker).

Kernels: fp32 roi_align_kernel<float>; fp16 roi_align_h8_kernel (C % 8 == 0, C <= 256, map below 2^32 elements) and
roi_align_kernel<_Float16> (C % 8 == 4 or C > 256). Each (precision, C, pooled) runs four RoI families, each through
checks (a) exact oracle bits, (b) float64 error bound and (c) guard zones:

* "edges"  (45 x 37 map, scale 1): the whole map, over each border, outside, zero area, inverted, sub-pixel, samples
  exactly on -1, 0, size - 1 and size, and random RoIs, all of them clear of pixel (0, 0). Pixel (0, 0) holds NaN, +Inf
  or -Inf in every channel, so any stray read of it (an out-of-map sample is loaded from there and must be dropped)
  shows up as a non-finite output.
* "origin" (same map): the RoIs of that list whose samples do read pixel (0, 0): NaN / Inf where the oracle has them.
* "direct" (400 x 13 map): RoIs 380 px tall, so pooled * gh > 336 and the kernels take their direct (non-table) path.
* "scaled" (23 x 29 map, scale 1 / 4): random RoIs.

The speed knobs TD_ROI_DEPTH / TD_ROI_PARTS / TD_ROI_H8 are read once per process, so the whole case list re-runs in
child processes (``python -m tests.test_roi_align_gpu --dump FILE``) and must give the parent's outputs bit for bit.
"""
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

from tests import roi_ref as rr

CS = (4, 8, 12, 64, 252, 256, 260, 512)
POOLEDS = (1, 2, 7, 11, 12, 14)
CMAX = max(CS)
TD_OK = 0

# name: (H, W, scale, seed)
MAPS = {"edges": (45, 37, 1.0, 1), "direct": (400, 13, 1.0, 2), "scaled": (23, 29, 0.25, 3)}
FAMILIES = ("edges", "origin", "direct", "scaled")


def kernel_of(fp16: bool, C: int) -> str:
    if not fp16:
        return "fp32 roi_align_kernel<float>"
    return "fp16 roi_align_h8_kernel" if C % 8 == 0 and C <= 256 else "fp16 roi_align_kernel<_Float16>"


def map_values(name: str, fp16: bool) -> np.ndarray:
    """[H, W, CMAX] float32 features (fp16-representable for fp16); the edges map has its (0, 0) pixel poisoned."""
    H, W, _, seed = MAPS[name]
    f = np.random.default_rng(seed).standard_normal((H, W, CMAX), dtype=np.float32)
    if fp16:
        f = f.astype(np.float16).astype(np.float32)
    if name == "edges":
        f[0, 0, 0::3] = np.nan
        f[0, 0, 1::3] = np.inf
        f[0, 0, 2::3] = -np.inf
    return f


def all_rois(name: str, pooled: int) -> np.ndarray:
    H, W, scale, seed = MAPS[name]
    rng = np.random.default_rng(100 * seed + pooled)
    if name == "edges":
        return np.concatenate([rr.edge_rois(H, W, pooled), rr.random_rois(rng, 24, H, W, 1.0, 30.0)])
    if name == "direct":
        return np.array([[1, 10, 9, 390], [-3, -5, 10.5, 395.25], [0, 0, W, H], [4.5, 0.25, 4.75, 399]], np.float32)
    return rr.random_rois(rng, 16, H, W, scale, 14.0)


def family_rois(fam: str, pooled: int):
    """(map name, RoIs, taps) of one family at one pooled size."""
    name = "edges" if fam == "origin" else fam
    H, W, scale, _ = MAPS[name]
    rois = all_rois(name, pooled)
    if name == "edges":
        hit = rr.touches_origin(rr.taps(rois, H, W, scale, pooled), rois.shape[0], pooled)
        rois = rois[hit] if fam == "origin" else rois[~hit]
    return name, rois, rr.taps(rois, H, W, scale, pooled)


_DEV = {}


def device_map(name: str, fp16: bool, C: int) -> torch.Tensor:
    key = (name, fp16, C)
    if key not in _DEV:
        if (name, fp16, CMAX) not in _DEV:
            _DEV[(name, fp16, CMAX)] = torch.from_numpy(map_values(name, fp16)).to(torch.float16 if fp16 else torch.float32).cuda()
        _DEV[key] = _DEV[(name, fp16, CMAX)][..., :C].contiguous()
    return _DEV[key]


def launch(feat: torch.Tensor, rois: np.ndarray, scale: float, pooled: int, fp16: bool) -> rr.Guarded:
    from treedetection_amd import _lib
    lib = _lib.load()
    H, W, C = feat.shape
    n = rois.shape[0]
    r = torch.from_numpy(np.ascontiguousarray(rois.reshape(-1, 4) if n else np.zeros((1, 4), np.float32))).cuda()
    out = rr.new_output(n * pooled * pooled, C, fp16, "cuda")
    _lib.check(lib.td_roi_align(feat.data_ptr(), H, W, C, r.data_ptr(), n, scale, pooled, out.data_ptr(), int(fp16),
                                _lib.stream_ptr()), "td_roi_align")
    torch.cuda.synchronize()
    return out


_REF = {}


def family_reference(fam: str, pooled: int, fp16: bool):
    key = (fam, pooled, fp16)
    if key not in _REF:
        name, rois, t = family_rois(fam, pooled)
        _REF[key] = (name, rois, rr.reference(t, rr.hwc_gather(map_values(name, fp16)), CMAX))
    return _REF[key]


STATS = {}       # kernel → [worst err / bound, exact elements, elements]


@pytest.mark.gpu
@pytest.mark.parametrize("pooled", POOLEDS)
@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
def test_roi_align_against_float64(fp16, C, pooled):
    fails = []
    for fam in FAMILIES:
        name, rois, ref = family_reference(fam, pooled, fp16)
        if rois.shape[0] == 0:
            continue
        out = launch(device_map(name, fp16, C), rois, MAPS[name][2], pooled, fp16)
        ref = ref.channels(C)
        v = rr.check(out, ref)
        fails += [f"{fam}: {f}" for f in v.failures]
        if fam != "origin":
            fin = np.isfinite(out.t.float().cpu().numpy())
            if not fin.all():
                fails.append(f"{fam}: {int((~fin).sum())} non-finite outputs from RoIs that never read pixel (0, 0)")
        s = STATS.setdefault(kernel_of(fp16, C), [0.0, 0, 0])
        s[0] = max(s[0], v.worst)
        s[1] += int(round(v.exact * out.n))
        s[2] += out.n
    assert not fails, "\n".join(fails)


@pytest.mark.gpu
def test_roi_families_cover_their_paths():
    """The case list reaches what it claims: RoIs that read pixel (0, 0) exist, the direct family's grids exceed the
    336-entry sample table, and the other families' grids fit it."""
    for pooled in POOLEDS:
        _, rois, _ = family_rois("origin", pooled)
        assert rois.shape[0] >= 3
        for fam, direct in (("direct", True), ("edges", False), ("scaled", False)):
            name, rois, _ = family_rois(fam, pooled)
            H, W, scale, _ = MAPS[name]
            side = np.maximum(rois[:, 2] - rois[:, 0], rois[:, 3] - rois[:, 1]) * np.float32(scale)
            assert ((pooled * np.ceil(side / np.float32(pooled)) > 336) == direct).all(), (fam, pooled)


@pytest.mark.gpu
def test_roi_align_zero_rois_writes_nothing():
    from treedetection_amd import _lib
    lib = _lib.load()
    for fp16 in (False, True):
        feat = device_map("scaled", fp16, 64)
        r = torch.zeros((1, 4), dtype=torch.float32, device="cuda")
        out = rr.new_output(7 * 7, 64, fp16, "cuda")
        st = lib.td_roi_align(feat.data_ptr(), 23, 29, 64, r.data_ptr(), 0, 0.25, 7, out.data_ptr(), int(fp16), _lib.stream_ptr())
        torch.cuda.synchronize()
        assert st == TD_OK
        assert out.guards_intact() and out.pattern_count() == out.n


@pytest.mark.gpu
def test_roi_align_report():
    """(prints the per-kernel summary of test_roi_align_against_float64: worst err / bound, share of exact elements)"""
    for k, (worst, ex, n) in sorted(STATS.items()):
        print(f"\n{k}: worst err/bound {worst:.3f}, exact {ex}/{n} = {ex / max(n, 1):.6f}")
    assert all(ex == n for _, ex, n in STATS.values())


# ---- the speed knobs, in child processes ------------------------------------------------------------------------------
def dump_outputs() -> dict:
    """sha256 of every output of the case list under this process's knobs."""
    h = {}
    for fp16 in (False, True):
        for C in CS:
            for pooled in POOLEDS:
                for fam in FAMILIES:
                    name, rois, _ = family_rois(fam, pooled)
                    if rois.shape[0] == 0:
                        continue
                    out = launch(device_map(name, fp16, C), rois, MAPS[name][2], pooled, fp16)
                    h[f"{'fp16' if fp16 else 'fp32'} C={C} pooled={pooled} {fam}"] = hashlib.sha256(
                        out.buf.cpu().numpy().tobytes()).hexdigest()
    return h


# Every instantiation of each dispatch switch: fp32 depths 1 2 3 4 6 8 (4: the parent), h8 depths 1 2 3 4 (2: the
# parent), roi_align_kernel<_Float16> depths 1 2 3 4 6 8 (through C % 8 == 4 and C > 256 in every process, and under
# TD_ROI_H8=0 on the h8-shaped C as well at 2 6 8); TD_ROI_PARTS 1-4 (1 and 4 also the parent's defaults for pooled 7 / 14).
KNOBS = [
    {"TD_ROI_DEPTH": "1", "TD_ROI_PARTS": "1"},
    {"TD_ROI_DEPTH": "2", "TD_ROI_PARTS": "2", "TD_ROI_H8": "0"},
    {"TD_ROI_DEPTH": "3", "TD_ROI_PARTS": "3"},
    {"TD_ROI_DEPTH": "4", "TD_ROI_PARTS": "4"},
    {"TD_ROI_DEPTH": "6", "TD_ROI_H8": "0"},
    {"TD_ROI_DEPTH": "8", "TD_ROI_PARTS": "3", "TD_ROI_H8": "0"},
]


@pytest.mark.gpu
def test_roi_speed_knobs_give_identical_outputs(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    base = dump_outputs()
    for k, knob in enumerate(KNOBS):
        env = {kk: v for kk, v in os.environ.items() if kk not in ("TD_ROI_DEPTH", "TD_ROI_PARTS", "TD_ROI_H8")}
        env.update(knob)
        path = str(tmp_path / f"child{k}.json")
        r = subprocess.run([sys.executable, "-m", "tests.test_roi_align_gpu", "--dump", path], env=env, cwd=root,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, f"{knob}: exit {r.returncode}\n{r.stdout[-2000:]}{r.stderr[-2000:]}"
        with open(path) as f:
            got = json.load(f)
        assert got.keys() == base.keys()
        diff = [c for c in base if got[c] != base[c]]
        assert not diff, f"{knob}: {len(diff)} of {len(base)} outputs differ from the default knobs', e.g. {diff[:5]}"


# ---- a map of more than 2^32 elements ---------------------------------------------------------------------------------
BIG = 4100           # fp16, C = 256: 4100 * 4100 * 256 = 4.30e9 elements (8.6 GB)


def big_values(y: np.ndarray, x: np.ndarray) -> np.ndarray:
    c = np.arange(256, dtype=np.int64)
    return (((3 * y.astype(np.int64)[:, None] + 5 * x.astype(np.int64)[:, None] + c[None, :]) % 61 - 30) / 8).astype(np.float32)


@pytest.mark.gpu
def test_fp16_map_beyond_2_32_elements():
    """32-bit element offsets would wrap past row 4092 of this map (the last 8 rows) and read the wrong pixels without a
    fault; the launch has to index it in 64 bits."""
    C = 256
    torch.cuda.reset_peak_memory_stats()
    feat = torch.empty((BIG, BIG, C), dtype=torch.float16, device="cuda")
    assert feat.numel() >= 2 ** 32
    x = torch.arange(BIG, dtype=torch.int32, device="cuda")[None, :, None]
    c = torch.arange(C, dtype=torch.int32, device="cuda")[None, None, :]
    for y0 in range(0, BIG, 64):
        y = torch.arange(y0, min(y0 + 64, BIG), dtype=torch.int32, device="cuda")[:, None, None]
        feat[y0:y0 + 64] = ((3 * y + 5 * x + c) % 61 - 30).to(torch.float16) / 8
    del x, c, y
    rois = np.array([[4090.25, 4091.5, 4100, 4100], [4080, 4085.75, 4099.5, 4099], [10, 4080, 60, 4100],   # far rows
                     [4070, 4060, 4100, 4100], [100, 200, 140, 230], [2000, 2000, 2050, 2030], [4000, 10, 4030, 40],
                     [2, 3, 9, 11]], np.float32)
    fails = []
    for pooled in (7, 14):
        t = rr.taps(rois, BIG, BIG, 1.0, pooled)
        assert (t.yh >= 4092).any()
        ref = rr.reference(t, big_values, C)
        out = launch(feat, rois, 1.0, pooled, True)
        fails += [f"pooled {pooled}: {f}" for f in rr.check(out, ref).failures]
    peak = torch.cuda.max_memory_allocated()
    print(f"\npeak device memory {peak / 1e9:.2f} GB")
    del feat
    torch.cuda.empty_cache()
    assert not fails, "\n".join(fails)


if __name__ == "__main__":
    assert sys.argv[1] == "--dump"
    t0 = time.time()
    hashes = dump_outputs()
    with open(sys.argv[2], "w") as f:
        json.dump(hashes, f)
    print(f"{len(hashes)} outputs in {time.time() - t0:.1f} s")
