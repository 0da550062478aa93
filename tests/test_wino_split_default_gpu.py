"""The fp32 engine's unfolded F(4x4) layers contract their planes on the split-bf16 tiles by default (engine.cpp f32_split_wino,
TD_F32_SPLIT_WINO), on the 600 x 600 two-tile fixture of tests/test_tail_split_default_gpu.py: the default engine is bit-equal to
the switch at its default mask; against the switch at 0 (fp32 planes) it has equal counts, scores within 1e-4, boxes within 1e-2
and mask_probs within 1e-3 (tests/test_golden_gpu.py's tolerances) — and is NOT bit-equal: equal bits would mean the split planes
never ran."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEFAULT_MASK = "7"          # engine.cpp WINO_SPLIT_DEFAULT: conv2 of res4 / res5, the FPN outputs, the RPN conv


def _engine_outputs(sd, tiles, switch):
    from treedetection_amd.engine import Engine, INPUT_U8_HWC
    if switch is not None:
        os.environ["TD_F32_SPLIT_WINO"] = switch
    try:
        eng = Engine(sd, device=0, precision="fp32")
        images, hw_valid, hw_out = eng.preprocess_tiles_u8(tiles)
        o = eng.alloc_outputs(2, 600, 600, paste=False)
        eng.forward_raw(images, INPUT_U8_HWC, hw_valid, hw_out, o)
        eng.forward_raw(images, INPUT_U8_HWC, hw_valid, hw_out, o)          # second pass: measured tile choices in use
        torch.cuda.synchronize()
        out = {k: v.cpu().numpy().copy() for k, v in o.items()}
        eng.close()
    finally:
        os.environ.pop("TD_F32_SPLIT_WINO", None)
    return out


def _same(a, b):
    return all(np.array_equal(a[k][i][:int(a["count"][i])], b[k][i][:int(a["count"][i])]) for k in ("boxes", "scores", "mask_probs") for i in range(2))


def test_default_engine_runs_the_split_planes_and_agrees_with_the_fp32_planes():
    from treedetection_amd.synth import make_tile
    from treedetection_amd.weights import make_synthetic_state_dict
    sd = make_synthetic_state_dict(50, seed=0)
    tiles = [torch.from_numpy(make_tile(i, 600)[0]).cuda() for i in range(2)]
    default, on, off = _engine_outputs(sd, tiles, None), _engine_outputs(sd, tiles, DEFAULT_MASK), _engine_outputs(sd, tiles, "0")
    assert default["count"].sum() > 0 and np.array_equal(default["count"], on["count"])
    assert _same(default, on), f"the default engine differs from TD_F32_SPLIT_WINO={DEFAULT_MASK}"
    print(f"\ncounts: split planes {default['count'].tolist()}, fp32 planes {off['count'].tolist()}")
    assert np.array_equal(default["count"], off["count"])
    for k, tol in (("scores", 1e-4), ("boxes", 1e-2), ("mask_probs", 1e-3)):
        d = max(float(np.abs(default[k][i][:int(default["count"][i])] - off[k][i][:int(default["count"][i])]).max()) for i in range(2))
        print(f"max |d {k}| = {d:.3g} (tolerance {tol})")
        assert d <= tol, k
    assert not _same(default, off), "the default engine equals TD_F32_SPLIT_WINO=0 bit for bit: the split planes did not run"
