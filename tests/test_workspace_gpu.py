"""The engine against its own workspace plan (csrc/workspace.cpp, read through td_workspace_plan): after a forward td_engine_tensor
answers with the plan's rows, a name exists only once its phase has run, a reservation that grows the workspace withdraws the
names of the freed buffers, and neither growing a plan nor running below it moves an output bit. tests/test_workspace_plan.py
ties the same rows to what the engine replied before the plan existed."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests.test_workspace_plan import D, FP16, FP32, P, SHAPE_A, SHAPE_B, widths
from treedetection_amd import _lib
from treedetection_amd.engine import INPUT_F32_CHW, PHASE_STEM, Engine, unpack_outputs
from treedetection_amd.weights import make_synthetic_state_dict

pytestmark = pytest.mark.gpu

WIDTH_DIV = {"fp32": 2, "fp16": 1}      # the fp16 kernels contract 64-channel chunks: no 32-channel res2


@functools.lru_cache(maxsize=None)
def state_dict(width_div):
    return make_synthetic_state_dict(50, seed=3, width_div=width_div)


@functools.lru_cache(maxsize=None)
def images(shape):
    """Seeded smooth float32 [B,3,Hp,Wp] batch (low-frequency field + blobs: the random-weight model finds detections in it)."""
    B, Hp, Wp = shape
    rng = np.random.default_rng(7)
    yy, xx = np.meshgrid(np.arange(Hp), np.arange(Wp), indexing="ij")
    x = np.zeros((B, 3, Hp, Wp), dtype=np.float64)
    for b in range(B):
        for c in range(3):
            for _ in range(5):
                x[b, c] += 30 * np.cos(rng.uniform(0.01, 0.08) * xx + rng.uniform(0.01, 0.08) * yy + rng.uniform(0, 6))
        for _ in range(15):
            cy, cx, s = rng.uniform(0, Hp), rng.uniform(0, Wp), rng.uniform(5, 25)
            x[b] += np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))[None] * rng.uniform(-90, 90, (3, 1, 1))
    return np.clip(np.rint(x + 115), 0, 255).astype(np.float32)


def forward(eng, shape):
    """One whole forward at `shape` → the detections of every image (boxes, scores, mask probabilities of the live rows)."""
    B, Hp, Wp = shape
    x = torch.from_numpy(images(shape)).cuda()
    out = eng.alloc_outputs(B, Hp, Wp, paste=False)
    eng.forward_raw(x, INPUT_F32_CHW, [(Hp, Wp)] * B, [(Hp, Wp)] * B, out)
    torch.cuda.synchronize()
    return unpack_outputs(out, [(Hp, Wp)] * B, paste=False)


def same_bits(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert len(g["scores"]) == len(w["scores"])
        for k in ("pred_boxes", "scores", "pred_classes", "mask_probs"):
            assert np.array_equal(g[k], w[k]), k
    return sum(len(w["scores"]) for w in want)


def ask(eng, name):
    """td_engine_tensor by status: (status, dims, elem, message)"""
    ptr, dims, elem = C.c_void_p(), (C.c_int64 * 4)(), C.c_int()
    st = eng.lib.td_engine_tensor(eng._h, name.encode(), C.byref(ptr), dims, C.byref(elem))
    return st, list(dims), elem.value, eng.lib.td_last_error().decode()


def refused(eng, name):
    st, _, _, msg = ask(eng, name)
    return st == _lib.ERR_INVALID and f"no tensor named '{name}'" in msg


@pytest.mark.parametrize("shape", [SHAPE_A, SHAPE_B], ids=["a", "b"])
@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_tensors_answer_with_the_plans_rows(precision, shape):
    eng = Engine(state_dict(WIDTH_DIV[precision]), precision=precision)
    try:
        forward(eng, shape)
        rows = [r for r in _lib.workspace_plan({"fp32": FP32, "fp16": FP16}[precision], 1, P, D, widths(WIDTH_DIV[precision]), *shape)
                if r["public"]]
        assert len(rows) == 43
        for r in rows:
            st, dims, elem, msg = ask(eng, r["public"])
            assert st == 0, msg
            assert (dims, elem) == (r["dims"], r["elem"]), r["public"]
            nbytes = int(np.prod([d for d in dims if d > 0])) * elem
            dst = torch.empty(nbytes + 8, dtype=torch.uint8, device="cuda")
            read = lambda n: eng.lib.td_engine_read_tensor(eng._h, r["public"].encode(), dst.data_ptr(), n, _lib.stream_ptr())
            assert read(nbytes) == 0, r["public"]
            assert read(nbytes + elem) == _lib.ERR_INVALID and read(nbytes - elem) == _lib.ERR_INVALID, r["public"]
        torch.cuda.synchronize()
    finally:
        eng.close()


def test_a_name_exists_once_its_phase_has_run():
    B, Hp, Wp = SHAPE_B
    eng = Engine(state_dict(2))
    try:
        x = torch.from_numpy(images(SHAPE_B)).cuda()
        out = eng.alloc_outputs(B, Hp, Wp, paste=False)
        st = torch.cuda.current_stream()
        eng.forward_phase(PHASE_STEM, st, x, INPUT_F32_CHW, [(Hp, Wp)], [(Hp, Wp)], out)
        assert ask(eng, "stem")[0] == 0 and ask(eng, "pool")[0] == 0 and refused(eng, "res2")
        eng.forward_phase(0, st)
        assert ask(eng, "stem")[0] == 0 and ask(eng, "p6")[0] == 0 and ask(eng, "rpn_head6")[0] == 0 and refused(eng, "proposals")
        eng.forward_phase(1, st)
        assert ask(eng, "pooled7")[0] == 0 and refused(eng, "box_pred")
        for phase in (2, 3, 4, 5):
            eng.forward_phase(phase, st)
        torch.cuda.synchronize()
        assert ask(eng, "mask_probs_compact")[0] == 0
    finally:
        eng.close()


def test_growing_the_plan_withdraws_the_names_and_moves_no_output_bit():
    sd = state_dict(2)
    grown, fresh = Engine(sd), Engine(sd)
    try:
        forward(grown, SHAPE_B)
        assert ask(grown, "stem")[0] == 0
        grown.reserve(*SHAPE_A)                            # frees every buffer of the plan at (b)
        assert refused(grown, "stem")                      # ... so its names are gone, not left pointing into freed memory
        fresh.reserve(*SHAPE_A)
        assert same_bits(forward(grown, SHAPE_A), forward(fresh, SHAPE_A)) > 0
    finally:
        grown.close()
        fresh.close()


def test_a_forward_below_the_reservation_moves_no_output_bit():
    sd = state_dict(2)
    roomy, fresh = Engine(sd), Engine(sd)
    try:
        roomy.reserve(*SHAPE_A)
        assert same_bits(forward(roomy, SHAPE_B), forward(fresh, SHAPE_B)) > 0
        assert ask(roomy, "p6")[1] == [1, 3, 4, 128]       # the batch in hand, not the reservation
    finally:
        roomy.close()
        fresh.close()
