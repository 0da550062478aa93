"""Harness shared by tests/test_det_select_gpu.py and tests/test_mask_tail_gpu.py: run the forward of a flat padded batch in
phases (td_engine_forward_phase), overwrite the inputs of phase 3 with a case of tests/det_cases.py, optionally the input
of phase 5 with a crafted ``mask_deconv``, and read everything back. Every output buffer and every intermediate buffer of
the stage is poisoned (NaN / 0xFF bytes) before the run, so "zeros beyond the count" is a statement about what the kernels
wrote."""
import numpy as np
import torch

from tests import det_cases as dc
from tests.gpu_util import engine_tensor_view

I32 = torch.int32
STAGE_F32 = ("det_all_boxes", "det_all_scores", "det_sorted_boxes", "det_sorted_scores", "det_boxes_net", "mask_logits",
             "mask_probs_compact")
STAGE_I32 = ("det_flags", "det_sorted_count", "det_keep", "det_keep_count")


def make_engine(kind, precision="fp32", sd=None):
    """A half-width synthetic engine of tests/det_cases.ENGINES, with every buffer name of the stage registered (one
    plain forward of the flat batch)."""
    from treedetection_amd.engine import Engine, INPUT_F32_CHW
    from treedetection_amd.weights import make_synthetic_state_dict
    if sd is None:
        sd = make_synthetic_state_dict(50, seed=3, width_div=2)
    eng = Engine(sd, precision=precision, **dc.ENGINES[kind])
    out = eng.alloc_outputs(3, 96, 144, paste=True)
    eng.forward_raw(flat_batch(), INPUT_F32_CHW, dc.HW_VALID, dc.HW_OUT, out)
    torch.cuda.synchronize()
    return eng


def flat_batch():
    x = torch.zeros((3, 3) + dc.SIZE, dtype=torch.float32, device="cuda")
    for b, (h, w) in enumerate(dc.HW_VALID):
        x[b, :, :h, :w] = 110.0
    return x


def poison(t):
    if t.dtype.is_floating_point:
        t.fill_(float("nan"))
    else:
        t.view(torch.uint8).fill_(0xFF)


def read(eng, name, dtype=None):
    return engine_tensor_view(eng, name, dtype).cpu().numpy()


def run_stage(eng, case, deconv_fn=None):
    """Phases 0..2, the case over ``proposals`` / ``proposal_count`` / ``box_pred``, phase 3, phase 4, optionally
    ``deconv_fn(total_rows, shape, dtype) -> tensor`` over ``mask_deconv``, phase 5. → dict of numpy arrays: the stage's
    buffers as phase 3 left them, the outputs after phase 5, and ``deconv`` (what phase 5 read, as stored)."""
    from treedetection_amd.engine import INPUT_F32_CHW
    B, P = 3, case["P"]
    assert eng.P == P and eng.D == dc.D and int(case["count"].max()) <= P and int(case["count"].min()) >= 0
    out = eng.alloc_outputs(B, 96, 144, paste=True)
    for t in out.values():
        poison(t)
    for n in STAGE_F32:
        poison(engine_tensor_view(eng, n))
    for n in STAGE_I32:
        poison(engine_tensor_view(eng, n, I32))
    st = torch.cuda.current_stream()
    eng.forward_phase(0, st, flat_batch(), INPUT_F32_CHW, case["hw_valid"], case["hw_out"], out)
    eng.forward_phase(1, st)
    eng.forward_phase(2, st)
    torch.cuda.synchronize()
    views = {"proposals": (case["props"], None), "proposal_count": (case["count"], I32), "box_pred": (case["box_pred"], None)}
    for n, (a, dt) in views.items():
        v = engine_tensor_view(eng, n, dt)
        assert tuple(v.shape) == a.shape, (n, tuple(v.shape), a.shape)
        v.copy_(torch.from_numpy(a))
    torch.cuda.synchronize()
    eng.forward_phase(3, st)
    torch.cuda.synchronize()
    got = {n: read(eng, n) for n in STAGE_F32[:5]}
    got.update({n: read(eng, n, I32) for n in STAGE_I32})
    for k in ("boxes", "scores", "classes", "count"):
        got[k] = out[k].cpu().numpy()
    eng.forward_phase(4, st)
    torch.cuda.synchronize()
    if deconv_fn is not None:
        v = engine_tensor_view(eng, "mask_deconv")
        crafted = deconv_fn(int(got["count"].sum()), tuple(v.shape), v.dtype)
        v.copy_(crafted.to(v.device))
        torch.cuda.synchronize()
    eng.forward_phase(5, st)
    torch.cuda.synchronize()
    for n, (a, dt) in views.items():               # the stage read what the case wrote, bit for bit
        back = read(eng, n, dt)
        assert np.array_equal(back.view(np.uint32), a.view(np.uint32)), n
    if deconv_fn is not None:
        back = engine_tensor_view(eng, "mask_deconv").cpu()
        assert torch.equal(back.view(torch.int16 if back.dtype == torch.float16 else torch.int32),
                           crafted.view(torch.int16 if crafted.dtype == torch.float16 else torch.int32)), "mask_deconv"
        got["deconv"] = back.numpy()
    for k in ("boxes", "scores", "classes", "count"):        # phases 4 and 5 leave the detections alone
        assert np.array_equal(out[k].cpu().numpy().view(np.uint32), got[k].view(np.uint32)), k
    for n in ("mask_logits", "mask_probs_compact"):
        got[n] = read(eng, n)
    for k in ("mask_probs", "mask_region", "mask_offset", "mask_bits"):
        got[k] = out[k].cpu().numpy()
    return got
