"""Harness of tests/test_mask_convs_gpu.py: phase 4 of the forward (mask_fcn1..4 and the 2x2 deconvolution, every launch
trimmed to the device row count ``mask_total_rows``) run ALONE on a crafted ``pooled14`` and a chosen count, in the manner of
tests/det_stage.py. Phases 0 to 3 of the flat 64 x 96 batch (B = 3, D = 100: 300 reserved RoIs) run once per engine; before
every run of phase 4 ``pooled14`` is overwritten (seeded fp16-representable values in the live RoIs, quiet NaN in every RoI at
or past the count), ``mask_total_rows`` is overwritten, and ``mask_fcn3`` / ``mask_fcn4`` / ``mask_deconv`` are filled with the
conv_ref sentinel, so "nothing past the count" is a statement about what the kernels wrote. The float64 side: the chain
pooled14 -> mask_fcn3 with its recursive error bound, and the weights as the engine holds them."""
import os

import numpy as np
import torch
import torch.nn.functional as F

from tests import conv_ref as cr
from tests import det_cases as dc
from tests.det_stage import flat_batch
from tests.gpu_util import engine_tensor_view

ROIS, SIDE = 3 * dc.D, 14
HW = SIDE * SIDE
BUFFERS = ("mask_fcn3", "mask_fcn4", "mask_deconv")


def make_engine(env, precision, sd):
    """An engine created under `env` (the variables are read at creation; restored after), with phases 0 to 3 of the flat
    batch done: one plain forward (tunes every launch, registers the names), then the phases one by one, so that phase 4 can
    be repeated on its own."""
    from treedetection_amd.engine import Engine, INPUT_F32_CHW
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        eng = Engine(sd, precision=precision)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    out = eng.alloc_outputs(3, 96, 144, paste=True)
    eng.forward_raw(flat_batch(), INPUT_F32_CHW, dc.HW_VALID, dc.HW_OUT, out)
    torch.cuda.synchronize()
    st = torch.cuda.current_stream()
    eng.forward_phase(0, st, flat_batch(), INPUT_F32_CHW, dc.HW_VALID, dc.HW_OUT, out)
    for ph in (1, 2, 3, 4):                       # (4 once: the phase registers the names of its own buffers)
        eng.forward_phase(ph, st)
    torch.cuda.synchronize()
    return eng


def seeded_pooled(C, seed=41):
    """[300, 14, 14, C] float32 on the host, every value fp16-representable: |N(0,1)| with ~15% exact zeros (a post-ReLU map)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((ROIS, SIDE, SIDE, C), generator=g).abs_()
    x *= (torch.rand(x.shape, generator=g) > 0.15)
    return x.half().float()


def _ibits(t):
    return t.reshape(-1).view(torch.int16 if t.dtype == torch.float16 else torch.int32)


class Stored:
    """An engine buffer dressed as conv_ref.Guarded for conv_ref.check (the engine's allocations have no guard zones)."""

    def __init__(self, t):
        self.t, self.n = t, t.numel()
        self.ity, self.pattern = cr.SENTINEL[t.dtype]

    def guards_intact(self):
        return True

    def pattern_count(self):
        return int((_ibits(self.t) == self.pattern).sum().item())


def run_phase4(eng, pooled_dev, count):
    """Phase 4 alone on `pooled_dev` ([300,14,14,C] in the engine's dtype, on the device) with `count` live RoIs.
    -> {name: copy of the buffer as stored}. Asserts that the phase left its two inputs alone, bit for bit."""
    p14 = engine_tensor_view(eng, "pooled14")
    rows = engine_tensor_view(eng, "mask_total_rows", torch.int32)
    assert tuple(p14.shape) == tuple(pooled_dev.shape) and p14.dtype == pooled_dev.dtype and rows.numel() == 1
    qi, qv = cr.QNAN[p14.dtype]
    p14.copy_(pooled_dev)
    p14[count:].view(qi).fill_(qv)
    rows.fill_(count)
    for n in BUFFERS:
        v = engine_tensor_view(eng, n)
        si, sv = cr.SENTINEL[v.dtype]
        v.view(si).fill_(sv)
    wrote = p14.clone()
    torch.cuda.synchronize()
    eng.forward_phase(4, torch.cuda.current_stream())
    torch.cuda.synchronize()
    assert int(engine_tensor_view(eng, "mask_total_rows", torch.int32).item()) == count, "mask_total_rows"
    assert torch.equal(_ibits(engine_tensor_view(eng, "pooled14")), _ibits(wrote)), "pooled14"
    return {n: engine_tensor_view(eng, n).clone() for n in BUFFERS}


def layer_weights(sd, fp16):
    """(w [Cout,k,k,Cin], bias) per mask-head layer as the engine holds them (fp16 engine: weights rounded to fp16, biases
    float32), on the host; the deconvolution as the 1x1 layer with rows n = (dy*2+dx)*Cq + co from ConvTranspose2d's [Cin,Cq,2,2]."""
    dt = torch.float16 if fp16 else torch.float32
    out = {}
    for i in range(1, 5):
        w = torch.from_numpy(np.asarray(sd[f"roi_heads.mask_head.mask_fcn{i}.weight"], dtype=np.float32))
        out[f"fcn{i}"] = (w.permute(0, 2, 3, 1).contiguous().to(dt), torch.from_numpy(np.asarray(sd[f"roi_heads.mask_head.mask_fcn{i}.bias"], dtype=np.float32)))
    wd = torch.from_numpy(np.asarray(sd["roi_heads.mask_head.deconv.weight"], dtype=np.float32))       # [Cin, Cq, dy, dx]
    ci, cq = wd.shape[:2]
    out["deconv"] = (wd.permute(2, 3, 1, 0).reshape(4 * cq, 1, 1, ci).contiguous().to(dt),
                     torch.from_numpy(np.asarray(sd["roi_heads.mask_head.deconv.bias"], dtype=np.float32)))
    return out


def own_bound(S, A, K, y64, prop, fp16, c_w):
    """The single-layer bound of one form (tests/conv_ref.py for the direct tiles, C_W 2^-24 A for a Winograd form; an fp16
    output adds its rounding of everything that can reach it), every term float64."""
    gamma = 1.05 * K * cr.U32
    own = c_w * cr.U32 * A if c_w else gamma * S + 4 * cr.U32 * A
    if fp16:
        own = own + cr.U16 * (y64.abs() + prop + own) + 2.0 ** -25
    return own


def chain_fcn3(pooled_rois, weights, fp16, c_w):
    """float64 mask_fcn1..3 of whole RoIs ([n,14,14,C] host) and the recursive bound on the engine's mask_fcn3:
    E_L = own_L + |W_L| * E_{L-1}, E_0 = 0 (no scale in the mask head; ReLU is 1-Lipschitz), own_L the single-layer bound
    of the form on inputs as large as |x64_{L-1}| + E_{L-1}. -> (y64, E) as [n,14,14,C]."""
    x = pooled_rois.double().permute(0, 3, 1, 2)
    E = torch.zeros_like(x)
    for i in (1, 2, 3):
        w, b = weights[f"fcn{i}"]
        w = w.double().permute(0, 3, 1, 2)
        b = b.double()[None, :, None, None]
        K = w[0].numel()
        prop = F.conv2d(E, w.abs(), padding=1)
        S = F.conv2d(x.abs() + E, w.abs(), padding=1)
        y = (F.conv2d(x, w, padding=1) + b).clamp_min(0)
        A = S * (1 + 1.05 * K * cr.U32) + b.abs()
        E = own_bound(S, A, K, y, prop, fp16, c_w) + prop
        x = y
    return x.permute(0, 2, 3, 1).contiguous(), E.permute(0, 2, 3, 1).contiguous()
