"""Helpers shared by the -m gpu tests: every call goes through the C ABI of libtreedet_hip.so."""
import numpy as np
import torch

from treedetection_amd import _lib


STRICT = 0x20000       # td_conv2d_nhwc precision bit: refuse a forced tile id the launch cannot run


def dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda().contiguous()


def conv2d_hip(x_nchw, w_oihw, scale=None, bias=None, residual_nchw=None, res_shift=0, stride=1, pad=0, relu=False,
               precision=0, tile_cfg=-1, out_f32=False, strict=False):
    """x [B,C,H,W] np → y [B,Co,Ho,Wo] np through td_conv2d_nhwc (``out_f32``: float16 tensors, float32 output;
    ``strict``: a forced ``tile_cfg`` this launch cannot run raises instead of running the heuristic tile)."""
    lib = _lib.load()
    dt = torch.float32 if precision == 0 else torch.float16
    x = dev(np.transpose(x_nchw, (0, 2, 3, 1)), dt)
    w = dev(np.transpose(w_oihw, (0, 2, 3, 1)), dt)
    B, H, W, Cin = x.shape
    Cout, KH, KW, _ = w.shape
    Ho = (H + 2 * pad - KH) // stride + 1
    Wo = (W + 2 * pad - KW) // stride + 1
    y = torch.empty((B, Ho, Wo, Cout), dtype=torch.float32 if out_f32 else dt, device="cuda")
    sc = dev(scale, torch.float32) if scale is not None else None
    bi = dev(bias, torch.float32) if bias is not None else None
    rs = dev(np.transpose(residual_nchw, (0, 2, 3, 1)), dt) if residual_nchw is not None else None
    p = lambda t: t.data_ptr() if t is not None else None
    st = lib.td_conv2d_nhwc(p(x), p(w), p(sc), p(bi), p(rs), res_shift, p(y), B, H, W, Cin, Cout, KH, KW, stride, pad,
                            int(relu), precision | ((tile_cfg + 1) << 8) | (0x10000 if out_f32 else 0) | (STRICT if strict else 0),
                            _lib.stream_ptr())
    _lib.check(st, "td_conv2d_nhwc")
    torch.cuda.synchronize()
    return y.float().cpu().numpy().transpose(0, 3, 1, 2)


def conv2d_head_hip(x_nchw, w_oihw, bias, head_w, head_b, pad, tile_cfg):
    """fp16 conv (+ bias, ReLU, 256 channels) with its 1x1 head fused (td_conv2d_head_nhwc) → head output [B,n,Ho,Wo] float32."""
    lib = _lib.load()
    x = dev(np.transpose(x_nchw, (0, 2, 3, 1)), torch.float16)
    w = dev(np.transpose(w_oihw, (0, 2, 3, 1)), torch.float16)
    B, H, W, Cin = x.shape
    Cout, KH, KW, _ = w.shape
    assert Cout == 256 and head_w.shape[1] == 256
    Ho, Wo = H + 2 * pad - KH + 1, W + 2 * pad - KW + 1
    n = head_w.shape[0]
    hw, hb, bi = dev(head_w.reshape(n, 256), torch.float16), dev(head_b, torch.float32), dev(bias, torch.float32)
    y = torch.full((B, Ho, Wo, n), float("nan"), dtype=torch.float32, device="cuda")
    st = lib.td_conv2d_head_nhwc(x.data_ptr(), w.data_ptr(), bi.data_ptr(), hw.data_ptr(), hb.data_ptr(), y.data_ptr(), B, H, W, Cin,
                                 KH, KW, pad, n, 1 | ((tile_cfg + 1) << 8) | STRICT, _lib.stream_ptr())
    _lib.check(st, "td_conv2d_head_nhwc")
    torch.cuda.synchronize()
    return y.cpu().numpy().transpose(0, 3, 1, 2)


class _DeviceArray:
    """A raw device pointer dressed as a __cuda_array_interface__ object (what torch.as_tensor takes for a zero-copy view)."""

    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False), "version": 2}


def engine_tensor_view(eng, name, dtype=None):
    """Zero-copy torch view of an engine buffer (the raw pointer td_engine_tensor returns), for stage tests that overwrite
    it between two phases: ``view.copy_(crafted)``. ``dtype``: None = the buffer's floating type (float32 for 4-byte
    elements, float16 for 2-byte ones); torch.int32 for the 4-byte integer buffers (counts, flags, index lists) — the ABI
    reports the element size only. The engine owns the memory; use the view at once."""
    import ctypes as C
    ptr, dims, elem = C.c_void_p(), (C.c_int64 * 4)(), C.c_int()
    _lib.check(eng.lib.td_engine_tensor(eng._h, name.encode(), C.byref(ptr), dims, C.byref(elem)), "td_engine_tensor")
    assert elem.value in (2, 4) and ptr.value, (name, elem.value)
    if dtype is None:
        dtype = torch.float32 if elem.value == 4 else torch.float16
    typestr = {torch.float32: "<f4", torch.int32: "<i4", torch.float16: "<f2"}[dtype]
    assert int(typestr[2]) == elem.value, (name, dtype, elem.value)
    return torch.as_tensor(_DeviceArray(ptr.value, [int(d) for d in dims if d > 0], typestr), device=torch.device("cuda", eng.device))
