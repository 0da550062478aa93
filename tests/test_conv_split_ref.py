"""The numerics of the split-bf16 contraction (conv_split.hip), emulated on the CPU and judged by the checker the GPU tests use
(tests/conv_ref.py: float64 reference, per-element bound, RMS criterion with RMS_MAX unchanged): the six-product form passes, and
each form that keeps less — one second-order product dropped, or two pieces per operand instead of three — is rejected. Short-K
shapes only (K <= 256): at K >= 1024 the fp32 accumulation's own roundings hide these defects from the RMS criterion."""
import pytest

from tests import conv_ref as cr
from tests.conv_split_cases import DEFECTS, SHORT_K, emulate

_CACHE = {}


def _setup(i):
    if i not in _CACHE:
        L, B = SHORT_K[i]
        inp = cr.make_inputs(L, False, B, "cpu", seed=23 + i)
        _CACHE[i] = (L, inp, cr.reference(L, inp, cr.sample_rows(L, B, seed=5)))
    return _CACHE[i]


IDS = [L.name for L, _ in SHORT_K]


@pytest.mark.parametrize("i", range(len(SHORT_K)), ids=IDS)
def test_six_product_form_passes(i):
    L, inp, ref = _setup(i)
    v = cr.check(L, emulate(L, inp), ref)
    print(f"\n[six products, {L.name}] err/bound {v.err_over_bound:.3g}, RMS {v.rms:.3g}")
    assert v.ok, v.why


@pytest.mark.parametrize("defect", list(DEFECTS))
@pytest.mark.parametrize("i", range(len(SHORT_K)), ids=IDS)
def test_defective_form_is_rejected(i, defect):
    L, inp, ref = _setup(i)
    v = cr.check(L, emulate(L, inp, DEFECTS[defect]), ref)
    print(f"\n[{defect}, {L.name}] err/bound {v.err_over_bound:.3g}, RMS {v.rms:.3g}: {v.why}")
    assert not v.ok, f"{defect} passed the checker (err/bound {v.err_over_bound:.3g}, RMS {v.rms:.3g})"
