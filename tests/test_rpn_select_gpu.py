"""The proposal-selection stage (rpn.hip: rpn_keys_hist, rpn_topk_decode, nms_mask / nms_scan, rpn_merge) on crafted RPN
heads at the production map sizes — 800x800 and 800x1344, p2 = 120 000 / 201 600 anchors — against oracle/ops_ref.py.

The engine runs phase 0 of td_engine_forward_phase on a padded batch (half-width synthetic network: the stage depends on the
map sizes only), the five ``rpn_head*`` buffers are overwritten with a case of tests/rpn_cases.py, and phases 1..5 run on
them. Every image, level and row of every case is compared; tests/test_rpn_cases.py proves on the CPU which path of
rpn_topk_decode_kernel (fast / general unordered / general ordered) each image and level takes.

  * rpn_cand_idx: the oracle's top-k indices exactly (scores descending, ties by lower index), -1 beyond k;
    rpn_cand_scores bit-equal to the logits at those indices (a zero may come back with either sign);
  * rpn_cand_valid / rpn_cand_boxes: for zero deltas (exp(0) = 1: the decode is exact) equal to the oracle's
    finite-and-non-empty rule and clipped boxes exactly; else boxes within TOL_BOX, the 1e-3 px that
    test_engine_gpu.py::test_rpn_topk_nms_bit_exact_on_identical_inputs allows for expf, and the validity flag equal
    wherever that tolerance cannot move the decision: a non-finite row is invalid, and a finite one may only differ
    where an oracle edge lies within 2 * TOL_BOX of a clipping bound or of its opposite edge;
  * rpn_keep / rpn_keep_count: R.nms at 0.7 on the ENGINE's candidate boxes and scores, exactly;
  * proposals / proposal_scores / proposal_count: a numpy merge of the engine's keep lists (score descending, then
    level-major candidate index) exactly, zeros beyond the count (what rpn_merge_kernel writes); for zero-delta images
    the oracle's rpn_proposals end to end, exactly.
"""
import numpy as np
import pytest
import torch

from oracle import ops_ref as R
from oracle.maskrcnn_ref import MaskRCNNOracle
from tests import rpn_cases as rc
from tests.gpu_util import engine_tensor_view
from treedetection_amd.weights import make_synthetic_state_dict

pytestmark = pytest.mark.gpu

TOL_BOX = 1e-3
CAND = 1024          # RPN_CAND: candidate slots per (image, level)
NAMES = ("rpn_cand_idx", "rpn_cand_scores", "rpn_cand_valid", "rpn_cand_boxes", "rpn_keep", "rpn_keep_count", "proposals",
         "proposal_scores", "proposal_count")


@pytest.fixture(scope="module")
def engine_for():
    """One engine per map size, built on first use."""
    from treedetection_amd.engine import Engine
    torch.set_num_threads(8)
    sd = make_synthetic_state_dict(50, seed=3, width_div=2)
    made = {}

    def get(size):
        if size not in made:
            made[size] = Engine(sd)
        return made[size]
    yield get
    for e in made.values():
        e.close()


def run_stage(eng, case):
    """Phase 0 on a padded batch, the crafted heads over the engine's, phases 1..5 → the stage's tensors as numpy."""
    from treedetection_amd.engine import INPUT_F32_CHW
    hp, wp = case["size"]
    hw = case["hw_valid"]
    B = len(hw)
    x = torch.zeros((B, 3, hp, wp), dtype=torch.float32, device="cuda")
    for b, (h, w) in enumerate(hw):
        x[b, :, :h, :w] = 110.0
    out = eng.alloc_outputs(B, hp, wp, paste=False)
    st = torch.cuda.current_stream()
    eng.forward_phase(0, st, x, INPUT_F32_CHW, hw, hw, out)
    torch.cuda.synchronize()
    heads = rc.head_arrays(case)
    for l, head in enumerate(heads):
        view = engine_tensor_view(eng, f"rpn_head{l + 2}")
        assert tuple(view.shape) == head.shape, (l, tuple(view.shape), head.shape)
        view.copy_(torch.from_numpy(head))
    torch.cuda.synchronize()
    for phase in range(1, 6):
        eng.forward_phase(phase, st)
    torch.cuda.synchronize()
    for l, head in enumerate(heads):           # the stage read what the case wrote, bit for bit
        back = eng.tensor(f"rpn_head{l + 2}").cpu().numpy()
        assert np.array_equal(back.view(np.uint32), head.view(np.uint32)), l
    got = {n: eng.tensor(n).cpu().numpy() for n in NAMES}
    got["det_count"] = out["count"].cpu().numpy()
    return got


def same_scores(a, b):
    """Bit-equal, or both zero (a zero's sign is not kept by the key)."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | ((a == 0) & (b == 0))).all())


def merge_ref(cand_boxes, cand_scores, keep, keep_count):
    """One image: the kept candidates of the five levels by (score descending, level-major candidate index ascending)."""
    lv = np.concatenate([np.full(int(keep_count[l]), l, dtype=np.int64) for l in range(5)])
    ci = np.concatenate([keep[l, : int(keep_count[l])].astype(np.int64) for l in range(5)])
    sc = cand_scores[lv, ci]
    order = np.lexsort((lv * CAND + ci, -sc.astype(np.float64)))[: rc.POST_K]
    return cand_boxes[lv[order], ci[order]], sc[order]


@pytest.mark.parametrize("name", rc.CASE_NAMES)
def test_selection_matches_the_oracle(name, engine_for):
    case = rc.make_case(name)
    got = run_stage(engine_for(case["size"]), case)
    hw = case["hw_valid"]
    B = len(hw)
    logits = [torch.from_numpy(a) for a in case["logits"]]
    deltas = [torch.from_numpy(a) for a in case["deltas"]]
    with np.errstate(all="ignore"):
        props, taps = MaskRCNNOracle({}).rpn_proposals(logits, deltas, case["feat_hw"], hw)
    assert got["rpn_cand_idx"].shape == (B, 5, CAND) and got["rpn_cand_boxes"].shape == (B, 5, CAND, 4)
    assert got["rpn_keep"].shape == (B, 5, CAND) and got["rpn_keep_count"].shape == (B, 5)
    assert got["proposals"].shape == (B, rc.POST_K, 4)
    for b in range(B):
        ih, iw = hw[b]
        exact = case["zero_deltas"][b]
        for l in range(5):
            at = (name, b, f"p{l + 2}", case["intent"][b][l])
            ref = taps[b]["per_level"][l]
            idx = ref["topk_idx"]
            k = len(idx)
            g_idx, g_sc = got["rpn_cand_idx"][b, l], got["rpn_cand_scores"][b, l]
            g_ok, g_box = got["rpn_cand_valid"][b, l], got["rpn_cand_boxes"][b, l]
            # ---- top-k: indices, order, scores; empty slots
            if not np.array_equal(g_idx[:k], idx):
                bad = np.nonzero(g_idx[:k] != idx)[0]
                raise AssertionError(f"{at}: top-k differs at {len(bad)} ranks, first {bad[0]}: engine {g_idx[bad[:8]]} "
                                     f"(scores {g_sc[bad[:8]]}), oracle {idx[bad[:8]]} (scores {ref['topk_scores'][bad[:8]]})")
            assert same_scores(g_sc[:k], case["logits"][l][b][idx]), at
            assert (g_idx[k:] == -1).all() and (g_sc[k:] == 0).all() and (g_ok[k:] == 0).all() and (g_box[k:] == 0).all(), at
            assert np.isin(g_ok, (0, 1)).all(), at
            # ---- decode, clip, validity
            dec = ref["decoded"]
            with np.errstate(all="ignore"):
                fin = np.isfinite(dec).all(axis=1) & np.isfinite(ref["topk_scores"])
                clipped = R.clip_boxes(dec, ih, iw)
                ne = ((clipped[:, 2] - clipped[:, 0]) > 0) & ((clipped[:, 3] - clipped[:, 1]) > 0)
            r_ok = fin & ne
            if exact:
                assert np.array_equal(g_ok[:k] > 0, r_ok), (at, int(((g_ok[:k] > 0) != r_ok).sum()))
                assert np.array_equal(g_box[:k][r_ok], clipped[r_ok]), at
            else:
                with np.errstate(all="ignore"):
                    edge = dec[:, [0, 2, 1, 3]]
                    bound = np.array([iw, iw, ih, ih], dtype=np.float32)
                    near = (np.abs(edge) <= 2 * TOL_BOX) | (np.abs(edge - bound) <= 2 * TOL_BOX)
                    thin = (np.abs(dec[:, 2] - dec[:, 0]) <= 2 * TOL_BOX) | (np.abs(dec[:, 3] - dec[:, 1]) <= 2 * TOL_BOX)
                open_ = fin & (near.any(axis=1) | thin)
                diff = ((g_ok[:k] > 0) != r_ok) & ~open_
                assert not diff.any(), (at, "validity differs at ranks", np.nonzero(diff)[0][:8], "deltas",
                                        case["deltas"][l][b][idx[diff]][:4], "engine boxes", g_box[:k][diff][:4])
                both = (g_ok[:k] > 0) & r_ok
                if both.any():
                    assert np.abs(g_box[:k][both] - clipped[both]).max() < TOL_BOX, at
            # ---- per-level NMS on the engine's own candidates
            v = g_ok > 0
            ref_keep = np.nonzero(v)[0][R.nms(g_box[v], g_sc[v], 0.7)]
            assert got["rpn_keep_count"][b, l] == len(ref_keep), at
            assert np.array_equal(got["rpn_keep"][b, l, : len(ref_keep)], ref_keep), at
        # ---- merge over the levels
        m_box, m_sc = merge_ref(got["rpn_cand_boxes"][b], got["rpn_cand_scores"][b], got["rpn_keep"][b], got["rpn_keep_count"][b])
        n = int(got["proposal_count"][b])
        assert n == len(m_sc), (name, b)
        assert same_scores(got["proposal_scores"][b, :n], m_sc), (name, b, "merge order")
        assert np.array_equal(got["proposals"][b, :n], m_box), (name, b, "merge boxes")
        assert (got["proposals"][b, n:] == 0).all() and (got["proposal_scores"][b, n:] == 0).all(), (name, b)
        if exact:
            r_box, r_sc = props[b]
            assert n == len(r_sc), (name, b, n, len(r_sc))
            assert np.array_equal(got["proposal_scores"][b, :n], r_sc), (name, b, "oracle order")
            assert np.array_equal(got["proposals"][b, :n], r_box), (name, b, "oracle boxes")
        if case["survivors"][b] == "0":
            assert n == 0 and (got["rpn_keep_count"][b] == 0).all() and (got["rpn_cand_valid"][b] == 0).all(), (name, b)
            assert got["det_count"][b] == 0, (name, b)
        elif case["survivors"][b] == ">":
            assert n == rc.POST_K and int(got["rpn_keep_count"][b].sum()) > rc.POST_K, (name, b)
        elif case["survivors"][b] == "<":
            assert 0 < n == int(got["rpn_keep_count"][b].sum()) < rc.POST_K, (name, b)
