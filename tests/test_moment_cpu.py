"""Host side of moment search (no GPU): the entry points are declared, exported and bound and the descriptor mirrors the C struct;
the float64 brute force (tests/moment_ref.py, the reference of tests/test_moment_gpu.py) equals torch's normalize of the masked mean
dotted with the query, orders equal scores as the contract says, reports (-1, 0, -inf) where it must and counts IoU thresholds in
integers; the fixed-seed inputs of the GPU parity test leave fewer pairs undecided than its cap; VideoIndex and eval_localization
refuse bad arguments before any device work."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

from univl_amd import _lib, ops
from univl_amd import eval as uev
from univl_amd.retrieval import VideoIndex

import moment_ref as R
from retrieval_cases import header_fields as _header_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "univl_hip.h")).read()
needs_lib = pytest.mark.skipif(not _lib.available(), reason="libunivl_hip.so is not built")
NEW = ("univl_moment_sizeof", "univl_window_norms", "univl_moment_localize")
TOL = 2e-4                       # tests/test_retrieve_gpu.py: the project's fp32 score tolerance, what the GPU parity test allows


# ------------------------------------------------------------------------------------------------ binding
@needs_lib
def test_entry_points_are_declared_exported_and_bound_and_the_descriptor_mirrors_the_header():
    L = _lib.lib()
    declared = set(re.findall(r"\b(univl_[a-z0-9_]+)\s*\(", HEADER))
    for name in NEW:
        assert name in declared and name in _lib.EXPORTED and hasattr(L, name), name
    assert declared == set(_lib.EXPORTED)
    for name in ("univl_window_norms", "univl_moment_localize"):
        fn = getattr(L, name)
        assert fn.restype is C.c_int32 and list(fn.argtypes) == [C.c_void_p, C.c_void_p]
    assert list(_lib.Moment._fields_) == _header_fields("UnivlMoment")
    assert L.univl_moment_sizeof() == C.sizeof(_lib.Moment)
    assert _lib.Moment not in _lib._STRUCTS and len(_lib._STRUCTS) == 12                      # the numbered size tables stay as they are
    assert int(re.search(r"#define UNIVL_MOMENT_F_MAX (\d+)", HEADER).group(1)) == _lib.MOMENT_F_MAX == 128
    for name in ("window_norms", "moment_localize"):
        assert callable(getattr(ops, name))


@needs_lib
def test_no_cpu_fallback_and_null_descriptors():
    x, m = torch.zeros(2, 4, 768), torch.ones(2, 4, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.window_norms(x, m)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.moment_localize(torch.zeros(1, 768), x, m, torch.zeros(1, 1, dtype=torch.int32), 1, 2, normalize=False)
    L = _lib.lib()
    assert L.univl_window_norms(None, None) == -1 and L.univl_moment_localize(None, None) == -1           # UNIVL_EINVAL before any device call
    assert b"univl_moment_localize" in L.univl_last_error()


# ------------------------------------------------------------------------------------------------ the reference, by itself
def test_ref_window_score_is_the_models_masked_mean_normalised_and_dotted():
    """_mean_pooling_for_similarity with the mask narrowed to the window, F.normalize, the inner product -- in float64."""
    rng = np.random.RandomState(3)
    F = 11
    frames = rng.standard_normal((F, R.H)) * 1.01
    q = rng.standard_normal(R.H)
    mask = np.ones(F, dtype=np.int64)
    S_n, T = R.row_scores(q[None], frames, mask, True)
    S_m, _ = R.row_scores(q[None], frames, mask, False)
    for s, L in [(0, 1), (0, F), (10, 1), (3, 4), (7, 4), (2, 9), (5, 1)]:
        wm = torch.zeros(F, dtype=torch.float64)
        wm[s:s + L] = 1
        x = torch.from_numpy(frames)
        mean = (x * wm[:, None]).sum(0) / wm.sum()                        # modeling.py:_mean_pooling_for_similarity's video half
        want_n = float(torch.dot(torch.nn.functional.normalize(mean, dim=-1), torch.from_numpy(q)))
        want_m = float(torch.dot(mean, torch.from_numpy(q)))
        assert abs(R.window_score(q, frames, s, L, True) - want_n) <= 1e-12
        assert abs(R.window_score(q, frames, s, L, False) - want_m) <= 1e-12
        assert abs(S_n[0, s, L - 1] - want_n) <= 1e-12 and abs(S_m[0, s, L - 1] - want_m) <= 1e-12
        assert abs(T[s, L - 1] - float(torch.linalg.norm(mean * L))) <= 1e-10
    for s in range(F):
        assert np.all(S_n[0, s, F - s:] == R.NEG_INF) and np.all(T[s, F - s:] == 0)      # windows past the row's end


def test_ref_zero_window_takes_the_eps_branch():
    frames = np.zeros((3, R.H))
    frames[1, 0], frames[2, 0] = 2.0, -2.0
    q = np.zeros(R.H)
    q[0] = 1.0
    assert R.window_score(q, frames, 0, 1, True) == 0.0 and R.window_score(q, frames, 1, 2, True) == 0.0      # 0 / (1e-12 L)
    assert R.window_score(q, frames, 1, 1, True) == 1.0 and R.window_score(q, frames, 2, 1, True) == -1.0


def test_ref_tie_order_on_constructed_equal_scores():
    q = np.zeros(R.H)
    q[0] = 1.0
    same = np.zeros((6, R.H))
    same[:, 0], same[:, 1] = 3.0, 4.0                                     # six identical frames: every window scores the same in both modes
    ones = np.ones(6, dtype=np.int64)
    for normalize in (True, False):
        for lmin, lmax, want in ((1, 6, (0, 1)), (2, 5, (0, 2)), (6, 6, (0, 6)), (4, 4, (0, 4))):
            s, L, sc, margin = (a[0, 0] for a in R.localize(q[None], same[None], ones[None], [[0]], lmin, lmax, normalize))
            assert (s, L) == want and margin == (np.inf if lmin == lmax == 6 else 0.0)
            assert sc == (0.6 if normalize else 3.0)
    # equal scores at different starts AND lengths: frames 1 and 3 are alike, window (1, 1) wins over (3, 1); use_mil
    f = np.zeros((5, R.H))
    f[:, 0] = [1.0, 5.0, 2.0, 5.0, 5.0]
    s, L, sc, margin = (a[0, 0] for a in R.localize(q[None], f[None], np.ones((1, 5), dtype=np.int64), [[0]], 1, 2, False))
    assert (s, L, sc, margin) == (1, 1, 5.0, 0.0)                         # (3, 1), (4, 1) and (3, 2) score 5 as well
    s, L, sc, _ = (a[0, 0] for a in R.localize(q[None], f[None], np.ones((1, 5), dtype=np.int64), [[0]], 2, 2, False))
    assert (s, L, sc) == (3, 2, 5.0)


def test_ref_no_candidate_cases():
    rng = np.random.RandomState(4)
    frames = rng.standard_normal((3, 8, R.H))
    q = rng.standard_normal((2, R.H))
    mask = np.array([[0] * 8, [1, 1, 0, 0, 0, 0, 0, 0], [1, 1, 1, 0, 1, 1, 1, 1]])
    none = lambda out, i, j: (out[0][i, j], out[1][i, j], out[2][i, j]) == (-1, 0, R.NEG_INF)
    out = R.localize(q, frames, mask, [[0, 1, 2], [-1, 3, 1]], 3, 4, True)
    assert none(out, 0, 0)                                                # all-zero mask
    assert none(out, 0, 1) and none(out, 1, 2)                            # valid prefix shorter than lmin
    assert none(out, 1, 0) and none(out, 1, 1)                            # ids outside the gallery
    assert out[1][0, 2] in (3, 4) and (out[0][0, 2] == 0 or out[0][0, 2] >= 4)         # the hole: windows on both sides, none across
    across = R.localize(q, frames, mask, [[2], [2]], 5, 8, True)
    assert none(across, 0, 0) and none(across, 1, 0)
    assert not R.is_candidate(mask[2], 2, 3, 1, 8) and R.is_candidate(mask[2], 4, 4, 1, 8) and not R.is_candidate(mask[2], 5, 4, 1, 8)


def test_ref_iou_counts_decide_thresholds_in_integers():
    #            found            annotated         inter union
    cases = [((2, 4), (2, 4)),    # identical          4     4     1.0
             ((0, 2), (1, 2)),    # one of three       1     3     0.33..  >= 0.3
             ((0, 3), (1, 3)),    # exactly one half   2     4     0.5
             ((0, 7), (0, 10)),   # exactly 0.7        7     10    0.7
             ((0, 3), (0, 10)),   # exactly 0.3        3     10    0.3
             ((0, 2), (5, 2)),    # disjoint           0     4     0
             ((-1, 0), (3, 2)),   # no window          0     2     0
             ((0, 29), (0, 100))]  # just under 0.3    29    100
    found, gt = np.array([c[0] for c in cases]), np.array([c[1] for c in cases])
    m = R.iou_counts(found[:, 0], found[:, 1], gt[:, 0], gt[:, 1])
    assert m["n"] == 8 and m["n_empty"] == 1
    assert m["R1@0.3"] == 5 / 8 and m["R1@0.5"] == 3 / 8 and m["R1@0.7"] == 2 / 8
    assert m["mIoU"] == float(np.mean(np.array([4 / 4, 1 / 3, 2 / 4, 7 / 10, 3 / 10, 0.0, 0.0, 29 / 100])))


def test_ref_rank_moments_orders_by_score_then_row_and_puts_the_empty_last():
    idx = np.array([4, 2, -1, 7, 0])
    score = np.array([0.5, 0.9, R.NEG_INF, 0.5, R.NEG_INF])
    assert R.rank_moments(idx, score, 5).tolist() == [1, 0, 3, 4, 2]
    assert R.rank_moments(idx, score, 2).tolist() == [1, 0]


@pytest.mark.parametrize("F", R.PARITY_F)
def test_parity_inputs_leave_few_pairs_undecided(F):
    """The GPU parity test compares start / length only where the reference's best two windows differ by more than its tolerance;
    on its fixed-seed inputs that leaves out less than the cap's share of the pairs it checks at this F, in either mode."""
    for normalize in (True, False):
        undecided = pairs = 0
        for P in R.PARITY_P:
            ref, _ = R.parity_reference(F, P, normalize)
            for w, (start, length, score, margin) in ref.items():
                undecided += int(np.sum((start >= 0) & (margin <= TOL)))
                pairs += P
                assert np.all((start >= 0) | (score == R.NEG_INF))
        print("F=%d normalize=%d: %d of %d pairs undecided" % (F, normalize, undecided, pairs))
        assert undecided < R.UNDECIDED_CAP * pairs, (F, normalize, undecided, pairs)


# ------------------------------------------------------------------------------------------------ refusals before any device work
def _fake_model(use_mil=False):
    return types.SimpleNamespace(task_config=types.SimpleNamespace(use_mil=use_mil), flat=types.SimpleNamespace(device="cpu"), training=False,
                                 eval=lambda: None, train=lambda mode=True: None)


def test_index_without_frames_refuses_to_localize():
    index = VideoIndex(_fake_model(), capacity=4)
    q = torch.zeros(2, 768)
    with pytest.raises(ValueError, match="keep_frames=True"):
        index.localize_vectors(q, torch.zeros(2, 1, dtype=torch.int32), (1, 2))
    with pytest.raises(ValueError, match="keep_frames=True"):
        VideoIndex(_fake_model(), capacity=4, keep_frames=True).localize_vectors(q, torch.zeros(2, 1, dtype=torch.int32), (1, 2))   # no videos yet
    ids = torch.zeros(2, 8, dtype=torch.int64)
    for kw in ({"k": 0}, {"k": 5, "shortlist": 4}, {"k": 1, "shortlist": _lib.TOPK_MAX + 1}):
        with pytest.raises(ValueError, match="shortlist"):
            index.search_moments(ids, ids, ids, window=(1, 2), **kw)
    with pytest.raises(ValueError, match="keep_frames=True"):
        index.search_moments(ids, ids, ids, k=2, window=(1, 2))
    assert index._wnorm is None and VideoIndex(_fake_model(True), keep_frames=True)._wnorm is None


def test_eval_localization_refuses_inconsistent_arguments():
    model = _fake_model()
    index = VideoIndex(model, capacity=4, keep_frames=True)
    with pytest.raises(ValueError, match="another model"):
        uev.eval_localization(_fake_model(), index, [], [0], [0], [1], (1, 2), device="cpu")
    with pytest.raises(ValueError, match="gt_start"):
        uev.eval_localization(model, index, [], [0, 0], [0], [1, 1], (1, 2), device="cpu")
    with pytest.raises(ValueError, match="targets must lie"):
        uev.eval_localization(model, index, [], [0], [0], [1], (1, 2), device="cpu")      # an empty index has no row 0
