"""Host side of ordered step alignment (no GPU): the entry point is declared, exported and bound and the descriptor mirrors the C
struct; the float64 suffix programme (tests/step_align_ref.py, the reference of tests/test_step_align_gpu.py) equals the exhaustive
enumeration of all alignments -- alignment and total -- at every small shape and window, masks with holes and constructed ties among
them; the feasibility edges; the counts of eval_step_alignment on hand-made cases; what the fixed-seed inputs of the GPU tests hold;
VideoIndex and eval_step_alignment refuse bad arguments before any device work."""
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
import step_align_ref as SR
from retrieval_cases import header_fields as _header_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "univl_hip.h")).read()
needs_lib = pytest.mark.skipif(not _lib.available(), reason="libunivl_hip.so is not built")
NEW = ("univl_step_align_sizeof", "univl_step_align")


# ------------------------------------------------------------------------------------------------ binding
@needs_lib
def test_entry_point_is_declared_exported_and_bound_and_the_descriptor_mirrors_the_header():
    L = _lib.lib()
    declared = set(re.findall(r"\b(univl_[a-z0-9_]+)\s*\(", HEADER))
    for name in NEW:
        assert name in declared and name in _lib.EXPORTED and hasattr(L, name), name
    assert declared == set(_lib.EXPORTED)
    fn = L.univl_step_align
    assert fn.restype is C.c_int32 and list(fn.argtypes) == [C.c_void_p, C.c_void_p]
    assert list(_lib.StepAlign._fields_) == _header_fields("UnivlStepAlign")
    assert L.univl_step_align_sizeof() == C.sizeof(_lib.StepAlign)
    assert _lib.StepAlign not in _lib._STRUCTS and len(_lib._STRUCTS) == 12                   # the numbered size tables stay as they are
    assert list(_lib.StepAlign._fields_[:8]) == list(_lib.Moment._fields_[:8]) == _header_fields("UnivlMoment")[:8]     # one gallery side
    assert int(re.search(r"#define UNIVL_STEP_K_MAX (\d+)", HEADER).group(1)) == _lib.STEP_K_MAX == SR.K_MAX == 32
    assert callable(ops.step_align) and callable(VideoIndex.align_steps) and callable(VideoIndex.align_vectors)
    assert callable(uev.eval_step_alignment)


@needs_lib
def test_no_cpu_fallback_and_null_descriptor():
    x, m = torch.zeros(2, 4, 768), torch.ones(2, 4, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.step_align(torch.zeros(1, 2, 768), torch.ones(1, dtype=torch.int32), x, m, torch.zeros(1, 1, dtype=torch.int32), 1, 2, normalize=False)
    L = _lib.lib()
    assert L.univl_step_align(None, None) == -1                           # UNIVL_EINVAL before any device call
    assert b"univl_step_align" in L.univl_last_error()


# ------------------------------------------------------------------------------------------------ the reference, by itself
def _same(a, b):
    if a is None or b is None:
        return a is None and b is None
    return list(a[0]) == list(b[0]) and list(a[1]) == list(b[1]) and list(a[2]) == list(b[2]) and a[3] == b[3]


def _masks(F):
    """Whole, a prefix, a hole, two holes, a single frame, nothing."""
    out = [np.ones(F, dtype=np.int64)]
    for zero in ([F - 1], [F // 2], [1, F - 2], list(range(1, F)), list(range(F))):
        m = np.ones(F, dtype=np.int64)
        m[[z for z in zero if 0 <= z < F]] = 0
        out.append(m)
    return out


@pytest.mark.parametrize("F", [1, 2, 3, 4, 5, 6, 7])
def test_the_programme_equals_the_enumeration_at_every_window(F):
    rng = np.random.RandomState(40 + F)
    frames = rng.standard_normal((F, R.H))
    q = rng.standard_normal((3, R.H))
    feasible = infeasible = 0
    for mask in _masks(F):
        for normalize in (True, False):
            S, _ = R.row_scores(q, frames, mask, normalize)
            for n in (1, 2, 3):
                for lmin in range(1, F + 1):
                    for lmax in range(lmin, F + 1):
                        a, b = SR.programme(S[:n], lmin, lmax), SR.enumerate_alignments(S[:n], lmin, lmax)
                        assert _same(a, b), (F, mask, normalize, n, lmin, lmax, a, b)
                        if a is None:
                            infeasible += 1
                            continue
                        feasible += 1
                        assert SR.is_alignment(mask, a[0], a[1], lmin, lmax)
                        assert a[3] == SR.total_of(S[:n], a[0], a[1])
                        for k in range(n):
                            assert abs(a[2][k] - R.window_score(q[k], frames, a[0][k], a[1][k], normalize)) <= 1e-12
    assert feasible > 0 and infeasible > 0


def test_constructed_ties_pack_left_in_both_pieces():
    q = np.zeros((3, R.H))
    q[:, 0] = 1.0
    same = np.zeros((7, R.H))
    same[:, 0], same[:, 1] = 3.0, 4.0                                     # identical frames: every window scores 0.6, or 3 under use_mil
    ones = np.ones(7, dtype=np.int64)
    for normalize in (True, False):
        S, _ = R.row_scores(q, same, ones, normalize)
        for n in (1, 2, 3):
            for lmin, lmax in ((1, 1), (1, 7), (2, 2), (2, 3)):
                if n * lmin > 7:
                    continue
                a, b = SR.programme(S[:n], lmin, lmax), SR.enumerate_alignments(S[:n], lmin, lmax)
                assert _same(a, b)
                assert a[0] == [k * lmin for k in range(n)] and a[1] == [lmin] * n          # (0, lmin), (lmin, lmin), ...
    # equal totals reached with different windows: steps 0 and 1 alike, frames 1 and 3 alike -- the earlier frames win
    f = np.zeros((5, R.H))
    f[:, 0] = [1.0, 5.0, 2.0, 5.0, 5.0]
    S, _ = R.row_scores(q[:2], f, np.ones(5, dtype=np.int64), False)
    a, b = SR.programme(S, 1, 1), SR.enumerate_alignments(S, 1, 1)
    assert _same(a, b) and a[0] == [1, 3] and a[3] == 10.0                # (1, 4) and (3, 4) total 10 as well
    a, b = SR.programme(S, 1, 2), SR.enumerate_alignments(S, 1, 2)
    assert _same(a, b) and a[0] == [1, 3] and a[1] == [1, 1]              # (3, 2) scores 5 too: the shorter stays


def test_feasibility_edges():
    rng = np.random.RandomState(41)
    F = 7
    frames, q = rng.standard_normal((F, R.H)), rng.standard_normal((3, R.H))
    for solve in (SR.programme, SR.enumerate_alignments):
        for n, lmin in ((3, 2), (2, 3), (3, 1), (1, 6)):
            mask = np.zeros(F, dtype=np.int64)
            mask[:n * lmin] = 1                                           # exactly n * lmin valid frames: one alignment
            S, _ = R.row_scores(q[:n], frames, mask, True)
            got = solve(S, lmin, F)
            assert got[0] == [k * lmin for k in range(n)] and got[1] == [lmin] * n
            mask[n * lmin - 1] = 0                                        # one frame fewer: none
            S, _ = R.row_scores(q[:n], frames, mask, True)
            assert solve(S, lmin, F) is None
        mask = np.array([1, 1, 0, 1, 0, 0, 0])                            # valid frames 0, 1, 3: one window of two frames, not two
        S, _ = R.row_scores(q[:2], frames, mask, True)
        assert solve(S, 2, 2) is None and solve(S, 2, 7) is None
        for m4 in ([1, 1, 1, 0, 1, 0, 0], [1, 0, 1, 1, 1, 0, 0]):          # four valid frames, the count of 2 x 2, but laid out 3 + 1
            S4, _ = R.row_scores(q[:2], frames, np.array(m4), True)
            assert solve(S4, 2, 2) is None and solve(S4, 2, 7) is None and solve(S4[:1], 2, 2) is not None
        assert solve(S, 1, 2)[0][0] in (0, 1)                             # two steps of one frame do fit
        mask = np.array([0, 0, 0, 1, 0, 0, 0])                            # a single valid frame
        S, _ = R.row_scores(q[:2], frames, mask, True)
        assert solve(S[:1], 1, 1)[:2] == ([3], [1]) and solve(S, 1, 1) is None


def test_align_reports_the_empty_cases_and_never_touches_the_padding():
    rng = np.random.RandomState(42)
    frames = rng.standard_normal((2, 6, R.H))
    mask = np.ones((2, 6), dtype=np.int64)
    mask[1, 2:] = 0
    q = rng.standard_normal((4, 3, R.H))
    counts = np.array([3, 2, 0, 4])
    q[1, 2:] = np.nan
    rows = np.array([[0, 1], [1, -1], [0, 0], [0, 2]])
    for solve in (SR.programme, SR.enumerate_alignments):
        start, length, score, total = SR.align(q, counts, frames, mask, rows, 1, 2, True, solve)
        assert np.all(start[0, 0] >= 0) and np.isfinite(total[0, 0])
        assert np.all(start[0, 1] == -1) and np.all(length[0, 1] == 0) and np.all(score[0, 1] == SR.NEG_INF) and total[0, 1] == SR.NEG_INF
        assert start[1, 0, :2].tolist() == [0, 1] and start[1, 0, 2] == -1 and score[1, 0, 2] == SR.NEG_INF       # the padding slot
        assert total[1, 1] == SR.NEG_INF                                  # a row outside the gallery
        assert np.all(total[2:] == SR.NEG_INF) and np.all(start[2:] == -1)                                      # counts 0 and K + 1
        assert not np.any(np.isnan(score)) and not np.any(np.isnan(total))


def test_eval_counts_on_hand_made_cases():
    #                 found            annotated
    start = np.array([[0, 4, 9], [2, 5, -1], [-1, -1, -1], [0, 3, 6]])
    length = np.array([[4, 3, 2], [1, 4, 0], [0, 0, 0], [3, 3, 3]])
    counts, total = np.array([3, 2, 3, 3]), np.array([1.0, 2.0, SR.NEG_INF, 0.5])
    gt_start = np.array([[1, 6, 0], [2, 7, 4], [0, 1, 2], [0, 0, 7]])
    gt_len = np.array([[1, 1, 0], [1, 2, 3], [1, 0, 1], [3, 0, 1]])
    m = SR.step_counts(start, length, counts, total, gt_start, gt_len)
    # list 0: length 4 from 0, centre 0 + 3 // 2 = 1: hit (even length: the lower middle frame); length 3 from 4, centre 5, segment
    #         6 .. 6: miss; step 2 not annotated.  list 1: length 1 at 2: hit; length 4 from 5, centre 6, segment 7 .. 8: miss; slot 2
    #         past the count although annotated.  list 2: infeasible, two annotated steps missed.  list 3: hit, -, hit (centre 7)
    assert m["hits"].tolist() == [1, 1, 0, 2] and m["annotated"].tolist() == [2, 2, 2, 2]
    assert m["n_lists"] == 4 and m["n_steps"] == 8 and m["n_infeasible"] == 1 and m["recall"] == 4 / 8
    assert m["mIoU"] == float(np.mean(np.array([1 / 4, 1 / 3, 1 / 1, 2 / 4, 0.0, 0.0, 3 / 3, 1 / 3])))


# ------------------------------------------------------------------------------------------------ the inputs of the GPU tests
@pytest.mark.parametrize("F,K", SR.parity_shapes())
def test_parity_cases_hold_feasible_and_infeasible_pairs(F, K):
    frames, mask, q, counts, rows = SR.parity_case(F, K)
    assert q.shape == (5, K, R.H) and rows.shape == (5, 3) and counts.max() == K and counts.min() == 1
    assert all(np.all(np.isnan(q[i, counts[i]:])) and not np.any(np.isnan(q[i, :counts[i]])) for i in range(5))
    assert (1, 1) in SR.parity_windows(F, K) and ((2, 5) in SR.parity_windows(F, K)) == (F >= 5)
    for normalize in (True, False):
        for w, (start, length, score, total) in SR.parity_reference(F, K, normalize).items():
            ok = np.isfinite(total)
            assert ok.any() and (~ok).any(), (F, K, w)
            assert not np.any(np.isnan(score)) and not np.any(np.isnan(total))
            for i, c in zip(*np.nonzero(ok)):
                n = counts[i]
                assert SR.is_alignment(mask[rows[i, c]], start[i, c, :n], length[i, c, :n], w[0], w[1])
                assert np.all(start[i, c, n:] == -1) and np.all(length[i, c, n:] == 0) and np.all(score[i, c, n:] == SR.NEG_INF)
            assert np.all(start[~ok] == -1) and np.all(length[~ok] == 0) and np.all(score[~ok] == SR.NEG_INF)


@pytest.mark.parametrize("F", SR.EXACT_F)
def test_exact_cases_are_exact_in_fp32_and_hold_both_kinds_of_pair(F):
    frames, mask, q, counts, rows = SR.exact_case(F)
    for w, (start, length, score, total) in SR.exact_reference(F).items():
        ok = np.isfinite(total)
        assert ok.any() and (~ok).any()
        assert np.array_equal(score[ok].astype(np.float32).astype(np.float64), score[ok])                        # scores and totals survive fp32
        assert np.array_equal(total[ok].astype(np.float32).astype(np.float64), total[ok])
        for i, c in zip(*np.nonzero(ok & (rows == 5))):                    # identical frames: packed to the left
            n = counts[i]
            assert start[i, c, :n].tolist() == [k * w[0] for k in range(n)] and np.all(length[i, c, :n] == w[0])


# ------------------------------------------------------------------------------------------------ refusals before any device work
def _fake_model(use_mil=False):
    return types.SimpleNamespace(task_config=types.SimpleNamespace(use_mil=use_mil), flat=types.SimpleNamespace(device="cpu"), training=False,
                                 eval=lambda: None, train=lambda mode=True: None)


def _index_with_frames(F):
    index = VideoIndex(_fake_model(), capacity=4, keep_frames=True)
    index._frames, index._fmask, index._n = torch.zeros(4, F, 768), torch.ones(4, F, dtype=torch.int64), 2
    return index


def test_index_refusals_that_need_no_gpu():
    q, counts, rows = torch.zeros(2, 3, 768), torch.tensor([3, 1]), torch.zeros(2, 1, dtype=torch.int32)
    ids = torch.zeros(2, 3, 8, dtype=torch.int64)
    for index in (VideoIndex(_fake_model(), capacity=4), VideoIndex(_fake_model(), capacity=4, keep_frames=True)):      # no frames kept; none yet
        with pytest.raises(ValueError, match="keep_frames=True"):
            index.align_vectors(q, counts, rows, (1, 2))
        with pytest.raises(ValueError, match="keep_frames=True"):
            index.align_steps(ids, ids, ids, counts, rows)
    index = _index_with_frames(6)
    for window in ((0, 2), (3, 2), (1, 7)):
        with pytest.raises(ValueError, match="window="):
            index.align_vectors(q, counts, rows, window)
        with pytest.raises(ValueError, match="window="):
            index.align_steps(ids, ids, ids, counts, rows, window)
    with pytest.raises(ValueError, match="at most 128"):
        _index_with_frames(129).align_vectors(q, counts, rows, (1, 2))
    with pytest.raises(ValueError, match="lists of 33 steps"):
        index.align_vectors(torch.zeros(2, 33, 768), counts, rows, (1, 2))
    with pytest.raises(ValueError, match="lists of 33 steps"):
        index.align_steps(torch.zeros(2, 33, 8, dtype=torch.int64), ids, ids, counts, rows, (1, 2))
    with pytest.raises(ValueError, match="dimensions"):
        index.align_vectors(torch.zeros(6, 768), counts, rows, (1, 2))
    assert index._wnorm is None


def test_eval_step_alignment_refuses_inconsistent_arguments():
    model = _fake_model()
    index = VideoIndex(model, capacity=4, keep_frames=True)
    z = np.zeros((1, 3), dtype=np.int64)
    with pytest.raises(ValueError, match="another model"):
        uev.eval_step_alignment(_fake_model(), index, [], [0], z, z + 1, (1, 1), device="cpu")
    with pytest.raises(ValueError, match="gt_start"):
        uev.eval_step_alignment(model, index, [], [0, 0], z, z + 1, (1, 1), device="cpu")           # one row of annotation for two lists
    with pytest.raises(ValueError, match="gt_start"):
        uev.eval_step_alignment(model, index, [], [0], z, np.zeros((1, 2), dtype=np.int64), (1, 1), device="cpu")
    with pytest.raises(ValueError, match="gt_start"):
        uev.eval_step_alignment(model, index, [], [0], z[0], z[0], (1, 1), device="cpu")            # not [lists, steps]
    with pytest.raises(ValueError, match="targets must lie"):
        uev.eval_step_alignment(model, index, [], [0], z, z + 1, (1, 1), device="cpu")              # an empty index has no row 0
    index = _index_with_frames(6)
    model = index.model
    with pytest.raises(ValueError, match="targets must lie"):
        uev.eval_step_alignment(model, index, [], [2], z, z + 1, (1, 1), device="cpu")
    with pytest.raises(ValueError, match="targets must lie"):
        uev.eval_step_alignment(model, index, [], [0], z, z - 1, (1, 1), device="cpu")              # gt_len < 0
    ids = torch.zeros(1, 2, 8, dtype=torch.int64)
    with pytest.raises(ValueError, match="steps per list"):
        uev.eval_step_alignment(model, index, [(ids, ids, ids, torch.ones(1))], [0], z, z + 1, (1, 1), device="cpu")      # K = 2 against 3
    with pytest.raises(ValueError, match="0 lists for 1 targets"):
        uev.eval_step_alignment(model, index, [], [0], z, z + 1, (1, 1), device="cpu")
