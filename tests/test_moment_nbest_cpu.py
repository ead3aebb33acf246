"""Host side of n-best moment search (no GPU): the entry point is declared, exported and bound and the descriptor mirrors the C struct
while UnivlMoment and the numbered size tables stay as they were; the two float64 statements of the contract (tests/moment_nbest_ref.py:
the literal greedy and the sorted sweep) agree on every input of the GPU parity test and on small exhaustive cases with constructed
ties and holes; the consequences the header states hold for them; the R@n counting on planted windows; the ranking rule of
search_moments(per_video=); every ValueError of the Python surface that needs no device."""
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
import moment_nbest_ref as NR
from retrieval_cases import header_fields as _header_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "univl_hip.h")).read()
needs_lib = pytest.mark.skipif(not _lib.available(), reason="libunivl_hip.so is not built")
NEW = ("univl_moment_nbest_sizeof", "univl_moment_nbest")


# ------------------------------------------------------------------------------------------------ binding
@needs_lib
def test_entry_point_is_declared_exported_and_bound_and_the_descriptor_mirrors_the_header():
    L = _lib.lib()
    declared = set(re.findall(r"\b(univl_[a-z0-9_]+)\s*\(", HEADER))
    for name in NEW:
        assert name in declared and name in _lib.EXPORTED and hasattr(L, name), name
    assert declared == set(_lib.EXPORTED)
    fn = L.univl_moment_nbest
    assert fn.restype is C.c_int32 and list(fn.argtypes) == [C.c_void_p, C.c_void_p]
    assert list(_lib.MomentNbest._fields_) == _header_fields("UnivlMomentNbest")
    assert L.univl_moment_nbest_sizeof() == C.sizeof(_lib.MomentNbest)
    # UnivlMoment's gallery and query side, field for field; then M and the threshold; then the outputs
    assert list(_lib.MomentNbest._fields_[:15]) == list(_lib.Moment._fields_[:15]) == _header_fields("UnivlMoment")[:15]
    assert [f[0] for f in _lib.MomentNbest._fields_[15:]] == ["M", "iou_num", "iou_den", "reserved", "start", "length", "score"]
    assert int(re.search(r"#define UNIVL_MOMENT_NBEST_MAX (\d+)", HEADER).group(1)) == _lib.MOMENT_NBEST_MAX == NR.NBEST_MAX == 16
    assert callable(ops.moment_nbest)


@needs_lib
def test_univl_moment_and_the_numbered_tables_are_unchanged():
    L = _lib.lib()
    assert list(_lib.Moment._fields_) == _header_fields("UnivlMoment") and L.univl_moment_sizeof() == C.sizeof(_lib.Moment) == 112
    assert _lib.MomentNbest not in _lib._STRUCTS and len(_lib._STRUCTS) == 12
    assert [L.univl_abi_sizeof(k) for k in range(12)] == [C.sizeof(st) for st in _lib._STRUCTS]
    assert L.univl_abi_sizeof(12) == -1                                   # the table ends where it ended


@needs_lib
def test_no_cpu_fallback_and_null_descriptor():
    x, m = torch.zeros(2, 4, 768), torch.ones(2, 4, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.moment_nbest(torch.zeros(1, 768), x, m, torch.zeros(1, 1, dtype=torch.int32), 1, 2, 3, normalize=False)
    L = _lib.lib()
    assert L.univl_moment_nbest(None, None) == -1                         # UNIVL_EINVAL before any device call
    assert b"univl_moment_nbest" in L.univl_last_error()


# ------------------------------------------------------------------------------------------------ the two statements of the contract
def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _consequences(S, lmin, lmax, M, num, den, got):
    """What the header promises of any result, checked on the reference's own: check_nbest at gate 0, slot 0 is best_window, M = 1 and
    shorter M are prefixes, (1, 1) is the plain top-M, (0, 1) is pairwise disjoint."""
    start, length, score = got
    assert NR.check_nbest(start, length, score, S, lmin, lmax, num, den, 0.0) == 0.0
    s0, l0, sc0, _ = R.best_window(S, lmin, lmax)
    assert (start[0], length[0], score[0]) == (s0, l0, sc0)
    n = int((length > 0).sum())
    assert np.all(length[:n] > 0) and np.all(length[n:] == 0) and np.all(np.diff(score[:n]) <= 0)
    if num == den:
        assert _same(got, NR.top_plain(S, lmin, lmax, M))
    if num == 0:
        frames = [f for s, L in zip(start[:n], length[:n]) for f in range(s, s + L)]
        assert len(frames) == len(set(frames))


@pytest.mark.parametrize("F", R.PARITY_F)
def test_greedy_equals_sweep_on_the_inputs_of_the_gpu_parity_test(F):
    pairs = empties = 0
    for normalize in (True, False):
        for P in R.PARITY_P:
            _, _, q, rows = R.parity_case(F, P)
            scores = NR.parity_scores(F, P, normalize)
            for i, j in np.ndindex(*rows.shape):
                S = scores[int(rows[i, j])][i]
                for lmin, lmax in R.parity_windows(F):
                    for M, (num, den) in NR.CONFIGS:
                        a, b = NR.nbest_greedy(S, lmin, lmax, M, num, den), NR.nbest_sweep(S, lmin, lmax, M, num, den)
                        assert _same(a, b), (F, P, normalize, i, j, lmin, lmax, M, num, den)
                        if a[1][0] > 0:
                            _consequences(S, lmin, lmax, M, num, den, a)
                        pairs += 1
                        empties += int(a[1][-1] == 0)
    assert pairs > 0 and (empties > 0 or F == 1)


def _small_masks(F):
    out = [np.ones(F, dtype=np.int64)]
    for zero in ([F - 1], [F // 2], [1, F - 2], list(range(1, F)), list(range(F))):
        m = np.ones(F, dtype=np.int64)
        m[[z for z in zero if 0 <= z < F]] = 0
        out.append(m)
    return out


@pytest.mark.parametrize("F", [1, 2, 3, 4, 5, 6, 7])
def test_greedy_equals_sweep_exhaustively_on_small_integer_scores_with_ties_and_holes(F):
    """Every (lmin, lmax), every small mask, M in {1, 3, 16}, four thresholds; the scores are small integers (a frame value in
    {0, 1, 2}, use_mil, q = e_0), so that ties across starts and lengths are everywhere."""
    rng = np.random.RandomState(60 + F)
    q = np.zeros((1, R.H))
    q[0, 0] = 1.0
    ties = n = 0
    for trial in range(3):
        frames = np.zeros((F, R.H))
        frames[:, 0] = rng.randint(0, 3, size=F) if trial else 2.0        # trial 0: identical frames
        for mask in _small_masks(F):
            S = R.row_scores(q, frames, mask, False)[0][0]
            for lmin in range(1, F + 1):
                for lmax in range(lmin, F + 1):
                    for M in (1, 3, 16):
                        for num, den in NR.NMS_SMALL:
                            a, b = NR.nbest_greedy(S, lmin, lmax, M, num, den), NR.nbest_sweep(S, lmin, lmax, M, num, den)
                            assert _same(a, b), (F, trial, mask, lmin, lmax, M, num, den, a, b)
                            n += 1
                            if a[1][0] > 0:
                                _consequences(S, lmin, lmax, M, num, den, a)
                                k = int((a[1] > 0).sum())
                                ties += int(k > 1 and np.any(np.diff(a[2][:k]) == 0))
                            if M == 16:                                   # a prefix of a longer run: the slots do not depend on M
                                assert _same([x[:3] for x in a], NR.nbest_greedy(S, lmin, lmax, 3, num, den))
    assert n > 0 and (ties > 0 or F == 1)


def test_constructed_cases_by_hand():
    q = np.zeros((1, R.H))
    q[0, 0] = 1.0
    f = np.zeros((6, R.H))
    f[:, 0] = [1.0, 5.0, 2.0, 5.0, 5.0, 0.0]
    ones = np.ones(6, dtype=np.int64)
    S = R.row_scores(q, f, ones, False)[0][0]
    # lengths 1 .. 2, use_mil: (1, 1), (3, 1), (3, 2), (4, 1) all score 5 -- ORDER: lower start, then smaller length
    for solve in (NR.nbest_greedy, NR.nbest_sweep):
        s, L, sc = solve(S, 1, 2, 4, 1, 1)
        assert list(zip(s, L)) == [(1, 1), (3, 1), (3, 2), (4, 1)] and np.all(sc == 5.0)
        s, L, sc = solve(S, 1, 2, 4, 1, 2)                                # IoU((3, 2), (3, 1)) = 1 / 2 is NOT above 1 / 2: it stays
        assert list(zip(s, L)) == [(1, 1), (3, 1), (3, 2), (4, 1)]
        s, L, sc = solve(S, 1, 2, 4, 49, 100)                             # ... and just under one half it goes, with all it overlaps by half
        assert list(zip(s, L))[:3] == [(1, 1), (3, 1), (4, 1)]
        s, L, sc = solve(S, 1, 2, 6, 0, 1)                                # disjoint: one-frame windows in score order, then nothing else fits
        assert list(zip(s, L)) == [(1, 1), (3, 1), (4, 1), (2, 1), (0, 1), (5, 1)]
        s, L, sc = solve(S, 2, 2, 5, 0, 1)                                # disjoint pairs run out before M: (3, 2), (1, 2) -- then frames 0 and 5 alone
        assert list(zip(s, L)) == [(3, 2), (1, 2), (-1, 0), (-1, 0), (-1, 0)] and np.all(sc[2:] == NR.NEG_INF)
        hole = np.array([1, 1, 1, 0, 1, 1])
        Sh = R.row_scores(q, f, hole, False)[0][0]
        s, L, sc = solve(Sh, 2, 3, 16, 1, 1)                              # the hole: windows beside it exist, none across it
        got = sorted((a, b) for a, b in zip(s, L) if b > 0)
        assert got == [(0, 2), (0, 3), (1, 2), (4, 2)]
        assert solve(np.full((4, 4), NR.NEG_INF), 1, 4, 3, 1, 2)[1].tolist() == [0, 0, 0]       # no candidate at all
    assert NR.suppresses(2, 3, 2, 3, 1, 1) and not NR.suppresses(2, 3, 2, 2, 1, 1) and NR.suppresses(2, 3, 4, 4, 0, 1)
    assert not NR.suppresses(2, 3, 5, 4, 0, 1) and NR.inter_frames(2, 3, 4, 4) == 1
    for ps, pl in ((0, 1), (2, 3), (4, 3)):
        m = NR.suppress_mask(7, ps, pl, 1, 2)
        assert all(m[s, L - 1] == NR.suppresses(ps, pl, s, L, 1, 2) for s in range(7) for L in range(1, 8))


def test_exact_scores_are_fp32_values_of_the_integer_case():
    frames, mask, q, rows = NR.int_case(16, 316)
    for r in (0, 4, 5, 6):
        S = NR.exact_scores(q, frames[r], mask[r])
        S64 = R.row_scores(q, frames[r], mask[r], False)[0]
        ok = S > NR.NEG_INF
        assert np.array_equal(ok, S64 > NR.NEG_INF)
        assert np.array_equal(S[ok].astype(np.float32).astype(np.float64), S[ok]) and np.abs(S[ok] - S64[ok]).max() <= 2.0 ** -9
    S5 = NR.exact_scores(q, frames[5], mask[5])
    assert all(len(set(S5[i][S5[i] > NR.NEG_INF])) == 1 for i in range(5))             # identical frames: every window ties


# ------------------------------------------------------------------------------------------------ counting and ranking
def test_rn_counts_on_planted_windows():
    #                 slot 0    slot 1    slot 2          annotated
    start = np.array([[2, 8, 0], [0, 5, 9], [0, 4, -1], [-1, -1, -1], [0, 10, 20]])
    length = np.array([[4, 2, 1], [2, 2, 2], [3, 6, 0], [0, 0, 0], [10, 10, 10]])
    gt_start, gt_len = np.array([2, 5, 4, 3, 13]), np.array([4, 4, 10, 2, 10])
    m = NR.rn_counts(start, length, gt_start, gt_len)
    # text 0: slot 0 is the segment.  text 1: slot 1 (5, 2) in (5, 4): 2 / 4.  text 2: slot 1 (4, 6) in (4, 10): 6 / 10; slot 0 disjoint.
    # text 3: no window.  text 4: slot 1 (10, 10) against (13, 10): 7 / 13 = 0.538; slot 2 (20, 10): 3 / 17; slot 0: 0
    assert m["R1@0.3"] == m["R1@0.5"] == m["R1@0.7"] == 1 / 5 and m["n"] == 5 and m["n_empty"] == 1
    assert m["R3@0.3"] == 4 / 5 and m["R3@0.5"] == 4 / 5 and m["R3@0.7"] == 1 / 5
    assert m["mIoU"] == float(np.mean([1.0, 0.0, 0.0, 0.0, 0.0]))
    one = NR.rn_counts(start[:, :1], length[:, :1], gt_start, gt_len)
    assert one == R.iou_counts(start[:, 0], length[:, 0], gt_start, gt_len) and set(one) == {"mIoU", "R1@0.3", "R1@0.5", "R1@0.7", "n", "n_empty"}
    # thresholds hit exactly, in integers: 3 / 10, 5 / 10 and 7 / 10 in the second slot
    st, ln = np.array([[50, 0]] * 3), np.array([[1, 3], [1, 5], [1, 7]])
    m = NR.rn_counts(st, ln, np.zeros(3, dtype=np.int64), np.full(3, 10))
    assert (m["R2@0.3"], m["R2@0.5"], m["R2@0.7"]) == (3 / 3, 2 / 3, 1 / 3) and m["R1@0.3"] == 0.0


def test_rank_moments_nbest_orders_by_score_then_row_then_pick():
    idx = np.array([4, 2, -1, 7])
    score = np.array([[0.9, 0.5, NR.NEG_INF], [0.9, 0.9, 0.1], [NR.NEG_INF] * 3, [0.95, 0.5, 0.5]])
    v, m = NR.rank_moments_nbest(idx, score, 12)
    got = list(zip(idx[v].tolist(), m.tolist()))
    assert got == [(7, 0), (2, 0), (2, 1), (4, 0), (4, 1), (7, 1), (7, 2), (2, 2), (4, 2), (-1, 0), (-1, 1), (-1, 2)]
    # the same rule as retrieval._rank_rows on the flattened list: ids ascending, then a stable sort by score
    from univl_amd.retrieval import _rank_rows
    flat_idx = torch.from_numpy(np.repeat(idx, 3)[None, :].astype(np.int32))
    sc, order = _rank_rows(torch.from_numpy(score.reshape(1, -1).astype(np.float32)), flat_idx, 12)
    assert order[0].tolist() == (v * 3 + m).tolist()


# ------------------------------------------------------------------------------------------------ refusals before any device work
def _fake_model(use_mil=False):
    return types.SimpleNamespace(task_config=types.SimpleNamespace(use_mil=use_mil), flat=types.SimpleNamespace(device="cpu"), training=False,
                                 eval=lambda: None, train=lambda mode=True: None)


def _index_with_frames(F):
    index = VideoIndex(_fake_model(), capacity=4, keep_frames=True)
    index._frames, index._fmask, index._n = torch.zeros(4, F, 768), torch.ones(4, F, dtype=torch.int64), 2
    return index


BAD_NBEST = (0, 17, -1, 2.0, "3", True)
BAD_NMS = ((1.0, 2), (1, 2.0), (1, 0), (1, 1025), (-1, 2), (3, 2), (1,), (1, 2, 3), 1, "12", (True, 2), None)


def test_localize_refuses_bad_n_best_and_nms_before_any_device_work():
    index = _index_with_frames(6)
    q, rows = torch.zeros(2, 768), torch.zeros(2, 1, dtype=torch.int32)
    ids = torch.zeros(2, 8, dtype=torch.int64)
    for call in (lambda **kw: index.localize_vectors(q, rows, (1, 2), **kw), lambda **kw: index.localize(ids, ids, ids, rows, (1, 2), **kw)):
        for bad in BAD_NBEST:
            with pytest.raises(ValueError, match="n_best="):
                call(n_best=bad)
        for bad in BAD_NMS:
            with pytest.raises(ValueError, match="nms="):
                call(n_best=3, nms=bad)
        for nms in ((1, 2), (0, 1), [1, 2]):                              # nms given without n_best, the default's value included
            with pytest.raises(ValueError, match="without n_best"):
                call(nms=nms)
    with pytest.raises(ValueError, match="window="):                      # the window is still checked on the n-best path
        index.localize_vectors(q, rows, (0, 2), n_best=3)
    with pytest.raises(ValueError, match="keep_frames=True"):
        VideoIndex(_fake_model(), capacity=4).localize_vectors(q, rows, (1, 2), n_best=3)
    assert index._wnorm is None


def test_search_moments_refuses_bad_per_video_k_and_nms():
    plain = VideoIndex(_fake_model(), capacity=4)
    ids = torch.zeros(2, 8, dtype=torch.int64)
    for bad in (0, 17, -1, 2.5, "3"):
        with pytest.raises(ValueError, match="per_video="):
            plain.search_moments(ids, ids, ids, k=2, window=(1, 2), per_video=bad)
    for bad in BAD_NMS:
        with pytest.raises(ValueError, match="nms="):
            plain.search_moments(ids, ids, ids, k=2, window=(1, 2), per_video=3, nms=bad)
        with pytest.raises(ValueError, match="nms="):
            plain.search_moments(ids, ids, ids, k=2, window=(1, 2), nms=bad)
    for kw in ({"k": 0}, {"k": 13, "shortlist": 4}, {"k": 4, "shortlist": _lib.TOPK_MAX + 1}, {"k": 4, "shortlist": 0}):
        with pytest.raises(ValueError, match="shortlist"):
            plain.search_moments(ids, ids, ids, window=(1, 2), per_video=3, **kw)
    with pytest.raises(ValueError, match="keep_frames=True"):             # k = 12 = shortlist * per_video is in range
        plain.search_moments(ids, ids, ids, k=12, window=(1, 2), shortlist=4, per_video=3)
    with pytest.raises(ValueError, match="keep_frames=True"):             # per_video = 1: today's checks, today's message
        plain.search_moments(ids, ids, ids, k=2, window=(1, 2), per_video=1)
    with pytest.raises(ValueError, match="need 1 <= k <= shortlist <= 64"):
        plain.search_moments(ids, ids, ids, k=5, window=(1, 2), shortlist=4)


def test_eval_localization_refuses_bad_n_best_and_nms():
    model = _fake_model()
    index = VideoIndex(model, capacity=4, keep_frames=True)
    for bad in BAD_NBEST[:-1] + (None,):
        with pytest.raises(ValueError, match="n_best="):
            uev.eval_localization(model, index, [], [0], [0], [1], (1, 2), device="cpu", n_best=bad)
    for bad in BAD_NMS:
        with pytest.raises(ValueError, match="nms="):
            uev.eval_localization(model, index, [], [0], [0], [1], (1, 2), device="cpu", n_best=5, nms=bad)
    with pytest.raises(ValueError, match="targets must lie"):             # good arguments pass on to the checks of before
        uev.eval_localization(model, index, [], [0], [0], [1], (1, 2), device="cpu", n_best=5, nms=(7, 10))
    with pytest.raises(ValueError, match="targets must lie"):
        uev.eval_localization(model, index, [], [0], [0], [1], (1, 2), device="cpu", n_best=1)
