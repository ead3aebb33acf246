"""Host side of frame-wise segmentation (no GPU): the entry point is declared, exported and bound and the descriptor mirrors the C
struct; the float64 suffix programme (tests/segment_ref.py, the reference of tests/test_segment_gpu.py) against the exhaustive
enumeration of all labellings -- the optimum is equal and the programme's labelling attains it -- at every small shape, masks with
holes and constructed ties among them; the consequences the contract states; the counts of eval_segmentation on hand-made labels; what
the fixed-seed inputs of the GPU tests hold; VideoIndex and eval_segmentation refuse bad arguments before any device work."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

from univl_amd import _lib, ops
from univl_amd import eval as uev
from univl_amd.retrieval import VideoIndex, check_segment_args

import moment_ref as R
import segment_ref as GR
from retrieval_cases import header_fields as _header_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "univl_hip.h")).read()
needs_lib = pytest.mark.skipif(not _lib.available(), reason="libunivl_hip.so is not built")
NEW = ("univl_frame_segment_sizeof", "univl_frame_segment")
NEG_INF = GR.NEG_INF


# ------------------------------------------------------------------------------------------------ binding
@needs_lib
def test_entry_point_is_declared_exported_and_bound_and_the_descriptor_mirrors_the_header():
    L = _lib.lib()
    declared = set(re.findall(r"\b(univl_[a-z0-9_]+)\s*\(", HEADER))
    for name in NEW:
        assert name in declared and name in _lib.EXPORTED and hasattr(L, name), name
    assert declared == set(_lib.EXPORTED)
    fn = L.univl_frame_segment
    assert fn.restype is C.c_int32 and list(fn.argtypes) == [C.c_void_p, C.c_void_p]
    assert list(_lib.FrameSegment._fields_) == _header_fields("UnivlFrameSegment")
    assert L.univl_frame_segment_sizeof() == C.sizeof(_lib.FrameSegment)
    assert _lib.FrameSegment not in _lib._STRUCTS and len(_lib._STRUCTS) == 12                # the numbered size tables stay as they are
    assert list(_lib.FrameSegment._fields_[:8]) == list(_lib.Moment._fields_[:8]) == _header_fields("UnivlMoment")[:8]  # one gallery side
    assert int(re.search(r"#define UNIVL_SEGMENT_K_MAX (\d+)", HEADER).group(1)) == _lib.SEGMENT_K_MAX == GR.K_MAX == 64
    assert callable(ops.frame_segment) and callable(VideoIndex.segment) and callable(VideoIndex.segment_vectors)
    assert callable(uev.eval_segmentation)


@needs_lib
def test_no_cpu_fallback_and_null_descriptor():
    x, m = torch.zeros(2, 4, 768), torch.ones(2, 4, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.frame_segment(torch.zeros(1, 2, 768), torch.ones(1, dtype=torch.int32), x, m, torch.zeros(1, 1, dtype=torch.int32), 0.5, normalize=False)
    L = _lib.lib()
    assert L.univl_frame_segment(None, None) == -1                        # UNIVL_EINVAL before any device call
    assert b"univl_frame_segment" in L.univl_last_error()


# ------------------------------------------------------------------------------------------------ the reference, by itself
def _masks(F):
    """Whole, a prefix, a hole, two holes, a masked first frame, a single frame."""
    out = [np.ones(F, dtype=np.int64)]
    for zero in ([F - 1], [F // 2], [1, F - 2], [0], list(range(1, F))):
        m = np.ones(F, dtype=np.int64)
        m[[z for z in zero if 0 <= z < F]] = 0
        out.append(m)
    return out


@pytest.mark.parametrize("F", [1, 2, 3, 4, 5, 6])
def test_the_programme_attains_the_enumerated_optimum(F):
    """T <= 6 valid frames, n <= 3 labels, lambda in {0, 0.5, 100}, b in {-inf, 0}: the optimum over all (n + 1)^T labellings equals the
    programme's total (to the rounding of two different float64 summation orders) and the labelling the programme returns attains it."""
    rng = np.random.RandomState(60 + F)
    frames = rng.standard_normal((F, R.H))
    q = rng.standard_normal((3, R.H))
    seen = one = 0
    for mask in _masks(F):
        for normalize in (True, False):
            for n in (1, 2, 3):
                E, vf = GR.frame_scores(q[:n], frames, mask, normalize)
                assert E.shape == (n, int(mask.sum())) and np.array_equal(vf, np.nonzero(mask)[0])
                for t, f in enumerate(vf):
                    assert abs(E[0, t] - R.window_score(q[0], frames, int(f), 1, normalize)) <= 1e-12        # the one-frame window's score
                if len(vf) == 0:
                    continue
                for lam in (0.0, 0.5, 100.0):
                    for b in (NEG_INF, 0.0):
                        y, sc, total, nseg = GR.programme(E, lam, b)
                        best, _ = GR.enumerate_labellings(E, lam, b)
                        Eb = GR.with_background(E, b)
                        tol = 1e-9 * max(1.0, abs(best))
                        assert abs(total - best) <= tol, (F, mask, n, lam, b, total, best)
                        assert abs(GR.objective(Eb, y, lam) - best) <= tol, (F, mask, n, lam, b, y)
                        assert np.all((0 <= y) & (y <= n)) and np.array_equal(sc, Eb[y, np.arange(len(y))])
                        assert nseg == GR.run_count(y, n)
                        if b == NEG_INF:
                            assert np.all(y < n)                              # no background label
                        if n == 1 and b == NEG_INF:
                            assert np.all(y == 0) and nseg == 1
                        if lam == 0.0:                                        # the per-frame arg-max (no ties in random floats)
                            assert np.array_equal(y, np.argmax(Eb, axis=0)) and total == GR.objective(Eb, y, 0.0)
                        live = Eb[np.isfinite(Eb[:, 0])]
                        if lam > float((live.max(0) - live.min(0)).sum()):    # more than any switch can gain: one label, the video's best
                            assert np.all(y == y[0]) and y[0] == int(np.argmax(Eb.sum(1)))
                            one += 1
                        seen += 1
    assert seen > 0 and one > 0


def test_exact_integer_scores_programme_and_enumeration_agree_exactly():
    """Small integers: both pieces are exact, so the totals are equal and the programme's labelling is one of the optimal ones."""
    rng = np.random.RandomState(61)
    for T in (1, 2, 3, 4, 5, 6):
        for n in (1, 2, 3):
            E = rng.randint(-3, 4, size=(n, T)).astype(np.float64)         # many ties
            for lam in (0.0, 1.0, 2.0, 100.0):
                for b in (NEG_INF, 0.0, 1.0):
                    y, _, total, _ = GR.programme(E, lam, b)
                    best, at = GR.enumerate_labellings(E, lam, b)
                    assert total == best and tuple(int(v) for v in y) in at, (T, n, lam, b)
                    if lam == 0.0:                                        # every frame gets a label of largest score, whatever the ties
                        Eb = GR.with_background(E, b)
                        assert np.array_equal(Eb[y, np.arange(T)], Eb.max(0))
                        assert y[0] == int(np.argmax(Eb[:, 0]))          # the first frame: the lowest among equals, the background last


@pytest.mark.parametrize("name,E,lam,b,want", GR.TIES, ids=[t[0] for t in GR.TIES])
def test_constructed_ties_resolve_as_the_contract_says(name, E, lam, b, want):
    E = np.asarray(E, dtype=np.float64)
    y, sc, total, nseg = GR.programme(E, lam, b)
    assert y.tolist() == want
    best, at = GR.enumerate_labellings(E, lam, b)
    assert total == best and tuple(want) in at
    # through the inputs the GPU test launches: the integers come back as the frame scores, with holes in the mask too
    for F, valid in ((None, None), (E.shape[1] + 3, np.arange(E.shape[1]) * 2)):
        frames, mask, q = GR.from_scores(E, F, valid)
        E2, vf = GR.frame_scores(q[0], frames[0], mask[0], False)
        assert np.array_equal(E2, E) and (valid is None or np.array_equal(vf, valid))
        label, score, tot, ns = GR.segment(q, [E.shape[0]], frames, mask, [[0]], lam, b, False)
        assert label[0, 0, vf].tolist() == [-1 if v == E.shape[0] else v for v in want] and tot[0, 0] == total and ns[0, 0] == nseg
        assert np.all(label[0, 0][mask[0] == 0] == -2) and np.all(score[0, 0][mask[0] == 0] == NEG_INF)


def test_a_switch_across_a_hole_costs_the_penalty_once():
    E = np.array([[9.0, 0.0], [0.0, 9.0]])
    frames, mask, q = GR.from_scores(E, 6, [1, 4])                        # frames 2 and 3 masked: the two valid frames are neighbours
    label, score, total, nseg = GR.segment(q, [2], frames, mask, [[0]], 3.0, NEG_INF, False)
    assert label[0, 0].tolist() == [-2, 0, -2, -2, 1, -2] and total[0, 0] == 9 + 9 - 3 and nseg[0, 0] == 2
    assert score[0, 0].tolist() == [NEG_INF, 9.0, NEG_INF, NEG_INF, 9.0, NEG_INF]


def test_segment_reports_the_empty_cases_and_never_touches_the_padding():
    rng = np.random.RandomState(62)
    frames = rng.standard_normal((3, 6, R.H))
    mask = np.ones((3, 6), dtype=np.int64)
    mask[1, 2:] = 0
    mask[2] = 0                                                           # row 2: no valid frame
    q = rng.standard_normal((4, 3, R.H))
    counts = np.array([3, 2, 0, 4])
    q[1, 2:] = np.nan
    rows = np.array([[0, 1], [1, -1], [0, 0], [0, 3]])
    label, score, total, nseg = GR.segment(q, counts, frames, mask, rows, 0.1, 0.0, True)
    assert np.all(label[0, 0] >= -1) and np.isfinite(total[0, 0]) and nseg[0, 0] >= 0
    assert np.all(label[0, 1, :2] >= -1) and np.all(label[0, 1, 2:] == -2) and np.all(score[0, 1, 2:] == NEG_INF)
    assert np.all(label[1, 0, :2] < 2) and np.isfinite(total[1, 0])       # the NaN slot is never read
    for i, c in ((1, 1), (2, 0), (2, 1), (3, 0), (3, 1)):                 # a row outside the gallery; counts 0 and K + 1
        assert np.all(label[i, c] == -2) and np.all(score[i, c] == NEG_INF) and total[i, c] == NEG_INF and nseg[i, c] == 0
    label, score, total, nseg = GR.segment(q[:1], counts[:1], frames, mask, np.array([[2]]), 0.1, 0.0, True)
    assert np.all(label == -2) and np.all(score == NEG_INF) and total[0, 0] == NEG_INF and nseg[0, 0] == 0       # nothing valid
    assert not np.any(np.isnan(score)) and not np.any(np.isnan(total))


def test_eval_counts_on_hand_made_labels():
    #                 found                          annotated
    label = np.array([[0, 0, 1, -1, -2, -2], [2, 2, 2, 2, 2, 2], [-2] * 6, [-1, -1, 0, 0, -1, 1]])
    gt = np.array([[0, 1, 1, -1, 0, -2], [2, -2, -1, 2, 0, 2], [0, 0, -1, -1, -2, -2], [-1, 0, 0, -2, -1, -1]])
    total, nseg = np.array([1.0, 2.0, NEG_INF, 0.5]), np.array([2, 1, 0, 2])
    m = GR.frame_counts(label, total, nseg, gt)
    # list 0: frames 0 .. 3 counted (frame 4 is masked in the video, frame 5 neither), right on 0, 2, 3.  list 1: frame 1 not annotated;
    #         right on 0, 3, 5 of 5.  list 2: nothing to label, nothing counted.  list 3: frame 3 not annotated; right on 0, 2, 4 of 5
    assert m["correct"].tolist() == [3, 3, 0, 3] and m["annotated"].tolist() == [4, 5, 0, 5]
    assert m["n_lists"] == 4 and m["n_frames"] == 14 and m["n_segments"] == 5 and m["n_empty"] == 1
    assert m["frame_accuracy"] == 9 / 14
    # foreground frames: list 0: 0, 1, 2 (right 0, 2); list 1: 0, 3, 4, 5 (right 0, 3, 5); list 3: 1, 2 (right 2)
    assert m["frame_accuracy_fg"] == 6 / 9
    assert m["correct"].dtype == m["annotated"].dtype == np.int64


# ------------------------------------------------------------------------------------------------ the inputs of the GPU tests
@pytest.mark.parametrize("F,K", GR.parity_shapes())
def test_parity_cases_hold_labelled_and_empty_pairs(F, K):
    frames, mask, q, counts, rows = GR.parity_case(F, K)
    assert q.shape == (5, K, R.H) and rows.shape == (5, 3) and counts.max() == K and counts.min() == 1
    assert all(np.all(np.isnan(q[i, counts[i]:])) and not np.any(np.isnan(q[i, :counts[i]])) for i in range(5))
    for normalize in (True, False):
        ref = GR.parity_reference(F, K, normalize)
        assert set(ref) == set(GR.PARITY_PARAMS) and len(ref) == 6
        for (lam, b), (label, score, total, nseg) in ref.items():
            ok = np.isfinite(total)
            assert ok.any() and (~ok).any() and not np.any(np.isnan(score)) and not np.any(np.isnan(total))
            for i, c in zip(*np.nonzero(ok)):
                valid = mask[rows[i, c]] != 0
                lab = label[i, c]
                assert np.all(lab[~valid] == -2) and np.all(lab[valid] >= (-1 if b > NEG_INF else 0)) and np.all(lab[valid] < counts[i])
                assert nseg[i, c] == GR.run_count(np.where(lab[valid] < 0, counts[i], lab[valid]), counts[i])
            assert np.all(label[~ok] == -2) and np.all(score[~ok] == NEG_INF) and np.all(nseg[~ok] == 0)


@pytest.mark.parametrize("F", GR.EXACT_F)
def test_exact_cases_are_exact_in_fp32_and_hold_every_kind_of_label(F):
    frames, mask, q, counts, rows = GR.exact_case(F)
    kinds = set()
    for (lam, b), (label, score, total, nseg) in GR.exact_reference(F).items():
        ok = np.isfinite(total)
        assert ok.all()                                                   # every row has a valid frame
        fin = np.isfinite(score)
        assert np.array_equal(score[fin].astype(np.float32).astype(np.float64), score[fin])                      # scores and totals survive fp32
        assert np.array_equal(total.astype(np.float32).astype(np.float64), total) and np.abs(total).max() < 2 ** 24
        assert not np.any(label[2:] == 1)                                 # label 1 repeats label 0 there: the lower one wins
        kinds |= {kind for kind, there in (("label", np.any(label >= 0)), ("background", np.any(label == -1)), ("masked", np.any(label == -2)))
                  if there}
        for i, c in zip(*np.nonzero(rows == 5)):                          # identical frames: one label, the video's best
            lab = label[i, c][mask[5] != 0]
            assert np.all(lab == lab[0]) and nseg[i, c] == (1 if lab[0] >= 0 else 0)
        if lam == 10 ** 7:
            for i, c in zip(*np.nonzero(ok)):
                lab = label[i, c][label[i, c] != -2]
                assert np.all(lab == lab[0])                              # never worth paying: one label per video
    assert kinds == {"label", "background", "masked"}


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
            index.segment_vectors(q, counts, rows, 0.5)
        with pytest.raises(ValueError, match="keep_frames=True"):
            index.segment(ids, ids, ids, counts, rows)
    index = _index_with_frames(6)
    with pytest.raises(ValueError, match="at most 128"):
        _index_with_frames(129).segment_vectors(q, counts, rows)
    with pytest.raises(ValueError, match="lists of 65 steps"):
        index.segment_vectors(torch.zeros(2, 65, 768), counts, rows)
    with pytest.raises(ValueError, match="lists of 65 steps"):
        index.segment(torch.zeros(2, 65, 8, dtype=torch.int64), ids, ids, counts, rows)
    with pytest.raises(ValueError, match="dimensions"):
        index.segment_vectors(torch.zeros(6, 768), counts, rows)
    for bad in (-0.5, float("nan"), float("inf"), 1e39, None, "1", True):
        with pytest.raises(ValueError, match="switch_penalty="):
            index.segment_vectors(q, counts, rows, bad)
        with pytest.raises(ValueError, match="switch_penalty="):
            index.segment(ids, ids, ids, counts, rows, bad)
    for bad in (float("nan"), float("inf"), 1e39, "0", False):
        with pytest.raises(ValueError, match="background="):
            index.segment_vectors(q, counts, rows, 0.5, bad)
        with pytest.raises(ValueError, match="background="):
            index.segment(ids, ids, ids, counts, rows, 0.5, background=bad)
    for who, ok in (("x", (0.0, None)), ("x", (1.5, float("-inf"))), ("x", (0, -1e39)), ("x", (2, 3))):
        check_segment_args(who, *ok)                                      # -1e39 is -inf in fp32: no background label
    assert index._wnorm is None


def test_eval_segmentation_refuses_inconsistent_arguments():
    model = _fake_model()
    index = VideoIndex(model, capacity=4, keep_frames=True)
    z = np.zeros((1, 6), dtype=np.int64)
    with pytest.raises(ValueError, match="another model"):
        uev.eval_segmentation(_fake_model(), index, [], [0], z, device="cpu")
    with pytest.raises(ValueError, match="switch_penalty="):
        uev.eval_segmentation(model, index, [], [0], z, switch_penalty=-1.0, device="cpu")
    with pytest.raises(ValueError, match="background="):
        uev.eval_segmentation(model, index, [], [0], z, background=float("nan"), device="cpu")
    with pytest.raises(ValueError, match="gt_labels"):
        uev.eval_segmentation(model, index, [], [0, 0], z, device="cpu")                           # one row of annotation for two lists
    with pytest.raises(ValueError, match="gt_labels"):
        uev.eval_segmentation(model, index, [], [0], z[0], device="cpu")                            # not [lists, frames]
    with pytest.raises(ValueError, match="targets must lie"):
        uev.eval_segmentation(model, index, [], [0], z, device="cpu")                               # an empty index has no row 0
    index = _index_with_frames(6)
    model = index.model
    with pytest.raises(ValueError, match="targets must lie"):
        uev.eval_segmentation(model, index, [], [2], z, device="cpu")
    with pytest.raises(ValueError, match="targets must lie"):
        uev.eval_segmentation(model, index, [], [0], z - 3, device="cpu")                           # a label below -2
    ids = torch.zeros(1, 8, dtype=torch.int64)
    with pytest.raises(ValueError, match="one count per list"):
        uev.eval_segmentation(model, index, [(ids, ids, ids, torch.ones(1))], [0], z, device="cpu") # texts without the label dimension
    ids = torch.zeros(2, 3, 8, dtype=torch.int64)
    with pytest.raises(ValueError, match="more lists than targets"):
        uev.eval_segmentation(model, index, [(ids, ids, ids, torch.ones(2))], [0], z, device="cpu")
    with pytest.raises(ValueError, match="0 lists for 1 targets"):
        uev.eval_segmentation(model, index, [], [0], z, device="cpu")
