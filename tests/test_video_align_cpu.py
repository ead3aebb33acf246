"""Host side of video-to-video alignment (no GPU): the entry point is declared, exported and bound and the descriptor mirrors the C
struct; the float64 programme (tests/video_align_ref.py, the reference of tests/test_video_align_gpu.py) against the exhaustive
enumeration of every monotone path -- the optimum is equal and the programme's path attains it -- at every Ta, Tb <= 5, both modes,
tau in {0, 0.5, 1}, masks with holes; on exact inputs the constructed ties resolve as the contract says and the reference alone
reproduces the enumeration; transfer_labels and eval_label_transfer's counts on hand-made results; every host refusal."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

from univl_amd import _lib, ops
from univl_amd import eval as uev
from univl_amd.retrieval import VideoAlignment, VideoIndex, check_valign_args

import video_align_ref as VR
from retrieval_cases import header_fields as _header_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "univl_hip.h")).read()
needs_lib = pytest.mark.skipif(not _lib.available(), reason="libunivl_hip.so is not built")
NEW = ("univl_video_align_sizeof", "univl_video_align")
NEG_INF = VR.NEG_INF


# ------------------------------------------------------------------------------------------------ binding
@needs_lib
def test_entry_point_is_declared_exported_and_bound_and_the_descriptor_mirrors_the_header():
    L = _lib.lib()
    declared = set(re.findall(r"\b(univl_[a-z0-9_]+)\s*\(", HEADER))
    for name in NEW:
        assert name in declared and name in _lib.EXPORTED and hasattr(L, name), name
    assert declared == set(_lib.EXPORTED)
    fn = L.univl_video_align
    assert fn.restype is C.c_int32 and list(fn.argtypes) == [C.c_void_p, C.c_void_p]
    assert list(_lib.VideoAlign._fields_) == _header_fields("UnivlVideoAlign")
    assert L.univl_video_align_sizeof() == C.sizeof(_lib.VideoAlign) == 120
    assert _lib.VideoAlign not in _lib._STRUCTS and len(_lib._STRUCTS) == 12                  # the numbered size tables stay as they are
    assert callable(ops.video_align) and callable(VideoIndex.align_videos) and callable(VideoIndex.transfer_labels)
    assert callable(uev.eval_label_transfer)
    assert os.path.exists(os.path.join(ROOT, "univl_amd", "csrc", "valign.hip"))


@needs_lib
def test_no_cpu_fallback_and_null_descriptor():
    x, m = torch.zeros(2, 4, 768), torch.ones(2, 4, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.video_align(x, m, torch.zeros(1, dtype=torch.int32), torch.zeros(1, 1, dtype=torch.int32), 1.0)
    L = _lib.lib()
    assert L.univl_video_align(None, None) == -1                          # UNIVL_EINVAL before any device call
    assert b"univl_video_align" in L.univl_last_error()


# ------------------------------------------------------------------------------------------------ the reference, by itself
def _small_pairs():
    """Every (Ta, Tb) with Ta, Tb <= 5 as a pair of 7-frame videos: dense prefixes, and the same frames behind holes and a masked
    first frame."""
    rng = np.random.RandomState(5)
    for Ta in range(1, 6):
        for Tb in range(1, 6):
            for holes in (False, True):
                frames = rng.standard_normal((2, 7, 16))
                frames[1, :Tb] += 0.8 * frames[0, np.minimum(np.arange(Tb), Ta - 1)]       # related videos: positive cosines occur
                mask = np.zeros((2, 7), dtype=np.int64)
                if holes:
                    mask[0, rng.choice(np.arange(1, 7), size=Ta, replace=False)] = 1
                    mask[1, rng.choice(7, size=Tb, replace=False)] = 1
                else:
                    mask[0, :Ta], mask[1, :Tb] = 1, 1
                yield Ta, Tb, frames, mask


def test_programme_against_the_enumeration_of_every_monotone_path():
    n = 0
    for Ta, Tb, frames, mask in _small_pairs():
        for tau in (0.0, 0.5, 1.0):
            E, fa, gb = VR.cell_scores(frames[0], mask[0], frames[1], mask[1], tau)
            assert E.shape == (Ta, Tb) and np.array_equal(fa, np.nonzero(mask[0])[0])
            for local in (0, 1):
                score, path = VR.programme(E, local)
                best = VR.enumerate_best(E, local)
                assert abs(float(score) - best) <= 1e-12, (Ta, Tb, tau, local)
                assert abs(VR.path_objective(E, path) - best) <= 1e-12, (Ta, Tb, tau, local)                    # the path attains it
                assert all((i1 - i0, j1 - j0) in VR.MOVES for (i0, j0), (i1, j1) in zip(path, path[1:]))
                if not local:
                    assert path[0] == (0, 0) and path[-1] == (Ta - 1, Tb - 1)
                n += 1
    assert n == 25 * 2 * 3 * 2


def test_symmetry_and_the_classic_dtw_reading():
    rng = np.random.RandomState(6)
    frames, mask = rng.standard_normal((2, 6, 16)), np.ones((2, 6), dtype=np.int64)
    mask[1, 4:] = 0
    E, _, _ = VR.cell_scores(frames[0], mask[0], frames[1], mask[1], 1.0)
    Et, _, _ = VR.cell_scores(frames[1], mask[1], frames[0], mask[0], 1.0)
    assert np.array_equal(E, Et.T)
    for local in (0, 1):
        assert VR.programme(E, local)[0] == VR.programme(Et, local)[0] or abs(VR.programme(E, local)[0] - VR.programme(Et, local)[0]) < 1e-12
    # tau = 1: -e is the cosine distance, the global score the negated DTW cost (min-plus over the same three moves)
    D = -E
    cost = np.full(D.shape, np.inf)
    for i in range(D.shape[0]):
        for j in range(D.shape[1]):
            prev = [cost[i - 1, j - 1] if i and j else np.inf, cost[i - 1, j] if i else np.inf, cost[i, j - 1] if j else np.inf]
            cost[i, j] = D[i, j] + (0.0 if i == j == 0 else min(prev))
    assert abs(cost[-1, -1] + VR.programme(E, 0)[0]) <= 1e-12
    # a video against itself: the diagonal
    Es, _, _ = VR.cell_scores(frames[0], mask[0], frames[0], mask[0], 1.0)
    assert VR.programme(Es, 0)[1] == [(i, i) for i in range(6)]


@pytest.mark.parametrize("name,Cm,tau,local,want", VR.TIES, ids=[t[0] for t in VR.TIES])
def test_constructed_ties_resolve_as_the_contract_says(name, Cm, tau, local, want):
    Cm = np.asarray(Cm)
    Ta, Tb = Cm.shape
    for F, va, vb in ((None, None, None), (9, np.arange(Ta) * 2 + 1, np.arange(Tb) * 2)):     # dense; across holes
        frames, mask = VR.from_overlaps(Cm, F, va, vb)
        E, fa, gb = VR.cell_scores(frames[0], mask[0], frames[1], mask[1], tau)
        assert np.array_equal(E, Cm / 16.0 - tau)                          # exact
        assert np.array_equal(E.astype(np.float32).astype(np.float64), E)
        score, path = VR.programme(E, local)
        assert path == want, name
        assert float(score) == VR.enumerate_best(E, local) == VR.path_objective(E, path)
        out = VR.align(frames, mask, [0], [[1]], tau, local)
        out32 = VR.align(frames, mask, [0], [[1]], tau, local, dtype=np.float32)
        for x, y in zip(out, out32):
            assert np.array_equal(x, y)
        assert out[2][0, 0, :len(want)].tolist() == [int(fa[i]) for i, _ in want]
        assert out[3][0, 0, :len(want)].tolist() == [int(gb[j]) for _, j in want]
    # match among equal e: the lowest i
    if Tb == 1 and not local:
        assert out[4][0, 0][gb[0]] == fa[0] and out[5][0, 0][gb[0]] == E[0, 0]


@pytest.mark.parametrize("F", VR.EXACT_F)
def test_exact_inputs_are_exact_and_the_reference_reproduces_the_enumeration(F):
    frames, mask, ref, rows = VR.exact_case(F)
    nz = np.count_nonzero(frames, axis=2)
    assert set(np.unique(nz)) <= {4, 16} and set(np.unique(frames)) <= {-1.0, 0.0, 1.0}
    assert mask[0].all() and mask[3].sum() == 1 and mask[1].sum() < F or F == 1
    for tau in VR.EXACT_TAUS:
        E, _, _ = VR.cell_scores(frames[0], mask[0], frames[2], mask[2], tau)
        assert np.array_equal(E * 16, np.round(E * 16))                   # multiples of 1/16
        for local in (0, 1):
            out64 = VR.align(frames, mask, ref, rows, tau, local)
            for x, y in zip(out64, VR.exact_reference(F, tau, local)):
                assert np.array_equal(x, y)                               # fp32 and fp64 programmes agree to the bit
            if F == 5:
                for p in range(2):
                    for c in range(3):
                        a, b = int(ref[p]), int(rows[p, c])
                        Ep, _, _ = VR.cell_scores(frames[a], mask[a], frames[b], mask[b], tau)
                        assert out64[0][p, c] == VR.enumerate_best(Ep, local)
    if F == 5:                                                            # ties do occur in these inputs
        Ep, _, _ = VR.cell_scores(frames[0], mask[0], frames[1], mask[1], 0.0)
        assert len(np.unique(Ep)) < Ep.size


def test_nothing_to_align_in_the_reference():
    frames, mask, ref, rows = VR.parity_case(2)
    out = VR.align(frames, mask, [0, 9, -1], [[1, 4, 5], [0, 0, 0], [0, 1, 2]], 0.5, 0)
    empty = np.array([[0, 1, 1], [1, 1, 1], [1, 1, 1]], dtype=bool)
    assert np.all(out[0][empty] == NEG_INF) and np.all(out[1][empty] == 0) and np.all(out[2][empty] == -1) and np.all(out[3][empty] == -1)
    assert np.all(out[4][empty] == -2) and np.all(out[5][empty] == NEG_INF) and np.isfinite(out[0][0, 0]) and out[1][0, 0] >= 1


# ------------------------------------------------------------------------------------------------ transfer_labels and the evaluator
def _hand_made():
    match = torch.tensor([[[0, 0, 2, -1, -2], [4, 3, -2, -2, -2]], [[1, 1, 1, 1, 1], [-2, -2, -2, -2, -2]]], dtype=torch.int32)
    ref_labels = torch.tensor([[5, 6, 7, 8, -1], [0, 3, 0, 0, 0]])
    P, C, F = match.shape
    z = torch.zeros(P, C)
    result = VideoAlignment(z, torch.tensor([[4, 2], [5, 0]], dtype=torch.int32), None, None, match, z)
    return ref_labels, result


def test_transfer_labels_on_a_hand_made_result():
    ref_labels, result = _hand_made()
    got = VideoIndex.transfer_labels(None, ref_labels, result)
    want = [[[5, 5, 7, -1, -2], [-1, 8, -2, -2, -2]], [[3, 3, 3, 3, 3], [-2, -2, -2, -2, -2]]]
    assert got.dtype == torch.int32 and got.tolist() == want
    assert np.array_equal(VR.transfer(ref_labels.numpy(), result.match.numpy()), np.array(want))
    with pytest.raises(ValueError, match="ref_labels"):
        VideoIndex.transfer_labels(None, ref_labels[:, :4], result)


def test_eval_label_transfer_counts_on_a_hand_made_result():
    ref_labels, result = _hand_made()
    seen = {}

    def align_videos(ref, rows, tau, local):
        seen.update(ref=ref, rows=rows, tau=tau, local=local)
        return result

    index = types.SimpleNamespace(align_videos=align_videos, transfer_labels=lambda labels, res: VideoIndex.transfer_labels(None, labels, res))
    #        predicted  [[5, 5, 7, -1, -2], [-1, 8, -2, -2, -2]], [[3, 3, 3, 3, 3], [-2 ..]]
    gt = np.array([[[5, 6, 7, -1, 5], [-2, 8, 8, -2, -2]], [[3, -1, -2, 3, 0], [0, 0, 0, 0, 0]]])
    m = uev.eval_label_transfer(index, [0, 1], ref_labels, [[1, 2], [0, 3]], gt, tau=0.75)
    assert seen["tau"] == 0.75 and seen["local"] is False
    assert m["correct"].tolist() == [[3, 1], [2, 0]] and m["annotated"].tolist() == [[4, 1], [4, 0]]
    assert m["correct"].dtype == m["annotated"].dtype == np.int64
    assert m["n_frames"] == 9 and m["frame_accuracy"] == 6 / 9 and m["n_pairs"] == 4 and m["n_empty"] == 1
    assert m["frame_accuracy_fg"] == 5 / 7                                # foreground: 3 + 1 + 3 annotated, 2 + 1 + 2 right
    want = VR.frame_counts(VR.transfer(ref_labels.numpy(), result.match.numpy()), gt)
    assert want["correct"].tolist() == m["correct"].tolist() and want["annotated"].tolist() == m["annotated"].tolist()
    assert want["frame_accuracy"] == m["frame_accuracy"] and want["frame_accuracy_fg"] == m["frame_accuracy_fg"]
    with pytest.raises(ValueError, match="gt_labels"):
        uev.eval_label_transfer(index, [0, 1], ref_labels, [[1, 2], [0, 3]], gt[:, :1])
    with pytest.raises(ValueError, match="no annotated valid frame"):
        uev.eval_label_transfer(index, [0, 1], ref_labels, [[1, 2], [0, 3]], np.full_like(gt, -2))


# ------------------------------------------------------------------------------------------------ refusals before any device work
def test_every_host_refusal():
    inf, nan = float("inf"), float("nan")
    check_valign_args("x", 1.0, False)
    check_valign_args("x", -3, True)
    check_valign_args("x", 0.25, 1)
    for tau in (nan, inf, -inf, 1e39, None, "1", True, 1j):
        with pytest.raises(ValueError, match="tau="):
            check_valign_args("x", tau, False)
    for local in (2, -1, None, "yes", 0.0):
        with pytest.raises(ValueError, match="local="):
            check_valign_args("x", 1.0, local)
    with pytest.raises(ValueError, match="explicit tau"):
        check_valign_args("x", 1.0, True, tau_given=False)

    index = VideoIndex.__new__(VideoIndex)
    index.keep_frames, index._frames = False, None
    with pytest.raises(ValueError, match="keep_frames=True"):
        index.align_videos([0], [[1]])
    with pytest.raises(ValueError, match="explicit tau"):                # no default is invented for local
        index.align_videos([0], [[1]], local=True)
    with pytest.raises(ValueError, match="tau="):
        index.align_videos([0], [[1]], tau=nan)
    with pytest.raises(ValueError, match="local="):
        index.align_videos([0], [[1]], 0.5, 2)
    index.keep_frames, index._frames, index._n = True, torch.zeros(2, 4, 768), 2
    index._fmask = torch.ones(2, 4, dtype=torch.int64)
    for ref, rows in (([[0]], [[1]]), ([0, 1], [[1]]), ([], []), ([0], [[]]), ([0], [[[1]]])):
        with pytest.raises(ValueError, match="ref .* and rows"):
            index.align_videos(ref, rows)
    with pytest.raises(RuntimeError, match="HIP device"):                 # past the refusals: the kernel or nothing
        index.align_videos([0], [1], 1.0, True)
