"""Video-to-video alignment: the kernel (csrc/valign.hip: univl_video_align), ops.video_align, VideoIndex.align_videos /
transfer_labels and eval.eval_label_transfer.

A  fp64 parity on time-warped noisy copies of one drifting sequence (tests/video_align_ref.py), F in {1, 2, 31, 32, 33, 65, 128}, both
   modes, tau in {0, 0.5, 1}, Ta != Tb through a prefix mask, holes, a masked first frame, a single valid frame, no valid frame:
   "nothing to align" exactly; every path monotone with legal moves between valid frames and the right end points; every match_score
   within the project's fp32 gate 2e-4 of the float64 e; the float64 objective of the path RETURNED within path_len x 2e-4 of the
   float64 optimum; score within path_len x 2e-4 of that objective.  No path position is compared under a tolerance;
B  exact inputs (entries in {0, +-1}, 4 or 16 non-zeros: every e a multiple of 1/16): all six outputs equal the reference programme
   element for element and bit for bit; the constructed ties, dense and across holes;
C  purity: a pair alone, moved within the launch, under another C, in deterministic mode -- all bit-identical; align(a, b) and
   align(b, a) have bit-equal scores; a video against itself at tau = 1, global, gives the diagonal;
D  rows out of range inside NaN-filled memory; every refusal;
E  through the model in fp32 and bf16: index.align_videos on rows added through add(), against the float64 reference fed
   index._frames; eval_label_transfer on ground truth planted from the kernel's own match.

The worst errors of A on an MI355X are in profiles/video_align.txt."""
import ctypes as C

import numpy as np
import pytest
import torch

from make_golden import case_config

import video_align_ref as VR
from retrieval_cases import batches as _batches, deterministic_models  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import univl_amd
    from univl_amd import _lib, ops
    from univl_amd import eval as uev
    from test_model_gpu import build

DEV = "cuda"
H = 768
TOL = 2e-4                       # tests/test_moment_gpu.py: the project's fp32 score gate
NEG_INF = float("-inf")


def _t(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _host(out):
    score, path_len, path_a, path_b, match, match_score = (t.cpu().numpy() for t in out)
    return score, path_len.astype(np.int64), path_a.astype(np.int64), path_b.astype(np.int64), match.astype(np.int64), match_score


def _align(frames, mask, ref, rows, tau, local):
    return _host(ops.video_align(_t(frames, torch.float32), _t(mask, torch.int64), _t(ref, torch.int32), _t(rows, torch.int32), tau, local))


def _check_empty(got, where):
    """(-inf, 0, -1, -1, -2, -inf) where `where` [P, C] says there is nothing to align, finite scores elsewhere, no NaN anywhere."""
    score, path_len, path_a, path_b, match, match_score = got
    assert np.all(score[where] == NEG_INF) and np.all(path_len[where] == 0)
    assert np.all(path_a[where] == -1) and np.all(path_b[where] == -1)
    assert np.all(match[where] == -2) and np.all(match_score[where] == NEG_INF)
    assert np.all(np.isfinite(score[~where])) and np.all(path_len[~where] >= 1)
    assert not np.any(np.isnan(score)) and not np.any(np.isnan(match_score))


def _assert_equal(got, want, what):
    for k, (g, w) in enumerate(zip(got, want)):
        if g.dtype.kind == "f":
            assert np.array_equal(g.view(np.int32), w.astype(np.float32).view(np.int32)), (what, k)          # exact, so bit-equal
        else:
            assert np.array_equal(g, w), (what, k)


# ------------------------------------------------------------------------------------------------ A: fp64 parity
@pytest.mark.parametrize("F", VR.PARITY_F)
def test_kernel_against_fp64(F):
    """fp32 against the float64 programme.  The largest errors are printed (over all shapes: profiles/video_align.txt)."""
    frames, mask, ref, rows = VR.parity_case(F)
    d_frames, d_mask, d_ref, d_rows = _t(frames), _t(mask), _t(ref), _t(rows)
    has = mask.any(1)
    empty = ~(has[ref][:, None] & has[rows])
    assert empty.any() and (~empty).sum() >= 6
    worst = np.zeros(3)
    for local in (0, 1):
        for tau in VR.PARITY_TAUS:
            got = _host(ops.video_align(d_frames, d_mask, d_ref, d_rows, tau, bool(local)))
            _check_empty(got, empty)                                      # "nothing to align" agrees exactly
            for p, c in zip(*np.nonzero(~empty)):
                E0, fa, gb = VR.parity_scores(F, int(ref[p]), int(rows[p, c]))
                worst = np.maximum(worst, VR.check_pair(got, p, c, E0 - tau, fa, gb, F, local, TOL))
    print("F=%d: max match_score error %.3e, max objective gap per cell %.3e, max score error per cell %.3e" % (F, *worst))


# ------------------------------------------------------------------------------------------------ B: exact inputs
@pytest.mark.parametrize("F", VR.EXACT_F)
def test_exact_inputs_bit_for_bit(F):
    frames, mask, ref, rows = VR.exact_case(F)
    dev = _t(frames), _t(mask), _t(ref), _t(rows)
    for tau in VR.EXACT_TAUS:
        for local in (0, 1):
            _assert_equal(_host(ops.video_align(*dev, tau, bool(local))), VR.exact_reference(F, tau, local), (F, tau, local))


@pytest.mark.parametrize("name,Cm,tau,local,want", VR.TIES, ids=[t[0] for t in VR.TIES])
def test_constructed_ties(name, Cm, tau, local, want):
    Cm = np.asarray(Cm)
    Ta, Tb = Cm.shape
    for F, va, vb in ((None, None, None), (9, np.arange(Ta) * 2 + 1, np.arange(Tb) * 2)):     # dense; across holes
        frames, mask = VR.from_overlaps(Cm, F, va, vb)
        ref, rows = np.array([0], dtype=np.int32), np.array([[1]], dtype=np.int32)
        got = _align(frames, mask, ref, rows, tau, bool(local))
        _assert_equal(got, VR.align(frames, mask, ref, rows, tau, local, dtype=np.float32), name)
        fa, gb = np.nonzero(mask[0])[0], np.nonzero(mask[1])[0]
        assert got[1][0, 0] == len(want)
        assert got[2][0, 0, :len(want)].tolist() == [int(fa[i]) for i, _ in want], name
        assert got[3][0, 0, :len(want)].tolist() == [int(gb[j]) for _, j in want], name


# ------------------------------------------------------------------------------------------------ C: purity
def test_purity_position_company_candidates_and_deterministic_mode():
    F = 65
    frames, mask, _, _ = VR.parity_case(F)
    rng = np.random.RandomState(41)
    ref = np.array([0, 2, 1, 0], dtype=np.int32)
    rows = rng.randint(0, 4, size=(4, 5)).astype(np.int32)
    d_frames, d_mask, d_ref, d_rows = _t(frames), _t(mask), _t(ref), _t(rows)
    was = univl_amd.deterministic()
    try:
        for tau, local in ((1.0, False), (0.5, True)):
            run = lambda r, c: ops.video_align(d_frames, d_mask, r, c, tau, local)
            univl_amd.set_deterministic(False)
            base = run(d_ref, d_rows)
            univl_amd.set_deterministic(True)
            det = run(d_ref, d_rows)
            univl_amd.set_deterministic(False)
            for x, y in zip(base, det):
                assert torch.equal(x, y)
            for p, c in ((0, 0), (1, 3), (3, 4)):                         # a pair alone
                alone = run(d_ref[p:p + 1].contiguous(), d_rows[p:p + 1, c:c + 1].contiguous())
                for x, y in zip(base, alone):
                    assert torch.equal(x[p, c], y[0, 0])
            moved = run(d_ref.flip(0).contiguous(), d_rows.flip(0).roll(2, 1).contiguous())
            for x, y in zip(base, moved):
                assert torch.equal(x.flip(0).roll(2, 1), y)
            fewer = run(d_ref, d_rows[:, 1:3].contiguous())              # another C
            for x, y in zip(base, fewer):
                assert torch.equal(x[:, 1:3], y)
    finally:
        univl_amd.set_deterministic(was)


@pytest.mark.parametrize("F", [33, 128])
def test_symmetry_and_a_video_against_itself(F):
    frames, mask, _, _ = VR.parity_case(F)
    d_frames, d_mask = _t(frames), _t(mask)
    a = torch.tensor([0, 0, 1, 2], dtype=torch.int32, device=DEV)
    b = torch.tensor([1, 2, 2, 3], dtype=torch.int32, device=DEV)
    for tau, local in ((1.0, False), (0.0, False), (0.5, True)):
        ab = ops.video_align(d_frames, d_mask, a, b.view(4, 1).contiguous(), tau, local)
        ba = ops.video_align(d_frames, d_mask, b, a.view(4, 1).contiguous(), tau, local)
        assert torch.equal(ab[0].view(torch.int32), ba[0].view(torch.int32))                  # bit-equal scores
    rows = torch.arange(4, dtype=torch.int32, device=DEV)
    score, path_len, path_a, path_b, match, match_score = _host(ops.video_align(d_frames, d_mask, rows, rows.view(4, 1).contiguous(), 1.0, False))
    for v in range(4):
        vf = np.nonzero(mask[v])[0]
        assert path_len[v, 0] == len(vf) and np.array_equal(path_a[v, 0, :len(vf)], vf) and np.array_equal(path_b[v, 0, :len(vf)], vf)
        assert np.array_equal(match[v, 0][vf], vf) and np.all(np.abs(match_score[v, 0][vf]) <= TOL) and abs(score[v, 0]) <= len(vf) * TOL


# ------------------------------------------------------------------------------------------------ D: poison and refusals
def test_rows_outside_the_gallery_inside_poisoned_memory():
    F, N = 33, 4
    frames, mask, _, _ = VR.parity_case(F)
    frames, mask = frames[:N], mask[:N]
    big = torch.full((N + 2, F, H), float("nan"), device=DEV)             # a read outside [0, N) would poison the result
    big[1:N + 1] = torch.from_numpy(frames).to(DEV)
    bigmask = torch.ones(N + 2, F, dtype=torch.int64, device=DEV)
    bigmask[1:N + 1] = torch.from_numpy(mask).to(DEV)
    d_frames, d_mask = big[1:N + 1], bigmask[1:N + 1]
    ref = np.array([0, -1, N, 2, 2 ** 31 - 1, 1], dtype=np.int32)
    one = np.array([1, -1, N, 2, -2 ** 31, 0], dtype=np.int32)
    rows = np.stack([one, one, one, np.roll(one, 2), one, one])
    for tau, local in ((1.0, 0), (0.5, 1)):
        got = _host(ops.video_align(d_frames, d_mask, _t(ref), _t(rows), tau, bool(local)))
        out = ((ref < 0) | (ref >= N))[:, None] | (rows < 0) | (rows >= N)
        _check_empty(got, out)
        assert (~out).sum() == 9
        for p, c in zip(*np.nonzero(~out)):
            E, fa, gb = VR.cell_scores(frames[ref[p]], mask[ref[p]], frames[rows[p, c]], mask[rows[p, c]], tau)
            VR.check_pair(got, p, c, E, fa, gb, F, local, TOL)


def _desc(frames, mask, ref, rows, out, F=None, Hh=H, tau=1.0, local=0):
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    d = _lib.VideoAlign()
    d.frames, d.ld_row, d.mask = p(frames), frames.stride(0), p(mask)
    d.N, d.F, d.H, d.local = frames.shape[0], frames.shape[1] if F is None else F, Hh, local
    d.ref, d.rows, d.P, d.C, d.tau = p(ref), p(rows), rows.shape[0], rows.shape[1], tau
    d.score, d.path_len, d.path_a, d.path_b, d.match, d.match_score = (p(t) for t in out)
    return d


def test_every_bad_argument_is_refused_with_a_message():
    L = _lib.lib()
    F = 8
    inf, nan = float("inf"), float("nan")
    frames, mask = torch.zeros(3, F, H, device=DEV), torch.ones(3, F, dtype=torch.int64, device=DEV)
    big = torch.zeros(3, 129, H, device=DEV)                              # room for the F = 129 descriptor: refused, but nothing dangles
    ref, rows = torch.zeros(4, dtype=torch.int32, device=DEV), torch.zeros(4, 2, dtype=torch.int32, device=DEV)
    out = (torch.zeros(4, 2, device=DEV), torch.zeros(4, 2, dtype=torch.int32, device=DEV), torch.zeros(4, 2, 258, dtype=torch.int32, device=DEV),
           torch.zeros(4, 2, 258, dtype=torch.int32, device=DEV), torch.zeros(4, 2, 129, dtype=torch.int32, device=DEV),
           torch.zeros(4, 2, 129, device=DEV))
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    good = lambda **kw: _desc(kw.pop("frames", frames), mask, ref, rows, out, **kw)
    fn, who = L.univl_video_align, b"univl_video_align"
    assert fn(C.byref(good()), stream) == 0 and fn(C.byref(good(local=1, tau=-3e38)), stream) == 0 and fn(C.byref(good(tau=3e38)), stream) == 0
    # case -> (descriptor, status, words only that case's message holds)
    bad = {"F = 129": (good(frames=big), -1, b"F=129"), "F = 0": (good(F=0), -1, b"F=0"), "H != 768": (good(Hh=512), -1, b"H=512"),
           "local = 2": (good(local=2), -1, b"local=2"), "local < 0": (good(local=-1), -1, b"local=-1"),
           "tau NaN": (good(tau=nan), -1, b"tau="), "tau +inf": (good(tau=inf), -1, b"tau=inf"), "tau -inf": (good(tau=-inf), -1, b"tau=-inf")}
    for name in ("ref", "rows", "score", "path_len", "path_a", "path_b", "match", "match_score"):
        d = good()
        setattr(d, name, None)
        bad["null " + name] = (d, -1, b"(ref, rows")
    for name in ("frames", "mask"):
        d = good()
        setattr(d, name, None)
        bad["null " + name] = (d, -1, b"(frames, mask)")
    d = good(); d.N = 0; bad["N < 1"] = (d, -1, b"N=0")
    d = good(); d.P = 0; bad["P < 1"] = (d, -1, b"P=0")
    d = good(); d.C = 0; bad["C < 1"] = (d, -1, b"C=0")
    d = good(); d.P, d.C = 2 ** 16, 2 ** 15; bad["P * C too large"] = (d, -1, b"P=65536 C=32768")
    d = good(); d.ld_row = F * H - 4; bad["ld_row < F * 768"] = (d, -1, b"ld_row=6140")
    d = good(); d.frames = C.c_void_p(frames.data_ptr() + 4); bad["misaligned frames"] = (d, -2, b"rows of frames")
    d = good(); d.ld_row = F * H + 2; bad["misaligned gallery rows"] = (d, -2, b"rows of frames")
    for name, (d, status, word) in bad.items():
        assert fn(C.byref(good()), stream) == 0                           # a good call in between: no message is left over
        rc = fn(C.byref(d), stream)
        assert rc == status, (name, rc)                                   # UNIVL_EINVAL / UNIVL_EALIGN
        msg = L.univl_last_error()
        assert who in msg and word in msg, (name, msg)
    assert fn(None, stream) == -1
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="tau="):
        ops.video_align(frames, mask, ref, rows, nan)
    with pytest.raises(RuntimeError, match="local=2"):
        ops.video_align(frames, mask, ref, rows, 1.0, 2)
    with pytest.raises(RuntimeError, match="H=512"):
        ops.video_align(torch.zeros(3, F, 512, device=DEV), mask, ref, rows, 1.0)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.video_align(frames.cpu(), mask, ref, rows, 1.0)


def test_captured_in_a_graph():
    frames, mask, ref, rows = VR.parity_case(33)
    dev = _t(frames), _t(mask), _t(ref), _t(rows)
    want = ops.video_align(*dev, 0.5, True)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            got = ops.video_align(*dev, 0.5, True)
    g.replay()
    torch.cuda.synchronize()
    for x, y in zip(want, got):
        assert torch.equal(x, y)


# ------------------------------------------------------------------------------------------------ E: through the model
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_align_videos_through_the_model_and_label_transfer(dtype, deterministic_models):
    from univl_amd.retrieval import VideoIndex
    cfg, _, dseed = case_config("joint_small")
    model, _ = build(cfg, dtype)
    model.eval()
    bs = _batches(cfg, [3, 3], dseed)
    index = VideoIndex(model, keep_frames=True, capacity=4)               # grows once
    for b in bs:
        index.add(b["video"], b["video_mask"])
    n, F = 6, cfg.max_frames
    frames = index._frames[:n].cpu().numpy()
    mask = index._fmask[:n].cpu().numpy()
    ref = np.array([0, 3, 5], dtype=np.int32)
    rows = np.array([[1, 2, 0], [4, 5, -1], [0, 5, 2]], dtype=np.int32)
    has = mask.any(1)
    empty = (rows < 0) | ~has[ref][:, None] | ~has[np.maximum(rows, 0)]
    assert empty.sum() <= 3
    for tau, local in ((1.0, False), (0.9, True)):
        res = index.align_videos(ref, rows, tau, local) if local else index.align_videos(ref, rows)
        got = _host(res)
        _check_empty(got, empty)
        for p, c in zip(*np.nonzero(~empty)):
            E, fa, gb = VR.cell_scores(frames[ref[p]], mask[ref[p]], frames[rows[p, c]], mask[rows[p, c]], tau)
            VR.check_pair(got, p, c, E, fa, gb, F, int(local), TOL)
    with pytest.raises(ValueError, match="explicit tau"):
        index.align_videos(ref, rows, local=True)

    # labels planted from the kernel's own match: every annotated valid frame is right
    res = index.align_videos(ref, rows)
    labels = torch.arange(3 * F, dtype=torch.int32).reshape(3, F) % 7 - 1                      # -1 .. 5: background and labels
    pred = index.transfer_labels(labels, res)
    got_match = res.match.cpu().numpy()
    assert pred.is_cuda and np.array_equal(pred.cpu().numpy(), VR.transfer(labels.numpy(), got_match))
    gt = pred.cpu().numpy().copy()
    lv = (gt != -2).sum(-1)
    assert np.array_equal(lv[~empty], mask[rows[~empty]].sum(-1)) and np.all(lv[empty] == 0) and np.all(got_match[~empty][mask[rows[~empty]] != 0] >= 0)
    m = uev.eval_label_transfer(index, ref, labels, rows, gt)
    assert m["frame_accuracy"] == 1.0 and m["correct"].tolist() == m["annotated"].tolist() == lv.tolist()
    assert m["n_pairs"] == 9 and m["n_frames"] == int(lv.sum()) and m["n_empty"] == int(empty.sum())
    # one frame flipped, one not annotated, a masked frame annotated
    f0 = int(np.nonzero(mask[1])[0][0])
    gt[0, 0, f0] = 6 if gt[0, 0, f0] != 6 else 0
    f1 = int(np.nonzero(mask[2])[0][0])
    gt[0, 1, f1] = -2
    gt[1, 2, 0] = 3                                                       # the pair has nothing to align: never counted
    m = uev.eval_label_transfer(index, ref, labels, rows, gt)
    want = VR.frame_counts(pred.cpu().numpy(), gt)
    correct, annotated = lv.copy(), lv.copy()
    correct[0, 0] -= 1
    correct[0, 1] -= 1
    annotated[0, 1] -= 1
    assert m["correct"].tolist() == want["correct"].tolist() == correct.tolist()
    assert m["annotated"].tolist() == want["annotated"].tolist() == annotated.tolist()
    assert m["frame_accuracy"] == want["frame_accuracy"] == correct.sum() / annotated.sum()
    assert m["frame_accuracy_fg"] == want["frame_accuracy_fg"]
