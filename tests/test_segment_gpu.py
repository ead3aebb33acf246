"""Frame-wise segmentation: the kernel (csrc/moment.hip: univl_frame_segment), ops.frame_segment, VideoIndex.segment / segment_vectors
and eval.eval_segmentation.

A  fp64 parity on LayerNorm-scale frames and unit label vectors (tests/segment_ref.py), both modes, F in {1, 15, 16, 17, 65, 128} x K in
   {1, 3, 64}, lambda in {0, 0.05, 1}, b in {-inf, 0.1}: "nothing to label" exactly; labels in [-1, n) on valid frames and -2 elsewhere;
   every score within the project's fp32 gate 2e-4 of that frame's fp64 score; the fp64 objective of the labelling RETURNED within
   2 T x 2e-4 of the fp64 optimum (each of T terms may be off by the gate once on the returned path and once on the optimal one); the
   total returned within T x 2e-4 of the returned labelling's fp64 objective; nseg the run count of the labels returned.  No label
   position is compared under a tolerance;
B  exact arithmetic (small integers, use_mil, integer lambda, integer or -inf b): labels, nseg, scores and totals equal element for
   element and bit for bit; the constructed ties;
C  masks: nothing valid, a single valid frame, a hole, a masked first frame; a switch across a hole costs lambda once;
D  rows outside the gallery, duplicates, counts outside [1, K], NaN around the gallery and in the padding of q;
E  purity: position, company, deterministic mode, the padding K; with one label, univl_moment_nbest's one-frame windows bit for bit;
   lambda = 0 against K one-label launches;
F  every argument the entry point refuses;
G  through the model: every frame's score against get_similarity_logits, eval_segmentation on planted ground truth, the lazily filled
   table across index growth.

Worst errors of A on an MI355X (profiles/segment.txt): score 2.1e-08 normalised and 4.8e-07 under use_mil (scores of magnitude
about 1); the fp64 objective of the labelling returned against the fp64 optimum 1.4e-14 (every labelling returned was an optimal one
of the fp64 scores; what is left is two float64 summation orders); the total against the returned labelling's objective, per frame,
1.1e-07 and 1.7e-06."""
import ctypes as C

import numpy as np
import pytest
import torch

from make_golden import case_config

import moment_ref as R
import segment_ref as GR
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


def _dev(frames, mask, q, counts, rows):
    return _t(frames, torch.float32), _t(mask, torch.int64), _t(q, torch.float32), _t(counts, torch.int32), _t(rows, torch.int32)


def _host(out):
    label, score, total, nseg = out
    return label.cpu().numpy().astype(np.int64), score.cpu().numpy(), total.cpu().numpy(), nseg.cpu().numpy().astype(np.int64)


def _segment(frames, mask, q, counts, rows, lam, b, normalize, wnorm=None):
    if normalize and wnorm is None:
        wnorm = ops.window_norms(frames, mask)
    return _host(ops.frame_segment(q, counts, frames, mask, rows, lam, None if b == NEG_INF else b, wnorm=wnorm, normalize=normalize))


def _check_empty(got, where):
    """-2 / -inf / -inf / 0 where `where` [Nl, C] says there is nothing to label, and a finite total elsewhere."""
    label, score, total, nseg = got
    assert np.all(label[where] == -2) and np.all(score[where] == NEG_INF) and np.all(total[where] == NEG_INF) and np.all(nseg[where] == 0)
    assert np.all(np.isfinite(total[~where])) and not np.any(np.isnan(score)) and not np.any(np.isnan(total))


def _check_pair(got, i, c, E, vf, n, lam, b, r_total, F):
    """The properties of section A for one labelled pair; E, vf: its float64 frame scores.  Returns (score error, objective gap, total
    error per frame)."""
    label, score, total, nseg = got
    T = len(vf)
    valid = np.zeros(F, dtype=bool)
    valid[vf] = True
    lab, sc = label[i, c], score[i, c]
    assert np.all(lab[~valid] == -2) and np.all(sc[~valid] == NEG_INF), (i, c)
    y = lab[vf]
    assert np.all((y >= (0 if b == NEG_INF else -1)) & (y < n)), (i, c, y)
    yy = np.where(y < 0, n, y)
    Eb = GR.with_background(E, b)
    err = float(np.abs(sc[vf].astype(np.float64) - Eb[yy, np.arange(T)]).max())
    obj = GR.objective(Eb, yy, lam)
    gap, terr = abs(obj - r_total), abs(float(total[i, c]) - obj)
    assert err <= TOL, (i, c, err)
    assert gap <= 2 * T * TOL, (i, c, gap)
    assert terr <= T * TOL, (i, c, terr)
    assert nseg[i, c] == GR.run_count(yy, n), (i, c)
    return err, gap, terr / T


# ------------------------------------------------------------------------------------------------ A: fp64 parity
@pytest.mark.parametrize("F,K", GR.parity_shapes())
def test_kernel_against_fp64(F, K):
    """fp32 against the float64 programme.  The largest errors are printed (over all shapes: profiles/segment.txt)."""
    frames, mask, q, counts, rows = GR.parity_case(F, K)
    dev = _dev(frames, mask, q, counts, rows)
    wnorm = ops.window_norms(dev[0], dev[1])
    for normalize in (True, False):
        worst = np.zeros(3)
        for (lam, b), (r_label, r_score, r_total, r_nseg) in GR.parity_reference(F, K, normalize).items():
            got = _segment(*dev, lam, b, normalize, wnorm)
            _check_empty(got, ~np.isfinite(r_total))                      # "nothing to label" agrees exactly
            for i, c in zip(*np.nonzero(np.isfinite(r_total))):
                E, vf = GR.parity_scores(F, K, int(i), int(rows[i, c]), normalize)
                worst = np.maximum(worst, _check_pair(got, i, c, E, vf, int(counts[i]), lam, b, r_total[i, c], F))
        print("F=%d K=%d %s: max score error %.3e, max objective gap %.3e, max total error per frame %.3e"
              % (F, K, "normalize" if normalize else "use_mil", worst[0], worst[1], worst[2]))


# ------------------------------------------------------------------------------------------------ B: exact arithmetic
def _assert_equal(got, want, what):
    label, score, total, nseg = got
    assert np.array_equal(label, want[0]), what
    assert np.array_equal(nseg, want[3]), what
    assert np.array_equal(score.view(np.int32), want[1].astype(np.float32).view(np.int32)), what                 # exact, so bit-equal
    assert np.array_equal(total, want[2].astype(np.float32)), what


@pytest.mark.parametrize("F", GR.EXACT_F)
def test_exact_integer_inputs_use_mil(F):
    frames, mask, q, counts, rows = GR.exact_case(F)
    dev = _dev(frames, mask, q, counts, rows)
    for (lam, b), want in GR.exact_reference(F).items():
        _assert_equal(_segment(*dev, lam, b, False), want, (F, lam, b))


@pytest.mark.parametrize("name,E,lam,b,want", GR.TIES, ids=[t[0] for t in GR.TIES])
def test_constructed_ties(name, E, lam, b, want):
    E = np.asarray(E, dtype=np.float64)
    n, T = E.shape
    for F, valid in ((None, None), (T + 3, np.arange(T) * 2)):            # every frame valid; holes between the frames
        frames, mask, q = GR.from_scores(E, F, valid)
        got = _segment(_t(frames), _t(mask), _t(q), _t(np.array([n], dtype=np.int32)), _t(np.zeros((1, 1), dtype=np.int32)), lam, b, False)
        _assert_equal(got, GR.segment(q, [n], frames, mask, [[0]], lam, b, False), name)
        assert got[0][0, 0][mask[0] != 0].tolist() == [-1 if v == n else v for v in want], name


# ------------------------------------------------------------------------------------------------ C: masks
def _mask_rows(F):
    mask = np.zeros((6, F), dtype=np.int64)                               # row 0: nothing valid
    mask[1, 7] = 1                                                        # a single valid frame, not the first
    mask[2, :] = 1
    mask[2, 9] = 0                                                        # a hole
    mask[3, 1:] = 1                                                       # a masked first frame
    mask[4, :] = 1
    mask[5, 2::3] = 1                                                     # more holes than frames
    return mask


def test_masks_exact():
    F, K = 20, 3
    rng = np.random.RandomState(31)
    frames = rng.randint(-8, 9, size=(6, F, H)).astype(np.float32)
    q = rng.randint(-8, 9, size=(3, K, H)).astype(np.float32)
    counts = np.array([1, 2, 3], dtype=np.int32)
    mask = _mask_rows(F)
    rows = np.tile(np.arange(6, dtype=np.int32), (3, 1))
    dev = _dev(frames, mask, q, counts, rows)
    for lam, b in ((0.0, NEG_INF), (500.0, NEG_INF), (500.0, 300.0), (10.0 ** 6, 0.0)):
        got = _segment(*dev, lam, b, False)
        _assert_equal(got, GR.segment(q, counts, frames, mask, rows, lam, b, False), (lam, b))
        label, score, total, nseg = got
        assert np.all(total[:, 0] == NEG_INF) and np.all(label[:, 0] == -2) and np.all(nseg[:, 0] == 0)          # nothing valid
        assert np.all(label[:, 1, 7] >= -1) and np.all(np.delete(label[:, 1], 7, axis=1) == -2)                  # a single valid frame
        assert np.array_equal(total[:, 1], score[:, 1, 7])
        assert np.all(label[:, 2, 9] == -2) and np.all(label[:, 3, 0] == -2) and np.all(label[:, 3, 1:] >= -1)
    # a switch across a hole costs the penalty once: frames 1 and 4 valid, the two between them masked
    E = np.array([[9.0, 0.0], [0.0, 9.0]])
    frames, mask, q = GR.from_scores(E, 6, [1, 4])
    label, score, total, nseg = _segment(_t(frames), _t(mask), _t(q), _t(np.array([2], dtype=np.int32)), _t(np.zeros((1, 1), dtype=np.int32)),
                                         3.0, NEG_INF, False)
    assert label[0, 0].tolist() == [-2, 0, -2, -2, 1, -2] and total[0, 0] == 9 + 9 - 3 and nseg[0, 0] == 2
    assert score[0, 0].tolist() == [NEG_INF, 9.0, NEG_INF, NEG_INF, 9.0, NEG_INF]


@pytest.mark.parametrize("normalize", [True, False], ids=["normalize", "use_mil"])
def test_masks_against_fp64(normalize):
    F, K = 20, 3
    rng = np.random.RandomState(32)
    frames = (rng.standard_normal((6, F, H)) * (28.0 / np.sqrt(H))).astype(np.float32)
    q = rng.standard_normal((3, K, H))
    q = (q / np.linalg.norm(q, axis=2, keepdims=True)).astype(np.float32)
    counts = np.array([1, 2, 3], dtype=np.int32)
    mask = _mask_rows(F)
    rows = np.tile(np.arange(6, dtype=np.int32), (3, 1))
    dev = _dev(frames, mask, q, counts, rows)
    for lam, b in ((0.0, NEG_INF), (0.02, 0.05), (1.0, 0.0)):
        lam, b = float(np.float32(lam)), float(np.float32(b))
        got = _segment(*dev, lam, b, normalize)
        r_total = GR.segment(q, counts, frames, mask, rows, lam, b, normalize)[2]
        _check_empty(got, ~np.isfinite(r_total))
        assert np.array_equal(np.isfinite(r_total), np.tile(np.arange(6) > 0, (3, 1)))
        for i, c in zip(*np.nonzero(np.isfinite(r_total))):
            E, vf = GR.frame_scores(q[i, :counts[i]], frames[c], mask[c], normalize)
            _check_pair(got, i, c, E, vf, int(counts[i]), lam, b, r_total[i, c], F)


# ------------------------------------------------------------------------------------------------ D: candidates, counts, poison
def test_rows_and_counts_outside_their_range_duplicates_and_poisoned_memory():
    F, N, K = 16, 4, 4
    rng = np.random.RandomState(33)
    frames = (rng.standard_normal((N, F, H)) * (28.0 / np.sqrt(H))).astype(np.float32)
    mask = np.ones((N, F), dtype=np.int64)
    counts = np.array([4, 2, 0, -1, K + 1, 1, 3], dtype=np.int32)
    q = rng.standard_normal((7, K, H)).astype(np.float32)
    q /= np.linalg.norm(q, axis=2, keepdims=True)
    for i, n in enumerate(counts):
        q[i, max(0, min(int(n), K)):] = np.nan                            # the rows past counts; all of them where the count is refused
    q[4] = np.nan
    # the gallery is the middle of a larger allocation whose other rows are NaN: a read outside [0, N) would poison the result
    big = torch.full((N + 2, F, H), float("nan"), device=DEV)
    big[1:N + 1] = torch.from_numpy(frames).to(DEV)
    bigmask = torch.ones(N + 2, F, dtype=torch.int64, device=DEV)
    d_frames, d_mask = big[1:N + 1], bigmask[1:N + 1]
    one = np.array([2, -1, N, 2, 2 ** 31 - 1, 0, -2 ** 31, 2], dtype=np.int32)
    rows = np.stack([one, np.roll(one, 3), one, one, one, np.array([-1, -1, 3, 3, N + 1, 1, 0, -7], dtype=np.int32), one])
    d_q, d_counts, d_rows = _t(q), _t(counts), _t(rows)
    lam, b = float(np.float32(0.03)), float(np.float32(0.02))
    for normalize in (True, False):
        wnorm = ops.window_norms(d_frames, d_mask) if normalize else None
        got = _host(ops.frame_segment(d_q, d_counts, d_frames, d_mask, d_rows, lam, b, wnorm=wnorm, normalize=normalize))
        label, score, total, nseg = got
        out = (rows < 0) | (rows >= N) | ((counts < 1) | (counts > K))[:, None]
        _check_empty(got, out)
        for i, a, c in ((0, 0, 3), (0, 0, 7), (5, 2, 3), (6, 0, 3)):                                              # duplicated candidates
            assert np.array_equal(label[i, a], label[i, c]) and np.array_equal(score[i, a], score[i, c])
            assert total[i, a] == total[i, c] and nseg[i, a] == nseg[i, c]
        r_total = GR.segment(np.nan_to_num(q), counts, frames, mask, rows, lam, b, normalize)[2]
        assert np.array_equal(np.isfinite(total), np.isfinite(r_total))
        for i, c in zip(*np.nonzero(~out)):
            E, vf = GR.frame_scores(q[i, :counts[i]], frames[rows[i, c]], mask[rows[i, c]], normalize)
            _check_pair(got, i, c, E, vf, int(counts[i]), lam, b, r_total[i, c], F)


# ------------------------------------------------------------------------------------------------ E: purity
def test_purity_position_company_deterministic_mode_and_padding():
    F, K = 65, 3
    frames, mask, q, counts, _ = GR.parity_case(F, K)
    rng = np.random.RandomState(34)
    rows = rng.randint(0, R.PARITY_ROWS, size=(5, 6)).astype(np.int32)
    rows[:, 0] = 0
    d_frames, d_mask, d_q, d_counts, d_rows = _dev(frames, mask, q, counts, rows)
    wnorm = ops.window_norms(d_frames, d_mask)
    wide = torch.full((5, 64, H), float("nan"), device=DEV)               # the same sets padded to K = 64
    wide[:, :K] = d_q
    was = univl_amd.deterministic()
    try:
        for normalize in (True, False):
            w = wnorm if normalize else None
            lam, b = (0.02, 0.03) if normalize else (0.5, 0.8)
            run = lambda qq, cc, rr: ops.frame_segment(qq, cc, d_frames, d_mask, rr, lam, b, wnorm=w, normalize=normalize)
            univl_amd.set_deterministic(False)
            base = run(d_q, d_counts, d_rows)
            univl_amd.set_deterministic(True)
            det = run(d_q, d_counts, d_rows)
            univl_amd.set_deterministic(False)
            for x, y in zip(base, det):
                assert torch.equal(x, y)
            assert bool((base[0] >= 0).any()) and bool((base[0] == -1).any()) and bool((base[3] > 1).any())      # labels, background, switches
            for i, j in ((0, 0), (2, 3), (4, 5)):                         # pair (i, j) alone
                alone = run(d_q[i:i + 1], d_counts[i:i + 1], d_rows[i:i + 1, j:j + 1].contiguous())
                for x, y in zip(base, alone):
                    assert torch.equal(x[i, j], y[0, 0])
            moved = run(d_q.flip(0).contiguous(), d_counts.flip(0).contiguous(), d_rows.flip(0).roll(2, 1).contiguous())
            for x, y in zip(base, moved):
                assert torch.equal(x.flip(0).roll(2, 1), y)
            padded = run(wide, d_counts, d_rows)
            for x, y in zip(base, padded):
                assert torch.equal(x, y)
    finally:
        univl_amd.set_deterministic(was)


@pytest.mark.parametrize("F", [1, 15, 16])
def test_one_label_is_the_one_frame_windows_of_moment_nbest_bit_for_bit(F):
    rng = np.random.RandomState(35 + F)
    frames = _t((rng.standard_normal((4, F, H)) * (28.0 / np.sqrt(H))).astype(np.float32))
    mask = torch.ones(4, F, dtype=torch.int64, device=DEV)
    q = rng.standard_normal((9, H))
    q = _t((q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32))
    rows = _t(rng.randint(0, 4, size=(9, 3)).astype(np.int32))
    ones = torch.ones(9, dtype=torch.int32, device=DEV)
    wnorm = ops.window_norms(frames, mask)
    for normalize in (True, False):
        w = wnorm if normalize else None
        start, length, want = ops.moment_nbest(q, frames, mask, rows, 1, 1, F, (1, 1), wnorm=w, normalize=normalize)      # every frame, best first
        assert bool((length == 1).all())
        by_frame = want.gather(2, start.long().argsort(dim=2))
        for lam in (0.0, 0.7):
            label, score, total, nseg = ops.frame_segment(q.view(9, 1, H), ones, frames, mask, rows, lam, None, wnorm=w, normalize=normalize)
            assert torch.equal(score.view(torch.int32), by_frame.view(torch.int32))                              # the bits, not only the values
            assert bool((label == 0).all()) and bool((nseg == 1).all())


def test_lambda_zero_is_the_arg_max_over_one_label_launches():
    F, K = 17, 3
    frames, mask, q, counts, rows = GR.parity_case(F, K)
    q = np.nan_to_num(q)                                                  # the one-label launches read every slot
    d_frames, d_mask, d_q, d_counts, d_rows = _dev(frames, mask, q, counts, rows)
    wnorm = ops.window_norms(d_frames, d_mask)
    ones = torch.ones(5, dtype=torch.int32, device=DEV)
    for normalize in (True, False):
        w = wnorm if normalize else None
        b = 0.03 if normalize else 0.8
        cand = torch.stack([ops.frame_segment(d_q[:, k:k + 1].contiguous(), ones, d_frames, d_mask, d_rows, 0.0, None, wnorm=w,
                                              normalize=normalize)[1] for k in range(K)])                         # [K, 5, 3, F]
        live = torch.arange(K, device=DEV)[:, None, None, None] < d_counts[None, :, None, None]
        cand = torch.where(live, cand, torch.full_like(cand, NEG_INF))
        for bg in (None, b):
            label, score, total, nseg = ops.frame_segment(d_q, d_counts, d_frames, d_mask, d_rows, 0.0, bg, wnorm=w, normalize=normalize)
            allc = cand if bg is None else torch.cat([cand, torch.where(cand[:1] > NEG_INF, torch.full_like(cand[:1], bg), cand[:1])])
            best, at = allc.max(0)
            assert torch.equal(score.view(torch.int32), best.view(torch.int32))
            at = torch.where(at == K, torch.full_like(at, -1), at)
            single = (allc == best[None]).sum(0) == 1                     # no two candidates alike: the label is decided
            valid = best > NEG_INF
            assert torch.equal(label[valid & single].long(), at[valid & single]) and bool((label[~valid] == -2).all())
            assert bool((valid & single).any())


# ------------------------------------------------------------------------------------------------ F: refusals
def _desc(frames, mask, wnorm, q, counts, rows, out, F=None, Hh=H, normalize=1, K=None, lam=0.5, b=0.0):
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    d = _lib.FrameSegment()
    d.frames, d.ld_row, d.mask, d.wnorm = p(frames), frames.stride(0), p(mask), p(wnorm)
    d.N, d.F, d.H, d.normalize = frames.shape[0], frames.shape[1] if F is None else F, Hh, normalize
    d.q, d.ldq, d.counts, d.rows = p(q), q.stride(1), p(counts), p(rows)
    d.Nl, d.C, d.K = rows.shape[0], rows.shape[1], q.shape[1] if K is None else K
    d.switch_penalty, d.background = lam, b
    d.label, d.score, d.total, d.nseg = p(out[0]), p(out[1]), p(out[2]), p(out[3])
    return d


def test_every_bad_argument_is_refused_with_a_message():
    L = _lib.lib()
    F, K = 8, 3
    inf, nan = float("inf"), float("nan")
    frames, mask = torch.zeros(3, F, H, device=DEV), torch.ones(3, F, dtype=torch.int64, device=DEV)
    big = torch.zeros(3, 129, H, device=DEV)                              # room for the F = 129 descriptor: refused, but nothing dangles
    wnorm = torch.zeros(3, 129, 129, device=DEV)
    q = torch.zeros(4, 65, H + 4, device=DEV)[:, :K, :H]                  # room for the K = 65 descriptor
    counts, rows = torch.ones(4, dtype=torch.int32, device=DEV), torch.zeros(4, 2, dtype=torch.int32, device=DEV)
    out = (torch.zeros(4, 2, 129, dtype=torch.int32, device=DEV), torch.zeros(4, 2, 129, device=DEV), torch.zeros(4, 2, device=DEV),
           torch.zeros(4, 2, dtype=torch.int32, device=DEV))
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    good = lambda **kw: _desc(kw.pop("frames", frames), mask, wnorm, q, counts, rows, out, **kw)
    fn, who = L.univl_frame_segment, b"univl_frame_segment"
    assert fn(C.byref(good()), stream) == 0 and fn(C.byref(good(normalize=0)), stream) == 0
    d = good(normalize=0); d.wnorm = None
    assert fn(C.byref(d), stream) == 0                                    # use_mil needs no table
    assert fn(C.byref(good(K=64)), stream) == 0 and fn(C.byref(good(K=1)), stream) == 0
    assert fn(C.byref(good(lam=0.0, b=-inf)), stream) == 0 and fn(C.byref(good(lam=3e38, b=-3e38)), stream) == 0
    # case -> (descriptor, status, words only that case's message holds)
    bad = {"F = 129": (good(frames=big), -1, b"F=129"), "F = 0": (good(F=0), -1, b"F=0"), "H != 768": (good(Hh=512), -1, b"H=512"),
           "normalize": (good(normalize=2), -1, b"normalize=2"),
           "K = 0": (good(K=0), -1, b"K=0"), "K = 65": (good(K=65), -1, b"K=65"), "K < 0": (good(K=-1), -1, b"K=-1"),
           "lambda < 0": (good(lam=-0.5), -1, b"switch_penalty=-0.5"), "lambda NaN": (good(lam=nan), -1, b"switch_penalty="),
           "lambda inf": (good(lam=inf), -1, b"switch_penalty=inf"), "b NaN": (good(b=nan), -1, b"background="),
           "b +inf": (good(b=inf), -1, b"background=inf")}
    for name, field, word in (("null frames", "frames", b"(frames, mask)"), ("null mask", "mask", b"(frames, mask)"), ("null wnorm", "wnorm", b"wnorm"),
                              ("null q", "q", b"(q, counts"), ("null counts", "counts", b"(q, counts"), ("null rows", "rows", b"(q, counts"),
                              ("null label", "label", b"(q, counts"), ("null score", "score", b"(q, counts"), ("null total", "total", b"(q, counts"),
                              ("null nseg", "nseg", b"(q, counts")):
        d = good()
        setattr(d, field, None)
        bad[name] = (d, -1, word)
    d = good(); d.N = 0; bad["N < 1"] = (d, -1, b"N=0")
    d = good(); d.Nl = 0; bad["Nl < 1"] = (d, -1, b"Nl=0")
    d = good(); d.C = 0; bad["C < 1"] = (d, -1, b"C=0")
    d = good(); d.Nl, d.C = 2 ** 16, 2 ** 15; bad["Nl * C = 2^31"] = (d, -1, b"Nl=65536 C=32768")
    d = good(); d.ld_row = F * H - 4; bad["ld_row < F * 768"] = (d, -1, b"ld_row=6140")
    d = good(); d.ldq = 764; bad["ldq < 768"] = (d, -1, b"ldq=764")
    d = good(); d.frames = C.c_void_p(frames.data_ptr() + 4); bad["misaligned frames"] = (d, -2, b"rows of frames")
    d = good(); d.ld_row = F * H + 2; bad["misaligned gallery rows"] = (d, -2, b"rows of frames")
    d = good(); d.q = C.c_void_p(q.data_ptr() + 4); bad["misaligned q"] = (d, -2, b"rows of q")
    d = good(); d.ldq = H + 2; bad["misaligned label rows"] = (d, -2, b"rows of q")
    for name, (d, status, word) in bad.items():
        assert fn(C.byref(good()), stream) == 0                           # a good call in between: no message is left over
        rc = fn(C.byref(d), stream)
        assert rc == status, (name, rc)                                   # UNIVL_EINVAL / UNIVL_EALIGN
        msg = L.univl_last_error()
        assert who in msg and word in msg, (name, msg)
    assert fn(None, stream) == -1
    torch.cuda.synchronize()
    qc = torch.zeros(4, K, H, device=DEV)
    with pytest.raises(RuntimeError, match="needs wnorm"):
        ops.frame_segment(qc, counts, frames, mask, rows, 0.5)
    with pytest.raises(RuntimeError, match="switch_penalty=-1"):
        ops.frame_segment(qc, counts, frames, mask, rows, -1.0, normalize=False)
    with pytest.raises(RuntimeError, match="background=nan"):
        ops.frame_segment(qc, counts, frames, mask, rows, 1.0, nan, normalize=False)
    with pytest.raises(RuntimeError, match="K=65"):
        ops.frame_segment(torch.zeros(4, 65, H, device=DEV), counts, frames, mask, rows, 0.5, normalize=False)
    with pytest.raises(RuntimeError, match="512 wide"):
        ops.frame_segment(torch.zeros(4, K, 512, device=DEV), counts, frames, mask, rows, 0.5, normalize=False)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.frame_segment(qc.cpu(), counts, frames, mask, rows, 0.5, normalize=False)


# ------------------------------------------------------------------------------------------------ G: through the model
def _index(model, bs, **kw):
    from univl_amd.retrieval import VideoIndex
    index = VideoIndex(model, keep_frames=True, **kw)
    for b in bs:
        index.add(b["video"], b["video_mask"])
    return index


def _sets(text, order):
    """[Nl, K, W] label sets out of the [n, W] text tensors: set i holds the texts order[i]."""
    idx = torch.as_tensor(order, device=DEV)
    return tuple(t[idx] for t in text)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_segment_against_the_public_path(dtype, deterministic_models):
    from test_model_gpu import GATES
    cfg, rows, dseed = case_config("joint_small")
    model, _ = build(cfg, dtype)
    model.eval()
    bs = _batches(cfg, [3, 3], dseed)
    cat = {k: torch.cat([b[k] for b in bs]) for k in bs[0]}
    text = tuple(cat[k].reshape(-1, cat[k].shape[-1]) for k in ("input_ids", "token_type_ids", "attention_mask"))        # [texts, W]
    tol = TOL if dtype == torch.float32 else GATES[torch.bfloat16]["sim"]
    n, F, K = 6, cfg.max_frames, 3
    index = _index(model, bs, capacity=8)
    fmask = index._fmask[:n].cpu().numpy()
    order = [[(i + k) % n for k in range(K)] for i in range(n)]
    counts = torch.tensor([K] * (n - 1) + [2], dtype=torch.int32)
    cand = torch.tensor([[i, (i + 1) % n] for i in range(n)], dtype=torch.int32)
    q, so, am = index.pool_text(*text)
    vo = index._frames[:n].clone()
    plain = index.segment(*_sets(text, order), counts, cand)              # lambda = 0, no background
    assert bool((plain[0][plain[0] != -2] >= 0).all())
    b = float(plain[1][torch.isfinite(plain[1])].median())                # a background score that some frames beat and some do not
    for lam, bg, got in ((0.0, None, plain), (0.01, b, index.segment(*_sets(text, order), counts, cand, 0.01, b))):
        label, score, total, nseg = (t.cpu() for t in got)
        assert bg is None or (bool((label == -1).any()) and bool((label >= 0).any()))
        for i in range(n):
            for c in range(2):
                v, nk = int(cand[i, c]), int(counts[i])
                lab = label[i, c].numpy()
                assert np.array_equal(lab == -2, fmask[v] == 0) and np.all(lab < nk)
                yy = np.where(lab[fmask[v] != 0] < 0, nk, lab[fmask[v] != 0])
                assert int(nseg[i, c]) == GR.run_count(yy, nk)
                for f in np.nonzero(fmask[v])[0]:
                    if lab[f] == -1:
                        assert float(score[i, c, f]) == np.float32(bg)
                        continue
                    if c == 1 and f % 3:                                  # the public path on every frame of the first candidate, a third of the second's
                        continue
                    wmask = torch.zeros(1, F, dtype=torch.int64, device=DEV)
                    wmask[0, f] = 1
                    t = order[i][lab[f]]
                    want = model.get_similarity_logits(so[t:t + 1], vo[v:v + 1], am[t:t + 1], wmask)
                    assert abs(float(want[0, 0]) - float(score[i, c, f])) <= tol, (i, c, f)


def test_eval_segmentation_on_planted_ground_truth_and_the_table_across_growth(deterministic_models):
    from univl_amd.retrieval import VideoIndex
    cfg, rows, dseed = case_config("joint_small")
    model, _ = build(cfg, torch.float32)
    model.eval()
    bs = _batches(cfg, [3, 3, 2], dseed)
    cat = {k: torch.cat([b[k] for b in bs]) for k in bs[0]}
    text = tuple(cat[k].reshape(-1, cat[k].shape[-1]) for k in ("input_ids", "token_type_ids", "attention_mask"))        # [texts, W]
    F, K, n = cfg.max_frames, 3, 8

    # 3 + 3 + 2 rows into a capacity of 4: the table is filled lazily and survives the growth bit for bit
    index = VideoIndex(model, capacity=4, keep_frames=True)
    index.add(bs[0]["video"], bs[0]["video_mask"])
    order3 = [[(i + k) % 3 for k in range(K)] for i in range(3)]
    counts3, cand3 = torch.tensor([3, 2, 1], dtype=torch.int32), torch.arange(3, dtype=torch.int32).repeat(3, 1)
    first = index.segment(*_sets(text, order3), counts3, cand3, 0.01)
    assert index._wnorm_rows == 3 and index._wnorm.shape == (4, F, F)
    kept = index._wnorm[:3].clone()
    index.add(bs[1]["video"], bs[1]["video_mask"])
    index.add(bs[2]["video"], bs[2]["video_mask"])
    again = index.segment(*_sets(text, order3), counts3, cand3, 0.01)
    assert index._wnorm_rows == 8 == len(index) and index._wnorm.shape == (8, F, F) and torch.equal(index._wnorm[:3], kept)
    for x, y in zip(first, again):
        assert torch.equal(x, y)

    # every set in its own video; the last set has a count of 0: nothing to label
    order = [[(i + k) % n for k in range(K)] for i in range(n)]
    counts = np.array([K] * (n - 2) + [2, 0], dtype=np.int32)
    sets = _sets(text, order)
    targets = np.arange(n)
    plain = index.segment(*sets, torch.from_numpy(counts), targets.reshape(n, 1))
    lam, b = 0.01, float(plain[1][torch.isfinite(plain[1])].median())
    label, _, total, nseg = (t.cpu().numpy() for t in index.segment(*sets, torch.from_numpy(counts), targets.reshape(n, 1), lam, b))
    label, total, nseg = label[:, 0].astype(np.int64), total[:, 0], nseg[:, 0]
    lv = index._fmask[:n].sum(1).cpu().numpy()
    lv[n - 1] = 0                                                         # the empty set counts no frame
    assert np.all(label[n - 1] == -2) and total[n - 1] == NEG_INF and np.any(label == -1) and np.any(label >= 0)
    batches = [tuple(t[lo:hi] for t in (sets[0], sets[2], sets[1])) + (torch.from_numpy(counts[lo:hi]),) for lo, hi in ((0, 3), (3, 6), (6, 8))]
    # the kernel's own labels as ground truth: every annotated valid frame is right
    m = uev.eval_segmentation(model, index, batches, targets, label, lam, b)
    assert m["frame_accuracy"] == 1.0 and m["correct"].tolist() == m["annotated"].tolist() == lv.tolist()
    assert m["n_lists"] == n and m["n_frames"] == int(lv.sum()) and m["n_segments"] == int(nseg.sum()) and m["n_empty"] == 1
    assert m["frame_accuracy_fg"] == 1.0 and m["correct"].dtype == m["annotated"].dtype == np.int64
    # frame 0 of lists 0 and 2 flipped (to another label or to the background), frame 0 of list 1 not annotated, a masked frame annotated
    gt = label.copy()
    assert np.all(label[:3, 0] != -2)                                     # frame 0 is a frame of these videos
    for i in (0, 2):
        gt[i, 0] = -1 if gt[i, 0] >= 0 else 0
    gt[1, 0] = -2
    masked = np.argwhere(label[:n - 1] == -2)
    if len(masked):
        gt[masked[0][0], masked[0][1]] = 0                                # the video has no such frame: never counted
    m = uev.eval_segmentation(model, index, batches, targets, gt, lam, b)
    want = GR.frame_counts(label, total, nseg, gt)
    correct, annotated = lv.copy(), lv.copy()
    correct[[0, 2]] -= 1
    correct[1] -= 1
    annotated[1] -= 1
    assert m["correct"].tolist() == want["correct"].tolist() == correct.tolist()
    assert m["annotated"].tolist() == want["annotated"].tolist() == annotated.tolist()
    assert m["frame_accuracy"] == want["frame_accuracy"] == correct.sum() / annotated.sum()
    assert m["frame_accuracy_fg"] == want["frame_accuracy_fg"] and m["n_frames"] == int(lv.sum()) - 1 and m["n_empty"] == 1
    with pytest.raises(ValueError, match="more lists than targets"):
        uev.eval_segmentation(model, index, batches, targets[:7], gt[:7], lam, b)
    with pytest.raises(ValueError, match="lists of 65 steps"):
        index.segment_vectors(torch.zeros(1, 65, H, device=DEV), [1], [[0]])
    with pytest.raises(ValueError, match="switch_penalty="):
        index.segment_vectors(torch.zeros(1, 2, H, device=DEV), [1], [[0]], -1.0)
