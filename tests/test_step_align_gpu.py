"""Ordered step alignment: the kernel (csrc/moment.hip: univl_step_align), ops.step_align, VideoIndex.align_steps / align_vectors and
eval.eval_step_alignment.

A  fp64 parity on LayerNorm-scale frames and unit step vectors (tests/step_align_ref.py), both modes: feasibility exactly, the
   alignment returned is one, every score within the project's fp32 gate 2e-4 of that window's fp64 score, the fp64 total of the
   alignment returned and the total returned within n * 2e-4 of the reference optimum.  No window position is compared under a
   tolerance;
B  exact arithmetic (small integers, use_mil, window lengths 1, 2, 4): alignments equal element for element, scores and totals
   bit-equal, identical frames packed to the left;
C  masks: none valid, a hole, the feasibility edges, a single valid frame;
D  candidates outside the gallery, duplicates, counts outside [1, K], NaN around the gallery and in the padding of q;
E  purity: position, company, deterministic mode, the padding K; with one step, univl_moment_localize bit for bit;
F  every argument the entry point refuses;
G  through the model: align_steps against localize and get_similarity_logits, eval_step_alignment on planted ground truth, the lazily
   filled table across index growth."""
import ctypes as C

import numpy as np
import pytest
import torch

from make_golden import case_config

import moment_ref as R
import step_align_ref as SR
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
    start, length, score, total = out
    return start.cpu().numpy().astype(np.int64), length.cpu().numpy().astype(np.int64), score.cpu().numpy(), total.cpu().numpy()


def _align(frames, mask, q, counts, rows, lmin, lmax, normalize, wnorm=None):
    if normalize and wnorm is None:
        wnorm = ops.window_norms(frames, mask)
    return _host(ops.step_align(q, counts, frames, mask, rows, lmin, lmax, wnorm=wnorm, normalize=normalize))


def _check_empty(got, where, counts):
    """Padding slots everywhere, and every slot and the total where `where` [Nl, C] says there is no alignment."""
    start, length, score, total = got
    K = start.shape[2]
    pad = np.arange(K)[None, None, :] >= np.clip(np.asarray(counts), 0, K)[:, None, None]
    empty = pad | where[:, :, None]
    assert np.all(start[empty] == -1) and np.all(length[empty] == 0) and np.all(score[empty] == NEG_INF)
    assert np.all(total[where] == NEG_INF) and np.all(np.isfinite(total[~where]))
    assert np.all(start[~empty] >= 0) and np.all(length[~empty] >= 1) and np.all(np.isfinite(score[~empty]))
    assert not np.any(np.isnan(score)) and not np.any(np.isnan(total))


# ------------------------------------------------------------------------------------------------ A: fp64 parity
@pytest.mark.parametrize("F,K", SR.parity_shapes())
def test_kernel_against_fp64(F, K):
    """fp32 against the float64 programme.  The largest score and total errors are printed (over all shapes: profiles/step_align.txt)."""
    frames, mask, q, counts, rows = SR.parity_case(F, K)
    dev = _dev(frames, mask, q, counts, rows)
    wnorm = ops.window_norms(dev[0], dev[1])
    worst_score = worst_total = 0.0
    for normalize in (True, False):
        for (lmin, lmax), (r_start, r_length, r_score, r_total) in SR.parity_reference(F, K, normalize).items():
            got = _align(*dev, lmin, lmax, normalize, wnorm)
            start, length, score, total = got
            _check_empty(got, ~np.isfinite(r_total), counts)              # feasibility agrees exactly
            for i, c in zip(*np.nonzero(np.isfinite(r_total))):
                n, r = int(counts[i]), int(rows[i, c])
                s, l = start[i, c, :n], length[i, c, :n]
                assert SR.is_alignment(mask[r], s, l, lmin, lmax), (F, K, lmin, lmax, i, c, s, l)
                S = SR.parity_scores(F, K, int(i), r, normalize)
                w64 = np.array([S[k, s[k], l[k] - 1] for k in range(n)])
                err = float(np.abs(score[i, c, :n].astype(np.float64) - w64).max())
                terr = max(abs(SR.total_of(S, s, l) - r_total[i, c]), abs(float(total[i, c]) - r_total[i, c]))
                worst_score, worst_total = max(worst_score, err), max(worst_total, terr / n)
                assert err <= TOL, (F, K, lmin, lmax, i, c, err)
                assert abs(SR.total_of(S, s, l) - r_total[i, c]) <= n * TOL, (F, K, lmin, lmax, i, c)
                assert abs(float(total[i, c]) - r_total[i, c]) <= n * TOL, (F, K, lmin, lmax, i, c)
    print("F=%d K=%d: max score error %.3e, max total error per step %.3e" % (F, K, worst_score, worst_total))


# ------------------------------------------------------------------------------------------------ B: exact arithmetic
@pytest.mark.parametrize("F", SR.EXACT_F)
def test_exact_integer_inputs_use_mil(F):
    frames, mask, q, counts, rows = SR.exact_case(F)
    dev = _dev(frames, mask, q, counts, rows)
    for (lmin, lmax), (r_start, r_length, r_score, r_total) in SR.exact_reference(F).items():
        start, length, score, total = _align(*dev, lmin, lmax, False)
        assert np.array_equal(start, r_start) and np.array_equal(length, r_length), (F, lmin, lmax)
        assert np.array_equal(score, r_score.astype(np.float32)) and np.array_equal(total, r_total.astype(np.float32))      # exact, so bit-equal
        for i, c in zip(*np.nonzero(np.isfinite(r_total) & (rows == 5))):                                           # identical frames
            n = counts[i]
            assert start[i, c, :n].tolist() == [k * lmin for k in range(n)] and np.all(length[i, c, :n] == lmin)
        assert np.isfinite(r_total).any() and (~np.isfinite(r_total)).any()


# ------------------------------------------------------------------------------------------------ C: masks
@pytest.mark.parametrize("normalize", [True, False], ids=["normalize", "use_mil"])
def test_masks(normalize):
    F, K = 20, 3
    rng = np.random.RandomState(21)
    frames = (rng.standard_normal((9, F, H)) * (28.0 / np.sqrt(H))).astype(np.float32)
    q = rng.standard_normal((3, K, H))
    q = (q / np.linalg.norm(q, axis=2, keepdims=True)).astype(np.float32)
    counts = np.array([1, 2, 3], dtype=np.int32)
    mask = np.zeros((9, F), dtype=np.int64)                               # row 0: nothing valid
    mask[1, :] = 1
    mask[1, 9] = 0                                                        # a hole: windows on both sides, none across
    mask[2, 7] = 1                                                        # a single valid frame, not the first
    mask[3, 2:8] = 1                                                      # exactly 3 * 2 valid frames
    mask[4, 2:7] = 1                                                      # one fewer
    mask[5, [0, 1, 3]] = 1                                                # frames 0, 1, 3
    mask[6, [0, 1, 2, 4]] = 1                                             # four valid frames laid out 3 + 1
    mask[7, :] = 1
    mask[8, 3:7] = 1                                                      # exactly 2 * 2 valid frames
    rows = np.tile(np.arange(9, dtype=np.int32), (3, 1))
    dev = _dev(frames, mask, q, counts, rows)
    for lmin, lmax in ((1, 1), (2, 2), (2, 6), (1, F), (8, 10)):
        got = _align(*dev, lmin, lmax, normalize)
        start, length, score, total = got
        r_start, r_length, r_score, r_total = SR.align(q, counts, frames, mask, rows, lmin, lmax, normalize)
        _check_empty(got, ~np.isfinite(r_total), counts)
        for i, c in zip(*np.nonzero(np.isfinite(r_total))):
            n = counts[i]
            assert SR.is_alignment(mask[c], start[i, c, :n], length[i, c, :n], lmin, lmax)
            S, _ = R.row_scores(q[i, :n], frames[c], mask[c], normalize)
            assert abs(SR.total_of(S, start[i, c, :n], length[i, c, :n]) - r_total[i, c]) <= n * TOL
            assert abs(float(total[i, c]) - r_total[i, c]) <= n * TOL
        assert np.all(total[:, 0] == NEG_INF)                             # nothing valid
        ends = start[:, 1] + length[:, 1]
        assert np.all((length[:, 1] == 0) | (ends <= 9) | (start[:, 1] >= 10))                                   # never across the hole
        if (lmin, lmax) == (8, 10):                                       # one window on each side of the hole and no room for a third
            assert start[1, 1, 0] + length[1, 1, 0] <= 9 and start[1, 1, 1] >= 10 and total[2, 1] == NEG_INF
        if lmin == 1:                                                     # a single valid frame: one step fits, two do not
            assert (start[0, 2, 0], length[0, 2, 0]) == (7, 1) and total[1, 2] == NEG_INF and total[2, 2] == NEG_INF
        else:
            assert np.all(total[:, 2] == NEG_INF)
        if lmin == 2:
            assert start[2, 3].tolist() == [2, 4, 6] and length[2, 3].tolist() == [2, 2, 2]                      # exactly n * lmin frames
            assert total[2, 4] == NEG_INF and np.isfinite(total[1, 4])                                           # one fewer
            assert total[1, 5] == NEG_INF and total[1, 6] == NEG_INF and np.isfinite(total[0, 5]) and np.isfinite(total[0, 6])
            assert start[1, 8, :2].tolist() == [3, 5] and length[1, 8, :2].tolist() == [2, 2] and total[2, 8] == NEG_INF


# ------------------------------------------------------------------------------------------------ D: candidates, counts, poison
def test_rows_and_counts_outside_their_range_duplicates_and_poisoned_memory():
    F, N, K = 16, 4, 4
    rng = np.random.RandomState(22)
    frames = (rng.standard_normal((N, F, H)) * (28.0 / np.sqrt(H))).astype(np.float32)
    mask = np.ones((N, F), dtype=np.int64)
    counts = np.array([4, 2, 0, -1, K + 1, 1, 3], dtype=np.int32)
    q = rng.standard_normal((7, K, H)).astype(np.float32)
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
    for normalize in (True, False):
        wnorm = ops.window_norms(d_frames, d_mask) if normalize else None
        got = _host(ops.step_align(d_q, d_counts, d_frames, d_mask, d_rows, 2, 5, wnorm=wnorm, normalize=normalize))
        start, length, score, total = got
        out = (rows < 0) | (rows >= N) | ((counts < 1) | (counts > K))[:, None]
        _check_empty(got, out, counts)
        for i, a, b in ((0, 0, 3), (0, 0, 7), (5, 2, 3), (6, 0, 3)):                                              # duplicated candidates
            assert np.array_equal(start[i, a], start[i, b]) and np.array_equal(length[i, a], length[i, b])
            assert np.array_equal(score[i, a], score[i, b]) and total[i, a] == total[i, b]
        r_total = SR.align(np.nan_to_num(q), counts, frames, mask, rows, 2, 5, normalize)[3]
        assert np.array_equal(np.isfinite(total), np.isfinite(r_total))
        assert np.abs(total[~out].astype(np.float64) - r_total[~out]).max() <= K * TOL


# ------------------------------------------------------------------------------------------------ E: purity
def test_purity_position_company_deterministic_mode_and_padding():
    F, K = 48, 3
    frames, mask, q, counts, _ = SR.parity_case(F, K)
    rng = np.random.RandomState(23)
    rows = rng.randint(0, R.PARITY_ROWS, size=(5, 6)).astype(np.int32)
    rows[:, 0] = 0
    d_frames, d_mask, d_q, d_counts, d_rows = _dev(frames, mask, q, counts, rows)
    wnorm = ops.window_norms(d_frames, d_mask)
    wide = torch.full((5, 32, H), float("nan"), device=DEV)               # the same lists padded to K = 32
    wide[:, :K] = d_q
    was = univl_amd.deterministic()
    try:
        for normalize in (True, False):
            w = wnorm if normalize else None
            run = lambda qq, cc, rr: ops.step_align(qq, cc, d_frames, d_mask, rr, 2, 5, wnorm=w, normalize=normalize)
            univl_amd.set_deterministic(False)
            base = run(d_q, d_counts, d_rows)
            univl_amd.set_deterministic(True)
            det = run(d_q, d_counts, d_rows)
            univl_amd.set_deterministic(False)
            for a, b in zip(base, det):
                assert torch.equal(a, b)
            assert bool(torch.isfinite(base[3]).any())
            for i, j in ((0, 0), (2, 3), (4, 5)):                         # pair (i, j) alone
                alone = run(d_q[i:i + 1], d_counts[i:i + 1], d_rows[i:i + 1, j:j + 1].contiguous())
                for a, b in zip(base, alone):
                    assert torch.equal(a[i, j], b[0, 0])
            moved = run(d_q.flip(0).contiguous(), d_counts.flip(0).contiguous(), d_rows.flip(0).roll(2, 1).contiguous())
            for a, b in zip(base, moved):
                assert torch.equal(a.flip(0).roll(2, 1), b)
            padded = run(wide, d_counts, d_rows)
            for a, b in zip(base[:3], padded[:3]):
                assert torch.equal(a, b[:, :, :K])
            assert torch.equal(base[3], padded[3]) and torch.all(padded[0][:, :, K:] == -1) and torch.all(padded[2][:, :, K:] == NEG_INF)
    finally:
        univl_amd.set_deterministic(was)


@pytest.mark.parametrize("F", R.PARITY_F)
def test_one_step_is_moment_localize_bit_for_bit(F):
    frames, mask, q, rows = R.parity_case(F, 37)
    rows = np.concatenate([rows, np.roll(rows, 5, 0), np.full_like(rows, -1)], 1)
    d_frames, d_mask, d_q, d_rows = _t(frames), _t(mask), _t(q), _t(rows)
    ones = torch.ones(37, dtype=torch.int32, device=DEV)
    wnorm = ops.window_norms(d_frames, d_mask)
    wide = torch.full((37, 4, H), float("nan"), device=DEV)
    wide[:, 0] = d_q
    for normalize in (True, False):
        w = wnorm if normalize else None
        for lmin, lmax in R.parity_windows(F):
            want = ops.moment_localize(d_q, d_frames, d_mask, d_rows, lmin, lmax, wnorm=w, normalize=normalize)
            for qq in (d_q.view(37, 1, H), wide):
                start, length, score, total = ops.step_align(qq, ones, d_frames, d_mask, d_rows, lmin, lmax, wnorm=w, normalize=normalize)
                assert torch.equal(start[:, :, 0], want[0]) and torch.equal(length[:, :, 0], want[1])
                assert torch.equal(score[:, :, 0], want[2]) and torch.equal(total, want[2])
                assert torch.equal(score[:, :, 0].view(torch.int32), want[2].view(torch.int32))                 # the bits, not only the values


# ------------------------------------------------------------------------------------------------ F: refusals
def _desc(frames, mask, wnorm, q, counts, rows, out, F=None, Hh=H, normalize=1, lmin=1, lmax=2, K=None):
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    d = _lib.StepAlign()
    d.frames, d.ld_row, d.mask, d.wnorm = p(frames), frames.stride(0), p(mask), p(wnorm)
    d.N, d.F, d.H, d.normalize = frames.shape[0], frames.shape[1] if F is None else F, Hh, normalize
    d.q, d.ldq, d.counts, d.rows = p(q), q.stride(1), p(counts), p(rows)
    d.Nl, d.C, d.K, d.lmin, d.lmax = rows.shape[0], rows.shape[1], q.shape[1] if K is None else K, lmin, lmax
    d.start, d.length, d.score, d.total = p(out[0]), p(out[1]), p(out[2]), p(out[3])
    return d


def test_every_bad_argument_is_refused_with_a_message():
    L = _lib.lib()
    F, K = 8, 3
    frames, mask = torch.zeros(3, F, H, device=DEV), torch.ones(3, F, dtype=torch.int64, device=DEV)
    big = torch.zeros(3, 129, H, device=DEV)                              # room for the F = 129 descriptor: refused, but nothing dangles
    wnorm = torch.zeros(3, 129, 129, device=DEV)
    q = torch.zeros(4, 33, H + 4, device=DEV)[:, :K, :H]                  # room for the K = 33 descriptor
    counts, rows = torch.ones(4, dtype=torch.int32, device=DEV), torch.zeros(4, 2, dtype=torch.int32, device=DEV)
    out = (torch.zeros(4, 2, 33, dtype=torch.int32, device=DEV), torch.zeros(4, 2, 33, dtype=torch.int32, device=DEV),
           torch.zeros(4, 2, 33, device=DEV), torch.zeros(4, 2, device=DEV))
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    good = lambda **kw: _desc(kw.pop("frames", frames), mask, wnorm, q, counts, rows, out, **kw)
    fn, who = L.univl_step_align, b"univl_step_align"
    assert fn(C.byref(good()), stream) == 0 and fn(C.byref(good(normalize=0)), stream) == 0
    d = good(normalize=0); d.wnorm = None
    assert fn(C.byref(d), stream) == 0                                    # use_mil needs no table
    assert fn(C.byref(good(K=32)), stream) == 0 and fn(C.byref(good(K=1)), stream) == 0
    # case -> (descriptor, status, words only that case's message holds)
    bad = {"F = 129": (good(frames=big), -1, b"F=129"), "F = 0": (good(F=0), -1, b"F=0"), "H != 768": (good(Hh=512), -1, b"H=512"),
           "normalize": (good(normalize=2), -1, b"normalize=2"), "lmin = 0": (good(lmin=0), -1, b"lmin=0"),
           "lmin > lmax": (good(lmin=3, lmax=2), -1, b"lmin=3 lmax=2"), "lmax > F": (good(lmax=F + 1), -1, b"lmax=9"),
           "K = 0": (good(K=0), -1, b"K=0"), "K = 33": (good(K=33), -1, b"K=33"), "K < 0": (good(K=-1), -1, b"K=-1")}
    for name, field, word in (("null frames", "frames", b"(frames, mask)"), ("null mask", "mask", b"(frames, mask)"), ("null wnorm", "wnorm", b"wnorm"),
                              ("null q", "q", b"(q, counts"), ("null counts", "counts", b"(q, counts"), ("null rows", "rows", b"(q, counts"),
                              ("null start", "start", b"(q, counts"), ("null length", "length", b"(q, counts"), ("null score", "score", b"(q, counts"),
                              ("null total", "total", b"(q, counts")):
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
    d = good(); d.ldq = H + 2; bad["misaligned step rows"] = (d, -2, b"rows of q")
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
        ops.step_align(qc, counts, frames, mask, rows, 1, 2)
    with pytest.raises(RuntimeError, match="lmin=5"):
        ops.step_align(qc, counts, frames, mask, rows, 5, 4, normalize=False)
    with pytest.raises(RuntimeError, match="K=33"):
        ops.step_align(torch.zeros(4, 33, H, device=DEV), counts, frames, mask, rows, 1, 2, normalize=False)
    with pytest.raises(RuntimeError, match="512 wide"):
        ops.step_align(torch.zeros(4, K, 512, device=DEV), counts, frames, mask, rows, 1, 2, normalize=False)


# ------------------------------------------------------------------------------------------------ G: through the model
def _index(model, bs, **kw):
    from univl_amd.retrieval import VideoIndex
    index = VideoIndex(model, keep_frames=True, **kw)
    for b in bs:
        index.add(b["video"], b["video_mask"])
    return index


def _lists(text, order):
    """[Nl, K, W] step lists out of the [n, W] text tensors: list i holds the texts order[i]."""
    idx = torch.as_tensor(order, device=DEV)
    return tuple(t[idx] for t in text)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_align_steps_against_localize_and_the_public_path(dtype, deterministic_models):
    from test_model_gpu import GATES
    cfg, rows, dseed = case_config("joint_small")
    model, _ = build(cfg, dtype)
    model.eval()
    bs = _batches(cfg, [3, 3], dseed)
    cat = {k: torch.cat([b[k] for b in bs]) for k in bs[0]}
    text = tuple(cat[k].reshape(-1, cat[k].shape[-1]) for k in ("input_ids", "token_type_ids", "attention_mask"))        # [texts, W]
    tol = TOL if dtype == torch.float32 else GATES[torch.bfloat16]["sim"]
    n, F = 6, cfg.max_frames
    index = _index(model, bs, capacity=8)
    lv = index._fmask[:n].sum(1).cpu().numpy()

    # one step per list: localize, bit for bit
    cand = torch.arange(n, dtype=torch.int32).repeat(n, 1)
    for window in ((1, 1), (1, 3), (2, F)):
        want = index.localize(*text, cand, window)
        start, length, score, total = index.align_steps(*(t[:, None] for t in text), torch.ones(n, dtype=torch.int32), cand, window)
        assert torch.equal(start[:, :, 0], want[0]) and torch.equal(length[:, :, 0], want[1])
        assert torch.equal(score[:, :, 0], want[2]) and torch.equal(total, want[2])

    # several steps: list i holds texts i, i + 1, i + 2 (mod n), the last list only two of them; every list against two videos
    K = 3
    order = [[(i + k) % n for k in range(K)] for i in range(n)]
    counts = torch.tensor([K] * (n - 1) + [2], dtype=torch.int32)
    cand = torch.tensor([[i, (i + 1) % n] for i in range(n)], dtype=torch.int32)
    lmax = max(1, int(lv.max()) // K)
    start, length, score, total = (t.cpu() for t in index.align_steps(*_lists(text, order), counts, cand, (1, lmax)))
    q, so, am = index.pool_text(*text)
    vo = index._frames[:n].clone()
    assert bool(torch.isfinite(total).any())
    for i in range(n):
        for c in range(2):
            v, nk = int(cand[i, c]), int(counts[i])
            assert bool(torch.isfinite(total[i, c])) == (lv[v] >= nk)     # one frame per step at the least
            if lv[v] < nk:
                assert torch.all(start[i, c] == -1) and torch.all(length[i, c] == 0) and torch.all(score[i, c] == NEG_INF)
                continue
            s, l = start[i, c, :nk].numpy(), length[i, c, :nk].numpy()
            assert SR.is_alignment(index._fmask[v].cpu().numpy(), s, l, 1, lmax)                                  # ordered, never overlapping
            assert np.all(s[1:] >= s[:-1] + l[:-1]) and torch.all(start[i, c, nk:] == -1)
            for k in range(nk):                                           # the public path with the video mask narrowed to the window
                wmask = torch.zeros(1, F, dtype=torch.int64, device=DEV)
                wmask[0, s[k]:s[k] + l[k]] = 1
                t = order[i][k]
                want = model.get_similarity_logits(so[t:t + 1], vo[v:v + 1], am[t:t + 1], wmask)
                assert abs(float(want[0, 0]) - float(score[i, c, k])) <= tol, (i, c, k)


def test_eval_step_alignment_on_planted_ground_truth_and_the_table_across_growth(deterministic_models):
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
    first = index.align_steps(*_lists(text, order3), counts3, cand3, (1, 2))
    assert index._wnorm_rows == 3 and index._wnorm.shape == (4, F, F)
    kept = index._wnorm[:3].clone()
    index.add(bs[1]["video"], bs[1]["video_mask"])
    index.add(bs[2]["video"], bs[2]["video_mask"])
    again = index.align_steps(*_lists(text, order3), counts3, cand3, (1, 2))
    assert index._wnorm_rows == 8 == len(index) and index._wnorm.shape == (8, F, F) and torch.equal(index._wnorm[:3], kept)
    for a, b in zip(first, again):
        assert torch.equal(a, b)

    # every list in its own video; a window so long that the shortest videos cannot hold three steps
    lv = index._fmask[:n].sum(1).cpu().numpy()
    lmin = int(lv.min()) // K + 1
    lmax = min(lmin + 1, F)
    assert (lv >= K * lmin).any() and (lv < K * lmin).any()
    order = [[(i + k) % n for k in range(K)] for i in range(n)]
    counts = np.full(n, K, dtype=np.int32)
    lists = _lists(text, order)
    targets = np.arange(n)
    start, length, _, total = (t.cpu().numpy() for t in index.align_steps(*lists, torch.from_numpy(counts), targets.reshape(n, 1), (lmin, lmax)))
    start, length, total = start[:, 0].astype(np.int64), length[:, 0].astype(np.int64), total[:, 0]
    found = np.isfinite(total)
    assert found.any() and (~found).any() and np.array_equal(found, lv >= K * lmin)
    # even lists are annotated with the windows found, odd ones with segments that begin where the windows end; step i % 3 of list i is
    # not annotated
    even = (np.arange(n) % 2 == 0)[:, None]
    gt_start = np.where(found[:, None] & even, start, np.where(found[:, None], start + length, 0))
    gt_len = np.where(found[:, None] & even, length, 2)
    gt_len[np.arange(n), np.arange(n) % K] = 0
    batches = [tuple(t[lo:hi] for t in (lists[0], lists[2], lists[1])) + (torch.from_numpy(counts[lo:hi]),) for lo, hi in ((0, 3), (3, 6), (6, 8))]
    m = uev.eval_step_alignment(model, index, batches, targets, gt_start, gt_len, (lmin, lmax))
    want = SR.step_counts(start, length, counts, total, gt_start, gt_len)
    hits = np.where(found & even[:, 0], K - 1, 0)
    assert m["hits"].tolist() == want["hits"].tolist() == hits.tolist() and m["annotated"].tolist() == want["annotated"].tolist() == [K - 1] * n
    assert m["hits"].dtype == m["annotated"].dtype == np.int64
    assert m["n_lists"] == n and m["n_steps"] == n * (K - 1) and m["n_infeasible"] == int((~found).sum()) == want["n_infeasible"]
    assert m["recall"] == want["recall"] == hits.sum() / (n * (K - 1)) and m["mIoU"] == want["mIoU"] == hits.sum() / (n * (K - 1))
    with pytest.raises(ValueError, match="more lists than targets"):
        uev.eval_step_alignment(model, index, batches, targets[:7], gt_start[:7], gt_len[:7], (lmin, lmax))
    with pytest.raises(ValueError, match="lists of 33 steps"):
        index.align_vectors(torch.zeros(1, 33, H, device=DEV), [1], [[0]], (1, 1))
