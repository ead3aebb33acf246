"""Moment search: the window-norm and localisation kernels (csrc/moment.hip: univl_window_norms, univl_moment_localize),
VideoIndex.localize / search_moments and eval.eval_localization.

A  fp64 parity on LayerNorm-scale frames and unit queries (tests/moment_ref.py), both modes, at the project's fp32 gate 2e-4: scores
   and table entries everywhere, start / length wherever the reference's best two windows differ by more than the gate;
B  exact arithmetic (small integers, use_mil, window lengths that are powers of two): bit-equal scores, equal windows, constructed ties;
C  masks: none valid, a valid prefix shorter than lmin, a hole, a single valid frame;
D  candidates outside the gallery and duplicated candidates;
E  purity: a pair's triple does not depend on its place in the launch, on the other pairs or on deterministic mode, a table row not on
   the rows computed with it;
F  every argument the entry points refuse;
G  through the model: against get_similarity_logits with the mask narrowed to one window, against search() on the whole video, the
   lazily filled table across index growth, search_moments against the brute force, eval_localization on planted ground truth."""
import ctypes as C

import numpy as np
import pytest
import torch

from make_golden import case_config

import moment_ref as R
from retrieval_cases import batches as _batches, deterministic_models  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import univl_amd
    from univl_amd import _lib, ops
    from univl_amd import eval as uev
    from test_model_gpu import build

DEV = "cuda"
H = 768
TOL = 2e-4                       # tests/test_retrieve_gpu.py: the project's fp32 score tolerance
NEG_INF = float("-inf")


def _dev(frames, mask, q, rows):
    return (torch.from_numpy(np.ascontiguousarray(frames)).float().to(DEV), torch.from_numpy(np.ascontiguousarray(mask)).long().to(DEV),
            torch.from_numpy(np.ascontiguousarray(q)).float().to(DEV), torch.from_numpy(np.ascontiguousarray(rows)).int().to(DEV))


def _host(out):
    start, length, score = out
    return start.cpu().numpy().astype(np.int64), length.cpu().numpy().astype(np.int64), score.cpu().numpy()


def _localize(frames, mask, q, rows, lmin, lmax, normalize, wnorm=None):
    if normalize and wnorm is None:
        wnorm = ops.window_norms(frames, mask)
    return _host(ops.moment_localize(q, frames, mask, rows, lmin, lmax, wnorm=wnorm, normalize=normalize))


def _check_against(got, ref, q, frames, mask, rows, normalize, tol):
    """got: the kernel's (start, length, score); ref: moment_ref.localize's four arrays.  Empty pairs agree exactly, scores within tol,
    windows equal where the reference's margin exceeds tol; elsewhere the window chosen scores, in float64, within tol of the best.
    Returns (max score error, pairs left undecided)."""
    start, length, score = got
    r_start, r_length, r_score, margin = ref
    none = r_start < 0
    assert np.array_equal(start < 0, none)
    assert np.all(start[none] == -1) and np.all(length[none] == 0) and np.all(score[none] == NEG_INF)
    err = float(np.abs(score[~none].astype(np.float64) - r_score[~none]).max()) if (~none).any() else 0.0
    assert err <= tol, err
    decided = ~none & (margin > tol)
    assert np.array_equal(start[decided], r_start[decided]) and np.array_equal(length[decided], r_length[decided])
    undecided = ~none & ~decided
    for i, j in zip(*np.nonzero(undecided)):
        r = int(rows[i, j])
        assert R.is_candidate(mask[r], start[i, j], length[i, j], 1, mask.shape[1])
        assert abs(R.window_score(q[i], frames[r], start[i, j], length[i, j], normalize) - r_score[i, j]) <= tol
    return err, int(undecided.sum())


# ------------------------------------------------------------------------------------------------ A: fp64 parity
@pytest.mark.parametrize("F", R.PARITY_F)
def test_kernels_against_fp64(F):
    """fp32 against the float64 brute force; the largest score error and relative table error of each F are printed (over all of them,
    profiles/moment_search.txt: 5.0e-7 and 1.2e-7).  tests/test_moment_cpu.py checks the share of undecided pairs on the CPU."""
    worst_score = worst_table = 0.0
    for normalize in (True, False):
        undecided = pairs = 0
        for P in R.PARITY_P:
            frames, mask, q, rows = R.parity_case(F, P)
            ref, tables = R.parity_reference(F, P, normalize)
            d_frames, d_mask, d_q, d_rows = _dev(frames, mask, q, rows)
            wnorm = None
            if normalize:
                wnorm = ops.window_norms(d_frames, d_mask)
                t = wnorm.cpu().numpy().astype(np.float64)
                assert np.all(t[tables == 0] == 0)                        # masked windows and the lengths past the row's end: exactly 0
                rel = np.abs(t - tables)[tables > 0] / tables[tables > 0]
                worst_table = max(worst_table, float(rel.max()))
                assert rel.max() <= TOL, (F, P, rel.max())
            for (lmin, lmax), want in ref.items():
                got = _localize(d_frames, d_mask, d_q, d_rows, lmin, lmax, normalize, wnorm)
                err, und = _check_against(got, want, q, frames, mask, rows, normalize, TOL)
                worst_score, undecided, pairs = max(worst_score, err), undecided + und, pairs + P
        assert undecided < R.UNDECIDED_CAP * pairs, (F, normalize, undecided, pairs)
        print("F=%d normalize=%d: %d of %d pairs undecided" % (F, normalize, undecided, pairs))
    print("F=%d: max score error %.3e, max relative table error %.3e" % (F, worst_score, worst_table))


# ------------------------------------------------------------------------------------------------ B: exact arithmetic
def _int_case(F, seed):
    """Integer frames and queries in [-8, 8] (every product sum is an integer below 2^24, exact in fp32 in any order), 7 rows with
    prefix masks; row 5 is one frame repeated, row 6 repeats a block of 3 frames."""
    rng = np.random.RandomState(seed)
    frames = rng.randint(-8, 9, size=(7, F, H)).astype(np.float32)
    frames[5] = frames[5, 0]
    frames[6] = frames[6, np.arange(F) % 3]
    mask = np.zeros((7, F), dtype=np.int64)
    for r, n in enumerate([F, max(1, F // 2), max(1, F - 1), 1, min(F, 9), F, F]):
        mask[r, :n] = 1
    q = rng.randint(-8, 9, size=(5, H)).astype(np.float32)
    rows = np.stack([rng.permutation(7) for _ in range(5)]).astype(np.int32)
    return frames, mask, q, rows


@pytest.mark.parametrize("F", [8, 16, 50, 128])
def test_exact_integer_inputs_use_mil(F):
    frames, mask, q, rows = _int_case(F, 300 + F)
    dev = _dev(frames, mask, q, rows)
    for L in (1, 2, 4, 8):
        start, length, score = _localize(*dev, L, L, False)
        r_start, r_length, r_score, _ = R.localize(q, frames, mask, rows, L, L, False)
        assert np.array_equal(start, r_start) and np.array_equal(length, r_length)
        assert np.array_equal(score, r_score.astype(np.float32))          # sums of integers over a power of two: exact, so bit-equal
        at = rows == 5                                                    # identical frames: every window ties, the first one wins
        assert np.all(start[at] == 0) and np.all(length[at] == L)
        assert np.all(start[rows == 6] < 3)                               # a period of 3: the best window recurs, the first one is reported
    # a range of lengths on the identical frames: the mean does not depend on L, so (0, lmin) wins
    start, length, _ = _localize(*dev, 2, 8, False)
    assert np.all(start[rows == 5] == 0) and np.all(length[rows == 5] == 2)


# ------------------------------------------------------------------------------------------------ C: masks
@pytest.mark.parametrize("normalize", [True, False], ids=["normalize", "use_mil"])
def test_masks(normalize):
    F = 20
    rng = np.random.RandomState(11)
    frames = (rng.standard_normal((5, F, H)) * (28.0 / np.sqrt(H))).astype(np.float32)
    q = rng.standard_normal((3, H))
    q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    mask = np.zeros((5, F), dtype=np.int64)
    mask[1, :3] = 1                                                       # a valid prefix shorter than lmin = 4
    mask[2, :] = 1
    mask[2, 9] = 0                                                        # a hole: windows on both sides, none across
    mask[3, 7] = 1                                                        # a single valid frame, not the first
    mask[4, :] = 1
    rows = np.tile(np.arange(5, dtype=np.int32), (3, 1))
    dev = _dev(frames, mask, q, rows)
    for lmin, lmax in ((4, 6), (1, 1), (1, F), (10, 12)):
        got = _localize(*dev, lmin, lmax, normalize)
        ref = R.localize(q, frames, mask, rows, lmin, lmax, normalize)
        _check_against(got, ref, q, frames, mask, rows, normalize, TOL)
        start, length, score = got
        assert np.all(start[:, 0] == -1) and np.all(length[:, 0] == 0) and np.all(score[:, 0] == NEG_INF)      # nothing valid
        if lmin > 3:
            assert np.all(start[:, 1] == -1)
        assert np.all((start[:, 2] + length[:, 2] <= 9) | (start[:, 2] >= 10))                                   # never across the hole
        if lmin == 1:
            assert np.all(start[:, 3] == 7) and np.all(length[:, 3] == 1)
        else:
            assert np.all(start[:, 3] == -1)
        if lmin == 10:
            assert np.all(start[:, 2] == 10) and np.all(length[:, 2] == 10)                                      # only frames 10 .. 19 hold such a window
    if normalize:
        t = ops.window_norms(dev[0], dev[1]).cpu().numpy()
        assert np.all(t[0] == 0) and np.all(t[1, 3:] == 0) and np.all(t[1, 0, 3:] == 0) and t[1, 0, 2] > 0
        assert np.all(t[2, 9] == 0) and np.all(t[2, 5, 4:] == 0) and t[2, 5, 3] > 0 and t[2, 10, 9] > 0
        assert t[3, 7, 0] > 0 and np.count_nonzero(t[3]) == 1


# ------------------------------------------------------------------------------------------------ D: candidates
def test_candidates_outside_the_gallery_and_duplicates():
    F, N = 16, 4
    rng = np.random.RandomState(12)
    frames = (rng.standard_normal((N, F, H)) * (28.0 / np.sqrt(H))).astype(np.float32)
    q = rng.standard_normal((2, H)).astype(np.float32)
    mask = np.ones((N, F), dtype=np.int64)
    # the gallery is the middle of a larger allocation whose other rows are NaN: a read outside [0, N) would poison the result
    big = torch.full((N + 2, F, H), float("nan"), device=DEV)
    big[1:N + 1] = torch.from_numpy(frames).to(DEV)
    bigmask = torch.ones(N + 2, F, dtype=torch.int64, device=DEV)
    d_frames, d_mask = big[1:N + 1], bigmask[1:N + 1]
    rows = np.array([[2, -1, N, 2, 2 ** 31 - 1, 0, -2 ** 31, 2], [-1, -1, 3, 3, N + 1, 1, 0, -7]], dtype=np.int32)
    d_q, d_rows = torch.from_numpy(q).to(DEV), torch.from_numpy(rows).to(DEV)
    for normalize in (True, False):
        wnorm = ops.window_norms(d_frames, d_mask) if normalize else None
        start, length, score = _host(ops.moment_localize(d_q, d_frames, d_mask, d_rows, 2, 5, wnorm=wnorm, normalize=normalize))
        out = (rows < 0) | (rows >= N)
        assert np.all(start[out] == -1) and np.all(length[out] == 0) and np.all(score[out] == NEG_INF)
        assert np.all(start[~out] >= 0) and np.all(np.isfinite(score[~out]))
        for a, b in (((0, 0), (0, 3)), ((0, 0), (0, 7)), ((1, 2), (1, 3))):                                      # duplicated candidates
            assert (start[a], length[a]) == (start[b], length[b]) and score[a] == score[b]
        _check_against((start, length, score), R.localize(q, frames, mask, rows, 2, 5, normalize), q, frames, mask, rows, normalize, TOL)


# ------------------------------------------------------------------------------------------------ E: purity
def test_purity_position_company_and_deterministic_mode():
    F = 48
    frames, mask, q, _ = R.parity_case(F, 37)
    d_frames, d_mask, d_q, _ = _dev(frames, mask, q, np.zeros((1, 1), dtype=np.int32))
    rng = np.random.RandomState(13)
    rows = torch.from_numpy(rng.randint(0, R.PARITY_ROWS, size=(37, 6)).astype(np.int32)).to(DEV)
    wnorm = ops.window_norms(d_frames, d_mask)
    # the table: all rows in one call, row by row, and a row as part of another set
    for r in range(R.PARITY_ROWS):
        assert torch.equal(ops.window_norms(d_frames[r:r + 1], d_mask[r:r + 1])[0], wnorm[r])
    assert torch.equal(ops.window_norms(d_frames[2:5], d_mask[2:5]), wnorm[2:5])
    was = univl_amd.deterministic()
    try:
        for normalize in (True, False):
            w = wnorm if normalize else None
            univl_amd.set_deterministic(False)
            base = ops.moment_localize(d_q, d_frames, d_mask, rows, 3, 7, wnorm=w, normalize=normalize)
            univl_amd.set_deterministic(True)
            det = ops.moment_localize(d_q, d_frames, d_mask, rows, 3, 7, wnorm=w, normalize=normalize)
            if normalize:
                assert torch.equal(ops.window_norms(d_frames, d_mask), wnorm)
            univl_amd.set_deterministic(False)
            for a, b in zip(base, det):
                assert torch.equal(a, b)
            # pair (i, j) alone, and at another place of another launch (the query rows reversed, the candidates rolled)
            for i, j in ((0, 0), (17, 3), (36, 5)):
                alone = ops.moment_localize(d_q[i:i + 1], d_frames, d_mask, rows[i:i + 1, j:j + 1].contiguous(), 3, 7, wnorm=w, normalize=normalize)
                for a, b in zip(base, alone):
                    assert torch.equal(a[i, j], b[0, 0])
            moved = ops.moment_localize(d_q.flip(0).contiguous(), d_frames, d_mask, rows.flip(0).roll(2, 1).contiguous(), 3, 7, wnorm=w,
                                        normalize=normalize)
            for a, b in zip(base, moved):
                assert torch.equal(a.flip(0).roll(2, 1), b)
    finally:
        univl_amd.set_deterministic(was)


# ------------------------------------------------------------------------------------------------ F: refusals
def _desc(frames, mask, wnorm, q, rows, out, F=None, Hh=H, normalize=1, lmin=1, lmax=2):
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    d = _lib.Moment()
    d.frames, d.ld_row, d.mask, d.wnorm = p(frames), frames.stride(0), p(mask), p(wnorm)
    d.N, d.F, d.H, d.normalize = frames.shape[0], frames.shape[1] if F is None else F, Hh, normalize
    d.q, d.ldq, d.rows, d.Nq, d.K, d.lmin, d.lmax = p(q), q.stride(0), p(rows), rows.shape[0], rows.shape[1], lmin, lmax
    d.start, d.length, d.score = p(out[0]), p(out[1]), p(out[2])
    return d


def test_every_bad_argument_is_refused_with_a_message():
    L = _lib.lib()
    F = 8
    frames, mask = torch.zeros(3, F, H, device=DEV), torch.ones(3, F, dtype=torch.int64, device=DEV)
    big = torch.zeros(3, 129, H, device=DEV)                              # room for the F = 129 descriptor: refused, but nothing dangles
    wnorm = torch.zeros(3, 129, 129, device=DEV)
    q, rows = torch.zeros(4, H + 4, device=DEV)[:, :H], torch.zeros(4, 2, dtype=torch.int32, device=DEV)
    out = (torch.zeros(4, 2, dtype=torch.int32, device=DEV), torch.zeros(4, 2, dtype=torch.int32, device=DEV), torch.zeros(4, 2, device=DEV))
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    good = lambda **kw: _desc(kw.pop("frames", frames), mask, wnorm, q, rows, out, **kw)
    fns = {"univl_window_norms": L.univl_window_norms, "univl_moment_localize": L.univl_moment_localize}
    for fn in fns.values():
        assert fn(C.byref(good()), stream) == 0
    assert L.univl_moment_localize(C.byref(good(normalize=0)), stream) == 0
    d = good(normalize=0); d.wnorm = None
    assert L.univl_moment_localize(C.byref(d), stream) == 0               # use_mil needs no table
    # case -> (entry points, descriptor, status, words only that case's message holds)
    both, loc = tuple(fns), ("univl_moment_localize",)
    bad = {"F = 129": (both, good(frames=big), -1, b"F=129"), "F = 0": (both, good(F=0), -1, b"F=0"), "H != 768": (both, good(Hh=512), -1, b"H=512"),
           "normalize": (both, good(normalize=2), -1, b"normalize=2"),
           "lmin = 0": (loc, good(lmin=0), -1, b"lmin=0"), "lmin > lmax": (loc, good(lmin=3, lmax=2), -1, b"lmin=3 lmax=2"),
           "lmax > F": (loc, good(lmax=F + 1), -1, b"lmax=9")}
    for name, field, who, word in (("null frames", "frames", both, b"(frames, mask)"), ("null mask", "mask", both, b"(frames, mask)"),
                                   ("null wnorm", "wnorm", both, b"wnorm"), ("null q", "q", loc, b"(q, rows"),
                                   ("null rows", "rows", loc, b"(q, rows"), ("null start", "start", loc, b"(q, rows"),
                                   ("null length", "length", loc, b"(q, rows"), ("null score", "score", loc, b"(q, rows")):
        d = good()
        setattr(d, field, None)
        bad[name] = (who, d, -1, word)
    d = good(); d.N = 0; bad["N < 1"] = (both, d, -1, b"N=0")
    d = good(); d.Nq = 0; bad["Nq < 1"] = (loc, d, -1, b"Nq=0")
    d = good(); d.K = 0; bad["K < 1"] = (loc, d, -1, b"K=0")
    d = good(); d.ld_row = F * H - 4; bad["ld_row < F * 768"] = (both, d, -1, b"ld_row=6140")
    d = good(); d.ldq = 764; bad["ldq < 768"] = (loc, d, -1, b"ldq=764")
    d = good(); d.frames = C.c_void_p(frames.data_ptr() + 4); bad["misaligned frames"] = (both, d, -2, b"rows of frames")
    d = good(); d.ld_row = F * H + 2; bad["misaligned gallery rows"] = (both, d, -2, b"rows of frames")
    d = good(); d.q = C.c_void_p(q.data_ptr() + 4); bad["misaligned q"] = (loc, d, -2, b"rows of q")
    d = good(); d.ldq = H + 2; bad["misaligned query rows"] = (loc, d, -2, b"rows of q")
    for name, (who, d, status, word) in bad.items():
        for w in who:
            assert fns[w](C.byref(good()), stream) == 0                   # a good call in between: no message is left over
            rc = fns[w](C.byref(d), stream)
            assert rc == status, (name, w, rc)                            # UNIVL_EINVAL / UNIVL_EALIGN
            msg = L.univl_last_error()
            assert w.encode() in msg and word in msg, (name, w, msg)
    assert L.univl_window_norms(None, stream) == -1 and L.univl_moment_localize(None, stream) == -1
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="needs wnorm"):
        ops.moment_localize(q, frames, mask, rows, 1, 2)
    with pytest.raises(RuntimeError, match="lmin=5"):
        ops.moment_localize(q, frames, mask, rows, 5, 4, normalize=False)


# ------------------------------------------------------------------------------------------------ G: through the model
def _index(model, bs, **kw):
    from univl_amd.retrieval import VideoIndex
    index = VideoIndex(model, keep_frames=True, **kw)
    for b in bs:
        index.add(b["video"], b["video_mask"])
    return index


def _valid(index):
    return index._fmask[:len(index)].sum(1).cpu().numpy()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_localize_against_the_public_path_and_the_whole_video_search(dtype, deterministic_models):
    from test_model_gpu import GATES
    cfg, rows, dseed = case_config("joint_small")
    model, _ = build(cfg, dtype)
    model.eval()
    bs = _batches(cfg, [3, 3], dseed)
    cat = {k: torch.cat([b[k] for b in bs]) for k in bs[0]}
    text = (cat["input_ids"], cat["token_type_ids"], cat["attention_mask"])
    tol = TOL if dtype == torch.float32 else GATES[torch.bfloat16]["sim"]
    n, F = 6, cfg.max_frames

    # whole-video consistency: the one window that covers the valid frames scores what search() scores the row
    index = _index(model, bs, capacity=8)
    lv = _valid(index)
    score, idx = index.search(*text, k=n)
    full = torch.empty(n, n, device=DEV).scatter_(1, idx.long(), score)
    for j in range(n):
        s, l, sc = index.localize(*text, torch.full((n, 1), j, dtype=torch.int32), (int(lv[j]), int(lv[j])))
        assert torch.all(s == 0) and torch.all(l == int(lv[j]))
        assert float((sc[:, 0] - full[:, j]).abs().max()) <= tol

    # one window per video, isolated by the mask: get_similarity_logits with the video mask narrowed to it
    q, so, am = index.pool_text(*text)
    vo = index._frames[:n].clone()
    windows = [(int(v) // 3, max(1, (int(v) - int(v) // 3) // 2)) for v in lv]
    wmask = torch.zeros(n, F, dtype=torch.int64, device=DEV)
    for j, (s0, L0) in enumerate(windows):
        wmask[j, s0:s0 + L0] = 1
    want = model.get_similarity_logits(so, vo, am, wmask)
    forced = _index(model, bs, capacity=8)
    forced._fmask[:n].copy_(wmask)                                        # before the first localisation: the table is built from this mask
    for j, (s0, L0) in enumerate(windows):
        s, l, sc = forced.localize(*text, torch.full((n, 1), j, dtype=torch.int32), (L0, L0))
        assert torch.all(s == s0) and torch.all(l == L0), (j, s0, L0)
        assert float((sc[:, 0] - want[:, j]).abs().max()) <= tol, (j, s0, L0)


def test_lazy_norms_growth_search_moments_and_eval_localization(deterministic_models):
    from univl_amd.retrieval import QueryBank, VideoIndex
    cfg, rows, dseed = case_config("joint_small")
    model, _ = build(cfg, torch.float32)
    model.eval()
    bs = _batches(cfg, [3, 3, 2], dseed)
    cat = {k: torch.cat([b[k] for b in bs]) for k in bs[0]}
    text = (cat["input_ids"], cat["token_type_ids"], cat["attention_mask"])
    F = cfg.max_frames

    # 3 + 3 + 2 rows into a capacity of 4: the table is filled lazily and survives the growth bit for bit
    index = VideoIndex(model, capacity=4, keep_frames=True)
    index.add(bs[0]["video"], bs[0]["video_mask"])
    assert index._wnorm is None and index._wnorm_rows == 0
    text3 = tuple(t[:3] for t in text)
    first = index.localize(*text3, torch.arange(3, dtype=torch.int32).repeat(3, 1), (1, 3))
    assert index._wnorm_rows == 3 and index._wnorm.shape == (4, F, F)
    kept = index._wnorm[:3].clone()
    index.add(bs[1]["video"], bs[1]["video_mask"])
    assert index._wnorm.shape == (8, F, F) and index._wnorm_rows == 3 and torch.equal(index._wnorm[:3], kept)
    index.add(bs[2]["video"], bs[2]["video_mask"])
    again = index.localize(*text3, torch.arange(3, dtype=torch.int32).repeat(3, 1), (1, 3))
    assert index._wnorm_rows == 8 == len(index) and torch.equal(index._wnorm[:3], kept)
    assert torch.equal(index._wnorm[:8], ops.window_norms(index._frames[:8], index._fmask[:8]))
    for a, b in zip(first, again):
        assert torch.equal(a, b)

    # search_moments over the whole index against the brute force on the kernel's own frames
    lv = _valid(index)
    lmin = int(lv.min()) + 1                                              # at least one video is too short for any window
    lmax = min(lmin + 2, F)
    assert (lv >= lmin).any() and (lv < lmin).any()
    q = index.pool_text(*text)[0]
    frames, mask, qh = index._frames[:8].cpu().numpy(), index._fmask[:8].cpu().numpy(), q.cpu().numpy()
    all_rows = np.tile(np.arange(8), (8, 1))
    r_start, r_length, r_score, _ = R.localize(qh, frames, mask, all_rows, lmin, lmax, True)
    k = 6
    score, idx, start, length = (t.cpu().numpy() for t in index.search_moments(*text, k=k, window=(lmin, lmax), shortlist=8))
    n_ok = int((lv >= lmin).sum())
    for i in range(8):
        assert len(set(idx[i].tolist())) == k and idx[i].min() >= 0 and idx[i].max() < 8
        assert np.all(score[i, 1:] <= score[i, :-1])
        m = min(k, n_ok)
        got64 = r_score[i, idx[i, :m]]
        assert np.abs(score[i, :m] - got64).max() <= TOL
        for j in range(m):                                                # the window reported scores, in float64, what the best one does
            assert abs(R.window_score(qh[i], frames[idx[i, j]], start[i, j], length[i, j], True) - got64[j]) <= TOL
        assert got64[m - 1] >= -np.sort(-r_score[i])[m - 1] - 2 * TOL     # tolerant at near-ties, as the top-k check of the search is
        if m == k:
            exact = R.rank_moments(np.arange(8), r_score[i], k + 1)
            if k < n_ok and np.all(-np.diff(r_score[i, exact]) > 2 * TOL):     # no near-tie among the first k + 1: the order is decided
                assert np.array_equal(idx[i], exact[:k])
        # videos without a candidate window come last, by row id
        empty = np.nonzero(lv < lmin)[0]
        assert np.array_equal(idx[i, m:], empty[:k - m]) and np.all(start[i, m:] == -1) and np.all(length[i, m:] == 0)
        assert np.all(score[i, m:] == NEG_INF)
    # a shortlist shorter than the index re-orders the whole-video top of the list
    s2, i2, st2, l2 = index.search_moments(*text, k=2, window=(1, 2), shortlist=4)
    _, top4 = index.search(*text, k=4)
    assert s2.shape == i2.shape == st2.shape == l2.shape == (8, 2) and i2.dtype == torch.int32
    assert all(set(i2[i].tolist()) <= set(top4[i].tolist()) for i in range(8))
    # the bank path runs
    bank = QueryBank(index, beta=20.0)
    bank.add(*text)
    bank.fit()
    s3, i3, st3, l3 = index.search_moments(*text, k=3, window=(1, 2), bank=bank)
    assert s3.shape == (8, 3) and int(i3.min()) >= 0 and torch.all(l3 >= 1) and torch.all(st3 >= 0)
    with pytest.raises(ValueError):
        VideoIndex(model, capacity=4).search_moments(*text, k=2, window=(1, 2))
    with pytest.raises(ValueError):
        index.localize(*text, torch.zeros(8, 1, dtype=torch.int32), (0, 2))

    # eval_localization: every text in its own video; even texts are annotated with the window found (IoU 1), odd ones with a segment
    # that begins where it ends (IoU 0); the texts of the short videos have no window at all
    targets = np.arange(8)
    f_start, f_length, _ = _host(index.localize(*text, torch.arange(8, dtype=torch.int32).reshape(8, 1), (lmin, lmax)))
    f_start, f_length = f_start[:, 0], f_length[:, 0]
    even = np.arange(8) % 2 == 0
    found = f_length > 0
    gt_start = np.where(found & even, f_start, np.where(found, f_start + f_length, 0))
    gt_len = np.where(found & even, f_length, 2)
    tb = [(b["input_ids"], b["attention_mask"], b["token_type_ids"]) for b in bs]
    m = uev.eval_localization(model, index, tb, targets, gt_start, gt_len, (lmin, lmax))
    hits = int((found & even).sum())
    assert m["n"] == 8 and m["n_empty"] == int((lv < lmin).sum()) == int((~found).sum()) and m["n_empty"] >= 1
    assert m["R1@0.3"] == m["R1@0.5"] == m["R1@0.7"] == hits / 8 and m["mIoU"] == hits / 8
    assert m == R.iou_counts(f_start, f_length, gt_start, gt_len)
    # exact threshold hits: a found window of length L annotated as twice as long from its start has IoU exactly 0.5
    m2 = uev.eval_localization(model, index, tb, targets, np.where(found, f_start, 0), np.where(found, 2 * f_length, 1), (lmin, lmax))
    n_found = int(found.sum())
    assert m2["R1@0.3"] == m2["R1@0.5"] == n_found / 8 and m2["R1@0.7"] == 0.0 and m2["mIoU"] == 0.5 * n_found / 8
    assert m2 == R.iou_counts(f_start, f_length, np.where(found, f_start, 0), np.where(found, 2 * f_length, 1))


def test_every_buffer_of_one_index_grows_in_the_same_run(deterministic_models):
    """Vectors, frames, masks, the window-norm table and the bank's column terms all outgrow their buffers between two uses (capacity
    2 -> 4 -> 8 in one add, the table and c partly filled); every result equals, bit for bit, the same five videos in an index that
    never grew, under a fresh fit."""
    from univl_amd.retrieval import QueryBank, VideoIndex
    cfg, rows, dseed = case_config("joint_small")
    model, _ = build(cfg, torch.float32)
    model.eval()
    bs = _batches(cfg, [2, 3], dseed)
    cat = {k: torch.cat([b[k] for b in bs]) for k in bs[0]}
    text = (cat["input_ids"], cat["token_type_ids"], cat["attention_mask"])
    bank_text = (bs[1]["input_ids"], bs[1]["token_type_ids"], bs[1]["attention_mask"])          # 3 texts
    F, W = cfg.max_frames, (1, min(3, cfg.max_frames))

    def grown(capacity, stop_after_first):
        index = VideoIndex(model, capacity=capacity, keep_frames=True)
        bank = QueryBank(index, beta=20.0, hub_k=2)
        bank.add(*bank_text)
        index.add(bs[0]["video"], bs[0]["video_mask"])
        if stop_after_first:
            bank.fit()
            short = index.search_moments(*text, k=5, window=W, shortlist=5, bank=bank)      # a gallery of 2: three empty slots per row
            assert index._cap == 2 and index._wnorm.shape == (2, F, F) and index._wnorm_rows == 2 and bank._c.numel() == 2
            assert torch.all(short[1][:, 2:] == -1) and torch.all(short[0][:, 2:] == NEG_INF)
        index.add(bs[1]["video"], bs[1]["video_mask"])
        if stop_after_first:
            assert index._cap == 8 and index._wnorm.shape == (8, F, F) and index._wnorm_rows == 2 and bank._covered == 2
            assert index._buf.shape[0] == index._frames.shape[0] == index._fmask.shape[0] == 8
        bank.fit()
        out = index.search_moments(*text, k=5, window=W, shortlist=5, bank=bank)
        assert index._wnorm_rows == 5 and bank._c.numel() == 8 and bank._covered == 5
        return out, bank.c.clone(), bank.hub.clone()

    (got, c, hub), (want, c0, hub0) = grown(2, True), grown(8, False)
    for a, b in zip(got, want):                                           # scores, ids, starts, lengths
        assert a.shape == (5, 5) and torch.equal(a, b)
    assert c.shape == (5,) and torch.equal(c, c0) and torch.equal(hub, hub0)
    assert int(got[1].min()) >= 0 and sorted(got[1][0].tolist()) == [0, 1, 2, 3, 4]
