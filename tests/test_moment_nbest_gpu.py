"""N-best moment search with temporal non-maximum suppression on the device (csrc/moment.hip: univl_moment_nbest; ops.moment_nbest;
VideoIndex.localize(n_best=), search_moments(per_video=); eval.eval_localization(n_best=)).

A  fp64 parity WITHOUT comparing a window position under a tolerance: every slot of every pair is judged by the properties of
   moment_nbest_ref.check_nbest, which are stated relative to the kernel's own earlier picks -- a near-tie may change which valid
   greedy run is taken but cannot excuse a wrong one, so no pair is left out; gate 2e-4, the project's gate for this score;
B  slot 0, and M = 1, against ops.moment_localize bit for bit at every parity case;
C  exact arithmetic (small integers, use_mil): element for element and bit for bit against the literal greedy reference, constructed
   ties, identical frames, (1, 1) against the plain sorted top-M, (0, 1) disjoint and running out before M, the whole score buffer;
D  masks: none valid, a prefix shorter than lmin, a hole, one valid frame;
E  row ids outside a gallery whose neighbours are NaN;
F  purity: alone, moved, deterministic mode, other K and Nq, M = 5 is the first five slots of M = 16;
G  every refusal of the C entry point;
H  through the model in fp32 and bf16, and one captured graph replayed on new queries."""
import ctypes as C

import numpy as np
import pytest
import torch

from make_golden import case_config

import moment_ref as R
import moment_nbest_ref as NR
from retrieval_cases import batches as _batches, deterministic_models  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import univl_amd
    from univl_amd import _lib, ops
    from univl_amd import eval as uev
    from test_model_gpu import build

DEV = "cuda"
H = 768
TOL = 2e-4                       # tests/test_retrieve_gpu.py: the project's fp32 score tolerance (profiles/moment_search.txt measured 5e-7)
NEG_INF = float("-inf")


def _dev(frames, mask, q, rows):
    return (torch.from_numpy(np.ascontiguousarray(frames)).float().to(DEV), torch.from_numpy(np.ascontiguousarray(mask)).long().to(DEV),
            torch.from_numpy(np.ascontiguousarray(q)).float().to(DEV), torch.from_numpy(np.ascontiguousarray(rows)).int().to(DEV))


def _host(out):
    start, length, score = out
    return start.cpu().numpy().astype(np.int64), length.cpu().numpy().astype(np.int64), score.cpu().numpy()


def _nbest(frames, mask, q, rows, lmin, lmax, M, nms, normalize, wnorm=None):
    if normalize and wnorm is None:
        wnorm = ops.window_norms(frames, mask)
    out = ops.moment_nbest(q, frames, mask, rows, lmin, lmax, M, nms, wnorm=wnorm, normalize=normalize)
    assert all(t.shape == (rows.shape[0], rows.shape[1], M) for t in out)
    assert out[0].dtype == out[1].dtype == torch.int32 and out[2].dtype == torch.float32
    return _host(out)


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


def _check_pairs(got, scores_of, rows, lmin, lmax, nms, tol):
    """check_nbest for every pair of a launch.  scores_of(i, r): the float64 [F, F] scores of query i in gallery row r, None outside."""
    worst = 0.0
    for i, j in np.ndindex(*rows.shape):
        S = scores_of(i, int(rows[i, j]))
        worst = max(worst, NR.check_nbest(got[0][i, j], got[1][i, j], got[2][i, j], S, lmin, lmax, nms[0], nms[1], tol))
    return worst


# ------------------------------------------------------------------------------------------------ A: fp64 parity by properties
@pytest.mark.parametrize("normalize", [True, False], ids=["normalize", "use_mil"])
@pytest.mark.parametrize("F", R.PARITY_F)
def test_kernel_against_fp64_by_properties(F, normalize):
    worst = 0.0
    pairs = empty_slots = 0
    for P in R.PARITY_P:
        frames, mask, q, rows = R.parity_case(F, P)
        scores = NR.parity_scores(F, P, normalize)
        dev = _dev(frames, mask, q, rows)
        wnorm = ops.window_norms(dev[0], dev[1]) if normalize else None
        for lmin, lmax in R.parity_windows(F):
            for M, nms in NR.CONFIGS:
                got = _nbest(*dev, lmin, lmax, M, nms, normalize, wnorm)
                worst = max(worst, _check_pairs(got, lambda i, r: scores[r][i], rows, lmin, lmax, nms, TOL))
                pairs += P
                empty_slots += int((got[1] == 0).sum())
    assert pairs == sum(R.PARITY_P) * len(R.parity_windows(F)) * len(NR.CONFIGS)              # no pair is left out
    print("F=%d normalize=%d: %d pairs, %d empty slots, max score error %.3e" % (F, normalize, pairs, empty_slots, worst))


# ------------------------------------------------------------------------------------------------ B: slot 0 and M = 1
@pytest.mark.parametrize("F", R.PARITY_F)
def test_slot_0_and_m_1_are_moment_localize_bit_for_bit(F):
    for normalize in (True, False):
        for P in R.PARITY_P:
            dev = _dev(*R.parity_case(F, P))
            wnorm = ops.window_norms(dev[0], dev[1]) if normalize else None
            for lmin, lmax in R.parity_windows(F):
                loc = _host(ops.moment_localize(dev[2], dev[0], dev[1], dev[3], lmin, lmax, wnorm=wnorm, normalize=normalize))
                for M, nms in NR.CONFIGS:
                    got = _nbest(*dev, lmin, lmax, M, nms, normalize, wnorm)
                    assert np.array_equal(got[0][:, :, 0], loc[0]) and np.array_equal(got[1][:, :, 0], loc[1]), (F, P, lmin, lmax, M, nms)
                    assert np.array_equal(_bits(got[2][:, :, 0]), _bits(loc[2])), (F, P, lmin, lmax, M, nms)


# ------------------------------------------------------------------------------------------------ C: exact arithmetic
EXACT_CONFIGS = ((16, (1, 2)), (16, (1, 1)), (16, (0, 1)), (5, (7, 10)), (1, (1, 2)))


@pytest.mark.parametrize("F", [1, 8, 50, 128])
def test_exact_integer_inputs_use_mil_element_for_element(F):
    """Integer frames and queries under use_mil: every numerator is an integer below 2^24 and every score one correctly rounded fp32
    division (moment_nbest_ref.exact_scores), so the kernel's slots equal the literal greedy reference's in every element and bit.
    Window (1, F) at F = 128 fills the whole score buffer; row 5 is one frame repeated, row 6 a period of three frames."""
    frames, mask, q, rows = NR.int_case(F, 300 + F)
    dev = _dev(frames, mask, q, rows)
    S = {r: NR.exact_scores(q, frames[r], mask[r]) for r in range(7)}
    ran_out = ties = 0
    for lmin, lmax in sorted({(1, F), (min(2, F), min(8, F)), (F, F)}):
        for M, (num, den) in EXACT_CONFIGS:
            got = _nbest(*dev, lmin, lmax, M, (num, den), False)
            for i, j in np.ndindex(*rows.shape):
                r = int(rows[i, j])
                want = NR.nbest_greedy(S[r][i], lmin, lmax, M, num, den)
                assert np.array_equal(got[0][i, j], want[0]) and np.array_equal(got[1][i, j], want[1]), (F, lmin, lmax, M, num, den, i, r)
                assert np.array_equal(_bits(got[2][i, j]), _bits(want[2])), (F, lmin, lmax, M, num, den, i, r)
                n = int((want[1] > 0).sum())
                ties += int(n > 1 and np.any(np.diff(want[2][:n]) == 0))
                if num == den:                                            # nothing suppressed but the pick: the plain sorted top-M
                    plain = NR.top_plain(S[r][i], lmin, lmax, M)
                    assert np.array_equal(got[0][i, j], plain[0]) and np.array_equal(got[1][i, j], plain[1])
                if num == 0:                                              # pairwise disjoint, and they may run out before M
                    cover = [f for s, L in zip(got[0][i, j][:n], got[1][i, j][:n]) for f in range(s, s + L)]
                    assert len(cover) == len(set(cover))
                    ran_out += int(n < M)
            at = rows == 5                                                # identical frames: every window ties, ORDER alone decides
            n5 = min(M, lmax - lmin + 1)
            if (num, den) == (1, 1):
                assert np.all(got[0][at][:, :n5] == 0) and np.all(got[1][at][:, :n5] == np.arange(lmin, lmin + n5))
            if num == 0:
                k = min(M, F // lmin)
                assert np.all(got[0][at][:, :k] == lmin * np.arange(k)) and np.all(got[1][at][:, :k] == lmin)
    assert ran_out > 0 and (ties > 0 or F == 1)


# ------------------------------------------------------------------------------------------------ D: masks
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
    S = {r: R.row_scores(q, frames[r], mask[r], normalize)[0] for r in range(5)}
    for lmin, lmax in ((4, 6), (1, 1), (1, F), (10, 12)):
        for M, nms in ((16, (0, 1)), (5, (1, 2)), (16, (1, 1))):
            start, length, score = got = _nbest(*dev, lmin, lmax, M, nms, normalize)
            _check_pairs(got, lambda i, r: S[r][i], rows, lmin, lmax, nms, TOL)
            assert np.all(start[:, 0] == -1) and np.all(length[:, 0] == 0) and np.all(score[:, 0] == NEG_INF)      # nothing valid
            if lmin > 3:
                assert np.all(start[:, 1] == -1) and np.all(length[:, 1] == 0)
            on = length[:, 2] > 0
            s2, e2 = start[:, 2][on], (start[:, 2] + length[:, 2])[on]
            assert np.all((e2 <= 9) | (s2 >= 10))                         # never across the hole ...
            if nms == (0, 1):                                             # ... and the windows beside it survive: both sides are used
                for i in range(3):
                    left = np.any((length[i, 2] > 0) & (start[i, 2] + length[i, 2] <= 9))
                    right = np.any((length[i, 2] > 0) & (start[i, 2] >= 10))
                    assert right and (left or lmin > 9), (lmin, lmax, i)
            if lmin == 1:                                                 # one valid frame: one window, then nothing
                assert np.all(start[:, 3, 0] == 7) and np.all(length[:, 3, 0] == 1)
                assert np.all(start[:, 3, 1:] == -1) and np.all(length[:, 3, 1:] == 0) and np.all(score[:, 3, 1:] == NEG_INF)
            else:
                assert np.all(start[:, 3] == -1)
            if lmin == 10:                                                # only frames 10 .. 19 hold such a window: exactly one
                assert np.all(start[:, 2, 0] == 10) and np.all(length[:, 2, 0] == 10) and np.all(length[:, 2, 1:] == 0)


# ------------------------------------------------------------------------------------------------ E: out of range
def test_rows_outside_the_gallery_are_empty_in_every_slot_and_read_nothing():
    F, N, M = 16, 4, 5
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
        S = {r: R.row_scores(q, frames[r], mask[r], normalize)[0] for r in range(N)}
        got = _nbest(d_frames, d_mask, d_q, d_rows, 2, 5, M, (1, 2), normalize)
        start, length, score = got
        out = (rows < 0) | (rows >= N)
        assert np.all(start[out] == -1) and np.all(length[out] == 0) and np.all(score[out] == NEG_INF)
        assert np.all(start[~out] >= 0) and np.all(np.isfinite(score[~out]))
        _check_pairs(got, lambda i, r: S[r][i] if 0 <= r < N else None, rows, 2, 5, (1, 2), TOL)
        for a, b in (((0, 0), (0, 3)), ((0, 0), (0, 7)), ((1, 2), (1, 3))):                                      # duplicated candidates
            assert all(np.array_equal(x[a], x[b]) for x in got)


# ------------------------------------------------------------------------------------------------ F: purity
def test_purity_position_company_shape_deterministic_mode_and_m():
    F, W, M, NMS = 48, (3, 7), 16, (1, 2)
    frames, mask, q, _ = R.parity_case(F, 37)
    d_frames, d_mask, d_q, _ = _dev(frames, mask, q, np.zeros((1, 1), dtype=np.int32))
    rng = np.random.RandomState(13)
    rows = torch.from_numpy(rng.randint(0, R.PARITY_ROWS, size=(37, 6)).astype(np.int32)).to(DEV)
    wnorm = ops.window_norms(d_frames, d_mask)
    was = univl_amd.deterministic()
    try:
        for normalize in (True, False):
            kw = {"wnorm": wnorm if normalize else None, "normalize": normalize}
            run = lambda qq, rr, m=M, nms=NMS: ops.moment_nbest(qq, d_frames, d_mask, rr, W[0], W[1], m, nms, **kw)
            univl_amd.set_deterministic(False)
            base = run(d_q, rows)
            univl_amd.set_deterministic(True)
            det = run(d_q, rows)
            univl_amd.set_deterministic(False)
            for a, b in zip(base, det):
                assert torch.equal(a, b)
            for i, j in ((0, 0), (17, 3), (36, 5)):
                alone = run(d_q[i:i + 1], rows[i:i + 1, j:j + 1].contiguous())                  # Nq = K = 1
                for a, b in zip(base, alone):
                    assert torch.equal(a[i, j], b[0, 0])
                row = run(d_q[i:i + 1], rows[i:i + 1].contiguous())                             # Nq = 1, K = 6
                wide = run(d_q[i:i + 1], rows[i:i + 1, j:j + 1].repeat(1, 11).contiguous())     # K = 11, the pair in every place
                for a, b, c in zip(base, row, wide):
                    assert torch.equal(a[i], b[0]) and all(torch.equal(a[i, j], c[0, k]) for k in range(11))
            moved = run(d_q.flip(0).contiguous(), rows.flip(0).roll(2, 1).contiguous())
            for a, b in zip(base, moved):
                assert torch.equal(a.flip(0).roll(2, 1), b)
            # the first slots do not depend on M, under either threshold
            for nms in (NMS, (0, 1)):
                full = run(d_q, rows, 16, nms)
                for m in (1, 5):
                    for a, b in zip(full, run(d_q, rows, m, nms)):
                        assert torch.equal(a[:, :, :m], b)
    finally:
        univl_amd.set_deterministic(was)


# ------------------------------------------------------------------------------------------------ G: refusals
def _desc(frames, mask, wnorm, q, rows, out, F=None, normalize=1, lmin=1, lmax=2, M=3, num=1, den=2):
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    d = _lib.MomentNbest()
    d.frames, d.ld_row, d.mask, d.wnorm = p(frames), frames.stride(0), p(mask), p(wnorm)
    d.N, d.F, d.H, d.normalize = frames.shape[0], frames.shape[1] if F is None else F, H, normalize
    d.q, d.ldq, d.rows, d.Nq, d.K, d.lmin, d.lmax = p(q), q.stride(0), p(rows), rows.shape[0], rows.shape[1], lmin, lmax
    d.M, d.iou_num, d.iou_den = M, num, den
    d.start, d.length, d.score = p(out[0]), p(out[1]), p(out[2])
    return d


def test_every_bad_argument_is_refused_with_a_message():
    L = _lib.lib()
    F = 8
    frames, mask = torch.zeros(3, F, H, device=DEV), torch.ones(3, F, dtype=torch.int64, device=DEV)
    wnorm = torch.zeros(3, F, F, device=DEV)
    q, rows = torch.zeros(4, H + 4, device=DEV)[:, :H], torch.zeros(4, 2, dtype=torch.int32, device=DEV)
    out = (torch.zeros(4, 2, 16, dtype=torch.int32, device=DEV), torch.zeros(4, 2, 16, dtype=torch.int32, device=DEV),
           torch.zeros(4, 2, 16, device=DEV))
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    good = lambda **kw: _desc(frames, mask, wnorm, q, rows, out, **kw)
    fn = L.univl_moment_nbest
    for kw in ({}, {"M": 1}, {"M": 16}, {"num": 0, "den": 1}, {"num": 1024, "den": 1024}, {"num": 0, "den": 1024}, {"normalize": 0}):
        assert fn(C.byref(good(**kw)), stream) == 0, kw
    d = good(normalize=0); d.wnorm = None
    assert fn(C.byref(d), stream) == 0                                    # use_mil needs no table
    # case -> (descriptor, status, words only that case's message holds)
    bad = {"M = 0": (good(M=0), -1, b"M=0"), "M = 17": (good(M=17), -1, b"M=17"),
           "iou_den = 0": (good(den=0, num=0), -1, b"iou_den=0"), "iou_den = 1025": (good(den=1025), -1, b"iou_den=1025"),
           "iou_num = -1": (good(num=-1), -1, b"iou_num=-1"), "iou_num = den + 1": (good(num=3, den=2), -1, b"iou_num=3"),
           "lmin = 0": (good(lmin=0), -1, b"lmin=0"), "lmax > F": (good(lmax=F + 1), -1, b"lmax=9"), "F = 0": (good(F=0), -1, b"F=0"),
           "normalize": (good(normalize=2), -1, b"normalize=2")}
    for name, field, word in (("null start", "start", b"(q, rows"), ("null length", "length", b"(q, rows"), ("null score", "score", b"(q, rows"),
                              ("null q", "q", b"(q, rows"), ("null rows", "rows", b"(q, rows"), ("null wnorm", "wnorm", b"wnorm"),
                              ("null frames", "frames", b"(frames, mask)")):
        d = good()
        setattr(d, field, None)
        bad[name] = (d, -1, word)
    d = good(); d.Nq = 0; bad["Nq < 1"] = (d, -1, b"Nq=0")
    d = good(); d.K = 0; bad["K < 1"] = (d, -1, b"K=0")
    d = good(); d.ldq = 764; bad["ldq < 768"] = (d, -1, b"ldq=764")
    d = good(); d.q = C.c_void_p(q.data_ptr() + 4); bad["misaligned q"] = (d, -2, b"rows of q")
    d = good(); d.ldq = H + 2; bad["misaligned query rows"] = (d, -2, b"rows of q")
    d = good(); d.frames = C.c_void_p(frames.data_ptr() + 4); bad["misaligned frames"] = (d, -2, b"rows of frames")
    for name, (d, status, word) in bad.items():
        assert fn(C.byref(good()), stream) == 0                           # a good call in between: no message is left over
        rc = fn(C.byref(d), stream)
        assert rc == status, (name, rc)                                   # UNIVL_EINVAL / UNIVL_EALIGN
        msg = L.univl_last_error()
        assert b"univl_moment_nbest" in msg and word in msg, (name, msg)
    assert fn(None, stream) == -1
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="needs wnorm"):
        ops.moment_nbest(q, frames, mask, rows, 1, 2, 3)
    for n_best, nms, word in ((0, (1, 2), "M=0"), (17, (1, 2), "M=17"), (3, (1, 0), "iou_den=0"), (3, (3, 2), "iou_num=3")):
        with pytest.raises(RuntimeError, match=word):
            ops.moment_nbest(q, frames, mask, rows, 1, 2, n_best, nms, normalize=False)


# ------------------------------------------------------------------------------------------------ H: through the model
def _index(model, bs, **kw):
    from univl_amd.retrieval import VideoIndex
    index = VideoIndex(model, keep_frames=True, **kw)
    for b in bs:
        index.add(b["video"], b["video_mask"])
    return index


def _valid(index):
    return index._fmask[:len(index)].sum(1).cpu().numpy()


def _model_case(dtype, sizes):
    cfg, rows, dseed = case_config("joint_small")
    model, _ = build(cfg, dtype)
    model.eval()
    bs = _batches(cfg, sizes, dseed)
    cat = {k: torch.cat([b[k] for b in bs]) for k in bs[0]}
    return cfg, model, bs, (cat["input_ids"], cat["token_type_ids"], cat["attention_mask"])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_localize_n_best_against_localize_and_the_public_path(dtype, deterministic_models):
    from test_model_gpu import GATES
    cfg, model, bs, text = _model_case(dtype, [3, 3])
    tol = TOL if dtype == torch.float32 else GATES[torch.bfloat16]["sim"]
    n, F, P = 6, cfg.max_frames, 3
    index = _index(model, bs, capacity=8)
    W = (1, min(3, F))
    all_rows = torch.arange(n, dtype=torch.int32).repeat(n, 1)
    one = index.localize(*text, all_rows, W)
    many = index.localize(*text, all_rows, W, n_best=P)
    assert all(t.shape == (n, n, P) for t in many) and all(t.shape == (n, n) for t in one)
    for a, b in zip(one, many):
        assert torch.equal(a, b[:, :, 0])                                 # slot 0 is localize()
    also = index.localize_vectors(index.pool_text(*text)[0], all_rows, W, n_best=P, nms=(1, 2))
    assert all(torch.equal(a, b) for a, b in zip(many, also))
    start, length, score = _host(many)
    assert np.all(length[:, :, 0] > 0) and np.all(score[:, :, 1:] <= score[:, :, :-1])        # -inf after -inf in the empty slots
    # every returned window: get_similarity_logits with the video mask narrowed to it
    q, so, am = index.pool_text(*text)
    vo = index._frames[:n].clone()
    checked = 0
    for i in range(n):
        for m in range(P):
            wmask = torch.zeros(n, F, dtype=torch.int64, device=DEV)
            for j in range(n):
                s0, L0 = (int(start[i, j, m]), int(length[i, j, m])) if length[i, j, m] > 0 else (0, 1)
                wmask[j, s0:s0 + L0] = 1
            want = model.get_similarity_logits(so, vo, am, wmask)[i].float().cpu().numpy()
            on = length[i, :, m] > 0
            assert np.abs(score[i, :, m][on] - want[on]).max() <= tol, (i, m)
            checked += int(on.sum())
    assert checked >= n * n


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_search_moments_per_video_and_eval_localization_n_best(dtype, deterministic_models):
    cfg, model, bs, text = _model_case(dtype, [3, 3, 2])
    F, P = cfg.max_frames, 3
    index = _index(model, bs, capacity=8)
    lv = _valid(index)
    W = (1, min(3, F))

    # search_moments(per_video=3) over the whole index against a numpy ranking of all (video, slot) moments
    all_rows = torch.arange(8, dtype=torch.int32).repeat(8, 1)
    a_start, a_length, a_score = _host(index.localize(*text, all_rows, W, n_best=P, nms=(1, 2)))
    k = 12
    score, idx, start, length = (t.cpu().numpy() for t in index.search_moments(*text, k=k, window=W, shortlist=8, per_video=P))
    assert score.shape == idx.shape == start.shape == length.shape == (8, k)
    for i in range(8):
        v, m = NR.rank_moments_nbest(np.arange(8), a_score[i], k)
        assert np.array_equal(idx[i], v) and np.array_equal(start[i], a_start[i, v, m]) and np.array_equal(length[i], a_length[i, v, m])
        assert np.array_equal(_bits(score[i]), _bits(a_score[i, v, m]))
        assert len(set(idx[i].tolist())) < k                              # 12 moments of 8 videos: some video appears more than once
        assert max(np.bincount(idx[i], minlength=8)) <= P
    # per_video = 1 is the call of before
    for a, b in zip(index.search_moments(*text, k=5, window=W, shortlist=8), index.search_moments(*text, k=5, window=W, shortlist=8, per_video=1)):
        assert torch.equal(a, b)
    # a shortlist shorter than the index, other thresholds: shapes, and the moments come from the whole-video top of the list
    s2, i2, st2, l2 = index.search_moments(*text, k=7, window=W, shortlist=4, per_video=2, nms=(0, 1))
    _, top4 = index.search(*text, k=4)
    assert s2.shape == i2.shape == st2.shape == l2.shape == (8, 7) and i2.dtype == torch.int32
    assert all(set(i2[i].tolist()) <= set(top4[i].tolist()) for i in range(8))

    # eval_localization(n_best=5): every text in its own video.  Even texts are annotated with the window of their slot 2 (or their
    # last one): found by R5 at every threshold, by R1 only if slot 0 overlaps enough.  Odd texts are annotated past the video's end.
    lmin = int(lv.min()) + 1                                              # at least one video is too short for any window
    lmax = min(lmin + 2, F)
    assert (lv >= lmin).any() and (lv < lmin).any()
    targets = np.arange(8)
    f_start, f_length, _ = _host(index.localize(*text, torch.arange(8, dtype=torch.int32).reshape(8, 1), (lmin, lmax), n_best=5, nms=(1, 2)))
    f_start, f_length = f_start[:, 0], f_length[:, 0]                     # [8, 5]
    n_found = (f_length > 0).sum(1)
    assert np.array_equal(n_found > 0, lv >= lmin)
    even = np.arange(8) % 2 == 0
    slot = np.clip(np.minimum(2, n_found - 1), 0, None)
    planted = even & (n_found > 0)
    gt_start = np.where(planted, f_start[np.arange(8), slot], F + 10)
    gt_len = np.where(planted, f_length[np.arange(8), slot], 2)
    tb = [(b["input_ids"], b["attention_mask"], b["token_type_ids"]) for b in bs]
    m5 = uev.eval_localization(model, index, tb, targets, gt_start, gt_len, (lmin, lmax), n_best=5, nms=(1, 2))
    assert m5 == NR.rn_counts(f_start, f_length, gt_start, gt_len)
    assert m5["R5@0.3"] == m5["R5@0.5"] == m5["R5@0.7"] == int(planted.sum()) / 8 and planted.sum() >= 1
    assert m5["n"] == 8 and m5["n_empty"] == int((lv < lmin).sum()) >= 1
    m1 = uev.eval_localization(model, index, tb, targets, gt_start, gt_len, (lmin, lmax))
    assert m1 == uev.eval_localization(model, index, tb, targets, gt_start, gt_len, (lmin, lmax), n_best=1)
    assert m1 == R.iou_counts(f_start[:, 0], f_length[:, 0], gt_start, gt_len)                # today's dictionary, key for key
    assert list(m1) == ["mIoU", "R1@0.3", "R1@0.5", "R1@0.7", "n", "n_empty"]
    assert all(m5[key] == m1[key] for key in m1) and m5["R5@0.7"] >= m5["R1@0.7"]


def test_one_captured_graph_is_replayed_on_new_queries():
    F, N, M = 16, 4, 5
    gen = torch.Generator(device=DEV).manual_seed(5)
    frames = torch.randn(N, F, H, device=DEV, generator=gen)
    mask = torch.ones(N, F, dtype=torch.int64, device=DEV)
    mask[1, 11:] = 0
    wnorm = ops.window_norms(frames, mask)
    q = torch.nn.functional.normalize(torch.randn(3, H, device=DEV, generator=gen), dim=-1)
    q2 = torch.nn.functional.normalize(torch.randn(3, H, device=DEV, generator=gen), dim=-1)
    rows = torch.tensor([[0, 1, 2, 3], [3, -1, 1, 0], [2, 2, 4, 1]], dtype=torch.int32, device=DEV)
    run = lambda x: ops.moment_nbest(x, frames, mask, rows, 2, 6, M, (1, 2), wnorm=wnorm)
    eager1, eager2 = run(q), run(q2)
    assert not torch.equal(eager1[2], eager2[2])
    qs = q.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run(qs)
    for src, want in ((q, eager1), (q2, eager2), (q, eager1)):
        qs.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(out, want))
