"""float64 numpy statement of n-best moment search with temporal non-maximum suppression (include/univl_hip.h: univl_moment_nbest),
shared by tests/test_moment_nbest_cpu.py and tests/test_moment_nbest_gpu.py.  Built on tests/moment_ref.py: the scores of a pair are
row_scores' [F, F] matrix indexed (s, L - 1), -inf where the window is no candidate by the mask or runs past the end.

nbest_greedy restates the contract literally (the first live candidate under ORDER, kill, repeat); nbest_sweep says the same thing
another way (sort once, walk down, keep a window iff no kept window suppresses it); tests/test_moment_nbest_cpu.py holds the two against
each other.  check_nbest judges a kernel's answer by properties stated relative to the kernel's OWN earlier picks, so that no window
position is ever compared under a tolerance.  rn_counts is eval_localization's dictionary with the R{n}@ columns."""
import functools

import numpy as np

import moment_ref as R

NEG_INF = R.NEG_INF
NBEST_MAX = 16                    # include/univl_hip.h: UNIVL_MOMENT_NBEST_MAX
CONFIGS = ((1, (1, 2)), (5, (1, 2)), (16, (0, 1)), (5, (7, 10)), (4, (1, 1)))      # (M, nms) of the GPU parity test
NMS_SMALL = ((0, 1), (1, 2), (7, 10), (1, 1))


def candidate_mask(S, lmin, lmax):
    """[F, F] bool over (s, L - 1): the pair's candidate windows of lengths lmin .. lmax."""
    L = np.arange(1, S.shape[0] + 1)
    return (S > NEG_INF) & (L >= lmin)[None, :] & (L <= lmax)[None, :]


def inter_frames(s, L, ps, pl):
    return max(0, min(s + L, ps + pl) - max(s, ps))


def suppresses(ps, pl, s, L, num, den):
    """Does the pick (ps, pl) kill the window (s, L)?  The pick itself, and every window with den * inter > num * union -- integers."""
    inter = inter_frames(s, L, ps, pl)
    return (s, L) == (ps, pl) or den * inter > num * (L + pl - inter)


def suppress_mask(F, ps, pl, num, den):
    """suppresses() for all windows at once: [F, F] bool over (s, L - 1), candidates or not."""
    s = np.arange(F, dtype=np.int64)[:, None]
    L = np.arange(1, F + 1, dtype=np.int64)[None, :]
    inter = np.maximum(0, np.minimum(s + L, ps + pl) - np.maximum(s, ps))
    return ((s == ps) & (L == pl)) | (den * inter > num * (L + pl - inter))


def _empty(M):
    return np.full(M, -1, dtype=np.int64), np.zeros(M, dtype=np.int64), np.full(M, NEG_INF)


def nbest_greedy(S, lmin, lmax, M, num, den):
    """The contract, literally.  S: [F, F] scores of one pair.  (start, length, score), each [M]; (-1, 0, -inf) from the first slot for
    which nothing is alive."""
    F = S.shape[0]
    start, length, score = _empty(M)
    alive = candidate_mask(S, lmin, lmax)
    for m in range(M):
        if not alive.any():
            break
        at = int(np.argmax(np.where(alive, S, NEG_INF).reshape(-1)))      # the first maximum in (s, L) order: ORDER
        s, L = at // F, at % F + 1
        start[m], length[m], score[m] = s, L, S[s, L - 1]
        alive &= ~suppress_mask(F, s, L, num, den)
    return start, length, score


def nbest_sweep(S, lmin, lmax, M, num, den):
    """The same windows, stated independently: all candidates sorted once under ORDER; walking down, a window is kept iff none of the
    windows kept before it suppresses it (scalar integer tests, no masks)."""
    start, length, score = _empty(M)
    ss, ll = np.nonzero(candidate_mask(S, lmin, lmax))
    ll = ll + 1
    order = np.lexsort((ll, ss, -S[ss, ll - 1]))
    kept = []
    for i in order:
        if len(kept) == M:
            break
        s, L = int(ss[i]), int(ll[i])
        if not any(suppresses(ps, pl, s, L, num, den) for ps, pl in kept):
            kept.append((s, L))
    for m, (s, L) in enumerate(kept):
        start[m], length[m], score[m] = s, L, S[s, L - 1]
    return start, length, score


def top_plain(S, lmin, lmax, M):
    """The plain top-M candidates under ORDER, no suppression: what nms = (1, 1) must give."""
    start, length, score = _empty(M)
    ss, ll = np.nonzero(candidate_mask(S, lmin, lmax))
    ll = ll + 1
    order = np.lexsort((ll, ss, -S[ss, ll - 1]))[:M]
    n = len(order)
    start[:n], length[:n], score[:n] = ss[order], ll[order], S[ss[order], ll[order] - 1]
    return start, length, score


def check_nbest(start, length, score, S, lmin, lmax, num, den, gate):
    """A kernel's M slots of one pair (start, length int arrays, score fp32 array) against the pair's float64 scores S [F, F], or S =
    None for a row id outside the gallery.  With every candidate alive at first, for each slot m in turn:
      (a) the window is a candidate of the pair;
      (b) its score is within `gate` of the window's float64 score;
      (c) scores never increase from slot to slot -- exact;
      (d) it is alive: not suppressed by an earlier returned window, not equal to one -- exact, integers;
      (e) the best float64 score among the windows alive after the kernel's OWN picks 0 .. m - 1 exceeds the float64 score of pick m by
          at most 2 x gate: both carry one gate of error, and that is the whole derivation;
      (f) an empty slot is (-1, 0, -inf), nothing is alive after the kernel's own picks before it, and all later slots are empty -- exact.
    Returns the largest score error."""
    start, length = np.asarray(start, dtype=np.int64), np.asarray(length, dtype=np.int64)
    M = len(start)
    if S is None:
        assert np.all(start == -1) and np.all(length == 0) and np.all(score == NEG_INF)
        return 0.0
    F = S.shape[0]
    cand = candidate_mask(S, lmin, lmax)
    alive = cand.copy()
    err = 0.0
    for m in range(M):
        s, L = int(start[m]), int(length[m])
        if L == 0:
            assert not alive.any(), ("(f) a live candidate is left", m)
            assert np.all(start[m:] == -1) and np.all(length[m:] == 0) and np.all(score[m:] == NEG_INF), ("(f)", m)
            break
        assert 0 <= s and 1 <= L and s + L <= F and cand[s, L - 1], ("(a)", m, s, L)
        assert alive[s, L - 1], ("(d)", m, s, L)
        e = abs(float(score[m]) - S[s, L - 1])
        assert e <= gate, ("(b)", m, e)
        err = max(err, e)
        assert m == 0 or score[m] <= score[m - 1], ("(c)", m)
        best = S[alive].max()
        assert best - S[s, L - 1] <= 2 * gate, ("(e)", m, best - S[s, L - 1])
        alive &= ~suppress_mask(F, s, L, num, den)
    return err


def rn_counts(start, length, gt_start, gt_len):
    """eval_localization's dictionary from the windows found ([n, n_best] integer arrays; length 0 = an empty slot) and the annotated
    ones ([n]): slot 0 gives moment_ref.iou_counts' entries, and n_best > 1 adds R{n_best}@0.3 / 0.5 / 0.7 -- a text counts if ANY of
    its windows meets 10 inter >= t union."""
    start, length = np.asarray(start, dtype=np.int64), np.asarray(length, dtype=np.int64)
    gt_start, gt_len = np.asarray(gt_start, dtype=np.int64).reshape(-1), np.asarray(gt_len, dtype=np.int64).reshape(-1)
    n, nb = start.shape
    out = R.iou_counts(start[:, 0], length[:, 0], gt_start, gt_len)
    if nb > 1:
        for t in (3, 5, 7):
            hit = 0
            for i in range(n):
                gt = set(range(gt_start[i], gt_start[i] + gt_len[i]))
                for m in range(nb):
                    w = set(range(start[i, m], start[i, m] + length[i, m]))
                    if length[i, m] > 0 and 10 * len(w & gt) >= t * len(w | gt):
                        hit += 1
                        break
            out["R%d@0.%d" % (nb, t)] = hit / n
    return out


def rank_moments_nbest(idx, score, k):
    """search_moments(per_video=P)'s order over one text's shortlist.  idx: [S] row ids, score: [S, P].  Window score descending, then
    lower row id (the -1 rows of a short gallery last), then the earlier pick.  Returns (video position, slot) of the first k."""
    idx, score = np.asarray(idx, dtype=np.int64), np.asarray(score, dtype=np.float64)
    S, P = score.shape
    key = np.repeat(np.where(idx < 0, np.iinfo(np.int64).max, idx), P)
    slot = np.tile(np.arange(P), S)
    order = np.lexsort((slot, key, -score.reshape(-1)))[:k]
    return order // P, order % P


# ------------------------------------------------------------------------------------------------ the inputs of the GPU tests
@functools.lru_cache(maxsize=None)
def parity_scores(F, P, normalize):
    """{gallery row: S [Nq, F, F]} in float64 for the rows parity_case(F, P) names."""
    frames, mask, q, rows = R.parity_case(F, P)
    return {r: R.row_scores(q, frames[r], mask[r], normalize)[0] for r in sorted(set(int(x) for x in rows.reshape(-1)))}


def exact_scores(q, frames, mask):
    """use_mil scores of integer inputs as the device computes them: the numerators are integers below 2^24 (exact in fp32 in any
    order) and the quotient by L is one correctly rounded fp32 division.  [Nq, F, F] float64 holding fp32 values, -inf off the mask."""
    q, frames = np.asarray(q).astype(np.int64), np.asarray(frames).astype(np.int64)
    F = frames.shape[0]
    d = q @ frames.T                                                      # [Nq, F]
    S = np.full((q.shape[0], F, F), NEG_INF)
    for s in range(F):
        num = np.cumsum(d[:, s:], axis=1)
        assert np.abs(num).max() < 2 ** 24
        ok = np.cumprod(np.asarray(mask)[s:] != 0).astype(bool)
        sc = (num.astype(np.float32) / np.arange(1, F - s + 1, dtype=np.float32)[None, :]).astype(np.float64)
        S[:, s, :F - s] = np.where(ok[None, :], sc, NEG_INF)
    return S


def int_case(F, seed):
    """The construction of tests/test_moment_gpu.py's integer test: frames and queries in [-8, 8], 7 rows with prefix masks; row 5 is
    one frame repeated (every window ties), row 6 repeats a block of 3 frames (ties across starts and lengths)."""
    rng = np.random.RandomState(seed)
    frames = rng.randint(-8, 9, size=(7, F, R.H)).astype(np.float32)
    frames[5] = frames[5, 0]
    frames[6] = frames[6, np.arange(F) % 3]
    mask = np.zeros((7, F), dtype=np.int64)
    for r, n in enumerate([F, max(1, F // 2), max(1, F - 1), 1, min(F, 9), F, F]):
        mask[r, :n] = 1
    q = rng.randint(-8, 9, size=(5, R.H)).astype(np.float32)
    rows = np.stack([rng.permutation(7) for _ in range(5)]).astype(np.int32)
    return frames, mask, q, rows
