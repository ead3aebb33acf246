"""float64 numpy reference of ordered step alignment (include/univl_hip.h: univl_step_align), shared by tests/test_step_align_cpu.py
and tests/test_step_align_gpu.py.  Two independent pieces over the window scores of tests/moment_ref.py (row_scores):

  programme   the suffix programme of the contract: A[k][s] the best w(k, s, L) + G[k+1][s + L] over ascending L with strict >, G[k][t]
              the maximum of A[k][s] over s >= t, the walk from (k, t) = (0, 0) taking the lowest s >= t with A[k][s] == G[k][t];
  enumerate   every alignment there is, its total summed from the last step to the first, the largest total and among equal totals the
              lexicographically smallest (s_0, L_0, s_1, L_1, ..).

tests/test_step_align_cpu.py holds the two against each other.  Also here: the fixed-seed inputs of the GPU tests, so that the CPU
suite can check what they hold, and the counts of eval.eval_step_alignment."""
import functools

import numpy as np

import moment_ref as R

H = R.H
NEG_INF = R.NEG_INF
K_MAX = 32


def is_alignment(mask, starts, lengths, lmin, lmax):
    """Windows of lmin .. lmax valid frames, in order, never overlapping."""
    t = 0
    for s, L in zip(starts, lengths):
        if s < t or not R.is_candidate(mask, int(s), int(L), lmin, lmax):
            return False
        t = s + L
    return True


def total_of(S, starts, lengths):
    """T_0 of an alignment: T_n = 0, T_k = w_k + T_{k+1}.  S: [n, F, F] window scores (moment_ref.row_scores)."""
    tot = 0.0
    for k in range(len(starts) - 1, -1, -1):
        tot = S[k, starts[k], lengths[k] - 1] + tot
    return float(tot)


def programme(S, lmin, lmax):
    """S: [n, F, F] scores of one (list, row) pair, -inf where a window is no candidate by the mask.  Returns (starts, lengths, scores,
    total), or None when no alignment exists."""
    n, F = S.shape[0], S.shape[1]
    G = np.full((n + 1, F + 1), NEG_INF)
    G[n] = 0.0
    A = np.full((n, F), NEG_INF)
    Lb = np.zeros((n, F), dtype=np.int64)
    s = np.arange(F)
    for k in range(n - 1, -1, -1):
        for L in range(lmin, lmax + 1):                                   # ascending, a later length only if strictly larger
            ok = s + L <= F
            v = np.full(F, NEG_INF)
            v[ok] = S[k, s[ok], L - 1] + G[k + 1, s[ok] + L]
            better = v > A[k]
            A[k, better], Lb[k, better] = v[better], L
        G[k, :F] = np.maximum.accumulate(A[k, ::-1])[::-1]
    if G[0, 0] == NEG_INF:
        return None
    starts, lengths, scores, t = [], [], [], 0
    for k in range(n):
        at = t + int(np.nonzero(A[k, t:] == G[k, t])[0][0])               # the lowest s >= t that attains G[k][t]
        starts.append(at)
        lengths.append(int(Lb[k, at]))
        scores.append(float(S[k, at, Lb[k, at] - 1]))
        t = at + lengths[-1]
    return starts, lengths, scores, float(G[0, 0])


def enumerate_alignments(S, lmin, lmax):
    """Every alignment of the pair, by brute force: the same four values as programme, or None.  Exponential: small F and n only."""
    n, F = S.shape[0], S.shape[1]
    best = None

    def rec(k, t, starts, lengths):
        nonlocal best
        if k == n:
            tot = total_of(S, starts, lengths)
            key = [x for pair in zip(starts, lengths) for x in pair]
            if best is None or tot > best[0] or (tot == best[0] and key < best[1]):
                best = (tot, key)
            return
        for s in range(t, F):
            for L in range(lmin, min(lmax, F - s) + 1):
                if S[k, s, L - 1] != NEG_INF:
                    rec(k + 1, s + L, starts + [s], lengths + [L])

    rec(0, 0, [], [])
    if best is None:
        return None
    starts, lengths = best[1][0::2], best[1][1::2]
    return starts, lengths, [float(S[k, starts[k], lengths[k] - 1]) for k in range(n)], best[0]


def align(Q, counts, frames, mask, rows, lmin, lmax, normalize, solve=programme):
    """Q: [Nl, K, H], counts: [Nl], frames: [N, F, H], mask: [N, F], rows: [Nl, C].  Returns (start, length [Nl, C, K] int64, score
    [Nl, C, K], total [Nl, C]): (-1, 0, -inf) in the slots past counts, and in every slot -- total -inf -- of a pair without an
    alignment, with a row id outside [0, N) or a count outside [1, K].  Q rows past counts are not touched."""
    return align_many(Q, counts, frames, mask, rows, [(lmin, lmax)], normalize, solve)[(lmin, lmax)]


def align_many(Q, counts, frames, mask, rows, windows, normalize, solve=programme, scores=None):
    """{(lmin, lmax): align(..., lmin, lmax, ...)} for several length ranges, each pair's windows scored once.  scores(i, r): the
    [n, F, F] window scores of list i on row r, for a caller that keeps them."""
    Q, rows, counts = np.asarray(Q), np.asarray(rows), np.asarray(counts)
    Nl, K = Q.shape[0], Q.shape[1]
    C, N = rows.shape[1], len(frames)
    out = {w: (np.full((Nl, C, K), -1, dtype=np.int64), np.zeros((Nl, C, K), dtype=np.int64), np.full((Nl, C, K), NEG_INF),
               np.full((Nl, C), NEG_INF)) for w in windows}
    for r in sorted(set(int(x) for x in rows.reshape(-1) if 0 <= x < N)):
        for i in range(Nl):
            n = int(counts[i])
            if not 1 <= n <= K or not np.any(rows[i] == r):
                continue
            S = scores(i, r) if scores else R.row_scores(Q[i, :n], frames[r], mask[r], normalize)[0]
            for w in windows:
                got = solve(S, w[0], w[1])
                if got is None:
                    continue
                start, length, score, total = out[w]
                for c in np.nonzero(rows[i] == r)[0]:
                    start[i, c, :n], length[i, c, :n], score[i, c, :n], total[i, c] = got
    return out


def step_counts(start, length, counts, total, gt_start, gt_len):
    """eval_step_alignment's dictionary from the windows found [n, K], the lists' counts and totals [n] and the annotation [n, K]."""
    start, length, gt_start, gt_len = (np.asarray(a, dtype=np.int64) for a in (start, length, gt_start, gt_len))
    n, K = start.shape
    hits, annotated, ious = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64), []
    for i in range(n):
        for k in range(min(max(int(counts[i]), 0), K)):
            if gt_len[i, k] == 0:
                continue
            annotated[i] += 1
            gt = set(range(gt_start[i, k], gt_start[i, k] + gt_len[i, k]))
            found = set(range(start[i, k], start[i, k] + length[i, k])) if length[i, k] > 0 else set()
            ious.append(len(found & gt) / len(found | gt))
            if length[i, k] > 0 and start[i, k] + (length[i, k] - 1) // 2 in gt:
                hits[i] += 1
    return {"recall": float(hits.sum()) / int(annotated.sum()), "mIoU": float(np.mean(np.array(ious, dtype=np.float64))), "n_lists": n,
            "n_steps": int(annotated.sum()), "n_infeasible": int(np.sum(np.isinf(np.asarray(total, dtype=np.float64)))), "hits": hits,
            "annotated": annotated}


# ------------------------------------------------------------------------------------------------ the inputs of the GPU tests
PARITY_F = R.PARITY_F
PARITY_K = (1, 3, 32)
PARITY_LISTS, PARITY_C = 5, 3


def parity_shapes():
    return [(F, K) for F in PARITY_F for K in PARITY_K if K <= F]


def parity_windows(F, K):
    """(1, 1), (1, max(1, F // K)), and (2, 5) where it fits."""
    return sorted(set([(1, 1), (1, max(1, F // K))] + ([(2, 5)] if F >= 5 else [])))


@functools.lru_cache(maxsize=None)
def parity_case(F, K):
    """moment_ref.parity_case's frames (norm about 28) and prefix masks; unit step vectors [5, K, 768] from a seeded generator, the
    slots past a list's count NaN (they are never read); counts mixing K, 1 and values between; rows [5, 3]: gallery rows, among them
    row 0 (every frame valid) and one id outside the gallery."""
    frames, mask, _, _ = R.parity_case(F, 5)
    rng = np.random.RandomState(9000 + 131 * F + K)
    q = rng.standard_normal((PARITY_LISTS, K, H))
    q /= np.linalg.norm(q, axis=2, keepdims=True)
    counts = np.array([K, 1, (K + 1) // 2, K, max(1, K - 1)], dtype=np.int32)
    for i in range(PARITY_LISTS):
        q[i, counts[i]:] = np.nan
    rows = rng.randint(0, R.PARITY_ROWS, size=(PARITY_LISTS, PARITY_C)).astype(np.int32)
    rows[0, 0], rows[1, 1], rows[3, 2] = 0, -1, 0
    return frames, mask, q.astype(np.float32), counts, rows


@functools.lru_cache(maxsize=16)
def parity_scores(F, K, i, r, normalize):
    """The float64 window scores [counts[i], F, F] of list i of parity_case(F, K) on gallery row r; the last pairs asked for are kept."""
    frames, mask, q, counts, _ = parity_case(F, K)
    return R.row_scores(q[i, :counts[i]], frames[r], mask[r], normalize)[0]


@functools.lru_cache(maxsize=None)
def parity_reference(F, K, normalize):
    """{(lmin, lmax): align(...)} of parity_case(F, K) in one mode."""
    frames, mask, q, counts, rows = parity_case(F, K)
    return align_many(q, counts, frames, mask, rows, parity_windows(F, K), normalize, scores=lambda i, r: parity_scores(F, K, i, r, normalize))


EXACT_F = (8, 16, 50, 128)
EXACT_COUNTS = (1, 2, 7, 32)
EXACT_WINDOWS = ((1, 1), (2, 2), (4, 4), (1, 2))


@functools.lru_cache(maxsize=None)
def exact_case(F):
    """Integer frames and step vectors in [-8, 8] (every product sum is an integer below 2^24; under use_mil with window lengths 1, 2
    and 4 every score is an integer over a power of two and every total of at most 32 of them exact in fp32).  The 7 rows of
    test_moment_gpu._int_case: prefix masks, row 5 one frame repeated, row 6 a block of 3 frames repeated.  Lists of 1, 2, 7 and 32
    steps padded to K = 32, each against all 7 rows."""
    rng = np.random.RandomState(500 + F)
    frames = rng.randint(-8, 9, size=(7, F, H)).astype(np.float32)
    frames[5] = frames[5, 0]
    frames[6] = frames[6, np.arange(F) % 3]
    mask = np.zeros((7, F), dtype=np.int64)
    for r, n in enumerate([F, max(1, F // 2), max(1, F - 1), 1, min(F, 9), F, F]):
        mask[r, :n] = 1
    q = rng.randint(-8, 9, size=(len(EXACT_COUNTS), K_MAX, H)).astype(np.float32)
    counts = np.array(EXACT_COUNTS, dtype=np.int32)
    rows = np.stack([rng.permutation(7) for _ in EXACT_COUNTS]).astype(np.int32)
    return frames, mask, q, counts, rows


@functools.lru_cache(maxsize=None)
def exact_reference(F):
    frames, mask, q, counts, rows = exact_case(F)
    return align_many(q, counts, frames, mask, rows, EXACT_WINDOWS, False)
