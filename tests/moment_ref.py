"""float64 numpy brute force of the moment-search contract (include/univl_hip.h: univl_window_norms, univl_moment_localize), shared by
tests/test_moment_cpu.py and tests/test_moment_gpu.py: every window of every pair, both modes, the tie order, the (-1, 0, -inf)
cases, search_moments' ranking and the IoU counts of eval_localization -- and the fixed-seed inputs of the GPU parity test, so that
the CPU suite can check what they leave undecided.

window_score sums one window from scratch.  row_scores is the same numbers for all windows of a row at once (float64 running sums
from every start: 1e-13 beside the 2e-4 the GPU tests allow); tests/test_moment_cpu.py holds the two against each other."""
import functools

import numpy as np

H = 768
NEG_INF = float("-inf")


def is_candidate(mask, s, L, lmin, lmax):
    F = len(mask)
    return lmin <= L <= lmax and 0 <= s and s + L <= F and bool(np.all(np.asarray(mask[s:s + L]) != 0))


def window_score(q, frames, s, L, normalize):
    """The score of window (s, L), whether or not it is a candidate.  q: [H], frames: [F, H]."""
    u = np.asarray(frames, dtype=np.float64)[s:s + L].sum(0)
    num = float(np.dot(np.asarray(q, dtype=np.float64), u))
    return num / max(float(np.sqrt(np.dot(u, u))), 1e-12 * L) if normalize else num / L


def row_scores(Q, frames, mask, normalize):
    """One gallery row against the queries Q [Nq, H].  Returns (S [Nq, F, F] scores indexed (s, L - 1), -inf where the window is no
    candidate by the mask or runs past the end; T [F, F] the window norms, 0 there)."""
    Q, frames, mask = np.asarray(Q, dtype=np.float64), np.asarray(frames, dtype=np.float64), np.asarray(mask)
    F = frames.shape[0]
    S = np.full((Q.shape[0], F, F), NEG_INF)
    T = np.zeros((F, F))
    for s in range(F):
        u = np.cumsum(frames[s:], axis=0)                                 # u(s, L), L = 1 .. F - s
        ok = np.cumprod(mask[s:] != 0).astype(bool)
        L = np.arange(1, F - s + 1, dtype=np.float64)
        nrm = np.sqrt((u * u).sum(1))
        num = Q @ u.T
        sc = num / np.maximum(nrm, 1e-12 * L) if normalize else num / L
        S[:, s, :F - s] = np.where(ok, sc, NEG_INF)
        T[s, :F - s] = np.where(ok, nrm, 0.0)
    return S, T


def norm_table(frames, mask):
    return row_scores(np.zeros((1, np.asarray(frames).shape[1])), frames, mask, True)[1]


def best_window(S, lmin, lmax):
    """S: [F, F] scores of one pair (row_scores).  (start, length, score, margin) of the best candidate with lmin <= L <= lmax: larger
    score, then lower s, then smaller L -- the first maximum in (s, L) order.  margin: best minus second best score (inf with fewer
    than two candidates).  (-1, 0, -inf, inf) without a candidate."""
    F = S.shape[0]
    L = np.arange(1, F + 1)
    C = np.where((L >= lmin) & (L <= lmax), S, NEG_INF).reshape(-1)
    at = int(np.argmax(C))
    if C[at] == NEG_INF:
        return -1, 0, NEG_INF, np.inf
    best = C[at]
    C[at] = NEG_INF
    second = C.max()
    return at // F, at % F + 1, float(best), (np.inf if second == NEG_INF else float(best - second))


def localize(Q, frames, mask, rows, lmin, lmax, normalize):
    """Q: [Nq, H], frames: [N, F, H], mask: [N, F], rows: [Nq, K] ints.  Returns (start, length, score, margin) arrays [Nq, K]:
    (-1, 0, -inf) for a pair without a candidate window or with a row id outside [0, N)."""
    return localize_many(Q, frames, mask, rows, [(lmin, lmax)], normalize)[(lmin, lmax)]


def localize_many(Q, frames, mask, rows, windows, normalize):
    """{(lmin, lmax): localize(..., lmin, lmax, ...)} for several length ranges, each row's windows scored once."""
    rows = np.asarray(rows)
    N = len(frames)
    out = {w: (np.full(rows.shape, -1, dtype=np.int64), np.zeros(rows.shape, dtype=np.int64), np.full(rows.shape, NEG_INF),
               np.full(rows.shape, np.inf)) for w in windows}
    for r in sorted(set(int(x) for x in rows.reshape(-1) if 0 <= x < N)):
        S, _ = row_scores(Q, frames[r], mask[r], normalize)
        for i, j in zip(*np.nonzero(rows == r)):
            for w in windows:
                start, length, score, margin = out[w]
                start[i, j], length[i, j], score[i, j], margin[i, j] = best_window(S[i], w[0], w[1])
    return out


def rank_moments(idx, score, k):
    """search_moments' order over one text's shortlist: window score descending, equal scores by lower row id; the -1 rows of a short
    gallery last.  idx, score: [S].  Returns the positions of the first k."""
    idx, score = np.asarray(idx, dtype=np.int64), np.asarray(score, dtype=np.float64)
    key = np.where(idx < 0, np.iinfo(np.int64).max, idx)
    return np.lexsort((key, -score))[:k]


def iou_counts(start, length, gt_start, gt_len):
    """eval_localization's dictionary from the windows found and the annotated ones (integer arrays [n]); length 0 = no window."""
    start, length, gt_start, gt_len = (np.asarray(a, dtype=np.int64).reshape(-1) for a in (start, length, gt_start, gt_len))
    n = len(start)
    inter = np.zeros(n, dtype=np.int64)
    for i in range(n):
        if length[i] > 0:
            inter[i] = len(set(range(start[i], start[i] + length[i])) & set(range(gt_start[i], gt_start[i] + gt_len[i])))
    union = length + gt_len - inter
    out = {"mIoU": float(np.mean(inter.astype(np.float64) / union.astype(np.float64)))}
    for name, num in (("R1@0.3", 3), ("R1@0.5", 5), ("R1@0.7", 7)):
        out[name] = float(np.sum(10 * inter >= num * union)) / n
    out["n"], out["n_empty"] = n, int(np.sum(length == 0))
    return out


# ------------------------------------------------------------------------------------------------ the inputs of the GPU parity test
PARITY_F = (1, 2, 16, 48, 50, 128)
PARITY_P = (1, 5, 37)
PARITY_ROWS = 6                   # gallery rows of a parity case
UNDECIDED_CAP = 0.10              # the share of pairs whose best two windows may lie within the tolerance of each other


def parity_windows(F):
    """(lmin, lmax) of the parity test at F frames: (1, 1), (1, F), (F, F), and (3, 7) where it fits."""
    w = [(1, 1), (1, F), (F, F)] + ([(3, 7)] if F >= 7 else [])
    return sorted(set(w))


@functools.lru_cache(maxsize=None)
def parity_case(F, P):
    """Fixed-seed inputs as float32 / int64 numpy arrays: frames [6, F, 768] with per-frame norm about 28 (the scale of LayerNorm
    output), masks [6, F] (rows 0 and 1 whole, the others a valid prefix of random length >= 1), unit queries [Nq, 768] and rows
    [Nq, K] with Nq * K = P (P = 5 is one query against five candidates, the others one candidate per query)."""
    rng = np.random.RandomState(7000 + 131 * F + P)
    frames = rng.standard_normal((PARITY_ROWS, F, H)) * (28.0 / np.sqrt(H))
    mask = np.zeros((PARITY_ROWS, F), dtype=np.int64)
    for r in range(PARITY_ROWS):
        mask[r, :F if r < 2 else rng.randint(1, F + 1)] = 1
    Nq, K = (1, 5) if P == 5 else (P, 1)
    q = rng.standard_normal((Nq, H))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    rows = rng.randint(0, PARITY_ROWS, size=(Nq, K)).astype(np.int32)
    return frames.astype(np.float32), mask, q.astype(np.float32), rows


@functools.lru_cache(maxsize=None)
def parity_reference(F, P, normalize):
    """{(lmin, lmax): localize(...)} of parity_case(F, P) in one mode, and the float64 norm tables [6, F, F]."""
    frames, mask, q, rows = parity_case(F, P)
    ref = localize_many(q, frames, mask, rows, parity_windows(F), normalize)
    tables = np.stack([norm_table(frames[r], mask[r]) for r in range(PARITY_ROWS)])
    return ref, tables
