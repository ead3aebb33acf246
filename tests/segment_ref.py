"""float64 numpy reference of frame-wise segmentation (include/univl_hip.h: univl_frame_segment), shared by tests/test_segment_cpu.py
and tests/test_segment_gpu.py.  Two independent pieces over the frame scores e(k, t) of a (label set, row) pair:

  programme   the suffix programme of the contract: V, M, a and stay from the last valid frame to the first, then the forward walk;
  enumerate   every labelling there is, (n + 1)^T of them, each one's objective summed by itself, and the largest.

tests/test_segment_cpu.py holds the two against each other.  Also here: the fixed-seed inputs of the GPU tests, so that the CPU suite can
check what they hold, and the counts of eval.eval_segmentation.

Inside this file the background label has index n, as in the contract; the outputs carry it as -1, and -2 on a masked frame."""
import functools
import itertools

import numpy as np

import moment_ref as R

H = R.H
NEG_INF = R.NEG_INF
K_MAX = 64
BACKGROUND, MASKED = -1, -2


def frame_scores(Q, frames, mask, normalize):
    """E [n + 0, T]: e(k, t) of the label vectors Q [n, H] on the VALID frames of one row, and vf [T], their frame indices.  The score
    of the one-frame window (f, 1): q . x_f / max(|x_f|, 1e-12), or q . x_f."""
    Q, frames = np.asarray(Q, dtype=np.float64), np.asarray(frames, dtype=np.float64)
    vf = np.nonzero(np.asarray(mask) != 0)[0]
    x = frames[vf]
    num = Q @ x.T
    if normalize:
        num = num / np.maximum(np.sqrt((x * x).sum(1)), 1e-12)[None, :]
    return num, vf


def with_background(E, b):
    """[n + 1, T]: the label scores and the background's row."""
    return np.vstack([E, np.full((1, E.shape[1]), float(b))])


def objective(Eb, y, lam):
    """sum_t e(y_t, t) - lam * #{t >= 1: y_t != y_{t-1}} of a labelling y [T] over Eb [n + 1, T], summed from the last frame to the first."""
    y = np.asarray(y, dtype=np.int64)
    tot = 0.0
    for t in range(len(y) - 1, -1, -1):
        tot = Eb[y[t], t] + tot - (lam if t + 1 < len(y) and y[t] != y[t + 1] else 0.0)
    return float(tot)


def run_count(y, n):
    """Maximal runs of equal non-background labels (background = n) in y."""
    y = np.asarray(y, dtype=np.int64)
    return int(sum(1 for t in range(len(y)) if y[t] != n and (t == 0 or y[t] != y[t - 1])))


def programme(E, lam, b):
    """E: [n, T] frame scores on the valid frames, T >= 1.  Returns (y [T] with the background as n, scores [T], total, nseg)."""
    n, T = E.shape
    Eb = with_background(E, b)
    V = Eb[:, T - 1].copy()
    M, a = np.empty(T), np.empty(T, dtype=np.int64)
    stay = np.zeros((T, n + 1), dtype=bool)
    M[T - 1], a[T - 1] = V.max(), int(np.argmax(V))                       # argmax: the lowest index among equals, the background last
    for t in range(T - 2, -1, -1):
        thr = M[t + 1] - lam
        stay[t] = V >= thr                                                # a tie stays
        V = Eb[:, t] + np.maximum(V, thr)
        M[t], a[t] = V.max(), int(np.argmax(V))
    y = np.empty(T, dtype=np.int64)
    y[0] = a[0]
    for t in range(T - 1):
        y[t + 1] = y[t] if stay[t, y[t]] else a[t + 1]
    return y, Eb[y, np.arange(T)], float(M[0]), run_count(y, n)


def enumerate_labellings(E, lam, b):
    """Every labelling of the pair by brute force: (the largest objective, the list of labellings that attain it exactly).  Exponential."""
    n, T = E.shape
    Eb = with_background(E, b)
    best, at = NEG_INF, []
    for y in itertools.product(range(n + 1), repeat=T):
        v = objective(Eb, y, lam)
        if v > best:
            best, at = v, [y]
        elif v == best:
            at.append(y)
    return best, at


def segment(Q, counts, frames, mask, rows, lam, b, normalize):
    """Q: [Nl, K, H], counts: [Nl], frames: [N, F, H], mask: [N, F], rows: [Nl, C].  Returns (label [Nl, C, F] int64, score [Nl, C, F],
    total [Nl, C], nseg [Nl, C] int64): label -2 and score -inf on a masked frame; everything -2 / -inf / 0 for a pair with a row id
    outside [0, N), a count outside [1, K] or no valid frame.  Q rows past counts are not touched."""
    return segment_many(Q, counts, frames, mask, rows, [(lam, b)], normalize)[(lam, b)]


def segment_many(Q, counts, frames, mask, rows, params, normalize, scores=None):
    """{(lam, b): segment(..., lam, b, ...)} for several parameter pairs, each pair's frame scores computed once.  scores(i, r): the
    (E, vf) of set i on row r, for a caller that keeps them."""
    Q, rows, counts = np.asarray(Q), np.asarray(rows), np.asarray(counts)
    Nl, K = Q.shape[0], Q.shape[1]
    C, N, F = rows.shape[1], len(frames), np.asarray(mask).shape[1]
    out = {pr: (np.full((Nl, C, F), MASKED, dtype=np.int64), np.full((Nl, C, F), NEG_INF), np.full((Nl, C), NEG_INF),
                np.zeros((Nl, C), dtype=np.int64)) for pr in params}
    for i in range(Nl):
        n = int(counts[i])
        if not 1 <= n <= K:
            continue
        for r in sorted(set(int(x) for x in rows[i] if 0 <= x < N)):
            E, vf = scores(i, r) if scores else frame_scores(Q[i, :n], frames[r], mask[r], normalize)
            if len(vf) == 0:
                continue
            for pr in params:
                y, sc, tot, ns = programme(E, pr[0], pr[1])
                label, score, total, nseg = out[pr]
                for c in np.nonzero(rows[i] == r)[0]:
                    label[i, c, vf], score[i, c, vf] = np.where(y == n, BACKGROUND, y), sc
                    total[i, c], nseg[i, c] = tot, ns
    return out


def frame_counts(label, total, nseg, gt):
    """eval_segmentation's dictionary from the labels found [n, F] (-2 on a masked frame), the totals and run counts [n] and the
    annotation gt [n, F] (-2: not annotated), frame by frame."""
    label, gt = np.asarray(label, dtype=np.int64), np.asarray(gt, dtype=np.int64)
    n = label.shape[0]
    correct, annotated = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    cfg = afg = 0
    for i in range(n):
        for f in range(label.shape[1]):
            if gt[i, f] == MASKED or label[i, f] == MASKED:
                continue
            annotated[i] += 1
            correct[i] += int(label[i, f] == gt[i, f])
            if gt[i, f] >= 0:
                afg += 1
                cfg += int(label[i, f] == gt[i, f])
    return {"frame_accuracy": float(correct.sum()) / int(annotated.sum()), "frame_accuracy_fg": float(cfg) / afg if afg else float("nan"),
            "correct": correct, "annotated": annotated, "n_lists": n, "n_frames": int(annotated.sum()),
            "n_segments": int(np.asarray(nseg, dtype=np.int64).sum()), "n_empty": int(np.sum(np.isinf(np.asarray(total, dtype=np.float64))))}


# ------------------------------------------------------------------------------------------------ the inputs of the GPU tests
PARITY_F = (1, 15, 16, 17, 65, 128)          # the 16-frame stride of the frame products, its ragged tail, a full wave of frames, the maximum
PARITY_K = (1, 3, 64)
PARITY_SETS, PARITY_C = 5, 3
PARITY_PARAMS = tuple((float(np.float32(lam)), float(np.float32(b))) for lam in (0.0, 0.05, 1.0) for b in (NEG_INF, 0.1))   # as fp32 holds them


def parity_shapes():
    return [(F, K) for F in PARITY_F for K in PARITY_K]


@functools.lru_cache(maxsize=None)
def parity_case(F, K):
    """moment_ref.parity_case's frames (norm about 28) and prefix masks; unit label vectors [5, K, 768] from a seeded generator, the
    slots past a set's count NaN (they are never read); counts mixing K, 1 and values between; rows [5, 3]: gallery rows, among them
    row 0 (every frame valid) and one id outside the gallery."""
    frames, mask, _, _ = R.parity_case(F, 5)
    rng = np.random.RandomState(11000 + 131 * F + K)
    q = rng.standard_normal((PARITY_SETS, K, H))
    q /= np.linalg.norm(q, axis=2, keepdims=True)
    counts = np.array([K, 1, (K + 1) // 2, K, max(1, K - 1)], dtype=np.int32)
    for i in range(PARITY_SETS):
        q[i, counts[i]:] = np.nan
    rows = rng.randint(0, R.PARITY_ROWS, size=(PARITY_SETS, PARITY_C)).astype(np.int32)
    rows[0, 0], rows[1, 1], rows[3, 2] = 0, -1, 0
    return frames, mask, q.astype(np.float32), counts, rows


@functools.lru_cache(maxsize=None)
def parity_scores(F, K, i, r, normalize):
    """The float64 (E, vf) of set i of parity_case(F, K) on gallery row r."""
    frames, mask, q, counts, _ = parity_case(F, K)
    return frame_scores(q[i, :counts[i]], frames[r], mask[r], normalize)


@functools.lru_cache(maxsize=None)
def parity_reference(F, K, normalize):
    """{(lam, b): segment(...)} of parity_case(F, K) in one mode."""
    frames, mask, q, counts, rows = parity_case(F, K)
    return segment_many(q, counts, frames, mask, rows, PARITY_PARAMS, normalize, scores=lambda i, r: parity_scores(F, K, i, r, normalize))


EXACT_F = (8, 17, 128)
EXACT_COUNTS = (1, 2, 7, 64)
EXACT_PARAMS = tuple((float(lam), b) for lam in (0, 3, 4000, 10 ** 7) for b in (NEG_INF, 0.0, 2500.0))


@functools.lru_cache(maxsize=None)
def exact_case(F):
    """Integer frames and label vectors in [-8, 8]: every frame score is an integer of magnitude at most 49152 under use_mil and every
    sum of at most 128 of them, and such a sum less an integer penalty of at most 10^7, is an integer below 2^24: exact in fp32.  7 rows:
    prefix masks, row 3 a single valid frame, row 4 a mask with holes, row 5 one frame repeated, row 6 a block of 3 frames repeated.
    Sets of 1, 2, 7 and 64 labels padded to K = 64, each against all 7 rows; in the last two sets label 1 repeats label 0 (equal scores
    on every frame: the lower label wins)."""
    rng = np.random.RandomState(600 + F)
    frames = rng.randint(-8, 9, size=(7, F, H)).astype(np.float32)
    frames[5] = frames[5, 0]
    frames[6] = frames[6, np.arange(F) % 3]
    mask = np.zeros((7, F), dtype=np.int64)
    for r, n in enumerate([F, max(1, F // 2), max(1, F - 1), 1, F, F, F]):
        mask[r, :n] = 1
    mask[3] = 0
    mask[3, F // 2] = 1
    mask[4, 1::3] = 0
    q = rng.randint(-8, 9, size=(len(EXACT_COUNTS), K_MAX, H)).astype(np.float32)
    q[2:, 1] = q[2:, 0]
    counts = np.array(EXACT_COUNTS, dtype=np.int32)
    rows = np.stack([rng.permutation(7) for _ in EXACT_COUNTS]).astype(np.int32)
    return frames, mask, q, counts, rows


@functools.lru_cache(maxsize=None)
def exact_reference(F):
    frames, mask, q, counts, rows = exact_case(F)
    return segment_many(q, counts, frames, mask, rows, EXACT_PARAMS, False)


def from_scores(E, F=None, valid=None):
    """Inputs whose frame scores under use_mil ARE the integers E [n, T]: label k is the unit vector of coordinate k, frame f_t holds
    E[k, t] in coordinate k.  valid: the T frame indices among F frames (default: all T).  Returns (frames [1, F, H], mask [1, F],
    q [1, n, H])."""
    E = np.asarray(E, dtype=np.float32)
    n, T = E.shape
    F = T if F is None else F
    valid = np.arange(T) if valid is None else np.asarray(valid)
    frames = np.full((1, F, H), 7.0, dtype=np.float32)                    # a masked frame would score 7 for every label, were it read
    mask = np.zeros((1, F), dtype=np.int64)
    frames[0, valid] = 0.0
    frames[0, valid, :n] = E.T
    mask[0, valid] = 1
    q = np.zeros((1, n, H), dtype=np.float32)
    q[0, np.arange(n), np.arange(n)] = 1.0
    return frames, mask, q


# Constructed ties: (name, E [n, T], lam, b, the labelling the contract gives with the background as n).
TIES = (
    ("lower label wins", [[5, 5, 5], [5, 5, 5]], 1.0, NEG_INF, [0, 0, 0]),
    ("label beats background", [[2, 2, 2]], 0.0, 2.0, [0, 0, 0]),
    ("background only when strictly larger", [[2, 1, 3]], 0.0, 2.0, [0, 1, 0]),
    # a tie stays even at lambda 0: once in the background, frame 2's equal scores keep it there
    ("the background stays on a tie once entered", [[2, 1, 2]], 0.0, 2.0, [0, 1, 1]),
    # 10 + 3 staying = 10 + 5 - 2 switching: stay
    ("stay beats switch", [[10, 3], [0, 5]], 2.0, NEG_INF, [0, 0]),
    ("one more and it switches", [[10, 3], [0, 6]], 2.0, NEG_INF, [0, 1]),
    # leaving label 0 for the background and returning costs 2 * 2 and gains 4: 18 either way, stay
    ("stay beats a detour over the background", [[9, 0, 9]], 2.0, 4.0, [0, 0, 0]),
    ("per-frame arg-max at lambda 0", [[1, 9, 1, 9], [9, 1, 9, 1], [9, 9, 0, 0]], 0.0, 5.0, [1, 0, 1, 0]),
    ("a large lambda keeps one label", [[1, 9, 1, 9], [9, 1, 9, 2], [0, 0, 0, 0]], 100.0, -50.0, [1, 1, 1, 1]),
)
