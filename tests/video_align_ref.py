"""Video-to-video alignment in numpy (include/univl_hip.h: univl_video_align): the contract's programme in float64, an exhaustive
enumeration of every monotone path to hold it against, the six outputs as the kernel writes them, and the cases the CPU and GPU tests
share.  Nothing here imports the package."""
import functools

import numpy as np

H = 768
NEG_INF = float("-inf")
MOVES = ((1, 1), (1, 0), (0, 1))                 # diagonal, up, left: the order that decides among equal predecessors


# ------------------------------------------------------------------------------------------------ the contract
def cell_scores(xa, ma, xb, mb, tau):
    """(E [Ta, Tb] float64, fa, gb): e(i, j) = cos(x_{f_i}, y_{g_j}) - tau over the valid frames of the two videos."""
    fa, gb = np.nonzero(np.asarray(ma) != 0)[0], np.nonzero(np.asarray(mb) != 0)[0]
    A, B = np.asarray(xa, dtype=np.float64)[fa], np.asarray(xb, dtype=np.float64)[gb]
    na = np.maximum(np.sqrt((A * A).sum(1)), 1e-12)
    nb = np.maximum(np.sqrt((B * B).sum(1)), 1e-12)
    return (A @ B.T) / (na[:, None] * nb[None, :]) - float(tau), fa, gb


def programme(E, local):
    """The programme of the contract on cell scores E [Ta, Tb] (in E's own dtype: additions and comparisons only).  Returns (score,
    path): H at the end cell and the path's cells (i, j), first to last."""
    E = np.asarray(E)
    Ta, Tb = E.shape
    Hh = np.zeros_like(E)
    code = np.zeros((Ta, Tb), dtype=np.int8)
    for i in range(Ta):
        for j in range(Tb):
            pm, c = None, 3
            if i > 0 and j > 0:
                pm, c = Hh[i - 1, j - 1], 0
            if i > 0 and (c == 3 or Hh[i - 1, j] > pm):
                pm, c = Hh[i - 1, j], 1
            if j > 0 and (c == 3 or Hh[i, j - 1] > pm):
                pm, c = Hh[i, j - 1], 2
            if c == 3 or (local and pm <= 0):
                Hh[i, j], code[i, j] = E[i, j], 3
            else:
                Hh[i, j], code[i, j] = E[i, j] + pm, c
    if local:
        i, j = np.unravel_index(np.argmax(Hh), Hh.shape)                  # the first maximum in row-major order: lowest i, then lowest j
    else:
        i, j = Ta - 1, Tb - 1
    score, path = Hh[i, j], []
    while True:
        path.append((int(i), int(j)))
        c = code[i, j]
        if c == 3:
            break
        i, j = i - (c != 2), j - (c != 1)
    return score, path[::-1]


def enumerate_best(E, local):
    """The largest sum of E over every monotone path (moves diagonal, up, left): from (0, 0) to the last cell, or with local between
    any two cells.  Exhaustive; small tables only."""
    E = np.asarray(E, dtype=np.float64)
    Ta, Tb = E.shape
    best = [NEG_INF]

    def walk(i, j, s):
        s += E[i, j]
        if local or (i, j) == (Ta - 1, Tb - 1):
            best[0] = max(best[0], s)
        for di, dj in MOVES:
            if i + di < Ta and j + dj < Tb:
                walk(i + di, j + dj, s)

    for i0, j0 in ([(i, j) for i in range(Ta) for j in range(Tb)] if local else [(0, 0)]):
        walk(i0, j0, 0.0)
    return best[0]


def path_objective(E, path):
    return float(sum(float(E[i, j]) for i, j in path))


def column_match(E, path, Tb):
    """(mi [Tb], ms [Tb]): for every column the path cell in it with the largest e, the lowest i among equals; (-1, -inf) unvisited."""
    mi, ms = np.full(Tb, -1, dtype=np.int64), np.full(Tb, NEG_INF)
    for i, j in path:
        if mi[j] < 0 or E[i, j] > ms[j]:
            mi[j], ms[j] = i, E[i, j]
    return mi, ms


def align(frames, mask, ref, rows, tau, local, dtype=np.float64):
    """The six outputs of univl_video_align, values in float64 (with dtype=np.float32 the programme runs on E rounded to fp32: the
    exact cases, where both agree to the bit)."""
    frames, mask = np.asarray(frames), np.asarray(mask)
    ref, rows = np.asarray(ref), np.asarray(rows)
    N, F = mask.shape
    P, C = rows.shape
    score = np.full((P, C), NEG_INF)
    path_len = np.zeros((P, C), dtype=np.int64)
    path_a, path_b = np.full((P, C, 2 * F), -1, dtype=np.int64), np.full((P, C, 2 * F), -1, dtype=np.int64)
    match, match_score = np.full((P, C, F), -2, dtype=np.int64), np.full((P, C, F), NEG_INF)
    for p in range(P):
        for c in range(C):
            a, b = int(ref[p]), int(rows[p, c])
            if not (0 <= a < N and 0 <= b < N) or not mask[a].any() or not mask[b].any():
                continue
            E, fa, gb = cell_scores(frames[a], mask[a], frames[b], mask[b], tau)
            E = E.astype(dtype)
            s, path = programme(E, local)
            mi, ms = column_match(E, path, len(gb))
            score[p, c], path_len[p, c] = s, len(path)
            path_a[p, c, :len(path)] = fa[[i for i, _ in path]]
            path_b[p, c, :len(path)] = gb[[j for _, j in path]]
            match[p, c, gb] = np.where(mi >= 0, fa[np.maximum(mi, 0)], -1)
            match_score[p, c, gb] = ms
    return score, path_len, path_a, path_b, match, match_score


def transfer(ref_labels, match):
    """VideoIndex.transfer_labels: the exemplar's label at match where match >= 0, else match's own -1 / -2."""
    ref_labels, match = np.asarray(ref_labels), np.asarray(match)
    P, C, F = match.shape
    got = np.take_along_axis(np.broadcast_to(ref_labels[:, None, :], (P, C, F)), np.maximum(match, 0), axis=2)
    return np.where(match >= 0, got, match)


def frame_counts(pred, gt):
    """eval_label_transfer's counters from predicted labels [P, C, F] and annotations of the same shape."""
    pred, gt = np.asarray(pred), np.asarray(gt)
    counted = (gt != -2) & (pred != -2)
    right = counted & (pred == gt)
    fg = counted & (gt >= 0)
    n, nfg = int(counted.sum()), int(fg.sum())
    return {"correct": right.sum(-1), "annotated": counted.sum(-1), "frame_accuracy": float(right.sum()) / n,
            "frame_accuracy_fg": float((right & fg).sum()) / nfg if nfg else float("nan"), "n_frames": n}


# ------------------------------------------------------------------------------------------------ exact inputs
def from_overlaps(Cm, F=None, valid_a=None, valid_b=None):
    """Two videos whose cell cosines are Cm[i, j] / 16 exactly: frames with 16 entries of +-1, frame i of a sharing |Cm[i, j]| <= 4
    private coordinates with frame j of b (opposite signs for a negative entry), the rest of each frame on coordinates of its own.
    Norms are 4, Gram entries integers: every e is a multiple of 1/16 in fp32 and fp64 alike.  Returns (frames [2, F, 768], mask
    [2, F]); valid_a / valid_b: the frame indices the Ta / Tb frames sit at (default: the first ones), the others masked and NaN-free
    garbage."""
    Cm = np.asarray(Cm, dtype=np.int64)
    Ta, Tb = Cm.shape
    assert Ta <= 4 and Tb <= 4 and np.abs(Cm).max() <= 4
    valid_a = np.arange(Ta) if valid_a is None else np.asarray(valid_a)
    valid_b = np.arange(Tb) if valid_b is None else np.asarray(valid_b)
    F = int(max(valid_a.max(), valid_b.max())) + 1 if F is None else F
    A, B = np.zeros((Ta, H), dtype=np.float32), np.zeros((Tb, H), dtype=np.float32)
    at = 0
    for i in range(Ta):
        for j in range(Tb):
            k = abs(int(Cm[i, j]))
            A[i, at:at + k] = 1.0
            B[j, at:at + k] = 1.0 if Cm[i, j] > 0 else -1.0
            at += 4
    for X in (A, B):
        for row in X:
            k = 16 - int(np.count_nonzero(row))
            row[at:at + k] = 1.0
            at += 16
    assert at <= H
    frames = np.full((2, F, H), 3.0, dtype=np.float32)                    # a masked frame: a value that would show if it were read
    mask = np.zeros((2, F), dtype=np.int64)
    frames[0, valid_a], frames[1, valid_b] = A, B
    mask[0, valid_a], mask[1, valid_b] = 1, 1
    return frames, mask


# name, overlaps Cm (e = Cm / 16 - tau), tau, local, the path the contract decides (positions)
TIES = [
    ("all zero, square: the diagonal before up and left", [[0, 0, 0], [0, 0, 0], [0, 0, 0]], 0.0, 0, [(0, 0), (1, 1), (2, 2)]),
    ("all zero, wide: the diagonal into the end cell, left before it", [[0, 0, 0], [0, 0, 0]], 0.0, 0, [(0, 0), (0, 1), (1, 2)]),
    ("all zero, tall: the diagonal into the end cell, up before it", [[0, 0], [0, 0], [0, 0]], 0.0, 0, [(0, 0), (1, 0), (2, 1)]),
    # H = [[0, 4], [4, 3]] / 16: at (1, 1) the diagonal holds 0, up 4, left 4 -> up
    ("up before left", [[0, 4], [4, -1]], 0.0, 0, [(0, 0), (0, 1), (1, 1)]),
    ("a column walked upwards: match takes the lowest of equal cells", [[2], [2], [2]], 0.0, 0, [(0, 0), (1, 0), (2, 0)]),
    ("local: equal ends, the lowest j", [[4, -4, 4], [-4, -4, -4]], 0.0, 1, [(0, 0)]),
    ("local: equal ends, the lowest i", [[-4, 4], [4, -4]], 0.0, 1, [(0, 1)]),
    ("local: Pm == 0 starts a path", [[4, -4, 4, 4]], 0.0, 1, [(0, 2), (0, 3)]),
    ("local: Pm == 0 starts a path, seen at the end", [[-4, 4, -4, 4]], 0.0, 1, [(0, 1)]),
    ("local with tau: a run of matches between mismatches", [[4, 0, 0, 0], [0, 4, 0, 0], [0, 0, 0, 4]], 0.125, 1, [(0, 0), (1, 1)]),
]


EXACT_F = (5, 33, 128)


@functools.lru_cache(maxsize=None)
def exact_case(F):
    """Videos whose frames hold 4 or 16 entries of +-1 on a few shared coordinates (norms 2 or 4, every e a multiple of 1/16, ties
    everywhere), prefix masks and holes.  (frames [4, F, 768], mask [4, F], ref [2], rows [2, 3])."""
    rng = np.random.RandomState(700 + F)
    frames = np.zeros((4, F, H), dtype=np.float32)
    for v in range(4):
        for f in range(F):
            k = 4 if rng.rand() < 0.5 else 16
            at = rng.choice(24, size=k, replace=False)                    # 24 shared coordinates: overlaps are common
            frames[v, f, at] = rng.choice([-1.0, 1.0], size=k, p=[0.2, 0.8])
    mask = np.ones((4, F), dtype=np.int64)
    mask[1, max(1, (2 * F) // 3):] = 0                                    # a prefix: Ta != Tb
    mask[2, 0] = 0 if F > 1 else 1                                        # a masked first frame
    mask[2, 3::5] = 0                                                     # holes
    mask[3, :] = 0
    mask[3, F // 2] = 1                                                   # a single valid frame
    ref = np.array([0, 2], dtype=np.int32)
    rows = np.array([[1, 2, 3], [0, 3, 2]], dtype=np.int32)
    return frames, mask, ref, rows


EXACT_TAUS = (0.0, 0.25, 0.5, 1.0)


@functools.lru_cache(maxsize=None)
def exact_reference(F, tau, local):
    frames, mask, ref, rows = exact_case(F)
    return align(frames, mask, ref, rows, tau, local, dtype=np.float32)


# ------------------------------------------------------------------------------------------------ fp64 parity
PARITY_F = (1, 2, 31, 32, 33, 65, 128)
PARITY_TAUS = (0.0, 0.5, 1.0)


@functools.lru_cache(maxsize=None)
def parity_case(F):
    """Five videos of one "task": a slowly drifting base sequence at LayerNorm scale, every video a time-warped, noisy copy.  Row 1 is a
    prefix, row 2 has holes and a masked first frame, row 3 a single valid frame, row 4 none.  (frames, mask, ref [2], rows [2, 4])."""
    rng = np.random.RandomState(900 + F)
    steps = rng.standard_normal((2 * F + 2, H))
    base = np.cumsum(steps, axis=0)
    base = base / np.linalg.norm(base, axis=1, keepdims=True) * 28.0
    frames = np.zeros((5, F, H), dtype=np.float32)
    for v in range(5):
        warp = np.sort(rng.randint(0, 2 * F + 2, size=F))
        frames[v] = base[warp] + rng.standard_normal((F, H)) * 0.3
    mask = np.ones((5, F), dtype=np.int64)
    mask[1, max(1, F // 2 + F // 4):] = 0
    if F > 1:
        mask[2, 0] = 0
        mask[2, 4::7] = 0
    mask[3, :] = 0
    mask[3, F - 1] = 1
    mask[4, :] = 0
    ref = np.array([0, 2], dtype=np.int32)
    rows = np.array([[1, 2, 3, 4], [1, 0, 2, 3]], dtype=np.int32)
    return frames, mask, ref, rows


@functools.lru_cache(maxsize=None)
def parity_scores(F, a, b):
    """(E at tau = 0, fa, gb) in float64 for the pair of rows (a, b) of parity_case(F)."""
    frames, mask, _, _ = parity_case(F)
    return cell_scores(frames[a], mask[a], frames[b], mask[b], 0.0)


def check_pair(out, p, c, E, fa, gb, F, local, tol):
    """The properties the GPU tests ask of one aligned pair against its float64 cell scores E (tau already subtracted): the path is
    monotone with legal moves between valid frames and has the right end points; match / match_score are the path's own; every
    match_score within tol of the float64 e; the float64 objective of the path RETURNED within path_len x tol of the float64 optimum;
    score within path_len x tol of that objective.  No path position is compared under a tolerance.  Returns (match_score error,
    objective gap per cell, score error per cell)."""
    score, path_len, path_a, path_b, match, match_score = out
    n = int(path_len[p, c])
    Ta, Tb = E.shape
    assert 1 <= n <= Ta + Tb - 1, (p, c, n)
    pa, pb = path_a[p, c], path_b[p, c]
    assert np.all(pa[n:] == -1) and np.all(pb[n:] == -1) and len(pa) == 2 * F, (p, c)
    posa, posb = {int(f): i for i, f in enumerate(fa)}, {int(g): j for j, g in enumerate(gb)}
    path = [(posa[int(x)], posb[int(y)]) for x, y in zip(pa[:n], pb[:n])]                     # KeyError: not a valid frame
    for (i0, j0), (i1, j1) in zip(path, path[1:]):
        assert (i1 - i0, j1 - j0) in MOVES, (p, c, path)
    if not local:
        assert path[0] == (0, 0) and path[-1] == (Ta - 1, Tb - 1), (p, c, path)
    r_score, _ = programme(E, local)
    obj = path_objective(E, path)
    gap, serr = abs(obj - float(r_score)), abs(float(score[p, c]) - obj)
    assert gap <= n * tol, (p, c, gap)
    assert serr <= n * tol, (p, c, serr)
    # match: decided among the path's own cells by the kernel's fp32 e, so only membership and the value are checked
    valid_b = np.zeros(F, dtype=bool)
    valid_b[gb] = True
    m, ms = match[p, c], match_score[p, c]
    assert np.all(m[~valid_b] == -2) and np.all(ms[~valid_b] == NEG_INF), (p, c)
    err = 0.0
    cols = {}
    for i, j in path:
        cols.setdefault(j, []).append(i)
    for j, g in enumerate(gb):
        if j not in cols:
            assert local and m[g] == -1 and ms[g] == NEG_INF, (p, c, g)
            continue
        i = posa[int(m[g])]
        assert i in cols[j], (p, c, g)
        err = max(err, abs(float(ms[g]) - float(E[i, j])))
        assert float(ms[g]) >= max(float(E[k, j]) for k in cols[j]) - 2 * tol, (p, c, g)
    assert err <= tol, (p, c, err)
    return err, gap / n, serr / n
