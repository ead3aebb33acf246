"""Numpy restatement of query-bank normalised search (include/univl_hip.h: univl_sim_colstat, univl_sim_topk_norm, univl_hub_flags,
univl_hub_gate) -- the reference of tests/test_qbnorm_gpu.py, checked by itself in tests/test_qbnorm_cpu.py.

Everything takes SCORE MATRICES (s[i, j] = score of query or bank row i against gallery row j), so a test decides where the scores
come from: int64 products where they are exact, fp64 products where a tolerance applies, the device's own scores where only the steps
after them are under test.  Order everywhere: larger score first, equal scores by LOWER gallery row first."""
import numpy as np


def ranked(s):
    """[rows, Ng] gallery rows of every row of s in the order of the tie rule."""
    return np.stack([np.lexsort((np.arange(s.shape[1]), -row)) for row in s])


def colstat(s_bank, beta):
    """c[j] = log(sum_b exp(beta s_bank[b, j])) / beta in fp64, max-shifted."""
    s = np.asarray(s_bank, dtype=np.float64)
    m = s.max(axis=0)
    return m + np.log(np.exp(beta * (s - m)).sum(axis=0)) / beta


def hub_flags(s_bank, hub_k):
    """hub[j] = 1 iff j is among the hub_k best gallery rows of some bank row."""
    hub = np.zeros(s_bank.shape[1], dtype=np.int32)
    hub[ranked(s_bank)[:, :hub_k].reshape(-1)] = 1
    return hub


def hub_gate(s_query, hub, dynamic=True):
    """gate[i] = hub[raw top-1 of query i]; all ones when not dynamic."""
    if not dynamic:
        return np.ones(s_query.shape[0], dtype=np.int32)
    return hub[ranked(s_query)[:, 0]].astype(np.int32)


def normalised(s_query, c, gate):
    """s' in fp32: ONE fp32 subtraction s - c where gate is set, s untouched elsewhere."""
    s = np.asarray(s_query, dtype=np.float32)
    sub = s - np.asarray(c, dtype=np.float32)[None, :]
    return np.where(np.asarray(gate)[:, None] != 0, sub, s).astype(np.float32)


def search(sp, k, target=None):
    """univl_sim_topk's outputs on the score matrix sp: (idx [Nq, k] with -1 tails, score [Nq, k] fp32 with -inf tails) and, with
    target, (gt, eq)."""
    Nq, Ng = sp.shape
    order = ranked(sp)
    n = min(k, Ng)
    idx = np.full((Nq, k), -1, dtype=np.int64)
    score = np.full((Nq, k), -np.inf, dtype=np.float32)
    idx[:, :n] = order[:, :n]
    score[:, :n] = np.take_along_axis(sp, order[:, :n], axis=1)
    if target is None:
        return idx, score
    ts = sp[np.arange(Nq), np.asarray(target)]
    return idx, score, (sp > ts[:, None]).sum(1), (sp == ts[:, None]).sum(1)


def hub_case(H=768):
    """The hand-made case: gallery rows j < 8 are 8 e_j and row 8, the hub, is 3 on the first eight coordinates; query i is 3 at
    coordinate i and 1 at the other seven; the bank is the same eight vectors; a ninth query is 9 e_0.  All integers.
    Raw scores of the eight: 24 for the true video, 8 for the others, 30 for the hub.  Returns (queries [9, H], gallery [9, H],
    bank [8, H]) as float32."""
    g = np.zeros((9, H), dtype=np.float32)
    g[np.arange(8), np.arange(8)] = 8.0
    g[8, :8] = 3.0
    q = np.zeros((9, H), dtype=np.float32)
    q[:8, :8] = 1.0
    q[np.arange(8), np.arange(8)] = 3.0
    q[8, 0] = 9.0
    return q, g, q[:8].copy()
