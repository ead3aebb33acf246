"""numpy restatement of the decoding-constraint contract (include/univl_hip.h: univl_decode_constrain), shared by
tests/test_constrain_cpu.py (hand-worked cases) and tests/test_constrain_gpu.py (the kernel bit for bit, and the reference beam loop).
Written from the header's words, row by row and n-gram by n-gram; it shares no code with the package."""
import numpy as np


def banned_by_ngram(p, t, n):
    """The set of tokens that would complete an n-gram already in p[0 .. t)."""
    out = set()
    if n < 1:
        return out
    tail = [int(v) for v in p[t - n + 1:t]] if n > 1 else []
    for j in range(0, t - n + 1):
        if [int(v) for v in p[j:j + n - 1]] == tail:
            out.add(int(p[j + n - 1]))
    return out


def constrain_ref(x, V, prefix, t, done, ngram, min_len, eos, suppress, done_stride=1):
    """x [R, ld] float32, prefix [R, >= t] integer tokens (each row's tokens at positions 0 .. t-1), done [ceil(R / done_stride)] or None.
    Returns a copy of x with the banned columns of every live row at -inf; columns >= V and the rows of done instances are not
    touched, ids outside [0, V) are skipped."""
    y = np.array(x, dtype=np.float32, copy=True)
    for r in range(y.shape[0]):
        if done is not None and done[r // done_stride]:
            continue
        ban = banned_by_ngram(prefix[r], t, ngram) if t > 0 else set()
        if t < min_len and eos >= 0:
            ban.add(int(eos))
        ban.update(int(v) for v in suppress)
        for v in ban:
            if 0 <= v < V:
                y[r, v] = -np.inf
    return y


def advance_prefix(prefix_in, src, last, t, before=None):
    """The prefix update of the beam form: row r continues row src[r] (None: the identity) and has emitted last[r] at position t-1.
    before: what prefix_out held (columns >= t keep it; default zeros).  t == 0 writes nothing."""
    R, Tmax = prefix_in.shape
    out = np.zeros_like(prefix_in) if before is None else np.array(before, copy=True)
    if t == 0:
        return out
    for r in range(R):
        s = r if src is None else int(src[r])
        out[r, :t - 1] = prefix_in[s, :t - 1]
        out[r, t - 1] = int(last[r])
    return out
