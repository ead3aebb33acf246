"""The fp64 reference of the clip + BertAdam kernels (csrc/optim.hip, csrc/adam_body.h), and the proof that the reference and the
bounds tests/test_optim_gpu.py applies are sound on their own -- no GPU, no library.

The reference restates modules/optimization.py in numpy float64, evaluated on the kernel's fp32 inputs and on the fp32-rounded constants
the kernel computes with (b1, 1.0f - b1, b2, 1.0f - b2, eps, lr, weight_decay):
    global clip      main_task_retrieval.py:347 (torch clip_grad_norm_)   coef = min(1, max_norm / (||g|| + 1e-6))
    per-tensor clip  optimization.py:135-136                              the same on one tensor, AFTER the global clip scaled it
    moments          optimization.py:141-143                              m' = b1 m + (1 - b1) g,  v' = b2 v + (1 - b2) g g
    update           optimization.py:144                                  m' / (sqrt(v') + e)      (no bias correction)
    weight decay     optimization.py:153-154                              update += weight_decay * p
    schedules        optimization.py:26-29, 31-36, 38-43                  warmup_cosine, warmup_constant, warmup_linear
    step             optimization.py:156-166                              p -= lr * schedule(step / t_total, warmup) * update; step += 1
It is tied to the pinned oracle (oracle/univl_oracle.py: bert_adam_step, clip_grad_norm_) to 1e-12.

Stagewise bounds, u = 2**-24 (what an fp32 evaluation in ANY association, FMA-contracted or not, stays inside: 8 = the rounded fp32
operations of a stage, the error of gr = g * gs entering v twice):
    |m' - ref| <= 8u S_m,   S_m = |m b1| + |(1 - b1) gr|
    |v' - ref| <= 8u S_v,   S_v = |v b2| + |(1 - b2) gr gr|
    |p' - ref| <= 8u S_p,   S_p = |p| + lr (|m'| / (sqrt(v') + eps) + wd |p|)      from the GIVEN m', v' (the evaluation's own outputs)
The p stage is chained behind the m / v stage instead of being bounded end to end: m' can cancel to far below S_m, and an end-to-end bound
on p would then have to allow everything.

Observed maxima of the plain numpy-fp32 restatement (test_fp32_restatement_stays_inside_the_stagewise_bounds, the families below at
gradient scales 1e-6 .. 30 and the device test's own buffer, 10 % exact zeros in g / m / v, lr in {3e-5, 1e-3}), in units of u S against the bound of 8:
    m stage 2.53      v stage 3.62      p stage 3.05
(the yardstick the kernel's own maxima in tests/test_optim_gpu.py are set next to)."""
import math

import numpy as np
import pytest
import torch

import univl_oracle as O

U = 2.0 ** -24
STAGE_BOUND = 8.0
GRAD_SCALES = (1e-6, 1e-3, 1.0, 30.0)
LRS = (3e-5, 1e-3)
B1, B2, EPS = 0.9, 0.999, 1e-6


def f32(x):
    """The double value of x rounded to fp32 (what a `float` field or literal of the kernel holds)."""
    return float(np.float32(x))


def family(n, scale, seed):
    """One tensor's fp32 p, g, m, v: gradients of the given scale, moments as a few steps at that scale leave them, 10 % exact zeros in
    each of g, m, v (independently, so every combination of zero / non-zero occurs) and 2 % where all three are."""
    r = np.random.RandomState(seed)
    p = (0.05 * r.standard_normal(n)).astype(np.float32)
    g = (scale * r.standard_normal(n)).astype(np.float32)
    m = (0.3 * scale * r.standard_normal(n)).astype(np.float32)
    v = (0.5 * (scale * r.standard_normal(n)) ** 2).astype(np.float32)
    for a in (g, m, v):
        a[r.random_sample(n) < 0.1] = 0.0
    both = r.random_sample(n) < 0.02            # ... and elements where all three are zero: the update is the weight decay alone
    both[n // 2] = n >= 4
    for a in (g, m, v):
        a[both] = 0.0
    return p, g, m, v


# ------------------------------------------------------------------------------------------------------ the fp64 restatement
def schedule_factor(x, warmup, schedule):
    """optimization.py:26-43 in Python doubles; schedule 0 warmup_linear, 1 warmup_cosine, 2 warmup_constant (UnivlAdam.schedule)."""
    if x < warmup:
        return x / warmup
    if schedule == 1:
        return 0.5 * (1.0 + math.cos(math.pi * x))          # :29
    if schedule == 2:
        return 1.0                                           # :36
    return max((x - 1.0) / (warmup - 1.0), 0.0)             # :43


def scheduled_lr(lr, step, t_total, warmup, schedule=0):
    """optimization.py:156-161."""
    if t_total == -1:
        return lr
    return lr * schedule_factor(step / t_total, warmup, schedule)


def global_clip(sumsqs, max_norm):
    """main_task_retrieval.py:347: (coef, total norm) from the per-tensor sums of squares of the tensors that take part."""
    total = math.sqrt(float(np.sum(np.asarray(sumsqs, dtype=np.float64))))
    return min(1.0, max_norm / (total + 1e-6)), total


def grad_scale(sumsq, gc, max_grad_norm):
    """What one tensor's gradient is multiplied by: the global coefficient gc, then optimization.py:135-136 on the tensor the global
    clip has already scaled (its norm is sqrt(sumsq) * gc)."""
    if max_grad_norm <= 0:
        return gc
    return gc * min(1.0, max_grad_norm / (math.sqrt(sumsq) * gc + 1e-6))


def _consts(b1, b2):
    b1, b2 = np.float32(b1), np.float32(b2)
    return float(b1), float(np.float32(1.0) - b1), float(b2), float(np.float32(1.0) - b2)       # b1, 1.0f - b1, b2, 1.0f - b2


def moments64(g, m, v, gs, b1=B1, b2=B2):
    """optimization.py:141-143 in float64 -> (m', v', S_m, S_v)."""
    b1, omb1, b2, omb2 = _consts(b1, b2)
    gr = g.astype(np.float64) * float(gs)
    m, v = m.astype(np.float64), v.astype(np.float64)
    return m * b1 + omb1 * gr, v * b2 + omb2 * gr * gr, np.abs(m * b1) + np.abs(omb1 * gr), np.abs(v * b2) + np.abs(omb2 * gr * gr)


def param64(p, m1, v1, lr, wd, eps=EPS):
    """optimization.py:144, 153-154, 163-164 in float64 from the given m', v' -> (p', S_p)."""
    p, m1, v1, lr, wd, eps = p.astype(np.float64), m1.astype(np.float64), v1.astype(np.float64), float(lr), f32(wd), f32(eps)
    den = np.sqrt(v1) + eps
    return p - lr * (m1 / den + wd * p), np.abs(p) + lr * (np.abs(m1) / den + wd * np.abs(p))


def stage_errors(p, g, m, v, p1, m1, v1, gs, lr, wd, b1=B1, b2=B2, eps=EPS):
    """Largest error of each stage of an fp32 result (p1, m1, v1) in units of u S: the m / v stage from the inputs, the p stage from
    the result's own m1, v1.  Where S = 0 the result must be exact (reported as 0, else inf)."""
    mr, vr, s_m, s_v = moments64(g, m, v, gs, b1, b2)
    pr, s_p = param64(p, m1, v1, lr, wd, eps)

    def worst(got, ref, s):
        err = np.abs(got.astype(np.float64) - ref)
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(s > 0, err / (U * s), np.where(err == 0, 0.0, np.inf))
        return float(q.max()) if q.size else 0.0
    return worst(m1, mr, s_m), worst(v1, vr, s_v), worst(p1, pr, s_p)


def step32(p, g, m, v, gs, lr, wd, b1=B1, b2=B2, eps=EPS):
    """The update as plain numpy fp32 arithmetic in the kernel's operation order (no FMA): the yardstick of the bounds."""
    f = np.float32
    b1, b2, eps, gs, lr, wd = f(b1), f(b2), f(eps), f(gs), f(lr), f(wd)
    gr = g * gs
    m1 = m * b1 + (f(1.0) - b1) * gr
    v1 = v * b2 + (f(1.0) - b2) * gr * gr
    upd = m1 / (np.sqrt(v1) + eps) + wd * p
    p1 = p - lr * upd
    assert p1.dtype == m1.dtype == v1.dtype == np.float32
    return p1, m1, v1


CASES = [(n, scale, lr, wd) for n in (1025,) for scale in GRAD_SCALES for lr in LRS for wd in (0.01, 0.0)]


# ------------------------------------------------------------------------------------------------------ the synthetic flat buffer
# (numel, offset modulo 4, active, row_len) per segment; tests/test_optim_gpu.py drives the C ABI on it.  Sizes around the vector width
# (1, 3, 4, 5), around one 256-thread trip of 4-vectors (1023, 1025), one full chunk and one element more (8192, 8193) and three chunks
# (2 * 8192 + 7); starts on and off the 16-byte boundary; an inactive tensor in the middle (NaN everywhere); a row-structured tensor of 520
# rows of 40; a second inactive tensor with FINITE data (a vector part and a tail) -- an update, a scaling or a sum that ran over it
# would change its bits, which NaN mostly hides.
CHUNK = 8192
ROW_LEN, ROW_STEP, ROW_FLAGGED = 40, 8160, 408
SEGMENTS = [(1, 0, 1, 0), (3, 0, 1, 0), (4, 1, 1, 0), (5, 0, 1, 0), (1023, 1, 1, 0), (1025, 0, 1, 0), (777, 0, 0, 0), (8192, 0, 1, 0),
            (8193, 2, 1, 0), (2 * 8192 + 7, 0, 1, 0), (520 * ROW_LEN, 0, 1, ROW_LEN), (1029, 0, 0, 0)]
INACTIVE_SEG, ROW_SEG, FINITE_INACTIVE_SEG = 6, 10, 11
SENTINEL = 12345.678
# chunk lengths per segment where they are not "CHUNK at a time": 8188 | 4100 (two-vector trip, single trip, no tail) | 4103 (... and a
# scalar tail) for the three-chunk tensor; the row tensor in steps of 204 rows, its SECOND chunk half a row longer, so that the third
# starts in the middle of row 408 (the kernel's floor / ceil row range) -- that row is the flagged one
CHUNK_LENS = {9: [8188, 4100, 4103], ROW_SEG: [ROW_STEP, ROW_STEP + ROW_LEN // 2, 520 * ROW_LEN - 2 * ROW_STEP - ROW_LEN // 2]}


class Layout:
    """offsets, chunk table and fp32 host images of p / g / m / v: sentinel guard bands before, between and behind the segments, NaN in
    the first inactive one, family() data at cycling gradient scales elsewhere (the second inactive one too); the row tensor is all-zero in g / m / v but for row
    ROW_FLAGGED (what UnivlAdam.row_flags promises of unflagged rows)."""

    def __init__(self, seed=0):
        self.segs, self.chunks = [], []
        cur = 8
        for s, (numel, mod, active, row_len) in enumerate(SEGMENTS):
            cur += 3
            cur += (mod - cur) % 4
            lr, wd, mgn = f32(LRS[s % 2]), f32((0.01, 0.0, 0.01)[(s + 1) % 3]), (1.0, 1.0, 0.0, -1.0)[s % 4]
            self.segs.append((cur, numel, lr, wd, mgn, active))
            o = 0
            for ln in CHUNK_LENS.get(s) or [min(CHUNK, numel - c) for c in range(0, numel, CHUNK)]:
                self.chunks.append((s, cur + o, ln))          # the inactive tensors are listed too: the kernels' own guards skip them
                o += ln
            assert o == numel
            cur += numel
        self.total = (cur + 8 + 3) // 4 * 4
        self.live = np.zeros(self.total, dtype=bool)                 # elements an update may write
        self.host = {k: np.full(self.total, SENTINEL, dtype=np.float32) for k in "pgmv"}
        for s, (off, numel, lr, wd, mgn, active) in enumerate(self.segs):
            sl = slice(off, off + numel)
            if s == INACTIVE_SEG:
                for k in "pgmv":
                    self.host[k][sl] = np.nan
                continue
            self.live[sl] = bool(active)
            p, g, m, v = family(numel, self.scale(s), seed=1000 * seed + s)
            if SEGMENTS[s][3]:
                keep = np.zeros(numel, dtype=bool)
                keep[ROW_FLAGGED * ROW_LEN:(ROW_FLAGGED + 1) * ROW_LEN] = True
                g, m, v = (np.where(keep, np.where(a == 0, np.float32(1e-3), a), np.float32(0)) for a in (g, m, v))
            for k, a in zip("pgmv", (p, g, m, v)):
                self.host[k][sl] = a

    @staticmethod
    def scale(s):
        return GRAD_SCALES[(s + s // 4) % len(GRAD_SCALES)]      # (not in step with the cycle of max_grad_norm)

    def chunks_of(self, s):
        return sum(1 for c in self.chunks if c[0] == s)

    def sumsq64(self, g=None):
        """Per tensor; NaN for the NaN tensor, and for the finite inactive one the sum of ITS squares (what a stale slot would hold)."""
        g = self.host["g"] if g is None else g
        return [float(np.sum(g[off:off + n].astype(np.float64) ** 2)) for off, n, _, _, _, _ in self.segs]

    def active_sumsq64(self):
        return [x for x, sg in zip(self.sumsq64(), self.segs) if sg[5]]


# ------------------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize("max_grad_norm", [1.0, -1.0])
@pytest.mark.parametrize("wd", [0.01, 0.0])
@pytest.mark.parametrize("scale", GRAD_SCALES)
def test_restatement_equals_the_pinned_oracle(scale, wd, max_grad_norm):
    """O.bert_adam_step in float64 on the same tensors: 1e-12 relative on p', m', v' and the step count.  The oracle's clip measures its
    norm in fp32 (clip_grad_norm_ converts), so the whole step is compared where the clip is exact on both sides -- switched off, or a
    tensor whose norm is below the limit (coefficient clamped to exactly 1) -- and on gradients scaled beforehand otherwise; the clip
    itself is tied in test_clip_equals_the_pinned_oracle."""
    p, g, m, v = family(1025, scale, seed=11)
    lr, warmup, t_total, step = f32(1e-3), 0.1, 50, 7
    sumsq = float(np.sum(g.astype(np.float64) ** 2))
    gs = grad_scale(sumsq, 1.0, max_grad_norm)
    below = math.sqrt(sumsq) < 0.5
    assert max_grad_norm <= 0 or below or gs < 1.0
    lr_s = scheduled_lr(lr, step, t_total, warmup)
    m1, v1, _, _ = moments64(g, m, v, gs)
    p1, _ = param64(p, m1, v1, lr_s, wd)
    t = lambda a: torch.from_numpy(a.astype(np.float64))
    if max_grad_norm > 0 and not below:
        tg, mgn = t(g) * gs, -1.0         # the scaled gradient, the oracle's own clip off
    else:
        tg, mgn = t(g), max_grad_norm
    tp, tm, tv = t(p), t(m), t(v)
    b1, omb1, b2, omb2 = _consts(B1, B2)
    assert O.bert_adam_step(tp, tg, tm, tv, step, lr, warmup, t_total, f32(wd), b1=b1, b2=b2, e=f32(EPS), max_grad_norm=mgn) == step + 1
    # the oracle forms 1 - b1 in double from the fp32-rounded b1; the kernel's 1.0f - b1 is the same number (the subtraction is exact)
    assert omb1 == 1.0 - b1 and omb2 == 1.0 - b2
    for got, ref in ((p1, tp), (m1, tm), (v1, tv)):
        ref = ref.numpy()
        assert np.all(np.abs(got - ref) <= 1e-12 * np.abs(ref)), float(np.abs(got - ref).max())


@pytest.mark.parametrize("scale", GRAD_SCALES)
def test_clip_equals_the_pinned_oracle(scale):
    """O.clip_grad_norm_ on ONE tensor (its multi-tensor norm is an fp32 norm of fp32 norms).  Its norm is an fp32 sum of n non-negative
    squares and a square root: (n / 2 + 2) u relative in the worst case, in any order of summation."""
    n = 1025
    _, g, _, _ = family(n, scale, seed=12)
    coef, total = global_clip([np.sum(g.astype(np.float64) ** 2)], 1.0)
    tg = torch.from_numpy(g.astype(np.float64))
    tot = float(O.clip_grad_norm_([tg], 1.0))
    tol = (n / 2 + 2) * U
    assert abs(tot - total) <= tol * total
    assert grad_scale(total * total, 1.0, 1.0) == pytest.approx(coef, rel=1e-15)
    ref = g.astype(np.float64) * coef
    assert np.all(np.abs(tg.numpy() - ref) <= (tol + 2 * U) * np.abs(ref))
    if total < 0.5:
        assert coef == 1.0 and np.array_equal(tg.numpy(), g.astype(np.float64))


def test_schedules_in_doubles():
    """The three schedules at the points the device test walks (t_total 50, warmup 0.1): 0 at step 0, the ramp, the boundary step (the
    first one past the ramp: warmup_cosine leaves 1 there, the other two do not), zero from t_total on for warmup_linear."""
    for sched, fn in ((0, O.warmup_linear),):
        for s in range(53):
            assert schedule_factor(s / 50, 0.1, sched) == fn(s / 50, 0.1)
    for sched in (0, 1, 2):
        assert schedule_factor(0.0, 0.1, sched) == 0.0
        assert schedule_factor(3 / 50, 0.1, sched) == (3 / 50) / 0.1
    assert not 5 / 50 < 0.1
    assert schedule_factor(5 / 50, 0.1, 0) == 1.0 and schedule_factor(5 / 50, 0.1, 2) == 1.0
    assert schedule_factor(5 / 50, 0.1, 1) == 0.5 * (1.0 + math.cos(math.pi * 0.1)) < 0.98
    assert schedule_factor(1.0, 0.1, 0) == 0.0 and schedule_factor(52 / 50, 0.1, 0) == 0.0
    assert schedule_factor(52 / 50, 0.1, 2) == 1.0
    assert scheduled_lr(0.25, 7, -1, 0.1, 1) == 0.25


def test_fp32_restatement_stays_inside_the_stagewise_bounds(capsys):
    """The bounds' own proof: a plain fp32 evaluation must sit well inside 8u S at every stage, on every family the device test uses.
    The p stage is checked from the evaluation's OWN m', v' and chained behind the m / v stage (module docstring)."""
    worst = [0.0, 0.0, 0.0]
    lay = Layout()
    tensors = [family(n, scale, seed=100 + i) + (lr, wd) for i, (n, scale, lr, wd) in enumerate(CASES)]
    tensors += [tuple(lay.host[k][off:off + n] for k in "pgmv") + (lr, wd) for off, n, lr, wd, _, active in lay.segs if active]
    for p, g, m, v, lr, wd in tensors:
        scale = float(np.abs(g).max())
        for gs in (1.0, 0.37):
            for factor in (1.0, 0.6, 0.0):
                lr_s = f32(f32(lr) * f32(factor))
                p1, m1, v1 = step32(p, g, m, v, gs, lr_s, wd)
                e = stage_errors(p, g, m, v, p1, m1, v1, f32(gs), lr_s, wd)
                assert max(e) <= STAGE_BOUND, (scale, lr, wd, gs, factor, e)
                worst = [max(a, b) for a, b in zip(worst, e)]
                if factor == 0.0:
                    assert np.array_equal(p1, p)
                z = (g == 0) & (m == 0) & (v == 0)
                assert (z.any() or g.size < 4) and np.array_equal(p1[z], (p - np.float32(lr_s) * (np.float32(wd) * p))[z])
                assert not np.any(m1[z]) and not np.any(v1[z])
    with capsys.disabled():
        print("\n[optim] fp32 restatement, largest stage errors in u*S (bound %g): m %.2f  v %.2f  p %.2f" % (STAGE_BOUND, *worst))
    assert max(worst) <= STAGE_BOUND / 2, worst             # (the module docstring records the figures: under half of the bound)


def test_the_bounds_notice_what_they_are_for():
    """Each stage's bound refuses the mistakes the device test exists to catch: eps inside the square root, a dropped clip factor,
    one element that did not take part."""
    p, g, m, v = family(1025, 1e-3, seed=7)
    f = np.float32
    gs, lr, wd = f32(0.37), f32(1e-3), 0.01
    p1, m1, v1 = step32(p, g, m, v, gs, lr, wd)
    bad_p = p - f(lr) * (m1 / np.sqrt(v1 + f(EPS)) + f(wd) * p)
    assert stage_errors(p, g, m, v, bad_p, m1, v1, gs, lr, wd)[2] > 100 * STAGE_BOUND
    _, bm, bv = step32(p, g, m, v, 1.0, lr, wd)
    e = stage_errors(p, g, m, v, p1, bm, bv, gs, lr, wd)
    assert e[0] > 100 * STAGE_BOUND and e[1] > 100 * STAGE_BOUND
    skipped = m1.copy()
    i = int(np.argmax(np.abs(m1 - m)))
    skipped[i] = m[i]
    assert stage_errors(p, g, m, v, p1, skipped, v1, gs, lr, wd)[0] > 100 * STAGE_BOUND


def test_layout_is_what_the_device_test_needs():
    lay = Layout()
    offs = [s[0] for s in lay.segs]
    assert {o % 4 for o in offs} >= {0, 1, 2} and 55000 < lay.total < 65000 and lay.total % 4 == 0
    lens = [c[2] for c in lay.chunks]
    assert {8192, 8188, 4100, 1, 3, ROW_STEP} <= set(lens) and max(lens) <= 8192
    for s in (INACTIVE_SEG, FINITE_INACTIVE_SEG):
        assert any(c[0] == s for c in lay.chunks) and not lay.segs[s][5] and not lay.live[lay.segs[s][0]]
    assert math.isnan(lay.sumsq64()[INACTIVE_SEG]) and lay.sumsq64()[FINITE_INACTIVE_SEG] > 0
    # full 8192-element chunks on the vector path and on the scalar path
    assert any(ln == 8192 and off % 4 == 0 for _, off, ln in lay.chunks) and any(ln == 8192 and off % 4 for _, off, ln in lay.chunks)
    prev_end = 0
    for off, n, _, _, _, _ in lay.segs:            # a guard band before every segment, and one behind the last
        assert off - prev_end >= 3 and np.all(lay.host["p"][prev_end:off] == np.float32(SENTINEL))
        prev_end = off + n
    assert lay.total - prev_end >= 8
    row_chunks = [(off - lay.segs[ROW_SEG][0], ln) for s, off, ln in lay.chunks if s == ROW_SEG]
    assert [o % ROW_LEN for o, _ in row_chunks] == [0, 0, ROW_LEN // 2] and row_chunks[2][0] // ROW_LEN == ROW_FLAGGED
    norms = [math.sqrt(x) for x, sg in zip(lay.sumsq64(), lay.segs) if sg[5] and sg[4] > 0]
    assert min(norms) < 0.5 and max(norms) > 2.0           # per-tensor clip: both sides of the limit
