"""Kernel-level parity of the clip + BertAdam family (csrc/optim.hip, csrc/adam_body.h) against the fp64 restatement of
tests/test_optim_cpu.py: every exported optimizer entry point and every launch form that can carry BertAdam chunks, driven through the C
ABI on ONE synthetic flat buffer of ~57 000 elements (test_optim_cpu.Layout) -- no model, no training loop, no graph.

Every buffer (p, g, m, v, p16, p16_lo) has sentinel guard bands before, between and behind the segments, an inactive NaN tensor in the
middle and an inactive tensor of finite data, both listed in the chunk table; every test asserts that none of those bytes changed.  Needs a real MI355X (`-m gpu`).

Bounds: the stagewise 8u S bounds of test_optim_cpu (u = 2**-24) on the kernel's outputs, from the kernel's own previous state and its
own per-tensor scalars (which test_prep_scalars_* gate on their own).  Largest errors observed on the MI355X, in u S, next to the plain
fp32 restatement's (test_optim_cpu: m 2.53, v 3.62, p 3.05):   m 1.94   v 3.50   p 2.76
(gradient norm 1.02 u of a bound of 43 u and more; gradient scale 0.62 u of 4 u; scheduled lr 1.57 u lr of 8 u lr).

The launch forms are compared on NON-ZERO moments: with the update left to the compiler's contraction, the kernels that carry chunks
(adam_chunk) and adam_apply_kernel rounded m and v differently in the last bit; adam_body.h now states the element update once, with
its multiply-adds written out."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import test_optim_cpu as R
from test_optim_cpu import U

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import univl_amd
    from univl_amd import ops, _lib

DEV = "cuda"
EINVAL = -1
KEYS = ("p", "g", "m", "v", "p16", "p16_lo")
_LAY = None


def layout():
    global _LAY
    if _LAY is None:
        _LAY = R.Layout()
    return _LAY


def bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


class State:
    """Device copies of the layout's buffers + tables; sumsq is the fp32 rounding of the fp64 sums (the gradient-norm kernel has its
    own test); the NaN tensor's slot is NaN, the finite inactive tensor's slot holds the finite sum of its own squares."""

    def __init__(self, lay=None, src=None):
        lay = self.lay = lay or layout()
        if src is not None:
            for k in KEYS + ("sumsq", "step", "scal", "coef"):
                setattr(self, k, getattr(src, k).clone())
            self.tb = src.tb
        else:
            for k in "pgmv":
                setattr(self, k, torch.from_numpy(lay.host[k]).to(DEV))
            self.p16 = self.p.to(torch.bfloat16)
            self.p16_lo = (self.p - self.p16.float()).to(torch.bfloat16)
            self.tb = ops.adam_tables(lay.segs, lay.chunks, DEV)
            self.sumsq = torch.tensor(lay.sumsq64(), dtype=torch.float64).to(torch.float32).to(DEV)
            self.step = torch.full((len(lay.segs),), 7, dtype=torch.int32, device=DEV)
            self.scal = torch.full((2 * len(lay.segs),), -77.0, device=DEV)
            gc, _ = R.global_clip(lay.active_sumsq64(), 1.0)
            self.coef = torch.tensor([gc, 0.0], device=DEV)
        self.orig = {k: getattr(self, k).clone() for k in KEYS}
        self.dead = torch.from_numpy(~lay.live).to(DEV)

    def clone(self):
        return State(self.lay, self)

    def desc(self, shadows=2, coef=True, **kw):
        kw.setdefault("warmup", 0.1)
        kw.setdefault("t_total", 50)
        return ops.adam_desc(self.tb, self.p, self.g, self.m, self.v, sumsq=self.sumsq, step=self.step, seg_scalars=self.scal,
                             p16=self.p16 if shadows >= 1 else None, p16_lo=self.p16_lo if shadows >= 2 else None,
                             coef=self.coef if coef else None, b1=R.B1, b2=R.B2, eps=R.EPS, **kw)

    def assert_guards(self, also_unchanged=()):
        """Guard bands and the inactive tensor bit-unchanged in all six buffers (and the whole of the buffers named)."""
        torch.cuda.synchronize()
        for k in KEYS:
            a, b = bits(getattr(self, k)), bits(self.orig[k])
            assert torch.equal(a[self.dead], b[self.dead]), "guard band / inactive tensor of %s written" % k
            if k in also_unchanged:
                assert torch.equal(a, b), "%s changed" % k
        assert math.isnan(float(self.sumsq[R.INACTIVE_SEG]))

    def host(self, k):
        return getattr(self, k).float().cpu().numpy()


def same_state(a, b, keys=KEYS):
    torch.cuda.synchronize()
    for k in keys:
        x, y = bits(getattr(a, k)), bits(getattr(b, k))
        if not torch.equal(x, y):
            i = int((x != y).nonzero()[0])
            s = max(s for s, sg in enumerate(a.lay.segs) if sg[0] <= i)
            raise AssertionError("%s: %d elements differ, first at %d (tensor %d + %d): %r vs %r, largest bit distance %d"
                                 % (k, int((x != y).sum()), i, s, i - a.lay.segs[s][0], float(getattr(a, k)[i]), float(getattr(b, k)[i]),
                                    int((x.long() - y.long()).abs().max())))
    assert torch.equal(a.step, b.step)


def rc_of(fn, *args):
    rc = fn(*args)
    return rc, _lib.lib().univl_last_error().decode()


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---------------------------------------------------------------------------------------------------------------- gradient norm
def sumsq_bound(lay, s):
    return (32 + 8 + lay.chunks_of(s) + 2) * U          # per-thread adds, the block tree, one add per chunk


@pytest.mark.parametrize("det", [False, True])
def test_grad_sumsq_vs_fp64(det):
    """univl_grad_sumsq, atomic and deterministic mode: all terms non-negative, so the relative error is bounded by the number of
    rounded adds on an element's way into the sum.  Both modes ADD to what sumsq holds (the step's callers rely on it)."""
    lay, st = layout(), State()
    ref = lay.sumsq64()
    was = univl_amd.deterministic()
    try:
        univl_amd.set_deterministic(det)
        outs = []
        for rep in range(2):
            base = [0.0 if rep == 0 else 0.5 * x + 0.25 for x in ref]
            base[R.INACTIVE_SEG], base[R.FINITE_INACTIVE_SEG] = float("nan"), 5.5          # inactive: the slot keeps its bits
            out = torch.tensor(base, dtype=torch.float64).to(torch.float32).to(DEV)
            for _ in range(2 if det else 1):
                o = out.clone()
                ops.grad_sumsq(st.g, st.tb, o)
                outs.append(o)
            got, b32 = outs[-1].double().cpu().numpy(), out.double().cpu().numpy()
            worst = 0.0
            for s, sg in enumerate(lay.segs):
                if not sg[5]:
                    assert torch.equal(bits(outs[-1])[s], bits(out)[s]), s
                    continue
                want = b32[s] + ref[s]
                err = abs(got[s] - want) / want
                worst = max(worst, err / U)
                assert err <= sumsq_bound(lay, s), (s, got[s], want, err / U)
            print("[optim] grad_sumsq det=%d rep=%d: largest error %.2f u" % (det, rep, worst))
            if det:
                assert torch.equal(bits(outs[-1]), bits(outs[-2])), "deterministic mode: two runs differ"
        st.assert_guards(also_unchanged=KEYS)
    finally:
        univl_amd.set_deterministic(was)


def test_clip_coef_cases():
    lay, st = layout(), State()
    act = lay.active_sumsq64()
    band = torch.full((10,), -5.0, device=DEV)              # coef with a guard band around it
    coef = band[4:6]
    inactive = torch.tensor([not sg[5] for sg in lay.segs], device=DEV)
    # norm above the limit; the inactive tensors' slots (one NaN, one finite) do not take part
    ops.clip_coef(st.sumsq, st.tb, 1.0, coef)
    gc, total = R.global_clip(act, 1.0)
    c = coef.double().cpu().numpy()
    bound = max(sumsq_bound(lay, s) for s in range(len(lay.segs))) + 2 * U
    assert total > 100 and abs(c[1] - total) <= bound * total, (c[1], total)
    assert abs(c[0] - gc) <= (bound + 2 * U) * gc, (c[0], gc)              # one add and one division more
    # norm below the limit: exactly 1
    ops.clip_coef(st.sumsq, st.tb, 1e6, coef)
    assert float(coef[0]) == 1.0 and abs(float(coef[1]) - total) <= bound * total
    small = torch.where(inactive, st.sumsq, torch.full_like(st.sumsq, 1e-4))
    ops.clip_coef(small, st.tb, 1.0, coef)
    assert float(coef[0]) == 1.0 and 0 < float(coef[1]) < 1
    # all-zero gradients: coefficient 1, norm 0
    zero = torch.where(inactive, st.sumsq, torch.zeros_like(st.sumsq))
    ops.clip_coef(zero, st.tb, 1.0, coef)
    assert float(coef[0]) == 1.0 and float(coef[1]) == 0.0
    # 300 tensors: the stride loop past the 256 threads (a few of them inactive, with NaN slots)
    n = 300
    r = np.random.RandomState(5)
    ss = (r.random_sample(n) * 3).astype(np.float32)
    active = np.ones(n, dtype=bool)
    active[[3, 255, 256, 299]] = False
    tb = ops.adam_tables([(i, 1, 1e-3, 0.0, 1.0, int(active[i])) for i in range(n)], [(i, i, 1) for i in range(n)], DEV)
    ss_dev = torch.from_numpy(np.where(active, ss, np.float32("nan"))).to(DEV)
    ops.clip_coef(ss_dev, tb, 1.0, coef)
    gc, total = R.global_clip(ss[active].astype(np.float64), 1.0)
    c = coef.double().cpu().numpy()
    b300 = (2 + 8) * U + 2 * U                    # two strided adds per thread, the block tree; square root and the store
    assert abs(c[1] - total) <= b300 * total and abs(c[0] - gc) <= (b300 + 2 * U) * gc and gc < 0.1, (c, gc, total)
    assert bool((band[:4] == -5.0).all()) and bool((band[6:] == -5.0).all())
    st.assert_guards(also_unchanged=KEYS)


def test_scale_grads_is_one_multiply():
    st = State()
    g0 = st.g.clone()
    coef = torch.tensor([0.37, 9.0], device=DEV)
    ops.scale_grads(st.g, st.tb, coef)
    live = ~st.dead
    assert torch.equal(bits(st.g)[live], bits(g0 * coef[0])[live])
    st.assert_guards(also_unchanged=("p", "m", "v", "p16", "p16_lo"))
    st2 = State()
    ops.scale_grads(st2.g, st2.tb, torch.tensor([1.0, 9.0], device=DEV))
    st2.assert_guards(also_unchanged=KEYS)


# ---------------------------------------------------------------------------------------------------------------- per-tensor scalars
@pytest.mark.parametrize("with_coef", [True, False])
def test_prep_scalars_gradient_scale(with_coef):
    """seg_scalars[2s] after the scalar kernel alone (count = 0, do_prep = 1) vs fp64: 4u relative.  max_grad_norm 1 / 0 / -1 cycle over
    the tensors; with the global coefficient every scaled norm is below the limit, without it the tensors lie on both sides."""
    lay, st = layout(), State()
    ops.bert_adam_range(st.desc(coef=with_coef), 0, 0, do_prep=True)
    st.assert_guards(also_unchanged=KEYS)
    scal, ss = st.scal.double().cpu().numpy(), st.sumsq.double().cpu().numpy()
    gc = float(st.coef[0]) if with_coef else 1.0
    sides, worst = set(), 0.0
    for s, (off, n, lr, wd, mgn, active) in enumerate(lay.segs):
        if not active:
            assert scal[2 * s] == -77.0 and scal[2 * s + 1] == -77.0
            continue
        want = R.grad_scale(ss[s], gc, mgn)
        if mgn > 0:
            sides.add(want < gc)
        else:
            assert scal[2 * s] == gc
        worst = max(worst, abs(scal[2 * s] - want) / want / U)
        assert abs(scal[2 * s] - want) <= 4 * U * want, (s, scal[2 * s], want)
    print("[optim] gradient scale with_coef=%d: largest error %.2f u" % (with_coef, worst))
    assert sides == ({False} if with_coef else {False, True})


@pytest.mark.parametrize("schedule", [0, 1, 2])
def test_prep_scalars_scheduled_lr(schedule):
    """Every step 0 .. t_total + 2 in one launch (one 1-element tensor per step value) against the Python-double schedules: 8u lr
    absolute (cosf).  Step 0 gives 0, step 5 is the first past the ramp, from t_total on warmup_linear gives 0; t_total = -1: lr itself."""
    t_total, warmup, lr = 50, 0.1, R.f32(1e-3)
    n = t_total + 3
    tb = ops.adam_tables([(4 * i, 1, lr, 0.0, -1.0, 1) for i in range(n)], [(i, 4 * i, 1) for i in range(n)], DEV)
    buf = lambda: torch.full((4 * n,), R.SENTINEL, device=DEV)
    p, g, m, v = buf(), buf(), buf(), buf()
    step_band = torch.full((n + 8,), -9, dtype=torch.int32, device=DEV)          # step and the scalars inside guard bands
    step = step_band[4:4 + n]
    step.copy_(torch.arange(n, dtype=torch.int32, device=DEV))
    scal_band, ss = torch.full((2 * n + 8,), -77.0, device=DEV), torch.zeros(n, device=DEV)
    scal = scal_band[4:4 + 2 * n]
    d = ops.adam_desc(tb, p, g, m, v, sumsq=ss, step=step, seg_scalars=scal, warmup=warmup, t_total=t_total, schedule=schedule)
    ops.bert_adam_range(d, 0, 0, do_prep=True)
    got = scal.double().cpu().numpy()[1::2]
    want = np.array([R.scheduled_lr(lr, s, t_total, warmup, schedule) for s in range(n)])
    print("[optim] schedule %d: largest lr error %.2f u lr" % (schedule, np.abs(got - want).max() / (U * lr)))
    assert np.all(np.abs(got - want) <= 8 * U * lr), (schedule, np.abs(got - want).max() / (U * lr))
    assert got[0] == 0.0 and (schedule != 0 or np.all(got[t_total:] == 0.0))
    assert torch.equal(step, torch.arange(1, n + 1, dtype=torch.int32, device=DEV))
    d = ops.adam_desc(tb, p, g, m, v, sumsq=ss, step=step, seg_scalars=scal, warmup=warmup, t_total=-1, schedule=schedule)
    ops.bert_adam_range(d, 0, 0, do_prep=True)
    assert np.all(scal.double().cpu().numpy()[1::2] == lr)
    assert bool((step_band[:4] == -9).all()) and bool((step_band[4 + n:] == -9).all())
    assert bool((scal_band[:4] == -77.0).all()) and bool((scal_band[4 + 2 * n:] == -77.0).all())
    for t in (p, g, m, v):
        assert bool((t == R.SENTINEL).all())


def test_step_counters():
    lay, st = layout(), State()
    active = torch.tensor([sg[5] for sg in lay.segs], dtype=torch.int32, device=DEV)
    d = st.desc()
    ops.bert_adam(d)
    assert torch.equal(st.step, 7 + active)
    n = st.tb.nchunk
    ops.bert_adam_range(d, 0, 5, do_prep=True)          # a partitioned run: the scalar kernel with its first launch only
    ops.bert_adam_range(d, 5, 3)
    ops.bert_adam_range(d, 8, n - 8)
    assert torch.equal(st.step, 7 + 2 * active)
    st.assert_guards()


# ---------------------------------------------------------------------------------------------------------------- the update
def check_step(lay, before, st, shadows, tag, segs=None):
    """The stagewise bounds on one step's outputs, per tensor, with the kernel's own scalars; shadows exact; returns the largest errors."""
    scal = st.scal.double().cpu().numpy()
    after = {k: st.host(k) for k in "pmv"}
    worst = [0.0, 0.0, 0.0]
    for s, (off, n, lr0, wd, mgn, active) in enumerate(lay.segs):
        if not active or (segs is not None and s not in segs):
            continue
        sl = slice(off, off + n)
        gs, lr = scal[2 * s], scal[2 * s + 1]
        e = R.stage_errors(before["p"][sl], before["g"][sl], before["m"][sl], before["v"][sl], after["p"][sl], after["m"][sl],
                           after["v"][sl], gs, lr, wd)
        assert max(e) <= R.STAGE_BOUND, (tag, s, e)
        worst = [max(a, b) for a, b in zip(worst, e)]
        # g = m = v = 0: exactly p - lr * (wd * p) as the kernels state it, fma(-lr, wd * p, p) -- one rounding of the multiply-subtract
        # (the double product lr * upd is exact, 48 bits)
        z = (before["g"][sl] == 0) & (before["m"][sl] == 0) & (before["v"][sl] == 0)
        p0, pz = before["p"][sl][z], after["p"][sl][z]
        upd = np.float32(wd) * p0
        fused = (p0.astype(np.float64) - float(np.float32(lr)) * upd.astype(np.float64)).astype(np.float32)
        assert np.array_equal(pz, fused), (tag, s)
        assert not np.any(after["m"][sl][z]) and not np.any(after["v"][sl][z]), (tag, s)
        if lr == 0.0:
            assert np.array_equal(after["p"][sl], before["p"][sl]), (tag, s)
    live = ~st.dead
    if shadows >= 1:
        hi = st.p.to(torch.bfloat16)
        assert torch.equal(bits(st.p16)[live], bits(hi)[live]), tag
        if shadows >= 2:
            assert torch.equal(bits(st.p16_lo)[live], bits((st.p - hi.float()).to(torch.bfloat16))[live]), tag
    return worst


@pytest.mark.parametrize("variant", ["pair", "p16", "none", "wd0", "lr0"])
def test_bert_adam_three_steps_stagewise(variant):
    """univl_bert_adam, 3 consecutive steps, each stage of each step from the kernel's previous state.  Variants: the shadow pair, the
    hi half only, no shadow, weight decay 0 everywhere, a first step whose scheduled lr is 0 (p bit-unchanged while m and v advance)."""
    lay = layout()
    if variant == "wd0":
        lay = R.Layout()
        lay.segs = [sg[:3] + (0.0,) + sg[4:] for sg in lay.segs]
    st = State(lay)
    shadows = {"pair": 2, "p16": 1}.get(variant, 0 if variant == "none" else 2)
    if variant == "lr0":
        st.step.zero_()
    d = st.desc(shadows=shadows)
    worst = [0.0, 0.0, 0.0]
    for it in range(3):
        before = {k: st.host(k) for k in "pgmv"}
        ops.bert_adam(d)
        torch.cuda.synchronize()
        if variant == "lr0" and it == 0:
            live = ~st.dead
            assert torch.equal(bits(st.p), bits(st.orig["p"]))
            assert not torch.equal(st.m[live], st.orig["m"][live]) and not torch.equal(st.v[live], st.orig["v"][live])
        worst = [max(a, b) for a, b in zip(worst, check_step(lay, before, st, shadows, (variant, it)))]
        st.assert_guards(also_unchanged=("g",) + (("p16_lo",) if shadows < 2 else ()) + (("p16",) if shadows < 1 else ()))
    print("[optim] bert_adam %s: largest stage errors in u*S: m %.2f  v %.2f  p %.2f" % (variant, *worst))


def row_flags(flagged=True):
    f = torch.zeros(R.SEGMENTS[R.ROW_SEG][0] // R.ROW_LEN, dtype=torch.uint8, device=DEV)
    if flagged:
        f[R.ROW_FLAGGED] = 1
    return f


def test_row_flags_shortcut():
    """UnivlAdam.row_flags: the chunk whose rows are all unflagged takes the 10-byte path -- p, p16, lo bit-identical to the full formula
    on the same inputs, m and v bit-unchanged at zero; the two chunks that share the flagged row (one ENDS in its middle, one STARTS
    there: the floor / ceil of the row range) take the full path, checked stagewise."""
    lay = layout()
    a, b = State(), State()
    flags = row_flags()
    before = {k: a.host(k) for k in "pgmv"}
    ops.bert_adam(a.desc(row_flags=flags, flag_seg=R.ROW_SEG, row_len=R.ROW_LEN))
    ops.bert_adam(b.desc())
    same_state(a, b)
    off, n = lay.segs[R.ROW_SEG][:2]
    first = slice(off, off + R.ROW_STEP)
    for k in "mv":
        assert not bool(getattr(a, k)[first].any()) and torch.equal(bits(getattr(a, k))[first], bits(a.orig[k])[first])
    assert not torch.equal(a.p[first], a.orig["p"][first])
    row = slice(off + R.ROW_FLAGGED * R.ROW_LEN, off + (R.ROW_FLAGGED + 1) * R.ROW_LEN)
    assert bool((a.m[row] != a.orig["m"][row]).all()) and bool((a.v[row] != a.orig["v"][row]).all())
    check_step(lay, before, a, 2, "row_flags", segs=(R.ROW_SEG,))
    a.assert_guards(also_unchanged=("g",))


# ---------------------------------------------------------------------------------------------------------------- partitions
def test_bert_adam_range_partitions_and_grids():
    ref = State()
    ops.bert_adam(ref.desc())
    n = ref.tb.nchunk
    parts = [[(0, n)], [(0, 2), (2, 9), (11, n - 11)], [(c, 1) for c in range(n)]]
    for pieces in parts:
        st = State()
        d = st.desc()
        for i, (b, cnt) in enumerate(pieces):
            ops.bert_adam_range(d, b, cnt, do_prep=(i == 0))
        same_state(st, ref)
    for mb in (1, 3, n + 5):
        st = State()
        ops.bert_adam_range(st.desc(), 0, n, do_prep=True, max_blocks=mb)
        same_state(st, ref)
    ref.assert_guards(also_unchanged=("g",))


def test_refusals_leave_everything_unchanged():
    """UNIVL_EINVAL with its message and no launch: a negative begin, a range past the table, a NULL mandatory field, and flat buffers
    that are not on the 16-byte (fp32) / 8-byte (bf16) boundaries the vector path assumes -- a one-element-offset view."""
    st = State()
    L, n = _lib.lib(), st.tb.nchunk
    d = st.desc()
    rc, msg = rc_of(L.univl_bert_adam_range, C.byref(d), -1, 2, 1, 0, stream())
    assert rc == EINVAL and "univl_bert_adam_range: chunks [-1, +2)" in msg
    rc, msg = rc_of(L.univl_bert_adam_range, C.byref(d), n - 1, 2, 1, 0, stream())
    assert rc == EINVAL and "univl_bert_adam_range: chunks [%d, +2) of %d" % (n - 1, n) in msg
    bad = st.desc()
    bad.g = None
    for fn, args in ((L.univl_bert_adam_range, (C.byref(bad), 0, n, 1, 0, stream())), (L.univl_bert_adam, (C.byref(bad), stream()))):
        rc, msg = rc_of(fn, *args)
        assert rc == EINVAL and "bad argument" in msg
    # misaligned bases (refused BEFORE any launch; nothing misaligned ever runs)
    a = torch.randn(192, 64, device=DEV).to(torch.bfloat16)
    w = torch.randn(64, 64, device=DEV).to(torch.bfloat16)
    out = torch.zeros(192, 64, device=DEV, dtype=torch.bfloat16)
    gd = ops.gemm_desc(a, w, 192, 64, 64, out16=out)
    ln = ops.layernorm_desc(ops.dtype_code(torch.bfloat16), 192, 64)
    ctr = torch.zeros(6, dtype=torch.int32, device=DEV)
    at = _lib.Attention()
    for field in ("p", "g", "m", "v", "p16", "p16_lo"):
        mis = st.desc()
        t = getattr(st, field)
        setattr(mis, field, C.c_void_p(t.data_ptr() + t.element_size()))
        for name, fn, args in (("univl_bert_adam", L.univl_bert_adam, (C.byref(mis), stream())),
                               ("univl_bert_adam_range", L.univl_bert_adam_range, (C.byref(mis), 0, n, 1, 0, stream())),
                               ("univl_gemm_rider", L.univl_gemm_rider, (C.byref(gd), C.byref(mis), 0, n, 0, stream())),
                               ("univl_gemm_ln", L.univl_gemm_ln, (C.byref(gd), C.byref(ln), C.c_void_p(ctr.data_ptr()), C.byref(mis), 0, n, 0,
                                                                   0, stream())),
                               ("univl_attention_fwd_fused", L.univl_attention_fwd_fused, (C.byref(at), C.byref(gd), C.byref(mis), 0, n, 0, 0,
                                                                                           stream()))):
            rc, msg = rc_of(fn, *args)
            assert rc == EINVAL and name in msg and "aligned" in msg, (field, name, rc, msg)
    with pytest.raises(RuntimeError, match="aligned"):
        ops.bert_adam(mis)
    torch.cuda.synchronize()
    st.assert_guards(also_unchanged=KEYS)
    assert not bool(out.any()) and not bool(ctr.any()) and bool((st.step == 7).all()) and bool((st.scal == -77.0).all())


# ---------------------------------------------------------------------------------------------------------------- rider forms
def prepared(shadows=2):
    """Two states after the scalar kernel: one for the launch form under test, one for univl_bert_adam_range on a copy."""
    a = State()
    da = a.desc(shadows=shadows)
    ops.bert_adam_range(da, 0, 0, do_prep=True)
    b = a.clone()
    return a, da, b, b.desc(shadows=shadows)


def gen(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


@pytest.mark.parametrize("begin,count,mb", [(2, None, 0), (0, None, 3), (0, None, 1000), (3, 0, 0)])
def test_gemm_rider_64_tile(begin, count, mb):
    """univl_gemm_rider on a 192 x 768 x 768 bf16 product (gemm_adam_kernel): a sub-range that starts after chunk 0, max_blocks below
    and above the count, no chunks at all.  Optimizer state bit-identical to univl_bert_adam_range on a copy, the product to univl_gemm."""
    M, N, K = 192, 768, 768
    x = gen(M, K, seed=1).to(DEV, torch.bfloat16)
    w = gen(N, K, seed=2, scale=K ** -0.5).to(DEV, torch.bfloat16)
    bias = gen(N, seed=3).to(DEV)
    a, da, b, db = prepared()
    n = a.tb.nchunk
    count = n - begin if count is None else count           # None: up to the table's end
    assert mb == 0 or (mb < count) == (mb == 3)
    out, ref = torch.zeros(M, N, device=DEV, dtype=torch.bfloat16), torch.zeros(M, N, device=DEV, dtype=torch.bfloat16)
    gd = ops.gemm_desc(x, w, M, N, K, out16=out, bias=bias)
    assert _lib.lib().univl_gemm_rider_fits(C.byref(gd)) == 1
    ops.gemm_rider(gd, da, begin, count, mb)
    ops.gemm(x, w, M, N, K, out16=ref, bias=bias)
    if count:
        ops.bert_adam_range(db, begin, count)
    same_state(a, b)
    assert torch.equal(bits(out), bits(ref)) and bool(out.any())
    a.assert_guards(also_unchanged=("g",) + (KEYS if count == 0 else ()))
    if begin == 2:                       # the chunks before the sub-range did not move
        off = a.lay.chunks[0][1]
        assert torch.equal(bits(a.p)[off:off + 1], bits(a.orig["p"])[off:off + 1])


@pytest.mark.parametrize("with_lo", [False, True])
def test_gemm_rider_64x128_tile(with_lo):
    """The 64 x 128 rider kernel (gemm_adam_rect_kernel) on the smallest product the library puts there by itself: the square choice
    must be the 128 tile (256 of them: 4096 x 1024; below that every product is a 64 x 64 one), which does not carry chunks, and the slot
    fill must favour the half tile.  Asked on the host: univl_gemm_rider_fits says 1 for the product as it is and 0 when it is pinned to
    the 128 tile.  That is INDIRECT: the library has no host-side answer that names the chosen form, and if GEMM_BIG_MIN or the fill rule
    of choose() (gemm.hip) moved, this product could fall to the 64 x 64 form with every assertion here still passing -- whoever changes
    either has to move this shape along.
    p16_lo = NULL: carried in the launch; p16_lo set: the kernel does not keep the lo half, the update follows the product -- lo exact."""
    M, N, K = 4096, 1024, 64
    x = gen(M, K, seed=1).to(DEV, torch.bfloat16)
    w = gen(N, K, seed=2, scale=K ** -0.5).to(DEV, torch.bfloat16)
    out, ref = torch.zeros(M, N, device=DEV, dtype=torch.bfloat16), torch.zeros(M, N, device=DEV, dtype=torch.bfloat16)
    gd = ops.gemm_desc(x, w, M, N, K, out16=out)
    L = _lib.lib()
    assert L.univl_gemm_rider_fits(C.byref(gd)) == 1
    assert L.univl_gemm_rider_fits(C.byref(ops.gemm_desc(x, w, M, N, K, out16=out, tile=128))) == 0
    assert L.univl_gemm_rider_fits(C.byref(ops.gemm_desc(x, w, M, N, K, out16=out, tile=64))) == 1            # (the 64 x 64 form)
    assert (M // 128) * (N // 128) == 256          # GEMM_BIG_MIN: one tile fewer and the product is a 64 x 64 one
    roles = []                                     # the launch below: 512 tile slots + 16 update workgroups (16 chunks, in groups of 8)
    for w0 in range(512 + 16):
        o3 = (C.c_int32 * 3)(w0, 0, 0)
        assert L.univl_gemm_tile_map(4, 512, 16, 1, 0, o3) == 0
        roles.append((o3[1], o3[0]))
    assert sorted(i for r, i in roles if r == 1) == list(range(16)) and sorted(i for r, i in roles if r == 0) == list(range(512))
    shadows = 2 if with_lo else 1
    a, da, b, db = prepared(shadows)
    n = a.tb.nchunk
    assert n - 1 == 16
    ops.gemm_rider(gd, da, 1, n - 1, 0)
    ops.gemm(x, w, M, N, K, out16=ref)
    ops.bert_adam_range(db, 1, n - 1)
    same_state(a, b)
    assert torch.equal(bits(out), bits(ref)) and bool(out.any())
    live = ~a.dead
    hi = a.p.to(torch.bfloat16)
    assert torch.equal(bits(a.p16)[live], bits(hi)[live])
    if with_lo:
        assert torch.equal(bits(a.p16_lo)[live], bits((a.p - hi.float()).to(torch.bfloat16))[live])
    a.assert_guards(also_unchanged=("g",) + (() if with_lo else ("p16_lo",)))


def test_gemm_ln_carrying_chunks():
    """univl_gemm_ln with riding chunks, the descriptors of test_gemm_ln_fold_matches_the_two_launches at (192, 768, 2).  Not available
    in deterministic mode."""
    was = univl_amd.deterministic()
    univl_amd.set_deterministic(False)
    try:
        M, K, N, ksplit, bf = 192, 768, 768, 2, torch.bfloat16
        x = gen(M, K, seed=1).to(DEV, bf)
        w = gen(N, K, seed=2, scale=K ** -0.5).to(DEV, bf)
        bias, res = gen(N, seed=3).to(DEV), gen(M, N, seed=4).to(DEV)
        gm, bt = (1.0 + 0.1 * gen(N, seed=5)).to(DEV), gen(N, seed=6).to(DEV)

        def bufs():
            return dict(x=torch.zeros(M, N, device=DEV), stats=torch.zeros(M, 2, device=DEV), out32=torch.zeros(M, N, device=DEV),
                        out16=torch.zeros(M, N, device=DEV, dtype=bf))

        def descs(bb):
            g = ops.gemm_desc(x, w, M, N, K, out32=bb["x"], bias=bias, ksplit=ksplit)
            ln = ops.layernorm_desc(ops.dtype_code(bf), M, N, x=bb["x"], residual=res, gamma=gm, beta=bt, y=bb["x"], stats=bb["stats"],
                                    out32=bb["out32"], out16=bb["out16"], p_pre=0.0, seed=7, off_pre=3 << 40)
            return g, ln

        ref, got = bufs(), bufs()
        g, ln = descs(ref)
        _lib.check(_lib.lib().univl_gemm(C.byref(g), None), "gemm")
        _lib.check(_lib.lib().univl_layernorm_fwd(C.byref(ln), None), "layernorm_fwd")
        a, da, b, db = prepared()
        n = a.tb.nchunk
        ctr = torch.zeros(2 * ((M + 63) // 64), dtype=torch.int32, device=DEV)
        g2, ln2 = descs(got)
        assert ops.gemm_ln(g2, ln2, ctr, adam=da, chunk_begin=1, chunk_count=n - 1, max_blocks=4)
        ops.bert_adam_range(db, 1, n - 1)
        same_state(a, b)
        assert int(ctr.abs().sum()) == 0
        for k in ("x", "stats", "out32", "out16"):           # (split product: its slices meet in atomics -- the existing test's bounds)
            err = float((got[k].double() - ref[k].double()).abs().max() / ref[k].double().abs().max())
            assert err < (1e-2 if k == "out16" else 2e-5), (k, err)
        a.assert_guards(also_unchanged=("g",))
        univl_amd.set_deterministic(True)
        assert not ops.gemm_ln(g2, ln2, ctr, dry_run=True, adam=da, chunk_begin=1, chunk_count=n - 1)
    finally:
        univl_amd.set_deterministic(was)


def test_attention_fwd_fused_carrying_chunks():
    """univl_attention_fwd_fused with riding chunks, the descriptors of
    test_attention_fwd_with_the_qkv_projection_inside_equals_the_two_launches at (4, 48)."""
    B, S, H, D, dtype = 4, 48, 12, 64, torch.bfloat16
    dt = ops.dtype_code(dtype)
    T, HD = B * S, H * D
    x = gen(T, HD, seed=1).to(DEV, dtype)
    W = gen(3 * HD, HD, seed=2, scale=0.05).to(DEV, dtype)
    bias = gen(3 * HD, seed=3).to(DEV)
    seed = torch.full((1,), 4321, dtype=torch.int64, device=DEV)
    kw = dict(key_mask=None, p_drop=0.1, offset=3 << 40, seed_dev=seed)
    a, da, b, db = prepared()
    n = a.tb.nchunk

    def run(fused):
        qkv = torch.full((T + 2, 3 * HD), 5.0, device=DEV, dtype=dtype)[:T]
        ctx = torch.zeros(T, HD, device=DEV, dtype=dtype)
        lse = torch.zeros(B, H, S, device=DEV)
        args = (dt, B, H, S, S, (qkv, 0), 3 * HD, (qkv, HD), 3 * HD, (qkv, 2 * HD), 3 * HD, ctx, HD, lse)
        if fused:
            assert ops.attention_fwd_fused(ops.attention_desc(*args, **kw), ops.gemm_desc(x, W, T, 3 * HD, HD, out16=qkv, bias=bias),
                                           adam=da, chunk_begin=0, chunk_count=n, max_blocks=5)
        else:
            ops.gemm(x, W, T, 3 * HD, HD, out16=qkv, bias=bias)
            ops.attention_fwd(*args, **kw)
            ops.bert_adam_range(db, 0, n)
        torch.cuda.synchronize()
        return qkv.clone(), ctx, lse

    q0, c0, l0 = run(False)
    q1, c1, l1 = run(True)
    assert torch.equal(bits(q1), bits(q0)) and torch.equal(bits(c1), bits(c0)) and torch.equal(l1, l0) and bool(c1.any())
    same_state(a, b)
    a.assert_guards(also_unchanged=("g",))


# ---------------------------------------------------------------------------------------------------------------- a plan that carries
def test_plan_deals_a_range_to_its_three_carrying_forms_once():
    """engine.Plan with engine.Riders set, on a hand-built plan at the smallest shapes the three carrying kernels accept (192 tokens,
    hidden 768, 12 heads): a fused attention forward, a (product, LayerNorm) launch (K = 3072 in 8 slices) and a rider product (768 ->
    3072, GELU) are slots 0 / 1 / 2 of 3 of ONE key; a second rider launch repeats slot 2 and must carry nothing.  The table has 7 chunks
    (2 / 2 / 3 over the slots), the last tensor's length is no multiple of 4.  After one eager run: p / m / v and both shadows
    bit-identical to one univl_bert_adam_range over the 7 chunks on a copy, exactly the three slots used, and the products equal to the
    same plan run with nothing riding -- bit for bit for the attention launch and the rider (the bounds of test_gemm_rider_64_tile and
    test_attention_fwd_fused_carrying_chunks), within test_gemm_ln_fold_matches_the_two_launches' bounds for the split product that
    meets in atomics (2e-5 relative to the largest value in fp32, 1e-2 in bf16)."""
    from univl_amd.engine import Plan, Riders
    B, S, NH, H, I, bf = 4, 48, 12, 768, 3072, torch.bfloat16
    T, dt = B * S, ops.dtype_code(torch.bfloat16)
    # update: three tensors in 2 + 3 + 2 chunks of at most 8192 elements, the last one 8192 + 1027 long
    CH = 8192
    segs = [(0, 2 * CH, 1e-3, 0.01, 1.0, 1), (2 * CH, 3 * CH, 2e-3, 0.0, 1.0, 1), (5 * CH, CH + 1027, 1e-3, 0.01, 1.0, 1)]
    chunks = [(0, 0, CH), (0, CH, CH), (1, 2 * CH, CH), (1, 3 * CH, CH), (1, 4 * CH, CH), (2, 5 * CH, CH), (2, 6 * CH, 1027)]
    total = 6 * CH + 1027
    tb = ops.adam_tables(segs, chunks, DEV)

    def state():
        s = {k: gen(total + 64, seed=i, scale=sc).to(DEV) for i, (k, sc) in enumerate((("p", 0.05), ("g", 0.01), ("m", 0.01), ("v", 0.01)))}
        s["v"] = s["v"].abs()
        s["p16"] = s["p"].to(bf)
        s["p16_lo"] = (s["p"] - s["p16"].float()).to(bf)
        s["sumsq"] = torch.stack([(s["g"][o:o + k].double() ** 2).sum() for o, k, *_ in segs]).float()
        s["step"] = torch.full((len(segs),), 7, dtype=torch.int32, device=DEV)
        s["scal"] = torch.zeros(2 * len(segs), device=DEV)
        s["coef"] = torch.tensor([1.0, 0.0], device=DEV)
        d = ops.adam_desc(tb, s["p"], s["g"], s["m"], s["v"], sumsq=s["sumsq"], step=s["step"], seg_scalars=s["scal"], p16=s["p16"],
                          p16_lo=s["p16_lo"], coef=s["coef"], b1=R.B1, b2=R.B2, eps=R.EPS, warmup=0.1, t_total=50)
        ops.bert_adam_range(d, 0, 0, do_prep=True)
        return s, d

    a, da = state()
    b, db = state()
    # products
    x = gen(T, H, seed=11).to(DEV, bf)
    wqkv, bqkv = gen(3 * H, H, seed=12, scale=0.05).to(DEV, bf), gen(3 * H, seed=13).to(DEV)
    qkv, ctx, lse = torch.zeros(T, 3 * H, device=DEV, dtype=bf), torch.zeros(T, H, device=DEV, dtype=bf), torch.zeros(B, NH, S, device=DEV)
    at = ops.attention_desc(dt, B, NH, S, S, (qkv, 0), 3 * H, (qkv, H), 3 * H, (qkv, 2 * H), 3 * H, ctx, H, lse)
    gq = ops.gemm_desc(x, wqkv, T, 3 * H, H, out16=qkv, bias=bqkv)
    f, w2, b2 = gen(T, I, seed=14).to(DEV, bf), gen(H, I, seed=15, scale=I ** -0.5).to(DEV, bf), gen(H, seed=16).to(DEV)
    res, gm, bt = gen(T, H, seed=17).to(DEV), (1.0 + 0.1 * gen(H, seed=18)).to(DEV), gen(H, seed=19).to(DEV)
    y, stats, o32, o16 = torch.zeros(T, H, device=DEV), torch.zeros(T, 2, device=DEV), torch.zeros(T, H, device=DEV), torch.zeros(T, H, device=DEV, dtype=bf)
    g2 = ops.gemm_desc(f, w2, T, H, I, out32=y, bias=b2, ksplit=8)
    ln = ops.layernorm_desc(dt, T, H, x=y, residual=res, gamma=gm, beta=bt, y=y, stats=stats, out32=o32, out16=o16)
    ctr = torch.zeros(2 * ((T + 63) // 64), dtype=torch.int32, device=DEV)
    w1, b1 = gen(I, H, seed=20, scale=H ** -0.5).to(DEV, bf), gen(I, seed=21).to(DEV)
    u, f1 = torch.zeros(T, I, device=DEV, dtype=bf), torch.zeros(T, I, device=DEV, dtype=bf)
    g1 = ops.gemm_desc(x, w1, T, I, H, out16=f1, bias=b1, aux=u, gelu="fwd")
    assert ops.attention_fwd_fused(at, gq, dry_run=True) and _lib.lib().univl_gemm_rider_fits(C.byref(g1)) == 1
    if not univl_amd.deterministic():
        assert ops.gemm_ln(g2, ln, ctr, dry_run=True)
    key = ("layer", "test", 1)
    plan = Plan()
    plan.add_attn_fwd_fused(at, gq, key, 0, 3)
    plan.add_gemm_ln(g2, ln, ctr, key, 1, 3)
    plan.add_gemm_rider(g1, key, 2, 3)
    plan.add_gemm_rider(g1, key, 2, 3)
    assert plan.rider_keys == {key} and len(plan) == 4
    outs = dict(qkv=qkv, ctx=ctx, lse=lse, y=y, stats=stats, o32=o32, o16=o16, u=u, f1=f1)
    plan.run()
    torch.cuda.synchronize()
    plain = {k: t.clone() for k, t in outs.items()}
    for k in "pmv":
        assert torch.equal(a[k], b[k])               # nothing rode
    for t in outs.values():
        t.zero_()
    plan.riders = Riders(da, {key: (0, len(chunks))})
    try:
        plan.run()
    finally:
        rd, plan.riders = plan.riders, None
    ops.bert_adam_range(db, 0, len(chunks))
    torch.cuda.synchronize()
    assert rd.used == {(key, 0), (key, 1), (key, 2)}
    for k in ("p", "m", "v", "p16", "p16_lo"):
        assert torch.equal(bits(a[k]), bits(b[k])), k
    assert torch.equal(a["g"], b["g"]) and torch.equal(a["step"], b["step"]) and not torch.equal(a["p"][:total], gen(total + 64, seed=0, scale=0.05).to(DEV)[:total])
    assert int(ctr.abs().sum()) == 0
    for k in ("qkv", "ctx", "lse", "u", "f1"):
        assert torch.equal(bits(outs[k]), bits(plain[k])) and bool(outs[k].any()), k
    for k in ("y", "stats", "o32", "o16"):
        err = float((outs[k].double() - plain[k].double()).abs().max() / plain[k].double().abs().max())
        print("plan carry: %s relative error %.3g" % (k, err))
        assert err < (1e-2 if k == "o16" else 2e-5), (k, err)
