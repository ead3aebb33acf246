"""fp64 parity of univl_attention_fwd / univl_attention_bwd at their sequence-length and mask edges: the shape table of
tests/attention_ref.py (pad boundaries, every MAXKT tier from both sides, one | two blocks of queries and of keys, the backward's small
and large paths, Sq > Sk, the LDS limits), without and with `causal`, packed / split / wide layouts, the key / value cache form, and
dropout at four odd shapes.  Needs a real MI355X (`-m gpu`).

Every table case asserts
  * out, dq, dk, dv under the per-row metric (attention_ref.row_err) and under the suite's whole-tensor rel_err with tol(dtype);
  * lse against the reference for every row;
  * dk and dv EXACTLY zero at keys that every query of the batch row blocks;
  * every output buffer's guard rows and guard columns bit-identical to their fill pattern, after the forward and after the backward;
  * a B = 1 launch on the ragged batch row alone, into pattern-filled buffers: the neighbouring batch rows stay untouched and the
    owned rows carry the bits of the B = 3 launch.

Gates: whole tensor -- the suite's numbers (fp32 1e-3; bf16 1e-2 for out, 2e-2 for gradients).  Per row and lse -- MARGIN (4) times the
worst error over the table of the reference evaluated at the kernel's precision (attention_ref.model_floors), computed on the CPU; never
taken from the kernels' output.  The whole-tensor metric is not applied to a reference tensor that is zero to rounding (dq, dk at
Sk = 1): there the per-row metric is the absolute error.  Model floors, gates and the measured worst values: profiles/attention_edges.txt."""
import pytest
import torch

import attention_ref as A
import dropout_ref as R

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from univl_amd import ops

DEV = "cuda"
D = A.D
B = A.B
DTYPES = [torch.float32, torch.bfloat16]
GUARD = 3                                                   # guard rows before and after every output buffer
PATTERN = {torch.float32: 0x7FC5A5A5, torch.bfloat16: 0x7FC5}      # a quiet NaN in both types: an unwritten element poisons its error


def rel_err(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def tol(dtype):
    return 1e-3 if dtype == torch.float32 else 1e-2


def _name(dtype):
    return str(dtype).replace("torch.", "")


def _report(what, dtype, errs, gates=None, label="gates"):
    print("[attention edges] %s %s  " % (what, _name(dtype)) + "  ".join("%s=%.3e" % kv for kv in errs.items())
          + ("" if gates is None else "  | " + label + " " + "  ".join("%s=%.3e" % kv for kv in gates.items())))


class Guarded:
    """A [rows, width] matrix of `dtype` with leading dimension ld inside a buffer that has GUARD rows before and after it (and
    ld - width guard columns), every element filled with PATTERN."""

    def __init__(self, rows, width, ld, dtype):
        self.rows, self.width, self.ld, self.dtype = rows, width, ld, dtype
        self.pat = PATTERN[dtype]
        self.raw = torch.full((rows + 2 * GUARD, ld), self.pat, dtype=torch.int32 if dtype == torch.float32 else torch.int16, device=DEV)
        self.t = self.raw.view(dtype)

    def at(self, row=0, col=0):
        """(tensor, element offset) of element [row, col] of the matrix, as ops.attention_desc takes pointers."""
        return (self.t, (GUARD + row) * self.ld + col)

    def body(self, col=0, width=None):
        return self.t[GUARD:GUARD + self.rows, col:col + (self.width if width is None else width)].float().cpu()

    def bits(self, r0, r1):
        return self.raw[GUARD + r0:GUARD + r1, :self.width].cpu()

    def untouched_outside(self, r0=0, r1=None):
        """Everything but rows [r0, r1) x the first `width` columns still holds the pattern."""
        raw = self.raw.cpu()
        free = torch.ones_like(raw, dtype=torch.bool)
        free[GUARD + r0:GUARD + (self.rows if r1 is None else r1), :self.width] = False
        return bool((raw[free] == self.pat).all())


class GuardedLse:
    def __init__(self, n):
        self.n = n
        self.raw = torch.full((n + 8,), PATTERN[torch.float32], dtype=torch.int32, device=DEV)
        self.t = self.raw.view(torch.float32)[4:4 + n]

    def untouched_outside(self):
        raw = self.raw.cpu()
        return bool((raw[:4] == PATTERN[torch.float32]).all() and (raw[4 + self.n:] == PATTERN[torch.float32]).all())


class Launch:
    """Device buffers of one problem in a layout, and the two launches.  b0 / nb: the batch rows the launch covers (pointers advanced to
    batch row b0, B = nb) -- the buffers always hold all B batch rows."""

    def __init__(self, dtype, Sq, Sk, H, layout, wide, q, k, v, dout, mask):
        self.dtype, self.Sq, self.Sk, self.H, self.layout = dtype, Sq, Sk, H, layout
        HD = H * D
        self.HD = HD
        pad = (8 if dtype == torch.bfloat16 else 4) if wide else 0           # one 16-byte piece
        f = lambda t, S: t.reshape(B * S, HD)
        if layout == "packed":
            assert Sq == Sk
            self.inp = torch.cat([f(q, Sq), f(k, Sk), f(v, Sk)], dim=1).to(DEV, dtype).contiguous()
            self.q, self.k, self.v, self.ldq, self.ldk = (self.inp, 0), (self.inp, HD), (self.inp, 2 * HD), 3 * HD, 3 * HD
        else:
            self.qb = f(q, Sq).to(DEV, dtype).contiguous()
            self.kvb = torch.cat([f(k, Sk), f(v, Sk)], dim=1).to(DEV, dtype).contiguous()
            self.q, self.k, self.v, self.ldq, self.ldk = (self.qb, 0), (self.kvb, 0), (self.kvb, HD), HD, 2 * HD
        self.dout = f(dout, Sq).to(DEV, dtype).contiguous()
        self.mask = None if mask is None else mask.to(DEV)
        self.ldo = HD + pad
        self.pad = pad

    def outputs(self):
        HD, pad, dt = self.HD, self.pad, self.dtype
        o = dict(out=Guarded(B * self.Sq, HD, self.ldo, dt), lse=GuardedLse(B * self.H * self.Sq))
        if self.layout == "packed":
            g = Guarded(B * self.Sq, 3 * HD, 3 * HD + pad, dt)
            o.update(bufs=[g], dq=(g, 0), dk=(g, HD), dv=(g, 2 * HD))
        elif pad:                                                                # ld = H * 64 + one piece for each of dq, dk, dv
            gq, gk, gv = (Guarded(B * s_, HD, HD + pad, dt) for s_ in (self.Sq, self.Sk, self.Sk))
            o.update(bufs=[gq, gk, gv], dq=(gq, 0), dk=(gk, 0), dv=(gv, 0))
        else:
            gq, gkv = Guarded(B * self.Sq, HD, HD, dt), Guarded(B * self.Sk, 2 * HD, 2 * HD, dt)
            o.update(bufs=[gq, gkv], dq=(gq, 0), dk=(gkv, 0), dv=(gkv, HD))
        return o

    def _args(self, o, b0, nb, out_src=None, lse=None):
        off = lambda p, S, ld: (p[0], p[1] + b0 * S * ld)
        out = (o["out"] if out_src is None else out_src).at(b0 * self.Sq)
        return (ops.dtype_code(self.dtype), nb, self.H, self.Sq, self.Sk, off(self.q, self.Sq, self.ldq), self.ldq,
                off(self.k, self.Sk, self.ldk), self.ldk, off(self.v, self.Sk, self.ldk), self.ldk, out, self.ldo,
                o["lse"].t if lse is None else lse)

    def _kw(self, b0, nb, causal, drop):
        return dict(key_mask=None if self.mask is None else self.mask[b0:b0 + nb].contiguous(), causal=causal, **drop)

    def fwd(self, o, causal, b0=0, nb=B, **drop):
        ops.attention_fwd(*self._args(o, b0, nb), **self._kw(b0, nb, causal, drop))

    def bwd(self, o, causal, b0=0, nb=B, out_src=None, lse=None, **drop):
        gq, cq = o["dq"]
        gk, ck = o["dk"]
        gv, cv = o["dv"]
        ops.attention_bwd(*self._args(o, b0, nb, out_src, lse), **self._kw(b0, nb, causal, drop),
                          dout=(self.dout, b0 * self.Sq * self.HD), lddo=self.HD, dq=gq.at(b0 * self.Sq, cq), lddq=gq.ld,
                          dk=gk.at(b0 * self.Sk, ck), lddk=gk.ld, dv=gv.at(b0 * self.Sk, cv), lddv=gv.ld)

    def read(self, o, back=True):
        HD = self.HD
        got = dict(out=o["out"].body().view(B, self.Sq, HD), lse=o["lse"].t.cpu().view(B, self.H, self.Sq))
        if back:
            for name, S in (("dq", self.Sq), ("dk", self.Sk), ("dv", self.Sk)):
                g, c = o[name]
                got[name] = g.body(c, HD).reshape(B, S, HD)
        return got


def _check(case_name, dtype, got, ref, H, gates):
    """Prints every figure, then asserts the per-row gates, the lse gate and the whole-tensor gates."""
    errs = A.errors(got, ref, H)
    whole = {}
    for name in A.QUANTITIES:
        if name in got and float(ref[name].abs().max()) > A.NULL_TENSOR:
            whole[name + "_whole"] = rel_err(got[name], ref[name])
    _report(case_name, dtype, dict(errs, **whole), {k_: gates[k_] for k_ in errs})
    for name, e in errs.items():
        assert e <= gates[name], (case_name, name, e, gates[name])
    for name, e in whole.items():
        t = tol(dtype) * (2 if dtype == torch.bfloat16 and name != "out_whole" else 1)
        assert e < t, (case_name, name, e, t)


@pytest.mark.parametrize("case", A.CASES, ids=A.case_id)
def test_attention_edges(case):
    i, causal, dtype = case
    Sq, Sk, H, layout, wide, _, masked = A.TABLE[i]
    d = A.case_data(case)
    gates = A.gates(dtype)
    L = Launch(dtype, Sq, Sk, H, layout, wide, d["q"], d["k"], d["v"], d["dout"], d["mask"])
    o = L.outputs()
    L.fwd(o, causal)
    torch.cuda.synchronize()
    assert o["out"].untouched_outside() and o["lse"].untouched_outside(), "the forward wrote outside out / lse"
    assert all(g.untouched_outside(0, 0) for g in o["bufs"])
    L.bwd(o, causal)
    torch.cuda.synchronize()
    assert o["out"].untouched_outside() and o["lse"].untouched_outside()
    assert all(g.untouched_outside() for g in o["bufs"]), "the backward wrote outside dq / dk / dv"
    got = L.read(o)
    _check(A.case_id(case), dtype, got, d["ref"], H, gates)

    # exact zeros: keys that every query of a (not fully masked) batch row blocks
    z = A.always_blocked(d["mask"], Sq, Sk, causal)
    if masked and Sk > 1:
        assert float(z[2].float().mean()) >= 0.1
    if bool(z.any()):
        for name in ("dk", "dv"):
            assert bool((got[name][z] == 0).all()), (name, int((got[name][z] != 0).sum()))
            assert bool((d["ref"][name][z] == 0).all())

    # the ragged batch row alone (B = 1) into fresh pattern-filled buffers: batch rows 0 and 1 are never touched, the bits are the same
    o1 = L.outputs()
    o1["lse"] = GuardedLse(H * Sq)
    L.fwd(o1, causal, b0=2, nb=1)
    L.bwd(o1, causal, b0=2, nb=1)
    torch.cuda.synchronize()
    assert o1["out"].untouched_outside(2 * Sq, 3 * Sq) and o1["lse"].untouched_outside()
    assert torch.equal(o1["out"].bits(2 * Sq, 3 * Sq), o["out"].bits(2 * Sq, 3 * Sq))
    assert torch.equal(o1["lse"].t.cpu(), o["lse"].t.cpu().view(B, -1)[2])
    for name, S in (("dq", Sq), ("dk", Sk), ("dv", Sk)):
        g1, g0 = o1[name][0], o[name][0]
        if layout == "packed":
            assert g1.untouched_outside(2 * Sq, 3 * Sq)
        else:
            assert g1.untouched_outside(2 * S, 3 * S), name
        assert torch.equal(g1.bits(2 * S, 3 * S), g0.bits(2 * S, 3 * S)), name


# ------------------------------------------------------------------------------------------------ key / value cache (bsk / bsv)
TMAX = 72


def _cache(dtype, H, Sk, k, v):
    """k, v [B,Sk,H*64] -> a [B, TMAX, 2*H*64] cache on the device whose slots >= Sk are NaN."""
    c = torch.full((B, TMAX, 2 * H * D), float("nan"))
    c[:, :Sk, :H * D] = k
    c[:, :Sk, H * D:] = v
    return c.to(DEV, dtype).contiguous()


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_kv_cache_sweep(dtype):
    """The form decode.py launches at every position: Sq = 1 over a cache of capacity TMAX, every prefix length 1 .. TMAX.  Slots >= t
    hold NaN: an output that read one is not finite."""
    H = 3
    HD = H * D
    q, k, v, _ = A.operands(1, TMAX, H, dtype, seed=77)
    qd = q.reshape(B, HD).to(DEV, dtype).contiguous()
    outs = torch.zeros(TMAX, B, HD, device=DEV, dtype=dtype)
    lses = torch.zeros(TMAX, B * H, device=DEV)
    ld = 2 * HD
    for t in range(1, TMAX + 1):
        c = _cache(dtype, H, t, k[:, :t], v[:, :t])
        ops.attention_fwd(ops.dtype_code(dtype), B, H, 1, t, qd, HD, (c, 0), ld, (c, HD), ld, (outs, (t - 1) * B * HD), HD, lses[t - 1],
                          bsk=TMAX * ld, bsv=TMAX * ld)
    torch.cuda.synchronize()
    outs, lses = outs.float().cpu(), lses.cpu()
    assert bool(torch.isfinite(outs).all()) and bool(torch.isfinite(lses).all()), "a cache slot beyond the prefix was read"
    gates = A.gates(dtype)
    worst = dict(out=0.0, lse=0.0, out_whole=0.0)
    zero = torch.zeros(B, 1, HD)
    for t in range(1, TMAX + 1):
        ref = A.reference(q, k[:, :t], v[:, :t], A.attn_bias(None, 1, t, False), H, zero)
        e = A.errors(dict(out=outs[t - 1].view(B, 1, HD), lse=lses[t - 1].view(B, H, 1)), ref, H)
        w = rel_err(outs[t - 1].view(B, 1, HD), ref["out"])
        assert e["out"] <= gates["out"] and e["lse"] <= gates["lse"] and w < tol(dtype), (t, e, w)
        worst = dict(out=max(worst["out"], e["out"]), lse=max(worst["lse"], e["lse"]), out_whole=max(worst["out_whole"], w))
    _report("kv cache Sq=1 t=1..%d" % TMAX, dtype, worst, {k_: gates[k_] for k_ in ("out", "lse")})


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("t", [5, 33, 64, 65])
def test_kv_cache_with_a_key_mask_and_three_queries(dtype, t):
    H, Sq = 3, 3
    HD = H * D
    q, k, v, _ = A.operands(Sq, t, H, dtype, seed=78 + t)
    mask = A.key_mask(t)
    c = _cache(dtype, H, t, k, v)
    out = Guarded(B * Sq, HD, HD, dtype)
    lse = GuardedLse(B * H * Sq)
    ld = 2 * HD
    ops.attention_fwd(ops.dtype_code(dtype), B, H, Sq, t, q.reshape(B * Sq, HD).to(DEV, dtype).contiguous(), HD, (c, 0), ld, (c, HD), ld,
                      out.at(), HD, lse.t, key_mask=mask.to(DEV), bsk=TMAX * ld, bsv=TMAX * ld)
    torch.cuda.synchronize()
    assert out.untouched_outside() and lse.untouched_outside()
    got = dict(out=out.body().view(B, Sq, HD), lse=lse.t.cpu().view(B, H, Sq))
    assert bool(torch.isfinite(got["out"]).all())
    ref = A.reference(q, k, v, A.attn_bias(mask, Sq, t, False), H, torch.zeros(B, Sq, HD))
    _check("kv cache Sq=3 t=%d masked" % t, dtype, got, ref, H, A.gates(dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("Sq,Sk", [(5, 17), (33, 65)])
def test_kv_cache_backward_reads_at_the_batch_stride_and_writes_dense(dtype, Sq, Sk):
    """univl_attention_bwd with bsk / bsv (include/univl_hip.h, UnivlAttention): K and V are READ at the batch stride, dk and dv are
    WRITTEN densely as [B * Sk, ld] -- the gradient of a cache prefix, not a cache-shaped buffer.  No caller uses the form today."""
    H = 3
    HD = H * D
    q, k, v, do = A.operands(Sq, Sk, H, dtype, seed=90 + Sk)
    mask = A.key_mask(Sk)
    c = _cache(dtype, H, Sk, k, v)
    ld = 2 * HD
    out, lse = Guarded(B * Sq, HD, HD, dtype), GuardedLse(B * H * Sq)
    gq, gk, gv = Guarded(B * Sq, HD, HD, dtype), Guarded(B * Sk, HD, HD, dtype), Guarded(B * Sk, HD, HD, dtype)
    args = (ops.dtype_code(dtype), B, H, Sq, Sk, q.reshape(B * Sq, HD).to(DEV, dtype).contiguous(), HD, (c, 0), ld, (c, HD), ld,
            out.at(), HD, lse.t)
    kw = dict(key_mask=mask.to(DEV), bsk=TMAX * ld, bsv=TMAX * ld)
    ops.attention_fwd(*args, **kw)
    ops.attention_bwd(*args, **kw, dout=do.reshape(B * Sq, HD).to(DEV, dtype).contiguous(), lddo=HD, dq=gq.at(), lddq=HD, dk=gk.at(), lddk=HD,
                      dv=gv.at(), lddv=HD)
    torch.cuda.synchronize()
    assert all(g.untouched_outside() for g in (out, gq, gk, gv)) and lse.untouched_outside()
    got = dict(out=out.body().view(B, Sq, HD), lse=lse.t.cpu().view(B, H, Sq), dq=gq.body().view(B, Sq, HD),
               dk=gk.body().view(B, Sk, HD), dv=gv.body().view(B, Sk, HD))
    assert all(bool(torch.isfinite(got[n]).all()) for n in got)
    ref = A.reference(q, k, v, A.attn_bias(mask, Sq, Sk, False), H, do)
    _check("kv cache backward %dx%d" % (Sq, Sk), dtype, got, ref, H, A.gates(dtype))
    z = A.always_blocked(mask, Sq, Sk, False)
    assert bool((got["dk"][z] == 0).all()) and bool((got["dv"][z] == 0).all())


# ------------------------------------------------------------------------------------------------ dropout at the edges
#               Sq   Sk  causal  dtypes                one per MAXKT tier (4 / 8 / 16 / 24; fp32 has no fourth tier: a second shape of the first)
DROP_CASES = [(17, 33, True, DTYPES), (129, 127, False, DTYPES), (5, 255, False, DTYPES), (193, 257, False, [torch.bfloat16]),
              (65, 63, False, [torch.float32])]


@pytest.mark.parametrize("case", [(c[:3], dt) for c in DROP_CASES for dt in c[3]], ids=lambda c: "%dx%d%s-%s" % (*c[0][:2], "-causal" if c[0][2] else "", _name(c[1])))
def test_attention_edges_with_dropout(case):
    """p_drop = 0.1 under the host-computed mask (dropout_ref.keep_mask), as test_attention_dropout_parity's step 2."""
    (Sq, Sk, causal), dtype = case
    H, p, seed, offset = 3, 0.1, 2 ** 63 + 11, 5 << 40
    q, k, v, do = A.operands(Sq, Sk, H, dtype, seed=300 + Sq)
    mask = A.key_mask(Sk)
    bias = A.attn_bias(mask, Sq, Sk, causal)
    scale = R.scale_of(R.keep_mask(R.effective_seed(seed), offset, R.attn_idx(B, H, Sq, Sk), p), p)
    L = Launch(dtype, Sq, Sk, H, "split", False, q, k, v, do, mask)
    o = L.outputs()
    drop = dict(p_drop=p, seed=seed, offset=offset)
    L.fwd(o, causal, **drop)
    L.bwd(o, causal, **drop)
    torch.cuda.synchronize()
    assert o["out"].untouched_outside() and o["lse"].untouched_outside() and all(g.untouched_outside() for g in o["bufs"])
    got = L.read(o)
    ref = A.reference(q, k, v, bias, H, do, scale=scale)
    errs = {n: rel_err(got[n], ref[n]) for n in A.QUANTITIES}
    rows = A.errors(got, ref, H)
    mdl = A.errors(A.model(q, k, v, bias, H, do, dtype, scale=scale), ref, H)
    _report("dropout p=%g %dx%d%s whole" % (p, Sq, Sk, " causal" if causal else ""), dtype, errs)
    _report("dropout p=%g %dx%d%s per row" % (p, Sq, Sk, " causal" if causal else ""), dtype, rows, mdl, label="model")
    t = tol(dtype) * (2 if dtype == torch.bfloat16 else 1)
    assert errs["out"] < tol(dtype), errs
    assert errs["dq"] < t and errs["dk"] < t and errs["dv"] < t, errs
    assert rows["lse"] <= A.gates(dtype)["lse"], rows
