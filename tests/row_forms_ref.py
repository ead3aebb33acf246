"""Cases, input builders, fp64 references and error measures for the row kernels in every launch form: LayerNorm forward / backward
(csrc/layernorm.hip, csrc/ln_body.h), the LayerNorm backward folded into a pair launch (csrc/gemm.hip: ln_fold_bwd), the text embedding
and the listed-rows bookkeeping of the word table (csrc/embed.hip).

tests/test_row_forms_gpu.py runs the kernels on the inputs built here; tests/test_row_forms_cpu.py evaluates the same formulas in
torch fp32 on the same inputs and requires that evaluation to sit within a quarter of every gate, so the gates are met with room
by reference-precision arithmetic alone and a kernel that misses one is wrong, not unlucky.

Every formula is stated once and works in the dtype of its operands: called on fp64 tensors it is the reference, on fp32 tensors the
margin evaluation.  The backward is the closed form of ln_body.h, computed from what the kernels read -- y, stats = (mean, rstd),
gamma, dout -- so a forward error can neither mask nor mimic a backward one:

    dy = dout * s_post        xh = (y - mean) * rstd        s1 = mean_c(dy g)        s2 = mean_c(dy g xh)
    dx = rstd * (dy g - s1 - xh s2)        dxd = dx * s_pre
    dgamma = sum_r dy xh      dbeta = sum_r dy      dbias = sum_r dxd      dpos[s] = sum over r % period == s of dx[r]

Inputs.  Row r of x and of dout carries the factor f(r), 10 ** u with u spread evenly over [-2, 2] in a seeded order (the last row
takes the largest, so that a lost tail row also shows in the column sums).  The values are uniform on (-1, 1), not normal: |xh| stays
under sqrt(3), |dx| and |out| under 5, so no reference value comes within 1 of a sentinel (12345 in fp32 buffers, 7 in bf16 ones) and
"still equals the sentinel" means "never written".

A plain module (no fixtures): tests import it as `row_forms_ref`."""
import functools
from collections import namedtuple
from types import SimpleNamespace

import torch

import dropout_ref as D

SENT32, SENT16, GUARD = 12345.0, 7.0, 8
GATE_FWD, GATE_BWD, GATE_SUMSQ = 1e-5, 1e-4, 1e-5
MARGIN = 0.25                                   # the fp32 evaluation must sit within this share of a gate
P_DROP = 0.1
SEED, OFF_PRE, OFF_POST = 2 ** 63 + 77, 2 << 40, 3 << 40
F64, F32 = torch.float64, torch.float32


def tol(dtype):
    """The gate of a compute-type ("16-bit") output: tests/test_kernels_gpu.py's."""
    return 1e-3 if dtype == torch.float32 else 1e-2


# ------------------------------------------------------------------------------------------------ error measures
def row_err(got, ref):
    """Worst row of: max |got - ref| over the row / max |ref| over the row.  A row whose reference is all zero must be all zero."""
    got, ref = got.detach().double().cpu().reshape(ref.shape[0], -1), ref.detach().double().cpu().reshape(ref.shape[0], -1)
    d, m = (got - ref).abs().max(1).values, ref.abs().max(1).values
    e = torch.where(m > 0, d / m.clamp_min(1e-300), torch.where(d > 0, torch.full_like(d, float("inf")), torch.zeros_like(d)))
    return float(e.max())


def rel_err(got, ref):
    """Whole tensor: max |got - ref| / max |ref| (the column sums)."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-300))


def stats_err(stats, mean, rstd):
    """-> (mean error, rstd error), worst row each.  A row mean is a cancelled sum: its error is measured against the row's own scale,
    the standard deviation 1 / rstd, as the error of every other output of the row is; rstd against itself."""
    stats = stats.detach().double().cpu()
    return float(((stats[:, 0] - mean).abs() * rstd).max()), float(((stats[:, 1] - rstd).abs() / rstd).max())


def clear_of_sentinel(ref, sent):
    """No reference value within 1 of the sentinel."""
    return not bool(((ref > sent - 1) & (ref < sent + 1)).any())


# ------------------------------------------------------------------------------------------------ input builders
def uniform(*shape, seed):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed), dtype=F64) * 2 - 1


def row_factors(rows, seed):
    u = torch.linspace(-2, 2, rows, dtype=F64) if rows > 1 else torch.zeros(1, dtype=F64)
    u = u[torch.randperm(rows, generator=torch.Generator().manual_seed(seed))]
    i = int(u.argmax())
    u[i], u[rows - 1] = u[rows - 1].clone(), u[i].clone()
    return 10.0 ** u


def gamma_beta(N, seed):
    """fp32 (gamma, beta): 1 +- 0.3 and +- 0.3."""
    return (1 + 0.3 * uniform(N, seed=seed)).float(), (0.3 * uniform(N, seed=seed + 1)).float()


def scales(rows, N, p_pre, p_post, seed=SEED, off_pre=OFF_PRE, off_post=OFF_POST):
    """-> (keep_pre, keep_post, s_pre, s_post): bool ndarrays and fp64 scale tensors, None where that dropout is off."""
    eff = D.effective_seed(seed)
    kp = D.keep_mask(eff, off_pre, D.ln_idx(rows, N), p_pre) if p_pre else None
    kq = D.keep_mask(eff, off_post, D.ln_idx(rows, N), p_post) if p_post else None
    return kp, kq, (D.scale_of(kp, p_pre) if p_pre else None), (D.scale_of(kq, p_post) if p_post else None)


def stats_of(y, eps=1e-12):
    """Two-pass mean and rstd of the rows of y, in y's dtype (ln_body.h)."""
    mean = y.mean(-1)
    var = ((y - mean[:, None]) ** 2).mean(-1)
    return mean, 1.0 / torch.sqrt(var + eps)


# ------------------------------------------------------------------------------------------------ the formulas
def ln_fwd(x, gamma, beta, s_post=None, eps=1e-12):
    """-> dict(y, mean, rstd, out) in x's dtype: dropout_ref.layernorm_ref, which computes the two-pass form."""
    y, mean, rstd, out = D.layernorm_ref(x, gamma, beta, scale_post=s_post, eps=eps)
    return dict(y=y, mean=mean, rstd=rstd, out=out)


def ln_bwd(y, mean, rstd, gamma, dout, s_pre=None, s_post=None, period=0):
    """The closed form above, in the operands' dtype.  -> dict(dx, dxd, dgamma, dbeta, dbias[, dpos])."""
    dy = dout if s_post is None else dout * s_post
    xh = (y - mean[:, None]) * rstd[:, None]
    gq = dy * gamma
    s1, s2 = gq.mean(-1, keepdim=True), (gq * xh).mean(-1, keepdim=True)
    dx = rstd[:, None] * (gq - s1 - xh * s2)
    dxd = dx if s_pre is None else dx * s_pre
    out = dict(dx=dx, dxd=dxd, dgamma=(dy * xh).sum(0), dbeta=dy.sum(0), dbias=dxd.sum(0))
    if period:
        out["dpos"] = torch.zeros(period, y.shape[1], dtype=y.dtype).index_add_(0, torch.arange(y.shape[0]) % period, dx)
    return out


def added(base, inc):
    """An accumulating output as the test sees it, `got - base`, when the increment `inc` is added to the fp32 `base` in inc's
    dtype: the fp32 evaluation pays the rounding of that addition, as a kernel does."""
    return (base.to(inc.dtype) + inc).double() - base.double()


# ------------------------------------------------------------------------------------------------ LayerNorm backward cases
# csrc/layernorm.hip, univl_layernorm_bwd: 1 row per wave below 640 rows, 2 from 640 to 1279, 4 from 1280 (four waves per workgroup:
# 4, 8, 16 rows each); from 3072 rows at N == 768 without dpos the eight-wave body at 3 rows per wave, 24 rows per workgroup.
# Deterministic mode keeps the four-wave body at every row count.
LnCase = namedtuple("LnCase", "rows N period p_pre p_post")


def ln_id(c):
    return "rows%d-N%d%s%s%s" % (c.rows, c.N, "-dpos%d" % c.period if c.period else "", "-pre" if c.p_pre else "", "-post" if c.p_post else "")


LN_ATOMIC_CASES = (
    # on and beside each switch
    [LnCase(r, 768, 0, 0.0, 0.0) for r in (639, 640, 1279, 1280, 3071, 3072)]
    # ragged tails: 1 and 7 live rows of 8 in the last workgroup, 1 and 15 of 16, 1 and 23 of 24
    + [LnCase(r, 768, 0, 0.0, 0.0) for r in (641, 647, 1281, 1295, 3073, 3095)]
    # from 3072 rows on but on the four-wave body: N = 1024, and N = 768 with a position table (period 7: row % period ragged)
    + [LnCase(3073, 1024, 0, 0.0, 0.0), LnCase(3073, 768, 48, 0.0, 0.0), LnCase(3073, 768, 7, 0.0, 0.0)]
    # dropout in each form: p_post is the video tail's LayerNorm (N = 1024), p_pre a layer's
    + [LnCase(647, 768, 0, P_DROP, 0.0), LnCase(647, 1024, 0, 0.0, P_DROP), LnCase(1295, 768, 0, P_DROP, 0.0),
       LnCase(3095, 1024, 0, 0.0, P_DROP), LnCase(3095, 768, 0, P_DROP, 0.0), LnCase(3095, 768, 0, 0.0, P_DROP)])

# one launch grid per rows-per-wave value; the periods give the gather's four partial sums every tail: rows per position % 4 is
# 1 / 0 at (61, 7), 2 / 1 at (647, 48), 3 / 2 at (1295, 48) and (3095, 7)
LN_DET_CASES = [LnCase(61, 768, 7, 0.0, 0.0), LnCase(647, 768, 48, P_DROP, 0.0), LnCase(647, 1024, 7, 0.0, P_DROP),
                LnCase(1295, 768, 48, 0.0, 0.0), LnCase(3095, 768, 7, P_DROP, 0.0)]
LN_DET_FORMS = ["dpos+dx32", "dpos-scratch", "no-dpos"]


@functools.lru_cache(maxsize=2)
def ln_case(c):
    """Inputs (fp32, as the kernel reads them), bases of the accumulating outputs and the fp64 reference of one LayerNorm backward."""
    sd = 1000 * c.rows + c.N
    f = row_factors(c.rows, sd)[:, None]
    y64 = f * uniform(c.rows, c.N, seed=sd + 1)
    mean64, rstd64 = stats_of(y64)
    gamma, _ = gamma_beta(c.N, sd + 2)
    i = SimpleNamespace(y=y64.float(), stats=torch.stack([mean64, rstd64], 1).float().contiguous(), gamma=gamma,
                        dout=(f * uniform(c.rows, c.N, seed=sd + 3)).float())
    i.keep_pre, i.keep_post, i.s_pre, i.s_post = scales(c.rows, c.N, c.p_pre, c.p_post)
    i.base = {k: uniform(c.N, seed=sd + 4 + j).float() for j, k in enumerate(("dgamma", "dbeta", "dbias"))}
    if c.period:
        i.base["dpos"] = uniform(c.period, c.N, seed=sd + 8).float()
    i.ref = ln_eval(i, c.period, F64)
    return i


def ln_eval(i, period, dtype):
    """ln_bwd on the case's inputs in `dtype`."""
    c = lambda t: None if t is None else t.to(dtype)
    return ln_bwd(c(i.y), c(i.stats[:, 0]), c(i.stats[:, 1]), c(i.gamma), c(i.dout), c(i.s_pre), c(i.s_post), period)


def ln_errors(got, i, dtype16, skip=()):
    """got: dict of outputs (accumulating ones as got - base, fp64).  -> {name: (error, gate)}."""
    r = i.ref
    e = {}
    for k, ref, gate in (("dx32", r["dx"], GATE_BWD), ("dxd32", r["dxd"], GATE_BWD), ("dxd16", r["dxd"], tol(dtype16))):
        if k in got and k not in skip:
            e[k] = (row_err(got[k], ref), gate)
    for k in ("dgamma", "dbeta", "dbias", "dpos"):
        if k in got and k in r:
            e[k] = (rel_err(got[k], r[k]), GATE_BWD)
    return e


def ln_eval32_errors(i, period, dtype16=torch.float32):
    """The margin evaluation of one case: the formulas in fp32 (the compute-type output rounded to dtype16), measured as the kernel's
    outputs are."""
    v = ln_eval(i, period, F32)
    got = dict(dx32=v["dx"], dxd32=v["dxd"], dxd16=v["dxd"].to(dtype16))
    for k in i.base:
        got[k] = added(i.base[k], v[k])
    return ln_errors(got, i, dtype16)


# ------------------------------------------------------------------------------------------------ the fold's LayerNorm backward
FOLD_CASES = [(100, 3072, 8, P_DROP), (624, 2304, 3, 0.0)]          # (T, K_out, ks, p_pre) of test_gemm_pair_ln_fold_matches_the_two_launches
FOLD_SEED, FOLD_OFF = 9, 2 << 40


@functools.lru_cache(maxsize=2)
def fold_case(T, K_out, ks, p_pre):
    """Operands of the pair launch (dY, W, X in bf16; the residual, y, stats, gamma in fp32).  dY, the residual and y carry the row
    factors; dY and the residual are kept small enough for |dx| < 5 (da = dY W + residual has a standard deviation near 0.2 f)."""
    H, sd = 768, 77 * T
    f = row_factors(T, sd)[:, None]
    i = SimpleNamespace(dY=(0.25 * f * uniform(T, K_out, seed=sd + 1)).to(torch.bfloat16),
                        W=(0.035 * uniform(K_out, H, seed=sd + 2)).to(torch.bfloat16),
                        X=uniform(T, H, seed=sd + 3).to(torch.bfloat16),
                        res=(0.25 * f * uniform(T, H, seed=sd + 4)).float(), gamma=gamma_beta(H, sd + 5)[0])
    y64 = f * uniform(T, H, seed=sd + 6)
    mean64, rstd64 = stats_of(y64)
    i.y, i.stats = y64.float(), torch.stack([mean64, rstd64], 1).float().contiguous()
    eff = D.effective_seed(FOLD_SEED)
    i.keep_pre = D.keep_mask(eff, FOLD_OFF, D.ln_idx(T, H), p_pre) if p_pre else None
    i.s_pre, i.s_post = (D.scale_of(i.keep_pre, p_pre) if p_pre else None), None
    i.base = {k: uniform(H, seed=sd + 7 + j).float() for j, k in enumerate(("dgamma", "dbeta", "dbias"))}
    # the dgrad product as fp64 arithmetic on the bf16 operands: what the launch's da equals up to fp32 summation noise
    i.da64 = i.dY.double() @ i.W.double() + i.res.double()
    return i


def fold_ref(i, da):
    """fp64 LayerNorm backward of the da the launch produced (fp32, read back)."""
    i.dout = da.detach().float().cpu()
    i.ref = ln_eval(i, 0, F64)
    return i.ref


# ------------------------------------------------------------------------------------------------ text embedding cases
EmbCase = namedtuple("EmbCase", "B S P ids types p_post")       # P: rows of the position table; types: rows of the type table (0: none)
EMB_V, EMB_N = 500, 768
EMB_CASES = [EmbCase(3, 21, 64, "mixed", 2, 0.0),        # 63 tokens: three live waves in the last workgroup
             EmbCase(3, 21, 21, "mixed", 3, P_DROP),     # a position table of exactly S rows; token types 0, 1, 2
             EmbCase(1, 1, 64, "mixed", 0, 0.0),         # one token, no type table (the decoder's form)
             EmbCase(5, 13, 64, "same", 3, 0.0),         # 65 tokens: one live wave in the last workgroup; every token the same id
             EmbCase(5, 13, 64, "distinct", 0, 0.0),
             EmbCase(5, 13, 13, "mixed", 2, P_DROP)]
EMB_SEED, EMB_OFF = 42, 4 << 40


def emb_id(c):
    return "B%d-S%d-P%d-%s-types%d%s" % (c.B, c.S, c.P, c.ids, c.types, "-post" if c.p_post else "")


def _emb_tables(wr, pr, tr, ids, tts, S):
    e = wr[ids] + pr[torch.arange(S)][None]
    return e if tr is None else e + tr[tts]


@functools.lru_cache(maxsize=None)
def emb_case(c):
    """Tables, ids, the kernel's backward inputs (y, stats rounded from fp64) and the fp64 references of both directions.  Row v of the
    word table carries the factor f(v), a token's dout row the factor of its word row; position and type rows are +- 0.5."""
    T, V, N, sd = c.B * c.S, EMB_V, EMB_N, 31 * c.B * c.S + c.types
    g = torch.Generator().manual_seed(sd)
    if c.ids == "same":
        ids = torch.full((T,), V - 1)
    elif c.ids == "distinct":
        ids = torch.cat([torch.tensor([0, V - 1]), 1 + torch.randperm(V - 2, generator=g)[:T - 2]])[torch.randperm(T, generator=g)]
    else:
        ids = torch.randint(0, V, (T,), generator=g)
        ids[0] = V - 1
        if T > 1:
            ids[T - 1] = 0
            ids[1:min(T - 1, 6)] = 7                       # repeated ids: several tokens meet in one table row
    ids = ids.view(c.B, c.S).contiguous()
    tts = (torch.randint(0, c.types, (c.B, c.S), generator=g) if c.types else None)
    if c.types and T >= c.types:
        tts.view(-1)[:c.types] = torch.arange(c.types)     # every type occurs
    fw = row_factors(V, sd + 1)
    i = SimpleNamespace(ids=ids, tts=tts, word=(fw[:, None] * uniform(V, N, seed=sd + 2)).float(), pos=(0.5 * uniform(c.P, N, seed=sd + 3)).float(),
                        typ=(0.5 * uniform(c.types, N, seed=sd + 4)).float() if c.types else None)
    i.gamma, i.beta = gamma_beta(N, sd + 5)
    i.dout = (fw[ids.view(-1)][:, None] * uniform(T, N, seed=sd + 6)).float()
    i.keep_pre, i.s_pre = None, None
    i.keep_post = D.keep_mask(D.effective_seed(EMB_SEED), EMB_OFF, D.ln_idx(T, N), c.p_post) if c.p_post else None
    i.s_post = D.scale_of(i.keep_post, c.p_post) if c.p_post else None
    e64 = _emb_tables(i.word.double(), i.pos.double(), None if i.typ is None else i.typ.double(), ids, tts, c.S).view(T, N)
    i.fwd_ref = ln_fwd(e64, i.gamma.double(), i.beta.double(), i.s_post)
    # the backward's own inputs: y and stats prepared in fp64 and rounded
    i.y, i.stats = e64.float(), torch.stack([i.fwd_ref["mean"], i.fwd_ref["rstd"]], 1).float().contiguous()
    i.base = dict(dword=uniform(V, N, seed=sd + 7).float(), dpos=uniform(c.P, N, seed=sd + 8).float(),
                  dgamma=uniform(N, seed=sd + 9).float(), dbeta=uniform(N, seed=sd + 10).float())
    if c.types:
        i.base["dtype_emb"] = uniform(c.types, N, seed=sd + 11).float()
    i.ref = emb_bwd(c, i, F64)
    return i


def emb_fwd32(c, i):
    """The embedding forward in fp32: the sum of the table rows, then ln_fwd."""
    e = _emb_tables(i.word, i.pos, i.typ, i.ids, i.tts, c.S).view(c.B * c.S, EMB_N)
    return ln_fwd(e, i.gamma, i.beta, None if i.s_post is None else i.s_post.float())


def emb_scatter(c, i, drows):
    """Per-token rows -> increments of the word / position / type tables, in drows' dtype."""
    t = dict(dword=torch.zeros(EMB_V, EMB_N, dtype=drows.dtype).index_add_(0, i.ids.view(-1), drows),
             dpos=torch.zeros(c.P, EMB_N, dtype=drows.dtype).index_add_(0, torch.arange(c.B * c.S) % c.S, drows))
    if c.types:
        t["dtype_emb"] = torch.zeros(c.types, EMB_N, dtype=drows.dtype).index_add_(0, i.tts.view(-1), drows)
    return t


def emb_bwd(c, i, dtype):
    """-> dict(drows, dword, dpos[, dtype_emb], dgamma, dbeta): increments, in `dtype`."""
    v = ln_eval(i, 0, dtype)
    out = dict(drows=v["dx"], dgamma=v["dgamma"], dbeta=v["dbeta"])
    out.update(emb_scatter(c, i, v["dx"]))
    return out


def emb_touched(c, i):
    """-> {table: bool [rows]}: the rows some token writes."""
    t = dict(dword=torch.zeros(EMB_V, dtype=torch.bool), dpos=torch.zeros(c.P, dtype=torch.bool))
    t["dword"][i.ids.view(-1)] = True
    t["dpos"][:c.S] = True
    if c.types:
        t["dtype_emb"] = torch.zeros(c.types, dtype=torch.bool)
        t["dtype_emb"][i.tts.view(-1)] = True
    return t


def emb_errors(c, i, got):
    """got: increments (got - base) of the tables and column sums, drows as stored.  Table rows that a token touches are measured
    per row, the column sums dgamma / dbeta over the whole tensor.  -> {name: (error, gate)}."""
    e, touched = {}, emb_touched(c, i)
    if "drows" in got:
        e["drows"] = (row_err(got["drows"], i.ref["drows"]), GATE_BWD)
    for k in ("dword", "dpos", "dtype_emb"):
        if k in got:
            e[k] = (row_err(got[k][touched[k]], i.ref[k][touched[k]]), GATE_BWD)
    for k in ("dgamma", "dbeta"):
        if k in got:
            e[k] = (rel_err(got[k], i.ref[k]), GATE_BWD)
    return e


def emb_eval32_errors(c, i):
    v = emb_bwd(c, i, F32)
    got = {k: added(i.base[k], v[k]) for k in i.base}
    got["drows"] = v["drows"]
    return emb_errors(c, i, got)


def fwd_errors(got, ref, dtype16):
    """got: dict(y, stats, out32, out16) -> {name: (error, gate)} against ln_fwd's fp64 dict."""
    em, er = stats_err(got["stats"], ref["mean"], ref["rstd"])
    return dict(y=(row_err(got["y"], ref["y"]), GATE_FWD), mean=(em, GATE_FWD), rstd=(er, GATE_FWD),
                out32=(row_err(got["out32"], ref["out"]), GATE_FWD), out16=(row_err(got["out16"], ref["out"]), tol(dtype16)))


def fwd_eval32_errors(v, ref, dtype16=torch.float32):
    """v: ln_fwd's dict from an fp32 evaluation."""
    return fwd_errors(dict(y=v["y"], stats=torch.stack([v["mean"], v["rstd"]], 1), out32=v["out"], out16=v["out"].to(dtype16)), ref, dtype16)


# ------------------------------------------------------------------------------------------------ LayerNorm forward, float64 input
FWD_CASES = [(61, 768), (61, 1024)]
FWD_ZERO_ROWS = [7, 8, 59]                              # all-zero input rows (padded video frames): out must be exactly beta


@functools.lru_cache(maxsize=None)
def fwd_case(rows, N):
    sd = 500 * rows + N
    x = row_factors(rows, sd)[:, None] * uniform(rows, N, seed=sd + 1)
    x[FWD_ZERO_ROWS] = 0.0
    i = SimpleNamespace(x=x)
    i.gamma, i.beta = gamma_beta(N, sd + 2)
    i.ref = ln_fwd(x, i.gamma.double(), i.beta.double())
    return i


# ------------------------------------------------------------------------------------------------ listed rows of the word table
ROWS_TOTAL, ROWS_CAP = 300, 320
ROWS_LISTS = ["distinct", "twice", "overflow", "empty"]


@functools.lru_cache(maxsize=None)
def rows_case(kind):
    """-> table [300, 768] fp32, list [ROWS_CAP] int64, meta [2] int32, the listed rows (sorted, each once), the scalar's base.
    `twice`: 290 entries over 280 rows -- a second listing below entry 256, and rows first listed at entries 260 .. 264 listed again
    behind them, so that the 256-wide scan for an earlier listing takes a second trip and finds one there."""
    g = torch.Generator().manual_seed(ROWS_LISTS.index(kind))
    table = (row_factors(ROWS_TOTAL, 5)[:, None] * uniform(ROWS_TOTAL, EMB_N, seed=6)).float()
    lst = torch.zeros(ROWS_CAP, dtype=torch.int64)
    if kind == "distinct":
        rows = torch.cat([torch.tensor([0, ROWS_TOTAL - 1]), 1 + torch.randperm(ROWS_TOTAL - 2, generator=g)[:38]])
        rows = rows[torch.randperm(40, generator=g)]
        lst[:40], meta = rows, [40, 0]
    elif kind == "twice":
        rows = torch.randperm(ROWS_TOTAL, generator=g)[:280]
        entries = torch.cat([rows[:100], rows[20:25], rows[100:], rows[255:260]])
        assert entries.numel() == 290 and torch.equal(entries[260:265], entries[285:])
        lst[:290], meta = entries, [290, 0]
    elif kind == "overflow":
        rows = torch.arange(ROWS_TOTAL)
        lst[:5], meta = torch.tensor([3, 4, 5, 6, 7]), [5, 1]
    else:
        rows = torch.zeros(0, dtype=torch.int64)
        lst[:3], meta = torch.tensor([1, 2, 3]), [0, 0]           # stale entries behind meta[0] == 0 are not listed
    listed = torch.unique(rows)
    return SimpleNamespace(table=table, list=lst, meta=torch.tensor(meta, dtype=torch.int32), listed=listed,
                           base=torch.tensor([0.37], dtype=F32), ref=float((table[listed].double() ** 2).sum()))


def sumsq_err(inc, ref):
    return abs(float(inc) - ref) / max(abs(ref), 1e-300)
