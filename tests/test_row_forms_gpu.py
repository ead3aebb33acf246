"""The row kernels against fp64 in every launch form: univl_layernorm_bwd at and beside its row-count switches, with the ragged tail of
each form, in atomic and in deterministic mode; the LayerNorm backward inside univl_gemm_pair_ln; the text embedding in both
directions and both modes, with its per-token-rows form; univl_rows_sumsq / univl_rows_zero; the float64-input LayerNorm forward with
a bf16 output.  Cases, inputs, references and error measures: tests/row_forms_ref.py.  Needs a real MI355X (`-m gpu`).

Launch forms of univl_layernorm_bwd (csrc/layernorm.hip): four waves per workgroup at 1 row per wave below 640 rows, 2 from 640 to
1279, 4 from 1280; from 3072 rows at N == 768 without dpos the eight-wave body ln_bwd_kernel<768, T, false, 8> at 3 rows per wave,
24 rows per workgroup.  Deterministic mode keeps the four-wave body and gathers dpos from the fp32 dx rows afterwards.

Conventions of every case:
  * stored outputs (dx32, dxd32, dxd16, drows, y, out32, out16, stats) have 8 guard rows and start as a sentinel everywhere (12345 in
    fp32 buffers, 7 in bf16 ones): the guard rows keep their bits, no live element keeps the sentinel -- no reference value lies
    within 1 of it (tests/test_row_forms_cpu.py), so a row the kernel did not write cannot pass on what an earlier case left behind;
  * accumulating outputs (dgamma, dbeta, dbias, dpos, dword, dtype_emb, the sum of squares) start from a random base; got - base is
    compared, and table rows that no token touches keep the base bit for bit;
  * rows of x and dout carry factors from 1e-2 to 1e2, and row outputs are gated per row: max |error| over the row's max |reference|,
    worst row -- a wrong row of small magnitude cannot hide under a large one.  Column sums keep the whole-tensor measure.

Gates: 1e-5 forward fp32 outputs and stats, 1e-4 backward fp32 outputs and column sums, tol(dtype) compute-type outputs.  The same
formulas in torch fp32 stay within a quarter of each on these inputs (tests/test_row_forms_cpu.py).  Every case prints its errors
(`pytest -s`); profiles/row_kernel_forms.txt is that output."""
import contextlib

import pytest
import torch

import row_forms_ref as R

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import univl_amd
    from univl_amd import ops

DEV = "cuda"
BF16 = torch.bfloat16
DTYPES = [torch.float32, BF16]
DTYPE_IDS = ["fp32", "bf16"]


@contextlib.contextmanager
def _mode(on):
    was = univl_amd.deterministic()
    univl_amd.set_deterministic(on)
    try:
        yield
    finally:
        univl_amd.set_deterministic(was)


@pytest.fixture(params=[False, True], ids=["atomic", "deterministic"])
def mode(request):
    with _mode(request.param):
        yield request.param


def _dev(t):
    return None if t is None else t.to(DEV)


def _sent(dtype):
    return R.SENT16 if dtype == BF16 else R.SENT32


def _guarded(rows, cols, dtype=torch.float32):
    return torch.full((rows + R.GUARD, cols), _sent(dtype), device=DEV, dtype=dtype)


def _check_guarded(case, bufs, rows):
    """The guard rows still hold the sentinel's bits; no live element does."""
    for k, b in bufs.items():
        assert torch.equal(_bits(b[rows:]), _bits(torch.full_like(b[rows:], _sent(b.dtype)))), (case, k, "guard rows written")
        assert not bool((b[:rows] == _sent(b.dtype)).any()), (case, k, "a live element was not written")


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same_bits(a, b):
    return all(torch.equal(_bits(a[k]), _bits(b[k])) for k in a)


def _report(case, errs):
    print("row-forms-gpu  %-60s %s" % (case, "  ".join("%s %.2e/%.0e" % (k, e, g) for k, (e, g) in errs.items())))


def _gate(case, errs):
    _report(case, errs)
    for k, (e, g) in errs.items():
        assert e < g, (case, k, e, g)


def _increments(acc, base):
    return {k: a.double().cpu() - base[k].double() for k, a in acc.items()}


# ------------------------------------------------------------------------------------------------ LayerNorm backward
def _ln_inputs(i):
    return dict(gamma=_dev(i.gamma), y=_dev(i.y), stats=_dev(i.stats), dout=_dev(i.dout))


def _ln_bwd_run(c, i, inp, dtype, dx32=True, dpos=True):
    """One launch on fresh output buffers.  -> (stored outputs with their guard rows, accumulating outputs)."""
    out = dict(dxd32=_guarded(c.rows, c.N), dxd16=_guarded(c.rows, c.N, dtype))
    if dx32:
        out["dx32"] = _guarded(c.rows, c.N)
    acc = {k: _dev(v) for k, v in i.base.items() if dpos or k != "dpos"}
    ops.layernorm_bwd(dtype=ops.dtype_code(dtype), rows=c.rows, N=c.N, pos_period=c.period if "dpos" in acc else 0,
                      p_pre=c.p_pre, p_post=c.p_post, seed=R.SEED, off_pre=R.OFF_PRE, off_post=R.OFF_POST, **inp, **out, **acc)
    torch.cuda.synchronize()
    return out, acc


def _ln_check(case, c, i, out, acc, dtype):
    _check_guarded(case, out, c.rows)
    got = {k: b[:c.rows] for k, b in out.items()}
    got.update(_increments(acc, i.base))
    _gate(case, R.ln_errors(got, i, dtype))
    if c.p_pre:
        dropped = ~torch.from_numpy(i.keep_pre)
        assert bool((got["dxd32"].cpu()[dropped] == 0).all()) and bool((got["dxd16"].cpu()[dropped] == 0).all()), \
            (case, "the gradient of a dropped input is not exactly 0.0")


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("c", R.LN_ATOMIC_CASES, ids=R.ln_id)
def test_layernorm_bwd_atomic_forms(c, dtype):
    with _mode(False):
        i = R.ln_case(c)
        out, acc = _ln_bwd_run(c, i, _ln_inputs(i), dtype)
        _ln_check("ln_bwd atomic %s %s" % (R.ln_id(c), DTYPE_IDS[DTYPES.index(dtype)]), c, i, out, acc, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("form", R.LN_DET_FORMS)
@pytest.mark.parametrize("c", R.LN_DET_CASES, ids=R.ln_id)
def test_layernorm_bwd_deterministic_forms(c, form, dtype):
    """dpos+dx32: the gather reads the caller's dx32; dpos-scratch: dx32 absent, the rows go through the scratch ring; no-dpos.
    Three launches from identically prepared buffers give the same bits."""
    with _mode(True):
        i = R.ln_case(c)
        inp = _ln_inputs(i)
        runs = [_ln_bwd_run(c, i, inp, dtype, dx32=form != "dpos-scratch", dpos=form != "no-dpos") for _ in range(3)]
        case = "ln_bwd det %s %s %s" % (R.ln_id(c), form, DTYPE_IDS[DTYPES.index(dtype)])
        _ln_check(case, c, i, runs[0][0], runs[0][1], dtype)
        for out, acc in runs[1:]:
            assert _same_bits(runs[0][0], out) and _same_bits(runs[0][1], acc), (case, "repeats differ")


# ------------------------------------------------------------------------------------------------ the fold's LayerNorm backward
@pytest.mark.parametrize("T,K_out,ks,p_pre", R.FOLD_CASES)
def test_fold_layernorm_bwd_against_fp64(T, K_out, ks, p_pre):
    """univl_gemm_pair_ln: one launch; the fp64 LayerNorm backward of the da that launch produced, under the same y, stats, gamma and
    pre-dropout mask -- the fold's rows and column sums compared with fp64 directly, not through univl_layernorm_bwd."""
    with _mode(False):
        H = 768
        i = R.fold_case(T, K_out, ks, p_pre)
        dY, W, X, res = _dev(i.dY), _dev(i.W), _dev(i.X), _dev(i.res)
        gamma, y, stats = _dev(i.gamma), _dev(i.y), _dev(i.stats)
        da, dW, db = torch.zeros(T, H, device=DEV), torch.zeros(K_out, H, device=DEV), torch.zeros(K_out, device=DEV)
        out = dict(dx32=_guarded(T, H), dxd16=_guarded(T, H, BF16))
        acc = {k: _dev(v) for k, v in i.base.items()}
        dg = ops.gemm_desc(dY, W, T, H, K_out, trans_b=True, out32=da, residual=res, ksplit=ks)
        wg = ops.gemm_desc(dY, X, K_out, H, T, trans_a=True, trans_b=True, out32=dW, dbias=db)
        ln = ops.layernorm_desc(ops.dtype_code(BF16), T, H, gamma=gamma, y=y, stats=stats, dout=da, p_pre=p_pre, seed=R.FOLD_SEED,
                                off_pre=R.FOLD_OFF, **out, **acc)
        ctr = torch.zeros(2 * ((T + 63) // 64), dtype=torch.int32, device=DEV)
        assert ops.gemm_pair_ln(dg, wg, ln, ctr, dry_run=True)
        assert ops.gemm_pair_ln(dg, wg, ln, ctr)
        torch.cuda.synchronize()
        assert int(ctr.abs().sum()) == 0, "arrival counters not back at zero"
        case = "fold T=%d K_out=%d ks=%d p_pre=%g" % (T, K_out, ks, p_pre)
        print("row-forms-gpu  %-60s da against the fp64 product of the same operands %.2e" % (case, R.row_err(da, i.da64)))
        ref = R.fold_ref(i, da)
        assert R.clear_of_sentinel(ref["dx"], R.SENT32) and R.clear_of_sentinel(ref["dxd"], R.SENT16)
        _check_guarded(case, out, T)
        got = {k: b[:T] for k, b in out.items()}
        got.update(_increments(acc, i.base))
        _gate(case, R.ln_errors(got, i, BF16))
        if p_pre:
            assert bool((got["dxd16"].cpu()[~torch.from_numpy(i.keep_pre)] == 0).all())


# ------------------------------------------------------------------------------------------------ text embedding
def _emb_args(c, i):
    return (c.B, c.S, _dev(i.ids), _dev(i.word), _dev(i.pos), _dev(i.gamma), _dev(i.beta)), \
        dict(type_ids=_dev(i.tts), type_emb=_dev(i.typ), p_post=c.p_post, seed=R.EMB_SEED, off_post=R.EMB_OFF)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("c", R.EMB_CASES, ids=R.emb_id)
def test_embed_text_fwd_forms(c, dtype):
    i, T, N = R.emb_case(c), c.B * c.S, R.EMB_N
    a, kw = _emb_args(c, i)
    out = dict(y=_guarded(T, N), stats=_guarded(T, 2), out32=_guarded(T, N), out16=_guarded(T, N, dtype))
    ops.embed_text_fwd(ops.dtype_code(dtype), *a, **kw, **out)
    torch.cuda.synchronize()
    case = "embed_fwd %s %s" % (R.emb_id(c), DTYPE_IDS[DTYPES.index(dtype)])
    _check_guarded(case, out, T)
    _gate(case, R.fwd_errors({k: b[:T] for k, b in out.items()}, i.fwd_ref, dtype))
    if c.p_post:
        dropped = ~torch.from_numpy(i.keep_post)
        assert bool((out["out32"][:T].cpu()[dropped] == 0).all()) and bool((out["out16"][:T].cpu()[dropped] == 0).all())


def _emb_bwd_run(c, i, a, kw, inp, drows=None):
    """One launch on fresh copies of the bases; with drows the position table is left to the caller (dpos null)."""
    acc = {k: _dev(v) for k, v in i.base.items()}
    ops.embed_text_bwd(ops.dtype_code(torch.float32), *a, **kw, **inp, dword=acc["dword"], dpos=None if drows is not None else acc["dpos"],
                       dtype_emb=acc.get("dtype_emb"), dgamma=acc["dgamma"], dbeta=acc["dbeta"], drows=drows)
    torch.cuda.synchronize()
    return acc


def _untouched_keep_the_base(case, c, i, acc, names):
    for k, t in R.emb_touched(c, i).items():
        if k in names:
            assert torch.equal(_bits(acc[k].cpu()[~t]), _bits(i.base[k][~t])), (case, k, "a row no token touches was written")


@pytest.mark.parametrize("c", R.EMB_CASES, ids=R.emb_id)
def test_embed_text_bwd_forms(c, mode):
    i = R.emb_case(c)
    a, kw = _emb_args(c, i)
    inp = dict(y=_dev(i.y), stats=_dev(i.stats), dout=_dev(i.dout))
    runs = [_emb_bwd_run(c, i, a, kw, inp) for _ in range(3 if mode else 1)]
    case = "embed_bwd %s %s" % (R.emb_id(c), "det" if mode else "atomic")
    _gate(case, R.emb_errors(c, i, _increments(runs[0], i.base)))
    _untouched_keep_the_base(case, c, i, runs[0], ("dword", "dpos", "dtype_emb"))
    for acc in runs[1:]:
        assert _same_bits(runs[0], acc), (case, "repeats differ")


@pytest.mark.parametrize("c", R.EMB_CASES, ids=R.emb_id)
def test_embed_text_bwd_drows_form(c, mode):
    """drows given, dpos null (the 128-pair plans): the per-token rows come out, the word table is left to the caller in both modes;
    then the tables are built from the rows as steps.py's _text_tail does."""
    i, T, N = R.emb_case(c), c.B * c.S, R.EMB_N
    a, kw = _emb_args(c, i)
    inp = dict(y=_dev(i.y), stats=_dev(i.stats), dout=_dev(i.dout))
    case = "embed_bwd drows %s %s" % (R.emb_id(c), "det" if mode else "atomic")
    runs = []
    for _ in range(3 if mode else 1):
        drows = _guarded(T, N)
        acc = _emb_bwd_run(c, i, a, kw, inp, drows=drows)
        for k in ("dword", "dpos"):
            assert torch.equal(_bits(acc[k].cpu()), _bits(i.base[k])), (case, k, "written although drows was given")
        ops.embed_scatter(a[2].view(-1), drows[:T], 1.0, acc["dword"])
        ops.rows_gather_sum(drows[:T], c.S, acc["dpos"][:c.S])
        torch.cuda.synchronize()
        runs.append(dict(acc, drows=drows))
    first = runs[0]
    _check_guarded(case, dict(drows=first["drows"]), T)
    got = _increments({k: v for k, v in first.items() if k != "drows"}, i.base)
    got["drows"] = first["drows"][:T]
    _gate(case, R.emb_errors(c, i, got))
    _untouched_keep_the_base(case, c, i, first, ("dword", "dpos", "dtype_emb"))
    for r in runs[1:]:
        assert _same_bits(first, r), (case, "repeats differ")


# ------------------------------------------------------------------------------------------------ listed rows of the word table
@pytest.mark.parametrize("kind", R.ROWS_LISTS)
def test_rows_sumsq_and_rows_zero(kind, mode):
    i = R.rows_case(kind)
    buf = torch.full((R.ROWS_TOTAL + R.GUARD, R.EMB_N), R.SENT32, device=DEV)
    buf[:R.ROWS_TOTAL] = _dev(i.table)
    table, lst, meta = buf[:R.ROWS_TOTAL], _dev(i.list), _dev(i.meta)
    outs = []
    for _ in range(3 if mode else 1):
        out = _dev(i.base.clone())
        ops.rows_sumsq(table, lst, meta, out)
        outs.append(out)
    torch.cuda.synchronize()
    case = "rows_sumsq %s %s" % (kind, "det" if mode else "atomic")
    assert torch.equal(_bits(table.cpu()), _bits(i.table)), (case, "the table was written")
    if kind == "empty":
        assert torch.equal(_bits(outs[0].cpu()), _bits(i.base)), (case, "nothing is listed, the sum moved")
    else:
        _gate(case, dict(sumsq=(R.sumsq_err(float(outs[0].double().cpu() - i.base.double()), i.ref), R.GATE_SUMSQ)))
    for o in outs[1:]:
        assert torch.equal(_bits(outs[0]), _bits(o)), (case, "repeats differ")
    ops.rows_zero(table, lst, meta)
    torch.cuda.synchronize()
    after = buf.cpu()
    listed = torch.zeros(R.ROWS_TOTAL + R.GUARD, dtype=torch.bool)
    listed[i.listed] = True
    assert bool((_bits(after[listed]) == 0).all()), (case, "a listed row is not zero")
    want = torch.cat([i.table, torch.full((R.GUARD, R.EMB_N), R.SENT32)])
    assert torch.equal(_bits(after[~listed]), _bits(want[~listed])), (case, "a row that is not listed was written")


# ------------------------------------------------------------------------------------------------ LayerNorm forward, float64 input
@pytest.mark.parametrize("rows,N", R.FWD_CASES)
def test_layernorm_fwd_f64_input_bf16_output(rows, N):
    """NormalizeVideo's form with the compute-type output in bf16; 61 rows leave one live wave in the last workgroup.  All-zero input
    rows give exactly beta, rounded to bf16 in out16."""
    i = R.fwd_case(rows, N)
    out = dict(y=_guarded(rows, N), stats=_guarded(rows, 2), out32=_guarded(rows, N), out16=_guarded(rows, N, BF16))
    ops.layernorm_fwd(dtype=ops.dtype_code(BF16), rows=rows, N=N, x=_dev(i.x), x_f64=True, gamma=_dev(i.gamma), beta=_dev(i.beta), **out)
    torch.cuda.synchronize()
    case = "ln_fwd f64-in rows=%d N=%d bf16" % (rows, N)
    _check_guarded(case, out, rows)
    _gate(case, R.fwd_errors({k: b[:rows] for k, b in out.items()}, i.ref, BF16))
    z = R.FWD_ZERO_ROWS
    assert torch.equal(out["out32"][z].cpu(), i.beta.expand(len(z), N)), "a zero row is not exactly beta"
    assert torch.equal(_bits(out["out16"][z].cpu()), _bits(i.beta.to(BF16).expand(len(z), N))), "a zero row is not exactly bf16(beta)"
