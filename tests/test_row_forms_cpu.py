"""The references and gates of tests/test_row_forms_gpu.py, checked without a GPU (tests/row_forms_ref.py).

1. The closed-form fp64 backward against torch autograd in fp64, to 1e-12: LayerNorm with both dropouts and a position table, and the
   text embedding with its table scatters.
2. Margin: on the exact inputs of every GPU case the same formulas evaluated in torch fp32, measured the way the GPU test measures the
   kernels, stay within a quarter of each gate.  The gates (1e-5 forward, 1e-4 backward and column sums, tol(dtype) for compute-type
   outputs) are therefore met with room by reference-precision arithmetic alone.  `pytest -s` prints the figures:
   profiles/row_kernel_forms.txt holds them.
3. No reference value lies within 1 of a buffer's sentinel, so "a live element still equals the sentinel" can only mean "not written".
4. The case lists reach what they claim: each launch form, each ragged tail, every tail term of the position gather."""
import pytest
import torch

import row_forms_ref as R

BF16 = torch.bfloat16


def _report(case, errs):
    print("row-forms-cpu  %-44s %s" % (case, "  ".join("%s %.2e/%.0e" % (k, e, g) for k, (e, g) in errs.items())))


def _within_margin(case, errs, errs16=None):
    """errs: the fp32 evaluation.  errs16: the same with the compute-type output rounded to bf16 -- that rounding alone is up to half
    an ulp, 2 ** -8 of the value, which is the number format's share of the 1e-2 gate and no part of the margin."""
    _report(case, errs)
    for k, (e, g) in errs.items():
        assert e <= R.MARGIN * g, (case, k, e, g)
    for k in ("dxd16", "out16"):
        if errs16 and k in errs16:
            _report(case + " bf16", {k: errs16[k]})
            assert errs16[k][0] <= 2.0 ** -8 + errs[k][0] < R.tol(BF16), (case, k, errs16[k])


# ------------------------------------------------------------------------------------------------ 1. the closed form against autograd
@pytest.mark.parametrize("p_pre,p_post,period", [(0.0, 0.0, 0), (0.1, 0.0, 7), (0.0, 0.1, 0), (0.1, 0.1, 5)])
def test_closed_form_layernorm_backward_equals_autograd(p_pre, p_post, period):
    rows, N = 23, 768
    _, _, s_pre, s_post = R.scales(rows, N, p_pre, p_post)
    f = R.row_factors(rows, 1)[:, None]
    x = (f * R.uniform(rows, N, seed=2)).requires_grad_(True)
    pos = R.uniform(max(period, 1), N, seed=3).requires_grad_(True)
    gamma, beta = (t.double().requires_grad_(True) for t in R.gamma_beta(N, 4))
    dout = f * R.uniform(rows, N, seed=6)
    rowpos = pos[torch.arange(rows) % period] if period else None
    y, mean, rstd, out = R.D.layernorm_ref(x, gamma, beta, rowpos=rowpos, scale_pre=s_pre, scale_post=s_post)
    y.retain_grad()
    out.backward(dout)
    v = R.ln_bwd(y.detach(), mean.detach(), rstd.detach(), gamma.detach(), dout, s_pre, s_post, period)
    want = dict(dx=y.grad, dxd=x.grad, dgamma=gamma.grad, dbeta=beta.grad, dbias=x.grad.sum(0))
    if period:
        want["dpos"] = pos.grad
    for k, w in want.items():
        assert R.rel_err(v[k], w) <= 1e-12, k
    assert R.row_err(v["dx"], y.grad) <= 1e-12 and R.row_err(v["dxd"], x.grad) <= 1e-11      # per row: dx is a cancelled difference


@pytest.mark.parametrize("c", R.EMB_CASES, ids=R.emb_id)
def test_closed_form_embedding_backward_equals_autograd(c):
    i = R.emb_case(c)
    wr, pr = i.word.double().requires_grad_(True), i.pos.double().requires_grad_(True)
    tr = i.typ.double().requires_grad_(True) if c.types else None
    gr, br = i.gamma.double().requires_grad_(True), i.beta.double().requires_grad_(True)
    e = R._emb_tables(wr, pr, tr, i.ids, i.tts, c.S).view(c.B * c.S, R.EMB_N)
    e.retain_grad()
    f = R.ln_fwd(e, gr, br, i.s_post)
    f["out"].backward(i.dout.double())
    # the closed form on the unrounded fp64 y and stats
    j = R.SimpleNamespace(**vars(i))
    j.y, j.stats = e.detach(), torch.stack([f["mean"], f["rstd"]], 1).detach()
    v = R.emb_bwd(c, j, R.F64)
    want = dict(drows=e.grad, dword=wr.grad, dpos=pr.grad, dgamma=gr.grad, dbeta=br.grad)
    if c.types:
        want["dtype_emb"] = tr.grad
    for k, w in want.items():
        assert R.rel_err(v[k], w) <= 1e-12, k
    # and the rounding of y and stats to fp32 moves the reference by far less than a gate
    for k, w in want.items():
        assert R.rel_err(i.ref[k], w) <= 1e-6, k


# ------------------------------------------------------------------------------------------------ 2. + 3. margins and sentinels
def _clear(ref, *names32, names16=()):
    for k in names32:
        assert R.clear_of_sentinel(ref[k], R.SENT32), k
    for k in names16:
        assert R.clear_of_sentinel(ref[k], R.SENT16), k


@pytest.mark.parametrize("c", R.LN_ATOMIC_CASES + R.LN_DET_CASES, ids=R.ln_id)
def test_layernorm_backward_margin(c):
    i = R.ln_case(c)
    _within_margin("ln_bwd %s" % R.ln_id(c), R.ln_eval32_errors(i, c.period), R.ln_eval32_errors(i, c.period, BF16))
    _clear(i.ref, "dx", "dxd", names16=("dxd",))
    if c.p_pre:
        assert bool((i.ref["dxd"][~torch.from_numpy(i.keep_pre)] == 0).all()) and float(i.ref["dx"].abs().min()) > 0


@pytest.mark.parametrize("T,K_out,ks,p_pre", R.FOLD_CASES)
def test_fold_layernorm_backward_margin(T, K_out, ks, p_pre):
    """The launch's da is not known here: the margin is taken on the fp64 product of the same bf16 operands, rounded to fp32, which the
    launch's da equals up to fp32 summation noise."""
    i = R.fold_case(T, K_out, ks, p_pre)
    ref = R.fold_ref(i, i.da64.float())
    _within_margin("fold T=%d K_out=%d ks=%d p_pre=%g" % (T, K_out, ks, p_pre), R.ln_eval32_errors(i, 0), R.ln_eval32_errors(i, 0, BF16))
    _clear(ref, "dx", names16=("dxd",))


@pytest.mark.parametrize("c", R.EMB_CASES, ids=R.emb_id)
def test_embedding_margin(c):
    i = R.emb_case(c)
    v = R.emb_fwd32(c, i)
    _within_margin("embed_fwd %s" % R.emb_id(c), R.fwd_eval32_errors(v, i.fwd_ref), R.fwd_eval32_errors(v, i.fwd_ref, BF16))
    _within_margin("embed_bwd %s" % R.emb_id(c), R.emb_eval32_errors(c, i))
    _clear(i.fwd_ref, "y", "out", names16=("out",))
    _clear(i.ref, "drows")
    assert float(i.stats.abs().max()) < 1000
    assert int(i.ids.min()) == 0 or c.B * c.S == 1 or c.ids == "same"
    assert int(i.ids.max()) == R.EMB_V - 1
    if c.types:
        assert sorted(set(i.tts.view(-1).tolist())) == list(range(c.types))


@pytest.mark.parametrize("rows,N", R.FWD_CASES)
def test_layernorm_forward_margin(rows, N):
    i = R.fwd_case(rows, N)
    v = R.ln_fwd(i.x.float(), i.gamma, i.beta)
    _within_margin("ln_fwd f64-in rows=%d N=%d" % (rows, N), R.fwd_eval32_errors(v, i.ref), R.fwd_eval32_errors(v, i.ref, BF16))
    _clear(i.ref, "y", "out", names16=("out",))
    assert torch.equal(i.ref["out"][R.FWD_ZERO_ROWS], i.beta.double().expand(len(R.FWD_ZERO_ROWS), N))
    assert torch.equal(v["out"][R.FWD_ZERO_ROWS], i.beta.expand(len(R.FWD_ZERO_ROWS), N))


@pytest.mark.parametrize("kind", R.ROWS_LISTS)
def test_rows_sumsq_margin(kind):
    i = R.rows_case(kind)
    n = int(i.meta[0])
    assert (kind == "overflow") == bool(i.meta[1]) and (kind == "empty") == (i.listed.numel() == 0)
    if kind == "twice":
        assert n > 256 + 5 and i.listed.numel() == n - 10
    if kind == "empty":
        assert i.ref == 0.0
        return
    got = R.added(i.base, (i.table[i.listed] ** 2).sum())
    e = R.sumsq_err(got, i.ref)
    _report("rows_sumsq %s" % kind, dict(sumsq=(e, R.GATE_SUMSQ)))
    assert e <= R.MARGIN * R.GATE_SUMSQ


# ------------------------------------------------------------------------------------------------ 4. the lists reach what they claim
def _ln_form(c, deterministic=False):
    """(waves, rows per wave) of univl_layernorm_bwd, restated from csrc/layernorm.hip."""
    if not deterministic and c.rows >= 3072 and c.N == 768 and not c.period:
        return 8, 3
    return 4, (1 if c.rows < 640 else 2 if c.rows < 1280 else 4)


def test_case_lists_cover_every_form_and_tail():
    forms = {}
    for c in R.LN_ATOMIC_CASES:
        w, rpw = _ln_form(c)
        forms.setdefault((w, rpw), set()).add(c.rows % (w * rpw))
    assert set(forms) == {(4, 1), (4, 2), (4, 4), (8, 3)}
    assert {1, 7, 0} <= forms[(4, 2)] and {1, 15, 0} <= forms[(4, 4)] and {1, 23, 0} <= forms[(8, 3)]
    for form in ((4, 2), (4, 4), (8, 3)):                 # dropout before and after, in every form that walks several rows
        cs = [c for c in R.LN_ATOMIC_CASES if _ln_form(c) == form]
        assert any(c.p_pre for c in cs) and any(c.p_post for c in cs)
    late = [c for c in R.LN_ATOMIC_CASES if c.rows >= 3072 and _ln_form(c)[0] == 4]
    assert any(c.N == 1024 for c in late) and {c.period for c in late if c.N == 768} == {48, 7}
    assert {_ln_form(c, True) for c in R.LN_DET_CASES} == {(4, 1), (4, 2), (4, 4)}
    # ln_dpos_gather_kernel: rows per position % 4 decides which of its tail terms run
    tails = set()
    for c in R.LN_DET_CASES:
        tails |= {len(range(s, c.rows, c.period)) % 4 for s in range(c.period)}
    assert tails == {0, 1, 2, 3}
    assert max(c.rows * c.N for c in R.LN_ATOMIC_CASES) == 3095 * 1024
    # embedding: 63 and 65 tokens leave three and one live waves in the last four-wave workgroup; B = 3 rows per position gives
    # univl_rows_gather_sum its third tail term
    assert {c.B * c.S % 4 for c in R.EMB_CASES} == {3, 1} and any(c.P == c.S for c in R.EMB_CASES)
    assert {c.types for c in R.EMB_CASES} == {0, 2, 3} and {c.ids for c in R.EMB_CASES} == {"mixed", "same", "distinct"}
