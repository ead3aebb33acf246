"""The references and gates of tests/test_pool_forms_gpu.py and tests/test_stream_kernels_gpu.py, checked without a GPU
(tests/pool_ref.py).

1. The closed-form fp64 pooling, forward and backward, against oracle.univl_oracle.mean_pooling_for_similarity + F.normalize under fp64
   autograd, to 1e-12, on every pooling case of the GPU file: each (S, mask set) in each (skip_first, normalize) form, the dsim form
   (the upstream gradient through autograd of sum(dsim * out @ other^T) * gscale) and both sides of the pair cases.
2. Margin: the same formulas evaluated in torch fp32 on the same inputs, measured the way the GPU test measures the kernels, stay
   within a quarter of every gate (1e-5 forward and store-form backward, 1e-4 dx - base).  `pytest -s` prints the figures.
3. No reference value lies within 1 of the sentinel.
4. The streaming formulas: torch fp32 against fp64 on the GPU file's inputs is far below half a bf16 step (the condition of the
   one-step bf16 check), the references saturate exactly where the GPU file asserts exact values.
5. The case lists reach what they claim."""
import pytest
import torch
import torch.nn.functional as F

import pool_ref as R
import univl_oracle as O


def _report(case, errs):
    print("pool-forms-cpu  %-52s %s" % (case, "  ".join("%s %.2e/%.0e" % (k, e, g) for k, (e, g) in errs.items())))


def _within_margin(case, errs):
    _report(case, errs)
    for k, (e, g) in errs.items():
        assert e <= R.MARGIN * g, (case, k, e, g)


def _autograd(side, skip_first, normalize, upstream=None):
    """The oracle's pooling of the side under fp64 autograd.  upstream(out) -> scalar loss, default sum(out * dout)."""
    x = torch.nan_to_num(side.x, nan=0.0, posinf=0.0).double().requires_grad_(True)
    t, v = O.mean_pooling_for_similarity(x, x, side.mask, side.mask)
    mean = t if skip_first else v
    out = F.normalize(mean, dim=-1) if normalize else mean
    ok = torch.isfinite(out).all(-1)               # rows whose count is 0 are NaN on both sides: they take no part in the loss
    live = torch.where(ok[:, None], out, torch.zeros_like(out))
    loss = (live * side.dout.double()).sum() if upstream is None else upstream(live)
    loss.backward()
    return mean.detach(), out.detach(), x.grad, ok


def _closed_form_equals_autograd(case, side, skip_first, normalize, g64=None, upstream=None):
    w = R.weights(side.mask, skip_first, R.F64)
    mean, out, cnt = R.pool_forward(side.x.double(), w, skip_first, normalize)
    dx = R.pool_backward(mean, side.dout.double() if g64 is None else g64, w, cnt, normalize)
    a_mean, a_out, a_dx, ok = _autograd(side, skip_first, normalize, upstream)
    assert torch.equal(ok, cnt != 0), (case, "the rows without a count differ")
    assert bool(torch.isnan(out[~ok]).all()) and bool(torch.isnan(a_out[~ok]).all())
    errs = dict(mean=R.row_err(mean, a_mean, ok), out=R.row_err(out, a_out, ok), dx=R.row_err(dx, a_dx, ok))
    _report(case + " vs autograd", {k: (e, 1e-12) for k, e in errs.items()})
    assert max(errs.values()) <= 1e-12, (case, errs)
    masked = (w == 0) & ok[:, None]
    assert bool((dx[masked] == 0).all()) and bool((a_dx[masked] == 0).all())


def _margins(case, side, ref, seed):
    """ref: pool_ref.side_ref's result.  The accumulate form's margin: the fp32 evaluation's dx added to the base in fp32."""
    ok = ref.ok
    base = R.acc_base(ref.dx, seed)
    acc = R.row_err(R.added(base, ref.dx32), ref.dx, ok)
    _within_margin(case, dict(mean=(ref.e32["mean"], R.GATE_FWD), out=(ref.e32["out"], R.GATE_FWD), dx=(ref.e32["dx"], R.GATE_BWD),
                              acc=(acc, R.GATE_ACC)))
    for k in ("mean", "out", "dx"):
        assert R.clear_of_sentinel(getattr(ref, k)), (case, k, "a reference value lies within 1 of the sentinel")
    assert R.clear_of_sentinel(base.double() + torch.nan_to_num(ref.dx)), (case, "base + dx lies within 1 of the sentinel")


# ------------------------------------------------------------------------------------------------ 1. - 3. pooling
@pytest.mark.parametrize("form", R.FORMS, ids=R.form_id)
@pytest.mark.parametrize("c", R.POOL_CASES, ids=R.pool_id)
def test_pool_closed_form_and_margin(c, form):
    side, ref = R.pool_case(c), R.pool_ref(c, form)
    case = "%s %s" % (R.pool_id(c), R.form_id(form))
    _closed_form_equals_autograd(case, side, *form)
    _margins(case, side, ref, seed=9)
    # the only rows without a count: S == 1 under skip_first, and the row without a valid frame under skip_first
    want = torch.tensor([form[0] and (c.S == 1 or k == "empty") for k in side.kinds])
    assert torch.equal(ref.nan_rows, want)


@pytest.mark.parametrize("c", R.DSIM_CASES, ids=R.dsim_id)
def test_dsim_form_closed_form_and_margin(c):
    i = R.dsim_case(c)
    r, k = (c.n_other, c.B) if c.transpose else (c.B, c.n_other)
    live = torch.zeros_like(i.dsim, dtype=torch.bool)
    live[:r, :k] = True
    assert bool((i.dsim[~live] == R.SENT).all()) and i.dsim.stride(0) > k and not bool((i.dsim[live].abs() > 1).any())
    view = (i.dsim[:r, :k].t() if c.transpose else i.dsim[:r, :k]).double()
    gs = 1.0 if c.gscale is None else c.gscale
    g64 = R.upstream(i.dsim.double(), i.other.double(), c.B, c.n_other, c.transpose, c.gscale)
    _closed_form_equals_autograd(R.dsim_id(c), i.side, i.skip_first, True, g64=g64,
                                 upstream=lambda out: ((out @ i.other.double().t()) * view).sum() * gs)
    _margins(R.dsim_id(c), i.side, i.ref, seed=10)
    assert not bool(i.ref.nan_rows.any())


@pytest.mark.parametrize("shape", R.PAIR_SHAPES, ids=lambda s: "%dx%d" % s)
def test_pair_cases_closed_form_and_margin(shape):
    i = R.pair_case(shape)
    assert (i.a.B, i.b.B) == (R.PAIR_BA, R.PAIR_BB) and i.a.B != i.b.B and (i.a.S, i.b.S) == shape
    for name, side, sf, ref, rd in (("a", i.a, True, i.ra, i.rda), ("b", i.b, False, i.rb, i.rdb)):
        case = "pair %dx%d %s" % (shape + (name,))
        _closed_form_equals_autograd(case, side, sf, True)
        _margins(case, side, ref, seed=11)
        _margins(case + " dsim", side, rd, seed=12)
        assert not bool(ref.nan_rows.any())
    assert bool((i.rb.out[3] == 0).all()) and bool((i.rb.dx[3] == 0).all())          # the video row without a valid frame


# ------------------------------------------------------------------------------------------------ 4. streaming formulas
@pytest.mark.parametrize("n", R.stream_sizes(R.CAP_CROSS))
def test_stream_formulas_fp32_margin_under_bf16(n):
    """Half a bf16 step is 2 ** -9 of the value's binade; the torch-fp32 evaluation of each formula stays within an eighth of it, so
    a kernel result more than one bf16 step from the rounded fp64 value is not explained by fp32 arithmetic."""
    x = R.tanh_input(n, seed=n)
    y = torch.tanh(x.double()).float()
    sat = x.abs() >= R.TANH_SATURATED
    assert bool((y[sat] == torch.sign(x[sat])).all()) and bool((R.tanh_grad(torch.ones_like(y), y)[sat] == 0).all())
    assert bool((y[~sat].abs() < 1).all())
    dy = R.uniform(n, seed=n + 1).float()
    s_t = R.bf16_half_ulp_share(R.tanh_grad(dy, y), R.tanh_grad(dy.double(), y.double()))
    dg, u = R.gelu_input(n, n + 2, R.BF16)
    ref = dg.double() * R.gelu_grad(u.double())
    s_g = R.bf16_half_ulp_share(dg * R.gelu_grad(u.float()), ref)
    z = R.uniform(n, seed=n + 3).to(R.BF16)
    s_s = R.bf16_half_ulp_share(z.float() * -0.37, z.double() * -0.37)
    print("stream-cpu  n=%-8d fp32 error / half a bf16 step: tanh_bwd %.2e  gelu_bwd %.2e  scale %.2e" % (n, s_t, s_g, s_s))
    assert max(s_t, s_g, s_s) <= 0.125
    at = R.grid_positions(n, len(R.GELU_GRID))
    up, lo = at & (u.float() >= R.GELU_TAIL), at & (u.float() <= -R.GELU_TAIL)
    r32 = ref.float()
    assert bool((r32[up] == 1).all()) and bool(((1 + r32[lo]) == 1).all()) and bool(torch.isfinite(ref).all())
    if n >= 2 * len(R.GELU_GRID):
        assert int(up.sum()) > 0 and int(lo.sum()) > 0 and float(u.float().abs().max()) == 10.0 and float(x.abs().max()) == 100.0


# ------------------------------------------------------------------------------------------------ 5. the lists reach what they claim
def test_case_lists_reach_the_edges():
    assert {S % R.PCHUNK for S in R.S_LIST if S > R.PCHUNK} >= {0, 1, 7} and {255, 256, 257, 512, 513} <= set(R.S_LIST)
    tails = {min(R.PCHUNK, S - (S - 1) // R.PCHUNK * R.PCHUNK) % 8 for S in R.S_LIST}           # last chunk's length mod 8
    assert {1, 7, 0} <= tails
    for c in R.POOL_CASES:
        i = R.pool_case(c)
        assert 3 <= i.B <= 5
        masked = i.mask == 0
        assert not bool(torch.isfinite(i.x[masked]).any())
        if c.S > 1:
            assert bool(torch.isinf(i.x[masked]).any()) and bool(torch.isnan(i.x[masked]).any())
        assert bool(torch.isfinite(i.x[~masked]).all())
        if c.kind == "basic":
            assert bool((i.mask[0] == 1).all()) and int(i.mask[3].sum()) == 0
            if c.S > 2:
                holes = i.mask[2]
                assert int(holes.sum()) < c.S and int(holes[-1]) == 1
        else:
            lo = (c.S - 1) // R.PCHUNK * R.PCHUNK
            assert int(i.mask[0, :lo].sum()) == 0 and int(i.mask[0, lo:].sum()) > 0              # valid in the last chunk only
            assert i.mask[1].nonzero().view(-1).tolist() == [R.PCHUNK]                           # position 0 of chunk 1 only
        if c.S > R.PCHUNK and c.kind == "basic":                                                 # poison in every chunk
            for lo in range(0, c.S, R.PCHUNK):
                assert bool(masked[:, lo:lo + R.PCHUNK].any())
    f = torch.cat([R.row_factors(4, 1), R.row_factors(3, 2)])
    assert float(f.min()) == pytest.approx(1e-2) and float(f.max()) == pytest.approx(1e2)
    assert {(c.B, c.n_other) for c in R.DSIM_CASES} == {(3, 5), (5, 3)} and {c.gscale for c in R.DSIM_CASES} == {None, 0.5}
    assert R.stream_sizes(R.CAP_CROSS)[3:] == [524287, 524288, 524289, 1048653] and R.CAP_SIMLOSS == 262144
    assert R.GATHER_BYTES == [0, 16, 262128, 262144, 262160, 600000] and all(b % 16 == 0 for b in R.GATHER_BYTES)
    assert sorted({P * (W + F) % 4 for P, W, F in R.CONCAT_SHAPES}) == [1, 2, 3]


@pytest.mark.parametrize("n", R.RANK_SIZES)
def test_rank_input_plants_what_it_claims(n):
    buf = R.rank_input(n, n + R.RANK_PAD, seed=n)
    x, d = buf[:, :n], buf[:, :n].diag()
    gt, eq = R.rank_counts_ref(buf, n)
    wide_gt, wide_eq = (buf > d[:, None]).sum(1), (buf == d[:, None]).sum(1)
    assert bool((wide_eq > eq).all()) and (n < 5 or bool((wide_gt > gt).any()))      # a loop to ld would count the padding
    assert torch.equal(R.rank_input(n, n, seed=n), x.contiguous())
    for col in (0, 255, 256, n - 1):
        if col < n and n > 1:
            assert int((x[:, col] == d).sum()) > 1
    if n > 4:
        assert float(d[n - 2]) == float("inf") and int(gt[n - 2]) == 0 and int(eq[n - 2]) > 1
        assert float(d[3]) == float("-inf") and int(gt[3]) >= n - 2
