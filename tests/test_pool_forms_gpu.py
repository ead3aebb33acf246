"""The similarity pooling against fp64 in every launch form: univl_pool_fwd / _bwd / _pair_fwd / _pair_bwd (csrc/simloss.hip) at and
beside the 256-position chunk edges, under full, prefix, holed, empty and late-chunk-only masks, with and without skip_first and
normalize, storing and accumulating, with the upstream gradient from dout and from dsim / other.  Cases, inputs, references and error
measures: tests/pool_ref.py.  Needs a real MI355X (`-m gpu`).

Conventions of every case:
  * mean, out and dx have 8 guard rows and start as the sentinel 12345 everywhere: the guard rows keep their bits, no live element
    keeps the sentinel -- no reference value lies within 1 of it (tests/test_pool_ref_cpu.py);
  * an accumulating dx starts from a random base; got - base is compared;
  * masked positions of x hold +inf or NaN: the forward is unaffected, dx there is exactly 0 (store) or the base bit for bit
    (accumulate); with ldx_row = 1536 x is the left half of a buffer whose right half is NaN;
  * pooled rows of x and dout carry factors from 1e-2 to 1e2 and every error is the worst pooled row's max |error| over that row's
    max |reference|;
  * a text row without a count (S = 1 under skip_first, or nothing valid after position 0) is NaN in the reference: exactly those rows
    of `out` are non-finite, every other row passes its gate, and the backward of those rows is not compared.

Gates: 1e-5 forward and store-form backward, 1e-4 dx - base (tests/test_kernels_gpu.py's).  The same formulas in torch fp32 stay within
a quarter of each on these inputs (tests/test_pool_ref_cpu.py).  Every case prints observed error / fp32 error / gate (`pytest -s`);
profiles/pool_stream_forms.txt is that output."""
import pytest
import torch

import pool_ref as R

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from univl_amd import ops

DEV = "cuda"


def _dev(t):
    return None if t is None else t.to(DEV)


def _guarded(rows):
    return torch.full((rows + R.GUARD, R.N), R.SENT, device=DEV)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _check_guarded(case, bufs, rows):
    """The guard rows still hold the sentinel's bits; no live element does."""
    for k, b in bufs.items():
        assert torch.equal(_bits(b[rows:]), _bits(torch.full_like(b[rows:], R.SENT))), (case, k, "guard rows written")
        assert not bool((b[:rows] == R.SENT).any()), (case, k, "a live element was not written")


def _gate(case, errs):
    """errs: name -> (observed, fp32 evaluation, gate)."""
    print("pool-forms-gpu  %-58s %s" % (case, "  ".join("%s %.2e/%.2e/%.0e" % ((k,) + v) for k, v in errs.items())))
    for k, (e, _, g) in errs.items():
        assert e < g, (case, k, e, g)


def _fwd(side, form, ldx_row=R.N):
    """-> (args, kwargs) of ops.pool_fwd / ops.pool_desc on fresh output buffers, and those buffers."""
    got = dict(mean=_guarded(side.B), out=_guarded(side.B))
    x = _dev(side.x if ldx_row == R.N else R.widened(side.x, ldx_row))
    return (side.B, side.S, x, _dev(side.mask)), dict(skip_first=form[0], normalize=form[1], ldx_row=ldx_row, **got), got


def _check_fwd(case, side, ref, got):
    _check_guarded(case, got, side.B)
    mean, out = got["mean"][:side.B].cpu(), got["out"][:side.B].cpu()
    bad = ~torch.isfinite(out).all(-1)
    assert torch.equal(bad, ref.nan_rows), (case, "non-finite rows of out", bad.tolist(), ref.nan_rows.tolist())
    _gate(case, dict(mean=(R.row_err(mean, ref.mean, ref.ok), ref.e32["mean"], R.GATE_FWD),
                     out=(R.row_err(out, ref.out, ref.ok), ref.e32["out"], R.GATE_FWD)))


def _bwd(side, ref, form, accumulate, seed, extra=None):
    """-> (args, kwargs) of ops.pool_bwd / ops.pool_desc, the dx buffer with its guard rows, the base (None when storing).
    extra: the dsim form's arguments in place of dout."""
    rows = side.B * side.S
    dx = _guarded(rows)
    base = None
    if accumulate:
        base = R.acc_base(ref.dx, seed)
        dx[:rows] = _dev(base.view(rows, R.N))
    up = dict(dout=side.dout) if extra is None else extra
    kw = dict(skip_first=form[0], normalize=form[1], mean=_dev(ref.mean32), dx=dx, accumulate=accumulate)
    kw.update({k: _dev(v) if torch.is_tensor(v) else v for k, v in up.items()})
    return (side.B, side.S, _dev(side.x), _dev(side.mask)), kw, dx, base


def _check_bwd(case, side, ref, dx, base):
    rows = side.B * side.S
    _check_guarded(case, dict(dx=dx), rows)
    got = dx[:rows].cpu().view(side.B, side.S, R.N)
    masked = (ref.w == 0) & ref.ok[:, None]
    if base is None:
        assert bool((got[masked] == 0).all()), (case, "dx at a masked position is not exactly 0")
        _gate(case, dict(dx=(R.row_err(got, ref.dx, ref.ok), ref.e32["dx"], R.GATE_BWD)))
    else:
        assert torch.equal(_bits(got[masked]), _bits(base[masked])), (case, "dx at a masked position moved off the base")
        e32 = R.row_err(R.added(base, ref.dx32), ref.dx, ref.ok)
        _gate(case, dict(acc=(R.row_err(got.double() - base.double(), ref.dx, ref.ok), e32, R.GATE_ACC)))


# ------------------------------------------------------------------------------------------------ single launches, dout form
@pytest.mark.parametrize("form", R.FORMS, ids=R.form_id)
@pytest.mark.parametrize("c", R.POOL_CASES, ids=R.pool_id)
def test_pool_forms_against_fp64(c, form):
    side, ref = R.pool_case(c), R.pool_ref(c, form)
    name = "%s %s" % (R.pool_id(c), R.form_id(form))
    for ldx_row in (R.N, 2 * R.N):
        a, kw, got = _fwd(side, form, ldx_row)
        ops.pool_fwd(*a, **kw)
        torch.cuda.synchronize()
        _check_fwd("%s fwd ldx=%d" % (name, ldx_row), side, ref, got)
    for accumulate in (False, True):
        a, kw, dx, base = _bwd(side, ref, form, accumulate, seed=9)
        ops.pool_bwd(*a, **kw)
        torch.cuda.synchronize()
        _check_bwd("%s bwd %s" % (name, "acc" if accumulate else "store"), side, ref, dx, base)


# ------------------------------------------------------------------------------------------------ the dsim form
def _dsim_extra(dsim, other, n_other, transpose, gscale):
    return dict(dsim=dsim, other=other, n_other=n_other, transpose=transpose,
                gscale=None if gscale is None else torch.tensor([gscale], dtype=torch.float32))


@pytest.mark.parametrize("c", R.DSIM_CASES, ids=R.dsim_id)
def test_pool_bwd_dsim_form_against_fp64(c):
    """The upstream gradient from d loss / d sim: rectangular (B != n_other), ldsim > n_other with sentinel padding columns and
    sentinel rows that must not enter the sum, both transpose values, gscale absent and 0.5."""
    i = R.dsim_case(c)
    a, kw, dx, base = _bwd(i.side, i.ref, (i.skip_first, True), c.accumulate, seed=10,
                           extra=_dsim_extra(i.dsim, i.other, c.n_other, c.transpose, c.gscale))
    assert kw["dsim"].stride(0) > max(c.n_other, c.B)
    ops.pool_bwd(*a, **kw)
    torch.cuda.synchronize()
    _check_bwd("dsim %s" % R.dsim_id(c), i.side, i.ref, dx, base)


# ------------------------------------------------------------------------------------------------ pair launches
@pytest.mark.parametrize("shape", R.PAIR_SHAPES, ids=lambda s: "%dx%d" % s)
def test_pool_pair_launches_equal_single_launches_and_fp64(shape):
    """a.B = 3 (text), b.B = 5 (video), a.S != b.S: the grid of the backward is sized for the longer sequence and the blocks past the
    shorter one return.  Every output of a pair launch has the bits of the two single launches, guard rows included, and passes the
    fp64 gates."""
    i = R.pair_case(shape)
    name = "pair %dx%d" % shape
    fa, fb = (True, True), (False, True)
    # forward
    (aa, ka, ga), (ab, kb, gb) = _fwd(i.a, fa), _fwd(i.b, fb)
    ops.pool_pair_fwd(ops.pool_desc(*aa, **ka), ops.pool_desc(*ab, **kb))
    (sa, ska, sga), (sb, skb, sgb) = _fwd(i.a, fa), _fwd(i.b, fb)
    ops.pool_fwd(*sa, **ska)
    ops.pool_fwd(*sb, **skb)
    torch.cuda.synchronize()
    for k in ("mean", "out"):
        assert torch.equal(_bits(ga[k]), _bits(sga[k])) and torch.equal(_bits(gb[k]), _bits(sgb[k])), (name, k, "pair != single")
    _check_fwd(name + " a fwd", i.a, i.ra, ga)
    _check_fwd(name + " b fwd", i.b, i.rb, gb)
    # backward: the dout form storing, the dsim form accumulating (each side's `other` is the other side's fp32 out)
    for tag, accumulate, ra, rb, xa, xb in (
            ("dout store", False, i.ra, i.rb, None, None),
            ("dsim acc", True, i.rda, i.rdb, _dsim_extra(i.dsim, i.out_b, i.b.B, False, 0.5), _dsim_extra(i.dsim, i.out_a, i.a.B, True, 0.5))):
        (aa, ka, dxa, base_a), (ab, kb, dxb, base_b) = _bwd(i.a, ra, fa, accumulate, 11, xa), _bwd(i.b, rb, fb, accumulate, 12, xb)
        ops.pool_pair_bwd(ops.pool_desc(*aa, **ka), ops.pool_desc(*ab, **kb))
        (sa, ska, sxa, _), (sb, skb, sxb, _) = _bwd(i.a, ra, fa, accumulate, 11, xa), _bwd(i.b, rb, fb, accumulate, 12, xb)
        ops.pool_bwd(*sa, **ska)
        ops.pool_bwd(*sb, **skb)
        torch.cuda.synchronize()
        assert torch.equal(_bits(dxa), _bits(sxa)) and torch.equal(_bits(dxb), _bits(sxb)), (name, tag, "pair != single")
        _check_bwd("%s a bwd %s" % (name, tag), i.a, ra, dxa, base_a)
        _check_bwd("%s b bwd %s" % (name, tag), i.b, rb, dxb, base_b)
