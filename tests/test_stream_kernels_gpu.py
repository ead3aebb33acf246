"""The streaming helper kernels past their grid caps: univl_tanh_fwd / _tanh_bwd / _gelu_bwd / _scale_ct_by_device_scalar (2048
workgroups), univl_scale_by_device_scalar (1024), univl_gather_rows (64 workgroups per row) rely on a grid-stride loop beyond
cap = workgroups x 256 elements (x 16 bytes for the gather); the model runs them there, on millions of elements and on 147 KB frame rows.
Each is run at n in {1, 255, 257, cap - 1, cap, cap + 1, 2 cap + 77} with a sentinel guard after element n.  univl_rank_counts and
univl_pair_concat_fwd are exact and are run past their 256-thread stride, with ld > n, and at every remainder of rows modulo the four
rows of a workgroup.  Cases, inputs, references and measures: tests/pool_ref.py.  Needs a real MI355X (`-m gpu`).

Gates.  fp32 results: max(1e-6 for tanh, 1e-5 otherwise; 8 x the torch-fp32 error of the same formula on the same inputs against fp64),
the error taken absolutely against |dy| (|dg|) times the function's range, elementwise -- never relative to a derivative that crosses
zero.  bf16 results: within one bf16 step of the fp64 value rounded to bf16; the fp32 evaluation is within an eighth of half a step
on these inputs (tests/test_pool_ref_cpu.py), so a result further off is a defect.  Saturated tanh is exactly +-1 and its backward
exactly 0; the GELU derivative is exactly 1 in the upper tail (u >= 8) and vanishes against 1 in the lower (1 + du == 1), never NaN.
Every case prints observed error / fp32 error / gate (`pytest -s`); profiles/pool_stream_forms.txt is that output."""
import pytest
import torch

import pool_ref as R

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from univl_amd import ops

DEV = "cuda"
BF16 = torch.bfloat16
DTYPES = [torch.float32, BF16]
DTYPE_IDS = ["fp32", "bf16"]
GUARD_ELEMS = 64


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64 if t.dtype == torch.int64 else torch.int16)


def _guarded(n, dtype=torch.float32, start=None):
    """n live elements and GUARD_ELEMS guard elements, all the sentinel; `start`: the live elements' initial value."""
    buf = torch.full((n + GUARD_ELEMS,), R.SENT, device=DEV, dtype=dtype)
    if start is not None:
        buf[:n] = start.to(DEV)
    return buf


def _guard_intact(case, buf, n, written=True):
    assert torch.equal(_bits(buf[n:]), _bits(torch.full_like(buf[n:], R.SENT))), (case, "guard elements written")
    if written:
        assert not bool((buf[:n] == torch.full_like(buf[:1], R.SENT)).any()), (case, "a live element was not written")


def _name(dtype):
    return DTYPE_IDS[DTYPES.index(dtype)]


def _gate32(case, e, e32, floor):
    g = R.gate(floor, e32)
    print("stream-gpu  %-44s %.2e/%.2e/%.0e" % (case, e, e32, g))
    assert e < g, (case, e, e32, g)


def _gate16(case, got, ref64):
    steps = R.bf16_ulps(got, ref64)
    print("stream-gpu  %-44s %d bf16 step(s) from the rounded fp64 value / gate 1" % (case, steps))
    assert steps <= 1, (case, steps)


# ------------------------------------------------------------------------------------------------ grid-stride kernels
@pytest.mark.parametrize("n", R.stream_sizes(R.CAP_CROSS))
def test_tanh_fwd_past_the_grid_cap(n):
    x = R.tanh_input(n, seed=n)
    y = _guarded(n)
    ops.tanh_fwd(x.to(DEV), y[:n])
    torch.cuda.synchronize()
    case = "tanh_fwd n=%d" % n
    _guard_intact(case, y, n)
    got, ref = y[:n].cpu(), torch.tanh(x.double())
    _gate32(case, R.abs_err(got, ref), R.abs_err(torch.tanh(x), ref), R.FLOOR_TANH)
    sat = x.abs() >= R.TANH_SATURATED
    assert bool((got[sat] == torch.sign(x[sat])).all()), (case, "saturated tanh is not exactly +-1")


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("n", R.stream_sizes(R.CAP_CROSS))
def test_tanh_bwd_past_the_grid_cap(n, dtype):
    x = R.tanh_input(n, seed=n)
    y = torch.tanh(x.double()).float()
    dy = R.uniform(n, seed=n + 1).float()
    dx = _guarded(n, dtype)
    ops.tanh_bwd(dy.to(DEV), y.to(DEV), dx[:n])
    torch.cuda.synchronize()
    case = "tanh_bwd %s n=%d" % (_name(dtype), n)
    _guard_intact(case, dx, n)
    got, ref = dx[:n].cpu(), R.tanh_grad(dy.double(), y.double())
    if dtype == BF16:
        _gate16(case, got, ref)
    else:
        _gate32(case, R.abs_err(got, ref, dy.abs()), R.abs_err(R.tanh_grad(dy, y), ref, dy.abs()), R.FLOOR_TANH)
    sat = x.abs() >= R.TANH_SATURATED
    assert bool((got[sat] == 0).all()), (case, "the backward of saturated tanh is not exactly 0")


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("n", R.stream_sizes(R.CAP_CROSS))
def test_gelu_bwd_past_the_grid_cap(n, dtype):
    dg, u = R.gelu_input(n, n + 2, dtype)
    du = _guarded(n, dtype)
    ops.gelu_bwd(dg.to(DEV), u.to(DEV), du[:n])
    torch.cuda.synchronize()
    case = "gelu_bwd %s n=%d" % (_name(dtype), n)
    _guard_intact(case, du, n)
    got, ref = du[:n].cpu(), dg.double() * R.gelu_grad(u.double())
    assert bool(torch.isfinite(got.float()).all()), (case, "not finite")
    if dtype == BF16:
        _gate16(case, got, ref)
    else:
        scale = dg.abs() * R.GELU_GRAD_RANGE
        _gate32(case, R.abs_err(got, ref, scale), R.abs_err(dg * R.gelu_grad(u), ref, scale), R.FLOOR)
    at = R.grid_positions(n, len(R.GELU_GRID))                       # dg == 1 there
    up, lo = at & (u.float() >= R.GELU_TAIL), at & (u.float() <= -R.GELU_TAIL)
    assert bool((got.float()[up] == 1).all()), (case, "the derivative in the upper tail is not exactly 1")
    assert bool(((1 + got.float()[lo]) == 1).all()), (case, "the derivative in the lower tail does not vanish")


@pytest.mark.parametrize("s", [1.0, 0.0, -0.25], ids=lambda s: "s%g" % s)
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("n", R.stream_sizes(R.CAP_CROSS))
def test_scale_ct_past_the_grid_cap(n, dtype, s):
    x = R.uniform(n, seed=n + 3).to(dtype)
    buf = _guarded(n, dtype, start=x)
    ops.scale_ct(buf[:n], torch.tensor([s], device=DEV))
    torch.cuda.synchronize()
    case = "scale_ct %s s=%g n=%d" % (_name(dtype), s, n)
    _guard_intact(case, buf, n, written=False)
    got, ref = buf[:n].cpu(), x.double() * s
    if s == 1.0:
        assert torch.equal(_bits(got), _bits(x)), (case, "s == 1 moved a bit")
    elif s == 0.0:
        assert bool((got == 0).all()), (case, "s == 0 left a value")
    elif dtype == BF16:
        _gate16(case, got, ref)
    else:
        _gate32(case, R.rel_err(got, ref), R.rel_err(x * s, ref), R.FLOOR)


@pytest.mark.parametrize("n", R.stream_sizes(R.CAP_SIMLOSS))
def test_scale_by_device_scalar_past_the_grid_cap(n):
    x = R.uniform(n, seed=n + 4).float()
    s = torch.tensor([-0.37])
    buf = _guarded(n, start=x)
    ops.scale_by_device_scalar(buf[:n], s.to(DEV))
    torch.cuda.synchronize()
    case = "scale_by_device_scalar n=%d" % n
    _guard_intact(case, buf, n, written=False)
    ref = x.double() * s.double()
    _gate32(case, R.rel_err(buf[:n].cpu(), ref), R.rel_err(x * s, ref), R.FLOOR)


# ------------------------------------------------------------------------------------------------ gather_rows
GATHER_CASES = [(k, cb, tail) for k, cb in enumerate(R.GATHER_BYTES) for tail in (False, True) if cb or tail]


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("k,copy_bytes,tail", GATHER_CASES, ids=lambda v: str(v))
def test_gather_rows_past_the_grid_cap(k, copy_bytes, tail, dtype):
    """Bit-exact; 1 to 5 destination rows from repeated, out-of-order source rows; copy_bytes == row_stride, and copy_bytes <
    row_stride where the tail of every destination row keeps its bits."""
    rows = (5, 1, 2, 3, 4, 5)[k]
    esize = 4 if dtype == torch.float32 else 2
    stride = copy_bytes + (R.GATHER_TAIL if tail else 0)
    cols, live = stride // esize, copy_bytes // esize
    src = torch.randn(R.GATHER_SRC_ROWS, cols, generator=torch.Generator().manual_seed(k)).to(dtype)
    dst = torch.full((rows + 1, cols), R.SENT, device=DEV, dtype=dtype)
    idx = torch.tensor(R.GATHER_IDX[:rows], dtype=torch.int32)
    assert int(idx.max()) < R.GATHER_SRC_ROWS and stride % 16 == 0 and copy_bytes % 16 == 0
    ops.gather_rows(src.to(DEV), dst, idx.to(DEV), rows, stride, copy_bytes)
    torch.cuda.synchronize()
    case = "gather_rows %s rows=%d copy=%d stride=%d" % (_name(dtype), rows, copy_bytes, stride)
    got = dst.cpu()
    assert torch.equal(_bits(got[:rows, :live]), _bits(src[idx.long(), :live])), (case, "copied bytes differ")
    want_rest = torch.full((rows + 1, cols), R.SENT, dtype=dtype)
    assert torch.equal(_bits(got[:rows, live:]), _bits(want_rest[:rows, live:])), (case, "the tail of a destination row was written")
    assert torch.equal(_bits(got[rows:]), _bits(want_rest[rows:])), (case, "the guard row was written")
    print("stream-gpu  %-44s exact" % case)


# ------------------------------------------------------------------------------------------------ rank_counts
@pytest.mark.parametrize("pad", [0, R.RANK_PAD])
@pytest.mark.parametrize("n", R.RANK_SIZES)
def test_rank_counts_past_one_stride(n, pad):
    buf = R.rank_input(n, n + pad, seed=n)
    gt, eq = ops.rank_counts(buf.to(DEV)[:, :n])
    torch.cuda.synchronize()
    want_gt, want_eq = R.rank_counts_ref(buf, n)
    case = "rank_counts n=%d ld=%d" % (n, n + pad)
    assert torch.equal(gt.cpu(), want_gt) and torch.equal(eq.cpu(), want_eq), case
    print("stream-gpu  %-44s exact" % case)


# ------------------------------------------------------------------------------------------------ pair_concat_fwd
@pytest.mark.parametrize("form", ["arange", "repeated"])
@pytest.mark.parametrize("P,W,F", R.CONCAT_SHAPES)
def test_pair_concat_fwd_every_row_remainder(P, W, F, form):
    i = R.concat_input(P, W, F, form, seed=P)
    rows = P * (W + F)
    out = torch.full((rows + R.GUARD, R.N), R.SENT, device=DEV)
    om = torch.full((rows + R.GUARD,), R.CONCAT_MASK_SENT, dtype=torch.int64, device=DEV)
    ops.pair_concat_fwd(i.seq.to(DEV), i.vis.to(DEV), i.am.to(DEV), i.vm.to(DEV), i.tidx.to(DEV), i.vidx.to(DEV), P, W, F, out, om)
    torch.cuda.synchronize()
    ref, refm = R.concat_ref(i)
    case = "pair_concat_fwd P=%d W=%d F=%d %s (rows %% 4 = %d)" % (P, W, F, form, rows % 4)
    assert torch.equal(_bits(out[:rows].cpu()), _bits(ref.reshape(rows, R.N))), (case, "rows differ")
    assert torch.equal(om[:rows].cpu(), refm.reshape(rows)), (case, "mask differs")
    assert torch.equal(_bits(out[rows:].cpu()), _bits(torch.full((R.GUARD, R.N), R.SENT))), (case, "guard rows of out written")
    assert bool((om[rows:] == R.CONCAT_MASK_SENT).all()), (case, "guard elements of the mask written")
    print("stream-gpu  %-44s exact" % case)
