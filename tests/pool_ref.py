"""Cases, input builders, fp64 references, error measures and gates for the similarity pooling (csrc/simloss.hip: univl_pool_fwd / _bwd /
_pair_fwd / _pair_bwd) and for the streaming helper kernels (csrc/cross.hip, csrc/simloss.hip: tanh, GELU backward, the device-scalar
scalings, univl_gather_rows, univl_rank_counts, univl_pair_concat_fwd).

tests/test_pool_forms_gpu.py and tests/test_stream_kernels_gpu.py run the kernels on the inputs built here; tests/test_pool_ref_cpu.py
checks the closed forms against fp64 autograd of the oracle and requires the same formulas, evaluated in torch fp32 on the same inputs,
to sit within a quarter of every gate.

Pooling, in closed form (every formula works in the dtype of its operands: fp64 is the reference, fp32 the margin evaluation):

    w[b, s] = mask[b, s], 0 at s == 0 with skip_first          cnt[b] = sum_s w[b, s], a video count of 0 replaced by 1
    mean[b] = sum_s (w != 0 ? x[b, s] w : 0) / cnt[b]          out[b] = mean[b] / max(|mean[b]|, 1e-12)  (normalize), else mean[b]
    g = dout,  or  gscale * dsim[b, :n_other] @ other  (dsim[:n_other, b] with transpose)
    gm = (g - mean (mean . g) / nrm^2) / nrm,  nrm = max(|mean|, 1e-12)  (normalize), else g          dx[b, s] = gm[b] w[b, s] / cnt[b]

The backward reference is computed from what the kernel reads -- the fp32 `mean` -- so that a forward error can neither mask nor mimic
a backward one.  A text row whose count is 0 (S == 1 with skip_first, or nothing valid after position 0) is 0 / 0 = NaN in the reference
model and here; such rows are listed in `nan_rows`, must be the only non-finite rows of `out`, and their backward is not compared.

Inputs.  Pooled row b of x and of dout carries a factor between 1e-2 and 1e2; errors are measured per pooled row against that row's own
maximum (`row_err`), so a large row cannot hide a small one.  Masked positions of x hold +inf (even s) or NaN (odd s).  The base of an
accumulating dx is drawn per pooled row at the magnitude of that row's reference increment, as the gradients that meet in such a buffer
are; `got - base` is compared.

A plain module (no fixtures): tests import it as `pool_ref`."""
import functools
import math
from collections import namedtuple
from types import SimpleNamespace

import torch

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
N = 768
PCHUNK = 256                                     # csrc/simloss.hip: sequence positions per staged chunk / per backward workgroup
SENT, GUARD = 12345.0, 8
GATE_FWD, GATE_BWD, GATE_ACC = 1e-5, 1e-5, 1e-4  # tests/test_kernels_gpu.py: forward, store-form backward, dx - base
MARGIN = 0.25                                    # the fp32 evaluation must sit within this share of a gate
EPS = 1e-12

S_LIST = [1, 2, 7, 8, 9, 15, 255, 256, 257, 263, 512, 513]
PoolCase = namedtuple("PoolCase", "S kind")
KINDS = {"basic": ("full", "prefix", "holes", "empty"),                  # B = 4
         "late": ("last", "chunk1", "prefix_late")}                      # B = 3, S > PCHUNK only
POOL_CASES = [PoolCase(S, "basic") for S in S_LIST] + [PoolCase(S, "late") for S in S_LIST if S > PCHUNK]
FORMS = [(sf, nz) for sf in (True, False) for nz in (True, False)]       # (skip_first, normalize)

DsimCase = namedtuple("DsimCase", "B n_other transpose gscale accumulate")
DSIM_S = 263                                     # three chunks, the last of 7 positions
DSIM_LD_PAD = 3                                  # ldsim = max(B, n_other) + 3
DSIM_CASES = [DsimCase(B, n, tr, gs, acc) for B, n in ((3, 5), (5, 3)) for tr in (False, True) for gs in (None, 0.5)
              for acc in (False, True)]

PAIR_SHAPES = [(300, 12), (12, 300), (257, 256), (48, 48)]               # (a.S, b.S); a: text, B = 3; b: video, B = 5
PAIR_BA, PAIR_BB = 3, 5


def pool_id(c):
    return "S%d-%s" % (c.S, c.kind)


def form_id(f):
    return ("skip" if f[0] else "all") + ("-norm" if f[1] else "-mean")


def dsim_id(c):
    return "B%d-other%d-%s-gscale%s-%s" % (c.B, c.n_other, "T" if c.transpose else "N", c.gscale, "acc" if c.accumulate else "store")


# ------------------------------------------------------------------------------------------------ error measures and gates
def row_err(got, ref, rows=None):
    """Worst row of: max |got - ref| over the row / max |ref| over the row.  A row whose reference is all zero must be all zero.
    rows: bool [B], the rows that are compared."""
    got, ref = got.detach().double().cpu().reshape(ref.shape[0], -1), ref.detach().double().cpu().reshape(ref.shape[0], -1)
    if rows is not None:
        got, ref = got[rows], ref[rows]
    if ref.shape[0] == 0:
        return 0.0
    d, m = (got - ref).abs().max(1).values, ref.abs().max(1).values
    d = torch.nan_to_num(d, nan=float("inf"))
    e = torch.where(m > 0, d / m.clamp_min(1e-300), torch.where(d > 0, torch.full_like(d, float("inf")), torch.zeros_like(d)))
    return float(e.max())


def clear_of_sentinel(ref, sent=SENT):
    """No reference value within 1 of the sentinel."""
    return not bool(((ref > sent - 1) & (ref < sent + 1)).any())


def gate(floor, e32):
    """tests/head_ref.py's rule: the floor the project already asks, or 8 x the torch-fp32 error of the same formula on the same inputs."""
    return max(floor, 8 * e32)


# ------------------------------------------------------------------------------------------------ pooling: inputs
def uniform(*shape, seed):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed), dtype=F64) * 2 - 1


def row_factors(rows, seed):
    u = torch.linspace(-2, 2, rows, dtype=F64) if rows > 1 else torch.zeros(1, dtype=F64)
    return 10.0 ** u[torch.randperm(rows, generator=torch.Generator().manual_seed(seed))]


def mask_row(kind, S, g):
    """One row of a key mask.  Every kind but `empty` keeps a valid position after position 0 when S > 1 (a text row pools it)."""
    s = torch.arange(S)
    if kind == "full":
        return torch.ones(S, dtype=torch.int64)
    if kind == "empty":
        return torch.zeros(S, dtype=torch.int64)
    if kind == "prefix":                          # 2 .. S - 1 valid positions (S from 3)
        k = S if S < 3 else int(torch.randint(2, S, (1,), generator=g))
        return (s < k).long()
    if kind == "prefix_late":                     # ends inside the last chunk
        lo = (S - 1) // PCHUNK * PCHUNK
        k = min(S, lo + 1 + int(torch.randint(0, S - lo, (1,), generator=g)))
        return (s < k).long()
    if kind == "holes":                           # position 0 masked (S from 2), the last position valid
        m = (torch.rand(S, generator=g) < 0.5).long()
        if S > 1:
            m[0] = 0
        m[S - 1] = 1
        return m
    if kind == "last":                            # valid in the last chunk only, with holes there
        lo = (S - 1) // PCHUNK * PCHUNK
        m = ((torch.rand(S, generator=g) < 0.5) & (s >= lo)).long()
        m[S - 1] = 1
        return m
    if kind == "chunk1":                          # valid at position 0 of chunk 1 only
        return (s == PCHUNK).long()
    raise ValueError(kind)


def make_side(kinds, S, seed):
    """One pooling input: mask [B, S] int64, x [B, S, 768] fp32 with its masked positions poisoned, dout [B, 768] fp32."""
    B = len(kinds)
    g = torch.Generator().manual_seed(seed)
    mask = torch.stack([mask_row(k, S, g) for k in kinds])
    x = (row_factors(B, seed + 1)[:, None, None] * uniform(B, S, N, seed=seed + 2)).float()
    s = torch.arange(S)
    x[(mask == 0) & (s % 2 == 0)[None]] = float("inf")
    x[(mask == 0) & (s % 2 == 1)[None]] = float("nan")
    dout = (row_factors(B, seed + 3)[:, None] * uniform(B, N, seed=seed + 4)).float()
    return SimpleNamespace(B=B, S=S, kinds=tuple(kinds), mask=mask, x=x, dout=dout)


@functools.lru_cache(maxsize=None)
def pool_case(c):
    return make_side(KINDS[c.kind], c.S, 1000 + 7 * c.S + (0 if c.kind == "basic" else 3))


def widened(x, ldx_row):
    """x as the left part of a [B, S, ldx_row] buffer whose remaining columns hold NaN."""
    wide = torch.full(x.shape[:2] + (ldx_row,), float("nan"), dtype=x.dtype)
    wide[..., :N] = x
    return wide


# ------------------------------------------------------------------------------------------------ pooling: the formulas
def weights(mask, skip_first, dtype):
    w = mask.to(dtype).clone()
    if skip_first:
        w[:, 0] = 0
    return w


def counts(w, skip_first):
    cnt = w.sum(1)
    return cnt if skip_first else torch.where(cnt == 0, torch.ones_like(cnt), cnt)


def pool_forward(x, w, skip_first, normalize):
    """-> (mean, out, cnt).  x may hold anything where w == 0."""
    cnt = counts(w, skip_first)
    wx = torch.where(w[..., None] != 0, x * w[..., None], torch.zeros((), dtype=x.dtype))
    mean = wx.sum(1) / cnt[:, None]
    out = mean / mean.norm(dim=-1, keepdim=True).clamp_min(EPS) if normalize else mean
    return mean, out, cnt


def pool_backward(mean, g, w, cnt, normalize):
    """-> dx [B, S, 768] from the pooled mean and the upstream gradient g of `out`."""
    if normalize:
        nrm = mean.norm(dim=-1, keepdim=True).clamp_min(EPS)
        g = (g - mean * ((mean * g).sum(-1, keepdim=True) / (nrm * nrm))) / nrm
    return g[:, None, :] * (w / cnt[:, None])[..., None]


def upstream(dsim, other, B, n_other, transpose, gscale):
    """The dsim form's upstream gradient [B, 768]: gscale * dsim[b, :n_other] @ other, or dsim[:n_other, b] with transpose."""
    view = dsim[:n_other, :B].t() if transpose else dsim[:B, :n_other]
    g = view.to(other.dtype) @ other[:n_other]
    return g if gscale is None else g * gscale


def side_ref(side, skip_first, normalize, g=None):
    """The fp64 reference of one pooling input and the fp32 evaluation of the same formulas.  g: the upstream gradient in fp64 and in
    fp32 (default: dout).  -> mean, out, dx (fp64; dx from the fp32-rounded mean), mean32 (what the backward kernel is given),
    nan_rows (bool [B]), ok (= ~nan_rows), w, cnt, dx32 and g32 (the fp32 evaluation's backward and its upstream gradient),
    e32 = dict(mean, out, dx): the fp32 evaluation's row errors."""
    g64, g32 = (side.dout.double(), side.dout) if g is None else g
    w64, w32 = weights(side.mask, skip_first, F64), weights(side.mask, skip_first, F32)
    mean, out, cnt = pool_forward(side.x.double(), w64, skip_first, normalize)
    nan_rows = cnt == 0
    ok = ~nan_rows
    mean32 = mean.float()
    dx = pool_backward(mean32.double(), g64, w64, cnt, normalize)
    m32, o32, c32 = pool_forward(side.x, w32, skip_first, normalize)
    d32 = pool_backward(mean32, g32, w32, c32, normalize)
    e32 = dict(mean=row_err(m32, mean, ok), out=row_err(o32, out, ok), dx=row_err(d32, dx, ok))
    return SimpleNamespace(mean=mean, out=out, cnt=cnt, dx=dx, mean32=mean32, nan_rows=nan_rows, ok=ok, e32=e32, w=w64, dx32=d32, g32=g32)


@functools.lru_cache(maxsize=None)
def pool_ref(c, form):
    return side_ref(pool_case(c), *form)


def acc_base(dx_ref, seed):
    """The fp32 base of an accumulating dx: uniform on (-1, 1) times the pooled row's largest reference increment (1 where that is 0
    or not finite)."""
    B = dx_ref.shape[0]
    m = torch.nan_to_num(dx_ref.reshape(B, -1).abs().max(1).values, nan=0.0, posinf=0.0)
    m = torch.where(m > 0, m, torch.ones_like(m))
    return (m[:, None, None] * uniform(*dx_ref.shape, seed=seed)).float()


def added(base, inc):
    """An accumulating output as the test sees it, `got - base`, when `inc` is added to the fp32 `base` in inc's dtype."""
    return (base.to(inc.dtype) + inc).double() - base.double()


# ------------------------------------------------------------------------------------------------ pooling: dsim form and pair launches
@functools.lru_cache(maxsize=None)
def dsim_case(c):
    """The pooled side (B rows of S = 263), the other side's [n_other, 768] matrix, and a dsim buffer of max(B, n_other) rows and
    ldsim = max(B, n_other) + 3 columns: the live block is [B, n_other] ([n_other, B] with transpose), everything else a sentinel."""
    kinds = ("last", "holes", "prefix_late", "prefix", "full")[:c.B]
    side = make_side(kinds, DSIM_S, 2000 + 10 * c.B + c.transpose)
    other = (row_factors(c.n_other, 31)[:, None] * uniform(c.n_other, N, seed=32)).float()
    m = max(c.B, c.n_other)
    dsim = torch.full((m, m + DSIM_LD_PAD), SENT)
    r, k = (c.n_other, c.B) if c.transpose else (c.B, c.n_other)
    dsim[:r, :k] = uniform(r, k, seed=33).float()
    skip_first = not c.transpose                   # the text side reads rows of dsim, the video side columns (csrc: UnivlPool.dsim)
    gs64 = None if c.gscale is None else float(c.gscale)
    g64 = upstream(dsim.double(), other.double(), c.B, c.n_other, c.transpose, gs64)
    g32 = upstream(dsim, other, c.B, c.n_other, c.transpose, gs64)
    ref = side_ref(side, skip_first, True, g=(g64, g32))
    return SimpleNamespace(side=side, other=other, dsim=dsim, skip_first=skip_first, ref=ref)


@functools.lru_cache(maxsize=None)
def pair_case(shape):
    """a: the text side (skip_first, B = 3), b: the video side (B = 5, one row without a valid frame); the similarity gradient
    dsim [3, 5 + 3] read by rows from a and by columns from b, as steps.py wires the pair launch."""
    sa, sb = shape
    a = make_side(("prefix", "holes", "last" if sa > PCHUNK else "full"), sa, 3000 + sa)
    b = make_side(("full", "prefix", "holes", "empty", "last" if sb > PCHUNK else "prefix"), sb, 4000 + sb)
    dsim = torch.full((PAIR_BB, PAIR_BB + DSIM_LD_PAD), SENT)
    dsim[:PAIR_BA, :PAIR_BB] = uniform(PAIR_BA, PAIR_BB, seed=5000 + sa).float()
    ra, rb = side_ref(a, True, True), side_ref(b, False, True)
    # the dsim form: each side's upstream gradient from the other side's fp32 `out`, scaled by 0.5
    oa, ob = ra.out.float(), rb.out.float()
    ga = tuple(upstream(dsim.to(t), ob.to(t), PAIR_BA, PAIR_BB, False, 0.5) for t in (F64, F32))
    gb = tuple(upstream(dsim.to(t), oa.to(t), PAIR_BB, PAIR_BA, True, 0.5) for t in (F64, F32))
    return SimpleNamespace(a=a, b=b, dsim=dsim, ra=ra, rb=rb, out_a=oa, out_b=ob, rda=side_ref(a, True, True, g=ga),
                           rdb=side_ref(b, False, True, g=gb))


# ------------------------------------------------------------------------------------------------ streaming kernels
# The grid caps, from the launch code: univl_tanh_fwd / _tanh_bwd / _gelu_bwd / _scale_ct_by_device_scalar clamp the grid to 2048
# workgroups of 256 threads (csrc/cross.hip), univl_scale_by_device_scalar to 1024 (csrc/simloss.hip); one element per thread and
# trip, so past cap elements the grid-stride loop takes a second trip.  univl_gather_rows clamps to 64 workgroups per row, 16 bytes per
# thread and trip: 64 * 256 * 16 = 262 144 bytes.
CAP_CROSS, CAP_SIMLOSS = 2048 * 256, 1024 * 256
GATHER_CAP_BYTES = 64 * 256 * 16


def stream_sizes(cap):
    return [1, 255, 257, cap - 1, cap, cap + 1, 2 * cap + 77]


TANH_GRID = [0.0, 1e-3, 0.25, 0.5, 1.0, 2.0, 3.0, 4.0, 20.0, 50.0, 100.0]      # and their negatives; from 20 on tanh rounds to +-1
TANH_SATURATED = 20.0
GELU_GRID = [0.0, 0.25, 0.5, 0.75, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 8.0, 9.5, 10.0]   # exact in bf16; |u| >= 8 is the far tail
GELU_TAIL = 8.0
GELU_GRAD_RANGE = 1.2579                         # gelu' runs from -0.1289 (u = -1.41) to 1.1289 (u = 1.41)
FLOOR_TANH, FLOOR = 1e-6, 1e-5


def with_grid(x, grid):
    """x with +-grid written over its first elements and (when it is long enough) over its last ones."""
    gv = torch.tensor([v for a in grid for v in (a, -a)], dtype=x.dtype)
    k = gv.numel()
    n = x.numel()
    if n >= k:
        x[:k] = gv
    else:
        x[:] = gv[-n:]
    if n >= 2 * k:
        x[n - k:] = gv
    return x


def tanh_input(n, seed):
    """Uniform on (-4, 4) with the grid at both ends."""
    return with_grid((4 * uniform(n, seed=seed)).float(), TANH_GRID)


def gelu_input(n, seed, dtype):
    """u: normal at scale 2 cut at +-10, in `dtype`, the grid at both ends; dg: uniform on (-1, 1), 1 at the grid positions."""
    g = torch.Generator().manual_seed(seed)
    u = with_grid((2 * torch.randn(n, generator=g)).clamp_(-10, 10).to(dtype), GELU_GRID)
    dg = uniform(n, seed=seed + 1).float()
    dg[grid_positions(n, len(GELU_GRID))] = 1.0
    return dg, u


def grid_positions(n, grid_len):
    """bool [n]: where with_grid wrote."""
    k = 2 * grid_len
    at = torch.zeros(n, dtype=torch.bool)
    at[:k] = True
    if n >= 2 * k:
        at[n - k:] = True
    return at


def tanh_grad(dy, y):
    return dy * (1 - y * y)


def gelu_grad(u):
    """d/du of the erf GELU: Phi(u) + u phi(u), with Phi(u) = erfc(-u / sqrt 2) / 2.  (1 + erf cancels in the negative tail: at u = -10
    even fp64 returns Phi = 0 there, a hundredth of the derivative; in fp32 the form is off by 3e-8 absolutely from u = -3.5 down.)"""
    return 0.5 * torch.special.erfc(u * (-1 / math.sqrt(2))) + u * torch.exp(-0.5 * u * u) * (1 / math.sqrt(2 * math.pi))


def abs_err(got, ref, scale=None):
    """max |got - ref| / scale elementwise (scale: |upstream| x the function's range; None: 1).  An element whose scale is 0 must be
    exact."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    d = torch.nan_to_num((got - ref).abs(), nan=float("inf"))
    if scale is None:
        return float(d.max())
    scale = scale.double()
    e = torch.where(scale > 0, d / scale.clamp_min(1e-300), torch.where(d > 0, torch.full_like(d, float("inf")), torch.zeros_like(d)))
    return float(e.max())


def rel_err(got, ref):
    """Whole tensor: max |got - ref| / max |ref|."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float(torch.nan_to_num((got - ref).abs(), nan=float("inf")).max() / (ref.abs().max() + 1e-300))


def _ordered(t):
    """bf16 -> int32, monotone in the value (+0 and -0 both 0)."""
    v = t.contiguous().view(torch.int16).int()
    return torch.where(v >= 0, v, -(v & 0x7FFF))


def bf16_ulps(got, ref64):
    """Largest distance, in bf16 steps, between `got` (bf16) and the fp64 reference rounded to bf16."""
    got = got.detach().cpu()
    assert got.dtype == BF16 and bool(torch.isfinite(got.float()).all())
    return int((_ordered(got) - _ordered(ref64.to(BF16))).abs().max())


def bf16_half_ulp_share(val32, ref64):
    """The distance of a torch-fp32 evaluation from fp64, as a share of half a bf16 step of the reference (2 ** -9 of its binade)."""
    ref64 = ref64.double()
    half = torch.where(ref64 != 0, 2.0 ** (torch.floor(torch.log2(ref64.abs().clamp_min(1e-300))) - 8), torch.zeros_like(ref64))
    d = (val32.double() - ref64).abs()
    return float(torch.where(half > 0, d / half.clamp_min(1e-300), torch.where(d > 0, torch.full_like(d, float("inf")), d)).max())


# ------------------------------------------------------------------------------------------------ exact references
RANK_SIZES = [1, 255, 256, 257, 600]
RANK_PAD = 3


def rank_input(n, ld, seed):
    """[n, ld] fp32.  Live n x n: values on the 1/8 grid (ties by themselves), ties with the diagonal planted at columns 0, 255, 256
    and n - 1, rows with +-inf entries, one row whose diagonal is +inf.  The ld - n padding columns hold diagonal + 1, the diagonal
    itself and +inf: counted by a loop that runs to ld."""
    g = torch.Generator().manual_seed(seed)
    x = torch.round(torch.randn(n, n, generator=g) * 16) / 8
    d = torch.arange(n)
    for col in (0, 255, 256, n - 1):
        if col < n:
            rows = d[(d % 3 == col % 3) | (d == col)]
            x[rows, col] = x[rows, rows]
    if n > 4:
        x[1, 3] = float("inf")
        x[2, 0] = float("-inf"); x[2, n - 1] = float("inf")
        x[n - 2, :] = torch.where(torch.rand(n, generator=g) < 0.3, torch.tensor(float("inf")), x[n - 2, :])
        x[n - 2, n - 2] = float("inf")                   # a diagonal of +inf: nothing is greater, the +inf entries are equal
        x[3, 3] = float("-inf")                          # a diagonal of -inf: every finite entry is greater
    buf = torch.empty(n, ld)
    buf[:, :n] = x
    if ld > n:
        diag = x.diag()
        pad = torch.stack([diag + 1, diag, torch.full_like(diag, float("inf"))], 1)
        buf[:, n:] = pad[:, :ld - n]
    return buf


def rank_counts_ref(buf, n):
    x = buf[:n, :n]
    d = x.diag()[:, None]
    return (x > d).sum(1).int(), (x == d).sum(1).int()


CONCAT_SHAPES = [(1, 2, 3), (2, 4, 3), (3, 5, 4), (5, 7, 6)]             # (P, W, F): P (W + F) % 4 = 1, 2, 3, 1 (17 workgroups)
CONCAT_MASK_SENT = -7


def concat_input(P, W, F, form, seed):
    """form 'arange': pair p = (text p, video p); 'repeated': rows drawn with repeats, out of order.  Every index is in range."""
    Bt, Bv = P + 1, P + 2
    g = torch.Generator().manual_seed(seed)
    seq, vis = torch.randn(Bt, W, N, generator=g), torch.randn(Bv, F, N, generator=g)
    am, vm = torch.randint(0, 2, (Bt, W), generator=g), torch.randint(0, 2, (Bv, F), generator=g)
    if form == "arange":
        tidx = vidx = torch.arange(P, dtype=torch.int32)
    else:
        tidx = torch.randint(0, Bt, (P,), generator=g).int()
        vidx = torch.randint(0, Bv, (P,), generator=g).int()
        if P > 1:
            tidx[-1], vidx[0] = tidx[0], vidx[-1]
    assert 0 <= int(tidx.min()) and int(tidx.max()) < Bt and 0 <= int(vidx.min()) and int(vidx.max()) < Bv
    return SimpleNamespace(seq=seq, vis=vis, am=am, vm=vm, tidx=tidx, vidx=vidx)


def concat_ref(i):
    t, v = i.tidx.long(), i.vidx.long()
    return torch.cat((i.seq[t], i.vis[v]), 1), torch.cat((i.am[t], i.vm[v]), 1)


GATHER_BYTES = [0, 16, GATHER_CAP_BYTES - 16, GATHER_CAP_BYTES, GATHER_CAP_BYTES + 16, 600000]
GATHER_TAIL = 48                                 # row_stride - copy_bytes of the cases that leave a tail
GATHER_IDX = [4, 0, 4, 2, 1]                     # repeated and out of order; the source has 6 rows
GATHER_SRC_ROWS = 6
