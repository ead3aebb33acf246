"""The similarity losses, the MFM / vocabulary loss kernels and the small cross-encoder head kernels (csrc/simloss.hip, csrc/cross.hip,
csrc/embed.hip) against the fp64 references of tests/head_ref.py, past one block stride (n > 256 for the 256-thread loops, more than 64
pairs / 256 tokens for the duplicate scans), on the padded views the step hands them (ld > n), at un-normalised magnitudes, and in both
sum modes.  Needs a real MI355X (`-m gpu`).

Tolerances: every loss and its gradient under head_ref.gate() (max(1e-5, 8 x the fp32-vs-fp64 error of the same formula in torch));
the bf16 gradient of ce_loss keeps the 1e-2 of tests/test_kernels_gpu.py; the plain sums keep that file's 1e-5 / 1e-6, which bound
k * 2**-24 for the k <= 300 terms summed here.  Every case prints its observed error, e32 and gate (`pytest -s`):
profiles/head_kernel_parity.txt is that output.

No label, id or index here is out of range: the kernels do not check them."""
import functools
import math

import pytest
import torch

import head_ref as R

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import univl_amd
    from univl_amd import ops

DEV = "cuda"
SENT = 12345.0                      # padding sentinel of the fp32 buffers (the compute-type gradient of ce_loss pads with 7: exact in bf16)
NAN, INF = float("nan"), float("inf")


@pytest.fixture(params=[False, True], ids=["atomic", "deterministic"])
def mode(request):
    was = univl_amd.deterministic()
    univl_amd.set_deterministic(request.param)
    try:
        yield request.param
    finally:
        univl_amd.set_deterministic(was)


def _report(case, **figures):
    print("head-parity  %-64s %s" % (case, "  ".join("%s %.2e" % kv for kv in figures.items())))


def _check(case, loss, grad, g, grad_tol=None):
    """Loss and gradient against the fp64 reference carried by the gate."""
    el, eg = R.loss_err(float(loss), g.ref_loss), R.grad_err(grad, g.ref_grad)
    _report(case, loss_err=el, e32_loss=g.e32_loss, loss_gate=g.loss, grad_err=eg, e32_grad=g.e32_grad, grad_gate=grad_tol or g.grad)
    assert bool(torch.isfinite(grad.float()).all()), case
    assert el <= g.loss, (case, el, g.loss, float(loss), g.ref_loss)
    assert eg <= (grad_tol or g.grad), (case, eg, grad_tol or g.grad)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same_bits(a, b):
    return all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _max_abs(t):
    return float(t.float().abs().max()) if t.numel() else 0.0


def _pad_ld(n, pad):
    return {"contiguous": n, "ldp": (n + 3) // 4 * 4, "n+3": n + 3}[pad]


# ----------------------------------------------------------------------------------------------- similarity losses
@functools.lru_cache(maxsize=None)
def _sim_ref(kind, bs, n_pair, scale):
    n = bs * n_pair
    if kind == "maxmargin":
        x = R.maxmargin_input(n, scale, R.SIM_SEED)
        return x, R.gate(R.maxmargin_f(bs, n_pair, weighted=n_pair > 1), x)
    x = R.sim_input(n, scale, R.SIM_SEED)
    return x, R.gate(R.crossen_f() if kind == "crossen" else R.milnce_f(bs, n_pair), x)


def _sim_run(kind, bs, n_pair, x, ld):
    """One launch on [:, :n] views of [n, ld] buffers: +inf in sim's padding (must not be read), NaN inside dsim's view (must be
    overwritten), a sentinel in dsim's padding (must keep its bits).  Returns (loss, dsim buffer)."""
    n = bs * n_pair
    sim = torch.full((n, ld), INF, device=DEV)
    sim[:, :n] = x.to(DEV)
    ds = torch.full((n, ld), SENT, device=DEV)
    ds[:, :n] = NAN
    loss = torch.full((1,), NAN, device=DEV)
    if kind == "maxmargin":
        w = R.simloss_weights(bs, n_pair).to(DEV) if n_pair > 1 else None
        ops.maxmargin_loss(sim[:, :n], R.MARGIN, w, loss, ds[:, :n])
    elif kind == "crossen":
        ops.crossen_loss(sim[:, :n], loss, ds[:, :n])
    else:
        ops.milnce_loss(sim[:, :n], bs, n_pair, loss, ds[:, :n])
    assert torch.equal(sim[:, :n].cpu(), x) and bool(torch.isinf(sim[:, n:]).all())
    assert bool((ds[:, n:] == SENT).all()), "dsim padding written"
    return loss, ds


SIM_CASES = [(k, n, 1) for k in ("maxmargin", "crossen") for n in R.SIM_SIZES] + [("maxmargin",) + R.WEIGHTED_SHAPE] \
    + [("milnce",) + s for s in R.MIL_SHAPES]


@pytest.mark.parametrize("pad", ["contiguous", "ldp", "n+3"])
@pytest.mark.parametrize("scale", R.SCALES)
@pytest.mark.parametrize("kind,bs,n_pair", SIM_CASES)
def test_similarity_losses(kind, bs, n_pair, scale, pad):
    n = bs * n_pair
    x, g = _sim_ref(kind, bs, n_pair, scale)
    loss, ds = _sim_run(kind, bs, n_pair, x, _pad_ld(n, pad))
    _check("%s bs=%d n_pair=%d scale=%g ld=%s" % (kind, bs, n_pair, scale, pad), loss, ds[:, :n], g)


@pytest.mark.parametrize("kind,bs,n_pair", [("maxmargin", 257, 1), ("maxmargin",) + R.WEIGHTED_SHAPE, ("crossen", 257, 1), ("milnce", 129, 2)])
def test_similarity_losses_repeat_bit_for_bit(kind, bs, n_pair, mode):
    """No similarity loss branches on the mode, and none may depend on arrival order in either: the weighted max-margin at n = 258
    sums two distinct weights (one not an integer) onto its diagonal."""
    n = bs * n_pair
    x, _ = _sim_ref(kind, bs, n_pair, 30.0)
    first = _sim_run(kind, bs, n_pair, x, n + 3)
    for _ in range(3):
        again = _sim_run(kind, bs, n_pair, x, n + 3)
        assert _same_bits((first[0], first[1][:, :n].contiguous()), (again[0], again[1][:, :n].contiguous()))


# ----------------------------------------------------------------------------------------------- MFM NCE
@functools.lru_cache(maxsize=None)
def _mfm_ref(B, F, selected_padded):
    x, vmask, labels = R.mfm_input(B, F, R.MFM_CASES[(B, F)], R.MFM_SEED, selected_padded)
    return x, vmask, labels, R.gate(R.mfm_f(labels), R.mfm_masked32(x, vmask))


def _mfm_run(x, vmask, labels):
    """As steps.py calls it: in place on buf[:, :n] of an [n, ld] buffer, ld > n."""
    n = x.shape[0]
    buf = torch.full((n, n + 5), SENT, device=DEV)
    buf[:, :n] = x.to(DEV)
    loss, scr = torch.full((1,), NAN, device=DEV), torch.full((2,), NAN, device=DEV)
    ops.mfm_nce_loss(buf[:, :n], vmask.to(DEV), labels.to(DEV), scr, loss, buf[:, :n])
    assert bool((buf[:, n:] == SENT).all()), "logits padding written"
    assert float(scr[0]) == float((labels != -1).sum())
    return loss, buf[:, :n].contiguous()


@pytest.mark.parametrize("B,F,selected_padded", [(1, 1, False), (6, 48, False), (6, 48, True), (11, 48, False), (11, 48, True)])
def test_mfm_nce_loss(B, F, selected_padded, mode):
    x, vmask, labels, g = _mfm_ref(B, F, selected_padded)
    assert (R.n_selected_padded(vmask, labels) > 0) == selected_padded
    loss, grad = _mfm_run(x, vmask, labels)
    case = "mfm B=%d F=%d %s %s" % (B, F, "selected-padded-rows" if selected_padded else "clean", "det" if mode else "atomic")
    _check(case, loss, grad, g)
    assert _max_abs(grad[(labels == -1).to(DEV)]) == 0.0, "unselected rows carry a gradient"
    if not selected_padded:
        # no selected row's own frame is padded: the mask applied in fp64 is the same operation
        l64, g64 = R.evaluate(R.mfm_f(labels), R.mfm_masked64(x, vmask))
        assert R.loss_err(float(loss), float(l64)) <= g.loss and R.grad_err(grad, g64) <= g.grad
    if mode:
        assert _same_bits((loss, grad), _mfm_run(x, vmask, labels))
    none = torch.full_like(labels, -1)
    loss, grad = _mfm_run(x, vmask, none)
    assert math.isnan(float(loss)) and float(grad.abs().max()) == 0.0


# ----------------------------------------------------------------------------------------------- vocabulary CE
@functools.lru_cache(maxsize=None)
def _ce_ref(rows, V, ignore):
    x, labels = R.ce_input(rows, V, ignore, seed=7)
    nvalid = int((labels != ignore).sum())
    return x, labels, nvalid, (R.gate(R.ce_f(labels, ignore), x) if nvalid else None)


def _ce_run(x, labels, V, ld, lddl, dtype, ignore):
    rows = x.shape[0]
    logits = torch.full((rows, ld), SENT, device=DEV)
    logits[:, :V] = x.to(DEV)
    dl = torch.full((rows, lddl), 7.0, device=DEV, dtype=dtype)
    dl[:, :V] = NAN
    loss, scr = torch.full((1,), NAN, device=DEV), torch.full((2,), NAN, device=DEV)
    ops.ce_loss(logits[:, :V], labels.to(DEV), V, scr, loss, dl[:, :V], ignore_index=ignore)
    assert torch.equal(logits[:, :V].cpu(), x) and bool((logits[:, V:] == SENT).all()), "logits written"
    assert bool((dl[:, V:].float() == 7.0).all()), "dlogits padding written"
    return loss, dl[:, :V].contiguous(), scr


# (V, ld, lddl).  1002 / 1003: with fp32 logits every other row (bf16 gradient: three rows in four) starts off the 16-byte (8-byte) grid
# and takes the scalar passes; 1008: every row takes the vector passes and their scalar tail
CE_LAYOUTS = [(1, 1, 1), (1, 3, 2), (3, 3, 5), (3, 4, 4), (1002, 1002, 1003), (1002, 1008, 1008)]


@pytest.mark.parametrize("ignore", [-1, 0])
@pytest.mark.parametrize("rows", [1, 300])
@pytest.mark.parametrize("V,ld,lddl", CE_LAYOUTS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_ce_loss(dtype, V, ld, lddl, rows, ignore, mode):
    x, labels, nvalid, g = _ce_ref(rows, V, ignore)
    loss, grad, scr = _ce_run(x, labels, V, ld, lddl, dtype, ignore)
    assert float(scr[0]) == float(nvalid)
    assert _max_abs(grad[(labels == ignore).to(DEV)]) == 0.0, "ignored rows carry a gradient"
    if nvalid == 0:                                       # nothing to average over: NaN, like torch; gradient all zero
        assert math.isnan(float(loss)) and float(grad.float().abs().max()) == 0.0
        return
    case = "ce %s V=%d ld=%d lddl=%d rows=%d ignore=%d %s" % ("bf16" if dtype == torch.bfloat16 else "fp32", V, ld, lddl, rows, ignore,
                                                              "det" if mode else "atomic")
    _check(case, loss, grad, g, grad_tol=1e-2 if dtype == torch.bfloat16 else None)
    if mode:
        again = _ce_run(x, labels, V, ld, lddl, dtype, ignore)
        assert _same_bits((loss, grad), again[:2])


# ----------------------------------------------------------------------------------------------- log-softmax rows
def _half_ulp32(v):
    return 2.0 ** (math.floor(math.log2(max(float(v), 2.0 ** -126))) - 24)


@pytest.mark.parametrize("n", [1, 255, 257])
def test_log_softmax_rows(n):
    rows, ld = 5, n + 3
    x = torch.randn(rows, n, generator=torch.Generator().manual_seed(3)) * 30.0
    buf = torch.full((rows, ld), SENT, device=DEV)
    buf[:, :n] = x.to(DEV)
    ops.log_softmax_rows(buf, n)
    ref = torch.log_softmax(x.double(), dim=-1)
    lse = torch.logsumexp(x.double(), dim=-1)
    # out = fl(x - fl(max + fl(log s))): half an ulp of the largest |lse|, half an ulp of the largest |out|, and 2e-6 for logf and the sum
    bound = _half_ulp32(lse.abs().max()) + _half_ulp32(ref.abs().max()) + 2e-6
    err = float((buf[:, :n].double().cpu() - ref).abs().max())
    _report("log_softmax_rows n=%d ld=%d scale=30" % (n, ld), abs_err=err, bound=bound)
    assert err <= bound
    assert bool((buf[:, n:] == SENT).all()), "padding written"


# ----------------------------------------------------------------------------------------------- similarity_dense
@pytest.mark.parametrize("rows", [1, 3, 5, 260])
def test_simdense_fwd_bwd(rows):
    gen = torch.Generator().manual_seed(rows)
    x, w, b = torch.randn(rows, 768, generator=gen), torch.randn(768, generator=gen) * 0.05, torch.randn(1, generator=gen)
    ds = torch.randn(rows, generator=gen)
    dw0, db0 = torch.randn(768, generator=gen), torch.randn(1, generator=gen)       # the kernel accumulates into both
    s = torch.full((rows,), NAN, device=DEV)
    ops.simdense_fwd(x.to(DEV), w.to(DEV), b.to(DEV), s)
    outs = []
    for _ in range(2):
        dx = torch.full((rows, 768), NAN, device=DEV)
        dw, db = dw0.to(DEV), db0.to(DEV)
        ops.simdense_bwd(ds.to(DEV), x.to(DEV), w.to(DEV), dx, dw, db)
        outs.append((dx, dw, db))
    dx, dw, db = outs[0]
    ref_db = float(db0.double() + ds.double().sum())
    errs = dict(fwd=R.grad_err(s, x.double() @ w.double() + b.double()), dx=R.grad_err(dx, ds.double()[:, None] * w.double()[None]),
                dw=R.grad_err(dw, dw0.double() + ds.double() @ x.double()), db=abs(float(db) - ref_db) / max(1.0, abs(ref_db)))
    _report("simdense rows=%d" % rows, **errs)
    assert errs["fwd"] <= 1e-5 and errs["dx"] <= 1e-6 and errs["dw"] <= 1e-5 and errs["db"] <= 1e-5
    assert _same_bits(outs[0], outs[1])


# ----------------------------------------------------------------------------------------------- pair concat backward
@pytest.mark.parametrize("form", ["all_pairs", "arange"])
def test_pair_concat_bwd(form, mode):
    """all_pairs: the index lists of _cross_similarity, Bt = 9 texts x Bv = 8 videos -> P = 72 pairs: the 64-lane duplicate scan of the
    deterministic kernel takes a second trip.  arange: the split of the pretraining step (steps.py, tidx = vidx = arange(B))."""
    W, F, S = 5, 7, 12
    if form == "all_pairs":
        Bt, Bv = 9, 8
        pairs = [(i, j) for i in range(Bt) for j in range(Bv)]
    else:
        Bt = Bv = 6
        pairs = [(i, i) for i in range(Bt)]
    P = len(pairs)
    gen = torch.Generator().manual_seed(P)
    d = torch.randn(P, S, 768, generator=gen)
    dseq0, dvis0 = torch.randn(Bt, W, 768, generator=gen), torch.randn(Bv, F, 768, generator=gen)
    tidx = torch.tensor([a for a, _ in pairs], dtype=torch.int32, device=DEV)
    vidx = torch.tensor([b for _, b in pairs], dtype=torch.int32, device=DEV)
    rs, rv = dseq0.double(), dvis0.double()
    rs.index_add_(0, tidx.long().cpu(), d[:, :W].double())
    rv.index_add_(0, vidx.long().cpu(), d[:, W:].double())
    outs = []
    for _ in range(2):
        dseq, dvis = dseq0.to(DEV).view(Bt * W, 768), dvis0.to(DEV).view(Bv * F, 768)
        ops.pair_concat_bwd(d.to(DEV).view(P * S, 768), tidx, vidx, P, W, F, dseq, dvis)
        outs.append((dseq, dvis))
    es, ev = R.grad_err(outs[0][0].view(Bt, W, 768), rs), R.grad_err(outs[0][1].view(Bv, F, 768), rv)
    _report("pair_concat_bwd %s P=%d %s" % (form, P, "det" if mode else "atomic"), dseq=es, dvis=ev)
    assert es <= 1e-6 and ev <= 1e-6
    if mode:
        assert _same_bits(outs[0], outs[1])


# ----------------------------------------------------------------------------------------------- embedding scatter
@pytest.mark.parametrize("scale", [1.0, 0.25])
def test_embed_scatter(scale, mode):
    """300 tokens over 40 distinct ids of a 50-row table: id 0, the last row, one id 70 times (the deterministic kernel's 256-wide
    duplicate scan takes a second trip from token 256 on); scale 0.25 is the 1 / world of the multi-GPU path."""
    T, rows_total = 300, 50
    gen = torch.Generator().manual_seed(17)
    last = rows_total - 1
    pool = torch.cat([torch.tensor([0]), 1 + torch.randperm(rows_total - 2, generator=gen)[:38]])
    ids = torch.cat([pool, torch.full((69,), int(pool[5])), pool[torch.randint(0, 39, (T - 2 - 39 - 69,), generator=gen)]])
    ids = ids[torch.randperm(T - 2, generator=gen)]
    # the last row's id occurs at tokens 270 and 295 only: the owner of its second occurrence is found on the scan's second trip
    ids = torch.cat([ids[:270], torch.tensor([last]), ids[270:294], torch.tensor([last]), ids[294:]]).contiguous()
    assert ids.shape == (T,) and len(set(ids.tolist())) == 40 and int(ids.min()) == 0 and int(ids.max()) == last
    assert (ids == last).nonzero().reshape(-1).tolist() == [270, 295] and int((ids == int(pool[5])).sum()) > 64
    rows = torch.randn(T, 768, generator=gen)
    table0 = torch.randn(rows_total, 768, generator=gen)
    ref = table0.double().index_add_(0, ids, rows.double() * scale)
    outs = []
    for _ in range(2):
        table = table0.to(DEV)
        ops.embed_scatter(ids.to(DEV), rows.to(DEV), scale, table)
        outs.append(table)
    err = R.grad_err(outs[0], ref)
    _report("embed_scatter scale=%g %s" % (scale, "det" if mode else "atomic"), err=err)
    assert err <= 1e-5                                     # <= 71 terms per element: 71 * 2**-24 of sum |terms| <= 1e-5 of the largest sum
    untouched = torch.tensor(sorted(set(range(rows_total)) - set(ids.tolist())))
    assert len(untouched) == 10 and torch.equal(outs[0][untouched.to(DEV)].cpu(), table0[untouched])
    if mode:
        assert _same_bits(outs[:1], outs[1:])


# ----------------------------------------------------------------------------------------------- column sums
@pytest.mark.parametrize("n", [1, 1000])
@pytest.mark.parametrize("rows", [1, 64, 65, 300])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_colsum(dtype, rows, n, mode):
    """Default mode: 64 rows per block, so 65 and 300 rows give 2 and 5 row blocks adding with atomics; deterministic mode: one block
    walks every row.  A strided, misaligned view; the output starts non-zero."""
    gen = torch.Generator().manual_seed(rows * 7 + n)
    big = torch.randn(rows, 1040, generator=gen).to(DEV, dtype)
    view = big[:, 3:3 + n]
    out0 = torch.randn(n, generator=gen)
    ref = out0.double() + view.double().cpu().sum(0)
    outs = []
    for _ in range(2):
        out = out0.to(DEV)
        ops.colsum(view, out)
        outs.append(out)
    err = R.grad_err(outs[0], ref)
    _report("colsum %s rows=%d n=%d %s" % ("bf16" if dtype == torch.bfloat16 else "fp32", rows, n, "det" if mode else "atomic"), err=err)
    assert err <= 1e-5
    if mode:
        assert _same_bits(outs[:1], outs[1:])


# ----------------------------------------------------------------------------------------------- position + type table
@pytest.mark.parametrize("W,S", [(0, 13), (1, 13), (12, 13), (13, 13), (5, 20)])
def test_postype_fwd_bwd(W, S):
    """Either half empty or not, halves of 1, 5, 8, 12, 13 and 15 positions: whole 8-wide groups and their tails."""
    gen = torch.Generator().manual_seed(W * 31 + S)
    pos, typ = torch.randn(32, 768, generator=gen), torch.randn(2, 768, generator=gen)
    tab = torch.full((S, 768), NAN, device=DEV)
    ops.postype_fwd(pos.to(DEV), typ.to(DEV), W, S, tab)
    assert torch.equal(tab.cpu(), pos[:S] + typ[(torch.arange(S) >= W).long()])
    dt_ = torch.randn(S, 768, generator=gen)
    dpos0, dtyp0 = torch.randn(32, 768, generator=gen), torch.randn(2, 768, generator=gen)
    outs = []
    for _ in range(2):
        dpos, dtyp = dpos0.to(DEV), dtyp0.to(DEV)
        ops.postype_bwd(dt_.to(DEV), W, S, dpos, dtyp)
        outs.append((dpos, dtyp))
    dpos, dtyp = outs[0]
    ref_typ = dtyp0.double() + torch.stack([dt_[:W].double().sum(0), dt_[W:].double().sum(0)])
    ep, et = R.grad_err(dpos[:S], dpos0[:S].double() + dt_.double()), R.grad_err(dtyp, ref_typ)
    _report("postype W=%d S=%d" % (W, S), dpos=ep, dtype=et)
    assert ep <= 1e-6 and et <= 1e-6
    assert torch.equal(dpos[S:].cpu(), dpos0[S:])
    if W == 0:
        assert torch.equal(dtyp[0].cpu(), dtyp0[0])
    if W == S:
        assert torch.equal(dtyp[1].cpu(), dtyp0[1])
    assert _same_bits(outs[0], outs[1])
