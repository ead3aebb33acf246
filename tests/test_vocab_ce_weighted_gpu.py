"""The weighted form of K16 (univl_vocab_ce_weighted_fwd / _bwd, csrc/vocab_ce.h): one fp32 weight per caption on the vocabulary
classifier's online log-softmax cross entropy.  Against fp64 on the SAME (rounded) operands with the gates of
tests/test_kernels_gpu.py::test_vocab_ce_online_log_softmax_matches_the_materialised_path, and bit for bit against the unweighted entry
points when every weight is 1.0f.  Needs a real MI355X (`-m gpu`).

Shapes (rows, V, seq_len), K = 768: V = 1002 leaves a partial column tile; seq_len = 24 makes caption 5 own rows 120 .. 143, so one
caption straddles the 128-row tile edge; 30522 is 238 full column tiles + 58 columns."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from univl_amd import ops

DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16]
SHAPES = [(48, 1000, 8), (192, 1002, 24), (96, 30522, 32)]
K = 768
GOUT = 0.37


def rel_err(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def tol(dtype):
    return 1e-3 if dtype == torch.float32 else 1e-2


def gen(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def operands(dtype, rows, V, seq_len):
    """x, table, bias, labels (every fifth row ignored, labels 0 and V - 1 present), weights in [-2, 2] with one caption exactly 0, one
    exactly 1 and one negative."""
    x = gen(rows, K, seed=1).to(DEV, dtype)
    table = gen(V, K, seed=2, scale=0.06).to(DEV, dtype)
    bias = gen(V, seed=3, scale=0.5).to(DEV)
    g = torch.Generator().manual_seed(4)
    labels = torch.randint(0, V, (rows,), generator=g)
    labels[::5] = -1
    labels[1], labels[2] = 0, V - 1
    n_seq = rows // seq_len
    w = (torch.rand(n_seq, generator=torch.Generator().manual_seed(5)) * 4.0 - 2.0).float()
    w[0], w[1], w[n_seq - 1] = 0.0, 1.0, -1.25
    return x, table, bias, labels, w


def run_weighted(x, table, bias, labels_d, w_d, V, seq_len, dtype, gout):
    rows = x.shape[0]
    ldv = (V + 7) // 8 * 8
    dl = torch.full((rows, ldv), 7.0, device=DEV, dtype=dtype)
    d, buf = ops.vocab_ce_weighted_desc(x, table, bias, labels_d, dl, V, w_d, seq_len)
    ops.vocab_ce_weighted_fwd(d)
    d.gout = gout.data_ptr()
    ops.vocab_ce_weighted_bwd(d)
    return d, buf, dl


@pytest.mark.parametrize("rows,V,seq_len", SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_weighted_vocab_ce_matches_fp64_on_the_same_operands(dtype, rows, V, seq_len):
    x, table, bias, labels, w = operands(dtype, rows, V, seq_len)
    labels_d, w_d = labels.to(DEV), w.to(DEV)
    gout = torch.tensor([GOUT], device=DEV)
    d, buf, dl = run_weighted(x, table, bias, labels_d, w_d, V, seq_len, dtype, gout)
    ldv = dl.shape[1]
    # ---- fp64 on the same rounded operands
    lr = (x.double().cpu() @ table.double().cpu().T + bias.double().cpu()).requires_grad_(True)
    counts = labels != -1
    n_valid = int(counts.sum())
    lse = torch.logsumexp(lr, 1)
    nll = lse[counts] - lr[counts, labels[counts]]
    wr = w.double().repeat_interleave(seq_len)[counts]
    ref = (wr * nll).sum() / n_valid
    (ref * GOUT).backward()
    ref = ref.detach()
    size = float((wr.abs() * nll.detach()).sum() / n_valid)         # mixed signs cancel: the gate scales with the size of the summed terms
    print("loss %.9g ref %.9g size %.4g; lse rel %.3g; dlogits rel %.3g" % (
        float(buf["loss"]), float(ref), size, rel_err(buf["lse"], lse.detach()), rel_err(dl[:, :V].float(), lr.grad)))
    assert abs(float(buf["loss"]) - float(ref)) < 3e-6 * max(1.0, size), (float(buf["loss"]), float(ref), size)
    assert float(buf["scratch"][0]) == float(n_valid)
    assert rel_err(buf["lse"], lse.detach()) < 1e-6
    assert rel_err(dl[:, :V].float(), lr.grad) < tol(dtype)
    rowloss_ref = torch.zeros(rows, dtype=torch.float64)
    rowloss_ref[counts] = (wr * nll).detach()
    assert rel_err(buf["rowloss"], rowloss_ref) < 3e-6
    # ---- ignored rows and zero-weight rows: exact zeros; padding columns untouched
    assert float(dl[::5, :V].float().abs().max()) == 0.0 and float(buf["rowloss"][::5].abs().max()) == 0.0
    assert float(dl[:seq_len, :V].float().abs().max()) == 0.0 and float(buf["rowloss"][:seq_len].abs().max()) == 0.0       # w[0] = 0
    assert float(dl[seq_len:2 * seq_len, :V].float().abs().max()) > 0.0                                                  # w[1] = 1
    if ldv > V:
        assert float((dl[:, V:].float() - 7.0).abs().max()) == 0.0
    # ---- bit-reproducible: fixed-order folds everywhere
    first = (buf["loss"].clone(), buf["lse"].clone(), buf["rowloss"].clone(), dl.clone())
    d.gout = None
    ops.vocab_ce_weighted_fwd(d)
    d.gout = gout.data_ptr()
    ops.vocab_ce_weighted_bwd(d)
    assert torch.equal(buf["loss"], first[0]) and torch.equal(buf["lse"], first[1]) and torch.equal(buf["rowloss"], first[2])
    assert torch.equal(dl, first[3])
    # ---- nothing to average over: NaN, like torch; dlogits all zero
    labels_d.fill_(-1)
    ops.vocab_ce_weighted_fwd(d)
    ops.vocab_ce_weighted_bwd(d)
    assert math.isnan(float(buf["loss"])) and float(dl[:, :V].float().abs().max()) == 0.0 and float(buf["scratch"][0]) == 0.0


@pytest.mark.parametrize("rows,V,seq_len", SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_all_weights_one_is_the_unweighted_entry_point_bit_for_bit(dtype, rows, V, seq_len):
    x, table, bias, labels, _ = operands(dtype, rows, V, seq_len)
    labels_d = labels.to(DEV)
    ones = torch.ones(rows // seq_len, device=DEV)
    gout = torch.tensor([GOUT], device=DEV)
    _, bw, dlw = run_weighted(x, table, bias, labels_d, ones, V, seq_len, dtype, gout)
    dl = torch.full_like(dlw, 7.0)
    d, b = ops.vocab_ce_desc(x, table, bias, labels_d, dl, V)
    ops.vocab_ce_fwd(d)
    d.gout = gout.data_ptr()
    ops.vocab_ce_bwd(d)
    for name in ("loss", "lse", "rowloss", "scratch"):
        assert torch.equal(bw[name], b[name]), name
    assert torch.equal(dlw, dl)


def test_weighted_vocab_ce_refuses_what_the_header_excludes():
    rows, V, seq_len = 48, 1000, 8
    x, table, bias, labels, w = operands(torch.float32, rows, V, seq_len)
    dl = torch.zeros(rows, V, device=DEV)
    for bad in (0, 7, -1):                                   # seq_len >= 1 dividing rows
        d, _ = ops.vocab_ce_weighted_desc(x, table, bias, labels.to(DEV), dl, V, torch.ones(rows, device=DEV), bad)
        with pytest.raises(RuntimeError):
            ops.vocab_ce_weighted_fwd(d)
        with pytest.raises(RuntimeError):
            ops.vocab_ce_weighted_bwd(d)
    d, _ = ops.vocab_ce_weighted_desc(x, table, bias, labels.to(DEV), dl, V, w.to(DEV), seq_len)
    d.seq_weight = None
    with pytest.raises(RuntimeError):
        ops.vocab_ce_weighted_fwd(d)
