"""The smoothed form of K16 (univl_vocab_ce_smooth_fwd / _bwd, csrc/vocab_ce.h): CrossEntropyLoss(ignore_index=-1, label_smoothing=eps) in
the epilogue of the vocabulary product, with an optional fp32 weight per caption; and UniVL.caption_label_smoothing on top of it.  Needs a
real MI355X (`-m gpu`).

Shapes (rows, V, seq_len, K):
  (130, 8300, 13, 64)    two row tiles, the second partial, caption 9 straddling row 128; 65 column tiles, so the row fold's lane stride
                         wraps past 64 slots; the last column tile has 108 columns; K is the bf16 minimum
  (48, 1000, 8, 768)     a small V with a partial last column tile (7 x 128 + 104): eps / V is large enough to be checked sharply
  (96, 30522, 32, 768)   the real table: 238 full tiles + 58 columns
Operands: the recipe of tests/test_vocab_ce_weighted_gpu.py (every fifth row ignored, labels 0 and V - 1 present, a bias, weights in
[-2, 2] with one caption exactly 0, one exactly 1 and one negative, gout = 0.37) plus one caption whose rows are all ignored.  The
fp64 reference of a (dtype, shape) is formed once on the CPU from the same rounded operands and shared."""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import univl_oracle as O
from make_golden import case_config

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import univl_amd
    from univl_amd import ops
    from test_model_gpu import build, call, gates_for, plan_ops

DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16]
IDS = ["fp32", "bf16"]
SHAPES = [(130, 8300, 13, 64), (48, 1000, 8, 768), (96, 30522, 32, 768)]
SMALL_V = (48, 1000, 8, 768)
EPS = [0.1, 0.5]
GOUT = 0.37
FILL = 7.0


def rel_err(a, b):
    """max-abs error over max-abs reference: the convention of the K16 tests"""
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def tol(dtype):
    return 1e-3 if dtype == torch.float32 else 1e-2


def gen(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def all_ignored_caption(n_seq):
    """the caption whose rows are all ignored: one of random weight where there is one, else the zero-weight caption 0"""
    return 2 if n_seq > 3 else 0


@functools.lru_cache(maxsize=None)
def operands(dtype, shape):
    """Host labels / weights and device operands.  Labels 0 and V - 1 sit in caption 1 (weight exactly 1)."""
    rows, V, seq_len, K = shape
    x = gen(rows, K, seed=1).to(DEV, dtype)
    table = gen(V, K, seed=2, scale=0.06).to(DEV, dtype)
    bias = gen(V, seed=3, scale=0.5).to(DEV)
    labels = torch.randint(0, V, (rows,), generator=torch.Generator().manual_seed(4))
    labels[::5] = -1
    r0, r1 = [r for r in range(seq_len, 2 * seq_len) if r % 5][:2]            # two counting rows of caption 1
    labels[r0], labels[r1] = 0, V - 1
    n_seq = rows // seq_len
    c = all_ignored_caption(n_seq)
    labels[c * seq_len:(c + 1) * seq_len] = -1
    w = (torch.rand(n_seq, generator=torch.Generator().manual_seed(5)) * 4.0 - 2.0).float()
    w[0], w[1], w[n_seq - 1] = 0.0, 1.0, -1.25
    return x, table, bias, labels, w


@functools.lru_cache(maxsize=None)
def logits64(dtype, shape):
    """fp64 logits of the rounded operands, on the CPU, once per (dtype, shape)"""
    x, table, bias, _, _ = operands(dtype, shape)
    return x.double().cpu() @ table.double().cpu().T + bias.double().cpu()


def reference(dtype, shape, eps, weighted):
    """torch's own smoothed cross entropy in float64, times the weights, over n_valid; its gradient under gout"""
    rows, V, seq_len, K = shape
    _, _, _, labels, w = operands(dtype, shape)
    lr = logits64(dtype, shape).clone().requires_grad_(True)
    ce = F.cross_entropy(lr, labels, ignore_index=-1, label_smoothing=eps, reduction="none")
    wr = w.double().repeat_interleave(seq_len) if weighted else torch.ones(rows, dtype=torch.float64)
    n_valid = int((labels != -1).sum())
    rowloss = wr * ce
    loss = rowloss.sum() / n_valid
    (loss * GOUT).backward()
    return dict(loss=loss.detach(), rowloss=rowloss.detach(), lse=torch.logsumexp(lr.detach(), 1), dlogits=lr.grad, n_valid=n_valid, wr=wr)


def run_smooth(dtype, shape, eps, weighted, labels=None, x=None, w=None):
    rows, V, seq_len, K = shape
    x0, table, bias, labels0, w0 = operands(dtype, shape)
    x = x0 if x is None else x
    labels_d = (labels0 if labels is None else labels).to(DEV)
    w_d = (w0 if w is None else w).to(DEV) if weighted else None
    dl = torch.full((x.shape[0], (V + 7) // 8 * 8), FILL, device=DEV, dtype=dtype)
    gout = torch.tensor([GOUT], device=DEV)
    d, buf = ops.vocab_ce_smooth_desc(x, table, bias, labels_d, dl, V, eps, w_d, seq_len if weighted else None)
    ops.vocab_ce_smooth_fwd(d)
    d.gout = gout.data_ptr()
    ops.vocab_ce_smooth_bwd(d)
    buf["gout"], buf["dl"], buf["labels_d"] = gout, dl, labels_d
    return d, buf


@functools.lru_cache(maxsize=None)
def smooth_case(dtype, shape, eps, weighted):
    """one run of the smoothed entry points, shared by the tests that only read its outputs"""
    return run_smooth(dtype, shape, eps, weighted)[1]


@functools.lru_cache(maxsize=None)
def plain_case(dtype, shape, weighted):
    """univl_vocab_ce_fwd / _bwd, or the weighted pair, on the same operands"""
    rows, V, seq_len, K = shape
    x, table, bias, labels, w = operands(dtype, shape)
    labels_d = labels.to(DEV)
    dl = torch.full((rows, (V + 7) // 8 * 8), FILL, device=DEV, dtype=dtype)
    gout = torch.tensor([GOUT], device=DEV)
    if weighted:
        d, buf = ops.vocab_ce_weighted_desc(x, table, bias, labels_d, dl, V, w.to(DEV), seq_len)
        ops.vocab_ce_weighted_fwd(d)
        d.gout = gout.data_ptr()
        ops.vocab_ce_weighted_bwd(d)
    else:
        d, buf = ops.vocab_ce_desc(x, table, bias, labels_d, dl, V)
        ops.vocab_ce_fwd(d)
        d.gout = gout.data_ptr()
        ops.vocab_ce_bwd(d)
    buf["dl"] = dl
    return buf


# ------------------------------------------------------------------------------------------------ 1. against fp64
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("eps", EPS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_smoothed_vocab_ce_matches_fp64_on_the_same_operands(dtype, shape, eps, weighted):
    V = shape[1]
    buf, ref = smooth_case(dtype, shape, eps, weighted), reference(dtype, shape, eps, weighted)
    err = dict(loss=abs(float(buf["loss"]) - float(ref["loss"])) / (abs(float(ref["loss"])) + 1e-30),
               rowloss=rel_err(buf["rowloss"], ref["rowloss"]), lse=rel_err(buf["lse"], ref["lse"]),
               dlogits=rel_err(buf["dl"][:, :V].float(), ref["dlogits"]))
    print("loss %.9g ref %.9g; " % (float(buf["loss"]), float(ref["loss"])) + " ".join("%s %.3g" % kv for kv in err.items()))
    assert float(buf["scratch"][0]) == float(ref["n_valid"])                    # n_valid: independent of weights and eps
    for name, e in err.items():
        assert e < tol(dtype), (name, e)


# ------------------------------------------------------------------------------------------------ 2. eps = 0
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_eps_zero_is_the_unsmoothed_entry_point_bit_for_bit(dtype, shape, weighted):
    got, want = smooth_case(dtype, shape, 0.0, weighted), plain_case(dtype, shape, weighted)
    for name in ("loss", "lse", "label_logit", "rowloss", "scratch", "dl"):
        assert torch.equal(got[name], want[name]), name


# ------------------------------------------------------------------------------------------------ 3. lse bits
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("eps", EPS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_lse_and_label_logit_are_the_unweighted_forwards_bits(dtype, shape, eps, weighted):
    got, want = smooth_case(dtype, shape, eps, weighted), plain_case(dtype, shape, False)
    assert torch.equal(got["lse"], want["lse"]) and torch.equal(got["label_logit"], want["label_logit"])
    assert torch.equal(got["scratch"][:1], want["scratch"][:1])


# ------------------------------------------------------------------------------------------------ 4. the uniform term
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("eps", EPS)
def test_uniform_term_is_on_every_column(eps, weighted):
    """The max-normalised gate cannot see eps / V (1e-4 of the largest entry at V = 1000).  d = (dlogits_eps - dlogits_0) / sc with
    sc = w_r gout / n_valid is -eps / V off the label and eps - eps / V on it, within 1e-6 absolute: each stored value is one fp32
    subtraction chain on numbers <= 1 and one product, a few ulps of 1 (~2e-7).  Rows sum to 0 within 1e-4."""
    dtype, shape = torch.float32, SMALL_V
    rows, V, seq_len, K = shape
    _, _, _, labels, w = operands(dtype, shape)
    a, b = smooth_case(dtype, shape, eps, weighted), smooth_case(dtype, shape, 0.0, weighted)
    n_valid = int((labels != -1).sum())
    wr = w.double().repeat_interleave(seq_len) if weighted else torch.ones(rows, dtype=torch.float64)
    live = (labels != -1) & (wr != 0)
    assert int(live.sum()) >= 20
    sc = (wr * GOUT / n_valid)[live][:, None]
    de, d0 = a["dl"][:, :V].double().cpu()[live], b["dl"][:, :V].double().cpu()[live]
    d = (de - d0) / sc
    hot = F.one_hot(labels[live], V).bool()
    off, on = (d[~hot] + eps / V).abs().max(), (d[hot] - (eps - eps / V)).abs().max()
    rowsum = (de / sc).sum(1).abs().max()
    print("off-label %.3g  label %.3g  row sums %.3g" % (float(off), float(on), float(rowsum)))
    assert float(off) < 1e-6 and float(on) < 1e-6
    assert float(rowsum) < 1e-4


# ------------------------------------------------------------------------------------------------ 5. exact zeros and bounds
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_ignored_and_zero_weight_rows_are_exact_zeros_and_padding_is_untouched(dtype, shape, weighted):
    rows, V, seq_len, K = shape
    buf = smooth_case(dtype, shape, 0.1, weighted)
    dl, rowloss = buf["dl"], buf["rowloss"]
    c = all_ignored_caption(rows // seq_len)
    dead = [slice(0, rows, 5), slice(c * seq_len, (c + 1) * seq_len)] + ([slice(0, seq_len)] if weighted else [])      # w[0] = 0
    for s in dead:
        assert float(dl[s, :V].float().abs().max()) == 0.0 and float(rowloss[s].abs().max()) == 0.0, s
    assert float(dl[seq_len:2 * seq_len, :V].float().abs().max()) > 0.0                                                    # w[1] = 1
    assert dl.shape[1] > V or V % 8 == 0
    if dl.shape[1] > V:
        assert float((dl[:, V:].float() - FILL).abs().max()) == 0.0


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
def test_no_counting_row_gives_nan_and_zero_gradient(weighted):
    shape = SMALL_V
    _, buf = run_smooth(torch.float32, shape, 0.1, weighted, labels=torch.full((shape[0],), -1, dtype=torch.int64))
    assert math.isnan(float(buf["loss"])) and float(buf["scratch"][0]) == 0.0
    assert float(buf["dl"][:, :shape[1]].abs().max()) == 0.0 and float(buf["rowloss"].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ 6. bit-reproducibility
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_two_runs_give_the_same_bits_and_rows_do_not_see_the_row_tile_count(dtype):
    shape = SHAPES[0]
    rows, V, seq_len, K = shape
    first = smooth_case(dtype, shape, 0.1, True)
    _, again = run_smooth(dtype, shape, 0.1, True)
    for name in ("loss", "lse", "label_logit", "rowloss", "scratch", "partial_sum", "dl"):
        assert torch.equal(first[name], again[name]), name
    # the same 130 rows as the first 130 of a 260-row problem (three row tiles instead of two)
    x, _, _, labels, w = operands(dtype, shape)
    x2 = torch.cat([x, gen(rows, K, seed=11).to(DEV, dtype)])
    labels2 = torch.cat([labels, torch.randint(0, V, (rows,), generator=torch.Generator().manual_seed(12))])
    w2 = torch.cat([w, torch.full((rows // seq_len,), 0.5)])
    _, big = run_smooth(dtype, shape, 0.1, True, labels=labels2, x=x2, w=w2)
    assert big["rowloss"].shape[0] == 2 * rows and float(big["rowloss"][rows:].abs().max()) > 0.0
    assert torch.equal(big["rowloss"][:rows], first["rowloss"]) and torch.equal(big["lse"][:rows], first["lse"])


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_smoothed_vocab_ce_refuses_what_the_header_excludes():
    shape = SMALL_V
    rows, V, seq_len, K = shape
    x, table, bias, labels, w = operands(torch.float32, shape)
    dl = torch.zeros(rows, V, device=DEV)
    labels_d, w_d = labels.to(DEV), w.to(DEV)
    for bad in (-0.1, 1.0, float("nan")):
        with pytest.raises((RuntimeError, ValueError)):
            d, _ = ops.vocab_ce_smooth_desc(x, table, bias, labels_d, dl, V, bad)
            ops.vocab_ce_smooth_fwd(d)
        d, _ = ops.vocab_ce_smooth_desc(x, table, bias, labels_d, dl, V, 0.1)
        d.smoothing = bad
        with pytest.raises(RuntimeError, match=r"\(-1\)"):                     # UNIVL_EINVAL
            ops.vocab_ce_smooth_fwd(d)
        with pytest.raises(RuntimeError, match=r"\(-1\)"):
            ops.vocab_ce_smooth_bwd(d)
    for eps in (0.0, 0.1):                                                     # a seq_len that does not divide rows, weights given
        d, _ = ops.vocab_ce_smooth_desc(x, table, bias, labels_d, dl, V, eps, torch.ones(rows, device=DEV), 7)
        with pytest.raises(RuntimeError, match=r"\(-1\)"):
            ops.vocab_ce_smooth_fwd(d)
        with pytest.raises(RuntimeError, match=r"\(-1\)"):
            ops.vocab_ce_smooth_bwd(d)
    d, _ = ops.vocab_ce_smooth_desc(x, table, bias, labels_d, dl, V, 0.1, w_d, seq_len)
    d.partial_sum = None
    with pytest.raises(RuntimeError, match=r"\(-1\)"):
        ops.vocab_ce_smooth_fwd(d)
    with pytest.raises(RuntimeError, match=r"\(-1\)"):
        ops.vocab_ce_smooth_bwd(d)
    d.smoothing = 0.0                                                          # eps = 0 does not look at partial_sum
    ops.vocab_ce_smooth_fwd(d)
    d, _ = ops.vocab_ce_smooth_desc(x, table, bias, labels_d, dl, V, 0.1)      # without weights seq_len is not looked at
    d.seq_len = 7
    ops.vocab_ce_smooth_fwd(d)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 8. through the model
@pytest.fixture
def deterministic_mode():
    was = univl_amd.deterministic()
    univl_amd.set_deterministic(True)
    yield
    univl_amd.set_deterministic(was)


BIAS = "decoder.classifier.cls.predictions.bias"


def _smoothed_reference(logits, labels, wr, eps):
    """float64: the smoothed loss sum_r w_r ce_r / n_valid and d loss / d bias = sum_r w_r (softmax_r - q_r) / n_valid"""
    lg = logits.double().cpu().requires_grad_(True)
    labels = labels.cpu().view(-1)
    n_valid = int((labels != -1).sum())
    ce = F.cross_entropy(lg, labels, ignore_index=-1, label_smoothing=eps, reduction="none")
    loss = (wr.double().cpu() * ce).sum() / n_valid
    loss.backward()
    return float(loss.detach()), lg.grad.sum(0)


def _check_loss_and_bias_gradient(tag, model, loss, ref_loss, ref_gbias, G):
    got = dict(model.named_parameters())[BIAS].grad.double().cpu()
    err = dict(loss=abs(float(loss) - ref_loss) / max(1.0, abs(ref_loss)),
               gnorm=abs(float(got.norm()) - float(ref_gbias.norm())) / float(ref_gbias.norm()),
               gsample=float((got - ref_gbias).norm() / ref_gbias.norm()))
    print("[%s] loss %.7f ref %.7f " % (tag, float(loss), ref_loss) + " ".join("%s=%.2e" % kv for kv in sorted(err.items())))
    for k, v in err.items():
        assert v < G[k], (tag, k, v, G[k])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_caption_label_smoothing_through_the_model(dtype, deterministic_mode):
    eps = 0.1
    cfg, rows, dseed = case_config("caption_small")
    model, _ = build(cfg, dtype)                                               # dropout 0
    G = gates_for("caption_small", dtype)
    batch = O.synthetic_batch(cfg, rows, seed=dseed)
    b = {k: v.to(DEV) for k, v in batch.items()}
    B, Wd = rows, cfg.max_words
    assert model.caption_label_smoothing == 0.0
    model.train()
    base = call(model, batch).detach().clone()
    assert "univl_vocab_ce_fwd" in plan_ops(model) and "univl_vocab_ce_smooth_fwd" not in plan_ops(model)
    # ---- the logits of the same inputs, from the evaluation surface
    model.eval()
    with torch.no_grad():
        seq, vis = model.get_sequence_visual_output(b["input_ids"], b["token_type_ids"], b["attention_mask"], b["video"], b["video_mask"])
        logits = model.decoder_caption(seq, vis, b["input_ids"], b["attention_mask"], b["video_mask"], b["input_caption_ids"],
                                       b["decoder_mask"], shaped=False, get_logits=True).float().reshape(B * Wd, -1).clone()
        # two captions per video: the batch's own and those of another seed
        other = O.synthetic_batch(cfg, rows, seed=dseed + 10)
        stack = lambda key: torch.stack([batch[key].view(B, Wd), other[key].view(B, Wd)], dim=1).contiguous().to(DEV)
        ids2, mask2, lab2 = stack("input_caption_ids"), stack("decoder_mask"), stack("output_caption_ids")
        rep = lambda t: t.repeat_interleave(2, dim=0)
        logits2 = model.decoder_caption(rep(seq), rep(vis), rep(b["input_ids"]), rep(b["attention_mask"]), rep(b["video_mask"]),
                                        ids2.view(B * 2, Wd), mask2.view(B * 2, Wd), shaped=False,
                                        get_logits=True).float().reshape(B * 2 * Wd, -1).clone()
    model.train()
    # ---- caption step
    model.caption_label_smoothing = eps
    loss = call(model, batch)
    loss.backward()
    ran = plan_ops(model)
    assert "univl_vocab_ce_smooth_fwd" in ran and "univl_vocab_ce_smooth_bwd" in ran and "univl_vocab_ce_fwd" not in ran
    ref_loss, ref_g = _smoothed_reference(logits, batch["output_caption_ids"], torch.ones(B * Wd), eps)
    _check_loss_and_bias_gradient("caption eps=%g %s" % (eps, dtype), model, loss, ref_loss, ref_g, G)
    assert abs(float(loss) - float(base)) > 1e-3                               # the smoothed loss is another number
    # ---- caption_weighted step, n_cand = 2
    model.zero_grad(set_to_none=True)
    w = torch.tensor([[1.5, -0.75], [0.5, 2.0]])[:B].to(DEV) if B <= 2 else (torch.arange(B * 2).view(B, 2).float() / B - 0.6).to(DEV)
    lw = model(b["input_ids"], b["token_type_ids"], b["attention_mask"], b["video"], b["video_mask"], input_caption_ids=ids2,
               decoder_mask=mask2, output_caption_ids=lab2, caption_weight=w)
    lw.backward()
    ref_loss, ref_g = _smoothed_reference(logits2, lab2, w.view(-1).repeat_interleave(Wd), eps)
    _check_loss_and_bias_gradient("caption_weighted eps=%g %s" % (eps, dtype), model, lw, ref_loss, ref_g, G)
    # ---- back to 0: the unsmoothed plans, the unsmoothed bits
    model.zero_grad(set_to_none=True)
    model.caption_label_smoothing = 0.0
    again = call(model, batch)
    assert torch.equal(again.detach(), base)
    assert "univl_vocab_ce_smooth_fwd" not in plan_ops(model)


def test_pretrain_mlm_term_does_not_see_the_property(deterministic_mode):
    cfg, rows, dseed = case_config("pretrain_small")
    model, _ = build(cfg, torch.float32)
    batch = O.synthetic_batch(cfg, rows, seed=dseed)
    model.train()
    step = lambda: next(st for st in model._steps.values() if getattr(st, "kind", None) == "pretrain")
    l0 = call(model, batch).detach().clone()
    mlm0, dec0 = step().heads.mlm.loss.clone(), step().decoder.loss.clone()
    model.caption_label_smoothing = 0.1
    l1 = call(model, batch).detach().clone()
    mlm1, dec1 = step().heads.mlm.loss.clone(), step().decoder.loss.clone()
    ran = plan_ops(model)
    assert "univl_vocab_ce_fwd" in ran and "univl_vocab_ce_smooth_fwd" in ran             # the MLM head / the decoder's head
    assert torch.equal(mlm0, mlm1)
    assert not torch.equal(dec0, dec1) and not torch.equal(l0, l1)
    assert np.isfinite(float(l1))
