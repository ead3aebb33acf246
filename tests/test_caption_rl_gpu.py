"""Reward-weighted caption training on the device: univl_caption_advantage (csrc/metric.hip), the "caption_weighted" training step
behind UniVL.forward(caption_weight=...), and univl_amd.rl (caption_rewards, advantages, scst_step).  Needs a real MI355X (`-m gpu`).

  (i)   the advantage kernel against the numpy fp64 restatement of tests/test_caption_rl_cpu.py, bit for bit;
  (ii)  the step at n_cand = 1 with weights of 1 against the existing `caption` step: loss and every gradient, bit for bit;
  (iii) the step at B = 2, n_cand = 3 with mixed-sign weights against the oracle (loss formed here from its decoder logits, gradients
        by autograd) under the gates tests/test_model_gpu.py applies to caption_small (gates_for("caption_small", dtype),
        compare_gradients, check_gates); accumulation and clip + BertAdam.step() + the next forward on top;
  (iv)  caption_rewards against the dictionary restatement of tests/test_caption_metrics_cpu.py (item_stats);
  (v)   scst_step on the toy model."""
import functools

import numpy as np
import pytest
import torch

import univl_oracle as O
from make_golden import case_config, sample_exact
from test_caption_metrics_cpu import item_stats
from test_caption_rl_cpu import advantage_restated

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import univl_amd
    from univl_amd import BertAdam, clip_grad_norm_, _lib, ops, rl
    from univl_amd.sample import CaptionSampler, SampleResult
    from test_model_gpu import build, call, check_gates, compare_gradients, gates_for

DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16]
IDS = ["fp32", "bf16"]
SCORE_GATE_FP32 = 2e-4          # tests/test_score_gpu.py: GATE[torch.float32], error / max(1, max |ref|)


@pytest.fixture(autouse=True)
def _deterministic_mode():
    was = univl_amd.deterministic()
    univl_amd.set_deterministic(True)
    yield
    univl_amd.set_deterministic(was)


# ------------------------------------------------------------------------------------------------ (i) the advantage kernel
def _rewards(n, ns, seed):
    return np.random.RandomState(seed).uniform(0.0, 1.0, size=(n, ns))


@pytest.mark.parametrize("n,ns", [(1, 2), (3, 5), (16, 64)])
def test_advantage_kernel_is_the_restatement_bit_for_bit(n, ns):
    r = _rewards(n, ns, 7 + n)
    b = np.random.RandomState(11).uniform(0.0, 1.0, size=n)
    rd = torch.from_numpy(r).to(DEV)
    for scale in (1.0, -0.37):
        w, st = ops.caption_advantage(rd, None, scale)
        want, flag = advantage_restated(r, None, scale)
        assert w.dtype == torch.float32 and np.array_equal(w.cpu().numpy().view(np.uint32), want.view(np.uint32)) and int(st) == flag == 0
        w, st = ops.caption_advantage(rd, torch.from_numpy(b).to(DEV), scale)
        want, flag = advantage_restated(r, b, scale)
        assert np.array_equal(w.cpu().numpy().view(np.uint32), want.view(np.uint32)) and int(st) == flag == 0
    assert torch.equal(rl.advantages(rd), ops.caption_advantage(rd)[0])
    assert torch.equal(rl.advantages(rd, torch.from_numpy(b).to(DEV), 2.0), ops.caption_advantage(rd, torch.from_numpy(b).to(DEV), 2.0)[0])


def test_advantage_kernel_never_hands_on_a_non_finite_reward():
    r = _rewards(3, 5, 3)
    r[1, 2], r[2, 0] = np.nan, np.inf
    b = np.array([0.5, 0.25, 0.125])
    for base in (None, b):
        w, st = ops.caption_advantage(torch.from_numpy(r).to(DEV), None if base is None else torch.from_numpy(base).to(DEV))
        want, flag = advantage_restated(r, base, 1.0)
        got = w.cpu().numpy()
        assert np.isfinite(got).all() and got[1, 2] == 0.0 and got[2, 0] == 0.0 and int(st) & _lib.ADV_NONFINITE and flag == 1
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert np.count_nonzero(got) == 13                                     # every other sample keeps a weight
    bn = b.copy()
    bn[0] = np.nan
    w, st = ops.caption_advantage(torch.from_numpy(_rewards(3, 5, 3)).to(DEV), torch.from_numpy(bn).to(DEV))
    assert int(st) == 1 and float(w[0].abs().max()) == 0.0 and float(w[1].abs().min()) > 0.0
    status = torch.zeros(1, dtype=torch.int32, device=DEV)                     # a caller's status word: OR-ed into, not overwritten
    ops.caption_advantage(torch.from_numpy(_rewards(3, 5, 3)).to(DEV), status=status)
    assert int(status) == 0
    ops.caption_advantage(torch.from_numpy(r).to(DEV), status=status)
    ops.caption_advantage(torch.from_numpy(_rewards(3, 5, 3)).to(DEV), status=status)
    assert int(status) == 1


def test_advantage_kernel_argument_range():
    one = torch.zeros(4, 1, dtype=torch.float64, device=DEV)
    with pytest.raises(RuntimeError, match=r"\(-1\)"):                         # UNIVL_EINVAL: the leave-one-out mean of one sample
        ops.caption_advantage(one)
    w, st = ops.caption_advantage(one + 0.75, torch.full((4,), 0.25, dtype=torch.float64, device=DEV))
    assert w.tolist() == [[0.5]] * 4 and int(st) == 0


# ------------------------------------------------------------------------------------------------ the step
def _weighted_call(model, b, ids, mask, lab, w):
    return model(b["input_ids"], b["token_type_ids"], b["attention_mask"], b["video"], b["video_mask"],
                 input_caption_ids=ids, decoder_mask=mask, output_caption_ids=lab, caption_weight=w)


def _grads(model):
    return {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_one_caption_of_weight_one_is_the_caption_step_bit_for_bit(dtype):
    cfg, rows, dseed = case_config("caption_small")
    model, _ = build(cfg, dtype)
    batch = O.synthetic_batch(cfg, rows, seed=dseed)
    b = {k: v.to(DEV) for k, v in batch.items()}
    model.train()
    loss = call(model, batch)
    loss.backward()
    base_loss, base = loss.detach().clone(), _grads(model)
    model.zero_grad(set_to_none=True)
    B, Wd = rows, cfg.max_words
    lw = _weighted_call(model, b, b["input_caption_ids"].view(B, 1, Wd), b["decoder_mask"].view(B, 1, Wd),
                        b["output_caption_ids"].view(B, 1, Wd), torch.ones(B, 1, device=DEV))
    lw.backward()
    got = _grads(model)
    assert torch.equal(lw.detach(), base_loss)
    assert set(got) == set(base)
    for n in base:
        assert torch.equal(got[n], base[n]), n
    kinds = sorted(st.kind for st in model._steps.values() if hasattr(st, "kind"))
    assert kinds == ["caption", "caption_weighted"]


@functools.lru_cache(maxsize=None)
def _oracle_case():
    """B = 2 videos x n_cand = 3 captions of caption_small with mixed-sign weights (one 0): the batch, the captions, the weights and the
    oracle's loss sum w nll / n_valid with its gradients (autograd), computed once."""
    cfg, rows, dseed = case_config("caption_small")
    B, nc, Wd = rows, 3, cfg.max_words
    batch = O.synthetic_batch(cfg, B, seed=dseed)
    caps = [O.synthetic_batch(cfg, B, seed=dseed + 10 * k) for k in range(nc)]
    stack = lambda key: torch.stack([c[key].view(B, Wd) for c in caps], dim=1).contiguous()        # [B, nc, Wd]
    ids, mask, lab = stack("input_caption_ids"), stack("decoder_mask"), stack("output_caption_ids")
    lab = torch.where(mask > 0, lab, torch.full_like(lab, -1))                 # positions past a caption's end do not count
    w = torch.tensor([[1.5, -0.75, 0.0], [-1.0, 0.5, 2.0]])
    P = O.procedural_params(cfg, 0)
    Pr = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    rep = {k: (v.repeat_interleave(nc, dim=0) if torch.is_tensor(v) and v.shape[0] == B else v) for k, v in batch.items()}
    rep["input_caption_ids"], rep["decoder_mask"], rep["output_caption_ids"] = ids.view(B * nc, Wd), mask.view(B * nc, Wd), lab.view(B * nc, Wd)
    _, parts = O.univl_forward(Pr, cfg, rep, training=True, return_parts=True)
    logits = parts["decoder_scores"].view(B * nc * Wd, -1)
    labels = lab.view(-1)
    counts = labels != -1
    nll = torch.logsumexp(logits[counts], -1) - logits[counts, labels[counts]]
    ref = (w.view(-1).repeat_interleave(Wd)[counts] * nll).sum() / int(counts.sum())
    ref.backward()
    names = [n for n in P if Pr[n].grad is not None]
    grads = [Pr[n].grad for n in names]
    norms = np.array([float(g.double().norm()) for g in grads])
    top = np.argsort(-norms)[:10]
    fixture = dict(names=names, norms=norms, samples=[sample_exact(g.float(), 256) for g in grads], top=top,
                   top_samples=[sample_exact(grads[int(i)].float(), 4096) for i in top], nograd=[n for n in P if Pr[n].grad is None])
    return cfg, batch, (ids, mask, lab, w), float(ref), fixture


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_weighted_step_against_the_oracle(dtype):
    cfg, batch, (ids, mask, lab, w), ref, fx = _oracle_case()
    model, _ = build(cfg, dtype)
    model.train()
    b = {k: v.to(DEV) for k, v in batch.items()}
    dev = lambda t: t.to(DEV)
    G, f32 = gates_for("caption_small", dtype), dtype == torch.float32
    loss = _weighted_call(model, b, dev(ids), dev(mask), dev(lab), dev(w))
    loss.backward()
    params = dict(model.named_parameters())
    for n in fx["nograd"]:
        if n in params:
            assert params[n].grad is None, n
    err, bad = compare_gradients(params, fx["names"], fx["norms"], fx["samples"], fx["top"], fx["top_samples"], G, f32)
    err["loss"] = abs(float(loss) - ref) / max(1.0, abs(ref))
    print("[caption_weighted vs oracle %s] loss %.6f ref %.6f " % (dtype, float(loss), ref) + " ".join("%s=%.2e" % kv for kv in sorted(err.items())))
    assert not bad, bad[:5]
    check_gates("caption_weighted", err, G)
    # ---- a second backward without clearing the gradients doubles them
    g1 = _grads(model)
    _weighted_call(model, b, dev(ids), dev(mask), dev(lab), dev(w)).backward()
    doubled = [(2.0 * np.asarray(x)) for x in fx["samples"]]
    err2, bad2 = compare_gradients(params, fx["names"], 2.0 * fx["norms"], doubled, fx["top"], [2.0 * np.asarray(x) for x in fx["top_samples"]], G, f32)
    assert not bad2, bad2[:5]
    check_gates("caption_weighted x2", err2, G)
    for n, g in g1.items():
        assert float((params[n].grad - 2.0 * g).abs().max()) <= 1e-5 + 1e-4 * float(g.abs().max()), n
    # ---- clip + one BertAdam.step() + the next forward, with the update pending in between
    opt = BertAdam([{"params": [p for p in model.parameters()]}], lr=1e-5, warmup=-1, t_total=-1, weight_decay=0.01, max_grad_norm=1.0)
    total = clip_grad_norm_(model.parameters(), 1.0)
    opt.step()
    opt.zero_grad()
    nxt = _weighted_call(model, b, dev(ids), dev(mask), dev(lab), dev(w))
    nxt.backward()
    torch.cuda.synchronize()
    assert np.isfinite(float(total)) and np.isfinite(float(nxt)) and float(nxt) != float(loss)


# ------------------------------------------------------------------------------------------------ (iv) caption_rewards
def _crafted_samples():
    """n = 3 videos x 4 samples over 7 symbols, lengths 1 .. 40, 2 references per video; sample (0, 1) equals reference (0, 0), sample
    (1, 2) is empty."""
    rng = np.random.RandomState(12)
    n, ns, n_ref, T = 3, 4, 2, 40
    slen = rng.randint(1, T + 1, size=(n, ns))
    rlen = rng.randint(1, T + 1, size=(n, n_ref))
    slen[0, 0], slen[2, 3], rlen[1, 1], rlen[2, 0] = 1, T, 1, T
    tok = rng.randint(0, 7, size=(n, ns, T)).astype(np.int32)
    ref = rng.randint(0, 7, size=(n, n_ref, T)).astype(np.int64)
    slen[0, 1] = rlen[0, 0]
    tok[0, 1] = ref[0, 0]
    slen[1, 2] = 0
    for i in range(n):
        for s in range(ns):
            tok[i, s, slen[i, s]:] = -1
    return tok, slen.astype(np.int32), ref, rlen.astype(np.int64)


def _as_result(tok, slen):
    t = torch.from_numpy(tok).to(DEV)
    z = torch.zeros(t.shape, device=DEV)
    return SampleResult(t, z, z.clone(), z[..., 0].clone(), z[..., 0].clone(), torch.from_numpy(slen).to(DEV))


@pytest.mark.parametrize("metric", ["rouge_l", "bleu"])
def test_caption_rewards_against_the_dictionary_restatement(metric):
    tok, slen, ref, rlen = _crafted_samples()
    n, ns, T = tok.shape
    res = _as_result(tok, slen)
    r, o = rl.caption_rewards(res, torch.from_numpy(ref).to(DEV), torch.from_numpy(rlen).to(DEV), eos=-1, pad=-1, metric=metric,
                              return_stats=True)
    assert r.shape == (n, ns) and r.dtype == torch.float64 and r.is_cuda and int(o["status"]) == 0
    got = r.cpu().numpy()
    for i in range(n):
        refs = [ref[i, k, :rlen[i, k]].tolist() for k in range(ref.shape[1])]
        for s in range(ns):
            it = item_stats(tok[i, s, :slen[i, s]].tolist(), refs)
            k = i * ns + s
            assert o["guess"][k].tolist() == it["guess"] and o["correct"][k].tolist() == it["correct"], (i, s)
            assert int(o["hyp_len"][k]) == it["hyp_len"] and int(o["ref_len"][k]) == it["ref_len"]
            assert o["lcs"][k * 2:k * 2 + 2].tolist() == it["lcs"]
            want = it[metric]
            assert abs(got[i, s] - want) <= 1e-12 * max(abs(want), 1e-300) or got[i, s] == want, (i, s, got[i, s], want)
    assert got[0, 1] > 0.99 and got[1, 2] == 0.0                               # the copy of a reference; the empty sample
    assert torch.equal(rl.caption_rewards(res, torch.from_numpy(ref).to(DEV), torch.from_numpy(rlen).to(DEV), -1, -1, metric=metric), r)


# ------------------------------------------------------------------------------------------------ (v) scst_step
BOS, T_RUN = 101, 6


@functools.lru_cache(maxsize=None)
def _toy():
    cfg, _, _ = case_config("caption_small")
    model, _ = build(cfg, torch.float32)
    model.train()
    n = 3
    batch = {k: v.to(DEV) for k, v in O.synthetic_batch(cfg, n, seed=31).items()}
    smp = CaptionSampler(model, n, cfg.max_words, cfg.max_frames, n_samp=4, max_len=T_RUN, top_k=20, temperature=1.3, top_p=0.95)
    return cfg, model, batch, smp


def test_scst_step_on_the_toy_model():
    cfg, model, batch, smp = _toy()
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    with torch.no_grad():
        seq, vis = model.get_sequence_visual_output(batch["input_ids"], batch["token_type_ids"], batch["attention_mask"], batch["video"],
                                                    batch["video_mask"])
        free = smp.sample(seq, vis, batch["attention_mask"].view(3, -1), batch["video_mask"].view(3, -1), BOS, -1, 9)
    eos = int(free.tokens.reshape(-1, T_RUN)[1, 2])                            # an end token that stops some rows early
    # references that share pieces with the samples: the first two free-running samples of every video, the second cut to 4 pieces
    ref_ids = free.tokens[:, :2].to(torch.int64).contiguous()
    ref_len = torch.tensor([[T_RUN, 4]] * 3, device=DEV)
    out = rl.scst_step(model, smp, batch, ref_ids, ref_len, BOS, eos, 0, seed=9)
    n, ns = 3, 4
    assert out.rewards.shape == out.advantages.shape == out.lengths.shape == (n, ns)
    assert out.rewards.dtype == torch.float64 and out.advantages.dtype == torch.float32 and out.rewards.is_cuda and out.advantages.is_cuda
    assert len(set(out.lengths.reshape(-1).tolist())) > 1
    # ---- the advantages are advantages(caption_rewards(...)) of the returned samples, bit for bit
    again = rl.advantages(rl.caption_rewards(out.samples, ref_ids, ref_len, eos, 0))
    assert torch.equal(again, out.advantages) and torch.equal(rl.caption_rewards(out.samples, ref_ids, ref_len, eos, 0), out.rewards)
    assert float(out.advantages.abs().max()) > 0.0
    # ---- the loss is the weighted loss of the sampler's own token log-probabilities (teacher forcing, dropout 0)
    tlp = out.samples.token_logprobs.double().cpu()
    n_valid = int(out.lengths.sum())
    want = float((out.advantages.double().cpu()[..., None] * -tlp).sum() / n_valid)
    size = float((out.advantages.double().cpu().abs()[..., None] * tlp.abs()).sum() / n_valid)
    print("[scst] loss %.7f from token_logprob %.7f (size of the summed terms %.4f); lengths %s" % (float(out.loss), want, size,
                                                                                                   out.lengths.tolist()))
    assert abs(float(out.loss) - want) <= SCORE_GATE_FP32 * max(1.0, size)
    out.loss.backward()
    grads = _grads(model)
    assert grads and all(bool(torch.isfinite(g).all()) for g in grads.values())
    assert all(float(grads[k].abs().max()) > 0.0 for k in ("bert.embeddings.word_embeddings.weight", "decoder.classifier.cls.predictions.bias",
                                                           "visual.embeddings.word_embeddings.weight"))
    first = out.loss.detach().clone()
    # ---- the same seed on the same parameters: the same bits
    model.zero_grad(set_to_none=True)
    for nme, p in model.named_parameters():
        assert torch.equal(p.detach(), before[nme]), nme
    rep = rl.scst_step(model, smp, batch, ref_ids, ref_len, BOS, eos, 0, seed=9)
    assert torch.equal(rep.loss.detach(), first) and torch.equal(rep.samples.tokens, out.samples.tokens)
    other = rl.scst_step(model, smp, batch, ref_ids, ref_len, BOS, eos, 0, seed=10)
    assert not torch.equal(other.samples.tokens, out.samples.tokens)
