"""Micro-benchmark of reward-weighted caption training (csrc/vocab_ce.h: univl_vocab_ce_weighted_fwd / _bwd; csrc/metric.hip:
univl_caption_advantage; steps.py: the caption_weighted step; univl_amd/rl.py).

    python scripts/mb_caption_rl.py [--rounds 3] [--out profiles/caption_rl.txt]

One process, alternating rounds (A, B, A, B, ...); every comparand is the existing unweighted code in the same process.  Times are
milliseconds per call between two HIP events around back-to-back calls (enqueue cost included).  Each table ends with the
round-to-round spread, (max - min) / median of a row's rounds: a difference between two rows below it is not a difference.

  (a) K16 forward + backward at 512 rows x 30522 (4 captions of 128 positions), bf16 and fp32: weighted against unweighted;
  (b) the training step (forward + backward) at the cfg4 shape (4 videos, 128 words, 96 frames, full depth), bf16: the existing
      `caption` step against `caption_weighted` with n_cand = 1 and weights of 1 (the same arithmetic, bit for bit);
  (c) `caption_weighted` with n_cand = 5 at the same shape;
  (d) a whole scst_step + backward at 16 videos x 5 samples x 32 positions (32 words, 96 frames, full depth), and its parts: sample
      (encoder features + CaptionSampler.sample), reward + advantage, train (teacher-forcing tensors + forward + backward)."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)
import univl_oracle as O  # noqa: E402
from univl_amd import UniVL, ops, rl  # noqa: E402
from univl_amd.sample import CaptionSampler  # noqa: E402
from univl_amd.score import beam_inputs_labels  # noqa: E402

DEV = "cuda"


def events(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def table(title, runs, rounds, calls, lines):
    for fn in runs.values():
        events(fn, 4)                       # warm: plans built, graphs captured
    torch.cuda.synchronize()
    times = {k: [] for k in runs}
    for _ in range(rounds):
        for name, fn in runs.items():
            times[name].append(events(fn, calls))
    lines.append("")
    lines.append(title)
    lines.append("%44s %s %10s %8s" % ("", " ".join("%9s" % ("round %d" % (i + 1)) for i in range(rounds)), "median", "spread"))
    for name, ts in times.items():
        med = statistics.median(ts)
        lines.append("%44s %s %10.4f %7.1f%%" % (name, " ".join("%9.4f" % t for t in ts), med, 100.0 * (max(ts) - min(ts)) / med))
    return {k: statistics.median(v) for k, v in times.items()}


def kernels(rounds, lines):
    rows, V, K, seq_len = 512, 30522, 768, 128
    ldv = (V + 7) // 8 * 8
    g = torch.Generator().manual_seed(0)
    labels = torch.randint(0, V, (rows,), generator=g)
    labels[::5] = -1
    labels = labels.to(DEV)
    w = (torch.rand(rows // seq_len, generator=g) * 4 - 2).to(DEV)
    gout = torch.ones(1, device=DEV)
    runs, keep = {}, []
    for dtype, tag in ((torch.bfloat16, "bf16"), (torch.float32, "fp32")):
        x = torch.randn(rows, K, generator=g).to(DEV, dtype)
        tab = (torch.randn(V, K, generator=g) * 0.06).to(DEV, dtype)
        bias = (torch.randn(V, generator=g) * 0.5).to(DEV)
        dl = torch.zeros(rows, ldv, device=DEV, dtype=dtype)
        du, bu = ops.vocab_ce_desc(x, tab, bias, labels, dl, V)
        dw, bw = ops.vocab_ce_weighted_desc(x, tab, bias, labels, dl, V, w, seq_len)
        du.gout = dw.gout = gout.data_ptr()
        keep += [bu, bw]
        runs["%s unweighted fwd + bwd" % tag] = lambda d=du: (ops.vocab_ce_fwd(d), ops.vocab_ce_bwd(d))
        runs["%s weighted fwd + bwd" % tag] = lambda d=dw: (ops.vocab_ce_weighted_fwd(d), ops.vocab_ce_weighted_bwd(d))
    return table("(a) K16 forward + backward, %d rows x %d, seq_len %d" % (rows, V, seq_len), runs, rounds, 20, lines)


def model_for(batch_size, max_words, max_frames):
    cfg = O.OracleConfig(batch_size=batch_size, stage_two=True, task_type="caption", max_words=max_words, max_frames=max_frames)
    ns = argparse.Namespace(**cfg.to_dict(), local_rank=0, compute_dtype="bf16")
    ns.dropout_prob = 0.0
    model = UniVL.from_pretrained("bert-base-uncased", "visual-base", "cross-base", "decoder-base", task_config=ns)
    P = O.procedural_params(cfg, 0)
    sd = dict(P)
    for alias, owner in O.tied_aliases(cfg).items():          # a state_dict lists tied tensors under both keys
        sd[alias] = P[owner]
    model.load_state_dict(sd)
    model.to(DEV).train()
    batch = {k: v.to(DEV) for k, v in O.synthetic_batch(cfg, batch_size, seed=3104).items()}
    return cfg, model, batch


def steps(rounds, lines):
    cfg, model, b = model_for(4, 128, 96)
    B, Wd = 4, cfg.max_words
    enc = (b["input_ids"], b["token_type_ids"], b["attention_mask"], b["video"], b["video_mask"])
    caps = lambda nc: dict(input_caption_ids=b["input_caption_ids"].view(B, 1, Wd).repeat(1, nc, 1).contiguous(),
                           decoder_mask=b["decoder_mask"].view(B, 1, Wd).repeat(1, nc, 1).contiguous(),
                           output_caption_ids=b["output_caption_ids"].view(B, 1, Wd).repeat(1, nc, 1).contiguous())
    one, five = caps(1), caps(5)
    w1, w5 = torch.ones(B, 1, device=DEV), (torch.rand(B, 5, device=DEV) * 2 - 1)
    plain = dict(input_caption_ids=b["input_caption_ids"], decoder_mask=b["decoder_mask"], output_caption_ids=b["output_caption_ids"])

    def step(kw):
        model(*enc, **kw).backward()
        model.zero_grad(set_to_none=True)
    runs = {"caption step": lambda: step(plain), "caption_weighted, n_cand = 1": lambda: step(dict(one, caption_weight=w1)),
            "caption_weighted, n_cand = 5": lambda: step(dict(five, caption_weight=w5))}
    return table("(b), (c) forward + backward at the cfg4 shape (4 videos x 128 words x 96 frames, bf16)", runs, rounds, 20, lines)


def scst(rounds, lines):
    n, ns, T = 16, 5, 32
    cfg, model, b = model_for(n, T, 96)
    enc = (b["input_ids"], b["token_type_ids"], b["attention_mask"], b["video"], b["video_mask"])
    smp = CaptionSampler(model, n, cfg.max_words, cfg.max_frames, n_samp=ns, max_len=T, top_k=50)
    g = torch.Generator().manual_seed(1)
    ref_ids = torch.randint(1000, 1400, (n, 2, T), generator=g).to(DEV)
    ref_len = torch.randint(4, T + 1, (n, 2), generator=g).to(DEV)
    bos, eos, pad, state = 101, 102, 0, {}

    def sample():
        with torch.no_grad():
            seq, vis = model.get_sequence_visual_output(*enc)
            state["res"] = smp.sample(seq, vis, b["attention_mask"].view(n, -1), b["video_mask"].view(n, -1), bos, eos, 7)

    def reward():
        state["adv"] = rl.advantages(rl.caption_rewards(state["res"], ref_ids, ref_len, eos, pad))

    def train():
        res = state["res"]
        inputs, labels, mask = beam_inputs_labels(res.tokens, res.lengths, bos, eos, pad, T)
        model(*enc, input_caption_ids=inputs, decoder_mask=mask, output_caption_ids=labels, caption_weight=state["adv"]).backward()
        model.zero_grad(set_to_none=True)

    def whole():
        rl.scst_step(model, smp, b, ref_ids, ref_len, bos, eos, pad, seed=7).loss.backward()
        model.zero_grad(set_to_none=True)
    sample(), reward()
    runs = {"sample (features + %d positions)" % T: sample, "reward + advantage": reward, "train (forward + backward)": train,
            "scst_step + backward": whole}
    return table("(d) scst_step at %d videos x %d samples x %d positions (bf16)" % (n, ns, T), runs, rounds, 5, lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="profiles/caption_rl.txt")
    a = ap.parse_args()
    lines = ["reward-weighted caption training on %s; milliseconds per call, alternating rounds" % torch.cuda.get_device_name(0)]
    kernels(a.rounds, lines)
    steps(a.rounds, lines)
    scst(a.rounds, lines)
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
