"""One fixed, seeded toy case through every caption session -- decode.CaptionBeamSearch, sample.CaptionSampler, score.CaptionScorer --
with every result tensor and every plan's launch names written to an .npz: run it once per version of the Python layer, each in a
fresh process on the same library, and compare the files bit for bit.

    python scripts/ab_decode_sessions.py --dump FILE.npz
    python scripts/ab_decode_sessions.py --compare A.npz B.npz      (exit status 1 on any difference)

Shapes: 3 instances, W = F = 8, 4 rows per instance, 6 positions -- a partial batch (n_active = 2), two groups of two beams, a reorder at
every position.  The toy model (1 text / 1 video / 1 cross / 2 decoder layers on procedural weights) and its features are built as
tests/test_sample_gpu.py and tests/test_constrain_gpu.py build theirs, restated here so that the script runs on a tree without them.
Deterministic mode, fp32 and bf16.  Per dtype:
  beam search (n_best = 4): full batch, the same session with n_active = 2, the full batch again -- for beam_step="device", "host", with
      DecodeConstraints(2, 3, two suppressed ids), and with beam_groups=2, diversity_penalty=0.5 (n_best = 2 per group); captions() of each;
  CaptionSampler.sample (seed 7, top_k = 8), with and without the constraints, full then n_active = 2; step_logits at positions 0 and 1;
  CaptionScorer.score at n_cand = 1 and 3, full and partial; score_beams on the first three hypotheses of the plain result.
Only public entry points and the `steps` / plan dictionaries are used."""
import argparse
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, W, F, ROWS, T, WD, BOS = 3, 8, 8, 4, 6, 8, 101


def dump(path):
    for p in (ROOT, os.path.join(ROOT, "oracle")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch
    import univl_amd
    import univl_oracle as O
    from univl_amd import UniVL
    from univl_amd.constrain import DecodeConstraints
    from univl_amd.decode import CaptionBeamSearch
    from univl_amd.sample import CaptionSampler
    from univl_amd.score import CaptionScorer
    dev = "cuda"
    univl_amd.set_deterministic(True)
    out, plans = {}, {}

    def keep(prefix, obj, fields):
        torch.cuda.synchronize()
        for f in fields:
            t = (obj[f] if isinstance(obj, dict) else getattr(obj, f)).detach().cpu()
            out[prefix + "." + f] = (t.view(torch.int16) if t.dtype == torch.bfloat16 else t).numpy()

    def keep_plans(prefix, ses):
        """the once-per-batch plan (named `setup` or `plan`, whichever the tree has) and every position's plan, by sorted key"""
        named = {"batch": ses.setup if hasattr(ses, "setup") else ses.plan}
        named.update({repr(k): pl for k, pl in getattr(ses, "steps", {}).items()})
        plans[prefix] = [[k, [op.name for op in named[k].ops]] for k in sorted(named)]

    def toy(dtype):
        cfg = O.OracleConfig(batch_size=N, text_num_hidden_layers=1, visual_num_hidden_layers=1, cross_num_hidden_layers=1,
                             decoder_num_hidden_layers=2, stage_two=True, task_type="caption", max_words=W, max_frames=F)
        ns = argparse.Namespace(**dict(cfg.to_dict(), local_rank=0, dropout_prob=0.0, compute_dtype="fp32" if dtype == torch.float32 else "bf16"))
        model = UniVL.from_pretrained("bert-base-uncased", "visual-base", "cross-base", "decoder-base", cache_dir=None, state_dict=None,
                                      task_config=ns)
        P = O.procedural_params(cfg, 0)
        sd = dict(P)
        for alias, owner in O.tied_aliases(cfg).items():
            sd[alias] = P[owner]
        model.load_state_dict(sd, strict=True)
        model.to(dev).eval()
        d = {k: v.to(dev) for k, v in O.synthetic_batch(cfg, N, seed=31).items()}
        with torch.no_grad():
            so, vo = model.get_sequence_visual_output(d["input_ids"], d["token_type_ids"], d["attention_mask"], d["video"], d["video_mask"])
        return model, (so, vo, d["attention_mask"].view(N, -1), d["video_mask"].view(N, -1))

    BEAM = ("tokens", "scores", "lengths", "parents", "step_tokens", "step_scores")
    SAMPLE = ("tokens", "token_logprobs", "token_q_logprobs", "seq_logprob", "seq_q_logprob", "lengths")
    SCORE = ("token_logprob", "top_token", "top_logprob", "seq_logprob", "seq_tokens", "seq_correct")
    for dtype, tag in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
        model, enc = toy(dtype)
        two = tuple(x[:2] for x in enc)
        mk = lambda **kw: CaptionBeamSearch(model, N, W, F, n_bm=ROWS, max_len=T, **kw)

        def beam_runs(name, bs, eos, n_best):
            last = None
            for leg, feats, na in (("full", enc, None), ("partial", two, 2), ("again", enc, None)):
                res = bs.decode(*feats, bos=BOS, eos=eos, n_best=n_best, sync_every=2, n_active=na)
                keep("%s.%s.%s" % (tag, name, leg), res, BEAM)
                cap, cap_len = res.captions(eos, 0, eos_dev=bs.eos_dev)
                keep("%s.%s.%s.captions" % (tag, name, leg), dict(cap=cap, cap_len=cap_len), ("cap", "cap_len"))
                last = res
            keep_plans("%s.%s" % (tag, name), bs)
            return last

        plain = mk()
        free = plain.decode(*enc, bos=BOS, eos=-1, n_best=ROWS)
        eos = int(free.tokens[0, 0, 2])                  # instance 0's best hypothesis ends at its third token
        suppress = sorted({int(free.tokens[1, 0, 0]), int(free.tokens[2, 0, 1])})
        cons = DecodeConstraints(2, 3, suppress)
        res_plain = beam_runs("plain", plain, eos, ROWS)
        beam_runs("host", mk(beam_step="host"), eos, ROWS)
        beam_runs("constrained", mk(constraints=cons), eos, ROWS)
        beam_runs("groups", mk(beam_groups=2, diversity_penalty=0.5), eos, ROWS // 2)

        for name, kw in (("sampler", {}), ("sampler_constrained", dict(constraints=cons))):
            smp = CaptionSampler(model, N, W, F, n_samp=ROWS, max_len=T, top_k=8, **kw)
            for leg, feats, na in (("full", enc, None), ("partial", two, 2)):
                res = smp.sample(*feats, bos=BOS, eos=eos, seed=7, sync_every=2, n_active=na)
                keep("%s.%s.%s" % (tag, name, leg), res, SAMPLE)
            first = res.tokens.new_zeros(N * ROWS).long()
            first[:2 * ROWS] = res.tokens[:, :, 0].reshape(-1).clamp(min=0)
            for t, ids in ((0, torch.full((N * ROWS,), BOS, dtype=torch.int64, device=dev)), (1, first)):
                keep("%s.%s.step_logits%d" % (tag, name, t), dict(x=smp.step_logits(t, ids).float()), ("x",))
            keep_plans("%s.%s" % (tag, name), smp)

        g = torch.Generator().manual_seed(5)
        for nc in (1, 3):
            sc = CaptionScorer(model, N, W, F, WD, n_cand=nc)
            ids = torch.randint(1000, 30000, (N, nc, WD), generator=g).to(dev)
            lens = torch.randint(2, WD + 1, (N, nc, 1), generator=g).to(dev)
            mask = (torch.arange(WD, device=dev) < lens).to(torch.int64)
            lab = torch.where(mask > 0, torch.randint(1000, 30000, (N, nc, WD), generator=g).to(dev), torch.full_like(mask, -1))
            keep("%s.scorer%d.full" % (tag, nc), sc.score(*enc, ids, mask, lab), SCORE)
            keep("%s.scorer%d.partial" % (tag, nc), sc.score(*two, ids[:2], mask[:2], lab[:2], n_active=2), SCORE)
            if nc == 3:
                top3 = types.SimpleNamespace(tokens=res_plain.tokens[:, :3].contiguous(), lengths=res_plain.lengths)
                keep("%s.scorer3.beams" % tag, sc.score_beams(top3, *enc, bos=BOS, eos=eos, pad=0), SCORE)
            keep_plans("%s.scorer%d" % (tag, nc), sc)

    out["plans"] = np.array(json.dumps(plans, sort_keys=True))
    np.savez(path, **out)
    print("wrote %d arrays and the plans of %d sessions to %s" % (len(out) - 1, len(plans), path))
    return 0


def compare(a_path, b_path):
    a, b = np.load(a_path), np.load(b_path)
    names = sorted((set(a.files) | set(b.files)) - {"plans"})
    differ = [k for k in names if k not in a.files or k not in b.files or a[k].dtype != b[k].dtype or a[k].shape != b[k].shape
              or a[k].tobytes() != b[k].tobytes()]
    pa, pb = json.loads(str(a["plans"])), json.loads(str(b["plans"]))
    plan_diff = sorted(k for k in set(pa) | set(pb) if pa.get(k) != pb.get(k))
    print("%d differing arrays of %d%s" % (len(differ), len(names), ": " + ", ".join(differ[:8]) if differ else ""))
    print("plan keys and op names: %s (%d sessions, %d plans)"
          % ("identical" if not plan_diff else "DIFFERENT in " + ", ".join(plan_diff), len(pa), sum(len(v) for v in pa.values())))
    return 1 if differ or plan_diff else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--dump", metavar="FILE")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    args = ap.parse_args()
    if bool(args.dump) == bool(args.compare):
        ap.error("give --dump FILE or --compare A B")
    sys.exit(dump(args.dump) if args.dump else compare(*args.compare))
