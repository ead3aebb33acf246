"""Evaluation side of the path: metrics.compute_metrics, the N x N similarity assembly and
the reference's multi-device pattern nn.parallel.replicate + one thread per replica (util.py:21-60)."""
import threading

import numpy as np
import pytest
import torch

import univl_oracle as O
from make_golden import case_config

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from univl_amd import metrics as M
    from univl_amd.eval import eval_retrieval
    from test_model_gpu import build

DEV = "cuda"


@pytest.mark.parametrize("n", [1, 7, 300, 1500])
def test_compute_metrics_matches_reference_semantics(n):
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, n, generator=g)
    if n >= 7:
        x[3, 5] = x[3, 3]                       # a tie with the diagonal: the reference counts both positions
        x[2, :] = 0.25                          # a constant row: n tied positions
        x[1, 1] = x[1].max() + 1                # a rank-0 row
    want = O.compute_metrics(x.numpy())
    for arg in (x.numpy(), x.to(DEV), x.to(DEV).t().contiguous().t()):     # numpy, device, non-unit-stride device
        got = M.compute_metrics(arg)
        assert got.keys() == want.keys()
        for k in want:
            assert got[k] == want[k], (k, got[k], want[k])
    ind = M.rank_positions(x.to(DEV))
    sx = np.sort(-x.numpy(), axis=1)
    ref = np.where(sx - np.diag(-x.numpy())[:, None] == 0)[1]
    np.testing.assert_array_equal(ind, ref)


def _batches(cfg, rows, seed, nb):
    out = []
    for b in range(nb):
        bt = O.synthetic_batch(cfg, rows, seed=seed + b)
        out.append((bt["input_ids"], bt["attention_mask"], bt["token_type_ids"], bt["video"], bt["video_mask"]))
    return out


@pytest.mark.parametrize("case", ["joint_small", "align_small"])
def test_eval_retrieval_and_replicas(case):
    cfg, rows, dseed = case_config(case)
    model, P = build(cfg, torch.float32)
    model.eval()
    batches = _batches(cfg, 3, dseed, 2)
    metrics, sim = eval_retrieval(model, batches)
    assert sim.shape == (6, 6)
    # oracle: features + similarity block by block, as _run_on_single_gpu does
    feats = []
    for ids, am, tt, video, vm in batches:
        so, vo = O.get_sequence_visual_output(P, cfg, ids, tt, am, video, vm, training=False)
        feats.append((so, vo, am.reshape(-1, am.shape[-1]), vm.reshape(-1, vm.shape[-1])))
    ref = torch.cat([torch.cat([O.similarity_logits(a[0], b[1], a[2], b[3], P, cfg, False) for b in feats], dim=1)
                     for a in feats], dim=0)
    assert float((sim.cpu() - ref).abs().max()) < 1e-3
    assert metrics == O.compute_metrics(sim.cpu().numpy())            # same matrix -> same numbers as metrics.py
    want = O.compute_metrics(ref.numpy())
    assert abs(metrics["R1"] - want["R1"]) <= 1.0 / 6 + 1e-9          # identical unless a near-tie flips one rank

    # util.parallel_apply pattern: replicate, one thread per replica, each on its own share of the text batches
    replicas = torch.nn.parallel.replicate(model, [0, 0], detach=True)
    assert all(r is not model and r._flat is None for r in replicas)
    results, errors = {}, []

    def worker(i, module, share):
        try:
            with torch.cuda.device(0), torch.no_grad():
                rows_ = []
                for ids, am, tt, video, vm in share:
                    so, _ = module.get_sequence_visual_output(ids.to(DEV), tt.to(DEV), am.to(DEV), video.to(DEV), vm.to(DEV))
                    row = []
                    for ids2, am2, tt2, video2, vm2 in batches:
                        _, vo = module.get_sequence_visual_output(ids2.to(DEV), tt2.to(DEV), am2.to(DEV), video2.to(DEV), vm2.to(DEV))
                        row.append(module.get_similarity_logits(so, vo, am.to(DEV), vm2.to(DEV)).cpu().numpy())
                    rows_.append(np.concatenate(row, axis=-1))
                results[i] = np.concatenate(rows_, axis=0)
        except Exception as ex:      # noqa: BLE001
            errors.append(ex)

    threads = [threading.Thread(target=worker, args=(i, r, [batches[i]])) for i, r in enumerate(replicas)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    par = np.concatenate([results[0], results[1]], axis=0)
    assert float(np.abs(par - sim.cpu().numpy()).max()) < 1e-5


def test_compute_metrics_matches_reference_golden(golden_dir):
    """GPU rank counts vs values produced by the reference's own metrics.compute_metrics (tests/golden/metrics.npz)."""
    import os
    g = np.load(os.path.join(golden_dir, "metrics.npz"))
    for n in (7, 60, 333):
        m = M.compute_metrics(torch.as_tensor(g["x%d" % n]).to(DEV))
        assert [m["R1"], m["R5"], m["R10"], float(m["MR"])] == list(g["m%d" % n])


# bf16 similarity gates at the benchmark's sizes, error / max(1, max|ref|), set to ~1.3 x the value measured on the MI355X (never
# looser than GATES[bf16]["sim"] = 1e-2): FT-Joint 8.34e-4 (fp32: 2.3e-7), FT-Align 3.81e-3 (fp32: 1.2e-6)
EVAL_BF16_SIM = {"eval_joint_full": 1.1e-3, "eval_align_full": 5e-3}


def _tie_aware_rank_bounds(ref, d):
    """Per row: the lowest and highest 0-based rank of the diagonal that a matrix within d of `ref` can give it."""
    diag = np.diag(ref)[:, None]
    return (ref > diag + d).sum(axis=1), (ref >= diag - d).sum(axis=1) - 1


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", ["eval_joint_full", "eval_align_full"])
def test_eval_retrieval_matches_reference_at_bench_size(golden_dir, name, dtype):
    """eval_retrieval at full depth and 48 x 48 in 64-item blocks (bench.py --measure eval_joint / eval_align) against the reference's
    _run_on_single_gpu + metrics.compute_metrics (oracle/make_golden.py::generate_eval): several text blocks written into one matrix,
    a partial last block, FT-Align's 5-row cross-encoder chunks with 4- and 1-row tails."""
    import json
    import os
    from make_golden import EVAL_CASES, eval_batches
    from test_model_gpu import GATES, _record
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    base, sizes, seed = EVAL_CASES[name]
    cfg, _, _ = case_config(base)
    assert json.loads(str(g["config_json"])) == cfg.to_dict()
    model, P = build(cfg, dtype)
    model.eval()
    batches = [(b["input_ids"], b["attention_mask"], b["token_type_ids"], b["video"], b["video_mask"])
               for b in eval_batches(cfg, sizes, seed)]
    metrics, sim = eval_retrieval(model, batches)
    ref = g["sim_matrix"].astype(np.float64)
    got = sim.cpu().double().numpy()
    assert got.shape == ref.shape
    scale = max(1.0, float(np.abs(ref).max()))
    err = float(np.abs(got - ref).max()) / scale
    gate = 1e-3 if dtype == torch.float32 else EVAL_BF16_SIM[name]
    assert gate <= GATES[dtype]["sim"]
    _record(name, dtype, sim=err)
    print("[eval %s %s] sim err / max(1, max|ref|) = %.3e (gate %.1e)" % (name, dtype, err, gate))
    assert err <= gate, (err, gate)
    # ranks, tie-aware: every row's rank in the device matrix must be one the reference matrix allows within d
    d = gate * scale
    lo, hi = _tie_aware_rank_bounds(ref, d)
    diag = np.diag(got)[:, None]
    r_first, r_last = (got > diag).sum(axis=1), (got >= diag).sum(axis=1) - 1
    bad = np.where((r_first < lo) | (r_last > hi))[0]
    assert bad.size == 0, [(int(i), int(r_first[i]), int(lo[i]), int(hi[i])) for i in bad[:8]]
    # the metrics follow from those ranks (metrics.py's semantics on the device matrix) ...
    assert metrics == O.compute_metrics(got.astype(np.float32))
    if not (r_first != r_last).any():
        n = len(r_first)
        assert [metrics["R1"], metrics["R5"], metrics["R10"]] == [float(np.sum(r_first < k)) / n for k in (1, 5, 10)]
        assert float(metrics["MR"]) == float(np.median(r_first) + 1)
    # ... and in fp32 they are the reference's own numbers unless a row's diagonal is within d of another score
    if dtype == torch.float32 and float(g["diag_gap"].min()) > d:
        assert [metrics["R1"], metrics["R5"], metrics["R10"], float(metrics["MR"])] == list(g["metrics"])


def test_evaluation_sessions_are_cached_named_objects():
    """get_similarity_logits (cross-encoder branch), decoder_caption and VideoIndex.search(rerank=True) keep their compiled plans in
    model._steps as steps.EvalSession objects: a repeated call with the same shapes builds nothing and gives the same bits (fixed-order
    sums: the library's deterministic mode), and no session can be mistaken for a training Step by the filters over model._steps
    (bench.py: `getattr(v, "kind", None) in (...) and v.cx.training`).  7 texts x 3 videos, 8 words, 6 frames: 7 text rows in chunks of
    5 are sessions of 5 and of 2 rows."""
    import univl_amd
    from univl_amd.retrieval import VideoIndex
    from univl_amd.steps import EvalSession, Step
    cfg = O.OracleConfig(batch_size=2, text_num_hidden_layers=1, visual_num_hidden_layers=1, cross_num_hidden_layers=1,
                         decoder_num_hidden_layers=2, stage_two=True, task_type="caption", max_words=8, max_frames=6)
    was = univl_amd.deterministic()
    univl_amd.set_deterministic(True)
    try:
        model, _ = build(cfg, torch.float32)
        model.eval()
        t = {k: v.to(DEV) for k, v in O.synthetic_batch(cfg, 7, seed=11).items()}
        v = {k: x.to(DEV) for k, x in O.synthetic_batch(cfg, 3, seed=12).items()}
        with torch.no_grad():
            so = model.get_sequence_output(t["input_ids"], t["token_type_ids"], t["attention_mask"])
            vo = model.get_visual_output(v["video"], v["video_mask"])
            am, vm = t["attention_mask"].view(7, -1), v["video_mask"].view(3, -1)
            first = model.get_similarity_logits(so, vo, am, vm)
            n_steps = len(model._steps)
            assert {k[:2] for k in model._steps if k[0] == "xsim"} == {("xsim", 5), ("xsim", 2)}
            second = model.get_similarity_logits(so, vo, am, vm)
            assert len(model._steps) == n_steps
            assert first.shape == (7, 3) and torch.equal(first, second)
            model.decoder_caption(so[:3], vo, t["input_ids"][:3], am[:3], vm, t["input_caption_ids"][:3], t["decoder_mask"][:3])
            index = VideoIndex(model, capacity=4, keep_frames=True)
            index.add(v["video"], v["video_mask"])
            index.search(t["input_ids"], t["token_type_ids"], t["attention_mask"], k=2, rerank=True)
        assert {k[0] for k in model._steps} >= {"xsim", "caption_eval", "rerank"}
        sessions = [s for s in model._steps.values() if not isinstance(s, Step)]
        assert len(sessions) >= 5                                   # xsim 5 + 2, caption_eval, rerank 5 + 2
        for s in sessions:
            assert type(s) is EvalSession and not isinstance(s, tuple)
            assert getattr(s, "kind", None) not in ("joint", "align", "caption", "pretrain")
            assert s.cx.training is False and not hasattr(s, "fwd")
    finally:
        univl_amd.set_deterministic(was)
