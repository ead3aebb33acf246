"""Retrieval search: the fused similarity + top-k kernel (csrc/retrieve.hip: univl_sim_topk), the single-modality feature calls of
UniVL, univl_amd.retrieval.VideoIndex and eval.eval_retrieval_streamed.

A  the kernel on exact-arithmetic inputs (integers in [-8, 8]: every partial sum is an integer below 2^24, exact in fp32 in any
   order) against an int64 CPU computation with the tie rule -- no tolerance;
B  the kernel on random unit vectors against fp64 scores, at the project's fp32 gate 2e-4;
C  purity of the score: bit-identical results for every slice count, for a row searched alone, for a gallery searched in pieces,
   for deterministic mode on and off; the rank counts agree exactly with the scores the call itself reports;
D  every argument the entry point refuses;
E  get_visual_output / get_sequence_output against the halves of get_sequence_visual_output;
F  VideoIndex (growth, search against eval_retrieval's matrix, streamed metrics) and the cross-encoder re-rank."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from make_golden import case_config
from retrieval_cases import batches as _batches, deterministic_models, int_gallery, padded as _padded  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import univl_amd
    from univl_amd import _lib, ops, metrics
    from univl_amd import eval as uev
    from test_model_gpu import build

DEV = "cuda"
H = 768
TOL = 2e-4                       # the project's fp32 gate (tests/test_eval_gpu.py: the fp32 similarity bound)
NEG_INF = float("-inf")


# ------------------------------------------------------------------------------------------------ references
def _ref_topk(s, k):
    """s: [Nq, Ng] numpy scores.  (idx [Nq, k] int64 with -1 tails, the sorted order) under the tie rule: score descending, equal
    scores by lower index first."""
    order = np.stack([np.lexsort((np.arange(s.shape[1]), -row)) for row in s])
    idx = np.full((s.shape[0], k), -1, dtype=np.int64)
    n = min(k, s.shape[1])
    idx[:, :n] = order[:, :n]
    return idx


@functools.lru_cache(maxsize=None)
def _int_case(Nq, Ng):
    """Integer queries and gallery; rows j with j % 4 == 1 duplicate an earlier row; targets sit on duplicated rows where there are any."""
    q, g, tgt, s = int_gallery(Nq, Ng)                                     # s: the int64 reference
    ts = s[np.arange(Nq), tgt.numpy()]
    gt = (s > ts[:, None]).sum(1)
    eq = (s == ts[:, None]).sum(1)
    return q, g, tgt, s, gt, eq


def _check_exact(score, idx, s, k):
    Ng = s.shape[1]
    ref_idx = _ref_topk(s, k)
    idx, score = idx.cpu().numpy().astype(np.int64), score.cpu().numpy()
    assert np.array_equal(idx, ref_idx)
    n = min(k, Ng)
    want = np.take_along_axis(s, ref_idx[:, :n], axis=1).astype(np.float32)
    assert np.array_equal(score[:, :n], want)
    assert np.all(score[:, n:] == NEG_INF)


# ------------------------------------------------------------------------------------------------ A: exact arithmetic
@pytest.mark.parametrize("Ng", [1, 3, 63, 64, 65, 1000, 4099])
@pytest.mark.parametrize("Nq", [1, 5, 17, 33])
def test_kernel_exact_integer_inputs(Nq, Ng):
    q, g, tgt, s, gt, eq = _int_case(Nq, Ng)
    assert Ng <= 5 or int(eq.max()) > 1                                   # the targets do sit on duplicated rows
    for n, k in enumerate([1, 5, 10, 64]):
        ldq, ldg = (768, 776) if (n + Nq) % 2 else (776, 768)
        qd, gd = _padded(q, ldq), _padded(g, ldg)
        score, idx, dgt, deq = ops.sim_topk(qd, gd, k, target=tgt.to(DEV))
        torch.cuda.synchronize()
        _check_exact(score, idx, s, k)                                    # Ng < k: -1 / -inf tails
        assert np.array_equal(dgt.cpu().numpy(), gt) and np.array_equal(deq.cpu().numpy(), eq)
        score2, idx2 = ops.sim_topk(qd, gd, k)                            # without target: the same lists
        assert torch.equal(score2, score) and torch.equal(idx2, idx)
    dgt, deq = ops.sim_topk(_padded(q, 776), _padded(g, 776), 0, target=tgt.to(DEV))      # k = 0: the counts alone
    assert np.array_equal(dgt.cpu().numpy(), gt) and np.array_equal(deq.cpu().numpy(), eq)


@pytest.mark.parametrize("Ng", [40, 1000])
def test_kernel_all_equal_gallery_returns_the_first_indices(Ng):
    gen = torch.Generator().manual_seed(3)
    q = torch.randint(-8, 9, (17, H), generator=gen).float()
    g = torch.randint(-8, 9, (1, H), generator=gen).float().repeat(Ng, 1)
    tgt = torch.arange(17, dtype=torch.int32) * 2
    for k in (1, 10, 64):
        score, idx, gt, eq = ops.sim_topk(q.to(DEV), g.to(DEV), k, target=tgt.to(DEV))
        n = min(k, Ng)
        assert torch.equal(idx[:, :n].cpu(), torch.arange(n, dtype=torch.int32).repeat(17, 1))
        assert torch.all(idx[:, n:] == -1) and torch.all(score[:, n:] == NEG_INF)
        assert torch.all(gt == 0) and torch.all(eq == Ng)
        assert torch.equal(score[:, :n].cpu(), (q @ g[0]).unsqueeze(1).repeat(1, n))


# ------------------------------------------------------------------------------------------------ B / C: random unit vectors
@functools.lru_cache(maxsize=None)
def _unit_case():
    gen = torch.Generator().manual_seed(20)
    q = torch.nn.functional.normalize(torch.randn(33, H, generator=gen, dtype=torch.float64), dim=-1)
    g = torch.nn.functional.normalize(torch.randn(4099, H, generator=gen, dtype=torch.float64), dim=-1)
    q, g = q.float(), g.float()
    s64 = (q.double() @ g.double().t()).numpy()
    return q.to(DEV), g.to(DEV), s64


def _check_tolerant(score, idx, s64, k, tol):
    """The tolerant top-k check: indices distinct and in range, scores non-increasing and within tol of the fp64 scores, and the k-th
    returned fp64 score no worse than the true k-th by more than 2 tol."""
    idx, score = idx.cpu().numpy().astype(np.int64), score.cpu().numpy().astype(np.float64)
    Nq, Ng = s64.shape
    assert idx.shape == (Nq, k) and idx.min() >= 0 and idx.max() < Ng
    for r in range(Nq):
        assert len(set(idx[r].tolist())) == k
    assert np.all(score[:, 1:] <= score[:, :-1])
    got = np.take_along_axis(s64, idx, axis=1)
    assert np.abs(score - got).max() <= tol
    true_kth = -np.sort(-s64, axis=1)[:, k - 1]
    assert np.all(got[:, k - 1] >= true_kth - 2 * tol)


def test_kernel_random_unit_vectors_against_fp64():
    q, g, s64 = _unit_case()
    score, idx = ops.sim_topk(q, g, 10)
    _check_tolerant(score, idx, s64, 10, TOL)


def test_purity_slice_counts_single_row_and_split_gallery():
    q, g, _ = _unit_case()
    score, idx = ops.sim_topk(q, g, 10)
    for slices in (1, _lib.TOPK_SLICES_MAX):
        s2, i2 = ops.sim_topk(q, g, 10, slices=slices)
        assert torch.equal(s2, score) and torch.equal(i2, idx), slices
    s7, i7 = ops.sim_topk(q[7:8], g, 10)                                  # a 16-row query tile instead of a 32-row one
    assert torch.equal(s7[0], score[7]) and torch.equal(i7[0], idx[7])
    # the gallery in two pieces, merged on the host by (score descending, global index ascending)
    sa, ia = ops.sim_topk(q, g[:2000], 10)
    sb, ib = ops.sim_topk(q, g[2000:], 10)
    sc = torch.cat([sa, sb], 1).cpu().numpy()
    ic = torch.cat([ia, ib + 2000], 1).cpu().numpy()
    for r in range(q.shape[0]):
        order = np.lexsort((ic[r], -sc[r]))[:10]
        assert np.array_equal(sc[r][order], score[r].cpu().numpy()) and np.array_equal(ic[r][order], idx[r].cpu().numpy())


def test_purity_counts_follow_the_reported_scores_and_deterministic_mode():
    q, g, _ = _unit_case()
    g40 = g[:40].clone()
    g40[11] = g40[3]                                                      # one exact tie
    tgt = (torch.arange(33, dtype=torch.int32) * 7 % 40)
    tgt[5] = 11
    tgt = tgt.to(DEV)
    was = univl_amd.deterministic()
    try:
        univl_amd.set_deterministic(False)
        score, idx, gt, eq = ops.sim_topk(q, g40, 40, target=tgt)
        univl_amd.set_deterministic(True)
        score_d, idx_d, gt_d, eq_d = ops.sim_topk(q, g40, 40, target=tgt)
    finally:
        univl_amd.set_deterministic(was)
    for a, b in ((score, score_d), (idx, idx_d), (gt, gt_d), (eq, eq_d)):
        assert torch.equal(a, b)
    assert torch.equal(idx.sort(1).values.cpu(), torch.arange(40, dtype=torch.int32).repeat(33, 1))
    at = (idx == tgt[:, None])
    ts = score[at]                                                        # the score reported at target[i], one per row
    assert ts.numel() == 33
    assert torch.equal((score > ts[:, None]).sum(1).int(), gt) and torch.equal((score == ts[:, None]).sum(1).int(), eq)
    assert int(eq[5]) == 2 and int(eq.min()) == 1


# ------------------------------------------------------------------------------------------------ D: refusals
def _desc(q, g, k, idx, score, ws, target=None, gt=None, eq=None, Hh=H, slices=0):
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    d = _lib.SimTopk()
    d.q, d.ldq, d.g, d.ldg = p(q), q.stride(0), p(g), g.stride(0)
    d.Nq, d.Ng, d.H, d.k, d.slices = q.shape[0], g.shape[0], Hh, k, slices
    d.idx, d.score, d.target, d.gt, d.eq = p(idx), p(score), p(target), p(gt), p(eq)
    d.ws, d.ws_bytes = p(ws), (ws.numel() if ws is not None else 0)
    return d


def test_every_bad_argument_is_refused_with_a_message():
    L = _lib.lib()
    q, g = torch.zeros(4, H, device=DEV), torch.zeros(9, H, device=DEV)
    idx = torch.zeros(4, 64, dtype=torch.int32, device=DEV)
    score = torch.zeros(4, 64, device=DEV)
    tgt = torch.zeros(4, dtype=torch.int32, device=DEV)
    gt, eq = torch.zeros_like(tgt), torch.zeros_like(tgt)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    good = lambda **kw: _desc(q, g, kw.pop("k", 5), idx, score, ws, **kw)
    assert L.univl_sim_topk(C.byref(good()), stream) == 0
    assert L.univl_sim_topk(C.byref(good(k=0, target=tgt, gt=gt, eq=eq)), stream) == 0
    # case -> (descriptor, words only that case's message holds)
    bad = {"H != 768": (good(Hh=512), b"H=512"), "k too large": (good(k=_lib.TOPK_MAX + 1), b"k=65"), "k negative": (good(k=-1), b"k=-1"),
           "k == 0 without target": (good(k=0), b"needs target"), "target without gt / eq": (good(target=tgt), b"(gt, eq"),
           "slices out of range": (good(slices=_lib.TOPK_SLICES_MAX + 1), b"slices=257")}
    for name, field, word in (("null q", "q", b"(q, g, ws)"), ("null g", "g", b"(q, g, ws)"), ("null ws", "ws", b"(q, g, ws)"),
                              ("null idx", "idx", b"(idx, score)"), ("null score", "score", b"(idx, score)")):
        d = good()
        setattr(d, field, None)
        bad[name] = (d, word)
    d = good(); d.ws_bytes = 4 * 1 * (8 * 5 + 8) - 1; bad["workspace too small"] = (d, b"workspace of 192 bytes needed")
    d = good(); d.Ng = 0; bad["Ng < 1"] = (d, b"Ng=0")
    d = good(); d.Nq = 0; bad["Nq < 1"] = (d, b"Nq=0")
    d = good(); d.ldg = 767; bad["ldg < H"] = (d, b"ldg=767")
    for name, (d, word) in bad.items():
        assert L.univl_sim_topk(C.byref(good()), stream) == 0            # a good call in between: no message is left over
        rc = L.univl_sim_topk(C.byref(d), stream)
        assert rc == -1, (name, rc)                                       # UNIVL_EINVAL
        msg = L.univl_last_error()
        assert b"univl_sim_topk" in msg and word in msg, (name, msg)
    assert L.univl_sim_topk(None, stream) == -1
    assert L.univl_sim_topk_workspace(4, 9, 5, 0) == 4 * 1 * (8 * 5 + 8) and L.univl_sim_topk_workspace(0, 9, 5, 0) < 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ E: single-modality feature calls
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_single_modality_outputs_equal_the_halves_of_the_joint_call(dtype, deterministic_models):
    from test_model_gpu import GATES
    cfg, rows, dseed = case_config("joint_small")
    b = _batches(cfg, [3], dseed)[0]
    for det in (True, False):
        univl_amd.set_deterministic(det)
        model, _ = build(cfg, dtype)
        model.eval()
        so, vo = model.get_sequence_visual_output(b["input_ids"], b["token_type_ids"], b["attention_mask"], b["video"], b["video_mask"])
        v1 = model.get_visual_output(b["video"], b["video_mask"])
        s1 = model.get_sequence_output(b["input_ids"], b["token_type_ids"], b["attention_mask"])
        assert s1.shape == so.shape and v1.shape == vo.shape and s1.dtype == torch.float32
        if det:
            assert torch.equal(s1, so) and torch.equal(v1, vo)
        else:
            for got, ref in ((s1, so), (v1, vo)):
                err = float((got - ref).abs().max())
                if dtype == torch.float32:
                    assert err <= 1e-5, err
                else:                                                     # the bf16 hidden-state gate of tests/test_model_gpu.py: absolute
                    assert err <= GATES[torch.bfloat16]["hidden"], err
        # a second call reuses the plan and sees new inputs
        v2 = model.get_visual_output(b["video"].flip(0), b["video_mask"].flip(0))
        assert v2.shape == v1.shape and not torch.equal(v2, v1)


def test_get_visual_output_shaped_equals_the_joint_call_shaped(deterministic_models):
    """shaped=True (video already float32 [B, F, video_dim] and normalised, modeling.py:300-305 skipped): the step kind
    `features_vis_shaped` against get_sequence_visual_output(shaped=True) on the same inputs, bit for bit in deterministic mode, and
    against the unshaped call within the bound tests/test_model_gpu.py::test_shaped_true_and_pretrain_without_captions uses."""
    import univl_oracle as O
    cfg, rows, dseed = case_config("joint_small")
    model, P = build(cfg, torch.float32)
    model.eval()
    batch = O.synthetic_batch(cfg, 3, seed=dseed)
    b = {k: batch[k].to(DEV) for k in ("input_ids", "attention_mask", "token_type_ids", "video", "video_mask")}
    flat = lambda t: t.view(-1, t.shape[-1])
    vnorm = O.normalize_video(batch["video"], P).to(DEV).view(-1, cfg.max_frames, cfg.video_dim)
    _, vo = model.get_sequence_visual_output(flat(b["input_ids"]), flat(b["token_type_ids"]), flat(b["attention_mask"]), vnorm,
                                             flat(b["video_mask"]), shaped=True)
    v1 = model.get_visual_output(vnorm, flat(b["video_mask"]), shaped=True)
    assert torch.equal(v1, vo)
    v0 = model.get_visual_output(b["video"], b["video_mask"])
    assert float((v1 - v0).abs().max()) < 1e-4
    s1 = model.get_sequence_output(flat(b["input_ids"]), flat(b["token_type_ids"]), flat(b["attention_mask"]), shaped=True)
    assert torch.equal(s1, model.get_sequence_output(b["input_ids"], b["token_type_ids"], b["attention_mask"]))


# ------------------------------------------------------------------------------------------------ F: the index
def _pooled(model, feats, masks, skip_first):
    out = torch.empty(feats.shape[0], H, device=DEV)
    ops.pool_fwd(feats.shape[0], feats.shape[1], feats.contiguous(), masks.reshape(-1, masks.shape[-1]).to(torch.int64).contiguous(),
                 skip_first=skip_first, normalize=not bool(model.task_config.use_mil), out=out)
    return out


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_index_growth_search_and_streamed_metrics(dtype, deterministic_models):
    from test_model_gpu import GATES
    from univl_amd.retrieval import VideoIndex
    cfg, rows, dseed = case_config("joint_small")
    model, _ = build(cfg, dtype)
    model.eval()
    bs = _batches(cfg, [3, 3, 2], dseed)
    index = VideoIndex(model, capacity=4)
    ids = [index.add(b["video"], b["video_mask"]) for b in bs]            # 3 + 3 + 2 into 4 rows: the buffer grows while it is part full
    assert len(index) == 8 and index.vectors.shape == (8, H) and index._cap == 8
    assert torch.equal(torch.cat(ids).cpu(), torch.arange(8, dtype=torch.int32))
    # the same items all at once
    cat = {k: torch.cat([b[k] for b in bs]) for k in bs[0]}
    so, vo = model.get_sequence_visual_output(cat["input_ids"], cat["token_type_ids"], cat["attention_mask"], cat["video"], cat["video_mask"])
    ref_v = _pooled(model, vo, cat["video_mask"], False)
    tol_v = 1e-5 if dtype == torch.float32 else GATES[torch.bfloat16]["hidden"]      # absolute, as tests/test_model_gpu.py applies it
    assert float((index.vectors - ref_v).abs().max()) <= tol_v
    # search against eval_retrieval's matrix on the same items
    batches = [(b["input_ids"], b["attention_mask"], b["token_type_ids"], b["video"], b["video_mask"]) for b in bs]
    m_ref, sim = uev.eval_retrieval(model, batches)
    tol = TOL if dtype == torch.float32 else GATES[torch.bfloat16]["sim"]
    score, idx = index.search(cat["input_ids"], cat["token_type_ids"], cat["attention_mask"], k=5)
    _check_tolerant(score, idx, sim.cpu().double().numpy(), 5, tol)
    # k = len(index): the kernel's own scores scattered into a matrix give exactly the streamed metrics
    score, idx, gt, eq = index.search(cat["input_ids"], cat["token_type_ids"], cat["attention_mask"], k=8,
                                      targets=torch.arange(8, dtype=torch.int32))
    mat = torch.empty(8, 8, device=DEV)
    mat.scatter_(1, idx.long(), score)
    tb = [(b["input_ids"], b["attention_mask"], b["token_type_ids"]) for b in bs]
    vb = [(b["video"], b["video_mask"]) for b in bs]
    m_stream, (gt_s, eq_s) = uev.eval_retrieval_streamed(model, tb, vb, list(range(8)))
    assert m_stream == metrics.compute_metrics(mat)
    assert np.array_equal(gt_s, gt.cpu().numpy()) and np.array_equal(eq_s, eq.cpu().numpy())
    # 8 texts on 6 videos, many-to-one
    targets = [0, 1, 2, 3, 4, 5, 0, 3]
    m2, (gt2, eq2) = uev.eval_retrieval_streamed(model, tb, vb[:2], targets)
    sub = mat[:, :6]
    ts = sub[torch.arange(8), torch.tensor(targets)]
    assert np.array_equal(gt2, (sub > ts[:, None]).sum(1).cpu().numpy()) and np.array_equal(eq2, (sub == ts[:, None]).sum(1).cpu().numpy())
    assert m2 == metrics.compute_metrics((gt2, eq2)) and set(m2) == {"R1", "R5", "R10", "MR"}
    # the opposite direction through add_vectors / search_vectors: videos query an index of text vectors
    tindex = VideoIndex(model, capacity=2)
    tindex.add_vectors(_pooled(model, so, cat["attention_mask"], True))
    s_t, i_t = tindex.search_vectors(index.vectors, 3)
    _check_tolerant(s_t, i_t, sim.t().cpu().double().numpy(), 3, tol)


def test_rerank_through_the_cross_encoder(deterministic_models):
    from univl_amd.retrieval import VideoIndex
    cfg, rows, dseed = case_config("align_small")
    model, _ = build(cfg, torch.float32)
    model.eval()
    bs = _batches(cfg, [3, 3, 2], dseed)
    index = VideoIndex(model, capacity=4, keep_frames=True)
    for b in bs:
        index.add(b["video"], b["video_mask"])
    cat = {k: torch.cat([b[k] for b in bs]) for k in bs[0]}
    so, vo = model.get_sequence_visual_output(cat["input_ids"], cat["token_type_ids"], cat["attention_mask"], cat["video"], cat["video_mask"])
    full = model.get_similarity_logits(so, vo, cat["attention_mask"], cat["video_mask"])      # every pair through the cross encoder
    score, idx = index.search(cat["input_ids"], cat["token_type_ids"], cat["attention_mask"], k=len(index), rerank=True, chunk_rows=3)
    assert score.shape == idx.shape == (8, 8) and idx.dtype == torch.int32
    assert torch.equal(idx.long().sort(1).values.cpu(), torch.arange(8).repeat(8, 1))        # each row a permutation of the gallery
    assert float((score - full.gather(1, idx.long())).abs().max()) <= TOL
    s, i = score.cpu().numpy(), idx.cpu().numpy()
    assert np.all((s[:, 1:] < s[:, :-1]) | ((s[:, 1:] == s[:, :-1]) & (i[:, 1:] > i[:, :-1])))     # sorted, ties by lower id first
    with pytest.raises(ValueError):
        VideoIndex(model, capacity=4).search(cat["input_ids"], cat["token_type_ids"], cat["attention_mask"], k=1, rerank=True)
    # a model without a cross encoder
    cfg_j, _, seed_j = case_config("joint_small")
    joint, _ = build(cfg_j, torch.float32)
    joint.eval()
    bj = _batches(cfg_j, [3], seed_j)[0]
    jindex = VideoIndex(joint, capacity=4, keep_frames=True)
    jindex.add(bj["video"], bj["video_mask"])
    with pytest.raises(ValueError):
        jindex.search(bj["input_ids"], bj["token_type_ids"], bj["attention_mask"], k=3, rerank=True)
