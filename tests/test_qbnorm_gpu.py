"""Query-bank normalised retrieval search: the column term (csrc/retrieve.hip: univl_sim_colstat), the normalised search
(univl_sim_topk_norm), the hub flags and gates, retrieval.QueryBank and eval.eval_retrieval_streamed(bank_batches=), against
tests/qbnorm_ref.py.

1  same chain: with one bank row c_j IS the score, bit for bit the one univl_sim_topk reports;
2  the column term on random unit vectors against fp64 at the project's fp32 gate 2e-4;
3  no overflow with scores in the thousands;
4  purity of c_j: pieces, a permuted gallery, deterministic mode, a row alone against the same row inside a full tile;
5  the normalised search on exact-arithmetic inputs against numpy fp32 with the tie rule -- no tolerance; an all-zero bias is the
   plain search; pieces merge exactly; forced slice counts agree;
6  the hand-made hub case: normalisation puts the true video first, the dynamic gate leaves a query outside the hub set alone;
7  the Python surface on the small deterministic model;
8  column term, gate and normalised search captured on one stream into one graph and replayed on new queries;
9  every argument the two entry points refuse."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from make_golden import case_config

import qbnorm_ref as R
from retrieval_cases import batches as _batches, deterministic_models, int_gallery, padded as _padded  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import univl_amd
    from univl_amd import _lib, ops, metrics
    from univl_amd import eval as uev
    from test_model_gpu import build

DEV = "cuda"
H = 768
TOL = 2e-4                       # the project's fp32 gate, the TOL of tests/test_retrieve_gpu.py


def _np(t):
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _int_case(Nq, Ng):
    """Integer queries and gallery in [-8, 8] (every partial sum exact in fp32), built as tests/test_retrieve_gpu.py builds them: rows
    j = 5, 9, 13, ... duplicate row j % 3, targets sit on duplicated rows where there are any.  (q, g, targets, int64 scores)."""
    return int_gallery(Nq, Ng)


def _matrix(q, g):
    """The device's own [Nq, Ng] score matrix: univl_sim_topk with k = Ng (<= 64) scattered by index."""
    score, idx = ops.sim_topk(q, g, g.shape[0])
    mat = torch.empty(q.shape[0], g.shape[0], device=DEV)
    mat.scatter_(1, idx.long(), score)
    return _np(mat)


# ------------------------------------------------------------------------------------------------ 1: same chain
@functools.lru_cache(maxsize=None)
def _unit_case():
    """1000 bank rows, 300 gallery rows, 33 queries: random unit vectors; fp64 scores of the bank, computed once."""
    gen = torch.Generator().manual_seed(31)
    unit = lambda n: torch.nn.functional.normalize(torch.randn(n, H, generator=gen, dtype=torch.float64), dim=-1).float()
    bank, g, q = unit(1000), unit(300), unit(33)
    s64 = (bank.double() @ g.double().t()).numpy()
    return bank.to(DEV), g.to(DEV), q.to(DEV), s64


@pytest.mark.parametrize("Ng", [1, 31, 33, 64])
def test_one_bank_row_gives_the_score_of_sim_topk_bit_for_bit(Ng):
    bank, g, _, _ = _unit_case()
    for row, beta in ((0, 20.0), (7, 1.0), (999, 100.0)):
        b = bank[row:row + 1]
        score, idx = ops.sim_topk(b, g[:Ng], Ng)
        want = torch.empty(Ng, device=DEV)
        want[idx[0].long()] = score[0]
        assert torch.equal(ops.sim_colstat(b, g[:Ng], beta), want), (row, beta)


# ------------------------------------------------------------------------------------------------ 2: against fp64
@pytest.mark.parametrize("Nb", [1, 5, 127, 128, 129, 1000])
def test_column_term_against_fp64(Nb):
    bank, g, _, s64 = _unit_case()
    worst = 0.0
    for beta in (1.0, 20.0, 100.0):
        for Ng in (1, 17, 33, 300):
            c = _np(ops.sim_colstat(bank[:Nb], g[:Ng], beta)).astype(np.float64)
            err = float(np.abs(c - R.colstat(s64[:Nb, :Ng], beta)).max())
            worst = max(worst, err)
            assert np.all(np.isfinite(c)) and err <= TOL, (beta, Ng, err)
    print("sim_colstat Nb=%d: max |c - c64| = %.3e" % (Nb, worst))


# ------------------------------------------------------------------------------------------------ 3: no overflow
def test_no_overflow_with_scores_in_the_thousands():
    """Non-negative integers: the leader (all eights) scores 8 sum(g_j), every other bank row at most half of that."""
    gen = torch.Generator().manual_seed(7)
    g = torch.randint(0, 9, (70, H), generator=gen).float()
    bank = torch.randint(0, 5, (130, H), generator=gen).float()
    bank[129] = 8.0                                                       # in the second bank tile = the second slice: the merge rescales
    s = (bank.to(torch.int64) @ g.to(torch.int64).t()).numpy()
    m = s.max(0)
    assert np.array_equal(s.argmax(0), np.full(70, 129)) and (m - np.sort(s, axis=0)[-2]).min() >= 200 and m.min() >= 1000
    c = _np(ops.sim_colstat(bank.to(DEV), g.to(DEV), 1.0))
    assert np.all(np.isfinite(c)) and np.abs(c.astype(np.float64) - m).max() <= TOL


# ------------------------------------------------------------------------------------------------ 4: purity
def test_column_term_is_a_pure_function_of_the_row_the_bank_and_beta():
    bank, g, _, _ = _unit_case()
    bank = bank[:200]
    c = ops.sim_colstat(bank, g, 20.0)
    assert torch.equal(torch.cat([ops.sim_colstat(bank, g[:129], 20.0), ops.sim_colstat(bank, g[129:], 20.0)]), c)     # 300 = 129 + 171
    perm = torch.randperm(300, generator=torch.Generator().manual_seed(2)).to(DEV)
    assert torch.equal(ops.sim_colstat(bank, g[perm].contiguous(), 20.0), c[perm])
    assert torch.equal(ops.sim_colstat(_padded(bank.cpu(), 776), _padded(g.cpu(), 772), 20.0), c)                     # row strides
    was = univl_amd.deterministic()
    try:
        univl_amd.set_deterministic(True)
        c_det = ops.sim_colstat(bank, g, 20.0)
        univl_amd.set_deterministic(False)
        c_not = ops.sim_colstat(bank, g, 20.0)
    finally:
        univl_amd.set_deterministic(was)
    assert torch.equal(c_det, c) and torch.equal(c_not, c)
    for j in (0, 45, 299):                                                # a row alone against the same row inside a full tile
        assert torch.equal(ops.sim_colstat(bank, g[j:j + 1], 20.0)[0], c[j])


# ------------------------------------------------------------------------------------------------ 2 - 4 again: several tiles per slice
# Up to 4096 bank rows a slice is ONE bank tile and every fold happens in the merge launch.  Beyond, a workgroup walks several tiles:
# the fold inside the scan, the second score buffer and the hand-over of the prefetched rows from tile to tile run only there.
LONG = {4227: 2, 8300: 3}        # Nb -> tiles per slice: 34 tiles (the last of 3 rows) in 17 slices; 65 tiles (the last of 108) in 22


@functools.lru_cache(maxsize=None)
def _long_case():
    """8300 bank rows, 33 gallery rows: random unit vectors, fp64 scores computed once."""
    gen = torch.Generator().manual_seed(47)
    unit = lambda n: torch.nn.functional.normalize(torch.randn(n, H, generator=gen, dtype=torch.float64), dim=-1).float()
    bank, g = unit(8300), unit(33)
    return bank.to(DEV), g.to(DEV), (bank.double() @ g.double().t()).numpy()


@pytest.mark.parametrize("Nb", sorted(LONG))
def test_long_bank_column_term_against_fp64_and_purity(Nb):
    bank, g, s64 = _long_case()
    T = -(-Nb // 128)
    assert -(-T // _lib.COLSTAT_SLICES) == LONG[Nb] and Nb % 128 != 0     # the walk is that long, and the last tile is partial
    assert _lib.lib().univl_sim_colstat_workspace(Nb, 33) == 8 * -(-T // LONG[Nb]) * 33
    bank = bank[:Nb]
    worst = 0.0
    for beta in (1.0, 20.0, 100.0):
        for Ng in (1, 33):
            c = _np(ops.sim_colstat(bank, g[:Ng], beta)).astype(np.float64)
            err = float(np.abs(c - R.colstat(s64[:Nb, :Ng], beta)).max())
            worst = max(worst, err)
            assert np.all(np.isfinite(c)) and err <= TOL, (beta, Ng, err)
    print("sim_colstat Nb=%d: max |c - c64| = %.3e" % (Nb, worst))
    c = ops.sim_colstat(bank, g, 20.0)
    assert torch.equal(torch.cat([ops.sim_colstat(bank, g[:17], 20.0), ops.sim_colstat(bank, g[17:], 20.0)]), c)       # pieces
    perm = torch.randperm(33, generator=torch.Generator().manual_seed(3)).to(DEV)
    assert torch.equal(ops.sim_colstat(bank, g[perm].contiguous(), 20.0), c[perm])
    assert torch.equal(ops.sim_colstat(_padded(bank.cpu(), 772), _padded(g.cpu(), 776), 20.0), c)                     # row strides
    for j in (0, 16, 32):                                                 # a row alone against the same row inside the tile
        assert torch.equal(ops.sim_colstat(bank, g[j:j + 1], 20.0)[0], c[j])
    was = univl_amd.deterministic()
    try:
        univl_amd.set_deterministic(True)
        c_det = ops.sim_colstat(bank, g, 20.0)
        univl_amd.set_deterministic(False)
        c_not = ops.sim_colstat(bank, g, 20.0)
    finally:
        univl_amd.set_deterministic(was)
    assert torch.equal(c_det, c) and torch.equal(c_not, c)


@pytest.mark.parametrize("leader", [5, 200, 300, 8299])
def test_long_bank_no_overflow_wherever_the_leader_sits(leader):
    """8300 rows, three tiles per slice (rows 0 .. 383 are slice 0).  The leader in the FIRST tile of its slice: the later tiles' pairs
    are scaled down to nothing inside the scan; in the second (200; 8299, the last row of the last, partial tile) or the third (300):
    the running pair itself is rescaled inside the scan."""
    gen = torch.Generator().manual_seed(11)
    g = torch.randint(0, 9, (33, H), generator=gen).float()
    bank = torch.randint(0, 5, (8300, H), generator=gen).float()
    bank[leader] = 8.0
    s = (bank.to(torch.int64) @ g.to(torch.int64).t()).numpy()
    m = s.max(0)
    assert np.array_equal(s.argmax(0), np.full(33, leader)) and (m - np.sort(s, axis=0)[-2]).min() >= 200 and m.min() >= 1000
    c = _np(ops.sim_colstat(bank.to(DEV), g.to(DEV), 1.0))
    assert np.all(np.isfinite(c)) and np.abs(c.astype(np.float64) - m).max() <= TOL


# ------------------------------------------------------------------------------------------------ 5: normalised search, exact
def _bias_and_gate(Nq, Ng):
    gen = torch.Generator().manual_seed(77 * Nq + Ng)
    bias = torch.randint(-8, 9, (Ng,), generator=gen).float() * 0.25      # multiples of 0.25 with many repeats: ties
    for j in range(5, Ng, 8):
        bias[j] = bias[j % 3]             # _int_case: row j duplicates row j % 3; with its bias too, the normalised scores tie
    gate = torch.tensor([0 if i % 3 == 1 else (1 if i % 3 == 0 else 5) for i in range(Nq)], dtype=torch.int32)     # nonzero = set
    return bias, gate


@pytest.mark.parametrize("Ng", [1, 3, 64, 65, 1000])
@pytest.mark.parametrize("Nq", [1, 5, 17, 33])
def test_normalised_search_exact_integer_inputs(Nq, Ng):
    q, g, tgt, s = _int_case(Nq, Ng)
    bias, gate = _bias_and_gate(Nq, Ng)
    sp = R.normalised(s, bias.numpy(), gate.numpy())                      # s is exact in fp32, multiples of 0.25 below 2^16 too
    qd, gd, bd, gated, td = _padded(q, 776), _padded(g, 772), bias.to(DEV), gate.to(DEV), tgt.to(DEV)
    for k in (1, 10, 64):
        ridx, rscore, rgt, req = R.search(sp, k, tgt.numpy())
        score, idx, gt, eq = ops.sim_topk_norm(qd, gd, k, bd, row_gate=gated, target=td)
        assert np.array_equal(_np(idx).astype(np.int64), ridx) and np.array_equal(_np(score), rscore), k
        assert np.array_equal(_np(gt), rgt) and np.array_equal(_np(eq), req), k
        score2, idx2 = ops.sim_topk_norm(qd, gd, k, bd, row_gate=gated)   # without target: the same lists
        assert torch.equal(score2, score) and torch.equal(idx2, idx)
    assert Ng < 64 or int(req.max()) > 1                                  # the bias does force ties with the target
    gt0, eq0 = ops.sim_topk_norm(qd, gd, 0, bd, row_gate=gated, target=td)         # k = 0: the counts alone
    assert np.array_equal(_np(gt0), rgt) and np.array_equal(_np(eq0), req)
    # no gates: every row is normalised
    ridx, rscore, rgt, req = R.search(R.normalised(s, bias.numpy(), np.ones(Nq)), 10, tgt.numpy())
    score, idx, gt, eq = ops.sim_topk_norm(qd, gd, 10, bd, target=td)
    assert np.array_equal(_np(idx).astype(np.int64), ridx) and np.array_equal(_np(score), rscore)
    assert np.array_equal(_np(gt), rgt) and np.array_equal(_np(eq), req)
    # an all-zero bias is the plain search, bit for bit
    plain = ops.sim_topk(qd, gd, 10, target=td)
    zero = ops.sim_topk_norm(qd, gd, 10, torch.zeros(Ng, device=DEV), target=td)
    assert all(torch.equal(a, b) for a, b in zip(plain, zero))


def test_normalised_search_pieces_merge_exactly_and_slice_counts_agree():
    Nq, Ng = 33, 1000
    q, g, tgt, s = _int_case(Nq, Ng)
    bias, gate = _bias_and_gate(Nq, Ng)
    qd, gd, bd, gated, td = q.to(DEV), g.to(DEV), bias.to(DEV), gate.to(DEV), tgt.to(DEV)
    whole = ops.sim_topk_norm(qd, gd, 10, bd, row_gate=gated, target=td)
    for slices in (1, 3, 8):
        forced = ops.sim_topk_norm(qd, gd, 10, bd, row_gate=gated, target=td, slices=slices)
        assert all(torch.equal(a, b) for a, b in zip(whole, forced)), slices
    sa, ia = ops.sim_topk_norm(qd, gd[:300], 10, bd[:300].contiguous(), row_gate=gated)
    sb, ib = ops.sim_topk_norm(qd, gd[300:], 10, bd[300:].contiguous(), row_gate=gated)
    sc, ic = _np(torch.cat([sa, sb], 1)), _np(torch.cat([ia, ib + 300], 1))
    for r in range(Nq):
        order = np.lexsort((ic[r], -sc[r]))[:10]
        assert np.array_equal(sc[r][order], _np(whole[0][r])) and np.array_equal(ic[r][order], _np(whole[1][r]))


# ------------------------------------------------------------------------------------------------ 6: what it is for
def test_hub_case_normalisation_restores_the_true_video():
    q, g, bank = (torch.from_numpy(x).to(DEV) for x in R.hub_case())
    raw_score, raw_idx = ops.sim_topk(q, g, 3)
    assert raw_idx[:, 0].tolist() == [8] * 8 + [0] and raw_score[:8, 0].tolist() == [30.0] * 8      # every raw top-1 is the hub
    hub = ops.hub_flags(ops.sim_topk(bank, g, 1)[1], 9)
    assert hub.tolist() == [0] * 8 + [1]                                  # the hub set is exactly {8}
    gate = ops.hub_gate(raw_idx, hub)                                     # the first column of the [9, 3] lists, in place
    assert gate.tolist() == [1] * 8 + [0] and torch.equal(ops.hub_gate(raw_idx[:, 0].contiguous(), hub), gate)
    c = ops.sim_colstat(bank, g, 1.0)
    assert abs(float(c[8]) - (30 + np.log(8))) <= TOL and float((c[:8] - 24).abs().max()) <= TOL
    score, idx = ops.sim_topk_norm(q, g, 3, c, row_gate=gate)
    assert idx[:8, 0].tolist() == list(range(8))                          # every normalised top-1 is the true video ...
    margin = score[:8, 0] - score[:8, 1]
    assert idx[:8, 1].tolist() == [8] * 8 and float((margin - np.log(8)).abs().max()) <= 2 * TOL     # ... ~2.08 ahead of the hub
    # the ninth query's raw top-1 is row 0, no hub: the dynamic search leaves it as the plain search has it, bit for bit
    assert torch.equal(score[8], raw_score[8]) and torch.equal(idx[8], raw_idx[8])
    s_static, i_static = ops.sim_topk_norm(q, g, 3, c)
    assert torch.equal(s_static[:8], score[:8]) and torch.equal(i_static[:8], idx[:8])
    assert float(s_static[8, 0]) == float(torch.tensor(72.0) - c[0].cpu()) and int(i_static[8, 0]) == 0
    # all of it against the reference on the device's own scores
    sq, sb = _matrix(q, g), _matrix(bank, g)
    rgate = R.hub_gate(sq, R.hub_flags(sb, 1))
    ridx, rscore = R.search(R.normalised(sq, _np(c), rgate), 3)
    assert np.array_equal(_np(gate), rgate) and np.array_equal(_np(idx).astype(np.int64), ridx) and np.array_equal(_np(score), rscore)


# ------------------------------------------------------------------------------------------------ 7: the Python surface
def _counts(sp, targets):
    ts = sp[np.arange(sp.shape[0]), np.asarray(targets)]
    return (sp > ts[:, None]).sum(1), (sp == ts[:, None]).sum(1)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_query_bank_search_fit_and_streamed_metrics(dtype, deterministic_models):
    from univl_amd.retrieval import QueryBank, VideoIndex
    cfg, rows, dseed = case_config("joint_small")
    model, _ = build(cfg, dtype)
    model.eval()
    bs = _batches(cfg, [3, 3, 2, 2, 2], dseed)                            # 12 texts; the videos of the first three batches: 8
    more, bank_bs = _batches(cfg, [3], dseed + 50)[0], _batches(cfg, [3, 3], dseed + 90)       # 3 more videos; a 6-text bank
    texts = lambda b: (b["input_ids"], b["token_type_ids"], b["attention_mask"])
    index = VideoIndex(model, capacity=4)
    for b in bs[:3]:
        index.add(b["video"], b["video_mask"])
    cat = {k: torch.cat([b[k] for b in bs]) for k in ("input_ids", "token_type_ids", "attention_mask")}
    q = index.pool_text(*texts(cat))[0]
    targets = [0, 1, 2, 3, 4, 5, 6, 7, 0, 3, 6, 6]
    for dynamic, hub_k in ((True, 1), (False, 1), (True, 2)):
        bank = QueryBank(index, beta=20.0, hub_k=hub_k, dynamic=dynamic)
        for b in bank_bs:
            bank.add(*texts(b))
        assert len(bank) == 6
        with pytest.raises(ValueError, match=r"bank\.fit\(\)"):
            index.search(*texts(cat), k=5, bank=bank)                     # never fitted
        assert bank.fit() is bank
        # search(bank=) is the composition of the ops calls, bit for bit
        g = index.vectors
        c = ops.sim_colstat(bank.vectors, g, 20.0)
        hub = ops.hub_flags(ops.sim_topk(bank.vectors, g, hub_k)[1], len(index))
        gate = ops.hub_gate(ops.sim_topk(q, g, 1)[1], hub) if dynamic else None
        assert torch.equal(bank.c, c) and torch.equal(bank.hub, hub)
        td = torch.tensor(targets, dtype=torch.int32, device=DEV)
        want = ops.sim_topk_norm(q, g, 5, c, row_gate=gate, target=td)
        got = index.search(*texts(cat), k=5, targets=targets, bank=bank)
        assert all(torch.equal(a, b) for a, b in zip(got, want))
        got_v = index.search_vectors(q, 5, targets, bank=bank)
        assert all(torch.equal(a, b) for a, b in zip(got_v, want))
        # ... and of the reference on the device's own scores and column terms
        sq, sb = _matrix(q, g), _matrix(bank.vectors, g)
        rhub = R.hub_flags(sb, hub_k)
        rgate = R.hub_gate(sq, rhub, dynamic)
        sp = R.normalised(sq, _np(c), rgate)
        ridx, rscore, rgt, req = R.search(sp, 5, targets)
        assert np.array_equal(_np(hub), rhub) and (gate is None or np.array_equal(_np(gate), rgate))
        assert np.array_equal(_np(got[1]).astype(np.int64), ridx) and np.array_equal(_np(got[0]), rscore)
        assert np.array_equal(_np(got[2]), rgt) and np.array_equal(_np(got[3]), req)
        # the streamed evaluation reports the metrics of those counts
        tb = [(b["input_ids"], b["attention_mask"], b["token_type_ids"]) for b in bs]
        vb = [(b["video"], b["video_mask"]) for b in bs[:3]]
        m, (gt_s, eq_s) = uev.eval_retrieval_streamed(model, tb, vb, targets, bank_batches=[
            (b["input_ids"], b["attention_mask"], b["token_type_ids"]) for b in bank_bs], beta=20.0, hub_k=hub_k, dynamic=dynamic)
        assert np.array_equal(gt_s, rgt) and np.array_equal(eq_s, req) and m == metrics.compute_metrics((rgt, req))
    # without bank_batches: what it returned before, the counts of the raw scores
    m0, (gt0, eq0) = uev.eval_retrieval_streamed(model, tb, vb, targets)
    rgt0, req0 = _counts(sq, targets)
    assert np.array_equal(gt0, rgt0) and np.array_equal(eq0, req0) and m0 == metrics.compute_metrics((rgt0, req0))
    # the index grows: a stale bank is refused, fit() covers the new rows only and equals a fresh bank bit for bit
    index.add(more["video"], more["video_mask"])
    with pytest.raises(ValueError, match=r"bank\.fit\(\)"):
        index.search_vectors(q, 5, bank=bank)
    old_c = bank.c.clone()
    bank.fit()
    fresh = QueryBank(index, beta=20.0, hub_k=2, dynamic=True)
    fresh.add_vectors(bank.vectors.clone())
    fresh.fit()
    assert len(index) == 11 and bank.c.shape == (11,) and torch.equal(bank.c[:8], old_c)
    assert torch.equal(bank.c, fresh.c) and torch.equal(bank.hub, fresh.hub)
    assert torch.equal(bank._top_idx, fresh._top_idx) and torch.equal(bank._top_score, fresh._top_score)
    a, b = index.search_vectors(q, 11, bank=bank), index.search_vectors(q, 11, bank=fresh)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    bank.add_vectors(q[:1])                                               # more bank rows: everything is recomputed
    with pytest.raises(ValueError, match=r"bank\.fit\(\)"):
        index.search_vectors(q, 5, bank=bank)
    assert torch.equal(bank.fit().c, ops.sim_colstat(bank.vectors, index.vectors, 20.0))


def test_rerank_takes_its_candidates_from_the_normalised_search(deterministic_models):
    from univl_amd.retrieval import QueryBank, VideoIndex
    cfg, rows, dseed = case_config("align_small")
    model, _ = build(cfg, torch.float32)
    model.eval()
    bs = _batches(cfg, [3, 3, 2], dseed)
    index = VideoIndex(model, capacity=8, keep_frames=True)
    for b in bs:
        index.add(b["video"], b["video_mask"])
    cat = {k: torch.cat([b[k] for b in bs]) for k in bs[0]}
    bank = QueryBank(index, beta=20.0, dynamic=False)
    bank.add(cat["input_ids"][2:7], cat["token_type_ids"][2:7], cat["attention_mask"][2:7])
    bank.fit()
    texts = (cat["input_ids"], cat["token_type_ids"], cat["attention_mask"])
    _, cand = index.search(*texts, k=3, bank=bank)
    score, idx = index.search(*texts, k=3, rerank=True, bank=bank, chunk_rows=3)
    assert torch.equal(idx.sort(1).values, cand.sort(1).values)           # the normalised candidates, re-ordered ...
    full, cand_all = index.search(*texts, k=8, rerank=True, chunk_rows=4)
    pos = (cand_all.unsqueeze(2) == idx.unsqueeze(1)).float().argmax(1)   # ... and scored by the cross encoder as ever
    assert float((score - full.gather(1, pos)).abs().max()) <= TOL


# ------------------------------------------------------------------------------------------------ 8: capture
def test_column_term_gate_and_search_replay_from_one_graph():
    bank, g, q, _ = _unit_case()
    bank = bank[:200]
    tgt = (torch.arange(33, dtype=torch.int32) * 7 % 300).to(DEV)

    def run(qq):
        c = ops.sim_colstat(bank, g, 20.0)
        hub = ops.hub_flags(ops.sim_topk(bank, g, 2)[1], 300)
        gate = ops.hub_gate(ops.sim_topk(qq, g, 1)[1], hub)
        return (c, hub, gate) + ops.sim_topk_norm(qq, g, 10, c, row_gate=gate, target=tgt)

    q2 = q.flip(0).contiguous() * 0.5 + q * 0.5                           # other queries
    eager1, eager2 = run(q), run(q2)                                      # also the launches' one-time set-up, outside the capture
    assert not torch.equal(eager1[4], eager2[4]) and 0 < int(eager1[2].sum()) < 33       # the gates do mix
    qs = q.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run(qs)
    for src, want in ((q, eager1), (q2, eager2), (q, eager1)):
        qs.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(out, want))


# ------------------------------------------------------------------------------------------------ 9: refusals
def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def test_every_bad_argument_is_refused_with_a_message():
    L = _lib.lib()
    q, g = torch.zeros(4, H, device=DEV), torch.zeros(9, H, device=DEV)
    idx, score = torch.zeros(4, 64, dtype=torch.int32, device=DEV), torch.zeros(4, 64, device=DEV)
    tgt = torch.zeros(4, dtype=torch.int32, device=DEV)
    gt, eq, gate = torch.zeros_like(tgt), torch.zeros_like(tgt), torch.ones_like(tgt)
    bias = torch.zeros(9, device=DEV)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def norm(k=5, **kw):
        d = _lib.SimTopkNorm()
        d.q, d.ldq, d.g, d.ldg, d.Nq, d.Ng, d.H, d.k = _p(q), H, _p(g), H, 4, 9, H, k
        d.idx, d.score, d.ws, d.ws_bytes, d.col_bias, d.row_gate = _p(idx), _p(score), _p(ws), ws.numel(), _p(bias), _p(gate)
        for name, v in kw.items():
            setattr(d, name, v)
        return d

    def col(**kw):
        d = _lib.SimColstat()
        d.bank, d.ldb, d.g, d.ldg, d.Nb, d.Ng, d.H, d.beta = _p(q), H, _p(g), H, 4, 9, H, 20.0
        d.c, d.ws, d.ws_bytes = _p(bias), _p(ws), ws.numel()
        for name, v in kw.items():
            setattr(d, name, v)
        return d

    counts = dict(target=_p(tgt), gt=_p(gt), eq=_p(eq))
    assert L.univl_sim_topk_norm(C.byref(norm()), stream) == 0 and L.univl_sim_topk_norm(C.byref(norm(k=0, **counts)), stream) == 0
    assert L.univl_sim_topk_norm(C.byref(norm(row_gate=None)), stream) == 0           # NULL gates: all ones
    assert L.univl_sim_colstat(C.byref(col()), stream) == 0
    EINVAL, EALIGN = -1, -2
    bad_norm = {"null bias": (norm(col_bias=None), EINVAL, b"(col_bias)"), "H != 768": (norm(H=512), EINVAL, b"H=512"),
                "k too large": (norm(k=_lib.TOPK_MAX + 1), EINVAL, b"k=65"), "k == 0 without target": (norm(k=0), EINVAL, b"needs target"),
                "target without gt / eq": (norm(target=_p(tgt)), EINVAL, b"(gt, eq"), "null q": (norm(q=None), EINVAL, b"(q, g, ws)"),
                "null idx": (norm(idx=None), EINVAL, b"(idx, score)"), "Ng < 1": (norm(Ng=0), EINVAL, b"Ng=0"),
                "workspace too small": (norm(ws_bytes=4 * (8 * 5 + 8) - 1), EINVAL, b"workspace of 192 bytes needed"),
                "misaligned rows": (norm(ldg=H + 1), EALIGN, b"16-byte aligned"),
                "misaligned base": (norm(q=C.c_void_p(q.data_ptr() + 4)), EALIGN, b"16-byte aligned"),
                "slices out of range": (norm(slices=_lib.TOPK_SLICES_MAX + 1), EINVAL, b"slices=257")}
    for name, (d, code, word) in bad_norm.items():
        assert L.univl_sim_topk_norm(C.byref(norm()), stream) == 0        # a good call in between: no message is left over
        assert L.univl_sim_topk_norm(C.byref(d), stream) == code, name
        msg = L.univl_last_error()
        assert b"univl_sim_topk_norm" in msg and word in msg, (name, msg)
    need = L.univl_sim_colstat_workspace(4, 9)
    assert need == 8 * 1 * 9
    bad_col = {"H != 768": (col(H=512), EINVAL, b"H=512"), "Nb < 1": (col(Nb=0), EINVAL, b"Nb=0"), "Ng < 1": (col(Ng=0), EINVAL, b"Ng=0"),
               "beta == 0": (col(beta=0.0), EINVAL, b"beta=0"), "beta < 0": (col(beta=-1.0), EINVAL, b"beta=-1"),
               "beta infinite": (col(beta=float("inf")), EINVAL, b"beta=inf"), "beta NaN": (col(beta=float("nan")), EINVAL, b"beta="),
               "null bank": (col(bank=None), EINVAL, b"(bank, g, c, ws)"), "null c": (col(c=None), EINVAL, b"(bank, g, c, ws)"),
               "ldb < H": (col(ldb=764), EINVAL, b"ldb=764"), "misaligned rows": (col(ldb=H + 2), EALIGN, b"16-byte aligned"),
               "workspace too small": (col(ws_bytes=need - 1), EINVAL, b"workspace of 72 bytes needed")}
    for name, (d, code, word) in bad_col.items():
        assert L.univl_sim_colstat(C.byref(col()), stream) == 0
        assert L.univl_sim_colstat(C.byref(d), stream) == code, name
        msg = L.univl_last_error()
        assert b"univl_sim_colstat" in msg and word in msg, (name, msg)
    assert L.univl_hub_flags(None, 4, 9, _p(tgt), stream) == -1 and b"univl_hub_flags" in L.univl_last_error()
    assert L.univl_hub_gate(_p(tgt), 1, 4, None, 9, _p(gate), stream) == -1 and b"univl_hub_gate" in L.univl_last_error()
    torch.cuda.synchronize()
