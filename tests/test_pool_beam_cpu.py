"""The pooled beam search without a GPU: the numpy reference (tests/pool_beam_ref.py) against the plain search it must reduce to, pool
order and replacement on hand-written cases, the weight table, the argument rule and where it is applied before any device work, and
the events that the generator of tests/test_pool_beam_gpu.py must produce -- checked here, on the reference's own runs."""
import ctypes as C

import numpy as np
import pytest
import torch

import pool_beam_ref as R
from group_beam_ref import GroupBeamRef
from pool_beam_ref import F32, PoolBeamRef
from univl_amd import _lib, ops
from univl_amd.decode import CaptionBeamSearch, PoolBeamResult, check_length_penalty
from univl_amd.eval import eval_caption


def _quarter_lp(rng, rows, V):
    return (rng.randint(-40, 0, size=(rows, V)) * 0.25).astype(F32)


def test_without_end_token_the_step_is_the_plain_step():
    """eos = -1: live state and history equal GroupBeamRef at G = 1 bit for bit over several positions; the pool stays empty."""
    rng = np.random.RandomState(1)
    n, nb, V, T = 3, 4, 23, 5
    lps = [_quarter_lp(rng, n * nb, V) for _ in range(T)]
    a, b = PoolBeamRef(n, nb, V, T, 0.6, eos=-1), GroupBeamRef(n, nb, 1, V, T, 0.0, eos=-1)
    for t in range(T):
        a.step(lps[t], t)
        b.step(lps[t], t)
        for f in ("scores", "tokens", "src", "done", "length", "hist_par", "hist_tok", "hist_sc"):
            x, y = getattr(a, f), getattr(b, f)
            assert np.array_equal(x.view(np.int32) if x.dtype == F32 else x, y.view(np.int32) if y.dtype == F32 else y), (t, f)
    assert all(len(p) == 0 for p in a.pool)


def test_without_penalty_and_end_token_the_finish_is_the_plain_search():
    """alpha = 0, eos = -1: the finish returns the plain search's beams in order -- tokens, raw scores = keys, the shared length."""
    rng = np.random.RandomState(2)
    n, nb, V, T = 2, 5, 19, 4
    lps = [_quarter_lp(rng, n * nb, V) for _ in range(T)]
    a, b = PoolBeamRef(n, nb, V, T, 0.0, eos=-1), GroupBeamRef(n, nb, 1, V, T, 0.0, eos=-1)
    for t in range(T):
        a.step(lps[t], t)
        b.step(lps[t], t)
    tok, raw, key, lens, fin = a.finish(nb)
    btok, bsc, blen = b.hypotheses(nb)
    assert np.array_equal(tok, btok) and np.array_equal(raw.view(np.int32), bsc.view(np.int32))
    assert np.array_equal(key.view(np.int32), raw.view(np.int32)) and not fin.any()
    assert np.array_equal(lens, np.repeat(blen, nb, axis=1))


def test_pool_order_and_replacement_by_hand():
    """Capacity 2.  Order: key, then end_t, then beam.  A full pool takes an entry only in front of its last one, in that one's slot."""
    r = PoolBeamRef(1, 2, 7, 4, 0.0)
    pool = []
    r.offer(pool, (F32(-3.0), F32(-3.0), 1, 1, 1))
    r.offer(pool, (F32(-1.0), F32(-1.0), 2, 0, 1))
    assert [e[0] for e in pool] == [-3.0, -1.0] and [e[0] for e in R.pool_sorted(pool)] == [-1.0, -3.0]          # slots: arrival order
    r.offer(pool, (F32(-3.0), F32(-3.0), 2, 0, 1))            # equal key as the last, later end_t: dropped
    assert r.events == {"drop"} and [e[2] for e in pool] == [1, 2]
    r.offer(pool, (F32(-3.0), F32(-3.0), 1, 0, 1))            # equal key and end_t, lower beam: replaces it in slot 0
    assert "replacement" in r.events and pool[0][2:4] == (1, 0) and pool[1][0] == -1.0
    r.offer(pool, (F32(-2.0), F32(-2.0), 3, 1, 1))
    assert [e[0] for e in pool] == [-2.0, -1.0]
    assert R.before((F32(-1.0), 0, 3, 1, 1), (F32(-1.0), 0, 4, 0, 1)) and R.before((F32(-1.0), 0, 3, 0, 1), (F32(-1.0), 0, 3, 1, 1))
    assert not R.before((F32(-1.0), 0, 3, 1, 1), (F32(-1.0), 0, 3, 1, 1))


def test_one_instance_by_hand():
    """n_bm = 2, V = 4, eos = 3, alpha = 1.  t = 0: candidates -1 (v1), -2 (eos), -3 (v0), -4 (v2): the end candidate has rank 1 < 2 and
    is pooled as the empty caption (raw -2, len 1, key -2); live beams v1, v0.  t = 1: row 0 (score -1): eos at -1.5 -> -2.5, v0 at
    -0.5 -> -1.5; row 1 (score -3): everything far down.  Candidates: -1.5 (b0 v0), -2.5 (b0 eos), ...: the end candidate of rank 1 is
    pooled with raw -2.5, len 2, key -1.25 -- in front of the shorter one.  The pool is full; the bound: best live -1.5 * w[4] = -0.375
    is above the last key -2: not done.  With early stopping: done."""
    lp0 = np.array([[-3.0, -1.0, -4.0, -2.0], [0, 0, 0, 0]], dtype=F32)
    lp1 = np.array([[-0.5, -9.0, -9.0, -1.5], [-9.0, -9.0, -9.0, -9.0]], dtype=F32)
    for early in (False, True):
        r = PoolBeamRef(1, 2, 4, 4, 1.0, early, eos=3)
        r.step(lp0, 0)
        assert r.tokens[0].tolist() == [1, 0] and r.scores[0].tolist() == [-1.0, -3.0] and r.pool[0] == [(-2.0, -2.0, 0, 0, 1)]
        assert not r.done[0]
        r.step(lp1, 1)
        assert r.tokens[0].tolist() == [0, 1] and r.scores[0].tolist() == [-1.5, -10.0] and r.src.tolist() == [0, 0]
        assert r.pool[0] == [(-2.0, -2.0, 0, 0, 1), (-1.25, -2.5, 1, 0, 1)]
        assert bool(r.done[0]) == early and r.length[0] == 2
        tok, raw, key, lens, fin = r.finish(2)
        if early:
            assert tok[0].tolist() == [[1, 3, -1, -1], [3, -1, -1, -1]] and lens[0].tolist() == [2, 1] and fin[0].tolist() == [1, 1]
            assert raw[0].tolist() == [-2.5, -2.0] and key[0].tolist() == [-1.25, -2.0]
        else:                                                 # the live beam (v1, v0), raw -1.5, len 2, key -0.75, displaces the last entry
            assert tok[0].tolist() == [[1, 0, -1, -1], [1, 3, -1, -1]] and lens[0].tolist() == [2, 2] and fin[0].tolist() == [0, 1]
            assert raw[0].tolist() == [-1.5, -2.5] and key[0].tolist() == [-0.75, -1.25]
            assert len(r.pool[0]) == 2 and r.pool[0][0][2] == 0          # the pool itself is left as it is


@pytest.mark.parametrize("alpha", [0.0, 0.6, 1.0, 2.0])
def test_weight_table(alpha):
    T = 32
    w = ops.length_weights(alpha, T)
    assert w.dtype == torch.float32 and w.shape == (T + 2,) and float(w[0]) == 1.0 and float(w[1]) == 1.0
    want = np.array([1.0] + [np.float32(np.float64(L) ** -alpha) for L in range(1, T + 2)], dtype=F32)
    assert np.array_equal(w.numpy().view(np.int32), want.view(np.int32))
    assert np.array_equal(R.weights(alpha, T).view(np.int32), want.view(np.int32))
    if alpha == 0.0:
        assert bool((w == 1.0).all())
    if alpha == 1.0:
        assert float(w[4]) == 0.25
    if alpha == 2.0:
        assert float(w[4]) == 0.0625


def test_argument_rule():
    assert check_length_penalty(None) is None and check_length_penalty(0) == (0.0, 0) and check_length_penalty(0.6, True) == (0.6, 1)
    for bad in (-0.5, float("nan"), float("inf"), -float("inf"), "1", True, [1.0]):
        with pytest.raises(ValueError):
            check_length_penalty(bad)
        with pytest.raises(ValueError):
            ops.length_weights(bad, 4)
    with pytest.raises(ValueError):
        check_length_penalty(1.0, "yes")
    with pytest.raises(ValueError):
        check_length_penalty(None, True)
    with pytest.raises(ValueError, match="out of scope"):
        check_length_penalty(1.0, False, beam_groups=2)
    with pytest.raises(ValueError, match="out of scope"):
        check_length_penalty(1.0, False, beam_step="host")


def test_sessions_refuse_bad_arguments_before_any_device_work():
    """The rule is applied first: a model of None is never looked at."""
    for kw in (dict(length_penalty=-1.0), dict(length_penalty=float("nan")), dict(length_penalty="a"), dict(n_bm=4, beam_groups=2, length_penalty=1.0),
               dict(length_penalty=1.0, early_stopping=3)):
        with pytest.raises(ValueError):
            CaptionBeamSearch(None, 2, 8, 8, **kw)
        with pytest.raises(ValueError):
            eval_caption(None, [], None, **kw)
    with pytest.raises(ValueError):
        CaptionBeamSearch(None, 2, 8, 8, length_penalty=1.0, beam_step="host")
    with pytest.raises(ValueError):                           # a supplied session owns its penalty and its mode
        eval_caption(None, [], None, session=object(), length_penalty=1.0)
    with pytest.raises(ValueError):
        eval_caption(None, [], None, session=object(), early_stopping=True)


def test_result_object_on_host_tensors():
    tok = torch.tensor([[[4, 5, 9, -1], [4, -1, -1, -1]]], dtype=torch.int32)
    z = torch.zeros(1, 2)
    r = PoolBeamResult(tok, z, z, torch.tensor([[3, 1]], dtype=torch.int32), torch.tensor([[1, 0]], dtype=torch.uint8),
                       torch.tensor([3], dtype=torch.int32), torch.zeros(3, 1, 2), torch.zeros(3, 1, 2), torch.zeros(3, 1, 2))
    assert r.hypotheses() == [[[4, 5, 9], [4]]] and r.steps_run == 3 and r.groups == 1


def test_binding_refuses_cpu_tensors():
    n, nb, V, T = 2, 4, 16, 3
    kw = dict(scores=torch.zeros(n, nb), done=torch.zeros(n, dtype=torch.uint8), length=torch.zeros(n, dtype=torch.int32),
              tokens=torch.zeros(n * nb, dtype=torch.int64), src=torch.zeros(n * nb, dtype=torch.int32),
              hist_parents=torch.zeros(T, n, nb, dtype=torch.int32), hist_tokens=torch.zeros(T, n, nb, dtype=torch.int32),
              hist_scores=torch.zeros(T, n, nb), ws=torch.zeros(n * nb * 8 * nb * 2), w=ops.length_weights(1.0, T),
              params=torch.zeros(2, dtype=torch.int32), **ops.beam_pool(n, nb, "cpu"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.beam_pool_step(torch.zeros(n * nb, V), V, n, nb, 0, **kw)


def test_abi_is_declared_and_sized():
    for name in ("univl_beam_pool_step", "univl_beam_pool_step_sizeof", "univl_beam_pool_finish"):
        assert name in _lib.EXPORTED
    assert _lib.BeamPoolStep not in _lib._STRUCTS and len(_lib._STRUCTS) == 12          # the numbered tables keep their length
    assert C.sizeof(_lib.BeamPoolStep) == C.sizeof(_lib.BeamStep) + 64
    if _lib.available():
        L = _lib.lib()
        assert L.univl_beam_pool_step_sizeof() == C.sizeof(_lib.BeamPoolStep) and hasattr(L, "univl_beam_pool_finish")


def test_generator_produces_every_event():
    """Every event the kernel test must contain occurs in the reference's own runs of the cases that test uses (the same seeds), each
    inside a position's offers rather than the finish's, and every width above 1 sees both sides of the rank edge."""
    seen, by_nb = set(), {nb: set() for nb in R.NBS}
    for nb in R.NBS:
        for V, ld, off in R.SHAPES[:2]:                       # the V = 30522 cases draw other numbers from the same generator
            for alpha in R.ALPHAS:
                for early in R.MODES:
                    ref = R.run_case(nb, V, ld, off, alpha, early)[1]
                    seen |= ref.events
                    by_nb[nb] |= ref.events
    assert not set(R.EVENTS) - seen, sorted(set(R.EVENTS) - seen)
    for nb in R.NBS[1:]:
        assert {"end_at_rank_nb_minus_1_taken", "end_at_rank_nb_not_taken", "done_by_early_stopping", "end_at_t0"} <= by_nb[nb], nb
