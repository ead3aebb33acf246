"""Group beam search without a GPU: the numpy reference (tests/group_beam_ref.py) against the two identities of the contract and a
hand-worked penalty case, the pure argument rule (decode.check_beam_groups) and where it is applied before any device work, and the
binding's refusal of CPU tensors."""
import ctypes as C

import numpy as np
import pytest
import torch

from group_beam_ref import F32, GroupBeamRef, plain_topk
from univl_amd import _lib, ops
from univl_amd.decode import BeamResult, CaptionBeamSearch, check_beam_groups
from univl_amd.eval import eval_caption


def _quarter_lp(rng, rows, V):
    """Quarter-valued fp32 in a narrow range: sums and penalties are exact, ties are plentiful."""
    return (rng.randint(-40, 0, size=(rows, V)) * 0.25).astype(F32)


def _run(n, nb, G, V, T, lam, lps, eos, done=None):
    ref = GroupBeamRef(n, nb, G, V, T, lam, eos=eos, done=done)
    for t in range(T):
        ref.step(lps[t], t)
    return ref


def _eos_of(n, nb, G, V, T, lps):
    """The token that instance 0's first group emits on top at position 1 of an unended run: as end token it freezes that group."""
    dry = _run(n, nb, G, V, 2, 0.0, lps, eos=-1)
    return int(dry.hist_tok[1, 0, 0])


def test_reference_with_one_group_is_stable_topk():
    """G = 1: per instance the n_bm best of the flattened lp + score, a stable descending sort, whatever the penalty; frozen
    instances repeat their state."""
    rng = np.random.RandomState(0)
    n, nb, V, T = 3, 4, 23, 4
    lps = [_quarter_lp(rng, n * nb, V) for _ in range(T)]
    eos = _eos_of(n, nb, 1, V, T, lps)
    ref = GroupBeamRef(n, nb, 1, V, T, 2.0, eos=eos)
    scores, tokens = np.zeros((n, nb), dtype=F32), np.zeros((n, nb), dtype=np.int64)
    done, length = np.zeros(n, dtype=bool), np.zeros(n, dtype=np.int64)
    for t in range(T):
        ref.step(lps[t], t)
        for i in range(n):
            if done[i]:
                par = np.arange(nb)
            else:
                x = lps[t][i * nb:(i + 1) * nb]
                cand = x[0] if t == 0 else (x + scores[i][:, None]).astype(F32).reshape(-1)
                val, flat = plain_topk(cand, nb)
                scores[i], par, tokens[i] = val, flat // V, flat % V
                length[i] += 1
                done[i] = tokens[i, 0] == eos
            assert np.array_equal(ref.hist_par[t, i], par) and np.array_equal(ref.hist_tok[t, i], tokens[i])
            assert np.array_equal(ref.hist_sc[t, i].view(np.int32), scores[i].view(np.int32))
            assert np.array_equal(ref.src[i * nb:(i + 1) * nb], i * nb + par)
        assert np.array_equal(ref.done.astype(bool), done) and np.array_equal(ref.length, length)
    assert done[0] and length[0] == 2                         # the frozen rule was exercised


@pytest.mark.parametrize("nb,G", [(6, 2), (6, 3), (6, 6), (8, 4)])
def test_reference_without_penalty_is_independent_searches(nb, G):
    """lambda = 0: G groups of k' on n instances are a plain search of width k' on n * G pseudo-instances, field for field."""
    rng = np.random.RandomState(nb * 10 + G)
    n, V, T, kp = 2, 19, 4, nb // G
    lps = [_quarter_lp(rng, n * nb, V) for _ in range(T)]
    eos = _eos_of(n, nb, G, V, T, lps)
    a = _run(n, nb, G, V, T, 0.0, lps, eos=eos)
    b = _run(n * G, kp, 1, V, T, 5.0, lps, eos=eos)
    for f in ("scores", "tokens", "src", "done", "length", "hist_par", "hist_tok", "hist_sc"):
        x, y = getattr(a, f), getattr(b, f)
        assert np.array_equal(x.reshape(-1), y.reshape(-1)), f
    assert a.done[0] and a.length[0] == 2


def test_reference_hand_worked_penalty():
    """One instance, n_bm = 4 in two groups, V = 5, first step; rows 0 and 2 (the groups' first beams) hold the same values.
    Group 0 takes columns 1 and 3 (-1, -2).  lambda = 3: group 1 sees -4 and -5 there and takes columns 0 (-3) and 2 (-3.25).
    lambda = 0.5: columns 1 (-1.5) and 3 (-2.5) still win, and are stored UNPENALISED as -1 and -2.  A frozen group 0 adds nothing to
    the counts: group 1 takes 1 and 3.  Last, the re-sort: group 1 selects column 2 (-2.5) ahead of column 1 (-1 - 1.6), and stores
    column 1 first because its unpenalised value is the larger."""
    lp = np.full((4, 5), -9.0, dtype=F32)
    lp[0] = lp[2] = [-3.0, -1.0, -3.25, -2.0, -8.0]
    for lam, tok, sc in ((3.0, [0, 2], [-3.0, -3.25]), (0.5, [1, 3], [-1.0, -2.0])):
        r = GroupBeamRef(1, 4, 2, 5, 1, lam)
        r.step(lp, 0)
        assert r.tokens[0].tolist() == [1, 3] + tok and r.scores[0].tolist() == [-1.0, -2.0] + sc
        assert r.src.tolist() == [0, 0, 2, 2] and r.hist_par[0, 0].tolist() == [0, 0, 0, 0] and r.length.tolist() == [1, 1]
    r = GroupBeamRef(1, 4, 2, 5, 1, 3.0, done=[1, 0], tokens=[4, 4, 0, 0])
    r.step(lp, 0)
    assert r.tokens[0].tolist() == [4, 4, 1, 3] and r.length.tolist() == [0, 1] and r.src.tolist() == [0, 1, 2, 2]
    lp = np.full((4, 5), -9.0, dtype=F32)
    lp[0] = [-9.0, -1.0, -9.0, -2.0, -9.0]
    lp[2] = [-9.0, -1.0, -2.5, -9.0, -9.0]
    r = GroupBeamRef(1, 4, 2, 5, 1, 1.6)
    r.step(lp, 0)
    assert r.tokens[0].tolist() == [1, 3, 1, 2] and r.scores[0].tolist() == [-1.0, -2.0, -1.0, -2.5]


def test_argument_rule():
    assert check_beam_groups(6, 3, 0.5) == (3, 2, 0.5) and check_beam_groups(5) == (1, 5, 0.0) and check_beam_groups(8, 8, 0) == (8, 1, 0.0)
    for bad in ((6, 4, 0.0), (6, 0, 0.0), (6, -1, 0.0), (6, 7, 0.0), (6, 12, 0.0), (6, 2.0, 0.0), (6, True, 0.0), (6, 3, -0.5),
                (6, 3, float("nan")), (6, 3, float("inf")), (6, 3, None), (6, 3, "x")):
        with pytest.raises(ValueError):
            check_beam_groups(*bad)


def test_sessions_refuse_bad_groups_before_any_device_work():
    """The rule is applied first: a model of None is never looked at."""
    for kw in (dict(n_bm=6, beam_groups=4), dict(n_bm=6, beam_groups=3, diversity_penalty=-1.0),
               dict(n_bm=4, beam_groups=2, diversity_penalty=float("nan"))):
        with pytest.raises(ValueError):
            CaptionBeamSearch(None, 2, 8, 8, **kw)
        with pytest.raises(ValueError):
            eval_caption(None, [], None, **kw)
    with pytest.raises(ValueError):                           # a supplied session owns its groups
        eval_caption(None, [], None, session=object(), beam_groups=2)


def test_beam_result_groups_default():
    z = torch.zeros(1)
    assert BeamResult(z, z, z, z, z, z).groups == 1 and BeamResult(z, z, z, z, z, z, groups=3).groups == 3


def test_binding_refuses_cpu_tensors():
    n, nb, G, V, T = 2, 4, 2, 16, 3
    kw = dict(scores=torch.zeros(n, nb), done=torch.zeros(n * G, dtype=torch.uint8), length=torch.zeros(n * G, dtype=torch.int32),
              tokens=torch.zeros(n * nb, dtype=torch.int64), src=torch.zeros(n * nb, dtype=torch.int32),
              hist_parents=torch.zeros(T, n, nb, dtype=torch.int32), hist_tokens=torch.zeros(T, n, nb, dtype=torch.int32),
              hist_scores=torch.zeros(T, n, nb), ws=torch.zeros(n * nb * 8 * nb * 2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.beam_group_step(torch.zeros(n * nb, V), V, n, nb, G, 0, diversity=0.5, **kw)


@pytest.mark.parametrize("builder", ["beam_step_desc", "beam_group_step_desc", "beam_pool_step_desc"])
def test_builders_refuse_the_same_wrong_common_arguments(builder):
    """The three descriptor builders check their common arguments through one helper: each refuses a strided `done`, a `length` of
    the wrong dtype and a `hist_tokens` whose first dimension is not hist_parents'.  No CPU test of these builders replaces
    ops._require_gpu, so this one stays with what is reachable before the device check: the helper looks at shapes and dtypes
    first, and CPU tensors are enough to reach every assertion.  With right arguments the device check is what refuses them."""
    n, nb, G, V, T = 2, 4, 2, 16, 3
    units = n * G if builder == "beam_group_step_desc" else n
    head = (torch.zeros(n * nb, V), V, n, nb) + ((G, 0) if builder == "beam_group_step_desc" else (0,))
    good = dict(scores=torch.zeros(n, nb), done=torch.zeros(units, dtype=torch.uint8), length=torch.zeros(units, dtype=torch.int32),
                tokens=torch.zeros(n * nb, dtype=torch.int64), src=torch.zeros(n * nb, dtype=torch.int32),
                hist_parents=torch.zeros(T, n, nb, dtype=torch.int32), hist_tokens=torch.zeros(T, n, nb, dtype=torch.int32),
                hist_scores=torch.zeros(T, n, nb), ws=torch.zeros(n * nb * 8 * nb * 2))
    if builder == "beam_pool_step_desc":
        good.update(w=torch.ones(T + 2), params=torch.zeros(2, dtype=torch.int32), **ops.beam_pool(n, nb, "cpu"))
    build = getattr(ops, builder)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        build(*head, **good)
    for wrong in (dict(done=torch.zeros(2 * units, dtype=torch.uint8)[::2]),
                  dict(length=torch.zeros(units, dtype=torch.int64)),
                  dict(hist_tokens=torch.zeros(T + 1, n, nb, dtype=torch.int32))):
        with pytest.raises(AssertionError):
            build(*head, **dict(good, **wrong))


def test_abi_is_declared_and_sized():
    assert "univl_beam_group_step" in _lib.EXPORTED and "univl_beam_group_step_sizeof" in _lib.EXPORTED
    assert _lib.BeamGroupStep not in _lib._STRUCTS and len(_lib._STRUCTS) == 12          # the numbered tables keep their length
    assert C.sizeof(_lib.BeamGroupStep) == C.sizeof(_lib.BeamStep) + 16
    if _lib.available():
        L = _lib.lib()
        assert L.univl_beam_group_step_sizeof() == C.sizeof(_lib.BeamGroupStep) and hasattr(L, "univl_beam_group_step")
