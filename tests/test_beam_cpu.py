"""What tests/test_beam_gpu.py rests on and a CPU can check: its seeded inputs are free of exact ties, its restatement of the
contract is torch.topk where there are none, and the reference's golden has the tie count its bound is derived from."""
import os

import numpy as np
import pytest
import torch

from test_beam_gpu import GOLDEN, _expect, _synthetic


@pytest.mark.parametrize("first", [True, False], ids=["first", "later"])
@pytest.mark.parametrize("V,ld", [(30522, 30528), (1000, 1000), (8, 8)])
@pytest.mark.parametrize("nb", [1, 2, 5, 8])
@pytest.mark.parametrize("n", [1, 3, 16])
def test_synthetic_inputs_are_tie_free(n, nb, V, ld, first):
    lp, scores, done, ids, length = _synthetic(n, nb, V, ld, first)
    k = min(nb + 1, V if first else nb * V)
    x = lp.view(n, nb, ld)[:, :, :V]
    cand = x[:, 0, :] if first else (x + scores[:, :, None]).reshape(n, nb * V)
    tv, ti = cand.topk(k, dim=1, largest=True, sorted=True)
    assert bool((tv[:, 1:] < tv[:, :-1]).all())
    assert done.any() == (n > 1) and not done.all()
    exp = _expect(lp, scores, done, ids, length, n, nb, V, first, int(ti[0, 0] % V), k)
    assert torch.equal(exp[0], tv) and torch.equal(exp[1], ti)
    assert bool(exp[6][0]) and torch.equal(exp[2][done], scores[done]) and torch.equal(exp[5][done], length[done])


def test_expectation_orders_ties_by_flat_index():
    lp = torch.full((2 * 3, 8), -9.0)
    lp[4, 2] = lp[3, 7] = lp[5, 0] = -1.0                   # instance 1: beams 1, 0, 2
    sc = torch.zeros(2, 3)
    z = torch.zeros(2, dtype=torch.bool)
    vals, flat, _, par, tok, _, _ = _expect(lp, sc, z, torch.zeros(2, 3, dtype=torch.int64), torch.zeros(2, dtype=torch.int64), 2, 3, 8, False, -1, 3)
    assert par[1].tolist() == [0, 1, 2] and tok[1].tolist() == [7, 2, 0]
    assert par[0].tolist() == [0, 0, 0] and tok[0].tolist() == [0, 1, 2]


def test_golden_adjacent_top6_ties():
    """The basis of the device-against-host bound (at most 2 of 16 instances may end at an exact tie): exact ties among adjacent
    top-6 values (5 kept + the first dropped) of the reference's golden at the bench shape -- 1 among 1660 + 2560 gaps."""
    g = np.load(os.path.join(GOLDEN, "beam_caption_full.npz"))
    ties = gaps = 0
    for sfx in ("", "2"):
        top6 = np.concatenate([g["step_scores" + sfx], g["next_score" + sfx][:, :, None]], axis=2)
        ok = np.isfinite(top6).all(axis=2)
        diff = top6[:, :, :-1] - top6[:, :, 1:]
        gaps += int(ok.sum()) * diff.shape[2]
        ties += int((diff[ok] == 0).sum())
    print("[golden] exact ties %d among %d adjacent top-6 gaps" % (ties, gaps))
    assert gaps == 1660 + 2560 and ties == 1
