"""Host side of the retrieval stack's shared statements (no GPU, CPU tensors): the ranking rule (retrieval._rank_rows) against
numpy.lexsort and as an exact merge, the row buffers of VideoIndex and QueryBank across their growths (retrieval._grown and the two
growth policies), and the text-row walk of eval_retrieval_streamed / eval_localization (eval._text_rows, eval._eval_mode)."""
import re
import types

import numpy as np
import pytest
import torch

from univl_amd import eval as uev
from univl_amd import retrieval
from univl_amd.retrieval import QueryBank, VideoIndex, _NO_ROW, _grown, _rank_rows

INF = float("inf")


def _cpu_index(capacity):
    """The fake-model pattern of tests/test_qbnorm_cpu.py: an index on the CPU, filled through add_vectors."""
    model = types.SimpleNamespace(flat=types.SimpleNamespace(device=torch.device("cpu")))
    return VideoIndex(model, capacity=capacity)


# ------------------------------------------------------------------------------------------------ the ranking rule
SCORE = torch.tensor([[1.0, 3.0, 3.0, 0.0, -INF, 2.0, -INF],           # equal scores on ids 9 and 2; two empty slots
                      [5.0, 5.0, 5.0, 5.0, 5.0, 5.0, 5.0],             # all equal: the ids alone decide
                      [-INF, 4.0, -INF, 4.0, -INF, 7.0, 4.0]])         # empty slots in front, and a REAL row that scores -inf (id 3)
IDX = torch.tensor([[4, 9, 2, 7, -1, 5, -1],
                    [6, 0, 5, 1, 4, 2, 3],
                    [-1, 8, -1, 1, 3, 0, 5]], dtype=torch.int32)


def _lexsort_order(score, idx):
    ids = np.where(idx < 0, _NO_ROW, idx).astype(np.int64)
    return np.stack([np.lexsort((i, -s)) for s, i in zip(score, ids)])      # score descending, then id ascending; stable


@pytest.mark.parametrize("keep", [None, 1, 7])
def test_rank_rows_is_lexsort_by_score_then_lower_id_with_empty_slots_last(keep):
    want = _lexsort_order(SCORE.numpy(), IDX.numpy())[:, :keep]
    sc, order = _rank_rows(SCORE, IDX, keep)
    assert order.shape == sc.shape == want.shape and sc.is_contiguous()
    assert np.array_equal(order.numpy(), want)
    assert np.array_equal(sc.numpy(), np.take_along_axis(SCORE.numpy(), want, 1))
    if keep is None:
        assert IDX.gather(1, order).tolist() == [[2, 9, 5, 4, 7, -1, -1], [0, 1, 2, 3, 4, 5, 6], [0, 1, 5, 8, 3, -1, -1]]
    assert IDX.dtype == torch.int32 and (IDX < 0).sum() == 4                # the inputs are left as they were


def test_merging_two_ranked_lists_is_ranking_their_concatenation():
    """QueryBank.fit's merge: the k best of each piece, ranked together, are the k best of both pieces -- empty slots stored as _NO_ROW."""
    k = 3
    a_s, a_i = SCORE[:, :4], IDX[:, :4].clone()
    b_s, b_i = SCORE[:, 4:], IDX[:, 4:].clone()
    lists = []
    for s, i in ((a_s, a_i), (b_s, b_i)):
        sc, order = _rank_rows(s, i, k)
        ids = i.gather(1, order)
        lists.append((sc, torch.where(ids < 0, torch.full_like(ids, _NO_ROW), ids)))      # as fit() keeps them
    both_s, both_i = torch.cat([lists[0][0], lists[1][0]], 1), torch.cat([lists[0][1], lists[1][1]], 1)
    sc, order = _rank_rows(both_s, both_i, k)
    want_s, want_o = _rank_rows(SCORE, IDX, k)
    want_i = IDX.gather(1, want_o)
    assert torch.equal(sc, want_s)
    assert torch.equal(both_i.gather(1, order), torch.where(want_i < 0, torch.full_like(want_i, _NO_ROW), want_i))


# ------------------------------------------------------------------------------------------------ the row buffers
def test_grown_copies_the_filled_rows_and_zeroes_only_on_request():
    old = torch.arange(12, dtype=torch.float32).reshape(4, 3)
    new = _grown(old, 2, 8, 3, device="cpu")
    assert new.shape == (8, 3) and new.dtype == torch.float32 and torch.equal(new[:2], old[:2])
    mask = _grown(torch.ones(2, 5, dtype=torch.int64), 1, 4, 5, device="cpu", dtype=torch.int64, zero=True)
    assert mask.dtype == torch.int64 and mask[0].tolist() == [1] * 5 and int(mask[1:].abs().sum()) == 0
    assert _grown(None, 0, 3, device="cpu").shape == (3,)                  # nothing to copy, no trailing shape: QueryBank's c


def test_video_index_doubles_and_keeps_its_rows():
    index = _cpu_index(2)
    gen = torch.Generator().manual_seed(3)
    fed, caps = [], []
    for b in (1, 2, 4):
        v = torch.randn(b, 768, generator=gen)
        ids = index.add_vectors(v)
        fed.append(v)
        caps.append(index._cap)
        assert ids.tolist() == list(range(len(index) - b, len(index))) and ids.dtype == torch.int32
        assert index._buf.shape == (index._cap, 768) and torch.equal(index.vectors, torch.cat(fed))
    assert caps == [2, 4, 8] and len(index) == 7
    assert index._frames is None and index._fmask is None and index._wnorm is None      # not an index that keeps frames


def test_query_bank_buffer_lengths_and_invalidation():
    bank = QueryBank(_cpu_index(4))
    a, b = torch.full((3, 768), 2.0), torch.full((70, 768), 3.0)
    assert bank.add_vectors(a) == 3 and bank._buf.shape == (64, 768)       # the minimum of 64
    bank._covered, bank._c, bank._hub = 4, torch.zeros(4), torch.zeros(4, dtype=torch.int32)       # as after fit()
    assert bank.add_vectors(b) == 73 and bank._buf.shape == (128, 768)     # max(2 * 64, 73, 64)
    assert torch.equal(bank.vectors, torch.cat([a, b]))
    assert bank._covered == 0 and bank._c is None and bank._hub is None and bank._top_idx is None
    with pytest.raises(ValueError, match=r"bank\.fit\(\)"):
        bank.c
    assert bank.add_vectors(torch.zeros(0, 768)) == 73 and bank._buf.shape == (128, 768)


# ------------------------------------------------------------------------------------------------ the text-row walk
class _FakeIndex:
    """What the two evaluators ask of an index, without a model behind it: five gallery rows, results of the right shapes."""

    def __init__(self, model, capacity=None):
        self.model = model

    def __len__(self):
        return 5

    def search(self, input_ids, segment_ids, input_mask, k, targets, bank):
        return torch.zeros(targets.numel(), dtype=torch.int32), torch.ones(targets.numel(), dtype=torch.int32)

    def localize(self, input_ids, segment_ids, input_mask, rows, window):
        z = torch.zeros(rows.shape, dtype=torch.int32)
        return z, z + 1, z.float()


def _texts(*sizes):
    return [(torch.zeros(b, 1, 4, dtype=torch.int64),) * 3 for b in sizes]       # the loader's [b, 1, W] shape: rows = numel / W


def _run(who, model, texts, n):
    if who == "eval_retrieval_streamed":
        return uev.eval_retrieval_streamed(model, texts, [], list(range(n)), device="cpu")
    return uev.eval_localization(model, _FakeIndex(model), texts, list(range(n)), [0] * n, [1] * n, (1, 1), device="cpu")


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("who", ["eval_retrieval_streamed", "eval_localization"])
def test_text_row_walk_raises_both_count_errors_and_restores_the_mode(who, training, monkeypatch):
    monkeypatch.setattr(retrieval, "VideoIndex", _FakeIndex)
    model = torch.nn.Module().train(training)
    with pytest.raises(ValueError, match="^" + re.escape("%s: more text rows than targets (3)" % who) + "$"):
        _run(who, model, _texts(2, 2), 3)
    assert model.training is training
    with pytest.raises(ValueError, match="^" + re.escape("%s: 2 text rows for 3 targets" % who) + "$"):
        _run(who, model, _texts(2), 3)
    assert model.training is training
    out = _run(who, model, _texts(2, 1), 3)                                 # and the matching count goes through
    assert model.training is training and (out["n"] if who == "eval_localization" else len(out[1][0])) == 3


def test_text_rows_yields_the_rows_of_every_batch_in_order():
    got = [(ids.shape, row, b) for ids, _, _, row, b in uev._text_rows("f", _texts(2, 3, 1), 6, "cpu")]
    assert got == [((2, 1, 4), 0, 2), ((3, 1, 4), 2, 3), ((1, 1, 4), 5, 1)]
    assert list(uev._text_rows("f", [], 0, "cpu")) == []
