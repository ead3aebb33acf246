"""Host side of query-bank normalised search (no GPU): the entry points are declared, exported and bound, the two descriptors mirror
the C structs and state their sizes through their own _sizeof functions while both numbered size tables stay as they are, the numpy
restatement (tests/qbnorm_ref.py, the reference of tests/test_qbnorm_gpu.py) agrees with the explicit softmax ratio and with the
hand-made hub case, and QueryBank / eval_retrieval_streamed refuse bad arguments before any device work."""
import ctypes as C
import inspect
import os
import re
import types

import numpy as np
import pytest
import torch

from univl_amd import _lib, ops
from univl_amd.retrieval import QueryBank, VideoIndex

import qbnorm_ref as R
from retrieval_cases import header_fields as _header_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "univl_hip.h")).read()
needs_lib = pytest.mark.skipif(not _lib.available(), reason="libunivl_hip.so is not built")
NEW = ("univl_sim_colstat", "univl_sim_colstat_sizeof", "univl_sim_colstat_workspace", "univl_sim_topk_norm", "univl_sim_topk_norm_sizeof",
       "univl_hub_flags", "univl_hub_gate")


# ------------------------------------------------------------------------------------------------ binding
def _params(ret, name):
    m = re.search(r"%s\s+%s\s*\(([^;]*)\)\s*;" % (ret, name), HEADER)
    assert m, "declaration of %s not found" % name
    return [p.strip() for p in m.group(1).split(",")]


@needs_lib
def test_entry_points_are_declared_exported_and_bound():
    L = _lib.lib()
    declared = set(re.findall(r"\b(univl_[a-z0-9_]+)\s*\(", HEADER))
    for name in NEW:
        assert name in declared and name in _lib.EXPORTED and hasattr(L, name), name
    assert declared == set(_lib.EXPORTED)
    for name in ("univl_sim_colstat", "univl_sim_topk_norm"):
        fn = getattr(L, name)
        assert fn.restype is C.c_int32 and len(fn.argtypes) == len(_params("int", name)) == 2
    for name in ("univl_hub_flags", "univl_hub_gate"):
        fn, params = getattr(L, name), _params("int", name)
        assert fn.restype is C.c_int32 and len(fn.argtypes) == len(params)
        for p, t in zip(params, fn.argtypes):
            want = C.c_void_p if ("*" in p or "hipStream_t" in p) else (C.c_int64 if p.startswith("int64_t") else C.c_int32)
            assert t is want, (name, p, t)
    fn, params = L.univl_sim_colstat_workspace, _params("int64_t", "univl_sim_colstat_workspace")
    assert fn.restype is C.c_int64 and len(fn.argtypes) == len(params) == 2
    assert all(t is C.c_int32 and p.startswith("int32_t ") for p, t in zip(params, fn.argtypes))
    for name in ("sim_colstat", "sim_topk_norm", "hub_flags", "hub_gate"):
        assert callable(getattr(ops, name))


@needs_lib
def test_descriptors_mirror_the_header_and_the_numbered_tables_are_unchanged():
    L = _lib.lib()
    assert list(_lib.SimColstat._fields_) == _header_fields("UnivlSimColstat")
    assert list(_lib.SimTopkNorm._fields_) == _header_fields("UnivlSimTopkNorm")
    assert _lib.SimTopkNorm._fields_[:len(_lib.SimTopk._fields_)] == _lib.SimTopk._fields_     # the plain search's fields come first
    assert L.univl_sim_colstat_sizeof() == C.sizeof(_lib.SimColstat)
    assert L.univl_sim_topk_norm_sizeof() == C.sizeof(_lib.SimTopkNorm) == C.sizeof(_lib.SimTopk) + 16
    assert _lib.SimColstat not in _lib._STRUCTS and _lib.SimTopkNorm not in _lib._STRUCTS and len(_lib._STRUCTS) == 12
    assert L.univl_abi_sizeof(12) == -1 and L.univl_struct_size(11) == -1
    assert int(re.search(r"#define UNIVL_COLSTAT_SLICES (\d+)", HEADER).group(1)) == _lib.COLSTAT_SLICES


@needs_lib
def test_colstat_workspace_is_a_function_of_the_bank_size_alone():
    """8 * S * Ng bytes with S as the header derives it from Nb; bad arguments < 0 with a message."""
    L = _lib.lib()
    for Nb in (1, 128, 129, 1000, 4096, 4097, 10 ** 4, 10 ** 6):
        T = -(-Nb // 128)
        S = -(-T // -(-T // _lib.COLSTAT_SLICES))
        assert 1 <= S <= _lib.COLSTAT_SLICES
        for Ng in (1, 33, 10 ** 5):
            assert L.univl_sim_colstat_workspace(Nb, Ng) == 8 * S * Ng, (Nb, Ng)
    for bad in ((0, 5), (5, 0), (-1, 5)):
        assert L.univl_sim_colstat_workspace(*bad) < 0
        assert b"univl_sim_colstat_workspace" in L.univl_last_error()


@needs_lib
def test_no_cpu_fallback_and_null_descriptors():
    x = torch.zeros(2, 768)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.sim_colstat(x, x, 1.0)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.sim_topk_norm(x, x, 1, torch.zeros(2))
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.hub_flags(torch.zeros(2, dtype=torch.int32), 4)
    L = _lib.lib()
    assert L.univl_sim_colstat(None, None) == -1 and L.univl_sim_topk_norm(None, None) == -1       # UNIVL_EINVAL before any device call


# ------------------------------------------------------------------------------------------------ the reference, by itself
def test_ref_ranking_by_s_minus_c_is_ranking_by_the_softmax_ratio():
    rng = np.random.default_rng(5)
    for beta in (1.0, 20.0):
        sb, sq = rng.normal(size=(40, 25)) * 0.3, rng.normal(size=(7, 25)) * 0.3
        c = R.colstat(sb, beta)
        assert np.allclose(c, np.log(np.exp(beta * sb).sum(0)) / beta, rtol=0, atol=1e-12)
        ratio = np.exp(beta * sq) / np.exp(beta * sb).sum(0)[None, :]                # QB-Norm's inverted softmax, explicitly
        assert np.array_equal(R.ranked(sq - c[None, :]), R.ranked(ratio))
        assert not np.array_equal(R.ranked(sq), R.ranked(ratio))                     # and it is not the raw ranking
    big = np.array([[3000.0, -2000.0], [2800.0, -2000.0]])                          # max-shifted: no overflow
    assert np.allclose(R.colstat(big, 1.0), [3000.0, -2000.0 + np.log(2.0)], rtol=0, atol=1e-9)


def test_ref_tie_rule_padding_and_counts():
    sp = np.array([[1.0, 3.0, 3.0, 0.0], [2.0, 2.0, 2.0, 2.0]], dtype=np.float32)
    idx, score, gt, eq = R.search(sp, 6, target=[2, 3])
    assert idx.tolist() == [[1, 2, 0, 3, -1, -1], [0, 1, 2, 3, -1, -1]]
    assert score[0].tolist() == [3.0, 3.0, 1.0, 0.0, -np.inf, -np.inf]
    assert gt.tolist() == [0, 0] and eq.tolist() == [2, 4]
    # the gate: zero leaves the row untouched, bit for bit
    s = np.array([[1.5, 2.5]], dtype=np.float32)
    assert np.array_equal(R.normalised(s, [0.25, 0.5], [0]), s) and R.normalised(s, [0.25, 0.5], [1]).tolist() == [[1.25, 2.0]]


def test_ref_hub_case_worked_by_hand():
    q, g, bank = R.hub_case()
    sq, sb = (q.astype(np.int64) @ g.astype(np.int64).T), (bank.astype(np.int64) @ g.astype(np.int64).T)
    want = np.full((8, 9), 8)
    want[np.arange(8), np.arange(8)] = 24
    want[:, 8] = 30
    assert np.array_equal(sq[:8], want) and sq[8].tolist() == [72, 0, 0, 0, 0, 0, 0, 0, 27]
    assert R.ranked(sq)[:, 0].tolist() == [8] * 8 + [0]                             # every raw top-1 of the eight is the hub
    hub = R.hub_flags(sb, 1)
    assert hub.tolist() == [0] * 8 + [1]
    assert R.hub_flags(sb, 2).tolist() == [1] * 9                                   # the second best of bank row i is video i
    c = R.colstat(sb, 1.0)
    assert abs(c[8] - (30 + np.log(8))) < 1e-12 and np.all(np.abs(c[:8] - (24 + np.log1p(7 * np.exp(-16.0)))) < 1e-12)   # 24 + 7.9e-7
    gate = R.hub_gate(sq, hub)
    assert gate.tolist() == [1] * 8 + [0] and R.hub_gate(sq, hub, dynamic=False).tolist() == [1] * 9
    sp = R.normalised(sq, c, gate)
    assert R.ranked(sp)[:8, 0].tolist() == list(range(8))                           # every normalised top-1 is the true video
    assert np.allclose(sp[np.arange(8), np.arange(8)] - sp[:8, 8], np.log(8), atol=1e-5)        # margin ~ 2.08 over the hub
    assert np.array_equal(sp[8], sq[8].astype(np.float32))                          # the ninth query is not gated ...
    assert R.normalised(sq, c, R.hub_gate(sq, hub, dynamic=False))[8, 0] == np.float32(72) - np.float32(c[0])   # ... unless static


# ------------------------------------------------------------------------------------------------ ValueErrors before any device work
def _cpu_index(n=0, device="cpu"):
    model = types.SimpleNamespace(flat=types.SimpleNamespace(device=torch.device(device)))
    index = VideoIndex(model, capacity=4)
    index._n = n
    return index


def test_query_bank_refuses_bad_arguments_on_the_host():
    index = _cpu_index()
    for beta in (0, -1.0, float("inf"), float("nan"), 1e-50, 1e39, "20", None, True):
        with pytest.raises(ValueError, match="beta"):
            QueryBank(index, beta=beta)
    for hub_k in (0, -1, _lib.TOPK_MAX + 1, 1.5, True):
        with pytest.raises(ValueError, match="hub_k"):
            QueryBank(index, hub_k=hub_k)
    bank = QueryBank(index)
    assert (bank.beta, bank.hub_k, bank.dynamic, len(bank)) == (20.0, 1, True, 0)
    assert QueryBank(index, beta=1, hub_k=_lib.TOPK_MAX, dynamic=False).hub_k == _lib.TOPK_MAX
    with pytest.raises(ValueError, match="empty"):
        bank.fit()                                                                  # an empty bank
    with pytest.raises(ValueError, match=r"bank\.fit\(\)"):
        bank.check_fitted(index)
    for prop in ("c", "hub"):                                                        # nothing fitted: the properties say so too
        with pytest.raises(ValueError, match=r"bank\.fit\(\)"):
            getattr(bank, prop)
    # a bank on another device than the index
    far = QueryBank(_cpu_index(device="cuda:0"))
    with pytest.raises(ValueError, match="index is on"):
        far.add_vectors(torch.zeros(2, 768))
    assert len(far) == 0


def test_stale_and_foreign_banks_are_refused_by_search():
    index = _cpu_index(n=3)
    bank = QueryBank(index)
    assert bank.add_vectors(torch.zeros(2, 768)) == 2 and bank.add_vectors(torch.ones(70, 768)) == 72      # growth keeps the rows
    assert bank.vectors.shape == (72, 768) and float(bank.vectors[:2].abs().max()) == 0.0 and float(bank.vectors[2:].min()) == 1.0
    with pytest.raises(ValueError, match=r"bank\.fit\(\)"):
        index.search_vectors(torch.zeros(1, 768), 1, bank=bank)                     # never fitted
    bank._covered = 3                                                               # as after fit() ...
    bank.check_fitted(index)
    index._n = 5                                                                    # ... then the index grew
    with pytest.raises(ValueError, match=r"bank\.fit\(\)"):
        index.search_vectors(torch.zeros(1, 768), 1, bank=bank)
    with pytest.raises(ValueError, match="another VideoIndex"):
        _cpu_index(n=3).search_vectors(torch.zeros(1, 768), 1, bank=bank)
    bank._covered = 5
    bank.add_vectors(torch.zeros(1, 768))                                           # more bank rows invalidate everything
    assert bank._covered == 0 and bank._c is None and bank._hub is None


def test_entry_points_take_the_bank():
    from univl_amd.eval import eval_retrieval_streamed
    assert inspect.signature(VideoIndex.search).parameters["bank"].default is None
    assert inspect.signature(VideoIndex.search_vectors).parameters["bank"].default is None
    p = inspect.signature(eval_retrieval_streamed).parameters
    assert list(p)[:6] == ["model", "text_batches", "video_batches", "targets", "device", "capacity"]        # unchanged in front
    assert (p["bank_batches"].default, p["beta"].default, p["hub_k"].default, p["dynamic"].default) == (None, 20.0, 1, True)
    with pytest.raises(ValueError, match="beta"):
        eval_retrieval_streamed(None, [], [], [], bank_batches=[], beta=0.0)        # before the model is touched
