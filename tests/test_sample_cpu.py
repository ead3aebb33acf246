"""Host side of caption sampling (no GPU): univl_sample_step is declared, exported and bound, the descriptor mirrors the C struct,
the CPU restatement of the contract (tests/test_sample_gpu.py: _expect) gives hand-computed answers, the seeded inputs of the GPU
tests are free of ties where it matters and leave few undecided draws, and there is no CPU fallback."""
import argparse
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import univl_oracle as O
from univl_amd import _lib, ops
from univl_amd.sample import CaptionSampler, SampleResult

import test_sample_gpu as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "univl_hip.h")).read()


def test_sample_step_is_declared_exported_and_bound():
    """The pattern of tests/test_retrieve_cpu.py::test_sim_topk_is_declared_exported_and_bound."""
    L = _lib.lib()
    declared = set(re.findall(r"\b(univl_[a-z0-9_]+)\s*\(", HEADER))
    for name in ("univl_sample_step", "univl_abi_sizeof"):
        assert name in declared and name in _lib.EXPORTED and hasattr(L, name)
    assert declared == set(_lib.EXPORTED)
    m = re.search(r"int\s+univl_sample_step\s*\(([^;]*)\)\s*;", HEADER)
    assert m, "declaration not found"
    params = [p.strip() for p in m.group(1).split(",")]
    fn = L.univl_sample_step
    assert fn.restype is C.c_int32 and len(fn.argtypes) == len(params) == 2
    for p, t in zip(params, fn.argtypes):
        assert (t is C.c_void_p) == ("*" in p or "hipStream_t" in p), (p, t)
    assert callable(ops.sample_step_desc) and callable(ops.sample_step) and callable(ops.sample_ws)


def test_sample_step_struct_mirrors_the_header():
    """Field for field (names, order, kinds), and sizeof against the library: struct #11 of univl_abi_sizeof, the table that continues
    univl_struct_size (whose own eleven entries and -1 past them stay as they are)."""
    body = re.search(r"typedef struct UnivlSampleStep \{(.*?)\} UnivlSampleStep;", HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    kinds = {"int32_t": _lib.i32, "int64_t": _lib.i64, "uint64_t": _lib.u64, "float": _lib.f32, "ptr": _lib.vp}
    want = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(const\s+)?(\w+)\s*(\*?)\s*(.*)", decl)
        for nm in m.group(4).split(","):
            want.append((nm.strip(), kinds["ptr" if m.group(3) else m.group(2)]))
    assert [(n, t) for n, t in _lib.SampleStep._fields_] == want
    L = _lib.lib()
    assert _lib._STRUCTS[11] is _lib.SampleStep and len(_lib._STRUCTS) == 12
    assert L.univl_abi_sizeof(11) == C.sizeof(_lib.SampleStep) and L.univl_abi_sizeof(12) == -1 and L.univl_abi_sizeof(-1) == -1
    for k in range(11):
        assert L.univl_abi_sizeof(k) == L.univl_struct_size(k) == C.sizeof(_lib._STRUCTS[k])
    assert int(re.search(r"#define UNIVL_SAMPLE_KMAX (\d+)", HEADER).group(1)) == _lib.SAMPLE_KMAX == 64
    assert int(re.search(r"#define UNIVL_SAMPLE_SLICES (\d+)", HEADER).group(1)) == _lib.SAMPLE_SLICES


def test_mix32_and_the_draw():
    """mix32 is the murmur3 64-bit finaliser's low word (fmix64(1) = 0xb456bcfc34c2cb2c), keyed as the dropout masks are."""
    assert G.mix32(0) == 0 and G.mix32(1) == 0x34C2CB2C
    key = ((5 * 0x9E3779B97F4A7C15) & G.MASK64) ^ ((3 * 0xD1B54A32D192ED03 + 2) & G.MASK64)
    assert G.draw_u(5, 3, 2) == (G.mix32(key) >> 8) / 2.0 ** 24
    assert 0.0 <= G.draw_u(G.MASK64, 31, 79) < 1.0
    assert G.draw_u(1 << 64, 0, 0) == G.draw_u(0, 0, 0)                   # the seed is a 64-bit word
    us = [G.draw_u(9, t, r) for t in range(4) for r in range(64)]
    assert len(set(us)) == len(us) and 0.4 < sum(us) / len(us) < 0.6


def _seed_with_u(lo, hi, t=0, r=0):
    for seed in range(10000):
        if lo <= G.draw_u(seed, t, r) < hi:
            return seed
    raise AssertionError("no seed")


def test_expect_on_hand_computed_cases():
    """x = [1, 3, 3, 2, 3]: the three equal maxima come in column order; w = (1, 1, 1, 1/e); m under top_p; the draw from a known u."""
    x = np.array([1.0, 3.0, 3.0, 2.0, 3.0], dtype=np.float32)
    e = G._expect(x, 4, 1.0, 1.0, 0, 0, 0)
    assert e["cols"].tolist() == [1, 2, 4, 3] and e["m"] == 4
    c = [1.0, 2.0, 3.0, 3.0 + np.exp(-1.0)]
    # top_p: c_{m-1} >= top_p * c_3 = top_p * 3.3679
    for top_p, m in ((0.2, 1), (0.5, 2), (0.6, 3), (0.85, 3), (0.95, 4), (1.0, 4), (7.0, 4)):
        assert G._expect(x, 4, 1.0, top_p, 0, 0, 0)["m"] == m, top_p
    # the draw: tau = u * c_{m-1}; j = the first c_j > tau
    for lo, hi, top_p, j in ((0.0, 0.25, 1.0, 0), (0.35, 0.55, 1.0, 1), (0.65, 0.85, 1.0, 2), (0.95, 1.0, 1.0, 3), (0.55, 0.95, 0.5, 1),
                             (0.05, 0.45, 0.5, 0)):
        seed = _seed_with_u(lo, hi, t=2, r=7)
        e = G._expect(x, 4, 1.0, top_p, seed, 2, 7)
        assert e["j"] == j and e["token"] == [1, 2, 4, 3][j], (lo, hi, top_p)
        assert abs(e["q_logprob"] - np.log([1.0, 1.0, 1.0, np.exp(-1.0)][j] / c[e["m"] - 1])) < 1e-12
        lse = np.log(np.exp(-2.0) + 3.0 + np.exp(-1.0))
        assert abs(e["tok_logprob"] - ((x[e["token"]] - 3.0) - lse)) < 1e-12
    # temperature: the fp32 product of the fp32 difference with fp32(1 / T)
    e = G._expect(x, 4, 0.7, 1.0, 0, 0, 0)
    a = np.float32(np.float32(-1.0) * np.float32(1.0 / 0.7))
    assert abs(e["q_logprob"] - np.log(1.0 / (3.0 + np.exp(np.float64(a))))) < 1e-12 and e["j"] == 0    # u(0, 0, 0) = 0
    # a draw that sits on a boundary is undecided, one in the middle of an interval is decided
    seed = _seed_with_u(0.4, 0.5, t=0, r=0)
    assert G._expect(x, 4, 1.0, 1.0, seed, 0, 0)["decided"]
    flat = np.array([0.0, -200.0, -300.0], dtype=np.float32)              # c = (1, 1, 1): tau within 1e-4 of them only for u > 0.9999
    assert G._expect(flat, 3, 1.0, 1.0, seed, 0, 0)["decided"] and G._expect(flat, 3, 1.0, 1.0, seed, 0, 0)["token"] == 0


def test_seeded_inputs_are_tie_free_where_it_matters():
    """Among every row's 65 largest candidates (the top 64 and the one behind them) no two are equal, so the order of the lists the
    GPU test compares does not hang on the tie rule in A; and no candidate reaches the padding's marker."""
    for V, ld in G.A_SHAPES:
        for R in G.A_ROWS:
            x = G.a_logits(V, ld, R)
            assert x.shape == (R, ld) and x.dtype == np.float32
            top = -np.sort(-x[:, :V], axis=1)[:, :min(65, V)]
            assert bool((top[:, 1:] < top[:, :-1]).all()), (V, R)
            assert float(x[:, :V].max()) < 100.0 and (ld == V or bool((x[:, V:] == np.float32(3e38)).all()))


def test_undecided_share_of_the_seeded_cases():
    """Every case of A and D that can be formed without a GPU: the undecided share of _expect alone stays under the 5 % cap, D's seeds
    pass the chi-square bound and the nucleus excludes columns."""
    worst = 0.0
    for V, ld in G.A_SHAPES:
        for R in G.A_ROWS:
            active = [not f for f in G.a_done(R)]
            for k in G.a_ks(V):
                for temperature, top_p in G.A_SAMPLING:
                    for t in G.A_POSITIONS:
                        share = G.undecided_share(G.a_case(V, ld, R, k, temperature, top_p, t)[1], active)
                        worst = max(worst, share)
                        assert share <= G.UNDECIDED_CAP, (V, R, k, temperature, top_p, t, share)
    for top_p in (1.0, 0.6):
        seed = G.d_seed(top_p)
        exps, counts = G.d_expect_counts(top_p, seed)
        p = G.d_probs(top_p)
        assert abs(p.sum() - 1.0) < 1e-12
        share = sum(1 for e in exps if not e["decided"]) / len(exps)
        worst = max(worst, share)
        assert share <= G.UNDECIDED_CAP and G.chi_square(counts, p) < G.CHI2_7DOF
        assert all(counts[v] == 0 for v in range(8) if p[v] == 0)
        assert (sum(1 for v in range(8) if p[v] == 0) == 5) if top_p < 1 else bool((p > 0).all())
    print("[sample cpu] worst undecided share %.2f %%" % (100 * worst))


def test_sample_result_reshapes_without_a_device():
    tok = torch.tensor([[[5, 6, -1], [7, -1, -1]]], dtype=torch.int32)
    z = torch.zeros(1, 2, 3)
    r = SampleResult(tok, z, z, z[..., 0], z[..., 0], torch.tensor([[2, 1]], dtype=torch.int32))
    assert r.hypotheses() == [[[5, 6], [7]]]
    with pytest.raises(RuntimeError, match="HIP device"):
        r.captions(6, -1)


def test_caption_sampler_has_no_cpu_fallback():
    cfg = O.OracleConfig(batch_size=2, text_num_hidden_layers=1, visual_num_hidden_layers=1, cross_num_hidden_layers=1,
                         decoder_num_hidden_layers=1, stage_two=True, task_type="caption", max_words=16, max_frames=16)
    ns = argparse.Namespace(**cfg.to_dict(), local_rank=0, compute_dtype="bf16")
    from univl_amd import UniVL
    model = UniVL.from_pretrained("bert-base-uncased", "visual-base", "cross-base", "decoder-base", task_config=ns)
    with pytest.raises(RuntimeError, match="HIP device"):             # the model was never moved to a device
        CaptionSampler(model, 2, 16, 16)
    for kw in (dict(n_samp=0), dict(n_samp=9), dict(top_k=0), dict(top_k=65), dict(temperature=0.0), dict(top_p=0.0)):
        with pytest.raises(ValueError):
            CaptionSampler(model, 2, 16, 16, **kw)
