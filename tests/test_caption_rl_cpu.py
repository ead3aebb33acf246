"""Reward-weighted caption training, the part that needs no GPU: the C surface of the three new entry points and the size statement of
the weighted descriptor, argument validation that raises before a device is asked for, and the numpy restatement of the advantage
that tests/test_caption_rl_gpu.py holds the kernel against, checked here on hand-computed cases."""
import argparse
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import univl_oracle as O
from make_golden import case_config
from univl_amd import UniVL, _lib, rl
from univl_amd.sample import SampleResult

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "include", "univl_hip.h")) as _f:
    HEADER = _f.read()


# ------------------------------------------------------------------------------------------------ the restatement
def advantage_restated(reward, baseline=None, scale=1.0):
    """include/univl_hip.h: univl_caption_advantage in numpy fp64, in the kernel's order.  reward [n, ns]; baseline None (leave one
    out) or [n].  Returns (weights [n, ns] float32, status bit)."""
    reward = np.asarray(reward, dtype=np.float64)
    n, ns = reward.shape
    out, flag = np.zeros((n, ns), dtype=np.float32), 0
    for i in range(n):
        total, m = np.float64(0.0), 0
        if baseline is None:
            for s in range(ns):                                  # left to right over the finite rewards
                if np.isfinite(reward[i, s]):
                    total = total + reward[i, s]
                    m += 1
            have = m >= 2
            flag |= int(m < ns)
        else:
            have = bool(np.isfinite(baseline[i]))
            flag |= int(not have)
        for s in range(ns):
            x = reward[i, s]
            if not np.isfinite(x):
                flag |= 1
            elif have:
                adv = x - (total - x) / np.float64(m - 1) if baseline is None else x - np.float64(baseline[i])
                with np.errstate(over="ignore"):
                    w = np.float32(adv * np.float64(scale))      # rounded once
                if np.isfinite(w):
                    out[i, s] = w
                else:
                    flag |= 1
    return out, flag


def test_advantage_restatement_on_hand_computed_cases():
    w, flag = advantage_restated([[1.0, 0.0]])
    assert w.tolist() == [[1.0, -1.0]] and flag == 0
    w, flag = advantage_restated([[0.5, 0.25, 0.75]], scale=2.0)             # others' means: 0.5, 0.625, 0.375
    assert w.tolist() == [[0.0, -0.75, 0.75]] and flag == 0
    w, flag = advantage_restated([[0.5, 0.25, 0.75], [1.0, 1.0, 1.0]], baseline=[0.25, 2.0])
    assert w.tolist() == [[0.25, 0.0, 0.5], [-1.0, -1.0, -1.0]] and flag == 0
    w, flag = advantage_restated([[0.5, float("nan"), 0.75, 0.25]])           # the NaN leaves the baseline of the others: means of two
    assert w.tolist() == [[0.0, 0.0, 0.375, -0.375]] and flag == 1
    w, flag = advantage_restated([[0.5, float("inf")]])                        # one finite reward left: no baseline, no weight
    assert w.tolist() == [[0.0, 0.0]] and flag == 1
    w, flag = advantage_restated([[0.5, 0.25]], baseline=[float("nan")])
    assert w.tolist() == [[0.0, 0.0]] and flag == 1
    w, flag = advantage_restated([[1.0, 0.0]], scale=1e300)                    # not finite in fp32: 0 and the flag
    assert w.tolist() == [[0.0, 0.0]] and flag == 1
    w, _ = advantage_restated([[0.1, 0.2, 0.7]])
    assert w.dtype == np.float32 and w[0, 0] == np.float32(0.1 - (1.0 - 0.1) / 2.0) and abs(float(w.sum())) < 1e-7


# ------------------------------------------------------------------------------------------------ the C surface
NEW = ("univl_vocab_ce_weighted_fwd", "univl_vocab_ce_weighted_bwd", "univl_caption_advantage")


def test_new_symbols_are_declared_exported_and_bound():
    L = _lib.lib()
    declared = set(re.findall(r"\b(univl_[a-z0-9_]+)\s*\(", HEADER))
    for name in NEW + ("univl_vocab_ce_weighted_sizeof",):
        assert name in declared and name in _lib.EXPORTED and hasattr(L, name), name
    assert declared == set(_lib.EXPORTED)
    for name in ("UNIVL_ADV_LOO 0", "UNIVL_ADV_GIVEN 1", "UNIVL_ADV_NONFINITE 1"):
        assert "#define " + name in HEADER
    assert (_lib.ADV_LOO, _lib.ADV_GIVEN, _lib.ADV_NONFINITE) == (0, 1, 1)


def test_weighted_descriptor_mirrors_the_header_and_states_its_size():
    body = re.search(r"typedef struct UnivlVocabCEW \{(.*?)\} UnivlVocabCEW;", HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    kinds = {"int32_t": _lib.i32, "int64_t": _lib.i64, "float": _lib.f32, "ptr": _lib.vp}
    want = []
    for decl in (d.strip() for d in body.split(";")):
        if not decl:
            continue
        m = re.match(r"(?:const\s+)?(\w+)\s*(\*?)\s*(.*)", decl)
        kind = "ptr" if m.group(2) else m.group(1)
        for name in m.group(3).split(","):
            want.append((name.strip().lstrip("*").strip(), kinds[kind]))
    assert [(n, t) for n, t in _lib.VocabCEW._fields_] == want
    assert _lib.VocabCEW._fields_[:len(_lib.VocabCE._fields_)] == _lib.VocabCE._fields_          # UnivlVocabCE's fields lead
    assert _lib.lib().univl_vocab_ce_weighted_sizeof() == C.sizeof(_lib.VocabCEW) == C.sizeof(_lib.VocabCE) + 16


def test_both_size_tables_keep_their_lengths():
    L = _lib.lib()
    assert _lib.VocabCEW not in _lib._STRUCTS and len(_lib._STRUCTS) == 12
    assert L.univl_abi_sizeof(11) > 0 and L.univl_abi_sizeof(12) == -1 and L.univl_struct_size(10) > 0 and L.univl_struct_size(11) == -1


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """Host-side range checks: UNIVL_EINVAL (-1) without touching a device."""
    L = _lib.lib()
    assert L.univl_vocab_ce_weighted_fwd(None, None) == -1 and L.univl_vocab_ce_weighted_bwd(None, None) == -1
    assert L.univl_caption_advantage(None, None, 1, 2, 0, 1.0, None, None, None) == -1
    one = C.c_void_p(16)                                                       # never dereferenced: the range check comes first
    assert L.univl_caption_advantage(one, None, 4, 1, _lib.ADV_LOO, 1.0, one, one, None) == -1          # ns = 1 with leave-one-out
    assert L.univl_caption_advantage(one, None, 4, 2, _lib.ADV_GIVEN, 1.0, one, one, None) == -1        # GIVEN without a baseline
    assert L.univl_caption_advantage(one, None, 0, 2, _lib.ADV_LOO, 1.0, one, one, None) == -1
    assert L.univl_caption_advantage(one, one, 4, 2, 2, 1.0, one, one, None) == -1                      # no such baseline kind
    d = _lib.VocabCEW()
    d.dtype, d.rows, d.V, d.K = _lib.DT_F32, 48, 1000, 768
    for f in ("x", "table", "labels", "partial", "label_logit", "lse", "rowloss", "scratch2", "loss", "dlogits", "seq_weight"):
        setattr(d, f, 16)
    d.ldx = d.ldt = 768
    d.lddl, d.slots, d.ignore_index = 1000, 8, -1
    for seq_len in (0, -3, 7):                                                 # seq_len >= 1 dividing rows
        d.seq_len = seq_len
        assert L.univl_vocab_ce_weighted_fwd(C.byref(d), None) == -1 and b"seq_len" in L.univl_last_error()
        assert L.univl_vocab_ce_weighted_bwd(C.byref(d), None) == -1
    d.seq_len, d.seq_weight = 8, None
    assert L.univl_vocab_ce_weighted_fwd(C.byref(d), None) == -1 and b"seq_weight" in L.univl_last_error()


# ------------------------------------------------------------------------------------------------ validation in Python
def _model(name):
    cfg, rows, seed = case_config(name)
    ns = argparse.Namespace(**cfg.to_dict(), local_rank=0, compute_dtype="fp32")
    model = UniVL.from_pretrained("bert-base-uncased", "visual-base", "cross-base", "decoder-base", task_config=ns)
    return cfg, model.train(), O.synthetic_batch(cfg, rows, seed=seed)


def _forward(model, b, **kw):
    return model(b["input_ids"], b["token_type_ids"], b["attention_mask"], b["video"], b["video_mask"], **kw)


def test_forward_refuses_a_bad_weighted_batch_before_any_device_work():
    """The models live on the CPU: anything that got past the checks would raise RuntimeError (no CPU fallback), not ValueError."""
    cfg, model, b = _model("caption_small")
    B, Wd = 2, cfg.max_words
    caps = lambda nc: dict(input_caption_ids=torch.zeros(B, nc, Wd, dtype=torch.int64), decoder_mask=torch.ones(B, nc, Wd, dtype=torch.int64),
                           output_caption_ids=torch.zeros(B, nc, Wd, dtype=torch.int64))
    with pytest.raises(ValueError, match="caption_weight of shape"):
        _forward(model, b, caption_weight=torch.ones(B), **caps(3))
    with pytest.raises(ValueError, match="caption_weight of shape"):
        _forward(model, b, caption_weight=torch.ones(B + 1, 3), **caps(3))
    with pytest.raises(ValueError, match="caption_weight of shape"):
        _forward(model, b, caption_weight=torch.ones(B, 0), **caps(3))
    with pytest.raises(ValueError, match="input_caption_ids of shape"):
        _forward(model, b, caption_weight=torch.ones(B, 2), **caps(3))
    bad = caps(3)
    bad["decoder_mask"] = bad["decoder_mask"][..., :-1]
    with pytest.raises(ValueError, match="decoder_mask of shape"):
        _forward(model, b, caption_weight=torch.ones(B, 3), **bad)
    with pytest.raises(ValueError, match="needs input_caption_ids"):
        _forward(model, b, caption_weight=torch.ones(B, 3))
    with pytest.raises(RuntimeError, match="HIP device"):                      # a well-formed call gets as far as asking for the device
        _forward(model, b, caption_weight=torch.ones(B, 3), **caps(3))
    cfg1, stage_one, b1 = _model("joint_small")
    with pytest.raises(ValueError, match="without a decoder"):
        _forward(stage_one, b1, caption_weight=torch.ones(b1["input_ids"].shape[0], 1))
    cfgp, pre, bp = _model("pretrain_small")
    with pytest.raises(ValueError, match="stage-two caption mode"):
        _forward(pre, bp, caption_weight=torch.ones(bp["input_ids"].shape[0], 1))
    model.eval()
    assert _forward(model, b, caption_weight=torch.ones(B, 3), **caps(3)) is None               # evaluation mode: no loss, as ever


def _fake_samples(n=2, ns=3, T=5):
    tok = torch.zeros(n, ns, T, dtype=torch.int32)
    z = torch.zeros(n, ns, T)
    return SampleResult(tok, z, z, z[..., 0], z[..., 0], torch.full((n, ns), T, dtype=torch.int32))


def test_caption_rewards_and_advantages_refuse_bad_arguments_before_any_device_work():
    res = _fake_samples()
    ref, rlen = torch.zeros(2, 2, 6, dtype=torch.int64), torch.full((2, 2), 6)
    with pytest.raises(ValueError, match="metric"):
        rl.caption_rewards(res, ref, rlen, 102, 0, metric="cider")
    with pytest.raises(ValueError, match="ref_ids of shape"):
        rl.caption_rewards(res, ref[:1], rlen[:1], 102, 0)
    with pytest.raises(ValueError, match="ref_ids of shape"):
        rl.caption_rewards(res, ref[:, 0], rlen, 102, 0)
    with pytest.raises(ValueError, match="ref_len of shape"):
        rl.caption_rewards(res, ref, rlen[:, :1], 102, 0)
    with pytest.raises(ValueError, match="integer"):
        rl.caption_rewards(res, ref.float(), rlen, 102, 0)
    with pytest.raises(ValueError, match="at most 128"):
        rl.caption_rewards(res, torch.zeros(2, 2, 129, dtype=torch.int64), rlen, 102, 0)
    with pytest.raises(RuntimeError, match="HIP device"):                      # well-formed: the device is asked for, and is not there
        rl.caption_rewards(res, ref, rlen, 102, 0)
    r = torch.zeros(2, 3, dtype=torch.float64)
    with pytest.raises(ValueError, match="float64"):
        rl.advantages(r.float())
    with pytest.raises(ValueError, match="float64"):
        rl.advantages(r[0])
    with pytest.raises(ValueError, match="baseline="):
        rl.advantages(r, baseline="greedy")
    with pytest.raises(ValueError, match="at least 2 samples"):
        rl.advantages(r[:, :1])
    with pytest.raises(ValueError, match="one reward per video"):
        rl.advantages(r, baseline=torch.zeros(3, dtype=torch.float64))
    with pytest.raises(ValueError, match="scale"):
        rl.advantages(r, scale=float("nan"))
    with pytest.raises(RuntimeError, match="HIP device"):
        rl.advantages(r)


def test_graphed_step_refuses_the_weighted_kind():
    from univl_amd.graphed import GraphedTrainStep
    step = GraphedTrainStep.__new__(GraphedTrainStep)                          # the refusal comes before any state is looked at
    with pytest.raises(NotImplementedError, match="caption_weight"):
        step(None, None, None, None, None, caption_weight=torch.ones(2, 3))
