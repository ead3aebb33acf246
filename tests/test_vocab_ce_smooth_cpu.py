"""Label smoothing of the caption loss, the part that needs no GPU: the C surface of the smoothed form of K16 (univl_vocab_ce_smooth_fwd /
_bwd) and the size statement of its descriptor, the range checks that come before any launch, UniVL.caption_label_smoothing (validation,
step key, plans that build on the CPU) and the refusal of the materialised-logits path."""
import argparse
import ctypes as C
import os
import re

import pytest
import torch

import univl_oracle as O
from univl_amd import UniVL, _lib
from univl_amd.engine import FlatParams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "include", "univl_hip.h")) as _f:
    HEADER = _f.read()

NEW = ("univl_vocab_ce_smooth_sizeof", "univl_vocab_ce_smooth_fwd", "univl_vocab_ce_smooth_bwd")


# ------------------------------------------------------------------------------------------------ the C surface
def test_new_symbols_are_declared_exported_and_bound():
    L = _lib.lib()
    declared = set(re.findall(r"\b(univl_[a-z0-9_]+)\s*\(", HEADER))
    for name in NEW:
        assert name in declared and name in _lib.EXPORTED and hasattr(L, name), name
    assert declared == set(_lib.EXPORTED)


def test_smoothed_descriptor_mirrors_the_header_and_states_its_size():
    body = re.search(r"typedef struct UnivlVocabCES \{(.*?)\} UnivlVocabCES;", HEADER, re.S).group(1)
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
    assert [(n, t) for n, t in _lib.VocabCES._fields_] == want
    assert _lib.VocabCES._fields_[:len(_lib.VocabCEW._fields_)] == _lib.VocabCEW._fields_          # UnivlVocabCEW's fields lead
    assert [n for n, _ in _lib.VocabCES._fields_[len(_lib.VocabCEW._fields_):]] == ["smoothing", "reserved2", "partial_sum"]
    assert _lib.lib().univl_vocab_ce_smooth_sizeof() == C.sizeof(_lib.VocabCES) == C.sizeof(_lib.VocabCEW) + 16


def test_both_size_tables_keep_their_lengths():
    L = _lib.lib()
    assert _lib.VocabCES not in _lib._STRUCTS and len(_lib._STRUCTS) == 12
    assert L.univl_abi_sizeof(11) > 0 and L.univl_abi_sizeof(12) == -1 and L.univl_struct_size(10) > 0 and L.univl_struct_size(11) == -1


def _descriptor(smoothing=0.1, weights=True):
    """Well-formed as far as the host-side checks go; the pointers are never dereferenced: a range check comes first."""
    d = _lib.VocabCES()
    d.dtype, d.rows, d.V, d.K = _lib.DT_F32, 48, 1000, 768
    for f in ("x", "table", "labels", "partial", "label_logit", "lse", "rowloss", "scratch2", "loss", "dlogits", "partial_sum"):
        setattr(d, f, 16)
    d.ldx = d.ldt = 768
    d.lddl, d.slots, d.ignore_index = 1000, 8, -1
    d.smoothing = smoothing
    if weights:
        d.seq_weight, d.seq_len = 16, 8
    return d


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """UNIVL_EINVAL (-1) without touching a device."""
    L = _lib.lib()
    both = (L.univl_vocab_ce_smooth_fwd, L.univl_vocab_ce_smooth_bwd)
    for fn in both:
        assert fn(None, None) == -1
    for weights in (False, True):
        for bad in (-0.1, 1.0, 1.5, float("nan"), float("inf"), float("-inf")):
            d = _descriptor(bad, weights)
            for fn in both:
                assert fn(C.byref(d), None) == -1 and b"smoothing" in L.univl_last_error(), bad
        d = _descriptor(0.1, weights)
        d.partial_sum = None
        for fn in both:
            assert fn(C.byref(d), None) == -1 and b"partial_sum" in L.univl_last_error()
    for eps in (0.0, 0.1):                                                     # with weights: seq_len >= 1 dividing rows
        for seq_len in (0, -3, 7):
            d = _descriptor(eps)
            d.seq_len = seq_len
            for fn in both:
                assert fn(C.byref(d), None) == -1 and b"seq_len" in L.univl_last_error(), (eps, seq_len)
    d = _descriptor(0.1)                                                       # the checks of the unsmoothed forms still apply
    d.lse = None
    assert L.univl_vocab_ce_smooth_fwd(C.byref(d), None) == -1 and b"null buffer" in L.univl_last_error()
    d = _descriptor(0.1)
    d.K = 100
    assert L.univl_vocab_ce_smooth_fwd(C.byref(d), None) == -1


# ------------------------------------------------------------------------------------------------ the property
def _model(dt="fp32", **kw):
    cfg = O.OracleConfig(**dict(dict(batch_size=2, text_num_hidden_layers=1, visual_num_hidden_layers=1, max_words=16, max_frames=16), **kw))
    ns = argparse.Namespace(**cfg.to_dict(), local_rank=0, compute_dtype=dt)
    m = UniVL.from_pretrained("bert-base-uncased", "visual-base", "cross-base", "decoder-base", task_config=ns)
    return m.train(), cfg


CAPTION = dict(stage_two=True, task_type="caption", cross_num_hidden_layers=1, decoder_num_hidden_layers=1)
PRETRAIN = dict(stage_two=True, do_pretrain=True, use_mil=True, cross_num_hidden_layers=1, decoder_num_hidden_layers=1)


def test_property_defaults_to_zero_and_validates_its_range():
    m, _ = _model(**CAPTION)
    assert m.caption_label_smoothing == 0.0
    for bad in (-0.1, 1.0, 1.5, float("nan"), float("inf"), "a lot", None):
        with pytest.raises(ValueError, match="caption_label_smoothing"):
            m.caption_label_smoothing = bad
        assert m.caption_label_smoothing == 0.0
    m.caption_label_smoothing = 0.1
    assert m.caption_label_smoothing == 0.1
    m.caption_label_smoothing = 0
    assert m.caption_label_smoothing == 0.0


def test_step_key_carries_the_value_and_the_setter_drops_the_cached_steps():
    m, _ = _model(**CAPTION)
    m._flat, m._seed_dev = FlatParams(list(m.named_parameters()), "cpu", torch.float32), torch.zeros(1, dtype=torch.int64)
    plain = {k: m._step_key(k, 2, 16, 16) for k in ("caption", "pretrain", "align", "joint")}
    assert plain["caption"] == ("caption", 2, 16, 16, True)                     # at 0: the keys of a model without the property
    assert m._step_key("caption_weighted", 2, 16, 16, 3, 16) == ("caption_weighted", 2, 16, 16, True, 3, 16)
    m._steps["sentinel"] = object()
    m.caption_label_smoothing = 0.0                                            # no change: nothing is dropped
    assert "sentinel" in m._steps
    m.caption_label_smoothing = 0.1
    assert m._steps == {}
    for kind in ("caption", "pretrain"):
        assert m._step_key(kind, 2, 16, 16) != plain[kind] and m._step_key(kind, 2, 16, 16)[:5] == plain[kind]
    assert m._step_key("caption_weighted", 2, 16, 16, 3, 16) != ("caption_weighted", 2, 16, 16, True, 3, 16)
    for kind in ("align", "joint"):                                            # no decoder loss in these
        assert m._step_key(kind, 2, 16, 16) == plain[kind]
    k1 = m._step_key("caption", 2, 16, 16)
    m._steps["sentinel"] = object()
    m.caption_label_smoothing = 0.2
    assert m._steps == {} and m._step_key("caption", 2, 16, 16) not in (k1, plain["caption"])
    m.caption_label_smoothing = 0.0
    assert m._step_key("caption", 2, 16, 16) == plain["caption"]


def _names(plan):
    return [op.name for op in plan.ops]


def _flat_on_cpu(m):
    m._flat, m._seed_dev = FlatParams(list(m.named_parameters()), "cpu", torch.float32), torch.zeros(1, dtype=torch.int64)
    return m


def test_caption_plans_take_the_smoothed_entry_points_only_when_asked():
    from univl_amd.steps import build_step
    m, _ = _model(**CAPTION)
    _flat_on_cpu(m)
    st0 = build_step(m, "caption", 2, 16, 16, True)
    f0, b0 = _names(st0.fwd), _names(st0.backward_plan(True))
    assert f0.count("univl_vocab_ce_fwd") == 1 and b0.count("univl_vocab_ce_bwd") == 1
    m.caption_label_smoothing = 0.1
    st = build_step(m, "caption", 2, 16, 16, True)
    f1, b1 = _names(st.fwd), _names(st.backward_plan(True))
    # one more plan node KIND, not one more node: the same plans with the two entry points exchanged
    assert f1 == [("univl_vocab_ce_smooth_fwd" if n == "univl_vocab_ce_fwd" else n) for n in f0]
    assert b1 == [("univl_vocab_ce_smooth_bwd" if n == "univl_vocab_ce_bwd" else n) for n in b0]
    head = st.decoder.head
    assert isinstance(head.k16["desc"], _lib.VocabCES) and abs(head.k16["desc"].smoothing - 0.1) < 1e-8
    assert tuple(head.k16["partial_sum"].shape) == (2 * 16, head.k16["desc"].slots)
    assert head.k16["desc"].partial_sum == head.k16["partial_sum"].data_ptr() and not head.k16["desc"].seq_weight
    stw = build_step(m, "caption_weighted", 2, 16, 16, True, n_cand=3, Wd=16)
    fw, bw = _names(stw.fwd), _names(stw.backward_plan(True))
    assert "univl_vocab_ce_smooth_fwd" in fw and "univl_vocab_ce_weighted_fwd" not in fw
    assert "univl_vocab_ce_smooth_bwd" in bw and "univl_vocab_ce_weighted_bwd" not in bw
    dw = stw.decoder.head.k16["desc"]
    assert dw.seq_weight == stw.decoder.head.weight.data_ptr() and dw.seq_len == 16 and dw.rows == 2 * 3 * 16
    m.caption_label_smoothing = 0.0
    st2 = build_step(m, "caption", 2, 16, 16, True)
    assert _names(st2.fwd) == f0 and _names(st2.backward_plan(True)) == b0
    assert isinstance(st2.decoder.head.k16["desc"], _lib.VocabCE) and "partial_sum" not in st2.decoder.head.k16


def test_pretrain_smooths_the_decoder_term_only():
    from univl_amd.steps import build_step
    m, _ = _model(**PRETRAIN)
    _flat_on_cpu(m)
    m.caption_label_smoothing = 0.1
    st = build_step(m, "pretrain", 2, 16, 16, True)
    f, b = _names(st.fwd), _names(st.backward_plan(True))
    assert f.count("univl_vocab_ce_fwd") == 1 and f.count("univl_vocab_ce_smooth_fwd") == 1
    assert b.count("univl_vocab_ce_bwd") == 1 and b.count("univl_vocab_ce_smooth_bwd") == 1
    assert isinstance(st.heads.mlm.k16["desc"], _lib.VocabCE) and st.heads.mlm.smoothing == 0.0
    assert isinstance(st.decoder.head.k16["desc"], _lib.VocabCES)
    nocap = build_step(m, "pretrain_nocap", 2, 16, 16, True)                    # no decoder term: nothing to smooth
    assert "univl_vocab_ce_smooth_fwd" not in _names(nocap.fwd)


def test_materialised_logits_path_refuses_label_smoothing(ab):
    from univl_amd.steps import build_step
    m, _ = _model(**CAPTION)
    _flat_on_cpu(m)
    ab(vocab_ce=0)
    assert "univl_vocab_ce_fwd" not in _names(build_step(m, "caption", 2, 16, 16, True).fwd)      # the 62 MB logits path, unsmoothed
    m.caption_label_smoothing = 0.1
    with pytest.raises(RuntimeError, match=r"label smoothing exists only in K16 \(univl_vocab_ce_smooth_fwd / _bwd\); UNIVL_VOCAB_CE=0 "
                                           r"has no smoothed form"):
        build_step(m, "caption", 2, 16, 16, True)
    with pytest.raises(RuntimeError, match="no smoothed form"):
        build_step(m, "caption_weighted", 2, 16, 16, True, n_cand=2, Wd=16)
