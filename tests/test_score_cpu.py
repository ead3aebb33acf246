"""Host-side pieces of caption scoring (univl_amd.score, eval.eval_caption_loss, ops.vocab_score): no GPU, no compute call into the
library.  The teacher-forcing construction of score_beams against a Python restatement, the arithmetic of normalized() and of the
loss result, the refusal of host tensors, and the ctypes mirror of UnivlVocabScore against the header and the library."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from univl_amd import _lib, ops
from univl_amd.eval import CaptionLossResult
from univl_amd.score import CaptionScores, beam_inputs_labels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def python_inputs_labels(hyp, length, bos, eos, pad, Wd):
    """One hypothesis (a list of Tmax ids, -1 padded) -> (inputs, labels, mask), each Wd long: the labels are the first `length` tokens
    up to and including the first eos, the inputs are [bos] + those labels without the last, the rest is pad / -1 / 0."""
    toks = list(hyp[:max(0, min(int(length), len(hyp)))])
    if eos >= 0 and eos in toks:
        toks = toks[:toks.index(eos) + 1]
    k = len(toks)
    return ([bos] + toks[:-1] if k else []) + [pad] * (Wd - k), toks + [-1] * (Wd - k), [1] * k + [0] * (Wd - k)


BOS, EOS, PAD = 101, 102, 0


@pytest.mark.parametrize("Wd", [6, 9])
def test_beam_inputs_labels_match_the_python_restatement(Wd):
    """eos inside the length, eos at the last position, no eos, length 0, eos only past the length, two eos, a length beyond Tmax; two
    hypotheses per instance that share the instance's length."""
    T = 6
    rows = [([7, 8, EOS, 9, 10, 11], [7, EOS, 8, 9, 10, 11], 5),          # eos inside
            ([7, 8, 9, 10, 11, EOS], [EOS, 8, 9, 10, 11, 12], 6),         # eos at the last position / at the first
            ([7, 8, 9, 10, 11, 12], [7, 8, 9, 10, 11, 12], 6),            # none
            ([7, 8, 9, -1, -1, -1], [EOS, 8, 9, -1, -1, -1], 0),          # length 0
            ([7, 8, 9, EOS, -1, -1], [7, 8, 9, 10, EOS, -1], 3),          # eos past the length does not cut
            ([7, EOS, 9, EOS, 11, 12], [7, 8, 9, 10, -1, -1], 4),         # the first of two
            ([7, 8, 9, 10, 11, 12], [7, 8, 9, 10, 11, EOS], 9)]           # length clamped to Tmax
    tokens = torch.tensor([[a, b] for a, b, _ in rows], dtype=torch.int32)
    lengths = torch.tensor([l for _, _, l in rows], dtype=torch.int32)
    inputs, labels, mask = beam_inputs_labels(tokens, lengths, BOS, EOS, PAD, Wd)
    assert inputs.shape == labels.shape == mask.shape == (len(rows), 2, Wd)
    assert inputs.dtype == labels.dtype == mask.dtype == torch.int64
    for i, (a, b, l) in enumerate(rows):
        for k, hyp in enumerate((a, b)):
            wi, wl, wm = python_inputs_labels(hyp, l, BOS, EOS, PAD, Wd)
            assert inputs[i, k].tolist() == wi and labels[i, k].tolist() == wl and mask[i, k].tolist() == wm, (i, k)
    assert labels[0, 0].tolist()[:4] == [7, 8, EOS, -1] and labels[3].eq(-1).all() and mask[3].sum() == 0      # the cases are what they say
    # no end token: the labels are the first `length` tokens
    _, labels, _ = beam_inputs_labels(tokens, lengths, BOS, -1, PAD, Wd)
    for i, (a, b, l) in enumerate(rows):
        assert labels[i, 0].tolist() == python_inputs_labels(a, l, BOS, -1, PAD, Wd)[1]
    with pytest.raises(ValueError):
        beam_inputs_labels(tokens, lengths, BOS, EOS, PAD, T - 1)


def test_normalized_arithmetic():
    lp = torch.tensor([[-6.0, -2.0, 0.0], [-9.0, -1.5, -4.0]])
    nt = torch.tensor([[3, 4, 0], [9, 1, 2]], dtype=torch.int32)
    z = torch.zeros(2, 3, 5)
    s = CaptionScores(z, z.to(torch.int32), z, lp, nt, torch.zeros_like(nt))
    assert torch.equal(s.normalized(), torch.tensor([[-2.0, -0.5, 0.0], [-1.0, -1.5, -2.0]]))          # a caption of no tokens: / 1
    assert torch.equal(s.normalized(0.0), lp)
    want = lp / torch.tensor([[3.0, 4.0, 1.0], [9.0, 1.0, 2.0]]) ** 0.5
    assert torch.allclose(s.normalized(0.5), want, rtol=1e-6, atol=0)
    assert int(s.normalized().argmax(dim=1)[1]) == 0                                                    # re-ranking: -1.0 beats -1.5


def test_caption_loss_result_from_counts():
    r = CaptionLossResult([-6.0, -2.0, 0.0, -4.0], [3, 4, 0, 1], [1, 2, 0, 1], "ses")
    assert r.loss == 12.0 / 8.0 and float(r) == r.loss
    assert r.perplexity == math.exp(1.5) and r.token_accuracy == 4.0 / 8.0 and r.session == "ses"
    assert r.seq_logprob.dtype == np.float32 and r.seq_tokens.dtype == np.int32 and r.seq_correct.dtype == np.int32
    assert r.seq_tokens.tolist() == [3, 4, 0, 1]
    empty = CaptionLossResult([], [], [], None)
    assert math.isnan(empty.loss) and math.isnan(float(empty)) and math.isnan(empty.perplexity) and math.isnan(empty.token_accuracy)
    assert empty.seq_logprob.shape == (0,) and empty.session is None
    none_counts = CaptionLossResult([0.0, 0.0], [0, 0], [0, 0], None)                                  # nothing to average over: NaN, like torch
    assert math.isnan(none_counts.loss)


def test_vocab_score_refuses_host_tensors():
    """There is no fallback: a CPU tensor is a RuntimeError before anything reaches the library (tests/test_host_cpu.py)."""
    x, table, bias = torch.zeros(4, 64), torch.zeros(130, 64), torch.zeros(130)
    labels = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="HIP device"):
        d, _ = ops.vocab_score_desc(x, table, bias, labels, 130, 2)
        ops.vocab_score(d)


def _header_struct(name):
    header = open(os.path.join(ROOT, "include", "univl_hip.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(const\s+)?(\w+)\s*(\*?)\s*(.*)", decl)
        ctype, ptr, names = m.group(2), m.group(3), m.group(4)
        for nm in names.split(","):
            fields.append((nm.strip(), "ptr" if ptr else ctype))
    return fields


def test_vocab_score_struct_matches_the_header():
    """Field for field against include/univl_hip.h (names, order, kinds), and sizeof against the library (struct #10)."""
    kinds = {"int32_t": _lib.i32, "int64_t": _lib.i64, "float": _lib.f32, "ptr": _lib.vp}
    want = [(n, kinds[k]) for n, k in _header_struct("UnivlVocabScore")]
    assert [(n, t) for n, t in _lib.VocabScore._fields_] == want
    L = _lib.lib()                                          # verifies every mirror's sizeof at load time
    assert _lib._STRUCTS[10] is _lib.VocabScore and L.univl_struct_size(10) == C.sizeof(_lib.VocabScore)
    assert L.univl_struct_size(11) == -1
    assert hasattr(L, "univl_vocab_score") and "univl_vocab_score" in _lib.EXPORTED
    # the same parser reads the K16 descriptor it was modelled on correctly
    assert [n for n, _ in _header_struct("UnivlVocabCE")] == [n for n, _ in _lib.VocabCE._fields_]
