"""Host side of caption evaluation (univl_amd.eval.eval_caption): the id-to-text rule against a literal restatement of the
reference's lines, the stage-one early return, and the C ABI inventory with univl_beam_captions in it.  No GPU."""
import ctypes as C
import os
import random
import re

import pytest

from univl_amd import _lib
from univl_amd.eval import eval_caption, ids_to_caption

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class SynthTokenizer:
    """The part of the reference's BertTokenizer that caption evaluation uses, over a vocabulary made up here: BERT's special ids,
    plain words and "##" pieces.  `special` overrides ids of specials (the GPU tests put "[SEP]" on a token the toy decoder emits)."""

    def __init__(self, vocab_size=64, special=None):
        ids = {"[PAD]": 0, "[UNK]": 100, "[CLS]": 101, "[SEP]": 102, "[MASK]": 103}
        ids.update(special or {})
        self.ids_to_tokens = {}
        for i in range(vocab_size):
            self.ids_to_tokens[i] = ("##p%d" % i) if i % 5 == 3 else ("w%d" % i)
        for tok, i in ids.items():
            if i < vocab_size:
                self.ids_to_tokens[i] = tok
        self.vocab = {tok: i for i, tok in self.ids_to_tokens.items()}
        self.vocab.update(ids)

    def convert_ids_to_tokens(self, ids):
        return [self.ids_to_tokens[int(i)] for i in ids]


def reference_text(tokenizer, re_list):
    """main_task_caption.py:554-562, line for line."""
    decode_text_list = tokenizer.convert_ids_to_tokens(re_list)
    if "[SEP]" in decode_text_list:
        SEP_index = decode_text_list.index("[SEP]")
        decode_text_list = decode_text_list[:SEP_index]
    if "[PAD]" in decode_text_list:
        PAD_index = decode_text_list.index("[PAD]")
        decode_text_list = decode_text_list[:PAD_index]
    decode_text = ' '.join(decode_text_list)
    decode_text = decode_text.replace(" ##", "").strip("##").strip()
    return decode_text


def _named_tokenizer():
    """A small vocabulary with readable entries: [PAD] 0, [CLS] 1, [SEP] 2, words, '##' pieces and a bare '#'."""
    words = ["[PAD]", "[CLS]", "[SEP]", "a", "man", "is", "play", "##ing", "guitar", "##s", "the", "#", "c", "##"]
    tk = SynthTokenizer(0)
    tk.ids_to_tokens = dict(enumerate(words))
    tk.vocab = {w: i for i, w in enumerate(words)}
    return tk


CASES = [
    # (tokens, expected text)
    (["a", "man", "[SEP]", "is", "[PAD]", "guitar"], "a man"),                 # [SEP] before [PAD]
    (["a", "man", "[PAD]", "is", "[SEP]", "guitar"], "a man"),                 # [PAD] before [SEP]
    (["a", "[PAD]", "[PAD]", "[SEP]"], "a"),
    (["a", "man", "is", "play", "##ing", "guitar", "##s"], "a man is playing guitars"),      # neither present
    (["##ing", "a", "man"], "ing a man"),                                       # a leading piece: strip("##") strips it
    (["a", "man", "##s"], "a mans"),                                            # a trailing piece is glued by the replace
    (["##s"], "s"),
    (["c", "#"], "c"),                                                          # strip("##") strips CHARACTERS: a trailing '#' goes too
    (["#", "#", "c", "##", "[SEP]", "a"], "# c"),                              # ... but only up to the first other character
    (["##"], ""),
    ([], ""),                                                                   # an empty hypothesis
    (["[SEP]", "a"], ""),
    (["[PAD]"], ""),
]


@pytest.mark.parametrize("tokens,expected", CASES, ids=[" ".join(c[0]) or "empty" for c in CASES])
def test_ids_to_caption_equals_the_reference_lines(tokens, expected):
    tk = _named_tokenizer()
    ids = [tk.vocab[t] for t in tokens]
    assert reference_text(tk, ids) == expected              # the case is what its comment says
    assert ids_to_caption(tk, ids) == expected


def test_ids_to_caption_equals_the_reference_lines_on_random_ids():
    tk = _named_tokenizer()
    rng = random.Random(7)
    n = len(tk.ids_to_tokens)
    for _ in range(2000):
        ids = [rng.randrange(n) for _ in range(rng.randrange(0, 12))]
        assert ids_to_caption(tk, ids) == reference_text(tk, ids), ids
    tk = SynthTokenizer(200)
    for _ in range(500):
        ids = [rng.choice([0, 102, rng.randrange(200)]) for _ in range(rng.randrange(0, 24))]
        assert ids_to_caption(tk, ids) == reference_text(tk, ids), ids


def test_eval_caption_returns_early_for_a_stage_one_model():
    """main_task_caption.py:495.  Neither the loader, the tokenizer nor any other attribute of the model may be touched."""

    class StageOne:
        _stage_one = True

        def __getattr__(self, name):
            raise AssertionError("eval_caption touched model.%s of a stage-one model" % name)

    class Untouchable:
        def __iter__(self):
            raise AssertionError("eval_caption iterated the loader of a stage-one model")

        def __getattr__(self, name):
            raise AssertionError("eval_caption touched .%s" % name)

    res = eval_caption(StageOne(), Untouchable(), Untouchable(), device="cpu")
    assert float(res) == 0.0 and res.hyps == [] and res.refs == [] and res.metrics is None and res.session is None


def test_beam_captions_is_declared_exported_and_bound():
    """The header declares univl_beam_captions, the library exports it, the inventory lists it, and the ctypes binding has one
    argument type per declared parameter (the pattern of tests/test_host_cpu.py::test_library_exports_every_declared_symbol)."""
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "univl_hip.h")).read()
    declared = set(re.findall(r"\b(univl_[a-z0-9_]+)\s*\(", header))
    assert "univl_beam_captions" in declared
    assert "univl_beam_captions" in _lib.EXPORTED and declared == set(_lib.EXPORTED)
    assert hasattr(L, "univl_beam_captions")
    m = re.search(r"int\s+univl_beam_captions\s*\(([^;]*)\)\s*;", header)
    assert m, "declaration not found"
    params = [p.strip() for p in m.group(1).split(",")]
    fn = L.univl_beam_captions
    assert fn.restype is C.c_int32 and len(fn.argtypes) == len(params) == 11
    for p, t in zip(params, fn.argtypes):
        assert (t is C.c_void_p) == ("*" in p or "hipStream_t" in p), (p, t)
        assert (t is C.c_int32) == p.startswith("int32_t "), (p, t)
    # the two earlier beam entry points keep their signatures
    assert len(L.univl_beam_backtrack.argtypes) == 11 and len(L.univl_beam_step.argtypes) == 2


def test_eval_caption_host_side_with_stub_model_and_session(tmp_path):
    """The loop's host side without a GPU: a stub model and a stub session that hands back fixed hypotheses.  Batches of 3 + 3 + 2 on
    a 3-slot session: n_active only for the short one, texts / files / metric call as the reference's lines give them."""
    import torch
    tk = SynthTokenizer(64, special={"[CLS]": 1, "[SEP]": 2})
    W, T = 4, 6
    calls = []

    class Model:
        _stage_one, training = False, True

        def eval(self):
            self.training = False

        def train(self, mode=True):
            self.training = mode

        def get_sequence_visual_output(self, input_ids, segment_ids, input_mask, video, video_mask):
            n = input_ids.shape[0]
            return torch.zeros(n, W, 8), torch.zeros(n, W, 8)

    class Result:
        def __init__(self, n, n_best, first):
            self.n, self.k = n, n_best
            tok = torch.full((n, n_best, T), -1, dtype=torch.int32)
            for i in range(n):
                for k in range(n_best):
                    tok[i, k, :4] = torch.tensor([10 + first + i, 13, 2 if k == 0 else 20, 11])      # "[SEP]" at 2 in the best one
            self.tokens = tok
            self.scores = -torch.arange(n_best, dtype=torch.float32).expand(n, n_best).contiguous()
            self.lengths = torch.full((n,), 4, dtype=torch.int32)

        def captions(self, eos, pad):
            cap, ln = self.tokens.clone(), torch.full((self.n, self.k), 4, dtype=torch.int32)
            cap[:, 0, 2:] = -1
            ln[:, 0] = 2
            return cap, ln

    class Session:
        n_inst = 3

        def __init__(self):
            self.seen = 0

        def decode(self, so, vo, am, vm, bos, eos, max_len=None, n_best=1, n_active=None):
            assert (bos, eos) == (1, 2) and so.shape[0] == (n_active or self.n_inst)
            calls.append(n_active)
            r = Result(so.shape[0], n_best, self.seen)
            self.seen += so.shape[0]
            return r

    def batch(n, first):
        z = torch.zeros(n, 1, W, dtype=torch.int64)
        truth = torch.tensor([[30 + first + i, 33, 0, 31] for i in range(n)]).view(n, 1, W)
        return (z, z, z, torch.zeros(n, 1, W, 8), z) + (z,) * 6 + (truth,)

    class Metric:
        def compute_metrics(self, ref_list, hyp_list):
            return {"Bleu_4": 0.5, "refs": ref_list, "hyps": hyp_list}

    model, session = Model(), Session()
    res = eval_caption(model, [batch(3, 0), batch(3, 3), batch(2, 6)], tk, n_best=2, session=session, output_dir=str(tmp_path),
                       nlg_eval=Metric(), device="cpu")
    assert calls == [None, None, 2] and model.training and res.session is session
    want_h = [reference_text(tk, [10 + i, 13, 2, 11]) for i in range(8)]
    want_r = [reference_text(tk, [30 + i, 33, 0, 31]) for i in range(8)]
    assert want_h[0] == "w10p13" and want_r[0] == "w30p33"
    assert res.hyps == want_h and res.refs == want_r
    assert (tmp_path / "hyp.txt").read_text(encoding="utf-8") == "".join(t + "\n" for t in want_h)
    assert (tmp_path / "ref.txt").read_text(encoding="utf-8") == "".join(t + "\n" for t in want_r)
    assert res.metrics["refs"] == [want_r] and res.metrics["hyps"] == want_h and float(res) == 0.5
    assert res.scores.shape == (8, 2) and res.lengths.tolist() == [4] * 8
    assert res.hyp_ids[7] == [[17, 13], [17, 13, 20, 11]]
    with pytest.raises(ValueError, match="4.*3"):
        eval_caption(model, [batch(4, 0)], tk, session=session, device="cpu")
    assert model.training
