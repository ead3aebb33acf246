"""Decoding constraints: what a caller may tell CaptionBeamSearch / CaptionSampler about the sequence they write.

  no_repeat_ngram  n in 0 .. 4 (0: off): no n-gram occurs twice in a caption -- a token that would complete an n-gram the row
                   already holds is banned at that position;
  min_len          the end token is banned at positions 0 .. min_len-1, so a caption has at least min_len tokens before it;
  suppress         ids that are never emitted ([UNK], [CLS], [MASK], [PAD], the [unusedNN] rows of the BERT table, ...).

A ban is a -inf written into the position's score row by one launch (include/univl_hip.h: univl_decode_constrain; csrc/constrain.hip)
between the vocabulary classifier and the selection kernel, so a constrained session still decodes with one graph replay per position
and no host read.  A DecodeConstraints object is plain configuration; a session BINDS it (a copy that owns the device suppress list and
the device words {ngram, min_len}).  The order and the minimum length are device words: session.set_constraints(ngram=, min_len=)
rewrites them and the captured graphs serve the new values.  The suppress list's LENGTH is baked into the captures, so another list is
another session.

The caller's condition: every live row keeps at least n_bm (beam search) or top_k (sampling) finite columns.  With a vocabulary of
30522 and lists of a few hundred ids that is not a concern; a suppress list close to the whole vocabulary would be.
"""
import torch

from ._lib import NGRAM_BLOCK_MAX


class DecodeConstraints:
    def __init__(self, no_repeat_ngram=0, min_len=0, suppress=()):
        self.no_repeat_ngram, self.min_len = self._check_words(no_repeat_ngram, min_len)
        self.suppress = tuple(int(v) for v in suppress)
        if any(v < 0 for v in self.suppress):
            raise ValueError("DecodeConstraints: suppress id %d is negative" % min(self.suppress))
        self.params_dev = self.suppress_dev = None       # device state: bound copies only
        self.V = self.Tmax = None

    @staticmethod
    def _check_words(ngram, min_len, Tmax=None):
        if isinstance(ngram, bool) or int(ngram) != ngram or not 0 <= int(ngram) <= NGRAM_BLOCK_MAX:
            raise ValueError("DecodeConstraints: no_repeat_ngram=%r, expected an integer in 0 .. %d" % (ngram, NGRAM_BLOCK_MAX))
        if isinstance(min_len, bool) or int(min_len) != min_len or int(min_len) < 0:
            raise ValueError("DecodeConstraints: min_len=%r, expected an integer >= 0" % (min_len,))
        if Tmax is not None and int(min_len) >= Tmax:
            raise ValueError("DecodeConstraints: min_len=%d, expected less than the session's max_len=%d" % (min_len, Tmax))
        return int(ngram), int(min_len)

    def bind(self, V, Tmax, device):
        """The copy a session of vocabulary V and Tmax positions keeps: validated against both BEFORE any device work, then the suppress
        list and the words {ngram, min_len} are put on `device`.  The end token may be in the suppress list, with or without a min_len."""
        self._check_words(self.no_repeat_ngram, self.min_len, Tmax)
        bad = [v for v in self.suppress if v >= V]
        if bad:
            raise ValueError("DecodeConstraints: suppress id %d is outside the vocabulary of %d" % (bad[0], V))
        b = DecodeConstraints(self.no_repeat_ngram, self.min_len, self.suppress)
        b.V, b.Tmax = int(V), int(Tmax)
        b.params_dev = torch.tensor([b.no_repeat_ngram, b.min_len], dtype=torch.int32, device=device)
        b.suppress_dev = torch.tensor(b.suppress, dtype=torch.int32, device=device) if b.suppress else None
        return b

    def set(self, ngram=None, min_len=None):
        """Rewrite the device words of a bound copy (None: keep).  No capture is touched: the launches read the words."""
        if self.params_dev is None:
            raise RuntimeError("DecodeConstraints.set: not bound to a session")
        n, m = self._check_words(self.no_repeat_ngram if ngram is None else ngram, self.min_len if min_len is None else min_len, self.Tmax)
        self.no_repeat_ngram, self.min_len = n, m
        self.params_dev[0:1].fill_(n)
        self.params_dev[1:2].fill_(m)

    def __repr__(self):
        return "DecodeConstraints(no_repeat_ngram=%d, min_len=%d, suppress=<%d ids>)" % (self.no_repeat_ngram, self.min_len, len(self.suppress))
