"""Host side of the decoding constraints (no GPU): DecodeConstraints validates before any device work, univl_decode_constrain is
declared, exported and bound, the descriptor mirrors the C struct and its size is stated by univl_decode_constrain_sizeof while both
numbered size tables stay as they are, and the numpy restatement of the contract (tests/constrain_ref.py, the reference of
tests/test_constrain_gpu.py) gives hand-worked answers."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from univl_amd import _lib, ops
from univl_amd.constrain import DecodeConstraints

from constrain_ref import advance_prefix, banned_by_ngram, constrain_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "univl_hip.h")).read()
needs_lib = pytest.mark.skipif(not _lib.available(), reason="libunivl_hip.so is not built")
NINF = -np.inf


# ------------------------------------------------------------------------------------------------ DecodeConstraints
def test_constraints_validation():
    c = DecodeConstraints()
    assert (c.no_repeat_ngram, c.min_len, c.suppress) == (0, 0, ()) and c.params_dev is None
    for bad in (dict(no_repeat_ngram=-1), dict(no_repeat_ngram=5), dict(no_repeat_ngram=1.5), dict(min_len=-1), dict(suppress=[3, -1])):
        with pytest.raises(ValueError):
            DecodeConstraints(**bad)
    for n in range(5):
        assert DecodeConstraints(no_repeat_ngram=n).no_repeat_ngram == n
    # against a session: min_len < Tmax, ids inside the vocabulary -- raised before anything is allocated
    with pytest.raises(ValueError, match="max_len"):
        DecodeConstraints(min_len=12).bind(100, 12, "cpu")
    with pytest.raises(ValueError, match="vocabulary"):
        DecodeConstraints(suppress=[5, 100]).bind(100, 12, "cpu")
    b = DecodeConstraints(3, 11, [99, 0, 0]).bind(100, 12, "cpu")
    assert b.params_dev.tolist() == [3, 11] and b.params_dev.dtype == torch.int32
    assert b.suppress_dev.tolist() == [99, 0, 0] and b.suppress_dev.dtype == torch.int32          # duplicates are kept
    assert DecodeConstraints(2, 0, ()).bind(100, 12, "cpu").suppress_dev is None
    # the end token in the suppress list is legal with and without a min_len (nothing here knows the end token)
    DecodeConstraints(0, 4, [7]).bind(100, 12, "cpu")
    DecodeConstraints(0, 0, [7]).bind(100, 12, "cpu")


def test_constraints_set_rewrites_the_words_in_place():
    user = DecodeConstraints(2, 4, [1])
    with pytest.raises(RuntimeError, match="not bound"):
        user.set(ngram=1)
    b = user.bind(50, 8, "cpu")
    ptr = b.params_dev.data_ptr()
    b.set(ngram=0, min_len=0)
    assert b.params_dev.tolist() == [0, 0] and b.params_dev.data_ptr() == ptr and (b.no_repeat_ngram, b.min_len) == (0, 0)
    b.set(min_len=7)
    assert b.params_dev.tolist() == [0, 7]
    for bad in (dict(ngram=5), dict(min_len=8), dict(min_len=-1)):
        with pytest.raises(ValueError):
            b.set(**bad)
    assert b.params_dev.tolist() == [0, 7]                     # a refused call changes nothing
    assert (user.no_repeat_ngram, user.min_len) == (2, 4)      # the caller's object is configuration, the session's copy is state


def test_sessions_take_the_keyword():
    import inspect
    from univl_amd.decode import CaptionBeamSearch
    from univl_amd.eval import eval_caption
    from univl_amd.sample import CaptionSampler
    for f in (CaptionBeamSearch.__init__, CaptionSampler.__init__, eval_caption):
        assert inspect.signature(f).parameters["constraints"].default is None
    assert callable(CaptionBeamSearch.set_constraints)


def test_eval_caption_refuses_constraints_beside_a_session():
    from univl_amd.eval import eval_caption
    with pytest.raises(ValueError, match="session"):
        eval_caption(None, [], None, session=object(), constraints=DecodeConstraints(1))


# ------------------------------------------------------------------------------------------------ binding
@needs_lib
def test_decode_constrain_is_declared_exported_and_bound():
    L = _lib.lib()
    declared = set(re.findall(r"\b(univl_[a-z0-9_]+)\s*\(", HEADER))
    for name in ("univl_decode_constrain", "univl_decode_constrain_sizeof"):
        assert name in declared and name in _lib.EXPORTED and hasattr(L, name)
    assert declared == set(_lib.EXPORTED)
    m = re.search(r"int\s+univl_decode_constrain\s*\(([^;]*)\)\s*;", HEADER)
    params = [p.strip() for p in m.group(1).split(",")]
    fn = L.univl_decode_constrain
    assert fn.restype is C.c_int32 and len(fn.argtypes) == len(params) == 2
    assert callable(ops.decode_constrain_desc) and callable(ops.decode_constrain)


@needs_lib
def test_descriptor_mirrors_the_header():
    """Field for field (names, order, kinds); sizeof through univl_decode_constrain_sizeof; the numbered tables keep their lengths."""
    body = re.search(r"typedef struct UnivlDecodeConstrain \{(.*?)\} UnivlDecodeConstrain;", HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    kinds = {"int32_t": _lib.i32, "int64_t": _lib.i64, "float": _lib.f32, "ptr": _lib.vp}
    want = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(const\s+)?(\w+)\s*(\*?)\s*(.*)", decl)
        for nm in m.group(4).split(","):
            want.append((nm.strip(), kinds["ptr" if m.group(3) else m.group(2)]))
    assert [(n, t) for n, t in _lib.DecodeConstrain._fields_] == want
    L = _lib.lib()
    assert L.univl_decode_constrain_sizeof() == C.sizeof(_lib.DecodeConstrain)
    assert _lib.DecodeConstrain not in _lib._STRUCTS and len(_lib._STRUCTS) == 12
    assert L.univl_abi_sizeof(12) == -1 and L.univl_struct_size(11) == -1
    assert int(re.search(r"#define UNIVL_NGRAM_BLOCK_MAX (\d+)", HEADER).group(1)) == _lib.NGRAM_BLOCK_MAX == 4


@needs_lib
def test_no_cpu_fallback_and_null_descriptor():
    x = torch.zeros(2, 8)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.decode_constrain(x, 8, 0, Tmax=4)
    assert _lib.lib().univl_decode_constrain(None, None) == -1            # UNIVL_EINVAL before any device call


# ------------------------------------------------------------------------------------------------ the reference, by hand
A, B, Cc, D = 3, 5, 6, 2        # four distinct tokens of a vocabulary of 7 (column 7 of ld = 8 is padding)


def _banned(prefix, t, **kw):
    """Columns that constrain_ref turns into -inf on a one-row input of ones."""
    args = dict(done=None, ngram=0, min_len=0, eos=-1, suppress=())
    args.update(kw)
    x = np.ones((1, 8), dtype=np.float32)
    p = np.array([list(prefix) + [0] * (8 - len(prefix))], dtype=np.int32)
    y = constrain_ref(x, 7, p, t, **args)
    assert y[0, 7] == 1.0                                                 # the padding column is never written
    assert bool(((y == 1.0) | (y == NINF)).all())
    return sorted(np.nonzero(y[0] == NINF)[0].tolist())


def test_ref_ngram_cases_worked_by_hand():
    # a b a b, n = 2, t = 4: the last 1-gram is b; b stands at j = 1 and is followed by a; (j = 3 is the tail itself) -> {a}
    assert _banned([A, B, A, B], 4, ngram=2) == [A]
    # the same prefix one position earlier, a b a, tail a at j = 0 followed by b -> {b}
    assert _banned([A, B, A, B], 3, ngram=2) == sorted([B])
    # a b c a b, n = 3, t = 5: the tail is (a, b), found at j = 0, followed by c -> {c}
    assert _banned([A, B, Cc, A, B], 5, ngram=3) == [Cc]
    # ... and with n = 2 the tail b at j = 1 is followed by c as well; with n = 4 the tail (c, a, b) occurs nowhere earlier
    assert _banned([A, B, Cc, A, B], 5, ngram=2) == [Cc]
    assert _banned([A, B, Cc, A, B], 5, ngram=4) == []
    # a a a, n = 2, t = 3: tail a at j = 0 and j = 1, both followed by a -> {a}; n = 3: tail (a, a) at j = 0 followed by a -> {a}
    assert _banned([A, A, A], 3, ngram=2) == [A] and _banned([A, A, A], 3, ngram=3) == [A]
    # n = 1: every prefix token, whatever the order
    assert _banned([A, B, Cc, A, B], 5, ngram=1) == sorted([A, B, Cc])
    assert _banned([A, B, Cc, A, B], 2, ngram=1) == sorted([A, B])
    assert _banned([A, B], 0, ngram=1) == []
    # t = n - 2 and t = n - 1 ban nothing (no complete n-gram can be in the prefix yet); t = n is the first that can
    for n in (2, 3, 4):
        assert _banned([A] * 6, n - 2, ngram=n) == [] and _banned([A] * 6, n - 1, ngram=n) == []
        assert _banned([A] * 6, n, ngram=n) == [A]
    assert banned_by_ngram([A, B, A, B], 4, 0) == set()
    # positions at and past t are not part of the prefix
    assert _banned([A, B, D, B, A], 2, ngram=2) == []


def test_ref_min_len_suppress_done_and_padding():
    # min_len: eos is banned at t = min_len - 1 and free at t = min_len; a negative eos bans nothing
    assert _banned([A, B, A], 2, min_len=3, eos=D) == [D]
    assert _banned([A, B, A], 3, min_len=3, eos=D) == []
    assert _banned([A, B, A], 0, min_len=3, eos=-1) == []
    assert _banned([], 0, min_len=1, eos=0) == [0]
    # suppress: duplicates are fine, -1 and V (= 7, the padding column!) and anything larger are skipped
    assert _banned([], 0, suppress=[4, 4, 1]) == [1, 4]
    assert _banned([], 0, suppress=[-1, 7, 8, 6]) == [6]
    assert _banned([], 0, min_len=2, eos=7) == []
    # everything at once is the union
    assert _banned([A, B, A, B], 4, ngram=2, min_len=5, eos=D, suppress=[0]) == sorted([A, D, 0])
    # done rows are untouched (done is per instance of done_stride rows); -inf already present stays; other values keep their bits
    x = np.arange(32, dtype=np.float32).reshape(4, 8)
    x[1, 2] = NINF
    p = np.full((4, 8), A, dtype=np.int32)
    y = constrain_ref(x, 7, p, 3, np.array([0, 1], dtype=np.uint8), 1, 0, -1, [0], done_stride=2)
    assert np.array_equal(y[2:], x[2:]) and y[1, 2] == NINF
    for r in (0, 1):
        assert y[r, A] == NINF and y[r, 0] == NINF
        keep = [c for c in range(8) if c not in (A, 0)]
        assert np.array_equal(y[r, keep], x[r, keep])
    assert x[0, A] == 3.0                                                 # the input is not edited


def test_ref_advance_prefix():
    pin = np.array([[1, 2, 3, 9], [4, 5, 6, 9], [7, 8, 9, 9]], dtype=np.int32)
    before = np.full((3, 4), -5, dtype=np.int32)
    out = advance_prefix(pin, np.array([1, 1, 0]), np.array([40, 41, 42]), 3, before)
    assert out.tolist() == [[4, 5, 40, -5], [4, 5, 41, -5], [1, 2, 42, -5]]
    assert advance_prefix(pin, None, np.array([40, 41, 42]), 1, before).tolist() == [[40, -5, -5, -5], [41, -5, -5, -5], [42, -5, -5, -5]]
    assert advance_prefix(pin, None, np.array([40, 41, 42]), 0, before).tolist() == before.tolist()
