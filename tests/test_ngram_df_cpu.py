"""Host side of the device-built document-frequency tables (no GPU): univl_ngram_df and its helpers are declared, exported and bound,
the descriptor mirrors the C struct and its size is stated by univl_ngram_df_sizeof while both numbered size tables stay as they
were, the header's workspace formula is what univl_ngram_df_ws_bytes evaluates, and the arguments a host can judge are refused before
a device is asked for."""
import ctypes as C
import os
import re

import pytest
import torch

from univl_amd import _lib, ops, rl
from univl_amd import caption_metrics as M
from univl_amd.sample import SampleResult

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "univl_hip.h")).read()


def test_ngram_df_symbols_are_declared_exported_and_bound():
    L = _lib.lib()
    declared = set(re.findall(r"\b(univl_[a-z0-9_]+)\s*\(", HEADER))
    for name in ("univl_ngram_df", "univl_ngram_df_sizeof", "univl_ngram_df_ws_bytes", "univl_ngram_df_tile"):
        assert name in declared and name in _lib.EXPORTED and hasattr(L, name)
    fn = L.univl_ngram_df
    assert fn.restype is C.c_int32 and list(fn.argtypes) == [C.c_void_p, C.c_void_p]
    fn = L.univl_ngram_df_ws_bytes
    assert fn.restype is C.c_int64 and list(fn.argtypes) == [C.c_int32, C.c_int32]
    assert callable(ops.ngram_df) and callable(M.DocumentFrequency.from_ids) and callable(M.DocumentFrequency.from_lists)


def test_ngram_df_struct_mirrors_the_header():
    body = re.search(r"typedef struct UnivlNgramDf \{(.*?)\} UnivlNgramDf;", HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    kinds = {"int32_t": _lib.i32, "int64_t": _lib.i64, "uint64_t": _lib.u64, "void": _lib.vp, "ptr": _lib.vp}
    want = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(const\s+)?(\w+)\s*(\*?)\s*(.*)", decl)
        for nm in m.group(4).split(","):
            want.append((nm.strip(), kinds["ptr" if m.group(3) else m.group(2)]))
    assert [(n, t) for n, t in _lib.NgramDf._fields_] == want
    L = _lib.lib()
    assert L.univl_ngram_df_sizeof() == C.sizeof(_lib.NgramDf)
    assert int(re.search(r"#define UNIVL_NGRAM_DF_OVERFLOW (\d+)", HEADER).group(1)) == _lib.NGRAM_DF_OVERFLOW == 16
    assert int(re.search(r"#define UNIVL_NGRAM_DF_TILE (\d+)", HEADER).group(1)) == _lib.NGRAM_DF_TILE == L.univl_ngram_df_tile()
    bits = (_lib.OVERLAP_BAD_LEN, _lib.OVERLAP_BAD_SYM, _lib.OVERLAP_BAD_ROW, _lib.OVERLAP_BAD_REFS, _lib.NGRAM_DF_OVERFLOW)
    assert sorted(bits) == [1, 2, 4, 8, 16]                                    # one status word carries all five


def test_both_size_tables_are_unchanged():
    L = _lib.lib()
    assert _lib.NgramDf not in _lib._STRUCTS and len(_lib._STRUCTS) == 12
    assert L.univl_abi_sizeof(12) == -1 and L.univl_abi_sizeof(13) == -1 and L.univl_struct_size(11) == -1
    for k in range(12):
        assert L.univl_abi_sizeof(k) == C.sizeof(_lib._STRUCTS[k])
    for k in range(11):
        assert L.univl_struct_size(k) == C.sizeof(_lib._STRUCTS[k])


def test_workspace_formula_of_the_header():
    """WORKSPACE: 64 + 16 N + 1024 ceil(N / UNIVL_NGRAM_DF_TILE) bytes with N = 4 T n_refs."""
    assert "64 + 16 N + 1024 ceil(N / UNIVL_NGRAM_DF_TILE) bytes with N = 4 T n_refs" in HEADER
    L = _lib.lib()
    tile = _lib.NGRAM_DF_TILE
    for n_refs, T in ((1, 1), (1, 128), (8, 128), (9, 128), (3, 7), (60000, 48), (4194303, 128)):
        N = 4 * T * n_refs
        assert L.univl_ngram_df_ws_bytes(n_refs, T) == 64 + 16 * N + 1024 * ((N + tile - 1) // tile), (n_refs, T)
    for n_refs, T in ((0, 8), (-1, 8), (4, 0), (4, 129), (4194304, 128)):       # the last: N = 2^31
        assert L.univl_ngram_df_ws_bytes(n_refs, T) == -1, (n_refs, T)


def _fake_samples(n=2, ns=3, T=5):
    tok = torch.zeros(n, ns, T, dtype=torch.int32)
    z = torch.zeros(n, ns, T)
    return SampleResult(tok, z, z, z[..., 0], z[..., 0], torch.full((n, ns), T, dtype=torch.int32))


def _host_table(n_docs):
    return M.DocumentFrequency(torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int32), [0] * 5, n_docs)


def test_cider_rewards_refuse_bad_tables_before_any_device_work():
    res = _fake_samples()
    ref, rlen = torch.zeros(2, 2, 6, dtype=torch.int64), torch.full((2, 2), 6)
    with pytest.raises(ValueError, match="needs df"):
        rl.caption_rewards(res, ref, rlen, 102, 0, metric="cider")
    with pytest.raises(ValueError, match="needs df"):
        rl.caption_rewards(res, ref, rlen, 102, 0, metric="cider", df=(None, None, [0] * 5, 3))       # a bare tuple is not a table
    with pytest.raises(ValueError, match="0 documents"):
        rl.caption_rewards(res, ref, rlen, 102, 0, metric="cider", df=_host_table(0))
    with pytest.raises(ValueError, match="metric"):
        rl.caption_rewards(res, ref, rlen, 102, 0, metric="meteor", df=_host_table(3))
    with pytest.raises(RuntimeError, match="HIP device"):                      # well-formed: the device is asked for, and is not there
        rl.caption_rewards(res, ref, rlen, 102, 0, metric="cider", df=_host_table(3))
    with pytest.raises(RuntimeError, match="HIP device"):                      # the other metrics ignore df
        rl.caption_rewards(res, ref, rlen, 102, 0, metric="rouge_l", df="ignored")
    t = _host_table(4)
    assert t.tables == (t.keys, t.cnt, [0, 0, 0, 0, 0], 4) and t.device == torch.device("cpu")


def test_caption_metrics_and_document_frequency_refuse_bad_arguments():
    with pytest.raises(ValueError, match="df="):
        M.CaptionMetrics(df="nonsense")
    assert M.CaptionMetrics().df == "host" and M.CaptionMetrics(df="device").df == "device"
    ids, lens = torch.zeros(2, 3, 5, dtype=torch.int64), torch.full((2, 3), 5)
    with pytest.raises(ValueError, match="ref_ids of shape"):
        M.DocumentFrequency.from_ids(ids[0], lens)
    with pytest.raises(ValueError, match="ref_ids of shape"):
        M.DocumentFrequency.from_ids(ids, lens[:, :2])
    with pytest.raises(ValueError, match="integer"):
        M.DocumentFrequency.from_ids(ids.float(), lens)
    with pytest.raises(ValueError, match="at most 128"):
        M.DocumentFrequency.from_ids(torch.zeros(2, 3, 129, dtype=torch.int64), lens)
    with pytest.raises(ValueError):
        M.DocumentFrequency.from_lists([])
    with pytest.raises(ValueError):
        M.DocumentFrequency.from_lists([[], []])
    with pytest.raises(ValueError):
        M.DocumentFrequency.from_lists([[[65535]]])
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            M.DocumentFrequency.from_ids(ids, lens)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            M.DocumentFrequency.from_lists([[[1, 2]], []])
