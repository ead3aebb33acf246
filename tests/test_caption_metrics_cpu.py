"""Host side of the caption metrics (no GPU): univl_caption_overlap / univl_consensus_pick are declared, exported and bound, the
descriptor mirrors the C struct and its size is stated by univl_caption_overlap_sizeof while both numbered size tables stay as they
were, the DICTIONARY RESTATEMENT of the contract (plain Python, below; tests/test_caption_metrics_gpu.py compares the kernel with it)
gives hand-computed answers, the host's document-frequency tables equal the restatement's, and the launcher shim's nlgeval stub
delegates to CaptionMetrics."""
import ctypes as C
import math
import os
import re
import sys
from collections import Counter

import numpy as np
import pytest
import torch

from univl_amd import _lib, ops
from univl_amd import caption_metrics as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "univl_hip.h")).read()
KEYS = ("Bleu_1", "Bleu_2", "Bleu_3", "Bleu_4", "METEOR", "ROUGE_L", "CIDEr")


# ------------------------------------------------------------------------------------------------ the restatement
def ngrams(row, n):
    return [tuple(row[i:i + n]) for i in range(len(row) - n + 1)]


def lcs_len(a, b):
    prev = [0] * (len(b) + 1)
    for x in a:
        cur = [0]
        for j, y in enumerate(b):
            cur.append(prev[j] + 1 if x == y else max(prev[j + 1], cur[j]))
        prev = cur
    return prev[len(b)]


def doc_freq(ref_lists):
    """df[n-1][g]: the number of items whose reference SET holds n-gram g."""
    df = [Counter() for _ in range(4)]
    for refs in ref_lists:
        for n in range(1, 5):
            df[n - 1].update(set(g for r in refs for g in ngrams(r, n)))
    return df


def item_stats(hyp, refs, df=None, n_docs=None):
    """One item by the formulas of include/univl_hip.h: UnivlCaptionOverlap, with dictionaries.  Rows are sequences of hashables."""
    L = len(hyp)
    out = dict(guess=[max(0, L - n + 1) for n in range(1, 5)], correct=[], hyp_len=L)
    for n in range(1, 5):
        ch = Counter(ngrams(hyp, n))
        cr = [Counter(ngrams(r, n)) for r in refs]
        out["correct"].append(sum(min(c, max(x[g] for x in cr)) for g, c in ch.items()))
    out["ref_len"] = min((abs(len(r) - L), len(r)) for r in refs)[1]
    out["lcs"] = [lcs_len(hyp, r) for r in refs]
    p = max(l / max(L, 1) for l in out["lcs"])
    q = max(l / max(len(r), 1) for l, r in zip(out["lcs"], refs))
    beta = 1.2
    out["rouge_l"] = (1 + beta ** 2) * p * q / (q + beta ** 2 * p) if p != 0 and q != 0 else 0.0
    bleu = 1.0
    for k in range(4):
        bleu *= (out["correct"][k] + 1e-15) / (out["guess"][k] + 1e-9)
    bleu = bleu ** 0.25
    ratio = (L + 1e-15) / (out["ref_len"] + 1e-9)
    out["bleu"] = bleu * math.exp(1 - 1 / ratio) if ratio < 1 else bleu
    if df is not None:
        def vec(row, n):
            v = {g: c * (math.log(n_docs) - math.log(max(1, df[n - 1][g]))) for g, c in Counter(ngrams(row, n)).items()}
            return v, math.sqrt(sum(w * w for w in v.values()))
        score = 0.0
        for r in refs:
            d = max(L - 1, 0) - max(len(r) - 1, 0)
            vals = []
            for n in range(1, 5):
                vh, nh = vec(hyp, n)
                vr, nr = vec(r, n)
                val = sum(min(w, vr.get(g, 0.0)) * vr.get(g, 0.0) for g, w in vh.items())
                if nh != 0 and nr != 0:
                    val /= nh * nr
                vals.append(val * math.exp(-(d ** 2) / (2 * 6.0 ** 2)))
            score += sum(vals) / 4
        out["cider"] = 10.0 * score / len(refs)
    return out


def restate(hyps, ref_lists):
    """The corpus: (metrics dictionary, per-item list).  ref_lists[i] = the references of item i; n_docs = the number of items."""
    df = doc_freq(ref_lists)
    items = [item_stats(h, refs, df, len(hyps)) for h, refs in zip(hyps, ref_lists)]
    out, bleu = {}, 1.0
    ratio = (sum(it["hyp_len"] for it in items) + 1e-15) / (sum(it["ref_len"] for it in items) + 1e-9)
    for k in range(4):
        bleu *= (sum(it["correct"][k] for it in items) + 1e-15) / (sum(it["guess"][k] for it in items) + 1e-9)
        out["Bleu_%d" % (k + 1)] = bleu ** (1.0 / (k + 1)) * (math.exp(1 - 1 / ratio) if ratio < 1 else 1.0)
    out["METEOR"] = float("nan")
    out["ROUGE_L"] = sum(it["rouge_l"] for it in items) / len(items)
    out["CIDEr"] = sum(it["cider"] for it in items) / len(items)
    return out, items


def key_of(gram):
    return sum((int(s) + 1) << (16 * j) for j, s in enumerate(gram))


def df_tables(df):
    """The restatement's document frequencies as the kernel's tables (integer symbols): (keys, counts, df_begin)."""
    keys, cnts, begin = [], [], [0]
    for n in range(4):
        pairs = sorted((key_of(g), c) for g, c in df[n].items())
        keys += [k for k, _ in pairs]
        cnts += [c for _, c in pairs]
        begin.append(len(keys))
    return np.array(keys, dtype=np.uint64), np.array(cnts, dtype=np.int32), begin


# ------------------------------------------------------------------------------------------------ the C surface
def test_overlap_symbols_are_declared_exported_and_bound():
    L = _lib.lib()
    declared = set(re.findall(r"\b(univl_[a-z0-9_]+)\s*\(", HEADER))
    for name in ("univl_caption_overlap", "univl_caption_overlap_sizeof", "univl_consensus_pick"):
        assert name in declared and name in _lib.EXPORTED and hasattr(L, name)
    assert declared == set(_lib.EXPORTED)
    fn = L.univl_caption_overlap
    assert fn.restype is C.c_int32 and list(fn.argtypes) == [C.c_void_p, C.c_void_p]
    m = re.search(r"int\s+univl_consensus_pick\s*\(([^;]*)\)\s*;", HEADER)
    params = [p.strip() for p in m.group(1).split(",")]
    fn = L.univl_consensus_pick
    assert fn.restype is C.c_int32 and len(fn.argtypes) == len(params) == 6
    for p, t in zip(params, fn.argtypes):
        assert (t is C.c_void_p) == ("*" in p or "hipStream_t" in p), (p, t)
    assert callable(ops.caption_overlap) and callable(ops.consensus_pick)


def test_overlap_struct_mirrors_the_header():
    body = re.search(r"typedef struct UnivlCaptionOverlap \{(.*?)\} UnivlCaptionOverlap;", HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    kinds = {"int32_t": _lib.i32, "int64_t": _lib.i64, "uint64_t": _lib.u64, "float": _lib.f32, "double": C.c_double, "ptr": _lib.vp}
    want = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(const\s+)?(\w+)\s*(\*?)\s*(.*)", decl)
        for nm in m.group(4).split(","):
            kind = kinds["ptr" if m.group(3) else m.group(2)]
            arr = re.match(r"(\w+)\[(\d+)\]", nm.strip())
            want.append((arr.group(1), kind * int(arr.group(2))) if arr else (nm.strip(), kind))
    assert [(n, t) for n, t in _lib.CaptionOverlap._fields_] == want
    L = _lib.lib()
    assert L.univl_caption_overlap_sizeof() == C.sizeof(_lib.CaptionOverlap)
    assert int(re.search(r"#define UNIVL_OVERLAP_TMAX (\d+)", HEADER).group(1)) == _lib.OVERLAP_TMAX == 128
    assert int(re.search(r"#define UNIVL_OVERLAP_SYM_MAX (\d+)", HEADER).group(1)) == _lib.OVERLAP_SYM_MAX == 65534
    for name in ("BAD_LEN", "BAD_SYM", "BAD_ROW", "BAD_REFS"):
        assert int(re.search(r"#define UNIVL_OVERLAP_%s (\d+)" % name, HEADER).group(1)) == getattr(_lib, "OVERLAP_" + name)


def test_both_size_tables_are_unchanged():
    """The descriptor is in neither numbered table: twelve structs in univl_abi_sizeof, eleven in univl_struct_size, -1 past them."""
    L = _lib.lib()
    assert _lib.CaptionOverlap not in _lib._STRUCTS and len(_lib._STRUCTS) == 12
    assert L.univl_abi_sizeof(12) == -1 and L.univl_abi_sizeof(13) == -1 and L.univl_struct_size(11) == -1
    for k in range(12):
        assert L.univl_abi_sizeof(k) == C.sizeof(_lib._STRUCTS[k])
    for k in range(11):
        assert L.univl_struct_size(k) == C.sizeof(_lib._STRUCTS[k])


# ------------------------------------------------------------------------------------------------ hand-computed cases
def test_restatement_identical():
    a, b = "a b c d".split(), "e f g h".split()
    m, items = restate([a, b], [[a], [b]])
    for it in items:
        assert it["guess"] == it["correct"] == [4, 3, 2, 1] and it["hyp_len"] == it["ref_len"] == 4 and it["lcs"] == [4]
        assert it["rouge_l"] == pytest.approx(1.0, abs=1e-15)
        assert it["cider"] == pytest.approx(10.0, abs=1e-12)            # idf = log 2 everywhere, cosine 1, no length penalty
        assert it["bleu"] == pytest.approx(1.0, abs=1e-9)
    for k in range(1, 5):
        assert m["Bleu_%d" % k] == pytest.approx(1.0, abs=1e-9)
    assert m["ROUGE_L"] == pytest.approx(1.0) and m["CIDEr"] == pytest.approx(10.0) and math.isnan(m["METEOR"])
    assert tuple(m) == KEYS


def test_restatement_disjoint():
    m, items = restate(["a b c".split(), "x y".split()], [["d e f g".split()], ["x y".split()]])
    it = items[0]
    assert it["guess"] == [3, 2, 1, 0] and it["correct"] == [0, 0, 0, 0] and it["lcs"] == [0] and it["ref_len"] == 4
    assert it["rouge_l"] == 0.0 and it["cider"] == 0.0
    assert it["bleu"] < 1e-6


def test_restatement_clipping():
    """`the the the the` against `the cat`, `the the`: a unigram counts at most as often as in the reference that holds it most."""
    hyp, refs = "the the the the".split(), ["the cat".split(), "the the".split()]
    it = item_stats(hyp, refs)
    assert it["guess"] == [4, 3, 2, 1] and it["correct"] == [2, 1, 0, 0]
    assert it["hyp_len"] == 4 and it["ref_len"] == 2 and it["lcs"] == [1, 2]
    assert it["rouge_l"] == pytest.approx(2.44 * 0.5 * 1.0 / (1.0 + 1.44 * 0.5), rel=1e-14)      # p = 2/4, q = max(1/2, 2/2)
    # ties of |l - L| go to the shorter reference
    assert item_stats("a b c".split(), ["a b c d".split(), "a b".split()])["ref_len"] == 2


def test_restatement_empty_hypothesis():
    m, items = restate([[], "a b".split()], [["a b c".split(), "a".split()], ["a b".split()]])
    it = items[0]
    assert it["guess"] == [0, 0, 0, 0] and it["correct"] == [0, 0, 0, 0] and it["hyp_len"] == 0 and it["ref_len"] == 1
    assert it["lcs"] == [0, 0] and it["rouge_l"] == 0.0 and it["cider"] == 0.0 and it["bleu"] == 0.0      # exp(1 - 1 / 1e-15) underflows
    assert all(math.isfinite(m[k]) for k in KEYS if k != "METEOR")


def test_restatement_idf_zero():
    """One item: every n-gram of its references has df == n_docs, so every idf, every weight and every norm is 0 and CIDEr is 0 even
    for a perfect hypothesis (the undivided val_n is a sum of zeros)."""
    row = "a b c d e".split()
    m, items = restate([row], [[row]])
    assert items[0]["cider"] == 0.0 and m["CIDEr"] == 0.0 and items[0]["rouge_l"] == pytest.approx(1.0)
    # two items sharing the unigram `a` (df 2 of 2: idf 0) but not the others
    m, items = restate(["a b".split(), "a c".split()], [["a b".split()], ["a c".split()]])
    w = math.log(2.0)
    assert items[0]["cider"] == pytest.approx(10.0 * (1.0 + 1.0 + 0.0 + 0.0) / 4, rel=1e-14) and w > 0


def test_lcs_and_keys():
    assert lcs_len("abcbdab", "bdcaba") == 4 and lcs_len("", "abc") == 0 and lcs_len("aaaa", "aa") == 2
    assert key_of((0,)) == 1 and key_of((65534,)) == 65535 and key_of((1, 2)) == 2 + (3 << 16)
    assert key_of((0, 0, 0, 65534)) == 1 + (1 << 16) + (1 << 32) + (65535 << 48) < 2 ** 64
    assert key_of((65534,)) < key_of((0, 0)) and key_of((65534, 65534, 65534)) < key_of((0, 0, 0, 0))       # tables of n follow each other


def test_host_document_frequency_equals_the_restatement():
    rng = np.random.RandomState(5)
    hyps = [rng.randint(0, 7, size=rng.randint(0, 12)).tolist() for _ in range(9)]
    refs = [[rng.randint(0, 7, size=rng.randint(0, 12)).tolist() for _ in range(1 + i % 3)] for i in range(9)]
    rows = hyps + [r for rr in refs for r in rr]
    sym, lens = M._pack(rows)
    ref_begin = np.concatenate([[0], np.cumsum([len(r) for r in refs])]).astype(np.int32)
    ref_rows = np.arange(9, 9 + int(ref_begin[-1]), dtype=np.int32)
    keys, cnts, begin = M.document_frequency(sym, lens, ref_begin, ref_rows)
    wk, wc, wb = df_tables(doc_freq(refs))
    assert begin == wb and keys.tolist() == wk.tolist() and cnts.tolist() == wc.tolist()
    assert keys.dtype == np.uint64 and bool((keys[1:] > keys[:-1]).all())


def test_corpus_arithmetic_equals_the_restatement():
    hyps = ["a b c d e".split(), "a a b".split(), []]
    refs = [["a b c e".split(), "b c d e f g".split()], ["a b".split()], ["c".split()]]
    want, items = restate(hyps, refs)
    arr = lambda k, dt: np.array([it[k] for it in items], dtype=dt)
    got = M.corpus_scores(arr("guess", np.int32), arr("correct", np.int32), arr("hyp_len", np.int32), arr("ref_len", np.int32),
                          arr("rouge_l", np.float64), arr("cider", np.float64))
    assert tuple(got) == KEYS
    for k in KEYS:
        assert math.isnan(got[k]) if k == "METEOR" else abs(got[k] - want[k]) <= 1e-12, k


def test_input_range_is_refused_on_the_host():
    """Arguments are validated before a device is asked for: the same ValueErrors with and without a GPU."""
    cm = M.CaptionMetrics()
    with pytest.raises(ValueError):
        M._pack([[1] * 129])
    with pytest.raises(ValueError):
        M._pack([[65535]])
    with pytest.raises(ValueError):
        M._pack([[-1]])
    assert M._pack([[65534], []])[0].tolist() == [[65534], [0]]
    for hyp_ids, ref_ids in (([], []), ([[1]], [[]]), ([[1]], [[[1]], [[2]]]), ([[1] * 129], [[[1]]]), ([[1]], [[[1] * 129]]),
                             ([[65535]], [[[1]]]), ([[1]], [[[-1]]])):
        with pytest.raises(ValueError):
            cm.compute_ids(hyp_ids, ref_ids)
    with pytest.raises(ValueError):
        cm.compute_metrics(ref_list=[["a", "b"]], hyp_list=["a"])                  # two references for one hypothesis
    with pytest.raises(ValueError):
        cm.compute_metrics(ref_list=[], hyp_list=["a"])
    with pytest.raises(ValueError, match="distinct words"):
        cm.compute_metrics(ref_list=[[" ".join("w%d" % i for i in range(40000))] * 2], hyp_list=["w1", " ".join("v%d" % i for i in range(40000))])
    with pytest.raises(ValueError, match="128"):
        cm.compute_metrics(ref_list=[["a"]], hyp_list=["a " * 129])
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            cm.compute_ids([[1]], [[[1]]])
        with pytest.warns(UserWarning, match="1 of 2 rows"), pytest.raises(RuntimeError, match="no CPU fallback"):
            M.CaptionMetrics(truncate=True).compute_ids([[1] * 129], [[[1]]])     # cut, warned, and only then the device is missed


def test_shim_stub_delegates_to_caption_metrics():
    """run_univl_amd.install_compat's nlgeval stub without a GPU: the constructor takes NLGEval's keywords, and compute_metrics is
    CaptionMetrics' -- malformed lists are its ValueError, well-formed ones reach the device check (no CPU fallback) instead of
    "nlgeval is not installed".  What it RETURNS is checked on the GPU (tests/test_caption_metrics_gpu.py).  Everything the shim
    installs is taken out again afterwards."""
    import run_univl_amd
    names = ("nlgeval", "boto3", "botocore", "botocore.exceptions")
    saved = {k: sys.modules.get(k) for k in names}
    np_had = {k: k in np.__dict__ for k in ("float", "int", "bool", "object", "long")}
    sys.modules.pop("nlgeval", None)
    try:
        run_univl_amd.install_compat()
        import nlgeval
        if hasattr(nlgeval, "__file__"):
            pytest.skip("a real nlgeval is installed: the shim leaves it alone")
        obj = nlgeval.NLGEval(no_overlap=False, no_skipthoughts=True, no_glove=True, metrics_to_omit=None)
        with pytest.raises(ValueError):
            obj.compute_metrics(ref_list=[["a", "b"]], hyp_list=["a"])
        if not torch.cuda.is_available():
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                obj.compute_metrics(ref_list=[["a man is cooking", "a dog runs"]], hyp_list=["a man cooking", "a dog runs"])
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
        for k, had in np_had.items():
            if not had and k in np.__dict__:
                delattr(np, k)
