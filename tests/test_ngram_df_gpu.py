"""Document-frequency tables built on the device: univl_ngram_df (csrc/ngram_df.hip), ops.ngram_df, caption_metrics.DocumentFrequency,
CaptionMetrics(df="device") and the CIDEr reward of univl_amd.rl.  Needs a real MI355X (`-m gpu`).

The comparand is caption_metrics.document_frequency (numpy on the host; tests/test_caption_metrics_cpu.py pins it to the dictionary
restatement): keys viewed as uint64, counts and the five begins are compared by exact integer equality.

A  smallest shapes, lane and word roles, deduplication, unsigned order, one bucket, the sort's tile edges, several workgroups, repeatability;
B  overflow, clamped device data, argument range;
C  DocumentFrequency and CaptionMetrics(df="device");  D  caption_rewards / scst_step with metric="cider".

GATE of D: the cider value is formed by the unchanged overlap kernel from tables that are equal to the host's, so the gate is the one
tests/test_caption_metrics_gpu.py uses for cider, 1e-10 relative + 1e-12 absolute."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

from test_caption_metrics_cpu import doc_freq, item_stats

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import univl_amd
    from univl_amd import _lib, ops, rl
    from univl_amd.caption_metrics import CaptionMetrics, DocumentFrequency, document_frequency

DEV = "cuda"
EINVAL = -1
CIDER_RTOL, CIDER_ATOL = 1e-10, 1e-12


def _dev(a, dtype=torch.int32):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV)


def _table(rows, T=None, junk_seed=None):
    """Lists of symbols -> (sym [rows, T] int64, lens).  junk_seed: positions past a length hold -1 / 70000, which must not be read."""
    T = T or max(1, max(len(r) for r in rows))
    sym = np.zeros((len(rows), T), dtype=np.int64)
    if junk_seed is not None:
        sym = np.where(np.random.RandomState(junk_seed).rand(len(rows), T) < 0.5, -1, 70000).astype(np.int64)
    for k, r in enumerate(rows):
        sym[k, :len(r)] = r
    return sym, np.array([len(r) for r in rows], dtype=np.int32)


def _lists(docs):
    ref_begin = np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.int32)
    return ref_begin, np.array([r for d in docs for r in d], dtype=np.int32)


def _launch(sym, lens, ref_begin, ref_rows, ld=None, capacity=None):
    """One ops.ngram_df launch -> (keys uint64 [begin[4]], counts, begin, status) on the host."""
    s = _dev(sym)
    if ld is not None:                                                         # a row stride above T
        wide = torch.full((s.shape[0], ld), 70000, dtype=torch.int32, device=DEV)
        wide[:, :s.shape[1]] = s
        s = wide[:, :s.shape[1]]
    keys, cnt, begin, status = ops.ngram_df(s, _dev(lens), _dev(ref_begin), _dev(ref_rows), len(ref_rows), capacity=capacity)
    torch.cuda.synchronize()
    begin = begin.cpu().tolist()
    return keys.cpu().numpy().view(np.uint64)[:begin[4]], cnt.cpu().numpy()[:begin[4]], begin, int(status.cpu()[0])


def _same(got, want, tag):
    keys, cnt, begin = got[:3]
    wk, wc, wb = want
    assert begin == [int(b) for b in wb], (tag, begin, wb)
    assert keys.dtype == np.uint64 and np.array_equal(keys, wk), tag
    assert np.array_equal(cnt, wc), tag


def _check(rows, docs, tag, T=None, ld=None, junk_seed=None):
    sym, lens = _table(rows, T, junk_seed)
    ref_begin, ref_rows = _lists(docs)
    clean = np.where(np.arange(sym.shape[1])[None, :] < lens[:, None], sym, 0)
    want = document_frequency(clean, lens, ref_begin, ref_rows)
    got = _launch(sym, lens, ref_begin, ref_rows, ld=ld)
    assert got[3] == 0, (tag, got[3])
    _same(got, want, tag)
    return got


# ------------------------------------------------------------------------------------------------ A: the tables
def test_smallest_shapes():
    keys, cnt, begin, _ = _check([[5]], [[0]], "one unigram")
    assert begin == [0, 1, 1, 1, 1] and keys.tolist() == [6] and cnt.tolist() == [1]
    rows = [[], [3], [3, 4], [3, 4, 5], [3, 4, 5, 6]]
    keys, cnt, begin, _ = _check(rows, [[k] for k in range(5)], "lengths 0 .. 4")
    assert begin == [0, 4, 7, 9, 10] and cnt[:4].tolist() == [4, 3, 2, 1]      # n-grams that do not fit are not counted
    _check(rows, [[4], [], [2]], "an empty document between two others")
    _check(rows, [[0], [0, 0]], "documents of empty rows only")
    assert _check(rows, [[], [0]], "nothing at all")[2] == [0, 0, 0, 0, 0]


def test_lane_and_word_roles():
    rng = np.random.RandomState(3)
    rows = [rng.randint(0, 7, size=l).tolist() for l in (63, 64, 65, 127, 128, 128)]
    _check(rows, [[0], [1], [2], [3], [4], [5, 0, 3]], "T = 128, ld = 136", T=128, ld=136, junk_seed=4)
    _check(rows, [[4, 5, 3, 2, 1, 0]], "one document of six long rows", T=128, ld=136, junk_seed=5)


def test_deduplication():
    rng = np.random.RandomState(8)
    rows = [rng.randint(0, 7, size=rng.randint(0, 25)).tolist() for _ in range(30)]
    docs = [[0], [1, 2], [3, 4, 5, 6, 7], list(range(8, 28)),                  # 1, 2, 5 and 20 rows
            [27, 5], [28, 5],                                                  # two documents sharing a row (and one with the 20)
            [12, 3, 29, 9], [4, 4]]                                            # non-monotone order; one row twice
    keys, cnt, begin, _ = _check(rows, docs, "repeats within rows, across rows and across documents", junk_seed=9)
    assert int(cnt.max()) == len(docs) and begin[1] == 7                       # a symbol in every document; seven unigrams


def test_unsigned_order():
    rng = np.random.RandomState(21)
    alphabet = np.array([0, 1, 32766, 32767, 32768, 65533, 65534])
    rows = [alphabet[rng.randint(0, 7, size=rng.randint(1, 13))].tolist() for _ in range(40)] + [[65534] * 4]
    keys, cnt, begin, _ = _check(rows, [[2 * k, 2 * k + 1] for k in range(20)] + [[40]], "bit 63 and the field boundaries")
    assert bool((keys[1:] > keys[:-1]).all()) and int(keys[-1]) == 2 ** 64 - 1 and int((keys >> np.uint64(63)).sum()) > 10
    assert keys.view(np.int64).min() < 0                                       # a signed order would have put these first


def test_one_bucket():
    keys, cnt, begin, _ = _check([[2, 2, 2, 2]] * 500, [[k] for k in range(500)], "500 x `a a a a`")
    assert begin == [0, 1, 2, 3, 4] and cnt.tolist() == [500] * 4


def _keys_of_length(L):
    return sum(max(0, L - n + 1) for n in range(1, 5))                         # 4 L - 6 from L = 4 on


@functools.lru_cache(maxsize=None)
def _distinct_rows(target):
    """Rows of pairwise distinct symbols, one document each, that hold exactly `target` n-grams: nothing is deduplicated, so the
    emitted count, the sorted count and the table size are all `target`."""
    lengths, left = [], target
    while left >= 1100:
        lengths.append(128)
        left -= _keys_of_length(128)
    best = {0: []}                                                              # fewest rows for every remainder
    for v in range(1, left + 1):
        for L in range(128, 0, -1):
            k = _keys_of_length(L)
            if k <= v and (v - k) in best and (v not in best or len(best[v - k]) + 1 < len(best[v])):
                best[v] = best[v - k] + [L]
    lengths += best[left]
    rows, at = [], 0
    for L in lengths:
        rows.append(list(range(at, at + L)))
        at += L
    assert sum(_keys_of_length(len(r)) for r in rows) == target and at <= 65534
    return rows


@pytest.mark.parametrize("which", ["tile - 1", "tile", "tile + 1", "3 tile + 5"])
def test_tile_edges_of_the_sort(which):
    tile = _lib.NGRAM_DF_TILE
    assert tile == _lib.lib().univl_ngram_df_tile()
    target = {"tile - 1": tile - 1, "tile": tile, "tile + 1": tile + 1, "3 tile + 5": 3 * tile + 5}[which]
    rows = _distinct_rows(target)
    keys, cnt, begin, _ = _check(rows, [[k] for k in range(len(rows))], which, T=128)
    assert begin[4] == target and bool((cnt == 1).all())


@functools.lru_cache(maxsize=None)
def _several_workgroups():
    rng = np.random.RandomState(17)
    rows = [rng.randint(0, 50, size=rng.randint(1, 25)).tolist() for _ in range(900)]
    return rows, [[3 * k, 3 * k + 1, 3 * k + 2] for k in range(300)]


def test_several_workgroups():
    rows, docs = _several_workgroups()
    keys, cnt, begin, _ = _check(rows, docs, "300 documents x 3 rows")
    assert begin[4] > 2 * _lib.NGRAM_DF_TILE                                   # the distinct keys alone fill more than two tiles


def test_two_launches_give_the_same_bits():
    rows, docs = _several_workgroups()
    sym, lens = _table(rows)
    ref_begin, ref_rows = _lists(docs)
    args = (_dev(sym), _dev(lens), _dev(ref_begin), _dev(ref_rows), len(ref_rows))
    a, b = ops.ngram_df(*args), ops.ngram_df(*args)
    torch.cuda.synchronize()
    n = int(a[2].cpu()[4])
    assert torch.equal(a[2], b[2]) and torch.equal(a[0][:n], b[0][:n]) and torch.equal(a[1][:n], b[1][:n]) and n > 0


# ------------------------------------------------------------------------------------------------ B: overflow, clamping, range
class _Raw:
    """The C entry point with caller-owned arrays: df_keys / df_cnt are `guard` entries longer than the stated capacity."""

    def __init__(self, sym, lens, ref_begin, ref_rows, capacity, guard=64):
        self.sym, self.lens, self.ref_begin, self.ref_rows = _dev(sym), _dev(lens), _dev(ref_begin), _dev(ref_rows)
        self.capacity, self.n_refs = capacity, len(ref_rows)
        self.keys = torch.full((capacity + guard,), -0x0123456789ABCDEF, dtype=torch.int64, device=DEV)
        self.cnt = torch.full((capacity + guard,), -77, dtype=torch.int32, device=DEV)
        self.begin = torch.full((5,), -77, dtype=torch.int32, device=DEV)
        self.status = torch.zeros(1, dtype=torch.int32, device=DEV)
        self.need = int(_lib.lib().univl_ngram_df_ws_bytes(self.n_refs, self.sym.shape[1]))
        self.ws = torch.zeros(self.need, dtype=torch.uint8, device=DEV)

    def call(self, **kw):
        p = lambda t: t.data_ptr()
        d = _lib.NgramDf()
        d.sym, d.ld, d.len, d.rows, d.T = p(self.sym), self.sym.stride(0), p(self.lens), self.sym.shape[0], self.sym.shape[1]
        d.items, d.n_refs, d.ref_begin, d.ref_rows = self.ref_begin.numel() - 1, self.n_refs, p(self.ref_begin), p(self.ref_rows)
        d.df_keys, d.df_cnt, d.df_begin, d.status, d.capacity = p(self.keys), p(self.cnt), p(self.begin), p(self.status), self.capacity
        d.ws, d.ws_bytes = p(self.ws), self.need
        for k, v in kw.items():
            setattr(d, k, v)
        rc = _lib.lib().univl_ngram_df(C.byref(d), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        return rc

    def untouched(self, start):
        return bool((self.keys[start:] == -0x0123456789ABCDEF).all()) and bool((self.cnt[start:] == -77).all())


def test_overflow_is_flagged_and_nothing_is_written_past_the_capacity():
    rng = np.random.RandomState(33)
    rows = [rng.randint(0, 9, size=rng.randint(1, 20)).tolist() for _ in range(40)]
    docs = [[2 * k, 2 * k + 1] for k in range(20)]
    sym, lens = _table(rows)
    ref_begin, ref_rows = _lists(docs)
    wk, wc, wb = document_frequency(sym, lens, ref_begin, ref_rows)
    true = int(wb[4])
    exact = _Raw(sym, lens, ref_begin, ref_rows, true)
    assert exact.call() == 0 and int(exact.status.cpu()[0]) == 0 and exact.untouched(true)
    _same((exact.keys.cpu().numpy().view(np.uint64)[:true], exact.cnt.cpu().numpy()[:true], exact.begin.cpu().tolist()), (wk, wc, wb), "capacity = count")
    short = _Raw(sym, lens, ref_begin, ref_rows, true - 1)
    assert short.call() == 0
    assert int(short.status.cpu()[0]) == _lib.NGRAM_DF_OVERFLOW and short.untouched(true - 1)
    begin = short.begin.cpu().tolist()
    assert begin[0] == 0 and all(0 <= b <= true - 1 for b in begin) and begin == sorted(begin)
    tiny = _Raw(sym, lens, ref_begin, ref_rows, 1)
    assert tiny.call() == 0 and int(tiny.status.cpu()[0]) == _lib.NGRAM_DF_OVERFLOW and tiny.untouched(1)
    assert all(0 <= b <= 1 for b in tiny.begin.cpu().tolist())


def test_clamped_device_data():
    """A length, a symbol, a row index or a reference offset out of range: flagged, never read out of range, and the tables are those
    of the clamped data (the pattern of test_largest_symbol_and_clamped_device_data)."""
    T = 8
    rows = [[1, 2, 3, 4, 5, 6, 7, 8], [65534, 0, 65534, 5], [0, 65534, 5], [4, 4, 1, 2, 2]]
    docs = [[0, 1], [2], [3, 1]]
    sym, lens = _table(rows, T)
    ref_begin, ref_rows = _lists(docs)

    def run(tag, flag, sym_=sym, lens_=lens, begin_=ref_begin, rows_=ref_rows, want=None):
        got = _launch(sym_, lens_, begin_, rows_)
        assert got[3] == flag, (tag, got[3])
        _same(got, want, tag)

    sym_full = sym.copy()
    sym_full[2, 3:], sym_full[3, 5:] = [7, 7, 7, 7, 7], [9, 8, 7]
    l_bad, l_clamped = lens.copy(), lens.copy()
    l_bad[2], l_bad[3], l_clamped[2], l_clamped[3] = T + 5, -1, T, 0
    run("lengths T + 5 and -1", _lib.OVERLAP_BAD_LEN, sym_=sym_full, lens_=l_bad, want=document_frequency(sym_full, l_clamped, ref_begin, ref_rows))
    s_bad, s_clamped = sym.copy(), sym.copy()
    s_bad[0, 1], s_bad[3, 0], s_clamped[0, 1], s_clamped[3, 0] = 70000, -7, 65534, 0
    run("symbols 70000 and -7", _lib.OVERLAP_BAD_SYM, sym_=s_bad, want=document_frequency(s_clamped, lens, ref_begin, ref_rows))
    r_bad, r_clamped = ref_rows.copy(), ref_rows.copy()
    r_bad[2], r_bad[0], r_clamped[2], r_clamped[0] = len(rows), -3, len(rows) - 1, 0
    run("row indices `rows` and -3", _lib.OVERLAP_BAD_ROW, rows_=r_bad, want=document_frequency(sym, lens, ref_begin, r_clamped))
    # decreasing offsets: document 1 = [3, 2) is empty and flagged; documents 0 = [0, 3) and 2 = [2, 5) share list entry 2
    b_bad = np.array([0, 3, 2, 5], dtype=np.int32)
    eq_begin, eq_rows = _lists([list(ref_rows[0:3]), [], list(ref_rows[2:5])])
    run("decreasing ref_begin", _lib.OVERLAP_BAD_REFS, begin_=b_bad, want=document_frequency(sym, lens, eq_begin, eq_rows))
    # offsets outside [0, n_refs]: clamped into the list
    b_out = np.array([-2, 3, 3, 9], dtype=np.int32)
    eq_begin, eq_rows = _lists([list(ref_rows[0:3]), [], list(ref_rows[3:5])])
    run("offsets outside the list", _lib.OVERLAP_BAD_REFS, begin_=b_out, want=document_frequency(sym, lens, eq_begin, eq_rows))


def test_argument_range():
    sym, lens = _table([[1, 2, 3], [4, 5]], 128)
    ref_begin, ref_rows = _lists([[0], [1]])
    r = _Raw(sym, lens, ref_begin, ref_rows, 16)
    L = _lib.lib()
    for kw in (dict(T=0), dict(T=129), dict(ld=127), dict(rows=0), dict(items=0), dict(n_refs=0), dict(capacity=0), dict(capacity=-4),
               dict(sym=None), dict(len=None), dict(ref_begin=None), dict(ref_rows=None), dict(df_keys=None), dict(df_cnt=None),
               dict(df_begin=None), dict(status=None), dict(ws=None), dict(ws_bytes=r.need - 1), dict(ws_bytes=0)):
        assert r.call(**kw) == EINVAL, kw
        assert L.univl_last_error()
    assert L.univl_ngram_df(None, None) == EINVAL
    assert r.untouched(0) and r.begin.cpu().tolist() == [-77] * 5 and int(r.status.cpu()[0]) == 0        # nothing was launched
    assert r.call() == 0 and r.begin.cpu().tolist() == [0, 5, 8, 9, 9] and r.untouched(9)


# ------------------------------------------------------------------------------------------------ C: DocumentFrequency, CaptionMetrics
def test_document_frequency_object():
    rng = np.random.RandomState(41)
    n, n_ref, T = 6, 3, 17
    ids = rng.randint(0, 9, size=(n, n_ref, T)).astype(np.int64)
    rlen = rng.randint(0, T + 1, size=(n, n_ref)).astype(np.int64)
    want = document_frequency(ids.reshape(n * n_ref, T), rlen.reshape(-1), np.arange(n + 1, dtype=np.int32) * n_ref,
                              np.arange(n * n_ref, dtype=np.int32))
    for where in ("cpu", DEV):
        df = DocumentFrequency.from_ids(torch.from_numpy(ids).to(where), torch.from_numpy(rlen).to(where), device=DEV)
        assert df.n_docs == n and df.keys.is_cuda and df.cnt.is_cuda and df.keys.dtype == torch.int64 and df.cnt.dtype == torch.int32
        assert df.keys.numel() == df.cnt.numel() == df.begin[4] and all(isinstance(b, int) for b in df.begin)
        assert df.tables == (df.keys, df.cnt, df.begin, n)
        _same(df.to_host(), want, "from_ids " + where)
    lists = [[ids[i, r, :rlen[i, r]].tolist() for r in range(n_ref)] for i in range(n)] + [[]]
    df = DocumentFrequency.from_lists(lists)
    assert df.n_docs == n + 1
    _same(df.to_host(), want, "from_lists")
    with pytest.raises(RuntimeError, match="status 2"):
        DocumentFrequency.from_ids(torch.full((1, 1, 4), 70000), torch.full((1, 1), 4))


def test_caption_metrics_with_device_tables():
    """The seeded sentences of tests/test_caption_metrics_gpu.py, three references each: the same tables go into the same kernel, so
    every number is EQUAL (METEOR is nan on both sides)."""
    from test_caption_metrics_gpu import WORDS, _sentences
    hyps = _sentences(37, 1)
    hyps[5] = ""
    single = _sentences(37, 2, lo=1)
    per_item = [[single[i]] + _sentences(2, 100 + i, lo=1) for i in range(37)]
    ids = {w: k for k, w in enumerate(WORDS)}
    enc = lambda s: [ids[w] for w in s.split()]
    args = ([enc(h) for h in hyps], [[enc(r) for r in rr] for rr in per_item])
    host, dev = CaptionMetrics(df="host"), CaptionMetrics(df="device")
    a, b = host.compute_ids(*args), dev.compute_ids(*args)
    assert tuple(a) == tuple(b) and math.isnan(a["METEOR"]) and math.isnan(b["METEOR"])
    assert {k: v for k, v in a.items() if k != "METEOR"} == {k: v for k, v in b.items() if k != "METEOR"}
    assert a["CIDEr"] > 0.0 and set(host.last) == set(dev.last)
    for k in host.last:
        assert np.array_equal(host.last[k], dev.last[k]), k


# ------------------------------------------------------------------------------------------------ D: the CIDEr reward
ABSENT, EVERYWHERE = 9, 8                                                      # a symbol of no document; a symbol of every document


def _cider_case():
    """The crafted samples of tests/test_caption_rl_gpu.py and a corpus of 12 documents: the batch's 3 videos and 9 more.  Every
    document holds symbol 8 (df = n_docs: idf 0); symbol 9 is in no document (df 0) but in two samples."""
    from test_caption_rl_gpu import _crafted_samples
    tok, slen, ref, rlen = _crafted_samples()
    ref[:, 0, 0] = EVERYWHERE
    tok[0, 1] = ref[0, 0]                                                      # sample (0, 1) stays the copy of reference (0, 0)
    tok[0, 1, slen[0, 1]:] = -1
    tok[2, 0, 0], tok[1, 0, 1] = ABSENT, ABSENT
    tok[2, 3, 5] = EVERYWHERE
    rng = np.random.RandomState(13)
    corpus = [[ref[i, k, :rlen[i, k]].tolist() for k in range(ref.shape[1])] for i in range(ref.shape[0])]
    corpus += [[[EVERYWHERE] + rng.randint(0, 7, size=rng.randint(1, 30)).tolist() for _ in range(1 + d % 3)] for d in range(9)]
    return tok, slen, ref, rlen, corpus


def test_cider_rewards_against_the_dictionary_restatement():
    from test_caption_rl_gpu import _as_result
    tok, slen, ref, rlen, corpus = _cider_case()
    n, ns, T = tok.shape
    df = doc_freq(corpus)
    assert len(corpus) == 12 and df[0][(EVERYWHERE,)] == 12 and df[0][(ABSENT,)] == 0
    table = DocumentFrequency.from_lists(corpus)
    assert table.n_docs == 12
    res = _as_result(tok, slen)
    ref_d, rlen_d = torch.from_numpy(ref).to(DEV), torch.from_numpy(rlen).to(DEV)
    r, o = rl.caption_rewards(res, ref_d, rlen_d, eos=-1, pad=-1, metric="cider", df=table, return_stats=True)
    assert r.shape == (n, ns) and r.dtype == torch.float64 and r.is_cuda and int(o["status"]) == 0
    got, worst = r.cpu().numpy(), 0.0
    want = np.zeros((n, ns))
    for i in range(n):
        refs = [ref[i, k, :rlen[i, k]].tolist() for k in range(ref.shape[1])]
        for s in range(ns):
            want[i, s] = item_stats(tok[i, s, :slen[i, s]].tolist(), refs, df, 12)["cider"]
            worst = max(worst, abs(got[i, s] - want[i, s]) / max(abs(want[i, s]), 1e-300) if got[i, s] != want[i, s] else 0.0)
    print("[cider reward] worst relative error %.2e; rewards %s" % (worst, np.round(got, 4).tolist()))
    assert (np.abs(got - want) <= CIDER_RTOL * np.abs(want) + CIDER_ATOL).all(), (got, want)
    assert got[0, 1] > got[0].mean() and got[1, 2] == 0.0 and (got >= 0.0).all() and got.max() > 1.0     # the copy; the empty sample; factor 10
    assert torch.equal(rl.caption_rewards(res, ref_d, rlen_d, -1, -1, metric="cider", df=table), r)
    # the other metrics ignore df
    assert torch.equal(rl.caption_rewards(res, ref_d, rlen_d, -1, -1, metric="rouge_l", df=table), rl.caption_rewards(res, ref_d, rlen_d, -1, -1))
    cpu_table = DocumentFrequency(table.keys.cpu(), table.cnt.cpu(), table.begin, table.n_docs)
    with pytest.raises(ValueError, match="the samples are on"):
        rl.caption_rewards(res, ref_d, rlen_d, -1, -1, metric="cider", df=cpu_table)


def test_cider_rewards_read_nothing_on_the_host(monkeypatch):
    """With the table built, rewards and advantages are device work only (the check of tests/test_caption_metrics_gpu.py:
    test_consensus_on_sampled_captions)."""
    import test_sample_gpu as G
    from test_caption_rl_gpu import _as_result
    tok, slen, ref, rlen, corpus = _cider_case()
    table = DocumentFrequency.from_lists(corpus)
    res = _as_result(tok, slen)
    ref_d, rlen_d = torch.from_numpy(ref).to(DEV), torch.from_numpy(rlen).to(DEV)
    want = rl.advantages(rl.caption_rewards(res, ref_d, rlen_d, -1, -1, metric="cider", df=table))
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    reads = G._HostReads(monkeypatch)
    try:
        torch.cuda.set_sync_debug_mode("error")
        adv = rl.advantages(rl.caption_rewards(res, ref_d, rlen_d, -1, -1, metric="cider", df=table), scale=0.1)
        n_reads = list(reads.calls)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert n_reads == []
    torch.cuda.synchronize()
    assert adv.shape == want.shape and float(adv.abs().max()) > 0.0


def test_scst_step_with_the_cider_reward():
    from test_caption_rl_gpu import BOS, T_RUN, _toy
    was = univl_amd.deterministic()
    univl_amd.set_deterministic(True)
    try:
        cfg, model, batch, smp = _toy()
        model.zero_grad(set_to_none=True)
        with torch.no_grad():
            seq, vis = model.get_sequence_visual_output(batch["input_ids"], batch["token_type_ids"], batch["attention_mask"], batch["video"],
                                                        batch["video_mask"])
            free = smp.sample(seq, vis, batch["attention_mask"].view(3, -1), batch["video_mask"].view(3, -1), BOS, -1, 9)
        eos = int(free.tokens.reshape(-1, T_RUN)[1, 2])
        ref_ids = free.tokens[:, :2].to(torch.int64).contiguous()
        ref_len = torch.tensor([[T_RUN, 4]] * 3, device=DEV)
        table = DocumentFrequency.from_ids(ref_ids, ref_len)
        assert table.n_docs == 3 and table.begin[4] > 0
        with pytest.raises(ValueError, match="needs df"):
            rl.scst_step(model, smp, batch, ref_ids, ref_len, BOS, eos, 0, seed=9, metric="cider")
        out = rl.scst_step(model, smp, batch, ref_ids, ref_len, BOS, eos, 0, seed=9, metric="cider", df=table, scale=0.1)
        assert out.rewards.shape == out.advantages.shape == (3, 4) and out.rewards.dtype == torch.float64
        assert math.isfinite(float(out.loss)) and bool((out.rewards >= 0.0).all()) and float(out.rewards.max()) > 0.0
        assert torch.equal(rl.caption_rewards(out.samples, ref_ids, ref_len, eos, 0, metric="cider", df=table), out.rewards)
        assert torch.equal(rl.advantages(out.rewards, scale=0.1), out.advantages)
        # leave-one-out advantages of a video sum to zero; each was rounded to fp32 once (relative 2^-24), the fp64 sums are far finer
        adv = out.advantages.double().cpu()
        assert bool((adv.sum(dim=1).abs() <= 2.0 ** -24 * adv.abs().sum(dim=1) + 1e-14).all()), adv
        out.loss.backward()
        grads = [p.grad for p in model.parameters() if p.grad is not None]
        assert grads and all(bool(torch.isfinite(g).all()) for g in grads)
        model.zero_grad(set_to_none=True)
    finally:
        univl_amd.set_deterministic(was)
