"""Caption metrics on the device: univl_caption_overlap / univl_consensus_pick (csrc/metric.hip), CaptionMetrics and consensus
(univl_amd/caption_metrics.py) against the dictionary restatement of tests/test_caption_metrics_cpu.py.

A  the kernel on seeded random rows over a 7-symbol alphabet (many repeats: clipping and LCS ties occur), every length at which a lane,
   a word of the bit vector or the staging changes role; integers exact, fp64 at the gates below;
B  symbol 65534, device data out of range (clamped and flagged, nothing faults), shared rows, argument range;
C  compute_ids / compute_metrics in both reference layouts, the launcher shim's nlgeval stub;  D  eval_caption with CaptionMetrics;  E  consensus.

GATES.  Integers: exact.  rouge_l: 1e-12 relative -- a handful of IEEE operations on small integers; contraction into fma may move
an ulp or two.  cider: 1e-10 relative + 1e-12 absolute -- about 1e3 terms at fp64 epsilon in a different order, with margin.  BLEU of
the corpus: 1e-12 (the same float64 host arithmetic on equal integers).  Sentence BLEU of an item (consensus): 1e-12 relative -- four
quotients, two square roots and one exponential whose argument is at most 128 in size."""
import functools
import math

import numpy as np
import pytest
import torch

from test_caption_metrics_cpu import KEYS, df_tables, doc_freq, item_stats, restate

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from univl_amd import _lib, ops
    from univl_amd.caption_metrics import CaptionMetrics, consensus

DEV = "cuda"
EINVAL = -1
LENGTHS = [0, 1, 3, 4, 63, 64, 65, 127, 128]
ROUGE_RTOL, CIDER_RTOL, CIDER_ATOL, BLEU_TOL = 1e-12, 1e-10, 1e-12, 1e-12


def _dev(a, dtype):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV)


def _launch(sym, lens, hyp_row, ref_lists, df=None, n_docs=None, bleu=True):
    """sym: [rows, T] host int array, lens: [rows]; ref_lists[i]: row indices.  Returns the kernel's outputs as host arrays."""
    ref_begin = np.concatenate([[0], np.cumsum([len(r) for r in ref_lists])]).astype(np.int32)
    ref_rows = np.array([r for rr in ref_lists for r in rr], dtype=np.int32)
    tables = None
    if df is not None:
        keys, cnts, begin = df_tables(df)
        tables = (_dev(keys.view(np.int64), torch.int64), _dev(cnts, torch.int32), begin, n_docs)
    o = ops.caption_overlap(_dev(sym, torch.int32), _dev(lens, torch.int32), _dev(hyp_row, torch.int32), _dev(ref_begin, torch.int32),
                            _dev(ref_rows, torch.int32), int(ref_begin[-1]), tables=tables, bleu=bleu)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items() if v is not None}


def _compare(got, want_items, ref_begin, tag, cider=True):
    """Prints the worst fp64 errors, then asserts: integers exact, fp64 at the gates."""
    worst = dict(rouge_l=0.0, cider=0.0, bleu=0.0)
    for i, w in enumerate(want_items):
        assert got["guess"][i].tolist() == w["guess"] and got["correct"][i].tolist() == w["correct"], (tag, i, got["correct"][i], w)
        assert int(got["hyp_len"][i]) == w["hyp_len"] and int(got["ref_len"][i]) == w["ref_len"], (tag, i)
        assert got["lcs"][ref_begin[i]:ref_begin[i + 1]].tolist() == w["lcs"], (tag, i)
        for k in ("rouge_l", "bleu") + (("cider",) if cider else ()):
            worst[k] = max(worst[k], abs(float(got[k][i]) - w[k]) / max(abs(w[k]), 1e-300) if w[k] != float(got[k][i]) else 0.0)
    print("[caption overlap %s] worst relative error: rouge_l %.2e, cider %.2e, sentence bleu %.2e" % (tag, worst["rouge_l"], worst["cider"], worst["bleu"]))
    for i, w in enumerate(want_items):
        assert abs(float(got["rouge_l"][i]) - w["rouge_l"]) <= ROUGE_RTOL * abs(w["rouge_l"]), (tag, i, float(got["rouge_l"][i]), w["rouge_l"])
        assert abs(float(got["bleu"][i]) - w["bleu"]) <= ROUGE_RTOL * abs(w["bleu"]), (tag, i, float(got["bleu"][i]), w["bleu"])
        if cider:
            assert abs(float(got["cider"][i]) - w["cider"]) <= CIDER_RTOL * abs(w["cider"]) + CIDER_ATOL, (tag, i, float(got["cider"][i]), w["cider"])


# ------------------------------------------------------------------------------------------------ A: seeded random rows
@functools.lru_cache(maxsize=None)
def _random_case(T, R):
    """Items for every hypothesis length of LENGTHS that fits T (and T itself): one whose first reference has the hypothesis' own
    length and shares its first half, and (R <= 2) one whose first reference has the next length of the set; further reference
    lengths are drawn from the set.  Rows past their length hold junk that must not be read as symbols (-1 and 70000)."""
    rng = np.random.RandomState(1000 * T + R)
    lens_set = sorted(set([l for l in LENGTHS if l <= T] + [T]))
    hyps, refs = [], []
    for shift in ((0, 1) if R <= 2 else (0,)):
        for i, L in enumerate(lens_set):
            hyp = rng.randint(0, 7, size=L).tolist()
            rl = [lens_set[(i + shift + r) % len(lens_set)] if r < 2 else int(rng.choice(lens_set)) for r in range(R)]
            rr = [rng.randint(0, 7, size=l).tolist() for l in rl]
            if shift == 0:
                rr[0] = hyp[:L // 2] + rr[0][L // 2:]
            hyps.append(hyp)
            refs.append(rr)
    rows = hyps + [r for rr in refs for r in rr]
    sym = np.where(rng.rand(len(rows), T) < 0.5, -1, 70000).astype(np.int64)
    lens = np.array([len(r) for r in rows], dtype=np.int32)
    for k, r in enumerate(rows):
        sym[k, :len(r)] = r
    at, ref_lists = len(hyps), []
    for rr in refs:
        ref_lists.append(list(range(at, at + len(rr))))
        at += len(rr)
    df = doc_freq(refs)
    want = [item_stats(h, rr, df, len(hyps)) for h, rr in zip(hyps, refs)]
    return sym, lens, ref_lists, df, want


@pytest.mark.parametrize("R", [1, 2, 20])
@pytest.mark.parametrize("T", [48, 128])
def test_overlap_matches_the_restatement(T, R):
    sym, lens, ref_lists, df, want = _random_case(T, R)
    n = len(want)
    got = _launch(sym, lens, np.arange(n), ref_lists, df, n)
    assert int(got["status"][0]) == 0                                           # junk past a row's length is not data
    ref_begin = np.concatenate([[0], np.cumsum([len(r) for r in ref_lists])])
    assert any(0 < w["correct"][k] < w["guess"][k] for w in want for k in range(4)) and any(0 < w["correct"][3] for w in want)
    _compare(got, want, ref_begin, "T=%d R=%d" % (T, R))
    # without the tables: the same integers and ROUGE_L, no cider
    plain = _launch(sym, lens, np.arange(n), ref_lists, bleu=False)
    assert "cider" not in plain and "bleu" not in plain
    for k in ("guess", "correct", "hyp_len", "ref_len", "lcs", "rouge_l"):
        assert np.array_equal(plain[k], got[k]), k


def test_overlap_does_not_depend_on_the_other_items():
    """An item alone gives the bits it gives among the others (fixed-order sums, no atomics on values)."""
    sym, lens, ref_lists, df, want = _random_case(128, 2)
    n = len(want)
    full = _launch(sym, lens, np.arange(n), ref_lists, df, n)
    for i in (3, n - 1):
        one = _launch(sym, lens, [i], [ref_lists[i]], df, n)
        for k in ("guess", "correct", "hyp_len", "ref_len", "rouge_l", "cider", "bleu"):
            assert np.array_equal(one[k][0], full[k][i]), (i, k)


# ------------------------------------------------------------------------------------------------ B: range, flags, shared rows
def test_largest_symbol_and_clamped_device_data():
    T = 8
    top = 65534
    rows = [[top, 0, top, 5], [top, 0, top, top], [0, top, 5], [1, 2, 3, 4, 5, 6, 7, 8]]
    sym = np.zeros((4, T), dtype=np.int64)
    for k, r in enumerate(rows):
        sym[k, :len(r)] = r
    lens = np.array([len(r) for r in rows], dtype=np.int32)
    df = doc_freq([[rows[1], rows[2]], [rows[3]]])
    want = [item_stats(rows[0], [rows[1], rows[2]], df, 2), item_stats(rows[3], [rows[3]], df, 2)]
    got = _launch(sym, lens, [0, 3], [[1, 2], [3]], df, 2)
    assert int(got["status"][0]) == 0
    _compare(got, want, [0, 2, 3], "symbol 65534")
    assert want[0]["correct"] == [4, 3, 2, 0]
    # symbols out of range are clamped to [0, 65534] and flagged; 65535 and 70000 both become 65534, -7 becomes 0
    bad = sym.copy()
    bad[0, 0], bad[1, 0], bad[0, 1] = 65535, 70000, -7
    got = _launch(bad, lens, [0, 3], [[1, 2], [3]], df, 2)
    assert int(got["status"][0]) == _lib.OVERLAP_BAD_SYM
    _compare(got, want, [0, 2, 3], "clamped symbols")
    # lengths out of range are clamped to [0, T] and flagged
    l2 = lens.copy()
    l2[3], l2[2] = T + 5, -2
    got = _launch(sym, l2, [0, 3], [[1, 2], [3]], bleu=True)
    assert int(got["status"][0]) == _lib.OVERLAP_BAD_LEN
    _compare(got, [item_stats(rows[0], [rows[1], []]), item_stats(rows[3], [rows[3]])], [0, 2, 3], "clamped lengths", cider=False)
    # row indices out of range are clamped into the table and flagged; an item without references is flagged
    got = _launch(sym, lens, [-1, 9], [[1, 2], [77]], bleu=True)
    assert int(got["status"][0]) == _lib.OVERLAP_BAD_ROW
    _compare(got, [item_stats(rows[0], [rows[1], rows[2]]), item_stats(rows[3], [rows[3]])], [0, 2, 3], "clamped rows", cider=False)
    o = ops.caption_overlap(_dev(sym, torch.int32), _dev(lens, torch.int32), _dev([0, 3], torch.int32), _dev([0, 0, 9], torch.int32),
                            _dev([1, 2, 3], torch.int32), 3)
    torch.cuda.synchronize()
    assert int(o["status"].cpu()[0]) == _lib.OVERLAP_BAD_REFS
    assert float(o["rouge_l"].cpu()[0]) == 0.0 and int(o["hyp_len"].cpu()[0]) == 4


def test_items_share_rows():
    """Reference lists that overlap, a row that is one item's hypothesis and another's reference, one row twice in a list."""
    rng = np.random.RandomState(11)
    T = 20
    rows = [rng.randint(0, 7, size=l).tolist() for l in (7, 20, 0, 13, 5, 20)]
    sym = np.zeros((6, T), dtype=np.int64)
    for k, r in enumerate(rows):
        sym[k, :len(r)] = r
    lens = np.array([len(r) for r in rows], dtype=np.int32)
    hyp_row, ref_lists = [0, 1, 3, 0], [[1, 2, 3], [3, 0, 4], [3, 3], [5]]
    lists = [[rows[r] for r in rr] for rr in ref_lists]
    df = doc_freq(lists)
    want = [item_stats(rows[h], rr, df, 4) for h, rr in zip(hyp_row, lists)]
    got = _launch(sym, lens, hyp_row, ref_lists, df, 4)
    assert int(got["status"][0]) == 0
    _compare(got, want, [0, 3, 6, 8, 9], "shared rows")
    assert want[2]["rouge_l"] == pytest.approx(1.0) and want[2]["lcs"] == [13, 13]


def test_argument_range():
    import ctypes as C
    L = _lib.lib()
    sym = torch.zeros(4, 128, dtype=torch.int32, device=DEV)
    z = lambda n: torch.zeros(n, dtype=torch.int32, device=DEV)
    length, hyp_row, ref_begin, ref_rows = z(4), z(2), torch.tensor([0, 1, 2], dtype=torch.int32, device=DEV), z(2)
    outs = [torch.full((8,), -7, dtype=torch.int32, device=DEV) for _ in range(5)]
    rouge = torch.full((2,), -7.0, dtype=torch.float64, device=DEV)
    status = z(1)
    p = lambda t: t.data_ptr()

    def rc(cider=False, **kw):
        d = _lib.CaptionOverlap()
        d.sym, d.ld, d.len, d.rows, d.T, d.items, d.n_refs = p(sym), 128, p(length), 4, 128, 2, 2
        d.hyp_row, d.ref_begin, d.ref_rows = p(hyp_row), p(ref_begin), p(ref_rows)
        d.guess, d.correct, d.hyp_len, d.ref_len, d.lcs = [p(t) for t in outs]
        d.rouge_l, d.status = p(rouge), p(status)
        if cider:
            d.cider, d.n_docs = p(rouge), 2
        for k, v in kw.items():
            setattr(d, k, v)
        r = L.univl_caption_overlap(C.byref(d), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        return r

    for kw in (dict(T=0), dict(T=129), dict(ld=127), dict(rows=0), dict(items=0), dict(n_refs=1), dict(sym=None), dict(len=None),
               dict(hyp_row=None), dict(ref_begin=None), dict(ref_rows=None), dict(guess=None), dict(lcs=None), dict(rouge_l=None),
               dict(status=None)):
        assert rc(**kw) == EINVAL, kw
        assert L.univl_last_error()
    assert rc(cider=True, n_docs=0) == EINVAL
    bad = _lib.CaptionOverlap()
    bad.df_begin[4] = 3
    assert rc(cider=True, df_begin=bad.df_begin) == EINVAL                      # entries stated, tables missing
    assert all(bool((t == -7).all()) for t in outs) and bool((rouge == -7.0).all())          # nothing was launched
    assert rc() == 0 and int(status.cpu()[0]) == 0 and outs[2][:2].tolist() == [0, 0]
    sc = torch.zeros(2, 3, dtype=torch.float64, device=DEV)
    pick = z(2)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for a in ((None, 2, 3, p(pick)), (p(sc), 0, 3, p(pick)), (p(sc), 2, 0, p(pick)), (p(sc), 2, 3, None)):
        assert L.univl_consensus_pick(*a, None, stream) == EINVAL


def test_consensus_pick_tie_rule():
    s = torch.tensor([[0.1, 0.7, 0.7, 0.2], [0.5, 0.5, 0.5, 0.5], [0.0, -1.0, float("nan"), 3.0], [float("nan"), 1.0, 1.0, 0.0]],
                     dtype=torch.float64, device=DEV)
    for n in (1, 4, 130):
        rep = s.repeat((n + 3) // 4, 1)[:n].contiguous()
        pick, best = ops.consensus_pick(rep)
        assert pick.cpu().tolist() == ([1, 0, 3, 1] * ((n + 3) // 4))[:n]
        assert best.cpu()[:1].tolist() == [0.7]


# ------------------------------------------------------------------------------------------------ C: CaptionMetrics
WORDS = "a the man woman dog is are cooking running in on kitchen park food".split()


def _sentences(n, seed, lo=0, hi=9):
    rng = np.random.RandomState(seed)
    return [" ".join(rng.choice(WORDS, size=rng.randint(lo, hi + 1))) for _ in range(n)]


def _check_metrics(got, want):
    assert tuple(got) == KEYS and math.isnan(got["METEOR"])
    print("[caption metrics] " + ", ".join("%s %.6f (%.1e)" % (k, got[k], abs(got[k] - want[k])) for k in KEYS if k != "METEOR"))
    for k in ("Bleu_1", "Bleu_2", "Bleu_3", "Bleu_4"):
        assert abs(got[k] - want[k]) <= BLEU_TOL, (k, got[k], want[k])
    assert abs(got["ROUGE_L"] - want["ROUGE_L"]) <= ROUGE_RTOL * abs(want["ROUGE_L"])
    assert abs(got["CIDEr"] - want["CIDEr"]) <= CIDER_RTOL * abs(want["CIDEr"]) + CIDER_ATOL


def test_compute_metrics_in_both_reference_layouts():
    """37 short sentences (one empty hypothesis among them).  [refs]: one reference each; MSRVTT: ref_list[r][i], three each."""
    hyps = _sentences(37, 1)
    hyps[5] = ""
    single = _sentences(37, 2, lo=1)
    cm = CaptionMetrics()
    want, _ = restate([h.split() for h in hyps], [[r.split()] for r in single])
    _check_metrics(cm.compute_metrics(ref_list=[single], hyp_list=hyps), want)
    assert cm.last["guess"].shape == (37, 4) and cm.last["lcs"].shape == (37,)
    per_item = [[single[i]] + _sentences(2, 100 + i, lo=1) for i in range(37)]
    transposed = [list(itms) for itms in zip(*per_item)]                        # main_task_caption.py:607
    assert len(transposed) == 3 and len(transposed[0]) == 37
    want3, _ = restate([h.split() for h in hyps], [[r.split() for r in rr] for rr in per_item])
    got3 = cm.compute_metrics(ref_list=transposed, hyp_list=hyps)
    _check_metrics(got3, want3)
    assert got3["Bleu_1"] >= want["Bleu_1"]                                     # more references never lower a clipped count
    # compute_ids is the same computation on integer rows
    ids = {w: k for k, w in enumerate(WORDS)}
    enc = lambda s: [ids[w] for w in s.split()]
    got_ids = cm.compute_ids([enc(h) for h in hyps], [[enc(r) for r in rr] for rr in per_item])
    for k in KEYS:
        assert k == "METEOR" or abs(got_ids[k] - got3[k]) <= 1e-12


def test_shim_stub_returns_the_metrics():
    """run_univl_amd.install_compat's nlgeval stub end to end: NLGEval(<its keywords>).compute_metrics(ref_list=, hyp_list=) in both
    reference layouts returns the seven keys, equal to CaptionMetrics' own and to the restatement's; a caption of more than 128
    words is cut with a warning instead of costing the epoch.  What the shim installed is taken out again."""
    import sys
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
        hyps = _sentences(37, 7)
        single = _sentences(37, 8, lo=1)
        per_item = [[single[i]] + _sentences(2, 300 + i, lo=1) for i in range(37)]
        transposed = [list(itms) for itms in zip(*per_item)]
        for ref_list, lists in (([single], [[r] for r in single]), (transposed, per_item)):
            got = obj.compute_metrics(ref_list=ref_list, hyp_list=hyps)
            want, _ = restate([h.split() for h in hyps], [[r.split() for r in rr] for rr in lists])
            _check_metrics(got, want)
            assert got["Bleu_1"] > 0.0 and got["CIDEr"] > 0.0
            own = CaptionMetrics().compute_metrics(ref_list=ref_list, hyp_list=hyps)
            for k in KEYS:
                assert k == "METEOR" or got[k] == own[k], k
        long_hyps = [hyps[0], " ".join(WORDS[i % len(WORDS)] for i in range(150))]
        long_refs = [[single[0], " ".join(WORDS[(3 * i) % len(WORDS)] for i in range(140))]]
        with pytest.warns(UserWarning, match="2 of 4 rows"):
            got = obj.compute_metrics(ref_list=long_refs, hyp_list=long_hyps)
        want, _ = restate([h.split()[:128] for h in long_hyps], [[r.split()[:128]] for r in long_refs[0]])
        _check_metrics(got, want)
        with pytest.raises(ValueError, match="128"):
            CaptionMetrics().compute_metrics(ref_list=long_refs, hyp_list=long_hyps)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
        for k, had in np_had.items():
            if not had and k in np.__dict__:
                delattr(np, k)


# ------------------------------------------------------------------------------------------------ D: eval_caption
def test_eval_caption_with_caption_metrics(tmp_path):
    import test_caption_eval_gpu as E
    from univl_amd.eval import eval_caption
    cfg, model, _, _ = E._toy(torch.float32)
    loader = E._loader(cfg, [16, 16, 5], seed=77)
    tk = E.SynthTokenizer(cfg.vocab_size, special={"[CLS]": E.BOS})
    res = eval_caption(model, loader, tk, n_bm=E.N_BM, max_len=E.T_DEC, nlg_eval=CaptionMetrics())
    assert len(res.hyps) == 37 and tuple(res.metrics) == KEYS
    assert float(res) == res.metrics["Bleu_4"]
    again = CaptionMetrics().compute_metrics(ref_list=[res.refs], hyp_list=res.hyps)
    for k in KEYS:
        assert k == "METEOR" or res.metrics[k] == again[k]
    want, _ = restate([h.split() for h in res.hyps], [[r.split()] for r in res.refs])
    _check_metrics(res.metrics, want)


# ------------------------------------------------------------------------------------------------ E: consensus
def _consensus_expect(cap, cap_len, metric):
    """cap [n, ns, T], cap_len [n, ns] host lists -> ([n][ns] restated scores)."""
    out = []
    for rows, lens in zip(cap, cap_len):
        cut = [r[:l] for r, l in zip(rows, lens)]
        out.append([item_stats(c, [o for j, o in enumerate(cut) if j != s])["bleu" if metric == "bleu" else "rouge_l"]
                    for s, c in enumerate(cut)])
    return out


def _check_consensus(res, eos, pad, metric):
    idx, score = consensus(res, eos, pad, metric=metric)
    assert idx.is_cuda and score.is_cuda and idx.dtype == torch.int32 and score.dtype == torch.float64
    cap, cap_len = res.captions(eos, pad)
    want = _consensus_expect(cap.cpu().tolist(), cap_len.cpu().tolist(), metric)
    idx, score = idx.cpu().tolist(), score.cpu().tolist()
    for i, w in enumerate(want):
        best = max(w)
        assert abs(score[i] - best) <= ROUGE_RTOL * abs(best), (i, score[i], w)
        near = [k for k, v in enumerate(w) if abs(v - best) <= ROUGE_RTOL * abs(best)]
        assert idx[i] in near, (i, idx[i], w)
        if all(v == best for v in (w[k] for k in near)):                        # exact ties in the restatement: the lower index
            assert idx[i] == near[0], (i, idx[i], w)
    return idx, want


def test_consensus_on_sampled_captions(monkeypatch):
    """4 instances x 5 samples of the toy sampler: the pick equals the restatement's, and sample() + consensus() read nothing on the
    host (the check of tests/test_sample_gpu.py part G)."""
    import test_sample_gpu as G
    from univl_amd.sample import SampleResult
    feats = G._toy(torch.bfloat16)[2]
    enc = tuple(torch.cat([a, b[:1]]) for a, b in zip(feats[0], feats[1]))
    smp = G._new_sampler(torch.bfloat16, 4, n_samp=5)
    eos = G._eos_for(smp, enc, 21)
    res = smp.sample(*enc, bos=G.BOS, eos=eos, seed=21)
    assert res.tokens.shape[:2] == (4, 5)
    for metric in ("rouge_l", "bleu"):
        _check_consensus(res, eos, -1, metric)
    # duplicates: samples 1 and 3 identical and best -> 1; all five identical -> 0
    tok = torch.tensor([[[5, 6, 7, 8], [5, 6, 9, 8], [1, 2, 3, 4], [5, 6, 9, 8], [5, 9, 8, 2]],
                        [[3, 3, 4, 4]] * 5], dtype=torch.int32, device=DEV)
    z = torch.zeros(2, 5, 4, device=DEV)
    dup = SampleResult(tok, z, z, z[..., 0], z[..., 0], torch.full((2, 5), 4, dtype=torch.int32, device=DEV))
    for metric in ("rouge_l", "bleu"):
        idx, want = _check_consensus(dup, -1, -1, metric)
        assert idx == [1, 0] and want[0][1] == want[0][3] == max(want[0])
    with pytest.raises(ValueError):
        consensus(dup, -1, -1, metric="meteor")
    # no host involvement between sample() and the returned tensors
    torch.cuda.synchronize()
    probe = torch.ones(1, device=DEV)
    prev = torch.cuda.get_sync_debug_mode()
    reads = G._HostReads(monkeypatch)
    try:
        torch.cuda.set_sync_debug_mode("error")
        r2 = smp.sample(*enc, bos=G.BOS, eos=-1, seed=2, sync_every=0)
        idx, score = consensus(r2, -1, -1)
        n_reads = list(reads.calls)
        try:
            probe.item()
            reports = False
        except RuntimeError:
            reports = True
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    print("[sync debug mode] reports synchronising calls on this build: %s; host reads counted: %s" % (reports, n_reads))
    assert n_reads == []
    torch.cuda.synchronize()
    assert idx.shape == (4,) and score.shape == (4,) and bool(((idx >= 0) & (idx < 5)).all())
