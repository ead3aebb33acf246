"""Caption evaluation end to end: the device-side cut (csrc/beam.hip: univl_beam_captions), partial batches in a compiled decoding
session (CaptionBeamSearch n_active) and the dataset loop (univl_amd.eval.eval_caption).

Every comparison is against code that existed before these: CaptionBeamSearch.__call__ / decode() on FULL batches, hypotheses(),
and the Python restatement of the reference's lines in tests/test_caption_eval_cpu.py.

A  the cut kernel against the Python cut of the same host-copied hypotheses, exactly; argument range;
B  idle slots: inert (two kinds of stale contents), partial == full, a fresh session whose first call is partial;
C  eval_caption over a loader of 16 + 16 + 5 items against full-batch sessions;
D  no host involvement in decode(n_active=...) + captions();  E  stage-one model."""
import ctypes as C
import functools

import pytest
import torch

import univl_oracle as O
from make_golden import case_config
from test_caption_eval_cpu import SynthTokenizer, reference_text

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from univl_amd import _lib, ops
    from univl_amd.decode import CaptionBeamSearch
    from univl_amd.eval import eval_caption, ids_to_caption
    from test_model_gpu import build

DEV = "cuda"
EINVAL = -1


@pytest.fixture(autouse=True)
def _deterministic_mode():
    """Fixed-order sums in the decoder's products (as tests/test_beam_gpu.py): B and C compare separate runs bit for bit, which
    split-K sums met in hardware order would not allow.  The cut kernel has no sums."""
    import univl_amd
    was = univl_amd.deterministic()
    univl_amd.set_deterministic(True)
    yield
    univl_amd.set_deterministic(was)


# ------------------------------------------------------------------------------------------------ A: the cut kernel
def python_cut(row, length, Tmax, eos, pad):
    """The reference's two successive cuts (main_task_caption.py:555-560) on token ids: the first length tokens of the row, cut at
    the first eos, then at the first pad; a negative id never matches.  Returns (row of Tmax entries, -1 past the cut; cut length)."""
    toks = list(row[:max(0, min(int(length), Tmax))])
    if eos >= 0 and eos in toks:
        toks = toks[:toks.index(eos)]
    if pad >= 0 and pad in toks:
        toks = toks[:toks.index(pad)]
    return toks + [-1] * (Tmax - len(toks)), len(toks)


def _expect(hyp, length, eos, pad):
    n, nb, Tmax = hyp.shape
    rows, lens = [], []
    for i in range(n):
        for k in range(nb):
            r, l = python_cut(hyp[i, k].tolist(), int(length[i]), Tmax, eos, pad)
            rows.append(r)
            lens.append(l)
    return torch.tensor(rows, dtype=torch.int32).view(n, nb, Tmax), torch.tensor(lens, dtype=torch.int32).view(n, nb)


def _check_cut(hyp, length, eos, pad):
    """hyp / length: host tensors.  All four call forms against the Python cut."""
    want, want_len = _expect(hyp, length, eos, pad)
    d_hyp, d_len = hyp.to(DEV), length.to(DEV)
    cap, cap_len = ops.beam_captions(d_hyp, d_len, eos, pad)
    assert torch.equal(cap.cpu(), want) and torch.equal(cap_len.cpu(), want_len)
    assert torch.equal(d_hyp.cpu(), hyp)                                        # the input is read only
    # the end token as a device word (the eos argument is then not read)
    word = torch.tensor([eos], dtype=torch.int32, device=DEV)
    cap, cap_len = ops.beam_captions(d_hyp, d_len, 12345 if eos != 12345 else 1, pad, eos_dev=word)
    assert torch.equal(cap.cpu(), want) and torch.equal(cap_len.cpu(), want_len)
    # in place
    buf = d_hyp.clone()
    cap, cap_len = ops.beam_captions(buf, d_len, eos, pad, out=buf)
    assert cap.data_ptr() == buf.data_ptr()
    assert torch.equal(buf.cpu(), want) and torch.equal(cap_len.cpu(), want_len)
    # neither token: the rows up to the clamped length
    want, want_len = _expect(hyp, length, -1, -1)
    cap, cap_len = ops.beam_captions(d_hyp, d_len, -1, -1)
    assert torch.equal(cap.cpu(), want) and torch.equal(cap_len.cpu(), want_len)
    assert want_len.tolist() == [[max(0, min(int(l), hyp.shape[2]))] * hyp.shape[1] for l in length.tolist()]


@pytest.mark.parametrize("Tmax", [1, 5, 32, 64, 65, 128])
@pytest.mark.parametrize("nb", [1, 5, 8])
@pytest.mark.parametrize("n", [1, 3, 16, 67])
def test_beam_captions_matches_python_cut(n, nb, Tmax):
    """Random rows over a small alphabet, so that the end and pad tokens are frequent and fall on every lane; lengths cover 0, Tmax
    and values past Tmax (clamped); tokens at and past an instance's length are junk that holds both tokens (must be ignored)."""
    g = torch.Generator().manual_seed(10000 * n + 100 * nb + Tmax)
    eos, pad = 7, 3
    for alphabet in (12, 4 * Tmax + 12):                                        # dense hits; hits about once per row
        hyp = torch.randint(0, alphabet, (n, nb, Tmax), generator=g, dtype=torch.int32)
        length = torch.randint(0, Tmax + 1, (n,), generator=g, dtype=torch.int32)
        length[0] = Tmax
        if n > 1:
            length[1] = 0
            length[n - 1] = Tmax + 5
        if n > 3:
            length[2] = -2
            length[3] = Tmax
            hyp[3] = 9                                                          # both absent on full-length rows
        _check_cut(hyp, length, eos, pad)


@pytest.mark.parametrize("Tmax", [8, 64, 70, 128])
def test_beam_captions_crafted_rows(Tmax):
    """One instance per case, n_best = 2 (row 1 is row 0 reversed in its first `length` tokens, so every case is also seen from
    the other end)."""
    eos, pad, L = 7, 3, Tmax - 2
    base = [9] * Tmax
    put = lambda at: [eos if j in at.get("eos", ()) else pad if j in at.get("pad", ()) else 9 for j in range(Tmax)]
    cases = [(put(dict(eos=[0])), L), (put(dict(eos=[L - 1])), L), (put(dict(eos=[L])), L), (put(dict(eos=[L, Tmax - 1], pad=[L + 1])), L),
             (put(dict(pad=[2], eos=[4])), L), (put(dict(eos=[2], pad=[4])), L), (put(dict(pad=[0])), L), (put(dict(pad=[L - 1])), L),
             (base, L), (base, 0), (base, Tmax), (base, Tmax + 9), (put(dict(eos=[Tmax - 1])), Tmax + 9), (put(dict(eos=[0])), 0),
             (put(dict(eos=[1, 3, 5], pad=[2, 4])), L), (put(dict(eos=[min(63, L - 1)])), L), (put(dict(eos=[min(64, L - 1)])), L),
             (put(dict(pad=[min(65, L - 1)], eos=[min(66, L - 1) + 1])), Tmax)]
    hyp = torch.zeros(len(cases), 2, Tmax, dtype=torch.int32)
    length = torch.zeros(len(cases), dtype=torch.int32)
    for i, (row, ln) in enumerate(cases):
        c = max(0, min(ln, Tmax))
        hyp[i, 0] = torch.tensor(row, dtype=torch.int32)
        hyp[i, 1] = torch.tensor(row[:c][::-1] + row[c:], dtype=torch.int32)
        length[i] = ln
    want, want_len = _expect(hyp, length, eos, pad)
    assert want_len[:4, 0].tolist() == [0, L - 1, L, L] and want_len[4:6, 0].tolist() == [2, 2]      # the cases are what they say
    _check_cut(hyp, length, eos, pad)
    _check_cut(hyp, length, eos, -1)
    _check_cut(hyp, length, -1, pad)


def test_beam_captions_argument_range():
    """Outside 1 <= n_best <= 8, n_inst >= 1, Tmax >= 1, or with a null pointer: UNIVL_EINVAL and nothing launched."""
    n, nb, Tmax = 3, 5, 16
    hyp = torch.zeros(n, nb, Tmax, dtype=torch.int32, device=DEV)
    length = torch.zeros(n, dtype=torch.int32, device=DEV)
    cap, cap_len = torch.full_like(hyp, -7), torch.full((n, nb), -7, dtype=torch.int32, device=DEV)
    L = _lib.lib()
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())

    def rc(hyp_=hyp, length_=length, n_=n, nb_=nb, T_=Tmax, cap_=cap, len_=cap_len):
        r = L.univl_beam_captions(p(hyp_), p(length_), n_, nb_, T_, 7, 3, None, p(cap_), p(len_),
                                  C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        return r

    for kw in (dict(nb_=0), dict(nb_=9), dict(nb_=-1), dict(T_=0), dict(T_=-4), dict(n_=0), dict(n_=-1), dict(hyp_=None),
               dict(length_=None), dict(cap_=None), dict(len_=None)):
        assert rc(**kw) == EINVAL, kw
        assert L.univl_last_error()
    assert bool((cap == -7).all()) and bool((cap_len == -7).all())              # nothing was launched
    assert rc() == 0
    assert bool((cap == -1).all()) and bool((cap_len == 0).all())


# ------------------------------------------------------------------------------------------------ B: idle slots
N_SLOTS, N_REAL, N_BM, T_DEC, BOS = 16, 6, 5, 8, 101


@functools.lru_cache(maxsize=None)
def _toy(dtype):
    """The caption_small toy model of tests/test_decode_gpu.py, three full batches of encoder features (seeds differ), and an end
    token that the top beam of instance 0 of batch 0 emits at its second step, so that lengths differ between instances."""
    cfg, _, dseed = case_config("caption_small")
    model, _ = build(cfg, dtype)
    model.eval()
    feats = []
    for k in range(3):
        d = {key: v.to(DEV) for key, v in O.synthetic_batch(cfg, N_SLOTS, seed=dseed + 11 + k).items()}
        with torch.no_grad():
            so, vo = model.get_sequence_visual_output(d["input_ids"], d["token_type_ids"], d["attention_mask"], d["video"], d["video_mask"])
        feats.append((so, vo, d["attention_mask"].view(N_SLOTS, -1), d["video_mask"].view(N_SLOTS, -1)))
    probe = _new_session(model, cfg)
    short, _ = probe(*feats[0], bos=BOS, eos=-1, max_len=2)
    return cfg, model, feats, int(short[0][1])


def _new_session(model, cfg, n=N_SLOTS):
    return CaptionBeamSearch(model, n, cfg.max_words, cfg.max_frames, n_bm=N_BM, max_len=T_DEC, use_graphs=True)


FIELDS = ("tokens", "scores", "lengths", "parents", "step_tokens", "step_scores")


def _same(a, b, rows=None):
    for f in FIELDS:
        x, y = getattr(a, f), getattr(b, f)
        if rows is not None:
            y = y[:, :rows] if f in FIELDS[3:] else y[:rows]
        assert x.shape == y.shape and torch.equal(x, y), f


def _head(enc, m):
    return tuple(t[:m] for t in enc)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_idle_slots_are_inert(dtype):
    """decode(n_active=6) of the same 6 instances after two different full batches went through the session: every field of the
    two results is bitwise equal.  n_best = 3, so hypotheses below the best are covered too."""
    cfg, model, feats, eos = _toy(dtype)
    bs = _new_session(model, cfg)
    six = _head(feats[0], N_REAL)
    res = []
    for stale in (feats[1], feats[2]):
        full = bs.decode(*stale, bos=BOS, eos=eos, n_best=3)
        assert full.tokens.shape[0] == N_SLOTS
        res.append(bs.decode(*six, bos=BOS, eos=eos, n_best=3, n_active=N_REAL))
    assert res[0].tokens.shape == (N_REAL, 3, T_DEC) and res[0].scores.shape == (N_REAL, 3) and res[0].lengths.shape == (N_REAL,)
    assert res[0].parents.shape == (T_DEC, N_REAL, N_BM)
    _same(res[0], res[1])
    assert len({int(l) for l in res[0].lengths.tolist()}) > 1 or eos < 0        # the end token did stop some instance early
    assert len([k for k in bs.steps if k[1]]) == T_DEC                          # one plan per position, whatever the batch size


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_partial_batch_equals_full_batch(dtype):
    """decode(n_active=6) against the first 6 instances of a full decode() whose other 10 instances are another batch's: bitwise.
    Rows are independent and the launch shapes identical, so any difference is a bug, not rounding.  __call__ likewise."""
    cfg, model, feats, eos = _toy(dtype)
    bs = _new_session(model, cfg)
    mixed = tuple(torch.cat([a[:N_REAL], b[N_REAL:]]) for a, b in zip(feats[0], feats[1]))
    for e in (eos, -1):
        full = bs.decode(*mixed, bos=BOS, eos=e, n_best=N_BM)
        part = bs.decode(*_head(feats[0], N_REAL), bos=BOS, eos=e, n_best=N_BM, n_active=N_REAL)
        _same(part, full, rows=N_REAL)
        hyp_f, sc_f = bs(*mixed, bos=BOS, eos=e)
        hyp_p, sc_p = bs(*_head(feats[0], N_REAL), bos=BOS, eos=e, n_active=N_REAL)
        assert hyp_p == hyp_f[:N_REAL] and torch.equal(sc_p, sc_f[:N_REAL])
        assert part.hypotheses() == full.hypotheses()[:N_REAL]
    # n_active = n_inst and None are the same call
    _same(bs.decode(*feats[0], bos=BOS, eos=eos, n_active=N_SLOTS), bs.decode(*feats[0], bos=BOS, eos=eos))
    for bad in (0, -1, N_SLOTS + 1):
        with pytest.raises(ValueError):
            bs.decode(*_head(feats[0], N_REAL), bos=BOS, eos=eos, n_active=bad)
    with pytest.raises(ValueError):
        bs.decode(*feats[0], bos=BOS, eos=eos, n_active=N_REAL)                 # 16 rows of features for 6 instances


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_idle_slots_from_the_start(dtype):
    """A fresh session whose FIRST call is partial: 6 instances come back, everything finite, and equal to the full-batch result of
    another session (the idle slots hold the zeros of construction here)."""
    cfg, model, feats, eos = _toy(dtype)
    bs = _new_session(model, cfg)
    r = bs.decode(*_head(feats[0], N_REAL), bos=BOS, eos=eos, n_best=N_BM, n_active=N_REAL)
    assert r.tokens.shape == (N_REAL, N_BM, T_DEC) and r.scores.shape == (N_REAL, N_BM) and r.lengths.shape == (N_REAL,)
    assert r.parents.shape == r.step_tokens.shape == r.step_scores.shape == (T_DEC, N_REAL, N_BM)
    assert bool(torch.isfinite(r.scores).all()) and bool(torch.isfinite(r.step_scores).all())
    assert bool(torch.isfinite(bs.head.logits[:N_REAL * N_BM, :bs.V]).all())
    lens = r.lengths.tolist()
    assert all(1 <= l <= T_DEC for l in lens)
    tok = r.tokens.cpu()
    for i, l in enumerate(lens):
        assert bool(((tok[i, :, :l] >= 0) & (tok[i, :, :l] < bs.V)).all()) and bool((tok[i, :, l:] == -1).all())
    assert bool((r.scores[:, 1:] <= r.scores[:, :-1]).all())
    other = _new_session(model, cfg)
    _same(r, other.decode(*feats[0], bos=BOS, eos=eos, n_best=N_BM), rows=N_REAL)
    # captions(): the device cut of these hypotheses against the Python cut of hypotheses()
    pad = int(tok[1, 0, 1])                                                     # a token instance 1's best hypothesis holds
    cap, cap_len = r.captions(eos, pad)
    assert cap.is_cuda and cap_len.is_cuda and cap.shape == (N_REAL, N_BM, T_DEC) and cap_len.shape == (N_REAL, N_BM)
    hyps, cap, cap_len = r.hypotheses(), cap.cpu(), cap_len.cpu()
    for i in range(N_REAL):
        for k in range(N_BM):
            row, l = python_cut(hyps[i][k], len(hyps[i][k]), T_DEC, eos, pad)
            assert cap[i, k].tolist() == row and int(cap_len[i, k]) == l
    assert int(cap_len[1, 0]) <= 1
    assert torch.equal(r.tokens.cpu(), tok)                                     # captions() leaves the result as it was


# ------------------------------------------------------------------------------------------------ C: the dataset loop
LOADER_ORDER = ("input_ids", "attention_mask", "token_type_ids", "video", "video_mask", "pairs_masked_text", "pairs_token_labels",
                "masked_video", "video_labels_index", "input_caption_ids", "decoder_mask", "output_caption_ids")


def _loader(cfg, sizes, seed):
    """Host 12-tuples in the reference loader's order (main_task_caption.py:504-506)."""
    b = O.synthetic_batch(cfg, sum(sizes), seed=seed)
    out, at = [], 0
    for s in sizes:
        out.append(tuple(b[k][at:at + s] for k in LOADER_ORDER))
        at += s
    return out


class _Metric:
    def compute_metrics(self, ref_list, hyp_list):
        self.seen = (ref_list, hyp_list)
        return {"Bleu_4": 0.25, "n": len(hyp_list)}


def test_eval_caption_over_a_loader(tmp_path, monkeypatch):
    """16 + 16 + 5 items.  The reference point is built here from code that predates eval_caption: a second session's __call__ on
    FULL batches, the 5-item tail filled up with the features of 11 items of the first batch, and ids_to_caption's restatement.
    (The tail is filled at the level of the encoder FEATURES: the encoders pick their launch shapes by batch size, so features
    of the same item computed in a 5-item and in a 16-item batch need not agree bit for bit, and that is not what is tested.)"""
    cfg, model, _, _ = _toy(torch.float32)
    sizes = [16, 16, 5]
    loader = _loader(cfg, sizes, seed=77)
    ref_bs = _new_session(model, cfg)
    # "[SEP]" is the token the top beam of the loader's first item emits at its second step: that item stops there
    d = [t.to(DEV) for t in loader[0]]
    with torch.no_grad():
        so, vo = model.get_sequence_visual_output(d[0], d[2], d[1], d[3], d[4])
    short, _ = ref_bs(so, vo, d[1].view(16, -1), d[4].view(16, -1), bos=BOS, eos=-1, max_len=2)
    eos = int(short[0][1])
    tk = SynthTokenizer(cfg.vocab_size, special={"[SEP]": eos, "[CLS]": BOS})
    built = []
    orig_init = CaptionBeamSearch.__init__

    def counting_init(self, *a, **kw):
        built.append(self)
        orig_init(self, *a, **kw)
    monkeypatch.setattr(CaptionBeamSearch, "__init__", counting_init)
    model.train()
    metric = _Metric()
    res = eval_caption(model, loader, tk, n_bm=N_BM, n_best=3, max_len=T_DEC, output_dir=str(tmp_path), nlg_eval=metric)
    assert model.training                                                       # restored
    model.eval()
    assert len(built) == 1 and res.session is built[0] and res.session.n_inst == 16
    assert len([k for k in res.session.steps if k[1]]) <= T_DEC                 # one set of plans: the tail captured nothing new
    monkeypatch.setattr(CaptionBeamSearch, "__init__", orig_init)
    # ---- the reference point
    want_hyps, want_refs, first = [], [], None
    for batch in loader:
        d = [t.to(DEV) for t in batch]
        with torch.no_grad():
            so, vo = model.get_sequence_visual_output(d[0], d[2], d[1], d[3], d[4])
        enc = (so, vo, d[1].view(so.shape[0], -1), d[4].view(so.shape[0], -1))
        n = so.shape[0]
        if first is None:
            first = enc
        if n < 16:
            enc = tuple(torch.cat([a, b[:16 - n]]) for a, b in zip(enc, first))
        hyp, _ = ref_bs(*enc, bos=BOS, eos=eos)
        want_hyps += [reference_text(tk, h) for h in hyp[:n]]
        want_refs += [reference_text(tk, row) for row in batch[11].view(-1, batch[11].shape[-1]).tolist()]
    assert len(res.hyps) == len(res.refs) == 37
    assert res.hyps == want_hyps
    assert res.refs == want_refs
    assert (tmp_path / "hyp.txt").read_text(encoding="utf-8") == "".join(h + "\n" for h in want_hyps)
    assert (tmp_path / "ref.txt").read_text(encoding="utf-8") == "".join(r + "\n" for r in want_refs)
    assert res.metrics == {"Bleu_4": 0.25, "n": 37} and float(res) == 0.25
    assert metric.seen[0] == [want_refs] and metric.seen[1] == want_hyps
    # ---- n_best = 3
    assert res.scores.shape == (37, 3) and res.lengths.shape == (37,) and len(res.hyp_ids) == 37
    assert bool((res.scores[:, 1:] <= res.scores[:, :-1]).all()) and bool(torch.isfinite(res.scores).all())
    for i in range(37):
        assert len(res.hyp_ids[i]) == 3
        assert ids_to_caption(tk, res.hyp_ids[i][0]) == res.hyps[i]
        for ids in res.hyp_ids[i]:
            assert eos not in ids and tk.vocab["[PAD]"] not in ids and len(ids) <= int(res.lengths[i])
    assert any(len(res.hyp_ids[i][0]) < int(res.lengths[i]) for i in range(37))       # the cut did cut something
    # ---- session=: reused, not rebuilt; a larger batch is refused with both sizes named
    again = eval_caption(model, loader[2:], tk, n_best=1, max_len=T_DEC, session=res.session)
    assert again.session is res.session and again.hyps == want_hyps[32:] and again.metrics is None and float(again) == 0.0
    small = _new_session(model, cfg, n=4)
    with pytest.raises(ValueError, match=r"16.*4|4.*16"):
        eval_caption(model, loader[:1], tk, max_len=T_DEC, session=small)


# ------------------------------------------------------------------------------------------------ D: no new host traffic
class _HostReads:
    """Counts Tensor.item / __bool__ / cpu / tolist calls on device tensors (as tests/test_beam_gpu.py)."""

    def __init__(self, monkeypatch):
        self.calls = []
        for name in ("item", "__bool__", "cpu", "tolist"):
            orig = getattr(torch.Tensor, name)

            def wrapped(t, *a, _orig=orig, _name=name, **kw):
                if t.is_cuda:
                    self.calls.append(_name)
                return _orig(t, *a, **kw)
            monkeypatch.setattr(torch.Tensor, name, wrapped)


def test_partial_decode_and_captions_have_no_host_involvement(monkeypatch):
    """After one warm-up call (graph capture), decode(n_active=6, sync_every=0) followed by captions() runs under
    torch.cuda.set_sync_debug_mode("error") without raising and without one Tensor.item / __bool__ / cpu / tolist on a device
    tensor."""
    cfg, model, feats, eos = _toy(torch.bfloat16)
    bs = _new_session(model, cfg)
    six = _head(feats[0], N_REAL)
    bs.decode(*six, bos=BOS, eos=eos, sync_every=0, n_active=N_REAL).captions(eos, 0)
    torch.cuda.synchronize()
    probe = torch.ones(1, device=DEV)
    prev = torch.cuda.get_sync_debug_mode()
    reads = _HostReads(monkeypatch)
    try:
        torch.cuda.set_sync_debug_mode("error")
        res = bs.decode(*six, bos=BOS, eos=eos, sync_every=0, n_best=3, n_active=N_REAL)
        cap, cap_len = res.captions(eos, 0)
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
    assert cap.shape == (N_REAL, 3, T_DEC) and cap_len.shape == (N_REAL, 3)


# ------------------------------------------------------------------------------------------------ E: stage one
def test_eval_caption_stage_one_model_returns_early(monkeypatch):
    cfg = O.OracleConfig(batch_size=2, text_num_hidden_layers=1, visual_num_hidden_layers=1, max_words=16, max_frames=16)
    model, _ = build(cfg, torch.bfloat16)
    assert model._stage_one and model.decoder is None

    def boom(*a, **kw):
        raise AssertionError("eval_caption of a stage-one model reached the encoders / the decoder")
    monkeypatch.setattr(model, "get_sequence_visual_output", boom)
    monkeypatch.setattr(CaptionBeamSearch, "__init__", boom)
    model.train()
    res = eval_caption(model, _loader(cfg, [2], seed=3), SynthTokenizer(cfg.vocab_size))
    assert float(res) == 0.0 and res.hyps == [] and res.refs == [] and res.metrics is None and res.session is None
    assert model.training
