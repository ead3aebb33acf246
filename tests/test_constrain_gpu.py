"""Decoding constraints on the device (csrc/constrain.hip: univl_decode_constrain) and the sessions that carry them
(CaptionBeamSearch / CaptionSampler / eval_caption with constraints=).

A  the kernel against tests/constrain_ref.py BIT FOR BIT: the whole [R, ld] array (padding columns included) and prefix_out;
B  further kernel cases: the min_len boundary, eos forms, params_dev rewritten between two runs of one descriptor, suppress lists,
   the sampler form, every argument-range error;
C  whole decoding runs on the small caption case: constraints=None changes nothing; device == host == a reference loop written here
   (an UNCONSTRAINED session's step_logprobs + constrain_ref + a numpy Beam.advance); the properties of the output, after showing
   that the unconstrained output violates them; set_constraints without a new capture; partial batches; the sampler; eval_caption."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import univl_oracle as O
from make_golden import case_config
from constrain_ref import advance_prefix, constrain_ref
from test_caption_eval_cpu import SynthTokenizer

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from univl_amd import _lib, ops
    from univl_amd.constrain import DecodeConstraints
    from univl_amd.decode import CaptionBeamSearch
    from univl_amd.eval import eval_caption
    from univl_amd.sample import CaptionSampler
    from test_model_gpu import build

DEV = "cuda"
EINVAL = -1
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(autouse=True)
def _deterministic_mode():
    """Fixed-order sums in the decoder's products (as tests/test_beam_gpu.py): C compares separate sessions bit for bit.  The
    constraint kernel has no sums at all."""
    import univl_amd
    was = univl_amd.deterministic()
    univl_amd.set_deterministic(True)
    yield
    univl_amd.set_deterministic(was)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ A: the kernel against the reference
def _case(R, nb, V, ld, Tmax, seed, alphabet):
    """Host inputs of one call: finite random rows with a few -inf already there and a marker in the padding columns; prefixes over
    a small alphabet (dense matches); a non-identity src in which rows 0 and 1 share a parent; one done instance in the middle."""
    rng = np.random.RandomState(seed)
    x = rng.standard_normal((R, ld)).astype(np.float32)
    x[:, V:] = np.float32(3e38)
    for r in range(R):
        x[r, rng.randint(0, V, size=2)] = -np.inf
    pin = rng.choice(alphabet, size=(R, Tmax)).astype(np.int32)
    last = rng.choice(alphabet, size=R).astype(np.int64)
    src = rng.permutation(R).astype(np.int32)
    if R > 1:
        src[0] = src[1]
    n_inst = R // nb
    done = np.zeros(n_inst, dtype=np.uint8)
    if n_inst > 1:
        done[n_inst // 2] = 1
    return x, pin, last, src, done


def _run_beam_form(x, V, t, pin, last, src, done, nb, **kw):
    """One call in the beam form; returns (x after, prefix_out after) as numpy, prefix_out pre-filled with -7."""
    xd = torch.from_numpy(x).to(DEV)
    pind, pout = torch.from_numpy(pin).to(DEV), torch.full(pin.shape, -7, dtype=torch.int32, device=DEV)
    ops.decode_constrain(xd, V, t, prefix_in=pind, prefix_out=pout, src=None if src is None else torch.from_numpy(src).to(DEV),
                         last=torch.from_numpy(last).to(DEV), done=None if done is None else torch.from_numpy(done).to(DEV),
                         done_stride=nb, **kw)
    torch.cuda.synchronize()
    assert torch.equal(pind.cpu(), torch.from_numpy(pin))                 # prefix_in is read only
    return xd.cpu().numpy(), pout.cpu().numpy()


def _expect_beam_form(x, V, t, pin, last, src, done, nb, ngram, min_len, eos, suppress):
    pout = advance_prefix(pin, src, last, t, before=np.full(pin.shape, -7, dtype=np.int32))
    return constrain_ref(x, V, pout, t, done, ngram, min_len, eos, suppress, done_stride=nb), pout


@pytest.mark.parametrize("V,ld", [(7, 8), (64, 64), (30522, 30528)])
@pytest.mark.parametrize("R,nb", [(1, 1), (3, 1), (10, 5)])
def test_kernel_matches_reference(R, nb, V, ld):
    """A.  Tmax = 12, t in {0, 1, 2, 3, 4, 11}, every order 0 .. 4, with a min_len, an end token and a suppress list riding along.
    Everything is compared as bits; columns V .. ld-1 must keep their marker."""
    alphabet = [1, 4, V - 1]
    sup = torch.tensor([0, 4, 0], dtype=torch.int32, device=DEV)
    for t in (0, 1, 2, 3, 4, 11):
        for ngram in range(5):
            x, pin, last, src, done = _case(R, nb, V, ld, 12, 1000 * t + ngram, alphabet)
            got_x, got_p = _run_beam_form(x, V, t, pin, last, src, done, nb, ngram=ngram, min_len=3, eos=2, suppress=sup)
            want_x, want_p = _expect_beam_form(x, V, t, pin, last, src, done, nb, ngram, 3, 2, [0, 4, 0])
            assert np.array_equal(got_p, want_p), (t, ngram)
            assert np.array_equal(_bits(got_x), _bits(want_x)), (t, ngram, np.argwhere(_bits(got_x) != _bits(want_x))[:4])
            live = [r for r in range(R) if not done[r // nb]]
            assert not live or t >= 3 or bool((got_x[live, 2] == -np.inf).all())          # the case is not vacuous
            assert np.array_equal(_bits(got_x[:, V:]), _bits(x[:, V:]))


def test_kernel_prefix_longer_than_a_wave():
    """Tmax = 80, t = 79: a lane handles more than one prefix position.  Two symbols, so that almost every position matches."""
    R, nb, V, ld, t = 3, 1, 64, 64, 79
    for ngram in (1, 2, 3, 4):
        x, pin, last, src, done = _case(R, nb, V, ld, 80, 77 + ngram, [5, 9])
        pin[:, 70:] = [[5, 9, 9, 5, 60, 61, 5, 9, 9, 5]]                   # tokens seen only past lane 63's first position
        got_x, got_p = _run_beam_form(x, V, t, pin, last, src, done, nb, ngram=ngram)
        want_x, want_p = _expect_beam_form(x, V, t, pin, last, src, done, nb, ngram, 0, -1, [])
        assert np.array_equal(got_p, want_p) and np.array_equal(_bits(got_x), _bits(want_x)), ngram
    x, pin, last, src, done = _case(R, nb, V, ld, 80, 5, [5, 9])
    pin[:, 70:] = [[5, 9, 9, 5, 60, 61, 5, 9, 9, 5]]
    got_x, _ = _run_beam_form(x, V, t, pin, last, src, done, nb, ngram=1)
    assert bool((got_x[[0, 2]][:, [60, 61]] == -np.inf).all())             # rows 0 and 2 are live (instance 1 of 3 is done)


# ------------------------------------------------------------------------------------------------ B: further kernel cases
def _small(seed=3, R=4, V=30, ld=32, Tmax=8):
    rng = np.random.RandomState(seed)
    x = rng.standard_normal((R, ld)).astype(np.float32)
    x[:, V:] = np.float32(3e38)
    pin = rng.randint(1, 6, size=(R, Tmax)).astype(np.int32)
    return x, pin


def test_min_len_boundary_and_eos_forms():
    x, pin = _small()
    R, V = x.shape[0], 30
    last = np.array([1, 2, 3, 4], dtype=np.int64)
    for t, banned in ((4, True), (5, False)):                               # min_len = 5: t = min_len - 1 and t = min_len
        got, _ = _run_beam_form(x, V, t, pin, last, None, None, 1, min_len=5, eos=17)
        want, _ = _expect_beam_form(x, V, t, pin, last, None, None, 1, 0, 5, 17, [])
        assert np.array_equal(_bits(got), _bits(want)) and bool((got[:, 17] == -np.inf).all()) == banned
    got, _ = _run_beam_form(x, V, 0, pin, last, None, None, 1, min_len=5, eos=-1)      # no end token: nothing to ban
    assert np.array_equal(_bits(got), _bits(x))
    got, _ = _run_beam_form(x, V, 0, pin, last, None, None, 1, min_len=5, eos=V)       # an end token in the padding: skipped
    assert np.array_equal(_bits(got), _bits(x))
    for word, col in ((11, 11), (-1, None)):                                # eos_dev is read INSTEAD of eos
        ed = torch.tensor([word], dtype=torch.int32, device=DEV)
        got, _ = _run_beam_form(x, V, 2, pin, last, None, None, 1, min_len=5, eos=17, eos_dev=ed)
        want, _ = _expect_beam_form(x, V, 2, pin, last, None, None, 1, 0, 5, word, [])
        assert np.array_equal(_bits(got), _bits(want)) and bool((got[:, 17] != -np.inf).all())
        assert col is None or bool((got[:, col] == -np.inf).all())


def test_params_dev_overrides_both_fields():
    """The same descriptor twice, the device words rewritten in between: {2, 0} then {0, 6}; the fields say {1, 1} and lose."""
    x, pin = _small(seed=9)
    pin[:] = [[1, 2, 1, 2, 1, 2, 1, 2]]
    R, V, t = x.shape[0], 30, 4
    xd, pind = torch.from_numpy(x).to(DEV), torch.from_numpy(pin).to(DEV)
    words = torch.tensor([2, 0], dtype=torch.int32, device=DEV)
    d = ops.decode_constrain_desc(xd, V, t, prefix_in=pind, ngram=1, min_len=1, eos=20, params_dev=words)
    L = _lib.lib()
    assert L.univl_decode_constrain(C.byref(d), ops._stream()) == 0
    torch.cuda.synchronize()
    want = constrain_ref(x, V, pin, t, None, 2, 0, 20, [])
    assert np.array_equal(_bits(xd.cpu().numpy()), _bits(want)) and bool((want[:, 1] == -np.inf).all()) and bool((want[:, 2] != -np.inf).all())
    xd.copy_(torch.from_numpy(x))
    words.copy_(torch.tensor([0, 6], dtype=torch.int32))
    assert L.univl_decode_constrain(C.byref(d), ops._stream()) == 0
    torch.cuda.synchronize()
    want = constrain_ref(x, V, pin, t, None, 0, 6, 20, [])
    assert np.array_equal(_bits(xd.cpu().numpy()), _bits(want)) and bool((want[:, 20] == -np.inf).all()) and bool((want[:, 1] != -np.inf).all())


def test_suppress_lists():
    x, pin = _small(seed=4)
    V = 30
    last = np.zeros(4, dtype=np.int64)
    for ids in ([], [7, 7, 7, 3], [-1, V, V + 1, 29, 0], list(range(100)) * 2):
        sup = torch.tensor(ids, dtype=torch.int32, device=DEV) if ids else None
        got, _ = _run_beam_form(x, V, 0, pin, last, None, None, 1, suppress=sup)
        want = constrain_ref(x, V, pin, 0, None, 0, 0, -1, ids)
        assert np.array_equal(_bits(got), _bits(want)), ids
        assert np.array_equal(_bits(got[:, V:]), _bits(x[:, V:]))
    assert np.array_equal(_bits(constrain_ref(x, V, pin, 0, None, 0, 0, -1, [])), _bits(x))


def test_sampler_form():
    """last = NULL, src = NULL, prefix_out = NULL: the prefix is read where it stands (the sampler's tokens_out, -1 past t), done is per row."""
    x, pin = _small(seed=5)
    V, t = 30, 5
    pin[:, t:] = -1
    pin[2, :t] = [3, 4, 3, 4, 3]
    done = np.array([0, 1, 0, 0], dtype=np.uint8)
    for ngram in (0, 1, 2, 3):
        xd, pind = torch.from_numpy(x).to(DEV), torch.from_numpy(pin).to(DEV)
        ops.decode_constrain(xd, V, t, prefix_in=pind, done=torch.from_numpy(done).to(DEV), done_stride=1, ngram=ngram, min_len=6, eos=8)
        torch.cuda.synchronize()
        want = constrain_ref(x, V, pin, t, done, ngram, 6, 8, [])
        assert np.array_equal(_bits(xd.cpu().numpy()), _bits(want)), ngram
        assert torch.equal(pind.cpu(), torch.from_numpy(pin))
    assert want[2, 4] == -np.inf and want[1, 8] != -np.inf and want[0, 8] == -np.inf
    # in place (prefix_in == prefix_out) is allowed with the identity
    xd, pind = torch.from_numpy(x).to(DEV), torch.from_numpy(pin).to(DEV)
    last = torch.tensor([9, 9, 9, 9], dtype=torch.int64, device=DEV)
    ops.decode_constrain(xd, V, t, prefix_in=pind, prefix_out=pind, last=last, ngram=1)
    torch.cuda.synchronize()
    pw = advance_prefix(pin, None, [9] * 4, t, before=pin)
    assert np.array_equal(pind.cpu().numpy(), pw) and np.array_equal(_bits(xd.cpu().numpy()), _bits(constrain_ref(x, V, pw, t, None, 1, 0, -1, [])))


def test_argument_range():
    x, pin = _small(seed=6)
    V, t = 30, 3
    xd, pind, pout = torch.from_numpy(x).to(DEV), torch.from_numpy(pin).to(DEV), torch.zeros(pin.shape, dtype=torch.int32, device=DEV)
    src = torch.arange(4, dtype=torch.int32, device=DEV)
    last = torch.zeros(4, dtype=torch.int64, device=DEV)
    done = torch.zeros(4, dtype=torch.uint8, device=DEV)
    sup = torch.tensor([1], dtype=torch.int32, device=DEV)
    L = _lib.lib()

    def desc(**kw):
        return ops.decode_constrain_desc(xd, V, t, prefix_in=pind, prefix_out=pout, src=src, last=last, done=done, ngram=2, min_len=1,
                                         eos=5, suppress=sup, **kw)
    bad = []
    for field, value in (("R", 0), ("V", 0), ("V", 33), ("t", -1), ("t", 8), ("Tmax", 3), ("ngram", -1), ("ngram", 5), ("min_len", -1),
                         ("n_suppress", -1), ("done_stride", 0), ("x", None), ("prefix_in", None), ("prefix_out", None), ("suppress", None),
                         ("prefix_out", pind.data_ptr()), ("prefix_out", pind.data_ptr() + 4 * 8)):
        d = desc()
        setattr(d, field, value)
        bad.append((field, value, d))
    d = desc()
    d.last, d.prefix_in = None, None                                        # ngram > 0 reads a prefix
    bad.append(("prefix_in without last", None, d))
    for field, value, d in bad:
        assert L.univl_decode_constrain(C.byref(d), ops._stream()) == EINVAL, (field, value)
        assert b"univl_decode_constrain" in L.univl_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(xd.cpu().numpy()), _bits(x)) and not bool(pout.any())          # nothing was launched
    # what is NOT an error: t == 0 without any prefix; the identity in place; optional pointers absent
    d = ops.decode_constrain_desc(xd, V, 0, Tmax=8, ngram=4, min_len=0)
    assert L.univl_decode_constrain(C.byref(d), ops._stream()) == 0
    d = ops.decode_constrain_desc(xd, V, t, prefix_in=pind, prefix_out=pind, last=last)
    assert L.univl_decode_constrain(C.byref(d), ops._stream()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(_bits(xd.cpu().numpy()), _bits(x))


# ------------------------------------------------------------------------------------------------ C: sessions
# The settings of the session tests.  The case is tests/golden/beam_caption_small.npz's (3 instances x 5 beams, vocabulary 30522, bos
# 101, end token eos2 = 4225: its config and seeds; the stored hypotheses are not used), decoded over T_DEC = 12 positions, because
# within the golden's own 5 no token ever repeats and n-gram blocking would never bind.  min_len = 4 as the issue states it; the
# suppress list holds BERT's special ids and 13251, the second token of instance 1's best caption; the blocked order is 1, the
# issue's fallback, because no 2-gram repeats within 12 positions either.
# OBSERVED on the MI355X (test_constrained_output_has_the_properties prints it):
#   unconstrained: lengths [2, 12, 12] -- all five n-best captions of instance 0 end on the end token at their second position, a
#   violation of min_len = 4 -- and 13251 is emitted;
#   (0, MIN_LEN, SUPPRESS), the same settings with the order at 0: hypothesis 2 of instance 2 holds one token twice;
#   (1, MIN_LEN, SUPPRESS): no caption does, and the n-best lists of the two differ.
T_DEC = 12
NGRAM, MIN_LEN = 1, 4
SUPPRESS = (0, 100, 101, 102, 103, 13251)
FIELDS = ("tokens", "scores", "lengths", "parents", "step_tokens", "step_scores")


@functools.lru_cache(maxsize=None)
def _small_case():
    g = np.load(os.path.join(GOLDEN, "beam_caption_small.npz"))
    cfg, _, dseed = case_config("caption_small")
    n, nb, T = int(g["n_inst"]), int(g["n_bm"]), T_DEC
    model, _ = build(cfg, torch.float32)
    model.eval()
    d = {k: v.to(DEV) for k, v in O.synthetic_batch(cfg, n, seed=int(g["data_seed"])).items()}
    with torch.no_grad():
        so, vo = model.get_sequence_visual_output(d["input_ids"], d["token_type_ids"], d["attention_mask"], d["video"], d["video_mask"])
    enc = (so, vo, d["attention_mask"].view(n, -1), d["video_mask"].view(n, -1))
    return dict(cfg=cfg, model=model, n=n, nb=nb, T=T, bos=int(g["bos"]), eos=int(g["eos2"]), enc=enc)


def _mk(mode="device", **kw):
    s = _small_case()
    return CaptionBeamSearch(s["model"], s["n"], s["cfg"].max_words, s["cfg"].max_frames, n_bm=s["nb"], max_len=s["T"], use_graphs=True,
                             beam_step=mode, **kw)


@functools.lru_cache(maxsize=None)
def _plain():
    """A session constructed WITHOUT the argument, and its decode of the case (n_best = n_bm)."""
    s = _small_case()
    bs = _mk()
    return bs, bs.decode(*s["enc"], bos=s["bos"], eos=s["eos"], n_best=s["nb"])


@functools.lru_cache(maxsize=None)
def _constrained(mode):
    s = _small_case()
    bs = _mk(mode, constraints=DecodeConstraints(NGRAM, MIN_LEN, SUPPRESS))
    return bs, bs.decode(*s["enc"], bos=s["bos"], eos=s["eos"], n_best=s["nb"])


@functools.lru_cache(maxsize=None)
def _unblocked():
    """The constrained settings with the blocked order at 0: what the n-gram property is measured against."""
    s = _small_case()
    bs = _mk(constraints=DecodeConstraints(0, MIN_LEN, SUPPRESS))
    return bs, bs.decode(*s["enc"], bos=s["bos"], eos=s["eos"], n_best=s["nb"])


def _same(a, b):
    for f in FIELDS:
        assert torch.equal(getattr(a, f), getattr(b, f)), f


def _violations(hyps, ngram, min_len, suppress, eos, max_len):
    """(captions with a repeated n-gram, captions shorter than min_len that did not run to max_len or with the end token before
    position min_len, captions holding a suppressed id), each a list of (instance, k)."""
    rep, short, sup = [], [], []
    for i, inst in enumerate(hyps):
        for k, h in enumerate(inst):
            grams = [tuple(h[j:j + ngram]) for j in range(len(h) - ngram + 1)] if ngram else []
            if len(set(grams)) < len(grams):
                rep.append((i, k))
            if (len(h) < min_len and len(h) < max_len) or eos in h[:min_len]:
                short.append((i, k))
            if set(h) & set(suppress):
                sup.append((i, k))
    return rep, short, sup


def test_constraints_none_changes_nothing():
    """constraints=None: tokens, scores, lengths and the history are bit-identical to a session constructed without the argument, every
    position's plan has the same number of entries, and there is no prefix buffer."""
    s = _small_case()
    plain, want = _plain()
    bs = _mk(constraints=None)
    got = bs.decode(*s["enc"], bos=s["bos"], eos=s["eos"], n_best=s["nb"])
    _same(got, want)
    assert len(bs.steps) == s["T"] and all(len(bs.steps[k]) == len(plain.steps[k]) for k in bs.steps)
    assert not hasattr(bs, "prefix") and bs.constraints is None
    assert not any(op.name == "univl_decode_constrain" for pl in bs.steps.values() for op in pl.ops)
    with pytest.raises(ValueError):
        bs.set_constraints(ngram=1)
    # the constrained session has exactly one more entry per position, in front of the beam step
    cs, _ = _constrained("device")
    for k in bs.steps:
        pl = cs.steps[k]
        names = [op.name for op in pl.ops]
        assert len(pl) == len(plain.steps[k]) + 1 and names.count("univl_decode_constrain") == 1
        assert names.index("univl_decode_constrain") == names.index("univl_beam_step") - 1


def _reference_loop(ngram, min_len, suppress):
    """Beam.advance in numpy over an UNCONSTRAINED session's log-probabilities with constrain_ref applied on the host: candidates
    lp + score (one fp32 addition; beam 0 alone at t = 0), the n_bm largest with equal values ordered by lower flat index, frozen
    instances as the header of univl_beam_step states them, then the walk-back.  Returns (tokens [n, nb, T], scores [n, nb], lengths)."""
    s = _small_case()
    n, nb, T, eos = s["n"], s["nb"], s["T"], s["eos"]
    plain, _ = _plain()
    V, R = plain.V, n * nb
    plain.encode(*s["enc"])
    base = (np.arange(n) * nb)[:, None]
    scores, done, length = np.zeros((n, nb), dtype=np.float32), np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.int64)
    tokens, parents = np.full((n, nb), s["bos"], dtype=np.int64), np.tile(np.arange(nb), (n, 1))
    prefix = np.zeros((R, T), dtype=np.int32)
    hist_par, hist_tok = np.zeros((T, n, nb), dtype=np.int64), np.zeros((T, n, nb), dtype=np.int64)
    for t in range(T):
        src = (base + parents).reshape(-1)
        lp = plain.step_logprobs(t, torch.from_numpy(tokens).to(DEV), torch.from_numpy(base + parents).to(DEV) if t > 0 else None)
        lp = lp.cpu().numpy()
        if t > 0:
            prefix = advance_prefix(prefix, src, tokens.reshape(-1), t)
        lp = constrain_ref(lp, V, prefix, t, done, ngram, min_len, eos, suppress, done_stride=nb).reshape(n, nb, V)
        for i in range(n):
            if done[i]:
                parents[i] = np.arange(nb)
            else:
                cand = lp[i, 0] if t == 0 else (lp[i] + scores[i][:, None]).astype(np.float32).reshape(-1)
                top = np.argsort(-cand, kind="stable")[:nb]                # descending; equal values: lower flat index first
                scores[i], parents[i], tokens[i] = cand[top], top // V, top % V
                length[i] += 1
                if tokens[i, 0] == eos:
                    done[i] = 1
            hist_par[t, i], hist_tok[t, i] = parents[i], tokens[i]
    out = np.full((n, nb, T), -1, dtype=np.int64)
    for i in range(n):
        for k in range(nb):
            b = k
            for j in range(length[i] - 1, -1, -1):
                out[i, k, j] = hist_tok[j, i, b]
                b = hist_par[j, i, b]
    return out, scores, length


def test_device_host_and_reference_loop_agree():
    """beam_step="device" and "host" under DecodeConstraints(NGRAM, MIN_LEN, SUPPRESS) give identical hypotheses and scores, and both
    equal the reference loop above, which shares no code with the feature."""
    _, rd = _constrained("device")
    _, rh = _constrained("host")
    tok, sc, ln = _reference_loop(NGRAM, MIN_LEN, SUPPRESS)
    for r in (rd, rh):
        assert np.array_equal(r.tokens.cpu().numpy().astype(np.int64), tok)
        assert np.array_equal(_bits(r.scores.cpu().numpy()), _bits(sc))
        assert r.lengths.tolist() == ln.tolist()
    assert torch.equal(rd.tokens, rh.tokens) and torch.equal(rd.scores, rh.scores) and torch.equal(rd.lengths, rh.lengths)
    assert bool(torch.isfinite(rd.scores).all())


def test_constrained_output_has_the_properties():
    """Non-vacuity first, for EACH of the three: the unconstrained n-best captions end too early and hold a suppressed id, and with
    the order alone switched off, (0, MIN_LEN, SUPPRESS), a caption repeats a token.  Then the constrained ones hold no repeated
    NGRAM-gram, none ends before MIN_LEN tokens unless it ran to max_len, none holds a suppressed id, and they differ from both."""
    s = _small_case()
    _, plain = _plain()
    _, res = _constrained("device")
    _, off = _unblocked()
    before = _violations(plain.hypotheses(), NGRAM, MIN_LEN, SUPPRESS, s["eos"], s["T"])
    mid = _violations(off.hypotheses(), NGRAM, MIN_LEN, SUPPRESS, s["eos"], s["T"])
    print("[constraints] unconstrained: repeated %d-gram %s, short %s, suppressed id %s; lengths %s"
          % (NGRAM, before[0], before[1], before[2], plain.lengths.tolist()))
    print("[constraints] order 0, same min_len and list: repeated %d-gram %s, short %s, suppressed id %s" % ((NGRAM,) + mid))
    assert before[1] and before[2], before            # instance 0 ends on the end token at its second position; 13251 is emitted
    assert mid[0] and mid[1:] == ([], []), mid        # blocking has something to do, and only blocking
    assert not torch.equal(res.tokens, off.tokens)
    after = _violations(res.hypotheses(), NGRAM, MIN_LEN, SUPPRESS, s["eos"], s["T"])
    print("[constraints] constrained lengths %s, best captions %s" % (res.lengths.tolist(), [h[0] for h in res.hypotheses()]))
    assert after == ([], [], []), after
    assert not torch.equal(res.tokens, plain.tokens)


def test_step_logprobs_under_forced_tokens():
    """The wiring of the launch inside the session, with tokens the test chooses: a constrained session's step_logprobs is driven
    through positions 0 .. 8 with tokens from a three-symbol alphabet and non-identity parents (two beams of an instance share a
    parent, rows change places), the middle instance marked done, order 2.  Every position's rows, all V columns (the padding
    columns are the kernel tests'), must equal, bit for bit, constrain_ref applied to an UNCONSTRAINED session's rows for the same tokens and parents, under the prefixes
    the test keeps itself.  Wrong src / last / buffer parity / done_stride / launch order each change the banned columns here."""
    s = _small_case()
    n, nb, eos = s["n"], s["nb"], s["eos"]
    plain, _ = _plain()
    cs = _mk(constraints=DecodeConstraints(2, MIN_LEN, SUPPRESS))
    V, R = cs.V, n * nb
    alphabet = np.array([2000, 2001, eos])
    done = np.array([0, 1, 0], dtype=np.uint8)
    for bs in (plain, cs):
        bs.encode(*s["enc"])
    cs.done.copy_(torch.from_numpy(done))                                   # what step_logprobs documents: the state is the caller's
    cs.eos_dev.fill_(eos)
    rng = np.random.RandomState(21)
    base = (np.arange(n) * nb)[:, None]
    prefix = np.zeros((R, s["T"]), dtype=np.int32)
    ngram_bans = 0
    for t in range(9):
        tokens = np.full((n, nb), s["bos"], dtype=np.int64) if t == 0 else rng.choice(alphabet, size=(n, nb))
        parents = np.stack([rng.permutation(nb) for _ in range(n)])
        parents[:, 0] = parents[:, 1]
        tok_d = torch.from_numpy(tokens).to(DEV)
        par_d = torch.from_numpy(base + parents).to(DEV) if t > 0 else None
        raw = plain.step_logprobs(t, tok_d, par_d).cpu().numpy()
        got = cs.step_logprobs(t, tok_d, par_d).cpu().numpy()
        if t > 0:
            prefix = advance_prefix(prefix, (base + parents).reshape(-1), tokens.reshape(-1), t)
        want = constrain_ref(raw, V, prefix, t, done, 2, MIN_LEN, eos, SUPPRESS, done_stride=nb)
        assert got.shape == (R, V) and np.array_equal(_bits(got), _bits(want)), (t, np.argwhere(_bits(got) != _bits(want))[:4])
        assert np.array_equal(_bits(got[nb:2 * nb]), _bits(raw[nb:2 * nb]))          # the done instance's rows are untouched
        ngram_bans += int((want[:, 2000:2002] == -np.inf).sum()) + (int((want[:, eos] == -np.inf).sum()) if t >= MIN_LEN else 0)
    assert ngram_bans >= 10, ngram_bans                                     # bans that only the 2-gram rule can have made


def test_set_constraints_needs_no_new_capture(monkeypatch):
    """A captured session with an empty suppress list: set_constraints(ngram=0, min_len=0) reproduces the unconstrained result and
    setting the words back reproduces the constrained one, with no graph captured in between."""
    s = _small_case()
    _, want = _plain()
    _unblocked()                                                            # its own captures happen here, before the count
    bs = _mk(constraints=DecodeConstraints(1, MIN_LEN, ()))
    first = bs.decode(*s["enc"], bos=s["bos"], eos=s["eos"], n_best=s["nb"])
    assert not torch.equal(first.tokens, want.tokens)
    captures = []
    enter = torch.cuda.graph.__enter__

    def counting(self):
        captures.append(1)
        return enter(self)
    monkeypatch.setattr(torch.cuda.graph, "__enter__", counting)
    bs.set_constraints(ngram=0, min_len=0)
    _same(bs.decode(*s["enc"], bos=s["bos"], eos=s["eos"], n_best=s["nb"]), want)
    bs.set_constraints(ngram=1, min_len=MIN_LEN)
    _same(bs.decode(*s["enc"], bos=s["bos"], eos=s["eos"], n_best=s["nb"]), first)
    assert captures == []
    # ... and the order alone, on a session where it binds: off gives the (0, MIN_LEN, SUPPRESS) session's result, on gives its own back
    cs = _mk(constraints=DecodeConstraints(NGRAM, MIN_LEN, SUPPRESS))
    own = cs.decode(*s["enc"], bos=s["bos"], eos=s["eos"], n_best=s["nb"])
    del captures[:]
    cs.set_constraints(ngram=0)
    got = cs.decode(*s["enc"], bos=s["bos"], eos=s["eos"], n_best=s["nb"])
    _same(got, _unblocked()[1])
    assert not torch.equal(got.tokens, own.tokens)
    cs.set_constraints(ngram=NGRAM)
    _same(cs.decode(*s["enc"], bos=s["bos"], eos=s["eos"], n_best=s["nb"]), own)
    assert captures == []
    for bad in (dict(ngram=5), dict(min_len=s["T"])):
        with pytest.raises(ValueError):
            bs.set_constraints(**bad)
    for bad in (DecodeConstraints(min_len=s["T"]), DecodeConstraints(suppress=[30522])):
        with pytest.raises(ValueError):
            _mk(constraints=bad)


def test_partial_batch_under_constraints():
    """n_active = 2 of 3: the active instances' results equal the full-batch run's (the idle slot's rows are untouched, its prefix
    rows are copied from defined memory).  The batch is taken in the order 2, 0, 1, so that instance 2, the one whose n-best list
    blocking changes, is among the two active ones."""
    s = _small_case()
    order = torch.tensor([2, 0, 1], device=DEV)
    enc = tuple(t[order] for t in s["enc"])
    bs, straight = _constrained("device")
    full = bs.decode(*enc, bos=s["bos"], eos=s["eos"], n_best=s["nb"])
    assert torch.equal(full.tokens[0], straight.tokens[2]) and not torch.equal(full.tokens[0], _unblocked()[1].tokens[2])
    part = bs.decode(*(t[:2] for t in enc), bos=s["bos"], eos=s["eos"], n_best=s["nb"], n_active=2)
    for f in FIELDS:
        x, y = getattr(part, f), getattr(full, f)
        assert torch.equal(x, y[:, :2] if f in FIELDS[3:] else y[:2]), f
    fresh = _mk(constraints=DecodeConstraints(NGRAM, MIN_LEN, SUPPRESS))             # a session whose FIRST call is partial
    part2 = fresh.decode(*(t[:2] for t in enc), bos=s["bos"], eos=s["eos"], n_best=s["nb"], n_active=2)
    _same(part2, part)


def test_sampler_under_constraints():
    """CaptionSampler(n_samp=3, top_k=8): constraints=None is bit-identical to a sampler built without the argument; with constraints
    the properties hold for every sampled caption and a fixed seed reproduces the result."""
    s = _small_case()
    cfg, T = s["cfg"], s["T"]
    mk = lambda **kw: CaptionSampler(s["model"], s["n"], cfg.max_words, cfg.max_frames, n_samp=3, max_len=T, top_k=8, temperature=1.5, **kw)
    draw = lambda sm, seed: sm.sample(*s["enc"], bos=s["bos"], eos=s["eos"], seed=seed)
    fields = ("tokens", "token_logprobs", "token_q_logprobs", "seq_logprob", "seq_q_logprob", "lengths")
    a, b = draw(mk(), 11), draw(mk(constraints=None), 11)
    for f in fields:
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    # the sampler's own suppress list: the tokens its unconstrained samples start with, so that the constraint binds
    firsts = sorted({h[0] for inst in a.hypotheses() for h in inst})
    sup = tuple(SUPPRESS) + tuple(firsts)
    sm = mk(constraints=DecodeConstraints(1, MIN_LEN, sup))
    r1, r2 = draw(sm, 11), draw(sm, 11)
    for f in fields:
        assert torch.equal(getattr(r1, f), getattr(r2, f)), f
    assert _violations(a.hypotheses(), 1, MIN_LEN, sup, s["eos"], T)[2]
    assert _violations(r1.hypotheses(), 1, MIN_LEN, sup, s["eos"], T) == ([], [], [])
    assert bool(torch.isfinite(r1.seq_logprob).all()) and bool((r1.lengths >= min(MIN_LEN, T)).all())
    assert not torch.equal(draw(sm, 12).tokens, r1.tokens)
    # Sampled captions of this model do not repeat a token on their own, so the property above cannot show that each row is blocked
    # on ITS OWN tokens_out row.  The masked logits of the last position can: with sync_every = 0 the session's logits are those of
    # position T - 1, where a live row's -inf columns must be exactly its own first T - 1 tokens and the list (t >= min_len: the end
    # token is free), and a row that finished earlier keeps raw logits.
    r3 = sm.sample(*s["enc"], bos=s["bos"], eos=s["eos"], seed=13, sync_every=0)
    logits, tok, lens = sm.head.logits[:, :sm.V].cpu().numpy(), r3.tokens.cpu().numpy().reshape(-1, T), r3.lengths.cpu().numpy().reshape(-1)
    assert np.isfinite(sm.step_logits(0, torch.full((logits.shape[0],), s["bos"], device=DEV)).cpu().numpy()).all()     # raw rows are finite
    live = 0
    for r in range(logits.shape[0]):
        banned = set(np.nonzero(logits[r] == -np.inf)[0].tolist())
        if lens[r] == T:
            assert banned == set(tok[r, :T - 1].tolist()) | set(sup), r
            live += 1
        else:
            assert banned == set(), r
    assert live >= 2 and len({tuple(row[:T - 1]) for row in tok}) > 1              # rows with different prefixes were checked


def test_eval_caption_with_constraints():
    """Two tiny batches (3 + 2 items): eval_caption builds the session with the constraints and every caption honours them; a
    supplied session beside the argument raises."""
    s = _small_case()
    cfg, T = s["cfg"], s["T"]
    order = ("input_ids", "attention_mask", "token_type_ids", "video", "video_mask", "pairs_masked_text", "pairs_token_labels",
             "masked_video", "video_labels_index", "input_caption_ids", "decoder_mask", "output_caption_ids")
    b = O.synthetic_batch(cfg, 5, seed=91)
    loader = [tuple(b[k][:3] for k in order), tuple(b[k][3:] for k in order)]
    tk = SynthTokenizer(cfg.vocab_size, special={"[SEP]": s["eos"], "[CLS]": s["bos"]})
    plain = eval_caption(s["model"], loader, tk, n_bm=s["nb"], n_best=2, max_len=T)
    firsts = sorted({ids[0][0] for ids in plain.hyp_ids if ids[0]})
    cons = DecodeConstraints(1, MIN_LEN, firsts + [tk.vocab["[PAD]"]])       # the cut also stops at "[PAD]"
    res = eval_caption(s["model"], loader, tk, n_bm=s["nb"], n_best=2, max_len=T, constraints=cons)
    assert res.session.constraints is not None and res.session.constraints is not cons and len(res.hyp_ids) == 5
    assert plain.session.constraints is None
    assert _violations(plain.hyp_ids, 1, 0, firsts, -1, T)[2]
    # hyp_ids are cut at the end token: a caption has MIN_LEN tokens in front of it unless max_len came first
    assert _violations(res.hyp_ids, 1, 0, firsts, -1, T) == ([], [], [])
    assert all(len(h) >= min(MIN_LEN, T) for ids in res.hyp_ids for h in ids)
    with pytest.raises(ValueError, match="session"):
        eval_caption(s["model"], loader, tk, session=res.session, constraints=cons)
