"""Beam search with a pool of finished hypotheses on the device (csrc/beam.hip: univl_beam_pool_step, univl_beam_pool_finish) and the
pooled mode of univl_amd.decode.CaptionBeamSearch.

A  the kernels against the numpy reference (tests/pool_beam_ref.py: all candidates sorted, the list walked), bit for bit after EVERY
   position of a whole run and after the finish, on quarter-valued log-probabilities; tests/test_pool_beam_cpu.py asserts that these
   runs contain every event of the rule;
B  no end token: univl_beam_step bit for bit;  C  frozen instances over four positions;  D  one captured graph, the device words;
E  the argument range;  F  sessions."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import pool_beam_ref as R
import univl_oracle as O
from make_golden import case_config
from pool_beam_ref import EOS, F32, PoolBeamRef
from test_caption_eval_cpu import SynthTokenizer

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from univl_amd import _lib, ops
    from univl_amd.constrain import DecodeConstraints
    from univl_amd.decode import CaptionBeamSearch, PoolBeamResult
    from univl_amd.eval import eval_caption
    from univl_amd.ops import beam_pool_step                  # the feature: without it this file fails at import
    from univl_amd.score import CaptionScorer
    from test_model_gpu import build

DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
OUT = ("scores", "tokens", "src", "done", "length", "hist_parents", "hist_tokens", "hist_scores")
POOL = ("pool_key", "pool_raw", "pool_end_t", "pool_beam", "pool_finished", "pool_count")


@pytest.fixture(autouse=True)
def _deterministic_mode():
    """Fixed-order sums in the decoder's products, the mode the session tests compare bit for bit in (as tests/test_beam_gpu.py)."""
    import univl_amd
    was = univl_amd.deterministic()
    univl_amd.set_deterministic(True)
    yield
    univl_amd.set_deterministic(was)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ------------------------------------------------------------------------------------------------ kernel harness
def _buffers(n, nb, ld, Tmax, alpha, early, max_len=None, offset=0, scores=None, done=None, length=None, tokens=None):
    """Device buffers of one run; src and the history pre-filled with the marker -7 (the reference's marker too), the pool empty."""
    z = lambda v, dt: torch.as_tensor(np.asarray(v), dtype=dt).to(DEV).contiguous()
    flat = torch.full((n * nb * ld + offset,), 1e30, device=DEV)
    d = dict(lp=flat[offset:].view(n * nb, ld),
             scores=z(np.zeros((n, nb)) if scores is None else scores, torch.float32),
             done=z(np.zeros(n) if done is None else done, torch.uint8), length=z(np.zeros(n) if length is None else length, torch.int32),
             tokens=z(np.zeros(n * nb) if tokens is None else np.asarray(tokens).reshape(-1), torch.int64),
             src=torch.full((n * nb,), -7, dtype=torch.int32, device=DEV),
             hist_parents=torch.full((Tmax, n, nb), -7, dtype=torch.int32, device=DEV),
             hist_tokens=torch.full((Tmax, n, nb), -7, dtype=torch.int32, device=DEV),
             hist_scores=torch.full((Tmax, n, nb), -7.0, device=DEV), ws=ops.beam_ws(n, nb, DEV),
             w=ops.length_weights(alpha, Tmax).to(DEV),
             params=torch.tensor([int(early), Tmax if max_len is None else max_len], dtype=torch.int32, device=DEV))
    d.update(ops.beam_pool(n, nb, DEV))
    assert d["lp"].data_ptr() % 16 == 4 * offset
    return d


def _state(d):
    return {k: v for k, v in d.items() if k != "lp"}


def _set_pool(d, ref):
    """The reference's pools into the device arrays (a preset)."""
    a = ref.pool_arrays()
    for k, name in (("key", "pool_key"), ("raw", "pool_raw"), ("end_t", "pool_end_t"), ("beam", "pool_beam"), ("finished", "pool_finished"),
                    ("count", "pool_count")):
        d[name].copy_(torch.as_tensor(a[k]).to(d[name].dtype).reshape(d[name].shape))


def _against_snapshot(d, s, t, n, nb):
    """State, history row t and the whole pool against the reference's snapshot after position t."""
    got = {k: d[k].cpu().numpy() for k in OUT + POOL}
    assert np.array_equal(_bits(got["scores"]), _bits(s["scores"])), "scores"
    assert np.array_equal(got["tokens"].reshape(n, nb), s["tokens"]), "tokens"
    assert np.array_equal(got["src"].astype(np.int64), s["src"]), "src"
    assert np.array_equal(got["done"], s["done"]), ("done", got["done"], s["done"])
    assert np.array_equal(got["length"].astype(np.int64), s["length"]), "length"
    assert np.array_equal(got["hist_parents"][t].astype(np.int64), s["hist_par"]), "hist_parents"
    assert np.array_equal(got["hist_tokens"][t].astype(np.int64), s["hist_tok"]), "hist_tokens"
    assert np.array_equal(_bits(got["hist_scores"][t]), _bits(s["hist_sc"])), "hist_scores"
    if t + 1 < got["hist_parents"].shape[0]:
        assert (got["hist_parents"][t + 1:] == -7).all(), "a later history row was written"
    p, m = s["pool"], s["pool"]["mask"]
    assert np.array_equal(got["pool_count"].astype(np.int64), p["count"]), ("pool_count", got["pool_count"], p["count"])
    assert np.array_equal(_bits(got["pool_key"])[m], _bits(p["key"])[m]), "pool_key"
    assert np.array_equal(_bits(got["pool_raw"])[m], _bits(p["raw"])[m]), "pool_raw"
    for k, name in (("end_t", "pool_end_t"), ("beam", "pool_beam"), ("finished", "pool_finished")):
        assert np.array_equal(got[name].astype(np.int64)[m], p[k][m]), name


def _against_finish(got, want):
    tok, raw, key, lens, fin = (x.cpu().numpy() for x in got)
    wtok, wraw, wkey, wlens, wfin = want
    assert np.array_equal(tok.astype(np.int64), wtok), "tokens"
    assert np.array_equal(_bits(raw), _bits(wraw)) and np.array_equal(_bits(key), _bits(wkey)), "raw / key"
    assert np.array_equal(lens.astype(np.int64), wlens) and np.array_equal(fin.astype(np.int64), wfin), "lengths / finished"


@pytest.mark.parametrize("early", R.MODES, ids=["bound", "early"])
@pytest.mark.parametrize("alpha", R.ALPHAS)
@pytest.mark.parametrize("V,ld,offset", R.SHAPES, ids=["vec37", "scalar37", "vec8slices"])
@pytest.mark.parametrize("nb", R.NBS)
def test_kernels_match_reference_over_a_run(nb, V, ld, offset, alpha, early):
    """A.  Tmax = 6, n_inst = 3.  V = 37 / ld = 40 aligned (16-byte loads whose last word is partly padding) and 4 bytes off
    alignment (the scalar path); V = 30522 / ld = 30528: all eight slices.  Everything is compared after every position, then the
    finish's five outputs at n_best = n_bm and at n_best = 1."""
    n, T = R.N_INST, R.TMAX
    lps, ref, snaps, fin = R.run_case(nb, V, ld, offset, alpha, early)
    d = _buffers(n, nb, ld, T, alpha, early, offset=offset)
    for t in range(T):
        d["lp"].copy_(torch.as_tensor(lps[t]))
        beam_pool_step(d["lp"], V, n, nb, t, eos=EOS, **_state(d))
        torch.cuda.synchronize()
        _against_snapshot(d, snaps[t], t, n, nb)
        assert int(d["tokens"].max()) < V and not bool((d["tokens"] == EOS).any())          # no padding column, never the end token
    desc = ops.beam_pool_step_desc(d["lp"], V, n, nb, 0, eos=EOS, **_state(d))
    keep = {k: d[k].clone() for k in POOL}
    _against_finish(ops.beam_pool_finish(desc, nb), fin)
    one = ops.beam_pool_finish(desc, 1)
    _against_finish(one, tuple(x[:, :1] for x in fin))
    for k in POOL:
        assert torch.equal(d[k], keep[k]), k                   # the finish only reads the pool


# ------------------------------------------------------------------------------------------------ B: identity
def _quarter(seed, n, nb, V, ld, first):
    rng = np.random.RandomState(seed)
    lp = (rng.randint(-200, 0, size=(n * nb, ld)) * 0.25).astype(F32)
    lp[:, V:] = 1e30
    scores = np.zeros((n, nb), dtype=F32) if first else (-rng.randint(0, 16, size=(n, nb)) * 0.25).astype(F32)
    done = np.zeros(n, dtype=np.uint8)
    if not first:
        done[1] = 1
    return lp, scores, done, rng.randint(0, V, size=(n, nb)), rng.randint(1, 3, size=n)


@pytest.mark.parametrize("first", [True, False], ids=["first", "later"])
@pytest.mark.parametrize("V,ld", [(30522, 30528), (37, 40)])
def test_without_end_token_is_the_plain_step(V, ld, first):
    """B.  eos = -1: every output bit-identical to univl_beam_step on the same buffers, and the pool is not written."""
    n, nb, T = 3, 6, 4
    lp, scores, done, tokens, length = _quarter(13 + V % 7, n, nb, V, ld, first)
    t = 0 if first else 2
    a, b = (_buffers(n, nb, ld, T, 0.6, False, scores=scores, done=done, length=length, tokens=tokens) for _ in range(2))
    for d in (a, b):
        d["lp"].copy_(torch.as_tensor(lp))
    for k in POOL:
        a[k].fill_(3)
    beam_pool_step(a["lp"], V, n, nb, t, eos=-1, first_step=first, **_state(a))
    ops.beam_step(b["lp"], V, n, nb, t, eos=-1, first_step=first, **{k: b[k] for k in OUT + ("ws",)})
    torch.cuda.synchronize()
    for k in OUT:
        assert torch.equal(a[k].reshape(-1), b[k].reshape(-1)), k
    for k in POOL:
        assert bool((a[k] == 3).all()), k


# ------------------------------------------------------------------------------------------------ C: frozen instances
def test_frozen_instances_over_four_positions():
    """C.  Four positions on device-resident state with instance 1 preset done and its pool preset: its state, its pool and its
    count stay as they are, its history rows repeat the state with identity parents; the other instances run as the reference."""
    n, nb, V, ld, T = 3, 4, 37, 40, 4
    lps = R.make_lps(77, nb, V, ld, Tmax=T, n=n)
    idle_tok = np.arange(n * nb).reshape(n, nb) % V
    idle_sc = -np.arange(n * nb, dtype=F32).reshape(n, nb)
    done0 = np.array([0, 1, 0], dtype=np.uint8)
    ref = PoolBeamRef(n, nb, V, T, 1.0, False, eos=EOS, done=done0, tokens=idle_tok, scores=idle_sc)
    ref.pool[1] = [(F32(-1.5), F32(-3.0), 1, 2, 1), (F32(-2.0), F32(-2.0), 0, 0, 1)]
    d = _buffers(n, nb, ld, T, 1.0, False, done=done0, tokens=idle_tok, scores=idle_sc)
    _set_pool(d, ref)
    for t in range(T):
        d["lp"].copy_(torch.as_tensor(lps[t]))
        beam_pool_step(d["lp"], V, n, nb, t, eos=EOS, first_step=(t == 0), **_state(d))
        ref.step(lps[t], t)
        torch.cuda.synchronize()
        snap = dict(scores=ref.scores, tokens=ref.tokens, src=ref.src, done=ref.done, length=ref.length, hist_par=ref.hist_par[t],
                    hist_tok=ref.hist_tok[t], hist_sc=ref.hist_sc[t], pool=ref.pool_arrays())
        _against_snapshot(d, snap, t, n, nb)
    assert d["length"].cpu().tolist()[1] == 0 and d["tokens"].cpu().view(n, nb)[1].tolist() == idle_tok[1].tolist()
    assert bool((d["hist_parents"][:, 1].cpu() == torch.arange(nb)).all())
    assert bool((d["hist_scores"][:, 1].cpu() == torch.as_tensor(idle_sc[1])).all())
    assert d["pool_count"].cpu().tolist()[1] == 2 and d["pool_key"].cpu()[1, :2].tolist() == [-1.5, -2.0]
    # the finish: a done instance's live beams are not offered -- instance 1 has its two entries and two idle slots
    tok, raw, key, lens, fin = ops.beam_pool_finish(ops.beam_pool_step_desc(d["lp"], V, n, nb, 0, eos=EOS, **_state(d)), nb)
    _against_finish((tok, raw, key, lens, fin), ref.finish(nb))
    assert key[1].cpu().tolist() == [-1.5, -2.0, -np.inf, -np.inf] and lens[1].cpu().tolist() == [2, 1, 0, 0]
    assert bool((tok[1, 2:] == -1).all()) and fin[1].cpu().tolist() == [1, 1, 0, 0]


# ------------------------------------------------------------------------------------------------ D: device words
def test_device_words_serve_every_setting_under_one_graph():
    """D.  One captured launch pair at t = 2 with full pools: best live score -12, last key -0.5.  (alpha 2, eos 5, max_len 4) and
    (alpha 2, eos 5, max_len 6) differ in max_len alone: -12 / 16 <= -0.5 is done, -12 / 36 is not.  (alpha 0, eos 5, max_len 6)
    differs from the second in the penalty alone: -12 <= -0.5 is done.  (alpha 0.6, eos 7, early stopping) is done by its mode, and
    its other end token changes the live beams: column 5 is a live beam there and column 7 is not.  Each replay equals the reference
    from the same state; the descriptor's own eos field (-1) is not read."""
    n, nb, V, ld, T, t = 2, 3, 37, 40, 6, 2
    rng = np.random.RandomState(9)
    lp = (rng.randint(-200, -40, size=(n * nb, ld)) * 0.25).astype(F32)
    lp[:, V:] = 1e30
    lp[::nb, 11] = -1.0                                       # the best continuation of every instance's beam 0
    lp[::nb, 5] = -1.25                                       # ... and either end column just behind it: rank 1 < n_bm
    lp[::nb, 7] = -1.5
    scores = np.tile(np.array([-11.0, -20.0, -21.0], dtype=F32), (n, 1))
    tokens, length = rng.randint(10, V, size=(n, nb)), np.full(n, 2)
    full = [(F32(-0.5), F32(-2.0), 1, 0, 1), (F32(-0.25), F32(-0.25), 0, 0, 1), (F32(-0.375), F32(-1.5), 1, 1, 1)]

    def mk(alpha, early, eos, max_len):
        r = PoolBeamRef(n, nb, V, T, alpha, early, eos=eos, max_len=max_len, scores=scores, tokens=tokens, length=length)
        r.pool = [list(full) for _ in range(n)]
        return r
    d = _buffers(n, nb, ld, T, 2.0, False, scores=scores, tokens=tokens, length=length)
    d["lp"].copy_(torch.as_tensor(lp))
    _set_pool(d, mk(2.0, False, 5, 4))
    keep = {k: d[k].clone() for k in OUT + POOL}
    word = torch.full((1,), 5, dtype=torch.int32, device=DEV)
    desc = ops.beam_pool_step_desc(d["lp"], V, n, nb, t, eos=-1, eos_dev=word, **_state(d))
    L = _lib.lib()
    assert L.univl_beam_pool_step(C.byref(desc), ops._stream()) == 0            # once outside the capture; the state is restored below
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        assert L.univl_beam_pool_step(C.byref(desc), ops._stream()) == 0
    dones = []
    for alpha, early, eos, max_len in ((2.0, False, 5, 4), (2.0, False, 5, 6), (0.0, False, 5, 6), (0.6, True, 7, 6)):
        for k in keep:
            d[k].copy_(keep[k])
        d["w"].copy_(ops.length_weights(alpha, T))
        d["params"].copy_(torch.tensor([int(early), max_len], dtype=torch.int32))
        word.fill_(eos)
        g.replay()
        torch.cuda.synchronize()
        ref = mk(alpha, early, eos, max_len)
        ref.step(lp, t, first=False)
        snap = dict(scores=ref.scores, tokens=ref.tokens, src=ref.src, done=ref.done, length=ref.length, hist_par=ref.hist_par[t],
                    hist_tok=ref.hist_tok[t], hist_sc=ref.hist_sc[t], pool=ref.pool_arrays())
        got = {k: d[k].cpu().numpy() for k in OUT + POOL}
        assert np.array_equal(got["done"], ref.done) and np.array_equal(got["tokens"].reshape(n, nb), ref.tokens)
        assert np.array_equal(_bits(got["scores"]), _bits(ref.scores)) and np.array_equal(got["pool_count"], snap["pool"]["count"])
        for k, name in (("key", "pool_key"), ("raw", "pool_raw")):
            assert np.array_equal(_bits(got[name]), _bits(snap["pool"][k])), name
        for k, name in (("end_t", "pool_end_t"), ("beam", "pool_beam")):
            assert np.array_equal(got[name].astype(np.int64), snap["pool"][k]), name
        dones.append(ref.done.tolist())
        assert float(ref.scores[0, 0]) == -12.0 and ref.tokens[0].tolist()[:2] == [11, 7 if eos == 5 else 5]
    assert dones == [[1, 1], [0, 0], [1, 1], [1, 1]]


# ------------------------------------------------------------------------------------------------ E: argument range
def test_argument_range():
    """E.  Outside the range: UNIVL_EINVAL with a message, and nothing launched -- the outputs keep their sentinels."""
    n, nb, V, ld, T = 2, 6, 64, 64, 4
    lp, scores, done, tokens, length = _quarter(3, n, nb, V, ld, False)
    d = _buffers(n, nb, ld, T, 1.0, False, scores=scores, done=done, length=length, tokens=tokens)
    d["lp"].copy_(torch.as_tensor(lp))
    keep = {k: d[k].clone() for k in OUT + POOL}
    L = _lib.lib()

    def rc(**kw):
        desc = ops.beam_pool_step_desc(d["lp"], V, n, nb, 1, eos=3, **_state(d))
        for k, v in kw.items():
            setattr(desc, k, v)
        r = L.univl_beam_pool_step(C.byref(desc), ops._stream())
        torch.cuda.synchronize()
        return r

    EINVAL = -1
    for kw in (dict(n_bm=0), dict(n_bm=9), dict(n_bm=-3), dict(V=5), dict(V=0), dict(ld=V - 1), dict(n_inst=0), dict(n_inst=-3),
               dict(t=T), dict(t=-1), dict(Tmax=0), dict(ws_bytes=n * nb * 8 * nb * 8 - 1), dict(ws=None), dict(lp=None),
               dict(scores=None), dict(done=None), dict(length=None), dict(tokens=None), dict(src=None), dict(hist_parents=None),
               dict(hist_tokens=None), dict(hist_scores=None), dict(w=None), dict(params=None), dict(pool_key=None), dict(pool_raw=None),
               dict(pool_end_t=None), dict(pool_beam=None), dict(pool_finished=None), dict(pool_count=None)):
        assert rc(**kw) == EINVAL, kw
        assert b"univl_beam_pool_step" in L.univl_last_error()
    assert L.univl_beam_pool_step(None, ops._stream()) == EINVAL
    desc = ops.beam_pool_step_desc(d["lp"], V, n, nb, 1, eos=3, **_state(d))
    out = [torch.zeros(n * nb * T, dtype=torch.int32, device=DEV) for _ in range(5)]
    ptr = [C.c_void_p(x.data_ptr()) for x in out]
    for bad in (0, nb + 1, -1):
        assert L.univl_beam_pool_finish(C.byref(desc), bad, *ptr, ops._stream()) == EINVAL
        assert b"univl_beam_pool_finish" in L.univl_last_error()
    assert L.univl_beam_pool_finish(C.byref(desc), 1, None, *ptr[1:], ops._stream()) == EINVAL
    assert L.univl_beam_pool_finish(None, 1, *ptr, ops._stream()) == EINVAL
    torch.cuda.synchronize()
    for k in keep:
        assert torch.equal(d[k], keep[k]), k                   # nothing was launched
    assert rc() == 0
    assert not torch.equal(d["hist_tokens"], keep["hist_tokens"])


# ------------------------------------------------------------------------------------------------ F: sessions
N_INST, N_BM, T_DEC, ALPHA = 2, 4, 6, 1.0


@functools.lru_cache(maxsize=None)
def _case(dtype):
    """The small decoder case of tests/test_group_beam_gpu.py.  The end token is the one instance 0's top beam emits at position 1 of
    an unended plain search: in the pooled search it is the best candidate there, so a hypothesis finishes."""
    g = np.load(os.path.join(GOLDEN, "beam_caption_small.npz"))
    cfg, _, _ = case_config("caption_small")
    model, _ = build(cfg, dtype)
    model.eval()
    d = {k: v.to(DEV) for k, v in O.synthetic_batch(cfg, N_INST, seed=int(g["data_seed"])).items()}
    with torch.no_grad():
        so, vo = model.get_sequence_visual_output(d["input_ids"], d["token_type_ids"], d["attention_mask"], d["video"], d["video_mask"])
    enc = (so, vo, d["attention_mask"].view(N_INST, -1), d["video_mask"].view(N_INST, -1))
    s = dict(cfg=cfg, model=model, bos=int(g["bos"]), enc=enc)
    plain = CaptionBeamSearch(model, N_INST, cfg.max_words, cfg.max_frames, n_bm=N_BM, max_len=T_DEC)
    s["plain"] = plain
    s["eos"] = int(plain.decode(*enc, bos=s["bos"], eos=-1, n_best=1).step_tokens[1, 0, 0])
    return s


def _mk(dtype, **kw):
    s = _case(dtype)
    return CaptionBeamSearch(s["model"], N_INST, s["cfg"].max_words, s["cfg"].max_frames, n_bm=N_BM, max_len=T_DEC, **kw)


@functools.lru_cache(maxsize=None)
def _pooled(dtype):
    s = _case(dtype)
    bs = _mk(dtype, length_penalty=ALPHA)
    return bs, bs.decode(*s["enc"], bos=s["bos"], eos=s["eos"], n_best=N_BM)


FIELDS = ("tokens", "scores", "norm_scores", "lengths", "finished", "positions", "parents", "step_tokens", "step_scores")


def _same(a, b):
    for f in FIELDS:
        assert torch.equal(getattr(a, f), getattr(b, f)), f


def _reference_run(dtype, alpha, early=False, driver=None, max_len=T_DEC):
    """A second session's log-probabilities, position by position through step_logprobs, with the numpy reference doing the search."""
    s = _case(dtype)
    bs = driver or s["plain"]
    bs.encode(*s["enc"])
    bs.done.zero_()
    bs.eos_dev.fill_(s["eos"])
    ref = PoolBeamRef(N_INST, N_BM, bs.V, T_DEC, alpha, early, eos=s["eos"], max_len=max_len, tokens=np.full((N_INST, N_BM), s["bos"]))
    for t in range(max_len):
        lp = bs.step_logprobs(t, torch.from_numpy(ref.tokens).to(DEV), torch.from_numpy(ref.src).to(DEV) if t > 0 else None)
        ref.step(lp.cpu().numpy(), t)
    return ref


def _result_against_ref(res, ref, n_best):
    tok, raw, key, lens, fin = ref.finish(n_best)
    assert np.array_equal(res.tokens.cpu().numpy().astype(np.int64), tok)
    assert np.array_equal(_bits(res.scores.cpu().numpy()), _bits(raw)) and np.array_equal(_bits(res.norm_scores.cpu().numpy()), _bits(key))
    assert np.array_equal(res.lengths.cpu().numpy().astype(np.int64), lens)
    assert np.array_equal(res.finished.cpu().numpy().astype(np.int64), fin)
    assert np.array_equal(res.positions.cpu().numpy().astype(np.int64), ref.length)
    return tok, lens, fin


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_session_matches_reference_run(dtype):
    """F (i).  decode() of a pooled session against the reference driven by a second session's rows: tokens, lengths, flags and
    positions exactly, raw scores and keys bit for bit, the history row for row; captions() and hypotheses() at each hypothesis's
    own length."""
    s = _case(dtype)
    bs, res = _pooled(dtype)
    ref = _reference_run(dtype, ALPHA)
    assert isinstance(res, PoolBeamResult) and res.tokens.shape == (N_INST, N_BM, T_DEC) and res.lengths.shape == (N_INST, N_BM)
    tok, lens, fin = _result_against_ref(res, ref, N_BM)
    ran = res.steps_run
    live = np.arange(ran)[:, None] < ref.length[None, :]                            # rows an instance ran; later rows are frozen rows
    assert np.array_equal(res.step_tokens.cpu().numpy().astype(np.int64)[live], ref.hist_tok[:ran][live])
    assert np.array_equal(res.parents.cpu().numpy().astype(np.int64)[live], ref.hist_par[:ran][live])
    assert np.array_equal(_bits(res.step_scores.cpu().numpy())[live], _bits(ref.hist_sc[:ran])[live])
    assert fin.any() and not fin.all()                                              # finished hypotheses and live beams both came back
    k = res.norm_scores
    assert bool((k[:, 1:] <= k[:, :-1]).all())                                      # pool order
    assert not bool((res.step_tokens == s["eos"]).any())                            # a live beam never holds the end token
    hyps = res.hypotheses()
    cap, cap_len = res.captions(s["eos"], -1)
    assert cap.shape == res.tokens.shape and cap_len.shape == res.lengths.shape
    for i in range(N_INST):
        for j in range(N_BM):
            want = [int(v) for v in tok[i, j, :lens[i, j]]]
            assert hyps[i][j] == want and (want[-1] == s["eos"]) == bool(fin[i, j]) and s["eos"] not in want[:-1]
            cut = len(want) - int(fin[i, j])
            assert int(cap_len[i, j]) == cut and cap[i, j, :cut].tolist() == want[:cut] and bool((cap[i, j, cut:] == -1).all())
    with pytest.raises(ValueError):
        bs.decode(*s["enc"], bos=s["bos"], eos=s["eos"], n_best=N_BM + 1)


def test_eager_sync_every_and_other_settings_agree():
    """F (ii).  use_graphs=False equals graphs; sync_every 0, 1 and the default give the same result (frozen instances); early
    stopping and another max_len equal their own reference runs."""
    s = _case(torch.float32)
    bs, res = _pooled(torch.float32)
    eager = _mk(torch.float32, length_penalty=ALPHA, use_graphs=False)
    _same(eager.decode(*s["enc"], bos=s["bos"], eos=s["eos"], n_best=N_BM), res)
    for every in (0, 1):
        _same(bs.decode(*s["enc"], bos=s["bos"], eos=s["eos"], n_best=N_BM, sync_every=every), res)
    es = _mk(torch.float32, length_penalty=ALPHA, early_stopping=True)
    for every in (0, 1):
        _result_against_ref(es.decode(*s["enc"], bos=s["bos"], eos=s["eos"], n_best=2, sync_every=every),
                            _reference_run(torch.float32, ALPHA, True), 2)
    short = bs.decode(*s["enc"], bos=s["bos"], eos=s["eos"], n_best=N_BM, max_len=4)
    assert short.steps_run == 4
    _result_against_ref(short, _reference_run(torch.float32, ALPHA, max_len=4), N_BM)
    _same(bs.decode(*s["enc"], bos=s["bos"], eos=s["eos"], n_best=N_BM), res)


def test_partial_batch():
    """F (iii).  n_active = 1: the result is the first instance of the full batch; the idle slot is preset done with an empty pool."""
    s = _case(torch.float32)
    bs, full = _pooled(torch.float32)
    so, vo, am, vm = s["enc"]
    part = bs.decode(so[:1], vo[:1], am[:1], vm[:1], bos=s["bos"], eos=s["eos"], n_best=N_BM, n_active=1)
    assert part.tokens.shape[0] == 1 and part.lengths.shape == (1, N_BM) and part.positions.shape == (1,)
    for f in ("tokens", "scores", "norm_scores", "lengths", "finished", "positions"):
        assert torch.equal(getattr(part, f), getattr(full, f)[:1]), f
    for f in ("parents", "step_tokens", "step_scores"):
        assert torch.equal(getattr(part, f), getattr(full, f)[:, :1]), f
    assert bs.done.cpu().tolist()[1] == 1 and bs.length.cpu().tolist()[1] == 0 and bs.pool["pool_count"].cpu().tolist()[1] == 0
    _same(bs.decode(*s["enc"], bos=s["bos"], eos=s["eos"], n_best=N_BM), full)      # and the full batch again


def test_under_constraints():
    """F (iv).  DecodeConstraints(min_len=3, no_repeat_ngram=2): the constraint launch sits in front of the pool step, no finished
    hypothesis is shorter than the minimum (3 tokens, then the end token), none repeats a bigram, and the run equals the reference
    run on a second session's constrained rows."""
    s = _case(torch.float32)
    cons = DecodeConstraints(min_len=3, no_repeat_ngram=2)
    bs = _mk(torch.float32, length_penalty=ALPHA, constraints=cons)
    res = bs.decode(*s["enc"], bos=s["bos"], eos=s["eos"], n_best=N_BM)
    names = [op.name for op in bs.steps[(1, True)].ops]
    assert names[-2:] == ["univl_decode_constrain", "univl_beam_pool_step"]
    driver = _mk(torch.float32, constraints=cons)
    tok, lens, fin = _result_against_ref(res, _reference_run(torch.float32, ALPHA, driver=driver), N_BM)
    assert (lens[fin == 1] >= 4).all()
    for inst in res.hypotheses():
        for h in inst:
            grams = [tuple(h[j:j + 2]) for j in range(len(h) - 1)]
            assert len(set(grams)) == len(grams), h


def test_set_length_penalty_needs_no_new_capture(monkeypatch):
    """F (v).  set_length_penalty rewrites the device table and the mode word: another penalty and mode give their reference run, the
    first ones give the first result back, with no graph captured in between."""
    s = _case(torch.float32)
    bs, first = _pooled(torch.float32)
    other = _reference_run(torch.float32, 0.0, True)
    captures = []
    enter = torch.cuda.graph.__enter__

    def counting(self):
        captures.append(1)
        return enter(self)
    monkeypatch.setattr(torch.cuda.graph, "__enter__", counting)
    bs.set_length_penalty(0.0, early_stopping=True)
    _result_against_ref(bs.decode(*s["enc"], bos=s["bos"], eos=s["eos"], n_best=N_BM), other, N_BM)
    bs.set_length_penalty(ALPHA, early_stopping=False)
    _same(bs.decode(*s["enc"], bos=s["bos"], eos=s["eos"], n_best=N_BM), first)
    assert captures == []
    for bad in (-1.0, float("nan"), None):
        with pytest.raises(ValueError):
            bs.set_length_penalty(bad)
    with pytest.raises(ValueError):
        s["plain"].set_length_penalty(1.0)


def test_no_penalty_builds_the_plans_of_before():
    """F (vi).  length_penalty=None: the entry names of every position's plan equal those of a session built without the argument,
    there is no pool buffer, and decode() returns the BeamResult of before; the pooled session's plans differ in the tail alone."""
    s = _case(torch.float32)
    plain, none = s["plain"], _mk(torch.float32, length_penalty=None, early_stopping=False)
    a = plain.decode(*s["enc"], bos=s["bos"], eos=s["eos"], n_best=N_BM)
    b = none.decode(*s["enc"], bos=s["bos"], eos=s["eos"], n_best=N_BM)
    for f in ("tokens", "scores", "lengths", "parents", "step_tokens", "step_scores"):
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    assert not isinstance(b, PoolBeamResult) and not hasattr(none, "pool") and not hasattr(none, "pool_w")
    keys = [(t, True) for t in range(T_DEC)]
    pooled, _ = _pooled(torch.float32)
    for k in keys:
        names = [op.name for op in plain.steps[k].ops]
        assert [op.name for op in none.steps[k].ops] == names and names[-1] == "univl_beam_step"
        assert [op.name for op in pooled.steps[k].ops] == names[:-1] + ["univl_beam_pool_step"]


def test_eval_caption_and_score_beams():
    """F (vii).  eval_caption(length_penalty=1.0) end to end on two tiny batches (2 + 1 items, the second with n_active): hyps take
    hypothesis 0, scores are the raw sums, lengths are per hypothesis.  score_beams accepts the result: the teacher-forced sum over
    a hypothesis's tokens, its end token included, is its raw score up to the cached step's tolerance of tests/test_score_gpu.py
    (2e-3 per position in fp32)."""
    s = _case(torch.float32)
    cfg = s["cfg"]
    order = ("input_ids", "attention_mask", "token_type_ids", "video", "video_mask", "pairs_masked_text", "pairs_token_labels",
             "masked_video", "video_labels_index", "input_caption_ids", "decoder_mask", "output_caption_ids")
    b = O.synthetic_batch(cfg, 3, seed=91)
    loader = [tuple(b[k][:2] for k in order), tuple(b[k][2:] for k in order)]
    tk = SynthTokenizer(cfg.vocab_size, special={"[SEP]": s["eos"], "[CLS]": s["bos"]})
    res = eval_caption(s["model"], loader, tk, n_bm=N_BM, n_best=2, max_len=T_DEC, length_penalty=1.0)
    assert res.session.pooled and res.session.length_penalty == 1.0 and len(res.hyps) == 3 and len(res.hyp_ids) == 3
    assert res.scores.shape == (3, 2) and res.lengths.shape == (3, 2)
    assert all(len(ids) == 2 and s["eos"] not in ids[0] and s["eos"] not in ids[1] for ids in res.hyp_ids)
    with pytest.raises(ValueError, match="session"):
        eval_caption(s["model"], loader, tk, session=res.session, length_penalty=1.0)
    bs, beams = _pooled(torch.float32)
    sc = CaptionScorer(s["model"], N_INST, cfg.max_words, cfg.max_frames, cfg.max_words, n_cand=N_BM)
    r = sc.score_beams(beams, *s["enc"], bos=s["bos"], eos=s["eos"], pad=0)
    assert torch.equal(r.seq_tokens.cpu().long(), beams.lengths.cpu().long())
    diff = (r.seq_logprob.cpu().double() - beams.scores.cpu().double()).abs() / beams.lengths.cpu().double()
    assert float(diff.max()) <= 2e-3, float(diff.max())


def test_value_errors():
    """F (viii).  The ValueErrors of the host interface, on a real model."""
    for kw in (dict(length_penalty=-0.5), dict(length_penalty=float("inf")), dict(length_penalty=1.0, beam_groups=2),
               dict(length_penalty=1.0, beam_step="host"), dict(early_stopping=True)):
        with pytest.raises(ValueError):
            _mk(torch.float32, **kw)
    with pytest.raises(ValueError, match="out of scope"):
        _mk(torch.float32, length_penalty=1.0, beam_groups=2)
