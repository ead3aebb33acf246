"""Diverse beam search on the device (csrc/beam.hip: univl_beam_group_step) and the group mode of univl_amd.decode.CaptionBeamSearch.

A  the kernel against the numpy reference (tests/group_beam_ref.py, brute force over all V columns), bit for bit, on quarter-valued
   log-probabilities: every sum and penalty is exact and equal values are plentiful, so the tie rule decides most places;
B  the edge of the sufficiency argument: n_bm = G = 8, identical rows, where group g needs entry g of a row's top-8 list;
C  the two identities against univl_beam_step;  D  frozen groups over four positions;  E  diversity_dev under one captured graph;
F  the argument range;  G  sessions."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import univl_oracle as O
from group_beam_ref import F32, GroupBeamRef
from make_golden import case_config

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from univl_amd import _lib, ops
    from univl_amd.constrain import DecodeConstraints
    from univl_amd.decode import CaptionBeamSearch
    from univl_amd.ops import beam_group_step              # the feature: without it this file fails at import
    from test_model_gpu import build

DEV = "cuda"
TMAX = 4
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
OUT = ("scores", "tokens", "src", "done", "length", "hist_parents", "hist_tokens", "hist_scores")


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
def _buffers(lp, n, nb, G, scores=None, done=None, length=None, tokens=None, Tmax=TMAX):
    """Device buffers of one call; src and the history pre-filled with the marker -7 (the reference's marker too)."""
    P = n * G
    z = lambda v, dt: torch.as_tensor(np.asarray(v), dtype=dt).to(DEV).contiguous()
    return dict(lp=torch.as_tensor(lp).to(DEV),
                scores=z(np.zeros((n, nb)) if scores is None else scores, torch.float32),
                done=z(np.zeros(P) if done is None else done, torch.uint8), length=z(np.zeros(P) if length is None else length, torch.int32),
                tokens=z(np.zeros(n * nb) if tokens is None else np.asarray(tokens).reshape(-1), torch.int64),
                src=torch.full((n * nb,), -7, dtype=torch.int32, device=DEV),
                hist_parents=torch.full((Tmax, n, nb), -7, dtype=torch.int32, device=DEV),
                hist_tokens=torch.full((Tmax, n, nb), -7, dtype=torch.int32, device=DEV),
                hist_scores=torch.full((Tmax, n, nb), -7.0, device=DEV), ws=ops.beam_ws(n, nb, DEV))


def _state(d):
    return {k: v for k, v in d.items() if k != "lp"}


def _against_ref(d, ref):
    """Every output of the device against the reference's (history rows not yet written keep the marker -7 on both sides)."""
    n, nb = ref.n, ref.nb
    got = {k: d[k].cpu().numpy() for k in OUT}
    assert np.array_equal(_bits(got["scores"]), _bits(ref.scores)), "scores"
    assert np.array_equal(got["tokens"].reshape(n, nb), ref.tokens), "tokens"
    assert np.array_equal(got["done"], ref.done) and np.array_equal(got["length"].astype(np.int64), ref.length), "done / length"
    assert np.array_equal(got["hist_parents"].astype(np.int64), ref.hist_par), "hist_parents"
    assert np.array_equal(got["hist_tokens"].astype(np.int64), ref.hist_tok), "hist_tokens"
    assert np.array_equal(_bits(got["hist_scores"]), _bits(ref.hist_sc)), "hist_scores"
    assert np.array_equal(got["src"].astype(np.int64), ref.src), "src"
    assert got["src"].min() >= 0 and got["src"].max() < n * nb


def _quarter(seed, n, nb, G, V, ld, first):
    """Quarter-valued lp in [-50, 0), quarter-valued scores, one frozen group (with its own tokens) at a later step, padding columns
    at +1e30 that must never win."""
    rng = np.random.RandomState(seed)
    lp = (rng.randint(-200, 0, size=(n * nb, ld)) * 0.25).astype(F32)
    lp[:, V:] = 1e30
    scores = np.zeros((n, nb), dtype=F32) if first else (-rng.randint(0, 16, size=(n, nb)) * 0.25).astype(F32)
    done = np.zeros(n * G, dtype=np.uint8)
    if not first:
        done[1] = 1
    tokens = rng.randint(0, V, size=(n, nb))
    length = rng.randint(1, 3, size=n * G)
    return lp, scores, done, tokens, length


@pytest.mark.parametrize("first", [True, False], ids=["first", "later"])
@pytest.mark.parametrize("lam", [0.0, 0.5, 2.0])
@pytest.mark.parametrize("G", [1, 2, 3, 6])
@pytest.mark.parametrize("V,ld,offset", [(30522, 30528, 0), (37, 40, 0), (37, 40, 1)], ids=["vec8slices", "vec37", "scalar37"])
def test_kernel_matches_reference(V, ld, offset, G, lam, first):
    """A.  n_inst = 3, n_bm = 6.  V = 30522 / ld = 30528: eight slices, 16-byte loads.  V = 37 / ld = 40, V barely above n_bm: once
    aligned (16-byte loads whose last word is partly padding) and once from a buffer that starts 4 bytes off 16-byte alignment, the
    scalar path.  The end token is the one instance 0's first group emits on top, so a done byte is set by the call."""
    n, nb = 3, 6
    lp, scores, done, tokens, length = _quarter(7 * G + int(lam * 4) + (100 if first else 0) + V % 11, n, nb, G, V, ld, first)
    t = 0 if first else 2
    mk = lambda eos: GroupBeamRef(n, nb, G, V, TMAX, lam, eos=eos, scores=scores, tokens=tokens, done=done, length=length)
    dry = mk(-1)
    dry.step(lp, t, first=first)
    eos = int(dry.tokens[0, 0])
    ref = mk(eos)
    ref.step(lp, t, first=first)
    assert ref.done[0] == 1
    d = _buffers(lp, n, nb, G, scores, done, length, tokens)
    if offset:
        flat = torch.full((n * nb * ld + offset,), 1e30, device=DEV)
        d["lp"] = flat[offset:].view(n * nb, ld)
        d["lp"].copy_(torch.as_tensor(lp))
        assert d["lp"].data_ptr() % 16 == 4 * offset
    ops.beam_group_step(d["lp"], V, n, nb, G, t, diversity=lam, eos=eos, first_step=first, **_state(d))
    torch.cuda.synchronize()
    _against_ref(d, ref)
    assert int(d["tokens"].max()) < V                          # no padding column won


def _edge_rows(V, ld, cols, n):
    """Eight identical rows per instance: background -50, strictly descending values -1 .. -8 at cols[0 .. 7]."""
    row = np.full(ld, -50.0, dtype=F32)
    row[V:] = 1e30
    for j, c in enumerate(cols):
        row[c] = -1.0 - j
    return np.tile(row, (n * 8, 1))


@pytest.mark.parametrize("name,n,cols", [
    ("slices", 1, [7 + 3816 * j for j in (3, 0, 7, 1, 6, 2, 5, 4)]),          # one winner in each of the eight slices of 3816 columns
    ("one_word", 1, [100 + j for j in (0, 1, 2, 3, 4, 5, 6, 7)]),             # two adjacent 16-byte words of one slice
    ("one_thread", 128, [13 + 1024 * j for j in (2, 0, 5, 1, 7, 3, 6, 4)]),   # 1024 rows: one slice, the stride of ONE thread's loads
])
def test_edge_of_the_sufficiency_argument(name, n, cols):
    """B.  n_bm = G = 8, k' = 1, the eight rows of an instance identical, lambda = 100: every earlier group's winner drops below the
    background, so group g must take the column of rank g of its row and group 7 the LAST entry of the row's top-8 list.  A list of
    fewer than n_bm entries per row, per slice or per thread goes wrong here."""
    V, ld, nb, G = 30522, 30528, 8, 8
    lp = _edge_rows(V, ld, cols, n)
    d = _buffers(lp, n, nb, G)
    ops.beam_group_step(d["lp"], V, n, nb, G, 1, diversity=100.0, **_state(d))
    torch.cuda.synchronize()
    tok = d["tokens"].cpu().view(n, nb)
    assert tok[0].tolist() == cols and bool((tok == tok[0]).all())
    assert d["scores"].cpu().view(n, nb)[n - 1].tolist() == [-1.0 - j for j in range(8)]
    ref = GroupBeamRef(1, nb, G, V, TMAX, 100.0)
    ref.step(lp[:8], 1)
    assert ref.tokens[0].tolist() == cols
    assert bool((d["hist_parents"][1] == 0).all()) and bool((d["hist_tokens"][1].cpu() == torch.tensor(cols)).all())
    assert torch.equal(d["src"].cpu().long(), torch.arange(n * nb))              # every group continues its own single beam
    assert d["length"].cpu().tolist() == [1] * (n * G)


# ------------------------------------------------------------------------------------------------ C: identities
def _same_outputs(a, b):
    for k in OUT:
        assert torch.equal(a[k].reshape(-1), b[k].reshape(-1)), k


@pytest.mark.parametrize("first", [True, False], ids=["first", "later"])
@pytest.mark.parametrize("V,ld", [(30522, 30528), (37, 40)])
def test_one_group_is_the_plain_step(V, ld, first):
    """C (i).  n_groups = 1, any penalty: every output bit-identical to univl_beam_step."""
    n, nb = 3, 6
    lp, scores, done, tokens, length = _quarter(11 + V % 7, n, nb, 1, V, ld, first)
    t, eos = (0 if first else 2), int(tokens[0, 0])
    a, b = (_buffers(lp, n, nb, 1, scores, done, length, tokens) for _ in range(2))
    ops.beam_group_step(a["lp"], V, n, nb, 1, t, diversity=2.0, eos=eos, first_step=first, **_state(a))
    ops.beam_step(b["lp"], V, n, nb, t, eos=eos, first_step=first, **_state(b))
    torch.cuda.synchronize()
    _same_outputs(a, b)


@pytest.mark.parametrize("first", [True, False], ids=["first", "later"])
@pytest.mark.parametrize("nb,G", [(6, 2), (6, 3), (6, 6), (8, 2), (8, 8)])
def test_no_penalty_is_the_plain_step_on_pseudo_instances(nb, G, first):
    """C (ii).  diversity = 0: every output bit-identical to univl_beam_step called with (n_inst * G, k') on the same buffers."""
    n, V, ld = 3, 30522, 30528
    lp, scores, done, tokens, length = _quarter(23 + nb + G, n, nb, G, V, ld, first)
    t, eos = (0 if first else 2), int(tokens[0, 0])
    a, b = (_buffers(lp, n, nb, G, scores, done, length, tokens) for _ in range(2))
    ops.beam_group_step(a["lp"], V, n, nb, G, t, diversity=0.0, eos=eos, first_step=first, **_state(a))
    kp = nb // G
    sb = _state(b)
    for k in ("hist_parents", "hist_tokens", "hist_scores"):
        sb[k] = sb[k].view(TMAX, n * G, kp)
    sb["ws"] = ops.beam_ws(n * G, kp, DEV)
    ops.beam_step(b["lp"], V, n * G, kp, t, eos=eos, first_step=first, **sb)
    torch.cuda.synchronize()
    _same_outputs(a, b)


# ------------------------------------------------------------------------------------------------ D: frozen groups
def test_frozen_groups_over_four_positions():
    """D.  n_bm = 4 in two groups, four positions on device-resident state.  The end token is the one group 0 of instance 0 emits on
    top at t = 1: from t = 2 its state and history repeat and it adds nothing to c(v) -- the reference that keeps counting its
    tokens (an unended run) gives group 1 other beams.  Instance 2 is an idle slot: both groups preset done, skipped entirely."""
    n, nb, G, V, ld, T, lam = 3, 4, 2, 37, 40, 4, 2.0
    rng = np.random.RandomState(5)
    lps = [(rng.randint(-12, 0, size=(n * nb, ld)) * 0.25).astype(F32) for _ in range(T)]
    for x in lps:
        x[:, V:] = 1e30
    done0 = np.array([0, 0, 0, 0, 1, 1], dtype=np.uint8)
    idle_tok = np.arange(n * nb).reshape(n, nb) % V

    def run(eos, upto=T):
        r = GroupBeamRef(n, nb, G, V, T, lam, eos=eos, done=done0, tokens=idle_tok)
        for t in range(upto):
            r.step(lps[t], t)
        return r
    eos = int(run(-1, 2).hist_tok[1, 0, 0])
    ref, unended = run(eos), run(-1)
    assert ref.done[0] == 1 and ref.length[0] == 2 and ref.length[1] == T          # group 0 ends at t = 1, group 1 runs every position
    assert not np.array_equal(ref.hist_tok[2:, 0, 2:], unended.hist_tok[2:, 0, 2:])          # group 0's silence is visible in group 1
    d = _buffers(lps[0], n, nb, G, done=done0, tokens=idle_tok, Tmax=T)
    for t in range(T):
        d["lp"].copy_(torch.as_tensor(lps[t]))
        ops.beam_group_step(d["lp"], V, n, nb, G, t, diversity=lam, eos=eos, **_state(d))
    torch.cuda.synchronize()
    _against_ref(d, ref)
    hp, ht, hs = (d[k].cpu() for k in ("hist_parents", "hist_tokens", "hist_scores"))
    for t in (2, 3):
        assert hp[t, 0, :2].tolist() == [0, 1] and torch.equal(ht[t, 0, :2], ht[1, 0, :2]) and torch.equal(hs[t, 0, :2], hs[1, 0, :2])
    assert d["length"].cpu().tolist()[4:] == [0, 0] and d["tokens"].cpu().view(n, nb)[2].tolist() == idle_tok[2].tolist()
    assert bool((hp[:, 2] == torch.tensor([0, 1, 0, 1])).all())


# ------------------------------------------------------------------------------------------------ E: diversity_dev
def test_diversity_dev_serves_two_penalties_under_one_graph():
    """E.  One captured launch pair, the penalty a device word: 0.25 and 4.0 each give their own reference result; the descriptor's
    own field (a value that would be refused without the word) is not read.  The six rows of an instance are identical and the scores
    zero, so every group wants the same tokens and the size of the penalty decides how far the later groups move away."""
    n, nb, G, V, ld, t = 3, 6, 3, 37, 40, 2
    rng = np.random.RandomState(41)
    lp = np.tile((rng.randint(-40, 0, size=(n, 1, ld)) * 0.25).astype(F32), (1, nb, 1)).reshape(n * nb, ld)
    lp[:, V:] = 1e30
    scores, done, tokens, length = np.zeros((n, nb), dtype=F32), np.zeros(n * G), np.zeros((n, nb)), np.zeros(n * G)
    d = _buffers(lp, n, nb, G, scores, done, length, tokens)
    keep = {k: d[k].clone() for k in OUT}
    word = torch.zeros(1, device=DEV)
    desc = ops.beam_group_step_desc(d["lp"], V, n, nb, G, t, diversity=-1.0, diversity_dev=word, **_state(d))
    L = _lib.lib()
    assert L.univl_beam_group_step(C.byref(desc), ops._stream()) == 0          # once outside the capture; the state is restored below
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        assert L.univl_beam_group_step(C.byref(desc), ops._stream()) == 0
    results = []
    for lam in (0.25, 4.0):
        for k in OUT:
            d[k].copy_(keep[k])
        word.fill_(lam)
        g.replay()
        torch.cuda.synchronize()
        ref = GroupBeamRef(n, nb, G, V, TMAX, lam, scores=scores, tokens=tokens, done=done, length=length)
        ref.step(lp, t, first=False)
        _against_ref(d, ref)
        results.append(d["tokens"].clone())
    assert not torch.equal(results[0], results[1])


# ------------------------------------------------------------------------------------------------ F: argument range
def test_argument_range():
    """F.  Outside the range: UNIVL_EINVAL with a message, and nothing launched -- the outputs keep their sentinels."""
    n, nb, G, V, ld = 2, 6, 3, 64, 64
    lp, scores, done, tokens, length = _quarter(3, n, nb, G, V, ld, False)
    d = _buffers(lp, n, nb, G, scores, done, length, tokens)
    keep = {k: d[k].clone() for k in OUT}
    L = _lib.lib()

    def rc(**kw):
        desc = ops.beam_group_step_desc(d["lp"], V, n, nb, G, 1, diversity=0.5, **_state(d))
        for k, v in kw.items():
            setattr(desc, k, v)
        r = L.univl_beam_group_step(C.byref(desc), ops._stream())
        torch.cuda.synchronize()
        return r

    EINVAL = -1
    for kw in (dict(n_groups=0), dict(n_groups=-1), dict(n_groups=4), dict(n_groups=5), dict(n_groups=7), dict(n_groups=12),
               dict(diversity=-0.5), dict(diversity=float("nan")), dict(diversity=float("inf")), dict(diversity=-float("inf")),
               dict(n_bm=0), dict(n_bm=9), dict(n_bm=-3), dict(V=5), dict(V=0), dict(ld=V - 1), dict(n_inst=0), dict(n_inst=-3),
               dict(t=TMAX), dict(t=-1), dict(Tmax=0), dict(ws_bytes=n * nb * 8 * nb * 8 - 1), dict(ws=None), dict(lp=None),
               dict(scores=None), dict(done=None), dict(length=None), dict(tokens=None), dict(src=None), dict(hist_parents=None),
               dict(hist_tokens=None), dict(hist_scores=None)):
        assert rc(**kw) == EINVAL, kw
        assert b"univl_beam_group_step" in L.univl_last_error()
    assert L.univl_beam_group_step(None, ops._stream()) == EINVAL
    for k in OUT:
        assert torch.equal(d[k], keep[k]), k                   # nothing was launched
    assert rc() == 0 and rc(n_groups=1) == 0 and rc(n_groups=6) == 0 and rc(diversity=0.0) == 0
    word = torch.full((1,), 0.25, device=DEV)
    assert rc(diversity=-1.0, diversity_dev=C.c_void_p(word.data_ptr())) == 0          # the word is read instead of the field
    assert not torch.equal(d["hist_tokens"], keep["hist_tokens"])


# ------------------------------------------------------------------------------------------------ G: sessions
N_INST, N_BM, GROUPS, T_DEC, LAM = 2, 4, 2, 6, 0.5
FIELDS = ("tokens", "scores", "lengths", "parents", "step_tokens", "step_scores")


@functools.lru_cache(maxsize=None)
def _case(dtype):
    g = np.load(os.path.join(GOLDEN, "beam_caption_small.npz"))
    cfg, _, _ = case_config("caption_small")
    model, _ = build(cfg, dtype)
    model.eval()
    d = {k: v.to(DEV) for k, v in O.synthetic_batch(cfg, N_INST, seed=int(g["data_seed"])).items()}
    with torch.no_grad():
        so, vo = model.get_sequence_visual_output(d["input_ids"], d["token_type_ids"], d["attention_mask"], d["video"], d["video_mask"])
    enc = (so, vo, d["attention_mask"].view(N_INST, -1), d["video_mask"].view(N_INST, -1))
    return dict(cfg=cfg, model=model, bos=int(g["bos"]), eos=int(g["eos2"]), enc=enc)


def _mk(dtype, **kw):
    s = _case(dtype)
    return CaptionBeamSearch(s["model"], N_INST, s["cfg"].max_words, s["cfg"].max_frames, n_bm=N_BM, max_len=T_DEC, use_graphs=True, **kw)


@functools.lru_cache(maxsize=None)
def _grouped(dtype):
    """The group session of the tests below and its decode of the case at LAM (n_best = k')."""
    s = _case(dtype)
    bs = _mk(dtype, beam_groups=GROUPS, diversity_penalty=LAM)
    return bs, bs.decode(*s["enc"], bos=s["bos"], eos=s["eos"], n_best=N_BM // GROUPS)


def _same(a, b):
    for f in FIELDS:
        assert torch.equal(getattr(a, f), getattr(b, f)), f


def _reference_run(dtype, lam):
    """The session's own log-probabilities, position by position through step_logprobs, with the numpy reference doing the search."""
    s = _case(dtype)
    bs, _ = _grouped(dtype)
    bs.encode(*s["enc"])
    ref = GroupBeamRef(N_INST, N_BM, GROUPS, bs.V, T_DEC, lam, eos=s["eos"], tokens=np.full((N_INST, N_BM), s["bos"]))
    for t in range(T_DEC):
        lp = bs.step_logprobs(t, torch.from_numpy(ref.tokens).to(DEV), torch.from_numpy(ref.src).to(DEV) if t > 0 else None)
        ref.step(lp.cpu().numpy(), t)
    return ref


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_session_matches_reference_run(dtype):
    """G (i).  decode() of a group session against the reference run on the same session's rows: history, hypotheses, scores and
    per-group lengths bit for bit; the shapes of the group-major result; captions() and hypotheses() cut at each group's length."""
    s = _case(dtype)
    bs, res = _grouped(dtype)
    ref = _reference_run(dtype, LAM)
    kp = N_BM // GROUPS
    tok, sc, ln = ref.hypotheses(kp)
    assert res.groups == GROUPS and res.tokens.shape == (N_INST, N_BM, T_DEC) and res.scores.shape == (N_INST, N_BM)
    assert res.lengths.shape == (N_INST, GROUPS)
    assert np.array_equal(res.parents.cpu().numpy().astype(np.int64), ref.hist_par)
    assert np.array_equal(res.step_tokens.cpu().numpy().astype(np.int64), ref.hist_tok)
    assert np.array_equal(_bits(res.step_scores.cpu().numpy()), _bits(ref.hist_sc))
    assert np.array_equal(res.tokens.cpu().numpy().astype(np.int64), tok)
    assert np.array_equal(_bits(res.scores.cpu().numpy()), _bits(sc))
    assert np.array_equal(res.lengths.cpu().numpy().astype(np.int64), ln)
    hyps = res.hypotheses()
    cap, cap_len = res.captions(s["eos"], -1)
    assert cap.shape == res.tokens.shape and cap_len.shape == res.scores.shape
    for i in range(N_INST):
        for j in range(N_BM):
            want = [int(v) for v in tok[i, j, :ln[i, j // kp]]]
            assert hyps[i][j] == want
            cut = want.index(s["eos"]) if s["eos"] in want else len(want)
            assert int(cap_len[i, j]) == cut and cap[i, j, :cut].tolist() == want[:cut] and bool((cap[i, j, cut:] == -1).all())
    sc_t = res.scores.view(N_INST, GROUPS, kp)
    assert bool((sc_t[:, :, 1:] <= sc_t[:, :, :-1]).all())                         # beam 0 of a group is its best
    with pytest.raises(ValueError):
        bs.decode(*s["enc"], bos=s["bos"], eos=s["eos"], n_best=kp + 1)
    with pytest.raises(ValueError):
        _mk(dtype, beam_groups=GROUPS, beam_step="host")


def test_one_group_is_the_default_session():
    """G (ii).  beam_groups = 1 returns what a session built without the argument returns, from plans with the same launch names and
    count, and has no penalty word."""
    s = _case(torch.float32)
    plain, one = _mk(torch.float32), _mk(torch.float32, beam_groups=1, diversity_penalty=3.0)
    a = plain.decode(*s["enc"], bos=s["bos"], eos=s["eos"], n_best=N_BM)
    b = one.decode(*s["enc"], bos=s["bos"], eos=s["eos"], n_best=N_BM)
    _same(a, b)
    assert b.groups == 1 and b.lengths.shape == (N_INST,) and not hasattr(one, "diversity_dev")
    assert sorted(plain.steps) == sorted(one.steps) and len(plain.steps) == T_DEC
    for k in plain.steps:
        assert [op.name for op in plain.steps[k].ops] == [op.name for op in one.steps[k].ops]
    grouped, _ = _grouped(torch.float32)                       # the group session: the same count, the tail renamed
    for k in plain.steps:
        names, gnames = [op.name for op in plain.steps[k].ops], [op.name for op in grouped.steps[k].ops]
        assert names[-1] == "univl_beam_step" and gnames == names[:-1] + ["univl_beam_group_step"]
    with pytest.raises(ValueError):
        one.set_diversity(0.5)


def test_partial_batch_in_group_mode():
    """G (iii).  n_active = 1: the result is the first instance of the full batch; the idle slot's groups are all preset done."""
    s = _case(torch.float32)
    bs, full = _grouped(torch.float32)
    so, vo, am, vm = s["enc"]
    part = bs.decode(so[:1], vo[:1], am[:1], vm[:1], bos=s["bos"], eos=s["eos"], n_best=N_BM // GROUPS, n_active=1)
    assert part.tokens.shape[0] == 1 and part.lengths.shape == (1, GROUPS)
    for f in ("tokens", "scores", "lengths"):
        assert torch.equal(getattr(part, f), getattr(full, f)[:1]), f
    for f in ("parents", "step_tokens", "step_scores"):
        assert torch.equal(getattr(part, f), getattr(full, f)[:, :1]), f
    assert bs.done.cpu().tolist()[GROUPS:] == [1] * GROUPS and bs.length.cpu().tolist()[GROUPS:] == [0] * GROUPS
    _same(bs.decode(*s["enc"], bos=s["bos"], eos=s["eos"], n_best=N_BM // GROUPS), full)      # and the full batch again


def test_group_mode_under_ngram_blocking():
    """G (iv).  With DecodeConstraints(no_repeat_ngram=2) (done_stride = k' in the constraint launch) no hypothesis of any group
    repeats a bigram, and the run equals the reference run on constrained rows."""
    s = _case(torch.float32)
    bs = _mk(torch.float32, beam_groups=GROUPS, diversity_penalty=LAM, constraints=DecodeConstraints(no_repeat_ngram=2))
    res = bs.decode(*s["enc"], bos=s["bos"], eos=-1, n_best=N_BM // GROUPS)
    names = [op.name for op in bs.steps[(1, True)].ops]
    assert names[-2:] == ["univl_decode_constrain", "univl_beam_group_step"]
    for inst in res.hypotheses():
        assert len(inst) == N_BM
        for h in inst:
            grams = [tuple(h[j:j + 2]) for j in range(len(h) - 1)]
            assert len(h) == T_DEC and len(set(grams)) == len(grams), h


def test_set_diversity_needs_no_new_capture(monkeypatch):
    """G (v).  set_diversity rewrites the device word: another penalty gives that penalty's reference run, and the first one gives
    the first result back, with no graph captured in between."""
    s = _case(torch.float32)
    bs, first = _grouped(torch.float32)
    other = _reference_run(torch.float32, 4.0)
    captures = []
    enter = torch.cuda.graph.__enter__

    def counting(self):
        captures.append(1)
        return enter(self)
    monkeypatch.setattr(torch.cuda.graph, "__enter__", counting)
    kp = N_BM // GROUPS
    bs.set_diversity(4.0)
    got = bs.decode(*s["enc"], bos=s["bos"], eos=s["eos"], n_best=kp)
    assert np.array_equal(got.tokens.cpu().numpy().astype(np.int64), other.hypotheses(kp)[0])
    assert np.array_equal(got.step_tokens.cpu().numpy().astype(np.int64), other.hist_tok)
    assert not torch.equal(got.step_tokens, first.step_tokens)
    bs.set_diversity(LAM)
    _same(bs.decode(*s["enc"], bos=s["bos"], eos=s["eos"], n_best=kp), first)
    assert captures == []
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError):
            bs.set_diversity(bad)
