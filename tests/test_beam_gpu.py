"""Device-side beam step and hypothesis walk-back (csrc/beam.hip: univl_beam_step, univl_beam_backtrack) and the decode() surface
of univl_amd.decode.CaptionBeamSearch built on them.

A  the kernel against torch.topk on synthetic log-probabilities free of exact ties;
B  crafted inputs: the tie rule (equal values: lower flat index b * V + v first), several winners in one thread / one 16-byte
   word, winners in the last V % 4 columns and in column 0, every argument-range violation;
C  whole decoding runs, beam_step="device" against beam_step="host" (the ATen bookkeeping this class had before);
D  no host involvement inside decode(); the result does not depend on sync_every;
E  n_best hypotheses against a Python walk-back of the returned history."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import univl_oracle as O
from make_golden import case_config

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from univl_amd import _lib, ops
    from univl_amd.decode import CaptionBeamSearch
    from test_model_gpu import build

DEV = "cuda"
TMAX = 4


@pytest.fixture(autouse=True)
def _deterministic_mode():
    """Fixed-order sums in the decoder's products (include/univl_hip.h: univl_set_deterministic), the mode the parity tests run
    in: C compares two sessions bit for bit, which split-K sums met in hardware order would not allow.  The beam kernels
    themselves have no such sums."""
    import univl_amd
    was = univl_amd.deterministic()
    univl_amd.set_deterministic(True)
    yield
    univl_amd.set_deterministic(was)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ------------------------------------------------------------------------------------------------ kernel harness
def _state(lp, scores, done, ids, length, n, nb, V):
    """Device buffers of one univl_beam_step call; history and outputs pre-filled with markers."""
    d = dict(lp=lp.to(DEV), scores=scores.to(DEV).contiguous(), done=done.to(torch.uint8).to(DEV), length=length.to(torch.int32).to(DEV),
             tokens=ids.to(torch.int64).reshape(-1).to(DEV), src=torch.full((n * nb,), -7, dtype=torch.int32, device=DEV),
             hist_parents=torch.full((TMAX, n, nb), -7, dtype=torch.int32, device=DEV),
             hist_tokens=torch.full((TMAX, n, nb), -7, dtype=torch.int32, device=DEV),
             hist_scores=torch.full((TMAX, n, nb), -7.0, device=DEV), ws=ops.beam_ws(n, nb, DEV))
    return d


def _run(d, n, nb, V, t, eos):
    ops.beam_step(d["lp"], V, n, nb, t, eos=eos, **{k: v for k, v in d.items() if k != "lp"})
    torch.cuda.synchronize()


def _expect(lp, scores, done, ids, length, n, nb, V, first, eos, k):
    """The contract restated with torch on the CPU: candidates in fp32, a STABLE descending sort (equal values: lower flat index
    first).  Returns the top-k values / flat indices and the state after the step."""
    x = lp.view(n, nb, -1)[:, :, :V]
    cand = x[:, 0, :] if first else (x + scores[:, :, None]).reshape(n, nb * V)
    vals, flat = torch.sort(cand, dim=1, descending=True, stable=True)
    vals, flat = vals[:, :k], flat[:, :k]
    act = ~done.bool()
    ident = torch.arange(nb).expand(n, nb)
    new_scores = torch.where(act[:, None], vals[:, :nb], scores)
    parents = torch.where(act[:, None], flat[:, :nb] // V, ident)
    tokens = torch.where(act[:, None], flat[:, :nb] % V, ids.view(n, nb))
    new_len = length + act.to(length.dtype)
    new_done = done.bool() | (act & (tokens[:, 0] == eos))
    return vals, flat, new_scores, parents, tokens, new_len, new_done


def _check(d, exp, n, nb, t):
    vals, flat, sc, par, tok, ln, dn = exp
    assert torch.equal(d["scores"].cpu().view(n, nb), sc)                      # bitwise: one fp32 addition, nothing re-associated
    assert torch.equal(d["tokens"].cpu().view(n, nb), tok)
    assert torch.equal(d["src"].cpu().view(n, nb).long(), torch.arange(n)[:, None] * nb + par)
    assert torch.equal(d["length"].cpu().long(), ln.long())
    assert torch.equal(d["done"].cpu().bool(), dn)
    assert torch.equal(d["hist_parents"][t].cpu().long(), par)
    assert torch.equal(d["hist_tokens"][t].cpu().long(), tok)
    assert torch.equal(d["hist_scores"][t].cpu(), sc)
    for r in range(TMAX):                                                      # the other history rows are not this call's
        if r != t:
            assert bool((d["hist_parents"][r] == -7).all()) and bool((d["hist_tokens"][r] == -7).all()) and bool((d["hist_scores"][r] == -7).all())


def _synthetic(n, nb, V, ld, first):
    g = torch.Generator().manual_seed(1000 * n + 100 * nb + V % 97 + (7 if first else 0))
    lp = torch.randn(n * nb, ld, generator=g) * 3.0 - 12.0
    lp[:, V:] = 1e30                                                           # padding columns must never be selected
    scores = -torch.rand(n, nb, generator=g).cumsum(1) * 4.0
    done = torch.tensor([(i % 3) == 1 for i in range(n)])
    ids = torch.randint(0, V, (n, nb), generator=g)
    length = torch.arange(n) % 3 + 1
    return lp, scores, done, ids, length


@pytest.mark.parametrize("first", [True, False], ids=["first", "later"])
@pytest.mark.parametrize("V,ld", [(30522, 30528), (1000, 1000), (8, 8)])
@pytest.mark.parametrize("nb", [1, 2, 5, 8])
@pytest.mark.parametrize("n", [1, 3, 16])
def test_beam_step_matches_topk(n, nb, V, ld, first):
    """A.  Synthetic log-probabilities; reference = torch.topk of lp[:, :, :V] + scores in fp32 with k = min(n_bm + 1, candidates),
    asserted free of exact ties among those k values (so topk's open tie order cannot matter); everything the step writes must
    equal it, bit for bit, and frozen instances keep their state."""
    lp, scores, done, ids, length = _synthetic(n, nb, V, ld, first)
    t = 0 if first else 2
    ncand = V if first else nb * V
    k = min(nb + 1, ncand)
    x = lp.to(DEV).view(n, nb, ld)[:, :, :V]
    cand = x[:, 0, :] if first else (x + scores.to(DEV)[:, :, None]).reshape(n, nb * V)
    tv, ti = cand.topk(k, dim=1, largest=True, sorted=True)
    tv, ti = tv.cpu(), ti.cpu()
    assert bool((tv[:, 1:] < tv[:, :-1]).all()), "the seeded input has an exact tie among its top k: choose another seed"
    eos = int(ti[0, 0] % V)                                                    # instance 0's top token: it finishes at this step
    exp = _expect(lp, scores, done, ids, length, n, nb, V, first, eos, k)
    assert torch.equal(exp[0], tv) and torch.equal(exp[1], ti)                 # the CPU restatement is torch.topk here (no ties)
    d = _state(lp, scores, done, ids, length, n, nb, V)
    _run(d, n, nb, V, t, eos)
    _check(d, exp, n, nb, t)
    frozen = done.bool()
    assert torch.equal(d["scores"].cpu().view(n, nb)[frozen], scores[frozen])
    assert torch.equal(d["tokens"].cpu().view(n, nb)[frozen], ids[frozen])
    assert torch.equal(d["length"].cpu().long()[frozen], length[frozen])
    assert bool(d["done"].cpu().bool()[0]) and exp[6][0]


def _crafted(n, nb, V, ld, plant, first=False):
    """A background of distinct, strictly decreasing values far below the planted ones; plant: [(instance, beam, column, value)].
    Scores are zero, so candidate values are the planted values exactly."""
    lp = (-50.0 - torch.arange(n * nb * ld, dtype=torch.float64) * 1e-4).to(torch.float32).view(n * nb, ld).clone()
    lp[:, V:] = 1e30
    for i, b, c, v in plant:
        lp[i * nb + b, c] = v
    scores = torch.zeros(n, nb)
    done = torch.zeros(n, dtype=torch.bool)
    ids = torch.zeros(n, nb, dtype=torch.int64)
    length = torch.zeros(n, dtype=torch.int64)
    t = 0 if first else 1
    exp = _expect(lp, scores, done, ids, length, n, nb, V, first, -1, nb)
    d = _state(lp, scores, done, ids, length, n, nb, V)
    _run(d, n, nb, V, t, -1)
    _check(d, exp, n, nb, t)
    return exp


def test_beam_step_tie_rule():
    """B (i).  Equal values at known flat indices, inside the kept set and straddling the n_bm-th place: lower flat index first."""
    V, ld, nb = 30522, 30528, 5
    plant = [(0, 3, 100, -1.0), (0, 1, 20000, -1.0), (0, 1, 5, -1.0),          # three equal values inside the kept set
             (0, 4, 7, -2.0), (0, 0, 30521, -2.0), (0, 2, 9, -2.0),            # three equal values for the two places left
             (1, 2, 4000, -3.0), (1, 2, 4001, -3.0), (1, 2, 3999, -3.0), (1, 0, 4000, -3.0), (1, 4, 0, -3.0), (1, 3, 30521, -3.0)]
    exp = _crafted(2, nb, V, ld, plant)
    assert exp[3][0].tolist() == [1, 1, 3, 0, 2] and exp[4][0].tolist() == [5, 20000, 100, 30521, 9]
    assert exp[3][1].tolist() == [0, 2, 2, 2, 3] and exp[4][1].tolist() == [4000, 3999, 4000, 4001, 30521]
    # the same at the first step (beam 0's row only; other rows' larger values must not be seen)
    plant = [(0, 0, 30000, -1.0), (0, 0, 3, -1.0), (0, 0, 1027, -1.0), (0, 0, 1024, -1.0), (0, 0, 8000, -1.0), (0, 0, 2, -1.0),
             (0, 1, 17, 5.0), (0, 4, 2, 5.0)]
    exp = _crafted(1, nb, V, ld, plant, first=True)
    assert exp[3][0].tolist() == [0] * 5 and exp[4][0].tolist() == [2, 3, 1024, 1027, 8000]


@pytest.mark.parametrize("nb", [5, 8])
def test_beam_step_winners_share_a_thread(nb):
    """B (ii).  The n_bm best values all in one row, at columns c, c + 256, c + 512, ... and at adjacent columns, so that they land
    in one thread / one 16-byte word of any reasonable layout: a per-thread top-1 shortcut fails here."""
    V, ld = 30522, 30528
    for stride in (256, 1024, 2048, 1):
        for c in (0, 13, 2048):
            plant = [(1, nb - 1, c + j * stride, -1.0 - 0.25 * ((j * 3) % nb)) for j in range(nb)]      # distinct values, shuffled order
            exp = _crafted(2, nb, V, ld, plant)
            assert sorted(exp[4][1].tolist()) == [c + j * stride for j in range(nb)] and exp[3][1].tolist() == [nb - 1] * nb
    plant = [(0, 0, 8 + j, -1.0 - j) for j in range(nb)]
    exp = _crafted(1, nb, V, ld, plant, first=True)
    assert exp[4][0].tolist() == [8 + j for j in range(nb)]


def test_beam_step_edge_columns():
    """B (iii).  The best values in the last V % 4 columns (the partly padded 16-byte word) and in column 0."""
    V, ld, nb = 30522, 30528, 5
    assert V % 4 == 2
    plant = [(0, 4, V - 1, -1.0), (0, 4, V - 2, -1.5), (0, 0, 0, -2.0), (0, 3, 0, -2.5), (0, 2, V - 1, -3.0)]
    exp = _crafted(1, nb, V, ld, plant)
    assert exp[3][0].tolist() == [4, 4, 0, 3, 2] and exp[4][0].tolist() == [V - 1, V - 2, 0, 0, V - 1]
    plant = [(0, 0, V - 1, -1.0), (0, 0, 0, -1.5), (0, 0, V - 2, -2.0), (0, 0, 1, -2.5), (0, 0, V - 3, -3.0)]
    exp = _crafted(1, nb, V, ld, plant, first=True)
    assert exp[4][0].tolist() == [V - 1, 0, V - 2, 1, V - 3]
    # a row stride that is not a multiple of 4 floats (the scalar path): same contract
    V, ld, nb = 1001, 1003, 3
    plant = [(1, 2, 1000, -1.0), (1, 0, 0, -1.5), (1, 1, 999, -2.0)]
    exp = _crafted(2, nb, V, ld, plant)
    assert exp[3][1].tolist() == [2, 0, 1] and exp[4][1].tolist() == [1000, 0, 999]


def test_beam_step_argument_range():
    """B (iv).  Outside 1 <= n_bm <= 8, n_bm <= V <= ld, n_inst >= 1, 0 <= t < Tmax, or with a short workspace / a null pointer:
    UNIVL_EINVAL and nothing launched -- never a wrong answer."""
    n, nb, V, ld = 2, 5, 64, 64
    lp, scores, done, ids, length = _synthetic(n, nb, V, ld, False)
    d = _state(lp, scores, done, ids, length, n, nb, V)
    L = _lib.lib()

    def rc(**kw):
        desc = ops.beam_step_desc(d["lp"], V, n, nb, 1, **{k: v for k, v in d.items() if k != "lp"})
        for k, v in kw.items():
            setattr(desc, k, v)
        r = L.univl_beam_step(C.byref(desc), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        return r

    assert rc() == 0
    EINVAL = -1
    for kw in (dict(n_bm=0), dict(n_bm=9), dict(n_bm=-1), dict(V=4), dict(V=0), dict(ld=V - 1), dict(n_inst=0), dict(n_inst=-3),
               dict(t=TMAX), dict(t=-1), dict(Tmax=0), dict(ws_bytes=n * nb * 8 * nb * 8 - 1), dict(ws=None), dict(lp=None),
               dict(scores=None), dict(done=None), dict(length=None), dict(tokens=None), dict(src=None), dict(hist_parents=None),
               dict(hist_tokens=None), dict(hist_scores=None)):
        assert rc(**kw) == EINVAL, kw
        assert L.univl_last_error()
    hp, ht = d["hist_parents"], d["hist_tokens"]
    args = lambda n_best, nb_=nb: (C.c_void_p(hp.data_ptr()), C.c_void_p(ht.data_ptr()), C.c_void_p(d["scores"].data_ptr()),
                                  C.c_void_p(d["length"].data_ptr()), n, nb_, n_best, TMAX, C.c_void_p(hp.data_ptr()),
                                  C.c_void_p(d["hist_scores"].data_ptr()), None)
    for a in (args(0), args(nb + 1), args(1, 9), args(1, 0)):
        assert L.univl_beam_backtrack(*a) == EINVAL


@pytest.mark.parametrize("entry", ["univl_beam_step", "univl_beam_group_step", "univl_beam_pool_step"])
def test_step_entry_points_share_the_common_argument_rule(entry):
    """The three step entry points refuse the same common arguments, each under its own name: UNIVL_EINVAL, univl_last_error()
    beginning with the entry point's name, and the state untouched (nothing launched).  No kernel runs in this test."""
    n, nb, G, V, ld, T = 2, 4, 2, 16, 16, 3
    units = n * G if entry == "univl_beam_group_step" else n
    z = lambda *shape, dt=torch.float32, fill=-7: torch.full(shape, fill, dtype=dt, device=DEV)
    state = dict(scores=z(n, nb), done=z(units, dt=torch.uint8, fill=0), length=z(units, dt=torch.int32, fill=1), tokens=z(n * nb, dt=torch.int64),
                 src=z(n * nb, dt=torch.int32), hist_parents=z(T, n, nb, dt=torch.int32), hist_tokens=z(T, n, nb, dt=torch.int32),
                 hist_scores=z(T, n, nb), ws=ops.beam_ws(n, nb, DEV))
    lp = torch.zeros(n * nb, ld, device=DEV)
    if entry == "univl_beam_step":
        desc = ops.beam_step_desc(lp, V, n, nb, 1, **state)
    elif entry == "univl_beam_group_step":
        desc = ops.beam_group_step_desc(lp, V, n, nb, G, 1, diversity=0.5, **state)
    else:
        pool = dict(ops.beam_pool(n, nb, DEV), w=ops.length_weights(0.6, T).to(DEV), params=torch.tensor([0, T], dtype=torch.int32, device=DEV))
        desc = ops.beam_pool_step_desc(lp, V, n, nb, 1, **state, **pool)
        state.update(pool)
    before = {k: v.clone() for k, v in state.items() if k != "ws"}
    L, EINVAL = _lib.lib(), -1
    need = n * nb * _lib.BEAM_SLICES * nb * 8
    assert desc.ws_bytes == need
    for field, bad in (("n_bm", 9), ("ld", V - 1), ("t", T), ("scores", None), ("ws_bytes", need - 1), ("ws", state["ws"].data_ptr() + 4)):
        good = getattr(desc, field)
        setattr(desc, field, bad)
        assert getattr(L, entry)(C.byref(desc), C.c_void_p(torch.cuda.current_stream().cuda_stream)) == EINVAL, field
        assert L.univl_last_error().decode().startswith(entry + ":"), (field, L.univl_last_error())
        setattr(desc, field, good)
    torch.cuda.synchronize()
    for k, v in before.items():
        assert torch.equal(state[k], v), k


# ------------------------------------------------------------------------------------------------ whole runs
def _walk_back(parents, tokens, t, i, k=0):
    hyp = []
    for j in range(t, -1, -1):
        hyp.append(int(tokens[j, i, k]))
        k = int(parents[j, i, k])
    return hyp[::-1]


@functools.lru_cache(maxsize=None)
def _session(case, dtype):
    """One model, one encoded batch and one decoding session per beam_step mode, shared by the tests of this file."""
    full = case == "caption_full"
    g = np.load(os.path.join(GOLDEN, "beam_caption_full.npz" if full else "beam_caption_small.npz"))
    cfg, _, dseed = case_config(case)
    n, nb, T = int(g["n_inst"]), int(g["n_bm"]), int(g["max_len"])
    model, _ = build(cfg, dtype)
    model.eval()
    d = {k: v.to(DEV) for k, v in O.synthetic_batch(cfg, n, seed=int(g["data_seed"])).items()}
    with torch.no_grad():
        so, vo = model.get_sequence_visual_output(d["input_ids"], d["token_type_ids"], d["attention_mask"], d["video"], d["video_mask"])
    enc = (so, vo, d["attention_mask"].view(n, -1), d["video_mask"].view(n, -1))
    mk = lambda mode: CaptionBeamSearch(model, n, cfg.max_words, cfg.max_frames, n_bm=nb, max_len=T, use_graphs=True, beam_step=mode)
    return dict(g=g, n=n, nb=nb, T=T, bos=int(g["bos"]), eos2=int(g["eos2"]), enc=enc, device=mk("device"), host=mk("host"))


@functools.lru_cache(maxsize=None)
def _compare_modes(case, dtype, with_eos):
    """C's comparison, kept for D.  Returns (tie-free instances, instances that ended at an exact tie, the device result)."""
    s = _session(case, dtype)
    eos = s["eos2"] if with_eos else -1
    rd = s["device"].decode(*s["enc"], bos=s["bos"], eos=eos)
    rh = s["host"].decode(*s["enc"], bos=s["bos"], eos=eos)
    n, nb = s["n"], s["nb"]
    assert rd.steps_run == rh.steps_run == s["T"]
    hd = [x.cpu() for x in (rd.parents, rd.step_tokens, rd.step_scores)]
    hh = [x.cpu() for x in (rh.parents, rh.step_tokens, rh.step_scores)]
    clean, tied = [], []
    for i in range(n):
        same = [all(torch.equal(a[t, i], b[t, i]) for a, b in zip(hd, hh)) for t in range(rd.steps_run)]
        if all(same):
            clean.append(i)
            continue
        t = same.index(False)
        sd, sh = hd[2][t, i], hh[2][t, i]
        # both modes saw the same log-probabilities up to here, so they can differ in nothing but the order of equal candidates
        assert torch.equal(sd, sh), (case, dtype, eos, i, t, sd.tolist(), sh.tolist())
        assert len(set(sd.tolist())) < nb or float(sd[-1]) in sh.tolist(), (case, dtype, eos, i, t, sd.tolist())
        tied.append((i, t))
    print("[beam modes %s %s eos=%d] instances ended at an exact tie: %d of %d %s" % (case, dtype, eos, len(tied), n, tied))
    for i in clean:
        assert torch.equal(rd.scores[i], rh.scores[i]) and torch.equal(rd.tokens[i], rh.tokens[i])
        assert int(rd.lengths[i]) == int(rh.lengths[i])
    return tuple(clean), tuple(tied), rd


@pytest.mark.parametrize("with_eos", [False, True], ids=["no_eos", "eos2"])
@pytest.mark.parametrize("case,dtype", [("caption_small", torch.float32), ("caption_full", torch.float32), ("caption_full", torch.bfloat16)],
                         ids=["small-fp32", "full-fp32", "full-bf16"])
def test_device_path_matches_host_path(case, dtype, with_eos):
    """C.  beam_step="device" against beam_step="host" over whole runs (caption_small 3 x 5; the bench shape 16 x 5 x 32 positions).
    Both modes run the same decoder launches, so the histories agree bit for bit until a position where candidates are EXACTLY
    equal (torch.topk's order is open there, the kernel's is fixed); there the two step-score rows must be bitwise equal, and the
    instance is not compared further.  At most 2 of 16 (1 of 3) instances may end that way: the reference's own golden at the bench
    shape has 1 exact tie among its 1660 + 2560 adjacent top-6 gaps, so 0 or 1 is the expectation."""
    clean, tied, _ = _compare_modes(case, dtype, with_eos)
    assert len(tied) <= (2 if case == "caption_full" else 1), tied


class _HostReads:
    """Counts Tensor.item / __bool__ / cpu / tolist calls (each one a host read of device data when made on a device tensor)."""

    def __init__(self, monkeypatch):
        self.calls = []
        for name in ("item", "__bool__", "cpu", "tolist"):
            orig = getattr(torch.Tensor, name)

            def wrapped(t, *a, _orig=orig, _name=name, **kw):
                if t.is_cuda:
                    self.calls.append(_name)
                return _orig(t, *a, **kw)
            monkeypatch.setattr(torch.Tensor, name, wrapped)


def test_decode_has_no_host_involvement(monkeypatch):
    """D (first half).  With eos = -1 and sync_every = 0, after one warm-up call (graph capture), decode() runs under
    torch.cuda.set_sync_debug_mode("error") without raising.  The mode does report on the ROCm build this was written on (an
    .item() the test makes itself under the mode raises; the test prints the probe's outcome), but torch calls it a prototype
    that does not see every synchronising call, so the test ALSO counts Tensor.item / __bool__ / cpu / tolist on device tensors
    through patched methods: none may happen."""
    s = _session("caption_full", torch.bfloat16)
    bs = s["device"]
    bs.decode(*s["enc"], bos=s["bos"], eos=-1, sync_every=0)
    torch.cuda.synchronize()
    probe = torch.ones(1, device=DEV)
    prev = torch.cuda.get_sync_debug_mode()
    reads = _HostReads(monkeypatch)
    try:
        torch.cuda.set_sync_debug_mode("error")
        res = bs.decode(*s["enc"], bos=s["bos"], eos=-1, sync_every=0)
        n_reads = list(reads.calls)
        try:
            probe.item()
            reports = False
        except RuntimeError:
            reports = True
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    print("[sync debug mode] reports synchronising calls on this build: %s; host reads counted in decode(): %s" % (reports, n_reads))
    assert n_reads == []
    torch.cuda.synchronize()
    assert res.lengths.tolist() == [s["T"]] * s["n"]


def test_result_does_not_depend_on_sync_every():
    """D (second half).  With the golden's eos2 the results for sync_every in {1, 3, 0} are identical in every field, and the
    lengths equal those of the golden's hyp2 on the instances C found free of exact ties."""
    s = _session("caption_full", torch.float32)
    clean, _, _ = _compare_modes("caption_full", torch.float32, True)
    res = [s["device"].decode(*s["enc"], bos=s["bos"], eos=s["eos2"], sync_every=k) for k in (1, 3, 0)]
    fields = ("tokens", "scores", "lengths", "parents", "step_tokens", "step_scores")
    for r in res[1:]:
        for f in fields:
            assert torch.equal(getattr(r, f), getattr(res[0], f)), f
    want = [int((row >= 0).sum()) for row in s["g"]["hyp2"]]
    got = res[0].lengths.tolist()
    print("[sync_every] lengths %s\n             golden  %s, tie-free instances %s" % (got, want, list(clean)))
    assert [got[i] for i in clean] == [want[i] for i in clean]


@pytest.mark.parametrize("case", ["caption_small", "caption_full"])
def test_n_best_hypotheses(case):
    """E.  For n_best in {1, 3, n_bm}: tokens[i, k] is the Python walk-back of the returned history from beam k, scores[i] is
    non-increasing in k, and __call__ returns hypotheses() of n_best = 1 with scores[:, 0]."""
    s = _session(case, torch.float32)
    bs, n, nb = s["device"], s["n"], s["nb"]
    for eos in (-1, s["eos2"]):
        for n_best in (1, 3, nb):
            r = bs.decode(*s["enc"], bos=s["bos"], eos=eos, n_best=n_best)
            assert r.tokens.shape == (n, n_best, bs.Tmax) and r.scores.shape == (n, n_best) and r.tokens.is_cuda and r.scores.is_cuda
            par, tok, lens, got = r.parents.cpu(), r.step_tokens.cpu(), r.lengths.tolist(), r.tokens.cpu()
            hyps = r.hypotheses()
            for i in range(n):
                assert 1 <= lens[i] <= s["T"]
                for k in range(n_best):
                    want = _walk_back(par, tok, lens[i] - 1, i, k)
                    assert got[i, k, :lens[i]].tolist() == want and bool((got[i, k, lens[i]:] == -1).all())
                    assert hyps[i][k] == want
                assert bool((r.scores[i, 1:] <= r.scores[i, :-1]).all())
                assert torch.equal(r.scores[i].cpu(), r.step_scores[lens[i] - 1, i, :n_best].cpu())
            if n_best == 1:
                hyp, sc = bs(*s["enc"], bos=s["bos"], eos=eos)
                assert hyp == [h[0] for h in hyps] and torch.equal(sc, r.scores[:, 0])
    with pytest.raises(ValueError):
        bs.decode(*s["enc"], bos=s["bos"], eos=-1, n_best=nb + 1)
