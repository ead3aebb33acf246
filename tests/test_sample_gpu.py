"""Caption sampling: the fused top-k / temperature / top-p sample step (csrc/sample.hip: univl_sample_step) and the session built on
it (univl_amd.sample.CaptionSampler).

_expect restates the contract of include/univl_hip.h on the CPU: a stable descending sort for step 1, mix32 with Python integers,
fp32 for the two rounded operations of step 2, float64 for the exponentials and the sums.  The kernel forms the weights with expf
and one fp32 chain, so a draw is compared only where it is DECIDED: tau farther than 1e-4 c_{m-1} from every c_j, and (top_p < 1)
top_p c_{k-1} farther than 1e-4 c_{k-1} from every c_j.  Margin: at most 64 terms x (2 ulp expf + 1 ulp add) x 2^-23 = 2.3e-5, times 4.
At most 5 % of the draws of any case may be undecided (the band's worst case is 64 x 2e-4 = 1.3 %); the top-k columns and their
order are compared exactly, always.

A  the kernel against _expect on seeded random logits free of exact ties;
B  crafted inputs: arg-max tie rule, padding columns, top_p -> m = 1, underflowing weights, frozen rows, argument range;
C  purity: a row's outputs do not depend on R or on deterministic mode;
D  frequencies against the exact probabilities (chi-square), and the nucleus' excluded columns;
E  whole runs on the toy caption model against a host loop of step_logits + _expect; seeds, sync_every, n_active;
F  top_k = 1 against CaptionBeamSearch(n_bm=1);  G  no host involvement inside sample();  H  captions() against a Python cut."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import univl_oracle as O
from make_golden import case_config

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from univl_amd import _lib, ops
    from univl_amd.decode import CaptionBeamSearch
    from univl_amd.sample import CaptionSampler
    from test_model_gpu import build, GATES

DEV = "cuda"
TMAX = 5
MASK64 = (1 << 64) - 1
DECIDED_MARGIN = 1e-4
UNDECIDED_CAP = 0.05
LOGPROB_TOL = 2e-6
CHI2_7DOF = 24.3


@pytest.fixture(autouse=True)
def _deterministic_mode():
    """Fixed-order sums in the decoder's products, as tests/test_beam_gpu.py: E and F compare separate runs bit for bit.  The sample
    kernels have no order-dependent sums in either mode (C checks that)."""
    import univl_amd
    was = univl_amd.deterministic()
    univl_amd.set_deterministic(True)
    yield
    univl_amd.set_deterministic(was)


# ------------------------------------------------------------------------------------------------ the contract on the CPU
def mix32(x):
    x &= MASK64
    x ^= x >> 33
    x = (x * 0xff51afd7ed558ccd) & MASK64
    x ^= x >> 33
    x = (x * 0xc4ceb9fe1a85ec53) & MASK64
    x ^= x >> 33
    return x & 0xFFFFFFFF


def draw_u(seed, t, r):
    r32 = mix32(((seed * 0x9E3779B97F4A7C15) & MASK64) ^ ((t * 0xD1B54A32D192ED03 + r) & MASK64))
    return (r32 >> 8) / 16777216.0


def _expect(x, k, temperature, top_p, seed, t, r):
    """One row.  x: the row's V candidate logits (fp32 array).  Returns a dict: cols (the top-k columns in order), m, token, j,
    tok_logprob, q_logprob (float64), decided."""
    x = np.asarray(x, dtype=np.float32)
    cols = np.argsort(-x, kind="stable")[:k]                       # equal values: lower column first
    xs = x[cols]
    inv_T = np.float32(1.0 / temperature)
    top_p = float(np.float32(top_p))
    d = (xs - xs[0]).astype(np.float32)                            # two separately rounded fp32 operations
    a = (d * inv_T).astype(np.float32)
    w = np.exp(a.astype(np.float64))
    c = np.cumsum(w)
    decided = True
    if top_p >= 1.0:
        m = k
    else:
        thr = top_p * c[-1]
        m = int(np.argmax(c >= thr)) + 1
        decided = bool(np.min(np.abs(c - thr)) > DECIDED_MARGIN * c[-1])
    tau = draw_u(seed, t, r) * c[m - 1]
    j = int(np.argmax(c[:m] > tau))
    decided = decided and bool(np.min(np.abs(c - tau)) > DECIDED_MARGIN * c[m - 1])
    x64 = x.astype(np.float64)
    mx = x64.max()
    tok_lp = (x64[cols[j]] - mx) - np.log(np.exp(x64 - mx).sum())
    q_lp = np.log(w[j] / c[m - 1])
    return dict(cols=cols, m=m, j=j, token=int(cols[j]), tok_logprob=float(tok_lp), q_logprob=float(q_lp), decided=decided)


def chi_square(counts, probs):
    n = float(sum(counts))
    return float(sum((o - n * p) ** 2 / (n * p) for o, p in zip(counts, probs) if p > 0))


# ------------------------------------------------------------------------------------------------ A: seeded cases
A_SHAPES = [(30522, 30528), (1000, 1000), (8, 8)]
A_ROWS = [1, 3, 80]
A_SAMPLING = [(1.0, 1.0), (0.7, 0.9)]
A_POSITIONS = [0, 3]


def a_ks(V):
    return [1, 5, min(64, V)]


@functools.lru_cache(maxsize=None)
def a_logits(V, ld, R):
    """Seeded logits [R, ld] fp32 (numpy); the padding columns hold +3e38 so that a kernel that read them as candidates would pick them.
    Standard deviation 6: the nucleus threshold top_p c_{k-1} is a fixed point of the row, not a uniform draw, and with flatter rows
    it falls where the 64 c_j lie 3e-3 c apart -- 7 % of such rows are undecided by the band alone."""
    g = torch.Generator().manual_seed(77 + 1000 * R + V % 97)
    x = torch.randn(R, ld, generator=g) * 6.0 + 1.5
    x[:, V:] = 3e38
    return x.numpy()


def a_done(R):
    return [(r % 3) == 1 for r in range(R)]


def undecided_share(exps, active):
    n = sum(1 for a in active if a)
    return sum(1 for e, a in zip(exps, active) if a and not e["decided"]) / max(n, 1)


@functools.lru_cache(maxsize=None)
def a_case(V, ld, R, k, temperature, top_p, t):
    """(seed, _expect of every row).  The seed is chosen on the CPU, as D's is: the first of a fixed sequence for which _expect alone
    leaves at most 5 % of the active rows undecided (with R = 1 or 3 that means none); tests/test_sample_cpu.py checks every case."""
    x = a_logits(V, ld, R)
    active = [not f for f in a_done(R)]
    for bump in range(16):
        seed = (0xC0FFEE + 7919 * V + 104729 * R + 31 * k + t + 1000003 * bump) & MASK64
        exps = [_expect(x[r, :V], k, temperature, top_p, seed, t, r) for r in range(R)]
        if undecided_share(exps, active) <= UNDECIDED_CAP:
            return seed, exps
    raise AssertionError("no seed of the sequence passes: the undecided share comes from the nucleus threshold, not from the draw")


def _state(x, R, k, done, seed=3):
    """Device buffers of one univl_sample_step call; history and outputs pre-filled with markers."""
    g = torch.Generator().manual_seed(seed)
    return dict(x=torch.as_tensor(x).to(DEV), done=torch.tensor(done, dtype=torch.uint8, device=DEV),
                length=(torch.arange(R, dtype=torch.int32) % 3 + 1).to(DEV), ids=torch.randint(0, 8, (R,), generator=g).to(DEV),
                tokens_out=torch.full((R, TMAX), -7, dtype=torch.int32, device=DEV), tok_logprob=torch.full((R, TMAX), -7.0, device=DEV),
                q_logprob=torch.full((R, TMAX), -7.0, device=DEV), seq_logprob=(-torch.rand(R, generator=g) * 9.0).to(DEV),
                seq_q_logprob=(-torch.rand(R, generator=g) * 5.0).to(DEV), topk_idx=torch.full((R, k), -7, dtype=torch.int32, device=DEV),
                topk_val=torch.full((R, k), -7.0, device=DEV), ws=ops.sample_ws(R, k, DEV))


def _host(d):
    return {n: v.cpu().clone() for n, v in d.items() if n not in ("x", "ws")}


def _run(d, V, k, t, **kw):
    ops.sample_step(d["x"], V, k, t, **{n: v for n, v in d.items() if n != "x"}, **kw)
    torch.cuda.synchronize()


def _check(before, after, exps, active, t, eos, tag):
    """Every buffer against the contract: column t of the active rows as _expect says (token on decided draws), everything else as
    it was.  Returns the undecided share."""
    R = len(exps)
    want_tok, want_lp, want_q = before["tokens_out"].clone(), before["tok_logprob"].clone(), before["q_logprob"].clone()
    want_ids, want_len, want_done = before["ids"].clone(), before["length"].clone(), before["done"].clone()
    want_seq, want_seqq = before["seq_logprob"].clone(), before["seq_q_logprob"].clone()
    want_ti, want_tv = before["topk_idx"].clone(), before["topk_val"].clone()
    worst = [0.0, 0.0]
    for r in range(R):
        if not active[r]:
            continue
        e = exps[r]
        got = int(after["tokens_out"][r, t])
        assert after["topk_idx"][r].tolist() == e["cols"].tolist(), (tag, r)
        want_ti[r] = after["topk_idx"][r]
        want_tv[r] = after["topk_val"][r]
        if e["decided"]:
            assert got == e["token"], (tag, r, got, e["token"])
        assert got in e["cols"][:e["m"] if e["decided"] else len(e["cols"])].tolist(), (tag, r, got)
        if got == e["token"]:
            worst[0] = max(worst[0], abs(float(after["tok_logprob"][r, t]) - e["tok_logprob"]))
            worst[1] = max(worst[1], abs(float(after["q_logprob"][r, t]) - e["q_logprob"]))
        want_tok[r, t], want_ids[r] = got, got
        want_lp[r, t], want_q[r, t] = after["tok_logprob"][r, t], after["q_logprob"][r, t]
        want_seq[r] = before["seq_logprob"][r] + after["tok_logprob"][r, t]            # one fp32 addition
        want_seqq[r] = before["seq_q_logprob"][r] + after["q_logprob"][r, t]
        want_len[r] += 1
        want_done[r] = 1 if got == eos else 0
    share = undecided_share(exps, active)
    print("[sample %s] undecided %.2f %%, worst |tok_logprob - f64| %.2e, |q_logprob - f64| %.2e" % (tag, 100 * share, worst[0], worst[1]))
    assert worst[0] <= LOGPROB_TOL and worst[1] <= LOGPROB_TOL, (tag, worst)
    for name, want in (("tokens_out", want_tok), ("tok_logprob", want_lp), ("q_logprob", want_q), ("ids", want_ids), ("length", want_len),
                       ("done", want_done), ("seq_logprob", want_seq), ("seq_q_logprob", want_seqq), ("topk_idx", want_ti),
                       ("topk_val", want_tv)):
        assert torch.equal(after[name], want), (tag, name)
    assert share <= UNDECIDED_CAP, (tag, share)
    return share


@pytest.mark.parametrize("t", A_POSITIONS)
@pytest.mark.parametrize("temperature,top_p", A_SAMPLING)
@pytest.mark.parametrize("R", A_ROWS)
@pytest.mark.parametrize("V,ld", A_SHAPES)
def test_sample_step_matches_contract(V, ld, R, temperature, top_p, t):
    """A.  Every k of the shape in one test (the logits and their sort are shared)."""
    x = a_logits(V, ld, R)
    done = a_done(R)
    active = [not f for f in done]
    for k in a_ks(V):
        seed, exps = a_case(V, ld, R, k, temperature, top_p, t)
        eos = exps[0]["token"]                                       # row 0 finishes at this step (on a decided draw)
        d = _state(x, R, k, done)
        before = _host(d)
        _run(d, V, k, t, inv_T=float(np.float32(1.0 / temperature)), top_p=top_p, seed=seed, eos=eos)
        after = _host(d)
        _check(before, after, exps, active, t, eos, "A V=%d R=%d k=%d T=%g p=%g t=%d" % (V, R, k, temperature, top_p, t))
        for r in range(R):
            if active[r]:
                assert torch.equal(after["topk_val"][r], torch.from_numpy(x[r, exps[r]["cols"]]))


# ------------------------------------------------------------------------------------------------ B: crafted inputs
def _background(R, V, ld):
    """Distinct, strictly decreasing values far below the planted ones; padding +3e38."""
    x = (-50.0 - torch.arange(R * ld, dtype=torch.float64) * 1e-4).to(torch.float32).view(R, ld).clone()
    x[:, V:] = 3e38
    return x


def _crafted(x, V, k, t=1, seed=5, temperature=1.0, top_p=1.0, done=None):
    R = x.shape[0]
    done = [False] * R if done is None else done
    exps = [_expect(x[r, :V].numpy(), k, temperature, top_p, seed, t, r) for r in range(R)]
    d = _state(x.numpy(), R, k, done)
    before = _host(d)
    _run(d, V, k, t, inv_T=float(np.float32(1.0 / temperature)), top_p=top_p, seed=seed)
    after = _host(d)
    return before, after, exps


def test_argmax_tie_rule():
    """B (i).  k = 1 is the arg-max; equal maxima resolve to the LOWER column: inside one 16-byte word, in different column slices,
    and between column 0 and the last V % 4 columns (the partly padded word)."""
    V, ld = 30522, 30528
    assert V % 4 == 2
    plants = [([100, 101, 102], 100), ([20001, 100, 9000], 100), ([30521, 4100], 4100), ([V - 1, 0, V - 2], 0), ([V - 1, V - 2], V - 2),
              ([V - 1], V - 1), ([0], 0)]
    x = _background(len(plants), V, ld)
    for r, (cols, _) in enumerate(plants):
        x[r, cols] = 2.0
    before, after, exps = _crafted(x, V, 1)
    for r, (_, want) in enumerate(plants):
        assert exps[r]["token"] == want and int(after["tokens_out"][r, 1]) == want == int(after["ids"][r]), (r, want)
        assert float(after["q_logprob"][r, 1]) == 0.0
    # with k = 3 the equal values fill the list in column order
    before, after, exps = _crafted(x, V, 3)
    assert after["topk_idx"][0].tolist() == [100, 101, 102] and after["topk_idx"][1].tolist() == [100, 9000, 20001]
    assert after["topk_idx"][3].tolist() == [0, V - 2, V - 1]
    for r in range(len(plants)):
        assert after["topk_idx"][r].tolist() == exps[r]["cols"].tolist()
    # a row stride that is no multiple of 4 floats (the scalar path): same contract
    V2, ld2 = 1001, 1003
    x2 = _background(2, V2, ld2)
    x2[0, [1000, 0]] = 2.0
    x2[1, [999, 1000]] = 2.0
    before, after, exps = _crafted(x2, V2, 1)
    assert [int(after["tokens_out"][r, 1]) for r in range(2)] == [0, 999] == [e["token"] for e in exps]


def test_padding_columns_are_never_read_as_candidates():
    """B (ii).  +3e38 in columns V .. ld-1: never chosen, not in the list, and not in the log-sum-exp (tok_logprob stays finite and
    equals the float64 value over the V candidates)."""
    V, ld, R, k = 30522, 30528, 4, 64
    x = torch.from_numpy(a_logits(V, ld, 80)[:R].copy())
    assert bool((x[:, V:] == 3e38).all())
    before, after, exps = _crafted(x, V, k, t=2, seed=11)
    _check(before, after, exps, [True] * R, 2, -1, "B padding")
    assert int(after["topk_idx"].max()) < V and bool(torch.isfinite(after["tok_logprob"][:, 2]).all())


def test_tiny_top_p_is_the_argmax_for_every_seed():
    """B (iii).  top_p = 1e-6 gives m = 1: the arg-max whatever the seed, q_logprob = log(w_0 / c_0) = 0."""
    V, ld, R, k = 1000, 1000, 3, 50
    x = torch.from_numpy(a_logits(V, ld, R).copy())
    for seed in (0, 1, 2, 12345, MASK64):
        before, after, exps = _crafted(x, V, k, seed=seed, temperature=2.0, top_p=1e-6)
        for r in range(R):
            assert exps[r]["m"] == 1 and int(after["tokens_out"][r, 1]) == int(np.argmax(x[r, :V].numpy())) == exps[r]["token"]
            assert float(after["q_logprob"][r, 1]) == 0.0


def test_underflowing_weights():
    """B (iv).  Every weight but w_0 underflows to 0: the chain stays at 1, the draw is column of x_0 for every seed."""
    V, ld, R, k = 1000, 1000, 2, 64
    x = torch.full((R, ld), -1000.0)
    x += torch.arange(ld, dtype=torch.float32) * -0.5               # distinct values
    x[0, 777] = 5.0
    x[1, 0] = 5.0
    for seed in (0, 7, 99):
        before, after, exps = _crafted(x, V, k, seed=seed, temperature=0.5)
        assert [int(after["tokens_out"][r, 1]) for r in range(R)] == [777, 0]
        for r in range(R):
            assert float(after["q_logprob"][r, 1]) == 0.0
            assert abs(float(after["tok_logprob"][r, 1]) - exps[r]["tok_logprob"]) <= LOGPROB_TOL
            assert after["topk_idx"][r].tolist() == exps[r]["cols"].tolist()


def test_frozen_rows():
    """B (v).  done != 0: nothing of the row is written, ids stays."""
    V, ld, R, k = 1000, 1000, 5, 5
    x = torch.from_numpy(a_logits(V, ld, 80)[:R].copy())
    before, after, exps = _crafted(x, V, k, done=[True] * R)
    for name in before:
        assert torch.equal(before[name], after[name]), name
    before, after, exps = _crafted(x, V, k, done=[True, False, True, True, False])
    _check(before, after, exps, [False, True, False, False, True], 1, -1, "B frozen")


def test_argument_range():
    """B (vi).  Every range violation, a null pointer or a short workspace: UNIVL_EINVAL, and nothing is written."""
    V, ld, R, k = 64, 64, 3, 5
    x = a_logits(1000, 1000, 3)[:, :ld].copy()
    d = _state(x, R, k, [False] * R)
    L = _lib.lib()

    def rc(**kw):
        desc = ops.sample_step_desc(d["x"], V, k, 1, **{n: v for n, v in d.items() if n != "x"})
        for n, v in kw.items():
            setattr(desc, n, v)
        r = L.univl_sample_step(C.byref(desc), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        return r

    before = _host(d)
    EINVAL = -1
    for kw in (dict(R=0), dict(R=-2), dict(k=0), dict(k=65), dict(k=-1), dict(V=4), dict(V=0), dict(ld=V - 1), dict(t=TMAX), dict(t=-1),
               dict(Tmax=0), dict(inv_T=0.0), dict(inv_T=-1.0), dict(inv_T=float("inf")), dict(inv_T=float("nan")), dict(top_p=0.0),
               dict(top_p=-0.5), dict(top_p=float("nan")), dict(ws_bytes=R * 8 * (8 * k + 16) - 1), dict(ws=None), dict(x=None),
               dict(done=None), dict(length=None), dict(ids=None), dict(tokens_out=None), dict(tok_logprob=None), dict(q_logprob=None),
               dict(seq_logprob=None), dict(seq_q_logprob=None)):
        assert rc(**kw) == EINVAL, kw
        assert L.univl_last_error()
    after = _host(d)
    for name in before:
        assert torch.equal(before[name], after[name]), name
    assert rc() == 0 and rc(topk_idx=None, topk_val=None) == 0
    assert int(_host(d)["length"][0]) == int(before["length"][0]) + 2


# ------------------------------------------------------------------------------------------------ C: purity
@pytest.mark.parametrize("V,ld,k", [(30522, 30528, 64), (1000, 1000, 5)])
def test_row_outputs_do_not_depend_on_the_batch(V, ld, k):
    """C.  The same row of logits at r = 2 of R = 3 and at r = 2 of R = 80: identical bits in every output, in deterministic mode and
    out of it; the scalars and the device words give the same bits too."""
    import univl_amd
    big = a_logits(V, ld, 80).copy()
    small = a_logits(V, ld, 3).copy()
    small[2] = big[2]
    outs = []
    for det in (True, False):
        univl_amd.set_deterministic(det)
        for x, R, dev_words in ((small, 3, False), (big, 80, False), (big, 80, True)):
            d = _state(x, R, k, [False] * R)
            for name in ("length", "ids", "seq_logprob", "seq_q_logprob"):
                d[name][2] = d[name][2] * 0 + 2                      # the row's own state is part of its inputs
            kw = dict(inv_T=float(np.float32(1.0 / 0.7)), top_p=0.9, seed=424242, eos=-1)
            if dev_words:
                kw = dict(sampling_dev=torch.tensor([1.0 / 0.7, 0.9], dtype=torch.float32, device=DEV),
                          seed_dev=torch.tensor([424242], dtype=torch.int64, device=DEV), eos_dev=torch.tensor([-1], dtype=torch.int32, device=DEV),
                          inv_T=123.0, top_p=0.001, seed=1, eos=int(np.argmax(big[2, :V])))
            _run(d, V, k, 3, **kw)
            outs.append({n: v[2].clone() for n, v in _host(d).items()})
    univl_amd.set_deterministic(True)
    for o in outs[1:]:
        for name in outs[0]:
            assert torch.equal(o[name], outs[0][name]), name
    assert int(outs[0]["length"]) == 3 and int(outs[0]["tokens_out"][3]) >= 0


# ------------------------------------------------------------------------------------------------ D: frequencies
D_ROW = [1.2, 0.3, -0.5, 2.0, 0.0, -1.5, 0.9, 1.6]
D_ROWS = 8192


def d_probs(top_p):
    """The exact distribution the contract defines for the row (float64): softmax over the 8 columns, cut to the nucleus."""
    x = np.asarray(D_ROW, dtype=np.float32)
    e = _expect(x, 8, 1.0, top_p, 0, 0, 0)
    w = np.exp((x[e["cols"]] - x[e["cols"][0]]).astype(np.float64))
    w[e["m"]:] = 0.0
    p = np.zeros(8)
    p[e["cols"]] = w / w.sum()
    return p


def d_expect_counts(top_p, seed):
    x = np.asarray(D_ROW, dtype=np.float32)
    exps = [_expect(x, 8, 1.0, top_p, seed, 2, r) for r in range(D_ROWS)]
    counts = np.bincount([e["token"] for e in exps], minlength=8)
    return exps, counts


def d_seed(top_p):
    """The first seed from 1 for which _expect itself passes the chi-square bound (chosen on the CPU; tests/test_sample_cpu.py pins it)."""
    for seed in range(1, 50):
        _, counts = d_expect_counts(top_p, seed)
        if chi_square(counts, d_probs(top_p)) < CHI2_7DOF:
            return seed
    raise AssertionError("no seed below 50 passes")


@pytest.mark.parametrize("top_p", [1.0, 0.6])
def test_frequencies(top_p):
    """D.  8192 rows of one 8-column row of logits, k = 8, T = 1: the counts of the kernel's draws against the exact probabilities,
    chi-square at 7 degrees of freedom < 24.3 (p about 1e-3); with top_p = 0.6 the excluded columns have count 0."""
    seed = d_seed(top_p)
    exps, _ = d_expect_counts(top_p, seed)
    x = np.tile(np.asarray(D_ROW, dtype=np.float32), (D_ROWS, 1))
    d = _state(x, D_ROWS, 8, [False] * D_ROWS)
    _run(d, 8, 8, 2, inv_T=1.0, top_p=top_p, seed=seed)
    tok = d["tokens_out"][:, 2].cpu().numpy()
    und = [not e["decided"] for e in exps]
    share = sum(und) / D_ROWS
    wrong = [r for r in range(D_ROWS) if exps[r]["decided"] and tok[r] != exps[r]["token"]]
    counts = np.bincount(tok, minlength=8)
    p = d_probs(top_p)
    chi2 = chi_square(counts, p)
    print("[sample D p=%g seed=%d] counts %s chi2 %.2f undecided %.2f %%" % (top_p, seed, counts.tolist(), chi2, 100 * share))
    assert not wrong and share <= UNDECIDED_CAP
    assert chi2 < CHI2_7DOF
    assert all(counts[v] == 0 for v in range(8) if p[v] == 0)
    if top_p < 1:
        assert sum(1 for v in range(8) if p[v] == 0) >= 1


# ------------------------------------------------------------------------------------------------ E .. H: whole runs
BOS, T_RUN, N_SAMP, TOP_K, TEMP, TOP_P = 101, 6, 4, 20, 1.3, 0.95


@functools.lru_cache(maxsize=None)
def _toy(dtype):
    cfg, _, _ = case_config("caption_small")
    model, _ = build(cfg, dtype)
    model.eval()
    feats = []
    for seed in (31, 32, 33):
        d = {k: v.to(DEV) for k, v in O.synthetic_batch(cfg, 3, seed=seed).items()}
        with torch.no_grad():
            so, vo = model.get_sequence_visual_output(d["input_ids"], d["token_type_ids"], d["attention_mask"], d["video"], d["video_mask"])
        feats.append((so, vo, d["attention_mask"].view(3, -1), d["video_mask"].view(3, -1)))
    return cfg, model, feats


def _new_sampler(dtype, n, **kw):
    cfg, model, _ = _toy(dtype)
    args = dict(n_samp=N_SAMP, max_len=T_RUN, top_k=TOP_K, temperature=TEMP, top_p=TOP_P)
    args.update(kw)
    return CaptionSampler(model, n, cfg.max_words, cfg.max_frames, **args)


@functools.lru_cache(maxsize=None)
def _sampler(dtype, n):
    return _new_sampler(dtype, n)


def _head(enc, n):
    return tuple(x[:n] for x in enc)


FIELDS = ("tokens", "token_logprobs", "token_q_logprobs", "seq_logprob", "seq_q_logprob", "lengths")


def _same(a, b, rows=None):
    for f in FIELDS:
        x, y = getattr(a, f), getattr(b, f)
        if rows is not None:
            x, y = x[:rows], y[:rows]
        assert torch.equal(x, y), f


def _eos_for(smp, enc, seed):
    """An end token that stops some rows early: what row 1 drew at position 2 of a run without one."""
    res = smp.sample(*enc, bos=BOS, eos=-1, seed=seed)
    return int(res.tokens.reshape(-1, res.tokens.shape[-1])[1, 2])


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_sample_matches_host_loop(dtype, n):
    """E (i).  sample() against a host loop over the positions: step_logits on the tokens the device drew (so both sides see the same
    logits, bit for bit), then _expect per row.  Tokens equal on decided draws (at most 5 % undecided), both log-probabilities
    within 2e-6 of the float64 values on those logits, the sequence sums the left-to-right fp32 sums, lengths and the -1 / 0 padding."""
    smp = _sampler(dtype, n)
    enc = _head(_toy(dtype)[2][0], n)
    seed = 2024
    eos = _eos_for(smp, enc, seed)
    res = smp.sample(*enc, bos=BOS, eos=eos, seed=seed)
    R, T = n * N_SAMP, T_RUN
    assert res.tokens.shape == (n, N_SAMP, T) and res.tokens.dtype == torch.int32 and res.tokens.is_cuda and res.lengths.shape == (n, N_SAMP)
    tok, lp, qlp = res.tokens.cpu().view(R, T), res.token_logprobs.cpu().view(R, T), res.token_q_logprobs.cpu().view(R, T)
    lens = res.lengths.cpu().view(R).tolist()
    assert min(lens) < T                                             # the end token did stop some row early
    draws = undecided = 0
    worst = [0.0, 0.0]
    for t in range(T):
        ids = torch.full((R,), BOS, dtype=torch.int64) if t == 0 else tok[:, t - 1].clamp(min=0).long()
        logits = smp.step_logits(t, ids.to(DEV)).cpu().numpy()
        for r in range(R):
            if t >= lens[r]:
                assert int(tok[r, t]) == -1 and float(lp[r, t]) == 0.0 and float(qlp[r, t]) == 0.0
                continue
            e = _expect(logits[r], TOP_K, TEMP, TOP_P, seed, t, r)
            draws += 1
            undecided += 0 if e["decided"] else 1
            got = int(tok[r, t])
            if e["decided"]:
                assert got == e["token"], (t, r, got, e["token"])
            if got == e["token"]:
                worst[0] = max(worst[0], abs(float(lp[r, t]) - e["tok_logprob"]))
                worst[1] = max(worst[1], abs(float(qlp[r, t]) - e["q_logprob"]))
            assert (got != eos) if t < lens[r] - 1 else (got == eos or lens[r] == T)    # a row ends with the end token or at Tmax
    print("[sample E %s n=%d] draws %d, undecided %.2f %%, worst |tok_logprob - f64| %.2e, |q_logprob - f64| %.2e, lengths %s"
          % (dtype, n, draws, 100.0 * undecided / draws, worst[0], worst[1], lens))
    assert undecided <= UNDECIDED_CAP * draws
    assert worst[0] <= LOGPROB_TOL and worst[1] <= LOGPROB_TOL
    for name, per_tok in (("seq_logprob", lp), ("seq_q_logprob", qlp)):
        acc = torch.zeros(R)
        for t in range(T):
            acc = torch.where(torch.tensor([t < l for l in lens]), acc + per_tok[:, t], acc)
        assert torch.equal(getattr(res, name).cpu().view(R), acc), name


def test_seeds_and_sync_every():
    """E (ii).  The same seed twice: bit-identical; sync_every in {0, 1, 8}: bit-identical; another seed, temperature or top_p: a
    different draw somewhere, from the same captured plans."""
    smp = _sampler(torch.float32, 3)
    enc = _toy(torch.float32)[2][0]
    eos = _eos_for(smp, enc, 7)
    plans = len(smp.steps)
    base = smp.sample(*enc, bos=BOS, eos=eos, seed=7)
    _same(base, smp.sample(*enc, bos=BOS, eos=eos, seed=7))
    for k in (0, 1, 8):
        _same(base, smp.sample(*enc, bos=BOS, eos=eos, seed=7, sync_every=k))
    other = smp.sample(*enc, bos=BOS, eos=eos, seed=8)
    assert not torch.equal(other.tokens, base.tokens)
    cold = smp.sample(*enc, bos=BOS, eos=eos, seed=7, temperature=0.05, top_p=0.5)
    assert not torch.equal(cold.token_q_logprobs, base.token_q_logprobs)
    _same(base, smp.sample(*enc, bos=BOS, eos=eos, seed=7))
    assert len(smp.steps) == plans                                   # no new plan, no new capture
    rows = base.tokens.view(-1, T_RUN)
    assert len({tuple(r.tolist()) for r in rows}) > 1               # the rows of an instance are different captions
    with pytest.raises(ValueError):
        smp.sample(*enc, bos=BOS, eos=eos, seed=7, temperature=0.0)
    with pytest.raises(ValueError):
        smp.sample(*enc, bos=BOS, eos=eos, seed=7, top_p=0.0)


def test_sampler_owns_no_beam_state_and_no_beam_form():
    """The sampler is a decode.CachedDecoder beside CaptionBeamSearch, not under it: no beam score, history or beam workspace exists on
    it, its plans are of the forms "logits" and "sample" only, and a request for any other form is an error that builds nothing."""
    smp = _sampler(torch.float32, 3)
    enc = _toy(torch.float32)[2][0]
    smp.sample(*enc, bos=BOS, eos=-1, seed=3)
    smp.step_logits(0, torch.full((3 * N_SAMP,), BOS, dtype=torch.int64, device=DEV))
    assert not isinstance(smp, CaptionBeamSearch)
    for name in ("hist_par", "hist_tok", "hist_sc", "beam_ws", "scores", "ident_nb"):
        assert not hasattr(smp, name), name
    keys = set(smp.steps)
    assert {form for _, form in keys} == {"logits", "sample"}
    for form in (True, False, "beam", None):
        with pytest.raises(ValueError, match="CaptionSampler"):
            smp._step_plan(0, form)
    assert set(smp.steps) == keys


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_partial_batches(dtype):
    """E (iii).  n_active = 2 of 3 after two different full batches went through the session (two kinds of stale contents in the idle
    slot), against the full batch and against a fresh session whose first call is partial: bit-identical on the shared slots."""
    smp = _sampler(dtype, 3)
    feats = _toy(dtype)[2]
    eos = _eos_for(smp, feats[0], 5)
    full = smp.sample(*feats[0], bos=BOS, eos=eos, seed=5)
    two = _head(feats[0], 2)
    res = []
    for stale in (feats[1], feats[2]):
        smp.sample(*stale, bos=BOS, eos=eos, seed=99)
        res.append(smp.sample(*two, bos=BOS, eos=eos, seed=5, n_active=2))
    assert res[0].tokens.shape == (2, N_SAMP, T_RUN) and res[0].lengths.shape == (2, N_SAMP)
    _same(res[0], res[1])
    _same(res[0], full, rows=2)
    fresh = _new_sampler(dtype, 3)
    _same(res[0], fresh.sample(*two, bos=BOS, eos=eos, seed=5, n_active=2))
    with pytest.raises(ValueError):
        smp.sample(*two, bos=BOS, eos=eos, seed=5, n_active=4)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_greedy_matches_beam_of_one(dtype):
    """F.  top_k = 1 against CaptionBeamSearch(n_bm=1).decode() on the same inputs: equal hypotheses wherever every position's
    top-1 / top-2 logit gap exceeds the logit gate of the parity tests (rows under the rule: at most a tenth), seq_logprob within
    1e-5 x length of the beam's score."""
    cfg, model, feats = _toy(dtype)
    n, enc = 3, feats[0]
    greedy = _new_sampler(dtype, n, n_samp=1, top_k=1, temperature=1.0, top_p=1.0)
    beam = CaptionBeamSearch(model, n, cfg.max_words, cfg.max_frames, n_bm=1, max_len=T_RUN)
    eos = int(greedy.sample(*enc, bos=BOS, eos=-1, seed=0).tokens[0, 0, 3])
    rs = greedy.sample(*enc, bos=BOS, eos=eos, seed=0)
    rb = beam.decode(*enc, bos=BOS, eos=eos)
    hs, hb = [h[0] for h in rs.hypotheses()], [h[0] for h in rb.hypotheses()]
    tok = rs.tokens.cpu().view(n, T_RUN)
    gate, under = GATES[dtype]["logits"], set()
    for t in range(T_RUN):
        ids = torch.full((n,), BOS, dtype=torch.int64) if t == 0 else tok[:, t - 1].clamp(min=0).long()
        top2 = greedy.step_logits(t, ids.to(DEV)).topk(2, dim=1).values.cpu()
        for r in range(n):
            if t < len(hs[r]) and float(top2[r, 0] - top2[r, 1]) <= gate:
                under.add(r)
    print("[sample F %s] rows under the gap rule: %d of %d; lengths %s" % (dtype, len(under), n, [len(h) for h in hs]))
    assert len(under) <= n / 10
    for r in range(n):
        if r not in under:
            assert hs[r] == hb[r], (r, hs[r], hb[r])
            assert abs(float(rs.seq_logprob[r, 0]) - float(rb.scores[r, 0])) <= 1e-5 * len(hs[r])
            assert float(rs.seq_q_logprob[r, 0]) == 0.0


class _HostReads:
    """Counts Tensor.item / __bool__ / cpu / tolist calls on device tensors (the mechanism of tests/test_beam_gpu.py part D)."""

    def __init__(self, monkeypatch):
        self.calls = []
        for name in ("item", "__bool__", "cpu", "tolist"):
            orig = getattr(torch.Tensor, name)

            def wrapped(t, *a, _orig=orig, _name=name, **kw):
                if t.is_cuda:
                    self.calls.append(_name)
                return _orig(t, *a, **kw)
            monkeypatch.setattr(torch.Tensor, name, wrapped)


def test_sample_has_no_host_involvement(monkeypatch):
    """G.  With eos = -1 and sync_every = 0, after one warm-up call (graph capture), sample() runs under
    torch.cuda.set_sync_debug_mode("error") without raising, and no Tensor.item / __bool__ / cpu / tolist happens on a device tensor."""
    smp = _sampler(torch.bfloat16, 3)
    enc = _toy(torch.bfloat16)[2][0]
    smp.sample(*enc, bos=BOS, eos=-1, seed=1, sync_every=0)
    torch.cuda.synchronize()
    probe = torch.ones(1, device=DEV)
    prev = torch.cuda.get_sync_debug_mode()
    reads = _HostReads(monkeypatch)
    try:
        torch.cuda.set_sync_debug_mode("error")
        res = smp.sample(*enc, bos=BOS, eos=-1, seed=2, sync_every=0)
        n_reads = list(reads.calls)
        try:
            probe.item()
            reports = False
        except RuntimeError:
            reports = True
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    print("[sync debug mode] reports synchronising calls on this build: %s; host reads counted in sample(): %s" % (reports, n_reads))
    assert n_reads == []
    torch.cuda.synchronize()
    assert res.lengths.cpu().view(-1).tolist() == [T_RUN] * (3 * N_SAMP)


def test_captions_match_python_cut():
    """H.  captions() against the reference's two cuts made in Python on hypotheses(), per ROW length."""
    smp = _sampler(torch.float32, 3)
    enc = _toy(torch.float32)[2][0]
    eos = _eos_for(smp, enc, 21)
    res = smp.sample(*enc, bos=BOS, eos=eos, seed=21)
    hyps = res.hypotheses()
    lens = res.lengths.cpu().tolist()
    pad = hyps[2][3][0]                                               # a token that does occur: the pad cut is exercised too
    word = torch.tensor([eos], dtype=torch.int32, device=DEV)
    for kw in (dict(eos=eos, pad=pad), dict(eos=-1, pad=-1), dict(eos=12345, pad=pad, eos_dev=word)):
        cap, cap_len = res.captions(**kw)
        assert cap.shape == (3, N_SAMP, T_RUN) and cap_len.shape == (3, N_SAMP) and cap.is_cuda
        e = eos if "eos_dev" in kw else kw["eos"]
        for i in range(3):
            for s in range(N_SAMP):
                toks = list(hyps[i][s])
                assert len(toks) == lens[i][s]
                if e >= 0 and e in toks:
                    toks = toks[:toks.index(e)]
                if kw["pad"] >= 0 and kw["pad"] in toks:
                    toks = toks[:toks.index(kw["pad"])]
                assert cap[i, s].tolist() == toks + [-1] * (T_RUN - len(toks)) and int(cap_len[i, s]) == len(toks)
