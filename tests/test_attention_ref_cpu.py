"""The fp64 attention reference, its per-row metric and its precision model (tests/attention_ref.py) against the oracle, autograd and
cases with a known answer.  No GPU."""
import math

import torch

import attention_ref as A
import dropout_ref as R
import univl_oracle as O


def _gen(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def test_bias_and_forward_equal_the_oracle_where_both_are_defined():
    """Sq == Sk, causal or not: the bias is the oracle's extended mask (the decoder's ((1 - mask) + triu) > 0 form under causal: one
    -10000, never -20000) and the forward is attention_core."""
    B, S, H = 3, 13, 2
    q, k, v, do = (_gen(B, S, H * 64, seed=s) for s in (1, 2, 3, 4))
    mask = torch.ones(B, S, dtype=torch.long)
    mask[1] = 0
    mask[2, 9:] = 0
    for causal in (False, True):
        bias = A.attn_bias(mask, S, S, causal)
        add = O.extended_mask(mask, torch.float64)
        if causal:
            sub = torch.triu(torch.ones(S, S, dtype=torch.float64), diagonal=1)
            add = ((1.0 - mask[:, None, None, :].double()) + sub[None, None]).gt(0).double() * -10000.0
        assert torch.equal(bias.expand(B, 1, S, S), add.expand(B, 1, S, S))
        assert set(bias.unique().tolist()) <= {0.0, A.NEG}
        ref = A.reference(q, k, v, bias, H, do)
        assert float((ref["out"] - O.attention_core(q, k, v, add, H)).abs().max()) < 1e-14
    # Sq != Sk under causal: key > q, whatever the lengths
    b = A.attn_bias(None, 3, 5, True)[0, 0]
    assert torch.equal(b != 0, torch.tensor([[0, 1, 1, 1, 1], [0, 0, 1, 1, 1], [0, 0, 0, 1, 1]], dtype=torch.bool))
    assert not bool(A.attn_bias(None, 5, 3, True)[0, 0][2:].any())


def test_lse_identity_and_the_fully_masked_row():
    B, Sq, Sk, H = 3, 5, 11, 2
    q, k, v, do = _gen(B, Sq, H * 64, seed=1), _gen(B, Sk, H * 64, seed=2), _gen(B, Sk, H * 64, seed=3), _gen(B, Sq, H * 64, seed=4)
    mask = A.key_mask(Sk)
    assert mask[0].all() and not mask[1].any() and int(mask[2].sum()) == A.ragged_len(Sk)
    for causal in (False, True):
        bias = A.attn_bias(mask, Sq, Sk, causal)
        out, lse, probs = R.attention_ref(q, k, v, bias, H, parts=True)
        s = A._heads(q, H) @ A._heads(k, H).transpose(-1, -2) / 8.0 + bias
        assert float((lse - torch.logsumexp(s, -1)).abs().max()) < 1e-11
        assert float((probs - torch.exp(s - lse.unsqueeze(-1))).abs().max()) < 1e-12
        # batch row 1: every key carries the one -10000, so the row is softmax(raw scores) over the Sk real keys, lse = that - 10000;
        # with q = 0 it is uniform: out = mean(v), lse = log(Sk) - 10000
        raw = A._heads(q, H)[1] @ A._heads(k, H)[1].transpose(-1, -2) / 8.0
        assert float((probs[1] - torch.softmax(raw, -1)).abs().max()) < 1e-12
        assert float((lse[1] - (torch.logsumexp(raw, -1) + A.NEG)).abs().max()) < 1e-10
        q0 = q.clone()
        q0[1] = 0
        out0, lse0, p0 = R.attention_ref(q0, k, v, bias, H, parts=True)
        assert torch.equal(p0[1], torch.full_like(p0[1], 1.0 / Sk))
        assert float((lse0[1] - (math.log(Sk) + A.NEG)).abs().max()) < 1e-11
        assert float((out0[1] - v[1].mean(0, keepdim=True)).abs().max()) < 1e-14


def test_analytic_gradients_equal_autograd():
    B, Sq, Sk, H = 3, 7, 10, 2
    for causal, p in ((False, 0.0), (True, 0.0), (True, 0.3)):
        q, k, v = (_gen(B, s_, H * 64, seed=n).requires_grad_(True) for n, s_ in ((1, Sq), (2, Sk), (3, Sk)))
        do = _gen(B, Sq, H * 64, seed=4)
        bias = A.attn_bias(A.key_mask(Sk), Sq, Sk, causal)
        scale = R.attn_scale(5, 1 << 40, B, H, Sq, Sk, p) if p else None
        R.attention_ref(q, k, v, bias, H, scale=scale).backward(do)
        ref = A.reference(q.detach(), k.detach(), v.detach(), bias, H, do, scale=scale)
        for name, t in (("dq", q), ("dk", k), ("dv", v)):
            assert float((ref[name] - t.grad).abs().max()) < 1e-12 * max(1.0, float(t.grad.abs().max())), name


def test_row_metric():
    ref = torch.zeros(1, 4, 128, dtype=torch.float64)
    ref[0, 0, :64] = 2.0
    ref[0, 1, :64] = 4.0
    ref[0, 0, 64:] = 1.0                    # head 1: rows 1 .. 3 are all-zero reference rows
    got = ref.clone()
    got[0, 1, 3] += 0.04                    # 1 % of that row's maximum
    got[0, 2, 70] = 1e-4                    # an all-zero row of head 1
    e = A.row_err(got, ref, 2)
    assert e.shape == (1, 2, 4)
    floor = (2.0 + 4.0 + 1.0) / 8 * A.FLOOR_FRAC                   # eight (head, row) pairs
    assert abs(float(e[0, 0, 1]) - 0.01) < 1e-12 and abs(float(e[0, 1, 2]) - 1e-4 / floor) < 1e-9
    assert int((e != 0).sum()) == 2
    assert abs(A.whole_err(got, ref) - 0.01) < 1e-12                         # the whole-tensor metric does not see the zero row at all
    z = torch.zeros(1, 2, 64, dtype=torch.float64)
    assert float(A.row_err(z + 3e-3, z, 1).max()) == 3e-3          # a null reference tensor: absolute


def test_noise_floor_model():
    """0 on an exactly representable case; on random data a small value for both dtypes that does not move with the seed; and over the
    shape table the floors the gates are built from."""
    B, Sq, Sk, H = 2, 4, 4, 1
    # one-hot rows in k, v and dout, q = 0: P = 1/4 exactly, every product and sum is a dyadic rational with a few bits
    q = torch.zeros(B, Sq, 64)
    k = torch.zeros(B, Sk, 64)
    v = torch.zeros(B, Sk, 64)
    do = torch.zeros(B, Sq, 64)
    for i in range(4):
        v[:, i, i] = 1.0 + i
        do[:, i, 2 * i] = 0.5 * (i + 1)
        k[:, i, 3 * i + 1] = 2.0
    bias = A.attn_bias(None, Sq, Sk, False)
    ref = A.reference(q, k, v, bias, H, do)
    for dt in (A.F32, A.BF16):
        e = A.errors(A.model(q, k, v, bias, H, do, dt), ref, H)
        assert all(e[k_] == 0.0 for k_ in A.QUANTITIES), e
        assert e["lse"] < 1e-7
    # random data, no mask: fp32 at a few ulp of fp32, bf16 at a few ulp of bf16, whatever the seed
    for dt, lo, hi in ((A.F32, 1e-8, 2e-5), (A.BF16, 1e-3, 4e-2)):
        vals = []
        for seed in (0, 100, 200):
            q, k, v, do = A.operands(20, 37, 2, dt, seed=seed)
            bias = A.attn_bias(None, 20, 37, False)
            e = A.errors(A.model(q, k, v, bias, 2, do, dt), A.reference(q, k, v, bias, 2, do), 2)
            vals.append(e)
            assert all(lo < e[k_] < hi for k_ in A.QUANTITIES), (dt, e)
            assert e["lse"] < 5e-6
        for k_ in A.QUANTITIES:
            assert max(e[k_] for e in vals) < 4 * min(e[k_] for e in vals), (dt, k_, vals)
    # the table's floors: fp32 is set by the fully masked rows (an fp32 score next to -10000 has an ulp of 1e-3), bf16 by its mantissa;
    # dq / dk carry the cancellation residue of rows that see (nearly) one key
    f32, b16 = A.model_floors(A.F32), A.model_floors(A.BF16)
    assert set(f32) == set(b16) == set(A.QUANTITIES) | {"lse"}
    for k_ in ("out", "dv"):
        assert 1e-4 < f32[k_][0] < 3e-3 and 2e-3 < b16[k_][0] < 1.6e-2, (k_, f32[k_], b16[k_])
    assert 1e-4 < f32["lse"][0] < 1.5e-3 and 1e-4 < b16["lse"][0] < 1.5e-3
    assert all(math.isfinite(x[0]) for x in list(f32.values()) + list(b16.values()))
    assert A.gates(A.F32)["out"] == A.MARGIN * f32["out"][0]


def test_shape_table_and_the_exact_zero_share():
    """Every masked case: the keys whose dk / dv must be exactly 0 are at least 10 % of the ragged batch row's keys (Sk = 1 has no
    ragged length below Sk), and the reference is exactly 0 there."""
    ids = [A.case_id(c) for c in A.CASES]
    assert len(set(ids)) == len(ids)
    for case in A.CASES:
        i, causal, dt = case
        Sq, Sk, H, layout, wide, dts, masked = A.TABLE[i]
        assert layout == "split" or Sq == Sk
        d = A.case_data(case)
        z = A.always_blocked(d["mask"], Sq, Sk, causal)
        if masked:
            assert A.ragged_len(Sk) % 2 == 1 and not bool(z[1].any())
            if Sk > 1:
                assert float(z[2].float().mean()) >= 0.1, (A.case_id(case), float(z[2].float().mean()))
        for name in ("dk", "dv"):
            g = d["ref"][name].reshape(A.B, Sk, H * 64)
            assert float(g[z].abs().max()) == 0.0 if bool(z.any()) else True, (A.case_id(case), name)
            assert float(d["model"][name].reshape(A.B, Sk, H * 64)[z].abs().max()) == 0.0 if bool(z.any()) else True
