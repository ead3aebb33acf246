"""The host restatement of the dropout masks (tests/dropout_ref.py) against a scalar restatement in Python integers, and the fp64
references of tests/test_dropout_parity_gpu.py against the oracle at p = 0.  No GPU."""
import random
import struct

import numpy as np
import torch

import dropout_ref as R
import univl_oracle as O

M64 = 2 ** 64


def _f32(x):
    return struct.unpack("f", struct.pack("f", x))[0]


def scalar_keep(seed, offset, idx, p):
    """csrc/common.h: dropout_scale, one element, Python big integers reduced % 2**64 where the device wraps."""
    x = ((seed * 0x9E3779B97F4A7C15) % M64) ^ ((offset * 0xD1B54A32D192ED03 + idx) % M64)
    x ^= x >> 33
    x = (x * 0xFF51AFD7ED558CCD) % M64
    x ^= x >> 33
    x = (x * 0xC4CEB9FE1A85EC53) % M64
    x ^= x >> 33
    r = x % 2 ** 32
    u = (r >> 8) / 16777216.0                     # < 2**24 integers times 2**-24: exact in fp32 and in double
    return not (u < _f32(p))


def _tuples():
    rng = random.Random(7)
    seeds = [0, 1, 42, 2 ** 63, 2 ** 63 + 12345, 2 ** 64 - 1, (42 + 2 ** 63 + 7) % M64] + [rng.getrandbits(64) for _ in range(9)]
    offsets = [0, 3, 11, 12] + [n << 40 for n in (1, 2, 3, 17, 40, 117, 1 << 20)] + [rng.getrandbits(64) for _ in range(3)]
    idxs = ([0, 1, 767, 768, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 2, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 33 + 5]
            + [rng.getrandbits(20) for _ in range(8)] + [2 ** 32 - 1 - rng.getrandbits(10) for _ in range(4)])
    out = [(s, o, i) for s in seeds for o in offsets for i in idxs]
    assert len(out) > 3000
    return out


def test_keep_mask_equals_the_scalar_restatement():
    tup = _tuples()
    assert any(s >= 2 ** 63 for s, _, _ in tup) and any(o and o % (1 << 40) == 0 for _, o, _ in tup)
    assert any(2 ** 32 - 4 <= i <= 2 ** 32 + 4 for _, _, i in tup)
    s = np.array([t[0] for t in tup], dtype=np.uint64)
    o = np.array([t[1] for t in tup], dtype=np.uint64)
    i = np.array([t[2] for t in tup], dtype=np.uint64)
    for p in (0.1, 0.5, 0.9, 1e-3):
        got = R.keep_mask(s, o, i, p)
        want = np.array([scalar_keep(a, b, c, p) for a, b, c in tup])
        assert got.dtype == np.bool_ and got.shape == want.shape
        np.testing.assert_array_equal(got, want)
        assert 0 < want.sum() < want.size
    # scalar seed / offset broadcast over an index array, as the kernel tests call it
    idx = R.ln_idx(5, 768)
    got = R.keep_mask(2 ** 63 + 5, 3 << 40, idx, 0.5)
    want = np.array([[scalar_keep(2 ** 63 + 5, 3 << 40, int(v), 0.5) for v in row] for row in idx])
    np.testing.assert_array_equal(got, want)
    assert abs(got.mean() - 0.5) < 0.03


def test_mix32_known_values_and_the_draw_threshold():
    assert int(R.mix32(0)[0]) == 0 and int(R.mix32(1)[0]) == 0x34C2CB2C              # fmix64(1) = 0xb456bcfc34c2cb2c
    # the threshold is float32(p): 0.1 * 2**24 = 1677721.6 and float32(0.1) * 2**24 = 1677721.625 bracket no integer draw, so the
    # fp32 and the double comparison agree for p = 0.1; the draw itself is an integer below 2**24 times 2**-24, exact in both
    assert 1677721 / 16777216.0 < _f32(0.1) < 1677722 / 16777216.0
    assert R.inv_keep(0.0) == 1.0 and R.inv_keep(0.5) == 2.0
    assert R.inv_keep(0.1) == float(np.float32(1.0) / np.float32(0.9)) and abs(R.inv_keep(0.1) - 1 / 0.9) < 1e-7


def test_effective_seed_and_index_helpers():
    assert R.effective_seed(42) == 42
    assert R.effective_seed(42, 0) == 42
    assert R.effective_seed(42, -(2 ** 63) + 7) == 2 ** 63 + 49                      # int64 storage read as unsigned
    assert R.effective_seed(2 ** 64 - 1, 2) == 1                                     # wraps
    assert R.effective_seed(5, torch.tensor([-1], dtype=torch.int64)[0]) == 4
    a = R.attn_idx(2, 3, 5, 7)
    assert a.shape == (2, 3, 5, 7) and a.dtype == np.uint64
    assert int(a[1, 2, 4, 6]) == ((1 * 3 + 2) * 5 + 4) * 7 + 6
    np.testing.assert_array_equal(a.ravel(), np.arange(2 * 3 * 5 * 7, dtype=np.uint64))
    n = R.ln_idx(4, 768)
    assert int(n[3, 5]) == 3 * 768 + 5 and n.shape == (4, 768)


def _gen(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def test_references_equal_the_oracle_without_dropout():
    B, Sq, Sk, H = 2, 9, 13, 4
    q, k, v = _gen(B, Sq, H * 16, seed=1), _gen(B, Sk, H * 16, seed=2), _gen(B, Sk, H * 16, seed=3)
    mask = torch.ones(B, Sk, dtype=torch.long)
    mask[0, 10:] = 0
    mask[1] = 0                                                                      # fully masked row
    add = O.extended_mask(mask, torch.float64)
    want = O.attention_core(q, k, v, add, H)
    got = R.attention_ref(q, k, v, add, H)
    assert float((got - want).abs().max()) < 1e-14
    ones = torch.ones(B, H, Sq, Sk, dtype=torch.float64)
    assert torch.equal(R.attention_ref(q, k, v, add, H, scale=ones), got)
    x, res, g, b = _gen(11, 768, seed=4), _gen(11, 768, seed=5), 1 + 0.1 * _gen(768, seed=6), 0.1 * _gen(768, seed=7)
    y, mean, rstd, out = R.layernorm_ref(x, g, b, residual=res)
    assert torch.equal(y, x + res)
    assert float((out - O.layer_norm(x + res, g, b)).abs().max()) < 1e-14
    assert float((mean - (x + res).mean(-1)).abs().max()) < 1e-15
    # the mask enters where the kernels apply it: before the residual, after the affine map
    sp, so = R.ln_scale(9, 1 << 40, 11, 768, 0.5), R.ln_scale(9, 2 << 40, 11, 768, 0.5)
    assert not torch.equal(sp, so) and set(sp.unique().tolist()) == {0.0, 2.0}
    y2, _, _, out2 = R.layernorm_ref(x, g, b, residual=res, scale_pre=sp, scale_post=so)
    assert torch.equal(y2, x * sp + res)
    assert float((out2 - so * O.layer_norm(x * sp + res, g, b)).abs().max()) < 1e-14
