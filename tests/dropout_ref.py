"""Host restatement of the dropout masks of csrc/common.h (mix32 / dropout_scale) and fp64 references that apply them.

The device mask is a pure integer hash of (seed, stream offset, element index):

    r    = mix32((seed * 0x9E3779B97F4A7C15) ^ (offset * 0xD1B54A32D192ED03 + idx))        64-bit wrap-around arithmetic
    drop = float32(r >> 8) * 2**-24 < float32(p)                                           every step exact in fp32
    kept elements are scaled by float32(1) / (float32(1) - float32(p))

so a test can rebuild the identical mask (bit for bit, not statistically) and ask of a kernel with p > 0 the same agreement with an
fp64 reference that the p = 0 tests ask.  A plain module (no fixtures): tests import it as `dropout_ref`."""
import math

import numpy as np
import torch

MASK64 = (1 << 64) - 1
C_SEED = 0x9E3779B97F4A7C15
C_OFF = 0xD1B54A32D192ED03
C_MIX1 = 0xFF51AFD7ED558CCD
C_MIX2 = 0xC4CEB9FE1A85EC53


def _u64(x):
    """Python ints (any sign, any size: reduced mod 2**64), int64 / uint64 arrays -> uint64 ndarray (at least 1-d)."""
    if isinstance(x, (int, np.integer)):
        return np.array([int(x) & MASK64], dtype=np.uint64)
    a = np.asarray(x)
    if a.dtype == np.uint64:
        return np.atleast_1d(a)
    if a.dtype == object:
        return np.atleast_1d(np.array([int(v) & MASK64 for v in a.ravel()], dtype=np.uint64).reshape(a.shape))
    return np.atleast_1d(a.astype(np.int64).view(np.uint64))


def mix32(x):
    """The murmur3 64-bit finaliser's low word, on a uint64 ndarray."""
    x = _u64(x).copy()
    x ^= x >> np.uint64(33)
    x *= np.uint64(C_MIX1)
    x ^= x >> np.uint64(33)
    x *= np.uint64(C_MIX2)
    x ^= x >> np.uint64(33)
    return (x & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def effective_seed(seed, seed_dev_word=None):
    """(seed + device word) mod 2**64; the device word is int64 storage read as unsigned.  None: the host seed alone."""
    if seed_dev_word is None:
        return int(seed) & MASK64
    return (int(seed) + (int(seed_dev_word) & MASK64)) & MASK64


def keep_mask(seed, offset, idx, p):
    """True where dropout_scale(seed, offset, idx, p, .) keeps the element.  seed / offset: ints or arrays that broadcast with idx."""
    s, o, i = _u64(seed), _u64(offset), _u64(idx)
    key = (s * np.uint64(C_SEED)) ^ (o * np.uint64(C_OFF) + i)          # unsigned array arithmetic wraps mod 2**64
    r = mix32(key)
    u = (r >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    return ~(u < np.float32(p))


def inv_keep(p):
    """The kernels' scale of a kept element, widened to double."""
    if not p > 0:
        return 1.0
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def ln_idx(rows, N):
    """row * N + col: layernorm.hip, ln_body.h, embed.hip."""
    return np.arange(rows, dtype=np.uint64)[:, None] * np.uint64(N) + np.arange(N, dtype=np.uint64)[None, :]


def attn_idx(B, H, Sq, Sk):
    """((b * H + h) * Sq + q) * Sk + key: attn_body.h."""
    bh = np.arange(B * H, dtype=np.uint64).reshape(B, H, 1, 1)
    q = np.arange(Sq, dtype=np.uint64).reshape(1, 1, Sq, 1)
    k = np.arange(Sk, dtype=np.uint64).reshape(1, 1, 1, Sk)
    return (bh * np.uint64(Sq) + q) * np.uint64(Sk) + k


def scale_of(keep, p):
    """bool ndarray -> fp64 torch tensor: 0 where dropped, 1 / (1 - p) (the kernels' fp32 quotient) where kept."""
    return torch.from_numpy(np.ascontiguousarray(keep)).to(torch.float64) * inv_keep(p)


def ln_scale(seed, offset, rows, N, p):
    return scale_of(keep_mask(seed, offset, ln_idx(rows, N), p), p)


def attn_scale(seed, offset, B, H, Sq, Sk, p):
    return scale_of(keep_mask(seed, offset, attn_idx(B, H, Sq, Sk), p), p)


# ----------------------------------------------------------------------------------------- fp64 references
def attention_ref(q, k, v, add_mask, nh, scale=None, parts=False, rnd=None):
    """softmax(Q K^T / sqrt(d) + add_mask) * scale @ V, heads merged.  q [B,Sq,nh*d], k / v [B,Sk,nh*d], add_mask broadcastable to
    [B,nh,Sq,Sk], scale [B,nh,Sq,Sk] (mask * 1/(1-p)) or None.  Written out on its own: at scale=None it must equal the oracle's
    attention_core (tests/test_dropout_ref_cpu.py).

    The arithmetic runs in the operands' dtype.  rnd: applied to the (scaled) probabilities before they meet V -- the rounding of a
    kernel's P operand (tests/attention_ref.py's precision model); None: none.  parts=True: -> (out, lse [B,nh,Sq], probs [B,nh,Sq,Sk]
    before scale and rnd) with lse = max + log(sum exp(. - max)), the row log-sum-exp of the biased scores."""
    B, Sq, HD = q.shape
    Sk = k.shape[1]
    d = HD // nh
    ql = q.reshape(B, Sq, nh, d).permute(0, 2, 1, 3)
    kl = k.reshape(B, Sk, nh, d).permute(0, 2, 1, 3)
    vl = v.reshape(B, Sk, nh, d).permute(0, 2, 1, 3)
    s = ql @ kl.transpose(-1, -2) / math.sqrt(d) + add_mask
    mx = s.max(-1, keepdim=True).values
    s = s - mx
    e = torch.exp(s)
    den = e.sum(-1, keepdim=True)
    probs = e / den
    pv = probs if scale is None else probs * scale
    if rnd is not None:
        pv = rnd(pv)
    out = (pv @ vl).permute(0, 2, 1, 3).reshape(B, Sq, HD)
    if parts:
        return out, (mx + torch.log(den)).squeeze(-1), probs
    return out


def layernorm_ref(x, gamma, beta, residual=None, rowpos=None, scale_pre=None, scale_post=None, eps=1e-12):
    """scale_post * LN(scale_pre * x + residual + rowpos) with the TF-style LayerNorm (biased variance, eps inside the root).
    Returns (y, mean, rstd, out): y is the LayerNorm's input, which the kernels save."""
    y = x if scale_pre is None else x * scale_pre
    if residual is not None:
        y = y + residual
    if rowpos is not None:
        y = y + rowpos
    mean = y.mean(-1, keepdim=True)
    var = ((y - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    out = (y - mean) * rstd * gamma + beta
    if scale_post is not None:
        out = out * scale_post
    return y, mean.squeeze(-1), rstd.squeeze(-1), out
