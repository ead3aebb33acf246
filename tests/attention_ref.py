"""fp64 reference, per-row error metric and precision-model noise floor for the attention kernels (csrc/attention.hip, csrc/attn_body.h),
and the shape table of tests/test_attention_edges_gpu.py.  A plain module (no fixtures, no GPU): tests import it as `attention_ref`.

The forward is dropout_ref.attention_ref (one statement of the math, shared with the dropout tests); this file adds the additive bias as
the kernels build it, the analytic backward, and the two things a gate needs:

  * row_err: one number per (batch, head, row) -- max |got - ref| over the head's 64 columns divided by max(max |ref| over that row,
    floor), floor = FLOOR_FRAC times the tensor's mean row maximum.  The floor only keeps a row whose reference is (nearly) zero from
    dividing by zero; a whole-tensor max|a-b| / max|b| hides a wrong short row or a wrong head slice under the largest element.
  * the precision model: the SAME reference evaluated in fp32 with the kernels' roundings (below), compared with fp64 under the same
    metric.  Gates are MARGIN times the model's worst value over the whole shape table, per dtype and quantity -- the reference's own
    error at the kernel's precision, never the kernel's output.

Roundings of the model (attn_body.h):
    fp32   everything in torch fp32: scores, the -10000 bias added to an fp32 score (1e-3 ulp at 1e4: the fully masked rows), softmax,
           lse, and the backward's P = exp(score - lse) from the fp32 lse.
    bf16   the same fp32 arithmetic on bf16 operands (fp32 accumulation), and bf16 roundings of: the (dropped) P that meets V and dO,
           dS, out (also as the backward reads it for rowsum(dO * out)), dq, dk, dv.
What the model cannot reproduce -- MFMA accumulation order, the device expf / logf -- is what MARGIN is for."""
import functools
import math

import torch

import dropout_ref as R

D = 64                       # head width of the kernels
NEG = -10000.0               # additive bias of a blocked key (module_bert.py: (1 - mask) * -10000); never -20000
FLOOR_FRAC = 1e-3            # row_err: floor = FLOOR_FRAC * mean over rows of max |ref|
NULL_TENSOR = 1e-9           # row_err: a reference tensor whose mean row maximum is below this is zero to rounding
MARGIN = 4.0                 # gate = MARGIN * the model's worst value over the table
QUANTITIES = ("out", "dq", "dk", "dv")


def gen(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def attn_bias(mask, Sq, Sk, causal):
    """[B,1,Sq,Sk] fp64 additive bias as key_bias() builds it: NEG where the key is masked OR (causal) key > q -- one NEG, not a sum --
    else 0.  mask: [B,Sk] {0,1} or None.  Nothing is added beyond Sk: the padded keys do not exist for the reference."""
    B = 1 if mask is None else mask.shape[0]
    blocked = torch.zeros(B, 1, Sq, Sk, dtype=torch.bool)
    if mask is not None:
        blocked = blocked | (mask[:, None, None, :] == 0)
    if causal:
        blocked = blocked | torch.triu(torch.ones(Sq, Sk, dtype=torch.bool), diagonal=1)[None, None]
    return blocked.double() * NEG


def bf16_round(x):
    return x.to(torch.bfloat16).to(x.dtype)


def _heads(x, nh):
    B, S, _ = x.shape
    return x.reshape(B, S, nh, D).permute(0, 2, 1, 3)


def _merge(x):
    B, nh, S, _ = x.shape
    return x.permute(0, 2, 1, 3).reshape(B, S, nh * D)


def forward_backward(q, k, v, bias, nh, dout, scale=None, dtype=torch.float64, rnd=None):
    """out, lse, dq, dk, dv of  out = (softmax(q k^T / 8 + bias) * scale) v  under the upstream gradient dout, evaluated in `dtype`
    with `rnd` applied where the bf16 kernels round (None: nowhere).  q, dout [B,Sq,nh*64], k, v [B,Sk,nh*64]: the operands as the
    kernel sees them (already rounded to the compute type); scale [B,nh,Sq,Sk] keep / (1 - p) or None.  Results are fp64 tensors.

    The backward is the kernels' formulation: P is rebuilt from lse, dS = P * (dP * scale - rowsum(dO * out)), and
    dq = dS k / 8, dk = dS^T q / 8, dv = (P * scale)^T dO.  In fp64 with rnd=None this is the exact gradient (checked against autograd
    in tests/test_attention_ref_cpu.py)."""
    one = (lambda x: x) if rnd is None else rnd
    q, k, v, dout, bias = (t.to(dtype) for t in (q, k, v, dout, bias))
    scale = None if scale is None else scale.to(dtype)
    out, lse, _ = R.attention_ref(q, k, v, bias, nh, scale=scale, parts=True, rnd=rnd)
    out = one(out)
    ql, kl, vl, dol, ol = (_heads(t, nh) for t in (q, k, v, dout, out))
    s = ql @ kl.transpose(-1, -2) / math.sqrt(D) + bias
    p = torch.exp(s - lse.unsqueeze(-1))
    dsum = (dol * ol).sum(-1, keepdim=True)
    dp = dol @ vl.transpose(-1, -2)
    pd = p
    if scale is not None:
        dp = dp * scale
        pd = p * scale
    ds = one(p * (dp - dsum))
    pd = one(pd)
    dq = one((ds @ kl) / math.sqrt(D))
    dk = one((ds.transpose(-1, -2) @ ql) / math.sqrt(D))
    dv = one(pd.transpose(-1, -2) @ dol)
    return dict(out=out.double(), lse=lse.double(), dq=_merge(dq).double(), dk=_merge(dk).double(), dv=_merge(dv).double())


def reference(q, k, v, bias, nh, dout, scale=None):
    return forward_backward(q, k, v, bias, nh, dout, scale=scale)


def model(q, k, v, bias, nh, dout, dtype, scale=None):
    """The reference at the kernel's precision: dtype torch.float32 or torch.bfloat16 (the kernel's compute type)."""
    return forward_backward(q, k, v, bias, nh, dout, scale=scale, dtype=torch.float32,
                            rnd=bf16_round if dtype == torch.bfloat16 else None)


def row_err(got, ref, nh):
    """[B,S,nh*64] x 2 -> [B,nh,S]: per (batch, head, row) max |got - ref| over the 64 columns / max(max |ref| of the row, floor).
    A reference that is zero to rounding as a WHOLE (dq and dk at Sk = 1: a softmax over one key is constant) has no scale of its own:
    there the floor is 1 and the number is the absolute error, in units of the O(1) operands."""
    B, S, _ = ref.shape
    g, r = got.double().reshape(B, S, nh, D), ref.double().reshape(B, S, nh, D)
    num = (g - r).abs().amax(-1)
    den = r.abs().amax(-1)
    mean = float(den.mean())
    floor = mean * FLOOR_FRAC if mean > NULL_TENSOR else 1.0
    return (num / den.clamp(min=floor)).permute(0, 2, 1)


def whole_err(got, ref):
    """The suite's whole-tensor metric (test_kernels_gpu.rel_err)."""
    a, b = got.double(), ref.double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def errors(got, ref, nh):
    """Worst per-row error of out / dq / dk / dv and the worst absolute lse error, of whatever `got` holds."""
    e = {k_: float(row_err(got[k_], ref[k_], nh).max()) for k_ in QUANTITIES if k_ in got}
    if "lse" in got:
        e["lse"] = float((got["lse"].double() - ref["lse"]).abs().max())
    return e


# ------------------------------------------------------------------------------------------------------ shape table
# B = 3 everywhere: batch row 0 full length, row 1 FULLY masked (uniform over the Sk real keys, causal or not: every key carries the one
# NEG), row 2 ragged with an odd valid length.  Crossed: the pad boundaries of both dtypes (16 / 32), every MAXKT tier from both sides
# (Sk 64 | 65, 127 | 129, 255 | 257), one block | two blocks of 64 in the queries and in the keys independently, the backward's small ->
# large and DUAL -> single-image switches (both at 64 padded positions), Sq > Sk, and the LDS limits (383 bf16; 256 fp32 with a mask --
# the one shape added to the issue's table: the limit itself was only run unmasked).
B = 3
F32, BF16 = torch.float32, torch.bfloat16
#         Sq   Sk   H  layout    wide   dtypes        masked
TABLE = [(1, 1, 3, "packed", False, (F32, BF16), True),
         (7, 1, 3, "split", False, (F32, BF16), True),
         (1, 7, 3, "split", True, (F32, BF16), True),
         (17, 33, 3, "split", True, (F32, BF16), True),
         (17, 33, 3, "split", False, (F32, BF16), False),
         (33, 17, 3, "split", False, (F32, BF16), True),
         (63, 64, 3, "split", False, (F32, BF16), True),
         (64, 65, 3, "split", True, (F32, BF16), True),
         (64, 65, 3, "split", False, (F32, BF16), False),
         (65, 63, 3, "split", False, (F32, BF16), True),
         (127, 129, 3, "split", False, (F32, BF16), True),
         (129, 127, 3, "split", True, (F32, BF16), True),
         (5, 255, 3, "split", False, (F32, BF16), True),
         (255, 255, 3, "packed", False, (F32, BF16), True),
         (256, 256, 3, "packed", False, (F32,), True),
         (193, 257, 3, "split", False, (BF16,), True),
         (257, 31, 3, "split", True, (BF16,), True),
         (383, 383, 3, "packed", False, (BF16,), True),
         (48, 48, 12, "packed", True, (F32, BF16), True)]
CASES = [(i, causal, dt) for i, row in enumerate(TABLE) for causal in (False, True) for dt in row[5]]


def case_id(case):
    i, causal, dt = case
    Sq, Sk, H, layout, wide, _, masked = TABLE[i]
    return "%dx%d-H%d-%s%s%s%s-%s" % (Sq, Sk, H, layout, "-wide" if wide else "", "" if masked else "-nomask", "-causal" if causal else "",
                                      "bf16" if dt == BF16 else "f32")


def ragged_len(Sk):
    """Odd valid length of batch row 2 that leaves at least 10 % of the keys masked (Sk = 1 has no such length: 1)."""
    n = Sk - math.ceil(0.1 * Sk)
    n -= 1 - n % 2
    return max(n, 1)


def key_mask(Sk):
    lens = torch.tensor([Sk, 0, ragged_len(Sk)])
    return (torch.arange(Sk)[None] < lens[:, None]).long()


def operands(Sq, Sk, H, dtype, seed=0):
    """q [B,Sq,H*64], k, v [B,Sk,H*64], dout [B,Sq,H*64] as fp32 tensors that hold values of `dtype` exactly."""
    q, k, v, do = (gen(B, s_, H * D, seed=seed + 10 * n).to(dtype).float() for n, s_ in enumerate((Sq, Sk, Sk, Sq), 1))
    return q, k, v, do


def always_blocked(mask, Sq, Sk, causal):
    """[B,Sk] bool: keys that EVERY query of the batch row blocks (masked, or under causal beyond the last query), in batch rows that
    are not fully masked.  There every probability is exp(-10000 - lse) = 0 in fp32 and in fp64, so dk and dv are exactly 0."""
    blk = torch.zeros(B, Sk, dtype=torch.bool) if mask is None else (mask == 0)
    if causal:
        blk = blk | (torch.arange(Sk)[None] > Sq - 1)
    if mask is not None:
        blk = blk & (mask.sum(1, keepdim=True) > 0)
    return blk


@functools.lru_cache(maxsize=None)
def case_data(case):
    """-> dict(q, k, v, dout, mask, bias, ref, model): computed once per case and shared (the GPU tests, the gates, the CPU tests)."""
    i, causal, dt = case
    Sq, Sk, H, _, _, _, masked = TABLE[i]
    q, k, v, do = operands(Sq, Sk, H, dt, seed=i)
    mask = key_mask(Sk) if masked else None
    bias = attn_bias(mask, Sq, Sk, causal)
    ref = reference(q, k, v, bias, H, do)
    return dict(q=q, k=k, v=v, dout=do, mask=mask, bias=bias, ref=ref, model=model(q, k, v, bias, H, do, dt))


@functools.lru_cache(maxsize=None)
def model_floors(dtype):
    """{quantity: (worst model-vs-fp64 value over the table, the case it comes from)} for out / dq / dk / dv (per-row metric) and lse
    (absolute)."""
    worst = {}
    for case in CASES:
        if case[2] != dtype:
            continue
        d = case_data(case)
        for k_, e in errors(d["model"], d["ref"], TABLE[case[0]][2]).items():
            if k_ not in worst or e > worst[k_][0]:
                worst[k_] = (e, case_id(case))
    return worst


def gates(dtype):
    return {k_: MARGIN * e for k_, (e, _) in model_floors(dtype).items()}
