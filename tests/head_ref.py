"""fp64 references, input builders and the tolerance gate for the similarity losses, the MFM / vocabulary losses and the small
cross-encoder head kernels (csrc/simloss.hip, csrc/cross.hip, csrc/embed.hip).

Every loss is stated once as a formula `f(x)` that works in the dtype of `x`; `gate(f, x)` evaluates it in torch fp32 and in fp64 on
the same fp32 inputs, hands back the fp64 loss and gradient as the reference, and derives the tolerance from the fp32 evaluation's
own distance to fp64 -- never from the kernel under test:

    gate = max(1e-5, 8 * e32)        loss:      |d| / max(1, |ref|)
                                     gradient:  max |d| / max |ref|

1e-5 is what tests/test_kernels_gpu.py asks of the same kernels at toy sizes; the factor 8 leaves room for the kernel's expf and its
different summation order.  A plain module (no fixtures): tests import it as `head_ref`."""
from collections import namedtuple

import numpy as np
import torch

import univl_oracle as O

FLOOR = 1e-5
MARGIN = 0.1

Gate = namedtuple("Gate", "loss grad e32_loss e32_grad ref_loss ref_grad")

# the shapes of tests/test_head_kernels_gpu.py (tests/test_head_ref_cpu.py checks the builders' conditions on the same lists)
SIM_SIZES = [1, 256, 257, 513]                 # one trip, exactly one trip, a second trip, a third trip of the j += 256 loops
SCALES = [0.5, 30.0]                           # normalised similarities; un-normalised ones (use_mil) reach tens
MIL_SHAPES = [(257, 1), (129, 2), (86, 3)]     # (batch, n_pair)
WEIGHTED_SHAPE = (86, 3)                       # negative weighting needs n_pair > 1: n = 258
SIM_SEED = 11
MFM_CASES = {                                  # (B, F): clip lengths (0, 1 and F among them)
    (1, 1): [1],
    (6, 48): [48, 0, 1, 17, 48, 30],
    (11, 48): [48, 0, 1, 5, 48, 33, 20, 48, 7, 40, 12],
}
MFM_SEED = 5


# ------------------------------------------------------------------------------------------------ metrics and the gate
def loss_err(a, ref):
    return abs(float(a) - float(ref)) / max(1.0, abs(float(ref)))


def grad_err(a, ref):
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    return float((a - ref).abs().max() / (ref.abs().max() + 1e-30))


def evaluate(f, x):
    x = x.detach().clone().requires_grad_(True)
    loss = f(x)
    loss.backward()
    return loss.detach(), x.grad


def gate(f, x):
    """x: fp32 tensor.  Returns the gates for the loss and the gradient, the e32 each came from and the fp64 reference itself."""
    assert x.dtype == torch.float32
    l32, g32 = evaluate(f, x)
    l64, g64 = evaluate(f, x.double())
    e_l, e_g = loss_err(l32, l64), grad_err(g32, g64)
    return Gate(max(FLOOR, 8 * e_l), max(FLOOR, 8 * e_g), e_l, e_g, float(l64), g64)


# ------------------------------------------------------------------------------------------------ similarity losses
def sim_input(n, scale, seed):
    return torch.randn(n, n, generator=torch.Generator().manual_seed(seed)) * scale


def hinge_arguments(sim, margin=MARGIN):
    """Both relu arguments of MaxMarginRankingLoss, in fp64."""
    s = sim.double()
    d = torch.diag(s)
    return torch.stack([margin + s - d.view(-1, 1), margin + s - d.view(1, -1)])


def maxmargin_input(n, scale, seed, margin=MARGIN):
    """Similarities on the 1/64 grid: every hinge argument is margin + k/64, at least 0.00625 away from zero for margin 0.1, so fp32
    and fp64 agree on which hinges are active.  The assertion is a condition on the inputs, not a tolerance."""
    sim = torch.round(sim_input(n, scale, seed) * 64) / 64
    assert float(hinge_arguments(sim, margin).abs().min()) >= 1e-3
    return sim


def simloss_weights(bs, n_pair, hard_negative_rate=0.5):
    """The weight matrix of negative weighting as steps.SimLoss builds it (until_module.py:238-243)."""
    easy = 1 - hard_negative_rate
    alpha = easy / ((bs - 1) * (1 - easy))
    mm = np.kron((1 - alpha) * np.eye(bs) + alpha, np.ones((n_pair, n_pair))) * (bs * (1 - easy))
    return torch.tensor(mm, dtype=torch.float32).contiguous()


def maxmargin_f(bs, n_pair=1, weighted=False, margin=MARGIN, hard_negative_rate=0.5):
    return lambda x: O.max_margin_ranking_loss(x, margin, 1 if weighted else 0, bs, n_pair, hard_negative_rate)


def crossen_f():
    return O.cross_en


def milnce_f(bs, n_pair):
    return lambda x: O.mil_nce_loss(x, bs, n_pair)


# ------------------------------------------------------------------------------------------------ vocabulary CE
def ce_f(labels, ignore_index=-1):
    return lambda x: O.cross_entropy_ignore(x, labels, ignore_index=ignore_index)


def ce_input(rows, V, ignore_index, seed, scale=30.0):
    """Logits at scale 30 with (from four rows on) a one-hot row at +-80 whose label is the hot column, one whose label is a cold
    column, and a row of equal logits.  Labels sit at 0, at V - 1 and inside the 4-wide group that holds V - 1; every label is in
    [0, V) or equal to ignore_index (the kernels do not check them)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, V, generator=g) * scale
    labels = torch.randint(0, V, (rows,), generator=g)
    if rows == 1:
        labels[0] = V - 1
    else:
        if ignore_index == -1:
            labels[::5] = -1
        group = list(range(4 * ((V - 1) // 4), V))
        for k, r in enumerate(range(6, rows, 7)):
            labels[r] = ([0, V - 1] + group)[k % (2 + len(group))]
        hot = V // 2
        x[1] = -80.0; x[1, hot] = 80.0; labels[1] = hot
        x[2] = -80.0; x[2, hot] = 80.0; labels[2] = (hot + 1) % V
        x[3] = 7.0; labels[3] = V - 1
    assert bool(((labels >= 0) & (labels < V) | (labels == ignore_index)).all())
    return x, labels


# ------------------------------------------------------------------------------------------------ MFM NCE
def mfm_masked32(x, vmask):
    """The reference model's masked matrix, formed as it forms it: ONE fp32 add of (1 - m m^T) * -1e8 (modeling.py:285-288)."""
    assert x.dtype == torch.float32
    vm = vmask.reshape(-1).float()
    return x + (1.0 - vm.view(-1, 1) @ vm.view(1, -1)) * -1e8


def mfm_masked64(x, vmask):
    """The same mask applied in fp64: NOT the same operation when a selected row's own frame is padded (at -1e8 the fp32 spacing is 8:
    the fp32 add loses x, the fp64 add keeps it)."""
    vm = vmask.reshape(-1).double()
    return x.double() + (1.0 - vm.view(-1, 1) @ vm.view(1, -1)) * -1e8


def mfm_f(labels):
    """Of the masked matrix: d loss / d x equals d loss / d masked."""
    sel = labels.reshape(-1) != -1
    return lambda m: (-torch.diag(torch.log_softmax(m, dim=-1)))[sel].mean()


def mfm_input(B, F, lengths, seed, selected_padded, scale=2.0):
    """Logits [B*F, B*F], the frame mask of clips of the given lengths, and labels that select about one row in seven.  selected_padded
    False: no selected row's own frame is padded; True: the selection is kept as drawn, padded rows included (asserted to exist)."""
    assert len(lengths) == B and all(0 <= k <= F for k in lengths)
    n = B * F
    x = torch.randn(n, n, generator=torch.Generator().manual_seed(seed)) * scale
    vmask = (torch.arange(F)[None] < torch.tensor(lengths)[:, None]).long()
    labels = torch.full((n,), -1, dtype=torch.int64)
    pick = (torch.arange(n) * 3 + seed) % 7 == 0
    labels[pick] = torch.arange(n)[pick] % F
    if n == 1:
        labels[0] = 0
    padded = vmask.reshape(-1) == 0
    if selected_padded:
        assert int(((labels != -1) & padded).sum()) > 0
    else:
        labels[padded] = -1
    return x, vmask, labels


def n_selected_padded(vmask, labels):
    return int(((labels.reshape(-1) != -1) & (vmask.reshape(-1) == 0)).sum())
