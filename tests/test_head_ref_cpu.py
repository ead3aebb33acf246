"""tests/head_ref.py against the oracle at the shapes tests/test_kernels_gpu.py already uses, the conditions its input builders
promise at every shape of tests/test_head_kernels_gpu.py, and the choice of the MFM reference.  No GPU."""
import pytest
import torch

import head_ref as R
import univl_oracle as O


def _oracle(f, x):
    x = x.double().requires_grad_(True)
    loss = f(x)
    loss.backward()
    return float(loss.detach()), x.grad


def _gen(*shape, seed, scale):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


@pytest.mark.parametrize("n", [4, 16, 37])
def test_maxmargin_and_crossen_helpers_reproduce_the_oracle(n):
    sim = _gen(n, n, seed=1, scale=0.5)
    for f, direct in ((R.maxmargin_f(n), lambda s: O.max_margin_ranking_loss(s, 0.1, 1, n, 1, 0.5)), (R.crossen_f(), O.cross_en)):
        g = R.gate(f, sim)
        loss, grad = _oracle(direct, sim)
        assert g.ref_loss == loss and torch.equal(g.ref_grad, grad)
        assert g.loss == R.FLOOR and g.grad == R.FLOOR


@pytest.mark.parametrize("bs,npair", [(2, 3), (4, 1), (5, 2)])
def test_milnce_helper_reproduces_the_oracle(bs, npair):
    sim = _gen(bs * npair, bs * npair, seed=2, scale=2.0)
    g = R.gate(R.milnce_f(bs, npair), sim)
    loss, grad = _oracle(lambda s: O.mil_nce_loss(s, bs, npair), sim)
    assert g.ref_loss == loss and torch.equal(g.ref_grad, grad)
    assert g.loss == R.FLOOR and g.grad == R.FLOOR


def test_weighted_maxmargin_helper_and_the_weight_matrix():
    bs, npair = 3, 2
    sim = _gen(bs * npair, bs * npair, seed=3, scale=0.5)
    g = R.gate(R.maxmargin_f(bs, npair, weighted=True), sim)
    loss, grad = _oracle(lambda s: O.max_margin_ranking_loss(s, 0.1, 1, bs, npair, 0.5), sim)
    assert g.ref_loss == loss and torch.equal(g.ref_grad, grad)
    # the explicit matrix handed to the kernel is the one the oracle multiplies by
    w = R.simloss_weights(bs, npair)
    explicit = (R.hinge_arguments(sim).clamp(min=0).sum(0) * w.double()).mean()
    assert abs(float(explicit) - loss) < 1e-12
    w = R.simloss_weights(*R.WEIGHTED_SHAPE)
    # two distinct values, one of them not an integer: an fp32 sum of them depends on its order
    assert len(set(w.reshape(-1).tolist())) == 2 and any(v != round(v) for v in set(w.reshape(-1).tolist()))


def test_ce_helper_reproduces_the_oracle_and_keeps_labels_in_range():
    T, V = 50, 1002
    logits = _gen(T, V, seed=1, scale=3.0)
    labels = torch.randint(0, V, (T,), generator=torch.Generator().manual_seed(2))
    labels[::5] = -1
    g = R.gate(R.ce_f(labels), logits)
    loss, grad = _oracle(lambda x: O.cross_entropy_ignore(x, labels), logits)
    assert g.ref_loss == loss and torch.equal(g.ref_grad, grad)
    assert g.loss == R.FLOOR and g.grad == R.FLOOR
    for V in (1, 3, 1002):
        for rows in (1, 300):
            for ignore in (-1, 0):
                x, lab = R.ce_input(rows, V, ignore, seed=7)
                assert x.shape == (rows, V) and bool(((lab == ignore) | ((lab >= 0) & (lab < V))).all())
                if rows > 1:
                    assert {0, V - 1} <= set(lab.tolist()) and 4 * ((V - 1) // 4) in set(lab.tolist())
                    assert float(x[1].max()) == 80.0 and float(x[1].min()) == (-80.0 if V > 1 else 80.0)
                    assert float(x[3].min()) == float(x[3].max())


def test_mfm_helper_reproduces_the_expression_of_the_existing_test():
    B, F = 3, 8
    n = B * F
    logits = _gen(n, n, seed=1, scale=2.0)
    vmask = (torch.arange(F)[None] < torch.tensor([[8], [3], [5]])).long()
    lab = torch.full((n,), -1, dtype=torch.int64)
    lab[[1, 4, 9, 17, 20]] = torch.tensor([1, 4, 1, 1, 4])
    assert R.n_selected_padded(vmask, lab) == 0
    x = logits.double().requires_grad_(True)
    vm = vmask.reshape(-1).double()
    masked = x + (1.0 - vm.view(-1, 1) @ vm.view(1, -1)) * -1e8
    ref = (-torch.diag(torch.log_softmax(masked, dim=-1)))[lab != -1].mean()
    ref.backward()
    g = R.gate(R.mfm_f(lab), R.mfm_masked32(logits, vmask))
    assert R.loss_err(g.ref_loss, ref.detach()) < 1e-12 and R.grad_err(g.ref_grad, x.grad) < 1e-12
    assert g.loss == R.FLOOR and g.grad == R.FLOOR


@pytest.mark.parametrize("scale", R.SCALES)
def test_maxmargin_builder_condition_holds_at_every_gpu_shape(scale):
    for n in R.SIM_SIZES + [R.WEIGHTED_SHAPE[0] * R.WEIGHTED_SHAPE[1]]:
        sim = R.maxmargin_input(n, scale, R.SIM_SEED)          # asserts min |argument| >= 1e-3 itself
        arg = R.hinge_arguments(sim)
        assert float(arg.abs().min()) >= 0.00625 - 1e-9
        # fp32 (margin + x - d, left to right, as the kernel evaluates it) and fp64 agree on every hinge
        d = torch.diag(sim)
        a32 = torch.stack([(R.MARGIN + sim) - d.view(-1, 1), (R.MARGIN + sim) - d.view(1, -1)])
        assert torch.equal(a32 > 0, arg > 0)
        assert torch.equal(sim * 64, torch.round(sim * 64))


@pytest.mark.parametrize("n", [257, 513])
def test_gate_stays_at_its_floor_for_benign_scales(n):
    cases = [("maxmargin", R.maxmargin_f(n), R.maxmargin_input(n, 0.5, R.SIM_SEED)),
             ("crossen", R.crossen_f(), R.sim_input(n, 0.5, R.SIM_SEED))]
    cases += [("milnce %dx%d" % s, R.milnce_f(*s), R.sim_input(s[0] * s[1], 0.5, R.SIM_SEED)) for s in R.MIL_SHAPES if n == 257]
    for name, f, x in cases:
        g = R.gate(f, x)
        assert g.loss == R.FLOOR and g.grad == R.FLOOR, (name, g.e32_loss, g.e32_grad)
        assert g.e32_loss > 0 or g.e32_grad > 0, name          # the fp32 evaluation really is a different computation


def test_gate_is_eight_times_the_fp32_error_above_the_floor():
    x = torch.tensor([[0.0, 1.0], [2.0, 3.0]])
    f = lambda t: (t * (1.0 + 2.0 ** -16)).sum() if t.dtype == torch.float64 else t.sum() * 1.0      # a known relative gap
    g = R.gate(f, x)
    assert abs(g.e32_loss - 2.0 ** -16) < 1e-9 and g.loss == 8 * g.e32_loss and g.loss > R.FLOOR


def test_mfm_masking_variants_agree_without_selected_padded_rows_and_differ_with_them():
    B, F = 11, 48
    lengths = R.MFM_CASES[(B, F)]
    x, vmask, labels = R.mfm_input(B, F, lengths, R.MFM_SEED, selected_padded=False)
    assert R.n_selected_padded(vmask, labels) == 0 and int((labels != -1).sum()) > 20
    f = R.mfm_f(labels)
    g = R.gate(f, R.mfm_masked32(x, vmask))
    l64, g64 = R.evaluate(f, R.mfm_masked64(x, vmask))
    assert R.loss_err(l64, g.ref_loss) < 1e-6 and R.grad_err(g64, g.ref_grad) < 1e-6
    x, vmask, labels = R.mfm_input(B, F, lengths, R.MFM_SEED, selected_padded=True)
    assert R.n_selected_padded(vmask, labels) >= 10
    f = R.mfm_f(labels)
    g = R.gate(f, R.mfm_masked32(x, vmask))
    l64, g64 = R.evaluate(f, R.mfm_masked64(x, vmask))
    assert abs(float(l64) - g.ref_loss) > 1e-2, (float(l64), g.ref_loss)
    assert R.grad_err(g64, g.ref_grad) > 1e-2
    assert g.loss == R.FLOOR and g.grad == R.FLOOR             # the fp32-faithful form is as well-conditioned as the plain one


def test_mfm_inputs_cover_the_clip_lengths_and_the_selection_rate():
    for (B, F), lengths in R.MFM_CASES.items():
        x, vmask, labels = R.mfm_input(B, F, lengths, R.MFM_SEED, selected_padded=False)
        n = B * F
        assert x.shape == (n, n) and vmask.shape == (B, F) and labels.shape == (n,)
        assert vmask.sum(1).tolist() == lengths
        assert bool(((labels == -1) | ((labels >= 0) & (labels < F))).all())
        if n > 1:
            assert {0, 1, F} <= set(lengths)
            _, _, drawn = R.mfm_input(B, F, lengths, R.MFM_SEED, selected_padded=True)
            assert abs(int((drawn != -1).sum()) - n / 7) <= 1
