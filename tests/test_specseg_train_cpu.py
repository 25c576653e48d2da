"""The reference of SpecSeg training (specseg_train_ref.py) against itself, without a GPU: the hand-written pool backward against
autograd on tied windows, the loss's written-out gradient against autograd, and every case of test_specseg_train_gpu.py's tables in the
branch it claims."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import specseg_train_ref as R
from oracle.specseg_torch import init_specseg, specseg_spec


@pytest.mark.parametrize("ties", R.POOL_TIES)
@pytest.mark.parametrize("hw", R.POOL_SIZES)
def test_hand_pool_backward_is_autograd(hw, ties):
    x, dy = R.pool_case(3, hw[0], hw[1], ties)
    t = torch.from_numpy(x).double().permute(0, 3, 1, 2).requires_grad_(True)
    F.max_pool2d(t, 2).backward(torch.from_numpy(dy).double().permute(0, 3, 1, 2))
    ref = t.grad.permute(0, 2, 3, 1).numpy()
    got = R.pool_bwd_first_max(x.astype(np.float64), dy.astype(np.float64))
    assert np.array_equal(got, ref)
    assert (np.count_nonzero(got.reshape(3, hw[0] // 2, 2, hw[1] // 2, 2, 16), axis=(2, 4)) <= 1).all()


@pytest.mark.parametrize("ties", R.POOL_TIES)
def test_pool_cases_tie_as_claimed(ties):
    x, _ = R.pool_case(1, 16, 16, ties)
    win = x.reshape(1, 8, 2, 8, 2, 16).transpose(0, 1, 3, 5, 2, 4).reshape(-1, 4)
    nmax = (win == win.max(1, keepdims=True)).sum(1)
    if ties == "all_equal":
        assert (nmax == 4).all()
    elif ties == "none":
        assert (nmax == 1).all() and np.unique(win).size == win.size
    else:
        assert (nmax == 2).all()
        seen = {tuple(np.flatnonzero(r == r.max())) for r in win}
        assert seen == set(R.PAIRS)                    # every position pair ties somewhere


@pytest.mark.parametrize("logits", R.LOSS_LOGITS)
@pytest.mark.parametrize("mask", R.LOSS_MASKS)
@pytest.mark.parametrize("npix", R.LOSS_NPIX)
def test_loss_gradient_is_autograd(npix, mask, logits):
    z, g = R.loss_case(npix, mask, logits)
    zt = torch.from_numpy(z).double().requires_grad_(True)
    L = R.seg_loss(zt, torch.from_numpy(g).double())
    L["loss"].backward()
    got = R.seg_loss_grad(zt.detach(), torch.from_numpy(g).double())
    assert torch.isfinite(L["loss"]) and torch.isfinite(got).all()
    scale = max(float(zt.grad.abs().max()), 1e-300)
    assert float((got - zt.grad).abs().max()) / scale < 1e-12
    if mask != "soft":
        assert all(float(L[k]) == round(float(L[k])) for k in ("tp", "fp", "fn"))
        assert float(L["tp"] + L["fp"] + L["fn"]) <= npix


def test_loss_cases_are_where_they_claim():
    assert [R.loss_blocks(n) for n in R.LOSS_NPIX] == [1, 1, 5]          # one thread, a ragged single block, several blocks with a ragged last
    z, _ = R.loss_case(255, "soft", "pm40")
    assert set(np.unique(z)) == {-40.0, 40.0}
    # |z| = 40: 1 - sigmoid(z) is 0 in float32, the naive log(1 - p) is -inf; the softplus form is finite
    assert float(1 - torch.sigmoid(torch.tensor(40.0))) == 0.0
    assert float(R.seg_loss(torch.tensor([40.0]), torch.tensor([0.0]))["focal"]) == pytest.approx(30.0)


def test_bn_cases_are_where_they_claim():
    assert {c[0] for c in R.BN_CASES} == {1, 3, 30, 1024} and {c[1] for c in R.BN_CASES} == {16, 256}
    assert R.chan_blocks(1, 16) == 1 and R.chan_blocks(1024, 16) == 4 and R.chan_blocks(1024, 256) == 64 and R.chan_blocks(30, 256) == 2
    a = R.bn_case(1024, 16, "offset")[0].astype(np.float64)
    assert abs(a.mean() - 1e3) < 1 and 0.9 < a[:, 0].std() < 1.1 and a[:, 1].std() == 0
    # the one-pass formula E[a^2] - E[a]^2 in float32 loses the variance at this offset; two passes keep it
    a32 = a.astype(np.float32)
    naive = (a32 * a32).mean(0, dtype=np.float32) - a32.mean(0, dtype=np.float32) ** 2
    assert np.abs(naive[0] - a[:, 0].var()) > 1e-3
    # moving statistics: the unbiased estimate, and n = 1 does not divide by zero
    mm, mv = R.bn_moving(0.0, 1.0, 2.0, 3.0, 4)
    assert mm == pytest.approx(0.02) and mv == pytest.approx(0.99 + 0.01 * 4.0)
    assert R.bn_moving(0.0, 1.0, 2.0, 0.0, 1)[1] == pytest.approx(0.99)


def test_convt_cases_are_where_they_claim():
    assert {(c[1], c[2]) for c in R.CONVT_CASES} >= {(1, 1), (1, 3), (5, 7), (16, 16)}
    assert {c[0] for c in R.CONVT_CASES} == {1, 3} and {c[3] for c in R.CONVT_CASES} == {16, 128}
    assert R.convt_split(1, 1, 1) == (1, 1, 1)              # one ragged chunk
    assert R.convt_split(3, 5, 7) == (2, 2, 1)              # 105 pixels: a ragged second chunk
    assert R.convt_split(3, 16, 16) == (12, 12, 1)
    assert R.convt_split(3, 32, 24) == (36, 18, 2)          # more than one chunk per split
    # the einsum restatement is the Conv2DTranspose of the inference oracle
    x, k = torch.randn(2, 3, 5, 32, dtype=torch.float64), torch.randn(2, 2, 16, 32, dtype=torch.float64)
    y = R.convt_fwd(x, k)
    assert float((y[:, 1::2, 0::2] - torch.einsum("nhwc,oc->nhwo", x, k[1, 0])).abs().max()) < 1e-12


def test_adam_step_is_the_clip_kernels_formula():
    w, m, v, g = (np.array([0.5, -0.25]), np.zeros(2), np.zeros(2), np.array([3.0, -0.5]))
    a = R.adam_alpha(1e-3, 0.9, 0.999, 0)
    w1, m1, v1 = R.adam_step(w, m, v, g, a, 0.9, 0.999, 1e-7, clip=1.0)
    assert m1 == pytest.approx([0.1, -0.05]) and v1 == pytest.approx([1e-3, 2.5e-4])
    assert w1 == pytest.approx(w - 1e-3 * np.sign(g), rel=1e-5)          # the first Adam step moves every weight by lr
    assert R.adam_step(w, m, v, g, a, 0.9, 0.999, 1e-7)[1] == pytest.approx([0.3, -0.05])


NET_CASES = {"S16_B1": (1, 16, 16), "S16_B3": (3, 16, 16), "16x48_B2": (2, 16, 48), "S32_B2": (2, 32, 32)}
# at one sample on a 16 x 16 map the bottleneck is 1 x 1: BatchNormalization over one value returns beta whatever its input, so the fifth
# pair's kernels and biases and that layer's gamma have a gradient of exactly zero (variables 32..36); nothing else may vanish
STRUCTURAL_ZEROS = {"S16_B1": {32, 33, 34, 35, 36}}


@pytest.mark.parametrize("name", NET_CASES)
def test_reference_gradients_do_not_vanish(name):
    n, H, W = NET_CASES[name]
    x, mask = R.discs(n, max(H, W), seed=5)
    x, mask = x[:, :H, :W], mask[:, :H, :W]
    L, grads, moving = R.loss_and_grads(init_specseg(trained_like=True), x, mask, R.random_keep((n, H, W), 7))
    assert np.isfinite(L["loss"]) and len(grads) == len(specseg_spec()) == 66 and sum(g is not None for g in grads) == 56
    zero = {i for i, g in enumerate(grads) if g is not None and not np.any(g)}
    assert zero == STRUCTURAL_ZEROS.get(name, set())
    assert len(moving) == 5


def test_reference_trajectory_learns_the_discs():
    """the step count and lr of the device's behaviour test, chosen here: the float64 reference's last loss is below half its first"""
    TRAJ = R.TRAJ
    x, mask = R.discs(TRAJ["B"], TRAJ["S"], seed=TRAJ["data_seed"])
    keeps = [R.random_keep((TRAJ["B"], TRAJ["S"], TRAJ["S"]), [3, t]) for t in range(TRAJ["steps"])]
    losses, _ = R.trajectory(init_specseg(trained_like=True), [x] * TRAJ["steps"], [mask] * TRAJ["steps"], keeps, TRAJ["lr"])
    print(losses)
    assert losses[-1] < 0.5 * losses[0]


def test_shape_errors_are_raised_on_the_host_before_any_launch():
    """SHM_E_SHAPE (-1) / SHM_E_WORKSPACE (-3) of the new entry points need no GPU: nothing is launched"""
    from shmgan_amd import _lib
    L = _lib.lib()
    p = 16                                             # a non-null pointer nobody dereferences
    big = 1 << 30
    assert L.shm_bn_train_fwd(p, 24, p, p, None, None, 0.99, 1e-3, p, 24, p, p, big, 8, 24, None) == -1 and b"power of two" in L.shm_last_error()
    assert L.shm_bn_train_fwd(p, 16, p, p, None, None, 0.99, 1e-3, p, 18, p, p, big, 8, 16, None) == -1 and b"pitches" in L.shm_last_error()
    assert L.shm_bn_train_fwd(p, 16, p, p, None, None, 0.99, 1e-3, p, 16, p, p, 8, 8, 16, None) == -3 and b"workspace" in L.shm_last_error()
    assert L.shm_bn_train_fwd(p, 16, p, p, None, None, 0.99, 1e-3, p, 16, p, p, big, 0, 16, None) == -1
    assert L.shm_bn_train_bwd(p, 16, p, 16, p, p, p, 16, p, None, p, big, 8, 16, None) == -1 and b"null" in L.shm_last_error()
    assert L.shm_bn_train_bwd(p, 16, p, 16, p, p, p, 16, p, p, p, 8, 8, 16, None) == -3
    assert L.shm_maxpool2_bwd(p, 16, p, 16, p, 16, 1, 3, 4, 16, 0, None) == -1 and b"bad size" in L.shm_last_error()
    assert L.shm_maxpool2_bwd(p, 16, p, 16, p, 12, 1, 2, 2, 16, 0, None) == -1
    assert L.shm_conv2d_transpose2x2_dgrad(p, 16, p, p, 48, 1, 4, 4, 48, 16, None) == -1 and b"multiple of 32" in L.shm_last_error()
    assert L.shm_conv2d_transpose2x2_dgrad(p, 16, p, p, 16, 1, 4, 4, 32, 16, None) == -1 and b"pitches" in L.shm_last_error()
    n = L.shm_conv2d_transpose2x2_wgrad_workspace(3, 32, 24, 32, 16)
    assert n == 256 * 16 * 8 + 18 * 4 * 16 * 32 * 4 and L.shm_conv2d_transpose2x2_wgrad_workspace(0, 1, 1, 32, 16) == 0
    assert L.shm_conv2d_transpose2x2_wgrad(p, 32, p, 16, p, p, p, n - 1, 3, 32, 24, 32, 16, None) == -3
    assert L.shm_conv2d_transpose2x2_wgrad(p, 32, p, 16, p, p, p, big, 3, 32, 24, 32, 24, None) == -1
    assert L.shm_head_logit_fwd(p, 16, p, None, p, 8, 12, None) == -1
    assert L.shm_head_logit_bwd(p, 16, p, p, p, 16, p, p, p, 8, 8, 16, None) == -3
    assert L.shm_seg_loss(p, p, None, p, p, big, 0, None) == -1 and b"no pixels" in L.shm_last_error()
    assert L.shm_seg_loss(p, p, None, p, p, 8, 4, None) == -3
    assert L.shm_adam(None, p, p, p, 4, 1e-3, 0.9, 0.999, 1e-7, 1.0, 0.0, None) == -1 and L.shm_adam(None, None, None, None, 0, 1e-3, 0.9, 0.999, 1e-7, 1.0, 0.0, None) == 0
