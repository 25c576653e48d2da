"""The teeth of test_rect_gpu.py, shown on the float64 reference alone (no GPU).

test_rect_gpu.py runs every convolution and InstanceNorm kernel family on maps whose height and width differ, and the stride-2
layers on odd sizes.  Here three faults of the kind those tests are for are MODELLED on NumPy arrays (oracle/tf_ops_np.py) and
put through the same comparison (util.rect_close: rel-L2 against float64 at the project's fp32 / bf16 tolerances; util.band_untouched
for the guard band behind every output):

  (a) the map read with height and width exchanged in the pixel index (a row pitch taken from the wrong axis);
  (b) the SAME padding's pad_before of the two axes swapped (`pt` / `pl` exchanged) on a stride-2 layer;
  (c) the 16 x 16 output patches placed on a transposed patch grid (patches per column taken from the width), which runs past the end
      of the tensor.

Each is rejected at the rectangles the GPU tests use and passes unnoticed at the square shape of the corresponding existing test --
which is the gap the rectangular module closes.  The unfaulted result, computed in float32 and in bf16-rounded form, is accepted.
"""
import numpy as np
import pytest
import torch

from oracle import tf_ops_np as tn
from util import SENTINEL, band_untouched, guard_elems, rect_close

N, CIN, COUT = 2, 8, 8


def _bf16(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).double().numpy()


def _operands(h, w, k=3, seed=0):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((N, h, w, CIN)), rng.standard_normal((k, k, CIN, COUT)) * 0.1


def _accepts_unfaulted(x, w, stride):
    ref = tn.conv2d_same(x, w, stride)
    assert rect_close(tn.conv2d_same(x.astype(np.float32), w.astype(np.float32), stride), ref, "f32")
    xb, wb = _bf16(x), _bf16(w)
    refb = tn.conv2d_same(xb, wb, stride)
    assert rect_close(_bf16(refb), refb, "bf16")
    return ref


# ---- (a) height and width exchanged in the pixel index
def _conv_hw_exchanged(x, w, stride=1):
    n, h, wd, c = x.shape
    y = tn.conv2d_same(x.reshape(n, wd, h, c), w, stride)          # the same bytes, walked with the other axis as the row pitch
    return y.reshape(n, -(-h // stride), -(-wd // stride), w.shape[-1])


@pytest.mark.parametrize("h,w", [(16, 48), (48, 16), (16, 32), (32, 16)])
def test_exchanged_axes_are_rejected_on_rectangles(h, w):
    x, wt = _operands(h, w)
    ref = _accepts_unfaulted(x, wt, 1)
    for dt in ("f32", "bf16"):
        assert not rect_close(_conv_hw_exchanged(x, wt), ref, dt)


@pytest.mark.parametrize("h", [16, 32])
def test_exchanged_axes_are_invisible_on_squares(h):
    """test_variants_gpu.test_conv3x3_s1_forced_variant: (n, h, h, c) maps only."""
    x, wt = _operands(h, h)
    ref = _accepts_unfaulted(x, wt, 1)
    assert np.array_equal(_conv_hw_exchanged(x, wt), ref)


# ---- (b) pad_before of the two axes swapped
def _conv_pads_swapped(x, w, stride):
    n, h, wd, ci = x.shape
    k = w.shape[0]
    ho, pt, pb = tn.same_pads(h, k, stride)
    wo, pl, pr = tn.same_pads(wd, k, stride)
    pt, pl = pl, pt                                                   # the fault
    pb, pr = max((ho - 1) * stride + k - h - pt, 0), max((wo - 1) * stride + k - wd - pl, 0)
    xp = np.zeros((n, h + pt + pb, wd + pl + pr, ci), x.dtype)
    xp[:, pt:pt + h, pl:pl + wd] = x
    y = np.zeros((n, ho, wo, w.shape[-1]), x.dtype)
    for a in range(k):
        for b in range(k):
            y += xp[:, a:a + (ho - 1) * stride + 1:stride, b:b + (wo - 1) * stride + 1:stride] @ w[a, b]
    return y


@pytest.mark.parametrize("h,w", [(9, 16), (16, 9)])
def test_swapped_pads_are_rejected_at_mixed_parity(h, w):
    assert tn.same_pads(9, 3, 2)[1] == 1 and tn.same_pads(16, 3, 2)[1] == 0
    x, wt = _operands(h, w, seed=1)
    ref = _accepts_unfaulted(x, wt, 2)
    for dt in ("f32", "bf16"):
        assert not rect_close(_conv_pads_swapped(x, wt, 2), ref, dt)


@pytest.mark.parametrize("h", [16, 32, 9])
def test_swapped_pads_are_invisible_on_squares(h):
    """every stride-2 case of the existing suite is an even square (pt == pl == 0); an odd square has pt == pl == 1"""
    x, wt = _operands(h, h, seed=1)
    ref = _accepts_unfaulted(x, wt, 2)
    assert np.array_equal(_conv_pads_swapped(x, wt, 2), ref)


# ---- (c) the patch grid transposed
def _store_patches(y, transposed, p=16):
    """Write y [n, h, w, c] patch by patch into a flat buffer with a guard band, as a tiled kernel's epilogue does: flat patch index
    -> (image, patch row, patch column) -> pixels at row pitch w.  transposed: patches numbered down the columns with the number of
    patches per column taken from the WIDTH (the grid of the transposed map); on a map one patch high a mere renumbering of the
    patches is the identity, so this is the form such a confusion takes there.  Returns (logical tensor, guard band)."""
    n, h, w, c = y.shape
    size, guard = y.size, guard_elems(y.shape)
    buf = np.full(size + guard, SENTINEL)
    rows, cols = h // p, w // p
    for img in range(n):
        for q in range(rows * cols):
            pr, pc = divmod(q, cols)                                  # where the patch's values come from
            tr, tc = (q % cols, q // cols) if transposed else (pr, pc)
            for r in range(p):
                o = ((img * h + tr * p + r) * w + tc * p) * c
                if o + p * c <= buf.size:                             # (the model stops at the end of the guard band)
                    buf[o:o + p * c] = y[img, pr * p + r, pc * p:(pc + 1) * p].ravel()
    return buf[:size].reshape(y.shape), buf[size:]


@pytest.mark.parametrize("h,w", [(16, 48), (48, 16)])
def test_transposed_patch_grid_is_rejected_on_rectangles(h, w):
    x, wt = _operands(h, w, seed=2)
    ref = _accepts_unfaulted(x, wt, 1)
    good, band = _store_patches(ref, False)
    assert np.array_equal(good, ref) and band_untouched(band)
    bad, band = _store_patches(ref, True)
    for dt in ("f32", "bf16"):
        assert not rect_close(bad, ref, dt)
    if h < w:                   # patches of the last image land behind the tensor: the guard band shows it without a fault
        assert not band_untouched(band)


@pytest.mark.parametrize("h", [16, 32])
def test_transposed_patch_grid_is_invisible_on_one_patch_squares(h):
    """(3, 16, 64, 0, 64) of test_conv3x3_s1_forced_variant is one patch per image; on the 2 x 2 patches of a 32 x 32 map the grid
    has the same extent both ways, and only the numbering differs -- which the float64 comparison does see."""
    x, wt = _operands(h, h, seed=2)
    ref = _accepts_unfaulted(x, wt, 1)
    bad, band = _store_patches(ref, True)
    assert band_untouched(band)
    if h == 16:
        assert np.array_equal(bad, ref)
    else:
        assert bad.shape == ref.shape and np.array_equal(np.sort(bad.ravel()), np.sort(ref.ravel()))      # every value stored, inside the tensor
