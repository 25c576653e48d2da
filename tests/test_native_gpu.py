"""Native-resolution test mode on the GPU (shmgan_amd.evaluate.test(eval_size="native")): the four new entry points against the
float64 restatement (tests/native_ref.py), the generator and SpecSeg on rectangular frames against the oracle, trainer.infer on a
frame, and the mode end to end.  Frames: (32, 48), (48, 32) -- one side at the minimum -- and (80, 32), an odd count of 16-blocks;
sources 37 x 53 (pads 11 / 11), 33 x 95 and 64 x 48 (no pad)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import specseg_torch as sp
from oracle import step_torch as st
from shmgan_amd import _lib, ops
from shmgan_amd import evaluate as ev

import export_ref as xr
import native_ref as nr
from util import SENTINEL, band_untouched, dev, host, rel_l2

pytestmark = pytest.mark.gpu

FRAMES = [(32, 48), (48, 32), (80, 32)]
SOURCES = [(37, 53), (33, 95), (64, 48)]
F32, FBF = 16, 32                # the smallest filter counts the float32 / bfloat16 generators take
BF16_FWD = 2e-2                  # rel-L2 of a bfloat16 forward (tests/test_bf16_gpu.py)


# ---------------------------------------------------------------------------------------------------- shared, read-only
@pytest.fixture(scope="module")
def params():
    g, _, gb, _ = st.init_params(F32, 32)
    return g, gb, sp.init_specseg(seed=3)


@pytest.fixture(scope="module")
def params_bf():
    g, _, gb, _ = st.init_params(FBF, 32)
    return g, gb


def _trainer(F=F32, **kw):
    from shmgan_amd import ShmGANwithSSpecSeg
    return ShmGANwithSSpecSeg(image_size=32, filter_size=F, batch_size=1, **kw).build()


@pytest.fixture(scope="module")
def m32(params):
    m = _trainer()
    m.SpecSeg.set_weights(params[2])
    return m


@pytest.fixture(scope="module")
def frames():
    rng = np.random.default_rng(77)
    return {hw: rng.uniform(0, 1, (2,) + hw + (3,)).astype(np.float32) for hw in FRAMES}


@pytest.fixture(scope="module")
def oracle_g1(params, frames):
    """The oracle's G1 pass (gen_Y, gen_rgb, SpecSeg mask) of every frame, computed once."""
    g, gb, sw = params
    return {hw: nr.infer_hw(g, gb, x, F32, specseg=sw, cyclic=False) for hw, x in frames.items()}


# ------------------------------------------------------------------------------------------------------ 1. load_pad_u8
@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("h,w", SOURCES)
@pytest.mark.parametrize("misalign", [0, 1])
def test_load_pad_u8_is_bit_equal_to_the_reflected_bytes(h, w, c, misalign):
    rng = np.random.default_rng(1000 * h + 10 * w + c)
    u8 = rng.integers(0, 256, (h, w, c), dtype=np.uint8)
    want, (top, left, _, _) = nr.load_pad_u8(u8)
    hp, wp = want.shape[:2]
    n, guard = hp * wp * c, 16 * wp * c
    flat = torch.full((misalign + n + guard,), SENTINEL, dtype=torch.float32, device="cuda")
    dst = flat[misalign:misalign + n].view(hp, wp, c)
    assert dst.data_ptr() % 16 == (4 * misalign) % 16
    ops.load_pad_u8(torch.from_numpy(u8).cuda(), dst, top, left, 1.0 / 255.0)
    got = dst.cpu().numpy()
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert band_untouched(flat[misalign + n:]) and band_untouched(flat[:misalign])


def test_load_pad_u8_refuses_bad_geometry_before_any_launch():
    u8 = torch.zeros((37, 53, 3), dtype=torch.uint8, device="cuda")
    dst = torch.full((48, 64, 3), SENTINEL, device="cuda")
    for top, left in ((12, 5), (5, 12), (-1, 0)):
        with pytest.raises(_lib.ShmError, match="inside"):
            ops.load_pad_u8(u8, dst, top, left)
    with pytest.raises(_lib.ShmError, match="pad wider"):
        ops.load_pad_u8(u8[:4].contiguous(), dst[:16].contiguous(), 6, 5)
    torch.cuda.synchronize()
    assert band_untouched(dst)


# --------------------------------------------------------------------------------------- 2. generator and SpecSeg on frames
def _gen_input(yuv_y, dtype, pad):
    """[n,H,W,1] float64 -> the generator's padded input as infer builds it for G1 (views 1..4 zero, one-hot = ED)."""
    n, H, W, _ = yuv_y.shape
    x = np.zeros((n, H, W, pad), np.float32)
    x[..., 0:1] = yuv_y
    x[..., 9] = 1.0
    return torch.from_numpy(x).cuda().to(dtype)


@pytest.mark.parametrize("hw", FRAMES)
def test_generator_and_specseg_forward_fp32_on_frames(hw, m32, params, frames, oracle_g1):
    g, gb, sw = params
    x = frames[hw]
    yuv, _ = st.per_image_standardization(st.rgb_to_yuv(torch.from_numpy(x).double()))
    y = m32.G.forward(_gen_input(yuv[..., 0:1].numpy(), torch.float32, 16), "t_native")
    err = np.abs(host(y) - oracle_g1[hw]["gen_Y"].numpy()).max()
    mask = m32.SpecSeg.forward_plane(dev(yuv.numpy()), 3, 0, 2, tag="t_native/specseg")
    merr = np.abs(host(mask) - oracle_g1[hw]["mask"].numpy()).max()
    print(f"frame {hw}: generator max-abs {err:.3e}, SpecSeg mask max-abs {merr:.3e}")
    assert tuple(y.shape) == (2,) + hw + (1,) and tuple(mask.shape) == (2,) + hw + (1,)
    assert err < 1e-4
    assert merr < 1e-5
    with pytest.raises(AssertionError, match="square"):       # training stays square: the backward refuses a frame
        m32.G.backward(torch.zeros_like(y), "t_native")
    m32.arena.drop("t_native")


@pytest.fixture(scope="module")
def mbf():
    return _trainer(FBF, compute_dtype="bfloat16")


@pytest.mark.parametrize("hw", FRAMES)
def test_generator_forward_bf16_on_frames(hw, params_bf, frames, mbf):
    g, gb = params_bf
    m = mbf
    x = frames[hw]
    yuv, _ = st.per_image_standardization(st.rgb_to_yuv(torch.from_numpy(x).double()))
    zeros, ones = torch.zeros_like(yuv[..., 0:1]), torch.ones_like(yuv[..., 0:1])
    ref = st.generator_forward([torch.from_numpy(a).double() for a in g], [torch.from_numpy(b).double() for b in gb],
                               torch.cat([yuv[..., 0:1]] + [zeros] * 8 + [ones], dim=3), FBF)
    y = m.G.forward(_gen_input(yuv[..., 0:1].numpy(), torch.bfloat16, 32), "t_native")
    r = rel_l2(host(y), ref.numpy())
    print(f"frame {hw}: bf16 generator rel-L2 {r:.3e}")
    assert r < BF16_FWD
    m.arena.drop("t_native")


@pytest.mark.parametrize("dt", ["float32", "bfloat16"])
def test_infer_with_live_attention_on_a_frame(dt, frames):
    """attention="live": the frame's SpecSeg mask goes through the four attention branches (shm_mask_pool_pack_hw) into the skips."""
    F = F32 if dt == "float32" else FBF
    hw = (32, 48)
    m = _trainer(F, compute_dtype=dt, attention="live")
    sw = sp.init_specseg(seed=3)
    m.SpecSeg.set_weights(sw)
    g, _, gb, _ = st.init_params(F, 32)
    att = st.init_attention(F, bias_std=0.05)["G"]           # non-trivial biases, as tests/test_attention_gpu.py: the maps are not small
    keras = []                                                # Keras order: a level's attention variables follow its two convolutions
    for lvl in range(4):
        keras += g[4 * lvl:4 * lvl + 4] + att[4 * lvl:4 * lvl + 4]
    m.G.set_weights(keras + g[16:])
    ref = nr.infer_hw(g, gb, frames[hw], F, specseg=sw, attention=att, cyclic=False)
    plain = nr.infer_hw(g, gb, frames[hw], F, cyclic=False)
    gen_rgb, cyc = m.infer(frames[hw], cyclic=False)
    got = host(gen_rgb)
    assert cyc == [None] * 5 and m.cyc_genED_rgb is None
    err, r = np.abs(got - ref["gen_rgb"].numpy()).max(), rel_l2(host(m.gen_Y), ref["gen_Y"].numpy())
    moved = np.abs(ref["gen_rgb"].numpy() - plain["gen_rgb"].numpy()).max()
    print(f"{dt} live attention on {hw}: gen_rgb max-abs {err:.3e}, gen_Y rel-L2 {r:.3e}; the branch moves gen_rgb by {moved:.3e}")
    assert moved > 1e-3                                        # the branch is live: the check below can tell
    if dt == "float32":
        assert err < 1e-4
        assert np.abs(host(m.specular_candidate) - ref["mask"].numpy()).max() < 1e-5
    else:
        assert r < BF16_FWD
    m.release()


@pytest.mark.parametrize("k", [1, 2, 4, 8])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_mask_pool_pack_hw(k, dt):
    B, H, W, ld = 2, 32, 48, 64 // torch.empty((), dtype=dt).element_size()
    mask = np.random.default_rng(k).uniform(0, 1, (B, H, W, 1)).astype(np.float32)
    n = B * (H // k) * (W // k) * ld
    flat = torch.full((n + 16 * ld,), SENTINEL, dtype=dt, device="cuda")
    dst = flat[:n].view(B, H // k, W // k, ld)
    ops.mask_pool_pack_hw(dev(mask), dst, B, H, W, k)
    want = torch.nn.functional.max_pool2d(torch.from_numpy(mask).permute(0, 3, 1, 2), k).permute(0, 2, 3, 1)
    assert torch.equal(dst[..., 0].float().cpu(), want[..., 0].to(dt).float())
    assert not dst[..., 1:].float().abs().max().item() and band_untouched(flat[n:])
    sq = torch.empty((B, H // k, H // k, ld), dtype=dt, device="cuda")          # the square call is the h = w case
    ops.mask_pool_pack(dev(mask[:, :, :H]), sq, B, H, k)
    sq2 = torch.empty_like(sq)
    ops.mask_pool_pack_hw(dev(mask[:, :, :H]), sq2, B, H, H, k)
    assert torch.equal(sq, sq2)


# -------------------------------------------------------------------------------------------------- 3. infer on a frame
def test_infer_cyclic_on_a_frame(m32, params, frames):
    g, gb, sw = params
    hw = (32, 48)
    ref = nr.infer_hw(g, gb, frames[hw], F32, specseg=sw)
    gen_rgb, cyc = m32.infer(frames[hw], cyclic=True)
    torch.cuda.synchronize()
    errs = [np.abs(host(gen_rgb) - ref["gen_rgb"].numpy()).max()] + [np.abs(host(cyc[k]) - ref["cyc_rgb"][k].numpy()).max() for k in range(5)]
    print("infer on (32, 48): max-abs of gen_rgb and the five cyclic images", ["%.2e" % e for e in errs])
    assert max(errs) < 1e-4
    # the attributes of the square path: gen_Y is G1's plane, not whatever the cyclic passes left in the shared buffers
    assert m32.gen_rgb is gen_rgb and tuple(m32.gen_Y.shape) == (2, 32, 48, 1) and tuple(m32.gen_input.shape) == (2, 32, 48, 16)
    yerr = np.abs(host(m32.gen_Y) - ref["gen_Y"].numpy()).max()
    print(f"gen_Y after the cyclic passes: max-abs {yerr:.2e}")
    assert yerr < 1e-4
    assert np.abs(ref["gen_Y"].numpy() - st.rgb_to_yuv(ref["cyc_rgb"][4])[..., 0:1].numpy()).max() > 1e-2    # ... which is another plane
    x = np.zeros((2, 32, 48, 10))                              # gen_input: view 0 = the standardised Y, one-hot = ED
    x[..., 0:1] = st.per_image_standardization(st.rgb_to_yuv(torch.from_numpy(frames[hw]).double()))[0][..., 0:1].numpy()
    x[..., 9] = 1.0
    assert np.abs(host(m32.gen_input)[..., :10] - x).max() < 1e-5
    assert "inf1" not in m32.G.ctx                             # no record describes a cyclic pass as G1
    for a, b in zip((m32.cyc_gen0_rgb, m32.cyc_gen45_rgb, m32.cyc_gen90_rgb, m32.cyc_gen135_rgb, m32.cyc_genED_rgb), cyc):
        assert a is b and tuple(a.shape) == (2, 32, 48, 3)
    assert len(m32.stddev_arr) == 1 and np.abs(host(m32.stddev_arr[0]) - ref["scale"].numpy()).max() < 1e-6
    assert np.abs(host(m32.specular_candidate) - ref["mask"].numpy()).max() < 1e-5
    for bad in ((2, 16, 48, 3), (2, 40, 48, 3), (2, 32, 48, 4)):
        with pytest.raises(ValueError):
            m32.infer(np.zeros(bad, np.float32))


def test_square_infer_keeps_the_batched_cyclic_pass(m32):
    """(H, W) == (S, S) is today's path: one batched cyclic pass under the same arena names."""
    rgb = np.random.default_rng(2).uniform(0, 1, (2, 32, 32, 3)).astype(np.float32)
    m32.infer(rgb)
    names = {k[0] for k in m32.arena.t}
    assert {"inf/in", "inf/rgb", "inf/cyc_in", "inf/cyc_rgb", "inf1/y", "inf5/y"} <= names
    assert tuple(m32.G.ctx["inf5"]["y"].shape) == (10, 32, 32, 1)


# ------------------------------------------------------------------------------------------------- 4. image_metrics_hw
def _check(got, ref):
    """The tolerances of tests/test_metrics_gpu.py."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert np.all(np.abs(got[:, 0] - ref[:, 0]) <= 1e-5 * np.abs(ref[:, 0])), (got[:, 0], ref[:, 0])
    assert np.all(np.abs(got[:, 1] - ref[:, 1]) <= 1e-4), (got[:, 1], ref[:, 1])
    assert np.all(np.abs(got[:, 2] - ref[:, 2]) <= 5e-5), (got[:, 2], ref[:, 2])
    for k in (3, 4):
        assert np.all(np.abs(got[:, k] - ref[:, k]) <= 1e-4 * np.abs(ref[:, k])), (k, got[:, k], ref[:, k])


def _metric_case(h, w, B=2):
    rng = np.random.default_rng(7 * h + w)
    hp, wp, top, left = nr.pad_geometry(h, w)
    pred = rng.uniform(-0.3, 1.3, (B, hp, wp, 3)).astype(np.float32)
    target = rng.uniform(-0.3, 1.3, (B, h, w, 3)).astype(np.float32)
    return pred, target, (top, left, h, w)


@pytest.mark.parametrize("h,w", SOURCES)
def test_image_metrics_hw_on_the_window(h, w):
    pred, target, win = _metric_case(h, w)
    out = ops.image_metrics_hw(dev(pred), win, dev(target))
    assert out.dtype == torch.float64 and tuple(out.shape) == (2, 5)
    got = host(out)
    _check(got, nr.metrics_hw(pred, win, target))
    # nothing outside the window enters: NaN in the pad changes no bit
    poisoned = np.full_like(pred, np.nan)
    top, left = win[:2]
    poisoned[:, top:top + h, left:left + w] = pred[:, top:top + h, left:left + w]
    assert (h, w) == pred.shape[1:3] or np.isnan(poisoned).any()
    assert np.array_equal(host(ops.image_metrics_hw(dev(poisoned), win, dev(target))), got)
    # batch invariance, bitwise
    for b in range(2):
        one = host(ops.image_metrics_hw(dev(pred[b:b + 1]), win, dev(target[b:b + 1])))
        assert np.array_equal(one[0], got[b]), b
    assert np.array_equal(host(ops.image_metrics_hw(dev(pred), win, dev(target))), got)


def test_image_metrics_hw_full_frame_equals_the_square_call():
    rng = np.random.default_rng(3)
    g = rng.uniform(-0.3, 1.3, (2, 37, 37, 3)).astype(np.float32)
    t = rng.uniform(-0.3, 1.3, (2, 37, 37, 3)).astype(np.float32)
    sq, hw = host(ops.image_metrics(dev(g), dev(t))), host(ops.image_metrics_hw(dev(g), (0, 0, 37, 37), dev(t)))
    _check(hw, sq)
    assert np.array_equal(hw, sq)            # the same kernels in the same order


def test_image_metrics_hw_error_codes_before_any_launch():
    pred = torch.zeros((1, 48, 64, 3), device="cuda")
    out = torch.full((1, 5), SENTINEL, dtype=torch.float64, device="cuda")
    with pytest.raises(_lib.ShmError, match="< 11"):
        ops.image_metrics_hw(pred, (0, 0, 10, 53), torch.zeros((1, 10, 53, 3), device="cuda"), out=out)
    with pytest.raises(_lib.ShmError, match="outside"):
        ops.image_metrics_hw(pred, (12, 5, 37, 53), torch.zeros((1, 37, 53, 3), device="cuda"), out=out)
    with pytest.raises(_lib.ShmError, match="outside"):
        ops.image_metrics_hw(pred, (5, 12, 37, 53), torch.zeros((1, 37, 53, 3), device="cuda"), out=out)
    torch.cuda.synchronize()
    assert band_untouched(out)


# ---------------------------------------------------------------------------------------------------- 5. export_u8_hw
def _unpack(out, offs, sizes, chans):
    o = out.cpu().numpy()
    return [o[off:off + h * w * c].reshape(h, w, c) for off, (h, w), c in zip(offs, sizes, chans)]


def test_export_u8_hw_copy_with_clip_is_exact():
    """Copy geometry: the window's own size.  Values are byte values / 255 (what the loader produces) with some below 0 and above 1,
    so no product lies near a rounding tie and every byte must equal the float64 reference's."""
    rng = np.random.default_rng(12)
    planes, wins, sizes, chans, want = [], [], [], [], []
    for (h, w), c, ld in zip(SOURCES, (3, 1, 3), (3, 1, 4)):
        hp, wp, top, left = nr.pad_geometry(h, w)
        x = (rng.integers(0, 256, (hp, wp, ld)).astype(np.float32) * np.float32(1 / 255.0))
        x[rng.uniform(size=x.shape) < 0.05] = -0.3
        x[rng.uniform(size=x.shape) < 0.05] = 1.4
        planes.append(dev(x)[..., :c] if ld > c else dev(x))
        wins.append((top, left, h, w))
        sizes.append((h, w))
        chans.append(c)
        want.append(nr.export_hw(x[..., :c], wins[-1], h, w, "clip"))
    out, offs = ops.export_u8_hw(planes, wins, sizes, ["clip"] * 3)
    for g, (b, y), win in zip(_unpack(out, offs, sizes, chans), want, wins):
        assert not xr.near_half(y).any()
        assert np.array_equal(g, b), win


def _resample_jobs(rng):
    mul_h = np.array([0.8, 1.3], np.float32)
    spec = [((48, 64), (5, 5, 37, 53), (40, 48), 3, 3, "rescale"), ((48, 96), (7, 0, 33, 95), (66, 190), 1, 1, ("scale", 1)),
            ((64, 48), (0, 0, 64, 48), (17, 23), 3, 4, "rescale"), ((48, 64), (5, 5, 37, 53), (37, 53), 3, 3, ("scale", 0)),
            ((48, 96), (7, 0, 33, 95), (33, 95), 1, 1, "rescale")]
    planes, hosts = [], []
    for (hs, ws), win, size, c, ld, mode in spec:
        x = rng.uniform(-0.4, 1.4, (hs, ws, ld)).astype(np.float32)
        planes.append(dev(x)[..., :c] if ld > c else dev(x))
        hosts.append(x[..., :c])
    return spec, planes, hosts, mul_h


def test_export_u8_hw_rescale_and_scale_with_resampling():
    rng = np.random.default_rng(21)
    spec, planes, hosts, mul_h = _resample_jobs(rng)
    wins, sizes, modes, chans = [s[1] for s in spec], [s[2] for s in spec], [s[5] for s in spec], [s[3] for s in spec]
    out, offs = ops.export_u8_hw(planes, wins, sizes, modes, dev(mul_h))
    left_out = total = 0
    for j, (g, x) in enumerate(zip(_unpack(out, offs, sizes, chans), hosts)):
        m = modes[j]
        b, y = nr.export_hw(x, wins[j], *sizes[j], "scale", float(mul_h[m[1]])) if isinstance(m, tuple) else nr.export_hw(x, wins[j], *sizes[j], m)
        near = xr.near_half(y)
        d = np.abs(g.astype(np.int64) - b.astype(np.int64))
        assert np.all(d[~near] == 0), (j, int((d[~near] != 0).sum()))
        assert np.all(d <= 1), j
        left_out += int(near.sum())
        total += near.size
    print(f"export: {left_out} of {total} bytes within 1e-3 of a rounding tie ({100.0 * left_out / total:.2f} %)")
    assert left_out <= 0.01 * total
    # RESCALE takes its range over the window: poison the pad of job 0 with values far outside
    x = hosts[0].copy()
    big = np.full_like(x, 50.0)
    big[5:42, 5:58] = x[5:42, 5:58]
    out2, o2 = ops.export_u8_hw([dev(big)], [wins[0]], [sizes[0]], ["rescale"])
    assert np.array_equal(_unpack(out2, o2, [sizes[0]], [3])[0], _unpack(out, offs, sizes, chans)[0])


def test_export_u8_hw_jobs_are_independent_and_checked():
    rng = np.random.default_rng(8)
    spec, planes, _, mul_h = _resample_jobs(rng)
    wins, sizes, modes, chans = [s[1] for s in spec], [s[2] for s in spec], [s[5] for s in spec], [s[3] for s in spec]
    mul = dev(mul_h)
    full, offs = ops.export_u8_hw(planes, wins, sizes, modes, mul)
    ref = _unpack(full, offs, sizes, chans)
    for j in range(len(planes)):
        alone, o1 = ops.export_u8_hw([planes[j]], [wins[j]], [sizes[j]], [modes[j]], mul)
        assert np.array_equal(_unpack(alone, o1, [sizes[j]], [chans[j]])[0], ref[j]), j
    perm = [3, 0, 4, 2, 1]
    sh, o2 = ops.export_u8_hw([planes[i] for i in perm], [wins[i] for i in perm], [sizes[i] for i in perm], [modes[i] for i in perm], mul)
    for g, i in zip(_unpack(sh, o2, [sizes[i] for i in perm], [chans[i] for i in perm]), perm):
        assert np.array_equal(g, ref[i]), i
    # a full window of a square plane is the square call
    sq = dev(rng.uniform(-0.4, 1.4, (32, 32, 3)).astype(np.float32))
    a, oa = ops.export_u8([sq], [(40, 48)], ["rescale"])
    b, ob = ops.export_u8_hw([sq], [(0, 0, 32, 32)], [(40, 48)], ["rescale"])
    assert np.array_equal(_unpack(a, oa, [(40, 48)], [3])[0], _unpack(b, ob, [(40, 48)], [3])[0])
    with pytest.raises(ValueError, match="window"):
        ops.export_u8_hw([planes[0]], [(12, 5, 37, 53)], [(37, 53)], ["clip"])
    L = _lib.lib()
    import ctypes as C
    desc = (C.c_size_t * 13)(48, 64, 3, 3, 5, 12, 37, 53, 37, 53, 2, 0, 0)
    src = (C.c_void_p * 1)(planes[0].data_ptr())
    rc = L.shm_export_u8_hw(src, desc, 1, None, 0, full.data_ptr(), full.numel(), full.data_ptr(), 1 << 20, None)
    assert rc == -1 and b"window" in L.shm_last_error()


# ------------------------------------------------------------------------------------------------------ 6. end to end
def _folder(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(3)
    data = {"test": [], "diffuse": []}
    for sub in data:
        (tmp_path / sub).mkdir()
        for i, (h, w) in enumerate((SOURCES[0], SOURCES[2], SOURCES[1])):
            a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
            Image.fromarray(a).save(tmp_path / sub / f"img{i}.png")
            data[sub].append(a)
    return data


def _e2e_trainer(tmp_path, tag):
    from shmgan_amd import ShmGANwithSSpecSeg
    return ShmGANwithSSpecSeg(image_size=32, filter_size=F32, batch_size=1, checkpoint_save_dir=str(tmp_path / "ckpt"),
                              log_dir=str(tmp_path / f"logs_{tag}"), result_dir=str(tmp_path / f"results_{tag}")).build()


def _args(tmp_path, **kw):
    return SimpleNamespace(test_dir=str(tmp_path / "test"), diffuse_dir=str(tmp_path / "diffuse"), calc_metrics=True,
                           eval_batch_size=1, **kw)


@pytest.mark.filterwarnings("ignore:no checkpoint")
def test_native_mode_end_to_end(tmp_path, params):
    from PIL import Image
    data = _folder(tmp_path)
    m = _e2e_trainer(tmp_path, "native")
    g, gb, _ = params
    r = ev.test(m, _args(tmp_path, eval_size="native", save_images="all", image_out_size="model"), print_fn=lambda *a: None)
    assert r["images"] == 3 and r["index"] == [1, 2, 3] and len(r["time"]) == 3 and len(r["files"]) == 3 * len(ev.IMAGE_TAGS)
    # every written PNG has its source's size (image_out_size is ignored)
    for i, a in enumerate(data["test"]):
        for tag in ev.IMAGE_TAGS:
            with Image.open(tmp_path / "results_native" / "images" / f"img{i}_{tag}.png") as im:
                assert (im.size[1], im.size[0]) == a.shape[:2], (i, tag, im.size)
    # metrics against the restatement: the oracle's inference on the reflected frame, scored on the window
    want = []
    for a, d in zip(data["test"], data["diffuse"]):
        frame, win = nr.load_pad_u8(a)
        ref = nr.infer_hw(g, gb, frame[None], F32, cyclic=False)
        want.append(nr.metrics_hw(ref["gen_rgb"].numpy(), win, (d.astype(np.float32) * np.float32(1 / 255.0))[None])[0])
    got = np.array([[r[k][i] for k in ev.METRIC_KEYS] for i in range(3)])
    print("native end to end: metrics", got.tolist(), "restatement", np.array(want).tolist())
    _check(got, np.array(want))
    # the G1 image on disk is the rescaled window of the oracle's gen_rgb
    frame, win = nr.load_pad_u8(data["test"][2])
    ref = nr.infer_hw(g, gb, frame[None], F32, cyclic=False)["gen_rgb"].numpy()[0]
    b, y = nr.export_hw(ref, win, win[2], win[3], "rescale")
    with Image.open(tmp_path / "results_native" / "images" / "img2_G1.png") as im:
        d = np.abs(np.asarray(im).astype(np.int64) - b.astype(np.int64))
    # the forward's 1e-4 bound is 0.0255 of a byte step (less after the division by the range): only bytes that close to a
    # rounding tie may differ, about 5 % of evenly spread values at the very most
    assert d.max() <= 1 and (d != 0).mean() < 0.06
    # ... and so are the G1 Y plane and the cyclic images (img0: the padded 37 x 53 photo), held to the same bound
    frame, win = nr.load_pad_u8(data["test"][0])
    ref = nr.infer_hw(g, gb, frame[None], F32, cyclic=True)
    for tag, plane in (("G1_Y", ref["gen_Y"]), ("cyc0", ref["cyc_rgb"][0]), ("cycED", ref["cyc_rgb"][4])):
        b, y = nr.export_hw(plane.numpy()[0], win, win[2], win[3], "rescale")
        with Image.open(tmp_path / "results_native" / "images" / f"img0_{tag}.png") as im:
            a = np.asarray(im)
        d = np.abs(a.reshape(b.shape).astype(np.int64) - b.astype(np.int64))
        print(f"img0_{tag}.png: {int((d != 0).sum())} of {d.size} bytes differ from the restatement, max {int(d.max())}")
        assert d.max() <= 1 and (d != 0).mean() < 0.06, tag
    # the arena holds one frame shape, and a second pass over the folder does not grow it
    torch.cuda.synchronize()
    n1 = m.arena.nbytes()
    r2 = ev.test(m, _args(tmp_path, eval_size="native", save_images="all"), print_fn=lambda *a: None)
    torch.cuda.synchronize()
    assert m.arena.nbytes() == n1
    for k in ev.METRIC_KEYS:
        assert r2[k] == r[k], k                       # bitwise: nothing of a frame leaks into the next
    for name in ("inf/in", "inf/rgb", "inf/cyc_in", "inf1/y", "specseg/inf/x16", "pre/yuv/inf", "metrics/ws"):
        keys = [k for k in m.arena.t if k[0] == name]
        assert len(keys) == 1, (name, keys)
    assert [k[1][1:3] for k in m.arena.t if k[0] == "inf/in"] == [(48, 96)]
    held = sum(t.numel() * t.element_size() for k, t in m.arena.t.items() if k[0].startswith(m._FRAME_BUFFERS))
    assert held <= ev.native_frame_bytes(48, 96, F32)          # the count from the layer tables covers what a frame holds
    # eval_size="model" afterwards is what a trainer that never ran the native mode returns
    after = ev.test(m, _args(tmp_path, eval_size="model"), print_fn=lambda *a: None)
    fresh = ev.test(_e2e_trainer(tmp_path, "fresh"), _args(tmp_path), print_fn=lambda *a: None)
    for k in ev.METRIC_KEYS:
        assert after[k] == fresh[k], k
    # G1 only: no cyclic pass is run, one file per image
    g1 = ev.test(m, _args(tmp_path, eval_size="native", save_images="g1", image_dir=str(tmp_path / "g1")), print_fn=lambda *a: None)
    assert len(g1["files"]) == 3 and m.cyc_genED_rgb is None
    for k in ev.METRIC_KEYS:
        assert g1[k] == r[k], k


# --------------------------------------------------------------------------------------------- 7. over-limit refusal
@pytest.mark.filterwarnings("ignore:no checkpoint")
def test_over_limit_image_is_refused_before_any_launch(tmp_path, monkeypatch):
    _folder(tmp_path)
    m = _e2e_trainer(tmp_path, "limit")
    m.G.prepare_weights()
    torch.cuda.synchronize()
    before, nbytes = ops.last_kernel(), m.arena.nbytes()
    # the first image (37 x 53 -> a 48 x 64 frame) is exactly at the limit: lowered through the constant, no large image needed
    monkeypatch.setattr(ev, "MAX_TENSOR_BYTES", ev.native_max_tensor_bytes(48, 64, F32))
    with pytest.raises(ValueError, match=r"img0\.png.*eval_size='model'"):
        ev.test(m, SimpleNamespace(test_dir=str(tmp_path / "test"), calc_metrics=False, eval_batch_size=1, eval_size="native"),
                print_fn=lambda *a: None)
    assert ops.last_kernel() == before and m.arena.nbytes() == nbytes
    # one byte more and the image runs
    monkeypatch.setattr(ev, "MAX_TENSOR_BYTES", ev.native_max_tensor_bytes(48, 64, F32) + 1)
    (tmp_path / "test" / "img1.png").unlink()
    (tmp_path / "test" / "img2.png").unlink()
    assert ev.test(m, SimpleNamespace(test_dir=str(tmp_path / "test"), calc_metrics=False, eval_batch_size=1, eval_size="native"),
                   print_fn=lambda *a: None)["images"] == 1
