"""Native-resolution test mode, the parts that need no GPU: the ABI of the four new entry points, the padding rule, the host-side
refusals, the buffer-bytes function, and the float64 restatement (tests/native_ref.py) against the oracle."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import step_torch as st
from shmgan_amd import _lib

import native_ref as nr

P, I, Z, F = C.c_void_p, C.c_int, C.c_size_t, C.c_float
SIZES = [(37, 53), (33, 95), (64, 48)]


def test_entry_points_exist_with_the_stated_types():
    want = {
        "shm_load_pad_u8": (I, [P, I, I, I, P, I, I, I, I, F, P]),
        "shm_image_metrics_hw_workspace": (Z, [I, I, I]),
        "shm_image_metrics_hw": (I, [P, I, I, I, I, P, I, I, P, P, Z, I, P]),
        "shm_export_u8_hw": (I, [P, P, I, P, I, P, Z, P, Z, P]),
        "shm_mask_pool_pack_hw": (I, [P, P, I, I, I, I, I, I, P]),
    }
    hdr = _lib.header_functions()
    L = _lib.lib()
    for name, sig in want.items():
        assert name in hdr and _lib.SIGNATURES[name] == sig and hasattr(L, name), name
    assert L.shm_version() >= 202
    # argument checks answer before any launch: safe without a GPU
    assert L.shm_image_metrics_hw_workspace(1, 37, 53) > 0 and L.shm_image_metrics_hw_workspace(1, 10, 53) == 0
    p = 16                      # a non-null pointer nobody dereferences
    assert L.shm_image_metrics_hw(p, 48, 64, 5, 5, p, 10, 53, p, p, 1 << 20, 1, None) == -1 and b"< 11" in L.shm_last_error()
    assert L.shm_image_metrics_hw(p, 48, 64, 12, 5, p, 37, 53, p, p, 1 << 20, 1, None) == -1 and b"outside" in L.shm_last_error()
    assert L.shm_image_metrics_hw(p, 48, 64, 5, 5, p, 37, 53, p, p, 8, 1, None) == -3
    assert L.shm_load_pad_u8(p, 37, 53, 3, p, 48, 64, 12, 5, 1.0, None) == -1 and b"inside" in L.shm_last_error()
    assert L.shm_load_pad_u8(p, 4, 53, 3, p, 16, 64, 6, 5, 1.0, None) == -1 and b"pad wider" in L.shm_last_error()
    assert L.shm_mask_pool_pack_hw(p, p, 16, 1, 48, 30, 4, _lib.F32, None) == -1
    desc = (Z * 13)(48, 64, 3, 3, 5, 5, 44, 53, 37, 53, 2, 0, 0)
    src = (P * 1)(p)
    assert L.shm_export_u8_hw(src, desc, 1, None, 0, p, 1 << 20, p, 1 << 20, None) == -1 and b"window" in L.shm_last_error()


def test_square_entries_refuse_what_their_windowed_twins_refuse():
    """Every square entry point answers an argument set with the code its _hw twin gives the full window (0, 0, s, s) of an s x s frame,
    and names itself in the text.  No case reaches a launch: an argument set that passes every shape check is stopped by a missing
    workspace (SHM_E_WORKSPACE) or an unknown dtype (SHM_E_DTYPE).  The stated exceptions: shm_image_metrics puts no limit on s where the
    _hw form holds the frame's sides to 32768; shm_mask_pool_pack takes s == 0 (an empty output, SHM_OK) and does not look at the sign
    of batch, both of which shm_mask_pool_pack_hw refuses."""
    L = _lib.lib()
    p = 256                     # a non-null, aligned pointer nobody dereferences
    seen = set()

    def twins(sq, hw, a, b, want=None):
        ra, ea = getattr(L, sq)(*a), L.shm_last_error()
        rb, eb = getattr(L, hw)(*b), L.shm_last_error()
        assert (ra, rb) == (want or (ra, ra)) and ra != 0, (sq, a, ra, rb, ea, eb)
        assert ea.startswith(sq.encode() + b":") and eb.startswith(hw.encode() + b":"), (ea, eb)
        seen.add(ra)

    # ---- metrics: nulls one at a time, sides around the SSIM window, batch limits, no and short workspace; the workspace queries
    for s in (0, 10, 11, 32768):
        for batch in (0, -1, 1, 65535, 65536):
            for pred, target, out, ws, nb in ((p, p, p, None, 0), (None, p, p, p, 0), (p, None, p, p, 0), (p, p, None, p, 0), (p, p, p, p, 8)):
                twins("shm_image_metrics", "shm_image_metrics_hw", (pred, target, out, ws, nb, batch, s, None),
                      (pred, s, s, 0, 0, target, s, s, out, ws, nb, batch, None))
            assert L.shm_image_metrics_workspace(batch, s) == L.shm_image_metrics_hw_workspace(batch, s, s)
            assert L.shm_image_losses_workspace(batch, min(s, 64)) == L.shm_image_losses_hw_workspace(batch, min(s, 64), min(s, 64))
    twins("shm_image_metrics", "shm_image_metrics_hw", (p, p, p, None, 0, 1, 32769, None), (p, 32769, 32769, 0, 0, p, 32769, 32769, p, None, 0, 1, None),
          want=(-3, -1))
    # ---- export: one job {s, c, ld, ho, wo, mode, k, off} and its windowed spelling
    K = _lib.CONSTANTS
    good = dict(s=16, c=3, ld=4, ho=16, wo=16, mode=K["SHM_EXPORT_CLIP"], k=0, off=0)
    bad_jobs = [dict(c=c) for c in (0, 2, 4)] + [dict(s=s) for s in (0, 32769)] + [dict(ho=0), dict(wo=32769), dict(ld=2), dict(ld=65537),
                dict(off=2), dict(off=1 << 40), dict(mode=3), dict(mode=K["SHM_EXPORT_SCALE"]), dict(s=32768), dict(ho=32768, wo=32768)]
    calls = [dict(), dict(s=10, c=1, ld=1), dict(s=11)] + bad_jobs        # the first three pass every shape check
    for kw in calls:
        j = dict(good, **kw)
        dsq = (Z * 8)(j["s"], j["c"], j["ld"], j["ho"], j["wo"], j["mode"], j["k"], j["off"])
        dhw = (Z * 13)(j["s"], j["s"], j["c"], j["ld"], 0, 0, j["s"], j["s"], j["ho"], j["wo"], j["mode"], j["k"], j["off"])
        src = (P * 1)(p)
        for s_, d_, n, dst, ws, nb in ((src, True, 1, p, None, 0), (src, True, 1, p, p, 8), (src, True, 1, p, p + 2, 1 << 20), (None, True, 1, p, p, 0),
                                       (src, False, 1, p, p, 0), (src, True, 1, None, p, 0), (src, True, 1, p + 2, p, 0), (src, True, 0, p, p, 0),
                                       (src, True, K["SHM_EXPORT_MAX_JOBS"] + 1, p, p, 0), ((P * 1)(None), True, 1, p, p, 0)):
            twins("shm_export_u8", "shm_export_u8_hw", (s_, dsq if d_ else None, n, None, 0, dst, 1 << 20, ws, nb, None),
                  (s_, dhw if d_ else None, n, None, 0, dst, 1 << 20, ws, nb, None))
    # ---- mask pool pack: dtype 7 stops what passes the shape check
    for s in (10, 11, 32, 32769):
        for k in (0, 1, 2, 3, 32, -1):
            for ld in (0, 1):
                for mask, dst, batch in ((p, p, 1), (p, p, 65536), (None, p, 1), (p, None, 1)):
                    twins("shm_mask_pool_pack", "shm_mask_pool_pack_hw", (mask, dst, ld, batch, s, k, 7, None), (mask, dst, ld, batch, s, s, k, 7, None))
    twins("shm_mask_pool_pack", "shm_mask_pool_pack_hw", (p, p, 1, -1, 32, 2, 7, None), (p, p, 1, -1, 32, 32, 2, 7, None), want=(-2, -1))
    assert L.shm_mask_pool_pack(p, p, 1, 1, 0, 2, 7, None) == 0 and L.shm_mask_pool_pack_hw(p, p, 1, 1, 0, 0, 2, 7, None) == -1
    assert seen == {-1, -2, -3}


@pytest.mark.parametrize("h,w", SIZES + [(32, 32), (48, 80)])
def test_pad_geometry_and_reflect_fill(h, w):
    from shmgan_amd.data import pad_geometry
    hp, wp, top, left = pad_geometry(h, w)
    assert (hp, wp, top, left) == nr.pad_geometry(h, w)
    assert hp % 16 == 0 and wp % 16 == 0 and 0 <= hp - h < 16 and 0 <= wp - w < 16
    assert top == (hp - h) // 2 and left == (wp - w) // 2
    img = np.random.default_rng(h * 100 + w).integers(0, 256, (h, w, 3), dtype=np.uint8)
    frame, win = nr.pad_reflect(img)
    assert win == (top, left, h, w)
    want = np.pad(img, ((top, hp - h - top), (left, wp - w - left), (0, 0)), mode="reflect")
    assert np.array_equal(frame, want)
    assert np.array_equal(nr.crop(frame, win), img)
    if (h % 16, w % 16) == (0, 0):                       # an exact multiple is the identity
        assert (hp, wp, top, left) == (h, w, 0, 0) and np.array_equal(frame, img)


def test_geometry_of_the_issue_sizes():
    from shmgan_amd.data import pad_geometry
    assert pad_geometry(37, 53) == (48, 64, 5, 5)
    assert pad_geometry(33, 95) == (48, 96, 7, 0)
    assert pad_geometry(64, 48) == (64, 48, 0, 0)


def _png(path, h, w, seed=0):
    from PIL import Image
    Image.fromarray(np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)).save(path)


class _Stub:
    """What evaluate.test reads of a trainer before it touches the device."""
    image_size, filter_size, device, compute_dtype, attention = 32, 16, "cpu", torch.float32, "executed"
    args = SimpleNamespace()
    G = None


def test_host_side_refusals(tmp_path, monkeypatch):
    from shmgan_amd import evaluate as ev
    from shmgan_amd.data import NativeEvalDataset, pad_geometry
    for h, w in ((31, 64), (64, 16)):
        with pytest.raises(ValueError, match="at least 32"):
            pad_geometry(h, w)
    (tmp_path / "t").mkdir()
    (tmp_path / "d").mkdir()
    _png(tmp_path / "t" / "a.png", 37, 53)
    _png(tmp_path / "d" / "a.png", 37, 52)
    base = dict(test_dir=str(tmp_path / "t"), diffuse_dir=str(tmp_path / "d"), calc_metrics=True)
    with pytest.raises(ValueError, match="eval_batch_size must be 1"):
        ev.test(_Stub(), SimpleNamespace(eval_size="native", eval_batch_size=2, **base))
    with pytest.raises(ValueError, match="eval_size"):
        ev.test(_Stub(), SimpleNamespace(eval_size="photo", eval_batch_size=1, **base))
    # a diffuse partner of another size: raised by the loader after the decode, before any upload; both files are named
    ds = NativeEvalDataset(base["test_dir"], base["diffuse_dir"], device="cpu")
    with pytest.raises(ValueError) as e:
        ds.batch(0)
    assert "a.png" in str(e.value) and str(tmp_path / "t") in str(e.value) and str(tmp_path / "d") in str(e.value)
    # an over-limit image: the derived limit, lowered through the constant; then the memory limit
    assert ev.check_native_limits("x.png", 37, 53, 16) == ev.native_frame_bytes(48, 64, 16)
    monkeypatch.setattr(ev, "MAX_TENSOR_BYTES", ev.native_max_tensor_bytes(48, 64, 16))
    with pytest.raises(ValueError, match=r"x\.png.*eval_size='model'"):
        ev.check_native_limits("x.png", 37, 53, 16)
    ev.check_native_limits("x.png", 32, 53, 16)                       # one block row less passes
    monkeypatch.undo()
    need = ev.native_frame_bytes(48, 64, 16)
    with pytest.raises(ValueError, match=r"x\.png.*eval_size='model'"):
        ev.check_native_limits("x.png", 37, 53, 16, free_bytes=need)       # headroom: need > 0.9 * free
    ev.check_native_limits("x.png", 37, 53, 16, free_bytes=2 * need)
    with pytest.raises(ValueError, match="side"):
        ev.check_native_limits("x.png", 32, 40000, 16)
    # the loader calls the check after the decode and before it uploads
    _png(tmp_path / "d" / "a.png", 37, 53)
    seen = []

    def refuse(path, h, w):
        seen.append((path, h, w))
        raise ValueError("refused")
    with pytest.raises(ValueError, match="refused"):
        NativeEvalDataset(base["test_dir"], base["diffuse_dir"], device="cpu", check=refuse).batch(0)
    assert seen == [(str(tmp_path / "t" / "a.png"), 37, 53)]


def test_the_limit_constant_is_the_launchers():
    """MAX_TENSOR_BYTES is the operand limit of the convolution launcher (csrc/conv_igemm.hip: 32-bit byte offsets)."""
    from pathlib import Path
    from shmgan_amd import evaluate as ev
    src = (Path(_lib.__file__).resolve().parent / "csrc" / "conv_igemm.hip").read_text()
    assert "const size_t lim = 0xfffffff0ull;" in src and "xb < lim && x2b < lim && wb < lim" in src
    assert ev.MAX_TENSOR_BYTES == 0xfffffff0
    # float32, filter_size 64: 256 bytes per pixel -> just under 4096 x 4096 pixels
    assert ev.native_max_tensor_bytes(4096, 4096, 64) == 1 << 32 and ev.native_max_tensor_bytes(4096, 4080, 64) < ev.MAX_TENSOR_BYTES
    assert ev.native_max_tensor_bytes(32, 32, 16) == 32 * 32 * 64              # the 64-byte-per-pixel inputs are the widest at F = 16
    assert ev.native_max_tensor_bytes(32, 32, 64, torch.bfloat16) == 32 * 32 * 128


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("cyclic,attention", [(True, False), (False, False), (True, True)])
def test_frame_bytes_are_monotone_and_linear_in_pixels(dtype, cyclic, attention):
    from shmgan_amd.evaluate import native_frame_bytes as nb
    F = 32
    one = nb(32, 32, F, dtype, cyclic, attention)
    assert one > 0
    for hp, wp in ((32, 48), (48, 32), (80, 32), (1024, 1536)):
        assert nb(hp, wp, F, dtype, cyclic, attention) * (32 * 32) == one * (hp * wp)          # linear, exactly
        assert nb(hp + 16, wp, F, dtype, cyclic, attention) > nb(hp, wp, F, dtype, cyclic, attention) < nb(hp, wp + 16, F, dtype, cyclic, attention)
    assert nb(32, 32, F, dtype, True, attention) > nb(32, 32, F, dtype, False, attention)
    assert nb(32, 32, F, dtype, cyclic, True) > nb(32, 32, F, dtype, cyclic, False)
    assert nb(32, 32, 2 * F, dtype, cyclic, attention) > one
    with pytest.raises(ValueError):
        nb(40, 32, F)


def test_frame_bytes_count_the_arena_of_a_forward():
    """The count written out by hand for one frame, buffer group by buffer group (generator, SpecSeg, inputs and outputs): a
    second statement of the formula, not a measurement.  The tie to what a forward really allocates is the GPU end-to-end test,
    which holds the arena's frame buffers to this count."""
    from shmgan_amd import evaluate as ev
    from shmgan_amd.model import generator_layers
    from shmgan_amd.specseg import WIDTHS
    hp, wp, F = 32, 48, 16
    px = hp * wp
    g = sum((hp >> l) * (wp >> l) * (F << l) * 4 * 4 + (hp >> (l + 1)) * (wp >> (l + 1)) * (F << l) * 4 for l in range(4))
    g += (hp >> 4) * (wp >> 4) * 8 * F * 4 * 4
    g += sum((hp >> l) * (wp >> l) * (F << l) * 4 * 5 for l in range(4)) - px * F * 4 + px * 4
    s = px * 64 + sum((hp >> l) * (wp >> l) * w * 12 + ((hp >> (l + 1)) * (wp >> (l + 1)) * w * 4 if l < 4 else 0) for l, w in enumerate(WIDTHS))
    s += sum((hp >> l) * (wp >> l) * WIDTHS[l] * 12 for l in range(4)) + px * 4
    io = px * (12 + 12 + 12 + 8 + 64 + 12) + px * 20
    assert generator_layers(F)[21][4] == F
    assert ev.native_frame_bytes(hp, wp, F, cyclic=False) == g + s + io
    assert ev.native_frame_bytes(hp, wp, F, cyclic=True) == g + s + io + px * (4 + 4 + 5 * 64 + 5 * 12)


def test_restatement_equals_the_oracle_on_a_square_input():
    """Ties tests/native_ref.infer_hw to oracle.step_torch.infer.  Both are test-side code, so this one test does not depend on the
    product: it holds before the native mode exists as well."""
    F_, S = 16, 32
    g, _, gb, _ = st.init_params(F_, S)
    rgb = np.random.default_rng(5).uniform(0, 1, (2, S, S, 3))
    ref = st.infer(g, gb, rgb, F_)
    got = nr.infer_hw(g, gb, rgb, F_)
    assert float((got["gen_rgb"] - ref["gen_rgb"]).abs().max()) <= 1e-12
    assert float((got["gen_Y"] - ref["gen_Y"]).abs().max()) <= 1e-12
    for a, b in zip(got["cyc_rgb"], ref["cyc_rgb"]):
        assert float((a - b).abs().max()) <= 1e-12
    assert float((got["scale"] - ref["scale"]).abs().max()) <= 1e-12
