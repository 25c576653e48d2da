"""The mask network's augmenting pair loader, the parts that need no GPU: the restatement of shm_augment_pairs_u8
(tests/pairs_ref.py) against today's path restated in plain NumPy; the comparison the device tests use, shown to see four modelled
faults at the case table's shapes; MaskDataset.split's planning; the view-2 rule of the polar source; the ABI of the new entry
points and their refusals (nothing is launched)."""
import ctypes as C

import numpy as np
import pytest

import pairs_ref as pf

DYADIC = [((37, 53), (16, 16)), ((9, 7), (32, 32))]        # source / output is a float32 value: fused and unfused coordinates agree


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("src,out", pf.SHAPES)
def test_identity_restatement_is_resize_then_yuv_then_standardise(src, out):
    img, mask = pf.images(*src)
    x, y, scale = pf.pair(img, mask, *out, dtype=np.float64)
    want_x, want_y = pf.plain_numpy_path(img, mask, *out)
    # the fused coordinate of augment_ref.coords and the unfused one of polar_ref.taps differ by a float32 rounding of the weight
    # where source / output is not a float32 value; where it is, the two paths are the same numbers up to float64 rounding
    tol = 1e-12 if (src, out) in DYADIC else 5e-6
    assert x.shape == y.shape == (*out, 1)
    assert np.abs(x - want_x).max() <= tol * max(1.0, np.abs(want_x).max()) and np.abs(y - want_y).max() <= tol
    assert scale >= pf.FLOOR and 0.0 <= y.min() and y.max() <= 1.0


def test_constant_image_takes_the_floor():
    img, mask = pf.images(16, 16, kind="const")
    for dtype in (np.float64, np.float32):
        x, _, scale = pf.pair(img, mask, 8, 8, dtype=dtype)
        assert scale == 1.0 / 256.0 and np.isfinite(x).all() and abs(float(x.max()) - 2.0 / 255.0 * 256.0) < 1e-5


def test_mirrors_are_on_the_read_side():
    img, mask = pf.images(12, 20)
    x0, y0, s0 = pf.pair(img, mask, 12, 20)
    x1, y1, s1 = pf.pair(img, mask, 12, 20, flip_ud=True, flip_lr=True)
    assert np.array_equal(x1, x0[::-1, ::-1]) and np.array_equal(y1, y0[::-1, ::-1]) and s0 == s1
    assert np.array_equal(y0[..., 0] * 255.0, mask.astype(np.float64) * (np.float64(pf.BYTE) * 255.0))       # same size: the bytes


# ------------------------------------------------------------------------------------------------ modelled faults
def _faulty(fault, src, out, name, kind="random"):
    img, mask = pf.images(*src, kind=kind)
    crop, fud, flr = pf.variant(name, *src)
    x, y, _ = pf.pair(img, mask, *out, crop, fud, flr, np.float32, fault=fault)
    return pf.compare(x, y, img, mask, *out, crop, fud, flr, label=f"{fault} {src}->{out} {name}")


@pytest.mark.parametrize("name", pf.VARIANTS)
@pytest.mark.parametrize("src,out", pf.SHAPES)
def test_the_comparison_passes_the_float32_restatement(src, out, name):
    for kind in ("random", "const", "zeros", "ones"):
        ok, text = _faulty(None, src, out, name, kind)
        assert ok, text


@pytest.mark.parametrize("name", pf.VARIANTS)
@pytest.mark.parametrize("src,out", pf.SHAPES)
def test_the_comparison_sees_statistics_without_u_and_v(src, out, name):
    ok, text = _faulty("no_uv", src, out, name)
    print(text)
    assert not ok, text


@pytest.mark.parametrize("name", pf.VARIANTS)
@pytest.mark.parametrize("src,out", pf.SHAPES)
def test_the_comparison_sees_a_missing_floor_on_a_constant_image(src, out, name):
    ok, text = _faulty("no_floor", src, out, name, kind="const")
    print(text)
    assert not ok, text


@pytest.mark.parametrize("name", [v for v in pf.VARIANTS if "flip" in v or v == "both"])
@pytest.mark.parametrize("src,out", [s for s in pf.SHAPES if s[1] != (1, 1)])          # one output pixel is its own mirror image
def test_the_comparison_sees_a_mask_sampled_without_the_mirror(src, out, name):
    ok, text = _faulty("mask_unmirrored", src, out, name)
    print(text)
    assert not ok, text


@pytest.mark.parametrize("name", pf.VARIANTS)
@pytest.mark.parametrize("src,out", pf.SHAPES)
def test_the_comparison_sees_statistics_over_the_source(src, out, name):
    ok, text = _faulty("source_stats", src, out, name)
    print(text)
    assert not ok, text


# ------------------------------------------------------------------------------------------------ split
def test_split_is_disjoint_complete_and_a_function_of_names_fraction_and_seed(monkeypatch):
    import torch
    from shmgan_amd.data import split_names
    monkeypatch.setattr(torch, "empty", None)                 # the planning makes no torch call
    monkeypatch.setattr(torch, "from_numpy", None)
    names = [f"img_{i:03d}" for i in range(23)]
    train, val = split_names(names, 0.25, seed=3)
    assert len(val) == 6 and len(train) == 17 and not set(train) & set(val) and sorted(train + val) == names
    assert train == sorted(train) and val == sorted(val)
    assert (train, val) == split_names(list(reversed(names)), 0.25, seed=3)          # of the SORTED names
    assert (train, val) == split_names(names, 0.25, seed=3)
    assert val != split_names(names, 0.25, seed=4)[1]
    assert len(split_names(names, 0.5, seed=3)[1]) == 12
    for bad in (0.0, 1.0, -0.1, 1.5, 0.01, 0.99, float("nan"), None):
        with pytest.raises(ValueError, match="split"):
            split_names(names, bad)
    assert [len(s) for s in split_names(["a", "b"], 0.5)] == [1, 1]
    with pytest.raises(ValueError):
        split_names(["a"], 0.5)


def _pair_dirs(root, n, hw=(12, 10)):
    from PIL import Image
    rng = np.random.default_rng(5)
    for sub in ("img", "mask"):
        (root / sub).mkdir()
    for i in range(n):
        Image.fromarray(rng.integers(0, 256, (*hw, 3)).astype(np.uint8)).save(root / "img" / f"p{i:02d}.png")
        Image.fromarray(rng.integers(0, 256, hw).astype(np.uint8)).save(root / "mask" / f"p{i:02d}.png")
    return str(root / "img"), str(root / "mask")


def test_dataset_split_needs_no_gpu(tmp_path):
    from shmgan_amd.data import Augment, MaskDataset, split_names
    ds = MaskDataset(*_pair_dirs(tmp_path, 10), 8, batch_size=4, augment=Augment(flip_lr=0.5, crop_min=0.5), shuffle=True, seed=9, cache_bytes=1 << 20)
    train, val = ds.split(0.3, seed=2)
    assert (train.names, val.names) == split_names(ds.names, 0.3, 2) and len(val.names) == 3
    assert [f[0] for f in train.files] == [f for n, (f, _) in zip(ds.names, ds.files) if n in set(train.names)]
    assert train.augment == ds.augment and train.shuffle and train.seed == 9 and train.cache_bytes == 1 << 20 and train.active
    assert val.augment is None and not val.shuffle and not val.active and val.B == 4
    assert (len(train), len(val), len(ds)) == (2, 1, 3)
    assert len(train.positions(0, 0)) == 4 and len(train.positions(1, 0)) == 3                      # the last batch holds 7 mod 4
    assert sorted(train.positions(0, 5) + train.positions(1, 5)) == list(range(7))
    assert ds.cache_stats() == {"resident": 0, "bytes": 0, "chunks": 0, "hits": 0, "misses": 0, "refused": 0}
    for bad in (0.0, 1.0, 0.04):
        with pytest.raises(ValueError, match="split"):
            ds.split(bad)
    with pytest.raises(ValueError, match="Augment"):
        MaskDataset(str(tmp_path / "img"), str(tmp_path / "mask"), 8, augment="flip")
    with pytest.raises(ValueError, match="cache_bytes"):
        MaskDataset(str(tmp_path / "img"), str(tmp_path / "mask"), 8, shuffle=True, cache_bytes=-1)


# ------------------------------------------------------------------------------------------------ the view-2 rule
def test_view_2_rule():
    from shmgan_amd.polar import mirror_keeps_view, mirror_views
    assert mirror_keeps_view([0, 45, 90, 135]) and mirror_keeps_view([0, 60, 90, 150])
    assert mirror_views([0, 45, 90, 135]) == ("permute", [0, 3, 2, 1])
    # 0/60/90/150: 60 becomes 120, which is not in the set, so the four views are re-mixed; row 2 of that matrix is the least-squares
    # fit of view 2 and no unit row, although 90 degrees is mirror-invariant: the rule goes by the angle
    kind, mix = mirror_views([0, 60, 90, 150])
    assert kind == "mix" and np.allclose(mix[2], [-0.25, 0.25, 0.75, 0.25], atol=1e-6)
    assert mirror_keeps_view([0, 60, 90, 150], view=0) and not mirror_keeps_view([0, 60, 90, 150], view=1)
    assert not mirror_keeps_view([0, 30, 60, 120])                 # 60 degrees becomes 120: view 2 is view 3 of the mirrored scene
    assert not mirror_keeps_view([0, 45, 90, 135], view=1) and mirror_keeps_view([0, 45, 90, 135], view=0)
    assert not mirror_keeps_view([10, 50, 100, 140])               # no mirrored angle is in the set and row 2 of the mix is no unit row


def _capture(root, subdirs, n=2, hw=(10, 12)):
    from PIL import Image
    rng = np.random.default_rng(8)
    for sub in subdirs:
        (root / sub).mkdir(parents=True)
        for i in range(n):
            Image.fromarray(rng.integers(0, 256, (*hw, 3)).astype(np.uint8)).save(root / sub / f"c{i}.png")
    return str(root)


def test_from_polar_refuses_a_mirror_that_moves_view_2(tmp_path):
    from shmgan_amd.data import PSD_SUBDIRS, SHMGAN_SUBDIRS, Augment, MaskDataset
    flip = Augment(flip_lr=0.5)
    for k, subdirs in enumerate((PSD_SUBDIRS, SHMGAN_SUBDIRS)):
        ds = MaskDataset.from_polar(_capture(tmp_path / f"ok{k}", subdirs[:4]), 8, subdirs=subdirs, augment=flip)
        assert ds.active and ds.augment == flip
    odd = ("I0", "I30", "I60", "I120")
    root = _capture(tmp_path / "odd", odd)
    with pytest.raises(ValueError, match=r"view 2.*views=\"keep\""):
        MaskDataset.from_polar(root, 8, subdirs=odd, augment=flip)
    with pytest.raises(ValueError, match=r"view 2.*views=\"keep\""):
        MaskDataset.from_polar(root, 8, subdirs=PSD_SUBDIRS[:0] + odd, angles=[0, 30, 60, 120], augment=Augment(flip_ud=1.0))
    # the geometric flip, a crop alone and no augmentation are fine for any angles
    assert MaskDataset.from_polar(root, 8, subdirs=odd, augment=Augment(flip_lr=0.5, views="keep")).active
    assert MaskDataset.from_polar(root, 8, subdirs=odd, augment=Augment(crop_min=0.5), shuffle=True).active
    assert not MaskDataset.from_polar(root, 8, subdirs=odd).active


# ------------------------------------------------------------------------------------------------ ABI and refusals
def test_abi_of_the_pair_entry_points():
    from shmgan_amd import _lib, ops
    assert _lib.SIGNATURES["shm_augment_pairs_ws_doubles"] == (C.c_size_t, [C.c_int] * 3)
    assert _lib.SIGNATURES["shm_augment_pairs_u8"] == (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p,
                                                                 C.c_void_p, C.c_void_p])
    st = ops._pair_sample_struct()
    assert C.sizeof(st) == 48 and st.hin.offset == 16 and st.crop_y.offset == 24 and st.flip_lr.offset == 44
    # blocks per sample: a function of ho * wo alone, one per 256 pixels up to 256
    ws = ops.augment_pairs_ws_doubles
    assert [ws(1, 16, 16), ws(1, 17, 19), ws(1, 32, 32), ws(1, 1, 1), ws(9, 32, 32), ws(1, 256, 256), ws(1, 512, 512)] == [2, 4, 8, 2, 72, 512, 512]
    assert ws(1, 19, 17) == ws(1, 17, 19) and ws(3, 17, 19) == 3 * ws(1, 17, 19)
    assert [ws(0, 16, 16), ws(1, 0, 16), ws(1, 16, 32769), ws(-1, 16, 16)] == [0, 0, 0, 0]


def test_refusals_before_any_launch():
    """SHM_E_SHAPE (-1) for everything the header lists; the pointers are never dereferenced on the host and nothing is launched"""
    from shmgan_amd import _lib, ops
    L, st = _lib.lib(), ops._pair_sample_struct()
    nan = float("nan")

    def call(edit=None, n=3, ho=16, wo=16, x=0x1000, y=0x2000, ws=0x3000, stride=256, samples=True):
        arr = (st * 9)()
        for i in range(9):
            arr[i].image, arr[i].mask, arr[i].hin, arr[i].win = 0x10000, 0x20000, 16, 20
            arr[i].crop_y, arr[i].crop_x, arr[i].crop_h, arr[i].crop_w = 0.0, 0.0, 16.0, 20.0
        if edit:
            edit(arr)
        rc = L.shm_augment_pairs_u8(arr if samples else None, n, x, y, stride, ho, wo, ws, None, None)
        return rc, L.shm_last_error().decode()

    def field(i, **kw):
        def edit(arr):
            for k, v in kw.items():
                setattr(arr[i], k, v)
        return edit

    cases = [(dict(n=0), "n 0 < 1"), (dict(n=-2), "n -2 < 1"),
             (dict(samples=False), "null pointer"), (dict(x=None), "null pointer"), (dict(y=None), "null pointer"), (dict(ws=None), "null pointer"),
             (dict(ho=0), "sizes ho 0, wo 16 outside [1, 32768]"), (dict(wo=32769), "wo 32769 outside"),
             (dict(stride=255), "sample_stride 255 is less than a plane of 16 x 16"),
             (dict(edit=field(2, image=None)), "sample 2: null pointer (image)"), (dict(edit=field(1, mask=None)), "sample 1: null pointer (mask)"),
             (dict(edit=field(2, hin=0)), "sample 2: sizes hin 0, win 20 outside"), (dict(edit=field(0, win=32769)), "sample 0: sizes hin 16, win 32769"),
             (dict(edit=field(1, crop_h=0.0)), "sample 1: empty crop"), (dict(edit=field(1, crop_w=nan)), "sample 1: empty crop"),
             (dict(edit=field(2, crop_y=0.5)), "sample 2: the crop 16 x 20 at (0.5, 0) does not lie inside the 16 x 20 image"),
             (dict(edit=field(2, crop_x=-1.0, crop_w=4.0)), "sample 2: the crop"), (dict(edit=field(0, crop_x=nan)), "sample 0: the crop"),
             (dict(n=9, edit=field(8, crop_y=nan)), "sample 8: the crop")]
    for kw, msg in cases:
        rc, err = call(**kw)
        assert rc == -1 and msg in err and err.startswith("shm_augment_pairs_u8: "), (kw, rc, err)
