"""Training on rectangular frames (image_hw = (H, W)) on the device: shm_image_losses_hw alone against the float64 image oracle,
the whole step against tests/rect_step_ref.train_step_hw, bf16 and live attention, the square frame through both spellings, the
loader, and train() / checkpoint / validation / test mode end to end."""
import argparse
import ctypes as C
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import rect_step_ref as R
from loss_edge_ref import image_oracle
from oracle import data_np as dn
from oracle import specseg_torch as sp
from oracle import step_torch as st
from util import cosine, dev, host, rel_l2, t64

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------- 1. the stand-alone kernel
def _image_call(ops, inp, o, flags, sf, B, h, w, entry="hw", ws=None):
    fmask = sum(1 << k for k in range(5) if flags[k])
    od = [dev(x) for x in inp.orig]
    dd = [dev(d.numpy()) for d in inp.ds]
    loss = torch.empty(32, dtype=torch.float64, device="cuda")
    dg = torch.empty((B, h, w, 1), device="cuda")
    dc = torch.empty((5 * B, h, w, 1), device="cuda")
    if ws is None:
        ws = torch.empty(ops.image_losses_hw_workspace(B, h, w) // 4 + 1, device="cuda")
    optr = (C.c_void_p * 5)(*[t.data_ptr() for t in od])
    dptr = (C.c_void_p * 5)(*[t.data_ptr() for t in dd])
    args = (dev(o.gen_rgb.numpy()), dev(torch.cat(o.crgb, 0).numpy()), dev(o.cyc_y.numpy()), dev(inp.cbcr.numpy()), optr, dptr, fmask, sf,
            loss, dg, dc, ws, B)
    if entry == "hw":
        ops.image_losses_hw(*args, h, w)
    else:
        ops.image_losses(*args, h)
    torch.cuda.synchronize()
    return host(loss), host(dg), host(dc)


@pytest.mark.parametrize("flags", R.IMAGE_FLAGS)
@pytest.mark.parametrize("B,h,w", R.IMAGE_SHAPES)
def test_image_losses_hw(B, h, w, flags):
    """ops.image_losses_hw against loss_edge_ref.image_oracle with the construction and the tolerances of
    tests/test_step_gpu.py::test_image_losses: one output row, one output column, one tile down and four across and its transpose,
    partial tiles on both axes."""
    from shmgan_amd import ops
    sf = 3.0e-3
    inp = R.image_inputs_hw(B, h, w, seed=21)
    o = image_oracle(inp, flags, sf=sf)
    L, dg, dc = _image_call(ops, inp, o, flags, sf, B, h, w)
    l1 = lambda a, b: (a - b).abs().mean(dim=(1, 2, 3))
    assert abs(L[0] - float(l1(o.gen_rgb, t64(inp.orig[4])).sum())) < 1e-5 * B
    for k in range(5):
        assert abs(L[1 + k] - float(l1(o.crgb[k], t64(inp.orig[k])).sum())) < 1e-5 * B
        assert abs(L[6 + k] - float(o.ssims[k].sum())) < 2e-5 * B, (k, L[6 + k], float(o.ssims[k].sum()))
        assert abs(L[11 + k] - float(o.sl[k].sum())) < 2e-5 * B
    assert abs(L[16] - float(o.content.sum())) < 1e-5 * B * max(1.0, float(o.content.max()))
    assert abs(L[17] - float(o.style.sum())) < 1e-5 * max(1.0, float(o.style.sum()))
    assert rel_l2(dg, o.rg.numpy()) < 1e-4
    assert rel_l2(dc, o.rc.numpy()) < 1e-4, cosine(dc, o.rc.numpy())


def test_image_losses_hw_refusals():
    """A side of 10 (either one) and a workspace one byte short are refused on the host, before any launch."""
    from shmgan_amd import ops
    from shmgan_amd._lib import ShmError
    B, h, w = 1, 11, 43
    x = torch.zeros((5 * B * h * w * 3,), device="cuda")
    ptr = (C.c_void_p * 5)(*[x.data_ptr()] * 5)
    loss = torch.full((32,), 7.0, dtype=torch.float64, device="cuda")
    total = ops.image_losses_hw_workspace(B, h, w)
    assert total > 0 and ops.image_losses_hw_workspace(B, 10, w) == 0 and ops.image_losses_hw_workspace(B, h, 10) == 0
    assert ops.image_losses_hw_workspace(2, 32, 32) == ops.image_losses_workspace(2, 32)
    ws = torch.zeros((total,), dtype=torch.uint8, device="cuda")
    for hh, ww in ((10, w), (h, 10)):
        with pytest.raises(ShmError, match="< 11"):
            ops.image_losses_hw(x, x, x, x, ptr, ptr, 0, 1.0, loss, x, x, ws, B, hh, ww)
    with pytest.raises(ShmError, match="workspace"):
        ops.image_losses_hw(x, x, x, x, ptr, ptr, 0, 1.0, loss, x, x, ws[:total - 1], B, h, w)
    torch.cuda.synchronize()
    assert (host(loss) == 7.0).all()          # nothing ran


def test_square_through_the_new_entry_is_the_old_entry():
    """h = w = 32 through image_losses_hw and through image_losses: one implementation, so the results agree to the bound of two runs
    of one call (tests/test_train_loop_gpu.py::test_step_is_reproducible_run_to_run, 1e-6: the loss sums are float64 atomics)."""
    from shmgan_amd import ops
    B, S, flags, sf = 2, 32, R.IMAGE_FLAGS[1], 3.0e-3
    inp = R.image_inputs_hw(B, S, S, seed=21)
    o = image_oracle(inp, flags, sf=sf)
    new = _image_call(ops, inp, o, flags, sf, B, S, S, "hw")
    old = _image_call(ops, inp, o, flags, sf, B, S, S, "square")
    assert np.all(np.abs(new[0] - old[0]) <= 1e-6 * np.maximum(1.0, np.abs(old[0])))
    assert rel_l2(new[1], old[1]) <= 1e-6 and rel_l2(new[2], old[2]) <= 1e-6


# ------------------------------------------------------------------------------------------------- 2. the whole step, fp32
def _mk(H, W, F, B, **kw):
    from shmgan_amd import ShmGANwithSSpecSeg
    m = ShmGANwithSSpecSeg(image_hw=(H, W), filter_size=F, batch_size=B, **kw).build()
    assert m.image_hw == (H, W) and (m.G.H, m.G.W, m.D.sh, m.D.sw) == (H, W, H // 32, W // 32)
    return m


def _check_init(m, params):
    g, d, _, _ = params
    for a, b in zip(m.G.get_weights(), g):         # the product's own init equals the reference's (same seeds, same order)
        assert np.array_equal(a, b)
    for a, b in zip(m.D.get_weights(), d):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("H,W,F,B,step", R.STEP_SHAPES)
def test_train_step_parity_hw(H, W, F, B, step):
    """tests/test_step_gpu.py::test_train_step_parity on rectangular frames, same assertions and tolerances, against train_step_hw
    with the device's LeakyReLU masks.  No gradient tensor is skipped: tests/test_rect_step_cpu.py shows that none vanishes."""
    m = _mk(H, W, F, B)
    g, d, gb, db = params = R.init_params_hw(F, H, W)
    _check_init(m, params)
    assert tuple(m.D.P.vars[6].shape) == ((H // 32) * (W // 32) * 16 * F, 5)
    inp = R.make_inputs_hw(B, H, W)
    dr = R.make_draws_hw(step, B, H, W, F)
    sf = R.style_factor_hw(H, W)
    assert m.style_factor == sf
    sw = sp.init_specseg(seed=44 + step)
    m.SpecSeg.set_weights(sw)
    m.train_step(*inp, draws=dr, style_factor=sf, apply=False)
    torch.cuda.synchronize()
    masks = {"g1": m.G.lrelu_masks("g1"), "cyc": m.G.lrelu_masks("cyc"), "d": m.D.lrelu_masks()}
    ref = R.train_step_hw(g, d, gb, db, inp, dr, sf, F, masks=masks)
    free = R.train_step_hw(g, d, gb, db, inp, dr, sf, F, need_grads=False, specseg=sw)
    assert np.abs(host(m.specular_candidate) - free["outs"]["specular_candidate"].numpy()).max() < 1e-5
    got = m.losses()
    for k, v in free["losses"].items():
        assert abs(got[k] - v) <= 1e-4 * max(1.0, abs(v)), (k, got[k], v)
    for k, v in ref["losses"].items():
        assert abs(got[k] - v) <= 1e-4 * max(1.0, abs(v)), (k, got[k], v)
    assert np.abs(host(m.gen_Y) - ref["outs"]["gen_Y"].numpy()).max() < 1e-4
    assert np.abs(host(m.gen_rgb) - ref["outs"]["gen_rgb"].numpy()).max() < 1e-4
    for name, P, rg in (("D", m.D.P, ref["gD"]), ("G", m.G.P, ref["gG"])):
        for i, (got_g, r) in enumerate(zip(P.grads, rg)):
            r = r.numpy()
            assert np.linalg.norm(r) > 1e-12, (name, i)
            e = rel_l2(host(got_g), r)
            assert e < 1e-3 and cosine(host(got_g), r) > 0.9999, (name, i, e)
    # both Adam checks of test_train_step_parity
    gv, dvv = [t64(a).clone() for a in g], [t64(a).clone() for a in d]
    sg = st.AdamState([torch.zeros_like(a) for a in gv], [torch.zeros_like(a) for a in gv])
    sd = st.AdamState([torch.zeros_like(a) for a in dvv], [torch.zeros_like(a) for a in dvv])
    st.adam_apply(dvv, [t64(host(t)) for t in m.D.P.grads], sd, 2e-5, 0.5, 0.99)
    st.adam_apply(gv, [t64(host(t)) for t in m.G.P.grads], sg, 2e-5, 0.5, 0.99)
    gv2, dvv2 = [t64(a).clone() for a in g], [t64(a).clone() for a in d]
    sg2 = st.AdamState([torch.zeros_like(a) for a in gv2], [torch.zeros_like(a) for a in gv2])
    sd2 = st.AdamState([torch.zeros_like(a) for a in dvv2], [torch.zeros_like(a) for a in dvv2])
    st.adam_apply(dvv2, ref["gD"], sd2, 2e-5, 0.5, 0.99)
    st.adam_apply(gv2, ref["gG"], sg2, 2e-5, 0.5, 0.99)
    m.optimizer_D.apply(m.D.P)
    m.optimizer_G.apply(m.G.P)
    torch.cuda.synchronize()
    for got_w, r, r2 in zip(m.G.P.vars + m.D.P.vars, gv + dvv, gv2 + dvv2):
        assert np.abs(host(got_w) - r.numpy()).max() < 1e-8 + 2e-7 * float(r.abs().max())
        e = np.abs(host(got_w) - r2.numpy())
        assert e.max() <= 2.02 * 2e-5 and (e > 2e-6).mean() < 1e-2, (e.max(), (e > 2e-6).mean())


# ------------------------------------------------------------------------------------------------- 3. bf16, live attention
def test_bf16_step_tracks_fp32_hw():
    """(64, 96), F = 64, B = 1 in bfloat16 against the fp32 device step: named losses within 2e-2 (the bound of
    test_other_image_sizes_run_and_track_fp32), finite losses, non-zero gradients."""
    H, W, F, B = 64, 96, 64, 1
    inp, dr = R.make_inputs_hw(B, H, W), R.make_draws_hw(5, B, H, W, F)
    res = {}
    for dt in ("bfloat16", "float32"):
        m = _mk(H, W, F, B, compute_dtype=dt)
        m.train_step(*inp, draws=dr, apply=False)
        torch.cuda.synchronize()
        res[dt] = m.losses()
        assert all(np.isfinite(v) for k, v in res[dt].items() if k != "ssim")
        assert float(m.G.P.grad.abs().sum()) > 0 and float(m.D.P.grad.abs().sum()) > 0
        m.release()
    for k, v in res["float32"].items():
        if k != "ssim":
            assert abs(res["bfloat16"][k] - v) <= 2e-2 * max(1.0, abs(v)), (k, res["bfloat16"][k], v)


def _keras_g(g, ga):
    out = []
    for lvl in range(4):
        out += g[4 * lvl:4 * lvl + 4] + ga[4 * lvl:4 * lvl + 4]
    return out + g[16:]


def test_live_attention_step_matches_the_reference_hw():
    """attention="live" in fp32 at (64, 96), F = 16, B = 1 against train_step_hw(attention=): the assertions of
    tests/test_attention_gpu.py::test_live_attention_step_matches_oracle (the discriminator pools the mask to (H/16, W/16))."""
    H, W, F, B, step = 64, 96, 16, 1, 0
    m = _mk(H, W, F, B, attention="live")
    g, d, gb, db = R.init_params_hw(F, H, W)
    att = st.init_attention(F, bias_std=0.05)
    m.G.set_weights(_keras_g(g, att["G"]))
    m.D.set_weights(d[:4] + att["D"] + d[4:])
    inp, dr, sf = R.make_inputs_hw(B, H, W), R.make_draws_hw(step, B, H, W, F), R.style_factor_hw(H, W)
    sw = sp.init_specseg(seed=44 + step)
    m.SpecSeg.set_weights(sw)
    m.train_step(*inp, draws=dr, style_factor=sf, apply=False)
    torch.cuda.synchronize()
    assert tuple(m.D.attn.ctx["y2"].shape[1:3]) == (H // 16, W // 16)
    masks = {"g1": m.G.lrelu_masks("g1"), "cyc": m.G.lrelu_masks("cyc"), "d": m.D.lrelu_masks(),
             "ga": m.G.attention_masks(), "da": m.D.attention_masks()}
    ref = R.train_step_hw(g, d, gb, db, inp, dr, sf, F, masks=masks, specseg=sw, attention=att)
    plain = R.train_step_hw(g, d, gb, db, inp, dr, sf, F, need_grads=False, specseg=sw)
    got = m.losses()
    for k, v in ref["losses"].items():
        assert abs(got[k] - v) <= 1e-4 * max(1.0, abs(v)), (k, got[k], v)
    assert abs(ref["losses"]["total_Generator_loss"] - plain["losses"]["total_Generator_loss"]) > 1e-5      # the branch is live
    assert np.abs(host(m.gen_Y) - ref["outs"]["gen_Y"].numpy()).max() < 1e-4
    ng, nd = 46, 7
    sets = (("G", m.G.P.grads[:ng], ref["gG"]), ("Ga", m.G.P.grads[ng:], ref["gGa"]),
            ("D", m.D.P.grads[:nd], ref["gD"]), ("Da", m.D.P.grads[nd:], ref["gDa"]))
    for name, got_l, ref_l in sets:
        assert len(got_l) == len(ref_l)
        for i, (gg, r) in enumerate(zip(got_l, ref_l)):
            r = r.numpy()
            if np.linalg.norm(r) < 1e-12:
                continue
            e = rel_l2(host(gg), r)
            assert e < 1e-3 and cosine(host(gg), r) > 0.9999, (name, i, e)


# ------------------------------------------------------------------------------------------------- 4. square, reproducibility
def _run(m, inp, dr):
    m.train_step(*inp, draws=dr, apply=False)
    torch.cuda.synchronize()
    return dict(m.losses()), host(m.G.P.grad).copy(), host(m.D.P.grad).copy(), host(m.gen_Y).copy()


def _same(a, b):
    (l0, g0, d0, y0), (l1, g1, d1, y1) = a, b
    for k, v in l0.items():
        if k != "ssim":
            assert abs(l1[k] - v) <= 1e-6 * max(1.0, abs(v)), (k, v, l1[k])
    assert rel_l2(y1, y0) <= 1e-6
    assert rel_l2(g1, g0) <= 1e-6 and rel_l2(d1, d0) <= 1e-6


def test_square_frame_by_either_spelling():
    """image_hw = (64, 64) and image_size = 64 are one step, to the run-to-run bound of the step (1e-6)."""
    from shmgan_amd import ShmGANwithSSpecSeg
    S, F, B = 64, 16, 2
    inp, dr = st.make_inputs(B, S), st.make_draws(4, B, S, F)
    a = _run(_mk(S, S, F, B), inp, dr)
    m = ShmGANwithSSpecSeg(image_size=S, filter_size=F, batch_size=B).build()
    assert m.image_hw == (S, S) and m.frame_arg() == S
    _same(a, _run(m, inp, dr))


def test_rectangular_step_is_reproducible():
    """Two identical steps at (96, 64) agree to the 1e-6 bound."""
    H, W, F, B = 96, 64, 16, 2
    m = _mk(H, W, F, B)
    inp, dr = R.make_inputs_hw(B, H, W), R.make_draws_hw(4, B, H, W, F)
    _same(_run(m, inp, dr), _run(m, inp, dr))


# ------------------------------------------------------------------------------------------------- 5. the loader
SRC_HW, N_IMG = (40, 50), 4


def _write_capture(root, n, seed):
    from PIL import Image
    from shmgan_amd.data import PSD_SUBDIRS
    rng = np.random.default_rng(seed)
    ref = {}
    for v, sub in enumerate(PSD_SUBDIRS):
        (root / sub).mkdir(parents=True)
        for i in range(n):
            ref[(v, i)] = rng.integers(0, 256, (*SRC_HW, 3)).astype(np.uint8)
            Image.fromarray(ref[(v, i)]).save(root / sub / f"img_{i:03d}.png")
    return ref


@pytest.mark.parametrize("cache", ["none", "device"])
def test_loader_yields_the_frame(tmp_path, cache):
    """PolarDataset at (32, 64) over 40 x 50 files, uncached and with cache="device", against the oracle's bilinear resize / 255,
    flipped as the loader flips, within the 2e-6 of the square loader test."""
    from shmgan_amd.data import PolarDataset
    H, W = 32, 64
    ref = _write_capture(tmp_path / "data", N_IMG, 3)
    ds = PolarDataset(str(tmp_path / "data"), (H, W), batch_size=2, rank=0, world=1, cache=cache)
    batches = [[host(t) for t in b] for b in ds]
    assert len(batches) == N_IMG // 2
    for j, batch in enumerate(batches):
        for v in range(5):
            assert batch[v].shape == (2, H, W, 3)
            for b in range(2):
                want = (dn.resize_bilinear(ref[(v, 2 * j + b)], H, W) * np.float32(1.0 / 255.0))[::-1]
                assert np.abs(batch[v][b] - want).max() < 2e-6, (j, v, b)


def test_loader_augments_onto_the_frame(tmp_path):
    """One augmented pass at (32, 64) against tests/augment_ref.augment_views(ho, wo) with the loader's own draws, held to the bound
    of tests/test_augment_gpu.py (the float32 restatement's own error through polar_ref.bound).  The crop keeps the source's aspect."""
    import augment_ref as ar
    import polar_ref as pr
    from shmgan_amd.data import Augment, PolarDataset
    H, W = 32, 64
    ref = _write_capture(tmp_path / "data", N_IMG, 4)
    ds = PolarDataset(str(tmp_path / "data"), (H, W), batch_size=2, rank=0, world=1, seed=5, augment=Augment(flip_lr=0.5, flip_ud=0.5, crop_min=0.4, views="keep"))
    batches = [[host(t) for t in b] for b in ds]
    for j, batch in enumerate(batches):
        for b in range(2):
            pos = 2 * j + b
            crop, fud, flr, _ = ar.draw(5, 0, pos, *SRC_HW, flip_lr=0.5, flip_ud=0.5, crop_min=0.4)
            assert abs(crop[2] / crop[3] - SRC_HW[0] / SRC_HW[1]) < 1e-6               # the source's aspect, not the frame's
            srcs = [ref[(v, pos)] for v in range(5)]
            kw = dict(crop=crop, flip_ud=not fud, flip_lr=flr)
            want = ar.augment_views(srcs, H, W, ar.DIR, dtype=np.float64, **kw)
            w32 = ar.augment_views(srcs, H, W, ar.DIR, dtype=np.float32, **kw)
            for v in range(5):
                e32 = float(np.abs(w32[v] - want[v]).max())
                err = float(np.abs(batch[v][b].astype(np.float64) - want[v]).max())
                assert err <= pr.bound(e32), (pos, v, err, e32)


# ------------------------------------------------------------------------------------------------- 6. train() end to end
def test_train_validate_checkpoint_and_test_mode(tmp_path):
    """train() at (64, 96), F = 16 on four tuples with a held-out fraction and val_region = "residual"; the checkpoint goes back into a
    trainer of the same frame bit for bit and is refused by a (96, 64) trainer (the Dense kernel D/var06 has the same shape there and
    another meaning); validation.jsonl holds finite metrics; model-size test mode scores and writes 64 x 96 images."""
    from PIL import Image
    from shmgan_amd import ShmGANwithSSpecSeg
    from shmgan_amd import evaluate as ev
    H, W, F = 64, 96, 16
    _write_capture(tmp_path / "data", 4, 6)
    base = dict(mode="train", image_hw=(H, W), batch_size=1, filter_size=F, num_epochs=2, g_lr=2e-5, d_lr=2e-5, beta1=0.5, beta2=0.99,
                data_dir=str(tmp_path / "data"), checkpoint_save_dir=str(tmp_path / "ckpt"), log_dir=str(tmp_path / "logs"),
                result_dir=str(tmp_path / "results"), log_step=1, checkpoint_save_step=1, val_fraction=0.25, val_region="residual")
    args = argparse.Namespace(**base)
    m = ShmGANwithSSpecSeg(args)
    n = m.train(args, print_fn=lambda *a: None)
    torch.cuda.synchronize()
    # three training tuples, batch 1: batches_per_epoch - 1 = 2 steps per epoch
    assert n == 4 and m.D.P.iterations == 4 and m.G.P.iterations == 4
    assert tuple(m.gen_rgb.shape) == (1, H, W, 3)
    text = (tmp_path / "logs" / "Discriminator_summary.txt").read_text()
    assert f"(None, {H // 32}, {W // 32}, 1)" in text and f"(None, {H}, {W}, 1)" in (tmp_path / "logs" / "Generator_summary.txt").read_text()
    lines = [json.loads(l) for l in (tmp_path / "logs" / "validation.jsonl").read_text().splitlines()]
    assert lines and all(l["n"] == 1 for l in lines)
    for l in lines:
        assert all(np.isfinite(l[k]) for k in ("mse", "psnr", "ssim", "de76", "de94"))
        assert l["n_in_images"] in (0, 1)
    latest = sorted((tmp_path / "ckpt").glob("ckpt-*.npz"))[-1]
    # the same frame: bit-equal weights
    again = ShmGANwithSSpecSeg(argparse.Namespace(**base)).build(seed=1)
    again.load_npz(str(latest))
    for P, Q in ((m.G.P, again.G.P), (m.D.P, again.D.P)):
        assert np.array_equal(host(P.flat).view(np.uint32), host(Q.flat).view(np.uint32))
    # the transposed frame: D/var06 has the same shape and does not fit
    other = ShmGANwithSSpecSeg(argparse.Namespace(**dict(base, image_hw=(W, H)))).build()
    assert tuple(other.D.P.vars[6].shape) == tuple(m.D.P.vars[6].shape)
    before = host(other.D.P.flat).copy()
    with pytest.raises(KeyError, match="D/var06"):
        other.load_npz(str(latest))
    assert np.array_equal(host(other.D.P.flat), before)
    # a square trainer whose Dense kernel differs in shape: the refusal that names both shapes
    with pytest.raises(KeyError, match="D/var06"):
        ShmGANwithSSpecSeg(argparse.Namespace(**dict(base, image_hw=None, image_size=64))).build().load_npz(str(latest))
    # model-size test mode
    test_dir, dif_dir = tmp_path / "test", tmp_path / "diffuse"
    test_dir.mkdir()
    dif_dir.mkdir()
    rng = np.random.default_rng(8)
    for i in range(2):
        for d in (test_dir, dif_dir):
            Image.fromarray(rng.integers(0, 256, (*SRC_HW, 3)).astype(np.uint8)).save(d / f"img{i:02d}.png")
    r = ev.test(again, SimpleNamespace(test_dir=str(test_dir), diffuse_dir=str(dif_dir), calc_metrics=True, eval_batch_size=2, eval_size="model",
                                       save_images="g1", image_out_size="model"), print_fn=lambda *a: None)
    assert r["images"] == 2 and all(np.isfinite(r[k]).all() and len(r[k]) == 2 for k in ev.METRIC_KEYS)
    assert len(r["files"]) == 2
    for f in r["files"]:
        with Image.open(f) as im:
            assert im.size == (W, H)
    assert sorted(os.listdir(tmp_path / "results" / "images")) == [ev.image_name(f"img{i:02d}", "G1") for i in range(2)]
