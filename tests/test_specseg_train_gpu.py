"""SpecSeg training on the device against the float64 reference of specseg_train_ref.py: every new kernel of csrc/specseg_train.hip on its
own, the gradients of the whole network, a 20-step trajectory, fit / predict / evaluate, the checkpoint round trip and MaskDataset.

Per-kernel bound (the rule of DESIGN.md section 6b): the larger of 1e-5 of the tensor's max-abs and 4x the error the float32 torch
restatement makes on the same inputs.  Whole-network bound per gradient tensor: 4x the rel-L2 error of the float32 reference run against
the float64 one on these exact inputs (device keep masks included), floor 1e-5; DESIGN.md section 6d records the measured values.  Every
check prints its figure before it asserts.
"""
import numpy as np
import pytest
import torch

import specseg_train_ref as R
from oracle.specseg_torch import init_specseg, specseg_spec
from util import dev, host, rel_l2

pytestmark = pytest.mark.gpu
NAN = float("nan")


def _ops():
    from shmgan_amd import ops
    return ops


def _t(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def _maxabs(a):
    a = np.asarray(a, np.float64)
    return float(np.abs(a).max()) if a.size else 0.0


def _check(what, got, ref64, ref32):
    """max-abs error of got against ref64, relative to ref64's max-abs, under max(1e-5, 4 x the float32 restatement's)"""
    ref64 = np.asarray(ref64, np.float64)
    scale = max(_maxabs(ref64), 1e-30)
    fig = _maxabs(np.asarray(got, np.float64) - ref64) / scale
    tol = max(1e-5, 4 * _maxabs(np.asarray(ref32, np.float64) - ref64) / scale)
    print(f"{what}: {fig:.3g} (bound {tol:.3g})")
    assert np.isfinite(np.asarray(got, np.float64)).all(), what
    assert fig <= tol, (what, fig, tol)


def _wide(a, ld):
    """a [rows, c] as a device tensor [rows, ld]; the gap holds NaN (a read of it shows in the result)"""
    t = torch.full((a.shape[0], ld), NAN, dtype=torch.float32)
    t[:, :a.shape[1]] = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    return t.cuda()


def _out(rows, ld, fill=7.0):
    return torch.full((rows, ld), fill, dtype=torch.float32, device="cuda")


def _gap_intact(t, c, fill=7.0):
    return bool((t[:, c:] == fill).all().item())


def _f64buf(n):
    return torch.zeros(n, dtype=torch.float64, device="cuda")


# ------------------------------------------------------------------------------------------------------ BatchNormalization
def _bn_ref(a, dy, gamma, beta, dtype):
    at = _t(a, dtype).requires_grad_(True)
    gt, bt = _t(gamma, dtype).requires_grad_(True), _t(beta, dtype).requires_grad_(True)
    out, mean, var = R.bn_train(at, gt, bt)
    out.backward(_t(dy, dtype))
    return [v.detach().double().numpy() for v in (out, mean, var, at.grad, gt.grad, bt.grad)]


def _bn_device(a, dy, gamma, beta, mm, mv, ld, calls=1):
    ops = _ops()
    npix, c = a.shape
    ad, dyd = _wide(a, ld), _wide(dy, ld)
    out, dx = _out(npix, ld), _out(npix, ld)
    save, ws = _f64buf(2 * c), _f64buf(ops.bn_train_ws_doubles(c))
    mmd, mvd = dev(mm), dev(mv)
    dg, db = torch.empty(c, device="cuda"), torch.empty(c, device="cuda")
    for _ in range(calls):
        ops.bn_train_fwd(ad, ld, dev(gamma), dev(beta), mmd, mvd, R.BN_MOMENTUM, 1e-3, out, ld, save, ws, npix, c)
    ops.bn_train_bwd(dyd, ld, ad, ld, dev(gamma), save, dx, ld, dg, db, ws, npix, c)
    torch.cuda.synchronize()
    return out, dx, save, mmd, mvd, dg, db


@pytest.mark.parametrize("npix,c,kind,wide", R.BN_CASES)
def test_bn_train_fwd_bwd(npix, c, kind, wide):
    a, dy, gamma, beta, mm, mv = R.bn_case(npix, c, kind)
    ld = c + 8 if wide else c
    out, dx, save, mmd, mvd, dg, db = _bn_device(a, dy, gamma, beta, mm, mv, ld)
    r64, r32 = _bn_ref(a, dy, gamma, beta, torch.float64), _bn_ref(a, dy, gamma, beta, torch.float32)
    tag = f"bn n{npix} c{c} {kind}"
    _check(f"{tag} out", host(out[:, :c]), r64[0], r32[0])
    _check(f"{tag} mean", host(save[:c]), r64[1], r32[1])
    inv = lambda r: 1.0 / np.sqrt(r[2] + 1e-3)
    _check(f"{tag} inv_std", host(save[c:]), inv(r64), inv(r32))
    _check(f"{tag} dx", host(dx[:, :c]), r64[3], r32[3])
    _check(f"{tag} dgamma", host(dg), r64[4], r32[4])
    _check(f"{tag} dbeta", host(db), r64[5], r32[5])
    assert _gap_intact(out, c) and _gap_intact(dx, c)
    # the constant channel: variance exactly 0, output exactly beta
    assert float(save[c + 1]) == pytest.approx(1.0 / np.sqrt(1e-3), rel=1e-6) and np.array_equal(host(out[:, 1]), np.full(npix, beta[1], np.float64))
    if npix == 1:
        assert not dx[:, :c].any() and not dg.any()          # one value: the output is beta whatever the input
    # moving statistics after one call
    m64 = R.bn_moving(mm.astype(np.float64), mv.astype(np.float64), r64[1], r64[2], npix)
    m32 = R.bn_moving(mm, mv, r32[1].astype(np.float32), r32[2].astype(np.float32), np.float32(npix), np.float32(R.BN_MOMENTUM))
    _check(f"{tag} moving_mean", host(mmd), m64[0], m32[0])
    _check(f"{tag} moving_var", host(mvd), m64[1], m32[1])


@pytest.mark.parametrize("npix,c", [(3, 16), (1024, 256)])
def test_bn_moving_statistics_after_two_calls_and_reproducible(npix, c):
    a, dy, gamma, beta, mm, mv = R.bn_case(npix, c, "normal")
    runs = [_bn_device(a, dy, gamma, beta, mm, mv, c, calls=2) for _ in range(2)]
    for x, y in zip(*runs):
        assert torch.equal(x, y)                               # bitwise, every output
    r64 = _bn_ref(a, dy, gamma, beta, torch.float64)
    m1 = R.bn_moving(mm.astype(np.float64), mv.astype(np.float64), r64[1], r64[2], npix)
    m2 = R.bn_moving(m1[0], m1[1], r64[1], r64[2], npix)
    f1 = R.bn_moving(mm, mv, r64[1].astype(np.float32), r64[2].astype(np.float32), np.float32(npix), np.float32(R.BN_MOMENTUM))
    f2 = R.bn_moving(f1[0], f1[1], r64[1].astype(np.float32), r64[2].astype(np.float32), np.float32(npix), np.float32(R.BN_MOMENTUM))
    _check(f"bn n{npix} c{c} moving_mean x2", host(runs[0][3]), m2[0], f2[0])
    _check(f"bn n{npix} c{c} moving_var x2", host(runs[0][4]), m2[1], f2[1])


# ------------------------------------------------------------------------------------------------------------- pool backward
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("ties", R.POOL_TIES)
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("hw", R.POOL_SIZES)
def test_maxpool2_bwd(hw, batch, ties, accumulate):
    ops = _ops()
    h, w = hw
    c, ld = 16, 24
    x, dy = R.pool_case(batch, h, w, ties)
    rng = np.random.default_rng(1)
    skip = rng.normal(0, 1, (batch * h * w, c)).astype(np.float32)
    xd, dyd = _wide(x.reshape(-1, c), ld), _wide(dy.reshape(-1, c), ld)
    dx = _out(batch * h * w, ld)
    dx[:, :c] = dev(skip)
    ops.maxpool2_bwd(xd, ld, dyd, ld, dx, ld, batch, h, w, c, accumulate)
    ref = R.pool_bwd_first_max(x.astype(np.float64), dy.astype(np.float64)).reshape(-1, c)
    ref32 = ref.astype(np.float32)
    if accumulate:
        ref, ref32 = ref + skip, ref32 + skip
    _check(f"pool bwd {h}x{w} b{batch} {ties} acc{int(accumulate)}", host(dx[:, :c]), ref, ref32)
    assert _gap_intact(dx, c)


# ------------------------------------------------------------------------------------------------- Conv2DTranspose backward
def _convt_ref(x, k, dy, dtype):
    xt, kt = _t(x, dtype).requires_grad_(True), _t(k, dtype).requires_grad_(True)
    bt = torch.zeros(k.shape[2], dtype=dtype, requires_grad=True)
    (R.convt_fwd(xt, kt) + bt).backward(_t(dy, dtype))
    return [v.grad.double().numpy() for v in (xt, kt, bt)]


@pytest.mark.parametrize("batch,hi,wi,cout", R.CONVT_CASES)
def test_conv2d_transpose2x2_backward(batch, hi, wi, cout):
    ops = _ops()
    cin = 2 * cout
    rng = np.random.default_rng([batch, hi, wi, cout])
    x = rng.normal(0, 1, (batch, hi, wi, cin)).astype(np.float32)
    k = rng.normal(0, 0.1, (2, 2, cout, cin)).astype(np.float32)
    dy = rng.normal(0, 1, (batch, 2 * hi, 2 * wi, cout)).astype(np.float32)
    ldx, lddy, lddx = cin + 4, cout + 8, cin + 12
    M = batch * hi * wi
    xd, dyd = _wide(x.reshape(M, cin), ldx), _wide(dy.reshape(4 * M, cout), lddy)
    dx = _out(M, lddx)
    ops.conv2d_transpose2x2_dgrad(dyd, lddy, dev(k), dx, lddx, batch, hi, wi, cin, cout)
    ws = torch.empty(ops.conv2d_transpose2x2_wgrad_workspace(batch, hi, wi, cin, cout) // 4 + 1, device="cuda")
    got = []
    for _ in range(2):
        dw, dbias = torch.full((2, 2, cout, cin), 7.0, device="cuda"), torch.full((cout,), 7.0, device="cuda")
        ops.conv2d_transpose2x2_wgrad(xd, ldx, dyd, lddy, dw, dbias, ws, batch, hi, wi, cin, cout)
        got.append((dw, dbias))
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])          # fixed-order split sums: bitwise
    r64, r32 = _convt_ref(x, k, dy, torch.float64), _convt_ref(x, k, dy, torch.float32)
    tag = f"convT2 b{batch} {hi}x{wi} co{cout}"
    _check(f"{tag} dx", host(dx[:, :cin]).reshape(x.shape), r64[0], r32[0])
    _check(f"{tag} dw", host(got[0][0]), r64[1], r32[1])
    _check(f"{tag} dbias", host(got[0][1]), r64[2], r32[2])
    assert _gap_intact(dx, cin)


# ---------------------------------------------------------------------------------------------------------------- head, loss
def _head_ref(x, w, b, dz, dtype):
    xt, wt, bt = _t(x, dtype).requires_grad_(True), _t(w, dtype).requires_grad_(True), _t(b, dtype).requires_grad_(True)
    z = xt @ wt + bt
    z.backward(_t(dz, dtype))
    return [v.double().numpy() for v in (z.detach(), xt.grad, wt.grad, bt.grad)]


@pytest.mark.parametrize("npix", [1, 255, 4097])
def test_head_logit_fwd_bwd(npix):
    ops = _ops()
    c, ld = 16, 20
    rng = np.random.default_rng(npix)
    x, w, b, dz = [rng.normal(0, 1, s).astype(np.float32) for s in ((npix, c), (c,), (1,), (npix,))]
    xd = _wide(x, ld)
    z, dx = torch.empty(npix, device="cuda"), _out(npix, ld)
    ops.head_logit_fwd(xd, ld, dev(w), dev(b), z, npix, c)
    ws = _f64buf(ops.bn_train_ws_doubles(c))
    runs = []
    for _ in range(2):
        dw, db = torch.empty(c, device="cuda"), torch.empty(1, device="cuda")
        ops.head_logit_bwd(xd, ld, dev(w), dev(dz), dx, ld, dw, db, ws, npix, c)
        runs.append((dw, db))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    r64, r32 = _head_ref(x, w, b, dz, torch.float64), _head_ref(x, w, b, dz, torch.float32)
    for name, got, i in (("z", z, 0), ("dx", dx[:, :c], 1), ("dw", runs[0][0], 2), ("db", runs[0][1], 3)):
        _check(f"head n{npix} {name}", host(got), r64[i], r32[i])
    assert _gap_intact(dx, c)


def _loss_ref(z, g, dtype):
    zt = _t(z, dtype).requires_grad_(True)
    L = R.seg_loss(zt, _t(g, dtype))
    L["loss"].backward()
    return {k: float(v.detach()) for k, v in L.items()}, zt.grad.double().numpy()


@pytest.mark.parametrize("logits", R.LOSS_LOGITS)
@pytest.mark.parametrize("mask", R.LOSS_MASKS)
@pytest.mark.parametrize("npix", R.LOSS_NPIX)
def test_seg_loss(npix, mask, logits):
    ops = _ops()
    z, g = R.loss_case(npix, mask, logits)
    ws = _f64buf(ops.SEG_LOSS_WS_DOUBLES)
    runs = []
    for _ in range(2):
        out, dz = torch.empty(8, dtype=torch.float64, device="cuda"), torch.full((npix,), 7.0, device="cuda")
        ops.seg_loss(dev(z), dev(g), dz, out, ws, npix)
        runs.append((out, dz))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    (L64, g64), (L32, g32) = _loss_ref(z, g, torch.float64), _loss_ref(z, g, torch.float32)
    out = host(runs[0][0])
    tag = f"loss n{npix} {mask} {logits}"
    for j, k in enumerate(ops.SEG_LOSS_NAMES[:5]):
        _check(f"{tag} {k}", [out[j]], [L64[k]], [L32[k]])
    _check(f"{tag} dz", host(runs[0][1]), g64, g32)
    if mask != "soft":
        on = z > 0
        assert [out[5], out[6], out[7]] == [float((g * on).sum()), float(((1 - g) * on).sum()), float((g * ~on).sum())]      # exact integers
    else:
        for j, k in ((5, "tp"), (6, "fp"), (7, "fn")):
            _check(f"{tag} {k}", [out[j]], [L64[k]], [L32[k]])
    # evaluation form: no gradient written, the same values
    out2 = torch.empty(8, dtype=torch.float64, device="cuda")
    ops.seg_loss(dev(z), dev(g), None, out2, ws, npix)
    assert torch.equal(out2, runs[0][0])


# ---------------------------------------------------------------------------------------------------------------------- Adam
def test_adam_with_clip_one_is_adam_clip_bitwise_and_clip_zero_is_plain_adam():
    ops = _ops()
    n = 100003
    rng = np.random.default_rng(3)
    w, m, v = rng.normal(0, 1, n), rng.normal(0, 0.1, n), rng.uniform(0, 0.1, n)
    g = rng.normal(0, 2, n)                                  # a good part beyond the clip bound
    a, b1, b2, eps, gs = 1.3e-3, 0.5, 0.99, 1e-7, 0.5
    A, B, Cz = [[dev(t) for t in (w, m, v)] for _ in range(3)]
    gd = dev(g)
    ops.adam_clip(*A, gd, n, a, b1, b2, eps, gs)
    ops.adam(*B, gd, n, a, b1, b2, eps, gs, 1.0)
    for x, y in zip(A, B):
        assert torch.equal(x, y)
    ops.adam(*Cz, gd, n, a, b1, b2, eps, gs, 0.0)
    f32 = lambda t: np.asarray(t, np.float32)
    g32 = f32(g) * np.float32(gs)
    r64 = R.adam_step(f32(w).astype(np.float64), f32(m).astype(np.float64), f32(v).astype(np.float64), g32.astype(np.float64), np.float32(a).astype(np.float64),
                      float(np.float32(b1)), float(np.float32(b2)), float(np.float32(eps)))
    r32 = R.adam_step(f32(w), f32(m), f32(v), g32, np.float32(a), np.float32(b1), np.float32(b2), np.float32(eps))
    for name, got, x, y in zip(("w", "m", "v"), Cz, r64, r32):
        _check(f"adam clip 0 {name}", host(got), x, y)
    assert float(Cz[1].abs().max()) > float(B[1].abs().max())          # the unclipped moments did see the large gradients


# ------------------------------------------------------------------------------------------------------------ whole network
NET_CASES = {"S16_B1": (1, 16, 16), "S16_B3": (3, 16, 16), "16x48_B2": (2, 16, 48), "S32_B2": (2, 32, 32)}
STRUCTURAL_ZEROS = {"S16_B1": {32, 33, 34, 35, 36}}          # test_specseg_train_cpu.py: BatchNormalization over one value


def _net(S=32):
    from shmgan_amd.model import Arena
    from shmgan_amd.specseg import SpecSeg
    d = torch.device("cuda")
    net = SpecSeg(S, d, Arena(d))
    net.set_weights(init_specseg(trained_like=True))
    return net


@pytest.mark.parametrize("name", NET_CASES)
def test_network_gradients(name):
    ops = _ops()
    n, H, W = NET_CASES[name]
    x, mask = R.discs(n, max(H, W), seed=5)
    x, mask = np.ascontiguousarray(x[:, :H, :W]), np.ascontiguousarray(mask[:, :H, :W])
    net = _net(16)
    weights = net.get_weights()
    keep = net.keep_masks(n, H, W, seed=7, counter=3)
    keep_h = [k.cpu().numpy() for k in keep]
    assert all(set(np.unique(k)) <= {0.0, 1.0} for k in keep_h)
    z = net.forward_train(dev(x), keep)                      # forward_train directly: H x W need not be S x S
    dz = torch.empty_like(z)
    out = net._loss(z, dev(mask), dz)
    net.backward(dz)
    torch.cuda.synchronize()
    L64, g64, mv64 = R.loss_and_grads(weights, x, mask, keep_h, torch.float64)
    L32, g32, _ = R.loss_and_grads(weights, x, mask, keep_h, torch.float32)
    o = host(out)
    for j, k in enumerate(ops.SEG_LOSS_NAMES[:3]):
        tol = max(1e-5, 4 * abs(L32[k] - L64[k]) / abs(L64[k]))
        print(f"{name} {k}: dev {o[j]:.9g} ref {L64[k]:.9g} (bound {tol:.3g})")
        assert abs(o[j] - L64[k]) / abs(L64[k]) <= tol
    worst = 0.0
    for i, ((kind, shape), gr) in enumerate(zip(specseg_spec(), g64)):
        got = host(net.grads[i])
        if gr is None:
            assert not got.any(), f"var {i} ({kind}) is not trainable"
            continue
        if i in STRUCTURAL_ZEROS.get(name, ()):
            assert not gr.any() and not got.any(), f"var {i}: the reference gradient is exactly zero, the device's must be"
            continue
        assert np.linalg.norm(gr) > 0
        fig, tol = rel_l2(got, gr), max(1e-5, 4 * rel_l2(g32[i], gr))
        print(f"{name} var{i:02d} {kind:8s} {str(shape):18s} rel-L2 {fig:.3g} (float32 reference {tol / 4:.3g}, bound {tol:.3g})")
        worst = max(worst, fig / tol)
        assert fig <= tol, (name, i, kind, fig, tol)
    bn_idx = [i for i, (k, _) in enumerate(specseg_spec()) if k == "bn_mean"]
    for i, (mm, mv) in zip(bn_idx, mv64):
        assert rel_l2(host(net.vars[i]), mm) < 1e-5 and rel_l2(host(net.vars[i + 1]), mv) < 1e-5
    print(f"{name}: worst figure / bound {worst:.3g}")


def test_trajectory_follows_the_reference():
    """20 train_steps at S = 32, B = 4 on the discs from the same weights, data and device keep masks as the float64 reference; the loss of
    every step within 4x the float32 reference's distance from the float64 one (floor 1e-5, relative)."""
    T = R.TRAJ
    B, S, steps = T["B"], T["S"], T["steps"]
    x, mask = R.discs(B, S, seed=T["data_seed"])
    net = _net(S)
    weights = net.get_weights()
    net.configure_optimizer(lr=T["lr"], beta1=0.9, beta2=0.999)
    keeps = [[k.cpu().numpy() for k in net.keep_masks(B, S, S, net.train_seed, t)] for t in range(steps)]
    recs = [net.train_step(x, mask) for _ in range(steps)]
    got = [r["loss"] for r in recs]
    l64, w64 = R.trajectory(weights, [x] * steps, [mask] * steps, keeps, T["lr"], dtype=torch.float64)
    l32, _ = R.trajectory(weights, [x] * steps, [mask] * steps, keeps, T["lr"], dtype=torch.float32)
    assert l64[-1] < 0.5 * l64[0]
    for t in range(steps):
        tol = max(1e-5, 4 * abs(l32[t] - l64[t]) / l64[t])
        fig = abs(got[t] - l64[t]) / l64[t]
        print(f"step {t:2d}: dev {got[t]:.7f} f64 {l64[t]:.7f} f32 {l32[t]:.7f} rel {fig:.3g} (bound {tol:.3g})")
    for t in range(steps):
        assert abs(got[t] - l64[t]) / l64[t] <= max(1e-5, 4 * abs(l32[t] - l64[t]) / l64[t]), t
    assert got[-1] < 0.5 * got[0] and net.iterations == steps


def test_fit_predict_evaluate():
    S = 32
    x, mask = R.discs(8, S, seed=21)
    xv, mv = R.discs(4, S, seed=22)
    net = _net(S)
    assert net.trainable is False
    before = net.predict(x[:2]).clone()
    ev0 = net.evaluate(xv, mv)
    lines = []
    hist = net.fit(x, mask, batch_size=4, epochs=6, lr=2e-3, shuffle=True, print_fn=lines.append)
    assert net.trainable is True and net.iterations == 12 and len(lines) == 6 and len(hist["loss"]) == 6
    assert hist["loss"][-1] < hist["loss"][0]
    after = net.predict(x[:2])
    assert float((after - before).abs().max()) > 1e-3
    assert float(after.min()) >= 0.0 and float(after.max()) <= 1.0
    ev1 = net.evaluate(xv, mv)
    print("evaluate before", ev0, "after", ev1)
    assert set(ev1) == {"loss", "dice", "focal", "iou", "f1"} and ev1["loss"] < ev0["loss"]


def test_checkpoint_roundtrip_and_resumed_fit_is_bitwise(tmp_path):
    from shmgan_amd import ShmGANwithSSpecSeg
    S = 32
    x, mask = R.discs(4, S, seed=31)

    def trainer():
        m = ShmGANwithSSpecSeg(image_size=S, filter_size=16, batch_size=1)
        m.build()
        return m
    a = trainer()
    old = tmp_path / "old.npz"
    a.save_npz(old)                                            # never trained: no optimiser keys
    with np.load(old) as z:
        assert not any(k.startswith("SpecSeg/adam") or k == "SpecSeg/iterations" for k in z.files)
    a.SpecSeg.fit(x, mask, batch_size=2, epochs=1, lr=1e-3, shuffle=False)
    ck = tmp_path / "ck.npz"
    a.save_npz(ck)
    with np.load(ck) as z:
        assert {"SpecSeg/adam_m", "SpecSeg/adam_v", "SpecSeg/iterations"} <= set(z.files) and int(z["SpecSeg/iterations"]) == 2
    a.SpecSeg.fit(x, mask, batch_size=2, epochs=1, shuffle=False)
    b = trainer()
    b.load_npz(ck)
    assert b.SpecSeg.iterations == 2 and b.SpecSeg.trainable
    b.SpecSeg.fit(x, mask, batch_size=2, epochs=1, lr=1e-3, shuffle=False)
    assert torch.equal(a.SpecSeg.flat, b.SpecSeg.flat) and torch.equal(a.SpecSeg.m, b.SpecSeg.m) and torch.equal(a.SpecSeg.v, b.SpecSeg.v)
    c = trainer()
    c.load_npz(old)                                            # a file without the new keys still loads
    assert c.SpecSeg.m is None and c.SpecSeg.iterations == 0 and not c.SpecSeg.trainable


def test_mask_dataset_and_train_specseg(tmp_path):
    from types import SimpleNamespace
    from PIL import Image
    from shmgan_amd import ShmGANwithSSpecSeg
    from shmgan_amd.data import MaskDataset
    S = 32
    x, mask = R.discs(4, 48, seed=41)
    idir, mdir = tmp_path / "img", tmp_path / "msk"
    idir.mkdir()
    mdir.mkdir()
    names = ["b", "d", "a", "c"]
    for k, nm in enumerate(names):
        g = x[k, ..., 0]
        g8 = np.uint8(np.clip((g - g.min()) / (g.max() - g.min()) * 255, 0, 255))
        Image.fromarray(np.stack([g8, g8, g8], -1)).save(idir / f"{nm}.png")
        Image.fromarray(np.uint8(mask[k, ..., 0] * 255)).save(mdir / f"{nm}.png")
    (mdir / "stray.png").write_bytes((mdir / "a.png").read_bytes())
    with pytest.raises(ValueError):
        MaskDataset(str(idir), str(mdir), S, 2)              # a mask without an image
    (mdir / "stray.png").unlink()
    ds = MaskDataset(str(idir), str(mdir), S, 2)
    assert ds.names == ["a", "b", "c", "d"] and len(ds) == 2
    xs, ms = ds.tensors()
    assert xs.shape == (4, S, S, 1) and ms.shape == (4, S, S, 1) and xs.is_cuda
    assert float(ms.min()) >= 0.0 and float(ms.max()) <= 1.0 and 0 < float(ms.mean()) < 1
    assert bool(((ms > 0) & (ms < 1)).any())                  # resized, not thresholded
    # the standardised Y plane exactly as train_step makes it: the loader's resize, rgb -> yuv + standardisation, channel 0
    m = ShmGANwithSSpecSeg(image_size=S, filter_size=16, batch_size=2)
    m.build()
    rgb = torch.empty((4, S, S, 3), device="cuda")
    for k, nm in enumerate(ds.names):
        with Image.open(idir / f"{nm}.png") as im:
            _ops().resize_bilinear_u8(torch.from_numpy(np.asarray(im.convert("RGB"), dtype=np.uint8)).cuda(), rgb[k])
    yuv, _ = m.preprocess(rgb, "chk")
    assert torch.allclose(xs, yuv[..., 0:1], rtol=1e-6, atol=1e-7)
    # pairing by name: image "a" is sample 2 of the generator above; its mask's disc area survives the resize
    assert abs(float(ms[0].mean()) - float(mask[2].mean())) < 0.02
    fx, fm = MaskDataset(str(idir), str(mdir), S, 2, flip_ud=True).tensors()
    # the flip applies to both (the image's standardisation scale comes from sums whose order is not fixed: the last bit may differ)
    assert torch.allclose(fx, xs.flip(1), rtol=1e-6, atol=1e-7) and torch.equal(fm, ms.flip(1))
    g0 = m.G.P.flat.clone()
    ev0 = m.SpecSeg.evaluate(xs, ms)
    log = []
    m.train_specseg(SimpleNamespace(specseg_image_dir=str(idir), specseg_mask_dir=str(mdir), specseg_epochs=8, specseg_lr=2e-3), print_fn=log.append)
    ev1 = m.SpecSeg.evaluate(xs, ms)
    print("train_specseg: evaluate before", ev0, "after", ev1)
    assert len(log) == 8 and all(k in log[-1] for k in ("loss", "dice", "focal", "iou", "f1"))
    assert m.SpecSeg.trainable and ev1["loss"] < ev0["loss"] and torch.equal(m.G.P.flat, g0)
