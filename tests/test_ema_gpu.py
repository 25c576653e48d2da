"""shm_ema_update on the device against its float64 restatement (tests/ema_ref.py), and the averaged generator weights through the
trainer: the schedule, what the option leaves alone, checkpoints and generator_weights()."""
import json

import numpy as np
import pytest
import torch

import ema_ref as er
from oracle import step_torch as st
from shmgan_amd import _lib, ops

pytestmark = pytest.mark.gpu

G = er.GUARD


def _views(n, oe, ow, rng):
    """ema and w as views at element offsets oe / ow into larger device buffers (so only 4-byte alignment is left of the allocation's),
    with sentinel guard bands around both; returns the device buffers, the views and the host values."""
    e, w = er.values(rng, n), er.values(rng, n)
    be = np.full(G + oe + n + G, er.SENTINEL, np.float32)
    bw = np.full(G + ow + n + G, er.SENTINEL, np.float32)
    be[G + oe:G + oe + n], bw[G + ow:G + ow + n] = e, w
    de, dw = torch.from_numpy(be).cuda(), torch.from_numpy(bw).cuda()
    ve, vw = de[G + oe:G + oe + n], dw[G + ow:G + ow + n]
    assert ve.data_ptr() % 16 == (4 * oe) % 16 and vw.data_ptr() % 16 == (4 * ow) % 16
    return (de, dw), (ve, vw), (e, w), (be, bw)


def _check_bands(de, dw, bw, oe, n):
    got = de.cpu().numpy()
    assert np.all(got[:G + oe] == er.SENTINEL) and np.all(got[G + oe + n:] == er.SENTINEL), "guard band of ema touched"
    assert np.array_equal(dw.cpu().numpy().view(np.uint32), bw.view(np.uint32)), "w changed"
    return got[G + oe:G + oe + n]


@pytest.mark.parametrize("decay", er.DECAYS)
def test_kernel_matches_the_restatement(decay):
    """Every size and every pair of offsets: |got - ref| <= 4 u max(|w|, |ema|) elementwise (ema_ref's derivation), the guard bands on
    both sides of ema keep their sentinel and w keeps its bits."""
    rng = np.random.default_rng(int(decay * 1e4))
    for n in er.SIZES:
        for oe, ow in er.OFFSETS:
            (de, dw), (ve, vw), (e, w), (_, bw) = _views(n, oe, ow, rng)
            ops.ema_update(ve, vw, n, decay)
            got = _check_bands(de, dw, bw, oe, n).astype(np.float64)
            ref = er.update(e, w, decay)
            err, tol = np.abs(got - ref), er.bound(e, w)
            assert np.all(err <= tol), (n, oe, ow, float((err / tol).max()))


def test_decay_zero_is_a_bitwise_copy():
    rng = np.random.default_rng(11)
    for n in er.SIZES:
        for oe, ow in er.OFFSETS:
            (de, dw), (ve, vw), (e, w), (_, bw) = _views(n, oe, ow, rng)
            if n >= 4:                           # a copy is a copy of the bits: NaN payloads, infinities and -0 included
                w[:4] = np.array([0x7fc01234, 0xff800000, 0x80000000, 0x00000001], np.uint32).view(np.float32)
                vw[:4] = torch.from_numpy(w[:4]).cuda()
                bw[G + ow:G + ow + 4] = w[:4]
            ops.ema_update(ve, vw, n, 0.0)
            got = _check_bands(de, dw, bw, oe, n)
            assert np.array_equal(got.view(np.uint32), w.view(np.uint32)), (n, oe, ow)


@pytest.mark.parametrize("mult", [1, 2])
def test_more_elements_than_one_trip_of_the_grid(mult):
    """n just above mult * 4 * 256 * SHM_EMA_MAX_BLOCKS (16 bytes per lane, 256 lanes per block, the capped grid): lanes take `mult` whole
    trips and the first ones one more, and n % 4 != 0 leaves a ragged tail -- in the 16-byte form behind a peeled head (offsets 1, 1)
    and in the 4-byte form (offsets 0, 1)."""
    cap = _lib.CONSTANTS["SHM_EMA_MAX_BLOCKS"]
    n = mult * 4 * 256 * cap + 1027
    assert n % 4 == 3
    rng = np.random.default_rng(3)
    for oe, ow in ((1, 1), (0, 1)):
        (de, dw), (ve, vw), (e, w), (_, bw) = _views(n, oe, ow, rng)
        ops.ema_update(ve, vw, n, 0.999)
        got = _check_bands(de, dw, bw, oe, n).astype(np.float64)
        assert np.all(np.abs(got - er.update(e, w, 0.999)) <= er.bound(e, w)), (oe, ow)


def test_nonfinite_weights_propagate():
    """Documented behaviour: the kernel does not look for NaN / Inf; they go into the average (the trainer's `nonfinite` option detects them)."""
    e = torch.ones(8, device="cuda")
    w = torch.tensor([1.0, float("nan"), float("inf"), -float("inf"), 2.0, 3.0, 4.0, 5.0], device="cuda")
    ops.ema_update(e, w, 8, 0.5)
    got = e.cpu().numpy()
    assert np.isnan(got[1]) and got[2] == np.inf and got[3] == -np.inf and np.array_equal(got[[0, 4]], np.float32([1.0, 1.5]))


def test_abort_word_and_reproducibility():
    rng = np.random.default_rng(5)
    n = 1025
    words = ops.AbortWords("cuda")
    (de, dw), (ve, vw), (e, w), (be, bw) = _views(n, 1, 1, rng)
    words.dev.fill_(1)
    ops.ema_update(ve, vw, n, 0.5, abort=words)
    assert np.array_equal(de.cpu().numpy().view(np.uint32), be.view(np.uint32))          # nothing written while the word is set
    ops.ema_update(ve, vw, n, 0.0, abort=words)
    assert np.array_equal(de.cpu().numpy().view(np.uint32), be.view(np.uint32))          # the copy form neither
    words.clear()
    ops.ema_update(ve, vw, n, 0.5, abort=words)
    first = _check_bands(de, dw, bw, 1, n)
    assert np.all(np.abs(first.astype(np.float64) - er.update(e, w, 0.5)) <= er.bound(e, w))
    # the same call on the same inputs, through the other access form (offsets 0, 1) and without abort words: the same bits
    for oe, ow in ((1, 1), (0, 1)):
        de2, dw2 = torch.from_numpy(np.concatenate([np.zeros(G + oe, np.float32), e])).cuda(), torch.from_numpy(np.concatenate([np.zeros(G + ow, np.float32), w])).cuda()
        ops.ema_update(de2[G + oe:], dw2[G + ow:], n, 0.5)
        assert np.array_equal(de2[G + oe:].cpu().numpy().view(np.uint32), first.view(np.uint32)), (oe, ow)


# ---------------------------------------------------------------------------------------------------------------- the trainer
S, F, B = 32, 16, 1
STEPS = 6


def _trainer(**kw):
    """S = 32, B = 1 and the smallest filter count the compute type takes: 16 in float32, 32 in bfloat16 (a multiple of its channel pad)."""
    from shmgan_amd import ShmGANwithSSpecSeg
    f = 32 if kw.get("compute_dtype") == "bfloat16" else F
    return ShmGANwithSSpecSeg(image_size=S, filter_size=f, batch_size=B, **kw).build()


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32).copy()


def _state(m):
    return [_bits(t) for P in (m.G.P, m.D.P) for t in (P.flat, P.m, P.v)]


@pytest.mark.parametrize("attention", ["executed", "live"])
def test_trainer_average_follows_the_schedule(attention):
    """Six steps at ema_decay = 0.9 with warm-up: G.P.ema against the restatement run on the host copies of G.P.flat, within
    K * 4 u M over the whole flat buffer -- with attention="live" that includes the branch's variables."""
    m = _trainer(ema_decay=0.9, attention=attention)
    inp = st.make_inputs(B, S)
    assert m.G.P.ema is None
    ema0 = m.G.P.flat.cpu().numpy()
    ws = []
    for _ in range(STEPS):
        m.train_step(*inp)
        ws.append(m.G.P.flat.cpu().numpy())
    assert m.G.P.ema_updates == STEPS and m.G.P.ema.numel() == m.G.P.n == ema0.size and m.G.P.ema.dtype == torch.float32
    assert any(not np.array_equal(a, b) for a, b in zip(ws, ws[1:]))
    if attention == "live":
        assert m.G.P.n > _trainer().G.P.n and m.G.attn_off < m.G.P.n
    ref, big = er.trajectory(ema0, ws, 0.9, warmup=True)
    got = m.G.P.ema.cpu().numpy().astype(np.float64)
    err, tol = np.abs(got - ref), STEPS * 4 * er.U * big
    assert np.all(err <= tol), float((err / np.maximum(tol, 1e-300)).max())
    assert not np.array_equal(got, ws[-1].astype(np.float64))                   # an average, not a copy
    # the public reader: Keras order, like get_weights()
    ew, gw = m.ema_weights(), m.G.get_weights()
    assert [a.shape for a in ew] == [a.shape for a in gw]
    k0 = m.G._korder()[0]
    o = m.G.P.offsets[k0]
    assert np.array_equal(ew[0].ravel(), m.G.P.ema[o:o + ew[0].size].cpu().numpy())
    # warm-up off: the plain recurrence
    m2 = _trainer(ema_decay=0.9, ema_warmup=False)
    e0, w2 = m2.G.P.flat.cpu().numpy(), []
    for _ in range(2):
        m2.train_step(*inp)
        w2.append(m2.G.P.flat.cpu().numpy())
    ref2, big2 = er.trajectory(e0, w2, 0.9, warmup=False)
    assert np.all(np.abs(m2.G.P.ema.cpu().numpy().astype(np.float64) - ref2) <= 2 * 4 * er.U * big2)


@pytest.mark.parametrize("dt", ["float32", "bfloat16"])
def test_average_changes_nothing_else(dt):
    """The same six steps with ema_decay 0 and 0.9: both models' weights and Adam moments and the host draw stream are bitwise equal."""
    runs = []
    inp = st.make_inputs(B, S)
    for decay in (0.0, 0.9):
        m = _trainer(ema_decay=decay, compute_dtype=dt)
        for _ in range(STEPS):
            m.train_step(*inp)
        torch.cuda.synchronize()
        runs.append((_state(m), m._rng.bit_generator.state, m._draw_count, m.G.P.ema))
    (s0, r0, c0, e0), (s1, r1, c1, e1) = runs
    assert e0 is None and e1 is not None
    assert all(np.array_equal(a, b) for a, b in zip(s0, s1))
    assert r0 == r1 and c0 == c1


def test_no_generator_update_no_average_update():
    inp = st.make_inputs(B, S)
    m = _trainer(ema_decay=0.9)
    w0 = _bits(m.G.P.flat)
    m.train_G_after = 3                          # above the epoch (0): the discriminator trains alone
    for _ in range(2):
        m.train_step(*inp)
    assert m.G.P.ema_updates == 0 and np.array_equal(_bits(m.G.P.ema), w0) and m.D.P.iterations == 2
    m.train_G_after = 0
    m.train_step(*inp, apply=False)
    assert m.G.P.ema_updates == 0 and np.array_equal(_bits(m.G.P.ema), w0)
    m.train_step(*inp)
    assert m.G.P.ema_updates == 1 and not np.array_equal(_bits(m.G.P.ema), w0)


PARENT_STATE_KEYS = {"attention", "epoch", "draw_count", "rng", "batch_step"}


def _parent_keys(m):
    """The key set of a save_npz file before the average existed: per model its variables, betas, Adam moments and counter,
    SpecSeg's variables, and the trainer state."""
    keys = {"trainer/state"}
    for name, M in (("G", m.G), ("D", m.D)):
        keys |= {f"{name}/var{i:02d}" for i in range(len(M.P.vars))} | {f"{name}/beta{i:02d}" for i in range(len(M.betas))}
        keys |= {f"{name}/adam_m", f"{name}/adam_v", f"{name}/iterations"}
    return keys | {f"SpecSeg/var{i:02d}" for i in range(len(m.SpecSeg.vars))}


def test_checkpoints(tmp_path):
    inp = st.make_inputs(B, S)
    on = _trainer(ema_decay=0.9)
    for _ in range(3):
        on.train_step(*inp)
    p_on = str(tmp_path / "on.npz")
    on.save_npz(p_on)
    with np.load(p_on) as z:
        assert set(z.files) == _parent_keys(on) | {"G/ema", "G/ema_updates"} and int(z["G/ema_updates"]) == 3
        assert z["G/ema"].shape == (on.G.P.n,) and set(json.loads(str(z["trainer/state"]))) == PARENT_STATE_KEYS
    # save and load restore the average and its counter bitwise
    back = _trainer(ema_decay=0.9)
    back.load_npz(p_on)
    assert back.G.P.ema_updates == 3 and np.array_equal(_bits(back.G.P.ema), _bits(on.G.P.ema))
    assert np.array_equal(_bits(back.G.P.flat), _bits(on.G.P.flat))
    # ... and the next step continues the schedule from there: the same bits as the run that never stopped
    on.train_step(*inp)
    back.train_step(*inp)
    assert np.array_equal(_bits(back.G.P.ema), _bits(on.G.P.ema)) and back.G.P.ema_updates == 4
    # a file written with the option off has exactly the keys it always had
    off = _trainer()
    for _ in range(2):
        off.train_step(*inp)
    p_off = str(tmp_path / "off.npz")
    off.save_npz(p_off)
    with np.load(p_off) as z:
        assert set(z.files) == _parent_keys(off) and set(json.loads(str(z["trainer/state"]))) == PARENT_STATE_KEYS
    # such a file in a trainer with the option on: average == the loaded weights, counter 0
    late = _trainer(ema_decay=0.9)
    late.train_step(*inp)
    late.load_npz(p_off)
    assert late.G.P.ema_updates == 0 and np.array_equal(_bits(late.G.P.ema), _bits(off.G.P.flat))
    assert np.array_equal(_bits(late.G.P.flat), _bits(off.G.P.flat))
    # a file with an average in a trainer with the option off: loads, and the keys are ignored
    plain = _trainer()
    plain.load_npz(p_on)
    assert plain.G.P.ema is None and plain.G.P.iterations == 3
    with pytest.raises(ValueError, match="ema"):
        plain.ema_weights()
    # a damaged average is refused before anything is touched
    with np.load(p_on) as z:
        d = {k: z[k] for k in z.files}
    d["G/ema"] = d["G/ema"][:-1]
    np.savez(str(tmp_path / "short.npz"), **d)
    before = _bits(plain.G.P.flat)
    with pytest.raises(KeyError, match="G/ema"):
        plain.load_npz(str(tmp_path / "short.npz"))
    assert np.array_equal(_bits(plain.G.P.flat), before)


@pytest.mark.parametrize("dt", ["float32", "bfloat16"])
def test_generator_weights_context(dt):
    inp = st.make_inputs(B, S)
    x = inp[0]
    a = _trainer(ema_decay=0.9, compute_dtype=dt)
    never = _trainer(ema_decay=0.9, compute_dtype=dt)          # the same run, never inside the context
    for _ in range(3):
        a.train_step(*inp)
        never.train_step(*inp)
    raw = _bits(a.G.P.flat)
    y_raw = _bits(a.infer(x, cyclic=False)[0])
    # a second trainer whose RAW weights are the average
    other = _trainer(compute_dtype=dt)
    other.G.set_weights(a.ema_weights())
    assert np.array_equal(_bits(other.G.P.flat), _bits(a.G.P.ema))
    y_other = _bits(other.infer(x, cyclic=False)[0])
    with a.generator_weights("ema") as inside:
        assert inside is a and np.array_equal(_bits(a.G.P.flat), _bits(a.G.P.ema)) and a.G.weights_dirty
        y_ema = _bits(a.infer(x, cyclic=False)[0])
    assert np.array_equal(y_ema, y_other) and not np.array_equal(y_ema, y_raw)
    assert np.array_equal(_bits(a.G.P.flat), raw) and a.G.weights_dirty
    assert np.array_equal(_bits(a.infer(x, cyclic=False)[0]), y_raw)           # the operands were redone from the restored weights
    with a.generator_weights("raw"):
        assert np.array_equal(_bits(a.G.P.flat), raw)
    # restored after an exception inside, too
    with pytest.raises(ZeroDivisionError):
        with a.generator_weights("ema"):
            a.infer(x, cyclic=False)
            1 / 0
    assert np.array_equal(_bits(a.G.P.flat), raw) and a.G.weights_dirty
    # the next step is the step of a run that never entered the context
    a.train_step(*inp)
    never.train_step(*inp)
    assert all(np.array_equal(p, q) for p, q in zip(_state(a), _state(never)))
    assert np.array_equal(_bits(a.G.P.ema), _bits(never.G.P.ema))
    with pytest.raises(ValueError, match="not one of"):
        with a.generator_weights("mean"):
            pass
    with pytest.raises(ValueError, match="no average"):
        with other.generator_weights("ema"):
            pass
