"""Training telemetry on the device: shm_tensor_stats against its numpy restatement (tests/telemetry_ref.py), its independence
and read-only guarantees, the statistics of a real step's gradients, and the logs of train()."""
import argparse

import numpy as np
import pytest
import torch

import telemetry_ref as tr
from oracle import step_torch as st
from shmgan_amd import ops
from shmgan_amd import telemetry as tel
from util import host

pytestmark = pytest.mark.gpu


def _random(n, seed, lo=-45.0, hi=2.0):
    """float32 values with exponents spread over 2^lo .. 2^hi, both signs."""
    rng = np.random.default_rng(seed)
    return (np.exp2(rng.uniform(lo, hi, n)) * rng.choice([-1.0, 1.0], n)).astype(np.float32)


def _model_table(kind, F):
    """(offsets, sizes, n) of a model's variables at filter size F (storage layout only: built on the CPU)."""
    from shmgan_amd.model import Arena, Discriminator, Generator
    cpu = torch.device("cpu")
    M = Generator(64, F, cpu, Arena(cpu), lambda n: None) if kind == "G" else Discriminator(64, F, cpu, Arena(cpu), lambda n: None, 0.2)
    tab = tel.variable_table(M, kind)
    return [o for _, o, _, _ in tab], [z for _, _, z, _ in tab], M.P.n


def _check(x, offsets, sizes, scale, got):
    """Histogram, counts, min and max exactly; the two sums within the bound of any summation order (printed before asserting)."""
    stats, hist = (t.cpu().numpy() for t in got)
    rs, rh = tr.tensor_stats(x, offsets, sizes, scale)
    assert (hist == rh).all(), np.argwhere(hist != rh)[:8]
    for k in (0, 1, 2, 7):
        assert (stats[:, k] == rs[:, k]).all(), (ops.TSTAT_NAMES[k], np.argwhere(stats[:, k] != rs[:, k])[:8])
    assert (stats[:, 3] == rs[:, 3]).all() and (stats[:, 4] == rs[:, 4]).all()
    worst = [0.0, 0.0]
    for s, (o, z) in enumerate(zip(offsets, sizes)):
        bs, bq = tr.sum_bounds(x[o:o + z], scale)
        es, eq = abs(stats[s, 5] - rs[s, 5]), abs(stats[s, 6] - rs[s, 6])
        worst = [max(worst[0], es / bs if bs else es), max(worst[1], eq / bq if bq else eq)]
        assert es <= bs and eq <= bq, (s, z, es, bs, eq, bq)
    print(f"tensor_stats: {len(sizes)} segments, scale {scale}: worst |sum error| / bound {worst[0]:.3g}, sumsq {worst[1]:.3g}")
    assert (hist.reshape(len(sizes), -1).sum(axis=1) == np.asarray(sizes)).all()


@pytest.mark.parametrize("kind,F", [("G", 16), ("D", 16), ("G", 64), ("D", 64)])
def test_kernel_matches_restatement_on_the_model_tables(kind, F):
    offsets, sizes, n = _model_table(kind, F)
    x = _random(n, 10 + F)
    # planted specials: NaN / Inf in the first and the largest variable, an all-zero variable, subnormals, exact +-1
    big = int(np.argmax(sizes))
    x[offsets[0] + 1] = np.nan
    x[offsets[big] + sizes[big] // 2] = np.inf
    x[offsets[big] + sizes[big] - 1] = -np.inf
    x[offsets[big] + 8191:offsets[big] + 8194] = [1.0, -1.0, np.float32(1.0000001)]
    zero = int(np.argmin(sizes))
    x[offsets[zero]:offsets[zero] + sizes[zero]] = 0.0
    x[offsets[big] + 5] = np.array([3], dtype=np.uint32).view(np.float32)[0]
    xd = torch.from_numpy(x).cuda()
    for scale in (1.0, 0.5, 1.0 / 3.0):
        _check(x, offsets, sizes, scale, ops.tensor_stats(xd, offsets, sizes, scale=scale))


def test_kernel_small_segments_odd_offsets_and_one_large_kernel():
    n = 3 * 3 * 512 * 512 + 64
    x = _random(n, 3)
    offsets = [1, 7, 13, 19, 37, 30]
    sizes = [1, 3, 4, 5, 3 * 3 * 512 * 512, 0]            # 37: the big kernel starts 4 bytes past a 16-byte boundary
    xd = torch.from_numpy(x).cuda()
    for scale in (1.0, 1.0 / 3.0):
        _check(x, offsets, sizes, scale, ops.tensor_stats(xd, offsets, sizes, scale=scale))
    # every alignment of a short segment, lengths around the vector width and the chunk size
    offsets, sizes, o = [], [], 0
    for z in (1, 2, 3, 4, 5, 7, 8, 9, 8191, 8192, 8193, 8195, 16385):
        for a in range(4):
            o = (o + 3) // 4 * 4 + a
            offsets.append(o)
            sizes.append(z)
            o += z
    assert o <= n and len(sizes) <= ops.TSTAT_MAX_SEGS
    _check(x, offsets, sizes, 1.0, ops.tensor_stats(xd, offsets, sizes))
    # all-NaN and all-zero segments: min = max = 0, no finite value / one class
    y = np.zeros(300, dtype=np.float32)
    y[100:200] = np.nan
    got = ops.tensor_stats(torch.from_numpy(y).cuda(), [0, 100], [100, 100])
    _check(y, [0, 100], [100, 100], 1.0, got)
    assert got[0].cpu().numpy()[1].tolist() == [0, 100, 0, 0, 0, 0, 0, 0] and int(got[1][0, 0, 0]) == 100


def test_segment_results_do_not_depend_on_the_other_segments():
    offsets, sizes, n = _model_table("G", 16)
    x = _random(n, 5, -30.0, 1.0)
    xd = torch.from_numpy(x).cuda()
    s_all, h_all = (t.cpu().numpy() for t in ops.tensor_stats(xd, offsets, sizes, scale=1.0 / 3.0))
    s_two, h_two = (t.cpu().numpy() for t in ops.tensor_stats(xd, offsets, sizes, scale=1.0 / 3.0))
    assert s_all.tobytes() == s_two.tobytes() and h_all.tobytes() == h_two.tobytes()          # run to run
    s_rev, h_rev = (t.cpu().numpy() for t in ops.tensor_stats(xd, offsets[::-1], sizes[::-1], scale=1.0 / 3.0))
    assert s_rev[::-1].tobytes() == s_all.tobytes() and h_rev[::-1].tobytes() == h_all.tobytes()
    for k in (0, int(np.argmax(sizes)), len(sizes) - 1):
        s_one, h_one = (t.cpu().numpy() for t in ops.tensor_stats(xd, [offsets[k]], [sizes[k]], scale=1.0 / 3.0))
        assert s_one[0].tobytes() == s_all[k].tobytes() and h_one[0].tobytes() == h_all[k].tobytes()


def test_call_only_reads_x_and_stays_inside_its_outputs():
    from shmgan_amd._lib import check, lib
    offsets, sizes, n = _model_table("D", 16)
    nseg = len(sizes)
    x = _random(n, 6)
    xd = torch.from_numpy(x).cuda()
    nb = ops.tensor_stats_workspace(nseg, n)
    assert nb % 8 == 0
    pad = 64                                             # sentinel words behind each buffer
    stats = torch.full((nseg * ops.TSTAT_N + pad,), -7.0, dtype=torch.float64, device="cuda")
    hist = torch.full((nseg * 2 * ops.THIST_BINS + pad,), -7, dtype=torch.int64, device="cuda")
    ws = torch.full((nb // 8 + pad,), -7, dtype=torch.int64, device="cuda")
    tab = ops.SegmentTable(offsets, sizes)
    check(lib().shm_tensor_stats(xd.data_ptr(), n, tab.off, tab.len, nseg, 0.5, stats.data_ptr(), hist.data_ptr(), ws.data_ptr(), nb,
                                 torch.cuda.current_stream().cuda_stream), "shm_tensor_stats")
    torch.cuda.synchronize()
    assert xd.cpu().numpy().tobytes() == x.tobytes()
    assert (stats[-pad:] == -7.0).all() and (hist[-pad:] == -7).all() and (ws[-pad:] == -7).all()
    _check(x, offsets, sizes, 0.5, (stats[:-pad].view(nseg, ops.TSTAT_N), hist[:-pad].view(nseg, 2, ops.THIST_BINS)))


@pytest.mark.parametrize("dtype,F", [("float32", 16), ("bfloat16", 32)])
def test_grad_stats_of_a_step(dtype, F):
    """S = 64, F = 16; the bf16 models take filter sizes that are multiples of 32 (MFMA operand rows), so F = 32 there."""
    from shmgan_amd import ShmGANwithSSpecSeg
    S, B = 64, 1
    m = ShmGANwithSSpecSeg(image_size=S, filter_size=F, batch_size=B, compute_dtype=dtype).build()
    try:
        m.train_step(*st.make_inputs(B, S), draws=st.make_draws(0, B, S, F), style_factor=st.style_factor_intended(S), apply=False)
        got = m.grad_stats()
        wgt = m.weight_stats()
        for M, tag in ((m.G, "G"), (m.D, "D")):
            g, w = M.P.grad.cpu().numpy(), M.P.flat.cpu().numpy()
            tab = tel.variable_table(M, tag)
            assert len(tab) == len(M.P.vars) and set(n for n, _, _, _ in tab) <= set(got)
            for name, off, size, shape in tab:
                for res, buf in ((got, g), (wgt, w)):
                    _check(buf, [off], [size], 1.0, (torch.from_numpy(res[name]["stats"][None]), torch.from_numpy(res[name]["hist"][None])))
                    assert res[name]["shape"] == shape
            assert got[f"{tag}/var00"]["stats"][0] == M.trainable_variables[0].numel()       # finite gradients, all of them
        assert len(got) == len(m.G.P.vars) + len(m.D.P.vars)
    finally:
        m.release()


def _write_dataset(root, n, rng, hw=(40, 50)):
    from PIL import Image
    from shmgan_amd.data import PSD_SUBDIRS
    for sub in PSD_SUBDIRS:
        (root / sub).mkdir(parents=True)
        for i in range(n):
            Image.fromarray(rng.integers(0, 256, (hw[0], hw[1], 3)).astype(np.uint8)).save(root / sub / f"img_{i:03d}.png")


def test_train_writes_the_logs(tmp_path):
    from shmgan_amd import ShmGANwithSSpecSeg
    _write_dataset(tmp_path / "data", 4, np.random.default_rng(1))

    def make_args(logs, **kw):
        return argparse.Namespace(mode="train", image_size=32, batch_size=1, filter_size=16, num_epochs=2, g_lr=2e-5, d_lr=2e-5,
                                  beta1=0.5, beta2=0.99, data_dir=str(tmp_path / "data"), checkpoint_save_dir=str(tmp_path / "ckpt"),
                                  log_dir=str(tmp_path / logs), log_step=1, checkpoint_save_step=1, **kw)

    args = make_args("logs", loss_log_step=1, histogram_step=2)
    shmgan = ShmGANwithSSpecSeg(args)
    seen = []
    step0 = shmgan.train_step

    def spy(*a, **k):
        r = step0(*a, **k)
        shmgan._loss_cache = None
        seen.append((shmgan.TARGET_LABELS, shmgan.epoch, dict(shmgan.losses())))
        return r

    shmgan.train_step = spy
    assert shmgan.train(args, print_fn=lambda *a: None) == 6
    log = tel.read_log(tmp_path / "logs")
    assert [r["step"] for r in log["losses"]] == [1, 2, 3, 4, 5, 6]
    for rec, (target, epoch, want) in zip(log["losses"], seen):
        assert rec["TARGET_LABELS"] == target and rec["epoch"] == epoch
        assert set(rec) == {"step", "epoch", "TARGET_LABELS", *want}
        for k, v in want.items():
            assert np.asarray(rec[k], dtype=np.float64).tobytes() == np.asarray(v, dtype=np.float64).tobytes(), (rec["step"], k, rec[k], v)
    nG, nD = len(shmgan.G.P.vars), len(shmgan.D.P.vars)
    for key in ("gradients", "weights"):
        recs = log[key]
        assert [(r["step"], r["model"]) for r in recs] == [(s, m) for s in (2, 4, 6) for m, n in (("G", nG), ("D", nD)) for _ in range(n)] \
            or [(r["step"], r["model"]) for r in recs] == [(s, m) for s in (2, 4, 6) for m, n in (("D", nD), ("G", nG)) for _ in range(n)]
        for r in recs:
            size = int(np.prod(r["shape"]))
            assert tel.hist_dense(r).sum() == size == r["finite"] + r["nan"] + r["inf"] and r["nan"] == 0 and r["inf"] == 0
            assert all(n > 0 for _, _, n in r["hist"])
        names = [r["name"] for r in recs if r["step"] == 2]
        assert sorted(names) == sorted([f"G/var{k:02d}" for k in range(nG)] + [f"D/var{k:02d}" for k in range(nD)])
    # the weights logged at step 6 are the weights the run ended with
    last = {r["name"]: r for r in log["weights"] if r["step"] == 6}
    ws = shmgan.weight_stats()
    for name, r in last.items():
        assert (tel.hist_dense(r) == ws[name]["hist"]).all() and r["sum"] == ws[name]["stats"][5]
    # the histogram is one of the clipped values once bin 42 is read as +-1: nothing to check beyond clipped <= bin 42
    for r in log["gradients"]:
        assert r["clipped"] <= tel.hist_dense(r)[:, 42].sum()
    shmgan.release()
    # a resumed run appends, and its steps go on counting
    args.num_epochs = 1
    again = ShmGANwithSSpecSeg(args)
    assert again.train(args, max_steps=2, print_fn=lambda *a: None) == 2
    again.release()
    log2 = tel.read_log(tmp_path / "logs")
    assert [r["step"] for r in log2["losses"]] == [1, 2, 3, 4, 5, 6, 7, 8] and log2["losses"][:6] == log["losses"]
    assert sorted(set(r["step"] for r in log2["gradients"])) == [2, 4, 6, 8] and len(log2["gradients"]) == 4 * (nG + nD)
    # both options off (the default): the log folder holds the three summaries and nothing else
    off = make_args("logs_off")
    off.checkpoint_save_dir = str(tmp_path / "ckpt_off")
    quiet = ShmGANwithSSpecSeg(off)
    assert quiet.train(off, max_steps=2, print_fn=lambda *a: None) == 2 and quiet.telemetry is None
    quiet.release()
    assert sorted(p.name for p in (tmp_path / "logs_off").iterdir()) == ["Discriminator_summary.txt", "Generator_summary.txt", "SpecSeg_summary.txt"]


def test_nonfinite_gradient_raises_and_names_the_variable(tmp_path):
    from shmgan_amd import NonFiniteGradientError, ShmGANwithSSpecSeg
    S, F, B = 64, 16, 1
    m = ShmGANwithSSpecSeg(image_size=S, filter_size=F, batch_size=B, log_dir=str(tmp_path), histogram_step=1, nonfinite="raise").build()
    try:
        inp = st.make_inputs(B, S)
        t = m.start_telemetry()
        m.train_step(*inp, apply=False)
        name, off, size, shape = tel.variable_table(m.D, "D")[3]
        m.D.P.grad[off + size // 2] = float("nan")          # a data value: the kernels only count it
        t.record_gradients("D", 1.0)
        t.record_gradients("G", 1.0)
        t.stage_histograms(1)
        with pytest.raises(NonFiniteGradientError, match=name):
            t.flush()
        recs = tel.read_log(tmp_path)["gradients"]
        assert [r["name"] for r in recs if r["nan"]] == [name] and len(recs) == len(m.G.P.vars) + len(m.D.P.vars)
        # the next train_step is where a running loop hears of it
        t.record_gradients("D", 1.0)
        t.stage_histograms(2)
        t._wait("hist", 0)
        t._wait("hist", 1)
        with pytest.raises(NonFiniteGradientError, match=name):
            m.train_step(*inp, apply=False)
        # "warn" reports and goes on
        t.nonfinite = "warn"
        t.record_gradients("D", 1.0)
        t.stage_histograms(3)
        with pytest.warns(RuntimeWarning, match=name):
            t.flush()
    finally:
        m.release()
