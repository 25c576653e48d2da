"""The trainer's checkpoint file: a neutral .npz with the weights in Keras variable order and layouts, the InstanceNorm betas, the
Adam state, SpecSeg and the trainer's own state.  `entries` is the one description of what the file holds; writing,
validating and applying are three loops over it.  Around it: the atomic write, the numbered files with their pruning, the
multi-rank restore and the best held-out value a resumed run has to beat.  Every function takes the trainer."""
import functools
import glob
import json
import os
import zipfile
from typing import Callable, NamedTuple

import numpy as np
import torch
import torch.distributed as td

from . import dist, telemetry

BEST_CHECKPOINT = "best.npz"          # in checkpoint_save_dir; not a ckpt-*.npz, so neither pruned nor picked by restore_latest


class Entry(NamedTuple):
    key: str
    get: Callable          # () -> the array to write; None: this trainer does not write the entry now
    put: Callable          # (array) -> None: into the trainer; None: this trainer has no use for the entry
    size: object = None    # what a file's array must look like: its shape (a tuple) or its element count (an int); None: anything
    needs: tuple = ()      # the keys a file must hold for the entry to be read from it; (): the file must hold the entry itself


def variable_keys(model, tag):
    """[(key, storage index)] of a model's variables: the file and the telemetry logs name them by their position in Keras
    variable order (<tag>/var00..), `P.vars` / `P.shapes` / `P.offsets` go by the storage index.  The two differ with the live
    attention branch, whose variables Keras creates in the middle of the layer list."""
    return [(f"{tag}/var{k:02d}", i) for k, i in enumerate(model._korder())]


def _tensor(key, buf, size=None, needs=(), owner=None):
    """A float32 device buffer, written as it is and read back in place; `owner` keeps operand copies of it (weights_dirty)."""
    def put(a):
        buf.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).reshape(buf.shape))
        if owner is not None:
            owner.weights_dirty = True
    return Entry(key, lambda: buf.detach().cpu().numpy(), put, size, needs)


def _state(t):
    """What a resumed run continues from instead of replaying the first run's opening steps: the step-level draw streams (flags / TARGET_LABELS
    generator, the Philox counter of the noise and dropout kernels), the epoch, which graph the variables belong to (`read` checks it) and, only with
    validation on (other files keep exactly the keys they always had), the best held-out value so far (best_to_beat).  Optional, for old files.
    Only with the image_hw option set: the frame (`read` checks it -- the Dense kernel D/var06 of an H x W and of a W x H frame have one
    shape and another meaning, its rows follow the NHWC flattening of the (H/32) x (W/32) map)."""
    def get():
        s = {"attention": t.attention, "epoch": int(t.epoch), "draw_count": int(t._draw_count), "rng": t._rng.bit_generator.state,
             "batch_step": int(t.batch_step)}
        if getattr(t, "_image_hw", None) is not None:
            s["image_hw"] = list(t._image_hw)
        return np.array(json.dumps(dict(s, best=t._best) if t._val_on else s))

    def put(a):
        s = json.loads(str(a))
        t.epoch, t._draw_count, t._rng.bit_generator.state, t._best = int(s["epoch"]), int(s["draw_count"]), s["rng"], s.get("best")
    return Entry("trainer/state", get, put, None, ("trainer/state",))


def entries(t):
    """Every entry of the file of trainer `t` (built)."""
    yield _state(t)
    for tag, M in (("G", t.G), ("D", t.D)):
        P = M.P
        for key, i in variable_keys(M, tag):
            yield _tensor(key, P.vars[i], tuple(P.shapes[i]), owner=M)
        for i, b in enumerate(M.betas):
            yield _tensor(f"{tag}/beta{i:02d}", b)
        yield _tensor(f"{tag}/adam_m", P.m, P.n)
        yield _tensor(f"{tag}/adam_v", P.v, P.n)
        yield Entry(f"{tag}/iterations", lambda P=P: np.int64(P.iterations), lambda a, P=P: setattr(P, "iterations", int(a)))
    # the average of the generator's weights as its flat buffer, like G/adam_m, with its update count: written only with ema_decay on,
    # accepted whenever a file has it, taken from the file by a trainer that keeps one (ema_decay on) or is to evaluate with one
    # (eval_weights "ema"); a trainer with neither option ignores the keys (`apply` deals with a file without them)
    P, on = t.G.P, t._ema_on()
    take = on or t.args.eval_weights == "ema"

    def put_ema(a):
        P.ema = torch.empty_like(P.flat)
        _tensor("G/ema", P.ema).put(a)
    yield Entry("G/ema", lambda: t._ensure_ema().cpu().numpy() if on else None, put_ema if take else None, P.n, ("G/ema",))
    yield Entry("G/ema_updates", lambda: np.int64(P.ema_updates) if on else None, (lambda a: setattr(P, "ema_updates", int(a))) if take else None,
                None, ("G/ema",))
    # the mask network: optional in a file, and beyond that its Adam state, there once it has been trained here (a resumed fit()
    # continues from it).  SpecSeg hands out and takes back those four values together: one call per save, one per load
    S = t.SpecSeg
    for i, v in enumerate(S.vars):
        yield _tensor(f"SpecSeg/var{i:02d}", v, needs=("SpecSeg/var00",), owner=S)
    opt, got = functools.lru_cache(None)(S.optimizer_state), {}

    def put_opt(k, a):
        got[k] = a
        if len(got) == 4:
            S.set_optimizer_state(**got)
    for k in ("adam_m", "adam_v", "iterations", "train_state"):
        yield Entry(f"SpecSeg/{k}", lambda k=k: (opt() or {}).get(k), functools.partial(put_opt, k), S.n if k.startswith("adam") else None,
                    ("SpecSeg/var00", "SpecSeg/adam_m"))


def save(t, file):
    """Weights + IN betas + Adam state of trainer `t` in a neutral .npz (Keras variable order and layouts), to a path or a file object."""
    arrays = {e.key: e.get() for e in entries(t)}
    np.savez(file, **{k: a for k, a in arrays.items() if a is not None})


def read(t, path):
    """Read and validate a file completely without mutating anything: every array this trainer's models need is decoded (zipfile
    checks the CRC of each member as it is read) and checked.  Returns {key: array}.  A mismatch raises KeyError; a file damaged as
    a file raises zipfile.BadZipFile, EOFError or ValueError."""
    if t.G is None:
        t.build()
    arrays = {}
    with np.load(path) as z:
        for e in entries(t):
            if not all(k in z.files for k in e.needs):
                continue
            a = arrays[e.key] = z[e.key]
            mode = json.loads(str(a))["attention"] if e.key == "trainer/state" else t.attention
            if mode != t.attention:
                raise KeyError(f"checkpoint {path} holds an attention='{mode}' model, this trainer was built with "
                               f"attention='{t.attention}' (the live branch adds 20 + 4 variables)")
            if e.key == "trainer/state":
                _check_frame(t, path, json.loads(str(a)).get("image_hw"), z["D/var06"] if "D/var06" in z.files else None)
            if isinstance(e.size, tuple) and tuple(a.shape) != e.size:
                raise KeyError(f"checkpoint {path}: {e.key} has shape {tuple(a.shape)}, this model's is {e.size}")
            if isinstance(e.size, int) and a.size != e.size:
                whose = "the network's" if e.key.startswith("SpecSeg/") else "this model's"
                raise KeyError(f"checkpoint {path}: {e.key} has {a.size} elements, {whose} flat buffer {e.size}")
    return arrays


def _check_frame(t, path, saved, dense):
    """The frame a file was trained on against this trainer's: `saved` is the file's image_hw (None: a file of a trainer without the
    option, whose frame is a square).  Only a trainer that knows its frame as a pair is checked; a mismatch is the Dense kernel's."""
    mine = getattr(t, "image_hw", None)
    if mine is None or (saved is None and mine[0] == mine[1]):
        return
    if saved is None or tuple(int(v) for v in saved) != tuple(mine):
        rows = "?" if dense is None else dense.shape[0]
        was = "a square frame" if saved is None else f"a {saved[0]} x {saved[1]} frame ({saved[0] // 32} x {saved[1] // 32} map)"
        raise KeyError(f"checkpoint {path}: D/var06 (the Dense kernel, {rows} rows) was trained on {was}, this model's frame is "
                       f"{mine[0]} x {mine[1]} ({mine[0] // 32} x {mine[1] // 32} map): its rows follow the NHWC flattening of that map")


def apply(t, arrays):
    """Put what `read` returned into the trainer.  A file without an average leaves a trainer with ema_decay on with average = the
    loaded weights and the counter at 0."""
    t.G.P.ema, t._loaded_ema = None, "G/ema" in arrays
    for e in entries(t):
        if e.key in arrays and e.put is not None:
            e.put(arrays[e.key])
    if t._ema_on():
        t._ensure_ema()


def write_atomic(t, path):
    """`save` under a temporary name, flushed to disk, then an atomic rename: no half-written file ever has the final name."""
    tmp = path + ".tmp"
    with open(tmp, "wb") as f:                 # a file object: np.savez would append ".npz" to a name
        save(t, f)
        f.flush()
        os.fsync(f.fileno())
    os.replace(tmp, path)


def checkpoints(directory):
    """The numbered files ckpt-<n>.npz of a directory, oldest first."""
    return sorted(glob.glob(os.path.join(directory, "ckpt-*.npz")), key=lambda p: int(os.path.basename(p)[5:-4]))


def save_numbered(t, max_to_keep=3):
    """tf.train.CheckpointManager(ckpt, checkpoint_dir, max_to_keep=3).save() (SHM.py:944, 1127).  Rank 0 writes (to a
    temporary name, then an atomic rename) and prunes; every rank leaves through a barrier, so nobody races ahead into a
    collective while the file is still being written and nobody deletes a file another rank is about to open."""
    if t.telemetry is not None:
        t.telemetry.flush()       # a log never trails a checkpoint
    path = None
    t._check_abort(sync=True)     # never write a checkpoint behind a step whose kernels gave up
    if dist.rank() == 0:
        c = checkpoints(t.checkpoint_save_dir)
        n = int(os.path.basename(c[-1])[5:-4]) + 1 if c else 1
        path = os.path.join(t.checkpoint_save_dir, f"ckpt-{n}.npz")
        write_atomic(t, path)
        for old in (c + [path])[:-max_to_keep]:
            os.remove(old)
    dist.barrier()
    return path


def restore_latest(t):
    """Load the newest checkpoint that reads back.  ONE rank decides: rank 0 reads every candidate completely (every array
    decoded, i.e. CRC-checked, names and shapes checked against this trainer) WITHOUT touching any state, newest first,
    skipping only files that are damaged as files (zipfile.BadZipFile / EOFError: a run killed mid-write by an older version,
    a full disk); the chosen path (or None) is broadcast, every rank loads exactly that file, and the ranks then agree on a
    success flag -- a rank that could not load what rank 0 chose ends the job (non-zero exit) instead of training on other
    weights, Adam state and draw streams than its peers.  Anything else (EACCES, EIO, a checkpoint of another model
    configuration or attention mode) is not a damaged file: rank 0 broadcasts the reason and EVERY rank raises it (round-4 advisor
    finding: rank 0 used to raise in front of the broadcast and leave its peers waiting in it).  Files are read through `t._read_npz`."""
    multi = dist.multi()
    if t.G is None:
        t.build()
    chosen, payload, fatal = None, None, None
    if dist.rank() == 0:
        try:
            for path in reversed(checkpoints(t.checkpoint_save_dir)):
                try:
                    payload = t._read_npz(path)
                    chosen = path
                    break
                except (zipfile.BadZipFile, EOFError, ValueError) as e:
                    # ValueError: np.load / json on an intact zip member with a damaged .npy header or state string -- a damaged file like
                    # the other two.  read's own checks (names, shapes, attention mode) raise KeyError, which is not swallowed here
                    print(f"checkpoint {path} is unreadable ({type(e).__name__}: {e}); trying the previous one")
        except Exception as e:                      # not a damaged file: every rank must hear about it before rank 0 raises
            fatal = e                                # (the others would sit in the broadcast until the collective times out)
    if multi:
        box = [chosen, None if fatal is None else repr(fatal)]
        td.broadcast_object_list(box, src=0)
        chosen, why = box
        if why is not None:
            raise RuntimeError(f"rank {dist.rank()}: rank 0 could not choose a checkpoint: {why}") from fatal
    elif fatal is not None:
        raise fatal
    ok, err = 1, None
    if chosen is not None:
        try:
            if payload is None:
                payload = t._read_npz(chosen)
            apply(t, payload)
        except Exception as e:                      # reported after the ranks have compared notes, never swallowed
            ok, err = 0, e
    if multi:
        flag = torch.tensor([ok], dtype=torch.int32, device=t.device if td.get_backend() == "nccl" else "cpu")
        td.all_reduce(flag, op=td.ReduceOp.MIN)
        if int(flag.item()) == 0:
            raise RuntimeError(f"rank {dist.rank()}: the ranks disagree about checkpoint {chosen} (this rank: "
                               f"{'loaded' if ok else repr(err)}); refusing to train on diverged replicas") from err
    elif err is not None:
        raise err
    return chosen


def best_to_beat(record, best_path, monitor, weights):
    """The best monitored value {"monitor", "weights", "value", "step"} a resumed run has to beat: `record`, that of the restored
    checkpoint's trainer state, and that of best.npz itself (written before the checkpoint of its epoch, so it may be the newer of
    the two), whichever is better; one recorded for another monitor or weight set does not count.  None: nothing to beat."""
    cands = [record]
    if os.path.exists(best_path):
        with np.load(best_path) as z:
            if "trainer/state" in z.files:
                cands.append(json.loads(str(z["trainer/state"])).get("best"))
    best = None
    for b in cands:
        if b and (b.get("monitor"), b.get("weights")) == (monitor, weights) and telemetry.improves(monitor, b["value"], None if best is None else best["value"]):
            best = dict(b)
    return best
