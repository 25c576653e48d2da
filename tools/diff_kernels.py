#!/usr/bin/env python3
"""Compare the gfx950 code of two builds of libshmgan_hip.so kernel by kernel (what a source move or a host-only change must leave alone).

    python tools/diff_kernels.py old/libshmgan_hip.so new/libshmgan_hip.so      exit 0 = same symbols, same instructions

The instruction text of every symbol is compared without its addresses (branch targets stay, as offsets from the symbol) and without the
filler behind its last instruction (`s_nop 0` / zero bytes up to the next symbol's alignment or the end of the code object, which depend
on what follows the kernel in its translation unit)."""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
from kernel_isa import kernels, parse  # noqa: E402


def text(lib):
    out = {}
    for name, body in kernels(Path(lib)):
        ins = [(m, ops) for _, m, ops in parse(body)]
        while ins and ins[-1][0] in ("s_nop", "..."):
            ins.pop()
        out[name] = ins
    return out


def main(argv):
    old, new = text(argv[1]), text(argv[2])
    for name in sorted(old.keys() - new.keys()):
        print(f"only in {argv[1]}: {name}")
    for name in sorted(new.keys() - old.keys()):
        print(f"only in {argv[2]}: {name}")
    differ = [name for name in sorted(old.keys() & new.keys()) if old[name] != new[name]]
    for name in differ:
        print(f"differs: {name} ({len(old[name])} -> {len(new[name])} instructions)")
    print(f"{len(old)} / {len(new)} kernels, {len(differ)} differ")
    return 0 if old.keys() == new.keys() and not differ else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv))
