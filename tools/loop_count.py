"""Count instructions in the main loop of kernels in a gfx950 assembly listing.

    hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -S conv.hip -o conv.s
    python tools/loop_count.py conv.s --kernel conv3x3_resident_kernel v_exp v_cndmask v_cvt_pk_bf16_f32 flat_ s_set_gpr_idx s_nop

For every function whose (mangled) name contains ``--kernel`` the largest loop -- the longest span between a label and a
branch back to it -- is taken as the kernel's main loop (for the resident conv kernels: the tile loop, two units).  Printed
per kernel: the loop's instruction total, MFMA and VALU counts, one count per mnemonic prefix given on the command line,
the ``s_waitcnt`` instructions by argument, and the register / scratch figures of the compiler's resource summary.
``--json`` prints one JSON object per kernel instead of the table.
"""

from __future__ import annotations

import argparse
import json
import re
from collections import Counter

LABEL = re.compile(r"^(\.LBB\d+_\d+):")
BRANCH = re.compile(r"^\s+s_c?branch\S*\s+(\.LBB\d+_\d+)")
INSTR = re.compile(r"^\s+([a-z][a-z0-9_]*)\b(.*)$")
RESOURCE = {"vgprs": "; NumVgprs:", "agprs": "; NumAgprs:", "scratch": "; ScratchSize:", "sgprs": "; NumSgprs:", "occupancy": "; Occupancy:"}


def functions(lines: list[str], needle: str):
    """Yield (name, first line, last line) of the functions whose name contains ``needle``."""
    start, name = None, None
    for i, line in enumerate(lines):
        if start is None:
            if line.startswith("_Z") and needle in line and line.split(":")[0].isidentifier() and ": " in line:
                name, start = line.split(":")[0], i
        elif line.startswith(".Lfunc_end"):
            yield name, start, i
            start = None


def main_loop(body: list[str]) -> tuple[int, int]:
    labels = {m.group(1): i for i, line in enumerate(body) if (m := LABEL.match(line))}
    best = (0, 0)
    for i, line in enumerate(body):
        m = BRANCH.match(line)
        if m and m.group(1) in labels and labels[m.group(1)] < i and i - labels[m.group(1)] > best[1] - best[0]:
            best = (labels[m.group(1)], i)
    return best


def count(body: list[str], prefixes: list[str]) -> dict:
    lo, hi = main_loop(body)
    total, per, waits = 0, Counter(), Counter()
    for line in body[lo : hi + 1]:
        m = INSTR.match(line)
        if not m or line.lstrip().startswith((";", ".")):
            continue
        op, rest = m.group(1), m.group(2).split(";")[0].strip()
        total += 1
        if op.startswith("v_mfma"):
            per["mfma"] += 1
        elif op.startswith("v_") and not op.startswith("v_accvgpr"):
            per["valu"] += 1
        if op == "s_waitcnt":
            waits[rest] += 1
        for p in prefixes:
            if op.startswith(p):
                per[p] += 1
    out = {"loop": total, "mfma": per["mfma"], "valu": per["valu"]}
    out.update({p: per[p] for p in prefixes})
    out["s_waitcnt"] = dict(sorted(waits.items()))
    return out


def resources(lines: list[str], end: int) -> dict:
    out = {}
    for line in lines[end : end + 40]:
        for key, tag in RESOURCE.items():
            if line.startswith(tag):
                out[key] = int(line[len(tag) :].split()[0])
    return out


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("asm")
    ap.add_argument("--kernel", required=True, help="substring of the mangled kernel names to report")
    ap.add_argument("--json", action="store_true")
    ap.add_argument("prefixes", nargs="*", help="mnemonic prefixes to count, e.g. v_exp flat_ s_nop")
    args = ap.parse_intermixed_args()
    with open(args.asm) as f:
        lines = f.read().splitlines()
    for name, a, b in functions(lines, args.kernel):
        row = {"kernel": name, **count(lines[a:b], args.prefixes), **resources(lines, b)}
        if args.json:
            print(json.dumps(row))
            continue
        waits = row.pop("s_waitcnt")
        print(" ".join(f"{k}={v}" for k, v in row.items()))
        print("    s_waitcnt: " + ", ".join(f"{k} x{v}" for k, v in waits.items()))


if __name__ == "__main__":
    main()
