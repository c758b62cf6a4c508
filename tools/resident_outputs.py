"""Outputs of the weight-resident 3x3 kernels for the cases of ``tests/test_resident_epilogue_gpu.py``, as ``.npy`` files.

    python tools/resident_outputs.py OUT_DIR            # run the cases on the library of this tree
    python tools/resident_outputs.py --compare A B      # are the files of two runs bitwise equal?

A kernel change that claims "same values" is checked by running this on the build before and on the build after, on the
same machine, and comparing: every file (``y``, ``g_x`` of the residual blocks, single and paired launches; ``h`` -- the plain
32 -> 64 forward -- and ``g_x`` of the first stack conv) must be bitwise equal.  The inputs come from the tests' fixed seeds.
The case builders are always this tree's ``tests/test_resident_epilogue_gpu.py``; to run an older build, start THIS tree's
script with ``--root PARENT_TREE`` (a checkout of the parent commit with its library built): only the package is taken
from there.
"""

from __future__ import annotations

import argparse
import hashlib
import sys
from pathlib import Path

import numpy as np


def compare(a: Path, b: Path) -> int:
    names_a, names_b = sorted(p.name for p in a.glob("*.npy")), sorted(p.name for p in b.glob("*.npy"))
    if names_a != names_b or not names_a:
        print(f"different file sets: {len(names_a)} in {a}, {len(names_b)} in {b}")
        return 1
    bad = [n for n in names_a if (a / n).read_bytes() != (b / n).read_bytes()]
    for n in bad:
        x, y = np.load(a / n), np.load(b / n)
        print(f"{n}: differs, max |diff| {float(np.abs(x.astype(np.float64) - y).max()):.3e} of max {float(np.abs(x).max()):.3e}")
    digest = hashlib.sha256(b"".join((a / n).read_bytes() for n in names_a)).hexdigest()[:16]
    print(f"{len(names_a)} files, {len(bad)} differ, sha256 of {a.name}: {digest}")
    return 1 if bad else 0


def run(out: Path, root: Path) -> None:
    import importlib.util

    import torch

    sys.path.insert(0, str(root))  # the package of the tree under test
    spec = importlib.util.spec_from_file_location(  # the case builders: always this tree's
        "resident_cases", Path(__file__).resolve().parent.parent / "tests" / "test_resident_epilogue_gpu.py")
    cases = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cases)
    import multimodal_mtrssm_amd as mt

    print(f"package: {Path(mt.__file__).parent}")
    out.mkdir(parents=True, exist_ok=True)

    def save(name: str, t: torch.Tensor) -> None:
        np.save(out / f"{name}.npy", t.detach().float().cpu().numpy())

    for mid, act, kind in cases.BLOCK_CASES:
        res = cases.run_block(cases.block_case(mid, act, kind), act)
        tag = f"block{mid}_act{act}_{kind}"
        for side in ("a", "v"):
            save(f"{tag}_{side}_y", res[side][0])
            save(f"{tag}_{side}_gx", res[side][1])
        for name, t in zip(("a_y", "a_gx", "v_y", "v_gx"), res["pair"], strict=True):
            save(f"{tag}_pair_{name}", t)
    for act in (cases.ELU, cases.RELU, cases.IDENTITY):
        for kind in ("two", "few", "multi"):
            y, gx, _, _ = cases.run_stack(cases.stack_case(act, kind), act)
            save(f"stack_act{act}_{kind}_h", y)
            save(f"stack_act{act}_{kind}_gx", gx)
    print(f"wrote {len(list(out.glob('*.npy')))} files to {out}")


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"), type=Path)
    ap.add_argument("--root", type=Path, default=Path(__file__).resolve().parent.parent, help="tree whose package runs the cases")
    ap.add_argument("out", nargs="?", type=Path)
    args = ap.parse_args()
    if args.compare:
        raise SystemExit(compare(*args.compare))
    if args.out is None:
        ap.error("OUT_DIR or --compare")
    run(args.out, args.root)


if __name__ == "__main__":
    main()
