#!/usr/bin/env python3
"""Compare the device assembly of two builds kernel by kernel.

Input: two sets of the device assembly files that ``hipcc --save-temps`` leaves
(``*-hip-amdgcn-amd-amdhsa-gfx950.s``), given as files or as directories that hold them:
the build before a change (``--old``) and the build after it (``--new``).  Each kernel
symbol is mapped to its text -- the instructions from its label to the end of the function,
with its ``.amdhsa_kernel ... .end_amdhsa_kernel`` descriptor block (registers, LDS, scratch)
-- after stripping ``;`` comments and the function index from the local labels
(``.LBB<n>_``, ``.Lfunc_end<n>``), which depends on a kernel's position in its file.

Reports the kernels present on one side only, the kernels that appear more than once on a
side, and the kernels whose text differs, with the first differing lines.  Exits 1 on any of
these.  ``--allow-dup NAME`` (substring of the symbol, repeatable) names kernels that may
appear more than once on the new side, e.g. a small kernel compiled into every unit that
launches it; every copy is still compared with the old one.

It is a plain text diff by symbol: it knows nothing about particular instructions.

    hipcc ... --save-temps -c old/glm.hip       (in directory old_s/)
    hipcc ... --save-temps -c new/glm_*.hip     (in directory new_s/)
    python tools/isa_diff.py --old old_s --new new_s --allow-dup glm_finish_kernel
"""
from __future__ import annotations

import argparse
import re
import sys
from pathlib import Path

_GLOB = "*-hip-amdgcn-amd-amdhsa-*.s"
_TYPE = re.compile(r"^\s*\.type\s+(\S+),@function")
_END = re.compile(r"^\.Lfunc_end\d+:")
_LOCAL = re.compile(r"\.(LBB|Lfunc_end)\d+")


def _files(args: list[str]) -> list[Path]:
    out: list[Path] = []
    for a in args:
        p = Path(a)
        found = sorted(p.glob(_GLOB)) if p.is_dir() else [p]
        if not found or not all(f.is_file() for f in found):
            raise SystemExit(f"isa_diff: no device assembly at {a}")
        out += found
    return out


def _normalise(line: str) -> str:
    return _LOCAL.sub(r".\1", line.split(";", 1)[0]).strip()


def kernels(path: Path) -> dict[str, list[str]]:
    """symbol -> normalised text of every kernel (function with a descriptor) in one file."""
    out: dict[str, list[str]] = {}
    name, text = None, []
    for raw in path.read_text().splitlines():
        if name is None:
            m = _TYPE.match(raw)
            if m:
                name, text = m.group(1), []
            continue
        if _END.match(raw):
            if any(t.startswith(".amdhsa_kernel ") for t in text):
                if name in out:
                    raise SystemExit(f"isa_diff: {name} twice in {path}")
                out[name] = text
            name = None
            continue
        t = _normalise(raw)
        if t:
            text.append(t)
    return out


def _collect(paths: list[Path]) -> dict[str, list[tuple[Path, list[str]]]]:
    out: dict[str, list[tuple[Path, list[str]]]] = {}
    for p in paths:
        for sym, text in kernels(p).items():
            out.setdefault(sym, []).append((p, text))
    return out


def _first_diff(a: list[str], b: list[str], context: int) -> list[str]:
    i = next((k for k, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
    rows = [f"    line {i + 1} of {len(a)} / {len(b)}"]
    for k in range(i, i + context):
        rows.append(f"    - {a[k] if k < len(a) else '<end>'}")
        rows.append(f"    + {b[k] if k < len(b) else '<end>'}")
    return rows


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--old", nargs="+", required=True, help="assembly files or directories of the old build")
    ap.add_argument("--new", nargs="+", required=True, help="assembly files or directories of the new build")
    ap.add_argument("--allow-dup", action="append", default=[], metavar="NAME",
                    help="kernels (substring of the symbol) that may appear more than once on the new side")
    ap.add_argument("--context", type=int, default=3, help="differing lines shown per kernel")
    a = ap.parse_args(argv)

    old, new = _collect(_files(a.old)), _collect(_files(a.new))
    bad = 0
    for sym in sorted(set(old) - set(new)):
        print(f"only in old: {sym}")
        bad += 1
    for sym in sorted(set(new) - set(old)):
        print(f"only in new: {sym}")
        bad += 1
    for sym, copies in sorted(old.items()):
        if len(copies) > 1:
            print(f"{len(copies)} copies in old: {sym}")
            bad += 1
    identical = differing = copies_compared = 0
    for sym in sorted(set(old) & set(new)):
        copies = new[sym]
        if len(copies) > 1 and not any(n in sym for n in a.allow_dup):
            print(f"{len(copies)} copies in new ({', '.join(p.name for p, _ in copies)}): {sym}")
            bad += 1
        ref = old[sym][0][1]
        same = True
        for p, text in copies:
            copies_compared += 1
            if text != ref:
                same = False
                print(f"differs ({p.name}): {sym}")
                print("\n".join(_first_diff(ref, text, a.context)))
        identical += same
        differing += not same
    bad += differing
    print(f"kernels: {len(old)} old, {len(new)} new; compared {identical + differing} "
          f"({copies_compared} copies): {identical} identical, {differing} differing")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
