#!/usr/bin/env python3
"""Compare the gfx950 assembly of the product's device code between two source trees.

    tools/isa_diff.py OLD_TREE NEW_TREE [--keep DIR] [--jobs N] [--flags "..."]

Each tree is a checkout of this repository (e.g. `git worktree add ../old <rev>`).
Every .hip file of kf2vecfsw_amd/csrc/ is compiled with the product's flags plus
`--cuda-device-only -S`, the text is cut per function (`<symbol>:` up to its
`.Lfunc_end`), comments and trailing blanks are dropped and `.LBB<n>_` becomes
`.LBB_` (label comments are padded to a column that moves with the function's
index in the file, basic-block labels carry that index).  A kernel's
`.amdhsa_kernel ... .end_amdhsa_kernel` descriptor is compared as well.

One line per function symbol: file, status, old hash, new hash, VGPRs / SGPRs /
scratch bytes / static LDS bytes of the (new, else old) descriptor, symbol.
Status: same | DIFF (instructions or descriptor differ) | old-only | new-only |
renamed (a symbol of one tree whose text equals a differently named symbol of
the other; the other name follows).  Exit status 1 if any symbol DIFFers.
"""
from __future__ import annotations

import argparse
import concurrent.futures
import hashlib
import os
import re
import subprocess
import sys
import tempfile

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = "--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall"
CSRC = os.path.join("kf2vecfsw_amd", "csrc")

_FUNC = re.compile(r"^\s*\.type\s+([\w.$]+),@function")
_LBB = re.compile(r"\.LBB\d+_")
_DESC = {"vgpr": ".amdhsa_next_free_vgpr", "sgpr": ".amdhsa_next_free_sgpr",
         "scratch": ".amdhsa_private_segment_fixed_size", "lds": ".amdhsa_group_segment_fixed_size"}


def compile_asm(tree: str, src: str, out: str, flags: str) -> str:
    cmd = [HIPCC] + flags.split() + ["--cuda-device-only", "-S", os.path.join(tree, CSRC, src), "-o", out]
    subprocess.run(cmd, check=True)
    return out


def norm(line: str) -> str:
    return _LBB.sub(".LBB_", line.split(";", 1)[0].rstrip())


def functions(path: str) -> dict[str, dict]:
    """symbol -> {"body": [normalised lines], "desc": [normalised lines], regs...}"""
    with open(path) as f:
        lines = f.read().splitlines()
    syms = {m.group(1) for m in map(_FUNC.match, lines) if m}
    out: dict[str, dict] = {}
    cur = desc = None   # function whose text we are in; kernel whose descriptor we are in
    for ln in lines:
        word = ln.split(None, 1)[0] if ln.strip() else ""
        if desc is not None:
            if word == ".end_amdhsa_kernel":
                desc = None
                continue
            n = norm(ln).strip()
            if n:
                desc["desc"].append(n)
            for key, tag in _DESC.items():
                if word == tag:
                    desc[key] = n.split()[-1]
        elif word == ".amdhsa_kernel":   # (the compiler puts it before the kernel's .Lfunc_end)
            desc = out.setdefault(ln.split()[1], {"body": [], "desc": []})
        elif cur is None:
            name = ln.split(":", 1)[0] if ":" in ln and not ln[:1].isspace() else ""
            if name in syms and name not in out:
                cur = name
                out[cur] = {"body": [], "desc": []}
        elif ln.startswith(".Lfunc_end"):
            cur = None
        else:
            n = norm(ln)
            if n:
                out[cur]["body"].append(n)
    return out


def digest(fn: dict) -> str:
    return hashlib.sha256("\n".join(fn["body"] + ["--"] + fn["desc"]).encode()).hexdigest()[:12]


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--keep", help="directory that keeps the .s files (default: a temporary one)")
    ap.add_argument("--jobs", type=int, default=min(10, os.cpu_count() or 1))
    ap.add_argument("--flags", default=FLAGS)
    a = ap.parse_args()
    srcs = sorted(set(s for t in (a.old, a.new) for s in os.listdir(os.path.join(t, CSRC)) if s.endswith(".hip")))
    with tempfile.TemporaryDirectory() as tmp:
        keep = a.keep or tmp
        os.makedirs(keep, exist_ok=True)
        with concurrent.futures.ThreadPoolExecutor(a.jobs) as ex:
            jobs = {(side, s): ex.submit(compile_asm, tree, s, os.path.join(keep, f"{side}.{s}.s"), a.flags)
                    for side, tree in (("old", a.old), ("new", a.new)) for s in srcs
                    if os.path.exists(os.path.join(tree, CSRC, s))}
            asm = {key: functions(j.result()) for key, j in jobs.items()}
    bad = 0
    print(f"# flags: {a.flags} --cuda-device-only -S")
    print("# file status old_hash new_hash vgpr/sgpr/scratch/lds symbol")
    for s in srcs:
        old, new = asm.get(("old", s), {}), asm.get(("new", s), {})
        oh = {k: digest(v) for k, v in old.items()}
        nh = {k: digest(v) for k, v in new.items()}
        for sym in sorted(set(old) | set(new)):
            fn = new.get(sym) or old[sym]
            regs = "/".join(fn.get(k, "-") for k in _DESC)
            ho, hn = oh.get(sym, "-"), nh.get(sym, "-")
            other = ""
            if sym in old and sym in new:
                st = "same" if ho == hn else "DIFF"
                bad += ho != hn
            else:
                mine, theirs = (oh, nh) if sym in old else (nh, oh)
                twin = [k for k, h in theirs.items() if h == mine[sym] and k not in mine]
                st = "renamed" if twin else ("old-only" if sym in old else "new-only")
                other = " <-> " + twin[0] if twin else ""
            print(f"{s} {st} {ho} {hn} {regs} {sym}{other}")
    print(f"# {bad} symbol(s) differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
