"""The device-built get_kmers matrix (kf_kmers_rows) measured two ways.

    python tools/kmers_bench.py kernel                     # (a)
    python tools/kmers_bench.py cli --parent <checkout>    # (b)

(a) kernel: kf_kmers_rows on 2^23 packed rows (64 segments) at k = 31 (1 GiB
    out) and k = 13, beside a torch device-to-device copy of the same number of
    OUTPUT bytes.  One process, device events, 5 warm-ups, then the two take
    turns for --reps timed repetitions; medians.  The copy reads its bytes and
    writes them, the kernel reads 12 B and writes 4 (k + 1) B per row: at k = 31
    the copy moves about twice the kernel's bytes.  The target is kernel <= copy.
      kernel.<k>.kernel_ms / copy_ms / ratio (kernel over copy)
      kernel.<k>.kernel_TBps   bytes the kernel moves (in + out) over its time
      kernel.<k>.copy_TBps     bytes the copy moves (2 x out) over its time
      *_of_spec                the same over the 8 TB/s HBM specification
(b) cli: wall time of `get_kmers -k 31` and `-k 7` on --files synthetic genomes
    of --seq-len bases (written to --dir, /dev/shm by default) with this tree and
    with the tree at --parent (a built checkout of the parent commit), fresh
    processes taking turns; main_s is the time inside main() (the import and the
    device start-up are in process_s only).  The two trees' .npy files are
    compared byte for byte (sha256 over all of them, in name order).
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import shutil
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_SPEC_TBPS = 8.0


def bench_kernel(a) -> dict:
    import numpy as np
    import torch
    from kf2vecfsw_amd import counter as C
    dev = torch.device("cuda:0")
    rows, nseg = 1 << a.log2_rows, 64
    out = {}
    for k in [int(x) for x in a.k.split(",")]:
        w = k + 1
        g = torch.Generator(device=dev).manual_seed(k)
        keys = torch.randint(0, 1 << (2 * k), (rows,), dtype=torch.int64, device=dev, generator=g)
        cnts = torch.randint(1, 50, (rows,), dtype=torch.int32, device=dev, generator=g)
        n = np.full(nseg, rows // nseg, np.int64)
        src0 = np.arange(nseg, dtype=np.int64) * (rows // nseg)
        tab = C.kmers_tables(src0, n, np.concatenate([[0], np.cumsum(n)]), C.kmers_denominators(cnts, src0, n), dev)
        dst = torch.empty(rows * w, dtype=torch.float32, device=dev)
        a_, b_ = torch.empty_like(dst), torch.empty_like(dst)
        a_.fill_(1.0)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        km, cm = [], []
        for r in range(5 + a.reps):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            e[0].record()
            C.kmers_rows(keys, cnts, tab, k, 0, rows, dst, status)
            e[1].record()
            e[2].record()
            b_.copy_(a_)
            e[3].record()
            torch.cuda.synchronize()
            if r >= 5:
                km.append(e[0].elapsed_time(e[1]))
                cm.append(e[2].elapsed_time(e[3]))
        assert int(status.item()) == 0
        # spot check against the host statement of the result
        from kf2vecfsw_amd import main as M
        m = 4099
        ref = M.sparse_kmers_matrix(keys[:m].cpu().numpy().view(np.uint64), cnts[:m].cpu().numpy().view(np.uint32), k)
        ref[:, k] = cnts[:m].cpu().numpy().astype(np.float32) / tab.denom[0].item()
        ok = bool(np.array_equal(dst[: m * w].cpu().numpy().reshape(m, w), ref))
        kms, cms = float(np.median(km)), float(np.median(cm))
        out_b, in_b = rows * w * 4, rows * 12
        out[k] = {"rows": rows, "out_bytes": out_b, "in_bytes": in_b, "kernel_ms": round(kms, 4),
                  "copy_ms": round(cms, 4), "ratio_kernel_over_copy": round(kms / cms, 3),
                  "kernel_ms_minmax": [round(min(km), 4), round(max(km), 4)],
                  "copy_ms_minmax": [round(min(cm), 4), round(max(cm), 4)],
                  "kernel_TBps": round((out_b + in_b) / kms / 1e9, 3), "copy_TBps": round(2 * out_b / cms / 1e9, 3),
                  "kernel_of_spec": round((out_b + in_b) / kms / 1e9 / HBM_SPEC_TBPS, 3),
                  "copy_of_spec": round(2 * out_b / cms / 1e9 / HBM_SPEC_TBPS, 3), "reps": a.reps, "rows_ok": ok}
        print(json.dumps({k: out[k]}), file=sys.stderr, flush=True)
        del keys, cnts, dst, a_, b_
        torch.cuda.empty_cache()
    return out


_DRIVER = """
import contextlib, io, json, sys, time
sys.path.insert(0, sys.argv[1])
from kf2vecfsw_amd import main as M
t0 = time.perf_counter()
with contextlib.redirect_stdout(io.StringIO()):
    M.main(["get_kmers", "-input_dir", sys.argv[2], "-output_dir", sys.argv[3], "-k", sys.argv[4]])
print(json.dumps({"main_s": time.perf_counter() - t0}))
"""


def write_genomes(d: str, files: int, seq_len: int) -> None:
    import numpy as np
    os.makedirs(d)
    for i in range(files):
        rng = np.random.default_rng(7000 + i)
        seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, seq_len)]
        pad = (-seq_len) % 80
        lines = np.concatenate([seq, np.full(pad, ord("A"), np.uint8)]).reshape(-1, 80)
        body = np.concatenate([lines, np.full((lines.shape[0], 1), 10, np.uint8)], axis=1).tobytes()
        with open(os.path.join(d, f"syn{i:02d}.fna"), "wb") as f:
            f.write(f">syn{i}\n".encode() + body)


def digest(d: str) -> tuple[str, int]:
    h, total = hashlib.sha256(), 0
    for name in sorted(os.listdir(d)):
        h.update(name.encode())
        with open(os.path.join(d, name), "rb") as f:
            while True:
                b = f.read(1 << 24)
                if not b:
                    break
                h.update(b)
                total += len(b)
    return h.hexdigest(), total


def bench_cli(a) -> dict:
    need = int(1.1 * a.files * a.seq_len * 4 * 32)   # the k = 31 matrices, and some
    if shutil.disk_usage(a.dir).free < need:   # a small /dev/shm: the files go to the temporary directory
        import tempfile
        a.dir = tempfile.gettempdir()
    work = os.path.join(a.dir, f"kf_kmers_bench_{os.getpid()}")
    inp, outd = os.path.join(work, "in"), os.path.join(work, "out")
    res = {"files": a.files, "seq_len": a.seq_len, "dir": a.dir, "k": {}}
    try:
        write_genomes(inp, a.files, a.seq_len)
        for k in [int(x) for x in a.k.split(",")]:
            runs = {"new": [], "parent": []}
            sums = {}
            for r in range(a.reps):
                for tag, tree in (("new", ROOT), ("parent", a.parent)):
                    shutil.rmtree(outd, ignore_errors=True)
                    t0 = time.perf_counter()
                    p = subprocess.run([sys.executable, "-c", _DRIVER, tree, inp, outd, str(k)], cwd=tree,
                                       capture_output=True, text=True, timeout=a.run_timeout)
                    wall = time.perf_counter() - t0
                    if p.returncode != 0:
                        raise RuntimeError(f"{tag} k={k} failed ({p.returncode}): {p.stderr[-2000:]}")
                    runs[tag].append({"main_s": round(json.loads(p.stdout.strip().splitlines()[-1])["main_s"], 3),
                                      "process_s": round(wall, 3)})
                    sums[tag] = digest(outd)
                    print(json.dumps({"k": k, "rep": r, tag: runs[tag][-1]}), file=sys.stderr, flush=True)
            best = {t: min(x["main_s"] for x in runs[t]) for t in runs}
            res["k"][k] = {"runs": runs, "best_main_s": best, "npy_bytes": sums["new"][1],
                           "parent_over_new": round(best["parent"] / best["new"], 2),
                           "same_bytes": sums["new"] == sums["parent"]}
    finally:
        shutil.rmtree(work, ignore_errors=True)
    return res


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernel", "cli"])
    ap.add_argument("--k", default=None)
    ap.add_argument("--reps", type=int, default=None)
    ap.add_argument("--log2-rows", type=int, default=23)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--files", type=int, default=16)
    ap.add_argument("--seq-len", type=int, default=5_000_000)
    ap.add_argument("--dir", default="/dev/shm" if os.access("/dev/shm", os.W_OK) else "/tmp")
    ap.add_argument("--run-timeout", type=int, default=420)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.what == "kernel":
        a.k, a.reps = a.k or "31,13", a.reps or 20
        res = {"kernel": bench_kernel(a)}
    else:
        if not a.parent:
            ap.error("cli needs --parent")
        a.k, a.reps = a.k or "31,7", a.reps or 2
        res = {"cli": bench_cli(a)}
    s = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")
    print(s)


if __name__ == "__main__":
    main()
