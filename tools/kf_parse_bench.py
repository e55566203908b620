"""kf_parse_kf_rows and chunks.chunk_store_from_kf measured on a get_chunks-like
`.kf` directory, against the HBM read rate and against the host parse the
reference's chunk trainers do.

    python tools/kf_parse_bench.py [--k 7] [--gib 1.0] [--files 64] [--max-count 65535] [--reps 10]
                                   [--e2e] [--dir /dev/shm/kf_parse_bench] [--out FILE.json]

The directory: --files files of random uint16 rows (values 0..--max-count, seeded)
written by kf_write_kf_segments16 as get_chunks writes them (window names, raw
counts), about --gib GiB of text in all.  It is removed at the end.

1. The kernel: the whole directory read as one batch of units (a file each),
   resident on the device.  In one process, device events, 3 warm-ups, then --reps
   timed repetitions in which the two take turns; medians and (min, max):
     kernel_ms  the five launches of kf_parse_kf_rows
     probe_ms   kf_stream_probe over the same bytes: the practical read ceiling
     moved_bytes = 3 x text (the line pass reads it twice, to count and to
                 scatter, and the row pass once) + the uint16 rows written;
                 kernel_GBps = moved_bytes / kernel_ms
     fraction_of_probe = kernel_GBps / probe_GBps
     text_GBps  the text alone over kernel_ms (what a caller sees)
     equal      the parsed rows are the rows that were written, bit for bit
2. --e2e: chunk_store_from_kf(dir, k) from the directory to the finished store
   (wall clock, the device idle before and after), at each --batch-gb, against
   what there was before it: the files parsed as my_read_csv_chunk parses them
   (pandas, uint16 columns) by a pool of --procs processes, then
   ChunkStore.from_host.  Without pandas the pool runs chunks.parse_kf_rows_host
   and "baseline" says so.  The two take turns, --e2e-reps times each after one
   warm-up of the new path.  read_GBps (pack_ranges into a pinned buffer) and
   h2d_GBps (that buffer to the device) are measured on the same bytes, so it is
   plain which stage sets the pace.
The pool is forked before the device is opened: its processes never touch it.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import shutil
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def pandas_rows(job):
    """One file as my_read_csv_chunk reads it (kf2vec/utils.py:402-405): uint16 [rows, nbins]."""
    path, nbins = job
    import numpy as np
    import pandas as pd
    dt = {0: str}
    dt.update((i, np.uint16) for i in range(1, nbins + 1))
    return pd.read_csv(path, sep=",", index_col=0, header=None, dtype=dt, low_memory=True).to_numpy()


def statement_rows(job):
    path, nbins = job
    from kf2vecfsw_amd import chunks as CH
    rows, status = CH.parse_kf_rows_host(open(path, "rb").read(), nbins)
    assert status == (0, 0, 0)
    return rows


def write_library(d: str, k: int, gib: float, files: int, max_count: int, threads: int):
    """The directory and the rows that were written: (paths, rows uint16 [R, nbins], rows per file, seconds of writing)."""
    import numpy as np
    from kf2vecfsw_amd import _native as N
    from kf2vecfsw_amd import counter as C
    nbins = C.num_bins(k)
    rng = np.random.default_rng(20 + k)
    probe = rng.integers(0, max_count + 1, size=1 << 16)
    per_field = float(np.mean([len(str(int(v))) for v in probe])) + 1 + 2 * (1 - (1 - 1 / (max_count + 1)) ** nbins)
    per_row = 45 + per_field * nbins
    R = max(files, int(gib * (1 << 30) / per_row))
    rows = rng.integers(0, max_count + 1, size=(R, nbins), dtype=np.uint16)
    row0 = (np.arange(files + 1, dtype=np.int64) * R // files).astype(np.int32)
    shutil.rmtree(d, ignore_errors=True)
    os.makedirs(d)
    paths = [os.path.join(d, "g%05d.kf" % f) for f in range(files)]
    enc = [os.fsencode(p) for p in paths]
    parr = (ctypes.c_char_p * files)(*enc)
    pre = [b"g%05d.part_ctg1.part_ctg1_sliding__" % f for f in range(files)]
    prearr = (ctypes.c_char_p * files)(*pre)
    rpre = np.repeat(np.arange(files, dtype=np.uint32), np.diff(row0)).astype(np.uint32)
    rpos = ((np.arange(R, dtype=np.uint64) - row0[rpre].astype(np.uint64)) * np.uint64(10000)).astype(np.uint64)
    app = np.zeros(files, np.uint8)
    t0 = time.perf_counter()
    N.check(N.lib().kf_write_kf_segments16(files, parr, row0.ctypes.data, app.ctypes.data, None, prearr,
                                           rpre.ctypes.data, rpos.ctypes.data, 10000, rows.ctypes.data, nbins, 0, 1,
                                           threads), "kf_write_kf_segments16")
    return paths, rows, np.diff(row0), time.perf_counter() - t0


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=7)
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--files", type=int, default=64)
    ap.add_argument("--max-count", type=int, default=65535)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--e2e-reps", type=int, default=2)
    ap.add_argument("--batch-gb", type=float, nargs="+", default=[1.0, 0.125])
    ap.add_argument("--procs", type=int, default=16)
    ap.add_argument("--dir", default="/dev/shm/kf_parse_bench")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pool = None
    if a.e2e:                                   # before the device is opened
        import multiprocessing as mp
        pool = mp.get_context("fork").Pool(a.procs)
    import numpy as np
    import torch
    from kf2vecfsw_amd import _native as N
    from kf2vecfsw_amd import chunks as CH
    from kf2vecfsw_amd import counter as C
    threads = min(16, os.cpu_count() or 1)
    nbins = C.num_bins(a.k)
    paths, rows, per_file, write_s = write_library(a.dir, a.k, a.gib, a.files, a.max_count, threads)
    text_bytes = sum(os.path.getsize(p) for p in paths)
    R = int(rows.shape[0])
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "k": a.k, "nbins": nbins, "files": a.files, "rows": R,
           "max_count": a.max_count, "text_bytes": text_bytes, "text_GiB": round(text_bytes / (1 << 30), 3),
           "bytes_per_field": round(text_bytes / (R * nbins), 2), "write_GBps": round(text_bytes / write_s / 1e9, 2),
           "reps": a.reps}
    try:
        # ---- 1. the kernel on resident bytes
        ranges = [(p, 0, os.path.getsize(p)) for p in paths]
        hb = C.pack_ranges(ranges, threads=threads)
        nbytes = int(hb.off[-1])
        t0 = time.perf_counter()
        hb = C.pack_ranges(ranges, threads=threads, buf=hb.data)
        read_s = time.perf_counter() - t0
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        d_bytes = hb.data[:nbytes].to(dev)
        torch.cuda.synchronize()
        e0.record()
        d_bytes.copy_(hb.data[:nbytes], non_blocking=True)
        e1.record()
        torch.cuda.synchronize()
        res.update({"read_GBps": round(nbytes / read_s / 1e9, 2), "h2d_GBps": round(nbytes / e0.elapsed_time(e1) / 1e6, 2)})
        d_off = torch.from_numpy(hb.off.view(np.int64).copy()).to(dev)
        n = len(paths)
        cap = (nbytes + n) // (2 * nbins + 1)
        d_rows = torch.empty((cap, nbins), dtype=torch.int16, device=dev)
        d_row0 = torch.empty(n + 1, dtype=torch.int64, device=dev)
        d_status = torch.empty(4, dtype=torch.int64, device=dev)
        need = int(N.lib().kf_parse_kf_scratch_bytes(nbytes, n, cap))
        scratch = torch.empty(need // 8, dtype=torch.int64, device=dev)
        probe_out = torch.zeros(1, dtype=torch.int32, device=dev)

        def kernel():
            N.check(N.lib().kf_parse_kf_rows(d_bytes.data_ptr(), d_off.data_ptr(), n, nbytes, nbins, cap,
                                             d_rows.data_ptr(), d_row0.data_ptr(), d_status.data_ptr(),
                                             scratch.data_ptr(), need, torch.cuda.current_stream(dev).cuda_stream),
                    "kf_parse_kf_rows")

        def probe():
            N.check(N.lib().kf_stream_probe(d_bytes.data_ptr(), nbytes // 16 * 16, probe_out.data_ptr(),
                                            torch.cuda.current_stream(dev).cuda_stream), "kf_stream_probe")

        kernel()
        torch.cuda.synchronize()
        assert d_status.cpu().tolist() == [0, 0, 0, 0], d_status.cpu().tolist()
        assert np.array_equal(np.diff(d_row0.cpu().numpy()), per_file)
        equal = True
        for r in range(0, R, 1 << 14):          # compared in slabs: the written rows stay on the host
            m = min(1 << 14, R - r)
            equal = equal and bool(torch.equal(d_rows[r: r + m], torch.from_numpy(rows[r: r + m].view(np.int16)).to(dev)))
        t = {"kernel": [], "probe": []}
        for r in range(3 + a.reps):
            for name, f in (("kernel", kernel), ("probe", probe)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                f()
                e1.record()
                torch.cuda.synchronize()
                if r >= 3:
                    t[name].append(e0.elapsed_time(e1))
        med = {k: float(np.median(v)) for k, v in t.items()}
        moved = 3 * nbytes + R * nbins * 2
        for k in t:
            res[k + "_ms"] = round(med[k], 3)
            res[k + "_ms_min_max"] = [round(min(t[k]), 3), round(max(t[k]), 3)]
        kg, pg = moved / med["kernel"] / 1e6, nbytes / med["probe"] / 1e6
        res.update({"batch_bytes": nbytes, "cap_rows": cap, "moved_bytes": moved, "kernel_GBps": round(kg, 1),
                    "text_GBps": round(nbytes / med["kernel"] / 1e6, 1), "probe_GBps": round(pg, 1),
                    "fraction_of_probe": round(kg / pg, 4), "rows_per_workgroup_slot": round(R / 2048, 2),
                    "equal": equal})
        del d_rows, d_bytes, scratch, hb
        torch.cuda.empty_cache()
        # ---- 2. the directory to the store, against the host parse
        if a.e2e:
            try:
                import pandas  # noqa: F401
                base_fn, base_name = pandas_rows, "pandas read_csv as my_read_csv_chunk, {} processes".format(a.procs)
            except ImportError:
                base_fn, base_name = statement_rows, "chunks.parse_kf_rows_host, {} processes (no pandas)".format(a.procs)
            samples = [os.path.basename(p)[:-3] for p in paths]
            ref = torch.from_numpy(rows.view(np.int16))

            def new(gb):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                st = CH.chunk_store_from_kf(a.dir, a.k, dev, batch_gb=gb)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                return dt, st

            def base():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                parsed = pool.map(base_fn, [(p, nbins) for p in paths], chunksize=1)
                t1 = time.perf_counter()
                st = CH.ChunkStore.from_host(parsed, samples, a.k, dev)
                torch.cuda.synchronize()
                return time.perf_counter() - t0, t1 - t0, st

            _, st = new(a.batch_gb[0])
            same = st.samples == samples and bool(torch.equal(st.counts.cpu(), ref))
            del st
            tn = {gb: [] for gb in a.batch_gb}
            tb, tparse = [], []
            for r in range(a.e2e_reps):
                for gb in a.batch_gb:
                    dt, st = new(gb)
                    tn[gb].append(dt)
                    del st
                dt, dp, st = base()
                if r == 0:
                    same = same and st.samples == samples and bool(torch.equal(st.counts.cpu(), ref))
                del st
                tb.append(dt)
                tparse.append(dp)
            res["e2e"] = {"baseline": base_name, "equal": same,
                          "baseline_s": [round(x, 3) for x in tb], "baseline_parse_s": [round(x, 3) for x in tparse],
                          "new_s": {str(gb): [round(x, 3) for x in v] for gb, v in tn.items()},
                          "new_text_GBps": {str(gb): round(text_bytes / min(v) / 1e9, 2) for gb, v in tn.items()},
                          "speedup_best_over_best": round(min(tb) / min(min(v) for v in tn.values()), 1)}
    finally:
        if pool is not None:
            pool.close()
            pool.join()
        shutil.rmtree(a.dir, ignore_errors=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
