"""kf_parse_kf_floats and features.features_from_kf measured on get_frequencies
`.kf` text, against the HBM read rate, against kf_parse_kf_rows on get_chunks
text of the same size, and against the pandas parse the reference's trainers do.

    python tools/kf_float_bench.py [--k 7 3 9] [--gib 1.0] [--reps 10] [--e2e] [--e2e-k 7]
                                   [--dir /dev/shm/kf_float_bench] [--out FILE.json]

1. The kernel, for each --k: about --gib GiB of genome rows (random counts,
   seeded; normalised frequencies printed as get_frequencies prints them, by
   kf_write_kf_rows) in 16 files of many rows, read as one batch of 16 units
   and resident on the device.  In one process, device events, 3 warm-ups, then
   --reps timed repetitions in which the legs take turns; medians and (min, max):
     float_ms   the copy of the powers of five and the five launches of
                kf_parse_kf_floats (float64 values, scaler 1)
     probe_ms   kf_stream_probe over the same bytes: the practical read ceiling
     rows_ms    kf_parse_kf_rows on get_chunks text of (about) the same size,
                written as tools/kf_parse_bench.py writes it: the same passes
                with the other field parser
     text_GBps of each = its text over its time; float_vs_rows = the ratio of
                the two readers' times per byte of text
     moved_bytes = 3 x text (the line pass reads it twice, the row pass once) +
                the float64 values written; fraction_of_probe as kf_parse_bench
     equal      the parsed values are counter.features of the counts that were
                written, bit for bit
2. --e2e: a directory of one-row files at --e2e-k (a file per genome, as
   get_frequencies writes them, by kf_write_kf_files), features_from_kf(dir, k)
   from the directory to the finished store (wall clock, the device idle before
   and after) against my_read_csv's call of pandas (kf2vec/utils.py:436-437) on
   a pool of --procs processes, the frames joined and copied to the device.  The
   two take turns, --e2e-reps times each after one warm-up of the new path.
   one_batch_stages: the pinned allocation, the read (pack_ranges) and the copy
   to the device of the whole directory as one batch, each timed alone.
   Skipped (and said so) without pandas.
The pool is forked before the device is opened: its processes never touch it.
Everything written under --dir is removed at the end.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

UNITS = 16


def pandas_frame(path):
    """One file as my_read_csv reads it (kf2vec/utils.py:436-437)."""
    import pandas as pd
    return pd.read_csv(path, index_col=0, header=None, sep=",")


def genome_counts(k: int, rows: int, seed: int):
    """Random count rows as a bacterial genome's look at k: about 4.6 M k-mers spread over the columns."""
    import numpy as np
    from kf2vecfsw_amd import counter as C
    nbins = C.num_bins(k)
    mean = max(4, 4_600_000 // nbins)
    return np.random.default_rng(seed).integers(mean // 4, 2 * mean, size=(rows, nbins), dtype=np.uint32)


def write_rows_files(d: str, k: int, gib: float, threads: int):
    """UNITS files of many genome rows each: (paths, counts uint32 [R, nbins], rows per file)."""
    import numpy as np
    from kf2vecfsw_amd import _native as N
    from kf2vecfsw_amd import counter as C
    nbins = C.num_bins(k)
    one = genome_counts(k, 1, 1)
    cap = 64 + 32 * nbins
    out = ctypes.create_string_buffer(cap)
    wrote = ctypes.c_uint64(0)
    N.check(N.lib().kf_format_kf(b"G000000000", one.ctypes.data, nbins, 0, 0, out, cap, ctypes.byref(wrote)), "kf_format_kf")
    R = max(UNITS, int(gib * (1 << 30) / wrote.value))
    counts = genome_counts(k, R, 30 + k)
    row0 = np.arange(UNITS + 1, dtype=np.int64) * R // UNITS
    os.makedirs(d, exist_ok=True)
    paths = []
    for u in range(UNITS):
        a, e = int(row0[u]), int(row0[u + 1])
        names = (ctypes.c_char_p * (e - a))(*[b"G%09d" % r for r in range(a, e)])
        paths.append(os.path.join(d, "lib%02d.kf" % u))
        N.check(N.lib().kf_write_kf_rows(os.fsencode(paths[-1]), names, e - a, counts[a:e].ctypes.data, nbins, 0, 0,
                                         threads), "kf_write_kf_rows")
    return paths, counts, np.diff(row0)


def timed(legs: dict, reps: int):
    """Each leg's times in ms (device events), the legs taking turns, after 3 warm-ups."""
    import torch
    t = {name: [] for name in legs}
    for r in range(3 + reps):
        for name, f in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            torch.cuda.synchronize()
            if r >= 3:
                t[name].append(e0.elapsed_time(e1))
    return t


def kernel_legs(a, k: int, dev, threads: int) -> dict:
    import numpy as np
    import torch
    from kf2vecfsw_amd import _native as N
    from kf2vecfsw_amd import counter as C
    from kf_parse_bench import write_library
    nbins = C.num_bins(k)
    stream = torch.cuda.current_stream(dev).cuda_stream
    d = os.path.join(a.dir, "rows_k%d" % k)
    paths, counts, per_file = write_rows_files(d, k, a.gib, threads)
    hb = C.pack_ranges([(p, 0, os.path.getsize(p)) for p in paths], threads=threads)
    shutil.rmtree(d, ignore_errors=True)
    nbytes = int(hb.off[-1])
    R = int(counts.shape[0])
    d_bytes = hb.data[:nbytes].to(dev)
    d_off = torch.from_numpy(hb.off.view(np.int64).copy()).to(dev)
    n = len(paths)
    cap = R + 1
    d_vals = torch.empty((cap, nbins), dtype=torch.float64, device=dev)
    d_names = torch.empty((cap, 2), dtype=torch.int32, device=dev)
    d_row0 = torch.empty(n + 1, dtype=torch.int64, device=dev)
    d_status = torch.empty(4, dtype=torch.int64, device=dev)
    need = int(N.lib().kf_parse_kf_floats_scratch_bytes(nbytes, n, cap))
    scratch = torch.empty(need // 8, dtype=torch.int64, device=dev)
    probe_out = torch.zeros(1, dtype=torch.int32, device=dev)

    def floats():
        N.check(N.lib().kf_parse_kf_floats(d_bytes.data_ptr(), d_off.data_ptr(), n, nbytes, nbins, cap, 1.0,
                                           d_vals.data_ptr(), 8, d_names.data_ptr(), d_row0.data_ptr(),
                                           d_status.data_ptr(), scratch.data_ptr(), need, stream), "kf_parse_kf_floats")

    def probe():
        N.check(N.lib().kf_stream_probe(d_bytes.data_ptr(), nbytes // 16 * 16, probe_out.data_ptr(), stream),
                "kf_stream_probe")

    floats()
    torch.cuda.synchronize()
    assert d_status.cpu().tolist() == [0, 0, 0, 0], d_status.cpu().tolist()
    assert np.array_equal(np.diff(d_row0.cpu().numpy()), per_file)
    equal = True
    for r in range(0, R, 1 << 12):              # compared in slabs: the counts stay on the host
        m = min(1 << 12, R - r)
        want = C.features(torch.from_numpy(counts[r: r + m].view(np.int32)).to(dev))
        equal = equal and bool(torch.equal(d_vals[r: r + m], want))
    spans = d_names[:R].cpu().numpy()
    text = hb.data.numpy()
    equal = equal and all(text[s: s + ln].tobytes() == b"G%09d" % r for r, (s, ln) in list(enumerate(spans.tolist()))[:: max(1, R // 997)])
    # the yardstick: get_chunks text of the same size through kf_parse_kf_rows
    d2 = os.path.join(a.dir, "chunks_k%d" % k)
    cpaths, crows, _, _ = write_library(d2, k, nbytes / (1 << 30), UNITS, 65535, threads)
    hc = C.pack_ranges([(p, 0, os.path.getsize(p)) for p in cpaths], threads=threads)
    shutil.rmtree(d2, ignore_errors=True)
    cbytes = int(hc.off[-1])
    c_bytes = hc.data[:cbytes].to(dev)
    c_off = torch.from_numpy(hc.off.view(np.int64).copy()).to(dev)
    ccap = int(crows.shape[0]) + 1
    c_rows = torch.empty((ccap, nbins), dtype=torch.int16, device=dev)
    cneed = int(N.lib().kf_parse_kf_scratch_bytes(cbytes, UNITS, ccap))
    cscratch = torch.empty(cneed // 8, dtype=torch.int64, device=dev)
    c_row0 = torch.empty(UNITS + 1, dtype=torch.int64, device=dev)
    c_status = torch.empty(4, dtype=torch.int64, device=dev)

    def rows():
        N.check(N.lib().kf_parse_kf_rows(c_bytes.data_ptr(), c_off.data_ptr(), UNITS, cbytes, nbins, ccap,
                                         c_rows.data_ptr(), c_row0.data_ptr(), c_status.data_ptr(),
                                         cscratch.data_ptr(), cneed, stream), "kf_parse_kf_rows")

    rows()
    torch.cuda.synchronize()
    assert c_status.cpu().tolist() == [0, 0, 0, 0]
    t = timed({"float": floats, "probe": probe, "rows": rows}, a.reps)
    med = {name: float(np.median(v)) for name, v in t.items()}
    res = {"k": k, "nbins": nbins, "rows": R, "text_bytes": nbytes, "text_GiB": round(nbytes / (1 << 30), 3),
           "bytes_per_field": round(nbytes / (R * nbins), 2), "chunk_text_bytes": cbytes, "chunk_rows": int(crows.shape[0]),
           "chunk_bytes_per_field": round(cbytes / (crows.shape[0] * nbins), 2)}
    for name in t:
        res[name + "_ms"] = round(med[name], 3)
        res[name + "_ms_min_max"] = [round(min(t[name]), 3), round(max(t[name]), 3)]
    moved = 3 * nbytes + R * nbins * 8
    fg, pg = moved / med["float"] / 1e6, nbytes / med["probe"] / 1e6
    res.update({"moved_bytes": moved, "float_text_GBps": round(nbytes / med["float"] / 1e6, 1),
                "probe_GBps": round(pg, 1), "rows_text_GBps": round(cbytes / med["rows"] / 1e6, 1),
                "fraction_of_probe": round(fg / pg, 4),
                "float_vs_rows_per_byte": round((med["float"] / nbytes) / (med["rows"] / cbytes), 2),
                "fields_per_us": round(R * nbins / med["float"] / 1e3, 1), "equal": equal})
    return res


def e2e_leg(a, pool, dev, threads: int) -> dict:
    import numpy as np
    import torch
    from kf2vecfsw_amd import _native as N
    from kf2vecfsw_amd import counter as C
    from kf2vecfsw_amd import features as F
    try:
        import pandas  # noqa: F401
    except ImportError:
        return {"skipped": "pandas is not installed here"}
    k = a.e2e_k
    nbins = C.num_bins(k)
    d = os.path.join(a.dir, "genomes_k%d" % k)
    os.makedirs(d, exist_ok=True)
    G = max(4, int(a.gib * (1 << 30) / (22.6 * nbins)))
    counts = genome_counts(k, G, 70 + k)
    samples = ["G%09d" % g for g in range(G)]
    names = (ctypes.c_char_p * G)(*[s.encode() for s in samples])
    N.check(N.lib().kf_write_kf_files(os.fsencode(d), names, G, counts.ctypes.data, nbins, 0, 0, threads),
            "kf_write_kf_files")
    paths = [os.path.join(d, s + ".kf") for s in samples]
    text_bytes = sum(os.path.getsize(p) for p in paths)
    want = torch.cat([C.features(torch.from_numpy(counts[r: r + 4096].view(np.int32)).to(dev)) for r in range(0, G, 4096)])

    def new(gb):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st = F.features_from_kf(d, k, dev, batch_gb=gb)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, st

    def base():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        frames = pool.map(pandas_frame, paths, chunksize=max(1, G // (8 * a.procs)))
        t1 = time.perf_counter()
        host = np.concatenate([f.to_numpy() for f in frames])
        index = [x for f in frames for x in f.index]
        vals = torch.from_numpy(host).to(dev)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, t1 - t0, vals, index

    # the stages of one batch of the whole directory, each alone: what a single-batch run cannot overlap
    ranges = [(q, 0, os.path.getsize(q)) for q in paths]
    t0 = time.perf_counter()
    buf = torch.empty(sum((e + 15) // 16 * 16 for _, _, e in ranges), dtype=torch.uint8, pin_memory=True)
    t1 = time.perf_counter()
    hb = C.pack_ranges(ranges, threads=threads, buf=buf)
    t2 = time.perf_counter()
    on_dev = hb.data.to(dev)
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    stages = {"pinned_alloc_s": round(t1 - t0, 3), "read_s": round(t2 - t1, 3), "h2d_s": round(t3 - t2, 3)}
    del on_dev, hb, buf
    _, st = new(a.batch_gb[0])
    same = st.names == samples and bool(torch.equal(st.values, want))
    del st
    tn = {gb: [] for gb in a.batch_gb}
    tb, tparse, rel = [], [], None
    for r in range(a.e2e_reps):
        for gb in a.batch_gb:
            dt, st = new(gb)
            tn[gb].append(dt)
            del st
        dt, dp, vals, index = base()
        if r == 0:       # pandas' default parser is not correctly rounded: how far it is from the rounded value
            rel = float(((vals - want).abs() / want).max())
            same = same and index == samples
        del vals
        tb.append(dt)
        tparse.append(dp)
    shutil.rmtree(d, ignore_errors=True)
    return {"k": k, "genomes": G, "text_bytes": text_bytes, "text_GiB": round(text_bytes / (1 << 30), 3),
            "baseline": "pandas read_csv as my_read_csv, {} processes".format(a.procs), "equal": same,
            "pandas_max_rel_diff": rel, "one_batch_stages": stages, "baseline_s": [round(x, 3) for x in tb],
            "baseline_parse_s": [round(x, 3) for x in tparse],
            "new_s": {str(gb): [round(x, 3) for x in v] for gb, v in tn.items()},
            "new_text_GBps": {str(gb): round(text_bytes / min(v) / 1e9, 2) for gb, v in tn.items()},
            "speedup_best_over_best": round(min(tb) / min(min(v) for v in tn.values()), 1)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, nargs="+", default=[7, 3, 9])
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--e2e-k", type=int, default=7)
    ap.add_argument("--e2e-reps", type=int, default=2)
    ap.add_argument("--batch-gb", type=float, nargs="+", default=[1.0, 0.125])
    ap.add_argument("--procs", type=int, default=16)
    ap.add_argument("--dir", default="/dev/shm/kf_float_bench")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pool = None
    if a.e2e:                                   # before the device is opened
        import multiprocessing as mp
        pool = mp.get_context("fork").Pool(a.procs)
    import torch
    threads = min(16, os.cpu_count() or 1)
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "gib": a.gib, "reps": a.reps, "kernel": []}
    shutil.rmtree(a.dir, ignore_errors=True)
    try:
        for k in a.k:
            res["kernel"].append(kernel_legs(a, k, dev, threads))
            torch.cuda.empty_cache()
        if a.e2e:
            res["e2e"] = e2e_leg(a, pool, dev, threads)
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
