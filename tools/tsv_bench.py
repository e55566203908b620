"""kf_parse_tsv_floats and tables.true_distances measured on a generated distance
matrix, against kf_parse_kf_floats on get_frequencies text of the same size and
against the pandas lines of the reference's distance trainers.

    python tools/tsv_bench.py [--n 4000] [--reps 10] [--e2e-reps 3] [--commit ID]
                              [--dir /dev/shm/tsv_bench] [--out profiles/r19/tsv_floats.json]

The input: an N x N symmetric matrix of repr(float64) distances under a header
line, as get_distances writes a `.di_mtrx` (N = 4,000: about 0.3 GB of text).
1. The kernel, the text behind the header resident on the device as one batch
   of 16 units (kf_line_pieces).  In one process, device events, 3 warm-ups, then
   --reps timed repetitions in which the legs take turns; medians and (min, max):
     tsv_ms     the copy of the powers of five and the five launches of
                kf_parse_tsv_floats, float64, the identity map (d_col_map NULL)
     tsv_map_ms the same with a shuffled column map (the strided store that
                true_distances asks for)
     kf_ms      kf_parse_kf_floats at k=7 on get_frequencies text of (about) the
                same byte count, written as tools/kf_float_bench.py writes it
     probe_ms   kf_stream_probe over the matrix's bytes
     tsv_vs_kf_per_byte = the ratio of the two readers' times per byte of text
     equal      the parsed values are the matrix that was written, bit for bit
2. End to end, wall clock, the device idle before and after, the two taking
   turns --e2e-reps times after one warm-up of the new path:
     new_s      tables.true_distances(path, order) with a shuffled order, from
                the file to the finished tensor on the device
     pandas_s   the reference's lines on the same file: pd.read_csv(path,
                sep='\\t', header=0, index_col=0), utils.sort_df's two reindex
                calls and to_numpy (kf2vec/utils.py:141-192), then the copy to
                the device; pandas_read_s is the read_csv part
     speedup_best_over_best = min(pandas_s) / min(new_s)
Everything written under --dir is removed at the end.
"""
from __future__ import annotations

import argparse
import json
import os
import shutil
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

UNITS = 16


def write_matrix(path: str, n: int, seed: int = 19):
    """An n x n symmetric matrix of distances with a zero diagonal as a `.di_mtrx`: (names, the float64 matrix)."""
    import numpy as np
    rng = np.random.default_rng(seed)
    m = rng.random((n, n)) * 3.0
    m = np.triu(m, 1)
    m = m + m.T
    names = ["G%09d" % i for i in range(n)]
    with open(path, "wb") as f:
        f.write(("\t" + "\t".join(names) + "\n").encode())
        for i in range(n):
            f.write((names[i] + "\t" + "\t".join(map(repr, m[i].tolist())) + "\n").encode())
    return names, m


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


def kernel_legs(a, path: str, m, dev, threads: int) -> dict:
    import numpy as np
    import torch
    from kf2vecfsw_amd import _native as N
    from kf2vecfsw_amd import chunks as CH
    from kf2vecfsw_amd import counter as C
    from kf2vecfsw_amd import tables as T
    from kf_float_bench import write_rows_files
    n = a.n
    stream = torch.cuda.current_stream(dev).cuda_stream
    _, behind = T._first_line(path)
    size = os.path.getsize(path)
    pieces = CH.kf_line_pieces(path, (size - behind) // UNITS + 1, behind)
    hb = C.pack_ranges([(path, s, e) for s, e in pieces], threads=threads)
    nbytes = int(hb.off[-1])
    d_bytes = hb.data[:nbytes].to(dev)
    d_off = torch.from_numpy(hb.off.view(np.int64).copy()).to(dev)
    nu = len(pieces)
    cap = n + 1
    d_vals = torch.empty((cap, n), dtype=torch.float64, device=dev)
    d_names = torch.empty((cap, 2), dtype=torch.int32, device=dev)
    d_row0 = torch.empty(nu + 1, dtype=torch.int64, device=dev)
    d_status = torch.empty(4, dtype=torch.int64, device=dev)
    need = int(N.lib().kf_parse_tsv_floats_scratch_bytes(nbytes, nu, cap))
    scratch = torch.empty(need // 8, dtype=torch.int64, device=dev)
    probe_out = torch.zeros(1, dtype=torch.int32, device=dev)
    perm = np.random.default_rng(1).permutation(n)
    d_map = torch.from_numpy(perm.astype(np.int32)).to(dev)

    def tsv(cmap=None):
        N.check(N.lib().kf_parse_tsv_floats(d_bytes.data_ptr(), d_off.data_ptr(), nu, nbytes, n,
                                            None if cmap is None else cmap.data_ptr(), n, cap, d_vals.data_ptr(), 8,
                                            d_names.data_ptr(), d_row0.data_ptr(), d_status.data_ptr(),
                                            scratch.data_ptr(), need, stream), "kf_parse_tsv_floats")

    def probe():
        N.check(N.lib().kf_stream_probe(d_bytes.data_ptr(), nbytes // 16 * 16, probe_out.data_ptr(), stream),
                "kf_stream_probe")

    want = torch.from_numpy(m).to(dev)
    tsv(d_map)
    torch.cuda.synchronize()
    assert d_status.cpu().tolist() == [0, 0, 0, 0], d_status.cpu().tolist()
    equal = bool(torch.equal(d_vals[:n].index_select(1, torch.from_numpy(perm).to(dev)), want))   # field j is column perm[j]
    tsv()
    torch.cuda.synchronize()
    assert d_status.cpu().tolist() == [0, 0, 0, 0], d_status.cpu().tolist()
    equal = equal and bool(torch.equal(d_vals[:n], want)) and int(d_row0[-1]) == n
    del want
    # the yardstick: get_frequencies text of the same size at k=7 through kf_parse_kf_floats
    k = 7
    nbins = C.num_bins(k)
    d = os.path.join(a.dir, "rows_k%d" % k)
    paths, counts, _ = write_rows_files(d, k, nbytes / (1 << 30), threads)
    hk = C.pack_ranges([(p, 0, os.path.getsize(p)) for p in paths], threads=threads)
    shutil.rmtree(d, ignore_errors=True)
    kbytes = int(hk.off[-1])
    k_bytes = hk.data[:kbytes].to(dev)
    k_off = torch.from_numpy(hk.off.view(np.int64).copy()).to(dev)
    kn = len(paths)
    kcap = int(counts.shape[0]) + 1
    k_vals = torch.empty((kcap, nbins), dtype=torch.float64, device=dev)
    k_names = torch.empty((kcap, 2), dtype=torch.int32, device=dev)
    k_row0 = torch.empty(kn + 1, dtype=torch.int64, device=dev)
    k_status = torch.empty(4, dtype=torch.int64, device=dev)
    kneed = int(N.lib().kf_parse_kf_floats_scratch_bytes(kbytes, kn, kcap))
    kscratch = torch.empty(kneed // 8, dtype=torch.int64, device=dev)

    def kf():
        N.check(N.lib().kf_parse_kf_floats(k_bytes.data_ptr(), k_off.data_ptr(), kn, kbytes, nbins, kcap, 1.0,
                                           k_vals.data_ptr(), 8, k_names.data_ptr(), k_row0.data_ptr(),
                                           k_status.data_ptr(), kscratch.data_ptr(), kneed, stream), "kf_parse_kf_floats")

    kf()
    torch.cuda.synchronize()
    assert k_status.cpu().tolist() == [0, 0, 0, 0]
    t = timed({"tsv": tsv, "tsv_map": lambda: tsv(d_map), "kf": kf, "probe": probe}, a.reps)
    med = {name: float(np.median(v)) for name, v in t.items()}
    res = {"n": n, "units": nu, "text_bytes": nbytes, "text_GiB": round(nbytes / (1 << 30), 3),
           "bytes_per_field": round(nbytes / (n * n), 2), "kf_k": k, "kf_rows": int(counts.shape[0]),
           "kf_text_bytes": kbytes, "kf_bytes_per_field": round(kbytes / (counts.shape[0] * nbins), 2)}
    for name in t:
        res[name + "_ms"] = round(med[name], 3)
        res[name + "_ms_min_max"] = [round(min(t[name]), 3), round(max(t[name]), 3)]
    res.update({"tsv_text_GBps": round(nbytes / med["tsv"] / 1e6, 1), "kf_text_GBps": round(kbytes / med["kf"] / 1e6, 1),
                "probe_GBps": round(nbytes / med["probe"] / 1e6, 1),
                "tsv_vs_kf_per_byte": round((med["tsv"] / nbytes) / (med["kf"] / kbytes), 2),
                "tsv_map_vs_kf_per_byte": round((med["tsv_map"] / nbytes) / (med["kf"] / kbytes), 2),
                "tsv_map_vs_identity": round(med["tsv_map"] / med["tsv"], 2),
                "fields_per_us": round(n * n / med["tsv"] / 1e3, 1), "equal": equal})
    return res


def e2e_leg(a, path: str, names, m, dev) -> dict:
    import numpy as np
    import pandas as pd
    import torch
    from kf2vecfsw_amd import tables as T
    order = [names[i] for i in np.random.default_rng(2).permutation(a.n)]
    at = {nm: i for i, nm in enumerate(names)}
    perm = [at[x] for x in order]
    text_bytes = os.path.getsize(path)

    def new():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        t = T.true_distances(path, order, dev)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, t

    def base():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        df = pd.read_csv(path, sep="\t", header=0, index_col=0)          # read_true_dist_mtrx
        t1 = time.perf_counter()
        ddf = df.reindex(index=order)                                    # sort_df
        if len(ddf.columns) > 1:
            ddf = ddf.reindex(columns=order)
        vals = torch.from_numpy(ddf.to_numpy()).to(dev)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, t1 - t0, vals

    _, t = new()
    want = torch.from_numpy(m[np.ix_(perm, perm)]).to(dev)
    same = t.row_names == order and t.col_names == order and bool(torch.equal(t.values, want))
    del t
    tn, tb, tr, rel = [], [], [], None
    for r in range(a.e2e_reps):
        dt, t = new()
        tn.append(dt)
        del t
        dt, dr, vals = base()
        if r == 0:       # pandas' default parser is not correctly rounded: how far it is from the rounded value
            nz = want != 0
            rel = float(((vals - want).abs()[nz] / want[nz]).max())
            differ = int((vals != want).sum())
        del vals
        tb.append(dt)
        tr.append(dr)
    return {"n": a.n, "text_bytes": text_bytes, "text_GiB": round(text_bytes / (1 << 30), 3),
            "baseline": "pd.read_csv(sep='\\t', header=0, index_col=0) + sort_df's reindex calls, one process", "equal": same,
            "pandas_entries_that_differ": differ, "pandas_max_rel_diff": rel,
            "pandas_s": [round(x, 3) for x in tb], "pandas_read_s": [round(x, 3) for x in tr],
            "new_s": [round(x, 3) for x in tn], "new_text_GBps": round(text_bytes / min(tn) / 1e9, 2),
            "speedup_best_over_best": round(min(tb) / min(tn), 1)}


def commit_id() -> str | None:
    try:
        out = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True)
        return out.stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        return None


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--e2e-reps", type=int, default=3)
    ap.add_argument("--commit", default=None, help="the commit measured (default: git rev-parse HEAD, if this is a checkout)")
    ap.add_argument("--dir", default="/dev/shm/tsv_bench")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19", "tsv_floats.json"))
    a = ap.parse_args()
    import torch
    from kf2vecfsw_amd import _native as N
    threads = min(16, os.cpu_count() or 1)
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "commit": a.commit or commit_id(), "build_id": N.build_id(),
           "n": a.n, "reps": a.reps}
    shutil.rmtree(a.dir, ignore_errors=True)
    os.makedirs(a.dir)
    try:
        path = os.path.join(a.dir, "bench_full.di_mtrx")
        names, m = write_matrix(path, a.n)
        res["kernel"] = kernel_legs(a, path, m, dev, threads)
        torch.cuda.empty_cache()
        res["e2e"] = e2e_leg(a, path, names, m, dev)
        res["tsv_vs_kf_per_byte"] = res["kernel"]["tsv_vs_kf_per_byte"]
        res["speedup_over_pandas"] = res["e2e"]["speedup_best_over_best"]
    finally:
        shutil.rmtree(a.dir, ignore_errors=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
