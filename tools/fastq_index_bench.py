"""Host against device FASTQ record index on one all-FASTQ batch of 150-base
reads (synthetic, written to a temporary directory: 16 files of 64 MiB by
default), and the k = 7 count over the device's pairs beside them.

    python tools/fastq_index_bench.py            # writes profiles/r07/fastq_index.json

host_index_ms   the index portion of pack_files(index=True) as the CLI runs it:
                kf_index_records per file on the CLI's host threads (wall clock,
                median), the files already in memory
device_index_ms events around kf_index_fastq with tables of the sizes to_device
                starts from (median after warm-up)
to_device_index_ms  index_fastq_on_device as to_device calls it: allocation,
                the launches and the read-back of counts and status (wall clock)
count_k7_ms     events around kf_count_batch at k = 7 over the device's pairs
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

READ = 150
HDR = 12   # "@r" + 10 digits


def write_fastq(path: str, nbytes: int, seed: int) -> int:
    """A four-line FASTQ file of 150-base reads, at most nbytes long."""
    import numpy as np
    rec = HDR + 1 + READ + 1 + 2 + READ + 1
    n = nbytes // rec
    rng = np.random.default_rng(seed)
    a = np.empty((n, rec), dtype=np.uint8)
    a[:, 0] = ord("@")
    a[:, 1] = ord("r")
    ids = np.arange(n, dtype=np.int64)
    for d in range(10):
        a[:, HDR - 1 - d] = ord("0") + (ids // 10 ** d) % 10
    a[:, HDR] = 10
    a[:, HDR + 1: HDR + 1 + READ] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=(n, READ), dtype=np.uint8)]
    p = HDR + 1 + READ
    a[:, p] = 10
    a[:, p + 1] = ord("+")
    a[:, p + 2] = 10
    a[:, p + 3: p + 3 + READ] = rng.integers(33, 74, size=(n, READ), dtype=np.uint8)
    a[:, rec - 1] = 10
    with open(path, "wb") as f:
        f.write(a.tobytes())
    return n


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=16)
    ap.add_argument("--file-mb", type=int, default=64)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07", "fastq_index.json"))
    a = ap.parse_args()
    from concurrent.futures import ThreadPoolExecutor

    import numpy as np
    import torch
    from kf2vecfsw_amd import _native as N
    from kf2vecfsw_amd import counter as C
    from kf2vecfsw_amd.main import host_threads

    dev = torch.device("cuda:0")
    threads = host_threads(os.cpu_count() or 1)   # the CLI's default -p, capped by the usable CPUs
    med = lambda xs: round(float(np.median(xs)), 3)   # noqa: E731
    with tempfile.TemporaryDirectory() as tmp:
        paths = [os.path.join(tmp, f"s{i:02d}.fq") for i in range(a.files)]
        reads = sum(write_fastq(p, a.file_mb << 20, 700 + i) for i, p in enumerate(paths))
        pool = ThreadPoolExecutor(max_workers=threads)
        t0 = time.perf_counter()
        hb = C.pack_files(paths, pool=pool, index=False)
        read_ms = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        ref = C.pack_files(paths, pool=pool, index=True)
        pack_index_ms = (time.perf_counter() - t0) * 1e3
    assert hb.excl is None and hb.fastq
    n, nbytes = hb.n, int(hb.off[-1])
    d = hb.data.numpy()

    # the host index alone, as pack_files maps it over its pool
    def host_index(i):
        lo, hi = int(hb.off[i]), int(hb.off[i + 1])
        return C.index_records(d[lo:hi], N.KF_FMT_FASTQ, lo)[0]

    host_ms = []
    for _ in range(3):
        t0 = time.perf_counter()
        list(pool.map(host_index, range(n)))
        host_ms.append((time.perf_counter() - t0) * 1e3)
    pool.shutdown()

    data = hb.data.to(dev)
    off = torch.from_numpy(hb.off.view(np.int64)).to(dev)
    L = N.lib()
    s = torch.cuda.current_stream(dev).cuda_stream
    cap_lines, cap_pairs = nbytes // 32 + 4 * n + 4096, nbytes // 128 + 2 * n + 4096   # to_device's first guesses
    need = int(L.kf_index_fastq_scratch_bytes(nbytes, n, cap_lines))
    scratch = torch.empty(need // 8, dtype=torch.int64, device=dev)
    excl = torch.empty(2 * cap_pairs, dtype=torch.int64, device=dev)
    info = torch.zeros(2 + (n + 1) // 2, dtype=torch.int64, device=dev)
    dev_ms = []
    for r in range(a.reps + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        N.check(L.kf_index_fastq(data.data_ptr(), off.data_ptr(), n, nbytes, excl.data_ptr(), cap_pairs, cap_lines,
                                 info.data_ptr(), info.data_ptr() + 16, scratch.data_ptr(), need, s), "kf_index_fastq")
        e1.record()
        torch.cuda.synchronize()
        if r >= 2:
            dev_ms.append(e0.elapsed_time(e1))
    h = info.cpu().numpy()
    m, lines = int(h[0]), int(h[1])
    assert m <= cap_pairs and lines <= cap_lines and not h[2:].any(), (m, lines)
    assert m == reads + n and lines == int(np.count_nonzero(d[:nbytes] == 10)), (m, lines)
    wall_ms = []
    for r in range(a.reps + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pairs, m2, regular = C.index_fastq_on_device(data, off, n, nbytes)
        if r >= 2:
            wall_ms.append((time.perf_counter() - t0) * 1e3)
    assert m2 == m and regular

    kc = C.KmerCounter(7, dev)
    db = C.DeviceBatch(data, off, pairs, n, m)
    counts, totals = kc.alloc_out(n)
    cnt_ms = []
    for r in range(a.reps + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        kc.count(db, counts, totals)
        e1.record()
        torch.cuda.synchronize()
        if r >= 2:
            cnt_ms.append(e0.elapsed_time(e1))
    # the same counts over the host's pairs
    ref_counts, ref_totals = kc.count(C.to_device(C.HostBatch(None, hb.off, ref.excl, hb.names, dev_data=data), dev))
    torch.cuda.synchronize()
    same = bool(torch.equal(counts, ref_counts) and torch.equal(totals, ref_totals))
    out = {"files": n, "file_MiB": a.file_mb, "batch_bytes": nbytes, "reads": reads, "read_len": READ,
           "pairs": m, "newlines": lines, "host_threads": threads,
           "read_files_ms": round(read_ms, 1), "pack_files_index_true_ms": round(pack_index_ms, 1),
           "host_index_ms": med(host_ms), "host_index_ms_all": [round(x, 1) for x in host_ms],
           "device_index_ms": med(dev_ms), "device_index_ms_min": round(min(dev_ms), 3),
           "device_index_GBs": round(nbytes / med(dev_ms) / 1e6, 1),
           "to_device_index_ms": med(wall_ms), "count_k7_ms": med(cnt_ms),
           "scratch_MB": round(need / 1e6, 1), "pair_table_MB": round(16 * cap_pairs / 1e6, 1),
           "counts_equal_host_index": same, "device": torch.cuda.get_device_name(dev)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out) + "\n")
    print(json.dumps(out))
    if not same:
        sys.exit("counts over the device's pairs differ from counts over the host's")


if __name__ == "__main__":
    main()
