"""kf_chunk_features measured at the chunk trainer's shape, against the HBM read
rate and against a torch statement of the same result.

    python tools/chunk_features_bench.py [--k 7] [--genomes 1000] [--windows 500] [--reps 10] [--out FILE.json]

A synthetic store at k=7: --genomes genomes of --windows windows each, random
uint16 rows of 8192 columns on the device (1000 x 500: 8.2 GB).  --k 8 has
32,896 columns (the kernel's two-launch regime, 32.9 GB), --k 6 has 2,080.
One epoch's draws: chunks.draw_ranges for every genome (two views each,
RandomState(0)), offset into the store, as ChunkStore.batch makes them -- 2 x
genomes samples in one call.  In one process, device events, 3 warm-ups, then
--reps timed repetitions in which the four take turns; medians and (min, max):
  kernel_ms   kf_chunk_features enqueued on tables already on the device
              (float32 out, scaler 1e4, no cap); kernel_TBps = the bytes the
              samples' rows cover over it
  call_ms     counter.chunk_features from host tables: upload, kernel, status
              read-back (what ChunkStore.batch pays per batch)
  probe_ms    kf_stream_probe over as many bytes of the store: the practical
              read ceiling; fraction_of_probe = probe_ms / kernel_ms
  torch_ms    the torch statement: per sample, its slice of rows widened and
              summed (torch.sum), then the float64 arithmetic on all samples
              (divide by the row total, NaN to 0, scale, to float32)
  torch_spread_ms = max - min of torch_ms: the margin allowed to the kernel
  not_slower  kernel_ms <= torch_ms + torch_spread_ms
  equal       the two results are the same float32 bits
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=7)
    ap.add_argument("--genomes", type=int, default=1000)
    ap.add_argument("--windows", type=int, default=500)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from kf2vecfsw_amd import _native as N
    from kf2vecfsw_amd import chunks as CH
    from kf2vecfsw_amd import counter as C
    dev = torch.device("cuda:0")
    nbins = C.num_bins(a.k)
    W = a.genomes * a.windows
    counts = torch.empty((W, nbins), dtype=torch.int16, device=dev)
    g = torch.Generator(device=dev).manual_seed(7)
    for r in range(0, W, 1 << 15):
        m = min(1 << 15, W - r)
        counts[r: r + m] = torch.randint(-(1 << 15), 1 << 15, (m, nbins), dtype=torch.int16, device=dev, generator=g)
    row0 = np.arange(a.genomes + 1, dtype=np.int64) * a.windows
    lo, n = CH.draw_ranges(np.full(a.genomes, a.windows), np.random.RandomState(0))
    lo = (lo + row0[:-1, None]).reshape(-1)
    n = n.reshape(-1)
    ns = lo.size
    covered = int(n.sum()) * nbins * 2
    d_lo, d_n = torch.from_numpy(lo).to(dev), torch.from_numpy(n).to(dev)
    out = torch.empty((ns, nbins), dtype=torch.float32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    need = int(N.lib().kf_chunk_features_scratch_bytes(ns))
    work = torch.empty(need // 8, dtype=torch.int64, device=dev)
    probe_out = torch.zeros(1, dtype=torch.int32, device=dev)
    probe_bytes = min(covered, W * nbins * 2) // 16 * 16
    bounds = list(zip(lo.tolist(), (lo + n).tolist()))
    sums = torch.empty((ns, nbins), dtype=torch.int64, device=dev)

    def kernel():
        N.check(N.lib().kf_chunk_features(counts.data_ptr(), 2, W, nbins, d_lo.data_ptr(), d_n.data_ptr(), ns,
                                          0xFFFFFFFF, 1e4, out.data_ptr(), 4, status.data_ptr(), work.data_ptr(), need,
                                          torch.cuda.current_stream(dev).cuda_stream), "kf_chunk_features")

    def call():
        return C.chunk_features(counts, lo, n, 1e4, None, torch.float32, out=out)

    def probe():
        N.check(N.lib().kf_stream_probe(counts.data_ptr(), probe_bytes, probe_out.data_ptr(),
                                        torch.cuda.current_stream(dev).cuda_stream), "kf_stream_probe")

    def torch_statement():
        for s, (r0, r1) in enumerate(bounds):
            torch.sum(counts[r0: r1].to(torch.int32) & 0xFFFF, dim=0, out=sums[s])
        v = sums.to(torch.float64)
        return (torch.nan_to_num(v / v.sum(dim=1, keepdim=True), nan=0.0, posinf=0.0, neginf=0.0) * 1e4).to(torch.float32)

    kernel()
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    equal = bool(torch.equal(out.view(torch.int32), torch_statement().view(torch.int32)))
    t = {"kernel": [], "call": [], "probe": [], "torch": []}
    for r in range(3 + a.reps):
        for name, f in (("kernel", kernel), ("call", call), ("probe", probe), ("torch", torch_statement)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            x = f()
            e1.record()
            torch.cuda.synchronize()
            del x
            if r >= 3:
                t[name].append(e0.elapsed_time(e1))
    med = {k: float(np.median(v)) for k, v in t.items()}
    spread = max(t["torch"]) - min(t["torch"])
    res = {"device": torch.cuda.get_device_name(0), "k": a.k, "nbins": nbins, "genomes": a.genomes, "windows": a.windows,
           "store_GB": round(W * nbins * 2 / 1e9, 2), "samples": ns, "rows_covered": int(n.sum()),
           "covered_GB": round(covered / 1e9, 3), "reps": a.reps, "equal": equal}
    for k in t:
        res[k + "_ms"] = round(med[k], 3)
        res[k + "_ms_min_max"] = [round(min(t[k]), 3), round(max(t[k]), 3)]
    res.update({"kernel_TBps": round(covered / med["kernel"] / 1e9, 3),
                "probe_TBps": round(probe_bytes / med["probe"] / 1e9, 3),
                "fraction_of_probe": round(med["probe"] / med["kernel"] * covered / probe_bytes, 3),
                "torch_spread_ms": round(spread, 3), "ratio_kernel_over_torch": round(med["kernel"] / med["torch"], 4),
                "not_slower": med["kernel"] <= med["torch"] + spread})
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
