"""kf_format_kf_rows16 alone, on one count launch's worth of get_chunks rows,
against a device copy of the text it writes.

    python tools/kf_format_bench.py [--k 3 7 10] [--rows 4096] [--reps 10] [--out-dir DIR]

Rows: uint16 counts of 10 kbp windows (Poisson with mean 10,000 / bins, seeded),
min(--rows, 1 GiB / (4 x bins)) of them, as get_chunks sizes a launch; names as
get_chunks builds them (a contig prefix per 100 windows).  In one process, device
events, 3 warm-ups, then --reps timed repetitions in which the two take turns;
medians and (min, max):
  kernel_ms  the launches of kf_format_kf_rows16 (rows, tables and text resident)
  copy_ms    a device-to-device copy of the same text bytes
  kernel_over_copy = kernel_ms / copy_ms
  text_GBps  the text written over kernel_ms
  equal      the first and last 64 rows equal chunks.format_rows_host byte for byte
One JSON line per k (also written to --out-dir/kf_format_k<k>.json)."""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, nargs="+", default=[3, 7, 10])
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--pseudocount", action="store_true")
    ap.add_argument("--out-dir", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from kf2vecfsw_amd import _native as N
    from kf2vecfsw_amd import chunks as CH
    from kf2vecfsw_amd import counter as C
    dev = torch.device("cuda:0")
    for k in a.k:
        nbins = C.num_bins(k)
        n = max(1, min(a.rows, (1 << 30) // (4 * nbins)))
        rng = np.random.default_rng(50 + k)
        rows = rng.poisson(CH.CHUNK_SZ / nbins, size=(n, nbins)).astype(np.uint16)
        pre = [b"B%04d.part_contig_%d.part_contig_%d_sliding__" % (g, g, g) for g in range((n + 99) // 100)]
        rpre = (np.arange(n) // 100).astype(np.uint32)
        rpos = ((np.arange(n) % 100) * 9900).astype(np.uint64)
        d_rows = torch.from_numpy(rows.view(np.int16)).to(dev)
        d_pre = torch.from_numpy(np.frombuffer(b"".join(pre), dtype=np.uint8).copy()).to(dev)
        d_pre_off = torch.from_numpy(np.cumsum([0] + [len(p) for p in pre]).astype(np.int64)).to(dev)
        d_rpre = torch.from_numpy(rpre.view(np.int32)).to(dev)
        d_rpos = torch.from_numpy(rpos.view(np.int64)).to(dev)
        cap = n * C.format_kf_row_bound(nbins, max(len(p) for p in pre), CH.CHUNK_SZ)
        assert cap <= C.KF_FORMAT_MAX_CAP
        text = torch.empty(cap, dtype=torch.uint8, device=dev)
        row_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        status = torch.empty(4, dtype=torch.int64, device=dev)
        need = int(N.lib().kf_format_kf_scratch_bytes(n, nbins))
        scratch = torch.empty(need // 8 + 1, dtype=torch.int64, device=dev)

        def kernel():
            N.check(N.lib().kf_format_kf_rows16(d_rows.data_ptr(), n, nbins, d_pre.data_ptr(), d_pre_off.data_ptr(),
                                                len(pre), d_rpre.data_ptr(), d_rpos.data_ptr(), CH.CHUNK_SZ,
                                                int(a.pseudocount), text.data_ptr(), cap, row_off.data_ptr(),
                                                status.data_ptr(), scratch.data_ptr(), need,
                                                torch.cuda.current_stream(dev).cuda_stream), "kf_format_kf_rows16")

        kernel()
        off = C.formatted_to_host(row_off, status, cap)
        total = int(off[-1])
        equal = True
        for lo, hi in ((0, min(64, n)), (max(0, n - 64), n)):
            exp, eoff = CH.format_rows_host(rows[lo:hi], pre, rpre[lo:hi], rpos[lo:hi], CH.CHUNK_SZ, a.pseudocount)
            got = text[int(off[lo]): int(off[hi])].cpu().numpy().tobytes()
            equal = equal and got == exp and (off[lo: hi + 1] - off[lo]).tolist() == eoff.tolist()
        dst = torch.empty(total, dtype=torch.uint8, device=dev)

        def copy():
            dst.copy_(text[:total], non_blocking=True)

        t = {"kernel": [], "copy": []}
        for r in range(3 + a.reps):
            for name, f in (("kernel", kernel), ("copy", copy)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                f()
                e1.record()
                torch.cuda.synchronize()
                if r >= 3:
                    t[name].append(e0.elapsed_time(e1))
        med = {x: float(np.median(v)) for x, v in t.items()}
        res = {"device": torch.cuda.get_device_name(0), "k": k, "nbins": nbins, "rows": n, "cells": n * nbins,
               "pseudocount": bool(a.pseudocount), "counts_bytes": 2 * n * nbins, "text_bytes": total,
               "bytes_per_cell": round(total / (n * nbins), 2), "reps": a.reps}
        for x in t:
            res[x + "_ms"] = round(med[x], 4)
            res[x + "_ms_min_max"] = [round(min(t[x]), 4), round(max(t[x]), 4)]
        res.update({"kernel_over_copy": round(med["kernel"] / med["copy"], 2),
                    "text_GBps": round(total / med["kernel"] / 1e6, 1),
                    "copy_GBps": round(total / med["copy"] / 1e6, 1), "equal": equal})
        if a.out_dir:
            os.makedirs(a.out_dir, exist_ok=True)
            with open(os.path.join(a.out_dir, "kf_format_k{}.json".format(k)), "w") as f:
                f.write(json.dumps(res, indent=1) + "\n")
        print(json.dumps(res), flush=True)
        del d_rows, text, dst, scratch
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
