"""The sorted merge of two (key, count) lists measured against the sort-based
path it replaces in get_kmers' piece loop.

    python tools/sparse_merge_bench.py [--log2-n 26] [--reps 10] [--out FILE.json]

Two lists of 2^log2-n keys each with u32 counts on the device, at 0 %, 50 % and
100 % shared keys (entry i of A is 4 i + {0, 1}, of B the same key if shared,
else 4 i + 2 + {0, 1}: strictly ascending, interleaved entry by entry).  Per
share, in one process: counter.merge_sorted (kf_sparse_merge) and
main._merge_sorted_counts (torch.cat, sort, unique_consecutive, index_add_: what
the piece loop ran before) on the same inputs, device events, 3 warm-ups, then
the two take turns for --reps timed repetitions; medians, and the spread
(min, max).  Each path's rise of torch.cuda.max_memory_allocated over one call
from an emptied cache.  The two results are compared entry by entry.
  new_ms / old_ms / ratio (new over old)
  new_rise_MB / old_rise_MB / bound_MB (16 (n_a + n_b) + scratch + 1 MiB)
  new_TBps   the HBM bytes kf_sparse_merge moves over new_ms: the keys three times
             (order check, count, scatter), the u32 counts once, 16 B per output
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
    ap.add_argument("--log2-n", type=int, default=26)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shares", default="0,50,100")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from kf2vecfsw_amd import counter as C
    from kf2vecfsw_amd import main as M
    dev = torch.device("cuda:0")
    n = 1 << a.log2_n
    res = {"n_a": n, "n_b": n, "reps": a.reps, "device": torch.cuda.get_device_name(0), "shares": {}}
    for share in [int(x) for x in a.shares.split(",")]:
        g = torch.Generator(device=dev).manual_seed(share)
        i4 = 4 * torch.arange(n, dtype=torch.int64, device=dev)
        ka = i4 + torch.randint(0, 2, (n,), dtype=torch.int64, device=dev, generator=g)
        same = torch.rand(n, device=dev, generator=g) * 100 < share
        kb = torch.where(same, ka, i4 + 2 + torch.randint(0, 2, (n,), dtype=torch.int64, device=dev, generator=g))
        ca = torch.randint(1, 1000, (n,), dtype=torch.int32, device=dev, generator=g)
        cb = torch.randint(1, 1000, (n,), dtype=torch.int32, device=dev, generator=g)
        n_same = int(same.sum())
        del i4, same

        def new():
            return C.merge_sorted(ka, ca, kb, cb)

        def old():
            return M._merge_sorted_counts([(ka, ca), (kb, cb)])

        def rise(f):
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats(dev)
            before = torch.cuda.memory_allocated(dev)
            r = f()
            torch.cuda.synchronize()
            up = torch.cuda.max_memory_allocated(dev) - before
            return r, up

        (k_, c_, n_out, status), new_rise = rise(new)
        m = C.merged_to_host(n_out, status)
        (hk, hc), old_rise = rise(old)
        equal = m == hk.numel() == 2 * n - n_same and bool((k_[:m] == hk).all()) and bool((c_[:m] == hc).all())
        del k_, c_, hk, hc
        tn, to = [], []
        for r in range(3 + a.reps):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            e[0].record()
            x = new()
            e[1].record()
            del x
            e[2].record()
            y = old()
            e[3].record()
            del y
            torch.cuda.synchronize()
            if r >= 3:
                tn.append(e[0].elapsed_time(e[1]))
                to.append(e[2].elapsed_time(e[3]))
        new_ms, old_ms = float(np.median(tn)), float(np.median(to))
        moved = 2 * n * (3 * 8 + 4) + 16 * m
        bound = 16 * 2 * n + C.merge_scratch_bytes(n, n) + (1 << 20)
        res["shares"][str(share)] = {
            "n_out": m, "equal": equal,
            "new_ms": round(new_ms, 3), "new_ms_min_max": [round(min(tn), 3), round(max(tn), 3)],
            "old_ms": round(old_ms, 3), "old_ms_min_max": [round(min(to), 3), round(max(to), 3)],
            "ratio": round(new_ms / old_ms, 4),
            "new_rise_MB": round(new_rise / 1e6, 1), "old_rise_MB": round(old_rise / 1e6, 1),
            "bound_MB": round(bound / 1e6, 1), "within_bound": new_rise <= bound,
            "new_moved_MB": round(moved / 1e6, 1), "new_TBps": round(moved / new_ms / 1e9, 3)}
        del ka, kb, ca, cb
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
