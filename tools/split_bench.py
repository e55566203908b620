"""get_frequencies on one large FASTQ file, counted whole (-split_gb 0: one
batch, one pinned slot and one device block of the file's size) against counted
in pieces (-split_gb S: kf_rows_accumulate sums the pieces' rows), and
kf_rows_accumulate alone beside kf_stream_probe over the same bytes.

    python tools/split_bench.py            # writes profiles/r07/split_file.json

The file (150-base reads, synthetic) is written to --dir (/dev/shm by default);
--gib sets its size: both runs must fit in pinned and device memory.

cli.<k>.<run>.wall_s       wall clock of main(["get_frequencies", ...]) (median; the
                           runs take turns, the first of each kind is a warm-up);
                           split_S_batch_S also passes -batch_gb S
cli.<k>.<run>.pinned_slot_bytes   slots x bytes of the pinned input slots
cli.<k>.<run>.batches      batches the run made (from its KF_TRACE line; its
                           index_paths are the process's counts so far, not the run's)
rows_accumulate_ms         kf_rows_accumulate(64 rows -> 1) at k = 11, per call (events
                           around 20 calls, median of 11 windows)
stream_probe_ms            kf_stream_probe over the same 64 rows, likewise
"""
from __future__ import annotations

import argparse
import contextlib
import io
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def write_big_fastq(path: str, nbytes: int, block_mb: int = 128) -> int:
    """A four-line FASTQ file of about nbytes: one block of synthetic reads
    (fastq_index_bench.write_fastq) repeated."""
    from fastq_index_bench import write_fastq
    blk = path + ".blk"
    write_fastq(blk, block_mb << 20, 4242)
    with open(blk, "rb") as f:
        b = f.read()
    os.remove(blk)
    n = max(1, nbytes // len(b))
    with open(path, "wb") as f:
        for _ in range(n):
            f.write(b)
    return n * len(b)


def cli_run(Mn, inp: str, out: str, k: int, split_gb: float, batch_gb: float | None) -> dict:
    for f in os.listdir(out):
        os.remove(os.path.join(out, f))
    err = io.StringIO()
    os.environ["KF_TRACE"] = "1"
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(err):
        Mn.main(["get_frequencies", "-input_dir", inp, "-output_dir", out, "-k", str(k), "-raw_cnt",
                 "-split_gb", repr(split_gb)] + (["-batch_gb", repr(batch_gb)] if batch_gb else []))
    wall = time.perf_counter() - t0
    tr = [json.loads(ln) for ln in err.getvalue().splitlines() if ln.startswith('{"kf_trace"')][-1]
    stage = {}
    for ev in tr["kf_trace"]:
        if ev[0] in ("read", "write", "got"):
            stage[ev[0]] = round(stage.get(ev[0], 0.0) + ev[3] - ev[2], 1)
        if ev[0] == "gpu":
            for name, (a, b) in ev[3].items():
                stage[name] = round(stage.get(name, 0.0) + b - a, 1)
    return {"wall_s": wall, "pinned_slot_bytes": tr["pinned_slots"][0] * tr["pinned_slots"][1],
            "batches": sum(1 for ev in tr["kf_trace"] if ev[0] == "issue"), "stage_ms_summed": stage,
            "index_paths": tr["index_paths"]}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=2.0)
    ap.add_argument("--dir", default="/dev/shm")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--splits", type=float, nargs="*", default=[1.0, 0.25])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07", "split_file.json"))
    a = ap.parse_args()

    import numpy as np
    import torch
    from kf2vecfsw_amd import _native as N
    from kf2vecfsw_amd import counter as C
    from kf2vecfsw_amd import main as Mn

    dev = torch.device("cuda:0")
    med = lambda xs: round(float(np.median(xs)), 3)   # noqa: E731
    out = {"device": torch.cuda.get_device_name(dev), "host_threads": Mn.host_threads(os.cpu_count() or 1), "cli": {}}
    with tempfile.TemporaryDirectory(dir=a.dir) as tmp:
        inp, outd = os.path.join(tmp, "in"), os.path.join(tmp, "out")
        os.makedirs(inp)
        os.makedirs(outd)
        out["file_bytes"] = write_big_fastq(os.path.join(inp, "reads.fq"), int(a.gib * (1 << 30)))
        configs = [("whole", 0.0, None)] + [(f"split_{s:g}", s, None) for s in a.splits] + \
            [(f"split_{s:g}_batch_{s:g}", s, s) for s in a.splits[-1:]]
        for k in (7, 11):
            runs: dict = {name: [] for name, _, _ in configs}
            kf = {}
            for rep in range(a.reps + 1):          # the configurations take turns; the first round is a warm-up
                for name, s, b in configs:
                    runs[name].append(cli_run(Mn, inp, outd, k, s, b))
                    if rep == 0:
                        with open(os.path.join(outd, "reads.kf"), "rb") as f:
                            kf[name] = f.read()
            res = {name: dict(r[-1], wall_s=med([x["wall_s"] for x in r[1:]]),
                              wall_s_runs=[round(x["wall_s"], 3) for x in r]) for name, r in runs.items()}
            res["kf_equal"] = all(v == kf["whole"] for v in kf.values())
            out["cli"][f"k{k}"] = res
            torch.cuda.empty_cache()

    # kf_rows_accumulate alone: 64 rows of k = 11 into one, beside the read ceiling over the same bytes
    nbins, n_src = C.num_bins(11), 64
    src = torch.randint(0, 1 << 20, (n_src, nbins), dtype=torch.int32, device=dev)
    tot = torch.ones(n_src, dtype=torch.int64, device=dev)
    seg = torch.tensor([0, n_src], dtype=torch.int32, device=dev)
    dst = torch.zeros((1, nbins), dtype=torch.int32, device=dev)
    dt, st = torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    fold = torch.zeros(1, dtype=torch.int32, device=dev)
    s = torch.cuda.current_stream(dev).cuda_stream
    nbytes = src.numel() * 4

    def timed(fn, calls=20):
        """ms per call: events around `calls` calls, 11 windows after two warm-ups."""
        ms = []
        for r in range(13):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            if r >= 2:
                ms.append(e0.elapsed_time(e1) / calls)
        return ms

    acc_ms = timed(lambda: C.accumulate_rows(src, tot, seg, dst, dt, st))
    same = bool(torch.equal(dst[0].to(torch.int64), src.to(torch.int64).sum(dim=0)) and st.item() == 0
                and dt.item() == n_src)
    probe_ms = timed(lambda: N.check(N.lib().kf_stream_probe(src.data_ptr(), nbytes, fold.data_ptr(), s),
                                     "kf_stream_probe"))
    out.update({"rows": n_src, "rows_bytes": nbytes, "rows_accumulate_ms": med(acc_ms),
                "rows_accumulate_ms_min": round(min(acc_ms), 3), "rows_accumulate_GBs": round(nbytes / med(acc_ms) / 1e6, 1),
                "stream_probe_ms": med(probe_ms), "stream_probe_GBs": round(nbytes / med(probe_ms) / 1e6, 1),
                "rows_sum_equals_torch": same})
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out) + "\n")
    print(json.dumps(out))
    if not same or not all(v["kf_equal"] for v in out["cli"].values()):
        sys.exit("split and whole runs differ, or kf_rows_accumulate differs from the sum")


if __name__ == "__main__":
    main()
