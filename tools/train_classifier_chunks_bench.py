"""kf_chunk_features8 against kf_chunk_features, `train_classifier_chunks` end to
end, and the memory of the uint8 store.

    python tools/train_classifier_chunks_bench.py [--parts kernel train memory] [--genomes 1000] [--windows 500]
                                                  [--hidden 2048] [--batch 16] [--epochs 10] [--reps 10]
                                                  [--work-dir /dev/shm/kf_train_classifier_chunks_bench]
                                                  [--out profiles/r26/train_classifier_chunks.json]

kernel  a synthetic store at k = 7: --genomes genomes of --windows windows each,
        uint16 rows of 8192 columns with counts on both sides of 255 (1000 x 500:
        8.2 GB) and the uint8 rows kf_rows_cap8 makes of them (4.1 GB).  One
        epoch's draws as tools/chunk_features_bench.py makes them
        (chunks.draw_ranges, two views per genome: 2 x --genomes samples), at two
        sizes: the whole table in one call, and one default batch of 16 samples
        (the table's batches in turn, so that no call finds its rows in a cache
        because the call before read them).  kf_chunk_features8 on the uint8
        rows against kf_chunk_features with cap = 255 on the uint16 rows, float32
        out, tables on the device; in one process, device events (around all
        batches of the table at the small size), 3 warm-ups, --reps repetitions
        in which the two and their two read probes take turns; medians and
        (min, max).  kf_stream_probe over as many bytes as each kernel's samples
        cover gives the practical read rate; *_fraction_of_probe is the kernel's
        bytes per second over the probe's.  equal: the two results are the same
        bits.  Also kf_rows_cap8 over the whole store.
train   a synthetic library in --work-dir (--train-genomes get_chunks `.kf` files
        of k = 7 with 5 to 12 windows each in 10 classes, their full-genome
        files): train_classifier_model_chunks_func as the command runs it, with
        -cap and without, for 1 epoch and for 1 + --epochs epochs (the four take
        turns, --turns times; medians), the steps of
        the --epochs epochs over the difference of the two times (reading the
        inputs, building the model and writing the outputs are in both);
        against a restatement of the reference's loop on the same device: per
        item the run drawn and its features built in numpy on the host
        (Dataset_chunks_1row), a copy per step, a numpy gather of the classes
        and a copy per step, loss.item() and a host accuracy per step, and
        model.to('cpu'), torch.save and model.to(device) at each improving
        epoch.
memory  torch's peak of allocated device memory while chunk_store_from_kf reads
        that library, with cap8 and without, over the bytes of the store it
        returns: with the default batch of 1 GiB of text, which holds this
        whole library, and with batches of 16 MiB, where the store and its
        parts outweigh a batch as they do in a library of many batches.
One JSON object with a key per part (also written to --out)."""
from __future__ import annotations

import argparse
import json
import os
import shutil
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from train_bench import median  # noqa: E402

WINDOW = 10000
CLASSES = 10


def bench_kernel(a, dev):
    import numpy as np
    import torch
    from kf2vecfsw_amd import _native as N
    from kf2vecfsw_amd import chunks as CH
    from kf2vecfsw_amd import counter as C
    nbins = C.num_bins(7)
    W = a.genomes * a.windows
    wide = torch.empty((W, nbins), dtype=torch.int16, device=dev)
    g = torch.Generator(device=dev).manual_seed(26)
    for r in range(0, W, 1 << 15):
        m = min(1 << 15, W - r)
        wide[r: r + m] = torch.randint(0, 600, (m, nbins), dtype=torch.int16, device=dev, generator=g)
    rows8 = C.rows_cap8(wide)
    row0 = np.arange(a.genomes + 1, dtype=np.int64) * a.windows
    lo, n = CH.draw_ranges(np.full(a.genomes, a.windows), np.random.RandomState(0))
    lo, n = (lo + row0[:-1, None]).reshape(-1), n.reshape(-1)
    ns = lo.size
    d_lo, d_n = torch.from_numpy(lo).to(dev), torch.from_numpy(n).to(dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    need = int(N.lib().kf_chunk_features_scratch_bytes(ns))
    work = torch.empty(need // 8, dtype=torch.int64, device=dev)
    probe_out = torch.zeros(1, dtype=torch.int32, device=dev)
    out8 = torch.empty((ns, nbins), dtype=torch.float32, device=dev)
    out16 = torch.empty((ns, nbins), dtype=torch.float32, device=dev)
    lib = N.lib()

    def stream():
        return torch.cuda.current_stream(dev).cuda_stream

    def k8(s0, s1):
        N.check(lib.kf_chunk_features8(rows8.data_ptr(), W, nbins, d_lo[s0:].data_ptr(), d_n[s0:].data_ptr(), s1 - s0, 1e4,
                                       out8[s0:].data_ptr(), 4, status.data_ptr(), work.data_ptr(), need, stream()),
                "kf_chunk_features8")

    def k16(s0, s1):
        N.check(lib.kf_chunk_features(wide.data_ptr(), 2, W, nbins, d_lo[s0:].data_ptr(), d_n[s0:].data_ptr(), s1 - s0,
                                      255, 1e4, out16[s0:].data_ptr(), 4, status.data_ptr(), work.data_ptr(), need,
                                      stream()), "kf_chunk_features")

    def probe(t, nbytes):
        N.check(lib.kf_stream_probe(t.data_ptr(), nbytes, probe_out.data_ptr(), stream()), "kf_stream_probe")

    def cap_rows():
        N.check(lib.kf_rows_cap8(wide.data_ptr(), W * nbins, rows8.data_ptr(), stream()), "kf_rows_cap8")

    result = {"k": 7, "nbins": nbins, "genomes": a.genomes, "windows": a.windows, "store_u16_GB": round(W * nbins * 2 / 1e9, 2),
              "store_u8_GB": round(W * nbins / 1e9, 2), "samples": ns, "rows_covered": int(n.sum()), "reps": a.reps}
    for name, per in (("epoch_{}".format(ns), ns), ("batch_16", 16)):
        calls = [(s, min(ns, s + per)) for s in range(0, ns, per)]
        covered = int(n.sum()) * nbins            # uint8 bytes the samples' rows cover; twice that in uint16
        cov8 = min(covered, W * nbins) // 16 * 16
        cov16 = min(2 * covered, 2 * W * nbins) // 16 * 16
        fns = (("u8", lambda: [k8(*c) for c in calls]), ("u16", lambda: [k16(*c) for c in calls]),
               ("probe_u8", lambda: probe(rows8, cov8)), ("probe_u16", lambda: probe(wide, cov16)))
        t = {k: [] for k, _ in fns}
        for r in range(3 + a.reps):
            for k, f in fns:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                f()
                e1.record()
                torch.cuda.synchronize()
                if r >= 3:
                    t[k].append(e0.elapsed_time(e1))
        assert int(status.item()) == 0
        med = {k: median(v) for k, v in t.items()}
        res = {"calls_per_timing": len(calls), "samples_per_call": per,
               "equal": bool(torch.equal(out8.view(torch.int32), out16.view(torch.int32)))}
        for k in t:
            res[k + "_ms"] = round(med[k], 4)
            res[k + "_ms_min_max"] = [round(min(t[k]), 4), round(max(t[k]), 4)]
        res["u8_us_per_call"] = round(med["u8"] / len(calls) * 1e3, 2)
        res["u16_us_per_call"] = round(med["u16"] / len(calls) * 1e3, 2)
        res["u16_over_u8"] = round(med["u16"] / med["u8"], 3)
        res["u8_TBps"] = round(covered / med["u8"] / 1e9, 3)
        res["u16_TBps"] = round(2 * covered / med["u16"] / 1e9, 3)
        res["probe_u8_TBps"] = round(cov8 / med["probe_u8"] / 1e9, 3)
        res["probe_u16_TBps"] = round(cov16 / med["probe_u16"] / 1e9, 3)
        res["u8_fraction_of_probe"] = round((covered / med["u8"]) / (cov8 / med["probe_u8"]), 3)
        res["u16_fraction_of_probe"] = round((2 * covered / med["u16"]) / (cov16 / med["probe_u16"]), 3)
        result[name] = res
        print(json.dumps({name: res}), flush=True)
    t = []
    for r in range(3 + a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        cap_rows()
        e1.record()
        torch.cuda.synchronize()
        if r >= 3:
            t.append(e0.elapsed_time(e1))
    result["rows_cap8"] = {"elements": W * nbins, "ms": round(median(t), 4), "ms_min_max": [round(min(t), 4), round(max(t), 4)],
                           "read_plus_write_TBps": round(3 * W * nbins / median(t) / 1e9, 3)}
    print(json.dumps({"rows_cap8": result["rows_cap8"]}), flush=True)
    return result


def make_library(a, work):
    """The synthetic library's files; returns the directories, the `.subtrees` path, the names, classes and window rows."""
    import numpy as np
    from kf2vecfsw_amd import chunks as CH
    from kf2vecfsw_amd import counter as C
    from kf2vecfsw_amd import main as M
    shutil.rmtree(work, ignore_errors=True)
    chunks, full = os.path.join(work, "chunks"), os.path.join(work, "full")
    for d in (chunks, full):
        os.makedirs(d)
    nbins = C.num_bins(7)
    rng = np.random.default_rng(26)
    names = ["G%07d" % i for i in range(a.train_genomes)]
    classes = [i % CLASSES for i in range(a.train_genomes)]
    base = [rng.dirichlet(np.full(nbins, 2.0)) for _ in range(CLASSES)]
    rows = []
    for nm, c in zip(names, classes):
        comp = 0.8 * base[c] + 0.2 * rng.dirichlet(np.full(nbins, 2.0))
        r = rng.multinomial(WINDOW - 6, comp, size=int(rng.integers(5, 13))).astype(np.uint16)
        rows.append(r)
        text, _ = CH.format_rows_host(r, [nm + ".part_c.part_c_sliding__"], np.zeros(r.shape[0], np.int64),
                                      np.arange(r.shape[0], dtype=np.int64) * WINDOW, WINDOW, False)
        with open(os.path.join(chunks, nm + ".kf"), "wb") as f:
            f.write(text)
    M.write_kf_files(full, names, np.stack([r.astype(np.uint32).sum(axis=0) for r in rows]).astype(np.uint32), False,
                     False, 16)
    sub = os.path.join(work, "synth.subtrees")
    with open(sub, "w") as f:
        f.write("genome clade\n" + "".join("{} {}\n".format(nm, c) for nm, c in zip(names, classes)))
    return chunks, full, sub, names, classes, rows


def reference_loop(a, dev, rows, classes, cap, out_dir, epochs):
    """train_classifier_model_chunks.py:354-497 restated on the device of this run; seconds for `epochs` epochs and the steps."""
    import numpy as np
    import torch
    from kf2vecfsw_amd import chunks as CH
    from kf2vecfsw_amd import classify as CL
    from kf2vecfsw_amd import train as TR
    from kf2vecfsw_amd import train_classifier as TCL
    os.makedirs(out_dir, exist_ok=True)
    if cap:
        rows = [np.minimum(r, 255).astype(np.uint8) for r in rows]           # my_read_csv_chunk_capped
    clade_input_sorted = np.asarray(classes, dtype=np.int64)
    input_size = rows[0].shape[1]
    torch.manual_seed(a.seed)
    model = CL.ClassifierNet(input_size, a.hidden, CLASSES).to(dev)
    criterion = torch.nn.NLLLoss()
    optimizer = torch.optim.Adam(model.parameters(), lr=a.lr)
    gen = torch.Generator().manual_seed(a.seed)
    rng = np.random.RandomState(a.seed)
    plan = TR.batch_plan(len(rows), a.batch)
    lowest, saves = float("inf"), 0
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()

    def item(g):                                              # Dataset_chunks_1row.__getitem__ (datasets.py:244-259)
        r = rows[g]
        lo, n = CH.draw_ranges([r.shape[0]], rng, views=1)
        c = r[int(lo[0, 0]): int(lo[0, 0]) + int(n[0, 0])].sum(axis=0, dtype=np.uint64).astype(np.float64)
        return np.nan_to_num(c / c.sum()) * 1e4

    for epoch in range(epochs):
        perm = torch.randperm(len(rows), generator=gen)
        train_loss, running_acc, items = 0.0, 0.0, 0
        for s, e in plan:
            labels = perm[s:e]
            images = torch.from_numpy(np.stack([item(int(g)) for g in labels])).reshape(-1, input_size).to(dev)
            true_class = torch.from_numpy(clade_input_sorted[np.ix_(list(labels))]).to(dev)
            model_class = torch.nn.functional.log_softmax(model(images.float()), dim=1)
            loss = criterion(model_class, true_class)
            train_loss += loss.item() * images.shape[0]
            items += images.shape[0]
            optimizer.zero_grad()
            loss.backward()
            optimizer.step()
            ps = torch.exp(model_class)
            _, top_class = ps.topk(1, dim=1)
            running_acc += float((true_class.to("cpu") == top_class.to("cpu")[:, 0]).double().mean()) * images.shape[0]
        train_loss /= items
        if train_loss < lowest:
            lowest = train_loss
            model.to("cpu")
            torch.save(TCL.checkpoint_state(input_size, a.hidden, CLASSES, model.state_dict()),
                       os.path.join(out_dir, "classifier_model.ckpt"))
            model.to(dev)
            saves += 1
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0, epochs * len(plan), saves, lowest


def bench_train(a, dev, lib):
    import glob
    import torch
    from kf2vecfsw_amd import train as TR
    from kf2vecfsw_amd import train_classifier_chunks as TCC
    work = a.work_dir
    chunks, full, sub, names, classes, rows = lib
    files = glob.glob(os.path.join(chunks, "*.kf"))
    order = {nm: i for i, nm in enumerate(names)}
    file_rows = [rows[order[os.path.basename(f)[:-3]]] for f in files]
    file_classes = [classes[order[os.path.basename(f)[:-3]]] for f in files]
    steps = a.epochs * len(TR.batch_plan(len(names), a.batch))
    out = {"genomes": len(names), "k": 7, "classes": CLASSES, "windows": int(sum(r.shape[0] for r in rows)),
           "hidden": a.hidden, "batch": a.batch, "epochs": a.epochs, "lr": a.lr, "steps": steps}

    def run(tag, epochs, cap):
        devnull = open(os.devnull, "w")
        stdout, sys.stdout = sys.stdout, devnull
        try:
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            kept = TCC.train_classifier_model_chunks_func(chunks, full, files, sub, epochs, a.hidden, a.batch, a.lr, 3e-6,
                                                          2000, a.seed, False, cap, os.path.join(work, tag), device=dev,
                                                          keep=True)
            torch.cuda.synchronize(dev)
            return time.perf_counter() - t0, kept
        finally:
            sys.stdout = stdout
            devnull.close()

    run("warm", 1, True)                                      # the library, pinned pools, the GEMMs' first calls
    run("warm", 1, False)
    ones, alls, last = {True: [], False: []}, {True: [], False: []}, {}
    for i in range(a.turns):                                  # the four take turns; medians
        for cap in (True, False):
            ones[cap].append(run("one", 1, cap)[0])
            t, last[cap] = run("out", 1 + a.epochs, cap)
            alls[cap].append(t)
    for cap in (True, False):
        kept = last[cap]
        per_turn = [steps / (b - o) for o, b in zip(ones[cap], alls[cap])]
        r = {"command_1_epoch_s": round(median(ones[cap]), 4), "command_s": round(median(alls[cap]), 4),
             "epochs_s": round(median(alls[cap]) - median(ones[cap]), 4),
             "steps_per_s": round(steps / (median(alls[cap]) - median(ones[cap])), 1),
             "steps_per_s_by_turn": [round(v, 1) for v in per_turn],
             "first_and_lowest_loss": [kept["losses"][0], kept["lowest_loss"]]}
        reference_loop(a, dev, file_rows, file_classes, cap, os.path.join(work, "ref_warm"), 1)     # its warm-up: one epoch
        ref_s, ref_steps, saves, lowest = reference_loop(a, dev, file_rows, file_classes, cap, os.path.join(work, "ref"),
                                                         a.epochs)
        r.update({"reference_loop_s": round(ref_s, 4), "reference_loop_steps_per_s": round(ref_steps / ref_s, 1),
                  "reference_loop_checkpoints": saves, "reference_loop_lowest_loss": lowest})
        r["speedup"] = round(r["steps_per_s"] / r["reference_loop_steps_per_s"], 2)
        out["cap" if cap else "no_cap"] = r
        print(json.dumps({"train": {"cap" if cap else "no_cap": r}}), flush=True)
    return out


def bench_memory(a, dev, lib):
    import torch
    from kf2vecfsw_amd import chunks as CH
    chunks, _, _, names, _, rows = lib
    out = {"genomes": len(names), "windows": int(sum(r.shape[0] for r in rows))}
    CH.chunk_store_from_kf(chunks, 7, dev, samples=names[:8])               # the library and the pinned buffers' first use
    # the default batch (1 GiB of text: this whole library is one batch, and the batch outweighs the store), and
    # batches of 16 MiB, where the store and its parts outweigh the batch as they do in a library of many batches
    for tag, batch_gb in (("batch_1GiB", 1.0), ("batch_16MiB", 1.0 / 64)):
        res = {}
        for cap8 in (False, True):
            torch.cuda.synchronize(dev)
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats(dev)
            before = torch.cuda.memory_allocated(dev)
            store = CH.chunk_store_from_kf(chunks, 7, dev, samples=names, batch_gb=batch_gb, cap8=cap8)
            torch.cuda.synchronize(dev)
            peak = torch.cuda.max_memory_allocated(dev) - before
            size = store.counts.numel() * store.counts.element_size()
            res["cap8" if cap8 else "uint16"] = {"store_bytes": size, "peak_allocated_bytes": int(peak),
                                                "peak_over_store": round(peak / size, 3)}
            del store
        res["peak_cap8_over_uint16"] = round(res["cap8"]["peak_allocated_bytes"] / res["uint16"]["peak_allocated_bytes"], 3)
        out[tag] = res
    print(json.dumps({"memory": out}), flush=True)
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", nargs="+", default=["kernel", "train", "memory"], choices=["kernel", "train", "memory"])
    ap.add_argument("--genomes", type=int, default=1000)
    ap.add_argument("--windows", type=int, default=500)
    ap.add_argument("--train-genomes", type=int, default=1000)
    ap.add_argument("--hidden", type=int, default=2048)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--turns", type=int, default=3)
    ap.add_argument("--lr", type=float, default=1e-5)
    ap.add_argument("--seed", type=int, default=28)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--work-dir", default="/dev/shm/kf_train_classifier_chunks_bench")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda:0")
    result = {"device": torch.cuda.get_device_name(0)}
    if "kernel" in a.parts:
        result["kernel"] = bench_kernel(a, dev)
        torch.cuda.empty_cache()
    if "train" in a.parts or "memory" in a.parts:
        t0 = time.perf_counter()
        lib = make_library(a, a.work_dir)
        result["make_library_s"] = round(time.perf_counter() - t0, 2)
        if "train" in a.parts:
            result["train"] = bench_train(a, dev, lib)
        if "memory" in a.parts:
            result["memory"] = bench_memory(a, dev, lib)
        shutil.rmtree(a.work_dir, ignore_errors=True)
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
