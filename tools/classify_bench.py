"""kf_class_probs alone and `classify` end to end.

    python tools/classify_bench.py [--parts kernel classify] [--queries 4000] [--classes 64] [--hidden 2048]
                                   [--reps 20] [--inner 50] [--work-dir /dev/shm/kf_classify_bench] [--out FILE]

kernel    kf_class_probs at Q = --queries and C in (16, 256, 4096) against the
          torch lines it replaces on the same device -- torch.exp(F.log_softmax(x,
          dim=1)), topk(1) and the cat into the [Q, C + 1] layout -- in one
          process: device events around --inner calls, 3 warm-ups, --reps
          repetitions in which the two take turns, medians per call.  Both are
          launch-bound at these sizes; the ratio is reported whatever it is.
          Values: the kernel within its bound of classify.class_probs_host, and
          the classes of the two equal on the rows whose two largest
          probabilities differ.
classify  a synthetic k = 7 library (--queries `.kf` files of one row, a
          classifier of 8192 x --hidden x --classes) in --work-dir: classify_func
          with times= (seconds per stage, a synchronisation per stage, so that
          run does not overlap them) and once without, against the reference's
          lines on the CPU of the same machine (the files read into StringIO and
          pandas, the forward pass, exp, topk, np.hstack with the object column
          and csv.writer, restated here), and whether the two files agree in
          header, labels, classes and width.
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


def median(x):
    x = sorted(x)
    return x[len(x) // 2]


def timed(fn, other, reps, inner):
    """Medians (ms per call) of fn and other, `inner` calls between two events, taking turns, after 3 warm-ups."""
    import torch
    a, b = [], []
    for i in range(3 + reps):
        for f, into in ((fn, a), (other, b)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                f()
            e1.record()
            e1.synchronize()
            if i >= 3:
                into.append(e0.elapsed_time(e1) / inner)
    return median(a), (min(a), max(a)), median(b), (min(b), max(b))


def bench_kernel(a, dev):
    import numpy as np
    import torch
    import torch.nn.functional as F
    from kf2vecfsw_amd import _native as N
    from kf2vecfsw_amd import classify as CL
    out = {}
    gen = torch.Generator(device=dev).manual_seed(21)
    q = a.queries
    s = torch.cuda.current_stream(dev).cuda_stream
    for c in (16, 256, 4096):
        x = torch.randn((q, c), generator=gen, device=dev, dtype=torch.float32) * 4.0
        o = torch.empty((q, c + 1), dtype=torch.float32, device=dev)
        t = torch.empty(q, dtype=torch.int32, device=dev)

        def kernel():
            N.check(N.lib().kf_class_probs(x.data_ptr(), q, c, o.data_ptr(), t.data_ptr(), s))

        ref = {}

        def torch_lines():
            ps = torch.exp(F.log_softmax(x, dim=1))
            top_p, top_class = ps.topk(1, dim=1)
            ref["out"], ref["top"] = torch.cat([top_p, ps], dim=1), top_class

        k_ms, k_rng, t_ms, t_rng = timed(kernel, torch_lines, a.reps, a.inner)
        h, ht = CL.class_probs_host(x.cpu().numpy())
        got, gt = o.cpu().numpy(), t.cpu().numpy()
        x64 = x.cpu().numpy().astype(np.float64)
        tt = np.abs(x64 - x64.max(axis=1, keepdims=True))
        bound = (tt + c + 8) * 2.0 ** -24 * h[:, 1:] + 2.0 ** -126
        used = float((np.abs(got[:, 1:].astype(np.float64) - h[:, 1:]) / bound).max())
        rt = ref["top"].cpu().numpy()[:, 0]
        srt = np.sort(h[:, 1:], axis=1)
        clear = srt[:, -1] > srt[:, -2] * (1 + 1e-5) if c > 1 else np.ones(q, bool)
        moved = q * c * 4 + q * (c + 1) * 4 + q * 4
        out["C={}".format(c)] = dict(rows=q, cols=c, kernel_us=round(k_ms * 1e3, 2),
                                     kernel_us_range=[round(v * 1e3, 2) for v in k_rng],
                                     torch_us=round(t_ms * 1e3, 2), torch_us_range=[round(v * 1e3, 2) for v in t_rng],
                                     torch_over_kernel=round(t_ms / k_ms, 2), bytes_moved=moved,
                                     kernel_GBps=round(moved / k_ms / 1e6, 1), share_of_error_bound=round(used, 3),
                                     classes_equal_host=bool(np.array_equal(gt[clear], ht[clear])),
                                     classes_equal_torch=bool(np.array_equal(gt[clear], rt[clear])))
        print(json.dumps({"C={}".format(c): out["C={}".format(c)]}), flush=True)
    return out


def make_library(a, work):
    import numpy as np
    import torch
    from kf2vecfsw_amd import classify as CL
    from kf2vecfsw_amd import counter as C
    from kf2vecfsw_amd import main as M
    shutil.rmtree(work, ignore_errors=True)
    kf, model = os.path.join(work, "kf"), os.path.join(work, "model")
    os.makedirs(kf)
    os.makedirs(model)
    nbins = C.num_bins(7)
    rng = np.random.default_rng(24)
    names = ["Q%07d" % i for i in range(a.queries)]
    counts = rng.poisson(300, size=(a.queries, nbins)).astype(np.uint32)
    M.write_kf_files(kf, names, counts, False, False, 16)
    torch.manual_seed(25)
    net = CL.ClassifierNet(nbins, a.hidden, a.classes)
    torch.save({"model_input_size": nbins, "model_hidden_size_fc1": a.hidden, "model_class_count": a.classes,
                "state_dict": net.state_dict()}, os.path.join(model, "classifier_model.ckpt"))
    return kf, model, names


def reference_lines(kf, model, names, out_dir, block):
    """kf2vec/classify.py:83-124 on the CPU; seconds per stage."""
    import csv
    from io import StringIO
    import numpy as np
    import pandas as pd
    import torch
    import torch.nn.functional as F
    from kf2vecfsw_amd import classify as CL
    os.makedirs(out_dir, exist_ok=True)
    tm = dict(model=0.0, read=0.0, forward=0.0, hstack=0.0, write=0.0)
    t0 = time.perf_counter()
    state = torch.load(os.path.join(model, "classifier_model.ckpt"))
    net = CL.ClassifierNet(state["model_input_size"], state["model_hidden_size_fc1"], state["model_class_count"])
    net.load_state_dict(state["state_dict"])
    net.eval()
    tm["model"] = time.perf_counter() - t0
    path = os.path.join(out_dir, "classes.out")
    with open(path, "w", newline="") as f:
        csv.writer(f, delimiter="\t").writerow(CL.classes_header(state["model_class_count"]))
    with torch.no_grad():
        for z in range(0, len(names), block):
            t0 = time.perf_counter()
            lines = []
            for nm in names[z: z + block]:
                with open(os.path.join(kf, nm + ".kf")) as ff:
                    lines.extend(ff)
            df = pd.read_csv(StringIO("".join(lines)), header=None)
            df.set_index(0, inplace=True)
            x = torch.from_numpy(df.values * 1e4).float()
            t1 = time.perf_counter()
            ps = torch.exp(F.log_softmax(net(x), dim=1))
            top_p, top_class = ps.topk(1, dim=1)
            t2 = time.perf_counter()
            results = np.hstack([df.index.values[:, None], top_class.numpy(), top_p.numpy(), ps.numpy()])
            t3 = time.perf_counter()
            with open(path, "a", newline="") as f:
                csv.writer(f, delimiter="\t").writerows(results)
            t4 = time.perf_counter()
            for key, d in (("read", t1 - t0), ("forward", t2 - t1), ("hstack", t3 - t2), ("write", t4 - t3)):
                tm[key] += d
    return tm


def bench_classify(a, dev):
    from kf2vecfsw_amd import classify as CL
    work = a.work_dir
    kf, model, names = make_library(a, work)
    files = [os.path.join(kf, nm + ".kf") for nm in names]
    out = {"queries": a.queries, "hidden": a.hidden, "classes": a.classes, "block": a.block, "work_dir": work}
    devnull = open(os.devnull, "w")
    stderr, sys.stderr = sys.stderr, devnull
    try:
        CL.classify_func(kf, files, model, 28, os.path.join(work, "warm"), a.block, dev)    # pinned pools, the library
        t0 = time.perf_counter()
        CL.classify_func(kf, files, model, 28, os.path.join(work, "out"), a.block, dev)
        out["device_s"] = round(time.perf_counter() - t0, 3)
        tm = {}
        t0 = time.perf_counter()
        CL.classify_func(kf, files, model, 28, os.path.join(work, "out_t"), a.block, dev, times=tm)
        out["device_staged_s"] = round(time.perf_counter() - t0, 3)
        out["device_stages_s"] = {k: round(v, 4) for k, v in tm.items()}
    finally:
        sys.stderr = stderr
    t0 = time.perf_counter()
    tm = reference_lines(kf, model, names, os.path.join(work, "ref"), a.block)
    out["reference_cpu_s"] = round(time.perf_counter() - t0, 3)
    out["reference_stages_s"] = {k: round(v, 3) for k, v in tm.items()}
    out["speedup"] = round(out["reference_cpu_s"] / out["device_s"], 2)
    g, r = os.path.join(work, "out", "classes.out"), os.path.join(work, "ref", "classes.out")
    out["classes_out_bytes"] = os.path.getsize(g)
    with open(g, "rb") as fg, open(r, "rb") as fr:
        lg, lr = fg.read().split(b"\r\n"), fr.read().split(b"\r\n")
    same = len(lg) == len(lr) and lg[0] == lr[0]
    differ = 0
    for x, y in zip(lg[1:-1], lr[1:-1]):
        cx, cy = x.split(b"\t"), y.split(b"\t")
        same = same and cx[0] == cy[0] and len(cx) == len(cy)
        differ += cx[1] != cy[1]
    out["files_alike"] = bool(same)
    out["rows_whose_class_differs"] = int(differ)
    print(json.dumps({"classify": out}), flush=True)
    shutil.rmtree(work, ignore_errors=True)
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", nargs="+", default=["kernel", "classify"], choices=["kernel", "classify"])
    ap.add_argument("--queries", type=int, default=4000)
    ap.add_argument("--classes", type=int, default=64)
    ap.add_argument("--hidden", type=int, default=2048)
    ap.add_argument("--block", type=int, default=4000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--work-dir", default="/dev/shm/kf_classify_bench")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda:0")
    result = {"device": torch.cuda.get_device_name(0)}
    if "kernel" in a.parts:
        result["kernel"] = bench_kernel(a, dev)
    if "classify" in a.parts:
        result["classify"] = bench_classify(a, dev)
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
