"""The float formatter, the distance kernel and `query` end to end.

    python tools/float_format_bench.py [--parts format sqdist query] [--queries 4000] [--backbone 10000]
                                       [--dim 1024] [--reps 10] [--work-dir /dev/shm/kf_query_bench] [--out FILE]

format   kf_format_float_rows alone on --queries x --backbone float32 (squared
         distances of the magnitude query writes) in the widened and in the
         float32-shortest form, and on a --queries x --queries float64 matrix;
         against a device copy of the same text bytes, in one process: device
         events, 3 warm-ups, --reps repetitions in which the two take turns,
         medians.  kernel_ms, copy_ms, text_bytes, text_GBps, kernel_over_copy;
         and whether the first and last 8 rows equal tables.format_float_rows_host.
sqdist   kf_sq_distances at Q = --queries, B = --backbone, D = --dim against
         torch.cdist(compute_mode='donot_use_mm_for_euclid_dist') with the
         square and the cut, on the device, in the same run: in one call, and
         in row chunks whose launches stay below 2^32 threads.  Values: all
         three against float64 on the device on rows sampled from the whole
         matrix (the first 8, the last 40 with the ragged tile, 64 at random),
         against each other over the whole matrix, and the kernel bit for bit
         with query.sq_distances_host on the first and the last 70 x 70 corner.
query    a synthetic k = 7 library (--queries `.kf` files of one row, a model of
         8192 x 2048 x --dim, --backbone backbone genomes) in --work-dir: query_func
         with times= (seconds per stage; the stage times of the device are taken
         with a synchronisation per stage, so this run does not overlap them)
         and once without, against the reference's lines on the CPU of the same
         machine (`cat` + pandas, the forward pass, cdist, .tolist() and
         csv.writer, restated here), and whether the files are equal in labels
         and shape.
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


def timed(fn, other, reps):
    """Medians (ms) of fn and other, taking turns, after 3 warm-ups of each."""
    import torch
    a, b = [], []
    for i in range(3 + reps):
        for f, into in ((fn, a), (other, b)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            if i >= 3:
                into.append(e0.elapsed_time(e1))
    return median(a), (min(a), max(a)), median(b), (min(b), max(b))


def bench_format(a, dev):
    import numpy as np
    import torch
    from kf2vecfsw_amd import _native as N
    from kf2vecfsw_amd import tables as T
    out = {}
    gen = torch.Generator(device=dev).manual_seed(20)
    shapes = [("float32_widened", (a.queries, a.backbone), torch.float32, T.KF_FLOAT_WIDENED),
              ("float32_shortest", (a.queries, a.backbone), torch.float32, T.KF_FLOAT_SHORTEST),
              ("float64", (a.queries, a.queries), torch.float64, T.KF_FLOAT_SHORTEST)]
    for name, (n, ncols), dtype, mode in shapes:
        vals = (torch.rand((n, ncols), generator=gen, device=dev, dtype=torch.float32) * 3.0).square().to(dtype)
        labels = [b"G%09d" % i for i in range(n)]
        cap = n * T.float_row_bound(ncols, 10)
        assert cap < 1 << 32
        pre_off = np.arange(n + 1, dtype=np.int64) * 10
        d_pre = torch.from_numpy(np.frombuffer(b"".join(labels), dtype=np.uint8).copy()).to(dev)
        d_pre_off = torch.from_numpy(pre_off).to(dev)
        d_rpre = torch.arange(n, dtype=torch.int32, device=dev)
        text = torch.empty(cap, dtype=torch.uint8, device=dev)
        row_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        status = torch.empty(4, dtype=torch.int64, device=dev)
        need = int(N.lib().kf_format_float_scratch_bytes(n, ncols))
        scratch = torch.empty(need // 8 + 1, dtype=torch.int64, device=dev)
        s = torch.cuda.current_stream(dev).cuda_stream

        def kernel():
            N.check(N.lib().kf_format_float_rows(vals.data_ptr(), vals.element_size(), n, ncols, mode, 9, 0x0A0D, 2, 0,
                                                 d_pre.data_ptr(), d_pre_off.data_ptr(), n, d_rpre.data_ptr(),
                                                 text.data_ptr(), cap, row_off.data_ptr(), status.data_ptr(),
                                                 scratch.data_ptr(), need, s))
        kernel()
        st = status.cpu().tolist()
        assert st[0] == 0, st
        total = st[1]
        dst = torch.empty(total, dtype=torch.uint8, device=dev)
        k_ms, k_rng, c_ms, c_rng = timed(kernel, lambda: dst.copy_(text[:total]), a.reps)
        off = row_off.cpu().numpy()
        equal = True
        for r0, r1 in ((0, min(8, n)), (max(0, n - 8), n)):
            exp, _ = T.format_float_rows_host(vals[r0:r1], [x.decode() for x in labels[r0:r1]], mode)
            equal = equal and text[int(off[r0]): int(off[r1])].cpu().numpy().tobytes() == exp
        out[name] = dict(rows=n, cols=ncols, text_bytes=total, bytes_per_field=round(total / (n * ncols), 2),
                         kernel_ms=round(k_ms, 3), kernel_ms_range=[round(x, 3) for x in k_rng],
                         copy_ms=round(c_ms, 3), copy_ms_range=[round(x, 3) for x in c_rng],
                         kernel_over_copy=round(k_ms / c_ms, 2), text_GBps=round(total / k_ms / 1e6, 1),
                         first_and_last_8_rows_equal_host_statement=bool(equal))
        print(json.dumps({name: out[name]}), flush=True)
        del vals, text, dst
    return out


def ref_cut(x, y):
    import torch
    d = torch.square(torch.cdist(x, y, p=2, compute_mode="donot_use_mm_for_euclid_dist"))
    return torch.where(d < 1.0e-6, torch.tensor(0, dtype=d.dtype, device=d.device), d)


def cdist_chunked(x, y):
    """ref_cut in row chunks whose launches stay below 2^32 threads (cdist's direct
    form runs a workgroup of 256 threads per output entry)."""
    import torch
    per = max(1, ((1 << 32) - 1) // (256 * max(1, y.shape[0])))
    return torch.cat([ref_cut(x[r: r + per], y) for r in range(0, x.shape[0], per)], 0)


def against_float64(t, x, y, rows):
    """t[rows] against the float64 value of the same float32 inputs (the cut applied): (largest relative error,
    entries off by more than 1e-4, the first few of them)."""
    import torch
    worst, n_bad, first = 0.0, 0, []
    y64 = y.double()
    for i in range(0, len(rows), 8):
        r = torch.as_tensor(rows[i: i + 8], device=x.device)
        exact = (x[r].double()[:, None, :] - y64[None, :, :]).square().sum(-1)
        exact = torch.where(exact < 1e-6, torch.zeros_like(exact), exact)
        rel = (t[r].double() - exact).abs() / exact.clamp_min(1e-300)
        worst = max(worst, float(rel.max()))
        bad = (rel > 1e-4).nonzero()
        n_bad += int(bad.shape[0])
        for k, j in bad[: max(0, 4 - len(first))].tolist():
            first.append([int(r[k]), j, float(t[int(r[k]), j]), float(exact[k, j])])
    return worst, n_bad, first


def bench_sqdist(a, dev):
    import numpy as np
    import torch
    from kf2vecfsw_amd import query as Q
    gen = torch.Generator(device=dev).manual_seed(21)
    x = torch.randn((a.queries, a.dim), generator=gen, device=dev)
    y = torch.randn((a.backbone, a.dim), generator=gen, device=dev)
    k_ms, k_rng, c_ms, c_rng = timed(lambda: Q.sq_distances(x, y), lambda: ref_cut(x, y), a.reps)
    _, _, cc_ms, cc_rng = timed(lambda: None, lambda: cdist_chunked(x, y), a.reps)
    got = Q.sq_distances(x, y)
    whole = ref_cut(x, y)
    chunked = cdist_chunked(x, y)
    # values: rows sampled from the whole matrix (the first, the last ragged tile, 64 at random), every column,
    # against float64 on the device; and the three results against each other over the whole matrix
    rs = np.random.default_rng(5)
    rows = sorted(set(list(range(min(8, a.queries))) + list(range(max(0, a.queries - 40), a.queries)) +
                      rs.integers(0, a.queries, 64).tolist()))
    checks = {}
    for name, t in (("kernel", got), ("cdist_one_call", whole), ("cdist_in_chunks", chunked)):
        worst, n_bad, first = against_float64(t, x, y, rows)
        checks[name] = dict(max_rel_err_to_float64=worst, entries_off_by_1e_4=n_bad, first_off=first)
    def rel(p, q):
        return float(((p - q).abs() / q.clamp_min(1e-30)).max())
    off = ((whole - chunked).abs() > 1e-4 * chunked).any(1).nonzero().reshape(-1)
    corner = Q.sq_distances_host(x[:70].cpu().numpy(), y[:70].cpu().numpy())
    tail = Q.sq_distances_host(x[-70:].cpu().numpy(), y[-70:].cpu().numpy())
    flops = 3.0 * a.queries * a.backbone * a.dim
    out = dict(Q=a.queries, B=a.backbone, D=a.dim, kernel_ms=round(k_ms, 3), kernel_ms_range=[round(v, 3) for v in k_rng],
               cdist_one_call_ms=round(c_ms, 3), cdist_one_call_ms_range=[round(v, 3) for v in c_rng],
               cdist_in_chunks_ms=round(cc_ms, 3), cdist_in_chunks_ms_range=[round(v, 3) for v in cc_rng],
               cdist_in_chunks_over_kernel=round(cc_ms / k_ms, 2), kernel_TFLOPs=round(flops / k_ms / 1e9, 2),
               sampled_rows=len(rows), against_float64_on_sampled_rows=checks,
               whole_matrix_max_rel_diff=dict(kernel_to_cdist_in_chunks=rel(got, chunked),
                                              kernel_to_cdist_one_call=rel(got, whole),
                                              cdist_one_call_to_cdist_in_chunks=rel(whole, chunked)),
               cdist_one_call_rows_off=dict(count=int(off.numel()), first=int(off[0]) if off.numel() else None,
                                            last=int(off[-1]) if off.numel() else None),
               corners_70x70_equal_host_statement=bool(
                   np.array_equal(got[:70, :70].cpu().numpy().view(np.uint32), corner.view(np.uint32)) and
                   np.array_equal(got[-70:, -70:].cpu().numpy().view(np.uint32), tail.view(np.uint32))))
    print(json.dumps({"sqdist": out}), flush=True)
    return out


def make_library(a, dev, work):
    """--queries `.kf` files of one k=7 row each, one clade, its model and backbone."""
    import numpy as np
    import torch
    from kf2vecfsw_amd import counter as C
    from kf2vecfsw_amd import main as M
    from kf2vecfsw_amd import query as Q
    from kf2vecfsw_amd import tables as T
    shutil.rmtree(work, ignore_errors=True)
    kf, model = os.path.join(work, "kf"), os.path.join(work, "model")
    os.makedirs(kf)
    os.makedirs(model)
    nbins = C.num_bins(7)
    rng = np.random.default_rng(22)
    names = ["Q%07d" % i for i in range(a.queries)]
    counts = rng.poisson(300, size=(a.queries, nbins)).astype(np.uint32)
    M.write_kf_files(kf, names, counts, False, False, 16)
    with open(os.path.join(work, "classes.out"), "w") as f:
        f.write("genome\ttop_class\ttop_p\n" + "".join("{}\t0.0\t0.9\n".format(nm) for nm in names))
    torch.manual_seed(23)
    net = Q.QueryNet(nbins, 2048, a.dim)
    torch.save({"model_input_size": nbins, "model_hidden_size_fc1": 2048, "model_embedding_size": a.dim,
                "state_dict": net.state_dict()}, os.path.join(model, "model_subtree_0.ckpt"))
    emb = torch.randn((a.backbone, a.dim), device=dev) * 0.5
    T.write_float_table(os.path.join(model, "embeddings_subtree_0.csv"), ["B%07d" % i for i in range(a.backbone)], emb,
                        mode=T.KF_FLOAT_SHORTEST, eol="\n", nan_empty=True, threads=16)
    return kf, model, names


def reference_lines(kf, model, names, out_dir, block):
    """kf2vec/query.py:108-192 for the one clade, on the CPU; seconds per stage."""
    import csv
    import subprocess
    from io import StringIO
    import pandas as pd
    import torch
    from kf2vecfsw_amd import query as Q
    os.makedirs(out_dir, exist_ok=True)
    tm = dict(read=0.0, forward=0.0, distances=0.0, tolist=0.0, write=0.0, backbone=0.0)
    t0 = time.perf_counter()
    state = torch.load(os.path.join(model, "model_subtree_0.ckpt"))
    net = Q.QueryNet(state["model_input_size"], state["model_hidden_size_fc1"], state["model_embedding_size"])
    net.load_state_dict(state["state_dict"])
    net.eval()
    de = pd.read_csv(os.path.join(model, "embeddings_subtree_0.csv"), sep="\t", header=None, index_col=0)
    et = torch.from_numpy(de.values).float()
    tm["backbone"] = time.perf_counter() - t0
    with open(os.path.join(out_dir, "apples_input_di_mtrx_subtree_0.csv"), "w", newline="") as fd, \
            open(os.path.join(out_dir, "embedding_subtree_0.emb"), "w", newline="") as fe, torch.no_grad():
        dw, ew = csv.writer(fd, delimiter="\t"), csv.writer(fe, delimiter="\t")
        dw.writerow([""] + de.index.tolist())
        for z in range(0, len(names), block):
            t0 = time.perf_counter()
            cat = subprocess.run(["cat"] + [os.path.join(kf, f + ".kf") for f in names[z: z + block]],
                                 capture_output=True, text=True)
            fi = pd.read_csv(StringIO(cat.stdout), index_col=None, header=None, sep=",")
            fi.set_index(0, inplace=True)
            fi = fi.iloc[:, :] * 1e4
            ql = fi.index.tolist()
            t1 = time.perf_counter()
            out = net(torch.from_numpy(fi.values).float())
            t2 = time.perf_counter()
            pw = ref_cut(out, et)
            t3 = time.perf_counter()
            db, eb = pw.numpy().tolist(), out.numpy().tolist()
            t4 = time.perf_counter()
            for lbl, row in zip(ql, db):
                dw.writerow([lbl] + row)
            for lbl, row in zip(ql, eb):
                ew.writerow([lbl] + row)
            t5 = time.perf_counter()
            for key, d in (("read", t1 - t0), ("forward", t2 - t1), ("distances", t3 - t2), ("tolist", t4 - t3),
                           ("write", t5 - t4)):
                tm[key] += d
    return tm


def bench_query(a, dev):
    from kf2vecfsw_amd import query as Q
    work = a.work_dir
    kf, model, names = make_library(a, dev, work)
    files = [os.path.join(kf, nm + ".kf") for nm in names]
    out = {"queries": a.queries, "backbone": a.backbone, "dim": a.dim, "block": a.block, "work_dir": work}
    devnull = open(os.devnull, "w")
    stdout, sys.stdout = sys.stdout, devnull
    try:
        Q.query_func(kf, files, model, work, 28, os.path.join(work, "warm"), None, a.block, dev)    # pinned pools, the library
        t0 = time.perf_counter()
        Q.query_func(kf, files, model, work, 28, os.path.join(work, "out"), None, a.block, dev)
        out["device_s"] = round(time.perf_counter() - t0, 3)
        tm = {}
        t0 = time.perf_counter()
        Q.query_func(kf, files, model, work, 28, os.path.join(work, "out_t"), None, a.block, dev, times=tm)
        out["device_staged_s"] = round(time.perf_counter() - t0, 3)
        out["device_stages_s"] = {k: round(v, 3) for k, v in tm.items()}
    finally:
        sys.stdout = stdout
    t0 = time.perf_counter()
    tm = reference_lines(kf, model, names, os.path.join(work, "ref"), a.block)
    out["reference_cpu_s"] = round(time.perf_counter() - t0, 3)
    out["reference_stages_s"] = {k: round(v, 3) for k, v in tm.items()}
    out["speedup"] = round(out["reference_cpu_s"] / out["device_s"], 2)
    same = True
    for f in ("apples_input_di_mtrx_subtree_0.csv", "embedding_subtree_0.emb"):
        g, r = os.path.join(work, "out", f), os.path.join(work, "ref", f)
        out[f + "_bytes"] = os.path.getsize(g)
        with open(g, "rb") as fg, open(r, "rb") as fr:
            lg, lr = fg.readline(), fr.readline()
            same = same and lg.split(b"\t")[0] == lr.split(b"\t")[0] and lg.count(b"\t") == lr.count(b"\t")
            if f.endswith(".csv"):
                same = same and lg == lr
        same = same and abs(os.path.getsize(g) - os.path.getsize(r)) < 0.01 * os.path.getsize(r)
    out["files_alike"] = bool(same)
    print(json.dumps({"query": out}), flush=True)
    shutil.rmtree(work, ignore_errors=True)
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", nargs="+", default=["format", "sqdist", "query"], choices=["format", "sqdist", "query"])
    ap.add_argument("--queries", type=int, default=4000)
    ap.add_argument("--backbone", type=int, default=10000)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--block", type=int, default=4000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--work-dir", default="/dev/shm/kf_query_bench")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda:0")
    result = {"device": torch.cuda.get_device_name(0)}
    if "format" in a.parts:
        result["format"] = bench_format(a, dev)
    if "sqdist" in a.parts:
        result["sqdist"] = bench_sqdist(a, dev)
    if "query" in a.parts:
        result["query"] = bench_query(a, dev)
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
