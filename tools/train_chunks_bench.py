"""kf_dist_loss_views alone and `train_model_set_chunks` end to end.

    python tools/train_chunks_bench.py [--parts kernel train] [--genomes 850] [--hidden 2048] [--embed 1024]
                                       [--batch 16] [--epochs 10] [--reps 20] [--inner 50]
                                       [--work-dir /dev/shm/kf_train_chunks_bench] [--out profiles/r25/train_chunks.json]

kernel  kf_dist_loss_views (views = 2, eps = 1000) with the gradient at 32 rows
        (the default batch of 16 genomes), 128 rows and 1,700 rows (an 850-genome
        clade in one batch), E = 1,024, against torch's sequence for the
        reference's lines on the same device -- repeat_interleave of the labels,
        the gather of the true distances (on the device here, which favours
        torch: the reference gathers on the host), cdist in the direct form,
        Loss_chunks, and backward down to the embeddings' gradient -- in one
        process: device events around --inner calls, 3 warm-ups, --reps
        repetitions in which the two take turns, medians per call.  The ratio is
        reported whatever it is.  Values: the kernel's loss and gradient against
        torch's in float64.
train   a synthetic clade (--genomes get_chunks `.kf` files of k = 7 with 5 to 12
        windows each, their full-genome files, a random symmetric distance
        matrix in (50, 3000)) in --work-dir: train_model_set_chunks_func as the
        command runs it for 1 epoch and for 1 + --epochs epochs, the steps of the
        --epochs epochs over the difference of the two times (reading the inputs,
        building the model and writing the outputs are in both); against a
        restatement of the reference's loop on the same device: per item the two
        runs drawn and their features built in numpy on the host
        (Dataset_chunks_2rows), a copy per step, a numpy gather of the true
        distances and a copy per step, loss.item() per step, and model.to('cpu'),
        torch.save and model.to(device) at each improving epoch.
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

from train_bench import median, timed  # noqa: E402

VIEWS, EPS = 2, 1000.0
WINDOW = 10000


def torch_loss(y, P, labels):
    """The reference's lines (train_model_set_chunks.py:397-418, losses.py:58-117) on the device."""
    import torch
    labels = torch.repeat_interleave(labels, VIEWS, dim=0)
    real_dist = P.index_select(0, labels).index_select(1, labels)
    train_dist = torch.cdist(y, y, p=2, compute_mode="donot_use_mm_for_euclid_dist")
    weight = 1 / (real_dist + 1000)
    true_dist = torch.sqrt(real_dist)
    return ((train_dist - true_dist) ** 2 * weight).mean()


def bench_kernel(a, dev):
    import torch
    from kf2vecfsw_amd import train as TR
    out = {}
    gen = torch.Generator(device=dev).manual_seed(25)
    n = 850
    P = torch.rand((n, n), generator=gen, device=dev, dtype=torch.float64) * 2950 + 50
    P = (P + P.T) / 2
    P.fill_diagonal_(0.0)
    for b, e in ((32, 1024), (128, 1024), (1700, 1024)):
        y = torch.randn((b, e), generator=gen, device=dev, dtype=torch.float32) * (32.0 / (2.0 * e) ** 0.5)
        labels = torch.randperm(n, generator=gen, device=dev)[:b // VIEWS]
        inner = a.inner if b < 1000 else max(1, a.inner // 10)
        kept, ref = {}, {}

        def kernel():
            kept["loss"], kept["grad"], _ = TR.dist_loss(y, P, labels, grad=True, views=VIEWS, eps=EPS)

        def torch_lines():
            yy = y.detach().requires_grad_(True)
            loss = torch_loss(yy, P, labels)
            loss.backward()
            ref["loss"], ref["grad"] = loss.detach(), yy.grad

        k_ms, k_rng, t_ms, t_rng = timed(kernel, torch_lines, a.reps, inner)
        g, r = kept["grad"].double(), ref["grad"].double()
        res = dict(rows=b, cols=e, kernel_us=round(k_ms * 1e3, 2), kernel_us_range=[round(v * 1e3, 2) for v in k_rng],
                   torch_us=round(t_ms * 1e3, 2), torch_us_range=[round(v * 1e3, 2) for v in t_rng],
                   torch_over_kernel=round(t_ms / k_ms, 2),
                   loss_rel_diff=float(abs(kept["loss"] - ref["loss"]) / abs(ref["loss"])),
                   grad_max_diff_over_max=float((g - r).abs().max() / r.abs().max()))
        out["{}x{}".format(b, e)] = res
        print(json.dumps({"{}x{}".format(b, e): res}), flush=True)
    return out


def make_clade(a, work):
    """The synthetic clade's files; returns the directories, the `.subtrees` path, the names and the window rows."""
    import numpy as np
    from kf2vecfsw_amd import chunks as CH
    from kf2vecfsw_amd import counter as C
    from kf2vecfsw_amd import main as M
    shutil.rmtree(work, ignore_errors=True)
    chunks, full, dist = (os.path.join(work, d) for d in ("chunks", "full", "dist"))
    for d in (chunks, full, dist):
        os.makedirs(d)
    nbins = C.num_bins(7)
    rng = np.random.default_rng(25)
    names = ["G%07d" % i for i in range(a.genomes)]
    rows = []
    for nm in names:
        comp = rng.dirichlet(np.full(nbins, 2.0))
        r = rng.multinomial(WINDOW - 6, comp, size=int(rng.integers(5, 13))).astype(np.uint16)
        rows.append(r)
        text, _ = CH.format_rows_host(r, [nm + ".part_c.part_c_sliding__"], np.zeros(r.shape[0], np.int64),
                                      np.arange(r.shape[0], dtype=np.int64) * WINDOW, WINDOW, False)
        with open(os.path.join(chunks, nm + ".kf"), "wb") as f:
            f.write(text)
    M.write_kf_files(full, names, np.stack([r.astype(np.uint32).sum(axis=0) for r in rows]).astype(np.uint32), False,
                     False, 16)
    p = rng.uniform(50.0, 3000.0, size=(a.genomes, a.genomes))
    p = (p + p.T) / 2
    np.fill_diagonal(p, 0.0)
    with open(os.path.join(dist, "synth_subtree_0.di_mtrx"), "w") as f:
        f.write("\t" + "\t".join(names) + "\n")
        for nm, row in zip(names, p):
            f.write(nm + "\t" + "\t".join(repr(float(v)) for v in row) + "\n")
    sub = os.path.join(dist, "synth.subtrees")
    with open(sub, "w") as f:
        f.write("genome clade\n" + "".join("{} 0\n".format(nm) for nm in names))
    return chunks, full, dist, sub, names, rows


def reference_loop(a, dev, rows, dist, names, out_dir):
    """train_model_set_chunks.py:380-558 restated on the device of this run; seconds for --epochs epochs and the steps."""
    import numpy as np
    import torch
    from kf2vecfsw_amd import chunks as CH
    from kf2vecfsw_amd import query as Q
    from kf2vecfsw_amd import tables as T
    from kf2vecfsw_amd import train as TR
    os.makedirs(out_dir, exist_ok=True)
    pdf_sorted = T.true_distances(os.path.join(dist, "synth_subtree_0.di_mtrx"), names, dev).values.cpu().numpy()
    input_size = rows[0].shape[1]
    torch.manual_seed(a.seed)
    model = Q.QueryNet(input_size, a.hidden, a.embed).to(dev)
    optimizer = torch.optim.Adam(model.parameters(), lr=a.lr)
    gen = torch.Generator().manual_seed(a.seed)
    rng = np.random.RandomState(a.seed)
    plan = TR.batch_plan(len(names), a.batch)
    lowest = float("inf")
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    saves = 0

    def item(g):                                              # Dataset_chunks_2rows.__getitem__ (datasets.py:47-62)
        r = rows[g]
        lo, n = CH.draw_ranges([r.shape[0]], rng)
        views = []
        for v in range(VIEWS):
            c = r[int(lo[0, v]): int(lo[0, v]) + int(n[0, v])].sum(axis=0, dtype=np.uint64).astype(np.float64)
            views.append(np.nan_to_num(c / c.sum()) * 1e4)
        return np.concatenate(views)

    for epoch in range(a.epochs):
        perm = torch.randperm(len(names), generator=gen)
        train_loss, items = 0.0, 0
        for s, e in plan:
            labels = perm[s:e]
            images = torch.from_numpy(np.stack([item(int(g)) for g in labels])).reshape(-1, input_size).to(dev)
            labels = torch.repeat_interleave(labels, VIEWS, dim=0)
            real_dist = torch.from_numpy(pdf_sorted[np.ix_(list(labels), list(labels))]).to(dev)
            outputs = model(images.float())
            train_dist = torch.cdist(outputs, outputs, p=2, compute_mode="donot_use_mm_for_euclid_dist")
            weight = 1 / (real_dist + 1000)
            loss = ((train_dist - torch.sqrt(real_dist)) ** 2 * weight).mean()
            train_loss += loss.item() * (images.shape[0] / 2)
            items += images.shape[0] / 2
            optimizer.zero_grad()
            loss.backward()
            optimizer.step()
        train_loss /= items
        if train_loss < lowest:
            lowest = train_loss
            model.to("cpu")
            torch.save(TR.checkpoint_state(input_size, a.hidden, a.embed, model.state_dict()),
                       os.path.join(out_dir, "model_subtree_0.ckpt"))
            model.to(dev)
            saves += 1
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0, a.epochs * len(plan), saves, lowest


def bench_train(a, dev):
    import glob
    from kf2vecfsw_amd import train as TR
    from kf2vecfsw_amd import train_chunks as TC
    work = a.work_dir
    t0 = time.perf_counter()
    chunks, full, dist, sub, names, rows = make_clade(a, work)
    files = glob.glob(os.path.join(chunks, "*.kf"))
    out = {"genomes": a.genomes, "k": 7, "windows": int(sum(r.shape[0] for r in rows)), "hidden": a.hidden,
           "embed": a.embed, "batch": a.batch, "epochs": a.epochs, "lr": a.lr,
           "make_clade_s": round(time.perf_counter() - t0, 2)}

    def run(tag, epochs):
        import torch
        devnull = open(os.devnull, "w")
        stdout, sys.stdout = sys.stdout, devnull
        try:
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            kept = TC.train_model_set_chunks_func(chunks, full, files, sub, dist, epochs, a.hidden, a.embed, a.batch, a.lr,
                                                  3e-6, 2000, [0], a.seed, False, os.path.join(work, tag), device=dev,
                                                  keep=True)
            torch.cuda.synchronize(dev)
            return time.perf_counter() - t0, kept[0]
        finally:
            sys.stdout = stdout

    run("warm", 1)                                            # the library, pinned pools, the GEMMs' first calls
    ones, alls = [], []
    for i in range(a.turns):                                  # the two take turns; medians
        ones.append(run("one", 1)[0])
        t, kept = run("out", 1 + a.epochs)
        alls.append(t)
    steps = a.epochs * len(TR.batch_plan(a.genomes, a.batch))
    out["command_1_epoch_s"] = round(median(ones), 4)
    out["command_s"] = round(median(alls), 4)
    out["epochs_s"] = round(median(alls) - median(ones), 4)
    out["steps"] = steps
    out["steps_per_s"] = round(steps / (median(alls) - median(ones)), 1)
    out["first_and_lowest_loss"] = [kept["losses"][0], kept["lowest_loss"]]
    saved, a.epochs = a.epochs, 1
    reference_loop(a, dev, rows, dist, names, os.path.join(work, "ref_warm"))    # its warm-up: one epoch
    a.epochs = saved
    ref_s, ref_steps, saves, lowest = reference_loop(a, dev, rows, dist, names, os.path.join(work, "ref"))
    out["reference_loop_s"] = round(ref_s, 4)
    out["reference_loop_steps_per_s"] = round(ref_steps / ref_s, 1)
    out["reference_loop_checkpoints"] = saves
    out["reference_loop_lowest_loss"] = lowest
    out["speedup"] = round(out["steps_per_s"] / out["reference_loop_steps_per_s"], 2)
    print(json.dumps({"train": out}), flush=True)
    shutil.rmtree(work, ignore_errors=True)
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", nargs="+", default=["kernel", "train"], choices=["kernel", "train"])
    ap.add_argument("--genomes", type=int, default=850)
    ap.add_argument("--hidden", type=int, default=2048)
    ap.add_argument("--embed", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--turns", type=int, default=3)
    ap.add_argument("--lr", type=float, default=1e-5)
    ap.add_argument("--seed", type=int, default=28)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--work-dir", default="/dev/shm/kf_train_chunks_bench")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda:0")
    result = {"device": torch.cuda.get_device_name(0)}
    if "kernel" in a.parts:
        result["kernel"] = bench_kernel(a, dev)
    if "train" in a.parts:
        result["train"] = bench_train(a, dev)
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
