"""kf_dist_loss alone and `train_model_set` end to end.

    python tools/train_bench.py [--parts kernel train] [--genomes 850] [--hidden 2048] [--embed 1024] [--batch 16]
                                [--epochs 10] [--reps 20] [--inner 50] [--work-dir /dev/shm/kf_train_bench]
                                [--out profiles/r22/train.json]

kernel  kf_dist_loss with and without the gradient at B, E = 16 x 1024, 64 x 1024
        and 850 x 1024 against torch's sequence for the reference's lines on the
        same device -- the gather of the true distances (on the device here,
        which favours torch: the reference gathers on the host), cdist in the
        direct form, the loss, and backward down to the embeddings' gradient; and
        for the loss alone the same lines under no_grad -- in one process: device
        events around --inner calls, 3 warm-ups, --reps repetitions in which the
        two take turns, medians per call.  The ratio is reported whatever it is.
        Values: the kernel's loss and gradient against torch's in float64.
train   a synthetic clade (--genomes `.kf` files of k = 7, a random symmetric
        distance matrix) in --work-dir: train_model_set_func as the command runs
        it for 1 epoch and for 1 + --epochs epochs, the steps of the --epochs
        epochs over the difference of the two times (reading the inputs, building
        the model and writing the outputs are in both); the split of an epoch from
        a copy of the command's step loop with a synchronisation behind every
        stage; against a restatement of the reference's loop on the
        same device: features on the host and a copy per step, a numpy gather of
        the true distances and a copy per step, loss.item() per step, and
        model.to('cpu'), torch.save and model.to(device) at each improving epoch.
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


def torch_loss(y, P, labels):
    """The reference's lines (utils.py:240-256, losses.py:13-49) on the device."""
    import torch
    real_dist = P.index_select(0, labels).index_select(1, labels)
    train_dist = torch.cdist(y, y, p=2, compute_mode="donot_use_mm_for_euclid_dist")
    weight = 1 / (real_dist + 1e-6)
    true_dist = torch.sqrt(real_dist)
    return ((train_dist - true_dist) ** 2 * weight).mean()


def bench_kernel(a, dev):
    import numpy as np
    import torch
    from kf2vecfsw_amd import train as TR
    out = {}
    gen = torch.Generator(device=dev).manual_seed(22)
    n = 850
    P = torch.rand((n, n), generator=gen, device=dev, dtype=torch.float64) * 3 + 0.05
    P = (P + P.T) / 2
    P.fill_diagonal_(0.0)
    for b, e in ((16, 1024), (64, 1024), (850, 1024)):
        y = torch.randn((b, e), generator=gen, device=dev, dtype=torch.float32) / (2.0 * e) ** 0.5
        labels = torch.randperm(n, generator=gen, device=dev)[:b]
        inner = a.inner if b < 850 else max(1, a.inner // 10)
        res = {"rows": b, "cols": e}
        for grad in (True, False):
            kept, ref = {}, {}

            def kernel():
                kept["loss"], kept["grad"], _ = TR.dist_loss(y, P, labels, grad=grad)

            def torch_lines():
                if grad:
                    yy = y.detach().requires_grad_(True)
                    loss = torch_loss(yy, P, labels)
                    loss.backward()
                    ref["loss"], ref["grad"] = loss.detach(), yy.grad
                else:
                    with torch.no_grad():
                        ref["loss"] = torch_loss(y, P, labels)

            k_ms, k_rng, t_ms, t_rng = timed(kernel, torch_lines, a.reps, inner)
            tag = "loss_and_grad" if grad else "loss_only"
            res[tag] = dict(kernel_us=round(k_ms * 1e3, 2), kernel_us_range=[round(v * 1e3, 2) for v in k_rng],
                            torch_us=round(t_ms * 1e3, 2), torch_us_range=[round(v * 1e3, 2) for v in t_rng],
                            torch_over_kernel=round(t_ms / k_ms, 2),
                            loss_rel_diff=float(abs(kept["loss"] - ref["loss"]) / abs(ref["loss"])))
            if grad:
                g, r = kept["grad"].double(), ref["grad"].double()
                res[tag]["grad_max_diff_over_max"] = float((g - r).abs().max() / r.abs().max())
        out["{}x{}".format(b, e)] = res
        print(json.dumps({"{}x{}".format(b, e): res}), flush=True)
    return out


def make_clade(a, work):
    import numpy as np
    from kf2vecfsw_amd import counter as C
    from kf2vecfsw_amd import main as M
    shutil.rmtree(work, ignore_errors=True)
    kf, dist = os.path.join(work, "kf"), os.path.join(work, "dist")
    os.makedirs(kf)
    os.makedirs(dist)
    nbins = C.num_bins(7)
    rng = np.random.default_rng(23)
    names = ["G%07d" % i for i in range(a.genomes)]
    base = rng.poisson(300, size=nbins)
    counts = np.maximum(1, base[None, :] + rng.normal(0, 60, size=(a.genomes, nbins))).astype(np.uint32)
    M.write_kf_files(kf, names, counts, False, False, 16)
    p = rng.uniform(0.05, 3.0, size=(a.genomes, a.genomes))
    p = (p + p.T) / 2
    np.fill_diagonal(p, 0.0)
    with open(os.path.join(dist, "synth_subtree_0.di_mtrx"), "w") as f:
        f.write("\t" + "\t".join(names) + "\n")
        for nm, row in zip(names, p):
            f.write(nm + "\t" + "\t".join(repr(float(v)) for v in row) + "\n")
    sub = os.path.join(dist, "synth.subtrees")
    with open(sub, "w") as f:
        f.write("genome clade\n" + "".join("{} 0\n".format(nm) for nm in names))
    return kf, dist, sub, names


def reference_loop(a, dev, kf, dist, names, out_dir):
    """train_model_set.py:430-504 restated on the device of this run; seconds for --epochs epochs and the steps."""
    import numpy as np
    import torch
    from kf2vecfsw_amd import features as F
    from kf2vecfsw_amd import query as Q
    from kf2vecfsw_amd import tables as T
    from kf2vecfsw_amd import train as TR
    os.makedirs(out_dir, exist_ok=True)
    x_host = F.features_from_kf(kf, 7, dev, samples=names, scaler=1e4, dtype=torch.float32).values.cpu()
    pdf_sorted = T.true_distances(os.path.join(dist, "synth_subtree_0.di_mtrx"), names, dev).values.cpu().numpy()
    torch.manual_seed(a.seed)
    model = Q.QueryNet(x_host.shape[1], a.hidden, a.embed).to(dev)
    optimizer = torch.optim.Adam(model.parameters(), lr=a.lr)
    gen = torch.Generator().manual_seed(a.seed)
    plan = TR.batch_plan(len(names), a.batch)
    lowest = float("inf")
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    saves = 0
    for epoch in range(a.epochs):
        perm = torch.randperm(len(names), generator=gen)
        train_loss, items = 0.0, 0
        for s, e in plan:
            labels = perm[s:e]
            images = x_host.index_select(0, labels).to(dev)
            real_dist = torch.from_numpy(pdf_sorted[np.ix_(list(labels), list(labels))]).to(dev)
            outputs = model(images.float())
            train_dist = torch.cdist(outputs, outputs, p=2, compute_mode="donot_use_mm_for_euclid_dist")
            weight = 1 / (real_dist + 1e-6)
            loss = ((train_dist - torch.sqrt(real_dist)) ** 2 * weight).mean()
            train_loss += loss.item() * images.shape[0]
            items += images.shape[0]
            optimizer.zero_grad()
            loss.backward()
            optimizer.step()
        train_loss /= items
        if train_loss < lowest:
            lowest = train_loss
            model.to("cpu")
            torch.save(TR.checkpoint_state(x_host.shape[1], a.hidden, a.embed, model.state_dict()),
                       os.path.join(out_dir, "model_subtree_0.ckpt"))
            model.to(dev)
            saves += 1
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0, a.epochs * len(plan), saves, lowest


def staged_epochs(a, dev, kf, dist, names):
    """The command's step loop (train.py) with a synchronisation behind every stage: seconds per stage and epoch."""
    import torch
    from kf2vecfsw_amd import features as F
    from kf2vecfsw_amd import query as Q
    from kf2vecfsw_amd import tables as T
    from kf2vecfsw_amd import train as TR
    x_all = F.features_from_kf(kf, 7, dev, samples=names, scaler=1e4, dtype=torch.float32).values
    P = T.true_distances(os.path.join(dist, "synth_subtree_0.di_mtrx"), names, dev).values
    torch.manual_seed(a.seed)
    model = Q.QueryNet(x_all.shape[1], a.hidden, a.embed).to(dev)
    optimizer = torch.optim.Adam(model.parameters(), lr=a.lr)
    gen = torch.Generator(device=dev)
    gen.manual_seed(a.seed)
    plan = TR.batch_plan(len(names), a.batch)
    rows = torch.arange(len(names), device=dev)
    tm = {"select": 0.0, "forward": 0.0, "loss": 0.0, "backward": 0.0, "step": 0.0, "epoch_read": 0.0}

    def lap(key, t0):
        torch.cuda.synchronize(dev)
        tm[key] += time.perf_counter() - t0
        return time.perf_counter()

    acc = torch.zeros(2, dtype=torch.float64, device=dev)
    for epoch in range(1 + a.epochs):
        if epoch == 1:                                        # the first epoch is the warm-up
            tm = dict.fromkeys(tm, 0.0)
        acc.zero_()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        perm = rows.index_select(0, torch.randperm(len(names), generator=gen, device=dev))
        for s, e in plan:
            labels = perm[s:e]
            images = x_all.index_select(0, labels)
            t0 = lap("select", t0)
            outputs = model(images)
            t0 = lap("forward", t0)
            loss, status = TR.dist_loss_fn(outputs, P, labels)
            acc[0] += loss.detach() * (e - s)
            acc[1] += status[0]
            t0 = lap("loss", t0)
            optimizer.zero_grad()
            loss.backward()
            t0 = lap("backward", t0)
            optimizer.step()
            t0 = lap("step", t0)
        acc.cpu()
        tm["epoch_read"] += time.perf_counter() - t0
    return {k: round(v / a.epochs, 5) for k, v in tm.items()}


def bench_train(a, dev):
    import glob
    from kf2vecfsw_amd import train as TR
    work = a.work_dir
    kf, dist, sub, names = make_clade(a, work)
    files = glob.glob(os.path.join(kf, "*.kf"))
    out = {"genomes": a.genomes, "k": 7, "hidden": a.hidden, "embed": a.embed, "batch": a.batch, "epochs": a.epochs,
           "lr": a.lr}

    def run(tag, epochs):
        import torch
        devnull = open(os.devnull, "w")
        stdout, sys.stdout = sys.stdout, devnull
        try:
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            kept = TR.train_model_set_func(kf, files, sub, dist, epochs, a.hidden, a.embed, a.batch, a.lr, 3e-6, 2000,
                                           [0], a.seed, os.path.join(work, tag), None, None, use_fsw=False, device=dev,
                                           keep=True)
            torch.cuda.synchronize(dev)
            return time.perf_counter() - t0, kept[0]
        finally:
            sys.stdout = stdout

    run("warm", 1)                                            # the library, pinned pools, the GEMMs' first calls
    ones, alls = [], []
    for i in range(3):                                        # the two take turns; medians
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
    out["stages_s_per_epoch"] = staged_epochs(a, dev, kf, dist, names)
    reference_loop(a, dev, kf, dist, names, os.path.join(work, "ref_warm"))      # its warm-up: one full pass
    ref_s, ref_steps, saves, lowest = reference_loop(a, dev, kf, dist, names, os.path.join(work, "ref"))
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
    ap.add_argument("--lr", type=float, default=1e-5)
    ap.add_argument("--seed", type=int, default=28)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--work-dir", default="/dev/shm/kf_train_bench")
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
