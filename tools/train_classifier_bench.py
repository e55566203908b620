"""kf_class_loss alone and `train_classifier` end to end.

    python tools/train_classifier_bench.py [--parts kernel train] [--genomes 850] [--classes 16] [--hidden 2048]
                                           [--batch 16] [--epochs 10] [--reps 20] [--inner 50]
                                           [--work-dir /dev/shm/kf_train_classifier_bench]
                                           [--out profiles/r23/train_classifier.json]

kernel  kf_class_loss (loss, gradient, hits) and its loss-only call at B x C =
        16 x 2, 16 x 256, 4,000 x 16 and 4,000 x 4,096 against torch's sequence
        for the reference's lines on the same device -- log_softmax, nll_loss,
        backward down to the logits, exp, topk, the comparison with the classes
        and its sum; for the loss alone the same lines under no_grad -- in one
        process: device events around --inner calls, 3 warm-ups, --reps
        repetitions in which the two take turns, medians per call.  The ratio is
        reported whatever it is.  Values: the kernel's loss, gradient and hits
        against torch's.
train   a synthetic library (--genomes `.kf` files of k = 7 in --classes clades)
        in --work-dir: train_classifier_model_func as the command runs it for 1
        epoch and for 1 + --epochs epochs, the steps of the --epochs epochs over
        the difference of the two times (reading the inputs, building the model
        and writing the outputs are in both); against a restatement of the
        reference's loop on the same device: features on the host and a copy per
        step, a numpy gather of the classes and a copy per step, loss.item() and
        accuracy_score on host copies per step, and model.to('cpu'), torch.save
        and model.to(device) at each improving epoch.
Each part runs in a process of its own under its own time limit (--limit
seconds); a part that fails or runs out of time ends the run.  One JSON object
with a key per part (also written to --out)."""
from __future__ import annotations

import argparse
import json
import os
import shutil
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((16, 2), (16, 256), (4000, 16), (4000, 4096))


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


def torch_lines(x, true, grad):
    """The reference's lines (models.py:126-132, train_classifier_model.py:326-342) on the device:
    (loss, the gradient with respect to the logits or None, the count of right classes)."""
    import torch
    import torch.nn.functional as F
    if grad:
        xx = x.detach().requires_grad_(True)
        model_class = F.log_softmax(xx, dim=1)
        loss = F.nll_loss(model_class, true)
        loss.backward()
        g = xx.grad
    else:
        with torch.no_grad():
            model_class = F.log_softmax(x, dim=1)
            loss = F.nll_loss(model_class, true)
        g = None
    ps = torch.exp(model_class.detach())
    _, top_class = ps.topk(1, dim=1)
    hits = (top_class[:, 0] == true).sum()
    return loss.detach(), g, hits


def bench_kernel(a, dev):
    import torch
    from kf2vecfsw_amd import train_classifier as TC
    out = {}
    gen = torch.Generator(device=dev).manual_seed(23)
    for b, c in SHAPES:
        x = (torch.rand((b, c), generator=gen, device=dev, dtype=torch.float32) - 0.5) * 16.0
        true = torch.randint(0, c, (b,), generator=gen, device=dev)
        inner = a.inner if b * c < 1 << 20 else max(1, a.inner // 5)
        res = {"rows": b, "cols": c}
        for grad in (True, False):
            kept, ref = {}, {}

            def kernel():
                kept["loss"], kept["grad"], _, kept["hits"], _ = TC.class_loss(x, true, grad=grad)

            def lines():
                ref["loss"], ref["grad"], ref["hits"] = torch_lines(x, true, grad)

            k_ms, k_rng, t_ms, t_rng = timed(kernel, lines, a.reps, inner)
            tag = "loss_grad_hits" if grad else "loss_and_hits_only"
            res[tag] = dict(kernel_us=round(k_ms * 1e3, 2), kernel_us_range=[round(v * 1e3, 2) for v in k_rng],
                            torch_us=round(t_ms * 1e3, 2), torch_us_range=[round(v * 1e3, 2) for v in t_rng],
                            torch_over_kernel=round(t_ms / k_ms, 2),
                            loss_rel_diff=float(abs(kept["loss"] - ref["loss"].double()) / abs(ref["loss"].double())),
                            hits=[int(kept["hits"][0]), int(ref["hits"])])
            if grad:
                g, r = kept["grad"].double(), ref["grad"].double()
                res[tag]["grad_max_diff"] = float((g - r).abs().max())
        out["{}x{}".format(b, c)] = res
        print(json.dumps({"{}x{}".format(b, c): res}), flush=True)
    return out


def make_library(a, work):
    """--genomes `.kf` files of k = 7 in --classes clades whose base composition differs, and the `.subtrees` file."""
    import numpy as np
    from kf2vecfsw_amd import counter as C
    from kf2vecfsw_amd import main as M
    shutil.rmtree(work, ignore_errors=True)
    kf = os.path.join(work, "kf")
    os.makedirs(kf)
    nbins = C.num_bins(7)
    rng = np.random.default_rng(23)
    names = ["G%07d" % i for i in range(a.genomes)]
    clades = [i % a.classes for i in range(a.genomes)]
    base = rng.poisson(300, size=(a.classes, nbins))
    counts = np.maximum(1, base[clades] + rng.normal(0, 60, size=(a.genomes, nbins))).astype(np.uint32)
    M.write_kf_files(kf, names, counts, False, False, 16)
    sub = os.path.join(work, "synth.subtrees")
    with open(sub, "w") as f:
        f.write("genome clade\n" + "".join("{} {}\n".format(nm, c) for nm, c in zip(names, clades)))
    return kf, sub, names, clades


def reference_loop(a, dev, kf, names, clades, out_dir):
    """train_classifier_model.py:303-460 restated on the device of this run; seconds for --epochs epochs and the steps."""
    import numpy as np
    import torch
    from kf2vecfsw_amd import classify as CL
    from kf2vecfsw_amd import features as F
    from kf2vecfsw_amd import train as TR
    from kf2vecfsw_amd import train_classifier as TC
    try:
        from sklearn.metrics import accuracy_score
    except ImportError:                                       # the same host work: two copies and a mean of equals
        def accuracy_score(y_true, y_pred):
            return float(np.mean(np.asarray(y_true) == np.asarray(y_pred)[:, 0]))
    os.makedirs(out_dir, exist_ok=True)
    x_host = F.features_from_kf(kf, 7, dev, samples=names, scaler=1e4, dtype=torch.float32).values.cpu()
    clade_input_sorted = np.asarray(clades, dtype=np.int64)
    torch.manual_seed(a.seed)
    model = CL.ClassifierNet(x_host.shape[1], a.hidden, a.classes).to(dev)
    criterion = torch.nn.NLLLoss()
    optimizer = torch.optim.Adam(model.parameters(), lr=a.lr)
    gen = torch.Generator().manual_seed(a.seed)
    plan = TR.batch_plan(len(names), a.batch)
    lowest = float("inf")
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    saves = 0
    for epoch in range(a.epochs):
        perm = torch.randperm(len(names), generator=gen)
        train_loss, running_acc, items = 0.0, 0.0, 0
        for s, e in plan:
            labels = perm[s:e]
            images = x_host.index_select(0, labels).to(dev)
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
            running_acc += accuracy_score(true_class.to("cpu"), top_class.to("cpu")) * images.shape[0]
        train_loss /= items
        if train_loss < lowest:
            lowest = train_loss
            model.to("cpu")
            torch.save(TC.checkpoint_state(x_host.shape[1], a.hidden, a.classes, model.state_dict()),
                       os.path.join(out_dir, "classifier_model.ckpt"))
            model.to(dev)
            saves += 1
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0, a.epochs * len(plan), saves, lowest, running_acc / items


def bench_train(a, dev):
    import glob
    from kf2vecfsw_amd import train as TR
    from kf2vecfsw_amd import train_classifier as TC
    work = a.work_dir
    kf, sub, names, clades = make_library(a, work)
    files = glob.glob(os.path.join(kf, "*.kf"))
    out = {"genomes": a.genomes, "k": 7, "hidden": a.hidden, "classes": a.classes, "batch": a.batch, "epochs": a.epochs,
           "lr": a.lr}

    def run(tag, epochs):
        import torch
        devnull = open(os.devnull, "w")
        stdout, sys.stdout = sys.stdout, devnull
        try:
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            kept = TC.train_classifier_model_func(kf, files, sub, epochs, a.hidden, a.batch, a.lr, 3e-6, 2000, a.seed,
                                                  False, os.path.join(work, tag), device=dev, keep=True)
            torch.cuda.synchronize(dev)
            return time.perf_counter() - t0, kept
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
    out["last_accuracy"] = kept["accuracies"][-1]
    reference_loop(a, dev, kf, names, clades, os.path.join(work, "ref_warm"))    # its warm-up: one full pass
    ref_s, ref_steps, saves, lowest, acc = reference_loop(a, dev, kf, names, clades, os.path.join(work, "ref"))
    out["reference_loop_s"] = round(ref_s, 4)
    out["reference_loop_steps_per_s"] = round(ref_steps / ref_s, 1)
    out["reference_loop_checkpoints"] = saves
    out["reference_loop_lowest_loss"] = lowest
    out["reference_loop_last_accuracy"] = acc
    out["speedup"] = round(out["steps_per_s"] / out["reference_loop_steps_per_s"], 2)
    print(json.dumps({"train": out}), flush=True)
    shutil.rmtree(work, ignore_errors=True)
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", nargs="+", default=["kernel", "train"], choices=["kernel", "train"])
    ap.add_argument("--genomes", type=int, default=850)
    ap.add_argument("--classes", type=int, default=16)
    ap.add_argument("--hidden", type=int, default=2048)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--lr", type=float, default=1e-5)
    ap.add_argument("--seed", type=int, default=28)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--limit", type=int, default=240, help="seconds a part may take")
    ap.add_argument("--work-dir", default="/dev/shm/kf_train_classifier_bench")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:                                               # one part, in this process
        import torch
        dev = torch.device("cuda:0")
        part = {"kernel": bench_kernel, "train": bench_train}[a.child](a, dev)
        print("RESULT " + json.dumps({"device": torch.cuda.get_device_name(0), a.child: part}), flush=True)
        return
    result = {}
    for part in a.parts:                                      # a process and a time limit per part; the first failure ends the run
        argv = [sys.executable, os.path.abspath(__file__), "--child", part] + \
            [x for k in ("genomes", "classes", "hidden", "batch", "epochs", "lr", "seed", "reps", "inner", "work_dir")
             for x in ("--" + k.replace("_", "-"), str(getattr(a, k)))]
        try:
            done = subprocess.run(argv, stdout=subprocess.PIPE, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            raise SystemExit("{}: no result within {} s".format(part, a.limit))
        sys.stdout.write(done.stdout)
        if done.returncode != 0:
            raise SystemExit("{}: exit status {}".format(part, done.returncode))
        result.update(json.loads([ln for ln in done.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]))
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
