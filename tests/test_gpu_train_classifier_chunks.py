"""GPU tests of train_classifier_chunks' loop: everything
train_classifier_chunks.py builds around kf_chunk_features / kf_chunk_features8
and kf_class_loss (the store and the classes lined up by name, the epoch's
permutation and its one run per genome, the uint8 store under -cap, the epoch's
mean and accuracy, the optimiser and its learning rate, the best epoch and its
checkpoint, the table from the full-genome features) against a restatement of
the reference's loop in torch, on a synthetic library
(chunk_classifier_library.py): 21 genomes at k = 3 in three classes.

The runs (hidden 16, seed 28, -lr 1e-5, -lr_min 3e-6, -lr_decay 2000, four
epochs each):
A  batch 21: an epoch is one step of all genomes;
B  batch 5: four steps of five genomes and a last batch of one;
C  batch 4 with -cap: the uint8 store and kf_chunk_features8.

The restatement starts from the trainer's initial parameters and takes the same
permutations and runs (torch.randperm and train_chunks.draw_runs(views=1) on a
generator seeded like the trainer's), then follows the reference's lines
(kf2vec/train_classifier_model_chunks.py:354-497): chunks.range_features_host of
the runs rounded to float32, log_softmax, NLLLoss and backward, Adam with the
schedule, exp, topk and the accuracy.  The bound is the reference's own spread,
as in test_gpu_train_chunks_loop.py: d is the largest difference of an epoch's
loss between that loop in float32 on the device and in float64 on the CPU; the
trainer's losses must stay within 4 d of the float64 loop's, and the weight
matrices after the last epoch within 4 times their own spread.  The accuracies
per epoch equal the float64 loop's; a row is left out of that (and listed) only
where the float64 loop's two largest probabilities are closer than float32
resolves there -- the largest difference of a probability between the float32
loop and the float64 loop in that epoch -- and at most 5 % of a run's rows may
be.  Conditions on the inputs, each asserted: the classes one place off against
the names, and in run C the features without the cap, must each move every
epoch's float64 loss by more than 100 * 4 d.

The figures are printed by test_the_record and written where KF_PARITY_JSON
names a file.  Measured on an MI355X (profiles/r26/train_classifier_chunks_parity.json):
run A  d = 3.0e-06 at losses of 3.0 to 3.9, the kernel path 3.1e-06 from the float64 run: 0.26 of 4 d;
run B  d = 4.1e-06 at losses of 2.9 to 3.9, the kernel path 4.1e-06 from the float64 run: 0.25 of 4 d;
run C  d = 4.8e-03 at losses of 5.3 to 6.8, the kernel path 4.8e-03 from the float64 run: 0.25 of 4 d;
The weight matrices of the float32 loop end 1.9e-08 to 1.9e-05 from the float64 loop's, and the
kernel path's 1.9e-08 to 1.9e-05.  The accuracies agree in every epoch (A: 0.76, 0.81, 0.81, 0.81; B: 0.76, 0.81, 0.81, 0.81; C: 0.76, 0.76, 0.76, 0.76), no rows left out;
the best epochs are 4, 4, 4 in the trainer and 4, 4, 4 in the float64 loop.  The classes one place
off move every epoch's float64 loss by at least 5,761,759 (A), 4,216,384 (B) and 1,523 (C) times
4 d, the features without the cap (C) by 120 times, where 100 times are asked for.
On the CPU, with a float32 CPU loop standing in for the device's and the CPU generator's
draws, the same conditions held at 66,126 times and above before the library was run on
the device.  Run C's d is large on the device's draws: float32 probabilities of its rows
underflow to zero where float64 keeps a tiny gradient that Adam scales up to a full step."""
import contextlib
import glob
import io
import json
import os
import re
import shutil

import numpy as np
import pytest

import chunk_classifier_library

pytestmark = pytest.mark.gpu

EPOCHS, HIDDEN, SEED, CLASSES = 4, 16, 28, 3
LR, LR_MIN, LR_DECAY = 1e-5, 3e-6, 2000
SCALER = 1e4                          # train_classifier_model_chunks.py:68
CKPT = "classifier_model.ckpt"
RUNS = ["A", "B", "C"]
PLAN = {"A": (21, False), "B": (5, False), "C": (4, True)}        # {run: (batch, cap)}


@pytest.fixture(scope="module")
def dev(native):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu tests need an MI355X")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib(native, tmp_path_factory):
    root = tmp_path_factory.mktemp("train_classifier_chunks_lib")
    made = chunk_classifier_library.make(root)
    made["root"] = root
    return made


# ---------------------------------------------------------------------------
# the inputs, read here by name: nothing of features.py or the store
# ---------------------------------------------------------------------------
def read_inputs(lib):
    """The names in the order of the file list, their classes from the `.subtrees` file, their
    window rows back to back with the row of every genome's first, and the full-genome
    features (float(field) * 1e4 rounded to float32)."""
    clade = {}
    with open(lib["subtrees"]) as f:
        for line in f.read().splitlines()[1:]:
            nm, c = line.split(" ")
            clade[nm] = int(c)
    names = [os.path.basename(p)[:-3] for p in lib["files"]]
    windows = []
    for nm in names:
        with open(os.path.join(lib["chunks"], nm + ".kf")) as f:
            windows.append(np.array([[int(float(v)) for v in line.split(",")[1:]] for line in f.read().splitlines()],
                                    dtype=np.uint16))
        assert np.array_equal(windows[-1], lib["rows"][nm])
    row0 = np.cumsum([0] + [w.shape[0] for w in windows]).astype(np.int64)
    full = []
    for nm in names:
        with open(os.path.join(lib["full"], nm + ".kf")) as f:
            cells = f.read().rstrip("\n").split(",")
        assert cells[0] == nm
        full.append([np.float32(float(v) * SCALER) for v in cells[1:]])
    return dict(names=names, classes=np.array([clade[nm] for nm in names], dtype=np.int64),
                windows=np.concatenate(windows), row0=row0, full=np.array(full, dtype=np.float32))


def epoch_draws(inp, device, epochs=EPOCHS):
    """Per epoch (the genomes in the epoch's order, lo, n) as the trainer draws them: a
    generator of `device` seeded with 28, a randperm of the genomes, then draw_runs with one
    view for their window counts in that order; lo counts from the first row of all windows."""
    import torch
    from kf2vecfsw_amd import train_chunks as TC
    gen = torch.Generator(device=device)
    gen.manual_seed(SEED)
    G = len(inp["names"])
    out = []
    for _ in range(epochs):
        order = torch.randperm(G, generator=gen, device=device).cpu().numpy()
        c = np.diff(inp["row0"])[order]
        lo, n = TC.draw_runs(torch.from_numpy(c).to(device), gen, views=1)
        lo, n = lo.cpu().numpy(), n.cpu().numpy()
        assert lo.shape == n.shape == (G, 1) and (n >= 1).all() and (lo >= 0).all() and (lo + n <= c[:, None]).all()
        out.append((order, lo + inp["row0"][order][:, None], n))
    return out


def epoch_features(inp, draws, cap):
    """[G, nbins] float32 per epoch: Dataset_chunks_1row's one view of every genome."""
    from kf2vecfsw_amd import chunks as CH
    return [CH.range_features_host(inp["windows"], lo.reshape(-1), n.reshape(-1), SCALER, 255 if cap else None)
            .astype(np.float32) for _, lo, n in draws]


# ---------------------------------------------------------------------------
# the reference's loop
# ---------------------------------------------------------------------------
def restate(inp, draws, feats, initial, device, dtype, batch, classes=None):
    """kf2vec/train_classifier_model_chunks.py:354-497 from the trainer's initial parameters
    and with its permutations and runs.  Returns a dict: losses and hits per epoch, per epoch
    the probabilities [G, C] (row i the epoch's i-th genome, at its step) and which rows were
    right, and the parameters after the last epoch.  classes: others than the inputs' own."""
    import torch
    from kf2vecfsw_amd import classify as CL
    classes = inp["classes"] if classes is None else classes
    input_size = feats[0].shape[1]
    model = CL.ClassifierNet(input_size, HIDDEN, CLASSES)
    model.load_state_dict(initial)
    model = model.to(device=device, dtype=dtype)
    criterion = torch.nn.NLLLoss()
    optimizer = torch.optim.Adam(model.parameters(), lr=LR)
    G = len(inp["names"])
    losses, hits, probs, right = [], [], [], []
    for epoch, ((order, _, _), z) in enumerate(zip(draws, feats)):
        model.train()
        train_loss, running, items_count, ps_all, right_all = 0.0, 0.0, 0, [], []
        for a in range(0, G, batch):
            labels = order[a: a + batch]
            images = torch.from_numpy(z[a: a + labels.shape[0]]).reshape(-1, input_size).to(device)
            true_class = torch.from_numpy(classes[np.ix_(list(labels))]).to(device)
            model_class = torch.nn.functional.log_softmax(model(images.to(dtype)), dim=1)
            loss = criterion(model_class, true_class)
            train_loss += loss.item() * images.shape[0]
            items_count += images.shape[0]
            optimizer.zero_grad()
            loss.backward()
            optimizer.step()
            ps = torch.exp(model_class.detach())
            _, top_class = ps.topk(1, dim=1)
            ok = (top_class[:, 0].cpu() == true_class.cpu()).numpy()
            running += float(ok.mean()) * images.shape[0]
            ps_all.append(ps.cpu().to(torch.float64).numpy())
            right_all.append(ok)
        losses.append(train_loss / items_count)
        hits.append(running / items_count)
        probs.append(np.concatenate(ps_all))
        right.append(np.concatenate(right_all))
        if epoch % 100 == 0:
            new_lr = LR_MIN + LR * (0.1 ** (epoch / LR_DECAY))
            for group in optimizer.param_groups:
                group["lr"] = new_lr
    state = {k: v.detach().to("cpu", torch.float64).numpy() for k, v in model.state_dict().items()}
    return dict(losses=losses, accuracies=hits, probs=probs, right=right, state=state)


# ---------------------------------------------------------------------------
# the runs
# ---------------------------------------------------------------------------
def train(dev, lib, out, batch, cap, epochs=EPOCHS, chunks=None, full=None, files=None, subtrees=None):
    """train_classifier_model_chunks_func; (kept, stdout)."""
    from kf2vecfsw_amd import train_classifier_chunks as TCC
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        kept = TCC.train_classifier_model_chunks_func(chunks or lib["chunks"], full or lib["full"], files or lib["files"],
                                                      subtrees or lib["subtrees"], epochs, HIDDEN, batch, LR, LR_MIN,
                                                      LR_DECAY, SEED, False, cap, out, device=dev, keep=True)
    return kept, buf.getvalue()


def load_state(path):
    import torch
    return {k: v.numpy() for k, v in torch.load(path, map_location="cpu", weights_only=True)["state_dict"].items()}


def numpy_state(state):
    return {k: v.detach().cpu().numpy() for k, v in state.items()}


def same_state(a, b):
    """Tensor for tensor, bit for bit."""
    return list(a) == list(b) and all(a[k].dtype == b[k].dtype == np.float32 and a[k].shape == b[k].shape and
                                      np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in a)


def tensor_distances(a, b):
    assert list(a) == list(b)
    return {k: float(np.abs(a[k].astype(np.float64) - b[k].astype(np.float64)).max()) for k in a}


def uncertain_rows(r32, r64):
    """Per epoch the rows (positions in the epoch's order) at which the float64 loop's two
    largest probabilities are no further apart than float32 resolves there: the largest
    difference of a probability between the float32 and the float64 loop in that epoch."""
    out = []
    for p32, p64 in zip(r32["probs"], r64["probs"]):
        res = float(np.abs(p32 - p64).max())
        srt = np.sort(p64, axis=1)
        out.append(np.nonzero(srt[:, -1] - srt[:, -2] <= res)[0])
    return out


def accuracy_check(mine, r32, r64, G):
    """(ok, the rows left out as (epoch, position) pairs): per epoch the trainer's hits are the
    float64 loop's over the rows that are not left out, plus any number of those that are."""
    left, ok = [], True
    for e, rows in enumerate(uncertain_rows(r32, r64)):
        left += [(e, int(i)) for i in rows]
        sure = int(np.delete(r64["right"][e], rows).sum())
        got = mine[e] * G
        ok = ok and abs(got - round(got)) < 1e-9 and sure <= round(got) <= sure + len(rows)
    return ok, left


_CASES = {}
_SHARED = {}


def shared(dev, lib):
    """The inputs and the epochs' draws, made once: the draws do not depend on the batch."""
    if not _SHARED:
        inp = read_inputs(lib)
        draws = epoch_draws(inp, dev)
        _SHARED.update(inp=inp, draws=draws, feats={cap: epoch_features(inp, draws, cap) for cap in (False, True)})
    return _SHARED


def case(dev, lib, run):
    """A run through the trainer and the restatements on its inputs, made once."""
    import torch
    if run in _CASES:
        return _CASES[run]
    batch, cap = PLAN[run]
    out = str(lib["root"] / "models_{}".format(run))
    kept, said = train(dev, lib, out, batch, cap)
    sh = shared(dev, lib)
    inp, draws, feats = sh["inp"], sh["draws"], sh["feats"][cap]
    initial = kept["initial"]
    cpu = torch.device("cpu")
    c = dict(run=run, out=out, kept=kept, log=said, batch=batch, cap=cap, inp=inp)
    c["r32"] = restate(inp, draws, feats, initial, dev, torch.float32, batch)
    c["r64"] = restate(inp, draws, feats, initial, cpu, torch.float64, batch)
    c["shifted"] = restate(inp, draws, feats, initial, cpu, torch.float64, batch, classes=np.roll(inp["classes"], 1))
    if cap:
        c["uncapped"] = restate(inp, draws, sh["feats"][False], initial, cpu, torch.float64, batch)
    c["last"] = numpy_state(kept["states"][-1])
    _CASES[run] = c
    return c


def spread(mine, l32, l64):
    """(d, the kernel path's distance from the float64 loop)."""
    assert len(mine) == len(l32) == len(l64) == EPOCHS
    return max(abs(a - b) for a, b in zip(l32, l64)), max(abs(a - b) for a, b in zip(mine, l64))


VARIANTS = [("A", "shifted", "the classes one place off against the names"),
            ("B", "shifted", "the classes one place off against the names"),
            ("C", "shifted", "the classes one place off against the names"),
            ("C", "uncapped", "the features without the cap")]


def test_the_record(dev, lib):
    """The figures of every run, printed, and written where KF_PARITY_JSON names a file.
    Measured on an MI355X (profiles/r26/train_classifier_chunks_parity.json): see the README's
    train_classifier_chunks paragraph for the numbers."""
    record = {"genomes": lib["G"], "classes": CLASSES, "hidden": HIDDEN, "epochs": EPOCHS, "lr": LR, "runs": {}}
    for run in RUNS:
        c = case(dev, lib, run)
        k = c["kept"]
        d, mine = spread(k["losses"], c["r32"]["losses"], c["r64"]["losses"])
        ok, left = accuracy_check(k["accuracies"], c["r32"], c["r64"], lib["G"])
        r = {"batch": c["batch"], "cap": c["cap"], "d": d, "kernel_path": mine,
             "losses_kernel_path": k["losses"], "losses_float32": c["r32"]["losses"], "losses_float64": c["r64"]["losses"],
             "accuracies_kernel_path": k["accuracies"], "accuracies_float32": c["r32"]["accuracies"],
             "accuracies_float64": c["r64"]["accuracies"], "accuracies_agree": ok, "rows_left_out": left,
             "parameters_float32_by_tensor": tensor_distances(c["r32"]["state"], c["r64"]["state"]),
             "parameters_kernel_path_by_tensor": tensor_distances(c["last"], c["r64"]["state"]),
             "best_epoch_kernel_path": k["best_epoch"] + 1,
             "best_epoch_float64": 1 + c["r64"]["losses"].index(min(c["r64"]["losses"]))}
        for key in ("shifted", "uncapped"):
            if key in c:
                moved = min(abs(a - b) for a, b in zip(c[key]["losses"], c["r64"]["losses"]))
                r["losses_float64_" + key] = c[key]["losses"]
                r["sensitivity_ratio_" + key] = moved / (4 * d) if d else None
        record["runs"][run] = r
    print(json.dumps(record, indent=1))
    path = os.environ.get("KF_PARITY_JSON")
    if path:
        with open(path, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")


def test_the_inputs_are_what_the_runs_need(dev, lib):
    G = lib["G"]
    sh = shared(dev, lib)
    inp = sh["inp"]
    assert G == 21 == len(inp["names"]) and inp["full"].shape == (G, 32) and G % 5 == 1 and G % 4 == 1
    assert sorted(set(inp["classes"].tolist())) == [0, 1, 2]
    n_windows = np.diff(inp["row0"])
    assert n_windows.min() == 1 and n_windows.max() == 12
    assert inp["windows"].max() > 255 and (inp["windows"] > 255).mean() > 0.2          # counts above 255 are there
    by_class = sorted(inp["names"], key=lambda nm: (lib["clade"][nm], nm))
    assert inp["names"] != sorted(inp["names"]) and inp["names"] != lib["subtree_order"] != sorted(inp["names"])
    assert inp["names"] != by_class
    # the runs differ from epoch to epoch, and the cap changes the features
    draws, feats = sh["draws"], sh["feats"]
    assert not np.array_equal(draws[0][0], draws[1][0]) and any(n.max() > 1 for _, _, n in draws)
    assert not np.array_equal(feats[False][0], feats[True][0])


@pytest.mark.parametrize("run", RUNS)
def test_train_loss_against_a_restatement_of_the_references_loop(dev, lib, run):
    c = case(dev, lib, run)
    k = c["kept"]
    steps = re.findall(r"Epoch \[(\d)/4\], Step \[(\d+)/(\d+)\], Train loss: (\d+\.\d{20}), (\d\.\d{20}), Time: ", c["log"])
    n = -(-lib["G"] // c["batch"])
    assert [(int(e), int(a), int(b)) for e, a, b, _, _ in steps] == [(e + 1, n, n) for e in range(EPOCHS)]
    assert n == {"A": 1, "B": 5, "C": 6}[run]
    assert [float(v) for _, _, _, v, _ in steps] == k["losses"]                 # the logged losses are the kept ones
    assert [float(v) for _, _, _, _, v in steps] == k["accuracies"]
    assert "Cap kmer frequencies: {}\n".format(c["cap"]) in c["log"]
    l32, l64 = c["r32"]["losses"], c["r64"]["losses"]
    d, mine = spread(k["losses"], l32, l64)
    print("run {}: losses: kernel path {}, float32 loop {}, float64 loop {}".format(run, k["losses"], l32, l64))
    print("run {}: d = {!r}; the kernel path differs from the float64 run by {!r}: {:.3f} of 4 d".format(
        run, d, mine, mine / (4 * d) if d else float("inf")))
    assert mine <= 4 * d


@pytest.mark.parametrize("run", RUNS)
def test_accuracies_against_the_float64_loop(dev, lib, run):
    c = case(dev, lib, run)
    k = c["kept"]
    ok, left = accuracy_check(k["accuracies"], c["r32"], c["r64"], lib["G"])
    print("run {}: accuracies: kernel path {}, float32 loop {}, float64 loop {}; rows left out (epoch, position): {}".format(
        run, k["accuracies"], c["r32"]["accuracies"], c["r64"]["accuracies"], left))
    assert len(left) <= 0.05 * EPOCHS * lib["G"], left
    assert ok


WEIGHTS = ("fc1.weight", "fc3.weight")


@pytest.mark.parametrize("run", RUNS)
def test_weight_matrices_after_the_last_epoch(dev, lib, run):
    """The parameters after the last epoch against the float64 loop's: each weight matrix no
    further than 4 times the float32 loop's is."""
    c = case(dev, lib, run)
    d32, mine = tensor_distances(c["r32"]["state"], c["r64"]["state"]), tensor_distances(c["last"], c["r64"]["state"])
    for k in d32:
        print("run {}: {}: the float32 loop is {!r} from the float64 loop, the kernel path {!r}: {:.3f} of 4 times".format(
            run, k, d32[k], mine[k], mine[k] / (4 * d32[k]) if d32[k] else float("inf")))
    for k in WEIGHTS:
        assert mine[k] <= 4 * d32[k], k


@pytest.mark.parametrize("run,key,what", VARIANTS, ids=["{}-{}".format(v[0], v[1]) for v in VARIANTS])
def test_a_wrong_loop_would_show(dev, lib, run, key, what):
    """A condition on the inputs, not on the trainer: the float64 loop with this one thing
    wrong must move every epoch's loss by more than 100 times the 4 d the kernel path is
    allowed."""
    c = case(dev, lib, run)
    d, _ = spread(c["kept"]["losses"], c["r32"]["losses"], c["r64"]["losses"])
    moved = min(abs(a - b) for a, b in zip(c[key]["losses"], c["r64"]["losses"]))
    print("run {}: {} moves an epoch's loss by at least {!r}: {:.1f} times 4 d".format(
        run, what, moved, moved / (4 * d) if d else float("inf")))
    assert moved > 100 * 4 * d, "these inputs cannot tell: the smallest move {!r} is not above 100 * 4 d = {!r}".format(
        moved, 400 * d)


@pytest.mark.parametrize("run", RUNS)
def test_best_epoch_and_its_checkpoint(dev, lib, run):
    from kf2vecfsw_amd import classify as CL
    c = case(dev, lib, run)
    k = c["kept"]
    losses = k["losses"]
    assert k["best_epoch"] == losses.index(min(losses)) and k["lowest_loss"] == min(losses)
    assert k["highest_accuracy"] == k["accuracies"][k["best_epoch"]]
    best = re.findall(r"Best Epoch \[(\d)/4\], Lowest loss: (\d+\.\d{20}), Highest accuracy: (\d\.\d{20})\n", c["log"])
    assert len(best) == 1 and int(best[0][0]) == k["best_epoch"] + 1 and float(best[0][1]) == min(losses)
    assert float(best[0][2]) == k["highest_accuracy"]
    states = [numpy_state(s) for s in k["states"]]
    assert len(states) == EPOCHS
    for i in range(EPOCHS):
        for j in range(i):
            assert not same_state(states[i], states[j]), (i, j)
    assert not same_state(states[0], numpy_state(k["initial"]))
    assert same_state(load_state(os.path.join(c["out"], CKPT)), states[k["best_epoch"]])
    model = CL.load_classifier(c["out"], dev)                                # classify's own loader takes the checkpoint
    assert (model.fc1.in_features, model.fc1.out_features, model.fc3.out_features) == (32, HIDDEN, CLASSES)
    logs = [f for f in os.listdir(c["out"]) if re.fullmatch(r"train_classifier_\d{8}_\d{6}\.log", f)]
    assert len(logs) == 1 and open(os.path.join(c["out"], logs[0])).read() == c["log"]
    assert sorted(os.listdir(c["out"])) == sorted(logs + [CKPT, "backbone_classes.out"])


def read_table(path):
    data = open(path, "rb").read()
    assert data.endswith(b"\n") and b"\r" not in data
    return [[cell.decode() for cell in ln.split(b"\t")] for ln in data[:-1].split(b"\n")]


@pytest.mark.parametrize("run", ["B", "C"])
def test_backbone_classes_are_the_best_model_on_the_full_genome_features(dev, lib, run):
    import torch
    from kf2vecfsw_amd import classify as CL
    c = case(dev, lib, run)
    k, out, names = c["kept"], c["out"], c["inp"]["names"]
    assert k["names"] == names and k["classes"] == c["inp"]["classes"].tolist()
    model = CL.load_classifier(out, dev)
    with torch.no_grad():
        probs, top = CL.class_probs(model(torch.from_numpy(c["inp"]["full"]).to(dev)))
    probs, top = probs.cpu().numpy(), top.cpu().numpy()
    assert probs.dtype == np.float32 and probs.shape == (lib["G"], 1 + CLASSES)
    assert np.array_equal(k["probabilities"].numpy().view(np.uint32), probs.view(np.uint32))
    rows = read_table(os.path.join(out, "backbone_classes.out"))
    assert rows[0] == ["genome", "true_class", "top_class", "top_p", "0", "1", "2"]
    assert [r[0] for r in rows[1:]] == names and all(len(r) == 4 + CLASSES for r in rows[1:])
    assert [r[1] for r in rows[1:]] == [str(int(v)) for v in c["inp"]["classes"]]
    assert [r[2] for r in rows[1:]] == ["{}.0".format(int(t)) for t in top]
    parsed = np.array([[np.float32(float(v)) for v in r[3:]] for r in rows[1:]], dtype=np.float32)
    assert np.array_equal(parsed.view(np.uint32), probs.view(np.uint32))
    assert "Dimensions of class output rows:{} cols:{}\n".format(lib["G"], CLASSES + 4) in c["log"]


def test_the_command_writes_the_same_files(dev, lib, capsys):
    """`train_classifier_chunks` in this process, two epochs in batches of 5 with -cap, against
    train_classifier_model_chunks_func with the same arguments and the file list the command globs."""
    from kf2vecfsw_amd import main as M
    out_f, out_c = str(lib["root"] / "models_func2"), str(lib["root"] / "models_cli2")
    order = glob.glob(os.path.join(lib["chunks"], "*.kf"))
    assert len(order) == lib["G"]
    train(dev, lib, out_f, 5, True, epochs=2, files=order)
    capsys.readouterr()
    M.main(["train_classifier_chunks", "-input_dir", lib["chunks"], "-input_dir_fullgenomes", lib["full"], "-subtrees",
            lib["subtrees"], "-e", "2", "-hidden_sz", str(HIDDEN), "-batch_sz", "5", "-lr", str(LR), "-cap", "-o", out_c,
            "-device", str(dev)])
    said = capsys.readouterr().out
    assert said.startswith("Running train_classifier_chunks\n") and "Cap kmer frequencies: True\n" in said
    assert len(re.findall(r"Train loss: ", said)) == 2
    assert same_state(load_state(os.path.join(out_c, CKPT)), load_state(os.path.join(out_f, CKPT)))
    assert open(os.path.join(out_c, "backbone_classes.out"), "rb").read() == \
        open(os.path.join(out_f, "backbone_classes.out"), "rb").read()
    assert sorted(f for f in os.listdir(out_c) if not f.endswith(".log")) == sorted([CKPT, "backbone_classes.out"])


def test_an_empty_chunk_file_is_refused_by_name(dev, lib):
    bad = lib["root"] / "chunks_one_empty"
    shutil.copytree(lib["chunks"], str(bad))
    victim = lib["names"][2]
    (bad / (victim + ".kf")).write_bytes(b"")
    out = str(lib["root"] / "models_empty")
    files = [os.path.join(str(bad), os.path.basename(p)) for p in lib["files"]]
    for cap in (False, True):
        with pytest.raises(ValueError, match=re.escape(os.path.join(str(bad), victim + ".kf"))) as e:
            train(dev, lib, out, 5, cap, chunks=str(bad), files=files)
        assert "no window row" in str(e.value)
        assert not os.path.exists(os.path.join(out, CKPT))


def test_a_genome_without_a_full_genome_file_is_refused_by_name(dev, lib):
    bad = lib["root"] / "full_one_missing"
    shutil.copytree(lib["full"], str(bad))
    victim = lib["names"][4]
    os.remove(str(bad / (victim + ".kf")))
    out = str(lib["root"] / "models_missing")
    with pytest.raises(ValueError, match=re.escape(os.path.join(str(bad), victim + ".kf"))):
        train(dev, lib, out, 5, False, full=str(bad))
    assert not os.path.exists(os.path.join(out, CKPT))


def test_a_genome_absent_from_the_subtrees_file_is_refused_by_name(dev, lib):
    victim = lib["names"][6]
    short = lib["root"] / "short.subtrees"
    short.write_text("".join(ln for ln in open(lib["subtrees"]) if not ln.startswith(victim + " ")))
    out = str(lib["root"] / "models_absent")
    with pytest.raises(ValueError) as e:
        train(dev, lib, out, 5, False, subtrees=str(short))
    assert victim in str(e.value) and str(short) in str(e.value)
    assert not os.path.exists(os.path.join(out, CKPT))
