"""GPU tests of train_model_set_chunks' loop: everything train_chunks.py builds
around kf_chunk_features and kf_dist_loss_views (the store and the matrix lined
up by name, the epoch's permutation and runs, the two views side by side and
their labels interleaved, the weight's 1000, the epoch's mean, the optimiser and
its learning rate, the best epoch and its checkpoint, the tables from the
full-genome features) against a restatement of the reference's loop in torch,
on a synthetic library (chunk_train_library.py) whose big clade has S / 2 + 5
genomes, S = kf_dist_loss_small_b(): a batch of all of them is on the tiled path.

The runs (clade 7, k = 3, hidden 16, embed 8, seed 28, -lr 1e-5, -lr_min 3e-6,
-lr_decay 2000, four epochs each; G = 21 genomes today):
A  batch G: an epoch is one step of 2 G rows on the tiled path;
B  batch 5: four steps of ten rows and a last batch of one genome, two rows;
C  batch 4 with -cap: window counts capped at 255.

The restatement starts from the trainer's initial parameters and takes the same
permutations and runs (torch.randperm and train_chunks.draw_runs on a generator
seeded like the trainer's), then follows the reference's lines:
chunks.range_features_host of the runs rounded to float32, repeat_interleave of
the labels, cdist, Loss_chunks, Adam with the schedule.  The bound is the
reference's own spread, as in test_gpu_train_loop.py: d is the largest
difference of an epoch's loss between that loop in float32 on the device and in
float64 on the CPU; the trainer's losses must stay within 4 d of the float64
loop's, and the weight matrices after the last epoch within 4 times their own
spread.  Conditions on the inputs, each asserted: the matrix rolled one place
against the names, eps = 1e-6 in place of 1000, and labels tiled instead of
interleaved must each move every epoch's float64 loss by more than 100 * 4 d.

The figures are printed by test_the_record and written where KF_PARITY_JSON
names a file.  Measured on an MI355X (profiles/r25/train_chunks_parity.json):
run A  d = 6.3e-06 at losses of 54.2 to 54.9, the kernel path 7.3e-06 from the
       float64 run: 0.29 of 4 d;
run B  d = 5.2e-06 at losses of 42.7 to 49.2, the kernel path 5.3e-06: 0.25 of 4 d;
run C  d = 1.1e-06 at losses of 9.1 to 14.6, the kernel path 1.3e-06: 0.30 of 4 d.
The weight matrices of the float32 loop end 1.7e-08 to 6.8e-08 from the float64
loop's, and the kernel path's at the same distances to every digit.  The best
epochs are 4, 1 and 2 in the trainer and in the float64 loop.  The matrix one
place off moves every epoch's float64 loss by at least 86,459 (A), 141,654 (B)
and 247,358 (C) times 4 d, labels tiled by 83,183, 398,185 and 599,060 times,
eps = 1e-6 by more than 8e10 times, where 100 times are asked for.  On the CPU,
with a float32 CPU loop standing in for the device's, the same conditions held
at 147,659 (A, rolled) and above before the library was run on the device."""
import contextlib
import io
import json
import os
import re
import shutil

import numpy as np
import pytest

import chunk_train_library

pytestmark = pytest.mark.gpu

CLADE = chunk_train_library.BIG
EPOCHS, HIDDEN, EMBED, SEED = 4, 16, 8, 28
LR, LR_MIN, LR_DECAY = 1e-5, 3e-6, 2000
SCALER = 1e4                          # train_model_set_chunks.py:59
CKPT = "model_subtree_{}.ckpt".format(CLADE)
RUNS = ["A", "B", "C"]


@pytest.fixture(scope="module")
def dev(native):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu tests need an MI355X")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib(native, tmp_path_factory):
    root = tmp_path_factory.mktemp("train_chunks_lib")
    made = chunk_train_library.make(root)
    made["root"] = root
    return made


def run_plan(lib):
    """{run: (batch, cap)}."""
    return {"A": (lib["G"], False), "B": (5, False), "C": (4, True)}


# ---------------------------------------------------------------------------
# the inputs, read here by name: nothing of tables.py, features.py or the store
# ---------------------------------------------------------------------------
def read_inputs(lib):
    """The clade's names in the order of the file list, their window rows back to back with
    the row of every genome's first, the full-genome features (float(field) * 1e4 rounded to
    float32) and the true distances reordered by name."""
    members = set()
    with open(lib["subtrees"]) as f:
        for line in f.read().splitlines()[1:]:
            nm, c = line.split(" ")
            if int(c) == CLADE:
                members.add(nm)
    names = [os.path.basename(p)[:-3] for p in lib["files"] if os.path.basename(p)[:-3] in members]
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
    with open(os.path.join(lib["dist"], "x_subtree_{}.di_mtrx".format(CLADE))) as f:
        lines = f.read().splitlines()
    head = lines[0].split("\t")[1:]
    by_name = {}
    for line in lines[1:]:
        cells = line.split("\t")
        by_name[cells[0]] = dict(zip(head, (float(v) for v in cells[1:])))
    P = np.array([[by_name[a][b] for b in names] for a in names], dtype=np.float64)
    return dict(names=names, windows=np.concatenate(windows), row0=row0, full=np.array(full, dtype=np.float32), P=P)


def epoch_draws(inp, device, epochs=EPOCHS):
    """Per epoch (the genomes in the epoch's order, lo, n) as the trainer draws them: a
    generator of `device` seeded with 28, a randperm of the genomes, then draw_runs for
    their window counts in that order; lo counts from the first row of all windows."""
    import torch
    from kf2vecfsw_amd import train_chunks as TC
    gen = torch.Generator(device=device)
    gen.manual_seed(SEED)
    G = len(inp["names"])
    out = []
    for _ in range(epochs):
        order = torch.randperm(G, generator=gen, device=device).cpu().numpy()
        c = np.diff(inp["row0"])[order]
        lo, n = TC.draw_runs(torch.from_numpy(c).to(device), gen)
        lo, n = lo.cpu().numpy(), n.cpu().numpy()
        assert lo.shape == n.shape == (G, 2) and (n >= 1).all() and (lo >= 0).all() and (lo + n <= c[:, None]).all()
        out.append((order, lo + inp["row0"][order][:, None], n))
    return out


def epoch_features(inp, draws, cap):
    """[2 G, nbins] float32 per epoch: Dataset_chunks_2rows' two views of every genome, side by side."""
    from kf2vecfsw_amd import chunks as CH
    return [CH.range_features_host(inp["windows"], lo.reshape(-1), n.reshape(-1), SCALER, 255 if cap else None)
            .astype(np.float32) for _, lo, n in draws]


# ---------------------------------------------------------------------------
# the reference's loop
# ---------------------------------------------------------------------------
def weighted_loss(model_dist, true_dist, eps=1000):
    """losses.Loss_chunks (kf2vec/losses.py:58-117)."""
    import torch
    assert model_dist.shape == true_dist.shape
    weight = 1 / (true_dist + eps)
    root = torch.sqrt(true_dist)
    return ((model_dist - root) ** 2 * weight).mean()


def restate(inp, draws, feats, initial, device, dtype, batch, P=None, eps=1000, tiled=False):
    """kf2vec/train_model_set_chunks.py:380-558 from the trainer's initial parameters and with
    its permutations and runs: (train loss per epoch, the parameters after the last epoch).
    P: another matrix than the inputs' own; eps: another weight; tiled: labels.repeat(2) in
    place of repeat_interleave."""
    import torch
    from kf2vecfsw_amd import query as Q
    P = inp["P"] if P is None else P
    input_size = feats[0].shape[1]
    model = Q.QueryNet(input_size, HIDDEN, EMBED)
    model.load_state_dict(initial)
    model = model.to(device=device, dtype=dtype)
    optimizer = torch.optim.Adam(model.parameters(), lr=LR)
    G = len(inp["names"])
    losses = []
    for epoch, ((order, _, _), z) in enumerate(zip(draws, feats)):
        model.train()
        train_loss, items_count = 0.0, 0
        for a in range(0, G, batch):
            labels = torch.from_numpy(order[a: a + batch])
            b = labels.shape[0]
            images = torch.from_numpy(z[2 * a: 2 * (a + b)]).reshape(-1, input_size).to(device)
            labels = labels.repeat(2) if tiled else torch.repeat_interleave(labels, 2, dim=0)
            lab = labels.numpy()
            real_dist = torch.from_numpy(P[np.ix_(lab, lab)]).to(device)
            outputs = model(images.to(dtype))
            train_dist = torch.cdist(outputs, outputs, p=2, compute_mode="donot_use_mm_for_euclid_dist")
            loss = weighted_loss(train_dist, real_dist, eps)
            batch_elmts = images.shape[0] / 2
            train_loss += loss.item() * batch_elmts
            items_count += batch_elmts
            optimizer.zero_grad()
            loss.backward()
            optimizer.step()
        losses.append(train_loss / items_count)
        if epoch % 100 == 0:
            new_lr = LR_MIN + LR * (0.1 ** (epoch / LR_DECAY))
            for group in optimizer.param_groups:
                group["lr"] = new_lr
    state = {k: v.detach().to("cpu", torch.float64).numpy() for k, v in model.state_dict().items()}
    return losses, state


# ---------------------------------------------------------------------------
# the runs
# ---------------------------------------------------------------------------
def train(dev, lib, out, batch, cap, epochs=EPOCHS, chunks=None, full=None, files=None):
    """train_model_set_chunks_func on the clade; (kept, stdout)."""
    from kf2vecfsw_amd import train_chunks as TC
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        kept = TC.train_model_set_chunks_func(chunks or lib["chunks"], full or lib["full"], files or lib["files"],
                                              lib["subtrees"], lib["dist"], epochs, HIDDEN, EMBED, batch, LR, LR_MIN,
                                              LR_DECAY, [CLADE], SEED, cap, out, device=dev, keep=True)
    assert len(kept) == 1 and kept[0]["clade"] == CLADE
    return kept[0], buf.getvalue()


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
    batch, cap = run_plan(lib)[run]
    out = str(lib["root"] / "models_{}".format(run))
    kept, said = train(dev, lib, out, batch, cap)
    sh = shared(dev, lib)
    inp, draws, feats = sh["inp"], sh["draws"], sh["feats"][cap]
    initial = kept["initial"]
    cpu = torch.device("cpu")
    c = dict(run=run, out=out, kept=kept, log=said, batch=batch, cap=cap, inp=inp)
    c["l32"], c["p32"] = restate(inp, draws, feats, initial, dev, torch.float32, batch)
    c["l64"], c["p64"] = restate(inp, draws, feats, initial, cpu, torch.float64, batch)
    c["rolled"], _ = restate(inp, draws, feats, initial, cpu, torch.float64, batch, P=np.roll(inp["P"], 1, axis=(0, 1)))
    c["eps"], _ = restate(inp, draws, feats, initial, cpu, torch.float64, batch, eps=1e-6)
    c["tiled"], _ = restate(inp, draws, feats, initial, cpu, torch.float64, batch, tiled=True)
    c["last"] = numpy_state(kept["states"][-1])
    _CASES[run] = c
    return c


def spread(mine, l32, l64):
    """(d, the kernel path's distance from the float64 loop)."""
    assert len(mine) == len(l32) == len(l64) == EPOCHS
    return max(abs(a - b) for a, b in zip(l32, l64)), max(abs(a - b) for a, b in zip(mine, l64))


VARIANTS = [("rolled", "the matrix one place off against the names"), ("eps", "eps = 1e-6 in place of 1000"),
            ("tiled", "labels tiled instead of interleaved")]


def test_the_record(dev, lib):
    """The figures of every run, printed, and written where KF_PARITY_JSON names a file."""
    record = {"genomes": lib["G"], "small_b": lib["S"], "hidden": HIDDEN, "embed": EMBED, "epochs": EPOCHS, "lr": LR,
              "runs": {}}
    for run in RUNS:
        c = case(dev, lib, run)
        d, mine = spread(c["kept"]["losses"], c["l32"], c["l64"])
        r = {"batch": c["batch"], "cap": c["cap"], "d": d, "kernel_path": mine,
             "losses_kernel_path": c["kept"]["losses"], "losses_float32": c["l32"], "losses_float64": c["l64"],
             "parameters_float32_by_tensor": tensor_distances(c["p32"], c["p64"]),
             "parameters_kernel_path_by_tensor": tensor_distances(c["last"], c["p64"]),
             "best_epoch_kernel_path": c["kept"]["best_epoch"] + 1,
             "best_epoch_float64": 1 + c["l64"].index(min(c["l64"]))}
        for key, _ in VARIANTS:
            moved = min(abs(a - b) for a, b in zip(c[key], c["l64"]))
            r["losses_float64_" + key] = c[key]
            r["sensitivity_ratio_" + key] = moved / (4 * d) if d else None
        record["runs"][run] = r
    print(json.dumps(record, indent=1))
    path = os.environ.get("KF_PARITY_JSON")
    if path:
        with open(path, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")


def test_the_inputs_are_what_the_runs_need(dev, lib):
    S, G = lib["S"], lib["G"]
    inp = shared(dev, lib)["inp"]
    assert G == S // 2 + 5 == len(inp["names"]) and inp["full"].shape == (G, 32) and inp["P"].shape == (G, G)
    assert 2 * G > S and 2 * 5 <= S and G % 5 == 1 and G % 4 == 1       # A is tiled; B and C are not, and leave one genome
    n_windows = np.diff(inp["row0"])
    assert n_windows.min() == 1 and n_windows.max() == 12 and inp["windows"].max() > 255
    P = inp["P"]
    assert np.array_equal(P, P.T) and not np.diagonal(P).any()
    off = P[np.triu_indices(G, 1)]
    assert np.unique(off).size == off.size and off.min() > 50 and off.max() < 3000
    assert inp["names"] != sorted(inp["names"]) and inp["names"] != lib["matrix_order"][CLADE]
    # the runs differ from epoch to epoch, and the cap changes the features
    draws, feats = shared(dev, lib)["draws"], shared(dev, lib)["feats"]
    assert not np.array_equal(draws[0][0], draws[1][0]) and any(n.max() > 1 for _, _, n in draws)
    assert not np.array_equal(feats[False][0], feats[True][0])


@pytest.mark.parametrize("run", RUNS)
def test_train_loss_against_a_restatement_of_the_references_loop(dev, lib, run):
    c = case(dev, lib, run)
    k = c["kept"]
    steps = re.findall(r"Epoch \[(\d)/4\], Step \[(\d+)/(\d+)\], Train loss: (\d+\.\d{20}), Time: ", c["log"])
    n = -(-lib["G"] // c["batch"])
    assert [(int(e), int(a), int(b)) for e, a, b, _ in steps] == [(e + 1, n, n) for e in range(EPOCHS)]
    assert n == {"A": 1, "B": 5, "C": 6}[run] and [len(s) for s in k["step_losses"]] == [n] * EPOCHS
    assert [float(v) for _, _, _, v in steps] == k["losses"]                   # the logged losses are the kept ones
    d, mine = spread(k["losses"], c["l32"], c["l64"])
    print("run {}: losses: kernel path {}, float32 loop {}, float64 loop {}".format(run, k["losses"], c["l32"], c["l64"]))
    print("run {}: d = {!r}; the kernel path differs from the float64 run by {!r}: {:.3f} of 4 d".format(
        run, d, mine, mine / (4 * d) if d else float("inf")))
    assert mine <= 4 * d


WEIGHTS = ("fc1.weight", "fc2.weight")


@pytest.mark.parametrize("run", RUNS)
def test_weight_matrices_after_the_last_epoch(dev, lib, run):
    """The parameters after the last epoch against the float64 loop's: each weight matrix no
    further than 4 times the float32 loop's is (test_gpu_train_loop.py has why the biases,
    whose exact gradients are zero, are not held to it)."""
    c = case(dev, lib, run)
    d32, mine = tensor_distances(c["p32"], c["p64"]), tensor_distances(c["last"], c["p64"])
    for k in d32:
        print("run {}: {}: the float32 loop is {!r} from the float64 loop, the kernel path {!r}: {:.3f} of 4 times".format(
            run, k, d32[k], mine[k], mine[k] / (4 * d32[k]) if d32[k] else float("inf")))
    for k in WEIGHTS:
        assert mine[k] <= 4 * d32[k], k


@pytest.mark.parametrize("run", RUNS)
@pytest.mark.parametrize("key,what", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_a_wrong_loop_would_show(dev, lib, run, key, what):
    """A condition on the inputs, not on the trainer: the float64 loop with this one thing
    wrong must move every epoch's loss by more than 100 times the 4 d the kernel path is
    allowed."""
    c = case(dev, lib, run)
    d, _ = spread(c["kept"]["losses"], c["l32"], c["l64"])
    moved = min(abs(a - b) for a, b in zip(c[key], c["l64"]))
    print("run {}: {} moves an epoch's loss by at least {!r}: {:.1f} times 4 d".format(
        run, what, moved, moved / (4 * d) if d else float("inf")))
    assert moved > 100 * 4 * d, "these inputs cannot tell: the smallest move {!r} is not above 100 * 4 d = {!r}".format(
        moved, 400 * d)


@pytest.mark.parametrize("run", RUNS)
def test_best_epoch_and_its_checkpoint(dev, lib, run):
    c = case(dev, lib, run)
    k = c["kept"]
    losses = k["losses"]
    assert k["best_epoch"] == losses.index(min(losses)) and k["lowest_loss"] == min(losses)
    best = re.findall(r"Best Epoch \[(\d)/4\], Lowest loss: (\d+\.\d{20})\n", c["log"])
    assert len(best) == 1 and int(best[0][0]) == k["best_epoch"] + 1 and float(best[0][1]) == min(losses)
    states = [numpy_state(s) for s in k["states"]]
    assert len(states) == EPOCHS
    for i in range(EPOCHS):
        for j in range(i):
            assert not same_state(states[i], states[j]), (i, j)
    assert same_state(load_state(os.path.join(c["out"], CKPT)), states[k["best_epoch"]])
    # the consecutive best: the rule over the logged losses
    from kf2vecfsw_amd import train_chunks as TC
    stop = -(-2 * lib["G"] // c["batch"])
    assert k["stop_epochs"] == stop and "Stopping epochs: {}\n".format(stop) in c["log"]
    cb = re.findall(r"Best consecutive Epoch \[(\d)/4\], Lowest loss: (\d+\.\d{20})\n", c["log"])
    want = TC.consecutive_best(losses, stop)
    assert len(cb) == 1 and int(cb[0][0]) == want[0] + 1 and cb[0][1] == "{:.20f}".format(want[1])


def read_table(path):
    data = open(path, "rb").read()
    assert data.endswith(b"\n") and b"\r" not in data
    return [[cell.decode() for cell in ln.split(b"\t")] for ln in data[:-1].split(b"\n")]


def test_embeddings_are_the_best_model_on_the_full_genome_features(dev, lib):
    import torch
    from kf2vecfsw_amd import query as Q
    c = case(dev, lib, "B")
    k, out, names = c["kept"], c["out"], c["inp"]["names"]
    assert k["names"] == names
    model = Q.load_model(os.path.join(out, CKPT), dev)                       # query's own loader takes the checkpoint
    assert (model.fc1.in_features, model.fc1.out_features, model.fc2.out_features) == (32, HIDDEN, EMBED)
    with torch.no_grad():
        emb = model(torch.from_numpy(c["inp"]["full"]).to(dev)).cpu().numpy()
    mine = k["embeddings"].numpy()
    assert mine.dtype == np.float32 and mine.shape == (lib["G"], EMBED)
    assert np.array_equal(mine.view(np.uint32), emb.view(np.uint32))
    rows = read_table(os.path.join(out, "embeddings_subtree_{}.csv".format(CLADE)))
    assert [r[0] for r in rows] == names and all(len(r) == 1 + EMBED for r in rows)
    assert np.array_equal(np.array([[np.float32(v) for v in r[1:]] for r in rows], dtype=np.float32).view(np.uint32),
                          mine.view(np.uint32))
    rows = read_table(os.path.join(out, "distortions_subtree_{}.csv".format(CLADE)))
    assert rows[0] == [""] + names and [r[0] for r in rows[1:]] == names and all(len(r) == 1 + len(names) for r in rows)
    logs = [f for f in os.listdir(out) if re.fullmatch(r"train_model_\d{8}_\d{6}_clade_%d\.log" % CLADE, f)]
    assert len(logs) == 1 and open(os.path.join(out, logs[0])).read() == c["log"]


def test_the_command_writes_the_same_files(dev, lib, capsys):
    """`train_model_set_chunks` in this process, two epochs in batches of 5 with -cap, against
    train_model_set_chunks_func with the same arguments and the file list the command globs."""
    import glob
    from kf2vecfsw_amd import main as M
    out_f, out_c = str(lib["root"] / "models_func2"), str(lib["root"] / "models_cli2")
    order = glob.glob(os.path.join(lib["chunks"], "*.kf"))
    assert len(order) == lib["G"] + 3
    train(dev, lib, out_f, 5, True, epochs=2, files=order)
    capsys.readouterr()
    M.main(["train_model_set_chunks", "-input_dir", lib["chunks"], "-input_dir_fullgenomes", lib["full"], "-true_dist",
            lib["dist"], "-subtrees", lib["subtrees"], "-e", "2", "-hidden_sz", str(HIDDEN), "-embed_sz", str(EMBED),
            "-batch_sz", "5", "-lr", str(LR), "-clade", str(CLADE), "-cap", "-o", out_c, "-device", str(dev)])
    said = capsys.readouterr().out
    assert said.startswith("Running train_model_set_chunks\n") and "Cap kmer frequencies: True\n" in said
    assert len(re.findall(r"Train loss: ", said)) == 2
    assert same_state(load_state(os.path.join(out_c, CKPT)), load_state(os.path.join(out_f, CKPT)))
    for f in ("embeddings_subtree_{}.csv".format(CLADE), "distortions_subtree_{}.csv".format(CLADE)):
        assert open(os.path.join(out_c, f), "rb").read() == open(os.path.join(out_f, f), "rb").read(), f
    assert sorted(f for f in os.listdir(out_c) if not f.endswith(".log")) == sorted(
        [CKPT, "embeddings_subtree_{}.csv".format(CLADE), "distortions_subtree_{}.csv".format(CLADE)])


def test_an_empty_chunk_file_is_refused_by_name(dev, lib):
    bad = lib["root"] / "chunks_one_empty"
    shutil.copytree(lib["chunks"], str(bad))
    victim = lib["clade"][CLADE][2]
    (bad / (victim + ".kf")).write_bytes(b"")
    out = str(lib["root"] / "models_empty")
    files = [os.path.join(str(bad), os.path.basename(p)) for p in lib["files"]]
    with pytest.raises(ValueError, match=re.escape(os.path.join(str(bad), victim + ".kf"))) as e:
        train(dev, lib, out, 5, False, chunks=str(bad), files=files)
    assert "no window row" in str(e.value)
    assert not os.path.exists(os.path.join(out, CKPT))


def test_a_genome_without_a_full_genome_file_is_refused_by_name(dev, lib):
    bad = lib["root"] / "full_one_missing"
    shutil.copytree(lib["full"], str(bad))
    victim = lib["clade"][CLADE][4]
    os.remove(str(bad / (victim + ".kf")))
    out = str(lib["root"] / "models_missing")
    with pytest.raises(ValueError, match=re.escape(os.path.join(str(bad), victim + ".kf"))):
        train(dev, lib, out, 5, False, full=str(bad))
    assert not os.path.exists(os.path.join(out, CKPT))
