"""GPU tests of train_model_set's loop: everything train.py builds around
kf_dist_loss (the matrix lined up with the features by name, the batches, the
epoch's mean, the test loss, the optimiser and its learning rate, the best
epoch and its checkpoint, the tables' row order) against a restatement of the
reference's loop in torch, on a synthetic library whose every order is a
different shuffle (train_library.py) and whose big clade is above
kf_dist_loss_small_b() rows, so that a batch of all of it is on the tiled path.

The runs (clade 7, hidden 16, embed 8, seed 28, -lr_min 3e-6, -lr_decay 2000;
G = S + 9 genomes, 41 today), five epochs each at -lr 1e-5:
A  batch G: an epoch is one step on the tiled path;
B  batch (G - 1) / 5: five steps on the one-workgroup path and a last batch of
   one row, a checkpoint every epoch;
C  batch 12 with a test set of 13 of the clade's genomes: train batches of 12,
   12 and 4, test batches of 12 and 1;
and D, eight epochs at a learning rate where the loss does not come down
steadily, which is compared with nothing but its own checkpoints.

The bound is the reference's own spread, as in test_gpu_train_classifier.py:
its loop in float32 on the device (l32) against the same loop in float64 on
the CPU (l64), d the largest difference of an epoch's loss; the kernel path
must stay within 4 d of l64 (the margin covers the differing summation order
of the matmul's backward).  The parameters after the last epoch are held to
the same rule with the parameters' own spread.

Measured on an MI355X (profiles/r24/train_loop_parity.json, written by
test_the_record where KF_PARITY_JSON names a file; printed on every run):
run A  d = 1.74e-02 at losses of 38,608 down to 38,469, the kernel path 1.90e-02
       from the float64 run: 0.27 of 4 d;
run B  d = 2.58e-03 at losses between 29,546 and 46,658, the kernel path
       4.44e-03: 0.43 of 4 d;
run C  d = 7.50e-03 at losses between 28,212 and 46,753, the kernel path
       7.39e-03: 0.25 of 4 d; its test loss (45,692 down to 45,528) d = 4.09e-03,
       the kernel path 6.69e-03: 0.41 of 4 d.
The weight matrices of the float32 loop end 2.8e-08 and 2.6e-08 (A), 7.7e-08 and
6.1e-08 (B), 5.3e-08 and 3.2e-08 (C) from the float64 loop's, and the kernel
path's at the same distances to every digit: 0.25 of 4 times.  All parameters
taken together: 5.2e-05, 1.5e-04 and 9.1e-05 for the float32 loop, 5.8e-05,
1.5e-04 and 9.9e-05 for the kernel path (0.28, 0.26 and 0.27 of 4 times); see
test_parameters_after_the_last_epoch for what these are.  The best epochs are 5,
2 and 5 in all three loops, and the float64 loop's two smallest losses are 37,
3,286 and 3,403 apart, so the comparison is made in every run.  A matrix one
place off against the names moves every epoch's loss of the float64 loop by at
least 1,795 (A), 264 (B) and 70 (C): 25,826, 25,616 and 2,343 times 4 d, where
100 times are asked for."""
import contextlib
import io
import json
import os
import re

import numpy as np
import pytest

import train_library

pytestmark = pytest.mark.gpu

CLADE = train_library.BIG
EPOCHS, HIDDEN, EMBED, SEED = 5, 16, 8, 28
LR, LR_MIN, LR_DECAY = 1e-5, 3e-6, 2000
SCALER = 1e4                          # train_model_set.py:66
D_EPOCHS, D_LR = 8, 0.3                # run D: batch G, as run A
CKPT = "model_subtree_{}.ckpt".format(CLADE)


@pytest.fixture(scope="module")
def dev(native):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu tests need an MI355X")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib(dev, tmp_path_factory):
    root = tmp_path_factory.mktemp("train_loop_lib")
    made = train_library.make(root)
    made["root"] = root
    # the test set of run C: 13 genomes of the clade with extensions, in an order of its own, one of the other
    # clade, and a name that no clade has
    rng = np.random.default_rng(77)
    big = made["clade"][CLADE]
    picked = [big[i] for i in rng.permutation(len(big))[:13]]
    lines = [nm + (".kf", ".fna", ".fa")[i % 3] for i, nm in enumerate(picked)]
    lines.insert(5, made["clade"][train_library.SMALL][1] + ".kf")
    lines.insert(9, "L0000_in_no_clade.kf")
    ts = root / "test_set.txt"
    ts.write_text("\n".join(lines) + "\n")
    made["test_set"] = str(ts)
    return made


def run_plan(lib):
    """{run: (batch, test set, save_interval, epochs, lr)}."""
    G = lib["G"]
    return {"A": (G, None, EPOCHS, EPOCHS, LR), "B": ((G - 1) // 5, None, 1, EPOCHS, LR),
            "C": (12, lib["test_set"], EPOCHS, EPOCHS, LR), "D": (G, None, 1, D_EPOCHS, D_LR)}


# ---------------------------------------------------------------------------
# the inputs, read here by name: nothing of tables.py or features.py
# ---------------------------------------------------------------------------
def read_inputs(lib, test_set=None):
    """The clade's names in the order of the file list, their features (float(field) * 1e4
    rounded to float32, what the reference's images.float() holds), the true distances
    reordered by name, and the train and test rows (train_model_set.py:309-314 with
    utils.process_file's names)."""
    members = set()
    with open(lib["subtrees"]) as f:
        for line in f.read().splitlines()[1:]:
            nm, c = line.split(" ")
            if int(c) == CLADE:
                members.add(nm)
    names = [os.path.basename(p)[:-3] for p in lib["files"] if os.path.basename(p)[:-3] in members]
    rows = []
    for nm in names:
        with open(os.path.join(lib["kf"], nm + ".kf")) as f:
            cells = f.read().rstrip("\n").split(",")
        assert cells[0] == nm
        rows.append([np.float32(float(v) * SCALER) for v in cells[1:]])
    x = np.array(rows, dtype=np.float32)
    with open(os.path.join(lib["dist"], "x_subtree_{}.di_mtrx".format(CLADE))) as f:
        lines = f.read().splitlines()
    head = lines[0].split("\t")[1:]
    by_name = {}
    for line in lines[1:]:
        cells = line.split("\t")
        by_name[cells[0]] = dict(zip(head, (float(v) for v in cells[1:])))
    P = np.array([[by_name[a][b] for b in names] for a in names], dtype=np.float64)
    test_ids = []
    if test_set is not None:
        with open(test_set) as f:
            test_ids = [os.path.splitext(line.strip())[0] for line in f]
    train = [i for i, nm in enumerate(names) if nm not in test_ids]
    test = [i for i, nm in enumerate(names) if nm in test_ids]
    return dict(names=names, x=x, P=P, train=np.array(train, dtype=np.int64), test=np.array(test, dtype=np.int64))


# ---------------------------------------------------------------------------
# the reference's loop
# ---------------------------------------------------------------------------
def weighted_loss(model_dist, true_dist):
    """losses.Loss (kf2vec/losses.py:13-49)."""
    import torch
    assert model_dist.shape == true_dist.shape
    weight = 1 / (true_dist + 1e-6)
    root = torch.sqrt(true_dist)
    return ((model_dist - root) ** 2 * weight).mean()


def restate(inp, device, dtype, batch, epochs, lr, P=None):
    """kf2vec/train_model_set.py:430-590 from the trainer's initial parameters
    (torch.manual_seed(28), the model made on the host) and with its batches (per epoch a
    device randperm of a device generator seeded with 28 over the train rows; the test rows
    in order): (train loss per epoch, test loss per epoch, the parameters after the last
    epoch).  P: another matrix than the inputs' own."""
    import torch
    from kf2vecfsw_amd import query as Q
    gpu = torch.device("cuda:0")
    P = inp["P"] if P is None else P
    x_all = torch.from_numpy(inp["x"]).to(device=device, dtype=dtype)
    input_size = x_all.shape[1]
    torch.manual_seed(SEED)
    model = Q.QueryNet(input_size, HIDDEN, EMBED).to(device=device, dtype=dtype)
    optimizer = torch.optim.Adam(model.parameters(), lr=lr)
    gen = torch.Generator(device=gpu)
    gen.manual_seed(SEED)
    train_size, test_size = len(inp["train"]), len(inp["test"])

    def step_loss(labels):
        images = x_all[torch.from_numpy(labels).to(device)].reshape(-1, input_size)
        real_dist = torch.from_numpy(P[np.ix_(list(labels), list(labels))]).to(device)
        outputs = model(images)
        train_dist = torch.cdist(outputs, outputs, p=2, compute_mode="donot_use_mm_for_euclid_dist")
        return weighted_loss(train_dist, real_dist), images.shape[0]

    train_losses, test_losses = [], []
    for epoch in range(epochs):
        model.train()
        train_loss, items_count = 0.0, 0
        order = inp["train"][torch.randperm(train_size, generator=gen, device=gpu).cpu().numpy()]
        for a in range(0, train_size, batch):
            loss, rows = step_loss(order[a: a + batch])
            train_loss += loss.item() * rows
            items_count += rows
            optimizer.zero_grad()
            loss.backward()
            optimizer.step()
        train_losses.append(train_loss / items_count)
        if test_size != 0:
            model.eval()
            test_loss, items_count = 0.0, 0
            with torch.no_grad():
                for a in range(0, test_size, batch):
                    loss, rows = step_loss(inp["test"][a: a + batch])
                    test_loss += loss.item() * rows
                    items_count += rows
            test_losses.append(test_loss / items_count)
        if epoch % 100 == 0:                                            # :585-590
            new_lr = LR_MIN + lr * (0.1 ** (epoch / LR_DECAY))
            for group in optimizer.param_groups:
                group["lr"] = new_lr
    state = {k: v.detach().to("cpu", torch.float64).numpy() for k, v in model.state_dict().items()}
    return train_losses, test_losses, state


# ---------------------------------------------------------------------------
# the runs
# ---------------------------------------------------------------------------
def train(dev, lib, out, batch, test_set, save_interval, epochs, lr):
    """train_model_set_func on the clade; (kept, stdout)."""
    from kf2vecfsw_amd import train as TR
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        kept = TR.train_model_set_func(lib["kf"], lib["files"], lib["subtrees"], lib["dist"], epochs, HIDDEN, EMBED,
                                       batch, lr, LR_MIN, LR_DECAY, [CLADE], SEED, out, test_set, save_interval,
                                       use_fsw=False, device=dev, keep=True)
    assert len(kept) == 1 and kept[0]["clade"] == CLADE
    return kept[0], buf.getvalue()


def load_state(path):
    import torch
    return {k: v.numpy() for k, v in torch.load(path, map_location="cpu", weights_only=True)["state_dict"].items()}


def same_state(a, b):
    """Tensor for tensor, bit for bit."""
    return list(a) == list(b) and all(a[k].dtype == b[k].dtype == np.float32 and a[k].shape == b[k].shape and
                                      np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in a)


def tensor_distances(a, b):
    """{tensor: the largest absolute difference of an entry}."""
    assert list(a) == list(b)
    return {k: float(np.abs(a[k].astype(np.float64) - b[k].astype(np.float64)).max()) for k in a}


def state_distance(a, b):
    return max(tensor_distances(a, b).values())


_CASES = {}


def case(dev, lib, run):
    """A run through the trainer and, for A, B and C, the restatements on its inputs, made once."""
    import torch
    if run in _CASES:
        return _CASES[run]
    batch, test_set, save_interval, epochs, lr = run_plan(lib)[run]
    out = str(lib["root"] / "models_{}".format(run))
    kept, said = train(dev, lib, out, batch, test_set, save_interval, epochs, lr)
    c = dict(run=run, out=out, kept=kept, log=said, batch=batch, epochs=epochs, lr=lr, inp=read_inputs(lib, test_set))
    c["test_losses"] = [float(v) for v in re.findall(r"Test loss: (\d+\.\d{20}), Time: ", said)]
    c["last"] = load_state(os.path.join(out, "model_epoch_{}".format(epochs), CKPT))
    if run != "D":
        inp = c["inp"]
        c["l32"], c["t32"], c["p32"] = restate(inp, dev, torch.float32, batch, epochs, lr)
        c["l64"], c["t64"], c["p64"] = restate(inp, torch.device("cpu"), torch.float64, batch, epochs, lr)
        # the matrix one place off against the names
        c["rolled"], _, _ = restate(inp, torch.device("cpu"), torch.float64, batch, epochs, lr,
                                    P=np.roll(inp["P"], 1, axis=(0, 1)))
    _CASES[run] = c
    return c


def spread(mine, l32, l64):
    """(d, the kernel path's distance from the float64 loop)."""
    assert len(mine) == len(l32) == len(l64) == EPOCHS
    return max(abs(a - b) for a, b in zip(l32, l64)), max(abs(a - b) for a, b in zip(mine, l64))


RUNS = ["A", "B", "C"]


def test_the_record(dev, lib):
    """The figures of every run, printed, and written where KF_PARITY_JSON names a file."""
    record = {"genomes": lib["G"], "small_b": lib["S"], "hidden": HIDDEN, "embed": EMBED, "epochs": EPOCHS, "lr": LR,
              "runs": {}}
    for run in RUNS:
        c = case(dev, lib, run)
        d, mine = spread(c["kept"]["losses"], c["l32"], c["l64"])
        moved = min(abs(a - b) for a, b in zip(c["rolled"], c["l64"]))
        two = sorted(c["l64"])[:2]
        r = {"batch": c["batch"], "d": d, "kernel_path": mine, "losses_kernel_path": c["kept"]["losses"],
             "losses_float32": c["l32"], "losses_float64": c["l64"], "losses_float64_matrix_one_place_off": c["rolled"],
             "parameters_float32": state_distance(c["p32"], c["p64"]),
             "parameters_kernel_path": state_distance(c["last"], c["p64"]),
             "parameters_float32_by_tensor": tensor_distances(c["p32"], c["p64"]),
             "parameters_kernel_path_by_tensor": tensor_distances(c["last"], c["p64"]),
             "sensitivity_ratio": moved / (4 * d) if d else None,
             "best_epoch_kernel_path": c["kept"]["best_epoch"] + 1, "best_epoch_float64": 1 + c["l64"].index(min(c["l64"])),
             "best_epoch_compared": bool(two[1] - two[0] > 8 * d)}
        if run == "C":
            td, tmine = spread(c["test_losses"], c["t32"], c["t64"])
            r.update({"test_d": td, "test_kernel_path": tmine, "test_losses_kernel_path": c["test_losses"],
                      "test_losses_float32": c["t32"], "test_losses_float64": c["t64"]})
        record["runs"][run] = r
    c = case(dev, lib, "D")
    record["runs"]["D"] = {"batch": c["batch"], "epochs": D_EPOCHS, "lr": D_LR, "losses_kernel_path": c["kept"]["losses"],
                           "best_epoch_kernel_path": c["kept"]["best_epoch"] + 1}
    print(json.dumps(record, indent=1))
    path = os.environ.get("KF_PARITY_JSON")
    if path:
        with open(path, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")


def test_the_inputs_are_what_the_runs_need(dev, lib):
    S, G = lib["S"], lib["G"]
    inp, inp_c = read_inputs(lib), read_inputs(lib, lib["test_set"])
    assert G == S + 9 == len(inp["names"]) and inp["x"].shape == (G, 32) and inp["P"].shape == (G, G)
    assert G > S >= (G - 1) // 5 and (G - 1) % 5 == 0                   # A is tiled; B's batches are not, and leave one row
    assert len(inp["train"]) == G and len(inp["test"]) == 0
    assert len(inp_c["train"]) == G - 13 and len(inp_c["test"]) == 13
    P = inp["P"]
    assert np.array_equal(P, P.T) and not np.diagonal(P).any()
    off = P[np.triu_indices(G, 1)]
    assert np.unique(off).size == off.size and off.min() > 0.05 and off.max() < 3.0
    assert inp["names"] != sorted(inp["names"]) and inp["names"] != lib["matrix_order"][CLADE]


@pytest.mark.parametrize("run", RUNS)
def test_train_loss_against_a_restatement_of_the_references_loop(dev, lib, run):
    c = case(dev, lib, run)
    k = c["kept"]
    steps = re.findall(r"Epoch \[(\d)/5\], Step \[(\d+)/(\d+)\], Train loss: (\d+\.\d{20}), Time: ", c["log"])
    n = -(-len(c["inp"]["train"]) // c["batch"])
    assert [(int(e), int(a), int(b)) for e, a, b, _ in steps] == [(e + 1, n, n) for e in range(EPOCHS)]
    assert n == {"A": 1, "B": 6, "C": -(-(lib["G"] - 13) // 12)}[run]  # C: 12, 12 and 4 of 28 today
    assert [float(v) for _, _, _, v in steps] == k["losses"]
    d, mine = spread(k["losses"], c["l32"], c["l64"])
    print("run {}: losses: kernel path {}, float32 loop {}, float64 loop {}".format(run, k["losses"], c["l32"], c["l64"]))
    print("run {}: d = {!r}; the kernel path differs from the float64 run by {!r}: {:.3f} of 4 d".format(
        run, d, mine, mine / (4 * d) if d else float("inf")))
    assert mine <= 4 * d


def test_test_loss_of_run_c(dev, lib):
    c = case(dev, lib, "C")
    steps = re.findall(r"Epoch \[(\d)/5\], Step \[(\d+)/(\d+)\], Test loss: ", c["log"])
    assert [(int(e), int(a), int(b)) for e, a, b in steps] == [(e + 1, 2, 2) for e in range(EPOCHS)]
    assert "Number of Train Samples: {}\n".format(lib["G"] - 13) in c["log"] and "Number of Test Samples: 13\n" in c["log"]
    d, mine = spread(c["test_losses"], c["t32"], c["t64"])
    print("run C: test losses: kernel path {}, float32 loop {}, float64 loop {}".format(c["test_losses"], c["t32"], c["t64"]))
    print("run C: test d = {!r}; the kernel path differs from the float64 run by {!r}: {:.3f} of 4 d".format(
        d, mine, mine / (4 * d) if d else float("inf")))
    assert mine <= 4 * d
    for run in ("A", "B"):
        assert not case(dev, lib, run)["test_losses"] and "Test loss" not in case(dev, lib, run)["log"]


WEIGHTS = ("fc1.weight", "fc2.weight")


@pytest.mark.parametrize("run", RUNS)
def test_parameters_after_the_last_epoch(dev, lib, run):
    """The written checkpoint of the last model_epoch_* directory against the float64 loop's
    parameters: no further than 4 times the float32 loop's are.  A learning rate set an epoch
    early or late, or another optimiser step, shows here.
    The loss depends on differences of embeddings alone, so in exact arithmetic fc2.bias has
    no gradient, and neither has the fc1.bias of a hidden unit that is active on every row of
    a batch (the features are all positive: most units are active on all rows or on none).
    In floating point those gradients are rounding noise, which Adam scales to steps of the
    size of the learning rate: in float64 these entries stay where they were, in float32 they
    walk at random (on an MI355X in run A: fc2.bias 5.2e-05 from the float64 loop's in the
    float32 loop and 5.8e-05 on the kernel path, fc1.bias 2.7e-05 and 4.0e-05, the weight
    matrices 2.8e-08 and 2.6e-08 on both), and the spread of all parameters taken together
    is that walk's.  So the rule is also applied to each weight matrix with its own spread,
    which is a thousand times tighter: with the learning rate set an epoch early fc1.weight
    is 3.0e-06, 1.7e-05 and 9.0e-06 away in runs A, B and C, which the rule over all
    parameters together would let pass in every run."""
    c = case(dev, lib, run)
    d32, mine = tensor_distances(c["p32"], c["p64"]), tensor_distances(c["last"], c["p64"])
    for k in d32:
        print("run {}: {}: the float32 loop is {!r} from the float64 loop, the kernel path {!r}: {:.3f} of 4 times".format(
            run, k, d32[k], mine[k], mine[k] / (4 * d32[k]) if d32[k] else float("inf")))
    assert max(mine.values()) <= 4 * max(d32.values())
    for k in WEIGHTS:
        assert mine[k] <= 4 * d32[k], k


@pytest.mark.parametrize("run", RUNS)
def test_best_epoch(dev, lib, run):
    c = case(dev, lib, run)
    k = c["kept"]
    losses = k["losses"]
    assert k["best_epoch"] == losses.index(min(losses)) and k["lowest_loss"] == min(losses)      # the first argmin
    best = re.findall(r"Best Epoch \[(\d)/5\], Lowest loss: (\d+\.\d{20})\n", c["log"])
    assert len(best) == 1 and int(best[0][0]) == k["best_epoch"] + 1 and float(best[0][1]) == min(losses)
    d, _ = spread(losses, c["l32"], c["l64"])
    two = sorted(c["l64"])[:2]
    decided = two[1] - two[0] > 8 * d
    print("run {}: best epoch {} of the kernel path, {} of the float64 loop, whose two smallest losses differ by {!r} "
          "({} 8 d = {!r}): the comparison was {}made".format(run, k["best_epoch"] + 1, 1 + c["l64"].index(min(c["l64"])),
                                                              two[1] - two[0], "above" if decided else "not above", 8 * d,
                                                              "" if decided else "not "))
    if decided:
        assert k["best_epoch"] == c["l64"].index(min(c["l64"]))


@pytest.mark.parametrize("run", RUNS)
def test_a_matrix_one_place_off_would_show(dev, lib, run):
    """A condition on the inputs, not on the trainer: the float64 loop with the matrix's rows
    and columns rolled by one place against the names must move every epoch's loss by more
    than 100 times the 4 d that the kernel path is allowed."""
    c = case(dev, lib, run)
    d, _ = spread(c["kept"]["losses"], c["l32"], c["l64"])
    moved = min(abs(a - b) for a, b in zip(c["rolled"], c["l64"]))
    print("run {}: a matrix one place off moves an epoch's loss by at least {!r}: {:.1f} times 4 d".format(
        run, moved, moved / (4 * d) if d else float("inf")))
    assert moved > 100 * 4 * d, ("these inputs cannot tell a trainer whose matrix is lined up with the names from one "
                                 "whose matrix is one place off: the smallest move {!r} is not above 100 * 4 d = {!r}"
                                 .format(moved, 400 * d))


def read_table(path):
    data = open(path, "rb").read()
    assert data.endswith(b"\n") and b"\r" not in data
    return [[cell.decode() for cell in ln.split(b"\t")] for ln in data[:-1].split(b"\n")]


def test_run_b_checkpoints_and_tables(dev, lib):
    import torch
    from kf2vecfsw_amd import query as Q
    c = case(dev, lib, "B")
    k, out, names = c["kept"], c["out"], c["inp"]["names"]
    dirs = [os.path.join(out, "model_epoch_{}".format(e + 1)) for e in range(EPOCHS)]
    assert sorted(k["intervals"]) == sorted(dirs)
    states = [load_state(os.path.join(d, CKPT)) for d in dirs]
    best = load_state(os.path.join(out, CKPT))
    assert same_state(best, states[k["best_epoch"]])
    for i in range(EPOCHS):
        for j in range(i):
            assert not same_state(states[i], states[j]), (i, j)
    # the best embeddings: the best checkpoint's network on the features, in the order of the file list
    assert k["names"] == names
    model = Q.load_model(os.path.join(out, CKPT), dev)
    with torch.no_grad():
        emb = model(torch.from_numpy(c["inp"]["x"]).to(dev)).cpu().numpy()
    mine = k["embeddings"].numpy()
    assert mine.dtype == np.float32 and mine.shape == (lib["G"], EMBED)
    assert np.array_equal(mine.view(np.uint32), emb.view(np.uint32))
    for d in [out] + dirs:
        rows = read_table(os.path.join(d, "embeddings_subtree_{}.csv".format(CLADE)))
        assert [r[0] for r in rows] == names and all(len(r) == 1 + EMBED for r in rows), d
        rows = read_table(os.path.join(d, "distortions_subtree_{}.csv".format(CLADE)))
        assert rows[0] == [""] + names and [r[0] for r in rows[1:]] == names, d
        assert all(len(r) == 1 + len(names) for r in rows), d


def test_run_d_the_best_checkpoint_is_the_best_epochs(dev, lib):
    """Eight epochs in batches of G at -lr 0.3, a checkpoint every epoch.  Not compared with
    the restatement: this is not the smooth regime.  Epoch 1's loss is that of the initial
    parameters; the first step then throws the model far off and it does not come back in
    eight epochs, so the best epoch is the first and not the last, and a best state that was
    the live parameters and no copy of them would be written as the last epoch's.
    Measured on an MI355X, the same digits in two runs: 38608.3 215077 356638 54372.2 60201
    109609 96877.2 61298.2.  The other rates tried there with batch G (1e-4, 1e-3, 1e-2,
    3e-2, 0.1) all had their best epoch last; 1.0 behaves as 0.3 does (38608.3, then 3.6e7
    and above).  In batches of 8 the rates 1e-2 and 3e-2 had their best epoch at 7 of 8 (229
    against 231, 208 against 307) and 0.3 at 1 (1.127e6 against 1.154e6 at epoch 8): narrower
    margins than 38,608 against 54,372."""
    c = case(dev, lib, "D")
    k, out = c["kept"], c["out"]
    losses = k["losses"]
    print("run D: losses", " ".join("{:.6g}".format(v) for v in losses), "best epoch", k["best_epoch"] + 1)
    assert len(losses) == D_EPOCHS and k["best_epoch"] == losses.index(min(losses))
    assert k["best_epoch"] != D_EPOCHS - 1
    best = load_state(os.path.join(out, CKPT))
    assert same_state(best, load_state(os.path.join(out, "model_epoch_{}".format(k["best_epoch"] + 1), CKPT)))
    assert not same_state(best, c["last"])
