"""train_model_set: the distance model of every clade, trained on the device.

The reference's trainer (kf2vec/train_model_set.py:96-698) goes through the host
at every step: a numpy gather of the batch's true distances and a copy to the
device, `loss.item()`, and at every improving epoch `model.to('cpu')` and
torch.save.  Its loss and backward are a dozen small torch launches, among them
cdist and cdist's backward, whose summation order torch does not promise.  Here
the features (features.features_from_kf) and the true distance matrix
(tables.true_distances) stay on the device for the whole clade, the batches come
from a device randperm, and a step is an index_select, the forward pass,
kf_dist_loss -- the weighted loss of the batch and its gradient with respect to
the embeddings in one call that gathers the true distances itself, with the
order of every sum fixed -- the backward pass and the optimiser step.  Nothing
inside an epoch waits for the device: loss * rows is accumulated in a float64
scalar there and read once per epoch together with the kernel's status.  The
best model is kept as a device copy of the parameters and written once per
clade; the embeddings and distortions are computed and written as text on the
device (query.sq_distances, tables.FloatTableWriter).

Only the NeuralNet model (-no_fsw) is trained: NeuralNetFSW needs fswlib.
"""
from __future__ import annotations

import math
import os
import sys
import time

import numpy as np
import torch

from . import _native as N
from . import counter as C
from . import features as F
from . import query as Q
from . import tables as T

features_scaler = 1e4                  # train_model_set.py:66
learning_rate_base = 0.1               # train_model_set.py:63
learning_rate_update_freq = 100        # train_model_set.py:64
start_epoch = 0                        # train_model_set.py:57

FSW_MESSAGE = ("train_model_set: the FSW model (NeuralNetFSW) needs fswlib, which this project does not have: "
               "only the NeuralNet model is trained here, pass -no_fsw")


# ---------------------------------------------------------------------------
# the loss
# ---------------------------------------------------------------------------
def dist_loss_small_b() -> int:
    """Rows up to which kf_dist_loss runs as one workgroup in one launch."""
    return int(N.lib().kf_dist_loss_small_b())


def dist_loss_tile() -> int:
    """Rows, and columns, per tile of kf_dist_loss above dist_loss_small_b() rows."""
    return int(N.lib().kf_dist_loss_tile())


def dist_loss_depth() -> int:
    """Columns of the embeddings, and rows j of the gradient's sum, per slice through LDS."""
    return int(N.lib().kf_dist_loss_depth())


def dist_loss_max_b() -> int:
    """The most rows kf_dist_loss takes in one call."""
    return int(N.lib().kf_dist_loss_max_b())


def dist_loss_scratch_bytes(b: int) -> int:
    import ctypes
    need = ctypes.c_uint64(0)
    N.check(N.lib().kf_dist_loss_scratch_bytes(int(b), ctypes.byref(need)), "kf_dist_loss_scratch_bytes")
    return int(need.value)


def dist_loss(y: torch.Tensor, table_values: torch.Tensor, labels: torch.Tensor, grad: bool = True,
              stream: int | None = None, views: int = 1, eps: float = 1e-6):
    """Enqueue kf_dist_loss: y [B, E] float32, table_values [N, N] float64 (the
    clade's true distances, FloatTable.values) and labels [B] int64 (rows and
    columns of the table), all on one device.  Returns (loss float64 [], grad
    float32 [B, E] or None, status int32 [1]) on the device: the reference's
    weighted loss of the batch (cdist in the direct form, Loss.my_mse_loss) and
    its gradient with respect to y, bit for bit dist_loss_host.  status is 1,
    and the loss NaN, if a label is outside [0, N).  grad=False: the loss alone,
    the same bits.  Nothing waits.
    With other views or eps than the defaults, kf_dist_loss_views: labels
    [B / views], one per run of `views` rows (repeat_interleave), and the weight
    1 / (T + eps) -- the chunk trainer's Loss_chunks at views=2, eps=1000."""
    views = int(views)
    assert y.dim() == 2 and y.dtype == torch.float32
    assert table_values.dim() == 2 and table_values.shape[0] == table_values.shape[1]
    assert table_values.dtype == torch.float64 and labels.dtype == torch.int64 and labels.dim() == 1
    assert views >= 1 and labels.shape[0] * views == y.shape[0] and y.device == table_values.device == labels.device
    y, table_values, labels = y.contiguous(), table_values.contiguous(), labels.contiguous()
    dev = y.device
    b, e = int(y.shape[0]), int(y.shape[1])
    loss = torch.empty((), dtype=torch.float64, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    g = torch.empty((b, e), dtype=torch.float32, device=dev) if grad else None
    need = dist_loss_scratch_bytes(b) if b else 0
    scratch = torch.empty((need + 7) // 8, dtype=torch.int64, device=dev) if need else None
    s = C._stream_ptr(dev) if stream is None else stream
    head = (y.data_ptr() if y.numel() else None, b, e, table_values.data_ptr(), int(table_values.shape[0]),
            labels.data_ptr() if b else None)
    tail = (loss.data_ptr(), g.data_ptr() if g is not None else None, status.data_ptr(),
            scratch.data_ptr() if scratch is not None else None, 8 * scratch.numel() if scratch is not None else 0, s)
    with torch.cuda.device(dev):
        if views == 1 and eps == 1e-6:
            N.check(N.lib().kf_dist_loss(*head, *tail), "kf_dist_loss")
        else:
            N.check(N.lib().kf_dist_loss_views(*head, views, float(eps), *tail), "kf_dist_loss_views")
    if stream is not None and scratch is not None:   # the scratch is the caller's stream's until the call is done
        scratch.record_stream(torch.cuda.ExternalStream(stream, device=dev))
    return loss, g, status


def dist_loss_host(y, P, labels, views: int = 1, eps: float = 1e-6):
    """The host statement of kf_dist_loss and kf_dist_loss_views in numpy, the
    same operations in the same order (include/kf2vec_gpu.h has the contract):
    returns (loss float64, grad float32 [B, E]).  y [B, E] float32, P [N, N]
    float64, labels [B / views] inside [0, N), row i's being labels[i // views].
    The tests compare the kernel with it; no product path calls it."""
    y = np.ascontiguousarray(y, dtype=np.float32)
    P = np.ascontiguousarray(P, dtype=np.float64)
    lab = np.asarray(labels, dtype=np.int64).reshape(-1)
    assert int(views) >= 1 and lab.shape[0] * int(views) == y.shape[0]
    lab = lab[np.arange(y.shape[0]) // int(views)]
    eps = float(eps)
    assert y.ndim == 2 and y.shape[0] == lab.shape[0] and y.shape[0] > 0 and y.shape[1] > 0
    assert P.ndim == 2 and P.shape[0] == P.shape[1] and lab.min() >= 0 and lab.max() < P.shape[0]
    b, e = y.shape
    with np.errstate(all="ignore"):
        s = np.zeros((b, b), dtype=np.float32)
        for k in range(e):
            t = y[:, k, None] - y[None, :, k]
            s = s + t * t
        d = np.sqrt(s)
        tt = P[np.ix_(lab, lab)]
        w = 1.0 / (tt + eps)
        r = np.sqrt(tt)
        u = d.astype(np.float64) - r
        v = (u * u) * w
        inv = 1.0 / float(b * b)
        rows = np.zeros(b, dtype=np.float64)
        for j in range(b):
            rows = rows + v[:, j]
        total = np.float64(0.0)
        for i in range(b):
            total = total + rows[i]
        loss = np.float64(total * inv)
        g = (((2.0 * u) * w) * inv).astype(np.float32)
        gs = g + g.T
        c = np.where(d == 0, np.float32(0), gs / d).astype(np.float32)
        grad = np.zeros((b, e), dtype=np.float32)
        for j in range(b):
            grad = grad + c[:, j, None] * (y - y[j][None, :])
    return loss, grad


class DistLoss(torch.autograd.Function):
    """kf_dist_loss under autograd: forward returns (loss, status); backward
    hands back the kernel's gradient times the upstream scalar."""

    @staticmethod
    def forward(ctx, y, table_values, labels, views=1, eps=1e-6):
        loss, g, status = dist_loss(y.detach(), table_values, labels, grad=True, views=views, eps=eps)
        ctx.save_for_backward(g)
        ctx.mark_non_differentiable(status)
        return loss, status

    @staticmethod
    def backward(ctx, grad_loss, _grad_status):
        (g,) = ctx.saved_tensors
        return g * grad_loss.to(torch.float32), None, None, None, None


def dist_loss_fn(y: torch.Tensor, table_values: torch.Tensor, labels: torch.Tensor, views: int = 1,
                 eps: float = 1e-6):
    """(loss, status) of the batch, differentiable with respect to y."""
    return DistLoss.apply(y, table_values, labels, views, eps)


# ---------------------------------------------------------------------------
# the pure parts of the trainer
# ---------------------------------------------------------------------------
def batch_plan(n_rows: int, batch_size: int) -> list:
    """[(start, end)] of an epoch's batches over a permutation of n_rows rows, as
    a DataLoader without drop_last cuts them: the last batch is kept short, and
    may hold one row."""
    batch_size = max(1, int(batch_size))
    return [(a, min(a + batch_size, int(n_rows))) for a in range(0, int(n_rows), batch_size)]


def read_test_ids(path) -> list:
    """utils.process_file (kf2vec/utils.py:440-451): the file's lines, stripped, with their extension cut."""
    if path is None:
        return []
    with open(path, "r") as f:
        return [os.path.splitext(line.strip())[0] for line in f]


def split_names(backbone_names, test_ids):
    """(train, test) as train_model_set.py:309-314 makes them."""
    if len(test_ids) != 0:
        train = [b for b in backbone_names if b not in test_ids]
        test = [b for b in backbone_names if b not in train]
        return train, test
    return list(backbone_names), []


def lr_after_epoch(epoch: int, in_lr: float, in_lr_min: float, in_lr_decay: float):
    """The learning rate set after epoch `epoch` (from 0), or None where the
    reference leaves it (train_model_set.py:585-590)."""
    if epoch % learning_rate_update_freq == 0:
        return in_lr_min + in_lr * (learning_rate_base ** (epoch / in_lr_decay))
    return None


def checkpoint_state(input_size: int, hidden_size_fc1: int, embedding_size: int, state_dict) -> dict:
    """utils.save_trained_model's dictionary (kf2vec/utils.py:358-371) with CPU tensors."""
    return {"model_name": "NeuralNet", "model_input_size": int(input_size),
            "model_hidden_size_fc1": int(hidden_size_fc1), "model_embedding_size": int(embedding_size),
            "state_dict": type(state_dict)((k, v.detach().to("cpu")) for k, v in state_dict.items())}


def read_subtrees(path: str):
    """The `.subtrees` file of divide_tree (a header `genome clade`, then a name
    and a clade per line, separated by a space): ([clades by first appearance],
    {clade: [genomes]})."""
    with open(path) as f:
        lines = [ln for ln in f.read().splitlines() if ln.strip()]
    if not lines:
        raise ValueError("{}: no line".format(path))
    head = lines[0].split(" ")
    try:
        gi, ci = head.index("genome"), head.index("clade")
    except ValueError:
        raise ValueError("{}: the header needs the columns genome and clade".format(path)) from None
    clades: dict = {}
    for n, ln in enumerate(lines[1:]):
        cells = ln.split(" ")
        if len(cells) <= max(gi, ci):
            raise ValueError("{}: row {}: {} cells".format(path, n, len(cells)))
        try:
            c = int(float(cells[ci]))
        except ValueError:
            raise ValueError("{}: row {}: clade {!r}".format(path, n, cells[ci])) from None
        clades.setdefault(c, []).append(cells[gi])
    return list(clades), clades


def find_true_dist(true_dist_dir: str, c) -> str:
    """The one file of the directory whose name contains `_subtree_<c>.di_mtrx`."""
    tag = "_subtree_{}.di_mtrx".format(c)
    found = sorted(f for f in os.listdir(true_dist_dir) if tag in f)
    if len(found) != 1:
        raise ValueError("{}: {} files whose name contains {} ({}): exactly one is needed".format(
            true_dist_dir, len(found), tag, ", ".join(found) if found else "none"))
    return os.path.join(true_dist_dir, found[0])


def _input_size(path: str) -> int:
    """The columns behind the name in the first line of a `.kf` file."""
    with open(path, "rb") as f:
        line = f.readline()
    return line.count(b",")


# ---------------------------------------------------------------------------
# train_model_set
# ---------------------------------------------------------------------------
def train_model_set_func(features_folder, features_csv, clades_info, true_dist_matrix, num_epochs, hidden_size_fc1,
                         embedding_size, in_batch_sz, in_lr, in_lr_min, in_lr_decay, clades_to_train, seed,
                         model_filepath, test_IDs_lst, save_interval, use_fsw=True, base_dim=4, fswout_dim=512,
                         device="cuda", keep: bool = False):
    """kf2vec/train_model_set.py:96-698 on the device, for the NeuralNet model
    (use_fsw=False; use_fsw=True ends with FSW_MESSAGE).  features_csv: the `.kf`
    files of features_folder; per clade c of clades_info (or of clades_to_train)
    the genomes are those files whose name is in the clade, in the order given,
    each of exactly one row; the true distances come from the one file of
    true_dist_matrix whose name contains `_subtree_<c>.di_mtrx`, in that order,
    and must be finite and not negative.  The model is query.QueryNet under
    torch.manual_seed(seed), the optimiser Adam(lr=in_lr) with the reference's
    schedule (lr_after_epoch).  An epoch walks a device randperm of the training
    rows (a generator seeded with `seed`) in batches of in_batch_sz, the last
    one short; a step is kf_dist_loss between the forward and the backward
    pass; the epoch's loss is read once, at its end.  The test rows
    (test_IDs_lst) are walked in order under no_grad.  Written to
    model_filepath: model_subtree_<c>.ckpt (the best epoch's parameters, once,
    at the end of the clade), embeddings_subtree_<c>.csv and
    distortions_subtree_<c>.csv for the best model and, with save_interval, for
    every model_epoch_<e+1> directory, and the log
    train_model_<timestamp>_clade_<...>.log, whose lines also go to stdout.
    keep=True (tests): returns per clade a dict with the names, the embedding
    and distortion tensors the files were written from (on the host), those of
    the interval directories, the losses per epoch and the best epoch."""
    if use_fsw:
        raise SystemExit(FSW_MESSAGE)
    torch.manual_seed(seed)
    torch.cuda.manual_seed_all(seed)
    since = time.time()
    device = torch.device(device)
    os.makedirs(model_filepath, exist_ok=True)
    features_csv = list(features_csv)
    kept = []
    clade_tag = "_".join(str(c) for c in clades_to_train) if clades_to_train is not None else "all"
    log_path = os.path.join(model_filepath, "train_model_{}_clade_{}.log".format(time.strftime("%Y%m%d_%H%M%S"),
                                                                                 clade_tag))
    with open(log_path, "w+") as logf:
        def log(msg):
            logf.write(msg + "\n")
            logf.flush()
            sys.stdout.write(msg + "\n")

        def stamp():
            return "{:02d}:{:02d}:{:02d}".format(*Q._hms(time.time() - since))

        log("\n==> Input arguments...\n")
        log("Feature directory: {}".format(features_folder))
        log("Clades information: {}".format(clades_info))
        log("Ground truth directory: {}".format(true_dist_matrix))
        log("Test set: {}".format(test_IDs_lst if test_IDs_lst is not None else "None"))
        log("\n==> Parameters...\n")
        log("GPU Support: {}".format("Yes" if device.type != "cpu" else "No"))
        log("Hidden Size fc1: {}".format(hidden_size_fc1))
        log("Embedding Size: {}".format(embedding_size))
        log("Starting Epoch: {}".format(start_epoch))
        log("Total Epochs: {}".format(num_epochs))
        log("Batch Size: {}".format(in_batch_sz))
        log("Learning Rate: %g" % in_lr)
        log("Learning Rate Min: %g" % in_lr_min)
        log("Learning Rate Decay: %g" % in_lr_decay)
        log("Clades to train: {}".format(" ".join(str(c) for c in clades_to_train)
                                         if clades_to_train is not None else "all"))
        log("Random Seed: {}".format(seed))
        log("Model save interval: {}".format(save_interval if save_interval is not None else "unspecified"))
        log("\n==> Subtree training...\n")
        clade_order, clade_genomes = read_subtrees(clades_info)
        class_count = list(clades_to_train) if clades_to_train is not None else clade_order
        log("Number of Classes: {}".format(len(class_count)))
        if not features_csv:
            raise ValueError("{}: no .kf file".format(features_folder))
        input_size = _input_size(features_csv[0])
        k = Q._k_of(input_size)
        feat_names = [os.path.basename(f).rsplit(".kf", 1)[0] for f in features_csv]
        path_name = os.path.split(features_csv[0])[0]
        test_ids = read_test_ids(test_IDs_lst)
        from . import main as M
        threads = M.host_threads(os.cpu_count() or 1)

        for c in class_count:
            ids = set(clade_genomes.get(c, []))
            log("\n==> Working on subtree {}...\n".format(c))
            log("\n==> Preparing Data...\n")
            backbone_names = [nm for nm in feat_names if nm in ids]
            log("Dimensions of feature matrix rows: {}, cols: {}".format(len(backbone_names), input_size))
            if not backbone_names:
                raise ValueError("{}: no .kf file of clade {}".format(features_folder, c))
            dist_path = find_true_dist(true_dist_matrix, c)
            store = F.features_from_kf(path_name, k, device, samples=backbone_names, scaler=features_scaler,
                                       dtype=torch.float32)
            n_rows = np.diff(store.file_row0)
            for nm, r in zip(backbone_names, n_rows):
                if int(r) != 1:
                    raise ValueError("{}: {} rows: a backbone genome's .kf file holds exactly one".format(
                        os.path.join(path_name, nm + ".kf"), int(r)))
            x_all = store.values.masked_fill(torch.isnan(store.values), 0.0)   # :290, .fillna(0): an empty genome's row
            table = T.true_distances(dist_path, backbone_names, device)
            P = table.values
            if tuple(P.shape) != (len(backbone_names), len(backbone_names)):
                raise ValueError("{}: a matrix of {} x {} for {} genomes".format(dist_path, P.shape[0], P.shape[1],
                                                                                len(backbone_names)))
            wrong = torch.nonzero(~(torch.isfinite(P) & (P >= 0)))
            if wrong.numel():
                r, q = (int(v) for v in wrong[0].tolist())
                raise ValueError("{}: the distance of {} and {} is {}: {} entr{} not finite or negative".format(
                    dist_path, backbone_names[r], backbone_names[q], float(P[r, q]), int(wrong.shape[0]),
                    "y is" if wrong.shape[0] == 1 else "ies are"))
            log("Dimensions of true distance matrix rows: {}, cols: {}".format(P.shape[0], P.shape[1]))
            train_names, test_names = split_names(backbone_names, test_ids)
            row_of = {nm: i for i, nm in enumerate(backbone_names)}
            train_rows = torch.tensor([row_of[nm] for nm in train_names], dtype=torch.int64, device=device)
            test_rows = torch.tensor([row_of[nm] for nm in test_names], dtype=torch.int64, device=device)
            train_size, test_size = len(train_names), len(test_names)
            if train_size == 0:
                raise ValueError("clade {}: every genome is in the test set {}".format(c, test_IDs_lst))
            log("Number of Train Samples: {}".format(train_size))
            if test_size != 0:
                log("Number of Test Samples: {}".format(test_size))
            log("\n==> Building model...\n")
            torch.manual_seed(seed)
            model = Q.QueryNet(input_size, hidden_size_fc1, embedding_size)
            sys.stdout.write("NeuralNet\n")
            model = model.to(device)
            log("\n==> Model parameters----------")
            log("Total parameters: {}".format(sum(p.numel() for p in model.parameters())))
            log("Trainable parameters: {}".format(sum(p.numel() for p in model.parameters() if p.requires_grad)))
            optimizer = torch.optim.Adam(model.parameters(), lr=in_lr)
            gen = torch.Generator(device=device)
            gen.manual_seed(seed)
            log("Time: {}".format(stamp()))
            log("\n==> Training model...\n")
            plan, test_plan = batch_plan(train_size, in_batch_sz), batch_plan(test_size, in_batch_sz)
            total_step = len(plan)
            lowest_loss, best_epoch, best_state = math.inf, -1, None
            interval_dirs, losses = [], []
            acc = torch.zeros(2, dtype=torch.float64, device=device)       # loss * rows, and the status
            for epoch in range(num_epochs):
                model.train()
                acc.zero_()
                perm = train_rows.index_select(0, torch.randperm(train_size, generator=gen, device=device))
                for a, b in plan:
                    labels = perm[a:b]
                    images = x_all.index_select(0, labels)
                    outputs = model(images)
                    loss, status = dist_loss_fn(outputs, P, labels)
                    acc[0] += loss.detach() * (b - a)
                    acc[1] += status[0]
                    optimizer.zero_grad()
                    loss.backward()
                    optimizer.step()
                if test_size != 0:
                    model.eval()
                    tacc = torch.zeros(2, dtype=torch.float64, device=device)
                    with torch.no_grad():
                        for a, b in test_plan:
                            labels = test_rows[a:b]
                            tl, _, ts = dist_loss(model(x_all.index_select(0, labels)), P, labels, grad=False)
                            tacc[0] += tl * (b - a)
                            tacc[1] += ts[0]
                    both = torch.cat([acc, tacc]).cpu().numpy()            # the epoch's one read
                else:
                    both = acc.cpu().numpy()
                if both[1] != 0 or (test_size != 0 and both[3] != 0):
                    raise N.NativeError("kf_dist_loss: a label outside the distance matrix (status 1)")
                train_loss = float(both[0]) / train_size
                losses.append(train_loss)
                if train_loss < lowest_loss:
                    lowest_loss, best_epoch = train_loss, epoch
                    best_state = {kk: v.detach().clone() for kk, v in model.state_dict().items()}
                if save_interval is not None and (epoch % save_interval == 0 or epoch == num_epochs - 1):
                    sub = os.path.join(model_filepath, "model_epoch_{}".format(epoch + 1))
                    os.makedirs(sub, exist_ok=True)
                    torch.save(checkpoint_state(input_size, hidden_size_fc1, embedding_size, model.state_dict()),
                               os.path.join(sub, "model_subtree_{}.ckpt".format(c)))
                    if sub not in interval_dirs:
                        interval_dirs.append(sub)
                log("Epoch [{}/{}], Step [{}/{}], Train loss: {:.20f}, Time: {}".format(
                    epoch + 1, num_epochs, total_step, total_step, train_loss, stamp()))
                if test_size != 0:
                    log("Epoch [{}/{}], Step [{}/{}], Test loss: {:.20f}, Time: {}".format(
                        epoch + 1, num_epochs, len(test_plan), len(test_plan), float(both[2]) / test_size, stamp()))
                log("Epoch {}\t                   LR:{:.20f}".format(epoch + 1, optimizer.param_groups[0]["lr"]))
                lr = lr_after_epoch(epoch, in_lr, in_lr_min, in_lr_decay)
                if lr is not None:
                    for group in optimizer.param_groups:
                        group["lr"] = lr
            log("Best Epoch [{}/{}], Lowest loss: {:.20f}".format(best_epoch + 1, num_epochs, lowest_loss))
            if best_state is None:     # no epoch, or no loss below infinity (NaN from the first epoch on)
                best_state = {kk: v.detach().clone() for kk, v in model.state_dict().items()}
            torch.save(checkpoint_state(input_size, hidden_size_fc1, embedding_size, best_state),
                       os.path.join(model_filepath, "model_subtree_{}.ckpt".format(c)))
            result = {"clade": c, "names": list(backbone_names), "losses": losses, "best_epoch": best_epoch,
                      "lowest_loss": lowest_loss, "intervals": {}}
            model.eval()
            with T.FloatTableWriter(device, threads) as writer, torch.no_grad():
                def outputs_of(state, out_dir):
                    model.load_state_dict(state)
                    emb = model(x_all)
                    dist = Q.sq_distances(emb, emb)
                    writer.write(os.path.join(out_dir, "distortions_subtree_{}.csv".format(c)), backbone_names, dist,
                                 header=[""] + list(backbone_names), mode=T.KF_FLOAT_SHORTEST, eol="\n",
                                 nan_empty=True)
                    writer.write(os.path.join(out_dir, "embeddings_subtree_{}.csv".format(c)), backbone_names, emb,
                                 mode=T.KF_FLOAT_SHORTEST, eol="\n", nan_empty=True)
                    return emb, dist

                emb, dist = outputs_of(best_state, model_filepath)
                log("Dimensions of distortion matrix rows:{} cols:{}".format(dist.shape[0], dist.shape[1] + 1))
                log("Dimensions of embedding output rows:{} cols:{}".format(emb.shape[0], emb.shape[1] + 1))
                if keep:
                    result["embeddings"], result["distortions"] = emb.cpu(), dist.cpu()
                for sub in interval_dirs:
                    log("Computing embeddings for interval: {}".format(sub))
                    state = torch.load(os.path.join(sub, "model_subtree_{}.ckpt".format(c)), map_location=device,
                                       weights_only=True)
                    e2, d2 = outputs_of(state["state_dict"], sub)
                    if keep:
                        result["intervals"][sub] = (e2.cpu(), d2.cpu())
                    log("Done with computing embeddings for interval: {}. Time: {}".format(sub, stamp()))
                writer.drain()
            kept.append(result)
            del store, x_all, table, P, model, optimizer, best_state
            log("\n==> Training for subtree {} completed!\n".format(c))
            log("Time: {}".format(stamp()))
        log("\n==> Training Completed!\n")
        log("Time: {}".format(stamp()))
    return kept if keep else None


def train_model_set(args) -> None:
    """The `train_model_set` subcommand (kf2vec/main.py:506-531)."""
    import glob
    print("Running train_model_set")
    if not args.no_fsw:
        raise SystemExit(FSW_MESSAGE)
    all_files = glob.glob(os.path.join(args.input_dir, "*.kf"))
    train_model_set_func(args.input_dir, all_files, args.subtrees, args.true_dist, args.e, args.hidden_sz,
                         args.embed_sz, args.batch_sz, args.lr, args.lr_min, args.lr_decay, args.clade, args.seed,
                         args.o, args.test_set, args.save_interval, use_fsw=False, base_dim=args.base_dim,
                         fswout_dim=args.fswout_dim, device=getattr(args, "device", None) or "cuda")
