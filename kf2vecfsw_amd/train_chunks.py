"""train_model_set_chunks: the distance model of every clade, trained on random
runs of its genomes' 10-kbp windows, on the device.

The reference's trainer (kf2vec/train_model_set_chunks.py:82-672) reads every
genome's window rows with pandas under mp.Pool, and per item and epoch its
Dataset_chunks_2rows draws two runs of rows on a numpy stream that every
DataLoader worker forks, sums and normalises them in numpy, and the step then
goes through the host as train_model_set's does.  Here the window rows stay on
the device (chunks.chunk_store_from_kf), an epoch's runs are drawn there by
torch (draw_runs: the distribution of chunks.draw_ranges, three random tensors
per call), the features are built there in slabs of whole batches
(kf_chunk_features), and a step is the forward pass on the 2 b rows of b
genomes, kf_dist_loss_views -- Loss_chunks, whose weight is 1 / (T + 1000), with
rows 2 i and 2 i + 1 sharing genome i's label -- the backward pass and Adam's
step.  Nothing inside an epoch waits for the device: every step's loss goes
into a device buffer that is read once per epoch, with the running sum of
loss * b and the status words of the loss and feature kernels.  The lines the
reference writes during an epoch are written after that read, in its order.
The best state is kept on the device and written once per clade; embeddings
and distortions are the best model's on the full-genome features
(features.features_from_kf), written as text on the device as train.py does.
"""
from __future__ import annotations

import math
import os
import sys
import time
import warnings

import numpy as np
import torch

from . import _native as N
from . import chunks as CH
from . import counter as C
from . import features as F
from . import query as Q
from . import tables as T
from . import train as TR

features_scaler = 1e4                  # train_model_set_chunks.py:59
VIEWS = 2                              # Dataset_chunks_2rows
LOSS_EPS = 1000.0                      # losses.py:70
CAP = 255                              # utils.cap_to_unit8
OUTLIER_LOSS, OUTLIER_AFTER = 0.2, 5   # train_model_set_chunks.py:419
FEATURE_SLAB_BYTES = 1 << 30           # float32 features built per kf_chunk_features call (at k = 11 a row is 8 MiB)


# ---------------------------------------------------------------------------
# the runs
# ---------------------------------------------------------------------------
def draw_runs(c: torch.Tensor, gen: torch.Generator, views: int = VIEWS):
    """The row runs of Dataset_chunks_2rows (kf2vec/datasets.py:47-52) for items
    with c[i] >= 1 window rows, drawn by torch on c's device from `gen` (a
    generator of that device): (lo, n) int64 [M, views], run (i, v) being the
    rows [lo, lo + n) of item i.  The distribution is chunks.draw_ranges':
    x = Exp(1) * (c / 5) in float64, m = floor(min(x, c)) + 1, and where that
    passes c a uniform length 1 + min(floor(u1 * c), c - 1) instead; the start
    is min(floor(u2 * (c - m + 1)), c - m).  Three random tensors [M, views] are
    consumed whatever the data (the exponential, u1, u2), so the stream behind a
    call does not depend on what it drew; nothing goes through the host."""
    assert c.dtype == torch.int64
    c = c.reshape(-1, 1)
    dev, shape = c.device, (c.shape[0], int(views))
    x = torch.empty(shape, dtype=torch.float64, device=dev).exponential_(1.0, generator=gen)
    u1 = torch.rand(shape, dtype=torch.float64, device=dev, generator=gen)
    u2 = torch.rand(shape, dtype=torch.float64, device=dev, generator=gen)
    cf = c.to(torch.float64)
    m = torch.floor(torch.minimum(x * (cf / 5), cf)).to(torch.int64) + 1
    again = 1 + torch.minimum(torch.floor(u1 * cf).to(torch.int64), c - 1)
    n = torch.where(m > c, again, m)
    lo = torch.minimum(torch.floor(u2 * (c - n + 1).to(torch.float64)).to(torch.int64), c - n)
    return lo, n


def slab_plan(plan, row_bytes: int, budget: int, views: int = VIEWS) -> list:
    """[(first batch, end batch)] of an epoch's batches `plan` ([(start, end)] in
    items): whole batches that follow each other, as many as stay under `budget`
    bytes of features (views * items rows of row_bytes each), one at least."""
    slabs, first = [], 0
    while first < len(plan):
        end = first + 1
        while end < len(plan) and views * (plan[end][1] - plan[first][0]) * row_bytes <= budget:
            end += 1
        slabs.append((first, end))
        first = end
    return slabs


def _row0_device(store) -> torch.Tensor:
    """store.row0 on the store's device, copied once per store."""
    d = getattr(store, "_row0_device", None)
    if d is None or d.device != store.counts.device:
        d = torch.from_numpy(np.ascontiguousarray(store.row0, dtype=np.int64)).to(store.counts.device)
        store._row0_device = d
    return d


def epoch_batches(store, rows: torch.Tensor, perm: torch.Tensor, plan, gen: torch.Generator,
                  scaler: float = features_scaler, cap: int | None = None, budget: int = FEATURE_SLAB_BYTES,
                  status: torch.Tensor | None = None, views: int = VIEWS):
    """An epoch's batches: yields (Z [2 b, nbins] float32, labels int64 [b]) on the
    store's device for every (start, end) of `plan` over the items rows[perm]
    (`rows`: the store's genome of every training item, which is also its row of
    the distance matrix; `perm`: an order of them; both int64 on the device).
    Rows 2 i and 2 i + 1 of Z are two views of genome labels[i]
    (Dataset_chunks_2rows, kf2vec/datasets.py:47-62): the whole epoch's
    2 * len(perm) runs are drawn first (one draw_runs call on `gen`), then the
    features are built by kf_chunk_features in slabs of whole batches that stay
    under `budget` bytes, so a batch's bits depend on the draws alone and not on
    the budget.  Nothing waits for the device: every slab's status word is added
    to `status` (a one-element tensor on the device, for the caller's own read);
    with status=None the words are read here after the last batch, and a run
    outside the store raises N.NativeError.  views: the runs per item (2 here;
    1 for Dataset_chunks_1row, the chunk classifier's: Z is then [b, nbins])."""
    views = int(views)
    counts = store.counts
    row0 = _row0_device(store)
    items = rows.index_select(0, perm)
    first = row0.index_select(0, items)
    c = row0.index_select(0, items + 1) - first
    lo, n = draw_runs(c, gen, views)
    lo = (lo + first.reshape(-1, 1)).reshape(-1).contiguous()
    n = n.reshape(-1).contiguous()
    folded = torch.zeros(1, dtype=torch.int64, device=counts.device) if status is None else status
    for b0, b1 in slab_plan(plan, 4 * counts.shape[1], budget, views):
        a, e = plan[b0][0], plan[b1 - 1][1]
        z, st = C.chunk_features(counts, lo[views * a: views * e], n[views * a: views * e], scaler, cap, torch.float32,
                                 check=False)
        folded.add_(st.to(folded.dtype))
        for s, t in plan[b0:b1]:
            yield z[views * (s - a): views * (t - a)], items[s:t]
        del z
    if status is None and int(folded.item()) != 0:
        raise N.NativeError("kf_chunk_features: a run's rows lie outside the count matrix")


# ---------------------------------------------------------------------------
# the pure parts
# ---------------------------------------------------------------------------
def stopping_epochs(n_genomes: int, batch_size: int) -> int:
    """train_model_set_chunks.py:373."""
    return int(math.ceil(n_genomes / batch_size * 2))


def consecutive_best(losses, stop_epochs: int):
    """(epoch from 0, lowest mean) of train_model_set_chunks.py:366-478: after
    every epoch the mean, NaN left out, of the last stop_epochs train losses,
    newest first (a queue that starts as stop_epochs NaN), and the first epoch
    at which that mean is below every earlier one; (-1, inf) if there is none."""
    stop_epochs = int(stop_epochs)
    lowest, best = math.inf, -1
    for epoch in range(len(losses)):
        window = [float(v) for v in losses[max(0, epoch + 1 - stop_epochs): epoch + 1]][::-1]
        window += [float("nan")] * (stop_epochs - len(window))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)       # a window of NaN alone
            mean = np.nanmean(window)
        if mean < lowest:
            lowest, best = mean, epoch
    return best, lowest


def epoch_lines(epoch: int, num_epochs: int, plan, losses) -> list:
    """The lines the reference writes inside epoch `epoch` (from 0) for the steps'
    losses (train_model_set_chunks.py:419-432), in its order."""
    out = []
    for i, ((a, b), loss) in enumerate(zip(plan, losses)):
        if epoch > OUTLIER_AFTER and loss > OUTLIER_LOSS:
            out.append("Epoch [{}/{}], Step [{}/{}], Outlier: {:.20f} batch size: {}".format(
                epoch + 1, num_epochs, i + 1, len(plan), loss, VIEWS * (b - a)))
        if math.isnan(loss):
            out.append("Loss: nan")
    return out


# ---------------------------------------------------------------------------
# train_model_set_chunks
# ---------------------------------------------------------------------------
def train_model_set_chunks_func(features_folder, input_dir_fullgenomes, features_csv, clades_info, true_dist_matrix,
                                num_epochs, hidden_size_fc1, embedding_size, in_batch_sz, in_lr, in_lr_min, in_lr_decay,
                                clades_to_train, seed, cap_data, model_filepath, device="cuda", keep: bool = False):
    """kf2vec/train_model_set_chunks.py:82-672 on the device.  features_csv: the
    get_chunks `.kf` files of features_folder; per clade c of clades_info (or of
    clades_to_train) the genomes are those files whose name is in the clade, in
    the order given; a file of no rows is a ValueError that names it.  Every
    genome needs its `<name>.kf` of exactly one row in input_dir_fullgenomes,
    read before any epoch (its values are not filled: the reference has no
    fillna here); the true distances are train.py's, with its checks.  The
    model is query.QueryNet under torch.manual_seed(seed), the optimiser
    Adam(lr=in_lr) with the reference's schedule.  An epoch is a device
    randperm of the genomes and then the runs of epoch_batches, both from one
    generator seeded with `seed`, in batches of in_batch_sz genomes (2 rows
    each), the last one short; cap_data caps every window count at 255.  There
    is no test set and no save interval.  Written to model_filepath:
    model_subtree_<c>.ckpt (the best epoch's parameters, once per clade),
    embeddings_subtree_<c>.csv and distortions_subtree_<c>.csv of the best model
    on the full-genome features, and the log
    train_model_<timestamp>_clade_<...>.log, whose lines also go to stdout.
    keep=True (tests): per clade a dict with the names, the embedding and
    distortion tensors (on the host), the losses per epoch and per step, the
    best epoch, the best consecutive epoch, the initial parameters and those
    after every epoch."""
    torch.manual_seed(seed)
    torch.cuda.manual_seed_all(seed)
    since = time.time()
    device = torch.device(device)
    os.makedirs(model_filepath, exist_ok=True)
    features_csv = list(features_csv)
    kept = []
    cap = CAP if cap_data else None
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
        log("Full genome feature directory: {}".format(input_dir_fullgenomes))
        log("Clades information: {}".format(clades_info))
        log("Ground truth directory: {}".format(true_dist_matrix))
        log("\n==> Parameters...\n")
        log("GPU Support: {}".format("Yes" if device.type != "cpu" else "No"))
        log("Hidden Size fc1: {}".format(hidden_size_fc1))
        log("Embedding Size: {}".format(embedding_size))
        log("Starting Epoch: {}".format(TR.start_epoch))
        log("Total Epochs: {}".format(num_epochs))
        log("Batch Size: {}".format(in_batch_sz))
        log("Learning Rate: %g" % in_lr)
        log("Learning Rate Min: %g" % in_lr_min)
        log("Learning Rate Decay: %g" % in_lr_decay)
        log("Clades to train: {}".format(" ".join(str(c) for c in clades_to_train)
                                         if clades_to_train is not None else "all"))
        log("Random Seed: {}".format(seed))
        log("Cap kmer frequencies: {}".format(cap_data))
        log("\n==> Subtree training...\n")
        clade_order, clade_genomes = TR.read_subtrees(clades_info)
        class_count = list(clades_to_train) if clades_to_train is not None else clade_order
        log("Number of Classes: {}".format(len(class_count)))
        if not features_csv:
            raise ValueError("{}: no .kf file".format(features_folder))
        input_size = next((n for n in (TR._input_size(f) for f in features_csv) if n), 0)
        k = Q._k_of(input_size)
        feat_names = [os.path.basename(f).rsplit(".kf", 1)[0] for f in features_csv]
        path_name = os.path.split(features_csv[0])[0]
        from . import main as M
        threads = M.host_threads(os.cpu_count() or 1)

        for c in class_count:
            ids = set(clade_genomes.get(c, []))
            log("\n==> Working on subtree {}...\n".format(c))
            log("\n==> Preparing Data...\n")
            backbone_names = [nm for nm in feat_names if nm in ids]
            G = len(backbone_names)
            log("Dimensions of feature matrix rows: {}, cols: {}".format(G, input_size))
            if not backbone_names:
                raise ValueError("{}: no .kf file of clade {}".format(features_folder, c))
            dist_path = TR.find_true_dist(true_dist_matrix, c)
            missing = [os.path.join(input_dir_fullgenomes, nm + ".kf") for nm in backbone_names
                       if not os.path.isfile(os.path.join(input_dir_fullgenomes, nm + ".kf"))]
            if missing:
                raise ValueError("{}: no full-genome .kf file for {} genome{} of clade {}".format(
                    ", ".join(missing[:5]), len(missing), "" if len(missing) == 1 else "s", c))
            store = CH.chunk_store_from_kf(path_name, k, device, samples=backbone_names)
            if store.excluded:
                empty = [os.path.join(path_name, nm + ".kf") for nm in backbone_names if nm in store.excluded]
                raise ValueError("{}: no window row: every genome of clade {} needs at least one ({} file{} without)"
                                 .format(", ".join(empty[:5]), c, len(empty), "" if len(empty) == 1 else "s"))
            assert store.samples == backbone_names
            full = F.features_from_kf(input_dir_fullgenomes, k, device, samples=backbone_names, scaler=features_scaler,
                                      dtype=torch.float32)
            for nm, r in zip(backbone_names, np.diff(full.file_row0)):
                if int(r) != 1:
                    raise ValueError("{}: {} rows: a backbone genome's full-genome .kf file holds exactly one".format(
                        os.path.join(input_dir_fullgenomes, nm + ".kf"), int(r)))
            x_full = full.values
            table = T.true_distances(dist_path, backbone_names, device)
            P = table.values
            if tuple(P.shape) != (G, G):
                raise ValueError("{}: a matrix of {} x {} for {} genomes".format(dist_path, P.shape[0], P.shape[1], G))
            wrong = torch.nonzero(~(torch.isfinite(P) & (P >= 0)))
            if wrong.numel():
                r, q = (int(v) for v in wrong[0].tolist())
                raise ValueError("{}: the distance of {} and {} is {}: {} entr{} not finite or negative".format(
                    dist_path, backbone_names[r], backbone_names[q], float(P[r, q]), int(wrong.shape[0]),
                    "y is" if wrong.shape[0] == 1 else "ies are"))
            log("Dimensions of true distance matrix rows: {}, cols: {}".format(P.shape[0], P.shape[1]))
            rows = torch.arange(G, dtype=torch.int64, device=device)
            log("Number of Train Samples: {}".format(G))
            log("\n==> Building model...\n")
            torch.manual_seed(seed)
            model = Q.QueryNet(input_size, hidden_size_fc1, embedding_size)
            initial = {kk: v.detach().clone() for kk, v in model.state_dict().items()} if keep else None
            model = model.to(device)
            log("\n==> Model parameters----------")
            log("Total parameters: {}".format(sum(p.numel() for p in model.parameters())))
            log("Trainable parameters: {}".format(sum(p.numel() for p in model.parameters() if p.requires_grad)))
            optimizer = torch.optim.Adam(model.parameters(), lr=in_lr)
            gen = torch.Generator(device=device)
            gen.manual_seed(seed)
            log("Time: {}".format(stamp()))
            log("\n==> Training model...\n")
            plan = TR.batch_plan(G, in_batch_sz)
            total_step = len(plan)
            stop_epochs = stopping_epochs(G, max(1, int(in_batch_sz)))
            log("Stopping epochs: {}".format(stop_epochs))
            lowest_loss, best_epoch, best_state = math.inf, -1, None
            losses, step_losses, states = [], [], []
            # the epoch's one read: every step's loss, then the sum of loss * b, then the status words
            buf = torch.zeros(total_step + 3, dtype=torch.float64, device=device)
            feat_status = torch.zeros(1, dtype=torch.int64, device=device)
            for epoch in range(num_epochs):
                model.train()
                buf.zero_()
                feat_status.zero_()
                perm = torch.randperm(G, generator=gen, device=device)
                for i, (images, labels) in enumerate(epoch_batches(store, rows, perm, plan, gen, features_scaler, cap,
                                                                   status=feat_status)):
                    outputs = model(images)
                    loss, status = TR.dist_loss_fn(outputs, P, labels, VIEWS, LOSS_EPS)
                    ld = loss.detach()
                    buf[i] = ld
                    buf[total_step] += ld * labels.shape[0]
                    buf[total_step + 1] += status[0]
                    optimizer.zero_grad()
                    loss.backward()
                    optimizer.step()
                buf[total_step + 2] = feat_status[0]
                host = buf.cpu().numpy()
                if host[total_step + 1] != 0:
                    raise N.NativeError("kf_dist_loss_views: a label outside the distance matrix (status 1)")
                if host[total_step + 2] != 0:
                    raise N.NativeError("kf_chunk_features: a run's rows lie outside the count matrix")
                steps = [float(v) for v in host[:total_step]]
                step_losses.append(steps)
                for line in epoch_lines(epoch, num_epochs, plan, steps):
                    log(line)
                train_loss = float(host[total_step]) / G
                losses.append(train_loss)
                if train_loss < lowest_loss:
                    lowest_loss, best_epoch = train_loss, epoch
                    best_state = {kk: v.detach().clone() for kk, v in model.state_dict().items()}
                if keep:
                    states.append({kk: v.detach().cpu() for kk, v in model.state_dict().items()})
                log("Epoch [{}/{}], Step [{}/{}], Train loss: {:.20f}, Time: {}".format(
                    epoch + 1, num_epochs, total_step, total_step, train_loss, stamp()))
                log("Epoch {}\t                   LR:{:.20f}".format(epoch + 1, optimizer.param_groups[0]["lr"]))
                lr = TR.lr_after_epoch(epoch, in_lr, in_lr_min, in_lr_decay)
                if lr is not None:
                    for group in optimizer.param_groups:
                        group["lr"] = lr
            log("Best Epoch [{}/{}], Lowest loss: {:.20f}".format(best_epoch + 1, num_epochs, lowest_loss))
            consec_best, consec_lowest = consecutive_best(losses, stop_epochs)
            log("Best consecutive Epoch [{}/{}], Lowest loss: {:.20f}".format(consec_best + 1, num_epochs,
                                                                              consec_lowest))
            if best_state is None:     # no epoch, or no loss below infinity (NaN from the first epoch on)
                best_state = {kk: v.detach().clone() for kk, v in model.state_dict().items()}
            torch.save(TR.checkpoint_state(input_size, hidden_size_fc1, embedding_size, best_state),
                       os.path.join(model_filepath, "model_subtree_{}.ckpt".format(c)))
            result = {"clade": c, "names": list(backbone_names), "losses": losses, "step_losses": step_losses,
                      "best_epoch": best_epoch, "lowest_loss": lowest_loss, "consecutive_best_epoch": consec_best,
                      "consecutive_lowest_loss": consec_lowest, "stop_epochs": stop_epochs, "initial": initial,
                      "states": states}
            model.eval()
            with T.FloatTableWriter(device, threads) as writer, torch.no_grad():
                model.load_state_dict(best_state)
                emb = model(x_full)
                dist = Q.sq_distances(emb, emb)
                writer.write(os.path.join(model_filepath, "distortions_subtree_{}.csv".format(c)), backbone_names, dist,
                             header=[""] + list(backbone_names), mode=T.KF_FLOAT_SHORTEST, eol="\n", nan_empty=True)
                writer.write(os.path.join(model_filepath, "embeddings_subtree_{}.csv".format(c)), backbone_names, emb,
                             mode=T.KF_FLOAT_SHORTEST, eol="\n", nan_empty=True)
                log("Dimensions of distortion matrix rows:{} cols:{}".format(dist.shape[0], dist.shape[1] + 1))
                log("Dimensions of embedding output rows:{} cols:{}".format(emb.shape[0], emb.shape[1] + 1))
                if keep:
                    result["embeddings"], result["distortions"] = emb.cpu(), dist.cpu()
                writer.drain()
            kept.append(result)
            del store, full, x_full, table, P, model, optimizer, best_state
            log("\n==> Training for subtree {} completed!\n".format(c))
            log("Time: {}".format(stamp()))
        log("\n==> Training Completed!\n")
        log("Time: {}".format(stamp()))
    return kept if keep else None


def train_model_set_chunks(args) -> None:
    """The `train_model_set_chunks` subcommand (kf2vec/main.py:934-957)."""
    import glob
    print("Running train_model_set_chunks")
    all_files = glob.glob(os.path.join(args.input_dir, "*.kf"))
    train_model_set_chunks_func(args.input_dir, args.input_dir_fullgenomes, all_files, args.subtrees, args.true_dist,
                                args.e, args.hidden_sz, args.embed_sz, args.batch_sz, args.lr, args.lr_min,
                                args.lr_decay, args.clade, args.seed, args.cap, args.o,
                                device=getattr(args, "device", None) or "cuda")
