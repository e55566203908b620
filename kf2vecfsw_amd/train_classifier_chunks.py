"""train_classifier_chunks: the clade classifier of a library, trained on random
runs of its genomes' 10-kbp windows, on the device.

The reference's trainer (kf2vec/train_classifier_model_chunks.py:76-567) reads
every genome's window rows with pandas under mp.Pool -- under -cap as uint8,
each count as min(count, 255) (utils.my_read_csv_chunk_capped), because this
trainer holds the whole library at once --, and per item and epoch its
Dataset_chunks_1row (datasets.py:244-259) draws one run of rows on a numpy
stream that every DataLoader worker forks, sums and normalises it in numpy, and
the step then goes through the host as train_classifier's does.  Here the window
rows stay on the device (chunks.chunk_store_from_kf; under -cap as uint8 rows
made by kf_rows_cap8, half the bytes), an epoch's runs are drawn there
(train_chunks.draw_runs, one per genome), the features are built there in slabs
of whole batches (train_chunks.epoch_batches: kf_chunk_features, or
kf_chunk_features8 over the uint8 store), and a step is the forward pass,
kf_class_loss, the backward pass and Adam's step, as in train_classifier.py.
Nothing inside an epoch waits for the device: the three totals and the feature
kernel's status word are read once, at its end.  The best state is kept on the
device and written once; backbone_classes.out is the best model on the
full-genome features (features.features_from_kf), written as text on the
device.
"""
from __future__ import annotations

import math
import os
import sys
import time

import numpy as np
import torch

from . import _native as N
from . import chunks as CH
from . import classify as CL
from . import features as F
from . import query as Q
from . import tables as T
from . import train as TR
from . import train_chunks as TC
from . import train_classifier as TCL

features_scaler = 1e4                  # train_classifier_model_chunks.py:68
VIEWS = 1                              # Dataset_chunks_1row
CAP = TC.CAP

MASK_MESSAGE = TCL.MASK_MESSAGE.replace("train_classifier:", "train_classifier_chunks:", 1)


def log_opening(features_folder, clades_info, gpu: bool, hidden_size_fc1, num_epochs, in_batch_sz, in_lr, in_lr_min,
                in_lr_decay, seed, custom_mask, cap_data) -> list:
    """The log's messages up to the data (train_classifier_model_chunks.py:113-149):
    train_classifier's, with the cap behind the mask."""
    lines = TCL.log_opening(features_folder, clades_info, gpu, hidden_size_fc1, num_epochs, in_batch_sz, in_lr,
                            in_lr_min, in_lr_decay, seed, custom_mask)
    at = lines.index("Masking: {}".format(custom_mask)) + 1
    return lines[:at] + ["Cap kmer frequencies: {}".format(cap_data)] + lines[at:]


def names_and_classes(features_folder, features_csv, clades_info):
    """(genome names in the files' order, their classes, the class count), with
    train_classifier's refusals: no file, a genome that the `.subtrees` file
    lacks, a clade outside [0, C)."""
    features_csv = list(features_csv)
    if not features_csv:
        raise ValueError("{}: no .kf file".format(features_folder))
    feat_names = [os.path.basename(f).rsplit(".kf", 1)[0] for f in features_csv]
    classes = TCL.clade_of_genomes(clades_info, feat_names)
    class_count = len(set(classes))
    for nm, c in zip(feat_names, classes):
        if not 0 <= c < class_count:
            raise ValueError("{}: the genome {} is in clade {}: with {} distinct clades the classes are 0 to {}".format(
                clades_info, nm, c, class_count, class_count - 1))
    return feat_names, classes, class_count


def train_classifier_model_chunks_func(features_folder, input_dir_fullgenomes, features_csv, clades_info, num_epochs,
                                       hidden_size_fc1, in_batch_sz, in_lr, in_lr_min, in_lr_decay, seed, custom_mask,
                                       cap_data, model_filepath, device="cuda", keep: bool = False):
    """kf2vec/train_classifier_model_chunks.py:76-567 on the device.  features_csv:
    the get_chunks `.kf` files of features_folder, in the order of the rows of
    backbone_classes.out; a genome's class is its clade in clades_info, and the
    class count the number of distinct clades, which must then be 0 .. C - 1.
    All files' window rows make one store (cap_data: uint8 rows, each count as
    min(count, 255)); every genome needs its `<name>.kf` of exactly one row in
    input_dir_fullgenomes, read before any epoch (its values are not filled).
    The model is classify.ClassifierNet under torch.manual_seed(seed), the
    optimiser Adam(lr=in_lr) with the reference's schedule.  An epoch is a
    device randperm of the genomes and then one run of window rows per genome
    (train_chunks.epoch_batches with views=1), both from one generator seeded
    with `seed`, in batches of in_batch_sz genomes, the last one short; a step
    is kf_class_loss between the forward and the backward pass.  There is no
    test set.  Written to model_filepath: classifier_model.ckpt (the best
    epoch's parameters, once, at the end), backbone_classes.out for the best
    model on the full-genome features, and the log
    train_classifier_<timestamp>.log, whose lines also go to stdout.
    Refused, with an error that names the file or the genome: -mask, a genome
    that the `.subtrees` file lacks, a clade outside [0, C), a chunk file of no
    row, a full-genome file that is missing or not of one row.
    keep=True (tests): what train_classifier's returns (the logits,
    probabilities and top classes are the full-genome rows'), and the initial
    parameters and those after every epoch (on the host)."""
    if custom_mask:
        raise SystemExit(MASK_MESSAGE)
    features_csv = list(features_csv)
    feat_names, classes, class_count = names_and_classes(features_folder, features_csv, clades_info)
    path_name = os.path.split(features_csv[0])[0]
    torch.manual_seed(seed)
    torch.cuda.manual_seed_all(seed)
    since = time.time()
    device = torch.device(device)
    os.makedirs(model_filepath, exist_ok=True)
    cap = CAP if cap_data else None
    log_path = os.path.join(model_filepath, "train_classifier_{}.log".format(time.strftime("%Y%m%d_%H%M%S")))
    with open(log_path, "w+") as logf:
        def log(msg):
            logf.write(msg + "\n")
            logf.flush()
            sys.stdout.write(msg + "\n")

        def stamp():
            return "{:02d}:{:02d}:{:02d}".format(*Q._hms(time.time() - since))

        for msg in log_opening(features_folder, clades_info, device.type != "cpu", hidden_size_fc1, num_epochs,
                               in_batch_sz, in_lr, in_lr_min, in_lr_decay, seed, bool(custom_mask), cap_data):
            log(msg)
        input_size = next((m for m in (TR._input_size(f) for f in features_csv) if m), 0)
        k = Q._k_of(input_size)
        n = len(feat_names)
        missing = [os.path.join(input_dir_fullgenomes, nm + ".kf") for nm in feat_names
                   if not os.path.isfile(os.path.join(input_dir_fullgenomes, nm + ".kf"))]
        if missing:
            raise ValueError("{}: no full-genome .kf file for {} genome{}".format(
                ", ".join(missing[:5]), len(missing), "" if len(missing) == 1 else "s"))
        store = CH.chunk_store_from_kf(path_name, k, device, samples=feat_names, cap8=bool(cap_data))
        if store.excluded:
            empty = [os.path.join(path_name, nm + ".kf") for nm in feat_names if nm in store.excluded]
            raise ValueError("{}: no window row: every genome needs at least one ({} file{} without)".format(
                ", ".join(empty[:5]), len(empty), "" if len(empty) == 1 else "s"))
        assert store.samples == feat_names
        full = F.features_from_kf(input_dir_fullgenomes, k, device, samples=feat_names, scaler=features_scaler,
                                  dtype=torch.float32)
        for nm, r in zip(feat_names, np.diff(full.file_row0)):
            if int(r) != 1:
                raise ValueError("{}: {} rows: a backbone genome's full-genome .kf file holds exactly one".format(
                    os.path.join(input_dir_fullgenomes, nm + ".kf"), int(r)))
        x_full = full.values
        true_all = torch.tensor(classes, dtype=torch.int64, device=device)
        rows = torch.arange(n, dtype=torch.int64, device=device)
        torch.manual_seed(seed)
        model = CL.ClassifierNet(input_size, hidden_size_fc1, class_count)
        initial = {kk: v.detach().clone() for kk, v in model.state_dict().items()} if keep else None
        model = model.to(device)
        optimizer = torch.optim.Adam(model.parameters(), lr=in_lr)
        gen = torch.Generator(device=device)
        gen.manual_seed(seed)
        for msg in TCL.log_model(n, input_size, class_count, sum(p.numel() for p in model.parameters()),
                                 sum(p.numel() for p in model.parameters() if p.requires_grad), stamp()):
            log(msg)
        plan = TCL.batch_plan(n, in_batch_sz)
        total_step = len(plan)
        lowest_loss, highest_acc, best_epoch, best_state = math.inf, -1, -1, None
        losses, accs, states = [], [], []
        acc = torch.zeros(4, dtype=torch.float64, device=device)      # loss * rows, hits, status; the feature status
        totals_dev = acc[:3]
        feat_status = torch.zeros(1, dtype=torch.int64, device=device)
        for epoch in range(num_epochs):
            model.train()
            acc.zero_()
            feat_status.zero_()
            perm = torch.randperm(n, generator=gen, device=device)
            for images, labels in TC.epoch_batches(store, rows, perm, plan, gen, features_scaler, cap,
                                                   status=feat_status, views=VIEWS):
                true_class = true_all.index_select(0, labels)
                loss, _, _ = TCL.class_loss_fn(model(images), true_class, totals_dev)
                optimizer.zero_grad()
                loss.backward()
                optimizer.step()
            acc[3] = feat_status[0]
            totals = acc.cpu().numpy()                                 # the epoch's one read
            if totals[2] != 0:
                raise N.NativeError("kf_class_loss: a class outside the model's classes (status 1)")
            if totals[3] != 0:
                raise N.NativeError("kf_chunk_features: a run's rows lie outside the count matrix")
            train_loss, running_acc = float(totals[0]) / n, float(totals[1]) / n
            losses.append(train_loss)
            accs.append(running_acc)
            if train_loss < lowest_loss:
                lowest_loss, highest_acc, best_epoch = train_loss, running_acc, epoch
                best_state = {kk: v.detach().clone() for kk, v in model.state_dict().items()}
            if keep:
                states.append({kk: v.detach().cpu() for kk, v in model.state_dict().items()})
            for msg in TCL.log_epoch(epoch, num_epochs, total_step, train_loss, running_acc, stamp(),
                                     optimizer.param_groups[0]["lr"]):
                log(msg)
            lr = TR.lr_after_epoch(epoch, in_lr, in_lr_min, in_lr_decay)
            if lr is not None:
                for group in optimizer.param_groups:
                    group["lr"] = lr
        if best_state is None:         # no epoch, or no loss below infinity (NaN from the first epoch on)
            best_state = {kk: v.detach().clone() for kk, v in model.state_dict().items()}
        torch.save(TCL.checkpoint_state(input_size, hidden_size_fc1, class_count, best_state),
                   os.path.join(model_filepath, "classifier_model.ckpt"))
        model.load_state_dict(best_state)
        model.eval()
        from . import main as M
        threads = M.host_threads(os.cpu_count() or 1)
        with T.FloatTableWriter(device, threads) as writer, torch.no_grad():
            logits = model(x_full)
            out, top = CL.class_probs(logits)
            top_host = top.cpu().numpy()
            writer.write(os.path.join(model_filepath, "backbone_classes.out"),
                         TCL.backbone_prefixes(feat_names, classes, top_host), out,
                         header=TCL.backbone_header(class_count), mode=T.KF_FLOAT_WIDENED, eol="\n", quoted=True)
            writer.drain()
        result = None
        if keep:
            result = {"names": list(feat_names), "classes": list(classes), "losses": losses, "accuracies": accs,
                      "best_epoch": best_epoch, "lowest_loss": lowest_loss, "highest_accuracy": highest_acc,
                      "logits": logits.cpu(), "probabilities": out.cpu(), "top": top_host.copy(), "initial": initial,
                      "states": states}
        for msg in TCL.log_closing(best_epoch, num_epochs, lowest_loss, highest_acc, n, class_count, stamp()):
            log(msg)
    return result


def train_classifier_chunks(args) -> None:
    """The `train_classifier_chunks` subcommand (kf2vec/main.py:960-967)."""
    import glob
    print("Running train_classifier_chunks")
    all_files = glob.glob(os.path.join(args.input_dir, "*.kf"))
    train_classifier_model_chunks_func(args.input_dir, args.input_dir_fullgenomes, all_files, args.subtrees, args.e,
                                       args.hidden_sz, args.batch_sz, args.lr, args.lr_min, args.lr_decay, args.seed,
                                       args.mask, args.cap, args.o, device=getattr(args, "device", None) or "cuda")
