"""train_classifier: the clade classifier of a library, trained on the device.

The reference's trainer (kf2vec/train_classifier_model.py:77-514) goes through
the host three times per step: `loss_b.item()`, `accuracy_score` on copies of
the classes, and a numpy gather of the batch's classes that is copied up; and at
every improving epoch it runs `model.to('cpu')`, torch.save and `.to(device)`.
Its loss is log_softmax, NLLLoss, their two backward nodes, exp and topk.  Here
the features (features.features_from_kf) and the classes stay on the device,
the batches come from a device randperm, and a step is two index_selects, the
forward pass, kf_class_loss -- the batch's loss, its gradient with respect to
the logits, the count of right classes and the epoch's running totals in one
call -- the backward pass and the optimiser step.  Nothing inside an epoch waits
for the device: the three totals are read once, at its end.  The best model is
kept as a device copy of the parameters and written once;
backbone_classes.out is computed (classify.class_probs) and written as text
(tables.FloatTableWriter) on the device.
"""
from __future__ import annotations

import math
import os
import sys
import time

import numpy as np
import torch

from . import _native as N
from . import classify as CL
from . import counter as C
from . import features as F
from . import query as Q
from . import tables as T
from . import train as TR

features_scaler = 1e4                  # train_classifier_model.py:69
start_epoch = 0                        # train_classifier_model.py:59

MASK_MESSAGE = ("train_classifier: -mask is not supported: the reference's mask reads vocabulary files from the "
                "working directory, and classify does not apply it")


# ---------------------------------------------------------------------------
# the loss
# ---------------------------------------------------------------------------
def class_loss_small_b() -> int:
    """Rows up to which kf_class_loss runs as one workgroup in one launch."""
    return int(N.lib().kf_class_loss_small_b())


def class_loss_max_b() -> int:
    """The most rows kf_class_loss takes in one call."""
    return int(N.lib().kf_class_loss_max_b())


def class_loss_scratch_bytes(b: int) -> int:
    import ctypes
    need = ctypes.c_uint64(0)
    N.check(N.lib().kf_class_loss_scratch_bytes(int(b), ctypes.byref(need)), "kf_class_loss_scratch_bytes")
    return int(need.value)


def class_loss(logits: torch.Tensor, true: torch.Tensor, grad: bool = True, totals: torch.Tensor | None = None,
               stream: int | None = None):
    """Enqueue kf_class_loss: logits [B, C] float32 (the output of fc3) and true
    [B] int64, on one device.  Returns (loss float64 [], grad float32 [B, C] or
    None, row_loss float32 [B], hits int32 [1], status int32 [1]) on the device:
    the mean of the rows' negative log likelihood, its gradient with respect to
    the logits, the rows' own values, the count of rows whose largest
    probability is the true class's (kf_class_probs' top rule), and 1 if a class
    is outside [0, C) (the loss is then NaN).  grad=False: the same without the
    gradient, the same bits.  totals: a float64 [3] tensor on the device, to
    which the call adds loss * B, hits and status; calls that share one must go
    on one stream.  class_loss_host states it in numpy.  Nothing waits."""
    assert logits.dim() == 2 and logits.dtype == torch.float32
    assert true.dim() == 1 and true.dtype == torch.int64 and true.shape[0] == logits.shape[0]
    assert logits.device == true.device
    logits, true = logits.contiguous(), true.contiguous()
    dev = logits.device
    b, c = int(logits.shape[0]), int(logits.shape[1])
    if totals is not None:
        assert totals.dtype == torch.float64 and totals.numel() == 3 and totals.is_contiguous()
        assert totals.device == dev
    loss = torch.empty((), dtype=torch.float64, device=dev)
    counts = torch.empty(2, dtype=torch.int32, device=dev)       # hits, status
    row_loss = torch.empty(b, dtype=torch.float32, device=dev)
    g = torch.empty((b, c), dtype=torch.float32, device=dev) if grad else None
    need = class_loss_scratch_bytes(b) if b else 0
    scratch = torch.empty((need + 7) // 8, dtype=torch.int64, device=dev) if need else None
    s = C._stream_ptr(dev) if stream is None else stream
    with torch.cuda.device(dev):
        N.check(N.lib().kf_class_loss(logits.data_ptr() if logits.numel() else None, b, c,
                                      true.data_ptr() if b else None, loss.data_ptr(),
                                      g.data_ptr() if g is not None else None, row_loss.data_ptr() if b else None,
                                      counts[0:].data_ptr(), counts[1:].data_ptr(),
                                      totals.data_ptr() if totals is not None else None,
                                      scratch.data_ptr() if scratch is not None else None,
                                      8 * scratch.numel() if scratch is not None else 0, s), "kf_class_loss")
    if stream is not None and scratch is not None:   # the scratch is the caller's stream's until the call is done
        scratch.record_stream(torch.cuda.ExternalStream(stream, device=dev))
    return loss, g, row_loss, counts[0:1], counts[1:2]


def loss_of_rows(row_loss) -> np.float64:
    """The contract's sum: from 0.0, the rows' float32 values widened to float64 and added
    with i ascending, times 1 / B."""
    rows = np.asarray(row_loss, dtype=np.float32).astype(np.float64)
    total = np.float64(0.0)
    with np.errstate(all="ignore"):
        for v in rows:
            total = total + v
        return np.float64(total * (1.0 / float(len(rows))))


def class_loss_host(logits, true):
    """The host statement of kf_class_loss in numpy (include/kf2vec_gpu.h has the
    contract): the softmax and the negative log likelihood of every row in
    float64 from the float32 logits; the gradient as p rounded to float32, the
    one-hot subtracted and times float32(1 / B) in float32; the hits by
    classify.class_probs_host's top rule; the loss as the contract's sum of
    float32(nll_i).  Returns (loss float64, grad float32 [B, C], nll float64 [B],
    hits int).  A refused row (NaN, +inf, all -inf) is NaN in nll and in its
    gradient row and no hit.  The classes must be inside [0, C).  The tests
    compare the kernel with it; no product path calls it."""
    x = np.ascontiguousarray(logits, dtype=np.float32)
    cls = np.asarray(true, dtype=np.int64).reshape(-1)
    assert x.ndim == 2 and x.shape[0] == cls.shape[0] and x.shape[0] > 0 and x.shape[1] > 0
    assert cls.min() >= 0 and cls.max() < x.shape[1]
    b, c = x.shape
    out, top = CL.class_probs_host(x)
    p = out[:, 1:]
    bad = np.isnan(out[:, 0])
    onehot = np.zeros((b, c), dtype=np.float32)
    onehot[np.arange(b), cls] = 1.0
    x64 = x.astype(np.float64)
    with np.errstate(all="ignore"):
        grad = ((p - onehot) * (np.float32(1.0) / np.float32(b))).astype(np.float32)
        m = np.max(np.where(np.isnan(x64), -np.inf, x64), axis=1)
        t = x64 - m[:, None]
        nll = np.log(np.exp(t).sum(axis=1)) - t[np.arange(b), cls]
    nll[bad] = np.nan
    hits = int(np.count_nonzero((top == cls) & ~bad))
    return loss_of_rows(nll.astype(np.float32)), grad, nll, hits


class ClassLoss(torch.autograd.Function):
    """kf_class_loss under autograd: forward returns (loss, hits, status);
    backward hands back the kernel's gradient times the upstream scalar."""

    @staticmethod
    def forward(ctx, logits, true, totals):
        loss, g, _, hits, status = class_loss(logits.detach(), true, grad=True, totals=totals)
        ctx.save_for_backward(g)
        ctx.mark_non_differentiable(hits, status)
        return loss, hits, status

    @staticmethod
    def backward(ctx, grad_loss, _grad_hits, _grad_status):
        (g,) = ctx.saved_tensors
        # as DistLoss: a cast and a product per step, on the device, so that a scaled loss gives a scaled gradient
        # without a read of the upstream scalar (which would wait for the device)
        return g * grad_loss.to(torch.float32), None, None


def class_loss_fn(logits: torch.Tensor, true: torch.Tensor, totals: torch.Tensor | None = None):
    """(loss, hits, status) of the batch, differentiable with respect to the logits."""
    return ClassLoss.apply(logits, true, totals)


# ---------------------------------------------------------------------------
# the pure parts of the trainer
# ---------------------------------------------------------------------------
batch_plan = TR.batch_plan
lr_after_epoch = TR.lr_after_epoch
read_subtrees = TR.read_subtrees


def checkpoint_state(input_size: int, hidden_size_fc1: int, class_count: int, state_dict) -> dict:
    """The reference's dictionary (train_classifier_model.py:370-377) with CPU
    tensors and Python ints, so that classify.load_classifier (weights_only)
    loads it; the keys of state_dict are the plain model's (fc1.*, fc3.*)."""
    return {"model_name": "NeuralNetClassifierOnly", "model_input_size": int(input_size),
            "model_hidden_size_fc1": int(hidden_size_fc1), "model_class_count": int(class_count),
            "state_dict": type(state_dict)((k, v.detach().to("cpu")) for k, v in state_dict.items())}


def backbone_header(class_count: int) -> list:
    """The header cells of backbone_classes.out (train_classifier_model.py:499-501)."""
    return ["genome", "true_class", "top_class", "top_p"] + [str(x) for x in range(int(class_count))]


def backbone_prefixes(names, true_classes, top_classes) -> list:
    """Each row's text in front of its probabilities: the genome, quoted as
    to_csv does, the true class as an int and the top class as the float that
    the reference's np.hstack makes of it."""
    return [T.quote_label(nm, "\t", "\n") + b"\t" + str(int(c)).encode() + b"\t" + repr(float(int(t))).encode()
            for nm, c, t in zip(names, true_classes, top_classes)]


def log_opening(features_folder, clades_info, gpu: bool, hidden_size_fc1, num_epochs, in_batch_sz, in_lr, in_lr_min,
                in_lr_decay, seed, custom_mask) -> list:
    """The log's messages up to the data (train_classifier_model.py:110-141)."""
    return ["\n==> Input arguments...\n", "Feature directory: {}".format(features_folder),
            "Clades information: {}".format(clades_info), "\n==> Parameters...\n",
            "GPU Support: {}".format("Yes" if gpu else "No"), "Hidden Size fc1: {}".format(hidden_size_fc1),
            "Starting Epoch: {}".format(start_epoch), "Total Epochs: {}".format(num_epochs),
            "Batch Size: {}".format(in_batch_sz), "Learning Rate: %g" % in_lr, "Learning Rate Min: %g" % in_lr_min,
            "Learning Rate Decay: %g" % in_lr_decay, "Random Seed: {}".format(seed), "Masking: {}".format(custom_mask),
            "\n==> Preparing Data...\n"]


def log_model(n_rows: int, input_size: int, class_count: int, parameters: int, trainable: int, stamp: str) -> list:
    """The messages from the feature matrix to the start of training (:151, :234-293)."""
    return ["Dimensions of feature matrix rows: {}, cols: {}".format(n_rows, input_size),
            "Number of Train Samples: {}".format(n_rows), "\n==> Building model...\n",
            "Number of Classes: {}".format(class_count), "\n==> Model parameters----------",
            "Total parameters: {}".format(parameters), "Trainable parameters: {}".format(trainable),
            "Time: {}".format(stamp), "\n==> Training model...\n"]


def log_epoch(epoch: int, num_epochs: int, total_step: int, train_loss: float, running_acc: float, stamp: str,
              lr: float) -> list:
    """An epoch's two messages (:394-395, :446-447); epoch counts from 0."""
    return ["Epoch [{}/{}], Step [{}/{}], Train loss: {:.20f}, {:.20f}, Time: {}".format(
        epoch + 1, num_epochs, total_step, total_step, train_loss, running_acc, stamp),
        "Epoch {}\t               LR:{:.20f}".format(epoch + 1, lr)]


def log_closing(best_epoch: int, num_epochs: int, lowest_loss: float, highest_acc: float, n_rows: int,
                class_count: int, stamp: str) -> list:
    """The messages behind the last epoch (:464-465, :505, :510-514)."""
    return ["Best Epoch [{}/{}], Lowest loss: {:.20f}, Highest accuracy: {:.20f}".format(
        best_epoch + 1, num_epochs, lowest_loss, highest_acc),
        "Dimensions of class output rows:{} cols:{}".format(n_rows, class_count + 4),
        "\n==> Training Completed!\n", "Time: {}".format(stamp)]


def clade_of_genomes(clades_info: str, names) -> list:
    """The clade of every genome of `names`, from the `.subtrees` file."""
    _, clade_genomes = read_subtrees(clades_info)
    where = {}
    for c, genomes in clade_genomes.items():
        for g in genomes:
            where[g] = c
    out = []
    for nm in names:
        if nm not in where:
            raise ValueError("{}: the genome {} is not in the file".format(clades_info, nm))
        out.append(where[nm])
    return out


# ---------------------------------------------------------------------------
# train_classifier
# ---------------------------------------------------------------------------
def train_classifier_model_func(features_folder, kf_files, clades_info, num_epochs, hidden_size_fc1, in_batch_sz,
                                in_lr, in_lr_min, in_lr_decay, seed, custom_mask, model_filepath, device="cuda",
                                keep: bool = False):
    """kf2vec/train_classifier_model.py:77-514 on the device.  kf_files: the
    `.kf` files of features_folder, one row each, in the order of the rows of
    backbone_classes.out; a genome's class is its clade in clades_info, and the
    class count the number of distinct clades, which must then be 0 .. C - 1.
    The model is classify.ClassifierNet under torch.manual_seed(seed), the
    optimiser Adam(lr=in_lr) with the reference's schedule (lr_after_epoch).  An
    epoch walks a device randperm of the rows (a generator seeded with `seed`)
    in batches of in_batch_sz, the last one short; a step is kf_class_loss
    between the forward and the backward pass, and adds to the epoch's three
    totals, which are read once, at its end.  Written to model_filepath:
    classifier_model.ckpt (the best epoch's parameters, once, at the end),
    backbone_classes.out for the best model, and the log
    train_classifier_<timestamp>.log, whose lines also go to stdout.
    Refused, with an error that names the file or the genome: -mask, a file of
    several rows, a genome that the `.subtrees` file lacks, a row of NaN
    features, a clade outside [0, C).
    keep=True (tests): returns a dict with the names, the classes, the losses
    and accuracies per epoch, the best epoch, and the logits, probabilities and
    top classes the file was written from (on the host)."""
    if custom_mask:
        raise SystemExit(MASK_MESSAGE)
    kf_files = list(kf_files)
    if not kf_files:
        raise ValueError("{}: no .kf file".format(features_folder))
    feat_names = [os.path.basename(f).rsplit(".kf", 1)[0] for f in kf_files]
    path_name = os.path.split(kf_files[0])[0]
    classes = clade_of_genomes(clades_info, feat_names)
    class_count = len(set(classes))
    for nm, c in zip(feat_names, classes):
        if not 0 <= c < class_count:
            raise ValueError("{}: the genome {} is in clade {}: with {} distinct clades the classes are 0 to {}".format(
                clades_info, nm, c, class_count, class_count - 1))
    torch.manual_seed(seed)
    torch.cuda.manual_seed_all(seed)
    since = time.time()
    device = torch.device(device)
    os.makedirs(model_filepath, exist_ok=True)
    log_path = os.path.join(model_filepath, "train_classifier_{}.log".format(time.strftime("%Y%m%d_%H%M%S")))
    with open(log_path, "w+") as logf:
        def log(msg):
            logf.write(msg + "\n")
            logf.flush()
            sys.stdout.write(msg + "\n")

        def stamp():
            return "{:02d}:{:02d}:{:02d}".format(*Q._hms(time.time() - since))

        for msg in log_opening(features_folder, clades_info, device.type != "cpu", hidden_size_fc1, num_epochs,
                               in_batch_sz, in_lr, in_lr_min, in_lr_decay, seed, bool(custom_mask)):
            log(msg)
        input_size = TR._input_size(kf_files[0])
        k = Q._k_of(input_size)
        store = F.features_from_kf(path_name, k, device, samples=feat_names, scaler=features_scaler,
                                   dtype=torch.float32)
        for nm, r in zip(feat_names, np.diff(store.file_row0)):
            if int(r) != 1:
                raise ValueError("{}: {} rows: a backbone genome's .kf file holds exactly one".format(
                    os.path.join(path_name, nm + ".kf"), int(r)))
        x_all = store.values
        nan_rows = torch.nonzero(torch.isnan(x_all).any(dim=1)).reshape(-1).tolist()
        if nan_rows:
            raise ValueError("{}: its features are NaN (an empty genome): the classifier would train to NaN "
                             "weights".format(os.path.join(path_name, feat_names[nan_rows[0]] + ".kf")))
        n = len(feat_names)
        true_all = torch.tensor(classes, dtype=torch.int64, device=device)
        torch.manual_seed(seed)
        model = CL.ClassifierNet(input_size, hidden_size_fc1, class_count).to(device)
        optimizer = torch.optim.Adam(model.parameters(), lr=in_lr)
        gen = torch.Generator(device=device)
        gen.manual_seed(seed)
        for msg in log_model(n, input_size, class_count, sum(p.numel() for p in model.parameters()),
                             sum(p.numel() for p in model.parameters() if p.requires_grad), stamp()):
            log(msg)
        plan = batch_plan(n, in_batch_sz)
        total_step = len(plan)
        lowest_loss, highest_acc, best_epoch, best_state = math.inf, -1, -1, None
        losses, accs = [], []
        acc = torch.zeros(3, dtype=torch.float64, device=device)      # loss * rows, hits, status
        for epoch in range(num_epochs):
            model.train()
            acc.zero_()
            perm = torch.randperm(n, generator=gen, device=device)
            for a, b in plan:
                rows = perm[a:b]
                images = x_all.index_select(0, rows)
                true_class = true_all.index_select(0, rows)
                loss, _, _ = class_loss_fn(model(images), true_class, acc)
                optimizer.zero_grad()
                loss.backward()
                optimizer.step()
            totals = acc.cpu().numpy()                                 # the epoch's one read
            if totals[2] != 0:
                raise N.NativeError("kf_class_loss: a class outside the model's classes (status 1)")
            train_loss, running_acc = float(totals[0]) / n, float(totals[1]) / n
            losses.append(train_loss)
            accs.append(running_acc)
            if train_loss < lowest_loss:
                lowest_loss, highest_acc, best_epoch = train_loss, running_acc, epoch
                best_state = {kk: v.detach().clone() for kk, v in model.state_dict().items()}
            for msg in log_epoch(epoch, num_epochs, total_step, train_loss, running_acc, stamp(),
                                 optimizer.param_groups[0]["lr"]):
                log(msg)
            lr = lr_after_epoch(epoch, in_lr, in_lr_min, in_lr_decay)
            if lr is not None:
                for group in optimizer.param_groups:
                    group["lr"] = lr
        if best_state is None:         # no epoch, or no loss below infinity (NaN from the first epoch on)
            best_state = {kk: v.detach().clone() for kk, v in model.state_dict().items()}
        torch.save(checkpoint_state(input_size, hidden_size_fc1, class_count, best_state),
                   os.path.join(model_filepath, "classifier_model.ckpt"))
        model.load_state_dict(best_state)
        model.eval()
        from . import main as M
        threads = M.host_threads(os.cpu_count() or 1)
        with T.FloatTableWriter(device, threads) as writer, torch.no_grad():
            logits = model(x_all)
            out, top = CL.class_probs(logits)
            top_host = top.cpu().numpy()
            writer.write(os.path.join(model_filepath, "backbone_classes.out"),
                         backbone_prefixes(feat_names, classes, top_host), out, header=backbone_header(class_count),
                         mode=T.KF_FLOAT_WIDENED, eol="\n", quoted=True)
            writer.drain()
        result = None
        if keep:
            result = {"names": list(feat_names), "classes": list(classes), "losses": losses, "accuracies": accs,
                      "best_epoch": best_epoch, "lowest_loss": lowest_loss, "highest_accuracy": highest_acc,
                      "logits": logits.cpu(), "probabilities": out.cpu(), "top": top_host.copy()}
        for msg in log_closing(best_epoch, num_epochs, lowest_loss, highest_acc, n, class_count, stamp()):
            log(msg)
    return result


def train_classifier(args) -> None:
    """The `train_classifier` subcommand (kf2vec/main.py:376-397)."""
    import glob
    kf_files = glob.glob(os.path.join(args.input_dir, "*.kf"))
    train_classifier_model_func(args.input_dir, kf_files, args.subtrees, args.e, args.hidden_sz, args.batch_sz, args.lr,
                                args.lr_min, args.lr_decay, args.seed, args.mask, args.o,
                                device=getattr(args, "device", None) or "cuda")
