"""classify: the clade of every query genome, computed and written as text on
the device.

The reference's classify (kf2vec/classify.py:57-129) reads a block of `.kf`
files through StringIO and pandas, runs the classifier (Linear, ReLU, Linear,
log_softmax; kf2vec/models.py:117-132) on the CPU, takes torch.exp of it and
topk(1), and appends `genome, top_class, top_p, p_0 .. p_{C-1}` per genome to
classes.out through np.hstack with the object column and csv.writer.  Here the
`.kf` text is parsed on the device (features.features_from_kf), the two Linear
layers run there in torch, and kf_class_probs turns the logits into the row
that the file holds behind its label and class: the softmax in the direct
form e_j / sum e (not exp(x - m - log s), which loses |x - m| units of float32
in small probabilities), the first index of the largest rounded probability,
and that probability in front.  One kf_format_float_rows call in
KF_FLOAT_WIDENED mode then writes the block's lines (tables.FloatTableWriter),
with the label and the class as each row's prefix.
"""
from __future__ import annotations

import os
import sys
import time

import numpy as np
import torch

from . import _native as N
from . import counter as C
from . import features as F
from . import tables as T

features_scaler = 1e4


# ---------------------------------------------------------------------------
# the classifier head
# ---------------------------------------------------------------------------
def class_probs_reg_cols() -> int:
    """Columns up to which kf_class_probs keeps a row in registers; above it the row is read three times."""
    return int(N.lib().kf_class_probs_reg_cols())


def class_probs_rows() -> int:
    """Rows per workgroup of kf_class_probs."""
    return int(N.lib().kf_class_probs_rows())


def class_probs(logits: torch.Tensor, stream: int | None = None):
    """Enqueue kf_class_probs on logits [Q, C] (float32 on the device): (out
    float32 [Q, C + 1], top int32 [Q]) on the device, out[r, 1 + j] the softmax
    of row r in the direct form, top[r] the first index of its largest rounded
    value and out[r, 0] that value.  A row with a NaN or +inf, or all -inf, is
    NaN throughout with top 0.  class_probs_host states it in numpy.  Nothing
    waits."""
    assert logits.dim() == 2 and logits.dtype == torch.float32
    logits = logits.contiguous()
    dev = logits.device
    q, c = int(logits.shape[0]), int(logits.shape[1])
    out = torch.empty((q, c + 1), dtype=torch.float32, device=dev)
    top = torch.empty(q, dtype=torch.int32, device=dev)
    s = C._stream_ptr(dev) if stream is None else stream
    with torch.cuda.device(dev):
        N.check(N.lib().kf_class_probs(logits.data_ptr() if q else None, q, c, out.data_ptr() if q else None,
                                       top.data_ptr() if q else None, s), "kf_class_probs")
    return out, top


def class_probs_host(logits):
    """The host statement of kf_class_probs in numpy: the softmax of every row
    of the float32 logits taken in float64 (m = max, e = exp(x - m), e / sum e)
    and rounded to float32; a row with a NaN or +inf, or all -inf, is NaN in all
    C + 1 outputs with top 0; top is the first index of the largest rounded
    value, out[:, 0] that value.  Returns (out float32 [Q, C + 1], top int32 [Q]).
    The kernel works in float32 and stays within (|x_j - m| + C + 8) * 2^-24
    relative of it (tests/test_gpu_classify.py); no product path calls it."""
    x = np.ascontiguousarray(logits, dtype=np.float32)
    assert x.ndim == 2 and x.shape[1] > 0
    q, c = x.shape
    out = np.full((q, c + 1), np.nan, dtype=np.float32)
    top = np.zeros(q, dtype=np.int32)
    if q == 0:
        return out, top
    x64 = x.astype(np.float64)
    with np.errstate(all="ignore"):
        m = np.max(np.where(np.isnan(x64), -np.inf, x64), axis=1)
        bad = np.isnan(x64).any(axis=1) | (x64 == np.inf).any(axis=1) | (m == -np.inf)
        ok = ~bad
        e = np.exp(x64[ok] - m[ok, None])
        p = (e / e.sum(axis=1, keepdims=True)).astype(np.float32)
    out[ok, 1:] = p
    top[ok] = np.argmax(p, axis=1).astype(np.int32)          # the first of equals
    out[ok, 0] = p[np.arange(p.shape[0]), top[ok]]
    return out, top


# ---------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------
class ClassifierNet(torch.nn.Module):
    """The classifier (kf2vec/models.py:117-132, NeuralNetClassifierOnly) with
    its parameter names, so the trainer's state_dict loads: Linear, ReLU,
    Linear.  forward returns the logits; the softmax is kf_class_probs'."""

    def __init__(self, input_size: int, hidden_size: int, num_classes: int):
        super().__init__()
        self.fc1 = torch.nn.Linear(input_size, hidden_size)
        self.fc3 = torch.nn.Linear(hidden_size, num_classes)
        self.relu = torch.nn.ReLU()

    def forward(self, x):
        return self.fc3(self.relu(self.fc1(x)))


def load_classifier(model_dir: str, device) -> ClassifierNet:
    """<model_dir>/classifier_model.ckpt (model_input_size, model_hidden_size_fc1, model_class_count, state_dict) on the device."""
    state = torch.load(os.path.join(model_dir, "classifier_model.ckpt"), map_location="cpu", weights_only=True)
    model = ClassifierNet(int(state["model_input_size"]), int(state["model_hidden_size_fc1"]),
                          int(state["model_class_count"]))
    model.load_state_dict(state["state_dict"])
    return model.to(device).eval()


def classes_header(class_count: int) -> list:
    """The header cells of classes.out (classify.py:96)."""
    return ["genome", "top_class", "top_p"] + [str(x) for x in range(int(class_count))]


# ---------------------------------------------------------------------------
# classify
# ---------------------------------------------------------------------------
def _blocks_by_dir(paths):
    """Consecutive files of one directory: [(directory, [sample names])], so that features_from_kf reads them in order."""
    out = []
    for q in paths:
        d, base = os.path.split(q)
        if not base.endswith(".kf"):
            raise ValueError("classify: {}: not a .kf file".format(q))
        if not out or out[-1][0] != d:
            out.append((d, []))
        out[-1][1].append(base[:-3])
    return out


def classify_func(features_folder, kf_files, model_dir, seed, out_dir, block_size: int = 4000, device="cuda",
                  keep: bool = False, p=None, times: dict | None = None):
    """kf2vec/classify.py:57-129 on the device.  kf_files: the `.kf` files to
    classify, in the order their rows are written, block_size files at a time.
    The classifier is <model_dir>/classifier_model.ckpt; its input size selects
    k.  Per block: the features (times 1e4, float32), the two Linear layers,
    kf_class_probs, one small copy of the classes to the host, and the block's
    lines appended to <out_dir>/classes.out: tab-separated, "\\r\\n" line ends, the
    header `genome, top_class, top_p, 0 .. C-1` first, then per row of the `.kf`
    files its index name (quoted as csv.writer does), the class as an int and
    C + 1 probabilities, each the repr of the float32 as a double.  A file of
    several rows gives several lines.  classes.out is removed first if it exists;
    with no input file it holds the header only, written without the device.
    The reference's messages go to <out_dir>/classification.log and to stderr.
    A block's copy to the host and file write run on a writer thread while the
    next block is read and computed.
    keep=True (tests): returns [(labels, logits, out, top)] per block, the tensors
    the file was written from, on the host.
    times (tools): a dict that receives the seconds spent per stage."""
    torch.manual_seed(seed)
    since = time.time()
    os.makedirs(out_dir, exist_ok=True)
    kf_files = list(kf_files)
    kept = []
    tm = {"read": 0.0, "forward": 0.0, "probs": 0.0, "format": 0.0}
    timed = times is not None

    with open(os.path.join(out_dir, "classification.log"), "w+") as logf:
        def log(msg):
            logf.write(msg + "\n")
            logf.flush()
            sys.stderr.write(msg + "\n")

        log("\n==> Input arguments...\n")
        log("Feature directory: {}".format(features_folder))
        log("Model: {}".format(model_dir))
        log("Seed: {}".format(seed))
        log("\n==> Building model...\n")
        classes_fname = os.path.join(out_dir, "classes.out")
        if os.path.exists(classes_fname):
            os.remove(classes_fname)
        if not kf_files:
            state = torch.load(os.path.join(model_dir, "classifier_model.ckpt"), map_location="cpu", weights_only=True)
            with open(classes_fname, "wb") as f:
                f.write(T.header_line(classes_header(state["model_class_count"])))
        else:
            device = torch.device(device)
            torch.cuda.manual_seed_all(seed)

            def lap(key, t0):
                if timed:                       # a stage's time needs the device to be done with it
                    torch.cuda.synchronize(device)
                    tm[key] += time.perf_counter() - t0
                return time.perf_counter()

            model = load_classifier(model_dir, device)
            from . import main as M
            from . import query as Q
            k = Q._k_of(model.fc1.in_features)
            header = classes_header(model.fc3.out_features)
            threads = M.host_threads(p if p is not None else os.cpu_count() or 1)
            block_size = max(1, int(block_size))
            with T.FloatTableWriter(device, threads) as writer, torch.no_grad():
                for z in range(0, len(kf_files), block_size):
                    t0 = time.perf_counter()
                    labels, parts = [], []
                    for d, samples in _blocks_by_dir(kf_files[z: z + block_size]):
                        store = F.features_from_kf(d, k, device, samples=samples, scaler=features_scaler,
                                                   dtype=torch.float32, p=p)
                        labels += list(store.names)
                        parts.append(store.values)
                    x = parts[0] if len(parts) == 1 else torch.cat(parts)
                    t0 = lap("read", t0)
                    logits = model(x)
                    t0 = lap("forward", t0)
                    out, top = class_probs(logits)
                    top_host = top.cpu().numpy()             # the labels need it: one small copy per block
                    t0 = lap("probs", t0)
                    prefixes = [T.quote_label(nm) + b"\t" + str(int(c)).encode() for nm, c in zip(labels, top_host)]
                    first = z == 0
                    writer.write(classes_fname, prefixes, out, header=header if first else None,
                                 mode=T.KF_FLOAT_WIDENED, append=not first, quoted=True)
                    lap("format", t0)
                    if keep:
                        kept.append((labels, logits.cpu(), out.cpu(), top_host.copy()))
                    del store, parts, x, logits, out, top
                writer.drain()
                if timed:
                    times.update(tm)
                    times.update(writer.times)
        log("\n==> Classification Completed!\n")
        log("Time: {:02d}:{:02d}:{:02d}".format(*_hms(time.time() - since)))
    return kept if keep else None


def _hms(seconds: float):
    return int(seconds // 3600), int(seconds % 3600 // 60), int(seconds % 3600 % 60)


def classify(args) -> None:
    """The `classify` subcommand (kf2vec/main.py:400-411)."""
    import glob
    kf_files = glob.glob(os.path.join(args.input_dir, "*.kf"))
    classify_func(args.input_dir, kf_files, args.model, args.seed, args.o, args.block,
                  getattr(args, "device", None) or "cuda")
