"""query: the distances of query genomes to a clade's backbone and their
embeddings, computed and written as text on the device.

The reference's query (kf2vec/query.py:53-200) reads a block of `.kf` files with
`cat` and pandas, runs the clade's Linear-ReLU-Linear model on the CPU, takes
torch.cdist(..., compute_mode='donot_use_mm_for_euclid_dist') squared to the
backbone embeddings, and writes a Q x B distance table and a Q x E embedding
table per clade through .tolist() and csv.writer, one repr(float) at a time.
Here the `.kf` text is parsed on the device (features.features_from_kf), the
backbone is read there (tables.backbone_embeddings), the distances are
kf_sq_distances -- the same direct form with the order of the sum fixed -- and
both tables become text on the device (kf_format_float_rows in KF_FLOAT_WIDENED
mode: the repr of every float32 as a double, which is what .tolist() and
csv.writer print), copied through a pinned buffer and written by
kf_write_text_segments on a thread of its own while the next block is computed.
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
# distances
# ---------------------------------------------------------------------------
def sq_distances_tile() -> int:
    """Rows of x, and of y, per workgroup of kf_sq_distances."""
    return int(N.lib().kf_sq_distances_tile())


def sq_distances(x: torch.Tensor, y: torch.Tensor, stream: int | None = None) -> torch.Tensor:
    """Enqueue kf_sq_distances: out[i, j] = the squared Euclidean distance of
    x[i] and y[j] (float32 [Q, D] and [B, D] on the device) in the direct form,
    as query.py:169-176 leaves it: differences first, summed over d ascending,
    every operation rounded to float32, then sqrt, square, and values below 1e-6
    set to 0.  sq_distances_host states it in numpy, bit for bit."""
    assert x.dim() == 2 and y.dim() == 2 and x.shape[1] == y.shape[1]
    assert x.dtype == torch.float32 and y.dtype == torch.float32 and x.device == y.device
    x, y = x.contiguous(), y.contiguous()
    dev = x.device
    out = torch.empty((x.shape[0], y.shape[0]), dtype=torch.float32, device=dev)
    s = C._stream_ptr(dev) if stream is None else stream
    with torch.cuda.device(dev):
        N.check(N.lib().kf_sq_distances(x.data_ptr() if x.numel() else None, int(x.shape[0]),
                                        y.data_ptr() if y.numel() else None, int(y.shape[0]), int(x.shape[1]),
                                        out.data_ptr() if out.numel() else None, s), "kf_sq_distances")
    return out


def sq_distances_host(x, y) -> np.ndarray:
    """The host statement of kf_sq_distances in numpy float32, the same
    operations in the same order: s = 0; for d ascending: t = x_d - y_d, s = s +
    t * t; r = sqrt(s); v = r * r; v < 1e-6 -> 0."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    y = np.ascontiguousarray(y, dtype=np.float32)
    assert x.ndim == 2 and y.ndim == 2 and x.shape[1] == y.shape[1] and x.shape[1] > 0
    s = np.zeros((x.shape[0], y.shape[0]), dtype=np.float32)
    with np.errstate(all="ignore"):
        for d in range(x.shape[1]):
            t = x[:, d, None] - y[None, :, d]
            s = s + t * t
        r = np.sqrt(s)
        v = r * r
        return np.where(v < np.float32(1e-6), np.float32(0), v).astype(np.float32)


# ---------------------------------------------------------------------------
# classes.out and the remap table, without pandas
# ---------------------------------------------------------------------------
def _tsv_rows(path: str):
    """(header cells, rows of cells) of a tab-separated file with a header; empty lines are skipped."""
    with open(path, newline="") as f:
        lines = [ln for ln in f.read().splitlines() if ln.strip()]
    if not lines:
        raise ValueError("{}: no line".format(path))
    return lines[0].split("\t"), [ln.split("\t") for ln in lines[1:]]


def read_classes(path: str, genomes=None):
    """classes.out of the classify command (tab-separated, a header with `genome`
    and `top_class`), as query.py:84-90 uses it: [(clade, [genomes])] with the
    clades in order of first appearance and a clade's genomes in file order.
    top_class such as "0.0" becomes the int 0.  genomes: keep these only."""
    head, rows = _tsv_rows(path)
    try:
        gi, ci = head.index("genome"), head.index("top_class")
    except ValueError:
        raise ValueError("{}: the header needs the columns genome and top_class".format(path)) from None
    keep = None if genomes is None else set(genomes)
    clades: dict = {}
    for n, cells in enumerate(rows):
        if len(cells) <= max(gi, ci):
            raise ValueError("{}: row {}: {} cells".format(path, n, len(cells)))
        if keep is not None and cells[gi] not in keep:
            continue
        try:
            c = int(float(cells[ci]))
        except ValueError:
            raise ValueError("{}: row {}: top_class {!r}".format(path, n, cells[ci])) from None
        clades.setdefault(c, []).append(cells[gi])
    return list(clades.items())


def read_remap(path: str) -> dict:
    """The remap table (tab-separated, a header with `label` and `new_label`) as {label: new_label}."""
    head, rows = _tsv_rows(path)
    li, ni = head.index("label"), head.index("new_label")
    return {cells[li]: cells[ni] for cells in rows}


# ---------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------
class QueryNet(torch.nn.Module):
    """The distance trainers' network (kf2vec/models.py:35-49): Linear, ReLU, Linear."""

    def __init__(self, input_size: int, hidden_size: int, embedding_size: int):
        super().__init__()
        self.fc1 = torch.nn.Linear(input_size, hidden_size)
        self.relu = torch.nn.ReLU()
        self.fc2 = torch.nn.Linear(hidden_size, embedding_size)

    def forward(self, x):
        return self.fc2(self.relu(self.fc1(x)))


def load_model(path: str, device) -> QueryNet:
    """model_subtree_<c>.ckpt (model_input_size, model_hidden_size_fc1, model_embedding_size, state_dict) on the device."""
    state = torch.load(path, map_location="cpu", weights_only=True)
    model = QueryNet(int(state["model_input_size"]), int(state["model_hidden_size_fc1"]),
                     int(state["model_embedding_size"]))
    model.load_state_dict(state["state_dict"])
    return model.to(device).eval()


def _k_of(input_size: int) -> int:
    from . import main as M
    for k in M.supported_k:
        if C.num_bins(k) == input_size:
            return k
    raise ValueError("a model of input size {} matches no supported k".format(input_size))


def _hms(seconds: float):
    return int(seconds // 3600), int(seconds % 3600 // 60), int(seconds % 3600 % 60)


# ---------------------------------------------------------------------------
# query
# ---------------------------------------------------------------------------
def query_func(features_folder, kf_files, model_dir, classes_dir, seed, out_dir, remap=None, block_size: int = 4000,
               device="cuda", keep: bool = False, p=None, times: dict | None = None):
    """kf2vec/query.py:53-200 on the device.  kf_files: the `.kf` files of
    features_folder to query (their basenames select the rows of
    <classes_dir>/classes.out).  Per clade c of classes.out: the model
    <model_dir>/model_subtree_<c>.ckpt and the backbone
    <model_dir>/embeddings_subtree_<c>.csv; then, per block of block_size
    genomes, the features (times 1e4, float32), the forward pass, the squared
    distances to the backbone, and both tables appended to
    <out_dir>/apples_input_di_mtrx_subtree_<c>.csv (a header row: an empty cell,
    then the backbone names) and <out_dir>/embedding_subtree_<c>.emb (no header),
    tab-separated, "\\r\\n" line ends, every value the repr of the float32 as a
    double.  Rows are labelled with the `.kf` index names, remapped through the
    `remap` table if one is given.  The log lines go to <out_dir>/query_run.log
    and to stdout.  A block's copy to the host and file write run on a writer
    thread while the next block is read and computed.
    keep=True (tests): returns [(clade, labels, embeddings, distances)] per
    block, the tensors the files were written from, on the host.
    times (tools): a dict that receives the seconds spent per stage."""
    torch.manual_seed(seed)
    torch.cuda.manual_seed_all(seed)
    since = time.time()
    device = torch.device(device)
    os.makedirs(out_dir, exist_ok=True)
    kept = []
    tm = {"read": 0.0, "forward": 0.0, "distances": 0.0, "format": 0.0}
    timed = times is not None

    def lap(key, t0):
        if timed:                       # a stage's time needs the device to be done with it
            torch.cuda.synchronize(device)
            tm[key] += time.perf_counter() - t0
        return time.perf_counter()

    with open(os.path.join(out_dir, "query_run.log"), "w+") as logf:
        def log(msg):
            logf.write(msg + "\n")
            logf.flush()
            sys.stdout.write(msg + "\n")

        log("\n==> Input arguments...\n")
        log("Query directory: {}".format(features_folder))
        log("Model directory: {}".format(model_dir))
        log("Class information: {}".format(classes_dir))
        log("Seed: {}".format(seed))
        log("\n==> Querying...\n")
        basenames = [os.path.basename(q).split(".kf")[0] for q in kf_files]
        clades = read_classes(os.path.join(classes_dir, "classes.out"), basenames)
        log("Total subtrees to query: {}".format(len(clades)))
        remap_dict = None
        if remap:
            try:
                remap_dict = read_remap(remap)
                log("Remap loaded: {} entries".format(len(remap_dict)))
            except Exception as e:
                log("Could not read remap file {}: {}".format(remap, e))
                remap_dict = None
        from . import main as M
        threads = M.host_threads(p if p is not None else os.cpu_count() or 1)
        with T.FloatTableWriter(device, threads) as writer, torch.no_grad():
            for c, contig_ids in clades:
                log("\n==> Working on subtree {} ({} contigs)...\n".format(c, len(contig_ids)))
                model = load_model(os.path.join(model_dir, "model_subtree_{}.ckpt".format(c)), device)
                k = _k_of(model.fc1.in_features)
                backbone = T.backbone_embeddings(os.path.join(model_dir, "embeddings_subtree_{}.csv".format(c)), device)
                dist_path = os.path.join(out_dir, "apples_input_di_mtrx_subtree_{}.csv".format(c))
                emb_path = os.path.join(out_dir, "embedding_subtree_{}.emb".format(c))
                block_size = max(1, int(block_size))
                for z in range(0, len(contig_ids), block_size):
                    t0 = time.perf_counter()
                    store = F.features_from_kf(features_folder, k, device, samples=contig_ids[z: z + block_size],
                                               scaler=features_scaler, dtype=torch.float32, p=p)
                    labels = list(store.names)
                    if remap_dict is not None:
                        labels = [remap_dict.get(q, q) for q in labels]
                    t0 = lap("read", t0)
                    outputs = model(store.values)
                    t0 = lap("forward", t0)
                    dist = sq_distances(outputs, backbone.values)
                    t0 = lap("distances", t0)
                    first = z == 0
                    writer.write(dist_path, labels, dist, header=[""] + backbone.row_names if first else None,
                                 mode=T.KF_FLOAT_WIDENED, append=not first)
                    writer.write(emb_path, labels, outputs, mode=T.KF_FLOAT_WIDENED, append=not first)
                    lap("format", t0)
                    if keep:
                        kept.append((c, labels, outputs.cpu(), dist.cpu()))
                    del store, outputs, dist
                writer.drain()
                log("Wrote distance matrix: {}".format(dist_path))
                log("Wrote embeddings: {}".format(emb_path))
                log("\n==> Computation is completed for subtree {}!\n".format(c))
                log("Time: {:02d}:{:02d}:{:02d}".format(*_hms(time.time() - since)))
            if timed:
                times.update(tm)
                times.update(writer.times)
        log("\n==> Computation Completed!\n")
        log("Total time: {:02d}:{:02d}:{:02d}".format(*_hms(time.time() - since)))
    return kept if keep else None


def query(args) -> None:
    """The `query` subcommand (kf2vec/main.py:535-553)."""
    import glob
    kf_files = glob.glob(os.path.join(args.input_dir, "*.kf"))
    query_func(args.input_dir, kf_files, args.model, args.classes, args.seed, args.o, args.remap, args.block,
               args.device or "cuda")
