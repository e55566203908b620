"""A synthetic library for the train_classifier_chunks loop tests
(test_gpu_train_classifier_chunks.py), on chunk_train_library.make's scheme:
21 genomes at k = 3 in three clades 0, 1 and 2, seven each; per genome a
get_chunks `.kf` file of 1 to 12 window rows (raw counts, written by the
project's own writer) and a full-genome `.kf` file of the windows' sum; a
`.subtrees` file; and the list of files to hand to the trainer.  The file order,
the `.subtrees` order and the sorted order all differ.  Every clade has a
composition of its own that its genomes share, each with a bend of its own, so
the classes can be told from the features and classes that are one place off
against the names compute something else.  The compositions are uneven
(Dirichlet 0.6 over the 32 bins, 9,998 3-mers per window), so that many counts
lie above 255 and the cap changes the features."""
import os

import numpy as np

from train_library import K, shuffled

CLASSES = 3
PER_CLASS = 7
G = CLASSES * PER_CLASS
WINDOW = 10000
SEED = 20261


def make(root, seed=SEED):
    """Write the library under `root` (a pathlib directory).  Returns a dict: chunks and full
    (directories), subtrees (path), files (the chunk files for the trainer, in an order of
    their own), names (the genomes in that order), clade ({name: its clade}), subtree_order
    (the names in the `.subtrees` file's order) and rows ({name: its uint16 window rows})."""
    from kf2vecfsw_amd import chunks as CH
    from kf2vecfsw_amd import counter as C
    from kf2vecfsw_amd import main as M
    rng = np.random.default_rng(seed)
    nbins = C.num_bins(K)
    ids = rng.permutation(9000)[:G] + 1000
    sorted_names = sorted("C{}".format(i) for i in ids)
    by_class = shuffled(rng, sorted_names)
    clade = {nm: i // PER_CLASS for i, nm in enumerate(by_class)}
    chunks, full = root / "chunks", root / "full"
    for d in (chunks, full):
        d.mkdir()
    n_windows = {nm: int(rng.integers(1, 13)) for nm in sorted_names}
    n_windows[sorted_names[3]], n_windows[sorted_names[8]] = 1, 12      # both ends are there
    base = [rng.dirichlet(np.full(nbins, 0.6)) for _ in range(CLASSES)]
    rows = {}
    for nm in sorted_names:
        comp = 0.8 * base[clade[nm]] + 0.2 * rng.dirichlet(np.full(nbins, 0.6))
        r = rng.multinomial(WINDOW - K + 1, comp, size=n_windows[nm]).astype(np.uint16)
        rows[nm] = r
        text, _ = CH.format_rows_host(r, [nm + ".part_c.part_c_sliding__"], np.zeros(r.shape[0], np.int64),
                                      np.arange(r.shape[0], dtype=np.int64) * WINDOW, WINDOW, False)
        (chunks / (nm + ".kf")).write_bytes(text)
        (full / (nm + ".kf")).write_bytes(M.format_kf(nm, r.astype(np.uint32).sum(axis=0).astype(np.uint32)))
    subtree_order = shuffled(rng, sorted_names, by_class)
    subtrees = root / "x.subtrees"
    subtrees.write_text("genome clade\n" + "".join("{} {}\n".format(nm, clade[nm]) for nm in subtree_order))
    names = shuffled(rng, sorted_names, by_class, subtree_order)
    files = [os.path.join(str(chunks), nm + ".kf") for nm in names]
    return dict(chunks=str(chunks), full=str(full), subtrees=str(subtrees), files=files, names=names, clade=clade,
                subtree_order=subtree_order, rows=rows, G=G)
