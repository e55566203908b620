"""A synthetic library for the train_model_set_chunks loop tests
(test_gpu_train_chunks_loop.py), on train_library.make's scheme: two clades of
k = 3 genomes, a `.subtrees` file, the clades' true distance matrices and the
list of files to hand to the trainer, every order a different seeded shuffle.
Added here: per genome a get_chunks `.kf` file of 1 to 12 window rows (raw
counts, written by the project's own writer) and a full-genome `.kf` file of
the windows' sum.  Every genome has a composition of its own that its windows
share, so two views of one genome lie nearer to each other than to any other
genome's: labels that are tiled and not interleaved compute something else.
Clade 7 has S / 2 + 5 genomes, S being kf_dist_loss_small_b() where the library
is made: a batch of all of them is 2 (S / 2 + 5) rows, on the tiled path.  The
matrices' entries off the diagonal are distinct and uniform in (50, 3000), where
Loss_chunks' 1000 tells."""
import os

import numpy as np

import train_library
from train_library import BIG, SMALL, K, matrix_text, shuffled

EXTRA = 5                            # genomes of the big clade above S / 2
WINDOW = 10000
SEED = 20251


def matrix(rng, n):
    """Symmetric, a zero diagonal, the entries above it pairwise distinct and uniform in (50, 3000)."""
    iu = np.triu_indices(n, 1)
    while True:
        v = rng.uniform(50.0, 3000.0, size=iu[0].size)
        if np.unique(v).size == v.size:
            break
    P = np.zeros((n, n), dtype=np.float64)
    P[iu] = v
    return P + P.T


def window_rows(rng, nbins, n_windows):
    """uint16 [n_windows, nbins]: the counts of a genome's windows, a composition of the genome's own."""
    comp = rng.dirichlet(np.full(nbins, 0.6))
    return rng.multinomial(WINDOW - K + 1, comp, size=n_windows).astype(np.uint16)


def make(root, seed=SEED):
    """Write the library under `root` (a pathlib directory).  Returns a dict: chunks, full and
    dist (directories), subtrees (path), files (the chunk files for
    train_model_set_chunks_func, the clades interleaved), clade ({clade: its names, sorted}),
    matrix_order and P ({clade: the names in the matrix file's order, and the matrix in that
    order}), rows ({name: its uint16 window rows}), S and G."""
    from kf2vecfsw_amd import chunks as CH
    from kf2vecfsw_amd import counter as C
    from kf2vecfsw_amd import main as M
    rng = np.random.default_rng(seed)
    S = train_library.small_b()
    G = S // 2 + EXTRA
    assert 2 * G > S and (G - 1) % 5 == 0 and (G - 1) % 4 == 0, \
        "{} genomes: runs B and C need batches of 5 and of 4 that leave one genome".format(G)
    nbins = C.num_bins(K)
    ids = rng.permutation(9000)[:G + 3] + 1000
    clade = {BIG: sorted("C{}".format(i) for i in ids[:G]), SMALL: sorted("C{}".format(i) for i in ids[G:])}
    chunks, full, dist = root / "chunks", root / "full", root / "dist"
    for d in (chunks, full, dist):
        d.mkdir()
    n_windows = {nm: int(rng.integers(1, 13)) for nm in clade[BIG] + clade[SMALL]}
    n_windows[clade[BIG][3]], n_windows[clade[BIG][8]] = 1, 12          # both ends are there
    rows = {}
    for nm in clade[BIG] + clade[SMALL]:
        r = window_rows(rng, nbins, n_windows[nm])
        rows[nm] = r
        text, _ = CH.format_rows_host(r, [nm + ".part_c.part_c_sliding__"], np.zeros(r.shape[0], np.int64),
                                      np.arange(r.shape[0], dtype=np.int64) * WINDOW, WINDOW, False)
        (chunks / (nm + ".kf")).write_bytes(text)
        (full / (nm + ".kf")).write_bytes(M.format_kf(nm, r.astype(np.uint32).sum(axis=0).astype(np.uint32)))
    both = shuffled(rng, clade[BIG] + clade[SMALL])
    subtree_order = {c: [nm for nm in both if nm in set(clade[c])] for c in clade}
    (dist / "x.subtrees").write_text("genome clade\n" + "".join(
        "{} {}\n".format(nm, BIG if nm in set(clade[BIG]) else SMALL) for nm in both))
    matrix_order, P = {}, {}
    for c in clade:
        matrix_order[c] = shuffled(rng, clade[c], subtree_order[c])
        P[c] = matrix(rng, len(clade[c]))
        (dist / "x_subtree_{}.di_mtrx".format(c)).write_text(matrix_text(matrix_order[c], P[c]))
    big = shuffled(rng, clade[BIG], subtree_order[BIG], matrix_order[BIG])
    small = shuffled(rng, clade[SMALL], subtree_order[SMALL], matrix_order[SMALL])
    names = list(big)
    for at, nm in zip((4, G // 2, G - 3), small):
        names.insert(at, nm)
    assert names[0] in clade[BIG] and names[-1] in clade[BIG]
    files = [os.path.join(str(chunks), nm + ".kf") for nm in names]
    return dict(chunks=str(chunks), full=str(full), dist=str(dist), subtrees=str(dist / "x.subtrees"), files=files,
                clade=clade, subtree_order=subtree_order, matrix_order=matrix_order, P=P, rows=rows, S=S, G=G)
