"""A synthetic library for the train_model_set loop tests (test_gpu_train_loop.py):
two clades of k = 3 `.kf` files written by the project's own writer from seeded
counts, a `.subtrees` file, the clades' true distance matrices and the list of
files to hand to the trainer, with every order a different seeded shuffle, so
that a trainer which lines two of them up by position and not by name computes
something else.  Clade 7 has S + 9 genomes, S being kf_dist_loss_small_b() where
the library is made: a batch of all of them is on the tiled path, and S + 8 is
a multiple of 5.  Clade 2 has three.  No distance off the diagonal is zero: the
kernel tests plant that case, and here its weight of 1e6 would swamp the sums."""
import os

import numpy as np

K = 3
BIG, SMALL = 7, 2                    # the clades
EXTRA = 9                            # genomes of the big clade above S
SEED = 20240


def small_b() -> int:
    from kf2vecfsw_amd import _native as N
    return int(N.lib().kf_dist_loss_small_b())


def shuffled(rng, names, *others):
    """A shuffle of `names` that differs from the names as given and from every one of `others`."""
    names = list(names)
    while True:
        out = [names[i] for i in rng.permutation(len(names))]
        if out != names and all(out != list(o) for o in others):
            return out


def matrix(rng, n):
    """Symmetric, a zero diagonal, the entries above it pairwise distinct and uniform in (0.05, 3)."""
    iu = np.triu_indices(n, 1)
    while True:
        v = rng.uniform(0.05, 3.0, size=iu[0].size)
        if np.unique(v).size == v.size and v.min() > 0.05:
            break
    P = np.zeros((n, n), dtype=np.float64)
    P[iu] = v
    return P + P.T


def matrix_text(order, P):
    """The `.di_mtrx` layout: a header of the names behind an empty cell, then a name and its row, every value its repr."""
    lines = ["\t" + "\t".join(order)]
    for nm, row in zip(order, P):
        lines.append(nm + "\t" + "\t".join(repr(float(v)) for v in row))
    return "\n".join(lines) + "\n"


def make(root, seed=SEED):
    """Write the library under `root` (a pathlib directory).  Returns a dict: kf, dist and
    subtrees (paths), files (the list for train_model_set_func, the clades interleaved),
    clade ({clade: its names, sorted}), subtree_order ({clade: its names in the `.subtrees`
    file's order}), matrix_order and P ({clade: the names in the matrix file's row and column
    order, and the matrix in that order}), S and G."""
    from kf2vecfsw_amd import counter as C
    from kf2vecfsw_amd import main as M
    rng = np.random.default_rng(seed)
    S = small_b()
    G = S + EXTRA
    assert (G - 1) % 5 == 0, "S + 8 = {} is no multiple of 5: run B's batches need another split".format(G - 1)
    nbins = C.num_bins(K)
    ids = rng.permutation(9000)[:G + 3] + 1000                       # names that say nothing about any order
    clade = {BIG: sorted("L{}".format(i) for i in ids[:G]), SMALL: sorted("L{}".format(i) for i in ids[G:])}
    kf, dist = root / "kf", root / "dist"
    kf.mkdir()
    dist.mkdir()
    for nm in clade[BIG] + clade[SMALL]:
        (kf / (nm + ".kf")).write_bytes(M.format_kf(nm, rng.integers(1, 4000, nbins).astype(np.uint32)))
    # the .subtrees file: one shuffle of both clades' names together
    both = shuffled(rng, clade[BIG] + clade[SMALL])
    subtree_order = {c: [nm for nm in both if nm in set(clade[c])] for c in clade}
    (dist / "x.subtrees").write_text("genome clade\n" + "".join(
        "{} {}\n".format(nm, BIG if nm in set(clade[BIG]) else SMALL) for nm in both))
    # the matrices, each in an order of its own
    matrix_order, P = {}, {}
    for c in clade:
        matrix_order[c] = shuffled(rng, clade[c], subtree_order[c])
        P[c] = matrix(rng, len(clade[c]))
        (dist / "x_subtree_{}.di_mtrx".format(c)).write_text(matrix_text(matrix_order[c], P[c]))
    # the files handed over: the big clade in an order of its own, the small clade's files among them
    big = shuffled(rng, clade[BIG], subtree_order[BIG], matrix_order[BIG])
    small = shuffled(rng, clade[SMALL], subtree_order[SMALL], matrix_order[SMALL])
    names = list(big)
    for at, nm in zip((4, G // 2, G - 3), small):
        names.insert(at, nm)
    orders = [clade[BIG], subtree_order[BIG], matrix_order[BIG], [nm for nm in names if nm in set(clade[BIG])]]
    assert all(orders[i] != orders[j] for i in range(4) for j in range(i)) and all(sorted(o) == orders[0] for o in orders)
    assert names[0] in clade[BIG] and names[-1] in clade[BIG]
    files = [os.path.join(str(kf), nm + ".kf") for nm in names]
    return dict(kf=str(kf), dist=str(dist), subtrees=str(dist / "x.subtrees"), files=files, clade=clade,
                subtree_order=subtree_order, matrix_order=matrix_order, P=P, S=S, G=G)
