"""CPU tests of train_library.py, the synthetic library of test_gpu_train_loop.py:
what the loop tests rely on holds of the files as written, read back here by the
trainer's own pure parts (read_subtrees, find_true_dist, read_test_ids,
split_names, batch_plan) and by plain Python."""
import os

import numpy as np

import train_library


def test_the_library_as_written(native, tmp_path):
    from kf2vecfsw_amd import counter as C
    from kf2vecfsw_amd import train as TR
    lib = train_library.make(tmp_path)
    S, G = lib["S"], lib["G"]
    big, small = train_library.BIG, train_library.SMALL
    assert S == native.kf_dist_loss_small_b() and G == S + 9 and (G - 1) % 5 == 0
    assert len(lib["clade"][big]) == G and len(lib["clade"][small]) == 3 and len(lib["files"]) == G + 3
    # the four orders of the big clade: all of the same names, pairwise different
    order, clades = TR.read_subtrees(lib["subtrees"])
    assert sorted(order) == [small, big] and clades[big] == lib["subtree_order"][big]
    path = TR.find_true_dist(lib["dist"], big)
    lines = open(path).read().splitlines()
    head = lines[0].split("\t")
    assert head[0] == "" and head[1:] == [ln.split("\t")[0] for ln in lines[1:]] == lib["matrix_order"][big]
    listed = [os.path.basename(f)[:-3] for f in lib["files"]]
    handed = [nm for nm in listed if nm in set(clades[big])]
    orders = [sorted(handed), clades[big], head[1:], handed]
    assert all(sorted(o) == orders[0] for o in orders) and len(set(orders[0])) == G
    assert all(orders[i] != orders[j] for i in range(4) for j in range(i))
    # the clades interleaved in the list: the small clade's files are apart, and inside
    at = [i for i, nm in enumerate(listed) if nm in set(clades[small])]
    assert len(at) == 3 and 0 < at[0] and at[0] + 1 < at[1] and at[1] + 1 < at[2] < len(listed) - 1
    # the matrix: repr round-trips, symmetric, a zero diagonal, distinct entries inside (0.05, 3)
    P = np.array([[float(v) for v in ln.split("\t")[1:]] for ln in lines[1:]], dtype=np.float64)
    assert np.array_equal(P, lib["P"][big]) and np.array_equal(P, P.T) and not np.diagonal(P).any()
    off = P[np.triu_indices(G, 1)]
    assert np.unique(off).size == off.size and 0.05 < off.min() and off.max() < 3.0
    # the .kf files: one row of k = 3 frequencies under the file's name
    for f in lib["files"]:
        cells = open(f).read().rstrip("\n").split(",")
        assert cells[0] == os.path.basename(f)[:-3] and len(cells) == 1 + C.num_bins(train_library.K)
        assert abs(sum(float(v) for v in cells[1:]) - 1.0) < 1e-9
    # a second library from the same seed is the same library
    again = tmp_path / "again"
    again.mkdir()
    lib2 = train_library.make(again)
    assert [os.path.basename(f) for f in lib2["files"]] == [os.path.basename(f) for f in lib["files"]]
    assert open(lib2["subtrees"]).read() == open(lib["subtrees"]).read()
    assert open(TR.find_true_dist(lib2["dist"], big)).read() == open(path).read()
    # run C's batches: 13 of the clade in the test set leave train batches of 12, 12 and 4, test batches of 12 and 1
    ts = tmp_path / "test_set.txt"
    ts.write_text("".join(nm + ".kf\n" for nm in handed[3:16]) + clades[small][0] + ".kf\nnobody.kf\n")
    train, test = TR.split_names(handed, TR.read_test_ids(str(ts)))
    assert test == handed[3:16] and train == handed[:3] + handed[16:]
    if G == 41:
        assert [b - a for a, b in TR.batch_plan(len(train), 12)] == [12, 12, 4]
        assert [b - a for a, b in TR.batch_plan(len(test), 12)] == [12, 1]
        assert [b - a for a, b in TR.batch_plan(G, (G - 1) // 5)] == [8] * 5 + [1]
