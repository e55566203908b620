"""CPU tests of chunk_train_library.py, the synthetic library of
test_gpu_train_chunks_loop.py: what the loop tests rely on holds of the files as
written; and the conditions those tests put on the inputs, checked here with the
reference's loop in float32 on the CPU standing in for the device's: the matrix
one place off against the names, eps = 1e-6 in place of 1000 and labels tiled
instead of interleaved each move every epoch's float64 loss by more than
100 * 4 d."""
import os

import numpy as np

import chunk_train_library
import test_gpu_train_chunks_loop as L


def test_the_library_as_written(native, tmp_path):
    from kf2vecfsw_amd import chunks as CH
    from kf2vecfsw_amd import counter as C
    from kf2vecfsw_amd import train as TR
    lib = chunk_train_library.make(tmp_path)
    S, G = lib["S"], lib["G"]
    big, small = chunk_train_library.BIG, chunk_train_library.SMALL
    assert S == native.kf_dist_loss_small_b() and G == S // 2 + 5 and 2 * G > S
    assert len(lib["clade"][big]) == G and len(lib["clade"][small]) == 3 and len(lib["files"]) == G + 3
    order, clades = TR.read_subtrees(lib["subtrees"])
    assert sorted(order) == [small, big] and clades[big] == lib["subtree_order"][big]
    path = TR.find_true_dist(lib["dist"], big)
    lines = open(path).read().splitlines()
    head = lines[0].split("\t")
    listed = [os.path.basename(f)[:-3] for f in lib["files"]]
    handed = [nm for nm in listed if nm in set(clades[big])]
    orders = [sorted(handed), clades[big], head[1:], handed]
    assert all(sorted(o) == orders[0] for o in orders) and len(set(orders[0])) == G
    assert all(orders[i] != orders[j] for i in range(4) for j in range(i))
    P = np.array([[float(v) for v in ln.split("\t")[1:]] for ln in lines[1:]], dtype=np.float64)
    assert np.array_equal(P, lib["P"][big]) and np.array_equal(P, P.T) and not np.diagonal(P).any()
    off = P[np.triu_indices(G, 1)]
    assert np.unique(off).size == off.size and 50 < off.min() and off.max() < 3000
    # the chunk files: 1 to 12 rows of raw k = 3 counts of a whole window, as the host parser reads them; the
    # full-genome file: one row of the frequencies of their sum
    nbins = C.num_bins(chunk_train_library.K)
    n_windows = []
    for f in lib["files"]:
        nm = os.path.basename(f)[:-3]
        rows, err = CH.parse_kf_rows_host(open(f, "rb").read(), nbins)
        rows = np.asarray(rows, dtype=np.uint16).reshape(-1, nbins)
        assert tuple(err) == (0, 0, 0) and np.array_equal(rows, lib["rows"][nm]) and 1 <= rows.shape[0] <= 12
        assert (rows.sum(axis=1) == chunk_train_library.WINDOW - chunk_train_library.K + 1).all()
        n_windows.append(rows.shape[0])
        cells = open(os.path.join(lib["full"], nm + ".kf")).read().rstrip("\n").split(",")
        total = rows.astype(np.uint64).sum(axis=0)
        assert cells[0] == nm and [float(v) for v in cells[1:]] == (total / total.sum()).tolist()
    assert min(n_windows) == 1 and max(n_windows) == 12 and max(r.max() for r in lib["rows"].values()) > 255
    assert [b - a for a, b in TR.batch_plan(G, 5)][-1] == 1 and [b - a for a, b in TR.batch_plan(G, 4)][-1] == 1


def test_the_conditions_on_the_inputs_hold_on_the_cpu(native, tmp_path):
    import torch
    from kf2vecfsw_amd import query as Q
    lib = chunk_train_library.make(tmp_path)
    inp = L.read_inputs(lib)
    cpu = torch.device("cpu")
    draws = L.epoch_draws(inp, cpu)
    torch.manual_seed(L.SEED)
    initial = Q.QueryNet(inp["full"].shape[1], L.HIDDEN, L.EMBED).state_dict()
    for run, (batch, cap) in L.run_plan(lib).items():
        feats = L.epoch_features(inp, draws, cap)
        l32, _ = L.restate(inp, draws, feats, initial, cpu, torch.float32, batch)
        l64, _ = L.restate(inp, draws, feats, initial, cpu, torch.float64, batch)
        d = max(abs(a - b) for a, b in zip(l32, l64))
        for key, kw in (("rolled", dict(P=np.roll(inp["P"], 1, axis=(0, 1)))), ("eps", dict(eps=1e-6)),
                        ("tiled", dict(tiled=True))):
            wrong, _ = L.restate(inp, draws, feats, initial, cpu, torch.float64, batch, **kw)
            moved = min(abs(a - b) for a, b in zip(wrong, l64))
            print("run {}: {}: the smallest move {!r}, d = {!r}: {:.1f} times 4 d".format(
                run, key, moved, d, moved / (4 * d) if d else float("inf")))
            assert moved > 100 * 4 * d, (run, key)
