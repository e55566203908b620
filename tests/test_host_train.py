"""CPU tests of train_model_set: the host statement train.dist_loss_host against
the reference's lines under torch autograd on the CPU (float64 inputs and a
float64 cdist as the truth, the reference's own float32 path as the yardstick);
the trainer's pure parts (batch plan, test-set partition, learning-rate
schedule, checkpoint) against values written out from the reference's lines;
the parser; the FSW refusal; and kf_dist_loss' C-ABI (every refusal before any
HIP call: fake non-null addresses, there is no device here)."""
import ctypes

import numpy as np
import pytest

import train_inputs


def fake(i, off=0):
    """A fake device address, aligned to 4 KiB plus `off`."""
    return (0x7000_0000_0000 + (i << 32)) + off


# ---------------------------------------------------------------- the host statement
def reference_lines(y, P, labels, dtype):
    """kf2vec/train_model_set.py:448-467 with losses.py:13-49 and utils.py:240-256
    under autograd on the CPU: (loss, the gradient with respect to the embeddings)."""
    import torch
    yt = torch.from_numpy(np.asarray(y)).to(dtype).requires_grad_(True)
    real_dist = torch.from_numpy(P[np.ix_(list(labels), list(labels))])            # pairwise_true_dist
    train_dist = torch.cdist(yt, yt, p=2, compute_mode="donot_use_mm_for_euclid_dist")
    weight = 1 / (real_dist + 1e-6)
    true_dist = torch.sqrt(real_dist)
    loss = ((train_dist - true_dist) ** 2 * weight).mean()
    loss.backward()
    return float(loss.detach().to(torch.float64)), yt.grad.detach().to(torch.float64).numpy()


@pytest.mark.parametrize("B,E", [(1, 5), (2, 3), (7, 1), (16, 1024), (65, 33)])
def test_dist_loss_host_is_as_accurate_as_the_reference(B, E):
    """Loss error and largest gradient error of the host statement against the
    float64 truth, at most twice the error of the reference's own float32 path
    against the same truth (measured here, not fixed in advance); where both are
    exactly 0, equal.  The factor 2 allows for a different but equally valid
    order of the sums.
    Both errors are a few roundings of float32, and at the small shapes one input
    holds a handful of values: at (2, 3) the gradient has 6 entries, and either
    path lands up to ten times nearer the truth than the other from one input to
    the next (of 16 inputs the statement's gradient error is above twice the
    reference's in 4, each time by about one unit of float32, and below half of
    it in as many).  So the factor 2 is asserted
      - over DRAWS seeded inputs per shape: the statement's worst error against
        twice the reference's worst error on the same inputs; and
      - on every input, down to a floor that no correct float32 evaluation of the
        contract's lines is held to, worked out from the roundings on the way to
        one value, each at most 2^-24 relative.  A gradient entry: the two g, their
        sum, the division, the difference and the product (6), the square root
        and the E additions under it, halved by the root (1 + E / 2), and B
        additions of terms: (8 + B + E / 2) * 2^-24 of the largest entry.  The
        loss: its float64 sums add nothing at this scale; d_ij carries (1 + E / 2)
        * 2^-24 relative, which moves v_ij by 2 |u| w times that: the floor is the
        mean of 2 |u| w d over the pairs times (1 + E / 2) * 2^-24, over the loss."""
    import torch
    from kf2vecfsw_amd import train as TR
    U = 2.0 ** -24
    host_err = ref_err = host_gerr = ref_gerr = 0.0
    for seed in range(DRAWS):
        y, P, labels = train_inputs.make(B, E, seed)
        true_loss, true_grad = reference_lines(y, P, labels, torch.float64)
        ref_loss, ref_grad = reference_lines(y, P, labels, torch.float32)
        loss, grad = TR.dist_loss_host(y, P, labels)
        assert isinstance(loss, np.float64) and grad.dtype == np.float32 and grad.shape == (B, E)
        assert np.isfinite(loss) and np.isfinite(grad).all()
        scale = abs(true_loss) if true_loss != 0 else 1.0
        gscale = float(np.abs(true_grad).max()) or 1.0
        y64 = y.astype(np.float64)
        d = np.sqrt(((y64[:, None, :] - y64[None, :, :]) ** 2).sum(-1))
        T = P[np.ix_(labels, labels)]
        moved = float((2 * np.abs(d - np.sqrt(T)) / (T + 1e-6) * d).mean())
        loss_floor, grad_floor = moved * (1 + E / 2) * U / scale, (8 + B + E / 2) * U
        h, r = abs(float(loss) - true_loss) / scale, abs(ref_loss - true_loss) / scale
        hg = float(np.abs(grad.astype(np.float64) - true_grad).max()) / gscale
        rg = float(np.abs(ref_grad - true_grad).max()) / gscale
        assert h <= max(2 * r, loss_floor), (seed, h, r, loss_floor)
        assert hg <= max(2 * rg, grad_floor), (seed, hg, rg, grad_floor)
        host_err, ref_err, host_gerr, ref_gerr = max(host_err, h), max(ref_err, r), max(host_gerr, hg), max(ref_gerr, rg)
        if B == 1:
            assert float(loss) == 0.0 and not grad.any()
    print("B={} E={}: loss error {:.3g} (reference {:.3g}), gradient error {:.3g} (reference {:.3g})".format(
        B, E, host_err, ref_err, host_gerr, ref_gerr))
    assert host_err <= 2 * ref_err
    assert host_gerr <= 2 * ref_gerr


DRAWS = 16


def test_dist_loss_host_planted_values():
    """Two points at distance 5 whose true distance is 4 one way and 9 the other."""
    from kf2vecfsw_amd import train as TR
    y = np.array([[0, 0], [3, 4]], dtype=np.float32)
    P = np.array([[0, 4.0], [9.0, 0]])
    loss, grad = TR.dist_loss_host(y, P, [0, 1])
    w01, w10 = 1.0 / (4.0 + 1e-6), 1.0 / (9.0 + 1e-6)
    assert loss == ((0.0 + (3.0 * 3.0) * w01) + ((2.0 * 2.0) * w10 + 0.0)) * 0.25
    g = np.float32(((2.0 * 3.0) * w01) * 0.25) + np.float32(((2.0 * 2.0) * w10) * 0.25)
    c = g / np.float32(5)
    assert np.array_equal(grad, np.array([[c * np.float32(-3), c * np.float32(-4)],
                                          [c * np.float32(3), c * np.float32(4)]], dtype=np.float32))
    # a zero distance gives a zero gradient, whatever the true distance
    loss, grad = TR.dist_loss_host(np.ones((2, 3), np.float32), P, [1, 0])
    assert not grad.any() and loss == ((0.0 + 3.0 * 3.0 * w10) + (2.0 * 2.0 * w01 + 0.0)) * 0.25


# ---------------------------------------------------------------- the pure parts
def test_batch_plan():
    from kf2vecfsw_amd import train as TR
    assert TR.batch_plan(5, 2) == [(0, 2), (2, 4), (4, 5)]          # a short last batch, of one row
    assert TR.batch_plan(3, 2) == [(0, 2), (2, 3)]
    assert TR.batch_plan(4, 2) == [(0, 2), (2, 4)]
    assert TR.batch_plan(3, 16) == [(0, 3)] and TR.batch_plan(0, 16) == []
    plan = TR.batch_plan(850, 16)
    assert len(plan) == 54 and plan[-1] == (848, 850)               # len(DataLoader) of 850 rows in batches of 16


def test_test_set_partition(tmp_path):
    from kf2vecfsw_amd import train as TR
    f = tmp_path / "test_set.txt"
    f.write_text("G2.kf\n  G4.fna  \nnobody\nG5\n")
    ids = TR.read_test_ids(str(f))
    assert ids == ["G2", "G4", "nobody", "G5"]                       # process_file: stripped, the extension cut
    names = ["G1", "G2", "G3", "G4", "G5"]
    # train_model_set.py:309-314
    train = [b for b in names if b not in ids]
    test = [b for b in names if b not in train]
    assert TR.split_names(names, ids) == (train, test) == (["G1", "G3"], ["G2", "G4", "G5"])
    assert TR.split_names(names, []) == (names, []) and TR.read_test_ids(None) == []


def test_learning_rate_schedule():
    from kf2vecfsw_amd import train as TR
    in_lr, lr_min, decay = 1e-5, 3e-6, 2000
    for epoch in (0, 100, 200, 7900, 8000):
        assert TR.lr_after_epoch(epoch, in_lr, lr_min, decay) == lr_min + in_lr * (0.1 ** (epoch / decay))
    assert TR.lr_after_epoch(0, in_lr, lr_min, decay) == lr_min + in_lr
    assert TR.lr_after_epoch(2000, 1e-3, 0.0, 2000) == 1e-3 * 0.1
    for epoch in (1, 99, 101, 7999):
        assert TR.lr_after_epoch(epoch, in_lr, lr_min, decay) is None


def test_checkpoint_keys_and_load(tmp_path):
    import torch
    from kf2vecfsw_amd import query as Q
    from kf2vecfsw_amd import train as TR
    torch.manual_seed(4)
    net = Q.QueryNet(32, 8, 5)
    state = TR.checkpoint_state(32, 8, 5, net.state_dict())
    # utils.save_trained_model (kf2vec/utils.py:358-371)
    assert list(state) == ["model_name", "model_input_size", "model_hidden_size_fc1", "model_embedding_size",
                           "state_dict"]
    assert (state["model_name"], state["model_input_size"], state["model_hidden_size_fc1"],
            state["model_embedding_size"]) == ("NeuralNet", 32, 8, 5)
    assert list(state["state_dict"]) == ["fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias"]
    assert all(v.device.type == "cpu" for v in state["state_dict"].values())
    path = str(tmp_path / "model_subtree_3.ckpt")
    torch.save(state, path)
    back = Q.load_model(path, "cpu")                                  # weights_only=True
    assert (back.fc1.in_features, back.fc1.out_features, back.fc2.out_features) == (32, 8, 5)
    for a, b in zip(back.state_dict().values(), net.state_dict().values()):
        assert torch.equal(a, b)


def test_subtrees_file_and_true_dist_lookup(tmp_path):
    import os
    from conftest import TOY
    from kf2vecfsw_amd import train as TR
    order, clades = TR.read_subtrees(os.path.join(TOY, "train_tree.subtrees"))
    assert order == [0, 1]
    assert clades == {0: ["G000830275", "G000402355"], 1: ["G001940645", "G001871415", "G000830295"]}
    d = tmp_path / "dist"
    d.mkdir()
    with pytest.raises(ValueError, match="_subtree_1.di_mtrx"):
        TR.find_true_dist(str(d), 1)
    (d / "t_subtree_1.di_mtrx").write_text("x")
    (d / "t_subtree_11.di_mtrx").write_text("x")
    assert TR.find_true_dist(str(d), 1) == str(d / "t_subtree_1.di_mtrx")
    (d / "u_subtree_1.di_mtrx").write_text("x")
    with pytest.raises(ValueError, match="2 files"):
        TR.find_true_dist(str(d), 1)


# ---------------------------------------------------------------- the CLI
def test_parser_lists_the_command_with_the_references_defaults():
    from kf2vecfsw_amd import main as M
    p = M.build_parser()
    assert "train_model_set " in p.format_help()
    a = p.parse_args(["train_model_set"])
    assert (a.e, a.hidden_sz, a.embed_sz, a.batch_sz, a.lr, a.lr_min, a.lr_decay, a.seed) == \
        (8000, 2048, 1024, 16, 0.00001, 3e-6, 2000, 28)
    assert (a.input_dir, a.test_set, a.true_dist, a.subtrees, a.clade, a.save_interval, a.o, a.device) == (None,) * 8
    assert (a.no_fsw, a.fswout_dim, a.base_dim) == (False, 512, 4) and a.func is M.train_model_set
    a = p.parse_args(["train_model_set", "-clade", "1", "3", "-no_fsw", "-save_interval", "10", "-device", "cuda:1"])
    assert (a.clade, a.no_fsw, a.save_interval, a.device) == ([1, 3], True, 10, "cuda:1")


def test_without_no_fsw_the_command_ends_with_the_fsw_message(tmp_path, capsys):
    from kf2vecfsw_amd import main as M
    from kf2vecfsw_amd import train as TR
    with pytest.raises(SystemExit) as e:
        M.main(["train_model_set", "-input_dir", str(tmp_path), "-o", str(tmp_path / "out")])
    assert e.value.code == TR.FSW_MESSAGE and "FSW" in TR.FSW_MESSAGE and "-no_fsw" in TR.FSW_MESSAGE
    assert "Running train_model_set" in capsys.readouterr().out
    assert not (tmp_path / "out").exists()
    with pytest.raises(SystemExit) as e:
        TR.train_model_set_func(str(tmp_path), [], "s", "t", 1, 8, 4, 2, 1e-3, 0.0, 2000, None, 28, str(tmp_path / "out"),
                                None, None)
    assert e.value.code == TR.FSW_MESSAGE


# ---------------------------------------------------------------- the C-ABI
def test_symbols_exported(native):
    from kf2vecfsw_amd import _native as N
    from kf2vecfsw_amd import build
    for s in ("kf_dist_loss", "kf_dist_loss_scratch_bytes", "kf_dist_loss_small_b", "kf_dist_loss_tile",
              "kf_dist_loss_depth", "kf_dist_loss_max_b"):
        assert hasattr(native, s) and s in N.SIGNATURES, s
    assert native.kf_dist_loss_max_b() >= 4096                       # a whole default clade in one batch
    assert 1 <= native.kf_dist_loss_small_b() < native.kf_dist_loss_max_b()
    assert native.kf_dist_loss_small_b() >= 16                       # the default batch is one workgroup
    assert native.kf_dist_loss_tile() > 0 and native.kf_dist_loss_depth() > 0
    assert "kf_distloss.hip" in build.SOURCES_HIP


def scratch_bytes(native, B):
    need = ctypes.c_uint64(12345)
    rc = native.kf_dist_loss_scratch_bytes(B, ctypes.byref(need))
    return rc, need.value


def test_scratch_bytes(native):
    from kf2vecfsw_amd import _native as N
    S, cap = native.kf_dist_loss_small_b(), native.kf_dist_loss_max_b()
    assert scratch_bytes(native, 1) == (N.KF_OK, 0) and scratch_bytes(native, S) == (N.KF_OK, 0)
    for B in (S + 1, 850, 4096, cap):
        assert scratch_bytes(native, B) == (N.KF_OK, 12 * B * B + 8 * B)
    assert scratch_bytes(native, 0) == (N.KF_EINVAL, 12345) and b"B == 0" in native.kf_last_error()
    assert scratch_bytes(native, cap + 1) == (N.KF_EINVAL, 12345) and b"rows at most" in native.kf_last_error()
    assert native.kf_dist_loss_scratch_bytes(16, None) == N.KF_EINVAL and b"null bytes" in native.kf_last_error()


REFUSALS = [
    ("B == 0", dict(B=0), b"B == 0"),
    ("E == 0", dict(E=0), b"E == 0"),
    ("B above the cap", dict(B="over"), b"rows at most"),
    ("B == 2^40", dict(B=1 << 40), b"rows at most"),
    ("E == 2^40", dict(E=1 << 40), b"columns at most"),
    ("N == 0", dict(N=0), b"N = 0"),
    ("N == 2^30", dict(N=1 << 30), b"N = "),
    ("null y", dict(y=None), b"null d_y"),
    ("null true", dict(P=None), b"null d_true"),
    ("null labels", dict(labels=None), b"null d_labels"),
    ("null loss", dict(loss=None), b"null d_loss"),
    ("null status", dict(status=None), b"null d_status"),
    ("null scratch", dict(scratch=None), b"null d_scratch"),
    ("y off by 2", dict(y=fake(1, 2)), b"misaligned d_y"),
    ("true off by 4", dict(P=fake(2, 4)), b"misaligned d_true"),
    ("labels off by 4", dict(labels=fake(3, 4)), b"misaligned d_labels"),
    ("loss off by 4", dict(loss=fake(4, 4)), b"misaligned d_loss"),
    ("grad off by 1", dict(grad=fake(5, 1)), b"misaligned d_grad"),
    ("status off by 2", dict(status=fake(6, 2)), b"misaligned d_status"),
    ("scratch off by 4", dict(scratch=fake(7, 4)), b"misaligned d_scratch"),
    ("scratch too small", dict(scratch_bytes="short"), b"needed"),
    ("no scratch bytes", dict(scratch_bytes=0), b"needed"),
    ("small B, misaligned grad", dict(B=16, scratch=None, scratch_bytes=0, grad=fake(5, 2)), b"misaligned d_grad"),
]


@pytest.mark.parametrize("what,kw,msg", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_dist_loss_refuses_before_any_hip_call(native, what, kw, msg):
    from kf2vecfsw_amd import _native as N
    B = 100
    a = dict(y=fake(1), B=B, E=16, P=fake(2), N=200, labels=fake(3), loss=fake(4), grad=fake(5), status=fake(6),
             scratch=fake(7), scratch_bytes=12 * B * B + 8 * B)
    a.update(kw)
    if a["B"] == "over":
        a["B"] = native.kf_dist_loss_max_b() + 1
    if a["scratch_bytes"] == "short":
        a["scratch_bytes"] = 12 * B * B + 8 * B - 1
    rc = native.kf_dist_loss(a["y"], a["B"], a["E"], a["P"], a["N"], a["labels"], a["loss"], a["grad"], a["status"],
                             a["scratch"], a["scratch_bytes"], None)
    assert rc == N.KF_EINVAL, what
    assert msg in native.kf_last_error(), native.kf_last_error()
