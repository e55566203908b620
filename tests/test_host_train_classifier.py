"""CPU tests of train_classifier: the host statement
train_classifier.class_loss_host against the reference's lines under torch
autograd on the CPU in float64; kf_class_loss' C-ABI (every refusal before any
HIP call: fake non-null addresses, there is no device here); the checkpoint; the
parser; the inputs refused before the device is touched; and the log's messages
against the log of the reference's own run of the toy example."""
import ctypes
import os
import re

import numpy as np
import pytest

import class_inputs
from conftest import GOLDEN, TOY

GOLD = os.path.join(GOLDEN, "train_classifier")


def fake(i, off=0):
    """A fake device address, aligned to 4 KiB plus `off`."""
    return (0x7000_0000_0000 + (i << 32)) + off


# ---------------------------------------------------------------- the host statement
def reference_lines(x, true):
    """kf2vec/models.py:126-132 and train_classifier_model.py:326-342 under autograd on the
    CPU, on logits cast to float64: (loss, the gradient with respect to the logits, the
    rows' nll, the classes topk(1) names)."""
    import torch
    xt = torch.from_numpy(np.asarray(x)).to(torch.float64).requires_grad_(True)
    tt = torch.from_numpy(np.asarray(true))
    model_class = torch.nn.functional.log_softmax(xt, dim=1)
    loss = torch.nn.NLLLoss()(model_class, tt)
    loss.backward()
    rows = torch.nn.functional.nll_loss(model_class.detach(), tt, reduction="none")
    _, top_class = torch.exp(model_class.detach()).topk(1, dim=1)
    return float(loss.detach()), xt.grad.numpy(), rows.numpy(), top_class.numpy()[:, 0]


@pytest.mark.parametrize("B,C", [(1, 1), (1, 2), (2, 3), (16, 2), (16, 65), (5, 257), (70, 7), (3, 1025)])
def test_class_loss_host_against_torch_in_float64(B, C):
    """The loss to 2^-22 * (1 + max |t|) -- the float32 rounding of nll_i is the statement's
    only float32 step on the way to it, 2^-24 of a value of at most max |t| + log C -- and the
    gradient to 2^-23 absolute: p <= 1 rounded to float32 (2^-25), the subtraction (2^-25),
    the product with float32(1 / B).  -inf logits are taken as -40 here, so that the loss is
    finite; the GPU tests and the last lines cover the infinite one."""
    from kf2vecfsw_amd import train_classifier as TC
    x, true, where = class_inputs.make(B, C)
    fin = np.where(np.isinf(x), np.float32(-40.0), x)
    loss, grad, nll, hits = TC.class_loss_host(fin, true)
    t_loss, t_grad, t_rows, t_top = reference_lines(fin, true)
    assert isinstance(loss, np.float64) and grad.dtype == np.float32 and grad.shape == (B, C) and nll.dtype == np.float64
    tmax = float(np.abs(fin.astype(np.float64) - fin.max(axis=1, keepdims=True)).max())
    print("B={} C={}: loss {!r} (torch {!r}), max |t| {:.4g}".format(B, C, float(loss), t_loss, tmax))
    assert abs(float(loss) - t_loss) <= 2.0 ** -22 * (1 + tmax)
    assert np.abs(nll - t_rows).max() <= 2.0 ** -40 * (1 + tmax)            # float64 both: the same value
    assert np.abs(grad.astype(np.float64) - t_grad).max() <= 2.0 ** -23
    srt = np.sort(fin, axis=1)
    clear = np.ones(B, bool) if C == 1 else srt[:, -1] != srt[:, -2]
    assert hits <= B
    if clear.all():
        assert hits == int(np.count_nonzero(t_top == true))
    else:                                        # the planted tie: the statement names the first maximum, not the true one
        r = where["two maxima"]
        assert not clear[r] and np.count_nonzero(~clear) == 1
        assert hits == int(np.count_nonzero((np.argmax(fin, axis=1) == true)[clear]))
    # the planted rows as they are
    loss2, grad2, nll2, _ = TC.class_loss_host(x, true)
    if "-inf at the true class" in where:
        r = where["-inf at the true class"]
        assert nll2[r] == np.inf and loss2 == np.inf and grad2[r, true[r]] == -np.float32(1) / np.float32(B)
    if "-inf elsewhere" in where:
        r = where["-inf elsewhere"]
        assert np.isfinite(nll2[r]) and np.count_nonzero(grad2[r] == 0) >= 1
    if "spread 120" in where:
        r = where["spread 120"]
        assert 119.0 < nll2[r] < 121.0 + np.log(C) and grad2[r, true[r]] == -np.float32(1) / np.float32(B)


def test_class_loss_host_planted_values():
    from kf2vecfsw_amd import train_classifier as TC
    x = np.array([[0.0, 0.0], [np.log(3.0), 0.0]], dtype=np.float32)
    loss, grad, nll, hits = TC.class_loss_host(x, [1, 0])
    assert nll[0] == np.log(2.0) and abs(nll[1] - np.log(4.0 / 3.0)) < 1e-7 and hits == 1     # a tie names class 0
    assert loss == (0.0 + np.float64(np.float32(nll[0])) + np.float64(np.float32(nll[1]))) * 0.5
    p = np.float32(0.75)
    assert np.allclose(grad, np.array([[0.5, -0.5], [p - 1, 1 - p]], dtype=np.float32) * np.float32(0.5), atol=1e-7)
    # C == 1: p = 1, nll = 0, g = 0
    loss, grad, nll, hits = TC.class_loss_host(np.array([[3.5], [-2.0]], dtype=np.float32), [0, 0])
    assert loss == 0.0 and not grad.any() and not nll.any() and hits == 2
    # a refused row: NaN in its nll, its gradient row and the loss, no hit
    loss, grad, nll, hits = TC.class_loss_host(np.array([[np.nan, 1.0], [0.0, 1.0]], dtype=np.float32), [1, 1])
    assert np.isnan(loss) and np.isnan(grad[0]).all() and np.isnan(nll[0]) and np.isfinite(grad[1]).all() and hits == 1
    assert TC.loss_of_rows([1.0, 2.0, 4.0]) == 7.0 * (1.0 / 3.0)


# ---------------------------------------------------------------- the C-ABI
def test_symbols_exported(native):
    from kf2vecfsw_amd import _native as N
    from kf2vecfsw_amd import build
    for s in ("kf_class_loss", "kf_class_loss_scratch_bytes", "kf_class_loss_small_b", "kf_class_loss_max_b"):
        assert hasattr(native, s) and s in N.SIGNATURES, s
    assert 16 <= native.kf_class_loss_small_b() < native.kf_class_loss_max_b()   # the default batch is one workgroup
    assert native.kf_class_loss_max_b() >= 4096
    assert "kf_classloss.hip" in build.SOURCES_HIP and "kf_softmax.h" in build.DEPS and "kf_softmax.h" in build.HEADERS


def scratch_bytes(native, B):
    need = ctypes.c_uint64(12345)
    rc = native.kf_class_loss_scratch_bytes(B, ctypes.byref(need))
    return rc, need.value


def test_scratch_bytes(native):
    from kf2vecfsw_amd import _native as N
    S, cap = native.kf_class_loss_small_b(), native.kf_class_loss_max_b()
    assert scratch_bytes(native, 1) == (N.KF_OK, 0) and scratch_bytes(native, S) == (N.KF_OK, 0)
    for B in (S + 1, 850, 4001, cap):
        assert scratch_bytes(native, B) == (N.KF_OK, 8 * B)
    assert scratch_bytes(native, 0) == (N.KF_EINVAL, 12345) and b"B == 0" in native.kf_last_error()
    assert scratch_bytes(native, cap + 1) == (N.KF_EINVAL, 12345) and b"rows at most" in native.kf_last_error()
    assert native.kf_class_loss_scratch_bytes(16, None) == N.KF_EINVAL and b"null bytes" in native.kf_last_error()


REFUSALS = [
    ("B == 0", dict(B=0), b"B == 0"),
    ("C == 0", dict(C=0), b"C == 0"),
    ("C == 2^31", dict(C=1 << 31), b"2^31 columns"),
    ("C == 2^40", dict(C=1 << 40), b"2^31 columns"),
    ("B above the cap", dict(B="over"), b"rows at most"),
    ("B == 2^40", dict(B=1 << 40), b"rows at most"),
    ("null logits", dict(logits=None), b"null d_logits"),
    ("null true", dict(true=None), b"null d_true"),
    ("null loss", dict(loss=None), b"null d_loss"),
    ("null hits", dict(hits=None), b"null d_hits"),
    ("null status", dict(status=None), b"null d_status"),
    ("null scratch", dict(scratch=None), b"null d_scratch"),
    ("scratch too small", dict(scratch_bytes="short"), b"needed"),
    ("no scratch bytes", dict(scratch_bytes=0), b"needed"),
    ("logits off by 2", dict(logits=fake(1, 2)), b"misaligned d_logits"),
    ("true off by 4", dict(true=fake(2, 4)), b"misaligned d_true"),
    ("loss off by 4", dict(loss=fake(3, 4)), b"misaligned d_loss"),
    ("grad off by 1", dict(grad=fake(4, 1)), b"misaligned d_grad"),
    ("row_loss off by 2", dict(row_loss=fake(5, 2)), b"misaligned d_row_loss"),
    ("hits off by 2", dict(hits=fake(6, 2)), b"misaligned d_hits"),
    ("status off by 1", dict(status=fake(7, 1)), b"misaligned d_status"),
    ("totals off by 4", dict(totals=fake(8, 4)), b"misaligned d_totals"),
    ("scratch off by 4", dict(scratch=fake(9, 4)), b"misaligned d_scratch"),
    ("small B, misaligned grad", dict(B=16, scratch=None, scratch_bytes=0, grad=fake(4, 2)), b"misaligned d_grad"),
    ("small B, misaligned totals", dict(B=16, scratch=None, scratch_bytes=0, totals=fake(8, 4)), b"misaligned d_totals"),
]


@pytest.mark.parametrize("what,kw,msg", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_class_loss_refuses_before_any_hip_call(native, what, kw, msg):
    from kf2vecfsw_amd import _native as N
    B = 100
    assert B > native.kf_class_loss_small_b()
    a = dict(logits=fake(1), B=B, C=16, true=fake(2), loss=fake(3), grad=fake(4), row_loss=fake(5), hits=fake(6),
             status=fake(7), totals=fake(8), scratch=fake(9), scratch_bytes=8 * B)
    a.update(kw)
    if a["B"] == "over":
        a["B"] = native.kf_class_loss_max_b() + 1
    if a["scratch_bytes"] == "short":
        a["scratch_bytes"] = 8 * B - 1
    rc = native.kf_class_loss(a["logits"], a["B"], a["C"], a["true"], a["loss"], a["grad"], a["row_loss"], a["hits"],
                              a["status"], a["totals"], a["scratch"], a["scratch_bytes"], None)
    assert rc == N.KF_EINVAL, what
    assert msg in native.kf_last_error(), native.kf_last_error()


# ---------------------------------------------------------------- the pure parts
def test_checkpoint_round_trips_through_load_classifier(tmp_path):
    import torch
    from kf2vecfsw_amd import classify as CL
    from kf2vecfsw_amd import train as TR
    from kf2vecfsw_amd import train_classifier as TC
    torch.manual_seed(4)
    net = CL.ClassifierNet(32, 8, 3)
    state = TC.checkpoint_state(np.int64(32), 8, np.int64(3), net.state_dict())
    # train_classifier_model.py:370-377
    assert list(state) == ["model_name", "model_input_size", "model_hidden_size_fc1", "model_class_count", "state_dict"]
    assert state["model_name"] == "NeuralNetClassifierOnly"
    assert all(type(state[k]) is int for k in ("model_input_size", "model_hidden_size_fc1", "model_class_count"))
    assert list(state["state_dict"]) == ["fc1.weight", "fc1.bias", "fc3.weight", "fc3.bias"]
    assert all(v.device.type == "cpu" for v in state["state_dict"].values())
    torch.save(state, str(tmp_path / "classifier_model.ckpt"))
    back = CL.load_classifier(str(tmp_path), "cpu")                   # weights_only=True
    assert (back.fc1.in_features, back.fc1.out_features, back.fc3.out_features) == (32, 8, 3)
    for a, b in zip(back.state_dict().values(), net.state_dict().values()):
        assert torch.equal(a, b)
    assert TC.batch_plan is TR.batch_plan and TC.lr_after_epoch is TR.lr_after_epoch
    assert TC.read_subtrees is TR.read_subtrees


def test_parser_lists_the_command_with_the_references_defaults():
    from kf2vecfsw_amd import main as M
    p = M.build_parser()
    assert "train_classifier " in p.format_help()
    a = p.parse_args(["train_classifier"])
    assert (a.e, a.hidden_sz, a.batch_sz, a.lr, a.lr_min, a.lr_decay, a.seed) == (2000, 2048, 16, 1e-5, 3e-6, 2000, 28)
    assert (a.input_dir, a.subtrees, a.o, a.device) == (None,) * 4 and a.mask is False and a.func is M.train_classifier
    import argparse
    sub = [x for x in p._actions if isinstance(x, argparse._SubParsersAction)][0].choices["train_classifier"]
    assert "-mask" not in sub.format_help() and "-lr_decay" in sub.format_help()      # hidden, as in the reference
    a = p.parse_args(["train_classifier", "-mask", "-e", "10", "-device", "cuda:1"])
    assert (a.mask, a.e, a.device) == (True, 10, "cuda:1")


def kf_names(tmp_path, names):
    """Paths of `.kf` files that need not exist: what is refused here is refused before a file is read."""
    return [str(tmp_path / (nm + ".kf")) for nm in names]


def test_refused_before_the_device_is_touched(tmp_path, capsys):
    from kf2vecfsw_amd import main as M
    from kf2vecfsw_amd import train_classifier as TC
    subtrees = os.path.join(TOY, "train_tree.subtrees")
    names = ["G000830275", "G000402355", "G001940645"]
    out = tmp_path / "out"

    def run(files, clades, mask=False):
        return TC.train_classifier_model_func(str(tmp_path), files, clades, 1, 8, 16, 1e-5, 3e-6, 2000, 28, mask, str(out))

    # -mask
    with pytest.raises(SystemExit) as e:
        run(kf_names(tmp_path, names), subtrees, mask=True)
    assert e.value.code == TC.MASK_MESSAGE and "-mask" in TC.MASK_MESSAGE
    with pytest.raises(SystemExit) as e:
        M.main(["train_classifier", "-input_dir", str(tmp_path), "-subtrees", subtrees, "-o", str(out), "-mask"])
    assert e.value.code == TC.MASK_MESSAGE and capsys.readouterr().out == ""
    # a genome that the .subtrees file lacks
    with pytest.raises(ValueError) as e:
        run(kf_names(tmp_path, names + ["G999"]), subtrees)
    assert "G999" in str(e.value) and subtrees in str(e.value)
    # a clade outside [0, C): two distinct clades, 0 and 2
    odd = tmp_path / "odd.subtrees"
    odd.write_text("genome clade\nG000830275 0\nG000402355 2\nG001940645 2\n")
    with pytest.raises(ValueError) as e:
        run(kf_names(tmp_path, names), str(odd))
    assert "G000402355" in str(e.value) and "clade 2" in str(e.value) and str(odd) in str(e.value)
    # no file
    with pytest.raises(ValueError, match="no .kf file"):
        run([], subtrees)
    assert not out.exists()


# ---------------------------------------------------------------- the log
def masked(text):
    """A log with what differs from run to run masked: the time stamps, and the digits of the losses and accuracies."""
    text = re.sub(r"\d\d:\d\d:\d\d", "HH:MM:SS", text)
    text = re.sub(r"(Train loss|Lowest loss|Highest accuracy): \d+\.\d{20}(, \d+\.\d{20})?",
                  lambda m: m.group(1) + ": X" + (", X" if m.group(2) else ""), text)
    return text


def test_log_messages_match_the_references_log():
    """The messages of the reference's own run of the toy example (five genomes, k = 7, two
    clades, -e 10, on a machine without a GPU), from the trainer's own formatters."""
    from kf2vecfsw_amd import classify as CL
    from kf2vecfsw_amd import train as TR
    from kf2vecfsw_amd import train_classifier as TC
    names = [f for f in os.listdir(GOLD) if re.fullmatch(r"train_classifier_\d{8}_\d{6}\.log", f)]
    assert len(names) == 1
    gold = open(os.path.join(GOLD, names[0])).read()
    net = CL.ClassifierNet(8192, 2048, 2)
    count = sum(p.numel() for p in net.parameters())
    lines = TC.log_opening("./toy_example/train_tree_kf", "./toy_example/train_tree_newick/train_tree.subtrees", False,
                           2048, 10, 16, 1e-5, 3e-6, 2000, 28, False)
    lines += TC.log_model(5, 8192, 2, count, count, "00:00:06")
    lr = 1e-5
    for epoch in range(10):
        lines += TC.log_epoch(epoch, 10, 1, 0.5 / (epoch + 1), 0.4, "00:00:15", lr)
        lr = TR.lr_after_epoch(epoch, 1e-5, 3e-6, 2000) or lr
    lines += TC.log_closing(9, 10, 0.05, 1.0, 5, 2, "00:01:31")
    mine = "".join(ln + "\n" for ln in lines)
    assert masked(mine) == masked(gold)
    assert masked(gold) != gold and "LR:0.00001300000000000000" in mine           # the schedule's digits are compared
