"""CPU tests of classify: kf_class_probs' C-ABI (every refusal before any HIP
call: fake non-null addresses, there is no device here); the host statement
class_probs_host against the reference's torch.exp(F.log_softmax(...)) on the
CPU and on planted rows; the parsers of `classify` and `process_query_data`;
ClassifierNet against a module with the reference's attribute names; and the
header-only classes.out of an empty file list, which needs no device."""
import os

import numpy as np
import pytest

U = 2.0 ** -24                       # half a unit in the last place of a float32, relative
TINY = 2.0 ** -126                   # the smallest normal float32: covers either denormal mode


def fake(i, off=0):
    """A fake device address, aligned to 4 KiB plus `off`."""
    return (0x7000_0000_0000 + (i << 32)) + off


# ---------------------------------------------------------------- the C-ABI
def test_symbols_exported(native):
    from kf2vecfsw_amd import _native as N
    from kf2vecfsw_amd import build
    for s in ("kf_class_probs", "kf_class_probs_reg_cols", "kf_class_probs_rows"):
        assert hasattr(native, s) and s in N.SIGNATURES, s
    assert native.kf_class_probs_reg_cols() >= 64 and native.kf_class_probs_rows() >= 1
    assert "kf_classprobs.hip" in build.SOURCES_HIP


def max_rows(native):
    """The most rows one call takes: fewer than 2^24 workgroups."""
    return native.kf_class_probs_rows() * ((1 << 24) - 1)


REFUSALS = [
    ("C == 0", dict(C=0), b"C == 0"),
    ("C == 2^31", dict(C=1 << 31), b"2^31 columns"),
    ("C == 2^40", dict(C=1 << 40), b"2^31 columns"),
    ("Q reaches 2^32 threads", dict(Q="over"), b"workgroups"),
    ("Q == 2^40", dict(Q=1 << 40), b"workgroups"),
    ("null logits", dict(x=None), b"null d_logits"),
    ("null out", dict(out=None), b"null d_out"),
    ("null top", dict(top=None), b"null d_top"),
    ("logits off by 2", dict(x=fake(1, 2)), b"misaligned d_logits"),
    ("out off by 1", dict(out=fake(2, 1)), b"misaligned d_out"),
    ("top off by 2", dict(top=fake(3, 2)), b"misaligned d_top"),
    ("misaligned without rows", dict(Q=0, out=fake(2, 2)), b"misaligned d_out"),
]


@pytest.mark.parametrize("what,kw,msg", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_class_probs_refuses_before_any_hip_call(native, what, kw, msg):
    from kf2vecfsw_amd import _native as N
    a = dict(x=fake(1), Q=100, C=16, out=fake(2), top=fake(3))
    a.update(kw)
    if a["Q"] == "over":
        a["Q"] = max_rows(native) + 1
    assert native.kf_class_probs(a["x"], a["Q"], a["C"], a["out"], a["top"], None) == N.KF_EINVAL, what
    assert msg in native.kf_last_error(), native.kf_last_error()


def test_no_rows_is_valid(native):
    from kf2vecfsw_amd import _native as N
    assert native.kf_class_probs(None, 0, 16, None, None, None) == N.KF_OK
    assert native.kf_class_probs(fake(1), 0, 1, fake(2), fake(3), None) == N.KF_OK


# ---------------------------------------------------------------- the host statement
@pytest.mark.parametrize("scale", [1, 10, 40, 100, 1000])
@pytest.mark.parametrize("C", [1, 2, 3, 63, 64, 65, 129, 1000])
def test_class_probs_host_and_torch_within_the_bound(C, scale):
    """The reference's torch.exp(F.log_softmax(x, dim=1)) on the CPU against the
    statement (the float64 softmax of the same float32 logits, rounded once).
    The bound (2|t_j| + C + 8) * 2^-24 * ref_j + 2^-126, t_j = x_j - max x in
    float64, counts the roundings of the reference's form: the two subtractions
    (by m, by log s), each scaled by |t| through exp; log, exp and the sum."""
    import torch
    import torch.nn.functional as F
    from kf2vecfsw_amd import classify as CL
    rng = np.random.default_rng(1000 * C + scale)
    x = (rng.standard_normal((48, C)) * scale).astype(np.float32)
    ref = torch.exp(F.log_softmax(torch.from_numpy(x), dim=1)).numpy()
    out, top = CL.class_probs_host(x)
    assert out.dtype == np.float32 and top.dtype == np.int32 and out.shape == (48, C + 1)
    x64 = x.astype(np.float64)
    t = np.abs(x64 - x64.max(axis=1, keepdims=True))
    r64 = ref.astype(np.float64)
    bound = (2 * t + C + 8) * U * r64 + TINY
    err = np.abs(out[:, 1:].astype(np.float64) - r64)
    used = float((err / bound).max())
    print("C={} scale={}: torch uses {:.3f} of its bound".format(C, scale, used))
    assert used <= 1.0
    assert np.array_equal(top, np.argmax(out[:, 1:], axis=1))
    assert np.array_equal(out[:, 0].view(np.uint32), out[np.arange(48), 1 + top].view(np.uint32))
    assert np.all(np.abs(out[:, 1:].astype(np.float64).sum(axis=1) - 1) <= (C + 8) * U)


def test_class_probs_host_planted_rows():
    from kf2vecfsw_amd import classify as CL
    inf, nan = np.inf, np.nan
    x = np.zeros((8, 5), dtype=np.float32)
    x[1] = [1, 7, 3, 7, 0]                     # two equal maxima: the first
    x[2] = [0, nan, 0, 0, 0]
    x[3] = [0, 0, inf, 0, 0]
    x[4] = -inf
    x[5] = [0, -inf, 0, 0, 300]                # a -inf among finite values; exact 0 and 1
    x[6] = [-inf, -inf, -inf, 2, -inf]
    x[7] = [3, 3, 3, 3, 3]
    out, top = CL.class_probs_host(x)
    assert top.tolist() == [0, 1, 0, 0, 0, 4, 3, 0]
    for r in (2, 3, 4):
        assert np.isnan(out[r]).all()
    assert not np.isnan(out[[0, 1, 5, 6, 7]]).any()
    assert np.all(out[0] == np.float32(1) / np.float32(5)) and np.all(out[7] == out[0])
    assert out[1, 2] == out[1, 4] and out[1, 0] == out[1, 2]
    assert out[5].tolist() == [1.0, 0.0, 0.0, 0.0, 0.0, 1.0]
    assert out[6].tolist() == [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]
    e, t = CL.class_probs_host(np.zeros((0, 3), np.float32))
    assert e.shape == (0, 4) and t.shape == (0,)


# ---------------------------------------------------------------- the CLI's parsers
def test_classify_parser_defaults():
    from kf2vecfsw_amd import main as M
    a = M.build_parser().parse_args(["classify"])
    assert (a.block, a.seed, a.input_dir, a.model, a.o, a.device) == (4000, 28, None, None, None, None)
    assert a.func is M.classify
    a = M.build_parser().parse_args(["classify", "-input_dir", "i", "-model", "m", "-o", "o", "-block", "7", "-seed",
                                     "3", "-device", "cuda:1"])
    assert (a.input_dir, a.model, a.o, a.block, a.seed, a.device) == ("i", "m", "o", 7, 3, "cuda:1")


def test_process_query_data_parser_defaults():
    import multiprocessing as mp
    from kf2vecfsw_amd import main as M
    p = M.build_parser()
    a = p.parse_args(["process_query_data"])
    assert (a.k, a.p, a.pseudocount, a.cl_seed, a.di_seed) == (7, mp.cpu_count(), False, 28, 28)
    assert (a.input_dir, a.output_dir, a.classifier_model, a.distance_model) == (None, None, None, None)
    # the three options the reference's parser lacks, with the values its subcommands default to
    assert (a.raw_cnt, a.block, a.remap, a.device) == (False, 4000, None, None)
    assert a.func is M.process_query_data
    for k in range(3, 11):
        assert p.parse_args(["process_query_data", "-k", str(k)]).k == k
    for k in ("2", "11"):
        with pytest.raises(SystemExit):
            p.parse_args(["process_query_data", "-k", k])
    a = p.parse_args(["process_query_data", "-raw_cnt", "-block", "2", "-remap", "r.tsv", "-pseudocount"])
    assert (a.raw_cnt, a.block, a.remap, a.pseudocount) == (True, 2, "r.tsv", True)
    text = p.format_help()
    assert "classify" in text and "process_query_data" in text


# ---------------------------------------------------------------- the model
def reference_named_module(n_in, hidden, classes):
    """A module with the three attribute names of the reference's classifier, in
    its order, whose forward is the reference's: log_softmax of fc3(relu(fc1(x)))."""
    import torch

    class Named(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.fc1 = torch.nn.Linear(n_in, hidden)
            self.fc3 = torch.nn.Linear(hidden, classes)
            self.relu = torch.nn.ReLU()

        def forward(self, x):
            return torch.nn.functional.log_softmax(self.fc3(self.relu(self.fc1(x))), dim=1)

    return Named()


def test_classifier_net_loads_the_trainers_state_dict(tmp_path):
    import torch
    from kf2vecfsw_amd import classify as CL
    torch.manual_seed(3)
    src = reference_named_module(32, 8, 3)
    torch.save({"model_input_size": 32, "model_hidden_size_fc1": 8, "model_class_count": 3,
                "state_dict": src.state_dict()}, str(tmp_path / "classifier_model.ckpt"))
    net = CL.load_classifier(str(tmp_path), "cpu")
    assert sorted(net.state_dict()) == sorted(src.state_dict()) == ["fc1.bias", "fc1.weight", "fc3.bias", "fc3.weight"]
    assert not net.training and (net.fc1.in_features, net.fc1.out_features, net.fc3.out_features) == (32, 8, 3)
    x = torch.randn(5, 32)
    with torch.no_grad():
        logits, ref = net(x), torch.exp(src.eval()(x))
    assert torch.equal(logits, src.fc3(torch.relu(src.fc1(x))))           # the logits: no softmax in forward
    out, top = CL.class_probs_host(logits.numpy())
    assert np.allclose(out[:, 1:], ref.numpy(), rtol=1e-5, atol=0) and np.array_equal(top, ref.argmax(1).numpy())


# ---------------------------------------------------------------- no input file: no device
def test_no_input_file_gives_the_header_only(tmp_path, capsys):
    import torch
    from kf2vecfsw_amd import classify as CL
    model, out = tmp_path / "model", tmp_path / "out"
    model.mkdir()
    torch.save({"model_input_size": 32, "model_hidden_size_fc1": 8, "model_class_count": 3,
                "state_dict": reference_named_module(32, 8, 3).state_dict()}, str(model / "classifier_model.ckpt"))
    out.mkdir()
    (out / "classes.out").write_bytes(b"stale\n")
    assert CL.classify_func(str(tmp_path / "kf"), [], str(model), 28, str(out)) is None
    assert (out / "classes.out").read_bytes() == b"genome\ttop_class\ttop_p\t0\t1\t2\r\n"
    text = (out / "classification.log").read_text()
    assert capsys.readouterr().err == text
    lines = text.split("\n")
    assert lines[:8] == ["", "==> Input arguments...", "", "Feature directory: {}".format(tmp_path / "kf"),
                         "Model: {}".format(model), "Seed: 28", "", "==> Building model..."]
    assert lines[8:13] == ["", "", "==> Classification Completed!", "", "Time: 00:00:00"] and lines[13:] == [""]
    assert CL.classify_func(str(tmp_path / "kf"), [], str(model), 28, str(out), keep=True) == []
    assert sorted(os.listdir(out)) == ["classes.out", "classification.log"]
