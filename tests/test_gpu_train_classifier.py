"""GPU tests of train_classifier: kf_class_loss against kf_class_probs bit for
bit (the gradient and the hits), against its own rows (the loss), against its
host statement within the header's bound (the rows), at the smallest shapes
where it can go wrong (one row and one column, the edges of a wave's 64 lanes,
of the register tiers and of the register threshold, the one-workgroup path and
the two-launch one with a shape either side of the cut-over); rows that do not
depend on the call; guard values around every output; the running totals; the
status; the autograd Function; and `train_classifier` end to end on the toy
example: files, log, checkpoint, backbone_classes.out byte for byte against the
host statement of the formatter and against the reference's own file, the round
trip through `classify`, and the losses against a restatement of the reference's
loop in torch."""
import contextlib
import csv
import gzip
import io
import json
import os
import re
import shutil

import numpy as np
import pytest

import class_inputs
from conftest import GOLDEN, TOY

pytestmark = pytest.mark.gpu

U = 2.0 ** -24                       # half a unit in the last place of a float32, relative
TINY = 2.0 ** -126                   # the smallest normal float32
GOLD = os.path.join(GOLDEN, "train_classifier")


@pytest.fixture(scope="module")
def dev(native):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu tests need an MI355X")
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------
# the kernel
# ---------------------------------------------------------------------------
# S = kf_class_loss_small_b() rows (the cut-over), R = kf_class_probs_reg_cols() columns (the register threshold)
SHAPES = [(1, 1), (1, 2), (2, 3), (16, 2), (16, 64), (16, 65), (5, 256), (5, 257),
          (3, "R"), (3, "R+1"), ("S-1", 7), ("S", 7), ("S+1", 7), (4001, 16)]


def size(native, v):
    if isinstance(v, int):
        return v
    m = re.fullmatch(r"([SR])([+-]\d+)?", v)
    val = {"S": native.kf_class_loss_small_b(), "R": native.kf_class_probs_reg_cols()}
    return val[m.group(1)] + int(m.group(2) or 0)


_HOST = {}


def host(B, C):
    """The inputs of a shape and the host statement on them, computed once."""
    from kf2vecfsw_amd import train_classifier as TC
    if (B, C) not in _HOST:
        x, true, where = class_inputs.make(B, C)
        loss, grad, nll, hits = TC.class_loss_host(x, true)
        for a in (grad, nll):
            a.setflags(write=False)
        _HOST[(B, C)] = (x, true, where, loss, grad, nll, hits)
    return _HOST[(B, C)]


def run_kernel(dev, x, true, grad=True, totals=None):
    """(loss float64 [], grad or None, row_loss, hits, status) on the host."""
    import torch
    from kf2vecfsw_amd import train_classifier as TC
    loss, g, rows, hits, status = TC.class_loss(torch.from_numpy(np.ascontiguousarray(x)).to(dev),
                                                torch.from_numpy(np.ascontiguousarray(true)).to(dev), grad=grad,
                                                totals=totals)
    return loss.cpu().numpy(), None if g is None else g.cpu().numpy(), rows.cpu().numpy(), int(hits.cpu()[0]), \
        int(status.cpu()[0])


def run_probs(dev, x):
    import torch
    from kf2vecfsw_amd import classify as CL
    out, top = CL.class_probs(torch.from_numpy(np.ascontiguousarray(x)).to(dev))
    return out.cpu().numpy(), top.cpu().numpy()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def same(a, b):
    """Equal bit for bit, any NaN taken as equal to any NaN."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def grad_from_probs(out, true):
    """(P - onehot) * float32(1 / B) in float32, from kf_class_probs' own output."""
    b, c = out.shape[0], out.shape[1] - 1
    onehot = np.zeros((b, c), dtype=np.float32)
    ok = (true >= 0) & (true < c)
    onehot[np.flatnonzero(ok), true[ok]] = 1.0
    with np.errstate(all="ignore"):
        return ((out[:, 1:] - onehot) * (np.float32(1.0) / np.float32(b))).astype(np.float32)


def row_bound(x, true):
    """The header's bound on |nll_i - nll| per row, from the float32 logits in float64:
    (T + C + 8 + 4 |log s| + |t_c| + |nll|) * 2^-24 + C * 2^-126 with T = sum_j p_j |t_j|."""
    x64 = x.astype(np.float64)
    b, c = x64.shape
    with np.errstate(all="ignore"):
        t = x64 - x64.max(axis=1, keepdims=True)
        e = np.exp(t)
        s = e.sum(axis=1)
        p = e / s[:, None]
        T = np.where(p > 0, p * np.abs(t), 0.0).sum(axis=1)
        tc = t[np.arange(b), true]
        nll = np.log(s) - tc
        return (T + c + 8 + 4 * np.abs(np.log(s)) + np.abs(tc) + np.abs(nll)) * U + c * TINY


@pytest.mark.parametrize("B,C", SHAPES, ids=["{}x{}".format(*s) for s in SHAPES])
def test_kernel_against_class_probs_its_rows_and_the_host_statement(dev, native, B, C):
    from kf2vecfsw_amd import train_classifier as TC
    B, C = size(native, B), size(native, C)
    x, true, where, h_loss, h_grad, h_nll, h_hits = host(B, C)
    loss, grad, rows, hits, status = run_kernel(dev, x, true)
    assert status == 0 and loss.dtype == np.float64 and grad.dtype == np.float32 and grad.shape == (B, C)
    assert rows.dtype == np.float32 and rows.shape == (B,)
    # parity with kf_class_probs, bit for bit
    out, top = run_probs(dev, x)
    assert not np.isnan(out).any()
    assert same(grad, grad_from_probs(out, true)), "the gradient is not (P - onehot) / B of kf_class_probs' P"
    assert hits == int(np.count_nonzero(top == true))
    # the loss is its rows' sum, bit for bit
    assert bits(loss) == bits(TC.loss_of_rows(rows))
    loss2, grad2, rows2, hits2, status2 = run_kernel(dev, x, true, grad=False)
    assert grad2 is None and status2 == 0 and hits2 == hits and bits(loss2) == bits(loss) and same(rows2, rows)
    # and with the planted -inf taken as -30, so that the sum is finite and its order shows
    xf = np.where(np.isinf(x), np.float32(-30.0), x)
    loss3, _, rows3, _, _ = run_kernel(dev, xf, true, grad=False)
    assert np.isfinite(loss3) and bits(loss3) == bits(TC.loss_of_rows(rows3))
    # the rows against the host statement, within the header's bound
    inf = np.isinf(h_nll)
    assert np.array_equal(np.isinf(rows), inf) and np.all(rows[inf] > 0) and not np.isnan(rows).any()
    assert int(np.count_nonzero(inf)) == (1 if "-inf at the true class" in where else 0)
    err = np.abs(rows[~inf].astype(np.float64) - h_nll[~inf])
    used = float((err / row_bound(x, true)[~inf]).max()) if err.size else 0.0
    print("B={} C={}: loss {!r} (host {!r}), hits {} (host {}), the rows use {:.3f} of their bound".format(
        B, C, float(loss), float(h_loss), hits, h_hits, used))
    assert used <= 1.0
    if C == 1:
        assert float(loss) == 0.0 and not grad.any() and not rows.any() and hits == B
    if "spread 120" in where:
        r = where["spread 120"]
        assert out[r, 1 + true[r]] == 0.0 and rows[r] > 119.0
    if "two maxima" in where:
        r = where["two maxima"]
        assert top[r] < true[r] and out[r, 1 + top[r]] == out[r, 1 + true[r]]        # the first maximum: no hit


def test_rows_do_not_depend_on_the_call(dev, native):
    """A row's row_loss bits, and grad * B where B is a power of two (the scaling is then
    exact), are the same in a batch of 1, of S, of S + 1 and of 2 S, at any position."""
    S, R = native.kf_class_loss_small_b(), native.kf_class_probs_reg_cols()
    assert S & (S - 1) == 0
    for C in (7, 65, 257, R + 1):
        x, true, where = class_inputs.make(2 * S, C, seed=3)
        assert len(where) == 4
        x[7, C // 2] = np.nan                                            # a refused row among them
        rev = np.arange(2 * S)[::-1].copy()
        _, g_all, r_all, _, _ = run_kernel(dev, x[rev], true[rev])       # 2 S rows, in reverse: the two-launch path
        g_all, r_all = g_all[rev], r_all[rev]
        _, g_s, r_s, _, _ = run_kernel(dev, x[:S], true[:S])             # S rows: one workgroup
        _, _, r_s1, _, _ = run_kernel(dev, x[:S + 1], true[:S + 1])      # S + 1 rows: two launches
        assert same(r_s, r_all[:S]) and same(r_s1, r_all[:S + 1]), C
        assert same(g_s * np.float32(S), g_all[:S] * np.float32(2 * S)), C
        for r in sorted(set(where.values()) | {0, 7, S - 1, S}):
            _, g1, r1, _, _ = run_kernel(dev, x[r: r + 1], true[r: r + 1])
            assert same(r1, r_all[r: r + 1]) and same(g1, g_all[r: r + 1] * np.float32(2 * S)), (C, r)
        assert np.isnan(r_all[7]) and np.isnan(g_all[7]).all() and np.count_nonzero(np.isnan(r_all)) == 1


def test_nothing_is_written_past_the_outputs_and_absent_outputs_stay(dev, native):
    """The raw call with guard values around the loss, the hits, the status, the gradient,
    the rows and the totals, with and without d_grad, d_row_loss and d_totals, on both paths."""
    import torch
    from kf2vecfsw_amd import _native as N
    from kf2vecfsw_amd import counter as CN
    from kf2vecfsw_amd import train_classifier as TC
    S = native.kf_class_loss_small_b()
    pad = 64
    for B, C in ((5, 7), (S + 3, 9), (3, native.kf_class_probs_reg_cols() + 1)):
        x, true, _, _, _, _, _ = host(B, C)
        ref_loss, ref_grad, ref_rows, ref_hits, _ = run_kernel(dev, x, true)
        d_x, d_t = torch.from_numpy(x).to(dev), torch.from_numpy(true).to(dev)
        need = TC.class_loss_scratch_bytes(B)
        scratch = torch.empty(need // 8 + 1, dtype=torch.int64, device=dev)
        for want_g, want_r, want_t in ((True, True, True), (False, False, False), (True, False, True),
                                       (False, True, False)):
            out = torch.full((3,), -7.5, dtype=torch.float64, device=dev)
            cnt = torch.full((5,), -77, dtype=torch.int32, device=dev)
            g = torch.full((B * C + 2 * pad,), -12345.5, dtype=torch.float32, device=dev)
            rl = torch.full((B + 2 * pad,), -54321.5, dtype=torch.float32, device=dev)
            tot = torch.full((5,), 2.0, dtype=torch.float64, device=dev)
            N.check(native.kf_class_loss(d_x.data_ptr(), B, C, d_t.data_ptr(), out[1:].data_ptr(),
                                         g[pad:].data_ptr() if want_g else None,
                                         rl[pad:].data_ptr() if want_r else None, cnt[1:].data_ptr(),
                                         cnt[3:].data_ptr(), tot[1:].data_ptr() if want_t else None,
                                         scratch.data_ptr() if need else None, need, CN._stream_ptr(dev)),
                    "kf_class_loss")
            what = (B, C, want_g, want_r, want_t)
            o, c, gh, rh, th = out.cpu().numpy(), cnt.cpu().numpy(), g.cpu().numpy(), rl.cpu().numpy(), tot.cpu().numpy()
            assert o[0] == -7.5 and o[2] == -7.5 and bits(o[1:2])[0] == bits(ref_loss), what
            assert c.tolist() == [-77, ref_hits, -77, 0, -77], what
            assert np.all(gh[:pad] == -12345.5) and np.all(gh[pad + B * C:] == -12345.5), what
            assert np.all(rh[:pad] == -54321.5) and np.all(rh[pad + B:] == -54321.5), what
            assert same(gh[pad: pad + B * C], ref_grad.reshape(-1)) if want_g else np.all(gh == -12345.5), what
            assert same(rh[pad: pad + B], ref_rows) if want_r else np.all(rh == -54321.5), what
            if want_t:
                assert th.tolist() == [2.0, 2.0 + float(ref_loss) * B, 2.0 + ref_hits, 2.0, 2.0], what
            else:
                assert np.all(th == 2.0), what


def test_totals_of_three_calls_on_one_stream(dev, native):
    import torch
    S = native.kf_class_loss_small_b()
    totals = torch.zeros(3, dtype=torch.float64, device=dev)
    want = np.zeros(3, dtype=np.float64)
    with np.errstate(all="ignore"):
        for B, C in ((5, 7), (S, 7), (S + 3, 9)):
            x, true, _, _, _, _, _ = host(B, C)
            x = np.where(np.isinf(x), np.float32(-30.0), x)                  # a finite loss, so that the sums say something
            loss, _, _, hits, status = run_kernel(dev, x, true, totals=totals)
            assert np.isfinite(loss) and status == 0
            want[0] = want[0] + np.float64(loss) * np.float64(B)
            want[1] = want[1] + hits
            want[2] = want[2] + status
        got = totals.cpu().numpy()
        assert np.array_equal(bits(got), bits(want)) and want[1] > 0
        # a class outside the model's: the third total counts it, the first is NaN from then on
        x, true, _, _, _, _, _ = host(5, 7)
        bad = true.copy()
        bad[2] = 7
        _, _, _, hits, status = run_kernel(dev, x, bad, grad=False, totals=totals)
        got = totals.cpu().numpy()
        assert status == 1 and np.isnan(got[0]) and got[1] == want[1] + hits and got[2] == 1.0


def test_a_class_outside_the_model_sets_the_status_and_a_nan_row_does_not(dev, native):
    S = native.kf_class_loss_small_b()
    for B, C in ((5, 7), (S + 3, 9)):
        x, true, _, _, _, _, _ = host(B, C)
        _, ref_grad, ref_rows, _, _ = run_kernel(dev, x, true)
        r = B // 2
        for bad in (C, -1, 1 << 40):
            cls = true.copy()
            cls[r] = bad
            for want in (True, False):
                loss, grad, rows, hits, status = run_kernel(dev, x, cls, grad=want)
                assert status == 1 and np.isnan(loss) and np.isnan(rows[r]) and hits <= B - 1, (B, bad, want)
                assert same(np.delete(rows, r), np.delete(ref_rows, r)), (B, bad, want)
                if want:
                    assert np.isnan(grad[r]).all() and same(np.delete(grad, r, 0), np.delete(ref_grad, r, 0)), (B, bad)
        for poison in (np.nan, np.inf):
            xn = x.copy()
            xn[r, C - 1] = poison
            loss, grad, rows, hits, status = run_kernel(dev, xn, true)
            assert status == 0 and np.isnan(loss) and np.isnan(rows[r]) and np.isnan(grad[r]).all(), (B, poison)
            assert same(np.delete(rows, r), np.delete(ref_rows, r)) and same(np.delete(grad, r, 0), np.delete(ref_grad, r, 0))
        xn = x.copy()
        xn[r] = -np.inf
        loss, grad, rows, _, status = run_kernel(dev, xn, true)
        assert status == 0 and np.isnan(loss) and np.isnan(rows[r]) and np.isnan(grad[r]).all()


def test_autograd_function(dev, native):
    import torch
    from kf2vecfsw_amd import train_classifier as TC
    S = native.kf_class_loss_small_b()
    for B, C in ((16, 65), (S + 1, 7)):
        x, true, _, _, _, _, _ = host(B, C)
        ref_loss, ref_grad, _, ref_hits, _ = run_kernel(dev, x, true)
        d_t = torch.from_numpy(true).to(dev)
        got = []
        for factor in (1.0, 1.0, 3.0):
            d_x = torch.from_numpy(x).to(dev).requires_grad_(True)
            totals = torch.zeros(3, dtype=torch.float64, device=dev)
            loss, hits, status = TC.class_loss_fn(d_x, d_t, totals)
            assert loss.dtype == torch.float64 and loss.dim() == 0 and not hits.requires_grad and not status.requires_grad
            assert bits(loss.detach().cpu().numpy()) == bits(ref_loss) and int(hits[0]) == ref_hits and int(status[0]) == 0
            assert float(totals[1]) == ref_hits
            (loss if factor == 1.0 else factor * loss).backward()
            got.append(d_x.grad.cpu().numpy())
        assert same(got[0], ref_grad) and same(got[1], got[0])                          # upstream 1: the kernel's bits
        with np.errstate(all="ignore"):
            assert same(got[2], ref_grad * np.float32(3.0))
    # through a model: the parameters receive a gradient
    torch.manual_seed(0)
    lin = torch.nn.Linear(6, 7).to(dev)
    x, true, _, _, _, _, _ = host(5, 7)
    loss, _, _ = TC.class_loss_fn(lin(torch.from_numpy(x[:, :6].clip(-8, 8)).to(dev)), torch.from_numpy(true).to(dev))
    loss.backward()
    assert lin.weight.grad is not None and bool(torch.isfinite(lin.weight.grad).all()) and bool(lin.weight.grad.any())


# ---------------------------------------------------------------------------
# train_classifier on the toy example
# ---------------------------------------------------------------------------
EPOCHS, HIDDEN, BATCH = 5, 64, 16
GENOMES = {"G000830275": 0, "G000402355": 0, "G001940645": 1, "G001871415": 1, "G000830295": 1}


def toy_inputs(root):
    """The five train_tree_kf files and the subtrees file."""
    kf = root / "train_tree_kf"
    kf.mkdir()
    for f in sorted(os.listdir(os.path.join(TOY, "train_tree_kf"))):
        (kf / f[:-3]).write_bytes(gzip.open(os.path.join(TOY, "train_tree_kf", f)).read())
    shutil.copy(os.path.join(TOY, "train_tree.subtrees"), str(root / "train_tree.subtrees"))
    files = sorted(os.path.join(str(kf), f) for f in os.listdir(str(kf)))
    assert len(files) == 5
    return str(kf), files, str(root / "train_tree.subtrees")


def train(dev, world, out, files=None, subtrees=None, mask=False, batch=BATCH, epochs=EPOCHS):
    """train_classifier_model_func as the CLI calls it; (kept, stdout)."""
    from kf2vecfsw_amd import train_classifier as TC
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        kept = TC.train_classifier_model_func(world["kf"], files or world["files"], subtrees or world["subtrees"], epochs,
                                              HIDDEN, batch, 1e-5, 3e-6, 2000, 28, mask, out, device=dev, keep=True)
    return kept, buf.getvalue()


@pytest.fixture(scope="module")
def world(dev, tmp_path_factory):
    root = tmp_path_factory.mktemp("train_classifier_toy")
    kf, files, subtrees = toy_inputs(root)
    return dict(root=root, kf=kf, files=files, subtrees=subtrees)


@pytest.fixture(scope="module")
def run(dev, world):
    """-hidden_sz 64 -e 5 -batch_sz 16 through the function, with the tensors kept."""
    out = str(world["root"] / "models")
    kept, said = train(dev, world, out)
    return dict(out=out, kept=kept, stdout=said)


def read_rows(path, eol):
    data = open(path, "rb").read()
    assert data.endswith(eol) and (eol == b"\r\n" or b"\r" not in data)
    return list(csv.reader(io.StringIO(data.decode(), newline=""), delimiter="\t"))


def test_files_log_and_checkpoint(dev, world, run):
    from kf2vecfsw_amd import classify as CL
    from kf2vecfsw_amd import tables as T
    from kf2vecfsw_amd import train_classifier as TC
    out, k = run["out"], run["kept"]
    logs = [f for f in os.listdir(out) if re.fullmatch(r"train_classifier_\d{8}_\d{6}\.log", f)]
    assert len(logs) == 1 and sorted(os.listdir(out)) == sorted(logs + ["classifier_model.ckpt", "backbone_classes.out"])
    model = CL.load_classifier(out, dev)
    assert (model.fc1.in_features, model.fc1.out_features, model.fc3.out_features) == (8192, HIDDEN, 2)
    rows = read_rows(os.path.join(out, "backbone_classes.out"), b"\n")
    gold = read_rows(os.path.join(GOLD, "backbone_classes.out"), b"\n")
    assert rows[0] == gold[0] == ["genome", "true_class", "top_class", "top_p", "0", "1"]
    names = [os.path.basename(f)[:-3] for f in world["files"]]
    assert [r[0] for r in rows[1:]] == names == k["names"] and sorted(names) == sorted(r[0] for r in gold[1:])
    assert [r[1] for r in rows[1:]] == [str(GENOMES[nm]) for nm in names]                # from the .subtrees file
    assert all(len(r) == 6 and r[2] in ("0.0", "1.0") for r in rows[1:])
    # the file's bytes: the host statement of the formatter on the kept tensors
    probs, top = k["probabilities"].numpy(), k["top"]
    assert probs.dtype == np.float32 and probs.shape == (5, 3) and k["logits"].shape == (5, 2)
    text, _ = T.format_float_rows_host(probs, TC.backbone_prefixes(names, k["classes"], top), T.KF_FLOAT_WIDENED, eol="\n")
    assert open(os.path.join(out, "backbone_classes.out"), "rb").read() == \
        T.header_line(TC.backbone_header(2), eol="\n") + text
    assert [r[2] for r in rows[1:]] == ["{}.0".format(int(t)) for t in top]
    # the log: the file is what went to stdout; a loss and a learning rate per epoch, one best epoch
    text = open(os.path.join(out, logs[0])).read()
    assert text == run["stdout"]
    for line in ("Feature directory: {}".format(world["kf"]), "Clades information: {}".format(world["subtrees"]),
                 "GPU Support: Yes", "Hidden Size fc1: 64", "Total Epochs: 5", "Batch Size: 16", "Learning Rate: 1e-05",
                 "Masking: False", "Dimensions of feature matrix rows: 5, cols: 8192", "Number of Train Samples: 5",
                 "Number of Classes: 2", "Dimensions of class output rows:5 cols:6", "\n==> Training Completed!\n"):
        assert line + "\n" in text, line
    found = re.findall(r"Epoch \[(\d)/5\], Step \[1/1\], Train loss: (\d+\.\d{20}), (\d\.\d{20}), Time: ", text)
    assert [int(e) for e, _, _ in found] == [1, 2, 3, 4, 5]
    assert [float(v) for _, v, _ in found] == pytest.approx(k["losses"], abs=1e-20)
    assert [float(a) for _, _, a in found] == pytest.approx(k["accuracies"], abs=1e-20)
    assert all(a in (0.0, 0.2, 0.4, 0.6, 0.8, 1.0) for a in k["accuracies"])
    assert [int(e) for e in re.findall(r"Epoch (\d)\t               LR:\d\.\d{20}\n", text)] == [1, 2, 3, 4, 5]
    best = re.findall(r"Best Epoch \[(\d)/5\], Lowest loss: (\d+\.\d{20}), Highest accuracy: (\d\.\d{20})\n", text)
    assert len(best) == 1 and int(best[0][0]) == k["best_epoch"] + 1 == 1 + k["losses"].index(min(k["losses"]))
    print("train losses per epoch:", " ".join("{:.6g}".format(v) for v in k["losses"]), "accuracies:", k["accuracies"])
    assert all(np.isfinite(v) and v > 0 for v in k["losses"])


def test_format_against_the_references_own_file(dev, tmp_path):
    """The numbers of the reference's backbone_classes.out (each a float32 printed widened)
    with its names and classes through the trainer's writer call: the file's bytes."""
    import torch
    from kf2vecfsw_amd import tables as T
    from kf2vecfsw_amd import train_classifier as TC
    gold_bytes = open(os.path.join(GOLD, "backbone_classes.out"), "rb").read()
    rows = read_rows(os.path.join(GOLD, "backbone_classes.out"), b"\n")
    names, true, top = [r[0] for r in rows[1:]], [int(r[1]) for r in rows[1:]], [int(float(r[2])) for r in rows[1:]]
    values = np.array([[float(v) for v in r[3:]] for r in rows[1:]], dtype=np.float64)
    assert np.array_equal(values.astype(np.float32).astype(np.float64), values) and values.shape == (5, 3)
    path = str(tmp_path / "backbone_classes.out")
    with T.FloatTableWriter(dev, 1) as writer:
        writer.write(path, TC.backbone_prefixes(names, true, top), torch.from_numpy(values.astype(np.float32)).to(dev),
                     header=TC.backbone_header(2), mode=T.KF_FLOAT_WIDENED, eol="\n", quoted=True)
    assert open(path, "rb").read() == gold_bytes


def test_round_trip_through_classify(dev, world, run):
    """classify on the same files with the written checkpoint, in one block: the same matrix
    shape as the trainer's last pass, and kf_class_probs does not depend on the batch."""
    from kf2vecfsw_amd import classify as CL
    out = str(world["root"] / "classified")
    err = io.StringIO()
    with contextlib.redirect_stderr(err):
        CL.classify_func(world["kf"], world["files"], run["out"], 28, out, max(4000, len(world["files"])), dev)
    mine = {r[0]: r for r in read_rows(os.path.join(run["out"], "backbone_classes.out"), b"\n")[1:]}
    theirs = read_rows(os.path.join(out, "classes.out"), b"\r\n")
    assert theirs[0] == ["genome", "top_class", "top_p", "0", "1"] and len(theirs) == 6
    for r in theirs[1:]:
        assert "{}.0".format(r[1]) == mine[r[0]][2] and r[2:] == mine[r[0]][3:], r[0]


def test_cli_writes_the_same_files(dev, world, run):
    from kf2vecfsw_amd import main as M
    out = str(world["root"] / "models_cli")
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        M.main(["train_classifier", "-input_dir", world["kf"], "-subtrees", world["subtrees"], "-e", str(EPOCHS),
                "-hidden_sz", str(HIDDEN), "-batch_sz", str(BATCH), "-o", out, "-device", str(dev)])
    logs = [f for f in os.listdir(out) if f.endswith(".log")]
    assert len(logs) == 1 and sorted(os.listdir(out)) == sorted(logs + ["classifier_model.ckpt", "backbone_classes.out"])
    assert buf.getvalue() == open(os.path.join(out, logs[0])).read()                    # nothing but the log's lines
    a = {r[0]: r for r in read_rows(os.path.join(out, "backbone_classes.out"), b"\n")}
    b = {r[0]: r for r in read_rows(os.path.join(run["out"], "backbone_classes.out"), b"\n")}
    assert sorted(a) == sorted(b) and all(a[nm][:2] == b[nm][:2] and len(a[nm]) == 6 for nm in a)
    # the command takes the genomes in the glob's order, which is the file system's: in the function's order the
    # files hold the same bits
    import glob
    if glob.glob(os.path.join(world["kf"], "*.kf")) == world["files"]:
        assert a == b


def test_refusals_write_no_checkpoint(dev, world, tmp_path):
    from kf2vecfsw_amd import main as M
    from kf2vecfsw_amd import train_classifier as TC
    out = tmp_path / "o1"
    with pytest.raises(SystemExit) as e:
        M.main(["train_classifier", "-input_dir", world["kf"], "-subtrees", world["subtrees"], "-e", "1", "-o", str(out),
                "-mask", "-device", str(dev)])
    assert e.value.code == TC.MASK_MESSAGE and not (out / "classifier_model.ckpt").exists()
    short = tmp_path / "short.subtrees"
    short.write_text("".join(ln for ln in open(world["subtrees"]) if "G001871415" not in ln))
    with pytest.raises(ValueError) as e:
        M.main(["train_classifier", "-input_dir", world["kf"], "-subtrees", str(short), "-e", "1", "-o", str(out),
                "-device", str(dev)])
    assert "G001871415" in str(e.value) and str(short) in str(e.value) and not (out / "classifier_model.ckpt").exists()
    # a .kf file of two rows, and a row of NaN features: refused with the file's name
    kf2 = tmp_path / "kf2"
    shutil.copytree(world["kf"], str(kf2))
    one = (kf2 / "G001871415.kf").read_bytes()
    (kf2 / "G001871415.kf").write_bytes(one + one)
    w2 = dict(world, kf=str(kf2), files=[os.path.join(str(kf2), os.path.basename(f)) for f in world["files"]])
    with pytest.raises(ValueError) as e:
        train(dev, w2, str(tmp_path / "o2"), epochs=1)
    assert str(kf2 / "G001871415.kf") in str(e.value) and "2 rows" in str(e.value)
    assert not (tmp_path / "o2" / "classifier_model.ckpt").exists()
    (kf2 / "G001871415.kf").write_bytes(b"G001871415," + b",".join([b"nan"] * 8192) + b"\n")    # an empty genome's file
    with pytest.raises(ValueError) as e:
        train(dev, w2, str(tmp_path / "o3"), epochs=1)
    assert str(kf2 / "G001871415.kf") in str(e.value) and "NaN" in str(e.value)
    assert not (tmp_path / "o3" / "classifier_model.ckpt").exists()


# ---------------------------------------------------------------------------
# against torch
# ---------------------------------------------------------------------------
def restate(world, device, dtype, epochs):
    """kf2vec/train_classifier_model.py:303-460 with its per-step .item() and host accuracy,
    from the trainer's initial parameters (torch.manual_seed(28), the model made on the
    host) and its batches (the device randperm of a generator seeded with 28): the losses
    and accuracies per epoch, and per epoch the smallest gap between a row's two largest
    probabilities."""
    import torch
    from kf2vecfsw_amd import classify as CL
    from kf2vecfsw_amd import features as F
    from kf2vecfsw_amd import train as TR
    names = [os.path.basename(f)[:-3] for f in world["files"]]
    gpu = torch.device("cuda:0")
    x_all = F.features_from_kf(world["kf"], 7, gpu, samples=names, scaler=1e4, dtype=torch.float32).values
    x_all = x_all.to(device=device, dtype=dtype)
    true_all = torch.tensor([GENOMES[nm] for nm in names], dtype=torch.int64, device=device)
    torch.manual_seed(28)
    model = CL.ClassifierNet(8192, HIDDEN, 2).to(device=device, dtype=dtype)
    criterion = torch.nn.NLLLoss()
    optimizer = torch.optim.Adam(model.parameters(), lr=1e-5)
    gen = torch.Generator(device=gpu)
    gen.manual_seed(28)
    n = len(names)
    losses, accs, gaps = [], [], []
    for epoch in range(epochs):
        model.train()
        rows = torch.randperm(n, generator=gen, device=gpu).to(device)
        images, true_class = x_all.index_select(0, rows), true_all.index_select(0, rows)
        model_class = torch.nn.functional.log_softmax(model(images), dim=1)
        loss = criterion(model_class, true_class)
        losses.append(loss.item())
        optimizer.zero_grad()
        loss.backward()
        optimizer.step()
        ps = torch.exp(model_class.detach())
        _, top_class = ps.topk(1, dim=1)
        accs.append(float((top_class[:, 0].cpu() == true_class.cpu()).double().mean()))
        srt = ps.sort(dim=1).values
        gaps.append(float((srt[:, -1] - srt[:, -2]).min()))
        lr = TR.lr_after_epoch(epoch, 1e-5, 3e-6, 2000)
        if lr is not None:
            for group in optimizer.param_groups:
                group["lr"] = lr
    return losses, accs, gaps


def test_losses_against_a_restatement_of_the_references_loop(dev, world, run):
    """-batch_sz 16 holds the five genomes, so a step is the whole set.  d is the reference's
    own spread: its loop in float32 on the device against the same loop in float64 on the
    CPU, the largest difference of an epoch's loss.  The kernel path must stay within 4 d of
    the float64 run (the margin covers the differing summation order of the matmul's
    backward), and give the same accuracy wherever the float64 run's two largest
    probabilities of every row differ by more than d.
    Measured on an MI355X (profiles/r23/train_classifier_parity.json, written by this test
    where KF_PARITY_JSON names a file): d = 4.98e-07 at losses of 0.73 down to 0.55, the
    kernel path 4.21e-07 from the float64 run, 0.21 of 4 d; the three accuracies agree in
    all five epochs (0.6), the smallest gap between a row's two largest probabilities being
    0.022.  The figures are printed on every run."""
    import torch
    k = run["kept"]
    l32, a32, _ = restate(world, dev, torch.float32, EPOCHS)
    l64, a64, gaps = restate(world, torch.device("cpu"), torch.float64, EPOCHS)
    d = max(abs(a - b) for a, b in zip(l32, l64))
    mine = max(abs(a - b) for a, b in zip(k["losses"], l64))
    print("losses: kernel path {}, float32 loop {}, float64 loop {}".format(k["losses"], l32, l64))
    print("d = {!r}; the kernel path differs from the float64 run by {!r}: {:.3f} of 4 d".format(
        d, mine, mine / (4 * d) if d else float("inf")))
    print("accuracies: kernel path {}, float32 loop {}, float64 loop {}; smallest gaps {}".format(
        k["accuracies"], a32, a64, gaps))
    path = os.environ.get("KF_PARITY_JSON")
    if path:
        with open(path, "w") as f:
            json.dump({"epochs": EPOCHS, "hidden": HIDDEN, "batch": BATCH, "genomes": 5, "d": d, "kernel_path": mine,
                       "losses_kernel_path": k["losses"], "losses_float32": l32, "losses_float64": l64,
                       "accuracies_kernel_path": k["accuracies"], "accuracies_float64": a64, "smallest_gaps": gaps},
                      f, indent=1)
            f.write("\n")
    assert mine <= 4 * d
    for e in range(EPOCHS):
        if gaps[e] > d:
            assert k["accuracies"][e] == a64[e], e
