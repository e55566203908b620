"""GPU tests of classify: kf_class_probs against its host statement at the
smallest shapes where it can go wrong (one column, the edges of a wave's 64
lanes, of the 1-, 4- and 16-register variants and of the register threshold;
ties, subnormal and exact probabilities, non-finite rows; row independence;
nothing written past the outputs), `classify_func` and the `classify`
subcommand on a synthetic library made here against a restatement of
kf2vec/classify.py:83-124 on the CPU (pandas, the model on the CPU, np.hstack
with the object column, csv.writer), and `process_query_data` against the three
subcommands run one after another."""
import contextlib
import csv
import glob
import io
import os
import re
import shutil

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -24                       # half a unit in the last place of a float32, relative
TINY = 2.0 ** -126                   # the smallest normal float32: covers the result of either denormal mode
K = 3
HIDDEN, CLASSES = 8, 3
BLOCK = 2


@pytest.fixture(scope="module")
def dev(native):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu tests need an MI355X")
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------
# the kernel
# ---------------------------------------------------------------------------
# the column counts: the edges of a wave's 64 lanes and of the 1-, 4- and 16-register variants, and the register
# threshold T = kf_class_probs_reg_cols() with one either side
COLUMNS = [1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000, "T-1", "T", "T+1"]


def planted(C, rng):
    """Rows whose outcome is known, for C columns: (logits float32 [n, C], {what: row})."""
    rows, where = [], {}

    def add(what, v):
        where[what] = len(rows)
        rows.append(np.asarray(v, dtype=np.float32))

    base = rng.standard_normal(C).astype(np.float32)
    add("equal", np.full(C, 3.25))
    # two equal maxima: 3 and 67 (one lane's first and second column), 3 and 40 (the wave's two halves), 5 and 6
    # (neighbours), the first and the last column
    for a, b in ((3, 67), (3, 40), (5, 6), (0, C - 1), (64, 130), (C - 2, C - 1)):
        if 0 <= a < b < C:
            v = base.copy()
            v[a] = v[b] = 9.0
            add("tie {} {}".format(a, b), v)
    for d in (90.0, 100.0, 200.0):    # subnormal, then (nearly) zero, then exactly 0 and 1
        v = base.copy()
        v[C // 2] = np.float32(d) + np.abs(base).max()
        add("peak {}".format(int(d)), v)
    v = base.copy()
    v[C // 3] = np.nan
    add("nan", v)
    v = base.copy()
    v[C - 1] = np.inf
    add("inf", v)
    add("all -inf", np.full(C, -np.inf))
    v = base.copy()
    v[0] = -np.inf
    add("-inf among finite", v if C > 1 else np.full(C, 1.0))
    return np.stack(rows), where


def run_kernel(dev, x):
    import torch
    from kf2vecfsw_amd import classify as CL
    out, top = CL.class_probs(torch.from_numpy(np.ascontiguousarray(x)).to(dev))
    return out.cpu().numpy(), top.cpu().numpy()


def check_against_host(x, out, top, what):
    """The properties every call must have, and the bound against class_probs_host."""
    from kf2vecfsw_amd import classify as CL
    q, c = x.shape
    assert out.shape == (q, c + 1) and out.dtype == np.float32 and top.shape == (q,) and top.dtype == np.int32, what
    ref, rtop = CL.class_probs_host(x)
    rows = np.arange(q)
    assert np.array_equal(out[:, 0].view(np.uint32), out[rows, 1 + top].view(np.uint32)), what
    assert np.array_equal(top, np.argmax(out[:, 1:], axis=1)), what           # argmax: the first index
    bad = np.isnan(ref[:, 0])
    assert np.array_equal(np.isnan(out), np.repeat(bad[:, None], c + 1, axis=1)), what   # the NaN rule, exactly
    assert np.all(top[bad] == 0), what
    if c == 1:
        assert np.all(out[~bad] == np.float32(1.0)), what
    x64 = x[~bad].astype(np.float64)
    t = np.abs(x64 - x64.max(axis=1, keepdims=True))
    t = np.where(np.isinf(t), 0.0, t)                                         # a -inf logit: p = 0 on both sides
    r64 = ref[~bad, 1:].astype(np.float64)
    bound = (t + c + 8) * U * r64 + TINY
    err = np.abs(out[~bad, 1:].astype(np.float64) - r64)
    used = float((err / bound).max()) if err.size else 0.0
    assert used <= 1.0, "{}: {:.3f} of the bound".format(what, used)
    return used


@pytest.mark.parametrize("C", COLUMNS)
def test_kernel_against_the_host_statement(dev, native, C):
    """Q in (1, 2, 5, 257) x logit scales 1, 40 and 1000, and the planted rows,
    for one column count.  The bound, relative (|t_j| + C + 8) * 2^-24 plus
    2^-126: the subtraction, whose |t| * 2^-24 passes through exp; expf, at most
    2 units; C - 1 additions of positives; one division."""
    if isinstance(C, str):
        C = native.kf_class_probs_reg_cols() + {"T-1": -1, "T": 0, "T+1": 1}[C]
    rng = np.random.default_rng(77 + C)
    worst = 0.0
    for Q in (1, 2, 5, 257):
        for scale in (1, 40, 1000):
            x = (rng.standard_normal((Q, C)) * scale).astype(np.float32)
            worst = max(worst, check_against_host(x, *run_kernel(dev, x), "Q={} C={} scale={}".format(Q, C, scale)))
    x, where = planted(C, rng)
    out, top = run_kernel(dev, x)
    worst = max(worst, check_against_host(x, out, top, "planted C={}".format(C)))
    print("C={}: the kernel uses {:.3f} of its bound".format(C, worst))
    r = where["equal"]
    assert np.all(out[r].view(np.uint32) == (np.float32(1) / np.float32(C)).view(np.uint32)) and top[r] == 0
    for what, r in where.items():
        if what.startswith("tie"):
            a, b = (int(s) for s in what.split()[1:])
            assert top[r] == a and out[r, 1 + a].view(np.uint32) == out[r, 1 + b].view(np.uint32), what
    if C > 1:
        r, j = where["peak 200"], C // 2
        assert top[r] == j and out[r, 1 + j] == 1.0 and out[r, 0] == 1.0
        assert np.all(np.delete(out[r, 1:], j) == 0.0)
        r = where["peak 90"]
        rest = np.delete(out[r, 1:], j)
        assert top[r] == j and np.all(rest < TINY) and np.all(rest >= 0)   # subnormal or, flushed, zero
        r = where["-inf among finite"]
        assert out[r, 1] == 0.0 and not np.isnan(out[r]).any()
    for what in ("nan", "inf", "all -inf"):
        assert np.isnan(out[where[what]]).all() and top[where[what]] == 0, what


def test_rows_do_not_depend_on_the_call(dev, native):
    """Rows [a:b] computed in a call of their own have the bits they have in the
    full call: cuts at 1, at the rows per workgroup and one either side of it."""
    R = native.kf_class_probs_rows()
    rng = np.random.default_rng(5)
    for C in (3, 65, 257, native.kf_class_probs_reg_cols() + 1):
        x = (rng.standard_normal((257, C)) * 40).astype(np.float32)
        px, _ = planted(C, rng)
        x[100: 100 + len(px)] = px
        out, top = run_kernel(dev, x)
        for cut in sorted({1, R - 1, R, R + 1} - {0}):
            for a, b in ((0, cut), (cut, 257), (cut, cut + 1)):
                o, t = run_kernel(dev, x[a:b])
                assert np.array_equal(o.view(np.uint32), out[a:b].view(np.uint32)), (C, a, b)
                assert np.array_equal(t, top[a:b]), (C, a, b)


def test_nothing_is_written_past_the_outputs(dev, native):
    import torch
    from kf2vecfsw_amd import _native as N
    from kf2vecfsw_amd import counter as CN
    pad = 192
    rng = np.random.default_rng(6)
    for Q, C in ((1, 1), (5, 3), (7, 65), (6, 129), (5, native.kf_class_probs_reg_cols() + 1)):
        x = (rng.standard_normal((Q, C)) * 40).astype(np.float32)
        x[Q // 2, 0] = np.nan                                     # the NaN row's stores are bounded too
        d_x = torch.from_numpy(x).to(dev)
        buf = torch.full((Q * (C + 1) + 2 * pad,), -12345.5, dtype=torch.float32, device=dev)
        tbuf = torch.full((Q + 2 * pad,), -77, dtype=torch.int32, device=dev)
        N.check(native.kf_class_probs(d_x.data_ptr(), Q, C, buf[pad:].data_ptr(), tbuf[pad:].data_ptr(),
                                      CN._stream_ptr(dev)), "kf_class_probs")
        h, th = buf.cpu().numpy(), tbuf.cpu().numpy()
        assert np.all(h[:pad] == -12345.5) and np.all(h[pad + Q * (C + 1):] == -12345.5), (Q, C)
        assert np.all(th[:pad] == -77) and np.all(th[pad + Q:] == -77), (Q, C)
        out, top = run_kernel(dev, x)
        assert np.array_equal(h[pad: pad + Q * (C + 1)].view(np.uint32), out.reshape(-1).view(np.uint32)), (Q, C)
        assert np.array_equal(th[pad: pad + Q], top), (Q, C)


# ---------------------------------------------------------------------------
# classify_func on a synthetic library
# ---------------------------------------------------------------------------
def reference_named_module(n_in, hidden, classes):
    """A module with the attribute names of the reference's classifier, in its
    order, and its forward: log_softmax of fc3(relu(fc1(x)))."""
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


def save_classifier(path, nbins, seed=26):
    """classifier_model.ckpt as the trainer saves it.  The last layer is scaled
    down so that, with features of about 300, the logits differ by a few units
    and every class has a probability worth printing.  The default seed gives
    the library's eight rows all three classes, the two largest probabilities
    of a row at least 0.08 apart."""
    import torch
    torch.manual_seed(seed)
    net = reference_named_module(nbins, HIDDEN, CLASSES)
    with torch.no_grad():
        net.fc3.weight.mul_(0.02)
    torch.save({"model_input_size": nbins, "model_hidden_size_fc1": HIDDEN, "model_class_count": CLASSES,
                "state_dict": net.state_dict()}, path)


@pytest.fixture(scope="module")
def library(dev, tmp_path_factory):
    """Seven `.kf` files of k = 3 frequencies written by the project's formatter:
    one file name with a space, one index name with a tab (csv quotes it), one
    file of two rows; and the classifier."""
    from kf2vecfsw_amd import counter as C
    from kf2vecfsw_amd import main as M
    root = tmp_path_factory.mktemp("classify_lib")
    kf, model = root / "kf", root / "model"
    kf.mkdir()
    model.mkdir()
    rng = np.random.default_rng(2021)
    nbins = C.num_bins(K)

    def line(name):
        return M.format_kf(name, rng.integers(1, 4000, nbins).astype(np.uint32))

    for nm in ("G000196015", "G000341695", "G001027105", "plain_one"):
        (kf / (nm + ".kf")).write_bytes(line(nm))
    (kf / "extra two.kf").write_bytes(line("extra two"))
    (kf / "tabbed.kf").write_bytes(line("tab\tname"))
    (kf / "pair.kf").write_bytes(line("pair_a") + line("pair_b"))
    (kf / "notes.txt").write_text("not a .kf file\n")
    save_classifier(str(model / "classifier_model.ckpt"), nbins)
    files = glob.glob(os.path.join(str(kf), "*.kf"))
    assert len(files) == 7
    return dict(kf=str(kf), model=str(model), files=files, root=root, nbins=nbins)


def restate(lib, files, out_dir, block):
    """kf2vec/classify.py:83-124 on the CPU with this test's layout: writes
    <out_dir>/classes.out; returns (labels, logits, probabilities, classes)."""
    import pandas as pd
    import torch
    os.makedirs(out_dir, exist_ok=True)
    state = torch.load(os.path.join(lib["model"], "classifier_model.ckpt"))
    net = reference_named_module(state["model_input_size"], state["model_hidden_size_fc1"], state["model_class_count"])
    net.load_state_dict(state["state_dict"])
    net.eval()
    path = os.path.join(out_dir, "classes.out")
    with open(path, "w", newline="") as f:
        csv.writer(f, delimiter="\t").writerow(["genome", "top_class", "top_p"]
                                               + [str(x) for x in range(state["model_class_count"])])
    labels, logits, probs, tops = [], [], [], []
    with torch.no_grad():
        for z in range(0, len(files), block):
            text = "".join(open(q).read() for q in files[z: z + block])
            df = pd.read_csv(io.StringIO(text), header=None)
            df.set_index(0, inplace=True)
            X = torch.from_numpy(df.values * 1e4).float()
            ps = torch.exp(net(X))
            top_p, top_class = ps.topk(1, dim=1)
            results = np.hstack([df.index.values[:, None], top_class.numpy(), top_p.numpy(), ps.numpy()])
            with open(path, "a", newline="") as f:
                csv.writer(f, delimiter="\t").writerows(results)
            labels += df.index.tolist()
            logits.append(net.fc3(net.relu(net.fc1(X))).numpy())
            probs.append(ps.numpy())
            tops.append(top_class.numpy()[:, 0])
    return labels, np.concatenate(logits), np.concatenate(probs), np.concatenate(tops)


def log_lines(text):
    """The log's messages without the time line."""
    assert text.endswith("\n")
    return re.sub(r"\n(Total time|Time): \d\d:\d\d:\d\d", "", text[:-1])


def table(path):
    """(the header line's bytes, the rows as csv reads them)."""
    data = open(path, "rb").read()
    assert data.endswith(b"\r\n") and b"\n" not in data.replace(b"\r\n", b"")
    rows = list(csv.reader(io.StringIO(data.decode(), newline=""), delimiter="\t"))
    return data.split(b"\r\n")[0], rows[1:]


@pytest.fixture(scope="module")
def run(dev, library):
    """One run of classify_func with the hook, and the restatement."""
    from kf2vecfsw_amd import classify as CL
    out = str(library["root"] / "out")
    os.makedirs(out)
    open(os.path.join(out, "classes.out"), "w").write("stale\n")
    err = io.StringIO()
    with contextlib.redirect_stderr(err):
        kept = CL.classify_func(library["kf"], library["files"], library["model"], 28, out, BLOCK, dev, keep=True)
    ref_out = str(library["root"] / "ref")
    ref = restate(library, library["files"], ref_out, BLOCK)
    return dict(out=out, kept=kept, stderr=err.getvalue(), ref_out=ref_out, ref=ref)


def test_file_header_labels_rows_classes_and_log(library, run):
    head, rows = table(os.path.join(run["out"], "classes.out"))
    ref_head, ref_rows = table(os.path.join(run["ref_out"], "classes.out"))
    assert head == ref_head == b"genome\ttop_class\ttop_p\t0\t1\t2"
    assert len(rows) == len(ref_rows) == 8 and len(run["kept"]) == 4          # seven files in blocks of two
    assert sum(len(b[0]) for b in run["kept"]) == 8                            # one file holds two rows
    for a, b in zip(rows, ref_rows):
        assert a[0] == b[0] and len(a) == len(b) == 3 + CLASSES          # labels, row order, width
        assert a[1] == b[1] and re.fullmatch(r"[0-9]+", a[1])            # the class as text: an int
    labels = [r[0] for r in rows]
    assert labels == run["ref"][0] and {"extra two", "tab\tname", "pair_a", "pair_b"} <= set(labels)
    assert labels.index("pair_b") == labels.index("pair_a") + 1
    assert b'"tab\tname"\t' in open(os.path.join(run["out"], "classes.out"), "rb").read()
    # the log: the reference's messages, in the file and on stderr
    text = open(os.path.join(run["out"], "classification.log")).read()
    assert text == run["stderr"]
    assert log_lines(text) == "\n".join(["\n==> Input arguments...\n", "Feature directory: {}".format(library["kf"]),
                                         "Model: {}".format(library["model"]), "Seed: 28",
                                         "\n==> Building model...\n", "\n==> Classification Completed!\n"])
    assert re.search(r"\nTime: \d\d:\d\d:\d\d\n$", text)
    assert sorted(os.listdir(run["out"])) == ["classes.out", "classification.log"]


def test_file_is_the_host_statement_of_the_runs_tensors(library, run):
    from kf2vecfsw_amd import classify as CL
    from kf2vecfsw_amd import tables as T
    labels = [x for b in run["kept"] for x in b[0]]
    out = np.concatenate([b[2].numpy() for b in run["kept"]])
    top = np.concatenate([b[3] for b in run["kept"]])
    logits = np.concatenate([b[1].numpy() for b in run["kept"]])
    assert out.dtype == np.float32 and top.dtype == np.int32 and logits.shape == (8, CLASSES)
    prefixes = [T.quote_label(nm) + b"\t" + str(int(c)).encode() for nm, c in zip(labels, top)]
    text, _ = T.format_float_rows_host(out, prefixes, T.KF_FLOAT_WIDENED)
    head = T.header_line(CL.classes_header(CLASSES))
    assert open(os.path.join(run["out"], "classes.out"), "rb").read() == head + text
    check_against_host(logits, out, top, "the run's logits")


LOGIT_MEASURED = 3.08e-07            # see test_tensors_match_the_cpu_restatement
LOGIT_MARGIN = 4.0
LOGIT_BOUND = LOGIT_MARGIN * LOGIT_MEASURED


def test_tensors_match_the_cpu_restatement(library, run):
    from kf2vecfsw_amd import query as Q
    labels, ref_logits, ref_p, ref_top = run["ref"]
    assert [x for b in run["kept"] for x in b[0]] == labels
    logits = np.concatenate([b[1].numpy() for b in run["kept"]])
    out = np.concatenate([b[2].numpy() for b in run["kept"]])
    top = np.concatenate([b[3] for b in run["kept"]])
    # the logits: torch's Linear on the device against the CPU's (whose features also went through pandas' parser,
    # not correctly rounded).  Measured on an MI355X for this model (32 inputs of about 300, 8 hidden units of up
    # to a few hundred, a last layer scaled by 0.02, logits up to 2.32): the largest difference is 3.08e-07 of the
    # largest |logit|, 7.1e-07 absolute, three units of float32 at 2.32 after the cancellation in the last layer.
    # LOGIT_BOUND allows LOGIT_MARGIN = 4 times that.
    scale = float(np.abs(ref_logits).max())
    worst = float(np.abs(logits - ref_logits).max()) / scale
    print("logits differ by at most {:.3g} of the largest logit {:.3g}".format(worst, scale))
    assert worst <= LOGIT_BOUND
    # the probabilities: torch's form is within (2|t| + C + 8) * 2^-24 of the softmax of its logits
    # (test_host_classify), the kernel within (|t| + C + 8) * 2^-24 of the softmax of its own; logits that differ by
    # at most d move a softmax by a factor within exp(+-2d): d on the entry's own exponent, d on the sum.
    d = LOGIT_BOUND * scale
    x64 = ref_logits.astype(np.float64)
    t = np.abs(x64 - x64.max(axis=1, keepdims=True))
    r64 = ref_p.astype(np.float64)
    tol = (np.expm1(2 * d) + np.exp(2 * d) * (3 * t + 2 * CLASSES + 16) * U) * r64 + 2 * TINY
    err = np.abs(out[:, 1:].astype(np.float64) - r64)
    print("probabilities use {:.3f} of their tolerance".format(float((err / tol).max())))
    assert np.all(err <= tol)
    # the classes: equal wherever the restatement's two largest probabilities are further apart than twice the
    # tolerance, which is every row here
    srt = np.sort(r64, axis=1)
    clear = srt[:, -1] - srt[:, -2] > 2 * tol.max(axis=1)
    assert clear.all()
    assert np.array_equal(top[clear], ref_top[clear])
    assert len(set(ref_top.tolist())) >= 2                         # more than one class among the eight rows
    # and query reads the file back into the groups that top names (the name with a tab aside: read_classes splits
    # at every tab)
    plain = [nm for nm in labels if "\t" not in nm]
    groups = dict(Q.read_classes(os.path.join(run["out"], "classes.out"), plain))
    want = {}
    for nm, c in zip(labels, top):
        if nm in plain:
            want.setdefault(int(c), []).append(nm)
    assert groups == want and list(groups) == list(want)


def test_cli_classify_writes_the_same_bytes(dev, library, run, capsys):
    from kf2vecfsw_amd import main as M
    out = str(library["root"] / "cli")
    M.main(["classify", "-input_dir", library["kf"], "-model", library["model"], "-o", out, "-block", str(BLOCK),
            "-device", str(dev)])
    assert "==> Classification Completed!" in capsys.readouterr().err
    assert open(os.path.join(out, "classes.out"), "rb").read() == open(os.path.join(run["out"], "classes.out"),
                                                                        "rb").read()
    assert log_lines(open(os.path.join(out, "classification.log")).read()) == \
        log_lines(open(os.path.join(run["out"], "classification.log")).read())


# ---------------------------------------------------------------------------
# process_query_data
# ---------------------------------------------------------------------------
EMB = 5


@pytest.fixture(scope="module")
def query_world(dev, tmp_path_factory):
    """A few FASTA files of a few kbp and one FASTQ, of different base
    composition; the classifier; a QueryNet and a backbone per class; a remap table."""
    import torch
    from kf2vecfsw_amd import counter as C
    from kf2vecfsw_amd import query as Q
    from kf2vecfsw_amd import tables as T
    root = tmp_path_factory.mktemp("pqd")
    fa, cm, dm = root / "fa", root / "classifier", root / "distance"
    for d in (fa, cm, dm):
        d.mkdir()
    rng = np.random.default_rng(99)
    nbins = C.num_bins(K)

    def seq(n, pr):
        return "".join(rng.choice(list("ACGT"), size=n, p=pr))

    comps = [(0.25, 0.25, 0.25, 0.25), (0.4, 0.1, 0.1, 0.4), (0.1, 0.4, 0.4, 0.1), (0.3, 0.3, 0.2, 0.2),
             (0.15, 0.35, 0.15, 0.35)]
    for i, pr in enumerate(comps):
        body = seq(3000 + 500 * i, pr)
        lines = "\n".join(body[j: j + 70] for j in range(0, len(body), 70))
        (fa / "genome_{}.{}".format(i, ("fna", "fa", "fasta")[i % 3])).write_text(
            ">contig_1 of genome {}\n{}\n>contig_2\n{}\n".format(i, lines, seq(400, pr)))
    reads = []
    for j in range(40):
        s = seq(100, (0.35, 0.15, 0.15, 0.35))
        reads.append("@read_{}\n{}\n+\n{}\n".format(j, s, "I" * len(s)))
    (fa / "reads.fq").write_text("".join(reads))
    save_classifier(str(cm / "classifier_model.ckpt"), nbins, seed=12)
    torch.manual_seed(13)
    for c in range(CLASSES):
        net = Q.QueryNet(nbins, HIDDEN, EMB)
        torch.save({"model_input_size": nbins, "model_hidden_size_fc1": HIDDEN, "model_embedding_size": EMB,
                    "state_dict": net.state_dict()}, str(dm / "model_subtree_{}.ckpt".format(c)))
        emb = (rng.standard_normal((3 + c, EMB)) * 40).astype(np.float32)
        T.write_float_table(str(dm / "embeddings_subtree_{}.csv".format(c)), ["B{}_{}".format(c, i) for i in range(3 + c)],
                            torch.from_numpy(emb).to(dev), mode=T.KF_FLOAT_SHORTEST, eol="\n", nan_empty=True)
    remap = root / "remap.tsv"
    remap.write_text("label\tnew_label\ngenome_1\tRenamed one\nreads\tthe reads\nnobody\tx\n")
    return dict(fa=str(fa), cm=str(cm), dm=str(dm), remap=str(remap), root=root)


def snapshot(d):
    """{file name: bytes} of a directory, the logs without their time lines."""
    out = {}
    for f in sorted(os.listdir(d)):
        data = open(os.path.join(d, f), "rb").read()
        out[f] = log_lines(data.decode()).encode() if f.endswith(".log") else data
    return out


@pytest.mark.parametrize("extra", [[], ["-raw_cnt", "-block", "2", "-remap", "REMAP"]], ids=["defaults", "raw_block_remap"])
def test_process_query_data_equals_the_three_subcommands(dev, query_world, capfd, extra):
    from kf2vecfsw_amd import main as M
    w = query_world
    extra = [w["remap"] if a == "REMAP" else a for a in extra]
    out = str(w["root"] / "out")
    shutil.rmtree(out, ignore_errors=True)
    os.makedirs(out)
    raw = ["-raw_cnt"] if "-raw_cnt" in extra else []
    blk = ["-block", "2"] if "-block" in extra else []
    rmp = ["-remap", w["remap"]] if "-remap" in extra else []
    M.main(["get_frequencies", "-input_dir", w["fa"], "-output_dir", out, "-k", str(K), "-device", str(dev)] + raw)
    M.main(["classify", "-input_dir", out, "-model", w["cm"], "-o", out, "-device", str(dev)] + blk)
    M.main(["query", "-input_dir", out, "-model", w["dm"], "-classes", out, "-o", out, "-device", str(dev)] + blk + rmp)
    want = snapshot(out)
    capfd.readouterr()
    kf = sorted(f for f in want if f.endswith(".kf"))
    assert kf == ["genome_{}.kf".format(i) for i in range(5)] + ["reads.kf"]
    clades = sorted(int(f[len("embedding_subtree_"):-4]) for f in want if f.startswith("embedding_subtree_"))
    assert clades and sorted(want) == sorted(kf + ["classes.out", "classification.log", "query_run.log"]
                                             + ["embedding_subtree_{}.emb".format(c) for c in clades]
                                             + ["apples_input_di_mtrx_subtree_{}.csv".format(c) for c in clades])
    assert want["classes.out"].count(b"\r\n") == 7
    if rmp:
        assert b"Renamed one\t" in b"".join(want[f] for f in want if f.endswith(".emb"))
    shutil.rmtree(out)
    os.makedirs(out)
    M.main(["process_query_data", "-input_dir", w["fa"], "-output_dir", out, "-k", str(K), "-classifier_model", w["cm"],
            "-distance_model", w["dm"], "-device", str(dev)] + extra)
    got = snapshot(out)
    assert sorted(got) == sorted(want)
    for f in want:
        assert got[f] == want[f], f
    said = capfd.readouterr().out
    banners = ["\n==> Computing k-mer frequences\n", "\n==> Classifying query samples\n",
               "\n==> Computing model distances\n", "\n==> Query processing step is completed!\n"]
    at = [said.find(b + "\n") for b in banners]
    assert -1 not in at and at == sorted(at)
