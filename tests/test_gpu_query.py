"""GPU test of the `query` subcommand on a synthetic library made here: two
clades, k = 3, a checkpoint per clade as the distance trainers save it, a
backbone of a few genomes written through tables.write_float_table, `.kf` files
named as the toy example's queries (and two more), a -block smaller than a
clade and a remap table.  The run's files are compared with a restatement of
kf2vec/query.py:108-192 on the CPU (pandas, the model on the CPU, torch.cdist,
.tolist() and csv.writer) and, byte for byte, with the host statement of the
formatter on the tensors the run produced."""
import csv
import io
import os
import re

import numpy as np
import pytest

from conftest import TOY

pytestmark = pytest.mark.gpu

K = 3
HIDDEN, EMB = 8, 5
BLOCK = 2
CLADES = {0: 3, 1: 4}            # genomes per clade, both above BLOCK
BACKBONE = {0: 4, 1: 6}


@pytest.fixture(scope="module")
def dev(native):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu tests need an MI355X")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def library(dev, tmp_path_factory):
    """The synthetic library on disk: (dirs, names per clade, backbone tables,
    models' state).  The `.kf` files carry the toy example's query names, but
    their rows are k = 3 frequencies of random counts written by the project's
    formatter: the toy fixtures are k = 7."""
    import torch
    from kf2vecfsw_amd import counter as C
    from kf2vecfsw_amd import main as M
    from kf2vecfsw_amd import tables as T
    root = tmp_path_factory.mktemp("query_lib")
    kf, model, classes = root / "kf", root / "model", root / "classes"
    for d in (kf, model, classes):
        d.mkdir()
    rng = np.random.default_rng(2020)
    nbins = C.num_bins(K)
    toy = sorted(f[:-6] for f in os.listdir(os.path.join(TOY, "test_kf")))       # G000196015 ...
    names = toy + ["extra_one", "extra two"]
    assert len(names) == sum(CLADES.values())
    for nm in names:
        counts = rng.integers(1, 4000, nbins).astype(np.uint32)
        (kf / (nm + ".kf")).write_bytes(M.format_kf(nm, counts))
    (kf / "not_classified.kf").write_bytes(M.format_kf("not_classified", rng.integers(1, 9, nbins).astype(np.uint32)))
    # classes.out: the clades interleaved, so that order of first appearance and file order both matter
    order = [names[i] for i in (3, 0, 4, 1, 5, 2, 6)]
    clade_of = {nm: (1 if i % 2 == 0 else 0) for i, nm in enumerate(order)}
    lines = ["genome\ttop_class\ttop_p\t0\t1"]
    for nm in order:
        lines.append("{}\t{}.0\t0.9\t0.5\t0.5".format(nm, clade_of[nm]))
    lines.append("absent_genome\t1.0\t0.9\t0.5\t0.5")                            # has no .kf: not queried
    (classes / "classes.out").write_text("\n".join(lines) + "\n")
    torch.manual_seed(5)
    states, backbones = {}, {}
    for c, nb in BACKBONE.items():
        from kf2vecfsw_amd import query as Q
        net = Q.QueryNet(nbins, HIDDEN, EMB)
        states[c] = {k: v.clone() for k, v in net.state_dict().items()}
        torch.save({"model_input_size": nbins, "model_hidden_size_fc1": HIDDEN, "model_embedding_size": EMB,
                    "state_dict": net.state_dict()}, str(model / "model_subtree_{}.ckpt".format(c)))
        emb = (rng.standard_normal((nb, EMB)) * 40).astype(np.float32)
        bnames = ["B{}_{}".format(c, i) for i in range(nb)]
        # as the trainers' to_csv(sep='\t', header=False) of a float32 frame writes it
        T.write_float_table(str(model / "embeddings_subtree_{}.csv".format(c)), bnames, torch.from_numpy(emb).to(dev),
                            mode=T.KF_FLOAT_SHORTEST, eol="\n", nan_empty=True)
        backbones[c] = (bnames, emb)
    remap = root / "remap.tsv"
    remap.write_text("label\tnew_label\n{}\tRenamed one\n{}\tcomma,name\nnobody\tx\n".format(names[0], names[5]))
    return dict(kf=str(kf), model=str(model), classes=str(classes), remap=str(remap), names=names, order=order,
                clade_of=clade_of, states=states, backbones=backbones, root=root)


def restate(lib, out_dir, block):
    """kf2vec/query.py:53-200 on the CPU, the reference's lines with this test's
    file layout: returns the log lines (without the two times) and per clade the
    labels, embeddings and distances."""
    import pandas as pd
    import torch
    from kf2vecfsw_amd import query as Q
    os.makedirs(out_dir, exist_ok=True)
    log = ["\n==> Input arguments...\n", "Query directory: {}".format(lib["kf"]),
           "Model directory: {}".format(lib["model"]), "Class information: {}".format(lib["classes"]), "Seed: 28",
           "\n==> Querying...\n"]
    files = [os.path.join(lib["kf"], f) for f in os.listdir(lib["kf"]) if f.endswith(".kf")]
    df_all = pd.read_csv(os.path.join(lib["classes"], "classes.out"), sep="\t", header=0)
    base = [os.path.basename(q).split(".kf")[0] for q in files]
    df = df_all.loc[df_all.genome.isin(base)].copy()
    df["top_class"] = df["top_class"].astype(int)
    log.append("Total subtrees to query: {}".format(df.top_class.unique().size))
    mp = pd.read_csv(lib["remap"], sep="\t", header=0)
    remap = pd.Series(mp.new_label.values, index=mp.label).to_dict()
    log.append("Remap loaded: {} entries".format(len(remap)))
    result = {}
    for c in df.top_class.unique():
        ids = df.loc[df["top_class"] == c]["genome"].to_list()
        log.append("\n==> Working on subtree {} ({} contigs)...\n".format(c, len(ids)))
        state = torch.load(os.path.join(lib["model"], "model_subtree_{}.ckpt".format(c)))
        net = Q.QueryNet(state["model_input_size"], state["model_hidden_size_fc1"], state["model_embedding_size"])
        net.load_state_dict(state["state_dict"])
        net.eval()
        de = pd.read_csv(os.path.join(lib["model"], "embeddings_subtree_{}.csv".format(c)), sep="\t", header=None,
                         index_col=0)
        et = torch.from_numpy(de.values).float()
        dist_path = os.path.join(out_dir, "apples_input_di_mtrx_subtree_{}.csv".format(c))
        emb_path = os.path.join(out_dir, "embedding_subtree_{}.emb".format(c))
        labels, embs, dists = [], [], []
        with open(dist_path, "w", newline="") as fd, open(emb_path, "w", newline="") as fe:
            dw, ew = csv.writer(fd, delimiter="\t"), csv.writer(fe, delimiter="\t")
            dw.writerow([""] + de.index.tolist())
            with torch.no_grad():
                for z in range(0, len(ids), block):
                    text = "".join(open(os.path.join(lib["kf"], f + ".kf")).read() for f in ids[z: z + block])
                    fi = pd.read_csv(io.StringIO(text), index_col=None, header=None, sep=",")
                    fi.set_index(0, inplace=True)
                    fi = fi.iloc[:, :] * 1e4
                    ql = [remap.get(q, q) for q in fi.index.tolist()]
                    out = net(torch.from_numpy(fi.values).float())
                    pw = torch.square(torch.cdist(out, et, p=2, compute_mode="donot_use_mm_for_euclid_dist"))
                    pw = torch.where(pw < 1.0e-6, torch.tensor(0, dtype=pw.dtype), pw)
                    for lbl, row in zip(ql, pw.numpy().tolist()):
                        dw.writerow([lbl] + row)
                    for lbl, row in zip(ql, out.numpy().tolist()):
                        ew.writerow([lbl] + row)
                    labels += ql
                    embs.append(out.numpy())
                    dists.append(pw.numpy())
        log += ["Wrote distance matrix: {}".format(dist_path), "Wrote embeddings: {}".format(emb_path),
                "\n==> Computation is completed for subtree {}!\n".format(c)]
        result[int(c)] = (labels, np.concatenate(embs), np.concatenate(dists), et.numpy())
    log.append("\n==> Computation Completed!\n")
    return log, result


def log_lines(text):
    """The log's messages without the two kinds of time lines."""
    msgs = text.split("\n")
    assert msgs[-1] == ""
    body = "\n".join(msgs[:-1])
    body = re.sub(r"\n(Total time|Time): \d\d:\d\d:\d\d", "", body)
    return body


@pytest.fixture(scope="module")
def run(dev, library):
    """One run of query_func with the hook, and the restatement."""
    import contextlib
    from kf2vecfsw_amd import query as Q
    out = str(library["root"] / "out")
    files = [os.path.join(library["kf"], f) for f in os.listdir(library["kf"]) if f.endswith(".kf")]
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        kept = Q.query_func(library["kf"], files, library["model"], library["classes"], 28, out, library["remap"],
                            BLOCK, dev, keep=True)
    ref_out = str(library["root"] / "ref")
    ref_log, ref = restate(library, ref_out, BLOCK)
    return dict(out=out, kept=kept, stdout=buf.getvalue(), ref_out=ref_out, ref_log=ref_log, ref=ref)


def test_files_header_labels_rows_and_log(library, run):
    out, ref_out = run["out"], run["ref_out"]
    assert sorted(os.listdir(out)) == sorted(os.listdir(ref_out) + ["query_run.log"])
    assert [c for c, *_ in run["kept"]] == [1, 1, 0, 0]      # clades by first appearance, blocks of two
    for f in sorted(os.listdir(ref_out)):
        got, exp = open(os.path.join(out, f), "rb").read(), open(os.path.join(ref_out, f), "rb").read()
        gl, el = got.split(b"\r\n"), exp.split(b"\r\n")
        assert gl[-1] == b"" and len(gl) == len(el), f
        assert b"\n" not in got.replace(b"\r\n", b""), f
        if f.endswith(".csv"):
            assert gl[0] == el[0] and gl[0].startswith(b"\tB"), f                   # the header, bytes
        for a, b in zip(gl[:-1], el[:-1]):
            fa, fb = a.split(b"\t"), b.split(b"\t")
            assert fa[0] == fb[0] and len(fa) == len(fb), f                         # labels, row order, width
    names = library["names"]
    emb1 = open(os.path.join(out, "embedding_subtree_1.emb"), "rb").read()
    assert b"Renamed one\t" in emb1 + open(os.path.join(out, "embedding_subtree_0.emb"), "rb").read()
    both = emb1 + open(os.path.join(out, "embedding_subtree_0.emb"), "rb").read()
    assert b'"comma,name"\t' not in both and b"comma,name\t" in both               # a comma needs no quotes with tabs
    assert names[0].encode() + b"\t" not in both and b"not_classified" not in both
    # the log: the same lines in the file and on stdout, the reference's messages
    text = open(os.path.join(out, "query_run.log")).read()
    assert text == run["stdout"]
    want = "\n".join(run["ref_log"]).replace(ref_out, out)
    assert log_lines(text) == want
    assert len(re.findall(r"\nTime: \d\d:\d\d:\d\d\n", text)) == 2 and re.search(r"\nTotal time: \d\d:\d\d:\d\d\n$", text)


def test_files_are_the_host_statement_of_the_runs_tensors(library, run):
    from kf2vecfsw_amd import tables as T
    for c in (0, 1):
        blocks = [b for b in run["kept"] if b[0] == c]
        labels = [x for b in blocks for x in b[1]]
        emb = np.concatenate([b[2].numpy() for b in blocks])
        dist = np.concatenate([b[3].numpy() for b in blocks])
        assert emb.dtype == np.float32 and dist.dtype == np.float32
        quoted = [T.quote_label(x).decode() for x in labels]
        text, _ = T.format_float_rows_host(emb, quoted, T.KF_FLOAT_WIDENED)
        assert open(os.path.join(run["out"], "embedding_subtree_{}.emb".format(c)), "rb").read() == text
        text, _ = T.format_float_rows_host(dist, quoted, T.KF_FLOAT_WIDENED)
        head = T.header_line([""] + library["backbones"][c][0])
        assert open(os.path.join(run["out"], "apples_input_di_mtrx_subtree_{}.csv".format(c)), "rb").read() == head + text


def test_tensors_match_the_cpu_restatement(library, run):
    from kf2vecfsw_amd import query as Q
    for c in (0, 1):
        blocks = [b for b in run["kept"] if b[0] == c]
        emb = np.concatenate([b[2].numpy() for b in blocks])
        dist = np.concatenate([b[3].numpy() for b in blocks])
        labels, ref_emb, ref_dist, backbone = run["ref"][c]
        assert [x for b in blocks for x in b[1]] == labels
        # the backbone went through write_float_table and backbone_embeddings: the same float32
        assert np.array_equal(backbone.view(np.uint32), library["backbones"][c][1].view(np.uint32))
        # the distances: the statement on the run's own embeddings bit for bit, and within
        # (D + 8) * 2^-24 (test_host_float_format) of their float64 value
        assert np.array_equal(dist.view(np.uint32), Q.sq_distances_host(emb, backbone).view(np.uint32))
        exact = ((emb.astype(np.float64)[:, None, :] - backbone.astype(np.float64)[None, :, :]) ** 2).sum(-1)
        assert exact.min() > 1e-3                                                  # none near the cut
        assert np.all(np.abs(dist - exact) <= (EMB + 8) * 2.0 ** -24 * exact)
        # the embeddings: torch's Linear on the device against the CPU's (whose features also went through pandas'
        # parser, not correctly rounded).  Measured on an MI355X for this model (32 inputs of about 300, 8 hidden
        # units, outputs up to 78 and 155): the largest difference is 1.87e-07 (clade 0) and 9.85e-08 (clade 1) of
        # the largest |output|, one to two units of float32 there; EMB_BOUND = 2^-20 = 9.5e-07 allows 5 times that.
        scale = float(np.abs(ref_emb).max())
        worst = float(np.abs(emb - ref_emb).max()) / scale
        print("clade {}: embeddings differ by at most {:.3g} of the largest output {:.3g}".format(c, worst, scale))
        assert worst <= EMB_BOUND
        # and the restatement's distances are those of its own embeddings: the two runs' distances differ by
        # what the embeddings' difference moves them, 2 * |e - e'| * sqrt(d) to first order, plus rounding
        delta = np.sqrt(EMB) * EMB_BOUND * scale
        move = 2 * np.sqrt(exact) * delta + delta ** 2 + 4 * (EMB + 8) * 2.0 ** -24 * exact
        assert np.all(np.abs(dist - ref_dist) <= move)


EMB_BOUND = 2.0 ** -20           # see test_tensors_match_the_cpu_restatement


def test_cli_writes_the_same_files(dev, library, run, capsys):
    from kf2vecfsw_amd import main as M
    out = str(library["root"] / "cli")
    M.main(["query", "-input_dir", library["kf"], "-model", library["model"], "-classes", library["classes"], "-o", out,
            "-block", str(BLOCK), "-remap", library["remap"], "-device", str(dev)])
    assert "Total subtrees to query: 2" in capsys.readouterr().out
    for f in os.listdir(run["out"]):
        if f != "query_run.log":
            assert open(os.path.join(out, f), "rb").read() == open(os.path.join(run["out"], f), "rb").read(), f
    assert M.build_parser().parse_args(["query"]).block == 4000 and M.build_parser().parse_args(["query"]).seed == 28
