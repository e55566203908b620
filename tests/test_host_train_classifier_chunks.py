"""CPU tests of train_classifier_chunks' pure parts: the runs of
Dataset_chunks_1row (train_chunks.draw_runs with views=1), the log's lines in
the reference's order (kf2vec/train_classifier_model_chunks.py:113-149), the
parser against the reference's options and defaults (kf2vec/main.py:1452-1486),
-mask, and the refusals that need no device."""
import argparse
import os

import pytest

from conftest import TOY


# ---------------------------------------------------------------- the runs
def test_draw_runs_one_view_invariants():
    import torch
    from kf2vecfsw_amd import train_chunks as TC
    gen = torch.Generator()
    gen.manual_seed(5)
    for c in (1, 2, 5, 37, 1000):
        ct = torch.full((4000,), c, dtype=torch.int64)
        lo, n = TC.draw_runs(ct, gen, views=1)
        assert lo.shape == n.shape == (4000, 1) and lo.dtype == n.dtype == torch.int64
        assert int(n.min()) >= 1 and int(n.max()) <= c
        assert int(lo.min()) >= 0 and bool((lo <= c - n).all())
        if c == 1:
            assert not bool(lo.any()) and bool((n == 1).all())           # always (0, 1)
        if c >= 5:
            assert int(n.max()) > 1 and int(lo.max()) > 0
    c = torch.tensor([1, 2, 5, 37, 1000])
    lo, n = TC.draw_runs(c, gen, views=1)                                 # a mixed table
    c = c.reshape(-1, 1)
    assert lo.shape == (5, 1) and bool(((n >= 1) & (n <= c) & (lo >= 0) & (lo <= c - n)).all())


def test_draw_runs_one_view_leaves_the_same_stream_whatever_the_data():
    import torch
    from kf2vecfsw_amd import train_chunks as TC
    after = []
    for c in (1, 7, 1000):
        gen = torch.Generator()
        gen.manual_seed(9)
        TC.draw_runs(torch.full((100,), c, dtype=torch.int64), gen, views=1)
        after.append(torch.rand(4, generator=gen))
    assert torch.equal(after[0], after[1]) and torch.equal(after[0], after[2])
    gen = torch.Generator()
    gen.manual_seed(9)
    torch.empty((100, 1), dtype=torch.float64).exponential_(1.0, generator=gen)
    torch.rand((100, 1), dtype=torch.float64, generator=gen)
    torch.rand((100, 1), dtype=torch.float64, generator=gen)
    assert torch.equal(torch.rand(4, generator=gen), after[0])


def test_epoch_batches_has_a_views_keyword_that_defaults_to_two():
    import inspect
    from kf2vecfsw_amd import train_chunks as TC
    p = inspect.signature(TC.epoch_batches).parameters["views"]
    assert p.default == TC.VIEWS == 2
    assert TC.slab_plan([(0, 4), (4, 8), (8, 9)], 100, 800, views=1) == [(0, 2), (2, 3)]
    assert TC.slab_plan([(0, 4), (4, 8), (8, 9)], 100, 800) == [(0, 1), (1, 2), (2, 3)]


# ---------------------------------------------------------------- the log
def test_log_opening_is_the_references_order():
    from kf2vecfsw_amd import train_classifier as TC
    from kf2vecfsw_amd import train_classifier_chunks as TCC
    for cap in (False, True):
        lines = TCC.log_opening("chunks_dir", "x.subtrees", True, 2048, 10, 16, 1e-5, 3e-6, 2000, 28, False, cap)
        assert lines == ["\n==> Input arguments...\n", "Feature directory: chunks_dir", "Clades information: x.subtrees",
                         "\n==> Parameters...\n", "GPU Support: Yes", "Hidden Size fc1: 2048", "Starting Epoch: 0",
                         "Total Epochs: 10", "Batch Size: 16", "Learning Rate: 1e-05", "Learning Rate Min: 3e-06",
                         "Learning Rate Decay: 2000", "Random Seed: 28", "Masking: False",
                         "Cap kmer frequencies: {}".format(cap), "\n==> Preparing Data...\n"]
        base = TC.log_opening("chunks_dir", "x.subtrees", True, 2048, 10, 16, 1e-5, 3e-6, 2000, 28, False)
        assert [ln for ln in lines if not ln.startswith("Cap kmer")] == base        # train_classifier's, and its omissions


# ---------------------------------------------------------------- the parser
def test_parser_lists_the_command_with_the_references_defaults():
    from kf2vecfsw_amd import main as M
    p = M.build_parser()
    assert "train_classifier_chunks " in p.format_help()
    a = p.parse_args(["train_classifier_chunks"])
    assert (a.e, a.hidden_sz, a.batch_sz, a.lr, a.lr_min, a.lr_decay, a.seed) == (2000, 2048, 16, 1e-5, 3e-6, 2000, 28)
    assert (a.input_dir, a.input_dir_fullgenomes, a.subtrees, a.o, a.device) == (None,) * 5
    assert a.mask is False and a.cap is False and a.func is M.train_classifier_chunks
    sub = [x for x in p._actions if isinstance(x, argparse._SubParsersAction)][0].choices["train_classifier_chunks"]
    text = sub.format_help()
    assert "-mask" not in text                                                       # hidden, as in the reference
    for opt in ("-input_dir", "-input_dir_fullgenomes", "-subtrees", "-e", "-hidden_sz", "-batch_sz", "-lr", "-lr_min",
                "-lr_decay", "-seed", "-cap", "-o", "-device"):
        assert opt + " " in text or opt + "\n" in text, opt
    a = p.parse_args(["train_classifier_chunks", "-mask", "-cap", "-e", "10", "-device", "cuda:1",
                      "-input_dir_fullgenomes", "full"])
    assert (a.mask, a.cap, a.e, a.device, a.input_dir_fullgenomes) == (True, True, 10, "cuda:1", "full")


# ---------------------------------------------------------------- refused without a device
def kf_names(tmp_path, names):
    """Paths of `.kf` files that need not exist: what is refused here is refused before a file is read."""
    return [str(tmp_path / (nm + ".kf")) for nm in names]


def test_refused_before_the_device_is_touched(tmp_path, capsys):
    from kf2vecfsw_amd import main as M
    from kf2vecfsw_amd import train_classifier as TC
    from kf2vecfsw_amd import train_classifier_chunks as TCC
    subtrees = os.path.join(TOY, "train_tree.subtrees")
    names = ["G000830275", "G000402355", "G001940645"]
    out = tmp_path / "out"

    def run(files, clades, mask=False, cap=False):
        return TCC.train_classifier_model_chunks_func(str(tmp_path), str(tmp_path), files, clades, 1, 8, 16, 1e-5, 3e-6,
                                                      2000, 28, mask, cap, str(out))

    # -mask: train_classifier's text, for this command
    assert TCC.MASK_MESSAGE.startswith("train_classifier_chunks: -mask is not supported")
    assert TCC.MASK_MESSAGE.split(": ", 1)[1] == TC.MASK_MESSAGE.split(": ", 1)[1]
    with pytest.raises(SystemExit) as e:
        run(kf_names(tmp_path, names), subtrees, mask=True, cap=True)
    assert e.value.code == TCC.MASK_MESSAGE
    with pytest.raises(SystemExit) as e:
        M.main(["train_classifier_chunks", "-input_dir", str(tmp_path), "-input_dir_fullgenomes", str(tmp_path),
                "-subtrees", subtrees, "-o", str(out), "-mask"])
    assert e.value.code == TCC.MASK_MESSAGE
    assert capsys.readouterr().out == "Running train_classifier_chunks\n"
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
