"""CPU tests of train_model_set_chunks: the parser; kf_dist_loss_views' symbol and
its refusals before any HIP call (fake non-null addresses, there is no device
here); train.dist_loss_host with views and eps against its own earlier form and
against the reference's lines (np.repeat of the labels, Loss_chunks) in float64;
train_chunks.draw_runs on a CPU generator (its invariants and, at c = 5, its
exact distribution); and the consecutive-best rule against a literal deque and
nanmean."""
import math
from collections import deque

import numpy as np
import pytest

import train_inputs


def fake(i, off=0):
    """A fake device address, aligned to 4 KiB plus `off`."""
    return (0x7000_0000_0000 + (i << 32)) + off


# ---------------------------------------------------------------- the CLI
def test_parser_lists_the_command_with_the_references_defaults():
    from kf2vecfsw_amd import main as M
    p = M.build_parser()
    assert "train_model_set_chunks " in p.format_help()
    a = p.parse_args(["train_model_set_chunks"])
    assert (a.e, a.hidden_sz, a.embed_sz, a.batch_sz, a.lr, a.lr_min, a.lr_decay, a.seed) == \
        (8000, 2048, 1024, 16, 1e-5, 3e-6, 2000, 28)
    assert (a.input_dir, a.input_dir_fullgenomes, a.true_dist, a.subtrees, a.clade, a.o, a.device) == (None,) * 7
    assert a.cap is False and a.func is M.train_model_set_chunks
    a = p.parse_args(["train_model_set_chunks", "-clade", "1", "3", "-cap", "-device", "cuda:1", "-input_dir_fullgenomes",
                      "full"])
    assert (a.clade, a.cap, a.device, a.input_dir_fullgenomes) == ([1, 3], True, "cuda:1", "full")
    with pytest.raises(SystemExit):
        p.parse_args(["train_model_set_chunks", "-test_set", "x"])    # the reference's command has no test set


# ---------------------------------------------------------------- the C-ABI
def test_symbol_exported(native):
    from kf2vecfsw_amd import _native as N
    assert hasattr(native, "kf_dist_loss_views") and "kf_dist_loss_views" in N.SIGNATURES


def call(native, **kw):
    B = 100
    a = dict(y=fake(1), B=B, E=16, P=fake(2), N=200, labels=fake(3), views=2, eps=1000.0, loss=fake(4), grad=fake(5),
             status=fake(6), scratch=fake(7), scratch_bytes=12 * B * B + 8 * B)
    a.update(kw)
    return native.kf_dist_loss_views(a["y"], a["B"], a["E"], a["P"], a["N"], a["labels"], a["views"], a["eps"], a["loss"],
                                     a["grad"], a["status"], a["scratch"], a["scratch_bytes"], None)


REFUSALS = [
    ("views == 0", dict(views=0), b"views == 0"),
    ("B no multiple of views", dict(views=3), b"no multiple of views"),
    ("views above B", dict(views=101), b"no multiple of views"),
    ("eps NaN", dict(eps=float("nan")), b"eps = "),
    ("eps infinite", dict(eps=float("inf")), b"eps = "),
    ("eps negative", dict(eps=-1e-6), b"eps = "),
    # kf_dist_loss' own, through this entry, named after it
    ("B == 0", dict(B=0), b"kf_dist_loss_views: B == 0"),
    ("null labels", dict(labels=None), b"kf_dist_loss_views: null d_labels"),
    ("scratch too small", dict(scratch_bytes=12 * 100 * 100 + 8 * 100 - 1), b"needed"),
    ("grad off by 1", dict(grad=fake(5, 1)), b"misaligned d_grad"),
]


@pytest.mark.parametrize("what,kw,msg", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_dist_loss_views_refuses_before_any_hip_call(native, what, kw, msg):
    from kf2vecfsw_amd import _native as N
    assert call(native, **kw) == N.KF_EINVAL, what
    assert msg in native.kf_last_error(), native.kf_last_error()


# ---------------------------------------------------------------- the host statement
def earlier_dist_loss_host(y, P, labels):
    """train.dist_loss_host as it stood before views and eps: a label per row and 1e-6."""
    y = np.ascontiguousarray(y, dtype=np.float32)
    lab = np.asarray(labels, dtype=np.int64).reshape(-1)
    b, e = y.shape
    with np.errstate(all="ignore"):
        s = np.zeros((b, b), dtype=np.float32)
        for k in range(e):
            t = y[:, k, None] - y[None, :, k]
            s = s + t * t
        d = np.sqrt(s)
        tt = P[np.ix_(lab, lab)]
        w = 1.0 / (tt + 1e-6)
        r = np.sqrt(tt)
        u = d.astype(np.float64) - r
        v = (u * u) * w
        inv = 1.0 / float(b * b)
        rows = np.zeros(b, dtype=np.float64)
        for j in range(b):
            rows = rows + v[:, j]
        total = np.float64(0.0)
        for i in range(b):
            total = total + rows[i]
        loss = np.float64(total * inv)
        g = (((2.0 * u) * w) * inv).astype(np.float32)
        gs = g + g.T
        c = np.where(d == 0, np.float32(0), gs / d).astype(np.float32)
        grad = np.zeros((b, e), dtype=np.float32)
        for j in range(b):
            grad = grad + c[:, j, None] * (y - y[j][None, :])
    return loss, grad


@pytest.mark.parametrize("B,E", [(1, 5), (2, 3), (7, 1), (16, 64), (65, 33)])
def test_dist_loss_host_defaults_give_the_bits_they_gave(B, E):
    from kf2vecfsw_amd import train as TR
    y, P, labels = train_inputs.make(B, E)
    want = earlier_dist_loss_host(y, P, labels)
    for got in (TR.dist_loss_host(y, P, labels), TR.dist_loss_host(y, P, labels, views=1, eps=1e-6)):
        assert got[0].tobytes() == want[0].tobytes()
        assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
    # views alone is the repeat of the labels
    a = TR.dist_loss_host(np.repeat(y, 2, axis=0), P, labels, views=2)
    b = TR.dist_loss_host(np.repeat(y, 2, axis=0), P, np.repeat(labels, 2))
    assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


VIEWS, EPS = 2, 1000.0


def chunk_inputs(G, E, seed):
    """train_inputs.make for 2 G rows, the inputs test_host_train.py's rule was made on, with the first G labels."""
    y, P, labels = train_inputs.make(VIEWS * G, E, seed)
    return y, P, labels[:G].copy()


def reference_lines(y, P, labels, dtype):
    """kf2vec/train_model_set_chunks.py:392-418 with losses.py:58-117 under autograd on the CPU."""
    import torch
    lab = np.repeat(np.asarray(labels), VIEWS)                                    # torch.repeat_interleave(labels, 2)
    yt = torch.from_numpy(np.asarray(y)).to(dtype).requires_grad_(True)
    real_dist = torch.from_numpy(P[np.ix_(list(lab), list(lab))])
    train_dist = torch.cdist(yt, yt, p=2, compute_mode="donot_use_mm_for_euclid_dist")
    weight = 1 / (real_dist + 1000)
    true_dist = torch.sqrt(real_dist)
    loss = ((train_dist - true_dist) ** 2 * weight).mean()
    loss.backward()
    return float(loss.detach().to(torch.float64)), yt.grad.detach().to(torch.float64).numpy()


DRAWS = 16


@pytest.mark.parametrize("G,E", [(1, 5), (2, 3), (8, 1024), (33, 33)])
def test_dist_loss_host_views_is_as_accurate_as_the_reference(G, E):
    """test_host_train.py's rule for the Loss form, at views = 2 and eps = 1000: the
    statement's loss and gradient errors against the reference's lines in float64 are at
    most twice those of the reference's own float32 path on the same inputs -- over DRAWS
    inputs per shape, and on every input down to the floor of the roundings on the way to
    one value ((8 + B + E / 2) * 2^-24 of the largest gradient entry; for the loss the mean
    of 2 |u| w d over the pairs times (1 + E / 2) * 2^-24), B = 2 G rows.
    The worst of DRAWS inputs is a noisy figure: measured here, the gradient's ratio is 0.94
    (8, 1024) and 1.21 (33, 33) on these inputs; with the same inputs scaled to true
    distances of (50, 3000) it was 1.00, 1.38 at (32, 33), 2.04 at (33, 33) and 1.35 at
    (65, 33): the sums of the contract are sequential, the reference's are not."""
    import torch
    from kf2vecfsw_amd import train as TR
    U = 2.0 ** -24
    B = VIEWS * G
    host_err = ref_err = host_gerr = ref_gerr = 0.0
    for seed in range(DRAWS):
        y, P, labels = chunk_inputs(G, E, seed)
        true_loss, true_grad = reference_lines(y, P, labels, torch.float64)
        ref_loss, ref_grad = reference_lines(y, P, labels, torch.float32)
        loss, grad = TR.dist_loss_host(y, P, labels, views=VIEWS, eps=EPS)
        assert isinstance(loss, np.float64) and grad.dtype == np.float32 and grad.shape == (B, E)
        assert np.isfinite(loss) and np.isfinite(grad).all()
        scale = abs(true_loss) if true_loss != 0 else 1.0
        gscale = float(np.abs(true_grad).max()) or 1.0
        y64 = y.astype(np.float64)
        d = np.sqrt(((y64[:, None, :] - y64[None, :, :]) ** 2).sum(-1))
        lab = np.repeat(labels, VIEWS)
        T = P[np.ix_(lab, lab)]
        moved = float((2 * np.abs(d - np.sqrt(T)) / (T + EPS) * d).mean())
        loss_floor, grad_floor = moved * (1 + E / 2) * U / scale, (8 + B + E / 2) * U
        h, r = abs(float(loss) - true_loss) / scale, abs(ref_loss - true_loss) / scale
        hg = float(np.abs(grad.astype(np.float64) - true_grad).max()) / gscale
        rg = float(np.abs(ref_grad - true_grad).max()) / gscale
        assert h <= max(2 * r, loss_floor), (seed, h, r, loss_floor)
        assert hg <= max(2 * rg, grad_floor), (seed, hg, rg, grad_floor)
        host_err, ref_err, host_gerr, ref_gerr = max(host_err, h), max(ref_err, r), max(host_gerr, hg), max(ref_gerr, rg)
    print("G={} E={}: loss error {:.3g} (reference {:.3g}), gradient error {:.3g} (reference {:.3g})".format(
        G, E, host_err, ref_err, host_gerr, ref_gerr))
    assert host_err <= 2 * ref_err
    assert host_gerr <= 2 * ref_gerr


def test_dist_loss_host_views_planted_values():
    """One genome, two views at distance 5: its own true distance P[0, 0] = 16 enters all four pairs."""
    from kf2vecfsw_amd import train as TR
    y = np.array([[0, 0], [3, 4]], dtype=np.float32)
    P = np.array([[16.0]])
    loss, grad = TR.dist_loss_host(y, P, [0], views=2, eps=1000.0)
    w = 1.0 / (16.0 + 1000.0)
    assert loss == (((4.0 * 4.0) * w + (1.0 * 1.0) * w) + ((1.0 * 1.0) * w + (4.0 * 4.0) * w)) * 0.25
    g = np.float32(((2.0 * 1.0) * w) * 0.25)
    c = (g + g) / np.float32(5)
    assert np.array_equal(grad, np.array([[c * np.float32(-3), c * np.float32(-4)],
                                          [c * np.float32(3), c * np.float32(4)]], dtype=np.float32))


# ---------------------------------------------------------------- the runs
def test_draw_runs_invariants():
    import torch
    from kf2vecfsw_amd import train_chunks as TC
    gen = torch.Generator()
    gen.manual_seed(5)
    for c in (1, 2, 5, 37, 1000):
        ct = torch.full((4000,), c, dtype=torch.int64)
        lo, n = TC.draw_runs(ct, gen)
        assert lo.shape == n.shape == (4000, 2) and lo.dtype == n.dtype == torch.int64
        assert int(n.min()) >= 1 and int(n.max()) <= c
        assert int(lo.min()) >= 0 and bool((lo <= c - n).all())
        if c >= 5:
            assert int(n.max()) > 1 and int(lo.max()) > 0
    lo, n = TC.draw_runs(torch.tensor([1, 2, 5, 37, 1000]), gen, views=3)     # a mixed table
    c = torch.tensor([1, 2, 5, 37, 1000]).reshape(-1, 1)
    assert lo.shape == (5, 3) and bool(((n >= 1) & (n <= c) & (lo >= 0) & (lo <= c - n)).all())


def test_draw_runs_consumes_three_tensors_whatever_the_data():
    import torch
    from kf2vecfsw_amd import train_chunks as TC
    after = []
    for c in (1, 1000):
        gen = torch.Generator()
        gen.manual_seed(9)
        TC.draw_runs(torch.full((100,), c, dtype=torch.int64), gen)
        after.append(torch.rand(4, generator=gen))
    assert torch.equal(after[0], after[1])
    gen = torch.Generator()
    gen.manual_seed(9)
    torch.empty((100, 2), dtype=torch.float64).exponential_(1.0, generator=gen)
    torch.rand((100, 2), dtype=torch.float64, generator=gen)
    torch.rand((100, 2), dtype=torch.float64, generator=gen)
    assert torch.equal(torch.rand(4, generator=gen), after[0])


def test_draw_runs_distribution_at_five_rows():
    """200,000 draws at c = 5: n = m with probability e^-(m-1) - e^-m (the floor of the
    exponential) plus e^-5 / 5 (the uniform redraw of a length that passed c); given n = 3
    the start is 0, 1 or 2 with probability 1/3 each.  Every observed frequency within six
    binomial standard errors of the exact value."""
    import torch
    from kf2vecfsw_amd import train_chunks as TC
    gen = torch.Generator()
    gen.manual_seed(20250)
    D = 200_000
    lo, n = TC.draw_runs(torch.full((D // 2,), 5, dtype=torch.int64), gen)
    lo, n = lo.reshape(-1).numpy(), n.reshape(-1).numpy()
    assert n.size == D
    for m in range(1, 6):
        p = math.exp(-(m - 1)) - math.exp(-m) + math.exp(-5) / 5
        f = float((n == m).mean())
        print("n = {}: {:.5f} observed, {:.5f} exact".format(m, f, p))
        assert abs(f - p) <= 6 * math.sqrt(p * (1 - p) / D), (m, f, p)
    at = lo[n == 3]
    assert set(at.tolist()) == {0, 1, 2}
    for s in range(3):
        f = float((at == s).mean())
        print("lo = {} given n = 3: {:.5f} observed of {}".format(s, f, at.size))
        assert abs(f - 1 / 3) <= 6 * math.sqrt((1 / 3) * (2 / 3) / at.size), (s, f)


def test_slab_plan_keeps_whole_batches_under_the_budget():
    from kf2vecfsw_amd import train as TR
    from kf2vecfsw_amd import train_chunks as TC
    plan = TR.batch_plan(9, 2)                                      # 2, 2, 2, 2, 1 genomes: 4, 4, 4, 4, 2 rows
    assert TC.slab_plan(plan, 10, 10 ** 9) == [(0, 5)]
    assert TC.slab_plan(plan, 10, 80) == [(0, 2), (2, 4), (4, 5)]   # 8 rows of 10 bytes each
    assert TC.slab_plan(plan, 10, 1) == [(i, i + 1) for i in range(5)]   # a batch alone passes: one at least
    assert TC.slab_plan([], 10, 80) == []


# ---------------------------------------------------------------- the consecutive best
def deque_and_nanmean(losses, stop_epochs):
    """train_model_set_chunks.py:366-374 and :471-478."""
    consec_lowest_loss, consec_best_epoch = math.inf, -1
    lq = deque([float("nan")] * stop_epochs, maxlen=stop_epochs)
    for epoch, train_loss in enumerate(losses):
        lq.appendleft(train_loss)
        with np.errstate(all="ignore"):
            import warnings
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)
                lq_mean = np.nanmean(lq)
        if lq_mean < consec_lowest_loss:
            consec_lowest_loss = lq_mean
            consec_best_epoch = epoch
    return consec_best_epoch, consec_lowest_loss


def test_consecutive_best_against_a_deque_and_nanmean():
    from kf2vecfsw_amd import train_chunks as TC
    rng = np.random.default_rng(3)
    nan = float("nan")
    cases = [([5.0, 4.0, nan, 3.0, 6.0, 1.0], 2), ([nan, nan, nan], 2), ([], 3), ([1.0], 1), ([3.0, 2.0, 1.0], 5),
             ([0.1, 0.3, 0.2, 0.25, 0.05, 0.4], 3)]
    for _ in range(20):
        v = rng.uniform(0.01, 1.0, size=int(rng.integers(1, 40))).tolist()
        if rng.random() < 0.5:
            v[int(rng.integers(0, len(v)))] = nan
        cases.append((v, int(rng.integers(1, 12))))
    for losses, stop in cases:
        want, got = deque_and_nanmean(losses, stop), TC.consecutive_best(losses, stop)
        assert got[0] == want[0], (losses, stop)
        assert np.float64(got[1]).tobytes() == np.float64(want[1]).tobytes(), (losses, stop)
    assert TC.consecutive_best([5.0, 4.0, nan, 3.0, 6.0, 1.0], 2) == (3, 3.0)
    assert TC.consecutive_best([nan, nan], 2) == (-1, math.inf)
    # train_model_set_chunks.py:373
    assert TC.stopping_epochs(850, 16) == int(math.ceil(850 / 16 * 2)) == 107 and TC.stopping_epochs(3, 16) == 1


def test_epoch_lines():
    from kf2vecfsw_amd import train_chunks as TC
    plan = [(0, 4), (4, 8), (8, 9)]
    assert TC.epoch_lines(5, 9, plan, [0.5, 0.1, 0.3]) == []             # epoch > 5 from 0: not yet
    assert TC.epoch_lines(6, 9, plan, [0.5, float("nan"), 0.3]) == [
        "Epoch [7/9], Step [1/3], Outlier: {:.20f} batch size: 8".format(0.5), "Loss: nan",
        "Epoch [7/9], Step [3/3], Outlier: {:.20f} batch size: 2".format(0.3)]
    assert TC.epoch_lines(0, 9, plan, [0.5, float("nan"), 0.3]) == ["Loss: nan"]
