"""GPU tests of the chunk trainer's provider (train_chunks.epoch_batches): an
epoch's batches against chunks.range_features_host of the runs that draw_runs
gives on an equally seeded generator, rounded to float32, bit for bit -- with
and without the cap of 255 on a store whose counts pass it, under a budget that
cuts the epoch into three slabs with a short last one, with a genome of exactly
one window and a window row of all zeros; and counter.chunk_features handing
its status word back unread."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K, NBINS = 3, 32
SEED = 77
BATCH = 2
WINDOWS = [5, 1, 12, 3, 2, 7, 1, 4, 9, 2, 6, 3, 8]            # per genome of the store; two genomes of one window


@pytest.fixture(scope="module")
def dev(native):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu tests need an MI355X")
    return torch.device("cuda:0")


def host_rows():
    """uint16 window rows per genome: counts up to 2,000, a row of all zeros in genome 2 and
    genome 6's only window all zeros."""
    rng = np.random.default_rng(11)
    rows = [rng.integers(0, 2000, size=(w, NBINS)).astype(np.uint16) for w in WINDOWS]
    rows[2][4] = 0
    rows[6][0] = 0
    return rows


@pytest.fixture(scope="module")
def store(dev):
    from kf2vecfsw_amd import chunks as CH
    return CH.ChunkStore.from_host(host_rows(), ["g{}".format(i) for i in range(len(WINDOWS))], K, dev)


# the training items: eleven of the store's thirteen genomes, in an order of their own
ROWS = np.array([12, 0, 6, 3, 9, 1, 2, 10, 5, 8, 4], dtype=np.int64)


def epoch(dev, store, cap, budget=None, status=None, seed=SEED):
    """[(Z, labels)] on the host, and what the host statement gives for the same draws."""
    import torch
    from kf2vecfsw_amd import chunks as CH
    from kf2vecfsw_amd import train as TR
    from kf2vecfsw_amd import train_chunks as TC
    rows = torch.from_numpy(ROWS).to(dev)
    plan = TR.batch_plan(len(ROWS), BATCH)
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    perm = torch.randperm(len(ROWS), generator=gen, device=dev)
    kw = {} if budget is None else {"budget": budget}
    got = [(z.cpu().numpy().copy(), l.cpu().numpy().copy())
           for z, l in TC.epoch_batches(store, rows, perm, plan, gen, 1e4, cap, status=status, **kw)]
    # the same draws on a generator of its own
    gen2 = torch.Generator(device=dev)
    gen2.manual_seed(seed)
    perm2 = torch.randperm(len(ROWS), generator=gen2, device=dev).cpu().numpy()
    assert np.array_equal(perm2, perm.cpu().numpy())
    items = ROWS[perm2]
    c = np.diff(store.row0)[items]
    lo, n = TC.draw_runs(torch.from_numpy(c).to(dev), gen2)
    lo, n = lo.cpu().numpy() + store.row0[items][:, None], n.cpu().numpy()
    want = CH.range_features_host(np.concatenate(host_rows()), lo.reshape(-1), n.reshape(-1), 1e4, cap).astype(np.float32)
    return got, plan, items, want, (lo, n)


@pytest.mark.parametrize("cap", [None, 255])
def test_batches_equal_the_host_statement_of_the_drawn_runs(dev, store, cap):
    got, plan, items, want, (lo, n) = epoch(dev, store, cap)
    assert len(got) == len(plan) == 6 and plan[-1] == (10, 11)                 # the last batch: one genome, two rows
    for (z, labels), (a, b) in zip(got, plan):
        assert z.dtype == np.float32 and z.shape == (2 * (b - a), NBINS) and labels.dtype == np.int64
        assert np.array_equal(labels, items[a:b])
        assert np.array_equal(z.view(np.uint32), want[2 * a: 2 * b].view(np.uint32)), (a, b)
    # the planted rows were drawn from: a genome of one window gives two equal views; genome 6's are zero
    at = {int(g): i for i, g in enumerate(items)}
    assert np.array_equal(want[2 * at[1]], want[2 * at[1] + 1]) and want[2 * at[1]].any()
    assert not want[2 * at[6]: 2 * at[6] + 2].any()
    assert (n > 1).any() and np.isfinite(want).all()


def test_the_cap_changes_the_features(dev, store):
    plain, _, _, want_plain, _ = epoch(dev, store, None)
    capped, _, _, want_capped, _ = epoch(dev, store, 255)
    assert np.concatenate(host_rows()).max() > 255
    assert not np.array_equal(want_plain, want_capped)
    assert not np.array_equal(np.concatenate([z for z, _ in plain]), np.concatenate([z for z, _ in capped]))


def test_the_bits_do_not_depend_on_the_budget(dev, store):
    from kf2vecfsw_amd import train as TR
    from kf2vecfsw_amd import train_chunks as TC
    plan = TR.batch_plan(len(ROWS), BATCH)
    budget = 2 * (2 * BATCH) * NBINS * 4                                       # two full batches of float32 rows
    assert TC.slab_plan(plan, NBINS * 4, budget) == [(0, 2), (2, 4), (4, 6)]   # three slabs, the last one a row pair short
    assert TC.slab_plan(plan, NBINS * 4, TC.FEATURE_SLAB_BYTES) == [(0, 6)]
    one, _, _, want, _ = epoch(dev, store, 255)
    for b in (budget, 1):                                                       # and a slab per batch
        cut, _, _, _, _ = epoch(dev, store, 255, budget=b)
        assert len(cut) == len(one)
        for (z1, l1), (z2, l2) in zip(one, cut):
            assert np.array_equal(z1.view(np.uint32), z2.view(np.uint32)) and np.array_equal(l1, l2)


def test_the_status_word_is_folded_not_read(dev, store):
    import torch
    from kf2vecfsw_amd import counter as C
    status = torch.zeros(1, dtype=torch.int64, device=dev)
    got, plan, _, want, _ = epoch(dev, store, None, budget=1, status=status)
    assert int(status.item()) == 0 and len(got) == len(plan)
    # chunk_features itself: check=False hands the word back; a run past the matrix sets it and writes nothing
    lo = torch.tensor([0, store.counts.shape[0] - 1], dtype=torch.int64, device=dev)
    n = torch.tensor([2, 1], dtype=torch.int64, device=dev)
    out, st = C.chunk_features(store.counts, lo, n, 1e4, None, torch.float32, check=False)
    assert st.dtype == torch.int32 and st.shape == (1,) and int(st.item()) == 0 and out.shape == (2, NBINS)
    assert torch.equal(out, C.chunk_features(store.counts, lo, n, 1e4, None, torch.float32))
    keep = torch.full((2, NBINS), -3.0, dtype=torch.float32, device=dev)
    _, st = C.chunk_features(store.counts, lo, torch.tensor([2, 2], dtype=torch.int64, device=dev), 1e4, None,
                             torch.float32, out=keep, check=False)
    assert int(st.item()) != 0 and bool((keep == -3.0).all())
