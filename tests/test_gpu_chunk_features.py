"""GPU tests of the chunk trainer hand-off: kf_chunk_features against its numpy
statement (chunks.range_features_host) bit for bit, in float32 and float64, on
every path of the kernel (scalar and 16-byte loads, u16 and u32 rows, one launch
up to 8192 columns and two launches past it); the device's table check; the
reference's dataset fixture through ChunkStore.batch; chunk_store against the
get_chunks CLI."""
import os

import numpy as np
import pytest

import gen
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0


@pytest.fixture(scope="module")
def dev(native):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu tests need an MI355X")
    return torch.device("cuda:0")


def to_dev(rows, dev):
    """uint16 / uint32 rows as the int16 / int32 tensor the wrapper takes."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(rows).view(np.int16 if rows.dtype == np.uint16 else np.int32)).to(dev)


def bits(a):
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def check(counts_dev, rows, lo, n, scaler, cap, what=""):
    """chunk_features == range_features_host bit for bit, float64 and float32."""
    import torch
    from kf2vecfsw_amd import chunks as CH
    from kf2vecfsw_amd import counter as C
    ref = CH.range_features_host(rows, lo, n, scaler, cap)
    for dt, r in ((torch.float64, ref), (torch.float32, ref.astype(np.float32))):
        got = C.chunk_features(counts_dev, lo, n, scaler, cap, dt).cpu().numpy()
        assert got.dtype == r.dtype and got.shape == r.shape, what
        assert np.array_equal(bits(got), bits(r)), (what, dt, cap)
    return ref


def sample_table(rng, n_rows, ns=64):
    """64 samples with the edges: empty at both ends, single rows, all rows, twins, overlaps."""
    q = n_rows // 4
    fixed = [(0, 0), (n_rows, 0), (5, 1), (n_rows - 1, 1), (0, n_rows), (q, q), (q, q), (q + 2, 2 * q), (q + 3, 2 * q),
             (0, 1), (n_rows - 7, 7)]
    lo = rng.integers(0, n_rows, size=ns)
    n = np.minimum(rng.integers(0, n_rows // 2, size=ns), n_rows - lo)
    for i, (a, b) in enumerate(fixed):
        lo[i], n[i] = a, b
    return lo.astype(np.int64), n.astype(np.int64)


@pytest.mark.parametrize("nbins", [10, 32, 136, 2080, 8192, 32896])
def test_shapes_caps_and_dtypes(dev, nbins):
    rng = np.random.default_rng(1000 + nbins)
    n_rows = 40 if nbins == 32896 else 300
    rows = rng.integers(0, 1 << 16, size=(n_rows, nbins)).astype(np.uint16)
    rows[rng.random(rows.shape) < 0.02] = 0xFFFF
    rows[rng.random(rows.shape) < 0.3] = 0
    lo, n = sample_table(rng, n_rows)
    d = to_dev(rows, dev)
    for cap in (None, 255, 0):
        ref = check(d, rows, lo, n, 1e4, cap, nbins)
        assert not np.isnan(ref).any() and (bits(ref[:2]) == 0).all()
        assert np.array_equal(bits(ref[5]), bits(ref[6]))
    # device int64 tables give the same
    import torch
    from kf2vecfsw_amd import chunks as CH
    from kf2vecfsw_amd import counter as C
    got = C.chunk_features(d, torch.from_numpy(lo).to(dev), torch.from_numpy(n).to(dev), 1.0, None, torch.float64)
    assert np.array_equal(bits(got.cpu().numpy()), bits(CH.range_features_host(rows, lo, n, 1.0, None)))


@pytest.mark.parametrize("nbins,n_rows,ns", [(32, 300, 5000), (32896, 40, 450)])
def test_more_items_than_workgroups(dev, nbins, n_rows, ns):
    """A launch has at most 2,048 workgroups: with 5,000 samples (one launch) and
    with 450 samples x 5 column tiles (two launches) every workgroup takes several
    (sample, tile) items in turn."""
    rng = np.random.default_rng(ns)
    rows = rng.integers(0, 1 << 16, size=(n_rows, nbins)).astype(np.uint16)
    lo, n = sample_table(rng, n_rows, ns)
    check(to_dev(rows, dev), rows, lo, n, 1e4, 255 if nbins == 32 else None, nbins)


@pytest.mark.parametrize("nbins", [10, 32])
def test_u16_sums_past_2_32(dev, nbins):
    """65,538 rows of 0xFFFF: a column sums to 4,295,032,830, past a 32-bit accumulator."""
    rows = np.full((65538, nbins), 0xFFFF, np.uint16)
    assert int(rows[:, 0].astype(np.uint64).sum()) == 4295032830
    rows[7, 1] = 3                                  # not every column alike
    ref = check(to_dev(rows, dev), rows, [0, 1], [65538, 65536], 1e4, None, nbins)
    assert ref[0, 0] == 4295032830 / (4295032830 * nbins - 65532) * 1e4


@pytest.mark.parametrize("nbins", [10, 32])
def test_u32_rows(dev, nbins):
    """u32 rows (a kf_count_batch matrix) near 2^32 - 1: column sums need 64 bits."""
    rng = np.random.default_rng(77)
    rows = ((1 << 32) - 1 - rng.integers(0, 3, size=(5, nbins))).astype(np.uint32)
    rows[2, 3] = 0
    rows[4] = rng.integers(0, 1000, size=nbins)
    lo, n = [0, 0, 1, 4, 5, 2], [5, 4, 3, 1, 0, 1]
    d = to_dev(rows, dev)
    for cap in (None, 255, 0, (1 << 32) - 2):
        check(d, rows, lo, n, 1e4, cap, nbins)
    check(d, rows, lo[:4], n[:4], -0.75, None, nbins)   # (no empty sample: the statement's 0 * scaler is -0.0)


@pytest.mark.parametrize("nbins", [10, 32, 32896])
def test_zero_total_is_plus_zero(dev, nbins):
    import torch
    from kf2vecfsw_amd import counter as C
    rng = np.random.default_rng(5)
    zeros = np.zeros((12, nbins), np.uint16)
    some = rng.integers(1, 500, size=(12, nbins)).astype(np.uint16)
    for rows, cap in ((zeros, None), (some, 0)):
        for dt in (torch.float32, torch.float64):
            out = torch.full((3, nbins), float("nan"), dtype=dt, device=dev)
            C.chunk_features(to_dev(rows, dev), [0, 3, 12], [12, 4, 0], 1e4, cap, dt, out=out)
            assert (bits(out.cpu().numpy()) == 0).all()


def raw_status(counts, lo, n, out):
    """kf_chunk_features called directly: (return code, status word)."""
    import torch
    from kf2vecfsw_amd import _native as N
    dev = counts.device
    t = torch.zeros((2, max(lo.size, 1)), dtype=torch.int64, device=dev)
    t[:, :lo.size] = torch.from_numpy(np.stack([lo, n]).view(np.int64))
    status = torch.full((1,), 77, dtype=torch.int32, device=dev)
    need = N.lib().kf_chunk_features_scratch_bytes(lo.size)
    work = torch.empty(need // 8, dtype=torch.int64, device=dev)
    rc = N.lib().kf_chunk_features(counts.data_ptr(), counts.element_size(), counts.shape[0], counts.shape[1],
                                   t[0].data_ptr(), t[1].data_ptr(), lo.size, 0xFFFFFFFF, 1.0, out.data_ptr(),
                                   out.element_size(), status.data_ptr(), work.data_ptr(), need,
                                   torch.cuda.current_stream(dev).cuda_stream)
    return rc, int(status.item())


@pytest.mark.parametrize("nbins", [10, 32, 32896])
@pytest.mark.parametrize("bad", ["one past the end", "wraps"])
def test_bad_table_writes_nothing(dev, nbins, bad):
    import torch
    from kf2vecfsw_amd import _native as N
    from kf2vecfsw_amd import counter as C
    rng = np.random.default_rng(9)
    n_rows = 40
    rows = rng.integers(0, 500, size=(n_rows, nbins)).astype(np.uint16)
    lo, n = sample_table(rng, n_rows)
    lo, n = lo.astype(np.uint64), n.astype(np.uint64)
    lo[-1], n[-1] = ((n_rows - 3, 4) if bad == "one past the end" else (1 << 63, 1 << 63))
    d = to_dev(rows, dev)
    for dt in (torch.float32, torch.float64):
        out = torch.full((64, nbins), SENTINEL, dtype=dt, device=dev)
        with pytest.raises(N.NativeError, match="kf_chunk_features"):
            C.chunk_features(d, lo, n, 1e4, None, dt, out=out)
        assert bool((out == SENTINEL).all())
        assert raw_status(d, lo, n, out) == (0, 2)
        assert bool((out == SENTINEL).all())
    lo[-1], n[-1] = n_rows - 3, 3                    # the same table made good: status 0 and every row written
    out = torch.full((64, nbins), SENTINEL, dtype=torch.float32, device=dev)
    assert raw_status(d, lo, n, out) == (0, 0)
    assert not bool((out == SENTINEL).any())


def test_no_samples_writes_status_only(dev):
    import torch
    from kf2vecfsw_amd import counter as C
    d = to_dev(np.ones((4, 32), np.uint16), dev)
    out = torch.full((1, 32), SENTINEL, device=dev)
    assert raw_status(d, np.zeros(0, np.uint64), np.zeros(0, np.uint64), out) == (0, 0)
    assert bool((out == SENTINEL).all())
    assert C.chunk_features(d, [], [], 1.0).shape == (0, 32)


@pytest.mark.parametrize("nbins", [10, 8192])
def test_nothing_outside_the_output(dev, nbins):
    import torch
    from kf2vecfsw_amd import chunks as CH
    from kf2vecfsw_amd import counter as C
    rng = np.random.default_rng(31)
    rows = rng.integers(0, 3000, size=(300, nbins)).astype(np.uint16)
    lo, n = sample_table(rng, 300)
    ref = CH.range_features_host(rows, lo, n, 1e4, None)
    d = to_dev(rows, dev)
    for dt, r in ((torch.float32, ref.astype(np.float32)), (torch.float64, ref)):
        buf = torch.full((66, nbins), SENTINEL, dtype=dt, device=dev)
        C.chunk_features(d, lo, n, 1e4, None, dt, out=buf[1:65])
        host = buf.cpu().numpy()
        assert (host[0] == SENTINEL).all() and (host[65] == SENTINEL).all()
        assert np.array_equal(bits(host[1:65]), bits(r))


@pytest.fixture(scope="module")
def fixture():
    f = np.load(os.path.join(GOLDEN, "ref_chunk_dataset", "chunk_dataset.npz"))
    return dict(counts=[f["counts_%d" % g] for g in range(5)], seed=int(f["seed"]), idx=f["idx"],
                scaler=float(f["scaler"]), Z={None: f["Z_frame"], 255: f["Z_frame_cap"]},
                Zn={None: f["Z_numpy"], 255: f["Z_numpy_cap"]})


@pytest.mark.parametrize("cap", [None, 255])
@pytest.mark.parametrize("per_batch", [None, 7])
def test_reference_dataset_through_the_device(dev, fixture, cap, per_batch):
    """ChunkStore.batch over the fixture's item sequence == the reference's
    Dataset_chunks_2rows items (both classes), float64 bit for bit and float32 as
    the trainer's `images.float()` makes them."""
    import torch
    from kf2vecfsw_amd import chunks as CH
    store = CH.ChunkStore.from_host(fixture["counts"], ["g%d" % g for g in range(5)], 3, dev)
    idx, Z = fixture["idx"], fixture["Z"][cap]
    assert np.array_equal(bits(Z), bits(fixture["Zn"][cap]))
    step = per_batch or idx.size
    for dt, exp in ((torch.float64, Z), (torch.float32, Z.astype(np.float32))):
        rs = np.random.RandomState(fixture["seed"])
        zs, ys = [], []
        for a in range(0, idx.size, step):
            z, y = store.batch(idx[a: a + step], rs, fixture["scaler"], cap, dt)
            assert z.shape == (min(step, idx.size - a), 64) and z.dtype == dt and y.dtype == torch.int64
            zs.append(z.cpu().numpy())
            ys.append(y.cpu().numpy())
        assert np.array_equal(bits(np.concatenate(zs)), bits(exp))
        assert np.array_equal(np.concatenate(ys), idx)


def _fasta(rng, contigs):
    return b"".join(b">ctg%d len %d\n" % (i, L) + gen.wrap(gen.random_seq(rng, L), 60)
                    for i, L in enumerate(contigs))


def test_chunk_store_equals_the_cli(dev, tmp_path, monkeypatch):
    """chunk_store == get_chunks -k 7 + parsing the .kf files: the genomes in input
    order, the last file of a shared sample name standing, the excluded absent."""
    from kf2vecfsw_amd import chunks as CH
    from kf2vecfsw_amd import main as M
    rng = np.random.default_rng(6060)
    files = {"g0.fna": [61000, 24000, 3000], "g1.fasta": [15000, 15000, 10001, 30000, 9999],
             "few.fna": [30000, 3000], "none.fna": [9999, 9000, 8000, 5000],
             "x.fna": [40000, 20000], "x.fa": [50000, 30000, 12000]}
    inp, out = tmp_path / "in", tmp_path / "out"
    inp.mkdir()
    out.mkdir()
    for name, contigs in files.items():
        (inp / name).write_bytes(_fasta(rng, contigs))
    M.main(["get_chunks", "-input_dir", str(inp), "-output_dir", str(out), "-k", "7"])
    assert sorted(f for f in os.listdir(out) if f.endswith(".kf")) == ["g0.kf", "g1.kf", "x.kf"]

    def parse(path):
        # (raw counts print as floats when a bin is empty: "3.0")
        rows = [ln.split(",")[1:] for ln in open(path).read().splitlines()]
        return np.asarray(rows).astype(np.float64).astype(np.uint16)
    # the order of the files that stand: a sample's place is its last file's
    names, samples = M.list_inputs(str(inp))
    order = [s for i, s in enumerate(samples) if s in ("g0", "g1", "x") and s not in samples[i + 1:]]
    exp = [parse(out / (s + ".kf")) for s in order]
    last_x = [f for f in names if f.startswith("x.")][-1]

    def windows(contigs):
        return sum(CH.window_plan(L)[0] for L in contigs if L >= CH.CHUNK_SZ)
    assert windows(files["x.fna"]) != windows(files["x.fa"])
    assert exp[order.index("x")].shape[0] == windows(files[last_x])
    for batch_gb in (1.0, 5 * 4 * 8192 / (1 << 30)):    # the second: 5 windows per count launch, a file per batch
        st = CH.chunk_store(str(inp), 7, dev, batch_gb=batch_gb)
        assert st.samples == order and st.k == 7
        assert st.excluded == {"few": "few", "none": "none"}
        assert st.row0.tolist() == np.cumsum([0] + [e.shape[0] for e in exp]).tolist()
        assert st.counts.dtype.is_signed and st.counts.shape == (st.row0[-1], 8192)
        assert np.array_equal(st.counts.cpu().numpy().view(np.uint16), np.concatenate(exp))
    # a file above SPLIT_BYTES is refused before anything is counted
    monkeypatch.setattr(M, "SPLIT_BYTES", 70000)

    def no_pipeline(*a, **kw):
        raise AssertionError("the pipeline was built before the refusal")
    monkeypatch.setattr(CH, "ChunkPipeline", no_pipeline)
    with pytest.raises(ValueError, match=r"g0\.fna"):
        CH.chunk_store(str(inp), 7, dev)
