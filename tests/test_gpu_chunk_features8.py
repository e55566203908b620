"""GPU tests of the uint8 window store: kf_chunk_features8 against the numpy
statement (chunks.range_features_host on the uint8 rows) and against
kf_chunk_features with cap = 255 on the uint16 rows the uint8 rows were capped
from, bit for bit, in float32 and float64, on every path of the kernel (16-byte
loads and scalar, one launch up to 8192 columns and two past it, the rounds of
R = 8 rows in flight, the fold of the 16-bit partial sums every 256 rows); the
device's table check; the bounds of the output and the scratch; kf_rows_cap8;
chunk_store_from_kf(cap8=True); train_chunks.epoch_batches on both stores."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
R = 8            # rows in flight per thread on the uint8 vector path (Shape<1, true>::R in csrc/kf_chunkfeat.hip)
FOLD = 256       # rows between two folds of its 16-bit partial sums (kCFold8)
NBINS = [32, 136, 2080, 8192, 32896]


@pytest.fixture(scope="module")
def dev(native):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu tests need an MI355X")
    return torch.device("cuda:0")


def bits(a):
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def dev16(rows, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(rows).view(np.int16)).to(dev)


def dev8(rows8, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(rows8)).to(dev)


def some_rows(rng, n_rows, nbins):
    """uint16 rows with counts on both sides of 255, and their uint8 cap."""
    rows = rng.integers(0, 600, size=(n_rows, nbins)).astype(np.uint16)
    rows[rng.random(rows.shape) < 0.02] = 0xFFFF
    rows[rng.random(rows.shape) < 0.3] = 0
    rows.reshape(-1)[:7] = [0, 254, 255, 256, 32767, 32768, 65535]
    return rows, np.minimum(rows, 255).astype(np.uint8)


def check(d8, d16, rows8, lo, n, scaler=1e4, what=""):
    """chunk_features on the uint8 rows == the statement on them == chunk_features(cap=255) on the uint16 rows."""
    import torch
    from kf2vecfsw_amd import chunks as CH
    from kf2vecfsw_amd import counter as C
    ref = CH.range_features_host(rows8, lo, n, scaler, None)
    for dt, r in ((torch.float64, ref), (torch.float32, ref.astype(np.float32))):
        got = C.chunk_features(d8, lo, n, scaler, None, dt).cpu().numpy()
        assert got.dtype == r.dtype and got.shape == r.shape, what
        assert np.array_equal(bits(got), bits(r)), (what, dt)
        if d16 is not None:
            wide = C.chunk_features(d16, lo, n, scaler, 255, dt).cpu().numpy()
            assert np.array_equal(bits(got), bits(wide)), (what, dt, "against kf_chunk_features(cap=255)")
    return ref


def sample_table(rng, n_rows, ns=64):
    """Samples with the edges: empty at both ends, single rows, all rows, twins, overlaps, and the
    row counts around the rounds of R rows."""
    q = n_rows // 4
    fixed = [(0, 0), (n_rows, 0), (5, 1), (n_rows - 1, 1), (0, n_rows), (q, q), (q, q), (q + 2, 2 * q), (q + 3, 2 * q),
             (0, 1), (n_rows - 7, 7), (3, R - 1), (3, R), (3, R + 1), (2, 2 * R + 1), (n_rows - R, R)]
    lo = rng.integers(0, n_rows, size=ns)
    n = np.minimum(rng.integers(0, n_rows // 2, size=ns), n_rows - lo)
    for i, (a, b) in enumerate(fixed):
        lo[i], n[i] = a, b
    return lo.astype(np.int64), n.astype(np.int64)


@pytest.mark.parametrize("nbins", NBINS)
def test_paths_shapes_and_dtypes(dev, nbins):
    rng = np.random.default_rng(8000 + nbins)
    n_rows = 40 if nbins == 32896 else 300
    rows, rows8 = some_rows(rng, n_rows, nbins)
    rows[20:26] = 0                                            # a run of all-zero rows: T == 0
    rows8[20:26] = 0
    lo, n = sample_table(rng, n_rows)
    lo[16], n[16] = 20, 6
    lo[17], n[17] = 21, 3
    d8, d16 = dev8(rows8, dev), dev16(rows, dev)
    ref = check(d8, d16, rows8, lo, n, 1e4, nbins)
    assert not np.isnan(ref).any() and (bits(ref[:2]) == 0).all() and (bits(ref[16:18]) == 0).all()
    assert np.array_equal(bits(ref[5]), bits(ref[6])) and ref[4].any()
    # cap = 255 (what the trainer passes under -cap) and above are no cap over uint8 rows; device tables give the same
    import torch
    from kf2vecfsw_amd import counter as C
    for cap in (255, 256, 0xFFFFFFFF):
        got = C.chunk_features(d8, torch.from_numpy(lo).to(dev), torch.from_numpy(n).to(dev), 1e4, cap, torch.float64)
        assert np.array_equal(bits(got.cpu().numpy()), bits(ref))
    check(d8, d16, rows8, lo[2:16], n[2:16], -0.75, nbins)     # (no empty sample: the statement's 0 * scaler is -0.0)


@pytest.mark.parametrize("nbins", [32, 136])
def test_row_counts_around_the_rows_in_flight(dev, nbins):
    rng = np.random.default_rng(88)
    rows, rows8 = some_rows(rng, 64, nbins)
    counts = [0, 1, R - 1, R, R + 1, 2 * R + 1]
    lo = np.asarray([0, 5, 9] * len(counts), dtype=np.int64)
    n = np.repeat(np.asarray(counts, dtype=np.int64), 3)
    check(dev8(rows8, dev), dev16(rows, dev), rows8, lo, n, 1e4, nbins)


@pytest.mark.parametrize("nbins", [32, 136, 8192])
def test_rows_of_255_past_a_16_bit_partial_sum(dev, nbins):
    """258 rows of 255 sum to 65,790 per column, past 16 bits: the partial sums are folded before."""
    n_rows = 2 * FOLD + 2 * R + 3
    rows8 = np.full((n_rows, nbins), 255, np.uint8)
    rows8[7, 1] = 3                                             # not every column alike
    rows8[n_rows - 1, nbins - 1] = 0
    assert 258 * 255 > 0xFFFF
    counts = [FOLD - 1, FOLD, FOLD + 1, 258, FOLD + R - 1, FOLD + R, FOLD + R + 1, 2 * FOLD, 2 * FOLD + 1, n_rows]
    lo = np.zeros(len(counts) + 1, dtype=np.int64)
    n = np.asarray(counts + [258], dtype=np.int64)
    lo[-1] = n_rows - 258
    ref = check(dev8(rows8, dev), dev16(rows8.astype(np.uint16), dev), rows8, lo, n, 1e4, nbins)
    total = 258 * 255 * nbins - 252
    assert ref[3, 0] == np.float64(258 * 255) / np.float64(total) * 1e4


@pytest.mark.parametrize("what", ["counts one byte off", "output one element off"])
@pytest.mark.parametrize("nbins", [32, 8192])
def test_misaligned_bases_take_the_scalar_path(dev, nbins, what):
    import torch
    from kf2vecfsw_amd import chunks as CH
    from kf2vecfsw_amd import counter as C
    rng = np.random.default_rng(3)
    n_rows = 300
    _, rows8 = some_rows(rng, n_rows, nbins)
    lo, n = sample_table(rng, n_rows)
    ref = CH.range_features_host(rows8, lo, n, 1e4, None)
    flat = torch.zeros(n_rows * nbins + 16, dtype=torch.uint8, device=dev)
    off = 1 if what == "counts one byte off" else 0
    d8 = flat[off: off + n_rows * nbins].view(n_rows, nbins)
    d8.copy_(torch.from_numpy(rows8))
    assert d8.data_ptr() % 16 == off and d8.is_contiguous()
    for dt, r in ((torch.float32, ref.astype(np.float32)), (torch.float64, ref)):
        buf = torch.full((64 * nbins + 16,), SENTINEL, dtype=dt, device=dev)
        o = 0 if off else 1
        out = buf[o: o + 64 * nbins].view(64, nbins)
        assert (out.data_ptr() % 16 != 0) == (not off)
        C.chunk_features(d8, lo, n, 1e4, None, dt, out=out)
        host = buf.cpu().numpy()
        assert np.array_equal(bits(host[o: o + 64 * nbins].reshape(64, nbins)), bits(r)), (what, dt)
        assert (host[:o] == SENTINEL).all() and (host[o + 64 * nbins:] == SENTINEL).all()


def raw(d8, lo, n, out, guard=4):
    """kf_chunk_features8 called directly, its scratch between guard words: (return code, status word, guards intact)."""
    import torch
    from kf2vecfsw_amd import _native as N
    dev = d8.device
    t = torch.zeros((2, max(lo.size, 1)), dtype=torch.int64, device=dev)
    t[:, :lo.size] = torch.from_numpy(np.stack([lo, n]).view(np.int64))
    status = torch.full((1,), 77, dtype=torch.int32, device=dev)
    need = N.lib().kf_chunk_features_scratch_bytes(lo.size)
    work = torch.full((need // 8 + 2 * guard,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=dev)
    rc = N.lib().kf_chunk_features8(d8.data_ptr(), d8.shape[0], d8.shape[1], t[0].data_ptr(), t[1].data_ptr(), lo.size,
                                    1e4, out.data_ptr(), out.element_size(), status.data_ptr(),
                                    work[guard:].data_ptr(), need, torch.cuda.current_stream(dev).cuda_stream)
    w = work.cpu().numpy()
    return rc, int(status.item()), bool((w[:guard] == 0x5A5A5A5A5A5A5A5A).all() and
                                        (w[guard + need // 8:] == 0x5A5A5A5A5A5A5A5A).all())


@pytest.mark.parametrize("nbins", [32, 136, 32896])
def test_bad_table_writes_nothing(dev, nbins):
    import torch
    from kf2vecfsw_amd import _native as N
    from kf2vecfsw_amd import counter as C
    rng = np.random.default_rng(9)
    n_rows = 40
    _, rows8 = some_rows(rng, n_rows, nbins)
    lo, n = sample_table(rng, n_rows)
    lo, n = lo.astype(np.uint64), n.astype(np.uint64)
    lo[-1], n[-1] = n_rows - 3, 4                               # one run past n_rows
    d8 = dev8(rows8, dev)
    for dt in (torch.float32, torch.float64):
        out = torch.full((64, nbins), SENTINEL, dtype=dt, device=dev)
        before = out.cpu().numpy().tobytes()
        with pytest.raises(N.NativeError, match="kf_chunk_features"):
            C.chunk_features(d8, lo, n, 1e4, None, dt, out=out)
        assert out.cpu().numpy().tobytes() == before
        assert raw(d8, lo, n, out) == (0, 2, True)
        assert out.cpu().numpy().tobytes() == before
    lo[-1], n[-1] = n_rows - 3, 3                               # the same table made good
    out = torch.full((64, nbins), SENTINEL, dtype=torch.float32, device=dev)
    assert raw(d8, lo, n, out) == (0, 0, True)
    assert not bool((out == SENTINEL).any())


@pytest.mark.parametrize("nbins", [32, 136, 8192, 32896])
def test_nothing_outside_the_output_and_the_scratch(dev, nbins):
    import torch
    from kf2vecfsw_amd import chunks as CH
    rng = np.random.default_rng(31)
    n_rows = 40 if nbins == 32896 else 300
    _, rows8 = some_rows(rng, n_rows, nbins)
    lo, n = sample_table(rng, n_rows)
    ref = CH.range_features_host(rows8, lo, n, 1e4, None)
    d8 = dev8(rows8, dev)
    for dt, r in ((torch.float32, ref.astype(np.float32)), (torch.float64, ref)):
        buf = torch.full((66, nbins), SENTINEL, dtype=dt, device=dev)
        assert raw(d8, lo.astype(np.uint64), n.astype(np.uint64), buf[1:65]) == (0, 0, True)
        host = buf.cpu().numpy()
        assert (host[0] == SENTINEL).all() and (host[65] == SENTINEL).all()
        assert np.array_equal(bits(host[1:65]), bits(r))


def test_no_samples_writes_status_only(dev):
    import torch
    from kf2vecfsw_amd import counter as C
    d8 = dev8(np.ones((4, 32), np.uint8), dev)
    out = torch.full((1, 32), SENTINEL, device=dev)
    assert raw(d8, np.zeros(0, np.uint64), np.zeros(0, np.uint64), out) == (0, 0, True)
    assert bool((out == SENTINEL).all())
    assert C.chunk_features(d8, [], [], 1.0).shape == (0, 32)


@pytest.mark.parametrize("nbins,n_rows,ns", [(32, 300, 5000), (32896, 40, 450)])
def test_more_items_than_workgroups(dev, nbins, n_rows, ns):
    rng = np.random.default_rng(ns)
    rows, rows8 = some_rows(rng, n_rows, nbins)
    lo, n = sample_table(rng, n_rows, ns)
    check(dev8(rows8, dev), dev16(rows, dev), rows8, lo, n, 1e4, nbins)


# ---------------------------------------------------------------- kf_rows_cap8
VALUES = [0, 254, 255, 256, 32767, 32768, 65535]


# (elements d_src lies behind a 16-byte line, bytes d_dst does): 16-byte loads and stores with no head, with a head
# of 8 and of 12 elements, and the three ways the pointers do not allow them
@pytest.mark.parametrize("src_off,dst_off", [(0, 0), (0, 8), (4, 4), (0, 3), (1, 0), (3, 5)])
@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, 4097])
def test_rows_cap8(dev, n, src_off, dst_off):
    import torch
    from kf2vecfsw_amd import _native as N
    rng = np.random.default_rng(n + 1)
    v = rng.integers(0, 1 << 16, size=n).astype(np.uint16)
    if n >= 15:
        v[rng.permutation(n)[:7]] = VALUES
        assert set(VALUES) <= set(v.tolist())
    elif n == 1:
        v[0] = 256
    src = torch.zeros(n + 16, dtype=torch.int16, device=dev)
    src[src_off: src_off + n] = torch.from_numpy(v.view(np.int16)).to(dev)
    dst = torch.full((n + 64,), 0xA5, dtype=torch.uint8, device=dev)
    s, d = src[src_off:], dst[16 + dst_off:]
    assert s.data_ptr() % 16 == 2 * src_off and d.data_ptr() % 16 == dst_off
    rc = N.lib().kf_rows_cap8(s.data_ptr(), n, d.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0
    host = dst.cpu().numpy()
    assert np.array_equal(host[16 + dst_off: 16 + dst_off + n], np.minimum(v, 255).astype(np.uint8))
    assert (host[:16 + dst_off] == 0xA5).all() and (host[16 + dst_off + n:] == 0xA5).all()


def test_rows_cap8_wrapper(dev):
    import torch
    from kf2vecfsw_amd import counter as C
    rng = np.random.default_rng(12)
    rows, rows8 = some_rows(rng, 37, 136)
    got = C.rows_cap8(dev16(rows, dev))
    assert got.dtype == torch.uint8 and got.shape == (37, 136) and np.array_equal(got.cpu().numpy(), rows8)
    assert C.rows_cap8(torch.zeros((0, 136), dtype=torch.int16, device=dev)).shape == (0, 136)


# ---------------------------------------------------------------- the store
WINDOW = 10000


@pytest.fixture(scope="module")
def kf_dir(tmp_path_factory):
    """A small get_chunks directory at k = 3, written with the project's writer: six genomes of 1 to 12
    window rows with counts above 255, and a file of no rows."""
    from kf2vecfsw_amd import chunks as CH
    root = tmp_path_factory.mktemp("cap8_store")
    rng = np.random.default_rng(77)
    rows = {}
    for nm, w in zip(["g3", "g1", "g5", "g0", "g4", "g2"], [1, 12, 5, 7, 2, 9]):
        comp = rng.dirichlet(np.full(32, 0.6))
        r = rng.multinomial(WINDOW - 2, comp, size=w).astype(np.uint16)
        rows[nm] = r
        text, _ = CH.format_rows_host(r, [nm + ".part_c.part_c_sliding__"], np.zeros(w, np.int64),
                                      np.arange(w, dtype=np.int64) * WINDOW, WINDOW, False)
        (root / (nm + ".kf")).write_bytes(text)
    (root / "empty.kf").write_bytes(b"")
    return str(root), rows


@pytest.mark.parametrize("batch_gb", [1.0, 2e-6])                # the second: a batch of a file or two
def test_chunk_store_from_kf_cap8(dev, kf_dir, batch_gb):
    import torch
    from kf2vecfsw_amd import chunks as CH
    path, rows = kf_dir
    for samples in (None, ["g3", "empty", "g1", "g5", "g0"]):
        wide = CH.chunk_store_from_kf(path, 3, dev, samples=samples, batch_gb=batch_gb)
        st = CH.chunk_store_from_kf(path, 3, dev, samples=samples, batch_gb=batch_gb, cap8=True)
        assert wide.counts.dtype == torch.int16 and st.counts.dtype == torch.uint8
        host = wide.counts.cpu().numpy().view(np.uint16)
        assert host.max() > 255 and np.array_equal(host, np.concatenate([rows[s] for s in wide.samples]))
        assert np.array_equal(st.counts.cpu().numpy(), np.minimum(host, 255).astype(np.uint8))
        assert st.counts.is_contiguous() and st.counts.shape == wide.counts.shape
        assert st.row0.tolist() == wide.row0.tolist() and st.samples == wide.samples and st.k == wide.k == 3
        assert st.excluded == wide.excluded == {"empty": "none"}
    none = CH.chunk_store_from_kf(path, 3, dev, samples=[], cap8=True)
    assert none.counts.dtype == torch.uint8 and none.counts.shape == (0, 32) and none.samples == []


@pytest.mark.parametrize("views", [1, 2])
def test_epoch_batches_on_the_two_stores(dev, kf_dir, views):
    """The uint8 store, and the uint16 store with cap = 255, under equally seeded generators: the same batches."""
    import torch
    from kf2vecfsw_amd import chunks as CH
    from kf2vecfsw_amd import train_chunks as TC
    path, _ = kf_dir
    names = ["g3", "g1", "g5", "g0", "g4", "g2"]
    wide = CH.chunk_store_from_kf(path, 3, dev, samples=names)
    st = CH.chunk_store_from_kf(path, 3, dev, samples=names, cap8=True)
    plan = [(0, 4), (4, 6)]
    got = []
    for store, cap in ((st, None), (st, 255), (wide, 255), (wide, None)):
        gen = torch.Generator(device=dev)
        gen.manual_seed(28)
        rows = torch.arange(6, dtype=torch.int64, device=dev)
        perm = torch.randperm(6, generator=gen, device=dev)
        kw = {} if views == 2 else {"views": 1}
        got.append([(z.cpu().numpy(), y.cpu().numpy()) for z, y in TC.epoch_batches(store, rows, perm, plan, gen, 1e4, cap,
                                                                                   **kw)])
    for other in got[1:3]:
        assert len(other) == len(got[0]) == 2
        for (z0, y0), (z1, y1) in zip(got[0], other):
            assert z0.dtype == np.float32 and z0.shape == (views * y0.size, 32) and np.array_equal(y0, y1)
            assert np.array_equal(bits(z0), bits(z1))
    assert not all(np.array_equal(a[0], b[0]) for a, b in zip(got[0], got[3]))        # the cap tells on these rows
