"""CPU tests of the chunk trainer hand-off: the host sampler and the numpy
statement of kf_chunk_features against the reference's dataset classes
(tests/golden/ref_chunk_dataset), and kf_chunk_features' C-ABI: the symbols, the
scratch size and every refusal of the contract in include/kf2vec_gpu.h.  Every
native call is given fake non-null addresses and must return before any HIP
call (no device here)."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

FIX = os.path.join(GOLDEN, "ref_chunk_dataset", "chunk_dataset.npz")


@pytest.fixture(scope="module")
def fixture():
    f = np.load(FIX)
    counts = [f["counts_%d" % g] for g in range(5)]
    return dict(counts=counts, row0=np.cumsum([0] + [c.shape[0] for c in counts]), rows=np.concatenate(counts),
                seed=int(f["seed"]), idx=f["idx"], scaler=float(f["scaler"]),
                runs={(kind, cap): (f["Z_%s%s" % (kind, "_cap" if cap else "")], f["y_%s%s" % (kind, "_cap" if cap else "")])
                      for kind in ("frame", "numpy") for cap in (None, 255)})


def test_fixture_is_what_the_issue_asks(fixture):
    assert [c.shape for c in fixture["counts"]] == [(1, 32), (3, 32), (5, 32), (7, 32), (40, 32)]
    assert all(c.dtype == np.uint16 for c in fixture["counts"])
    assert not fixture["counts"][1].any() and not fixture["counts"][2][3].any()
    assert fixture["rows"].max() > 255 and fixture["idx"].size >= 200 and fixture["scaler"] == 1e4
    assert set(fixture["idx"].tolist()) == set(range(5))


@pytest.mark.parametrize("kind", ["frame", "numpy"])
@pytest.mark.parametrize("cap", [None, 255])
def test_sampler_and_statement_reproduce_the_reference(fixture, kind, cap):
    from kf2vecfsw_amd import chunks as CH
    Z, y = fixture["runs"][(kind, cap)]
    idx, row0 = fixture["idx"], fixture["row0"]
    lo, n = CH.draw_ranges(row0[idx + 1] - row0[idx], np.random.RandomState(fixture["seed"]))
    assert lo.shape == n.shape == (idx.size, 2) and lo.dtype == n.dtype == np.int64
    got = CH.range_features_host(fixture["rows"], (lo + row0[idx][:, None]).reshape(-1), n.reshape(-1),
                                 fixture["scaler"], cap).reshape(idx.size, -1)
    assert got.dtype == np.float64 and got.shape == Z.shape
    assert np.array_equal(got.view(np.uint64), Z.view(np.uint64))
    assert np.array_equal(y, idx)
    assert not np.isnan(got).any()


def test_draws_from_the_numpy_module_like_the_reference(fixture):
    """`rng` may be numpy.random itself, seeded as the reference's trainer seeds it."""
    from kf2vecfsw_amd import chunks as CH
    c = fixture["row0"][fixture["idx"] + 1] - fixture["row0"][fixture["idx"]]
    state = np.random.get_state()
    try:
        np.random.seed(fixture["seed"])
        a = CH.draw_ranges(c, np.random)
    finally:
        np.random.set_state(state)
    b = CH.draw_ranges(c, np.random.RandomState(fixture["seed"]))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_draw_ranges_bounds():
    from kf2vecfsw_amd import chunks as CH
    rs = np.random.RandomState(7)
    lo, n = CH.draw_ranges(np.ones(50, np.int64), rs)
    assert (lo == 0).all() and (n == 1).all()
    c = np.asarray([1, 2, 3, 5, 7, 40, 500] * 60)
    lo, n = CH.draw_ranges(c, rs)
    assert (n >= 1).all() and (lo >= 0).all() and (lo + n <= c[:, None]).all()
    lo3, n3 = CH.draw_ranges(c[:5], rs, views=3)
    assert lo3.shape == n3.shape == (5, 3)
    with pytest.raises(ValueError):
        CH.draw_ranges([3, 0], rs)


def test_statement_zero_total_and_cap():
    from kf2vecfsw_amd import chunks as CH
    rows = np.asarray([[0, 0, 0, 0], [1, 300, 0, 3], [65535, 2, 0, 1]], np.uint16)
    z = CH.range_features_host(rows, [0, 0, 1, 1], [0, 1, 2, 2], 2.0, None)
    assert z[:2].view(np.uint64).max() == 0           # no rows, all zeros: +0.0
    tot = 1 + 300 + 3 + 65535 + 2 + 1
    assert np.array_equal(z[2], np.asarray([65536, 302, 0, 4], np.float64) / np.float64(tot) * 2.0)
    zc = CH.range_features_host(rows, [1], [2], 1.0, 255)
    assert np.array_equal(zc[0], np.asarray([256, 257, 0, 4], np.float64) / np.float64(517))
    assert CH.range_features_host(rows, [1], [2], 1.0, 0).view(np.uint64).max() == 0


# ---------------------------------------------------------------- the C-ABI
def fake(i, off=0):
    """A fake device address, aligned to 4 KiB plus `off`."""
    return (0x7000_0000_0000 + (i << 32)) + off


def call(L, **kw):
    a = dict(counts=fake(1), cb=2, n_rows=300, nbins=8192, lo=fake(2), n=fake(3), ns=64, cap=0xFFFFFFFF, scaler=1e4,
             out=fake(4), ob=4, st=fake(5), work=fake(6), work_bytes=None, stream=None)
    a.update(kw)
    if a["work_bytes"] is None:
        a["work_bytes"] = L.kf_chunk_features_scratch_bytes(a["ns"])
    return L.kf_chunk_features(a["counts"], a["cb"], a["n_rows"], a["nbins"], a["lo"], a["n"], a["ns"], a["cap"],
                               a["scaler"], a["out"], a["ob"], a["st"], a["work"], a["work_bytes"], a["stream"])


def test_chunk_features_symbols_exported(native):
    from kf2vecfsw_amd import _native as N
    for s in ("kf_chunk_features_scratch_bytes", "kf_chunk_features"):
        assert hasattr(native, s) and s in N.SIGNATURES, s
    assert native.kf_abi_version() == 1


def test_chunk_features_scratch_bytes(native):
    f = native.kf_chunk_features_scratch_bytes
    sizes = [0, 1, 2, 63, 64, 65, 4096, 1 << 20, (1 << 31) - 1]
    got = [f(n) for n in sizes]
    assert all(x > 0 and x % 8 == 0 for x in got)
    assert got == sorted(got)
    assert got[-1] >= 8 * sizes[-1]          # a u64 total per sample


REFUSALS = [
    ("count_bytes 1", dict(cb=1), b"count_bytes"),
    ("count_bytes 8", dict(cb=8), b"count_bytes"),
    ("out_bytes 2", dict(ob=2), b"out_bytes"),
    ("out_bytes 16", dict(ob=16), b"out_bytes"),
    ("nbins 0", dict(nbins=0), b"nbins"),
    ("negative n_samples", dict(ns=-1, work_bytes=1 << 20), b"negative sample count"),
    ("scaler nan", dict(scaler=float("nan")), b"scaler"),
    ("scaler inf", dict(scaler=float("inf")), b"scaler"),
    ("scaler -inf", dict(scaler=float("-inf")), b"scaler"),
    ("null counts with rows", dict(counts=None), b"null d_counts"),
    ("null lo", dict(lo=None), b"null sample table"),
    ("null n", dict(n=None), b"null sample table"),
    ("null out", dict(out=None), b"null d_out"),
    ("null status", dict(st=None), b"null d_status"),
    ("null work", dict(work=None), b"null d_work"),
    ("u16 counts off by 1", dict(counts=fake(1, 1)), b"misaligned d_counts"),
    ("u32 counts off by 2", dict(cb=4, counts=fake(1, 2)), b"misaligned d_counts"),
    ("lo off by 4", dict(lo=fake(2, 4)), b"misaligned sample table"),
    ("n off by 4", dict(n=fake(3, 4)), b"misaligned sample table"),
    ("work off by 4", dict(work=fake(6, 4)), b"misaligned d_work"),
    ("f32 out off by 2", dict(out=fake(4, 2)), b"misaligned d_out"),
    ("f64 out off by 4", dict(ob=8, out=fake(4, 4)), b"misaligned d_out"),
    ("status off by 2", dict(st=fake(5, 2)), b"misaligned d_status"),
]


@pytest.mark.parametrize("what,kw,word", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_chunk_features_refuses(native, what, kw, word):
    from kf2vecfsw_amd import _native as N
    assert call(native, **kw) == N.KF_EINVAL, what
    msg = native.kf_last_error()
    assert msg.startswith(b"kf_chunk_features: ") and word in msg, (what, msg)


def test_chunk_features_refusals_have_their_own_messages(native):
    """One message per kind of refusal: a caller can tell them apart."""
    seen = {}
    for what, kw, word in REFUSALS:
        call(native, **kw)
        seen[word] = native.kf_last_error()
    assert len(set(seen.values())) == len(seen) >= 13


def test_chunk_features_scratch_one_byte_short(native):
    from kf2vecfsw_amd import _native as N
    need = native.kf_chunk_features_scratch_bytes(64)
    assert call(native, work_bytes=need - 1) == N.KF_ERANGE
    assert b"scratch needs %d bytes" % need in native.kf_last_error()
    # these pass every argument check, so they are asked with a scratch one byte short and end there:
    # null counts with no rows, u16 counts 2-byte aligned, float32 out 4-byte aligned, both cap extremes
    assert call(native, counts=None, n_rows=0, work_bytes=need - 1) == N.KF_ERANGE
    assert call(native, counts=fake(1, 2), out=fake(4, 4), work_bytes=need - 1) == N.KF_ERANGE
    assert call(native, cb=4, ob=8, cap=0, scaler=-2.5, nbins=10, work_bytes=need - 1) == N.KF_ERANGE


def test_chunk_store_from_host_refuses_other_widths(native):
    from kf2vecfsw_amd import chunks as CH
    from kf2vecfsw_amd.counter import num_bins
    assert num_bins(3) == 32
    with pytest.raises(ValueError, match="k=3"):
        CH.ChunkStore.from_host([np.zeros((4, 31), np.uint16)], ["a"], 3, "cpu")
    with pytest.raises(ValueError, match="k=4"):
        CH.ChunkStore.from_host([np.zeros((4, 32), np.uint16)], ["a"], 4, "cpu")
    with pytest.raises(ValueError, match="uint16"):
        CH.ChunkStore.from_host([np.zeros((4, 32), np.int32)], ["a"], 3, "cpu")
    with pytest.raises(ValueError, match="sample names"):
        CH.ChunkStore.from_host([np.zeros((4, 32), np.uint16)], ["a", "b"], 3, "cpu")
    st = CH.ChunkStore.from_host([np.zeros((4, 32), np.uint16), np.ones((2, 32), np.uint16)], ["a", "b"], 3, "cpu")
    assert st.row0.tolist() == [0, 4, 6] and st.counts.shape == (6, 32) and st.counts.dtype.is_signed
    assert st.samples == ["a", "b"] and st.excluded == {} and st.k == 3
