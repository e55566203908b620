"""CPU tests of the uint8 window store's native entries: kf_chunk_features8 and
kf_rows_cap8 are exported and refuse what the contract in include/kf2vec_gpu.h
says, each before any HIP call (every call is given fake non-null addresses:
there is no device here); the numpy statement on rows capped to uint8 equals
itself with cap=255 on the uint16 rows, which anchors the oracle of
test_gpu_chunk_features8.py; ChunkStore.from_host takes uint8 rows; the wrapper
refuses a cap below 255 over uint8 rows."""
import numpy as np
import pytest


def fake(i, off=0):
    """A fake device address, aligned to 4 KiB plus `off`."""
    return (0x7000_0000_0000 + (i << 32)) + off


def call(L, **kw):
    a = dict(counts=fake(1), n_rows=300, nbins=8192, lo=fake(2), n=fake(3), ns=64, scaler=1e4, out=fake(4), ob=4,
             st=fake(5), work=fake(6), work_bytes=None, stream=None)
    a.update(kw)
    if a["work_bytes"] is None:
        a["work_bytes"] = L.kf_chunk_features_scratch_bytes(a["ns"])
    return L.kf_chunk_features8(a["counts"], a["n_rows"], a["nbins"], a["lo"], a["n"], a["ns"], a["scaler"], a["out"],
                                a["ob"], a["st"], a["work"], a["work_bytes"], a["stream"])


def test_symbols_exported(native):
    from kf2vecfsw_amd import _native as N
    for s in ("kf_chunk_features8", "kf_rows_cap8"):
        assert hasattr(native, s) and s in N.SIGNATURES, s
    assert native.kf_abi_version() == 1


REFUSALS = [
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
    ("lo off by 4", dict(lo=fake(2, 4)), b"misaligned sample table"),
    ("n off by 4", dict(n=fake(3, 4)), b"misaligned sample table"),
    ("work off by 4", dict(work=fake(6, 4)), b"misaligned d_work"),
    ("f32 out off by 2", dict(out=fake(4, 2)), b"misaligned d_out"),
    ("f64 out off by 4", dict(ob=8, out=fake(4, 4)), b"misaligned d_out"),
    ("status off by 2", dict(st=fake(5, 2)), b"misaligned d_status"),
]


@pytest.mark.parametrize("what,kw,word", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_chunk_features8_refuses(native, what, kw, word):
    from kf2vecfsw_amd import _native as N
    assert call(native, **kw) == N.KF_EINVAL, what
    msg = native.kf_last_error()
    assert msg.startswith(b"kf_chunk_features8: ") and word in msg, (what, msg)


def test_chunk_features8_refusals_have_their_own_messages(native):
    seen = {}
    for what, kw, word in REFUSALS:
        call(native, **kw)
        seen[word] = native.kf_last_error()
    assert len(set(seen.values())) == len(seen) >= 11


def test_chunk_features8_scratch_one_byte_short(native):
    from kf2vecfsw_amd import _native as N
    need = native.kf_chunk_features_scratch_bytes(64)
    assert call(native, work_bytes=need - 1) == N.KF_ERANGE
    msg = native.kf_last_error()
    assert msg.startswith(b"kf_chunk_features8: ") and b"scratch needs %d bytes" % need in msg
    # these pass every argument check, so they are asked with a scratch one byte short and end there:
    # null counts with no rows, counts at any byte (1-byte alignment), float32 out 4-byte aligned
    assert call(native, counts=None, n_rows=0, work_bytes=need - 1) == N.KF_ERANGE
    for off in (1, 2, 3, 7):
        assert call(native, counts=fake(1, off), out=fake(4, 4), work_bytes=need - 1) == N.KF_ERANGE
    assert call(native, ob=8, scaler=-2.5, nbins=10, work_bytes=need - 1) == N.KF_ERANGE


CAP_REFUSALS = [
    ("null src", dict(src=None), b"null d_src"),
    ("null dst", dict(dst=None), b"null d_dst"),
    ("odd src", dict(src=fake(1, 1)), b"misaligned d_src"),
    ("odd src, 16-aligned dst", dict(src=fake(1, 7), dst=fake(2, 16)), b"misaligned d_src"),
]


@pytest.mark.parametrize("what,kw,word", CAP_REFUSALS, ids=[r[0] for r in CAP_REFUSALS])
def test_rows_cap8_refuses(native, what, kw, word):
    from kf2vecfsw_amd import _native as N
    a = dict(src=fake(1), n=4097, dst=fake(2, 3))
    a.update(kw)
    assert native.kf_rows_cap8(a["src"], a["n"], a["dst"], None) == N.KF_EINVAL, what
    msg = native.kf_last_error()
    assert msg.startswith(b"kf_rows_cap8: ") and word in msg, (what, msg)


def test_rows_cap8_of_nothing_is_a_no_op(native):
    """n == 0 returns before any HIP call (there is no device here), whatever the pointers."""
    assert native.kf_rows_cap8(fake(1), 0, fake(2), None) == 0
    assert native.kf_rows_cap8(None, 0, None, None) == 0


# ---------------------------------------------------------------- the oracle's anchor
def test_statement_on_capped_rows_is_the_statement_with_cap_255():
    from kf2vecfsw_amd import chunks as CH
    rng = np.random.default_rng(255)
    rows = rng.integers(0, 700, size=(300, 136)).astype(np.uint16)
    rows[rng.random(rows.shape) < 0.05] = 0xFFFF
    for v, at in zip((0, 254, 255, 256, 32767, 32768, 65535), range(7)):
        rows[at, at] = v
    rows[40:44] = 0
    rows8 = np.minimum(rows, 255).astype(np.uint8)
    assert rows.max() > 255 and (rows8 == 255).any() and (rows8 == 254).any()
    lo = np.concatenate([[0, 40, 40, 0, 299], rng.integers(0, 200, size=40)])
    n = np.concatenate([[300, 4, 0, 7, 1], rng.integers(1, 100, size=40)])
    a = CH.range_features_host(rows8, lo, n, 1e4, None)
    b = CH.range_features_host(rows, lo, n, 1e4, 255)
    assert a.dtype == b.dtype == np.float64 and np.array_equal(a.view(np.uint64), b.view(np.uint64))
    assert np.array_equal(a.view(np.uint64), CH.range_features_host(rows8, lo, n, 1e4, 255).view(np.uint64))
    assert not np.array_equal(a, CH.range_features_host(rows, lo, n, 1e4, None))       # the cap tells here
    assert (a[1].view(np.uint64) == 0).all() and (a[2].view(np.uint64) == 0).all()      # T == 0: +0.0


def test_from_host_takes_uint8_rows():
    import torch
    from kf2vecfsw_amd import chunks as CH
    a, b = np.arange(4 * 32, dtype=np.uint8).reshape(4, 32), np.full((2, 32), 255, np.uint8)
    st = CH.ChunkStore.from_host([a, b], ["a", "b"], 3, "cpu")
    assert st.counts.dtype == torch.uint8 and st.row0.tolist() == [0, 4, 6]
    assert np.array_equal(st.counts.numpy(), np.concatenate([a, b]))
    with pytest.raises(ValueError, match="uint16"):                                    # one width per store
        CH.ChunkStore.from_host([a, b.astype(np.uint16)], ["a", "b"], 3, "cpu")
    st = CH.ChunkStore.from_host([a.astype(np.uint16)], ["a"], 3, "cpu")
    assert st.counts.dtype == torch.int16


def test_wrapper_refuses_a_lower_cap_over_uint8_rows():
    """Before anything is sent to a device: a cap below 255 needs the rows that were not capped."""
    import torch
    from kf2vecfsw_amd import counter as C
    rows = torch.zeros((4, 32), dtype=torch.uint8)
    for cap in (254, 0):
        with pytest.raises(ValueError, match="cap={}".format(cap)):
            C.chunk_features(rows, [0], [1], 1.0, cap)
