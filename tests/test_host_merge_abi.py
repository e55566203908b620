"""CPU tests of kf_sparse_merge's C-ABI: the symbols, the tile and scratch sizes
and every refusal of the contract in include/kf2vec_gpu.h.  Every call is given
fake non-null addresses and must return before any HIP call (no device here)."""
import pytest

LIMIT = 1 << 34   # entries: the documented limit of n_a + n_b


def fake(i, off=0):
    """A fake device address, aligned to 4 KiB plus `off`."""
    return (0x7000_0000_0000 + (i << 32)) + off


def call(L, **kw):
    a = dict(ka=fake(1), ca=fake(2), cba=4, na=1000, kb=fake(3), cb=fake(4), cbb=8, nb=3000, ko=fake(5), co=fake(6),
             no=fake(7), st=fake(8), scr=fake(9), scr_bytes=None, stream=None)
    a.update(kw)
    if a["scr_bytes"] is None:
        a["scr_bytes"] = L.kf_sparse_merge_scratch_bytes(a["na"], a["nb"])
    return L.kf_sparse_merge(a["ka"], a["ca"], a["cba"], a["na"], a["kb"], a["cb"], a["cbb"], a["nb"], a["ko"],
                             a["co"], a["no"], a["st"], a["scr"], a["scr_bytes"], a["stream"])


def test_merge_symbols_exported(native):
    from kf2vecfsw_amd import _native as N
    for s in ("kf_sparse_merge_tile", "kf_sparse_merge_scratch_bytes", "kf_sparse_merge"):
        assert hasattr(native, s) and s in N.SIGNATURES, s


def test_merge_tile_is_a_multiple_of_64(native):
    T = native.kf_sparse_merge_tile()
    assert T > 0 and T % 64 == 0


def test_merge_scratch_bytes(native):
    T = native.kf_sparse_merge_tile()
    f = native.kf_sparse_merge_scratch_bytes
    assert f(0, 0) > 0
    sizes = [0, 1, T - 1, T, T + 1, 1000 * T, 1024 * T + 1, 1 << 26, 1 << 27, (1 << 30) + 5, 1 << 33, LIMIT]
    got = [f(n // 2, n - n // 2) for n in sizes]
    assert all(x > 0 and x % 8 == 0 for x in got)
    assert got == sorted(got)
    assert f(0, 3 * T + 7) == f(3 * T + 7, 0) == f(T, 2 * T + 7)      # a function of n_a + n_b
    assert got[-1] >= 8 * (LIMIT // T)                                  # something per tile


@pytest.mark.parametrize("what,kw", [
    ("null keys_out", dict(ko=None)),
    ("null counts_out", dict(co=None)),
    ("null n_out", dict(no=None)),
    ("null status", dict(st=None)),
    ("null scratch", dict(scr=None)),
    ("null keys_a with n_a > 0", dict(ka=None)),
    ("null counts_b with n_b > 0", dict(cb=None)),
    ("count_bytes_a 3", dict(cba=3)),
    ("count_bytes_b 0", dict(cbb=0)),
    ("count_bytes_b 16", dict(cbb=16)),
    ("keys_a off by 4", dict(ka=fake(1, 4))),
    ("keys_b off by 4", dict(kb=fake(3, 4))),
    ("u64 counts_b off by 4", dict(cb=fake(4, 4))),
    ("u32 counts_a off by 2", dict(ca=fake(2, 2))),
    ("keys_out off by 4", dict(ko=fake(5, 4))),
    ("counts_out off by 4", dict(co=fake(6, 4))),
    ("n_out off by 4", dict(no=fake(7, 4))),
    ("status off by 2", dict(st=fake(8, 2))),
    ("one entry past the limit", dict(na=LIMIT // 2, nb=LIMIT // 2 + 1, scr_bytes=1 << 40)),
    ("n_a alone past the limit", dict(na=LIMIT + 1, nb=0, scr_bytes=1 << 40)),
    ("n_a + n_b wraps", dict(na=(1 << 64) - 1, nb=2, scr_bytes=1 << 40)),
])
def test_merge_refuses(native, what, kw):
    from kf2vecfsw_amd import _native as N
    native.kf_sparse_merge(None, None, 3, 0, None, None, 3, 0, None, None, None, None, None, 0, None)   # another message
    before = native.kf_last_error()
    assert call(native, **kw) == N.KF_EINVAL, what
    msg = native.kf_last_error()
    assert msg.startswith(b"kf_sparse_merge:") and (msg != before or "count_bytes" in what), what


def test_merge_scratch_one_byte_short(native):
    from kf2vecfsw_amd import _native as N
    need = native.kf_sparse_merge_scratch_bytes(1000, 3000)
    assert call(native, scr_bytes=need - 1) == N.KF_ERANGE
    assert b"scratch needs %d bytes" % need in native.kf_last_error()
    # u32 counts need 4-byte alignment only; an empty list may have null pointers -- these pass
    # every argument check, so they are asked with a scratch one byte short and end there
    assert call(native, ca=fake(2, 4), scr_bytes=need - 1) == N.KF_ERANGE
    assert call(native, ka=None, ca=None, na=0, nb=4000, scr_bytes=need - 1) == N.KF_ERANGE
    assert call(native, na=LIMIT // 2, nb=LIMIT // 2, scr_bytes=8) == N.KF_ERANGE    # the limit itself is accepted
