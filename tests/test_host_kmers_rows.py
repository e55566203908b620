"""Host side of the device-built get_kmers matrix (kf_kmers_rows): the entry's
argument checks (nothing is launched), the denominator rule that keeps the
weights equal to main.kmers_matrix's bit for bit, and the column -> standard
code table of the dense path.  No GPU needed."""
import numpy as np
import pytest


def _call(L, **kw):
    """kf_kmers_rows with made-up, well-aligned, never dereferenced pointers;
    keyword arguments replace single ones."""
    a = dict(keys=0x10000, counts=0x20000, count_bytes=4, src0=0x30000, n=0x40000, dst0=0x50000, denom=0x60000,
             n_seg=1, k=21, row_lo=0, row_hi=8, out=0x70000, status=0x80000)
    a.update(kw)
    return L.kf_kmers_rows(a["keys"], a["counts"], a["count_bytes"], a["src0"], a["n"], a["dst0"], a["denom"],
                           a["n_seg"], a["k"], a["row_lo"], a["row_hi"], a["out"], a["status"], None)


@pytest.mark.parametrize("kw, word", [
    (dict(k=1), b"k=1"), (dict(k=32), b"k=32"), (dict(count_bytes=2), b"count_bytes"), (dict(n_seg=-1), b"negative"),
    (dict(row_lo=9, row_hi=8), b"row_lo"), (dict(keys=None), b"null"), (dict(counts=None), b"null"),
    (dict(src0=None), b"null"), (dict(n=None), b"null"), (dict(dst0=None), b"null"), (dict(denom=None), b"null"),
    (dict(out=None), b"null"), (dict(status=None), b"null"), (dict(out=0x70008), b"misaligned"),
    (dict(out=0x70004), b"misaligned"), (dict(keys=0x10004), b"misaligned"),
    (dict(counts=0x20004, count_bytes=8), b"misaligned"), (dict(dst0=0x50004), b"misaligned"),
])
def test_kmers_rows_rejects_bad_args(native, kw, word):
    """KF_EINVAL with a message, before anything is launched."""
    from kf2vecfsw_amd import _native as N
    assert _call(native, **kw) == N.KF_EINVAL
    assert word in native.kf_last_error(), native.kf_last_error()


def test_kmers_tile_rows(native):
    t = native.kf_kmers_tile_rows()
    assert t > 0 and t % 4 == 0   # every tile starts 16-byte aligned in the slab


def test_kmers_denominators_rule(native):
    """Below 2^24 the divisor is float32(total); from 2^24 on it is np.sum of the
    float32 counts (what main.kmers_matrix divides by), not float32(total)."""
    import torch
    from kf2vecfsw_amd import counter as C
    big = np.array([1 << 24, 1, 1], np.uint32)
    assert np.sum(big.astype(np.float32)) != np.float32((1 << 24) + 2)   # the case tells the two rules apart
    rng = np.random.default_rng(3)
    small = rng.integers(1, 1000, 500).astype(np.uint32)
    edge = np.array([(1 << 24) - 2, 1], np.uint32)           # total 2^24 - 1: still exact
    wide = np.array([0xFFFFFFFF, 0x80000000, 5], np.uint32)   # bit patterns that are negative as int32
    many = rng.integers(1, 1 << 20, 3000).astype(np.uint32)   # a pairwise np.sum with inexact partial sums
    segs = [big, small, edge, np.zeros(0, np.uint32), wide, many]
    flat = np.concatenate([np.array([7, 7, 7], np.uint32)] + segs)   # three counts that belong to no segment
    n = np.array([s.size for s in segs])
    src0 = 3 + np.concatenate([[0], np.cumsum(n)[:-1]])
    want = np.array([np.sum(s.astype(np.float32)) for s in segs], np.float32)
    got = C.kmers_denominators(torch.from_numpy(flat.view(np.int32)), src0, n)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert got[0] == np.float32(1 << 24) and got[1] == np.float32(int(small.sum())) and got[2] == np.float32((1 << 24) - 1)
    # int64 counts (the merged pieces of a large file)
    c64 = np.array([1 << 40, 1, 1 << 32, 3, 9], np.int64)
    got = C.kmers_denominators(torch.from_numpy(c64), [0, 3], [3, 2])
    want = np.array([np.sum(c64[:3].astype(np.float32)), 12.0], np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert C.kmers_denominators(torch.zeros(4, dtype=torch.int32), [], []).size == 0


@pytest.mark.parametrize("k", [3, 4, 7])
def test_vocab_std_codes(native, k):
    """Column -> standard code (A0 C1 G2 T3) of the vocab's k-mer: its digits are
    vocab_digits(k), it is ascending, and it is the vocab's text."""
    from kf2vecfsw_amd import counter as C
    from kf2vecfsw_amd import main as M
    code = C.vocab_std_codes(k)
    assert code.dtype == np.uint64 and code.shape == (C.num_bins(k),)
    assert (np.diff(code.astype(np.int64)) > 0).all()
    shifts = 2 * np.arange(k - 1, -1, -1, dtype=np.uint64)
    std = ((code[:, None] >> shifts[None, :]) & np.uint64(3)).astype(np.intp)
    assert np.array_equal(np.array([0, 2, 3, 1], np.uint8)[std], M.vocab_digits(k))
    text = b"".join(bytes(b"ACGT"[d] for d in row) + b"\n" for row in std)
    assert text == C.vocab_text(k)
