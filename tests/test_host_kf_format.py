"""CPU tests of the `.kf` formatter: kf_format_kf_rows16's C-ABI (the symbols,
the scratch size and every refusal of the contract in include/kf2vec_gpu.h, each
before any HIP call: every native call is given fake non-null addresses, there
is no device here), the native writer of finished text (kf_write_text_segments)
and the host statement chunks.format_rows_host against the reference's chunk
files."""
import ctypes
import gzip
import os

import numpy as np
import pytest

from conftest import TOY

CHUNK_DIR = os.path.join(TOY, "train_tree_chunks")
CHUNK_FILES = ["G000402355.kf.gz", "G000830275.kf.gz", "G000830295.kf.gz"]


# ---------------------------------------------------------------- the C-ABI
def fake(i, off=0):
    """A fake device address, aligned to 4 KiB plus `off`."""
    return (0x7000_0000_0000 + (i << 32)) + off


def call(L, **kw):
    a = dict(counts=fake(1), n_rows=64, nbins=8192, pre=fake(2), pre_off=fake(3), n_pre=3, rpre=fake(4), rpos=fake(5),
             win=10000, pseudo=0, text=fake(6), cap=1 << 20, row_off=fake(7), st=fake(8), scratch=fake(9),
             scratch_bytes=None, stream=None)
    a.update(kw)
    if a["scratch_bytes"] is None:
        a["scratch_bytes"] = L.kf_format_kf_scratch_bytes(a["n_rows"], a["nbins"])
    return L.kf_format_kf_rows16(a["counts"], a["n_rows"], a["nbins"], a["pre"], a["pre_off"], a["n_pre"], a["rpre"],
                                 a["rpos"], a["win"], a["pseudo"], a["text"], a["cap"], a["row_off"], a["st"],
                                 a["scratch"], a["scratch_bytes"], a["stream"])


def test_symbols_exported(native):
    from kf2vecfsw_amd import _native as N
    for s in ("kf_format_kf_scratch_bytes", "kf_format_kf_rows16", "kf_write_text_segments"):
        assert hasattr(native, s) and s in N.SIGNATURES, s


def test_scratch_bytes_grow_with_every_argument(native):
    f = native.kf_format_kf_scratch_bytes
    rows = [0, 1, 2, 255, 256, 257, 4096, 1 << 20, (1 << 31) - 1]
    bins = [1, 2, 32, 136, 2047, 2048, 2049, 8192, 1 << 21]
    for b in bins:
        got = [f(n, b) for n in rows]
        assert all(x > 0 and x % 8 == 0 for x in got) and got == sorted(got), b
    for n in rows:
        got = [f(n, b) for b in bins]
        assert got == sorted(got), n
    # 16 bytes per row and 8 per tile of 2,048 cells
    assert f(4096, 8192) >= 16 * 4096 + 8 * (4096 * 8192 // 2048)
    assert f(4096, 8192) < 1 << 20


REFUSALS = [
    ("nbins 0", dict(nbins=0), b"nbins"),
    ("2^31 rows", dict(n_rows=1 << 31, nbins=1), b"fewer than 2^31"),
    ("cap of 4 GiB", dict(cap=1 << 32), b"at most 4 GiB"),
    ("cap above 4 GiB", dict(cap=(1 << 40) + 1), b"at most 4 GiB"),
    ("negative n_prefixes", dict(n_pre=-1), b"negative prefix count"),
    ("too many cells", dict(n_rows=(1 << 31) - 1, nbins=1 << 21), b"cells"),
    ("null counts", dict(counts=None), b"null d_counts"),
    ("null prefix bytes", dict(pre=None), b"null d_prefix_bytes"),
    ("null prefix_off", dict(pre_off=None), b"null d_prefix_off"),
    ("null row_prefix", dict(rpre=None), b"null d_row_prefix"),
    ("null row_start", dict(rpos=None), b"null d_row_start"),
    ("null text", dict(text=None), b"null d_text"),
    ("null row_off", dict(row_off=None), b"null d_row_off"),
    ("null status", dict(st=None), b"null d_status"),
    ("null scratch", dict(scratch=None), b"null d_scratch"),
    ("counts off by 1", dict(counts=fake(1, 1)), b"misaligned d_counts"),
    ("row_prefix off by 2", dict(rpre=fake(4, 2)), b"misaligned d_row_prefix"),
    ("prefix_off off by 4", dict(pre_off=fake(3, 4)), b"misaligned d_prefix_off"),
    ("row_start off by 4", dict(rpos=fake(5, 4)), b"misaligned d_row_start"),
    ("row_off off by 4", dict(row_off=fake(7, 4)), b"misaligned d_row_off"),
    ("status off by 4", dict(st=fake(8, 4)), b"misaligned d_status"),
    ("scratch off by 4", dict(scratch=fake(9, 4)), b"misaligned d_scratch"),
]


@pytest.mark.parametrize("what,kw,word", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refuses_before_any_hip_call(native, what, kw, word):
    from kf2vecfsw_amd import _native as N
    assert call(native, **kw) == N.KF_EINVAL, what
    msg = native.kf_last_error()
    assert msg.startswith(b"kf_format_kf_rows16: ") and word in msg, (what, msg)


def test_scratch_one_byte_short(native):
    from kf2vecfsw_amd import _native as N
    need = native.kf_format_kf_scratch_bytes(64, 8192)
    assert call(native, scratch_bytes=need - 1) == N.KF_ERANGE
    assert b"scratch needs %d bytes" % need in native.kf_last_error()
    assert call(native, scratch_bytes=0) == N.KF_ERANGE
    # these pass every argument check, so they are asked with a scratch one byte short and end there:
    # counts 2-byte aligned, row_prefix 4-byte aligned, text and prefix bytes at any address, the largest cap
    assert call(native, counts=fake(1, 2), rpre=fake(4, 4), text=fake(6, 1), pre=fake(2, 3), cap=(1 << 32) - 1,
                scratch_bytes=need - 1) == N.KF_ERANGE
    assert call(native, n_pre=0, win=0, pseudo=1, scratch_bytes=need - 1) == N.KF_ERANGE


# ---------------------------------------------------------------- the writer of finished text
def write_text(native, segs, text: bytes, threads=4):
    """kf_write_text_segments: segs = [(path, append, lo, hi)], back to back in text."""
    paths = (ctypes.c_char_p * len(segs))(*[os.fsencode(str(s[0])) for s in segs])
    app = np.asarray([1 if s[1] else 0 for s in segs], dtype=np.uint8)
    off = np.asarray([segs[0][2]] + [s[3] for s in segs], dtype=np.uint64) if segs else np.zeros(1, np.uint64)
    assert all(segs[i][3] == segs[i + 1][2] for i in range(len(segs) - 1))
    buf = np.frombuffer(text, dtype=np.uint8) if text else np.zeros(1, np.uint8)
    return native.kf_write_text_segments(len(segs), paths, app.ctypes.data, off.ctypes.data, buf.ctypes.data, threads)


def test_text_writer_truncates_and_appends(native, tmp_path):
    a, b = tmp_path / "a.kf", tmp_path / "b.kf"
    a.write_bytes(b"old contents that are longer than the new ones\n")
    b.write_bytes(b"kept,")
    text = b"??" + b"first\n" + b"second\n" + b"!!"
    assert write_text(native, [(a, False, 2, 8), (b, True, 8, 15)], text) == 0     # two segments in one call
    assert a.read_bytes() == b"first\n" and b.read_bytes() == b"kept,second\n"
    assert write_text(native, [(a, True, 8, 15)], text) == 0                        # appended by a later call
    assert a.read_bytes() == b"first\nsecond\n"
    assert write_text(native, [(b, False, 4, 4)], text) == 0                        # an empty segment truncates
    assert b.read_bytes() == b""
    c = tmp_path / "c.kf"
    assert write_text(native, [(c, True, 2, 8)], text) == 0                         # appending creates the file
    assert c.read_bytes() == b"first\n"
    assert write_text(native, [], b"") == 0


@pytest.mark.parametrize("threads", [1, 5])
def test_text_writer_segment_of_many_blocks(native, tmp_path, threads):
    rng = np.random.default_rng(9)
    block = 4 << 20
    n = 2 * block + 12345                                   # more than two write blocks
    text = rng.integers(0, 256, size=n + 700, dtype=np.uint8).tobytes()
    big, small = tmp_path / "big.kf", tmp_path / "small.kf"
    big.write_bytes(b"head\n")
    assert write_text(native, [(small, False, 3, 500), (big, True, 500, 500 + n)], text, threads) == 0
    assert small.read_bytes() == text[3:500]
    assert big.read_bytes() == b"head\n" + text[500: 500 + n]


def test_text_writer_unwritable_path(native, tmp_path):
    from kf2vecfsw_amd import _native as N
    ok = tmp_path / "ok.kf"
    bad = tmp_path / "no_such_dir" / "x.kf"
    assert write_text(native, [(ok, False, 0, 3), (bad, False, 3, 6)], b"abcdef") == N.KF_EINVAL
    msg = native.kf_last_error()
    assert b"cannot write" in msg and b"no_such_dir" in msg
    # a decreasing offset table is refused before any file is touched
    paths = (ctypes.c_char_p * 1)(os.fsencode(str(tmp_path / "never.kf")))
    off = np.asarray([5, 2], dtype=np.uint64)
    buf = np.zeros(8, np.uint8)
    assert native.kf_write_text_segments(1, paths, None, off.ctypes.data, buf.ctypes.data, 2) == N.KF_EINVAL
    assert not (tmp_path / "never.kf").exists()


# ---------------------------------------------------------------- the statement
@pytest.mark.parametrize("name", CHUNK_FILES)
def test_statement_writes_the_reference_chunk_files(native, name):
    """The rows that the reference's chunk files hold, formatted by the statement, are those files."""
    from kf2vecfsw_amd import chunks as CH
    text = gzip.open(os.path.join(CHUNK_DIR, name)).read()
    lines = text.decode().splitlines()
    names = [ln.split(",", 1)[0] for ln in lines]
    rows = np.asarray([ln.split(",")[1:] for ln in lines]).astype(np.float64).astype(np.uint16)
    assert rows.shape[0] >= 5 and rows.shape[1] == 8192
    # whole names (win_len = 0)
    got, off = CH.format_rows_host(rows, names, np.arange(len(names)), np.zeros(len(names), np.uint64), 0, False)
    assert got == text
    assert off.tolist() == np.cumsum([0] + [len(ln) + 1 for ln in lines]).tolist()
    # names from contig prefixes and window starts, as Genome.names builds them
    pre, rpre, rpos = [], [], []
    for nm in names:
        head, _, span = nm.rpartition("__")
        a, b = span.split("-")
        assert int(b) - int(a) == CH.CHUNK_SZ - 1
        if head + "__" not in pre:
            pre.append(head + "__")
        rpre.append(pre.index(head + "__"))
        rpos.append(int(a) - 1)
    got2, off2 = CH.format_rows_host(rows.view(np.int16), [p.encode() for p in pre], rpre, rpos, CH.CHUNK_SZ, False)
    assert got2 == text and off2.tolist() == off.tolist()
    # with pseudocount every column is "c.5"
    ps, _ = CH.format_rows_host(rows[:2], names[:2], [0, 1], [0, 0], 0, True)
    exp = "".join(names[i] + "," + ",".join("%d.5" % v for v in rows[i]) + "\n" for i in range(2))
    assert ps == exp.encode()


def test_statement_forms_and_names(native):
    from kf2vecfsw_amd import chunks as CH
    rows = np.asarray([[0, 0, 0], [1, 65535, 10], [0, 7, 0]], dtype=np.uint16)
    got, off = CH.format_rows_host(rows, [b"", b"p\xc3\xa9\xff_"], [1, 0, 1], [0, (1 << 64) - 1, (1 << 32) - 1],
                                   10000, False)
    lines = [b"p\xc3\xa9\xff_1-10000,0,0,0\n",             # only zero columns: integer text
             b"0-9999,1,65535,10\n",                       # no zero column: integer text; s + 1 wraps
             b"p\xc3\xa9\xff_4294967296-4294977295,0.0,7.0,0.0\n"]
    assert got == b"".join(lines)
    assert off.tolist() == np.cumsum([0] + [len(x) for x in lines]).tolist()
