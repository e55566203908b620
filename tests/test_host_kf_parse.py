"""CPU tests of the `.kf` reader: kf_parse_kf_rows' C-ABI (the symbols, the
scratch size and every refusal of the contract in include/kf2vec_gpu.h, each
before any HIP call: every native call is given fake non-null addresses, there
is no device here), its host statement chunks.parse_kf_rows_host against the
reference's chunk files and against every malformed input of the contract, and
chunks.kf_line_pieces."""
import gzip
import io
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
    a = dict(data=fake(1), goff=fake(2), n_units=3, nbytes=1 << 20, nbins=8192, cap=64, rows=fake(3), row0=fake(4),
             st=fake(5), scratch=fake(6), scratch_bytes=None, stream=None)
    a.update(kw)
    if a["scratch_bytes"] is None:
        a["scratch_bytes"] = L.kf_parse_kf_scratch_bytes(min(a["nbytes"], (1 << 32) - 1), max(a["n_units"], 0), a["cap"])
    return L.kf_parse_kf_rows(a["data"], a["goff"], a["n_units"], a["nbytes"], a["nbins"], a["cap"], a["rows"],
                              a["row0"], a["st"], a["scratch"], a["scratch_bytes"], a["stream"])


def test_symbols_exported(native):
    from kf2vecfsw_amd import _native as N
    for s in ("kf_parse_kf_scratch_bytes", "kf_parse_kf_rows"):
        assert hasattr(native, s) and s in N.SIGNATURES, s
    assert native.kf_abi_version() == 1


def test_scratch_bytes_grow_with_every_argument(native):
    f = native.kf_parse_kf_scratch_bytes
    sizes = [0, 1, 15, 16, 4095, 4096, 4097, 1 << 20, 1 << 30, (1 << 32) - 1]
    caps = [0, 1, 2, 63, 64, 4096, 1 << 20, 1 << 31, 1 << 40]
    units = [0, 1, 2, 1000, (1 << 31) - 1]
    for n in units:
        for c in caps:
            got = [f(b, n, c) for b in sizes]
            assert all(x > 0 and x % 8 == 0 for x in got) and got == sorted(got), (n, c)
        for b in sizes:
            got = [f(b, n, c) for c in caps]
            assert got == sorted(got), (n, b)
    for b in sizes:
        for c in caps:
            got = [f(b, n, c) for n in units]
            assert got == sorted(got), (b, c)
    # a word per 4 KiB of text and a word per row allowed for (a batch has no more rows than bytes)
    assert f(1 << 30, 1, 1 << 20) >= 4 * ((1 << 18) + (1 << 20))
    assert f(1 << 20, 1, 1 << 40) == f(1 << 20, 1, 1 << 20) < 8 << 20


REFUSALS = [
    ("nbins 0", dict(nbins=0), b"nbins"),
    ("negative n_units", dict(n_units=-1), b"negative unit count"),
    ("batch of 4 GiB", dict(nbytes=1 << 32), b"at most 4 GiB"),
    ("batch above 4 GiB", dict(nbytes=(1 << 40) + 16), b"at most 4 GiB"),
    ("null bytes", dict(data=None), b"null d_bytes"),
    ("null goff", dict(goff=None), b"null d_goff"),
    ("null rows", dict(rows=None), b"null d_rows"),
    ("null unit_row0", dict(row0=None), b"null d_unit_row0"),
    ("null status", dict(st=None), b"null d_status"),
    ("null scratch", dict(scratch=None), b"null d_scratch"),
    ("bytes off by 8", dict(data=fake(1, 8)), b"misaligned d_bytes"),
    ("bytes off by 1", dict(data=fake(1, 1)), b"misaligned d_bytes"),
    ("rows off by 1", dict(rows=fake(3, 1)), b"misaligned d_rows"),
    ("goff off by 4", dict(goff=fake(2, 4)), b"misaligned d_goff"),
    ("unit_row0 off by 4", dict(row0=fake(4, 4)), b"misaligned d_unit_row0"),
    ("status off by 4", dict(st=fake(5, 4)), b"misaligned d_status"),
    ("scratch off by 4", dict(scratch=fake(6, 4)), b"misaligned d_scratch"),
]


@pytest.mark.parametrize("what,kw,word", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refuses_before_any_hip_call(native, what, kw, word):
    from kf2vecfsw_amd import _native as N
    assert call(native, **kw) == N.KF_EINVAL, what
    msg = native.kf_last_error()
    assert msg.startswith(b"kf_parse_kf_rows: ") and word in msg, (what, msg)


def test_refusals_have_their_own_messages(native):
    seen = {}
    for what, kw, word in REFUSALS:
        call(native, **kw)
        seen[word] = native.kf_last_error()
    assert len(set(seen.values())) == len(seen) >= 15


def test_scratch_one_byte_short(native):
    from kf2vecfsw_amd import _native as N
    need = native.kf_parse_kf_scratch_bytes(1 << 20, 3, 64)
    assert call(native, scratch_bytes=need - 1) == N.KF_ERANGE
    assert b"scratch needs %d bytes" % need in native.kf_last_error()
    assert call(native, scratch_bytes=0) == N.KF_ERANGE
    # these pass every argument check, so they are asked with a scratch one byte short and end there:
    # rows 2-byte aligned, no unit, no row allowed for, the largest batch
    assert call(native, rows=fake(3, 2), scratch_bytes=need - 1) == N.KF_ERANGE
    assert call(native, n_units=0, cap=0, scratch_bytes=native.kf_parse_kf_scratch_bytes(1 << 20, 0, 0) - 1) \
        == N.KF_ERANGE
    big = (1 << 32) - 1
    assert call(native, nbytes=big, nbins=1, scratch_bytes=native.kf_parse_kf_scratch_bytes(big, 3, 64) - 1) \
        == N.KF_ERANGE


# ---------------------------------------------------------------- the statement
@pytest.fixture(scope="module")
def chunk_texts():
    return {f: gzip.open(os.path.join(CHUNK_DIR, f)).read() for f in CHUNK_FILES}


def split_parse(text: bytes) -> np.ndarray:
    """The independent reading: line.split(","), floats, uint16."""
    rows = [ln.split(",")[1:] for ln in text.decode().splitlines() if ln]
    v = np.asarray(rows).astype(np.float64)
    assert (v == np.floor(v)).all() and v.min() >= 0 and v.max() <= 65535
    return v.astype(np.uint16)


@pytest.mark.parametrize("name", CHUNK_FILES)
def test_statement_reads_the_reference_chunk_files(chunk_texts, name):
    from kf2vecfsw_amd import chunks as CH
    text = chunk_texts[name]
    rows, status = CH.parse_kf_rows_host(text, 8192)
    exp = split_parse(text)
    assert status == (0, 0, 0)
    assert rows.dtype == np.uint16 and rows.shape == exp.shape and exp.shape[0] >= 5 and exp.shape[1] == 8192
    assert np.array_equal(rows, exp)
    assert exp.any()


@pytest.mark.parametrize("name", CHUNK_FILES)
def test_statement_equals_pandas_as_the_reference_calls_it(chunk_texts, name):
    """my_read_csv_chunk (kf2vec/utils.py:402-405): read_csv without a header, column 0 the
    index and a string, every other column uint16."""
    pd = pytest.importorskip("pandas")
    from kf2vecfsw_amd import chunks as CH
    text = chunk_texts[name]
    dtypes = {0: str}
    dtypes.update((i, np.uint16) for i in range(1, 8193))
    frame = pd.read_csv(io.BytesIO(text), sep=",", header=None, index_col=0, dtype=dtypes, low_memory=True)
    rows, status = CH.parse_kf_rows_host(text, 8192)
    assert status == (0, 0, 0)
    assert np.array_equal(rows, frame.to_numpy())
    assert list(frame.index) == [ln.split(",", 1)[0] for ln in text.decode().splitlines()]


def k3_row(name: bytes, fields) -> bytes:
    return name + b"".join(b"," + f for f in fields)


GOOD = [b"%d.0" % (i % 7) for i in range(32)]

# (what, the row's fields or the whole row, code, column)
MALFORMED = [
    ("short row", k3_row(b"w", GOOD[:31]), 1, 31),
    ("name only", b"w", 1, 0),
    ("long row", k3_row(b"w", GOOD + [b"1.0"]), 2, 32),
    ("16.5", k3_row(b"w", GOOD[:5] + [b"16.5"] + GOOD[6:]), 3, 5),
    ("1e2", k3_row(b"w", GOOD[:5] + [b"1e2"] + GOOD[6:]), 3, 5),
    ("-1", k3_row(b"w", [b"-1"] + GOOD[1:]), 3, 0),
    ("blank before 7", k3_row(b"w", GOOD[:9] + [b" 7"] + GOOD[10:]), 3, 9),
    ("7 and CR", k3_row(b"w", GOOD[:31] + [b"7\r"]), 3, 31),
    ("65536", k3_row(b"w", GOOD[:20] + [b"65536"] + GOOD[21:]), 4, 20),
    ("70000.0", k3_row(b"w", GOOD[:20] + [b"70000.0"] + GOOD[21:]), 4, 20),
    ("a digit string that would wrap 64 bits", k3_row(b"w", GOOD[:2] + [b"18446744073709551617"] + GOOD[3:]), 4, 2),
    ("empty field", k3_row(b"w", GOOD[:13] + [b""] + GOOD[14:]), 3, 13),
    ("empty last field", k3_row(b"w", GOOD[:31] + [b""]), 3, 31),
    ("a lone point", k3_row(b"w", GOOD[:13] + [b"."] + GOOD[14:]), 3, 13),
    ("malformed before too many", k3_row(b"w", GOOD[:30] + [b"x"] + GOOD[31:] + [b"1"]), 3, 30),
    ("too many before malformed", k3_row(b"w", GOOD + [b"x"]), 2, 32),
]
FINE = [
    ("65535", k3_row(b"w", GOOD[:20] + [b"65535"] + GOOD[21:]), 20, 65535),
    ("65535.0", k3_row(b"w", GOOD[:20] + [b"65535.0"] + GOOD[21:]), 20, 65535),
    ("00012.000", k3_row(b"w", GOOD[:20] + [b"00012.000"] + GOOD[21:]), 20, 12),
    ("16.", k3_row(b"w", GOOD[:20] + [b"16."] + GOOD[21:]), 20, 16),
    ("16", k3_row(b"w", GOOD[:31] + [b"16"]), 31, 16),
    ("an empty name", k3_row(b"", [b"3"] + GOOD[1:]), 0, 3),
    ("a name of points, blanks and CR", k3_row(b"a.b c\r-_", [b"3"] + GOOD[1:]), 0, 3),
]


def batch_around(row: bytes, before: int = 3, after: int = 2, newline: bool = True) -> bytes:
    lines = [k3_row(b"r%d" % i, GOOD) for i in range(before)] + [row] + \
        [k3_row(b"s%d" % i, GOOD) for i in range(after)]
    return b"\n".join(lines) + (b"\n" if newline else b"")


@pytest.mark.parametrize("what,row,code,col", MALFORMED, ids=[m[0] for m in MALFORMED])
def test_statement_error_positions(what, row, code, col):
    from kf2vecfsw_amd import chunks as CH
    for before, newline in ((3, True), (0, False), (4, False)):
        rows, status = CH.parse_kf_rows_host(batch_around(row, before, 2 if newline else 0, newline), 32)
        assert status == (code, before, col), (what, before)
        assert rows.shape == (before, 32)


@pytest.mark.parametrize("what,row,col,value", FINE, ids=[m[0] for m in FINE])
def test_statement_accepts(what, row, col, value):
    from kf2vecfsw_amd import chunks as CH
    rows, status = CH.parse_kf_rows_host(b"\n\n" + batch_around(row, newline=False), 32)
    assert status == (0, 0, 0) and rows.shape == (6, 32)
    assert rows[3, col] == value
    assert np.array_equal(rows[2], [i % 7 for i in range(32)])


def test_statement_first_error_and_cap():
    from kf2vecfsw_amd import chunks as CH
    two = batch_around(MALFORMED[3][1]) + batch_around(MALFORMED[0][1])
    assert CH.parse_kf_rows_host(two, 32)[1] == (3, 3, 5)
    good = batch_around(k3_row(b"w", GOOD))
    assert CH.parse_kf_rows_host(good, 32, cap_rows=6)[1] == (0, 0, 0)
    assert CH.parse_kf_rows_host(good, 32, cap_rows=5)[1] == (5, 5, 0)
    assert CH.parse_kf_rows_host(two, 32, cap_rows=3)[1] == (5, 3, 0)    # the row that errs is not read
    assert CH.parse_kf_rows_host(two, 32, cap_rows=4)[1] == (3, 3, 5)
    assert CH.parse_kf_rows_host(b"", 32) [1] == (0, 0, 0) and CH.parse_kf_rows_host(b"\n\n\n", 32)[0].shape == (0, 32)


# ---------------------------------------------------------------- kf_line_pieces
def check_pieces(path, data: bytes, piece: int):
    from kf2vecfsw_amd import chunks as CH
    pcs = CH.kf_line_pieces(str(path), piece)
    assert pcs[0][0] == 0 and pcs[-1][1] == len(data)
    assert all(a < e or len(data) == 0 for a, e in pcs)
    assert all(pcs[i][1] == pcs[i + 1][0] for i in range(len(pcs) - 1))       # they tile the file
    assert all(data[a - 1: a] == b"\n" for a, _ in pcs[1:])                    # every cut is a line start
    # a piece is as short as the lines allow: it ends at the first line start at or after a + piece
    for a, e in pcs[:-1]:
        assert e - a >= piece and data.find(b"\n", a + piece - 1) + 1 == e
    assert b"".join(data[a:e] for a, e in pcs) == data
    return pcs


@pytest.mark.parametrize("final_newline", [True, False])
def test_kf_line_pieces(tmp_path, final_newline):
    rng = np.random.default_rng(12)
    lines = [b"w%d," % i + b",".join(b"%d.0" % v for v in rng.integers(0, 50, size=int(rng.integers(1, 120))))
             for i in range(400)]
    lines[37] = b"long," + b"1.0," * 6000 + b"2.0"         # 24 KB: longer than the pieces below
    data = b"\n".join(lines) + (b"\n" if final_newline else b"")
    path = tmp_path / "x.kf"
    path.write_bytes(data)
    from kf2vecfsw_amd import chunks as CH
    assert CH.kf_line_pieces(str(path), len(data)) == [(0, len(data))]
    assert CH.kf_line_pieces(str(path)) == [(0, len(data))]
    for piece in (1, 100, 4096, 10000, len(data) - 1):
        pcs = check_pieces(path, data, piece)
        if piece <= 10000:
            assert len(pcs) > 3
        whole = [(a, e) for a, e in pcs if a <= data.index(b"long,") < e]
        assert len(whole) == 1 and whole[0][1] >= data.index(b"long,") + len(lines[37])   # the long line is not cut
        # the last line is kept whether or not a newline ends it
        assert data[pcs[-1][0]: pcs[-1][1]].rstrip(b"\n").split(b"\n")[-1] == lines[-1]
    empty = tmp_path / "empty.kf"
    empty.write_bytes(b"")
    assert CH.kf_line_pieces(str(empty), 16) == [(0, 0)]
