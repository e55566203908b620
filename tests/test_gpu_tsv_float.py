"""GPU tests of the reader of tab-separated float tables: kf_parse_tsv_floats
against its host statement (tables.parse_tsv_floats_host) on bit patterns, NaN
positions compared as positions -- values where the column map places them,
every row's name, every unit's row range and, for text it refuses, code, unit,
row and column -- with sentinels around d_vals and d_row_name and in every entry
that no field maps to, which must stay intact; tables.true_distances,
backbone_embeddings and table_from_tsv against tables.table_host, whole and in
pieces; FloatTable.pairs against numpy."""
import os

import numpy as np
import pytest

from test_host_tsv_float import (COL_MAP, EMBEDDINGS, FINE, GOOD, MALFORMED, MATRICES, NCOLS, OUT_COLS, TSV, batch_around,
                                 row, same_bits)

pytestmark = pytest.mark.gpu

TILE = 4096
GUARD = 3                 # sentinel rows on either side of d_vals and d_row_name
SENTINEL = -6.02e23       # no value of the tests' rows
NAME_SENTINEL = -77


@pytest.fixture(scope="module")
def dev(native):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu tests need an MI355X")
    return torch.device("cuda:0")


def layout(units):
    """The units back to back as pack_ranges lays them out: 16-byte aligned, '\\n' padding."""
    buf, off = bytearray(), [0]
    for u in units:
        buf += u
        buf += b"\n" * (-len(buf) % 16)
        off.append(len(buf))
    return bytes(buf), np.asarray(off, dtype=np.int64)


def n_lines(units):
    return sum(len([ln for ln in u.split(b"\n") if ln]) for u in units)


def expected(units, ncols, col_map, out_cols, cap):
    """The statement, unit after unit: (values, names, unit_row0, (code, unit, row, column))."""
    from kf2vecfsw_amd import tables as T
    parts, names, row0 = [], [], [0]
    for u, text in enumerate(units):
        vals, nm, (code, r, c) = T.parse_tsv_floats_host(text, ncols, col_map, out_cols, cap - row0[-1])
        if code:
            return None, None, None, (code, u, r, c)
        parts.append(vals)
        names += nm
        row0.append(row0[-1] + vals.shape[0])
    return (np.concatenate(parts) if parts else np.zeros((0, out_cols))), names, row0, (0, 0, 0, 0)


def run(dev, units, ncols, col_map, out_cols, cap, val_bytes=8):
    """kf_parse_tsv_floats on the units, d_vals and d_row_name pre-filled with sentinels and between sentinel rows:
    (values [cap, out_cols], name spans, unit_row0, status) on the host, after the outer sentinels were found intact."""
    import torch
    from kf2vecfsw_amd import _native as N
    text, off = layout(units)
    dtype = torch.float64 if val_bytes == 8 else torch.float32
    d_text = torch.from_numpy(np.frombuffer(text + b"\0" * 16, dtype=np.uint8).copy()).to(dev)
    d_off = torch.from_numpy(off).to(dev)
    d_map = None if col_map is None else torch.from_numpy(np.asarray(col_map, dtype=np.int32)).to(dev)
    buf = torch.full((cap + 2 * GUARD, out_cols), SENTINEL, dtype=dtype, device=dev)
    spans = torch.full((cap + 2 * GUARD, 2), NAME_SENTINEL, dtype=torch.int32, device=dev)
    row0 = torch.full((len(units) + 3,), -7, dtype=torch.int64, device=dev)
    status = torch.full((6,), -7, dtype=torch.int64, device=dev)
    need = N.lib().kf_parse_tsv_floats_scratch_bytes(len(text), len(units), cap)
    scratch = torch.empty(need // 8, dtype=torch.int64, device=dev)
    N.check(N.lib().kf_parse_tsv_floats(d_text.data_ptr(), d_off.data_ptr(), len(units), len(text), ncols,
                                        None if d_map is None else d_map.data_ptr(), out_cols, cap,
                                        buf[GUARD:].data_ptr(), val_bytes, spans[GUARD:].data_ptr(), row0[1:].data_ptr(),
                                        status[1:].data_ptr(), scratch.data_ptr(), need,
                                        torch.cuda.current_stream(dev).cuda_stream), "kf_parse_tsv_floats")
    host, spans = buf.cpu().numpy(), spans.cpu().numpy()
    sent = np.asarray(SENTINEL, dtype=host.dtype)
    assert (host[:GUARD] == sent).all() and (host[GUARD + cap:] == sent).all(), "written outside d_vals"
    assert (spans[:GUARD] == NAME_SENTINEL).all() and (spans[GUARD + cap:] == NAME_SENTINEL).all(), \
        "written outside d_row_name"
    row0, status = row0.cpu().numpy(), status.cpu().numpy()
    assert row0[0] == row0[-1] == -7 and status[0] == status[-1] == -7, "written outside unit_row0 or status"
    return host[GUARD: GUARD + cap], spans[GUARD: GUARD + cap], row0[1:-1].tolist(), tuple(int(x) for x in status[1:5])


def check(dev, units, ncols, col_map=None, out_cols=None, cap=None, val_bytes=8):
    """The kernel equals the statement; returns the statement's (values, names, unit_row0, status)."""
    out_cols = ncols if out_cols is None else out_cols
    if cap is None:
        cap = n_lines(units) + 2
    vals, spans, row0, status = run(dev, units, ncols, col_map, out_cols, cap, val_bytes)
    evals, enames, erow0, estatus = expected(units, ncols, col_map, out_cols, cap)
    assert status == estatus
    cmap = np.arange(ncols) if col_map is None else np.asarray(col_map, dtype=np.int64)
    placed = np.zeros(out_cols, dtype=bool)
    placed[cmap[(cmap >= 0) & (cmap < out_cols)]] = True
    sent = np.asarray(SENTINEL, dtype=vals.dtype)
    assert (vals[:, ~placed] == sent).all(), "an entry that no field maps to was written"
    if estatus[0] == 0:
        n = erow0[-1]
        assert row0 == erow0
        want, got = evals[:, placed], vals[:n][:, placed]
        if val_bytes == 4:
            with np.errstate(over="ignore"):
                want = want.astype(np.float32)
            assert got.dtype == np.float32
            a, b = np.isnan(got), np.isnan(want)
            assert np.array_equal(a, b) and np.array_equal(got[~a].view(np.uint32), want[~b].view(np.uint32))
        else:
            assert same_bits(got, want)
        assert (vals[n:] == sent).all() and (spans[n:] == NAME_SENTINEL).all()   # no row past the last is touched
        text, _ = layout(units)
        assert [text[a: a + ln] for a, ln in spans[:n].tolist()] == enames
    return evals, enames, erow0, estatus


def write(path, data: bytes) -> str:
    path.write_bytes(data)
    return str(path)


def table_equals_host(table, text, header, rows=None, cols=None, dtype=np.float64):
    from kf2vecfsw_amd import tables as T
    vals, names, cnames = T.table_host(text, header, rows=rows, cols=cols)
    got = table.values.cpu().numpy()
    assert got.dtype == dtype and got.shape == vals.shape and table.values.is_contiguous()
    assert table.row_names == names and table.col_names == cnames
    with np.errstate(over="ignore"):
        want = vals.astype(dtype)
    a, b = np.isnan(got), np.isnan(want)
    bits = np.uint64 if dtype == np.float64 else np.uint32
    assert np.array_equal(a, b) and np.array_equal(got[~a].view(bits), want[~b].view(bits))
    return vals


# ---------------------------------------------------------------- the golden tables
@pytest.mark.parametrize("name", MATRICES)
def test_golden_matrices(dev, name):
    import torch
    from kf2vecfsw_amd import tables as T
    path = os.path.join(TSV, name)
    text = open(path, "rb").read()
    cols = text.split(b"\n")[0].decode().split("\t")[1:]
    for order in (cols, cols[::-1], cols[1:], ["nowhere"] + cols[::-1]):
        t = T.true_distances(path, order, dev)
        assert t.row_names == order and t.col_names == order and t.values.dtype == torch.float64
        table_equals_host(t, text, True, rows=order, cols=order)
    full = T.true_distances(path, cols, dev, dtype=torch.float32)
    table_equals_host(full, text, True, rows=cols, cols=cols, dtype=np.float32)
    assert bool((torch.diagonal(full.values) == 0).all())


def test_golden_embeddings(dev):
    import io
    import pandas as pd
    import torch
    from kf2vecfsw_amd import tables as T
    path = os.path.join(TSV, EMBEDDINGS)
    text = open(path, "rb").read()
    t = T.backbone_embeddings(path, dev)
    assert t.values.dtype == torch.float32 and t.values.shape == (2, 1024) and t.col_names is None
    table_equals_host(t, text, False, dtype=np.float32)
    df = pd.read_csv(io.BytesIO(text), sep="\t", header=None, index_col=0, float_precision="round_trip")
    assert torch.equal(t.values.cpu(), torch.from_numpy(df.values).float())       # query.py:129-134
    assert t.row_names == [str(x) for x in df.index]


# ---------------------------------------------------------------- small tables
SMALL = [
    ("1 x 1", b"\tA\nA\t0.0\n"),
    ("1 x 1 without a final newline", b"\tA\nA\t-2.5e-3"),
    ("2 x 2", b"\tA\tB\nB\t1.5\t0.0\nA\t0.0\t1.5\n"),
    ("2 x 2 without a final newline", b"\tA\tB\nB\t1.5\t0.0\nA\t0.0\t1.5"),
    ("blank lines between the rows", b"\n\tA\tB\tC\n\nC\t1\t2\t0\n\n\nA\t0\t-0.0\t1\n\nB\tnan\t0\t2\n\n"),
    ("one column", b"\td\nB\t1.5\nA\t0.25\nC\t7\n"),
]


@pytest.mark.parametrize("what,text", SMALL, ids=[s[0] for s in SMALL])
def test_small_tables(dev, tmp_path, what, text):
    from kf2vecfsw_amd import tables as T
    path = write(tmp_path / "m.di_mtrx", text)
    table_equals_host(T.table_from_tsv(path, dev, header=True), text, True)
    cols = text.lstrip(b"\n").split(b"\n")[0].decode().split("\t")[1:]
    for order in (["A"], ["B", "A"], ["C", "A", "zz", "B"]):
        many = len(cols) > 1
        t = T.true_distances(path, order, dev)
        assert t.row_names == order and t.col_names == (order if many else cols)
        table_equals_host(t, text, True, rows=order, cols=order if many else None)
    # the same bytes without their header line are a table without a header
    body = text.lstrip(b"\n").split(b"\n", 1)[1]
    t = T.table_from_tsv(write(tmp_path / "e.csv", body), dev, header=False)
    assert t.col_names is None
    table_equals_host(t, body, False)
    units = [body]
    check(dev, units, len(cols))
    check(dev, units, len(cols), cap=n_lines(units))


# ---------------------------------------------------------------- a 260 x 260 matrix
N260 = 260


def fields_260(rng, n):
    """Fields of 1..24 bytes: 17-digit reprs of both signs (most of them: a row is longer than a tile), short ones,
    exponents, nan."""
    bits = rng.integers(600, 1400, size=n, dtype=np.uint64) << np.uint64(52) | rng.integers(0, 1 << 52, size=n, dtype=np.uint64)
    anyd = bits.view(np.float64)
    short = [b"0", b"0.0", b"1e-05", b"7", b"-0.0", b"nan", b"12.5", b"-3", b"1.5E+3", b"-2.", b"0.1", b"-1e-7"]
    kind = rng.integers(0, 10, size=n)
    out = []
    for i in range(n):
        if kind[i] < 7:
            out.append(repr(float(anyd[i]) * (-1 if kind[i] & 1 else 1)).encode())
        elif kind[i] == 7:
            out.append(repr(float(rng.integers(0, 400000)) / 1e5).encode())
        else:
            out.append(short[int(rng.integers(len(short)))])
    return out


@pytest.fixture(scope="module")
def matrix260():
    """(names, header line, row lines): names of 0..40 bytes (one empty, some with ',' and blanks), all different."""
    rng = np.random.default_rng(260)
    names = []
    for i in range(N260):
        ln = i % 41
        tail = ("%d" % i).encode()
        body = bytes(rng.choice(list(b"abcXYZ019._-, "), size=max(ln - len(tail), 0)).astype(np.uint8))
        names.append((body + tail)[:ln] if ln >= len(tail) else tail)
    names[0] = b""
    assert len(set(names)) == N260 and max(map(len, names)) == 40
    lines = [row(nm, fields_260(rng, N260)) for nm in names]
    flen = {len(f) for ln in lines for f in ln.split(b"\t")[1:]}
    assert min(flen) == 1 and max(flen) == 24 and all(len(ln) > TILE for ln in lines)
    for f in (b"0", b"0.0", b"1e-05"):
        assert any(b"\t" + f + b"\t" in ln for ln in lines)
    assert any(len(f.lstrip(b"-").replace(b".", b"").split(b"e")[0].lstrip(b"0")) == 17 for f in lines[1].split(b"\t")[1:])
    header = b"\t" + b"\t".join(names)
    return names, header, lines


def maps_260():
    n = N260
    rng = np.random.default_rng(7)
    strided = np.full(n, -1)
    strided[::3] = np.arange(len(strided[::3]))
    wild = rng.permutation(n).astype(np.int64)                 # out_cols = 100: the entries 100..259 are out of range
    wild[::7] = -5                                             # and so are these
    wild[3::7] = (1 << 31) - 1
    wild[5::7] = -(1 << 31)
    wider = rng.permutation(n + 40)[:n]
    return [
        ("identity", None, n),
        ("reversed", np.arange(n)[::-1].copy(), n),
        ("strided subset", strided, len(strided[::3])),
        ("all skipped", np.full(n, -1), 5),
        ("out-of-range entries", wild, 100),
        ("out_cols above ncols", wider, n + 40),
    ]


@pytest.mark.parametrize("val_bytes", [8, 4])
@pytest.mark.parametrize("what,col_map,out_cols", maps_260(), ids=[m[0] for m in maps_260()])
def test_matrix_260(dev, matrix260, what, col_map, out_cols, val_bytes):
    names, header, lines = matrix260
    text = b"\n".join(lines) + b"\n"
    third = len(lines) // 3
    units = [b"\n".join(lines[:third]) + b"\n", b"\n".join(lines[third: 2 * third]), b"\n".join(lines[2 * third:]) + b"\n"]
    if col_map is not None:
        ok = col_map[(col_map >= 0) & (col_map < out_cols)]
        assert len(set(ok.tolist())) == len(ok)                 # no destination twice: every placed entry is decided
    evals, enames, erow0, status = check(dev, [text], N260, col_map, out_cols, val_bytes=val_bytes)
    assert status == (0, 0, 0, 0) and enames == names and evals.shape == (N260, out_cols)
    check(dev, units, N260, col_map, out_cols, cap=N260, val_bytes=val_bytes)    # three units, no slack


def test_two_columns_to_one_destination(dev):
    lines = [row(b"r%d" % i, [b"1.5", b"-2.5", b"7"]) for i in range(5)]
    vals, _, row0, status = run(dev, [b"\n".join(lines)], 3, [1, 1, 0], 2, cap=5)
    assert status == (0, 0, 0, 0) and row0 == [0, 5]
    assert (vals[:, 0] == 7).all() and np.isin(vals[:, 1], [1.5, -2.5]).all()


def test_field_starts_at_every_offset(dev):
    """ncols = 3, names of 0..15 bytes: fields of 1 byte and of 24 bytes start at every offset of a 16-byte word."""
    long = [b"-1.2345678901234567e-100", b"-9.8765432109876543e+200", b"-0.000001234567890123456"]
    assert all(len(f) == 24 for f in long)
    lines = []
    for n in range(16):
        lines.append(row(b"n" * n, [b"0", long[n % 3], b"7"]))
        lines.append(row(b"n" * n, [long[n % 3], b"0", long[(n + 1) % 3]]))
    evals, _, _, _ = check(dev, lines, 3, [2, 0, 1], 3)        # a unit each: every row starts a 16-byte word
    assert evals.shape == (32, 3) and (evals < 0).sum() == 48
    check(dev, [b"\n".join(lines) + b"\n"], 3)                 # and back to back in one unit


# ---------------------------------------------------------------- a file in pieces
@pytest.mark.parametrize("piece,batch", [(8 << 10, 64 << 10), (64 << 10, 256 << 10)], ids=["8K", "64K"])
def test_pieces_equal_the_whole_file(dev, matrix260, tmp_path, monkeypatch, piece, batch):
    import torch
    from kf2vecfsw_amd import chunks as CH
    from kf2vecfsw_amd import tables as T
    names, header, lines = matrix260
    text = header + b"\n" + b"\n".join(lines[:100]) + b"\n\n" + b"\n".join(lines[100:])       # no final newline
    path = write(tmp_path / "m.di_mtrx", text)
    tnames = [nm.decode() for nm in names]
    rng = np.random.default_rng(piece)
    order = [tnames[i] for i in rng.permutation(N260)][:200] + ["absent one", "absent two"]
    whole = T.table_from_tsv(path, dev, header=True)
    whole_sorted = T.true_distances(path, order, dev)
    assert whole.row_names == tnames and whole.col_names == tnames
    table_equals_host(whole_sorted, text, True, rows=order, cols=order)
    monkeypatch.setattr(CH, "KF_PIECE_BYTES", piece)
    calls = []
    real = T.parse_tsv_floats

    def counted(data, off, *a, **kw):
        calls.append(len(off) - 1)
        return real(data, off, *a, **kw)
    monkeypatch.setattr(T, "parse_tsv_floats", counted)
    gb = batch / (1 << 30)
    got = T.table_from_tsv(path, dev, header=True, batch_gb=gb)
    assert len(calls) >= 4 and max(calls) >= 2                  # several batches, several units in a batch
    assert got.row_names == tnames and got.col_names == tnames
    assert torch.equal(torch.nan_to_num(got.values, nan=-1.0), torch.nan_to_num(whole.values, nan=-1.0))
    calls.clear()
    got = T.table_from_tsv(path, dev, header=True, rows=order, cols=order, batch_gb=gb)
    assert len(calls) >= 4 and got.row_names == order and got.col_names == order
    assert torch.equal(torch.isnan(got.values), torch.isnan(whole_sorted.values))
    assert torch.equal(torch.nan_to_num(got.values, nan=-1.0), torch.nan_to_num(whole_sorted.values, nan=-1.0))
    # a refusal names the file, the row behind the header and the column, whichever piece and batch hold it
    f = lines[201].split(b"\t")
    f[1 + 77] = b"1-"
    bad = header + b"\n" + b"\n".join(lines[:201] + [b"\t".join(f)] + lines[202:]) + b"\n"
    path = write(tmp_path / "bad.di_mtrx", bad)
    for g in (1.0, gb):
        with pytest.raises(ValueError,
                           match=r"bad\.di_mtrx: row 201, column 77: malformed field \(kf_parse_tsv_floats status 3\)"):
            T.table_from_tsv(path, dev, header=True, batch_gb=g)
    with pytest.raises(ValueError, match=r"bad\.di_mtrx: row 201, column 77: malformed field"):
        T.true_distances(path, order, dev)


def test_duplicate_row_names_across_batches(dev, matrix260, tmp_path, monkeypatch):
    from kf2vecfsw_amd import chunks as CH
    from kf2vecfsw_amd import tables as T
    names, header, lines = matrix260
    twice = lines[:40] + [lines[3]]
    path = write(tmp_path / "dup.di_mtrx", header + b"\n" + b"\n".join(twice) + b"\n")
    monkeypatch.setattr(CH, "KF_PIECE_BYTES", 16 << 10)
    with pytest.raises(ValueError, match="row names: the name .* comes twice"):
        T.table_from_tsv(path, dev, header=True, rows=[names[5].decode()], batch_gb=(32 << 10) / (1 << 30))
    assert len(T.table_from_tsv(path, dev, header=True).row_names) == 41      # without rows= they are kept


# ---------------------------------------------------------------- refusals
def good_unit(n):
    return b"\n".join(row(b"u%d" % i, GOOD) for i in range(n)) + b"\n"


@pytest.mark.parametrize("what,bad,code,col", MALFORMED, ids=[m[0] for m in MALFORMED])
def test_error_positions(dev, what, bad, code, col):
    units = [good_unit(5), good_unit(4), good_unit(3)]
    for at in (0, 1, 2):                                        # the first, a middle and the last unit
        us = list(units)
        us[at] = batch_around(bad, 3, 2) if at != 2 else batch_around(bad, 4, 0, newline=False)
        assert check(dev, us, NCOLS, COL_MAP, OUT_COLS)[3] == (code, at, 3 if at != 2 else 4, col), at
    assert check(dev, [bad], NCOLS, COL_MAP, OUT_COLS)[3] == (code, 0, 0, col)


@pytest.mark.parametrize("what,line", FINE, ids=[m[0] for m in FINE])
def test_accepted_forms(dev, what, line):
    evals, enames, _, status = check(dev, [batch_around(line), batch_around(line, 0, 0, newline=False)], NCOLS, COL_MAP,
                                     OUT_COLS)
    assert status == (0, 0, 0, 0) and enames[3] == enames[6] == line.split(b"\t")[0]
    assert same_bits(evals[3], evals[6])


def test_first_error_and_row_cap(dev):
    bad_a = next(m[1] for m in MALFORMED if m[0] == "1-")
    bad_b = next(m[1] for m in MALFORMED if m[0] == "too few fields")
    bad_c = next(m[1] for m in MALFORMED if m[0] == "1e400")
    good = good_unit(12)
    two = batch_around(bad_a, 3, 2) + batch_around(bad_b, 3, 2)
    assert check(dev, [good, two], NCOLS)[3] == (3, 1, 3, 5)                # the lower offset of two errors
    assert check(dev, [good, batch_around(bad_b, 3, 2) + batch_around(bad_a, 3, 2)], NCOLS)[3] == (1, 1, 3, 11)
    assert check(dev, [good, batch_around(bad_c, 3, 2), batch_around(bad_a, 0, 0)], NCOLS)[3] == (7, 1, 3, 8)
    assert check(dev, [good, good], NCOLS, cap=24)[3] == (0, 0, 0, 0)
    assert check(dev, [good, good], NCOLS, cap=23)[3] == (5, 1, 11, 0)      # one below the true row count
    assert check(dev, [good, good], NCOLS, cap=12)[3] == (5, 1, 0, 0)
    assert check(dev, [good, two], NCOLS, cap=15)[3] == (5, 1, 3, 0)        # the row that errs is not read
    assert check(dev, [good, two], NCOLS, cap=16)[3] == (3, 1, 3, 5)
    # no unit at all, only empty ones, and units with no row allowed for
    assert run(dev, [], NCOLS, None, NCOLS, cap=4)[2:] == ([0], (0, 0, 0, 0))
    assert run(dev, [b"", b""], NCOLS, COL_MAP, OUT_COLS, cap=4)[2:] == ([0, 0, 0], (0, 0, 0, 0))
    assert run(dev, [b"\n" * 5000], NCOLS, None, NCOLS, cap=0)[2:] == ([0, 0], (0, 0, 0, 0))


@pytest.mark.parametrize("what", ["random bytes", "tabs only", "the grammar's bytes"])
def test_any_bytes_stay_inside_the_buffers(dev, what):
    rng = np.random.default_rng(64)
    n = 64 << 10
    if what == "random bytes":
        soup = rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()
    elif what == "tabs only":
        soup = b"\t" * n
    else:
        soup = bytes(rng.choice(list(b"\t\n\t0.e1-9n\t-a"), size=n).astype(np.uint8))
    units = [soup[: n // 3], soup[n // 3: 2 * n // 3 + 5], soup[2 * n // 3 + 5:]]
    once = rng.integers(-3, OUT_COLS + 3, size=NCOLS)          # a random map, some entries outside [0, out_cols)
    for j in range(NCOLS):                                      # no destination twice: every placed entry is decided
        if 0 <= once[j] < OUT_COLS and once[j] in once[:j]:
            once[j] = -1
    assert ((once >= 0) & (once < OUT_COLS)).sum() >= 4 and (once >= OUT_COLS).any() and (once < 0).any()
    for us in (units, [good_unit(4)] + units):
        for cap in (0, 1, 7, 3000):
            assert check(dev, us, NCOLS, once, OUT_COLS, cap=cap)[3][0] != 0
    if what == "tabs only":
        assert check(dev, [soup], NCOLS, once, OUT_COLS, cap=7)[3] == (3, 0, 0, 0)


# ---------------------------------------------------------------- the wrapper and pairs
def test_wrapper_and_refusal_text(dev):
    import torch
    from kf2vecfsw_amd import counter as C
    from kf2vecfsw_amd import tables as T
    units = [good_unit(6), good_unit(6)[:-1]]
    text, off = layout(units)
    d = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).to(dev)
    for dtype in (torch.float64, torch.float32):
        vals, spans, row0, status = T.parse_tsv_floats(d, off, NCOLS, COL_MAP, OUT_COLS, dtype=dtype, fill=float("nan"))
        assert vals.dtype == dtype and vals.shape[1] == OUT_COLS and vals.shape[0] >= 12
        assert C.parsed_to_host(row0, status, what="kf_parse_tsv_floats").tolist() == [0, 6, 12]
        want = expected(units, NCOLS, COL_MAP, OUT_COLS, 12)[0]
        got = vals[:12].cpu().numpy()
        assert np.array_equal(np.isnan(got), np.isnan(want))
        assert np.array_equal(np.nan_to_num(got), np.nan_to_num(want.astype(got.dtype)))
    vals, _, row0, status = T.parse_tsv_floats(d, torch.from_numpy(off).to(dev), NCOLS)       # the identity
    assert vals.shape[1] == NCOLS and C.parsed_to_host(row0, status).tolist() == [0, 6, 12]
    units[1] += b"\t1"
    text, off = layout(units)
    d = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).to(dev)
    _, _, row0, status = T.parse_tsv_floats(d, off, NCOLS)
    with pytest.raises(ValueError, match=r"b\.tsv: row 45, column 12: too many fields \(kf_parse_tsv_floats status 2\)"):
        C.parsed_to_host(row0, status, ["a.tsv", "b.tsv"], [0, 40], what="kf_parse_tsv_floats")


def test_pairs(dev, tmp_path):
    import torch
    from kf2vecfsw_amd import tables as T
    rng = np.random.default_rng(12)
    names = ["G%03d" % i for i in range(37)]
    m = rng.integers(0, 4000, size=(37, 37)) / 1000.0
    text = ("\t" + "\t".join(names) + "\n" + "".join(
        nm + "".join("\t" + repr(float(x)) for x in m[i]) + "\n" for i, nm in enumerate(names))).encode()
    order = [names[i] for i in rng.permutation(37)]
    t = T.true_distances(write(tmp_path / "t.di_mtrx", text), order, dev)
    host = t.values.cpu().numpy()                               # pdf_sorted
    perm = [names.index(x) for x in order]
    assert np.array_equal(host, m[np.ix_(perm, perm)])
    for labels in ([3, 0, 36, 3, 17], torch.tensor([5, 6, 7]), np.asarray([36]), []):
        lab = [int(x) for x in labels]
        r = host[np.ix_(lab, lab)]                              # utils.pairwise_true_dist
        got = t.pairs(labels)
        assert got.device.type == "cuda" and got.dtype == torch.float64
        assert np.array_equal(got.cpu().numpy(), r)
        r2 = np.repeat(np.repeat(r, 2, axis=0), 2, axis=1)     # utils.pairwise_true_dist_2rows
        assert np.array_equal(t.pairs(labels, repeat=2).cpu().numpy(), r2)
