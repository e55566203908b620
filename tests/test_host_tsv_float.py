"""CPU tests of the reader of tab-separated float tables: kf_parse_tsv_floats'
C-ABI (the symbols, the scratch size and every refusal of the contract in
include/kf2vec_gpu.h, each before any HIP call: every native call is given fake
non-null addresses, there is no device here); the host statement
tables.parse_tsv_floats_host with the Python reindexing (tables.table_host)
against pandas' round-trip parser and DataFrame.reindex on the four golden
tables and on generated ones; every malformed input of the contract; names that
come twice."""
import io
import os

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

TSV = os.path.join(GOLDEN, "tsv")
MATRICES = ["train_tree_newick_subtree_0.di_mtrx", "train_tree_newick_subtree_1.di_mtrx",
            "train_tree_newick_single_clade_subtree_0.di_mtrx"]
EMBEDDINGS = "embeddings_subtree_0.csv"


# ---------------------------------------------------------------- the C-ABI
def fake(i, off=0):
    """A fake device address, aligned to 4 KiB plus `off`."""
    return (0x7000_0000_0000 + (i << 32)) + off


def call(L, **kw):
    a = dict(data=fake(1), goff=fake(2), n_units=3, nbytes=1 << 20, ncols=300, cmap=fake(8), out_cols=200, cap=64,
             vals=fake(3), val_bytes=8, names=fake(7), row0=fake(4), st=fake(5), scratch=fake(6), scratch_bytes=None,
             stream=None)
    a.update(kw)
    if a["scratch_bytes"] is None:
        a["scratch_bytes"] = L.kf_parse_tsv_floats_scratch_bytes(min(a["nbytes"], (1 << 32) - 1), max(a["n_units"], 0),
                                                                 a["cap"])
    return L.kf_parse_tsv_floats(a["data"], a["goff"], a["n_units"], a["nbytes"], a["ncols"], a["cmap"], a["out_cols"],
                                 a["cap"], a["vals"], a["val_bytes"], a["names"], a["row0"], a["st"], a["scratch"],
                                 a["scratch_bytes"], a["stream"])


def test_symbols_exported(native):
    from kf2vecfsw_amd import _native as N
    for s in ("kf_parse_tsv_floats_scratch_bytes", "kf_parse_tsv_floats"):
        assert hasattr(native, s) and s in N.SIGNATURES, s
    assert native.kf_abi_version() == 1
    header = open(os.path.join(ROOT, "include", "kf2vec_gpu.h")).read()
    assert "int kf_parse_tsv_floats(" in header and "uint64_t kf_parse_tsv_floats_scratch_bytes(" in header


def test_scratch_bytes_grow_with_every_argument(native):
    f = native.kf_parse_tsv_floats_scratch_bytes
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
    assert f(1 << 30, 1, 1 << 20) == native.kf_parse_kf_floats_scratch_bytes(1 << 30, 1, 1 << 20)


REFUSALS = [
    ("ncols 0", dict(ncols=0), b"ncols == 0"),
    ("out_cols 0", dict(out_cols=0), b"out_cols == 0"),
    ("no map and out_cols below ncols", dict(cmap=None), b"no d_col_map"),
    ("no map and out_cols above ncols", dict(cmap=None, out_cols=301), b"no d_col_map"),
    ("negative n_units", dict(n_units=-1), b"negative unit count"),
    ("val_bytes 2", dict(val_bytes=2), b"val_bytes 2"),
    ("val_bytes 0", dict(val_bytes=0), b"val_bytes 0"),
    ("val_bytes 16", dict(val_bytes=16), b"val_bytes 16"),
    ("batch of 4 GiB", dict(nbytes=1 << 32), b"at most 4 GiB"),
    ("batch above 4 GiB", dict(nbytes=(1 << 40) + 16), b"at most 4 GiB"),
    ("null bytes", dict(data=None), b"null d_bytes"),
    ("null goff", dict(goff=None), b"null d_goff"),
    ("null vals", dict(vals=None), b"null d_vals"),
    ("null row_name", dict(names=None), b"null d_row_name"),
    ("null unit_row0", dict(row0=None), b"null d_unit_row0"),
    ("null status", dict(st=None), b"null d_status"),
    ("null scratch", dict(scratch=None), b"null d_scratch"),
    ("bytes off by 8", dict(data=fake(1, 8)), b"misaligned d_bytes"),
    ("bytes off by 1", dict(data=fake(1, 1)), b"misaligned d_bytes"),
    ("col_map off by 2", dict(cmap=fake(8, 2)), b"misaligned d_col_map"),
    ("col_map off by 1", dict(cmap=fake(8, 1)), b"misaligned d_col_map"),
    ("float64 vals off by 4", dict(vals=fake(3, 4)), b"misaligned d_vals"),
    ("float32 vals off by 2", dict(vals=fake(3, 2), val_bytes=4), b"misaligned d_vals (needs 4"),
    ("row_name off by 2", dict(names=fake(7, 2)), b"misaligned d_row_name"),
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
    assert msg.startswith(b"kf_parse_tsv_floats: ") and word in msg, (what, msg)


def test_scratch_one_byte_short(native):
    from kf2vecfsw_amd import _native as N
    need = native.kf_parse_tsv_floats_scratch_bytes(1 << 20, 3, 64)
    assert call(native, scratch_bytes=need - 1) == N.KF_ERANGE
    assert b"scratch needs %d bytes" % need in native.kf_last_error()
    assert call(native, scratch_bytes=0) == N.KF_ERANGE
    # these pass every argument check, so they are asked with a scratch one byte short and end there: no map with
    # out_cols == ncols, a map 4-byte aligned, out_cols above ncols, float32 values 4-byte aligned, no unit, no row
    # allowed for, the largest batch
    assert call(native, cmap=None, out_cols=300, scratch_bytes=need - 1) == N.KF_ERANGE
    assert call(native, cmap=fake(8, 4), scratch_bytes=need - 1) == N.KF_ERANGE
    assert call(native, out_cols=1 << 20, scratch_bytes=need - 1) == N.KF_ERANGE
    assert call(native, vals=fake(3, 4), val_bytes=4, scratch_bytes=need - 1) == N.KF_ERANGE
    assert call(native, n_units=0, cap=0, scratch_bytes=native.kf_parse_tsv_floats_scratch_bytes(1 << 20, 0, 0) - 1) \
        == N.KF_ERANGE
    big = (1 << 32) - 1
    assert call(native, nbytes=big, ncols=1, out_cols=1,
                scratch_bytes=native.kf_parse_tsv_floats_scratch_bytes(big, 3, 64) - 1) == N.KF_ERANGE


# ---------------------------------------------------------------- the statement against pandas
def same_bits(a: np.ndarray, b: np.ndarray) -> bool:
    """Equal float64 bit patterns, NaN positions compared as positions."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64))


def pandas_sorted(text: bytes, order, **kw):
    """read_true_dist_mtrx and sort_df (kf2vec/utils.py:141-192) with the one pandas setting that is correctly
    rounded; the index is read as text, as this project keeps it."""
    import pandas as pd          # the reference this test is about: without it the test fails, it does not skip
    df = pd.read_csv(io.BytesIO(text), sep="\t", header=0, index_col=0, float_precision="round_trip",
                     dtype={"Unnamed: 0": str}, keep_default_na=False, na_values=["nan"], **kw)
    ddf = df.reindex(index=order)
    if len(ddf.columns) > 1:
        ddf = ddf.reindex(columns=order)
    return ddf.to_numpy().astype(np.float64)


def statement_sorted(text: bytes, order):
    """tables.true_distances on the host: tables.table_host with true_distances' rows= and cols=."""
    from kf2vecfsw_amd import tables as T
    many = text.lstrip(b"\n").split(b"\n")[0].count(b"\t") > 1
    return T.table_host(text, True, rows=order, cols=order if many else None)


def orders_of(names, rng):
    """Orders to reindex by: the file's, shuffled, a strict subset, and one with names the file lacks."""
    names = list(names)
    shuffled = [names[i] for i in rng.permutation(len(names))]
    return [names, shuffled, shuffled[: max(1, len(names) // 2)], ["nowhere"] + shuffled[::-1] + ["G_absent"]]


@pytest.mark.parametrize("name", MATRICES)
def test_golden_matrices_equal_pandas_round_trip(name):
    from kf2vecfsw_amd import tables as T
    text = open(os.path.join(TSV, name), "rb").read()
    assert len(text) in (61, 103, 271)
    vals, names, cols = T.table_host(text, True)
    n = len(names)
    assert vals.shape == (n, n) and sorted(names) == sorted(cols) and names != cols     # the rows come in another order
    for order in orders_of(cols, np.random.default_rng(n)):
        got, rows, gcols = statement_sorted(text, order)
        assert rows == order and gcols == order
        assert same_bits(got, pandas_sorted(text, order))
    full, _, _ = statement_sorted(text, cols)
    assert not np.isnan(full).any() and (np.diag(full) == 0).all() and (full >= 0).all()


def test_pandas_default_parser_differs_on_the_single_clade_matrix():
    """pandas' default float parser, which the reference's trainers use, is not correctly rounded: on
    train_tree_newick_single_clade's 5 x 5 matrix it reads 2 of the 25 entries one unit in the last place away from
    the correctly rounded value (1.2999999999999998 and its mirror entry), so this reader is compared with
    float_precision="round_trip" and not with the default."""
    import pandas as pd
    from kf2vecfsw_amd import tables as T
    text = open(os.path.join(TSV, MATRICES[2]), "rb").read()
    vals, names, cols = T.table_host(text, True)
    default = pd.read_csv(io.BytesIO(text), sep="\t", header=0, index_col=0).to_numpy()
    exact = pd.read_csv(io.BytesIO(text), sep="\t", header=0, index_col=0, float_precision="round_trip").to_numpy()
    assert same_bits(vals, exact)
    assert vals.shape == default.shape == (5, 5)
    assert np.count_nonzero(vals.view(np.uint64) != default.view(np.uint64)) == 2
    assert np.allclose(vals, default, rtol=1e-15, atol=0)


def test_golden_embeddings_equal_pandas_round_trip():
    import pandas as pd
    from kf2vecfsw_amd import tables as T
    text = open(os.path.join(TSV, EMBEDDINGS), "rb").read()
    vals, names, cols = T.table_host(text, False)
    df = pd.read_csv(io.BytesIO(text), sep="\t", header=None, index_col=0, float_precision="round_trip")
    assert cols is None and names == [str(x) for x in df.index] and len(names) == 2
    assert vals.shape == df.shape and vals.shape[1] == 1024 and (vals < 0).any()
    assert same_bits(vals, df.to_numpy())
    assert np.array_equal(vals.astype(np.float32).view(np.uint32), df.to_numpy().astype(np.float32).view(np.uint32))


def field_of(rng, kind):
    """One field of the grammar: repr of any normal double (with exponents), of a distance, whole numbers, zeros of
    both signs, nan."""
    if kind == 0:
        bits = int(rng.integers(1, 2047)) << 52 | int(rng.integers(0, 1 << 52))
        x = float(np.uint64(bits).view(np.float64))
        return repr(x if rng.integers(2) else -x)
    if kind == 1:
        return repr(float(rng.integers(0, 400000)) / 1e5 * float(rng.integers(1, 9)))
    if kind == 2:
        return ["0", "0.0", "-0.0", "-0", "1e-05", "-1E+3", "7.", "16.e1"][int(rng.integers(8))]
    if kind == 3:
        return "nan"
    return repr(-float(rng.integers(1, 10 ** 6)) / 7.0)


def generated_matrix(rng, names, cols=None):
    cols = names if cols is None else cols
    lines = ["\t" + "\t".join(cols)]
    for nm in names:
        lines.append(nm + "".join("\t" + field_of(rng, int(rng.integers(5))) for _ in cols))
    return ("\n".join(lines) + "\n").encode()


def test_generated_matrices_equal_pandas_round_trip():
    from kf2vecfsw_amd import tables as T
    rng = np.random.default_rng(19)
    names = ["G%09d" % i for i in range(20)] + ["a,b", "with blank", " lead", "x,y z", "0012", "77"]
    text = generated_matrix(rng, names)
    vals, rows, cols = T.table_host(text, True)
    assert rows == names and cols == names                      # all-digit names stay text
    assert np.isnan(vals).any() and (vals < 0).any() and np.signbit(vals[vals == 0]).any() and (np.abs(vals) > 1e100).any()
    for order in orders_of(names, rng):
        got, grows, gcols = statement_sorted(text, order)
        assert grows == order and gcols == order
        assert same_bits(got, pandas_sorted(text, order))
    # blank lines between the rows and no final newline change nothing
    spaced = text.replace(b"\n", b"\n\n", 7)[:-1]
    assert same_bits(T.table_host(spaced, True)[0], vals)


def test_one_column_file_keeps_its_column():
    """sort_df reindexes the columns only if there is more than one (utils.py:167): a one-column file keeps its column,
    whatever the order names."""
    from kf2vecfsw_amd import tables as T
    rng = np.random.default_rng(3)
    names = ["A", "B", "C", "D"]
    text = generated_matrix(rng, names, cols=["C"])
    for order in orders_of(names, rng):
        got, rows, cols = statement_sorted(text, order)
        assert rows == order and cols == ["C"] and got.shape == (len(order), 1)
        assert same_bits(got, pandas_sorted(text, order))


def test_columns_skipped_and_absent():
    """cols= alone: a strict subset in another order (the others are skipped) and names the file lacks (NaN)."""
    import pandas as pd
    from kf2vecfsw_amd import tables as T
    rng = np.random.default_rng(4)
    names = ["r%d" % i for i in range(6)]
    cols = ["c%d" % i for i in range(9)]
    text = generated_matrix(rng, names, cols)
    df = pd.read_csv(io.BytesIO(text), sep="\t", header=0, index_col=0, float_precision="round_trip")
    for want in (cols[::-1], ["c7", "c2", "c3"], ["zz", "c8", "c0", "yy"]):
        got, rows, gcols = T.table_host(text, True, cols=want)
        assert rows == names and gcols == want
        assert same_bits(got, df.reindex(columns=want).to_numpy().astype(np.float64))
    with pytest.raises(ValueError, match="needs a header"):
        T.table_host(text, False, cols=["c1"])


# ---------------------------------------------------------------- the statement on malformed text
def row(name: bytes, fields) -> bytes:
    return name + b"".join(b"\t" + f for f in fields)


GOOD = [[b"0.03125", b"-1.2345e-05", b"12.0", b"-12.5", b"1.2999999999999998", b"7", b"nan", b"-0.0"][i % 8]
        for i in range(12)]
NINETEEN = b"1234567890123456789"


def swap(j, f, fields=GOOD):
    return list(fields[:j]) + [f] + list(fields[j + 1:])


# (what, the row, code, column), for ncols = 12 and COL_MAP below, which skips columns 4 and 9
MALFORMED = [
    ("too few fields", row(b"g", GOOD[:11]), 1, 11),
    ("name only", b"g", 1, 0),
    ("a name with commas only", b"g,1,2,3", 1, 0),
    ("too many fields", row(b"g", GOOD + [b"1.0"]), 2, 12),
    ("an empty field", row(b"g", swap(3, b"")), 3, 3),
    ("an empty last field", row(b"g", swap(11, b"")), 3, 11),
    ("+1", row(b"g", swap(0, b"+1")), 3, 0),
    ("a lone -", row(b"g", swap(5, b"-")), 3, 5),
    ("a lone - at the row's end", row(b"g", swap(11, b"-")), 3, 11),
    ("-nan", row(b"g", swap(5, b"-nan")), 3, 5),
    ("1-", row(b"g", swap(5, b"1-")), 3, 5),
    ("--1", row(b"g", swap(5, b"--1")), 3, 5),
    ("-.5", row(b"g", swap(5, b"-.5")), 3, 5),
    ("1e--5", row(b"g", swap(5, b"1e--5")), 3, 5),
    ("7 and CR", row(b"g", swap(11, b"7\r")), 3, 11),
    ("CR in the middle", row(b"g", swap(2, b"7\r")), 3, 2),
    ("inf", row(b"g", swap(6, b"inf")), 3, 6),
    ("-inf", row(b"g", swap(6, b"-inf")), 3, 6),
    ("blank before 7", row(b"g", swap(6, b" 7")), 3, 6),
    ("blank after 7", row(b"g", swap(6, b"7 ")), 3, 6),
    ("a comma inside a field", row(b"g", swap(6, b"1,5")), 3, 6),
    ("NaN", row(b"g", swap(6, b"NaN")), 3, 6),
    ("20 digits", row(b"g", swap(7, NINETEEN + b"0")), 6, 7),
    ("20 digits behind a sign", row(b"g", swap(7, b"-" + NINETEEN + b"0")), 6, 7),
    ("20 digits then a malformed byte", row(b"g", swap(7, NINETEEN + b"5x")), 6, 7),
    ("a malformed byte then 20 digits", row(b"g", swap(7, b"1x" + NINETEEN + b"5")), 3, 7),
    ("1e400", row(b"g", swap(8, b"1e400")), 7, 8),
    ("-1e400", row(b"g", swap(8, b"-1e400")), 7, 8),
    ("-1e-400", row(b"g", swap(8, b"-1e-400")), 7, 8),
    ("a subnormal", row(b"g", swap(8, b"-5e-324")), 7, 8),
    ("out of range in the last field, then too many", row(b"g", swap(11, b"1e400") + [b"1"]), 7, 11),
    ("out of range before malformed", row(b"g", swap(2, b"1e400", swap(3, b"x"))), 7, 2),
    ("a skipped column with x", row(b"g", swap(4, b"x")), 3, 4),
    ("a skipped column with 20 digits", row(b"g", swap(9, NINETEEN + b"0")), 6, 9),
    ("a skipped column with -nan", row(b"g", swap(9, b"-nan")), 3, 9),
    ("a skipped 1e400, then malformed", row(b"g", swap(4, b"1e400", swap(10, b"1-"))), 3, 10),
]
# (what, the row): accepted
FINE = [
    ("a skipped column with 1e400", row(b"g", swap(4, b"1e400"))),
    ("a skipped column with -1e-400", row(b"g", swap(9, b"-1e-400"))),
    ("19 digits behind a sign", row(b"g", swap(7, b"-" + NINETEEN))),
    ("an empty name", row(b"", GOOD)),
    ("a name of commas, blanks, CR and signs", row(b"a,b c\r-+_", GOOD)),
    ("the extremes", row(b"g", swap(0, b"-2.2250738585072014e-308", swap(1, b"-1.7976931348623157e308")))),
]
NCOLS, OUT_COLS = 12, 11
COL_MAP = [10, 0, 1, 2, -1, 3, 4, 5, 6, 11, 8, 9]          # 4 skipped by -1, 9 by an entry == out_cols; 7 is no one's


def batch_around(bad: bytes, before: int = 3, after: int = 2, newline: bool = True) -> bytes:
    lines = [row(b"r%d" % i, GOOD) for i in range(before)] + [bad] + [row(b"s%d" % i, GOOD) for i in range(after)]
    return b"\n".join(lines) + (b"\n" if newline else b"")


@pytest.mark.parametrize("what,bad,code,col", MALFORMED, ids=[m[0] for m in MALFORMED])
def test_statement_error_positions(what, bad, code, col):
    from kf2vecfsw_amd import tables as T
    for before, newline in ((3, True), (0, False), (4, False)):
        vals, names, status = T.parse_tsv_floats_host(batch_around(bad, before, 2 if newline else 0, newline), NCOLS,
                                                      COL_MAP, OUT_COLS)
        assert status == (code, before, col), (what, before)
        assert vals.shape == (before, OUT_COLS) and len(names) == before


@pytest.mark.parametrize("what,line", FINE, ids=[m[0] for m in FINE])
def test_statement_accepts(what, line):
    from kf2vecfsw_amd import tables as T
    vals, names, status = T.parse_tsv_floats_host(b"\n\n" + batch_around(line, newline=False), NCOLS, COL_MAP, OUT_COLS)
    assert status == (0, 0, 0) and vals.shape == (6, OUT_COLS)
    assert names[3] == line.split(b"\t")[0] and names[2] == b"r2"
    fields = line.split(b"\t")[1:]
    for j, d in enumerate(COL_MAP):
        if 0 <= d < OUT_COLS:
            assert same_bits(vals[3, d], float(fields[j])), (j, d)
    assert np.isnan(vals[:, 7]).all()                           # no column maps there
    assert same_bits(vals[2, 10], float(GOOD[0])) and np.signbit(vals[2, 5]) and vals[2, 5] == 0   # "-0.0"


def test_statement_first_error_and_cap():
    from kf2vecfsw_amd import tables as T
    bad_a = next(m[1] for m in MALFORMED if m[0] == "1-")
    bad_b = next(m[1] for m in MALFORMED if m[0] == "too few fields")
    two = batch_around(bad_a) + batch_around(bad_b)
    assert T.parse_tsv_floats_host(two, NCOLS)[2] == (3, 3, 5)
    assert T.parse_tsv_floats_host(batch_around(bad_b) + batch_around(bad_a), NCOLS)[2] == (1, 3, 11)
    good = batch_around(row(b"g", GOOD))
    assert T.parse_tsv_floats_host(good, NCOLS, cap_rows=6)[2] == (0, 0, 0)
    assert T.parse_tsv_floats_host(good, NCOLS, cap_rows=5)[2] == (5, 5, 0)
    assert T.parse_tsv_floats_host(two, NCOLS, cap_rows=3)[2] == (5, 3, 0)    # the row that errs is not read
    assert T.parse_tsv_floats_host(two, NCOLS, cap_rows=4)[2] == (3, 3, 5)
    assert T.parse_tsv_floats_host(b"", NCOLS)[2] == (0, 0, 0)
    assert T.parse_tsv_floats_host(b"\n\n\n", NCOLS, COL_MAP, OUT_COLS)[0].shape == (0, OUT_COLS)
    with pytest.raises(ValueError, match=r"m\.di_mtrx: row 3, column 5: malformed field \(kf_parse_tsv_floats status 3\)"):
        T.table_host(b"\t" + b"\t".join(b"c%d" % i for i in range(12)) + b"\n" + two, True, path="m.di_mtrx")


# ---------------------------------------------------------------- names that come twice
def test_duplicate_names_are_refused(tmp_path):
    from kf2vecfsw_amd import tables as T
    text = open(os.path.join(TSV, MATRICES[1]), "rb").read()
    names = ["G001871415", "G001940645", "G000830295"]
    with pytest.raises(ValueError, match="header.*'G001871415' comes twice"):
        T.table_host(text.replace(b"G001940645\tG000830295\n", b"G001871415\tG000830295\n"), True)
    with pytest.raises(ValueError, match="row names.*'G000830295' comes twice"):
        T.table_host(text.replace(b"\nG001940645\t", b"\nG000830295\t"), True, rows=names)
    with pytest.raises(ValueError, match="rows.*'G001940645' comes twice"):
        T.table_host(text, True, rows=names + names[1:2])
    with pytest.raises(ValueError, match="cols.*'G001940645' comes twice"):
        T.table_host(text, True, cols=names + names[1:2])
    # the device path refuses the same before it touches a device: the header and the orders are the host's
    path = tmp_path / "dup.di_mtrx"
    path.write_bytes(text.replace(b"G001940645\tG000830295\n", b"G001871415\tG000830295\n"))
    with pytest.raises(ValueError, match="header.*comes twice"):
        T.table_from_tsv(str(path), "cpu", header=True)
    path.write_bytes(text)
    with pytest.raises(ValueError, match="rows.*comes twice"):
        T.true_distances(str(path), names + names[:1], "cpu")
    # row names that come twice without rows= are kept, as pandas keeps them
    vals, rows, _ = T.table_host(text.replace(b"\nG001940645\t", b"\nG000830295\t"), True)
    assert rows.count("G000830295") == 2 and vals.shape == (3, 3)


def test_line_pieces_from_a_start_offset(tmp_path):
    """kf_line_pieces with a start tiles the file from there on and says what it said before without one."""
    from kf2vecfsw_amd import chunks as CH
    lines = [b"n%d" % i + b"\t0.5" * (i % 7 + 1) for i in range(200)]
    text = b"\n".join(lines) + b"\n"
    path = tmp_path / "t.tsv"
    path.write_bytes(text)
    assert CH.kf_line_pieces(str(path)) == [(0, len(text))] and CH.kf_line_pieces(str(path), 100, 0) == \
        CH.kf_line_pieces(str(path), 100)
    start = len(lines[0]) + 1
    for piece in (64, 100, 1000, 1 << 20):
        got = CH.kf_line_pieces(str(path), piece, start)
        assert got[0][0] == start and got[-1][1] == len(text) and all(a[1] == b[0] for a, b in zip(got, got[1:]))
        assert all(text[a - 1: a] == b"\n" and e > a for a, e in got)
        assert b"".join(text[a:e] for a, e in got) == text[start:]
    assert CH.kf_line_pieces(str(path), 64, len(text)) == [(len(text), len(text))]
