"""CPU tests of the get_frequencies `.kf` reader: kf_parse_kf_floats' C-ABI (the
symbols, the scratch size and every refusal of the contract in
include/kf2vec_gpu.h, each before any HIP call: every native call is given fake
non-null addresses, there is no device here); the conversion core
kf_decimal_to_double (csrc/kf_decimal.h, the code the kernel runs per field)
against Python's float() on bit patterns; and the host statement
features.parse_kf_floats_host against pandas' round-trip parser and
counter.features on every golden `.kf` file, and against every malformed input
of the contract."""
import decimal
import glob
import gzip
import io
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, TOY

POSTPROC = os.path.join(GOLDEN, "ref_postproc")
DBL_MIN_EXACT = 1 << 1022          # 2^-1022 is 1 / this


# ---------------------------------------------------------------- the C-ABI
def fake(i, off=0):
    """A fake device address, aligned to 4 KiB plus `off`."""
    return (0x7000_0000_0000 + (i << 32)) + off


def call(L, **kw):
    a = dict(data=fake(1), goff=fake(2), n_units=3, nbytes=1 << 20, nbins=8192, cap=64, scaler=1.0, vals=fake(3),
             val_bytes=8, names=fake(7), row0=fake(4), st=fake(5), scratch=fake(6), scratch_bytes=None, stream=None)
    a.update(kw)
    if a["scratch_bytes"] is None:
        a["scratch_bytes"] = L.kf_parse_kf_floats_scratch_bytes(min(a["nbytes"], (1 << 32) - 1), max(a["n_units"], 0),
                                                                a["cap"])
    return L.kf_parse_kf_floats(a["data"], a["goff"], a["n_units"], a["nbytes"], a["nbins"], a["cap"], a["scaler"],
                                a["vals"], a["val_bytes"], a["names"], a["row0"], a["st"], a["scratch"],
                                a["scratch_bytes"], a["stream"])


def test_symbols_exported(native):
    from kf2vecfsw_amd import _native as N
    for s in ("kf_parse_kf_floats_scratch_bytes", "kf_parse_kf_floats", "kf_decimal_to_double"):
        assert hasattr(native, s) and s in N.SIGNATURES, s
    assert native.kf_abi_version() == 1
    from kf2vecfsw_amd import counter as C
    assert C.KF_PARSE_ERRORS[4] == "value above 65535" and 6 in C.KF_PARSE_ERRORS and 7 in C.KF_PARSE_ERRORS


def test_scratch_bytes_grow_with_every_argument(native):
    f = native.kf_parse_kf_floats_scratch_bytes
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
    # kf_parse_kf_rows' scratch and the table of powers of five: two words for each q in [-342, 308]
    assert f(1 << 30, 1, 1 << 20) == native.kf_parse_kf_scratch_bytes(1 << 30, 1, 1 << 20) + 16 * 651


REFUSALS = [
    ("nbins 0", dict(nbins=0), b"nbins"),
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
    assert msg.startswith(b"kf_parse_kf_floats: ") and word in msg, (what, msg)


def test_scratch_one_byte_short(native):
    from kf2vecfsw_amd import _native as N
    need = native.kf_parse_kf_floats_scratch_bytes(1 << 20, 3, 64)
    assert call(native, scratch_bytes=need - 1) == N.KF_ERANGE
    assert b"scratch needs %d bytes" % need in native.kf_last_error()
    assert call(native, scratch_bytes=0) == N.KF_ERANGE
    # these pass every argument check, so they are asked with a scratch one byte short and end there:
    # float32 values 4-byte aligned, no unit, no row allowed for, the largest batch
    assert call(native, vals=fake(3, 4), val_bytes=4, scratch_bytes=need - 1) == N.KF_ERANGE
    assert call(native, n_units=0, cap=0, scratch_bytes=native.kf_parse_kf_floats_scratch_bytes(1 << 20, 0, 0) - 1) \
        == N.KF_ERANGE
    big = (1 << 32) - 1
    assert call(native, nbytes=big, nbins=1, scratch_bytes=native.kf_parse_kf_floats_scratch_bytes(big, 3, 64) - 1) \
        == N.KF_ERANGE


# ---------------------------------------------------------------- the conversion core
def convert(native, w, q):
    """kf_decimal_to_double on the pairs: (bit patterns uint64, in_range bool)."""
    w = np.ascontiguousarray(w, dtype=np.uint64)
    q = np.ascontiguousarray(q, dtype=np.int32)
    out = np.full(w.size, -1.0)
    ok = np.full(w.size, 7, dtype=np.uint8)
    assert native.kf_decimal_to_double(w.ctypes.data, q.ctypes.data, w.size, out.ctypes.data, ok.ctypes.data) == 0
    assert set(np.unique(ok).tolist()) <= {0, 1}
    return out.view(np.uint64), ok.astype(bool)


def in_contract(w: int, q: int) -> bool:
    """Whether the contract of csrc/kf_decimal.h calls w * 10^q in range, in exact arithmetic."""
    if w == 0:
        return True
    if q < -342 or q > 308:
        return False
    if q < 0 and w * DBL_MIN_EXACT < 10 ** -q:      # below 2^-1022
        return False
    return float("{}e{}".format(w, q)) != float("inf")


def check_pairs(native, pairs, all_in_range=False):
    """Every (w, q): the bit pattern of float(f"{w}e{q}") where the contract has it in range, reported else."""
    w = [p[0] for p in pairs]
    q = [p[1] for p in pairs]
    bits, ok = convert(native, w, q)
    exp = np.asarray([float("{}e{}".format(a, b)) for a, b in pairs], dtype=np.float64)
    want = np.ones(len(pairs), bool) if all_in_range else np.asarray([in_contract(a, b) for a, b in pairs])
    bad = np.flatnonzero(ok != want)
    assert bad.size == 0, ("in_range", [(pairs[i], bool(ok[i])) for i in bad[:5]])
    bad = np.flatnonzero(want & (bits != exp.view(np.uint64)))
    assert bad.size == 0, ("value", [(pairs[i], hex(int(bits[i])), exp[i].hex()) for i in bad[:5]])
    assert (bits[~want] == 0).all()
    return want


def normal_doubles(rng, n, max_exp_field=2046):
    """Doubles drawn uniformly over the bit patterns of positive normal numbers."""
    bits = rng.integers(1, max_exp_field + 1, size=n, dtype=np.uint64) << np.uint64(52) \
        | rng.integers(0, 1 << 52, size=n, dtype=np.uint64)
    return bits.view(np.float64)


def sci_pair(s: str):
    """(w, q) of a decimal in repr or %e form: the digits as an integer, the exponent moved past them."""
    m, _, e = s.partition("e")
    ip, _, fp = m.partition(".")
    return int(ip + fp), int(e or 0) - len(fp)


def test_decimal_repr_of_random_doubles(native):
    d = normal_doubles(np.random.default_rng(2023), 1_000_000)
    pairs = [sci_pair(repr(x)) for x in d.tolist()]
    bits, ok = convert(native, [p[0] for p in pairs], [p[1] for p in pairs])
    assert ok.all()
    assert np.array_equal(bits, d.view(np.uint64))         # repr round-trips: the double itself
    sample = pairs[::97]
    check_pairs(native, sample, all_in_range=True)          # and float(f"{w}e{q}") says the same
    # the same doubles printed with 19 significant digits
    pairs = [(int(s[0] + s[2:20]), int(s[21:]) - 18) for s in ("%.18e" % x for x in d.tolist())]
    assert all(10 ** 18 <= p[0] < 10 ** 19 for p in pairs[:1000])
    check_pairs(native, pairs, all_in_range=True)


def test_decimal_midpoints_of_adjacent_doubles(native):
    rng = np.random.default_rng(64)
    a = normal_doubles(rng, 100_000, max_exp_field=2045)
    b = np.nextafter(a, np.inf)
    ctx = decimal.Context(prec=1200)
    down = decimal.Context(prec=19, rounding=decimal.ROUND_DOWN)
    pairs = []
    for x, y in zip(a.tolist(), b.tolist()):
        mid = ctx.divide(ctx.add(decimal.Decimal(x), decimal.Decimal(y)), 2)       # exact
        t = down.plus(mid).as_tuple()
        w = int("".join(map(str, t.digits)))
        w, q = w * 10 ** (19 - len(t.digits)), t.exponent - (19 - len(t.digits))
        assert 10 ** 18 <= w < 10 ** 19
        pairs += [(w - 1, q), (w, q), (w + 1, q)]
    check_pairs(native, pairs, all_in_range=True)
    # the truncation lies at or below the midpoint and one more lies above it: both neighbours are hit
    bits, _ = convert(native, [p[0] for p in pairs], [p[1] for p in pairs])
    lo, hi = bits[0::3], bits[2::3]
    assert np.array_equal(lo, a.view(np.uint64)) and np.array_equal(hi, b.view(np.uint64))


def test_decimal_ties_powers_and_extremes(native):
    pairs = []
    for w in (9007199254740993, 9007199254740995, (1 << 53) + 1, (1 << 53) + 3, (1 << 54) + 2, (1 << 54) + 6,
              (1 << 63) + (1 << 10), (1 << 63) + 3 * (1 << 10)):
        pairs += [(w, 0)]
        for k in range(1, 23):
            if w * 10 ** k < 1 << 64:
                pairs.append((w * 10 ** k, -k))          # the tie itself, written with trailing zeros
            pairs.append((w, k))                         # scaled up: exact while 5^k fits
            pairs.append((w, -k))
    for k in range(0, 28):                               # ties that 5^k divides out of: (2^53 + 1) * 5^k * 10^-k
        w = ((1 << 53) + 1) * 5 ** k
        if w < 1 << 64:
            pairs.append((w, -k))
    pairs += [(1, q) for q in range(-342, 309)]          # every power of ten the table covers
    pairs += [((1 << 64) - 1, q) for q in range(-345, 312)]
    pairs += [(0, q) for q in (-100000, -343, -342, 0, 308, 309, 100000)]
    pairs += [(1, q) for q in (-2 ** 31, -100000, -343, 309, 100000, 2 ** 31 - 1)]
    # the smallest normal number, 2^-1022 = 2.2250738585072013830902...e-308, and its neighbours
    pairs += [(22250738585072014, -324), (22250738585072013, -324), (22250738585072011, -324),
              (2225073858507201383, -326), (2225073858507201384, -326), (2225073858507201382, -326),
              (22250738585072019, -324), (4450147717014403, -323), (49406564584124654, -340), (5, -324)]
    # the largest, DBL_MAX = 1.7976931348623157081...e308; halfway to 2^1024 is 1.79769313486231580793...e308
    pairs += [(17976931348623157, 292), (17976931348623158, 292), (17976931348623159, 292),
              (1797693134862315807, 290), (1797693134862315808, 290), (1797693134862315708, 290),
              (17976931348623158079, 289), (17976931348623158080, 289), (18, 307), (2, 308), (1, 308)]
    want = check_pairs(native, pairs)
    said = dict(zip(pairs, want.tolist()))
    assert said[(22250738585072014, -324)] and not said[(22250738585072013, -324)]
    assert not said[(2225073858507201383, -326)] and said[(2225073858507201384, -326)]
    assert said[(17976931348623158, 292)] and not said[(17976931348623159, 292)]
    assert said[(17976931348623158079, 289)] and not said[(17976931348623158080, 289)]
    assert not said[(5, -324)] and not said[(1, 309)] and said[(0, 100000)]


# ---------------------------------------------------------------- the statement on the golden files
def golden_kf_files():
    files = sorted(glob.glob(os.path.join(POSTPROC, "kf", "*.kf.gz")))
    for d in ("train_tree_kf", "test_kf"):
        files += sorted(glob.glob(os.path.join(TOY, d, "*.kf.gz")))
    return files


GOLDEN_KF = golden_kf_files()


def same_bits(a: np.ndarray, b: np.ndarray) -> bool:
    """Equal float64 bit patterns, NaN positions compared as positions."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64))


def test_golden_files_are_all_there():
    assert len(glob.glob(os.path.join(POSTPROC, "kf", "*.kf.gz"))) == 44 and len(GOLDEN_KF) >= 44 + 7


@pytest.mark.parametrize("path", GOLDEN_KF, ids=[os.path.relpath(p, GOLDEN) for p in GOLDEN_KF])
def test_statement_equals_pandas_round_trip(path):
    """my_read_csv (kf2vec/utils.py:436-437) with the one pandas setting that is correctly rounded."""
    import pandas as pd          # the reference this test is about: without it the test fails, it does not skip
    from kf2vecfsw_amd import features as F
    text = gzip.open(path).read()
    nbins = text.split(b"\n")[0].count(b",")
    vals, names, status = F.parse_kf_floats_host(text, nbins)
    assert status == (0, 0, 0)
    frame = pd.read_csv(io.BytesIO(text), index_col=0, header=None, sep=",", float_precision="round_trip")
    assert vals.dtype == np.float64 and vals.shape == frame.shape and vals.shape[0] >= 1
    assert same_bits(vals, frame.to_numpy().astype(np.float64))
    assert [n.decode() for n in names] == [str(x) for x in frame.index]
    # the slow reading of the statement (field by field) says the same as its fast one
    for line, row in zip([ln for ln in text.split(b"\n") if ln][:1], vals[:1]):
        got = [F._float_field(f) for f in line.split(b",")[1:][:: max(1, nbins // 257)]]
        assert all(e == 0 for e, _ in got) and same_bits([x for _, x in got], row[:: max(1, nbins // 257)])


def manifest_cases():
    m = json.load(open(os.path.join(POSTPROC, "manifest.json")))
    return [(e["file"], e["input"], e["k"], e["pseudocount"], e["raw_cnt"]) for e in m["kf"]]


@pytest.mark.parametrize("kf,inp,k,pseudo,raw", manifest_cases(), ids=[c[0] for c in manifest_cases()])
def test_statement_equals_counter_features(oracle, kf, inp, k, pseudo, raw):
    """The files' numbers are counter.features of the counts they were written from, bit for bit."""
    import torch
    from kf2vecfsw_amd import counter as C
    from kf2vecfsw_amd import features as F
    text = gzip.open(os.path.join(POSTPROC, kf)).read()
    counts, _ = oracle.count(gzip.open(os.path.join(POSTPROC, inp)).read(), k)
    vals, names, status = F.parse_kf_floats_host(text, counts.size)
    assert status == (0, 0, 0) and vals.shape == (1, counts.size)
    c = torch.from_numpy(np.ascontiguousarray(counts, dtype=np.uint32).view(np.int32).reshape(1, -1))
    assert same_bits(vals, C.features(c, pseudo, raw).numpy())
    assert same_bits(vals * 1e4, C.features(c, pseudo, raw, scaler=1e4).numpy())


def test_statement_equals_counter_features_on_the_toy_genomes(oracle, toy):
    import torch
    from kf2vecfsw_amd import counter as C
    from kf2vecfsw_amd import features as F
    for name, sample, data, exp in toy:
        counts, _ = oracle.count(data, 7)
        vals, names, status = F.parse_kf_floats_host(exp, 8192)
        assert status == (0, 0, 0) and names == [sample.encode()]
        c = torch.from_numpy(np.ascontiguousarray(counts, dtype=np.uint32).view(np.int32).reshape(1, -1))
        assert same_bits(vals, C.features(c).numpy()), name


def test_golden_fields_census():
    """What the golden files hold: every form of the grammar, and no field that the 19-digit limit refuses."""
    n = 0
    seen = set()
    most = 0
    for path in GOLDEN_KF:
        for line in gzip.open(path).read().split(b"\n"):
            for f in line.split(b",")[1:]:
                n += 1
                seen.add("nan" if f == b"nan" else "e" if b"e" in f else "." if b"." in f else "int")
                if len(f) > 17 and f != b"nan":
                    most = max(most, len(f.split(b"e")[0].replace(b".", b"").lstrip(b"0")))
    assert n == 880_032 and seen == {"nan", "e", ".", "int"} and most == 17


# ---------------------------------------------------------------- name spans
def test_name_spans_are_unsigned(tmp_path):
    """The kernel writes a name's offset and length as uint32 and a batch may be 4 GiB - 1 bytes: an offset of 2^31
    or more, held in the int32 tensor that parse_kf_floats returns, names the same bytes."""
    import torch
    from kf2vecfsw_amd import features as F
    offs = [0, 17, (1 << 31) - 10, 1 << 31, 3_000_000_000, (1 << 32) - 40]     # the third ends where the fourth starts
    lens = [3, 0, 10, 7, 12, 24]
    u32 = np.asarray(list(zip(offs, lens)) + [(123, 4)], dtype=np.uint32)
    row_name = torch.from_numpy(u32.view(np.int32).copy())
    assert int(row_name[4, 0]) == 3_000_000_000 - (1 << 32)                   # what the int32 storage shows
    spans = F.name_spans_to_host(row_name, len(offs))
    assert spans.dtype == np.int64 and spans.tolist() == [list(x) for x in zip(offs, lens)]
    assert F.name_spans_to_host(row_name, 0).shape == (0, 2)
    # the names cut out of a text of 4 GiB - 16 bytes (a sparse file: only the names' pages exist)
    path = tmp_path / "batch.bin"
    want = []
    with open(path, "wb") as f:
        f.truncate((1 << 32) - 16)
        for i, (a, n) in enumerate(zip(offs, lens)):
            name = (b"G%09d_genome_name_x" % i)[:n].ljust(n, b"z")
            f.seek(a)
            f.write(name)
            want.append(name.decode())
    text = np.memmap(path, dtype=np.uint8, mode="r")
    assert F.names_from_spans(text, spans) == want
    del text


# ---------------------------------------------------------------- the statement on malformed text
def k3_row(name: bytes, fields) -> bytes:
    return name + b"".join(b"," + f for f in fields)


GOOD = [[b"0.03125", b"1.2345e-05", b"12.0", b"12.5", b"0.00012207403790398877", b"7", b"nan"][i % 7] for i in range(32)]
NINETEEN = b"1234567890123456789"

# (what, the row, code, column)
MALFORMED = [
    ("too few fields", k3_row(b"g", GOOD[:31]), 1, 31),
    ("name only", b"g", 1, 0),
    ("too many fields", k3_row(b"g", GOOD + [b"1.0"]), 2, 32),
    ("an empty field", k3_row(b"g", GOOD[:13] + [b""] + GOOD[14:]), 3, 13),
    ("an empty last field", k3_row(b"g", GOOD[:31] + [b""]), 3, 31),
    ("1.2.3", k3_row(b"g", GOOD[:5] + [b"1.2.3"] + GOOD[6:]), 3, 5),
    ("1e", k3_row(b"g", GOOD[:5] + [b"1e"] + GOOD[6:]), 3, 5),
    ("1e+", k3_row(b"g", GOOD[:5] + [b"1e+"] + GOOD[6:]), 3, 5),
    ("1e+ at the row's end", k3_row(b"g", GOOD[:31] + [b"1e+"]), 3, 31),
    ("-1.0", k3_row(b"g", [b"-1.0"] + GOOD[1:]), 3, 0),
    ("+1.0", k3_row(b"g", [b"+1.0"] + GOOD[1:]), 3, 0),
    ("inf", k3_row(b"g", GOOD[:9] + [b"inf"] + GOOD[10:]), 3, 9),
    ("nan0", k3_row(b"g", GOOD[:9] + [b"nan0"] + GOOD[10:]), 3, 9),
    ("NaN", k3_row(b"g", GOOD[:9] + [b"NaN"] + GOOD[10:]), 3, 9),
    ("na", k3_row(b"g", GOOD[:9] + [b"na"] + GOOD[10:]), 3, 9),
    (".5", k3_row(b"g", GOOD[:9] + [b".5"] + GOOD[10:]), 3, 9),
    ("0x10", k3_row(b"g", GOOD[:9] + [b"0x10"] + GOOD[10:]), 3, 9),
    ("blank before 7", k3_row(b"g", GOOD[:9] + [b" 7"] + GOOD[10:]), 3, 9),
    ("7 and CR", k3_row(b"g", GOOD[:31] + [b"7\r"]), 3, 31),
    ("1e5.0", k3_row(b"g", GOOD[:9] + [b"1e5.0"] + GOOD[10:]), 3, 9),
    ("20 significant digits", k3_row(b"g", GOOD[:20] + [NINETEEN + b"0"] + GOOD[21:]), 6, 20),
    ("20 significant digits across the point", k3_row(b"g", GOOD[:20] + [b"0.00" + NINETEEN + b"1e3"] + GOOD[21:]), 6, 20),
    ("a digit string that would wrap 64 bits", k3_row(b"g", GOOD[:2] + [b"18446744073709551617"] + GOOD[3:]), 6, 2),
    ("20 digits then a malformed byte", k3_row(b"g", GOOD[:2] + [NINETEEN + b"5x"] + GOOD[3:]), 6, 2),
    ("a malformed byte then 20 digits", k3_row(b"g", GOOD[:2] + [b"1x" + NINETEEN + b"5"] + GOOD[3:]), 3, 2),
    ("1e400", k3_row(b"g", GOOD[:20] + [b"1e400"] + GOOD[21:]), 7, 20),
    ("1e-400", k3_row(b"g", GOOD[:20] + [b"1e-400"] + GOOD[21:]), 7, 20),
    ("1e309", k3_row(b"g", GOOD[:20] + [b"1e309"] + GOOD[21:]), 7, 20),
    ("a subnormal", k3_row(b"g", GOOD[:20] + [b"5e-324"] + GOOD[21:]), 7, 20),
    ("just below 2^-1022", k3_row(b"g", GOOD[:20] + [b"2.2250738585072013e-308"] + GOOD[21:]), 7, 20),
    ("above DBL_MAX", k3_row(b"g", GOOD[:20] + [b"1.7976931348623159e308"] + GOOD[21:]), 7, 20),
    ("an exponent that would wrap 32 bits", k3_row(b"g", GOOD[:20] + [b"1e4294967297"] + GOOD[21:]), 7, 20),
    ("out of range in the last field, then too many", k3_row(b"g", GOOD[:31] + [b"1e400", b"1"]), 7, 31),
    ("malformed before too many", k3_row(b"g", GOOD[:30] + [b"x"] + GOOD[31:] + [b"1"]), 3, 30),
    ("too many before malformed", k3_row(b"g", GOOD + [b"x"]), 2, 32),
    ("out of range before malformed", k3_row(b"g", GOOD[:4] + [b"1e400", b"x"] + GOOD[6:]), 7, 4),
]
# (what, the row, column, the value as float() reads it)
FINE = [
    ("19 significant digits", k3_row(b"g", GOOD[:20] + [NINETEEN] + GOOD[21:]), 20, NINETEEN),
    ("19 digits behind leading zeros", k3_row(b"g", GOOD[:20] + [b"000.000" + NINETEEN + b"e-3"] + GOOD[21:]), 20, None),
    ("a trailing point", k3_row(b"g", GOOD[:20] + [b"16."] + GOOD[21:]), 20, None),
    ("a point then an exponent", k3_row(b"g", GOOD[:20] + [b"16.e1"] + GOOD[21:]), 20, None),
    ("E and +", k3_row(b"g", GOOD[:20] + [b"1.5E+3"] + GOOD[21:]), 20, None),
    ("zero with a huge exponent", k3_row(b"g", GOOD[:20] + [b"0.0e99999999999"] + GOOD[21:]), 20, None),
    ("the smallest normal number", k3_row(b"g", GOOD[:31] + [b"2.2250738585072014e-308"]), 31, None),
    ("DBL_MAX", k3_row(b"g", GOOD[:31] + [b"1.7976931348623157e308"]), 31, None),
    ("an empty name", k3_row(b"", [b"3"] + GOOD[1:]), 0, None),
    ("a name of points, blanks and CR", k3_row(b"a.b c\r-_", [b"3"] + GOOD[1:]), 0, None),
]


def batch_around(row: bytes, before: int = 3, after: int = 2, newline: bool = True) -> bytes:
    lines = [k3_row(b"r%d" % i, GOOD) for i in range(before)] + [row] + \
        [k3_row(b"s%d" % i, GOOD) for i in range(after)]
    return b"\n".join(lines) + (b"\n" if newline else b"")


@pytest.mark.parametrize("what,row,code,col", MALFORMED, ids=[m[0] for m in MALFORMED])
def test_statement_error_positions(what, row, code, col):
    from kf2vecfsw_amd import features as F
    for before, newline in ((3, True), (0, False), (4, False)):
        vals, names, status = F.parse_kf_floats_host(batch_around(row, before, 2 if newline else 0, newline), 32)
        assert status == (code, before, col), (what, before)
        assert vals.shape == (before, 32) and len(names) == before


@pytest.mark.parametrize("what,row,col,value", FINE, ids=[m[0] for m in FINE])
def test_statement_accepts(what, row, col, value):
    from kf2vecfsw_amd import features as F
    vals, names, status = F.parse_kf_floats_host(b"\n\n" + batch_around(row, newline=False), 32)
    assert status == (0, 0, 0) and vals.shape == (6, 32)
    field = row.split(b",")[1 + col]
    assert vals[3, col] == float(value if value is not None else field)
    assert names[3] == row.split(b",")[0] and names[2] == b"r2"
    assert same_bits(vals[2], [float(f) for f in GOOD])


def test_statement_first_error_and_cap():
    from kf2vecfsw_amd import features as F
    bad_a = next(m[1] for m in MALFORMED if m[0] == "1.2.3")
    bad_b = next(m[1] for m in MALFORMED if m[0] == "too few fields")
    two = batch_around(bad_a) + batch_around(bad_b)
    assert F.parse_kf_floats_host(two, 32)[2] == (3, 3, 5)
    good = batch_around(k3_row(b"g", GOOD))
    assert F.parse_kf_floats_host(good, 32, cap_rows=6)[2] == (0, 0, 0)
    assert F.parse_kf_floats_host(good, 32, cap_rows=5)[2] == (5, 5, 0)
    assert F.parse_kf_floats_host(two, 32, cap_rows=3)[2] == (5, 3, 0)    # the row that errs is not read
    assert F.parse_kf_floats_host(two, 32, cap_rows=4)[2] == (3, 3, 5)
    assert F.parse_kf_floats_host(b"", 32)[2] == (0, 0, 0) and F.parse_kf_floats_host(b"\n\n\n", 32)[0].shape == (0, 32)
