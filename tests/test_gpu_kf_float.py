"""GPU tests of the get_frequencies `.kf` reader: kf_parse_kf_floats against its
host statement (features.parse_kf_floats_host) on bit patterns, NaN positions
compared as positions -- values, every row's name, every unit's row range and,
for text it refuses, code, unit, row and column -- with sentinels around d_vals
and d_row_name that must stay intact; features_from_kf against counter.features
of the counts that the CLI wrote its directory from."""
import decimal
import gzip
import os

import numpy as np
import pytest

from conftest import TOY
from test_host_kf_float import FINE, GOOD, MALFORMED, batch_around, k3_row, same_bits

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


def expected(units, nbins, cap):
    """The statement, unit after unit: (values, names, unit_row0, (code, unit, row, column))."""
    from kf2vecfsw_amd import features as F
    parts, names, row0 = [], [], [0]
    for u, text in enumerate(units):
        vals, nm, (code, r, c) = F.parse_kf_floats_host(text, nbins, cap - row0[-1])
        if code:
            return None, None, None, (code, u, r, c)
        parts.append(vals)
        names += nm
        row0.append(row0[-1] + vals.shape[0])
    return (np.concatenate(parts) if parts else np.zeros((0, nbins))), names, row0, (0, 0, 0, 0)


def run(dev, units, nbins, cap, scaler=1.0, val_bytes=8):
    """kf_parse_kf_floats on the units, d_vals and d_row_name between sentinel rows: (values [cap, nbins], names of
    the rows (from the spans), unit_row0, status) on the host, after the sentinels were found intact."""
    import torch
    from kf2vecfsw_amd import _native as N
    text, off = layout(units)
    dtype = torch.float64 if val_bytes == 8 else torch.float32
    d_text = torch.from_numpy(np.frombuffer(text + b"\0" * 16, dtype=np.uint8).copy()).to(dev)
    d_off = torch.from_numpy(off).to(dev)
    buf = torch.full((cap + 2 * GUARD, nbins), SENTINEL, dtype=dtype, device=dev)
    spans = torch.full((cap + 2 * GUARD, 2), NAME_SENTINEL, dtype=torch.int32, device=dev)
    row0 = torch.full((len(units) + 3,), -7, dtype=torch.int64, device=dev)
    status = torch.full((6,), -7, dtype=torch.int64, device=dev)
    need = N.lib().kf_parse_kf_floats_scratch_bytes(len(text), len(units), cap)
    scratch = torch.empty(need // 8, dtype=torch.int64, device=dev)
    N.check(N.lib().kf_parse_kf_floats(d_text.data_ptr(), d_off.data_ptr(), len(units), len(text), nbins, cap,
                                       float(scaler), buf[GUARD:].data_ptr(), val_bytes, spans[GUARD:].data_ptr(),
                                       row0[1:].data_ptr(), status[1:].data_ptr(), scratch.data_ptr(), need,
                                       torch.cuda.current_stream(dev).cuda_stream), "kf_parse_kf_floats")
    host, spans = buf.cpu().numpy(), spans.cpu().numpy()
    sent = np.asarray(SENTINEL, dtype=host.dtype)
    assert (host[:GUARD] == sent).all() and (host[GUARD + cap:] == sent).all(), "written outside d_vals"
    assert (spans[:GUARD] == NAME_SENTINEL).all() and (spans[GUARD + cap:] == NAME_SENTINEL).all(), \
        "written outside d_row_name"
    row0, status = row0.cpu().numpy(), status.cpu().numpy()
    assert row0[0] == row0[-1] == -7 and status[0] == status[-1] == -7, "written outside unit_row0 or status"
    return host[GUARD: GUARD + cap], spans[GUARD: GUARD + cap], row0[1:-1].tolist(), tuple(int(x) for x in status[1:5])


def check(dev, units, nbins, cap=None, scaler=1.0, val_bytes=8):
    """The kernel equals the statement; returns the statement's (values, names, unit_row0, status)."""
    if cap is None:
        cap = n_lines(units) + 2
    vals, spans, row0, status = run(dev, units, nbins, cap, scaler, val_bytes)
    evals, enames, erow0, estatus = expected(units, nbins, cap)
    assert status == estatus
    if estatus[0] == 0:
        n = erow0[-1]
        assert row0 == erow0
        with np.errstate(over="ignore"):
            want = evals * scaler                              # one float64 multiply
        if val_bytes == 4:
            with np.errstate(over="ignore"):
                want = want.astype(np.float32)
            assert vals.dtype == np.float32
            a, b = np.isnan(vals[:n]), np.isnan(want)
            assert np.array_equal(a, b) and np.array_equal(vals[:n][~a].view(np.uint32), want[~b].view(np.uint32))
        else:
            assert same_bits(vals[:n], want)
        sent = np.asarray(SENTINEL, dtype=vals.dtype)
        assert (vals[n:] == sent).all() and (spans[n:] == NAME_SENTINEL).all()   # no row past the last is touched
        text, _ = layout(units)
        assert [text[a: a + ln] for a, ln in spans[:n].tolist()] == enames
    return evals, enames, erow0, estatus


def random_fields(rng, n):
    """Fields of every form that `.kf` writers emit: repr of normalised frequencies and of any normal double, raw
    counts as "12.0", "12.5" and "12", zeros, nan."""
    bits = rng.integers(1, 2047, size=n, dtype=np.uint64) << np.uint64(52) | rng.integers(0, 1 << 52, size=n, dtype=np.uint64)
    anyd = bits.view(np.float64)
    freq = rng.integers(1, 50000, size=n) / 7654321.0
    cnt = rng.integers(0, 3_000_000, size=n)
    kind = rng.integers(0, 8, size=n)
    out = []
    for i in range(n):
        t = kind[i]
        out.append(repr(float(anyd[i])) if t == 0 else repr(float(freq[i])) if t in (1, 2, 3) else
                   "%d.0" % cnt[i] if t == 4 else "%d.5" % cnt[i] if t == 5 else "%d" % (cnt[i] % 100) if t == 6 else
                   ("nan" if cnt[i] % 3 == 0 else "0.0"))
    return [s.encode() for s in out]


def synth_rows(rng, n, nbins, name_len):
    rows = []
    for i in range(n):
        name = bytes(rng.choice(list(b"abcXYZ019._-"), size=name_len(i)).astype(np.uint8))
        rows.append(k3_row(name, random_fields(rng, nbins)))
    return rows


def field_spans(text):
    """(start, end) of every field of a well-formed text."""
    a = np.frombuffer(text, dtype=np.uint8)
    commas = np.flatnonzero(a == 44)
    ends = np.flatnonzero((a == 44) | (a == 10))
    return commas + 1, ends[np.searchsorted(ends, commas + 1)]


@pytest.mark.parametrize("nbins,n_rows", [(1, 40), (2, 40), (32, 60)])
def test_short_rows(dev, nbins, n_rows):
    rng = np.random.default_rng(100 + nbins)
    lines = synth_rows(rng, n_rows, nbins, lambda i: (i * 5) % 23)
    text = b"\n".join(lines) + b"\n"
    evals, enames, _, _ = check(dev, [text], nbins)
    assert evals.shape == (n_rows, nbins) and np.isnan(evals).any() and (evals == 0).any()
    if nbins == 32:
        assert len(text) > 3 * TILE                                   # more than one tile, rows across tile edges
    # the same rows as three units and with no slack: every row is allowed for and no more
    a, b = n_rows // 3, n_rows // 3 + 1
    check(dev, [b"\n".join(lines[:a]) + b"\n", b"\n".join(lines[a:b]), b"\n".join(lines[b:]) + b"\n"], nbins, cap=n_rows)


def test_k7_rows_of_many_tiles(dev):
    rng = np.random.default_rng(707)
    lines = synth_rows(rng, 2, 8192, lambda i: 20 + i)
    end = len(lines[0])
    lines[0] = b"p" * ((0 - end) % TILE) + lines[0]           # row 0's '\n' opens a tile: row 1 starts one byte in
    text = b"\n".join(lines) + b"\n"
    fs, fe = field_spans(text)
    assert fs.size == 2 * 8192 and all(len(x) > 20 * TILE for x in lines)
    over = (fs // TILE != (fe - 1) // TILE) & (fe - fs > 1)
    assert np.count_nonzero(over) >= 20                        # fields that start in one tile and end in the next
    assert np.count_nonzero(over & (fs % TILE >= TILE - 3)) >= 1    # one of them in a tile's last bytes
    evals, _, _, _ = check(dev, [text], 8192)
    assert evals.shape == (2, 8192)
    check(dev, [text[:-1]], 8192, cap=2)                      # the last row ended by the unit's end


def test_field_starts_at_every_offset(dev):
    """nbins = 3, names of 0..15 bytes: fields of 1 byte and of 24 bytes start at every offset of a 16-byte word."""
    long = [b"1.23456789012345678e-100", b"9.87654321098765432e+200", b"0.0000001234567890123456"]
    assert all(len(f) == 24 for f in long)
    lines = []
    for n in range(16):
        lines.append(k3_row(b"n" * n, [b"0", long[n % 3], b"7"]))
        lines.append(k3_row(b"n" * n, [long[n % 3], b"0", long[(n + 1) % 3]]))
    text, off = layout(lines)                                  # a unit each: every row starts a 16-byte word
    fs, fe = field_spans(text + b"\n")
    first = np.isin(fs - 1, np.flatnonzero(np.frombuffer(text, dtype=np.uint8) == 44)[::3])
    for size in (1, 24):
        assert set((fs[first & (fe - fs == size)] % 16).tolist()) == set(range(16)), size
    evals, _, _, _ = check(dev, lines, 3)
    assert evals.shape == (32, 3)
    check(dev, [b"\n".join(lines) + b"\n"], 3)                 # and back to back in one unit


def test_units_by_their_offsets(dev, tmp_path):
    from kf2vecfsw_amd import chunks as CH
    rng = np.random.default_rng(11)
    lines = synth_rows(rng, 12, 32, lambda i: 3 + i)
    with_nl = b"\n".join(lines[:3]) + b"\n"
    ragged = b"\n".join(lines[3:6])
    if len(ragged) % 16 == 0:
        ragged = b"x" + ragged
    full = b"\n".join(lines[6:8])
    full = b"n" * (-len(full) % 16) + full        # a multiple of 16: no padding, the next unit follows directly
    nxt = b"\n".join(lines[8:10]) + b"\n"
    units = [with_nl, ragged, full, nxt, b"", b"\n" * 40, b"\n\n" + lines[10] + b"\n\n\n" + lines[11]]
    assert len(ragged) % 16 and not ragged.endswith(b"\n")
    assert len(full) % 16 == 0 and not full.endswith(b"\n")
    text, off = layout(units)
    assert text[off[3] - 1] != 10 and text[off[3]: off[3] + 4] == lines[8][:4]     # two lines that would fuse
    _, _, erow0, _ = check(dev, units, 32)
    assert erow0 == [0, 3, 6, 8, 10, 10, 10, 12]
    # no unit at all, only empty ones, and units with no row allowed for
    assert run(dev, [], 32, cap=4)[2:] == ([0], (0, 0, 0, 0))
    assert run(dev, [b"", b""], 32, cap=4)[2:] == ([0, 0, 0], (0, 0, 0, 0))
    assert run(dev, [b"\n" * 5000], 32, cap=0)[2:] == ([0, 0], (0, 0, 0, 0))
    # the pieces of a larger file, cut at line starts by kf_line_pieces, as units of their own
    whole = b"\n".join(lines) + b"\n"
    path = tmp_path / "lib.kf"
    path.write_bytes(whole)
    pieces = CH.kf_line_pieces(str(path), 1000)
    assert len(pieces) >= 4
    evals, enames, erow0, _ = check(dev, [whole[a:e] for a, e in pieces], 32, cap=12)
    assert erow0[-1] == 12 and same_bits(evals, expected([whole], 32, 12)[0])


def adversarial_fields(n):
    """Decimals that sit at the rounding decisions: 19-digit prints of random doubles, 19-digit truncations of the
    midpoints of adjacent doubles and their neighbours in the last digit, exact ties, powers of ten."""
    rng = np.random.default_rng(1964)
    bits = rng.integers(1, 2046, size=n, dtype=np.uint64) << np.uint64(52) | rng.integers(0, 1 << 52, size=n, dtype=np.uint64)
    d = bits.view(np.float64)
    out = [("%.18e" % x).encode() for x in d[: n // 4].tolist()]
    ctx = decimal.Context(prec=1200)
    down = decimal.Context(prec=19, rounding=decimal.ROUND_DOWN)
    for x in d[n // 4: n // 2].tolist():
        y = float(np.nextafter(x, np.inf))
        t = down.plus(ctx.divide(ctx.add(decimal.Decimal(x), decimal.Decimal(y)), 2)).as_tuple()
        w = int("".join(map(str, t.digits))) * 10 ** (19 - len(t.digits))
        q = t.exponent - (19 - len(t.digits))
        out += [b"%de%d" % (w + dw, q) for dw in (-1, 0, 1)]
    for w in (9007199254740993, 9007199254740995, (1 << 53) + 1, (1 << 54) + 2, (1 << 54) + 6):
        out += [b"%d" % w, b"%d.0" % w]
        out += [b"%de%d" % (w, k) for k in range(-22, 23)]
        out += [b"%de-%d" % (w * 5 ** k, k) for k in range(1, 5) if w * 5 ** k < 10 ** 19]
    out += [b"1e%d" % q for q in range(-307, 309)]
    out += [b"2.2250738585072014e-308", b"1.7976931348623157e308", b"1.7976931348623158e308",
            b"1797693134862315807e290", b"2225073858507201384e-326"]
    return out


def test_adversarial_decimals(dev):
    fields = adversarial_fields(2400)
    fields += [b"0.5"] * (-len(fields) % 64)
    assert 3000 <= len(fields) <= 6000
    lines = [k3_row(b"r%d" % i, fields[i: i + 64]) for i in range(0, len(fields), 64)]
    evals, _, _, _ = check(dev, [b"\n".join(lines) + b"\n"], 64)
    assert np.isfinite(evals).all() and (evals > 0).all()


@pytest.mark.parametrize("val_bytes", [8, 4])
@pytest.mark.parametrize("scaler", [1.0, 1e4])
def test_output_types_and_scaler(dev, val_bytes, scaler):
    rng = np.random.default_rng(48)
    lines = synth_rows(rng, 9, 32, lambda i: 4)
    lines.append(k3_row(b"edge", [b"3.4028235677973366e+38", b"3.4028234e34", b"1e-46", b"1.7976931348623157e308"] * 8))
    evals, _, _, _ = check(dev, [b"\n".join(lines)], 32, scaler=scaler, val_bytes=val_bytes)
    assert evals.shape == (10, 32)


@pytest.mark.parametrize("what,row,code,col", MALFORMED, ids=[m[0] for m in MALFORMED])
def test_error_positions(dev, what, row, code, col):
    first = batch_around(k3_row(b"g", GOOD), 5, 4)
    units = [first, batch_around(row, 3, 2), batch_around(row, 4, 0, newline=False)]
    assert check(dev, units, 32)[3] == (code, 1, 3, col)
    assert check(dev, [first, units[2]], 32)[3] == (code, 1, 4, col)     # the row that errs ends at the unit's end
    assert check(dev, [row], 32)[3] == (code, 0, 0, col)


@pytest.mark.parametrize("what,row,col,value", FINE, ids=[m[0] for m in FINE])
def test_accepted_forms(dev, what, row, col, value):
    evals, enames, _, status = check(dev, [batch_around(row), batch_around(row, 0, 0, newline=False)], 32)
    assert status == (0, 0, 0, 0) and enames[3] == enames[6] == row.split(b",")[0]
    assert evals[3, col] == evals[6, col] == float(value if value is not None else row.split(b",")[1 + col])


def test_first_error_and_row_cap(dev):
    bad_a = next(m[1] for m in MALFORMED if m[0] == "1.2.3")
    bad_b = next(m[1] for m in MALFORMED if m[0] == "too few fields")
    bad_c = next(m[1] for m in MALFORMED if m[0] == "1e400")
    good = batch_around(k3_row(b"g", GOOD), 6, 5)                       # 12 rows
    two = batch_around(bad_a, 3, 2) + batch_around(bad_b, 3, 2)
    assert check(dev, [good, two], 32)[3] == (3, 1, 3, 5)                # the lower offset of two errors
    assert check(dev, [good, batch_around(bad_b, 3, 2) + batch_around(bad_a, 3, 2)], 32)[3] == (1, 1, 3, 31)
    assert check(dev, [good, batch_around(bad_c, 3, 2), batch_around(bad_a, 0, 0)], 32)[3] == (7, 1, 3, 20)
    assert check(dev, [good, good], 32, cap=24)[3] == (0, 0, 0, 0)
    assert check(dev, [good, good], 32, cap=23)[3] == (5, 1, 11, 0)      # one below the true row count
    assert check(dev, [good, good], 32, cap=12)[3] == (5, 1, 0, 0)
    assert check(dev, [good, two], 32, cap=15)[3] == (5, 1, 3, 0)        # the row that errs is not read
    assert check(dev, [good, two], 32, cap=16)[3] == (3, 1, 3, 5)


@pytest.mark.parametrize("what", ["random bytes", "commas only", "digits only", "digits, points and e"])
def test_any_bytes_stay_inside_the_buffers(dev, what):
    rng = np.random.default_rng(64)
    n = 64 << 10
    if what == "random bytes":
        unit = rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()
    elif what == "commas only":
        unit = b"," * n
    elif what == "digits only":
        unit = b"g," + b"0" * (n - 3) + b"7"          # 64 KiB of leading zeros and one digit: fine; the row is short
    else:
        unit = bytes(rng.choice(list(b",\n,0.e1-9n"), size=n).astype(np.uint8))
    good = b"\n".join(synth_rows(rng, 4, 32, lambda i: 5)) + b"\n"
    for units in ([unit], [good, unit, good]):
        for cap in (0, 1, 7, 3000):
            assert check(dev, units, 32, cap=cap)[3][0] != 0
    if what == "commas only":
        assert check(dev, [unit], 32, cap=7)[3] == (3, 0, 0, 0)
    if what == "digits only":
        assert check(dev, [unit], 32, cap=7)[3] == (1, 0, 0, 1)
        evals = check(dev, [unit], 1, cap=7)[0]
        assert evals.tolist() == [[7.0]]
        assert check(dev, [b"g,0." + b"0" * (n - 5) + b"7"], 1, cap=7)[3] == (7, 0, 0, 0)   # 7e-65531


def test_wrapper_and_refusal_text(dev):
    import torch
    from kf2vecfsw_amd import counter as C
    from kf2vecfsw_amd import features as F
    rng = np.random.default_rng(5)
    lines = [k3_row(b"", [b"0"] * 32)] * 3 + synth_rows(rng, 9, 32, lambda i: 1 + i)   # the shortest rows there are
    units = [b"\n".join(lines[:6]) + b"\n", b"\n".join(lines[6:])]
    text, off = layout(units)
    d = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).to(dev)
    for dtype in (torch.float64, torch.float32):
        vals, spans, row0, status = F.parse_kf_floats(d, off, 32, scaler=100.0, dtype=dtype)
        assert vals.dtype == dtype and vals.shape[1] == 32 and 12 <= vals.shape[0] <= len(text) // 64 + 2
        assert spans.shape == (vals.shape[0], 2) and spans.dtype == torch.int32
        assert C.parsed_to_host(row0, status).tolist() == [0, 6, 12]
        want = expected(units, 32, 12)[0] * 100.0
        got = vals[:12].cpu().numpy()
        assert np.array_equal(np.isnan(got), np.isnan(want))
        with np.errstate(over="ignore"):
            assert np.array_equal(np.nan_to_num(got), np.nan_to_num(want.astype(got.dtype)))
    units[1] += b",1"
    text, off = layout(units)
    d = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).to(dev)
    _, _, row0, status = F.parse_kf_floats(d, torch.from_numpy(off).to(dev), 32)
    with pytest.raises(ValueError, match=r"b\.kf: row 45, column 32: too many fields"):
        C.parsed_to_host(row0, status, ["a.kf", "b.kf"], [0, 40])
    units[1] = units[1][:-2].replace(b",0.0", b",1e-320", 1)
    assert b"1e-320" in units[1]
    text, off = layout(units)
    d = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).to(dev)
    _, _, row0, status = F.parse_kf_floats(d, off, 32)
    with pytest.raises(ValueError, match=r"unit 1: row \d, column \d+: magnitude outside the normal float64 range"):
        C.parsed_to_host(row0, status)


# ---------------------------------------------------------------- a directory
def toy_fasta_dir(root):
    inp = root / "fna"
    inp.mkdir()
    for d in ("train_tree_fna", "test_fna"):
        for f in sorted(os.listdir(os.path.join(TOY, d))):
            (inp / f[:-3]).write_bytes(gzip.open(os.path.join(TOY, d, f)).read())
    (inp / "Empty.fna").write_bytes(b">nothing\nNNNNNN\n")            # a genome without a k-mer
    return inp


@pytest.fixture(scope="module")
def toy_counts(dev, tmp_path_factory):
    """(fasta dir, sample names in file order, {k: counts int32 [G, nbins] of KmerCounter.count on the files})."""
    from kf2vecfsw_amd import counter as C
    inp = toy_fasta_dir(tmp_path_factory.mktemp("kf_float_library"))
    files = sorted(os.listdir(inp))
    counts = {}
    for k in (7, 3):
        hb = C.pack_files([str(inp / f) for f in files])
        counts[k] = C.KmerCounter(k, dev).count(C.to_device(hb, dev))[0]
    return inp, [f.rsplit(".f", 1)[0] for f in files], counts


CLI_CASES = [(7, False, False), (3, True, False), (3, False, True), (3, True, True)]


@pytest.mark.parametrize("k,pseudo,raw", CLI_CASES, ids=["k7", "k3_pseudo", "k3_raw", "k3_pseudo_raw"])
def test_directory_equals_counter_features(dev, toy_counts, tmp_path, k, pseudo, raw):
    import torch
    from kf2vecfsw_amd import counter as C
    from kf2vecfsw_amd import features as F
    from kf2vecfsw_amd import main as M
    inp, samples, counts = toy_counts
    out = tmp_path / "kf"
    out.mkdir()
    M.main(["get_frequencies", "-input_dir", str(inp), "-output_dir", str(out), "-k", str(k), "-p", "4"]
           + (["-pseudocount"] if pseudo else []) + (["-raw_cnt"] if raw else []))
    order = sorted(samples)
    assert sorted(f[:-3] for f in os.listdir(out)) == order and "Empty" in order
    idx = torch.tensor([samples.index(s) for s in order], device=dev)
    for scaler, dtype in ((1.0, torch.float64), (1e4, torch.float64), (1e4, torch.float32)):
        store = F.features_from_kf(str(out), k, dev, scaler=scaler, dtype=dtype)
        assert store.names == order and store.files == order and store.k == k
        assert store.file_row0.tolist() == list(range(len(order) + 1))
        want = C.features(counts[k][idx], pseudo, raw, scaler).to(dtype)
        assert store.values.dtype == dtype and store.values.shape == want.shape and store.values.is_contiguous()
        nan = torch.isnan(want)
        assert torch.equal(torch.isnan(store.values), nan)
        assert torch.equal(torch.where(nan, 0, store.values), torch.where(nan, 0, want))       # bit for bit: no zero is negative
        e = order.index("Empty")
        assert bool(nan[e].all()) != (pseudo or raw) and not bool(nan[:e].any()) and not bool(nan[e + 1:].any())
    # the order given, a file named twice, and a missing file refused before anything is read
    pick = [order[3], order[0], order[3]]
    store = F.features_from_kf(str(out), k, dev, samples=pick)
    assert store.names == pick and torch.equal(store.values[0], store.values[2])
    assert torch.equal(torch.nan_to_num(store.values[1]), torch.nan_to_num(C.features(counts[k][idx[:1]], pseudo, raw)[0]))
    with pytest.raises(ValueError, match=r"nowhere\.kf"):
        F.features_from_kf(str(out), k, dev, samples=[order[0], "nowhere"])


def test_concatenated_library_in_pieces(dev, toy_counts, tmp_path, monkeypatch):
    """One file of every genome's row, blank lines between some, read whole and in pieces over many batches."""
    import torch
    from kf2vecfsw_amd import chunks as CH
    from kf2vecfsw_amd import counter as C
    from kf2vecfsw_amd import features as F
    from kf2vecfsw_amd import main as M
    inp, samples, counts = toy_counts
    out, lib = tmp_path / "kf", tmp_path / "lib"
    out.mkdir()
    lib.mkdir()
    M.main(["get_frequencies", "-input_dir", str(inp), "-output_dir", str(out), "-k", "7", "-p", "4"])
    order = sorted(samples)
    rows = [(out / (s + ".kf")).read_bytes() for s in order]
    assert all(r.endswith(b"\n") and r.count(b"\n") == 1 for r in rows)
    (lib / "all.kf").write_bytes(b"".join(rows[:3]) + b"\n\n" + b"".join(rows[3:])[:-1])      # no final newline
    (lib / "blank.kf").write_bytes(b"\n")
    (lib / "one.kf").write_bytes(rows[1])
    idx = torch.tensor([samples.index(s) for s in order + [order[1]]], device=dev)
    want = torch.nan_to_num(C.features(counts[7][idx]), nan=-1.0)
    whole = F.features_from_kf(str(lib), 7, dev)
    assert whole.names == order + [order[1]] and whole.files == ["all", "blank", "one"]
    assert whole.file_row0.tolist() == [0, len(order), len(order), len(order) + 1]
    assert torch.equal(torch.nan_to_num(whole.values, nan=-1.0), want)
    monkeypatch.setattr(CH, "KF_PIECE_BYTES", 64 << 10)
    calls = []
    real = F.parse_kf_floats

    def counted(data, off, *a, **kw):
        calls.append(len(off) - 1)
        return real(data, off, *a, **kw)
    monkeypatch.setattr(F, "parse_kf_floats", counted)
    assert len(CH.kf_line_pieces(str(lib / "all.kf"))) >= len(order) - 1          # a row is above 64 KiB
    for gb, least in (((64 << 10) / (1 << 30), len(order) - 2), ((512 << 10) / (1 << 30), 2)):
        calls.clear()
        got = F.features_from_kf(str(lib), 7, dev, batch_gb=gb)
        assert len(calls) >= least
        assert got.names == whole.names and got.file_row0.tolist() == whole.file_row0.tolist()
        assert torch.equal(torch.nan_to_num(got.values, nan=-1.0), want)
    # a refusal names the file and the row within the file, whichever piece and batch hold it
    f = rows[4].split(b",")
    f[1 + 4097] = b"-" + f[1 + 4097]
    (lib / "all.kf").write_bytes(b"".join(rows[:4]) + b",".join(f) + b"".join(rows[5:]))
    for gb in (1.0, (64 << 10) / (1 << 30), (512 << 10) / (1 << 30)):
        with pytest.raises(ValueError, match=r"all\.kf: row 4, column 4097: malformed field \(kf_parse_kf_floats status 3\)"):
            F.features_from_kf(str(lib), 7, dev, batch_gb=gb)
