"""GPU tests of the `.kf` reader: kf_parse_kf_rows against its host statement
(chunks.parse_kf_rows_host) bit for bit -- rows, every unit's row range and, for
text it refuses, code, unit, row and column -- with sentinel rows before and
after d_rows that must stay intact whatever the bytes; chunk_store_from_kf
against chunk_store on the FASTA files its directory was made from."""
import gzip
import os

import numpy as np
import pytest

from conftest import TOY
from test_host_kf_parse import FINE, GOOD, MALFORMED, batch_around, k3_row

pytestmark = pytest.mark.gpu

TILE = 4096
GUARD = 3                 # sentinel rows on either side of d_rows
SENTINEL = 0x5A5B         # no count of the tests' rows


@pytest.fixture(scope="module")
def dev(native):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu tests need an MI355X")
    return torch.device("cuda:0")


def layout(units, pad=True):
    """The units back to back as pack_ranges lays them out: 16-byte aligned, '\\n' padding."""
    buf, off = bytearray(), [0]
    for u in units:
        buf += u
        if pad:
            buf += b"\n" * (-len(buf) % 16)
        off.append(len(buf))
    return bytes(buf), np.asarray(off, dtype=np.int64)


def expected(units, nbins, cap):
    """The statement, unit after unit: (rows, unit_row0, (code, unit, row, column))."""
    from kf2vecfsw_amd import chunks as CH
    parts, row0 = [], [0]
    for u, text in enumerate(units):
        rows, (code, r, c) = CH.parse_kf_rows_host(text, nbins, cap - row0[-1])
        if code:
            return None, None, (code, u, r, c)
        parts.append(rows)
        row0.append(row0[-1] + rows.shape[0])
    return np.concatenate(parts) if parts else np.zeros((0, nbins), np.uint16), row0, (0, 0, 0, 0)


def run(dev, units, nbins, cap=None, slack=2):
    """kf_parse_kf_rows on the units, d_rows between sentinel rows: (rows uint16
    [cap, nbins], unit_row0, status) on the host, after the sentinels were found intact."""
    import torch
    from kf2vecfsw_amd import _native as N
    text, off = layout(units)
    if cap is None:
        cap = sum(len([ln for ln in u.split(b"\n") if ln]) for u in units) + slack
    d_text = torch.from_numpy(np.frombuffer(text + b"\0" * 16, dtype=np.uint8).copy()).to(dev)
    d_off = torch.from_numpy(off).to(dev)
    buf = torch.full((cap + 2 * GUARD, nbins), SENTINEL, dtype=torch.int16, device=dev)
    row0 = torch.full((len(units) + 3,), -7, dtype=torch.int64, device=dev)
    status = torch.full((6,), -7, dtype=torch.int64, device=dev)
    need = N.lib().kf_parse_kf_scratch_bytes(len(text), len(units), cap)
    scratch = torch.empty(need // 8, dtype=torch.int64, device=dev)
    N.check(N.lib().kf_parse_kf_rows(d_text.data_ptr(), d_off.data_ptr(), len(units), len(text), nbins, cap,
                                     buf[GUARD:].data_ptr(), row0[1:].data_ptr(), status[1:].data_ptr(),
                                     scratch.data_ptr(), need, torch.cuda.current_stream(dev).cuda_stream),
            "kf_parse_kf_rows")
    host = buf.cpu().numpy().view(np.uint16)
    assert (host[:GUARD] == SENTINEL).all() and (host[GUARD + cap:] == SENTINEL).all(), "written outside d_rows"
    row0, status = row0.cpu().numpy(), status.cpu().numpy()
    assert row0[0] == row0[-1] == -7 and status[0] == status[-1] == -7, "written outside unit_row0 or status"
    return host[GUARD: GUARD + cap], row0[1:-1].tolist(), tuple(int(x) for x in status[1:5])


def check(dev, units, nbins, cap=None):
    """The kernel equals the statement; returns the statement's (rows, unit_row0, status)."""
    if cap is None:
        cap = sum(len([ln for ln in u.split(b"\n") if ln]) for u in units) + 2
    rows, row0, status = run(dev, units, nbins, cap)
    erows, erow0, estatus = expected(units, nbins, cap)
    assert status == estatus
    if estatus[0] == 0:
        assert row0 == erow0
        assert np.array_equal(rows[: erow0[-1]], erows)
        assert (rows[erow0[-1]:] == SENTINEL).all()       # no row past the last is touched
    return erows, erow0, estatus


VALUES = [0, 9, 10, 99, 100, 999, 1000, 9999, 10000, 65535]


def synth_rows(rng, n, nbins, name_len):
    out = []
    for i in range(n):
        name = bytes(rng.choice(list(b"abcXYZ019._-"), size=name_len(i)).astype(np.uint8))
        out.append(name + b"".join(b",%d.0" % v for v in rng.choice(VALUES, size=nbins)))
    return out


def starts_and_fields(text):
    """Offsets of the row starts and (start, end) of every field of a well-formed text."""
    a = np.frombuffer(text, dtype=np.uint8)
    nl = np.flatnonzero(a == 10)
    row_starts = np.concatenate([[0], nl + 1])
    row_starts = row_starts[(row_starts < a.size)]
    row_starts = row_starts[a[row_starts] != 10]
    commas = np.flatnonzero(a == 44)
    ends = np.flatnonzero((a == 44) | (a == 10))
    return row_starts, commas + 1, ends[np.searchsorted(ends, commas + 1)]


def test_k3_every_offset_and_tile_edges(dev):
    rng = np.random.default_rng(303)
    lines = synth_rows(rng, 200, 32, lambda i: 1 + (i * 37 + i // 16) % 300)
    text = b"\n".join(lines) + b"\n"
    rs, fs, fe = starts_and_fields(text)
    assert rs.size == 200 and fs.size == 200 * 32
    assert set((fe - fs).tolist()) == {3, 4, 5, 6, 7}
    assert set((rs % 16).tolist()) == set(range(16)) and set((fs % 16).tolist()) == set(range(16))
    assert len(text) > 10 * TILE
    assert np.count_nonzero(fs // TILE != (fe - 1) // TILE) >= 3             # fields across a tile edge
    rows_over = np.count_nonzero(rs[:-1] // TILE != (rs[1:] - 2) // TILE)
    assert rows_over >= 10                                                    # rows across a tile edge
    erows, _, _ = check(dev, [text], 32)
    assert erows.shape == (200, 32) and set(np.unique(erows).tolist()) == set(VALUES)
    # the same rows as three units and with no slack: every row is allowed for and no more
    check(dev, [b"\n".join(lines[:70]) + b"\n", b"\n".join(lines[70:71]), b"\n".join(lines[71:]) + b"\n"], 32, cap=200)


def test_k7_rows_of_many_tiles(dev):
    rng = np.random.default_rng(707)
    lines = synth_rows(rng, 5, 8192, lambda i: 20 + i)

    def pad_to(i, want):
        """Pad row i's name so that its '\\n' lies at offset `want` mod 4096."""
        end = sum(len(x) + 1 for x in lines[:i]) + len(lines[i])
        lines[i] = b"p" * ((want - end) % TILE) + lines[i]
    pad_to(1, 0)               # row 1 ends exactly on a tile edge: its '\n' opens the next tile
    pad_to(3, TILE - 1)        # row 3's '\n' closes a tile: row 4 starts exactly on the edge
    text = b"\n".join(lines) + b"\n"
    nl = np.flatnonzero(np.frombuffer(text, dtype=np.uint8) == 10)
    assert nl[1] % TILE == 0 and nl[3] % TILE == TILE - 1 and (nl[3] + 1) % TILE == 0
    assert all(len(x) >= 8 * TILE for x in lines)
    erows, _, _ = check(dev, [text], 8192)
    assert erows.shape == (5, 8192)
    check(dev, [text[:-1]], 8192, cap=5)          # the last row ended by the unit's end


def test_units_by_their_offsets(dev):
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
    erows, erow0, _ = check(dev, units, 32)
    assert erow0 == [0, 3, 6, 8, 10, 10, 10, 12]
    # no unit at all, only empty ones, and units with no row allowed for
    assert run(dev, [], 32, cap=4)[1:] == ([0], (0, 0, 0, 0))
    assert run(dev, [b"", b""], 32, cap=4)[1:] == ([0, 0, 0], (0, 0, 0, 0))
    assert run(dev, [b"\n" * 5000], 32, cap=0)[1:] == ([0, 0], (0, 0, 0, 0))


@pytest.mark.parametrize("what", ["random bytes", "commas only", "digits only", "newlines and commas"])
def test_any_bytes_stay_inside_the_buffers(dev, what):
    rng = np.random.default_rng(64)
    n = 64 << 10
    if what == "random bytes":
        unit = rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()
    elif what == "commas only":
        unit = b"," * n
    elif what == "digits only":
        unit = b"w," + b"0" * (n - 2)             # one field of 64 KiB of zeros is fine; the row is short
    else:
        unit = bytes(rng.choice(list(b",\n,0."), size=n).astype(np.uint8))
    good = b"\n".join(synth_rows(rng, 4, 32, lambda i: 5)) + b"\n"
    for units in ([unit], [good, unit, good]):
        for cap in (0, 1, 7, 3000):
            status = check(dev, units, 32, cap=cap)[2]
            assert status[0] != 0
    if what == "commas only":
        assert check(dev, [unit], 32, cap=7)[2] == (3, 0, 0, 0)
    if what == "digits only":
        assert check(dev, [unit], 32, cap=7)[2] == (1, 0, 0, 1)
        assert check(dev, [unit], 1, cap=7)[2] == (0, 0, 0, 0)


@pytest.mark.parametrize("what,row,code,col", MALFORMED, ids=[m[0] for m in MALFORMED])
def test_error_positions(dev, what, row, code, col):
    first = batch_around(k3_row(b"w", GOOD), 5, 4)
    units = [first, batch_around(row, 3, 2), batch_around(row, 4, 0, newline=False)]
    assert check(dev, units, 32)[2] == (code, 1, 3, col)
    assert check(dev, [first, units[2]], 32)[2] == (code, 1, 4, col)     # the row that errs ends at the unit's end
    assert check(dev, [row], 32)[2] == (code, 0, 0, col)


@pytest.mark.parametrize("what,row,col,value", FINE, ids=[m[0] for m in FINE])
def test_accepted_forms(dev, what, row, col, value):
    erows, _, status = check(dev, [batch_around(row), batch_around(row, 0, 0, newline=False)], 32)
    assert status == (0, 0, 0, 0) and erows[3, col] == value and erows[6, col] == value


def test_first_error_and_row_cap(dev):
    bad_a, bad_b = MALFORMED[3][1], MALFORMED[0][1]
    good = batch_around(k3_row(b"w", GOOD), 6, 5)                       # 12 rows
    two = batch_around(bad_a, 3, 2) + batch_around(bad_b, 3, 2)
    assert check(dev, [good, two], 32)[2] == (3, 1, 3, 5)                # the lower offset of two errors
    assert check(dev, [good, batch_around(bad_b, 3, 2) + batch_around(bad_a, 3, 2)], 32)[2] == (1, 1, 3, 31)
    assert check(dev, [good, batch_around(bad_b, 3, 2), batch_around(bad_a, 0, 0)], 32)[2] == (1, 1, 3, 31)
    assert check(dev, [good, good], 32, cap=24)[2] == (0, 0, 0, 0)
    assert check(dev, [good, good], 32, cap=23)[2] == (5, 1, 11, 0)      # one below the true row count
    assert check(dev, [good, good], 32, cap=12)[2] == (5, 1, 0, 0)
    assert check(dev, [good, two], 32, cap=15)[2] == (5, 1, 3, 0)        # the row that errs is not read
    assert check(dev, [good, two], 32, cap=16)[2] == (3, 1, 3, 5)


def test_wrapper_default_cap_and_refusal_text(dev):
    import torch
    from kf2vecfsw_amd import counter as C
    rng = np.random.default_rng(5)
    lines = [b"" + ln[ln.index(b","):] for ln in synth_rows(rng, 9, 32, lambda i: 1)]
    lines = [b",".join([b""] + [b"0"] * 32)] * 3 + lines                # the shortest rows there are: 64 bytes
    units = [b"\n".join(lines[:6]) + b"\n", b"\n".join(lines[6:])]
    text, off = layout(units)
    d = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).to(dev)
    rows, row0, status = C.parse_kf_rows(d, off, 32)
    assert rows.dtype == torch.int16 and rows.shape[1] == 32 and 12 <= rows.shape[0] <= len(text) // 64 + 2
    assert C.parsed_to_host(row0, status).tolist() == [0, 6, 12]
    assert np.array_equal(rows[:12].cpu().numpy().view(np.uint16), expected(units, 32, 12)[0])
    units[1] = units[1].replace(b",65535.0", b",65536.0", 1) if b",65535.0" in units[1] else units[1] + b",1"
    text, off = layout(units)
    d = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).to(dev)
    _, row0, status = C.parse_kf_rows(d, torch.from_numpy(off).to(dev), 32)
    _, _, (code, u, r, c) = expected(units, 32, 100)
    assert code in (2, 4) and u == 1
    with pytest.raises(ValueError, match=r"b\.kf: row %d, column %d: " % (r + 40, c)):
        C.parsed_to_host(row0, status, ["a.kf", "b.kf"], [0, 40])
    with pytest.raises(ValueError, match=r"unit 1: row %d, column %d: " % (r, c)):
        C.parsed_to_host(row0, status)


# ---------------------------------------------------------------- a directory
@pytest.fixture(scope="module")
def library(dev, tmp_path_factory):
    """get_chunks -k 7 of the toy train_tree_fna: (fasta dir, kf dir, chunk_store of the FASTA files)."""
    from kf2vecfsw_amd import chunks as CH
    from kf2vecfsw_amd import main as M
    root = tmp_path_factory.mktemp("kf_library")
    inp, out = root / "fna", root / "kf"
    inp.mkdir()
    out.mkdir()
    src = os.path.join(TOY, "train_tree_fna")
    for f in sorted(os.listdir(src)):
        (inp / f[:-3]).write_bytes(gzip.open(os.path.join(src, f)).read())
    M.main(["get_chunks", "-input_dir", str(inp), "-output_dir", str(out), "-k", "7"])
    return str(inp), str(out), CH.chunk_store(str(inp), 7, dev)


def same_store(got, ref, order):
    """`got` holds the genomes `order` of `ref`, in that order, bit for bit."""
    assert got.samples == order and got.k == ref.k
    idx = [ref.samples.index(s) for s in order]
    n = [int(ref.row0[i + 1] - ref.row0[i]) for i in idx]
    assert got.row0.dtype == np.int64 and got.row0.tolist() == np.cumsum([0] + n).tolist()
    exp = np.concatenate([ref.counts[int(ref.row0[i]): int(ref.row0[i + 1])].cpu().numpy() for i in idx])
    assert got.counts.dtype == ref.counts.dtype and got.counts.is_contiguous()
    assert got.counts.shape == exp.shape and np.array_equal(got.counts.cpu().numpy(), exp)


def test_round_trip_equals_chunk_store(dev, library):
    from kf2vecfsw_amd import chunks as CH
    inp, out, ref = library
    order = sorted(ref.samples)
    assert len(order) >= 3 and sorted(f[:-3] for f in os.listdir(out) if f.endswith(".kf")) == order
    got = CH.chunk_store_from_kf(out, 7, dev)
    same_store(got, ref, order)
    assert got.excluded == {}
    # the trainer's batches from either store are the same tensors
    idx = np.asarray([0, 2, 1, 1, 0, 2, 2])
    za, ya = got.batch(idx, np.random.RandomState(77))
    zb, yb = ref.batch(np.asarray([ref.samples.index(order[i]) for i in idx]), np.random.RandomState(77))
    assert za.shape == (7, 2 * 8192) and bool((za == zb).all()) and ya.tolist() == idx.tolist()


def test_reference_chunk_files(dev, tmp_path):
    """A library the reference wrote (its toy train_tree_chunks): the store equals a split(",") reading."""
    from kf2vecfsw_amd import chunks as CH
    src = os.path.join(TOY, "train_tree_chunks")
    exp = []
    for f in sorted(os.listdir(src)):
        text = gzip.open(os.path.join(src, f)).read()
        (tmp_path / f[:-3]).write_bytes(text)
        exp.append(np.asarray([ln.split(",")[1:] for ln in text.decode().splitlines()]).astype(np.float64))
    got = CH.chunk_store_from_kf(str(tmp_path), 7, dev)
    assert got.samples == sorted(f[:-6] for f in os.listdir(src))
    assert got.row0.tolist() == np.cumsum([0] + [e.shape[0] for e in exp]).tolist()
    assert np.array_equal(got.counts.cpu().numpy().view(np.uint16), np.concatenate(exp).astype(np.uint16))


def test_pieces_and_batches(dev, library, monkeypatch, tmp_path):
    """64 KiB pieces and 64 KiB batches: every file is many pieces over many batches."""
    from kf2vecfsw_amd import chunks as CH
    from kf2vecfsw_amd import counter as C
    inp, out, ref = library
    order = sorted(ref.samples)
    monkeypatch.setattr(CH, "KF_PIECE_BYTES", 64 << 10)
    calls = []
    real = C.parse_kf_rows

    def counted(data, off, *a, **kw):
        calls.append(len(off) - 1)
        return real(data, off, *a, **kw)
    monkeypatch.setattr(C, "parse_kf_rows", counted)
    assert all(len(CH.kf_line_pieces(os.path.join(out, s + ".kf"))) > 20 for s in order)
    got = CH.chunk_store_from_kf(out, 7, dev, batch_gb=(64 << 10) / (1 << 30))
    assert len(calls) > 60
    same_store(got, ref, order)
    calls.clear()
    same_store(CH.chunk_store_from_kf(out, 7, dev, batch_gb=(1 << 20) / (1 << 30)), ref, order)   # several pieces a batch
    assert len(calls) > 5 and max(calls) > 4
    # a refusal names the file and the row within the file, whichever piece and batch hold it
    text = open(os.path.join(out, order[1] + ".kf"), "rb").read()
    lines = text.split(b"\n")
    f = lines[41].split(b",")
    f[1 + 4097] = b"7e0"
    lines[41] = b",".join(f)
    for s in order:
        (tmp_path / (s + ".kf")).write_bytes(b"\n".join(lines) if s == order[1]
                                             else open(os.path.join(out, s + ".kf"), "rb").read())
    for gb in (1.0, (64 << 10) / (1 << 30), (1 << 20) / (1 << 30)):
        with pytest.raises(ValueError, match=order[1] + r"\.kf: row 41, column 4097: malformed field"):
            CH.chunk_store_from_kf(str(tmp_path), 7, dev, batch_gb=gb)


def test_samples_argument(dev, library, monkeypatch, tmp_path):
    from kf2vecfsw_amd import chunks as CH
    from kf2vecfsw_amd import counter as C
    inp, out, ref = library
    order = sorted(ref.samples)
    pick = [order[2], order[0]]
    same_store(CH.chunk_store_from_kf(out, 7, dev, samples=pick), ref, pick)
    # a zero-byte file and one of empty lines are excluded; the others keep their places
    for s in order:
        os.symlink(os.path.join(out, s + ".kf"), tmp_path / (s + ".kf"))
    (tmp_path / "A_empty.kf").write_bytes(b"")
    (tmp_path / "blank.kf").write_bytes(b"\n\n")
    got = CH.chunk_store_from_kf(str(tmp_path), 7, dev)
    same_store(got, ref, order)
    assert got.excluded == {"A_empty": "none", "blank": "none"}
    got = CH.chunk_store_from_kf(str(tmp_path), 7, dev, samples=["A_empty", order[1], "blank"])
    same_store(got, ref, [order[1]])
    assert got.excluded == {"A_empty": "none", "blank": "none"}
    only = CH.chunk_store_from_kf(str(tmp_path), 7, dev, samples=["A_empty"])
    assert only.samples == [] and only.counts.shape == (0, 8192) and only.row0.tolist() == [0]

    # a missing file is refused before anything is read
    def no_read(*a, **kw):
        raise AssertionError("a file was read before the refusal")
    monkeypatch.setattr(C, "pack_ranges", no_read)
    with pytest.raises(ValueError, match=r"nowhere\.kf"):
        CH.chunk_store_from_kf(out, 7, dev, samples=[order[0], "nowhere"])
