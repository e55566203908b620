"""GPU tests of the `.kf` formatter: kf_format_kf_rows16 against its host
statement (chunks.format_rows_host, i.e. the C++ formatter of the writer) byte
for byte -- the text, every row's offset and the status -- with d_text between
sentinel bytes and d_row_off and d_status between sentinel words that must stay
intact whatever the input; the text read back by kf_parse_kf_rows; and the
get_chunks CLI, which formats on the device, against kf_write_kf_segments16 on
chunk_store's rows."""
import ctypes
import gzip
import json
import os

import numpy as np
import pytest

from conftest import TOY

pytestmark = pytest.mark.gpu

TILE = 2048               # cells per workgroup
STAGE = 20 << 10          # bytes of LDS stage: a tile's text above it leaves in several windows
GUARD = 64                # sentinel bytes on either side of d_text
SENTINEL = 0xA7
VALUES = [0, 1, 9, 10, 99, 100, 999, 1000, 9999, 10000, 65535]


@pytest.fixture(scope="module")
def dev(native):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu tests need an MI355X")
    return torch.device("cuda:0")


def run(dev, rows, prefixes, rpre, rpos, win_len, pseudo, cap, shift=0, pre_off=None):
    """kf_format_kf_rows16 with d_text (at `shift` bytes past a 256-byte boundary)
    between sentinel bytes and d_row_off, d_status between sentinel words: (text
    bytes [cap], row_off, status) on the host, after the sentinels were found intact."""
    import torch
    from kf2vecfsw_amd import _native as N
    rows = np.ascontiguousarray(rows, dtype=np.uint16)
    n, nbins = rows.shape
    d_rows = torch.from_numpy(rows.view(np.int16).copy()).to(dev) if n else torch.zeros(8, dtype=torch.int16, device=dev)
    blob = b"".join(prefixes)
    if pre_off is None:
        pre_off = np.cumsum([0] + [len(p) for p in prefixes])
    d_pre = torch.from_numpy(np.frombuffer(blob + b"\0", dtype=np.uint8).copy()).to(dev)
    d_pre_off = torch.from_numpy(np.asarray(pre_off, dtype=np.int64)).to(dev)
    d_rpre = torch.from_numpy(np.asarray(list(rpre) + [0], dtype=np.uint32).view(np.int32).copy()).to(dev)
    d_rpos = torch.from_numpy(np.asarray(list(rpos) + [0], dtype=np.uint64).view(np.int64).copy()).to(dev)
    buf = torch.full((512 + shift + cap + GUARD,), SENTINEL, dtype=torch.uint8, device=dev)
    t0 = (-buf.data_ptr()) % 256 + 256 + shift            # d_text = shift mod 256, sentinels on either side
    assert t0 >= GUARD and t0 + cap + GUARD <= buf.numel()
    row_off = torch.full((n + 3,), -7, dtype=torch.int64, device=dev)
    status = torch.full((6,), -7, dtype=torch.int64, device=dev)
    need = N.lib().kf_format_kf_scratch_bytes(n, nbins)
    scratch = torch.empty(need // 8 + 1, dtype=torch.int64, device=dev)
    N.check(N.lib().kf_format_kf_rows16(d_rows.data_ptr(), n, nbins, d_pre.data_ptr(), d_pre_off.data_ptr(),
                                        len(prefixes), d_rpre.data_ptr(), d_rpos.data_ptr(), win_len, int(pseudo),
                                        buf.data_ptr() + t0, cap, row_off[1:].data_ptr(), status[1:].data_ptr(),
                                        scratch.data_ptr(), need, torch.cuda.current_stream(dev).cuda_stream),
            "kf_format_kf_rows16")
    host = buf.cpu().numpy()
    assert (host[:t0] == SENTINEL).all() and (host[t0 + cap:] == SENTINEL).all(), "written outside d_text"
    row_off, status = row_off.cpu().numpy(), status.cpu().numpy()
    assert row_off[0] == row_off[-1] == -7 and status[0] == status[-1] == -7, "written outside row_off or status"
    return host[t0: t0 + cap].tobytes(), row_off[1:-1], tuple(int(x) for x in status[1:5])


def check(dev, rows, prefixes, rpre, rpos, win_len, pseudo, shift=0):
    """The kernel equals the statement with cap_bytes equal to the text's size; returns the text."""
    from kf2vecfsw_amd import chunks as CH
    exp, eoff = CH.format_rows_host(rows, prefixes, rpre, rpos, win_len, pseudo)
    got, off, status = run(dev, rows, prefixes, rpre, rpos, win_len, pseudo, len(exp), shift)
    assert status == (0, len(exp), 0, 0)
    assert off.tolist() == eoff.tolist()
    assert got == exp
    return exp


def plain(n):
    """Names of n rows from one short prefix: (prefixes, row_prefix, row_start)."""
    return [b"w_"], [0] * n, [10 * i for i in range(n)]


@pytest.mark.parametrize("pseudo", [False, True])
def test_digits_and_forms(dev, pseudo):
    rng = np.random.default_rng(32)
    n = 200                                               # 6,400 cells: four tiles, rows of all forms in each
    rows = rng.choice(VALUES, size=(n, 32)).astype(np.uint16)
    rows[0::3] = 0                                        # only zero columns
    nz = rng.choice(VALUES[1:], size=(n, 32)).astype(np.uint16)
    rows[1::3] = nz[1::3]                                 # no zero column
    mixed = rows[2::3]
    mixed[:, 0] = 0                                       # a zero column and a non-zero one
    mixed[:, 5] = 65535
    rows[2::3] = mixed
    assert set(np.unique(rows).tolist()) == set(VALUES)
    text = check(dev, rows, *plain(n), 10000, pseudo)
    lines = text.split(b"\n")
    if pseudo:
        assert lines[0].endswith(b",0.5,0.5") and b",65535.5," in lines[2]
    else:
        assert lines[0].endswith(b",0,0") and b"." not in lines[1] and b",65535.0," in lines[2]
        assert lines[3].endswith(b",0,0") and b"." not in lines[4] and lines[5].count(b".0") == 32


@pytest.mark.parametrize("nbins,n", [(1, 5000), (2, 3000), (136, 100), (8192, 5), (131072, 3)])
def test_column_counts(dev, nbins, n):
    rng = np.random.default_rng(nbins)
    rows = rng.choice(VALUES, size=(n, nbins), p=[0.5] + [0.05] * 10).astype(np.uint16)
    assert n * nbins > 2 * TILE                           # more than one workgroup
    text = check(dev, rows, *plain(n), 10000, False)
    if nbins == 1:
        assert b"." not in text                           # one column: no zero column or only zero columns
    else:
        assert b".0," in text
    check(dev, rows, *plain(n), 10000, True, shift=5)


def test_row_form_decided_far_from_its_use(dev):
    nbins = 131072
    rows = np.full((4, nbins), 3, dtype=np.uint16)
    rows[0, -1] = 0                                       # a single zero in the last column only
    rows[1, 0] = 0                                        # a single zero in the first column only
    rows[3] = 0                                           # row 2 has no zero, row 3 only zeros
    text = check(dev, rows, *plain(4), 10000, False)
    lines = text.split(b"\n")
    assert lines[0].endswith(b",3.0,0.0") and lines[1].startswith(b"w_11-10010,0.0,3.0,")
    assert lines[2].endswith(b",3,3") and lines[3].endswith(b",0,0")


NAME_PREFIXES = [b"", b"a", b"abc", b"seventeen_bytes_x", b"L" * 300, b"caf\xc3\xa9_\xff\x80\xfe.part_", b"Q" * 45000]
NAME_STARTS = [0, 9, 99999, (1 << 32) - 1]


@pytest.mark.parametrize("win_len", [10000, 0])
@pytest.mark.parametrize("shift", [0, 1, 7, 15])
def test_names(dev, win_len, shift):
    """Empty, short, long and non-ASCII prefixes (one longer than the LDS stage), window numbers of every
    digit count, rows that share a prefix: everything after a name is shifted off alignment."""
    assert len(NAME_PREFIXES[3]) == 17 and len(NAME_PREFIXES[-1]) > 2 * STAGE
    rng = np.random.default_rng(win_len + shift)
    rpre = [0, 1, 1, 2, 3, 4, 5, 5, 6, 0, 6, 2] + [int(x) for x in rng.integers(0, 6, size=120)]
    n = len(rpre)
    rpos = [NAME_STARTS[i % 4] for i in range(n)]
    rpos[1], rpos[2] = 9, 99999                           # two rows of one prefix, different digit counts
    rows = rng.choice(VALUES, size=(n, 32)).astype(np.uint16)
    text = check(dev, rows, NAME_PREFIXES, rpre, rpos, win_len, False, shift)
    first = text.split(b"\n")[0]
    assert first.startswith(b"1-10000," if win_len else b",")
    if win_len:
        assert b"\nabc4294967296-4294977295," in text
    check(dev, rows[:16], NAME_PREFIXES, rpre[:16], rpos[:16], win_len, True, shift)


def test_capacity(dev):
    from kf2vecfsw_amd import chunks as CH
    rng = np.random.default_rng(77)
    n = 300
    rows = rng.choice(VALUES, size=(n, 32)).astype(np.uint16)
    names = plain(n)
    exp, eoff = CH.format_rows_host(rows, *names, 10000, False)
    total = len(exp)
    for cap in (total - 1, total // 2, 17, 0):
        got, off, status = run(dev, rows, *names, 10000, False, cap, shift=3)
        assert status == (1, total, 0, 0), cap
        assert off.tolist() == eoff.tolist(), cap       # row_off is complete
    got, off, status = run(dev, rows, *names, 10000, False, total + 100)
    assert status == (0, total, 0, 0) and got[:total] == exp
    assert got[total:] == bytes([SENTINEL]) * 100         # nothing past the text is touched
    # no rows
    got, off, status = run(dev, np.zeros((0, 32), np.uint16), [b"x"], [], [], 10000, False, 50)
    assert status == (0, 0, 0, 0) and off.tolist() == [0] and got == bytes([SENTINEL]) * 50


def test_bad_tables(dev):
    rng = np.random.default_rng(78)
    n = 150
    rows = rng.choice(VALUES, size=(n, 32)).astype(np.uint16)
    pre = [b"aa_", b"bbbb_", b"c_"]
    rpre = [i % 3 for i in range(n)]
    rpos = list(range(n))
    cap = 40000
    rpre_bad = list(rpre)
    rpre_bad[97] = 3                                      # == n_prefixes
    rpre_bad[120] = 0xFFFFFFFF
    got, off, status = run(dev, rows, pre, rpre_bad, rpos, 10000, False, cap)
    assert status == (2, 0, 97, 0) and off[-1] == 0
    assert got == bytes([SENTINEL]) * cap                 # nothing is formatted
    got, off, status = run(dev, rows, pre, rpre, rpos, 10000, False, cap, pre_off=[0, 7, 3, 9])   # decreasing
    assert status == (2, 0, 1, 0)                         # row 1 is the first with prefix 1
    assert got == bytes([SENTINEL]) * cap
    # decreasing entries that are no row's prefix: refused all the same
    got, off, status = run(dev, rows, pre + [b"", b""], rpre, rpos, 10000, False, cap, pre_off=[0, 3, 8, 10, 9, 10])
    assert status == (2, 0, n, 0) and got == bytes([SENTINEL]) * cap


@pytest.mark.parametrize("k,nbins,n", [(3, 32, 700), (7, 8192, 9)])
def test_round_trip_through_the_parser(dev, k, nbins, n):
    import torch
    from kf2vecfsw_amd import counter as C
    rng = np.random.default_rng(k)
    rows = rng.choice(VALUES, size=(n, nbins), p=[0.6] + [0.04] * 10).astype(np.uint16)
    rows[3] = 0
    rows[4] = 7
    d_rows = torch.from_numpy(rows.view(np.int16).copy()).to(dev)
    pre = ["g.part_c1.part_c1_sliding__", "g.part_c2.part_c2_sliding__"]
    rpre = np.asarray([i % 2 for i in range(n)], dtype=np.uint32)
    rpos = np.arange(n, dtype=np.uint64) * 9973
    text, row_off, status = C.format_kf_rows(d_rows, pre, rpre, rpos, 10000, False)
    off = C.formatted_to_host(row_off, status)
    total = int(off[-1])
    assert off[0] == 0 and (np.diff(off) > 2 * nbins).all() and total <= text.numel()
    pad = torch.full((total + 32,), 10, dtype=torch.uint8, device=dev)     # the parser's batch: 16-byte aligned, padded
    pad[:total] = text[:total]
    back, unit_row0, pstatus = C.parse_kf_rows(pad, np.asarray([0, total], dtype=np.int64), nbins)
    assert C.parsed_to_host(unit_row0, pstatus).tolist() == [0, n]
    assert np.array_equal(back[:n].cpu().numpy().view(np.uint16), rows)
    # the wrapper raises what the status says
    with pytest.raises(ValueError, match=r"row 5: .*status 2"):
        bad = rpre.copy()
        bad[5] = 2
        C.formatted_to_host(*C.format_kf_rows(d_rows, pre, bad, rpos, 10000, False)[1:])
    from kf2vecfsw_amd import _native as N
    with pytest.raises(N.NativeError, match=r"needs %d bytes" % total):
        C.formatted_to_host(*C.format_kf_rows(d_rows, pre, rpre, rpos, 10000, False, cap_bytes=total - 1)[1:])


# ---------------------------------------------------------------- the CLI
@pytest.fixture(scope="module")
def toy(dev, tmp_path_factory):
    """The toy train genomes unpacked, their chunk_store rows (k=7) and every genome's row names."""
    import torch
    from kf2vecfsw_amd import chunks as CH
    from kf2vecfsw_amd import main as M
    from kf2vecfsw_amd.counter import KmerCounter, pack_files
    inp = tmp_path_factory.mktemp("kf_format_fna")
    src = os.path.join(TOY, "train_tree_fna")
    for f in sorted(os.listdir(src)):
        (inp / f[:-3]).write_bytes(gzip.open(os.path.join(src, f)).read())
    store = CH.chunk_store(str(inp), 7, dev)
    files, samples = M.list_inputs(str(inp))
    hb = pack_files([os.path.join(str(inp), f) for f in files], samples, fmt=M.N.KF_FMT_FASTA)
    genomes = [CH.Genome(f, s) for f, s in zip(files, samples)]
    pipe = CH.ChunkPipeline(KmerCounter(7, dev), dev, 64, 2)
    pipe.prepare(hb, genomes)
    pipe.close()
    torch.cuda.synchronize()
    names = {g.sample: g.names for g in genomes if g.excluded is None}
    assert sorted(names) == sorted(store.samples) and len(names) >= 3
    return str(inp), store, names


def host_writer_file(native, store, names, sample, pseudo, path):
    """kf_write_kf_segments16 on chunk_store's rows of one genome, named by Genome.names."""
    i = store.samples.index(sample)
    rows = np.ascontiguousarray(store.counts[int(store.row0[i]): int(store.row0[i + 1])].cpu().numpy().view(np.uint16))
    assert rows.shape[0] == len(names[sample]) >= 5
    enc = [os.fsencode(x) for x in names[sample]]
    arr = (ctypes.c_char_p * len(enc))(*enc)
    paths = (ctypes.c_char_p * 1)(os.fsencode(str(path)))
    row0 = np.asarray([0, rows.shape[0]], dtype=np.int32)
    assert native.kf_write_kf_segments16(1, paths, row0.ctypes.data, None, arr, None, None, None, 0, rows.ctypes.data,
                                         rows.shape[1], int(pseudo), 1, 4) == 0
    return open(path, "rb").read()


@pytest.mark.parametrize("mode", ["raw", "pseudocount", "many launches and slabs"])
def test_cli_equals_the_host_writer(dev, native, toy, tmp_path, monkeypatch, capfd, mode):
    """get_chunks -k 7 through the device formatter.  The CLI formats on the device only at the k of
    chunks.DEVICE_FORMAT_K, where it measured no slower than the host writer; k=7 is not among them
    (profiles/r17), so the test adds it: the path ships and is checked whatever the routing is."""
    from kf2vecfsw_amd import chunks as CH
    from kf2vecfsw_amd import counter as C
    from kf2vecfsw_amd import main as M
    inp, store, names = toy
    monkeypatch.setattr(CH, "DEVICE_FORMAT_K", frozenset(CH.DEVICE_FORMAT_K | {7}))
    out = tmp_path / "out"
    out.mkdir()
    monkeypatch.setattr(CH, "TRACE", CH.TRACE)            # get_chunks sets it from the environment: put it back
    monkeypatch.setenv("KF_TRACE", "1")
    calls = []
    real = C.format_kf_rows

    def counted(c16, *a, **kw):
        calls.append(int(c16.shape[0]))
        return real(c16, *a, **kw)
    monkeypatch.setattr(C, "format_kf_rows", counted)
    args = ["get_chunks", "-input_dir", inp, "-output_dir", str(out), "-k", "7"]
    pseudo = mode == "pseudocount"
    if pseudo:
        args.append("-pseudocount")
    if mode == "many launches and slabs":
        # three windows per count launch (3 x 32 KiB of counts), and slabs below one row's text: a genome's
        # text is appended across launches and across slabs
        args += ["-batch_gb", str(3 * 32768 / (1 << 30))]
        monkeypatch.setattr(CH, "TEXT_SLAB", 20000)
        monkeypatch.setattr(CH, "TEXT_SMALL", 5000)      # the pieces go through the two slabs, short tails beside them
    M.main(args)
    err = capfd.readouterr().err
    trace = json.loads([ln for ln in err.splitlines() if ln.startswith('{"kf_chunks_trace"')][-1])["kf_chunks_trace"]
    stages = {t[0] for t in trace}
    assert {"format_device", "text_d2h", "write_text"} <= stages and "format_write" not in stages
    assert sorted(f for f in os.listdir(out) if f.endswith(".kf")) == sorted(s + ".kf" for s in store.samples)
    assert not [f for f in os.listdir(out) if f.endswith(".parts")]
    n_rows = int(store.row0[-1])
    assert sum(calls) == n_rows
    if mode == "many launches and slabs":
        assert max(calls) <= 3 and len(calls) >= n_rows // 3
        assert sum(1 for t in trace if t[0] == "write_text") > 2 * len(calls)
    for s in store.samples:
        exp = host_writer_file(native, store, names, s, pseudo, tmp_path / "host.kf")
        assert (out / (s + ".kf")).read_bytes() == exp, s


def test_cli_routing_follows_the_constant(dev, toy, tmp_path, monkeypatch, capfd):
    """A k of DEVICE_FORMAT_K formats on the device, any other on the host; the files are the same bytes."""
    from kf2vecfsw_amd import chunks as CH
    from kf2vecfsw_amd import main as M
    inp, _store, _names = toy
    monkeypatch.setattr(CH, "TRACE", CH.TRACE)
    monkeypatch.setenv("KF_TRACE", "1")
    k = min(CH.DEVICE_FORMAT_K)
    files = {}
    for how, ks in (("device", CH.DEVICE_FORMAT_K), ("host", frozenset())):
        monkeypatch.setattr(CH, "DEVICE_FORMAT_K", ks)
        out = tmp_path / how
        out.mkdir()
        M.main(["get_chunks", "-input_dir", inp, "-output_dir", str(out), "-k", str(k)])
        err = capfd.readouterr().err
        trace = json.loads([ln for ln in err.splitlines() if ln.startswith('{"kf_chunks_trace"')][-1])["kf_chunks_trace"]
        stages = {t[0] for t in trace}
        assert ("format_device" in stages) == (how == "device") and ("format_write" in stages) == (how == "host")
        files[how] = {f: (out / f).read_bytes() for f in sorted(os.listdir(out)) if f.endswith(".kf")}
    assert len(files["device"]) >= 3 and files["device"] == files["host"]
