"""GPU checks of get_frequencies' piece-wise path: kf_rows_accumulate against
numpy's u64 sums, and the CLI with -split_gb against the whole-file run and the
oracle."""
import numpy as np
import pytest

import gen
from split_inputs import fastq_reads

pytestmark = pytest.mark.gpu

U32 = 0xFFFFFFFF
GiB = 1 << 30


@pytest.fixture(scope="module")
def torch_dev(native):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu tests need an MI355X")
    return torch.device("cuda:0")


def dev_u32(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32)).to(dev)


def run_accumulate(src, src_tot, seg, dst, dst_tot, status, accumulate, dev, n_src=None):
    """kf_rows_accumulate on host arrays (u32 rows, u64 totals, i32 seg, u32
    status); dst, its totals and status carry a guard row that must come back as
    it went in.  Returns (dst, totals, status) after the call."""
    import torch
    from kf2vecfsw_amd import _native as N
    n_dst, nbins = dst.shape
    guard = np.full((1, nbins), 0xABCD1234, np.uint32)
    d_src, d_dst = dev_u32(src, dev), dev_u32(np.concatenate([dst, guard]), dev)
    d_st = torch.from_numpy(src_tot.astype(np.uint64).view(np.int64)).to(dev)
    d_dt = torch.from_numpy(np.concatenate([dst_tot.astype(np.uint64), [np.uint64(77)]]).view(np.int64)).to(dev)
    d_seg = torch.from_numpy(np.asarray(seg, np.int32)).to(dev)
    d_status = dev_u32(np.concatenate([status, [0x55]]), dev)
    N.check(N.lib().kf_rows_accumulate(d_src.data_ptr(), d_st.data_ptr(), src.shape[0] if n_src is None else n_src,
                                       d_seg.data_ptr(), n_dst, nbins, d_dst.data_ptr(), d_dt.data_ptr(),
                                       d_status.data_ptr(), N.KF_ACCUMULATE if accumulate else 0,
                                       torch.cuda.current_stream(dev).cuda_stream), "kf_rows_accumulate")
    torch.cuda.synchronize()
    out = d_dst.cpu().numpy().view(np.uint32)
    tot = d_dt.cpu().numpy().view(np.uint64)
    st = d_status.cpu().numpy().view(np.uint32)
    assert np.all(out[n_dst] == 0xABCD1234) and tot[n_dst] == 77 and st[n_dst] == 0x55
    return out[:n_dst], tot[:n_dst], st[:n_dst]


def expect(src, src_tot, seg, dst, dst_tot, status, accumulate):
    n_dst = dst.shape[0]
    e = dst.astype(np.uint64) if accumulate else np.zeros(dst.shape, np.uint64)
    t = dst_tot.astype(np.uint64).copy() if accumulate else np.zeros(n_dst, np.uint64)
    st = status.copy() if accumulate else np.zeros(n_dst, np.uint32)
    for r in range(n_dst):
        e[r] += src[seg[r]: seg[r + 1]].sum(axis=0, dtype=np.uint64)
        t[r] += src_tot[seg[r]: seg[r + 1]].sum(dtype=np.uint64)
        if (e[r] > U32).any():
            st[r] |= 1
    return np.minimum(e, U32).astype(np.uint32), t, st


# nbins of k = 2 (4-byte path), 3, 7 and 11; segments that are empty, of one row and of 33 rows
@pytest.mark.parametrize("nbins,seg", [(10, [0, 0, 1, 34, 34, 70]), (32, [0, 0, 1, 34, 34, 70]),
                                       (8192, [0, 0, 1, 34, 34, 70]), (2098176, [0, 0, 1, 34, 35])])
@pytest.mark.parametrize("accumulate", [False, True])
def test_rows_accumulate_equals_numpy(torch_dev, nbins, seg, accumulate):
    rng = np.random.default_rng(nbins + accumulate)
    n_src, n_dst = seg[-1], len(seg) - 1
    src = rng.integers(0, 1 << 25, size=(n_src, nbins), dtype=np.uint32)   # 71 rows of it stay below 2^32
    src_tot = rng.integers(0, 1 << 50, size=n_src, dtype=np.uint64)
    dst = rng.integers(0, 1 << 25, size=(n_dst, nbins), dtype=np.uint32)
    dst_tot = rng.integers(0, 1 << 50, size=n_dst, dtype=np.uint64)
    status = np.full(n_dst, 4, np.uint32)   # a bit the kernel never sets: kept under KF_ACCUMULATE, cleared without
    got = run_accumulate(src, src_tot, seg, dst, dst_tot, status, accumulate, torch_dev)
    want = expect(src, src_tot, seg, dst, dst_tot, status, accumulate)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    empty = [r for r in range(n_dst) if seg[r] == seg[r + 1]]
    assert empty
    for r in empty:
        if accumulate:   # left alone
            assert np.array_equal(got[0][r], dst[r]) and got[1][r] == dst_tot[r] and got[2][r] == 4
        else:            # zeroed
            assert not got[0][r].any() and got[1][r] == 0 and got[2][r] == 0


def test_rows_accumulate_unaligned_rows_take_the_4_byte_path(torch_dev):
    """nbins % 4 == 0 but a matrix that is not 16-byte aligned."""
    import torch
    from kf2vecfsw_amd import _native as N
    rng = np.random.default_rng(4)
    nbins, n_src = 32, 9
    src = rng.integers(0, 1 << 28, size=(n_src, nbins), dtype=np.uint32)
    flat = torch.zeros(n_src * nbins + 1, dtype=torch.int32, device=torch_dev)
    flat[1:] = dev_u32(src.reshape(-1), torch_dev)
    tot = torch.arange(n_src, dtype=torch.int64, device=torch_dev)
    seg = torch.tensor([0, 4, 9], dtype=torch.int32, device=torch_dev)
    dst = torch.zeros(2 * nbins + 1, dtype=torch.int32, device=torch_dev)
    dt = torch.zeros(2, dtype=torch.int64, device=torch_dev)
    st = torch.zeros(2, dtype=torch.int32, device=torch_dev)
    assert (flat.data_ptr() + 4) % 16 == 4
    N.check(N.lib().kf_rows_accumulate(flat.data_ptr() + 4, tot.data_ptr(), n_src, seg.data_ptr(), 2, nbins,
                                       dst.data_ptr() + 4, dt.data_ptr(), st.data_ptr(), 0,
                                       torch.cuda.current_stream(torch_dev).cuda_stream), "kf_rows_accumulate")
    torch.cuda.synchronize()
    got = dst.cpu().numpy().view(np.uint32)
    assert got[0] == 0
    assert np.array_equal(got[1:].reshape(2, nbins), np.stack([src[:4].sum(axis=0), src[4:].sum(axis=0)]))
    assert dt.tolist() == [0 + 1 + 2 + 3, 4 + 5 + 6 + 7 + 8] and st.tolist() == [0, 0]


@pytest.mark.parametrize("nbins", [10, 8192])
def test_rows_accumulate_overflow_saturates_and_sticks(torch_dev, nbins):
    """0xFFFFFFFF + 1 saturates and sets bit 0, a sum of exactly 0xFFFFFFFF does
    not; a second accumulating call keeps both the flag and the saturation."""
    src = np.zeros((6, nbins), np.uint32)
    src[0, 3], src[1, 3] = U32, 1                  # row 0: column 3 passes by one
    src[0, 5], src[1, 5] = U32 - 7, 7              # ... column 5 reaches 0xFFFFFFFF exactly
    src[2, nbins - 1], src[3, nbins - 1] = 1 << 31, (1 << 31) - 1   # row 1: exactly 0xFFFFFFFF, no overflow
    src[4, 0], src[5, 0] = 1 << 31, 1 << 31        # row 2: exactly 2^32, in the last wave of the row too
    src[4, nbins - 2], src[5, nbins - 2] = U32, U32
    tot = np.arange(6, dtype=np.uint64)
    seg = [0, 2, 4, 6]
    z = np.zeros((3, nbins), np.uint32)
    d, t, st = run_accumulate(src, tot, seg, z, np.zeros(3, np.uint64), np.zeros(3, np.uint32), False, torch_dev)
    want = expect(src, tot, seg, z, np.zeros(3, np.uint64), np.zeros(3, np.uint32), False)
    assert np.array_equal(d, want[0]) and np.array_equal(t, want[1])
    assert st.tolist() == [1, 0, 1]
    assert d[0, 3] == U32 and d[0, 5] == U32 and d[1, nbins - 1] == U32 and d[2, 0] == U32 and d[2, nbins - 2] == U32
    # a second, accumulating call: zeros keep the rows, the flag stays; one more count on a saturated
    # column saturates again, on row 1's full column it overflows now
    more = np.zeros((3, nbins), np.uint32)
    more[1, nbins - 1] = 1
    more[2, 0] = 5
    d2, t2, st2 = run_accumulate(more, np.ones(3, np.uint64), [0, 1, 2, 3], d, t, st, True, torch_dev)
    assert st2.tolist() == [1, 1, 1]
    assert np.array_equal(d2, d) and d2[2, 0] == U32 and d2[1, nbins - 1] == U32
    assert np.array_equal(t2, t + np.uint64(1))


@pytest.mark.parametrize("seg", [[0, 5, 3, 10], [0, 5, 8, 71], [-1, 5, 8, 10], [0, 0, 0, 71]])
@pytest.mark.parametrize("accumulate", [False, True])
def test_rows_accumulate_bad_segment_table(torch_dev, seg, accumulate):
    """A table that decreases, starts below 0 or ends past n_src: status 2
    everywhere, d_dst and its totals untouched (the device checks it: the source
    has 70 rows, so no row of a bad table is read either)."""
    rng = np.random.default_rng(3)
    nbins = 8192
    src = rng.integers(0, 1 << 20, size=(70, nbins), dtype=np.uint32)
    dst = rng.integers(0, 1 << 20, size=(3, nbins), dtype=np.uint32)
    dtot = np.array([5, 6, 7], np.uint64)
    d, t, st = run_accumulate(src, np.ones(70, np.uint64), seg, dst, dtot, np.array([0, 1, 0], np.uint32), accumulate,
                              torch_dev)
    assert st.tolist() == [2, 2, 2]
    assert np.array_equal(d, dst) and np.array_equal(t, dtot)


def test_accumulate_rows_wrapper_carries_a_file_over_batches(torch_dev):
    """counter.accumulate_rows as the CLI uses it: one accumulator row, the rows
    of a file's pieces added batch by batch."""
    import torch
    from kf2vecfsw_amd import counter as C
    rng = np.random.default_rng(8)
    nbins = 8192
    batches = [rng.integers(0, 1 << 24, size=(n, nbins), dtype=np.uint32) for n in (1, 3, 2)]
    row = torch.zeros((1, nbins), dtype=torch.int32, device=torch_dev)
    tot = torch.zeros(1, dtype=torch.int64, device=torch_dev)
    st = torch.zeros(1, dtype=torch.int32, device=torch_dev)
    for b in batches:
        seg = torch.tensor([0, len(b)], dtype=torch.int32, device=torch_dev)
        C.accumulate_rows(dev_u32(b, torch_dev), torch.full((len(b),), 10, dtype=torch.int64, device=torch_dev), seg,
                          row, tot, st, accumulate=True)
    torch.cuda.synchronize()
    assert np.array_equal(row.cpu().numpy().view(np.uint32)[0], np.concatenate(batches).sum(axis=0, dtype=np.uint64))
    assert tot.item() == 60 and st.item() == 0


# ---------------------------------------------------------------------------
# the CLI
# ---------------------------------------------------------------------------
SPLIT = 16384 / GiB      # -split_gb: files above 16 KiB go in pieces of 16 KiB
BATCH = 40960 / GiB      # -batch_gb: two pieces per batch (the first two batches fewer), so a file spans batches


@pytest.fixture(scope="module")
def split_dir(tmp_path_factory):
    """A multi-record FASTA and a FASTQ of 150-base reads (quality lines starting
    with '@' and '+') of about 100 KiB each, and a small file of each kind."""
    rng = np.random.default_rng(1234)
    d = tmp_path_factory.mktemp("split_in")
    recs = [b">ctg%d some text\n" % i + gen.wrap(gen.random_seq(rng, int(L), n_rate=0.002, lower=0.02), w)
            for i, (L, w) in enumerate([(30000, 60), (8000, 80), (45000, 70), (5, 60), (17000, 0)])]
    blobs = {"big.fa": b"".join(recs), "reads.fq": fastq_reads(rng, 310, length=150, qual_first=b"@+I"),
             "small.fna": gen.random_fasta(rng, 3000, max_records=3), "few.fastq": fastq_reads(rng, 9, length=150)}
    assert 95000 < len(blobs["big.fa"]) < 120000 and 95000 < len(blobs["reads.fq"]) < 120000
    for f, b in blobs.items():
        (d / f).write_bytes(b)
    return d, blobs


def run_cli(inp, out, k, extra, monkeypatch):
    from kf2vecfsw_amd import counter as C
    from kf2vecfsw_amd import main as Mn
    out.mkdir()
    # the count-matrix cap follows -batch_gb (one 8 MiB row at k = 11 is more than 40 KiB): lift it, so
    # that the byte budget alone makes the batches
    monkeypatch.setenv("KF_COUNT_BUDGET_MB", "64")
    before = dict(C.INDEX_PATHS)
    Mn.main(["get_frequencies", "-input_dir", str(inp), "-output_dir", str(out), "-k", str(k), "-p", "2"] + extra)
    return {p: C.INDEX_PATHS[p] - before[p] for p in before}


@pytest.mark.parametrize("k,mode", [(3, []), (7, ["-pseudocount"]), (8, ["-raw_cnt"]), (9, []), (10, ["-raw_cnt"]),
                                    (11, ["-pseudocount"])])
def test_cli_split_equals_whole_and_oracle(torch_dev, oracle, split_dir, tmp_path, monkeypatch, capsys, k, mode):
    """Files above -split_gb counted in pieces that span several batches: the
    `.kf` bytes of the same run with -split_gb 0, and the oracle's; the FASTQ
    pieces indexed on the device; the per-file lines once per file."""
    from kf2vecfsw_amd import main as Mn
    inp, blobs = split_dir
    fq = Mn.fastq_pieces(str(inp / "reads.fq"), 16384)
    fa = Mn.fasta_pieces(str(inp / "big.fa"), k, 16384)
    assert len(fq) >= 6 and len(fa) >= 6
    capsys.readouterr()
    moved = run_cli(inp, tmp_path / "split", k, mode + ["-split_gb", repr(SPLIT), "-batch_gb", repr(BATCH)],
                    monkeypatch)
    printed = capsys.readouterr().out
    # two 16 KiB pieces per 40 KiB batch at most: each file's pieces span at least three batches
    assert moved["fastq_device"] >= len(fq) // 2 and moved["fasta_device"] >= len(fa) // 2, moved
    assert moved["fastq_host_fallback"] == 0, moved
    moved0 = run_cli(inp, tmp_path / "whole", k, mode + ["-split_gb", "0", "-batch_gb", repr(BATCH)], monkeypatch)
    assert moved0["fastq_host_fallback"] == 0 and moved0["fastq_device"] <= 2, moved0
    for f, b in blobs.items():
        name = f.rsplit(".f", 1)[0]
        got = (tmp_path / "split" / f"{name}.kf").read_bytes()
        assert got == (tmp_path / "whole" / f"{name}.kf").read_bytes(), f
        c, _ = oracle.count(b, k)
        assert got == oracle.kf_line(name, c, pseudocount="-pseudocount" in mode, raw_cnt="-raw_cnt" in mode).encode(), f
        for line, on in ((">>> Adding pseudocounts. Sample: " + f, "-pseudocount" in mode),
                         (">>> Normalizing. Sample: " + f, "-raw_cnt" not in mode)):
            assert printed.count(line + "\n") == int(on), line


def miscut_fastq(rng):
    """Regular four-line FASTQ of about 40 KiB in which the first line at or after
    byte 16384 is a sequence line that starts with '@' and whose quality line
    starts with '+': the cut rule accepts it."""
    head = fastq_reads(rng, 60, length=150)
    head = head[: head.rindex(b"@r", 0, 16000)]                    # whole records, below 16000 bytes
    hdr = b"@trap " + b"x" * (16384 - len(head) - 6 + 3) + b"\n"   # its sequence line starts at 16388
    seq = b"@" + gen.random_seq(rng, 149).tobytes()                # '@' is no base: 149 bases are counted
    rec = hdr + seq + b"\n+\n" + b"+" + b"I" * 149 + b"\n"
    blob = head + rec + fastq_reads(rng, 70, length=150, name=b"t")
    assert len(head) + len(hdr) == 16388
    return blob


def test_cli_miscut_file_is_refused(torch_dev, oracle, tmp_path, monkeypatch):
    """A cut at a line that is no record start: the device index flags the piece,
    the run raises a ValueError that names the file and points at -split_gb 0,
    and no `.kf` is written for it; the other files' are right or absent.  Counted
    whole, the same file is fine."""
    import fastq_model as FM
    from kf2vecfsw_amd import main as Mn
    rng = np.random.default_rng(31)
    inp = tmp_path / "in"
    inp.mkdir()
    blobs = {"trap.fq": miscut_fastq(rng), "ok.fq": fastq_reads(rng, 20, length=150),
             "ok2.fa": gen.random_fasta(rng, 2000, max_records=2)}
    assert FM.is_regular(blobs["trap.fq"])
    for f, b in blobs.items():
        (inp / f).write_bytes(b)
    cuts = [a for a, _ in Mn.fastq_pieces(str(inp / "trap.fq"), 16384)]
    assert 16388 in cuts and blobs["trap.fq"][16388: 16389] == b"@"
    with pytest.raises(ValueError) as ei:
        run_cli(inp, tmp_path / "out", 7, ["-raw_cnt", "-split_gb", repr(SPLIT)], monkeypatch)
    assert "trap.fq" in str(ei.value) and "-split_gb 0" in str(ei.value)
    assert not (tmp_path / "out" / "trap.kf").exists()
    for f in ("ok.fq", "ok2.fa"):
        name = f.rsplit(".f", 1)[0]
        p = tmp_path / "out" / f"{name}.kf"
        if p.exists():
            assert p.read_bytes() == oracle.kf_line(name, oracle.count(blobs[f], 7)[0], raw_cnt=True).encode()
    run_cli(inp, tmp_path / "whole", 7, ["-raw_cnt", "-split_gb", "0"], monkeypatch)
    for f, b in blobs.items():
        name = f.rsplit(".f", 1)[0]
        assert (tmp_path / "whole" / f"{name}.kf").read_bytes() == \
            oracle.kf_line(name, oracle.count(b, 7)[0], raw_cnt=True).encode()


@pytest.mark.parametrize("order", [["x.fq", "x.fa"], ["x.fa", "x.fq"]])
def test_cli_same_sample_name_last_file_wins(torch_dev, oracle, tmp_path, monkeypatch, order):
    """x.fq (counted in pieces) and a small x.fa share the sample name x: the one
    that comes last in the input order is the one written, as without pieces."""
    from kf2vecfsw_amd import main as Mn
    rng = np.random.default_rng(17)
    inp = tmp_path / "in"
    inp.mkdir()
    blobs = {"x.fq": fastq_reads(rng, 130, length=150, qual_first=b"@+"),
             "x.fa": gen.random_fasta(rng, 4000, max_records=2), "y.fa": gen.random_fasta(rng, 2500, max_records=2)}
    for f, b in blobs.items():
        (inp / f).write_bytes(b)
    files = order + ["y.fa"]
    monkeypatch.setattr(Mn, "list_inputs", lambda d: (files, [f.rsplit(".f", 1)[0] for f in files]))
    moved = run_cli(inp, tmp_path / "out", 7, ["-raw_cnt", "-split_gb", repr(SPLIT), "-batch_gb", repr(BATCH)],
                    monkeypatch)
    assert moved["fastq_device"] >= 2, moved
    for name, f in (("x", order[-1]), ("y", "y.fa")):
        assert (tmp_path / "out" / f"{name}.kf").read_bytes() == \
            oracle.kf_line(name, oracle.count(blobs[f], 7)[0], raw_cnt=True).encode(), f
