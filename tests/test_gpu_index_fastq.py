"""GPU parity of the device FASTQ record index (kf_index_fastq) against the host
index (kf_index_records), the pairs of tests/fastq_model.py and, through
kf_count_batch and the CLI, the oracle."""
import numpy as np
import pytest

import fastq_model as M
import gen

pytestmark = pytest.mark.gpu

FQ = 2   # KF_FMT_FASTQ


@pytest.fixture(scope="module")
def torch_dev(native):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu tests need an MI355X")
    return torch.device("cuda:0")


def raw_index(hb, dev, cap_pairs=None, cap_lines=None):
    """kf_index_fastq itself on a host batch, with tables that hold anything the
    batch can make unless told otherwise: (pairs, n_pairs, n_lines, status)."""
    import torch
    from kf2vecfsw_amd import _native as N
    n, nbytes = hb.n, int(hb.off[-1])
    cap_lines = nbytes if cap_lines is None else cap_lines
    cap_pairs = nbytes // 4 + 2 * n + 1 if cap_pairs is None else cap_pairs
    data = hb.data.to(dev)
    off = torch.from_numpy(hb.off.view(np.int64)).to(dev)
    need = int(N.lib().kf_index_fastq_scratch_bytes(nbytes, n, cap_lines))
    scratch = torch.empty(need // 8 + 1, dtype=torch.int64, device=dev)
    excl = torch.full((2 * cap_pairs + 2,), -1, dtype=torch.int64, device=dev)
    cnt = torch.full((2,), -1, dtype=torch.int64, device=dev)
    status = torch.full((n + 1,), -1, dtype=torch.int32, device=dev)
    N.check(N.lib().kf_index_fastq(data.data_ptr(), off.data_ptr(), n, nbytes, excl.data_ptr(), cap_pairs, cap_lines,
                                   cnt.data_ptr(), status.data_ptr(), scratch.data_ptr(), need,
                                   torch.cuda.current_stream(dev).cuda_stream), "kf_index_fastq")
    torch.cuda.synchronize()
    m, lines = (int(x) for x in cnt.cpu().numpy())
    ex = excl.cpu().numpy()
    assert np.all(ex[2 * min(m, cap_pairs):] == -1)          # nothing written past the count or the table
    assert int(status[n].item()) == -1
    return ex[: 2 * min(m, cap_pairs)], m, lines, status[:n].cpu().numpy()


def host_mask(hb, n):
    return M.mask_of(hb.excl, n)


def check_batch(blobs, dev):
    """Regular genomes: status 0, the model's pairs exactly, the host's excluded
    bytes away from newlines."""
    from kf2vecfsw_amd import counter as C
    hb = C.pack_genomes(blobs, fmt=FQ)
    n = int(hb.off[-1])
    pairs, m, lines, status = raw_index(hb, dev)
    d = hb.data.numpy()[:n]
    assert lines == int(np.count_nonzero(d == 10))
    assert not status.any(), status
    assert 2 * m == pairs.size
    want = sum((M.device_pairs(b, int(hb.off[i])) for i, b in enumerate(blobs)), [])
    assert pairs.tolist() == want
    nl = d == 10
    assert np.array_equal(M.mask_of(pairs, n) & ~nl, host_mask(hb, n) & ~nl)
    p = pairs.reshape(-1, 2)
    assert np.all(p[:, 1] > p[:, 0]) and np.all(p[1:, 0] >= p[:-1, 1])      # non-empty, sorted, disjoint
    g = np.searchsorted(hb.off, p[:, 0].astype(np.uint64), side="right") - 1
    assert np.all(p[:, 1].astype(np.uint64) <= hb.off[g + 1])               # no pair crosses a genome end
    return hb, pairs


EDGES = [b"", b"@r\n", b"@r\nACGT", b"@r\nACGT\n+", b"@e\n\n+\n\n@f\nAC\n+\nII\n",
         b"@q\nACGTAC\n+\n@IIIII\n@p\nACGTAC\n+x\n+IIIII\n", b"@c\r\nACGT\r\n+\r\nIIII\r\n@d\r\nGG\r\n+c\r\nII\r\n",
         b"\n\n\n", b"@r\nACGT\n+\nIIIII\n\n\n\n\n\n\n", b"@r1\nACGT\n+\nIIII\n@r2\nGGCC\n"]


def corpus(rng):
    blobs = [gen.random_fastq(rng, int(rng.integers(0, 400)), n_rate=0.01, lower=0.05) for _ in range(12)]
    blobs[3] = b""
    # no final newline and a size that is a multiple of 16: the next genome's '@' follows directly
    tight = b"@t\nACGTACGTACGTA\n+\n" + b"I" * 13
    assert len(tight) % 16 == 0 and M.is_regular(tight)
    return blobs[:6] + [tight] + blobs[6:] + EDGES


def test_fastq_index_matches_host(torch_dev):
    rng = np.random.default_rng(61)
    blobs = corpus(rng)
    assert all(M.is_regular(b) for b in blobs)
    hb, _ = check_batch(blobs, torch_dev)
    i = next(i for i, b in enumerate(blobs) if b.startswith(b"@t\n"))
    assert int(hb.off[i + 1]) - int(hb.off[i]) == len(blobs[i])   # no padding after it
    for b in EDGES:                                                # each alone, too
        check_batch([b], torch_dev)


def irregular_cases(rng):
    return [gen.random_fastq(rng, 30, multiline=True), gen.random_fastq(rng, 200, multiline=True),
            b"@a\nACGT\n+\nIIII\n\n@b\nACGT\n+\nIIII\n",          # a blank line between records
            b"@a\nACGT\n+\nIII\n@b\nACGT\n+\nIIII\n",             # quality shorter than the sequence
            b"@a\n+CGT\n+\nIIII\n",                               # a sequence line starting with '+'
            b"a\nACGT\n+\nIIII\n",                                # a first line not starting with '@'
            b"@a\n\n+\nI\n",                                      # empty sequence, non-empty quality
            b"@a\nACGT\nIIII\n"]                                  # no '+' line


def test_irregular_genomes_are_flagged_and_fall_back(torch_dev):
    import torch
    from kf2vecfsw_amd import counter as C
    rng = np.random.default_rng(62)
    bad = irregular_cases(rng)
    assert not any(M.is_regular(b) for b in bad)
    good = [gen.random_fastq(rng, int(rng.integers(1, 60))) for _ in range(len(bad) + 1)]
    for b in bad:                                                   # alone
        hb = C.pack_genomes([b], fmt=FQ)
        pairs, m, _, status = raw_index(hb, torch_dev)
        assert status[0] != 0, b
        assert pairs.size == 0 or (pairs.min() >= 0 and pairs.max() <= int(hb.off[-1]))
    mixed = [x for pair in zip(good, bad) for x in pair] + [good[-1]]
    hb = C.pack_genomes(mixed, fmt=FQ)
    pairs, m, _, status = raw_index(hb, torch_dev)
    assert [bool(s) for s in status] == [not M.is_regular(b) for b in mixed]
    p = pairs.reshape(-1, 2)
    g = np.searchsorted(hb.off, p[:, 0].astype(np.uint64), side="right") - 1
    assert np.all(p[:, 0] <= p[:, 1]) and np.all(p[:, 1].astype(np.uint64) <= hb.off[g + 1])
    # through to_device: the host's pairs (whole-batch fallback)
    before = dict(C.INDEX_PATHS)
    db = C.to_device(C.HostBatch(hb.data, hb.off, None, hb.names, fastq=True), torch_dev)
    torch.cuda.synchronize()
    assert C.INDEX_PATHS["fastq_host_fallback"] == before["fastq_host_fallback"] + 1
    assert C.INDEX_PATHS["fastq_device"] == before["fastq_device"]
    n = int(hb.off[-1])
    got = db.excl[: 2 * db.n_excl].cpu().numpy()
    nl = hb.data.numpy()[:n] == 10
    assert np.array_equal(M.mask_of(got, n) & ~nl, host_mask(hb, n) & ~nl)


@pytest.mark.parametrize("k", [7, 11])
def test_fastq_index_counts_equal_oracle(torch_dev, oracle, k):
    import torch
    from kf2vecfsw_amd import counter as C
    rng = np.random.default_rng(63 + k)
    blobs = corpus(rng)
    hb = C.pack_genomes(blobs, fmt=FQ)
    before = dict(C.INDEX_PATHS)
    db = C.to_device(C.HostBatch(hb.data, hb.off, None, hb.names, fastq=True), torch_dev)
    assert C.INDEX_PATHS["fastq_device"] == before["fastq_device"] + 1
    assert C.INDEX_PATHS["fastq_host_fallback"] == before["fastq_host_fallback"]
    cnt, tot = C.KmerCounter(k, torch_dev).count(db)
    torch.cuda.synchronize()
    c = C.counts_to_numpy(cnt)
    t = tot.cpu().numpy()
    for i, b in enumerate(blobs):
        oc, ot = oracle.count(b, k, fmt=FQ)
        assert int(t[i]) == ot, (i, int(t[i]), ot)
        assert np.array_equal(c[i], oc), i


B, W = 4096, 1024   # bytes per index block, blocks per scan level (kISpan, kQLevel in csrc/kf_index.hip)


def boundary_batch():
    """Two genomes of 150-base reads over 2 W + 3 blocks, written record by
    record: (bytes, start of the second genome, the pairs, where the '+' lines at
    the level boundaries start)."""
    g1 = W * B + 300 * B + 1616
    stop = (2 * W + 2) * B + 1000
    assert g1 % 16 == 0 and g1 % B != 0
    rng = np.random.default_rng(64)
    buf = bytearray()
    exp = []

    def record(i, hdr_len, ls, first, final_nl=True):
        p = len(buf)
        hdr = (b"@%d" % i).ljust(hdr_len, b"h")
        seq = gen.BASES[rng.integers(0, 4, size=ls)].tobytes()
        if first:
            exp.extend([p, p + hdr_len])
        else:
            exp.append(p + hdr_len)              # ends the pair that the previous record's '+' began
        exp.append(p + hdr_len + 1 + ls + 1)     # the '+'
        buf.extend(hdr + b"\n" + seq + b"\n+\n" + b"I" * ls + (b"\n" if final_nl else b""))
        return p + hdr_len + 1 + ls + 1

    i = 0
    plus_at = []
    for end in (g1, stop):
        first = True
        while True:
            p = len(buf)
            nxt = (p // (W * B) + 1) * W * B      # the next level boundary
            if nxt - p < 700 and nxt < end:       # the sequence line's '\n' at nxt - 1, the '+' at nxt
                plus_at.append(record(i, 6, nxt - p - 8, first))
            elif end == g1 and end - p < 700:     # the first genome's last record ends at g1 without '\n'
                hl = 6 if (end - p) % 2 == 0 else 7
                record(i, hl, (end - p - hl - 4) // 2, first, final_nl=False)
                exp.append(len(buf))
                break
            elif p >= end:
                exp.append(len(buf) - 1)          # the last quality line, up to its '\n'
                break
            else:
                record(i, 6, 150, first)
            first = False
            i += 1
        assert end != g1 or len(buf) == g1
    return bytes(buf), g1, exp, plus_at


def test_fastq_index_scan_level_boundaries(torch_dev):
    """One batch of 2,051 index blocks of 4 KiB.  A scan level holds 1,024
    blocks, so the block prefixes take the second level from block 1024 and
    again from block 2048.  Two genomes of 150-base reads; the second starts
    mid-block (16-aligned, not a multiple of 4,096) right after the first's last
    quality byte (no newline).  At each level boundary a record straddles it with
    the '\\n' of its sequence line as the last byte of block 1023 / 2047 and its
    '+' as the first byte of block 1024 / 2048."""
    import torch
    from kf2vecfsw_amd import counter as C
    buf, g1, exp, plus_at = boundary_batch()
    n = (len(buf) + 15) // 16 * 16
    assert plus_at == [W * B, 2 * W * B] and (n + B - 1) // B == 2 * W + 3
    assert all(buf[x - 1] == 10 and buf[x] == ord("+") for x in plus_at)
    assert buf[g1 - 1] == ord("I") and buf[g1] == ord("@")
    off = np.array([0, g1, n], dtype=np.uint64)
    data = torch.full((n,), 10, dtype=torch.uint8)
    d = data.numpy()
    d[: len(buf)] = np.frombuffer(buf, np.uint8)
    hb = C.HostBatch(data, off, None, ["a", "b"], fastq=True)
    pairs, m, lines, status = raw_index(hb, torch_dev, cap_pairs=len(exp) // 2 + 7, cap_lines=n // 64)
    assert not status.any() and lines == int(np.count_nonzero(d == 10))
    assert pairs.tolist() == exp
    host = np.concatenate([C.index_records(d[int(off[i]): int(off[i + 1])], FQ, int(off[i]))[0] for i in range(2)])
    nl = d == 10
    assert np.array_equal(M.mask_of(pairs, n) & ~nl, M.mask_of(host, n) & ~nl)
    db = C.to_device(hb, torch_dev)                 # and the same through to_device
    assert db.n_excl == len(exp) // 2 and db.excl[: 2 * db.n_excl].cpu().numpy().tolist() == exp


def test_fastq_index_long_lines(torch_dev):
    """A read of 10,000 bases (one line longer than two 4 KiB blocks) between
    short reads is regular; with a 9,999-byte quality line it is flagged."""
    from kf2vecfsw_amd import counter as C
    rng = np.random.default_rng(65)
    short = gen.random_fastq(rng, 5)
    seq = gen.random_seq(rng, 10000).tobytes()
    good = short + b"@long\n" + seq + b"\n+\n" + b"I" * 10000 + b"\n" + short
    check_batch([short, good, short], torch_dev)
    bad = short + b"@long\n" + seq + b"\n+\n" + b"I" * 9999 + b"\n" + short
    _, _, _, status = raw_index(C.pack_genomes([short, bad, short], fmt=FQ), torch_dev)
    assert [bool(s) for s in status] == [False, True, False]


def test_fastq_index_tables_regrow(torch_dev):
    """30,000 records of 8 bytes: a '\\n' every other byte and a pair per 8 bytes
    exceed to_device's first guesses (a line per 32 bytes, a pair per 128), and
    the result is complete."""
    import torch
    from kf2vecfsw_amd import counter as C
    blob = b"@\nA\n+\nI\n" * 30000
    hb = C.pack_genomes([blob], fmt=FQ)
    n = int(hb.off[-1])
    _, m, lines, _ = raw_index(hb, torch_dev, cap_pairs=100, cap_lines=n)     # pairs past the table: counted only
    assert (m, lines) == (30001, 120000)
    _, m, lines, status = raw_index(hb, torch_dev, cap_pairs=n, cap_lines=100)   # newline table too small
    assert (m, lines) == (0, 120000)
    db = C.to_device(C.HostBatch(hb.data, hb.off, None, ["x"], fastq=True), torch_dev)
    torch.cuda.synchronize()
    assert db.n_excl == 30001
    got = db.excl[: 2 * db.n_excl].cpu().numpy()
    assert got.tolist() == M.device_pairs(blob)
    nl = hb.data.numpy()[:n] == 10
    assert np.array_equal(M.mask_of(got, n) & ~nl, host_mask(hb, n) & ~nl)


def test_cli_get_frequencies_fastq(torch_dev, oracle, tmp_path):
    """get_frequencies on a directory of .fq / .fastq files: the device index,
    `.kf` files byte-equal to the oracle's; with a multi-line file added, the same
    through the host fallback."""
    from kf2vecfsw_amd import counter as C
    from kf2vecfsw_amd import main as Mn
    rng = np.random.default_rng(66)
    inp = tmp_path / "in"
    inp.mkdir()
    blobs = {"s0.fq": gen.random_fastq(rng, 300), "s1.fq": gen.random_fastq(rng, 40, n_rate=0.01),
             "s2.fq": gen.random_fastq(rng, 1), "s3.fastq": gen.random_fastq(rng, 150, lower=0.1)}
    for f, b in blobs.items():
        (inp / f).write_bytes(b)

    def run(tag, extra, want_path):
        out = tmp_path / tag
        out.mkdir()
        before = dict(C.INDEX_PATHS)
        Mn.main(["get_frequencies", "-input_dir", str(inp), "-output_dir", str(out), "-k", "7", "-p", "2"] + extra)
        moved = {p: C.INDEX_PATHS[p] - before[p] for p in before}
        assert moved[want_path] >= 1 and moved["fasta_device"] == 0, moved
        if want_path == "fastq_device":
            assert moved["fastq_host_fallback"] == 0, moved
        for f, b in blobs.items():
            name = f.rsplit(".f", 1)[0]
            c, _ = oracle.count(b, 7)
            assert (out / f"{name}.kf").read_bytes() == oracle.kf_line(name, c, raw_cnt=bool(extra)).encode(), f

    run("norm", [], "fastq_device")
    run("raw", ["-raw_cnt"], "fastq_device")
    blobs["s4.fq"] = gen.random_fastq(rng, 50, multiline=True)
    assert not M.is_regular(blobs["s4.fq"])
    (inp / "s4.fq").write_bytes(blobs["s4.fq"])
    run("fallback", ["-raw_cnt"], "fastq_host_fallback")
