"""GPU parity of the device FASTA record index (kf_index_fasta) against the host
index (kf_index_records) and, through kf_count_batch, against the oracle."""
import numpy as np
import pytest

import gen

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_dev(native):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu tests need an MI355X")
    return torch.device("cuda:0")


def excluded_mask(pairs: np.ndarray, n: int) -> np.ndarray:
    m = np.zeros(n, dtype=bool)
    for s, e in pairs.reshape(-1, 2):
        m[int(s): int(e)] = True
    return m


def corpus(rng):
    blobs = [gen.random_fasta(rng, int(rng.integers(0, 40000)), n_rate=0.01, lower=0.05, crlf_rate=0.2)
             for _ in range(12)]
    blobs += [b"", b">only\n", b">a\n>b\n>c\nACGT\n", b"ACGT>ACGT\n>h>x\nGG>\n", b">no newline at the end",
              b"junk before\n>r1\nACGTACGT\n\n\n>r2 x>y\nTTTT", b">" * 50 + b"\nACGT\n", b"\n>\n>\n\n>\nA"]
    return blobs


def test_device_index_matches_host(torch_dev):
    """The same excluded bytes as the host index on ragged multi-record FASTA:
    headers with '>' inside, consecutive header lines, CRLF, a header at the very
    end without '\\n', bytes before the first header, genomes that end without a
    newline right before the next genome's '>'."""
    import torch
    from kf2vecfsw_amd import counter as C
    rng = np.random.default_rng(41)
    blobs = corpus(rng)
    hb_host = C.pack_genomes(blobs)
    hb = C.HostBatch(hb_host.data, hb_host.off, None, hb_host.names)
    db = C.to_device(hb, torch_dev)
    torch.cuda.synchronize()
    n = int(hb.off[-1])
    # the host merges header lines that follow each other (their '\n' inside the
    # merged range); newlines are transparent either way, so compare the rest
    nl = hb_host.data.numpy()[:n] == 10
    got = excluded_mask(db.excl[: 2 * db.n_excl].cpu().numpy(), n)
    exp = excluded_mask(hb_host.excl, n)
    assert np.array_equal(got & ~nl, exp & ~nl)
    pairs = db.excl[: 2 * db.n_excl].cpu().numpy()
    assert np.all(np.diff(pairs) >= 0)   # sorted, disjoint
    # genomes packed without '\n' padding between them: the next genome's '>' starts a header
    tight = [b"ACGTACGTACGTACGT", b">x\nACGT\n", b"CCCCCCCCCCCCCCCC", b">y\nGG"]
    off = np.cumsum([0] + [len(b) for b in tight]).astype(np.uint64)
    data = torch.full((int(off[-1]) + 16,), 10, dtype=torch.uint8)
    data.numpy()[: int(off[-1])] = np.frombuffer(b"".join(tight), np.uint8)
    db = C.to_device(C.HostBatch(data, off, None, ["t"] * 4), torch_dev)
    pairs = db.excl[: 2 * db.n_excl].cpu().numpy().tolist()
    assert pairs == [16, 18, 40, 42], pairs


@pytest.mark.parametrize("k", [7, 11])
def test_device_index_counts_equal_oracle(torch_dev, oracle, k):
    """kf_count_batch over the device index == the oracle, genome by genome."""
    import torch
    from kf2vecfsw_amd import counter as C
    rng = np.random.default_rng(43 + k)
    blobs = corpus(rng)
    hb_host = C.pack_genomes(blobs)
    db = C.to_device(C.HostBatch(hb_host.data, hb_host.off, None, hb_host.names), torch_dev)
    cnt, tot = C.KmerCounter(k, torch_dev).count(db)
    torch.cuda.synchronize()
    c = C.counts_to_numpy(cnt)
    t = tot.cpu().numpy()
    for i, b in enumerate(blobs):
        oc, ot = oracle.count(b, k)
        assert int(t[i]) == ot, (i, int(t[i]), ot)
        assert np.array_equal(c[i], oc), i


def test_device_index_table_regrows(torch_dev):
    """More header lines than the first table holds (one per 4 bytes): the index
    is run again with a table of the reported size."""
    import torch
    from kf2vecfsw_amd import counter as C
    blob = b"".join(b">%d\nA\n" % i for i in range(30000))
    hb_host = C.pack_genomes([blob])
    db = C.to_device(C.HostBatch(hb_host.data, hb_host.off, None, ["x"]), torch_dev)
    torch.cuda.synchronize()
    assert db.n_excl == 30000
    n = int(hb_host.off[-1])
    nl = hb_host.data.numpy()[:n] == 10
    got = excluded_mask(db.excl[: 2 * db.n_excl].cpu().numpy(), n)
    assert np.array_equal(got & ~nl, excluded_mask(hb_host.excl, n) & ~nl)


def test_device_index_scan_carry_past_1024_blocks(torch_dev):
    """One batch of 2,050 index blocks of 4 KiB (2 x 1024 x 4096 + 4096 + 5 bytes),
    so the one-workgroup block scan runs three 1,024-block iterations and the pairs
    of blocks 1024.. and 2048.. depend on its carry.  Two genomes; header lines
    start in blocks 0, 1023, 1024, 2047, 2048 and 2049: one '>' is the last byte
    of block 1023 (its line runs to the genome end, no newline) and the second
    genome's '>' is the first byte of block 1024 with no newline before it."""
    import torch
    from kf2vecfsw_amd import counter as C
    from kf2vecfsw_amd import _native as N
    B = 4096
    n = 2 * 1024 * B + B + 5
    g1 = 1024 * B                                   # start of the second genome
    rng = np.random.default_rng(47)
    d = gen.BASES[rng.integers(0, 4, size=n)].copy()
    d[60::61] = 10
    exp = []

    def header(at, text, newline=True):             # a header line at `at` (a line start)
        if at not in (0, g1):
            d[at - 1] = 10
        d[at: at + len(text)] = np.frombuffer(text, np.uint8)
        if newline:
            d[at + len(text)] = 10
        exp.extend([at, at + len(text)])

    header(0, b">g0 first")                          # block 0
    header(g1 - 1, b">", newline=False)              # last byte of block 1023, ends with its genome
    header(g1, b">g1 no newline before")             # first byte of block 1024
    header(2047 * B + 100, b">in 2047")
    header(2048 * B + 7, b">in 2048 > x")
    header(n - 4, b">end", newline=False)            # block 2049 (5 bytes), runs to the batch end
    assert [e // B for e in exp[0::2]] == [0, 1023, 1024, 2047, 2048, 2049]
    assert d[g1 - 2] == 10 and d[g1 - 1] == ord(">") and d[g1] == ord(">")
    off = np.array([0, g1, n], dtype=np.uint64)
    data = torch.full((n + 16,), 10, dtype=torch.uint8)
    data.numpy()[:n] = d
    db = C.to_device(C.HostBatch(data, off, None, ["a", "b"]), torch_dev)
    torch.cuda.synchronize()
    pairs = db.excl[: 2 * db.n_excl].cpu().numpy()
    assert pairs.tolist() == exp, (pairs.tolist(), exp)
    host = np.concatenate([C.index_records(d[int(off[i]): int(off[i + 1])], N.KF_FMT_FASTA, int(off[i]))[0]
                           for i in range(2)])
    nl = d == 10
    assert np.array_equal(excluded_mask(pairs, n) & ~nl, excluded_mask(host, n) & ~nl)


# ------------------------------------------------------------------ exact pairs
def device_pairs(dev, data: np.ndarray, off) -> list:
    """counter.index_on_device on a buffer of exactly off[-1] bytes: the pairs as a list."""
    import torch
    from kf2vecfsw_amd import counter as C
    off = np.asarray(off, dtype=np.int64)
    n = int(off[-1])
    assert data.size == n
    d = torch.from_numpy(np.ascontiguousarray(data)).to(dev)
    with torch.cuda.device(dev):
        excl, m = C.index_on_device(d, torch.from_numpy(off).to(dev), off.size - 1, n)
    pairs = excl.cpu().numpy().tolist()
    assert len(pairs) == 2 * m
    return pairs


def strings6() -> np.ndarray:
    """All 4^6 = 4,096 strings of length 6 over ">A\\n\\r", [4096, 6]."""
    x = np.arange(4 ** 6)
    digits = np.stack([(x // 4 ** (5 - p)) % 4 for p in range(6)], axis=1)
    return np.frombuffer(b">A\n\r", np.uint8)[digits]


@pytest.mark.parametrize("layout", ["one_genome", "genome_per_string", "genome_per_3_strings"])
def test_device_index_exact_pairs_every_6_byte_string(torch_dev, layout):
    """The pairs themselves (not the mask of excluded bytes) equal gen.header_pairs
    on every string of length 6 over ">A\\n\\r", back to back after 0..15 bytes
    'A' (every phase of a thread's 16 bytes): a pair that ends a byte late on its
    '\\n', or a header split in two, fails here.  With a genome boundary at every
    string's start (unaligned offsets: a '>' whose predecessor is not '\\n' is a
    header only if the binary search finds a genome start there) and at every
    third string."""
    body = strings6().reshape(-1)
    every = {"one_genome": 4096, "genome_per_string": 1, "genome_per_3_strings": 3}[layout]
    n_pairs = 0
    for pad in range(16):
        data = np.concatenate([np.full(pad, ord("A"), np.uint8), body])
        off = sorted({0, data.size} | ({pad + 6 * s for s in range(0, 4096, every)} if every < 4096 else set()))
        exp = gen.header_pairs(data, off)
        assert device_pairs(torch_dev, data, off) == exp, (layout, pad)
        n_pairs += len(exp) // 2
    assert n_pairs > 16 * 1000, n_pairs


INDEX_MOTIFS = [b">", b">\n", b"\n>", b"A>", b"\r>", b">>\n>", b"\n>hd"]


@pytest.mark.parametrize("boundary", [False, True])
def test_device_index_exact_pairs_across_tile_edges(torch_dev, boundary):
    """'>' alone, before and after a '\\n', after 'A' and '\\r', doubled, and a header
    that runs to its genome's end, with each byte in turn first after a thread,
    wave and workgroup edge (16, 1024, 4096, 8192); with a genome boundary exactly
    on the edge, and with none."""
    places = [(E, m, k) for E in (16, 1024, 4096, 8192) for m in INDEX_MOTIFS for k in range(len(m) + 1)]
    data = np.full((len(places) + 2) * 3 * 4096, ord("A"), np.uint8)
    data[97::101] = 10
    cuts = {0, data.size}
    for c, (E, m, k) in enumerate(places):
        edge = (c + 1) * 3 * 4096 + E                 # the copies are three workgroup spans apart
        data[edge - 8: edge + 8] = ord("A")
        data[edge - k: edge - k + len(m)] = np.frombuffer(m, np.uint8)
        if boundary:
            cuts.add(edge)
    off = sorted(cuts)
    exp = gen.header_pairs(data, off)
    assert len(exp) // 2 >= len(places) // 2
    assert device_pairs(torch_dev, data, off) == exp


def test_device_index_cap_pairs(torch_dev):
    """kf_index_fasta with a table of exactly m pairs, of m - 1 (the count is still
    m, the first m - 1 pairs are right and nothing is written from entry 2 (m - 1)
    on) and of none (a null table: only the count)."""
    import torch
    from kf2vecfsw_amd import _native as N
    data = np.concatenate([np.full(5, ord("A"), np.uint8), strings6().reshape(-1)])
    off = np.asarray(sorted({0, data.size} | {5 + 18 * s for s in range(1366)}), dtype=np.int64)
    exp = gen.header_pairs(data, off)
    m, n = len(exp) // 2, int(data.size)
    assert m > 1000
    d = torch.from_numpy(data).to(torch_dev)
    d_off = torch.from_numpy(off).to(torch_dev)
    words = (n + 4095) // 4096 + 1
    scratch = torch.empty(words, dtype=torch.int32, device=torch_dev)
    mark = -0x5A5A5A5A5A5A5A5B
    for cap, null_table in ((m, False), (m - 1, False), (0, True)):
        table = torch.full((2 * m + 8,), mark, dtype=torch.int64, device=torch_dev)
        count = torch.full((1,), mark, dtype=torch.int64, device=torch_dev)
        N.check(N.lib().kf_index_fasta(d.data_ptr(), d_off.data_ptr(), off.size - 1, n,
                                       None if null_table else table.data_ptr(), cap, count.data_ptr(),
                                       scratch.data_ptr(), words, torch.cuda.current_stream(torch_dev).cuda_stream),
                "kf_index_fasta")
        torch.cuda.synchronize()
        assert int(count.item()) == m, cap
        got = table.cpu().numpy()
        assert got[: 2 * cap].tolist() == exp[: 2 * cap], cap
        assert (got[2 * cap:] == mark).all(), cap
