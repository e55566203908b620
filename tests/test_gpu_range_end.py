"""GPU parity at the ends of the wave ranges of the k <= 9 count kernels.  The
register ring of x_range runs two 3 KiB iterations ahead of the walk and every
load of it is cut at the last 1 KiB third its range consumes, so a clamp that is
off by one shows as counts missing at a range end: these shapes put range ends
everywhere -- ranges shorter than the ring, piece ends at every position of an
iteration, the 16-byte split of long pieces, and the last genome of the buffer.
Every count is compared bit for bit against the CPU oracle, as in
test_gpu_parity.py.  Run on an MI355X: `pytest -m gpu`."""
import numpy as np
import pytest

import gen
from test_gpu_parity import counter, torch_dev  # noqa: F401  (torch_dev: the module's fixture)
from test_gpu_piece_edges import check, count, device_batch, genome_of

pytestmark = pytest.mark.gpu

KS = [3, 7, 8, 9]
ITER = 3072                      # bytes of a wave iteration
WAVES = 16                       # wave ranges per piece
# genome length = WAVES x ITER x m + d: a piece end at, next to and a 1 KiB third or
# a 16-byte unit away from an iteration boundary of the lattice
END_M = [1, 2, 5]
END_D = [-1025, -1024, -1023, -17, -16, -1, 0, 1, 15, 16, 17, 1023, 1024, 1025, 2047, 2048, 2049]


@pytest.fixture(scope="module")
def short(torch_dev):
    """300 genomes of 200 B to 20 kB (about 3 MB: spans of about 12 kB): pieces of
    0 to 7 iterations, so wave ranges of 0, 1 and 2 iterations -- none as long as
    the ring runs ahead -- and waves whose range is empty."""
    rng = np.random.default_rng(1024)
    lens = np.concatenate([[200, 201, 1023, 1024, 1025, 3071, 3072, 3073, 6144, 9216, 20000],
                           rng.integers(200, 20001, size=289)])
    blobs = [genome_of(rng, int(L), (60, 80)[i % 2]) for i, L in enumerate(lens)]
    return blobs, device_batch(blobs, rng.integers(0, 41, size=len(blobs)), torch_dev)


@pytest.fixture(scope="module")
def ends(torch_dev):
    """The range-end genomes (every m, d and line width: 102 genomes, about 13 MB,
    each cut by several of the 256 spans) and the same genomes between pad genomes
    of about 150 kB (about 44 MB: most are whole pieces on the lattice, the spans
    cut the rest)."""
    rng = np.random.default_rng(3 * 1024)
    small = [genome_of(rng, WAVES * ITER * m + d, w) for m in END_M for d in END_D for w in (60, 80)]
    small = [small[i] for i in rng.permutation(len(small))]
    pads = [genome_of(rng, L, w) for L, w in ((150001, 80), (149983, 60), (150032, 80))]
    padded = []
    for i, b in enumerate(small):
        padded += [pads[(2 * i) % 3], b, pads[(2 * i + 1) % 3]]
    return {"alone": (small, device_batch(small, rng.integers(0, 41, size=len(small)), torch_dev)),
            "padded": (padded, device_batch(padded, rng.integers(0, 41, size=len(padded)), torch_dev))}


@pytest.mark.parametrize("k", KS)
def test_ranges_shorter_than_the_ring(torch_dev, oracle, short, k):
    blobs, db = short
    assert len(blobs) == 300 and 2_000_000 < int(db.off[-1]) < 4_000_000
    _, _, counts, totals = count(db, k, torch_dev)
    check(oracle, blobs, k, counts, totals, tag="short")


@pytest.mark.parametrize("k", KS)
def test_range_ends_alone(torch_dev, oracle, ends, k):
    blobs, db = ends["alone"]
    assert len(blobs) == 102 and 12_000_000 < int(db.off[-1]) < 15_000_000
    _, _, counts, totals = count(db, k, torch_dev)
    check(oracle, blobs, k, counts, totals, tag="ends-alone")


@pytest.mark.parametrize("k", KS)
def test_range_ends_between_pads(torch_dev, oracle, ends, k):
    blobs, db = ends["padded"]
    assert len(blobs) == 306 and 40_000_000 < int(db.off[-1]) < 48_000_000
    _, _, counts, totals = count(db, k, torch_dev)
    check(oracle, blobs, k, counts, totals, tag="ends-padded")


@pytest.mark.parametrize("k", KS)
def test_range_ends_accumulate_twice(torch_dev, oracle, ends, k):
    """Two KF_ACCUMULATE calls onto zeroed rows (every piece through the atomic
    flush): exactly twice the counts."""
    import torch
    blobs, db = ends["alone"]
    cnt, tot = counter(k, torch_dev).alloc_out(db.n)
    cnt.zero_()
    tot.zero_()
    count(db, k, torch_dev, into=(cnt, tot), accumulate=True)
    _, _, counts, totals = count(db, k, torch_dev, into=(cnt, tot), accumulate=True)
    torch.cuda.synchronize()
    check(oracle, blobs, k, counts, totals, scale=2, tag="ends-accumulate")


@pytest.mark.parametrize("k", [3, 7, 9])
def test_last_genome_ends_at_the_padding(torch_dev, oracle, k):
    """The batch's last genome ends on the last byte before the buffer's padding
    and its final line is one base long (with and without its newline), at every
    alignment of the batch end that a shift of 0 to 16 bytes gives."""
    rng = np.random.default_rng(4096 + k)
    head = [genome_of(rng, L, 80) for L in (70_001, 5_000)]
    seq = gen.random_seq(rng, 80 * 700 + 1)
    last_nl = b">last\n" + gen.wrap(seq, 80)
    assert last_nl.endswith(b"\n" + seq[-1:].tobytes() + b"\n")
    for last in (last_nl, last_nl[:-1], genome_of(rng, 2 * ITER + 1, 60)[:-2] + b"\nC"):
        for shift in (0, 1, 7, 15, 16):
            blobs = head + [last]
            db = device_batch(blobs, [0, shift, 0], torch_dev)
            assert int(db.off[-1]) + 16 <= db.data.numel() < int(db.off[-1]) + 32
            _, _, counts, totals = count(db, k, torch_dev)
            check(oracle, blobs, k, counts, totals, tag=f"last-shift{shift}")


@pytest.fixture(scope="module")
def tiled(torch_dev):
    """One blob of about 8.1 MB (three records, an odd length) tiled on the device,
    once per workgroup of the grid: the batch passes grid x 7.5 MiB, a span is as
    long as the blob and is cut at most 15 bytes before a genome start, so every
    span holds a piece of a few bytes and one above kLatticeMaxIters iterations,
    which takes the 16-byte split: its range ends fall anywhere in an iteration."""
    import torch
    from kf2vecfsw_amd import counter as C
    rng = np.random.default_rng(8100)
    blob = b"".join(b">rec%d\n" % i + gen.wrap(gen.random_seq(rng, n, n_rate=0.0005), 80)
                    for i, n in enumerate((3_000_000, 4_500_000, 500_000)))
    blob = blob[: len(blob) - 5]   # (ends inside a line; the length is odd)
    L = len(blob)
    assert 8_000_000 < L < 8_200_000 and L % 16 != 0
    n = counter(7, torch_dev).launch_info()[0]
    assert n * L > n * 2560 * ITER
    host = np.frombuffer(blob, np.uint8)
    ex = C.index_records(host, 0, 0)[0].astype(np.int64)
    data = torch.full(((n * L + 15) // 16 * 16 + 16,), 10, dtype=torch.uint8, device=torch_dev)
    data[: n * L].view(n, L).copy_(torch.from_numpy(host.copy()).to(torch_dev).expand(n, L))
    off = torch.arange(n + 1, dtype=torch.int64, device=torch_dev) * L
    excl = (torch.from_numpy(ex).to(torch_dev).view(1, -1) + off[:n].view(n, 1)).reshape(-1).contiguous()
    return blob, C.DeviceBatch(data, off, excl, n, excl.numel() // 2)


@pytest.mark.parametrize("k", [7, 9])
def test_sixteen_byte_split_of_long_pieces(torch_dev, oracle, tiled, k):
    import torch
    blob, db = tiled
    c, t = oracle.count(blob, k)
    cnt, tot = counter(k, torch_dev).count(db)
    torch.cuda.synchronize()
    want = torch.from_numpy(c.view(np.int32)).to(torch_dev)
    bad_t = torch.nonzero(tot != t).flatten()
    bad_c = torch.nonzero((cnt != want).any(dim=1)).flatten()
    assert bad_t.numel() == 0 and bad_c.numel() == 0, (k, bad_t[:8].tolist(), bad_c[:8].tolist())
