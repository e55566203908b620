"""GPU parity at the edges of the bucket count kernels (k = 10, 11, 12;
bucket_kernel<K> in csrc/kf_bucket.hip): rounds whose windows all fall into one
bucket, pieces at the size limit kPieceMax, the phase-2 round shares of the 16
waves (rw0 / rw1) over a lattice of round counts, piece and wave boundaries
(split_at) placed against headers, N runs and newline runs, a count after
kf_workspace_release, and a piece table of more than 2,048 genomes (three rounds
of piece_scan_kernel).  Every count row and total is compared bit for bit
against the CPU oracle, as in test_gpu_parity.py.  Run on an MI355X:
`pytest -m gpu`."""
import numpy as np
import pytest

import gen
from test_gpu_parity import counter, torch_dev  # noqa: F401  (torch_dev: the module's fixture)
from test_gpu_piece_edges import _oracle_cache, check, count, device_batch, genome_of, oracle_count

pytestmark = pytest.mark.gpu

KS = [10, 11, 12]
P = 8_323_072          # kPieceMax of kf_bucket.hip: 8 MiB - 64 KiB, the largest piece of one workgroup
ROUND = 16 * 1024      # bytes of one round: one 1 KiB chunk per wave
BUCKET_BITS = 15       # kBkBits: a bucket is 32,768 consecutive standard codes


def forget(blobs, k):
    """Drop the oracle rows of a finished test (33.5 MB each at k = 12)."""
    for b in blobs:
        _oracle_cache.pop((id(b), k, 0), None)


_buckets = {}


def column_buckets(oracle, k):
    """Bucket of every column: the standard code (A0 C1 G2 T3, first base highest)
    of its vocab line, shifted right by 15."""
    if k not in _buckets:
        v = np.frombuffer(oracle.vocab_text(k), np.uint8).reshape(-1, k + 1)[:, :k]
        lut = np.zeros(256, np.uint32)
        lut[list(b"ACGT")] = [0, 1, 2, 3]
        code = np.zeros(v.shape[0], np.uint32)
        for i in range(k):
            code = (code << 2) | lut[v[:, i]]
        _buckets[k] = code >> BUCKET_BITS
    return _buckets[k]


def buckets_hit(oracle, row, k):
    return set(np.unique(column_buckets(oracle, k)[np.nonzero(row)[0]]).tolist())


def rep(unit, n):
    return np.frombuffer(unit * n, np.uint8)


# ------------------------------------------------------------------ 1. skew
# name -> buckets hit at k = 10, 11, 12
SKEW_BUCKETS = {
    "A": ({0}, {0}, {0}),
    "T": ({0}, {0}, {0}),                      # its canonical form is poly-A
    "C": ({10}, {42}, {170}),
    "TA": ({6, 25}, {25}, {102, 409}),
    "AC": ({2, 8}, {8, 34}, {34, 136}),
}
LAST_VOCAB = {10: b"TTTTTAAAAA", 11: b"TTTTTCAAAAA", 12: b"TTTTTTAAAAAA"}


def skew_inputs(k):
    """[(name, blob)] of the skew batch at k (only the last-bucket genome depends on k)."""
    rng = np.random.default_rng(1500)
    line = lambda unit, n: b">x\n" + unit * n + b"\n"
    out = [("A", line(b"A", 2_000_000)), ("C", line(b"C", 2_000_000)), ("TA", line(b"TA", 1_000_000)),
           ("AC", line(b"AC", 1_000_000)), ("GATTACA", line(b"GATTACA", 300_000)),
           ("last", line(LAST_VOCAB[k] + b"N", 150_000))]
    for name, unit, n in (("T", b"T", 2_000_000), ("TA", b"TA", 1_000_000), ("GATTACA", b"GATTACA", 300_000)):
        out += [(name, b">w%d\n" % w + gen.wrap(rep(unit, n), w)) for w in (60, 61, 70, 80)]
    half = np.concatenate([gen.random_seq(rng, 2_000_000), rep(b"A", 2_000_000)])
    out.append(("half", b">half\n" + gen.wrap(half, 80)))
    out.append(("A20M", b">polyA\n" + gen.wrap(rep(b"A", 20_000_000), 80)))
    rnd = [("rnd", b">r\n" + gen.wrap(gen.random_seq(rng, L), w))
           for L, w in ((100_003, 60), (300_000, 80), (177_777, 61), (250_001, 70))]
    for i, r in enumerate(rnd):            # spread over the batch: pieces on both halves of the grid
        out.insert(5 * i + 2, r)
    return out


def check_skew_guards(oracle, named, k):
    """Conditions on the inputs, from the oracle rows alone."""
    nbk = (1 << (2 * k)) >> BUCKET_BITS
    for name, b in named:
        c, t = oracle_count(oracle, b, k)
        hit = buckets_hit(oracle, c, k)
        if name in SKEW_BUCKETS:
            assert hit == SKEW_BUCKETS[name][k - 10], (name, k, hit)
        elif name == "GATTACA":
            assert np.count_nonzero(c) == 7 and len(hit) == 7, (k, hit)
        elif name == "last":
            assert t == 150_000 and hit == {nbk - 1} and np.count_nonzero(c) == 1, (k, t, hit)
        elif name == "A20M":
            assert -(-len(b) // P) == 3 and int(c.max()) > 1 << 24 and hit == {0}, (k, len(b), int(c.max()))
        elif name == "half":
            assert len(b) < P and len(hit) > nbk // 2 and int(c[0]) > 1_900_000, (k, len(hit))


@pytest.mark.parametrize("k", KS)
def test_single_bucket_rounds(torch_dev, oracle, k):
    """Homopolymers, tandem repeats and a repeat of the last vocab line: rounds
    whose 16,384 windows all fall into one or two buckets (one rank counter, or
    its 16 replicas at k = 10, takes every add; one run of 2,048 units, every
    other run empty), unwrapped (the dense path without a newline) and wrapped;
    a piece that is half random, half poly-A; 20 Mbp of poly-A in three pieces
    (atomic flushes into one bin past 2^24).  Twice (equal), then accumulated
    on top (exactly double)."""
    import torch
    named = skew_inputs(k)
    blobs = [b for _, b in named]
    check_skew_guards(oracle, named, k)
    rng = np.random.default_rng(1510 + k)
    db = device_batch(blobs, rng.integers(0, 41, size=len(blobs)), torch_dev)
    a, ta, counts, totals = count(db, k, torch_dev)
    check(oracle, blobs, k, counts, totals, tag="skew")
    del counts
    b, tb, _, _ = count(db, k, torch_dev)
    assert torch.equal(a, b) and torch.equal(ta, tb), k
    del a, ta
    _, _, counts, totals = count(db, k, torch_dev, into=(b, tb), accumulate=True)
    check(oracle, blobs, k, counts, totals, scale=2, tag="skew-accumulate")
    forget(blobs, k)


# ------------------------------------------------------- 2. piece-size limits
@pytest.fixture(scope="module")
def limit_master():
    """One genome of 2 P + 1 bytes; genome_of(L) is its first L bytes."""
    return genome_of(np.random.default_rng(8323), 2 * P + 1, 80)


@pytest.mark.parametrize("k", KS)
def test_piece_size_limits(torch_dev, oracle, limit_master, k):
    """Genomes of exactly kPieceMax bytes (one piece of 508 rounds at an aligned
    start, of 509 rounds at a start = 5 mod 16: the longest a piece gets; the
    record slot, meta and roff hold Bk::rmax = 510) and of one byte less and
    more (two half pieces), 2 kPieceMax (two full pieces) and 2 kPieceMax + 1
    (three) at k = 10; kPieceMax and kPieceMax + 1 at k = 11, 12."""
    full = limit_master[:P]
    if k == 10:
        blobs = [full, full, limit_master[: P - 1], limit_master[: P + 1], limit_master[: 2 * P], limit_master]
        gaps = [5, 7, 3, 9, 11, 0]
    else:
        blobs = [full, full, limit_master[: P + 1]]
        gaps = [5, 7, 0]
    off = np.concatenate([[0], np.cumsum([len(b) + g for b, g in zip(blobs, gaps)])])
    assert off[0] % 16 == 0 and off[1] % 16 == 5 and all(o % 16 for o in off[1:-1])
    assert [-(-len(b) // P) for b in blobs] == ([1, 1, 1, 2, 2, 3] if k == 10 else [1, 1, 2])
    db = device_batch(blobs, gaps, torch_dev)
    cnt, tot, counts, totals = count(db, k, torch_dev)
    check(oracle, blobs, k, counts, totals, tag="piece-limit")
    _, _, counts, totals = count(db, k, torch_dev, into=(cnt, tot), accumulate=True)
    check(oracle, blobs, k, counts, totals, scale=2, tag="piece-limit-accumulate")
    forget(blobs, k)


# ------------------------------------------------------ 3. round-count lattice
LATTICE_ROUNDS = [1, 2, 15, 16, 17, 47, 48, 63, 64, 65]
# A piece of 16384 r + d bytes at any start: r rounds at d = -512 (every wave
# range, its 16-byte alignment slack included, stays within r chunks), r + 1 at
# d = 17 (the 16 ranges cover more than 16 r chunks), r or r + 1 in between.
LATTICE_DELTAS = (-512, -17, 0, 17)


@pytest.fixture(scope="module")
def round_lattice(torch_dev):
    """Single-piece genomes of 16384 r + d bytes, line widths 60 and 80
    alternating so that every r has both, shuffled, at unaligned offsets."""
    rng = np.random.default_rng(16384)
    blobs = [genome_of(rng, ROUND * r + d, (60, 80)[(i + j) % 2])
             for i, r in enumerate(LATTICE_ROUNDS) for j, d in enumerate(LATTICE_DELTAS)]
    blobs = [blobs[i] for i in rng.permutation(len(blobs))]
    assert max(len(b) for b in blobs) < P
    return blobs, device_batch(blobs, rng.integers(0, 41, size=len(blobs)), torch_dev)


@pytest.mark.parametrize("k", KS)
def test_round_count_lattice(torch_dev, oracle, round_lattice, k):
    """nround = 1 .. 66: phase 2 deals the rounds to the waves by
    kBkRoundWeights (rw0, rw1), so at 15-17 rounds some waves have no run, and
    at 47-65 the oldest waves hold up to seven runs, lane j its run j."""
    blobs, db = round_lattice
    _, _, counts, totals = count(db, k, torch_dev)
    check(oracle, blobs, k, counts, totals, tag="round-lattice")
    forget(blobs, k)


# ------------------------------------------------ 4. boundaries against content
def split_at(plo, phi, w, n):
    """kf_front.h split_at, restated to place features (never asserted on)."""
    if w == 0:
        return plo
    if w >= n:
        return phi
    ln = phi - plo
    s = (plo + ln // n * w + (ln % n) * w // n) & ~15
    return min(max(s, plo), phi)


def boundaries(glo, ghi):
    """The piece boundaries of genome [glo, ghi), then the wave boundaries of every piece."""
    npiece = max(1, -(-(ghi - glo) // P))
    cuts = [split_at(glo, ghi, i, npiece) for i in range(npiece + 1)]
    return cuts[1:-1] + [split_at(a, b, w, 16) for a, b in zip(cuts, cuts[1:]) for w in range(1, 16)]


HDR = b">ACGTTGCA boundary ACGTAC\n"     # bases in the header: counting it would show
N_FEATURES = 7


def plant(a, p, feat, k, rng, width):
    """Overwrite genome bytes `a` around the boundary at local position p."""
    assert 6000 < p < a.size - 2000
    h = np.frombuffer(HDR, np.uint8)
    bases = lambda n: gen.BASES[rng.integers(0, 4, size=n)]
    if feat == 0:      # a header line that straddles the boundary
        s = p - h.size // 2
        a[s - 1], a[s: s + h.size] = 10, h
    elif feat == 1:    # ... that ends exactly at it (its '\n' is the last byte before)
        a[p - h.size - 1], a[p - h.size: p] = 10, h
    elif feat == 2:    # ... that starts exactly at it
        a[p - 1], a[p: p + h.size] = 10, h
    elif feat == 3:    # an N run across it
        a[p - 9: p + 8] = ord("N")
    elif feat == 4:    # a header, then only k - 2 bases before the boundary
        s = p - (k - 2) - h.size
        a[s - 1], a[s: s + h.size], a[p - (k - 2): p] = 10, h, bases(k - 2)
    elif feat == 5:    # k - 1 bases, then 5,000 newlines that end just before the boundary
        a[p - 5000: p] = 10
        a[p - 5000 - (k - 1): p - 5000] = bases(k - 1)
        a[p - 5000 - k] = ord("N")
    else:              # 2 kB of lines of `width` bases across it
        n = 2000 // (width + 1)
        a[p - 1000: p - 1000 + n * (width + 1)] = np.frombuffer(gen.wrap(bases(n * width), width), np.uint8)


def boundary_genome(rng, glo, nbytes, k, shift):
    a = np.frombuffer(genome_of(rng, nbytes, 80), np.uint8).copy()
    feats = set()
    for i, x in enumerate(boundaries(glo, glo + nbytes)):
        feat = (i + k + shift) % N_FEATURES
        plant(a, x - glo, feat, k, rng, (1, 2, 5, 11)[(i // N_FEATURES) % 4])
        feats.add(feat)
    assert len(feats) == N_FEATURES
    return a.tobytes()


@pytest.mark.parametrize("k", KS)
def test_boundaries_against_content(torch_dev, oracle, k):
    """A two-piece genome (kPieceMax + 4096 bytes: 1 piece and 30 wave
    boundaries) and a one-piece genome (15 wave boundaries) with a feature at
    every boundary: header lines across, up to and from it, an N run across it,
    a header k - 2 bases before it, 5,000 newlines before it after k - 1 bases
    (Range::warm walks back five chunks for a context that fills the carry at
    k = 12), lines of 1 to 11 bases across it.  The piece boundary gets the N
    run at k = 10, the short record at k = 11, the newline run at k = 12.
    With the host's record index, then with the device's (kf_index_fasta)."""
    import torch
    from kf2vecfsw_amd import counter as C
    rng = np.random.default_rng(1600 + k)
    la, gap, lb = P + 4096, 7, 1_500_003
    blobs = [boundary_genome(rng, 0, la, k, 0), boundary_genome(rng, la + gap, lb, k, 3)]
    db = device_batch(blobs, [gap, 0], torch_dev)
    assert db.n_excl > 15 and db.off.cpu().numpy().tolist() == [0, la + gap, la + gap + lb]
    _, _, counts, totals = count(db, k, torch_dev)
    check(oracle, blobs, k, counts, totals, tag="boundaries")
    # the same bytes, indexed on the device
    off = np.asarray([0, la + gap, la + gap + lb], np.uint64)
    data = torch.full(((int(off[-1]) + 15) // 16 * 16 + 16,), 10, dtype=torch.uint8)
    for o, b in zip(off, blobs):
        data.numpy()[int(o): int(o) + len(b)] = np.frombuffer(b, np.uint8)
    db2 = C.to_device(C.HostBatch(data, off, None, ["a", "b"]), torch_dev)
    assert db2.n_excl > 15
    _, _, counts, totals = count(db2, k, torch_dev)
    check(oracle, blobs, k, counts, totals, tag="boundaries-device-index")
    forget(blobs, k)


# -------------------------------------------------------- 5. workspace release
def test_count_after_workspace_release(torch_dev, oracle, native):
    """kf_workspace_release frees the bucket tables, the scratch and the piece
    table (the event and the CU count stay): the next count rebuilds them and
    gives the same rows, and so does a count at another k on the fresh scratch.
    (A KmerCounter holds its code2col / col2rep tensors only, nothing of the
    workspace.)"""
    import torch
    rng = np.random.default_rng(1700)
    blobs = [b"", b">t\nACGTACGTACGTA\n", b">r\n" + gen.wrap(gen.random_seq(rng, 300_000, n_rate=0.0005), 80),
             b">big\n" + gen.wrap(gen.random_seq(rng, 9_000_000, n_rate=1e-5), 70)]
    assert -(-len(blobs[3]) // P) == 2
    db = device_batch(blobs, [3, 5, 9, 0], torch_dev)
    a, ta, counts, totals = count(db, 10, torch_dev)
    check(oracle, blobs, 10, counts, totals, tag="before-release")
    assert native.kf_workspace_release() == 0
    b, tb, counts, totals = count(db, 10, torch_dev)
    assert b.data_ptr() != a.data_ptr() and torch.equal(a, b) and torch.equal(ta, tb)
    check(oracle, blobs, 10, counts, totals, tag="after-release")
    _, _, counts, totals = count(db, 11, torch_dev)
    check(oracle, blobs, 11, counts, totals, tag="after-release-k11")
    forget(blobs, 10)
    forget(blobs, 11)


# ------------------------------------------ 6. piece table past two scan rounds
PIECE_TABLE_GENOMES = 2050
PIECE_TABLE_ROWS = (0, 1022, 1023, 1024, 2046, 2047, 2048, 2049)   # around the rounds' ends (1,024 genomes each)


def test_piece_table_third_scan_round(torch_dev, oracle, native):
    """2,050 genomes at k = 10: piece_scan_kernel scans the pieces per genome in
    rounds of 1,024 and carries the sum over, so genomes 2,048 and 2,049 take
    their first piece from the carry of two rounds.  Genomes of 0 to 300 bases,
    two in three with a header, at unaligned offsets; genomes 1,023 and 2,047
    (the last of a round) are empty and still own a piece.  On the device:
    every row's sum equals its total, and both the oracle's total.  The rows
    around the rounds' ends bit for bit; the count matrix (4.3 GB) stays on the
    device."""
    import torch
    from kf2vecfsw_amd import counter as C
    k, n = 10, PIECE_TABLE_GENOMES
    rng = np.random.default_rng(2050)
    blobs = [(b">g%d\n" % i if i % 3 else b"") + gen.wrap(gen.random_seq(rng, int(rng.integers(0, 301))),
                                                          (None, 60, 80)[i % 3]) for i in range(n)]
    gaps = rng.integers(0, 41, size=n)
    for i in (1023, 2047):
        blobs[i], gaps[i] = b"", 0
    db = device_batch(blobs, gaps, torch_dev)
    off = db.off.cpu().numpy()
    assert db.n == n and off[1023] == off[1024] and off[2047] == off[2048]
    want = np.asarray([oracle.count(b, k)[1] for b in blobs], np.int64)
    assert want[1023] == 0 and want[2047] == 0 and want[2048] > 0 and want[2049] > 0 and (want[:2048] > 0).sum() > 1500
    try:
        cnt, tot = counter(k, torch_dev).count(db)
        sums = cnt.sum(dim=1, dtype=torch.int64)
        torch.cuda.synchronize()
        bad = torch.nonzero((sums != tot) | (tot != torch.from_numpy(want).to(torch_dev))).flatten()[:5].tolist()
        assert not bad, [(i, int(sums[i]), int(tot[i]), int(want[i])) for i in bad]
        for i in PIECE_TABLE_ROWS:
            assert (C.counts_to_numpy(cnt[i]) == oracle.count(blobs[i], k)[0]).all(), i
    finally:
        cnt = sums = None
        assert native.kf_workspace_release() == 0
