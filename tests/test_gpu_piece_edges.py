"""GPU parity at the edges of the k <= 9 count kernels' per-piece code: wave
ranges split on the 3 KiB iteration lattice (split_at_lattice), the hinted
interval search (interval_after: a 64-interval window from the wave's previous
cursor, then the search over the rest) and the two-step zeroing of the flush.
Every count is compared bit for bit against the CPU oracle, as in
test_gpu_parity.py.  Run on an MI355X: `pytest -m gpu`."""
import numpy as np
import pytest

import gen
from test_gpu_parity import counter, torch_dev  # noqa: F401  (torch_dev: the module's fixture)

pytestmark = pytest.mark.gpu

KS = [3, 7, 8, 9]
# genome lengths in bytes around the lattice: below / at / above one and two
# 3 KiB iterations, 16 iterations (one per wave), 32, and a pad-sized one
LATTICE_LENGTHS = [1, 15, 3071, 3072, 3073, 6143, 6145, 49151, 49152, 49153, 98304 - 17, 98304 + 17, 150001]

_oracle_cache = {}


def oracle_count(oracle, blob, k, fmt=0):
    """The oracle's (counts, total) of a blob, computed once per (blob, k, fmt)."""
    key = (id(blob), k, fmt)
    if key not in _oracle_cache:
        _oracle_cache[key] = (blob,) + tuple(oracle.count(blob, k, fmt))   # (the blob is kept: its id stays its own)
    return _oracle_cache[key][1:]


def check(oracle, blobs, k, counts, totals, fmt=0, scale=1, tag=""):
    for i, b in enumerate(blobs):
        c, t = oracle_count(oracle, b, k, fmt)
        assert int(totals[i]) == scale * t, (tag, k, i, len(b), int(totals[i]), scale * t)
        if not (counts[i] == scale * c).all():
            bad = np.nonzero(counts[i] != scale * c)[0]
            pytest.fail(f"{tag} genome {i} ({len(b)} bytes) k={k}: {bad.size} bins differ, e.g. cols "
                        f"{bad[:5].tolist()} got {counts[i][bad[:5]].tolist()} want {(scale * c[bad[:5]]).tolist()}")


def genome_of(rng, nbytes, width):
    """A one-record FASTA genome of exactly nbytes bytes (its last line cut short)."""
    if nbytes < 4:
        return b"ACG"[:nbytes]
    return (b">h\n" + gen.wrap(gen.random_seq(rng, nbytes, n_rate=0.0005), width))[:nbytes]


def device_batch(blobs, gaps, dev, fmt=0):
    """Blobs at explicit (unaligned) offsets: blob i ends gaps[i] bytes before the next."""
    import torch
    from kf2vecfsw_amd import counter as C
    off = [0]
    for b, g in zip(blobs, gaps):
        off.append(off[-1] + len(b) + int(g))
    data = torch.full(((off[-1] + 15) // 16 * 16 + 16,), 10, dtype=torch.uint8)
    d = data.numpy()
    ex = []
    for i, b in enumerate(blobs):
        d[off[i]: off[i] + len(b)] = np.frombuffer(b, np.uint8)
        ex.append(C.index_records(d[off[i]: off[i] + len(b)], fmt, off[i])[0])
    excl = np.concatenate(ex).astype(np.uint64) if ex else np.zeros(0, np.uint64)
    # genome i = [off[i], off[i] + len): the gap bytes are newlines of genome i, which count nothing
    hb = C.HostBatch(data, np.asarray(off, np.uint64), excl, [str(i) for i in range(len(blobs))])
    return C.to_device(hb, dev)


def count(db, k, dev, into=None, accumulate=False):
    import torch
    from kf2vecfsw_amd import counter as C
    if into is None:
        cnt, tot = counter(k, dev).count(db)
    else:
        cnt, tot = counter(k, dev).count(db, into[0], into[1], accumulate=accumulate)
    torch.cuda.synchronize()
    return cnt, tot, C.counts_to_numpy(cnt), tot.cpu().numpy()


@pytest.fixture(scope="module")
def lattice(torch_dev):
    """The lattice genomes (every length at line widths 60 and 80, three times:
    about 3.1 MB, so every genome but the smallest is split over several of the
    256 workgroups) and the same genomes among 600 pad genomes of about 150 kB
    (about 90 MB: a span holds whole genomes with a partial piece at each end)."""
    rng = np.random.default_rng(3072)
    small = [genome_of(rng, L, w) for _ in range(3) for L in LATTICE_LENGTHS for w in (60, 80)]
    order = rng.permutation(len(small))
    small = [small[i] for i in order]
    pads = [genome_of(rng, L, w) for L, w in ((150001, 80), (149983, 60), (150032, 80))]
    padded = []
    for i in range(600):
        padded.append(pads[i % 3])
        if i % 6 == 0 and i // 6 < len(small):
            padded.append(small[i // 6])
    padded += small[100:]
    g_small = rng.integers(0, 41, size=len(small))
    g_pad = rng.integers(0, 41, size=len(padded))
    return {"small": (small, device_batch(small, g_small, torch_dev)),
            "padded": (padded, device_batch(padded, g_pad, torch_dev))}


@pytest.mark.parametrize("k", KS)
def test_lattice_small_batch(torch_dev, oracle, lattice, k):
    """Every genome split over several workgroups: pieces of a few iterations,
    some waves with empty ranges, a piece end one byte off the lattice."""
    blobs, db = lattice["small"]
    assert 2_000_000 < int(db.off[-1]) < 4_000_000
    _, _, counts, totals = count(db, k, torch_dev)
    check(oracle, blobs, k, counts, totals, tag="lattice-small")


@pytest.mark.parametrize("k", KS)
def test_lattice_padded_batch_and_accumulate(torch_dev, oracle, lattice, k):
    """Whole genomes inside a span (plain row stores) with partial pieces at both
    ends of it; then the same batch added on top with KF_ACCUMULATE, which sends
    the whole pieces through the atomic flush: every row doubles."""
    blobs, db = lattice["padded"]
    assert len(blobs) > 600 and 80_000_000 < int(db.off[-1]) < 100_000_000
    cnt, tot, counts, totals = count(db, k, torch_dev)
    check(oracle, blobs, k, counts, totals, tag="lattice-padded")
    _, _, counts, totals = count(db, k, torch_dev, into=(cnt, tot), accumulate=True)
    check(oracle, blobs, k, counts, totals, scale=2, tag="lattice-accumulate")


def test_lattice_deterministic(torch_dev, lattice):
    import torch
    for name in ("small", "padded"):
        db = lattice[name][1]
        for k in (7, 9):
            a, ta, _, _ = count(db, k, torch_dev)
            a, ta = a.clone(), ta.clone()
            b, tb, _, _ = count(db, k, torch_dev)
            assert torch.equal(a, b) and torch.equal(ta, tb), (name, k)


def many_records(rng, n, base_len, tail=0):
    """n records of base_len bases each (headers: dense excluded intervals), then
    one record of `tail` bases."""
    seq = gen.random_seq(rng, n * base_len).tobytes()
    out = [b">r%d\n" % i + seq[i * base_len: (i + 1) * base_len] + b"\n" for i in range(n)]
    if tail:
        out.append(b">long\n" + gen.wrap(gen.random_seq(rng, tail), 80))
    return b"".join(out)


@pytest.mark.parametrize("k", [7, 9])
def test_hint_window_dense_headers(torch_dev, oracle, k):
    """Genomes of about 5,000 records of 30 bases followed by one 200 kB record,
    40 of them (about 16 MB, spans of about 60 kB = 1,600 headers): a wave's range
    in the dense part of a genome starts hundreds of intervals past its cursor in
    the previous piece (the 200 kB record of the genome before), so the 64-interval
    window misses and the search over the rest runs; inside the long record the
    window holds no interval that ends after the range start at all."""
    rng = np.random.default_rng(640 + k)
    kinds = [many_records(rng, n, 30, tail=200_000) for n in (5000, 4300, 5600)]
    blobs = [kinds[i % 3] for i in range(40)]
    db = device_batch(blobs, rng.integers(0, 41, size=len(blobs)), torch_dev)
    assert db.n_excl > 64 * 1000
    _, _, counts, totals = count(db, k, torch_dev)
    check(oracle, blobs, k, counts, totals, tag="hint-dense")


@pytest.mark.parametrize("k", [7, 9])
def test_hint_window_fastq_reads(torch_dev, oracle, k):
    """A FASTQ batch of a few thousand short reads, indexed as FASTQ (format 2:
    excluded intervals at every read, every wave range starts many intervals
    past the last) and with the format forced to 1 (the same bytes read as
    FASTA: nothing excluded, quality lines counted where they spell bases)."""
    rng = np.random.default_rng(650 + k)
    blobs = [gen.random_fastq(rng, 400, n_rate=0.01, multiline=bool(i % 2)) for i in range(8)]
    for fmt in (2, 1):
        db = device_batch(blobs, [0] * len(blobs), torch_dev, fmt=fmt)
        assert fmt != 2 or db.n_excl >= 3000
        _, _, counts, totals = count(db, k, torch_dev)
        check(oracle, blobs, k, counts, totals, fmt=fmt, tag=f"hint-fastq-fmt{fmt}")


@pytest.mark.parametrize("k", [7, 9])
def test_hint_window_headerless_between_many_records(torch_dev, oracle, k):
    """Genomes with no header at all (no interval) between genomes of many short
    records: a range of a headerless genome finds the window's first interval
    already past its end, and the next genome's ranges are many intervals on."""
    rng = np.random.default_rng(660 + k)
    dense = [many_records(rng, n, 45) for n in (900, 1500)]
    bare = [gen.wrap(gen.random_seq(rng, L), 60) for L in (70_001, 20_000)]
    blobs = [(dense if i % 2 == 0 else bare)[(i // 2) % 2] for i in range(48)] + [bare[0], bare[1], dense[0]]
    db = device_batch(blobs, rng.integers(0, 41, size=len(blobs)), torch_dev)
    _, _, counts, totals = count(db, k, torch_dev)
    check(oracle, blobs, k, counts, totals, tag="hint-bare")


@pytest.mark.parametrize("k", [7, 9])
def test_no_excluded_intervals(torch_dev, oracle, k):
    """A batch with n_excl == 0: the window loads nothing and every search ends at 0."""
    rng = np.random.default_rng(670 + k)
    blobs = [gen.wrap(gen.random_seq(rng, int(L), n_rate=0.001), 80) for L in rng.integers(1, 90_000, size=60)]
    db = device_batch(blobs, rng.integers(0, 41, size=len(blobs)), torch_dev)
    assert db.n_excl == 0
    _, _, counts, totals = count(db, k, torch_dev)
    check(oracle, blobs, k, counts, totals, tag="no-excl")


def test_pieces_on_both_sides_of_the_lattice_limit(torch_dev, oracle):
    """Pieces above kLatticeMaxIters iterations (2,560 x 3 KiB = 7.5 MiB) keep the
    16-byte split, shorter ones take the lattice: 170 device-generated genomes of
    12 Mbp (2.06 GB, spans of 8.07 MB), so a span that lies inside one genome is
    one piece above the limit and the pieces at genome ends are of every length
    below it.  Every total is L - k + 1; two genomes that hold a whole span and
    one that does not are compared with the oracle bit for bit."""
    import torch
    from kf2vecfsw_amd import counter as C
    n, L = 170, 12_000_000
    db = C.synth_device_batch(n, L, seed0=707, width=80, device=torch_dev)
    off = db.off.cpu().numpy().astype(np.int64)
    grid = counter(7, torch_dev).launch_info()[0]
    total = int(off[-1] - off[0])
    cuts = [int(off[0]) + ((total // grid * b + (total % grid) * b // grid) & ~15) for b in range(grid)] + [int(off[-1])]
    assert min(b - a for a, b in zip(cuts, cuts[1:])) > 2560 * 3072
    holds = [any(off[g] <= a and b <= off[g + 1] for a, b in zip(cuts, cuts[1:])) for g in range(n)]
    pick = [g for g in range(n) if holds[g]][:2] + [g for g in range(n) if not holds[g]][:1]
    assert len(pick) == 3
    for k in (7, 9):
        cnt, tot = counter(k, torch_dev).count(db)
        torch.cuda.synchronize()
        assert (tot.cpu().numpy() == L - k + 1).all()
        for g in pick:
            c, t = oracle.count(db.data[int(off[g]): int(off[g + 1])].cpu().numpy().tobytes(), k)
            assert t == L - k + 1 and (C.counts_to_numpy(cnt[g]) == c).all(), (k, g)
        del cnt, tot
    del db
    torch.cuda.empty_cache()


def test_drain_across_the_lattice(torch_dev, oracle):
    """One 400 kB poly-A genome and one random genome at k = 7: the u16 halves of
    AAAAAAAA drain (0x4000 at a time) in ranges that now end on iteration
    boundaries, i.e. from fast iterations only, and the flush adds with atomics."""
    rng = np.random.default_rng(680)
    blobs = [b">polyA\n" + gen.wrap(np.frombuffer(b"A" * 400_000, np.uint8), 80),
             b">r\n" + gen.wrap(gen.random_seq(rng, 300_000), 80)]
    for gaps in ([0, 0], [7, 0]):
        db = device_batch(blobs, gaps, torch_dev)
        _, _, counts, totals = count(db, 7, torch_dev)
        check(oracle, blobs, 7, counts, totals, tag="drain")
