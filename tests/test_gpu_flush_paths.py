"""GPU parity of the k <= 6 piece flush (x_flush -> flush_small_pairs) on rows
that a drain has already written.  At k <= 6 a u16 half of the pair table drains
at 0x8000 (kHot6): x_drain adds the drained step to the count row while the
piece is still being counted, so the flush of that piece must add with atomics
even when the workgroup holds the whole genome -- a plain store would overwrite
what the drain put there.  The other drain tests pin k = 7, 8 or 9.  Every count
is compared bit for bit against the CPU oracle, as in test_gpu_piece_edges.py.
Run on an MI355X: `pytest -m gpu`."""
import numpy as np
import pytest

import gen
from test_gpu_parity import counter, torch_dev  # noqa: F401  (torch_dev: the module's fixture)
from test_gpu_piece_edges import check, count, device_batch

pytestmark = pytest.mark.gpu

WIDTH = 70
# 70,000 bases are above the 65,536 windows (32,768 pairs) at which the half of
# the (k+1)-mer TT..T reaches 0x8000
MIN_BASES, MAX_BASES = 70_000, 100_000
# A poly-T piece of this many bytes has drained for certain when its flush
# starts: a 71-byte line is about 4.4 16-byte regions of 8 pairs each (7 and a
# single in the one with the newline), 0.486 pairs per byte; the piece's first and
# last 3 KiB iteration may count singles only: (80,000 - 6,144) x 0.486 = 35,900
# adds to the one half, above 32,768
DRAINED_PIECE_BYTES = 80_000
MID_BASES = 60_000   # a random genome of this size drains nothing (4^(k+1) >= 64 halves share its pairs)
MID_EVERY = 5        # one after every fifth poly-T genome
MAX_GAP = 40
SEED = 6000

_batches = {}


def poly_t(n):
    line = b"T" * WIDTH + b"\n"
    return b">t\n" + line * (n // WIDTH) + (b"T" * (n % WIDTH) + b"\n" if n % WIDTH else b"")


def spans(off, grid):
    """The workgroups' byte spans (wg_span of kf_count.hip, restated)."""
    total = int(off[-1] - off[0])
    cuts = [int(off[0]) + ((total // grid * b + (total % grid) * b // grid) & ~15) for b in range(grid)]
    cuts.append(int(off[-1]))
    return list(zip(cuts, cuts[1:]))


def layout(grid):
    """The batch for a grid, on the host: (blobs, gaps, offsets, kinds).
    3 x grid poly-T genomes (a span is about three of them: some lie wholly in
    one span, some are cut by a span edge), a random 60 kbp genome after every
    fifth of them and a random 200 kbp genome at each end of the batch.  The
    asserts are on the offsets alone: nothing has touched the GPU yet."""
    rng = np.random.default_rng(SEED)
    ends = [b">r\n" + gen.wrap(gen.random_seq(rng, 200_000), WIDTH) for _ in range(2)]
    mids = [b">m\n" + gen.wrap(gen.random_seq(rng, MID_BASES), WIDTH) for _ in range(3)]
    blobs, kinds = [ends[0]], ["end"]
    for i, n in enumerate(rng.integers(MIN_BASES, MAX_BASES + 1, size=3 * grid)):
        blobs.append(poly_t(int(n)))
        kinds.append("poly")
        if i % MID_EVERY == MID_EVERY - 1:
            blobs.append(mids[(i // MID_EVERY) % 3])
            kinds.append("mid")
    blobs.append(ends[1])
    kinds.append("end")
    gaps = rng.integers(0, MAX_GAP + 1, size=len(blobs))
    # genome i = [off[i], off[i + 1]): its bytes, then gaps[i] newlines (as device_batch lays them out)
    off = np.concatenate([[0], np.cumsum([len(b) + int(g) for b, g in zip(blobs, gaps)])]).astype(np.int64)
    sp = spans(off, grid)

    def span_of(g):   # the span that holds all of genome g, or None
        return next(((a, b) for a, b in sp if a <= off[g] and off[g + 1] <= b), None)

    poly = [g for g, kd in enumerate(kinds) if kd == "poly"]
    whole = [g for g in poly if span_of(g)]
    cut = [g for g in poly if any(off[g] < a < off[g + 1] for a, _ in sp)]
    # a random genome wholly in a span (no drain: plain stores), directly after
    # a poly-T piece of the same span that has drained: its flush finds the
    # flag words and F's words of the drained piece zeroed, or counts them
    follows = [g for g, kd in enumerate(kinds) if kd == "mid" and kinds[g - 1] == "poly" and span_of(g)
               and off[g] - MAX_GAP - max(off[g - 1], span_of(g)[0]) >= DRAINED_PIECE_BYTES]
    # (a failure here asks for another SEED, not for a weaker assertion)
    assert whole and cut and follows, (grid, len(whole), len(cut), len(follows))
    assert set(whole).isdisjoint(cut) and len(whole) + len(cut) == len(poly)
    return blobs, gaps, off, kinds


def batch_for(grid, dev):
    """The layout of a grid on the device, one batch per grid shared by every k."""
    if grid not in _batches:
        blobs, gaps, off, _ = layout(grid)
        db = device_batch(blobs, gaps, dev)
        assert (db.off.cpu().numpy().astype(np.int64) == off).all()
        _batches[grid] = (blobs, db)
    return _batches[grid]


@pytest.mark.parametrize("k", [2, 3, 4, 5, 6])
def test_small_pairs_flush_on_drained_rows(torch_dev, oracle, k):
    """Poly-T genomes of 70,000 to 100,000 bases at k <= 6: a whole genome in one
    span that drained (atomics, not the plain store its `whole` alone would
    take), genomes cut by a span edge (atomics from two workgroups), and a random
    genome wholly in a span directly after a drained poly-T piece of the same
    workgroup (the table and the drain flags of the piece before are zero again:
    plain stores of its own counts).  Then the same batch once more with
    KF_ACCUMULATE onto those rows: every row doubles."""
    grid = counter(k, torch_dev).launch_info()[0]
    blobs, db = batch_for(grid, torch_dev)
    cnt, tot, counts, totals = count(db, k, torch_dev)
    check(oracle, blobs, k, counts, totals, tag="flush-small")
    _, _, counts, totals = count(db, k, torch_dev, into=(cnt, tot), accumulate=True)
    check(oracle, blobs, k, counts, totals, scale=2, tag="flush-small-accumulate")
