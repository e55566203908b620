"""The inputs of the kf_chunk_compact tests, shared by the host tests
(tests/test_host_chunk_compact.py: statement vs per-byte model, fault separation)
and the GPU tests (tests/test_gpu_chunk_compact.py: kernel vs statement).

Every case is (name, data uint8 array, se uint64 [2n]): a buffer and sorted,
disjoint [start, end) ranges inside it, as kf_chunk_compact takes them.  The
kernels tile the buffer by 16 bytes per thread, 1,024 per wave and 4,096 per
workgroup, and scan the workgroups' counts in rounds of 1,024; the groups are
  a  every string of length 5 over "ANn|-\\n\\r", one range each, at every phase of a thread's 16 bytes
  b  hand-made motifs with each of their bytes in turn first after a tile edge
  c  buffer lengths around the block-count edges, with unequal kept counts per block
  d  degenerate inputs
  e  random bytes with random cuts
"""
from __future__ import annotations

import functools

import numpy as np

SPAN = 4096
GROUPS = "abcde"


def _u8(b: bytes) -> np.ndarray:
    return np.frombuffer(b, np.uint8)


def _se(pairs) -> np.ndarray:
    return np.asarray(pairs, dtype=np.uint64).reshape(-1)


# ------------------------------------------------------------------ a
ALPHABET5 = b"ANn|-\n\r"


def _patterns5() -> np.ndarray:
    """All 7^5 = 16,807 strings of length 5 over ALPHABET5, [16807, 5]."""
    x = np.arange(7 ** 5)
    digits = np.stack([(x // 7 ** (4 - p)) % 7 for p in range(5)], axis=1)
    return _u8(ALPHABET5)[digits]


def group_a():
    """The patterns back to back, one range per pattern (the ranges touch), after
    0..15 bytes 'N' that belong to no range; then the same with one byte that
    belongs to no range between consecutive ranges, 'N' and '\\r' in turn."""
    pat = _patterns5()
    n = pat.shape[0]
    between = np.where(np.arange(n) % 2 == 0, ord("N"), ord("\r")).astype(np.uint8)
    cases = []
    for sep in (0, 1):
        body = (np.concatenate([pat, between[:, None]], axis=1) if sep else pat).reshape(-1)
        for pad in range(16):
            data = np.concatenate([np.full(pad, ord("N"), np.uint8), body])
            s = pad + np.arange(n, dtype=np.uint64) * np.uint64(5 + sep)
            cases.append(("a/pad{}{}".format(pad, "/sep" if sep else ""), data,
                          np.stack([s, s + np.uint64(5)], axis=1).reshape(-1)))
    return cases


# ------------------------------------------------------------------ b
EDGES = (16, 1024, 4096, 8192, 12288)
# (content, ranges relative to its first byte); the bytes around a copy are 'N' and belong to no range
MOTIFS = [
    (b"ANNnn||NNA", [(0, 10)]),
    (b"AN\r\nNA", [(0, 6)]),
    (b"AN\r\r\nNA", [(0, 7)]),
    (b"AN\n\n\nNA", [(0, 7)]),
    (b"AN-NA", [(0, 5)]),
    (b"N-.- \tn", [(0, 7)]),
    (b"A|\r\n\r\nnA", [(0, 8)]),
    (b"AA\r", [(0, 3)]),                          # '\r' is the last byte of its range
    (b"AA\r\nA", [(0, 3)]),                       # ... with a '\n' after it that belongs to no range
    (b"AA\rA", [(0, 4)]),                         # a '\r' inside a line stays
    (b"NNNN", [(0, 4)]),                          # a range that starts, and one that ends, at the edge
    (b"NNNNNN", [(0, 3), (3, 3), (3, 6)]),        # an empty range between two that touch
    (b"NNNNNN", [(0, 2), (3, 3), (4, 6)]),        # an empty range among bytes of no range
    (b"ANNNNNNA", [(0, 4), (4, 8)]),              # two touching ranges split an N run
    (b"AN\nNA", [(0, 2), (2, 5)]),                # ... and the second begins with a line break
    (b"ANN\nN|NA", [(0, 2), (6, 8)]),             # bytes of no range lie across the edge
]


def group_b():
    """One buffer per edge E: every motif placed so that each of its bytes in turn
    (and the byte after its last) is the byte at E, the copies three workgroup
    spans apart."""
    cases = []
    for E in EDGES:
        places = [(m, rng, k) for m, rng in MOTIFS for k in range(len(m) + 1)]
        data = np.full((len(places) + 2) * 3 * SPAN, ord("N"), np.uint8)
        pairs = []
        for c, (m, rng, k) in enumerate(places):
            at = (c + 1) * 3 * SPAN + E - k
            data[at: at + len(m)] = _u8(m)
            pairs += [(at + s, at + e) for s, e in rng]
        cases.append(("b/edge{}".format(E), data, _se(pairs)))
    return cases


# ------------------------------------------------------------------ c, e
# all 256 values, the ones the rule looks at common
_WEIGHTS = np.ones(256)
for _c, _w in ((b"Nn|", 40), (b"-. \t", 25), (b"\r", 40), (b"\n", 60), (b"ACGT", 30)):
    _WEIGHTS[list(_c)] = _w
_WEIGHTS /= _WEIGHTS.sum()


def _random_bytes(rng, n: int) -> np.ndarray:
    return rng.choice(256, size=n, p=_WEIGHTS).astype(np.uint8)


def _cut_ranges(rng, n: int, n_cuts: int, gaps: bool) -> np.ndarray:
    """Ranges from random sorted cuts of [0, n] (so they start and end mid-line);
    gaps: every range loses up to 3 of its last bytes to no range.  The last
    range ends at n."""
    cuts = np.unique(np.concatenate([[0, n], rng.integers(0, n + 1, size=n_cuts)]))
    s, e = cuts[:-1].copy(), cuts[1:].copy()
    if gaps:
        e[:-1] = np.maximum(s[:-1], e[:-1] - rng.integers(0, 4, size=e.size - 1))
    return _se(np.stack([s, e], axis=1))


BLOCK_COUNTS = (1, 2, 1023, 1024, 1025, 2049)


def group_c():
    """len = nb * 4096 - 4095 and nb * 4096; a block is all '\\n', all kept bytes or
    mixed, drawn per block, so the scanned counts differ.  The range table is, in
    turn, one range over the buffer, touching ranges of 4 KiB - 1, 4 KiB or
    4 KiB + 1 bytes, and random cuts with bytes left out whose last range ends
    exactly at len."""
    cases = []
    lens = [nb * SPAN - d for nb in BLOCK_COUNTS for d in (SPAN - 1, 0)]
    for x, n in enumerate(lens):
        rng = np.random.default_rng(7000 + x)
        nb = (n + SPAN - 1) // SPAN
        data = _random_bytes(rng, nb * SPAN)
        kind = rng.integers(0, 3, size=nb)
        blocks = data.reshape(nb, SPAN)
        blocks[kind == 0] = 10
        full = np.flatnonzero(kind == 1)
        blocks[full] = _u8(b"ACGT")[rng.integers(0, 4, size=(full.size, SPAN))]
        data = data[:n].copy()
        if x % 3 == 0:
            se, tag = _se([(0, n)]), "one"
        elif x % 3 == 1:
            cuts = np.concatenate([[0], np.cumsum(rng.integers(SPAN - 1, SPAN + 2, size=n // SPAN + 2))])
            cuts = np.unique(np.minimum(cuts, n))
            se, tag = _se(np.stack([cuts[:-1], cuts[1:]], axis=1)), "4k"
        else:
            se, tag = _cut_ranges(rng, n, max(2, n // 3000), gaps=True), "cuts"
        assert int(se[-1]) == n
        cases.append(("c/len{}/{}".format(n, tag), data, se))
    return cases


def group_d():
    dropped = b"\n\r\n- \t.\n\r\n\n--..\r"
    return [
        ("d/len0", np.zeros(0, np.uint8), _se([(0, 0), (0, 0)])),
        ("d/all_ranges_empty", _u8(b"NNANN\nN"), _se([(0, 0), (2, 2), (2, 2), (7, 7)])),
        ("d/nothing_kept", _u8(dropped), _se([(0, len(dropped))])),
        ("d/only_n_class", _u8(b"Nn|" * 700), _se([(0, 2100)])),
        ("d/long_look_back", _u8(b"N" + b"\n" * 20000 + b"N"), _se([(0, 20002)])),
    ]


def group_e():
    cases = []
    for seed in range(4):
        rng = np.random.default_rng(9000 + seed)
        data = _random_bytes(rng, 200_000)
        for gaps in (False, True):
            cases.append(("e/seed{}{}".format(seed, "/gaps" if gaps else ""), data,
                          _cut_ranges(rng, data.size, 400, gaps)))
    return cases


_MAKERS = {"a": group_a, "b": group_b, "c": group_c, "d": group_d, "e": group_e}


@functools.lru_cache(maxsize=None)
def group(g: str):
    """The cases of one group, built once per process."""
    cases = _MAKERS[g]()
    for _name, data, se in cases:
        data.setflags(write=False)
        se.setflags(write=False)
    return cases


@functools.lru_cache(maxsize=None)
def expected(g: str):
    """chunks.compact_records_host of every case of the group, computed once."""
    from kf2vecfsw_amd import chunks as CH
    return [CH.compact_records_host(data, se) for _name, data, se in group(g)]
