"""Pure-Python statements of the FASTQ regularity predicate (include/kf2vec_gpu.h,
kf_index_fastq) and of the pairs the device index writes for one genome, shared
by the CPU model check and the GPU parity tests."""
from __future__ import annotations

import numpy as np


def split_lines(blob: bytes) -> list[tuple[int, int]]:
    """[start, end) of every line up to the last non-empty one (lines end at
    '\\n' only; a '\\r' belongs to its line)."""
    out, i = [], 0
    for part in blob.split(b"\n"):
        out.append((i, i + len(part)))
        i += len(part) + 1
    while out and out[-1][0] == out[-1][1]:
        out.pop()
    return out


def is_regular(blob: bytes) -> bool:
    """The four-line form: '@' line, sequence line, '+' line, quality line at
    least as long as the sequence (and empty if the sequence is)."""
    lines = split_lines(blob)
    for j, (s, e) in enumerate(lines):
        L = e - s
        if j % 4 == 0 and not (L > 0 and blob[s] == ord("@")):
            return False
        if j % 4 == 1 and L > 0 and blob[s] == ord("+"):
            return False
        if j % 4 == 2 and not (L > 0 and blob[s] == ord("+")):
            return False
        if j % 4 == 3:
            ls = lines[j - 2][1] - lines[j - 2][0]
            if L != 0 if ls == 0 else L < ls:
                return False
    return True


def rule_mask(blob: bytes) -> np.ndarray:
    """Excluded bytes by the line rule: the bytes of every line with j % 4 != 1."""
    m = np.zeros(len(blob), dtype=bool)
    for j, (s, e) in enumerate(split_lines(blob)):
        if j % 4 != 1:
            m[s:e] = True
    return m


def device_pairs(blob: bytes, base: int = 0) -> list[int]:
    """The pairs kf_index_fastq writes for a genome at `base`, computed as the
    kernels do: from the table of newline positions and the run of newlines
    that ends the genome."""
    d = np.frombuffer(blob, np.uint8)
    nl = np.flatnonzero(d == 10)
    t = 0
    while t < d.size and d[d.size - 1 - t] == 10:
        t += 1
    cend = d.size - t
    if cend == 0:
        return []
    lines = (nl.size - t) + 1

    def start(j):
        return 0 if j == 0 else int(nl[j - 1]) + 1

    def end(j):
        return int(nl[j]) if j + 1 < lines else cend

    out = [0, end(0)]
    for r in range(1, 1 + (lines + 1) // 4):
        plus = 4 * r - 2
        out += [start(plus), end(min(plus + 2, lines - 1))]
    return [x + base for x in out]


def mask_of(pairs, n: int, base: int = 0) -> np.ndarray:
    m = np.zeros(n, dtype=bool)
    p = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    for s, e in p:
        m[int(s) - base: int(e) - base] = True
    return m
