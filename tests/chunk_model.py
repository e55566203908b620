"""A per-byte restatement of kf_chunk_compact's rule (csrc/kf_chunks.hip:
keep_byte, line_break), with one wrong rule at a time switchable, shared by the
CPU model check and the fault-separation test of tests/test_host_chunk_compact.py.

A byte i of a range [a, b) is kept unless
  * it is '\\n';
  * it is a '\\r' followed by '\\n' (inside the range), or the last byte of the range;
  * it is a gap letter ("- \\t.");
  * it is N-class (N, n, '|') and the nearest earlier byte of the range that is
    not such a line break is N-class.
Kept N-class bytes are written as 'N'.  The rule is evaluated for every byte of
the buffer at once (numpy), each byte against its own range; nothing here is
shared with chunks.compact_records_host, which states the operation with
regular expressions and no look-back.
"""
from __future__ import annotations

import numpy as np

FAULTS = {
    1: "look-back not stopped at a",
    2: "every '\\r' dropped",
    3: "no '\\r' dropped",
    4: "look-back skips gap letters",
    5: "a '\\r' that is the last byte of the range is kept",
    6: "'|' is not N-class",
    7: "a kept N-class byte is written as it is",
    8: "look-back steps over at most one line break",
    9: "look-back does not treat \"\\r\\n\" as a line break",
}


def _among(d: np.ndarray, letters: bytes) -> np.ndarray:
    m = np.zeros(d.size, dtype=bool)
    for c in letters:
        m |= d == c
    return m


def compact_model(data, se, fault: int | None = None) -> tuple[bytes, np.ndarray]:
    """(out, out_se uint64 [2n]) by the per-byte rule, for the sorted, disjoint
    ranges se = [a0, b0, a1, b1, ...] of `data`; fault: None, or the number of
    the one wrong rule (FAULTS) to apply."""
    if fault is not None and fault not in FAULTS:
        raise ValueError("no such fault: {}".format(fault))
    d = np.frombuffer(bytes(data), np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else \
        np.ascontiguousarray(data, dtype=np.uint8)
    se = np.asarray(se, dtype=np.uint64).reshape(-1).astype(np.int64)
    n = d.size
    starts, ends = se[0::2], se[1::2]
    out_se = np.zeros(se.size, dtype=np.uint64)
    if n == 0 or starts.size == 0:
        return b"", out_se
    i = np.arange(n, dtype=np.int64)
    # the range of every byte: the last one that starts at or before it
    r = np.searchsorted(starts, i, side="right") - 1
    a = np.where(r >= 0, starts[np.maximum(r, 0)], 0)
    b = np.where(r >= 0, ends[np.maximum(r, 0)], 0)
    inside = (r >= 0) & (i < b)

    nl, cr = d == 10, d == 13
    next_nl = np.zeros(n, dtype=bool)
    next_nl[:-1] = nl[1:]
    last = i + 1 == b
    crlf = cr & ~last & next_nl            # d[i + 1] is read only inside the range
    if fault == 2:
        lb = lb_back = nl | cr
    elif fault == 3:
        lb = lb_back = nl
    else:
        lb = nl | crlf | (cr & last if fault != 5 else False)
        # the look-back never meets the range's last byte: only "\r\n" counts there
        lb_back = nl if fault == 9 else nl | (cr & next_nl)
    gap = _among(d, b"- \t.")
    isn = _among(d, b"Nn" if fault == 6 else b"Nn|")

    # prev[i]: the nearest earlier byte that the look-back does not step over (-1: none)
    if fault == 8:
        prev = np.where(np.concatenate([[False], lb_back[:-1]]), i - 2, i - 1)
    else:
        skip = lb_back | gap if fault == 4 else lb_back
        at = np.maximum.accumulate(np.where(skip, -1, i))
        prev = np.concatenate([[-1], at[:-1]])
    has = prev >= (0 if fault == 1 else a)
    pred_n = has & (prev >= 0) & isn[np.maximum(prev, 0)]

    keep = inside & ~lb & ~gap & ~(isn & pred_n)
    written = d if fault == 7 else np.where(isn, np.uint8(ord("N")), d)
    before = np.concatenate([[0], np.cumsum(keep, dtype=np.int64)])   # kept bytes before position p
    out_se[0::2] = before[np.minimum(starts, n)]
    out_se[1::2] = before[np.minimum(ends, n)]
    return written[keep].tobytes(), out_se
