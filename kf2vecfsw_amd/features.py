"""A directory of get_frequencies `.kf` files as the float64 feature matrix the
trainers hold, parsed on the device (kf_parse_kf_floats).

The reference reads such a directory -- this tool's, its own, or a published
backbone library -- with my_read_csv (kf2vec/utils.py:436-437: pandas read_csv,
index_col=0, header=None) under mp.Pool, in train_classifier, train_model_set,
classify, query and the -input_dir_fullgenomes side of both chunk trainers, and
multiplies by features_scaler.  features_from_kf gives the same matrix without
pandas: the text goes to the device as it is and every field becomes the
correctly rounded float64 of its decimal there (csrc/kf_decimal.h).
"""
from __future__ import annotations

import dataclasses
import os
import re
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import _native as N
from . import counter as C

MAX_DIGITS = 19            # significant digits of a field (include/kf2vec_gpu.h)
MAX_EXP = 99999            # the explicit exponent's magnitude saturates here
MAX_FRAC = 1 << 20         # and the count of fraction digits here
MIN_Q, MAX_Q = -342, 308   # the decimal exponents the conversion covers


def parse_kf_floats(data: torch.Tensor, off, nbins: int, cap_rows: int | None = None, scaler: float = 1.0,
                    dtype: torch.dtype = torch.float64, stream: int | None = None):
    """Enqueue kf_parse_kf_floats: the get_frequencies `.kf` text of a batch of
    units (files, or pieces cut at line starts: chunks.kf_line_pieces) parsed
    into feature rows on the device, every value float(field) * scaler in
    float64, stored as `dtype` (float64, or float32: rounded once more).
    parse_kf_floats_host states what it computes.

    data, off, cap_rows: as counter.parse_kf_rows takes them (the default
    cap_rows, (batch_bytes + n) // (2 * nbins + 1), is what no batch can exceed).
    Returns (values [cap_rows, nbins] of dtype, row_name int32 [cap_rows, 2]:
    every row's name as (byte offset in the batch, length), unit_row0 int64 [n +
    1], status int64 [4]) on the device: unit u's rows are values[unit_row0[u]:
    unit_row0[u + 1]]; counter.parsed_to_host brings unit_row0 to the host and
    raises what status says.  row_name holds UNSIGNED 32-bit values in int32
    storage (a batch may be 4 GiB - 1 bytes, so an offset may be 2^31 or more
    and then reads as a negative int32): name_spans_to_host widens them.
    Outputs and scratch are allocated here."""
    assert data.dtype == torch.uint8 and data.dim() == 1 and data.is_contiguous()
    assert dtype in (torch.float64, torch.float32)
    dev = data.device
    if isinstance(off, torch.Tensor) and off.is_cuda:
        assert off.dtype == torch.int64 and off.is_contiguous() and off.device == dev
        d_off = off
        nbytes = int(off[-1].item()) if off.numel() else 0
    else:
        o = np.asarray(off.cpu() if isinstance(off, torch.Tensor) else off)
        o = np.ascontiguousarray(o.view(np.int64) if o.dtype == np.uint64 else o.astype(np.int64))
        nbytes = int(o[-1]) if o.size else 0
        d_off = torch.from_numpy(o).to(dev)
    n = max(d_off.numel() - 1, 0)
    assert nbytes <= data.numel()
    nbins = int(nbins)
    if cap_rows is None:
        cap_rows = (nbytes + n) // (2 * nbins + 1)
    cap_rows = int(cap_rows)
    vals = torch.empty((cap_rows, nbins), dtype=dtype, device=dev)
    row_name = torch.empty((cap_rows, 2), dtype=torch.int32, device=dev)
    unit_row0 = torch.empty(n + 1, dtype=torch.int64, device=dev)
    status = torch.empty(4, dtype=torch.int64, device=dev)
    need = int(N.lib().kf_parse_kf_floats_scratch_bytes(nbytes, n, cap_rows))
    scratch = torch.empty(need // 8 + 1, dtype=torch.int64, device=dev)
    one = torch.empty(2, dtype=torch.int64, device=dev)   # an address for the outputs of a call that allows for no row
    s = C._stream_ptr(dev) if stream is None else stream
    with torch.cuda.device(dev):
        N.check(N.lib().kf_parse_kf_floats(
            data.data_ptr(), d_off.data_ptr(), n, nbytes, nbins, cap_rows, float(scaler),
            vals.data_ptr() if vals.numel() else one.data_ptr(), vals.element_size(),
            row_name.data_ptr() if row_name.numel() else one.data_ptr(), unit_row0.data_ptr(), status.data_ptr(),
            scratch.data_ptr(), 8 * scratch.numel(), s), "kf_parse_kf_floats")
    return vals, row_name, unit_row0, status


def name_spans_to_host(row_name: torch.Tensor, n_rows: int) -> np.ndarray:
    """The first n_rows entries of parse_kf_floats' row_name on the host as int64
    [n_rows, 2] (offset, length): the kernel's uint32 values, whatever their top
    bit (one small copy)."""
    spans = row_name[:int(n_rows)].cpu().numpy()
    return np.ascontiguousarray(spans).view(np.uint32).astype(np.int64)


def names_from_spans(text: np.ndarray, spans: np.ndarray) -> list:
    """The names that the spans (name_spans_to_host) cut out of the batch's text (uint8), as str."""
    return [text[a: a + n].tobytes().decode(errors="surrogateescape") for a, n in spans.tolist()]


# ---------------------------------------------------------------------------
# the host statement
# ---------------------------------------------------------------------------
def _float_field(f: bytes):
    """One field read left to right as the kernel reads it: (code, value), code 0
    and float(f), or the first error (3 malformed, 6 more than 19 significant
    digits, 7 outside the normal float64 range) and None."""
    w = nd = frac = ex = 0
    st, neg = 0, False     # st: 0 nothing yet, 1 integer digits, 2 after '.', 3 after 'e', 4 after its sign,
    for c in f:            # 5 exponent digits, 6 after "n", 7 after "na", 8 after "nan"
        if 48 <= c <= 57:
            d = c - 48
            if st >= 3:
                if st > 5:
                    return 3, None
                st, ex = 5, min(ex * 10 + d, MAX_EXP)
                continue
            if st == 0:
                st = 1
            if st == 2:
                frac = min(frac + 1, MAX_FRAC)
            if w == 0 and d == 0:
                continue
            if nd == MAX_DIGITS:
                return 6, None
            w, nd = w * 10 + d, nd + 1
        elif c == 46 and st == 1:
            st = 2
        elif c in (69, 101) and st in (1, 2):
            st = 3
        elif c in (43, 45) and st == 3:
            st, neg = 4, c == 45
        elif c == 110 and st in (0, 7):
            st = 6 if st == 0 else 8
        elif c == 97 and st == 6:
            st = 7
        else:
            return 3, None
    if st == 8:
        return 0, float("nan")
    if st not in (1, 2, 5):
        return 3, None
    if w == 0:
        return 0, 0.0
    q = (-ex if neg else ex) - frac
    if q < MIN_Q or q > MAX_Q or (q < 0 and (w << 1022) < 10 ** -q):   # below 2^-1022, exactly
        return 7, None
    v = float("{}e{}".format(w, q))
    return (7, None) if v == float("inf") else (0, v)


_FIELD = rb"(?:[0-9]+(?:\.[0-9]*)?(?:[eE][+-]?[0-9]+)?|nan)"
_WELL = re.compile(rb"[^,]*(?:," + _FIELD + rb")*")
_LONG = re.compile(rb"[0-9.]{20}")        # no field without such a run has 20 digits in a row
_ZEROS = frozenset([b"0", b"0.0", b"0.", b"0.00"])


def parse_kf_floats_host(data: bytes, nbins: int, cap_rows: int | None = None):
    """The host statement of kf_parse_kf_floats for ONE unit of `.kf` text
    (include/kf2vec_gpu.h has the contract): (values float64 [n, nbins], names
    [n] bytes, (code, row, column)).  Lines, rows, the name and the field count
    are kf_parse_kf_rows' (chunks.parse_kf_rows_host); a field is digits [ '.'
    digits* ] [ e|E [+|-] digits ] or "nan", of at most 19 significant digits
    (leading zeros apart, trailing ones counted), and its value is Python's
    float(field), the correctly rounded binary64.  (0, 0, 0) and every row if the
    text is fine; else the code of the error at the lowest byte offset -- 1 too
    few fields, 2 too many, 3 malformed field, 5 a row numbered cap_rows exists,
    6 more than 19 significant digits, 7 a magnitude outside the normal float64
    range -- with its row and column, and the rows before that row.  The tests
    compare the kernel with it; no product path calls it."""
    nbins = int(nbins)
    rows, names = [], []

    def result(status):
        return (np.stack(rows) if rows else np.zeros((0, nbins), np.float64)), names, status

    tiny = float.fromhex("0x1p-1021")
    for line in bytes(data).split(b"\n"):
        if not line:
            continue
        r = len(rows)
        if cap_rows is not None and r >= cap_rows:
            return result((5, r, 0))
        fields = line.split(b",")
        name, fields = fields[0], fields[1:]
        if _WELL.fullmatch(line) and len(fields) == nbins and not _LONG.search(line):   # the usual row, without a loop
            v = np.asarray(fields, dtype="S").astype(np.float64)     # numpy's bytes to float64 is correctly rounded
            a = np.abs(v)
            odd = np.flatnonzero(~np.isnan(v) & ((a < tiny) | np.isinf(v)))
            if all(fields[i] in _ZEROS for i in odd):
                rows.append(v)
                names.append(name)
                continue
        vals = []
        for j, f in enumerate(fields):
            if j >= nbins:
                return result((2, r, nbins))
            e, x = _float_field(f)
            if e:
                return result((e, r, j))
            vals.append(x)
        if len(fields) < nbins:
            return result((1, r, len(fields)))
        rows.append(np.asarray(vals, dtype=np.float64))
        names.append(name)
    return result((0, 0, 0))


# ---------------------------------------------------------------------------
# a get_frequencies .kf directory as a FeatureStore
# ---------------------------------------------------------------------------
@dataclasses.dataclass
class FeatureStore:
    """The rows of a directory of get_frequencies `.kf` files on the device."""
    values: torch.Tensor        # [G, nbins] float64 or float32 on the device, already times the scaler
    names: list                 # [G] the index column: every row's name as the file holds it
    files: list                 # the samples read, in order (`<sample>.kf`)
    file_row0: np.ndarray       # int64 [len(files) + 1]: file i's rows are values[file_row0[i]: file_row0[i + 1]]
    k: int


def features_from_kf(kf_dir: str, k: int, device="cuda", samples=None, scaler: float = 1.0,
                     dtype: torch.dtype = torch.float64, batch_gb: float = 1.0, p=None) -> FeatureStore:
    """The feature matrix of a directory of get_frequencies `.kf` files (this
    tool's or the reference's), as the trainers hold it after my_read_csv under
    mp.Pool and `* features_scaler` (kf2vec/utils.py:436-437,
    train_classifier_model.py:144-148, train_model_set.py:285-291), with the text
    parsed on the device (kf_parse_kf_floats).

    samples=None: every `*.kf` of kf_dir, sorted by name; else `<sample>.kf` for
    each name in the order given (a missing file is a ValueError before anything
    is read).  A file may hold several rows (a concatenated library) or none;
    rows come in file order, then line order.  Files of any size: one above
    chunks.KF_PIECE_BYTES goes through in kf_line_pieces.  The units (files and
    pieces) are read in batches of about batch_gb GiB (a larger unit alone, below
    4 GiB) by pack_ranges on a reader thread, one batch ahead of the device, into
    two pinned buffers in turn; each batch is copied to the device and parsed
    there.  Two small copies per batch come back: the units' row counts with any
    refusal (a ValueError naming file, row and column), then the name spans of
    the rows there are; the names are taken from the pinned text.  The batches'
    rows are joined by one torch.cat at the end.

    The values equal counter.features(counts, pseudocount, raw_cnt, scaler) for
    the counts the files were written from, bit for bit: both are the correctly
    rounded float64 (repr round-trips it), times the scaler.  pandas' default
    parser, which my_read_csv uses, is not correctly rounded: about half the
    entries of a k=7 row read differently, by at most ~1e-12 relative;
    `pd.read_csv(..., float_precision="round_trip")` is the pandas setting that
    agrees with this function bit for bit.  An empty genome's normalised row is
    "nan" in every column and comes out as NaN."""
    from . import chunks as CH
    from . import main as M
    if k not in M.supported_k:
        raise ValueError("k={} has no vocabulary: supported k are {}..{}".format(
            k, M.supported_k.start, M.supported_k.stop - 1))
    if samples is None:
        samples = sorted(f[:-3] for f in os.listdir(kf_dir) if f.endswith(".kf"))
    samples = list(samples)
    paths = [os.path.join(kf_dir, s + ".kf") for s in samples]
    missing = [q for q in paths if not os.path.isfile(q)]
    if missing:
        raise ValueError("features_from_kf: no such file(s): {}".format(", ".join(missing[:5])))
    device = torch.device(device)
    nbins = C.num_bins(k)
    budget = max(1, int(float(batch_gb or 1.0) * (1 << 30)))
    threads = M.host_threads(p if p is not None else os.cpu_count() or 1)
    units = [(fi, a, e) for fi, q in enumerate(paths) for a, e in CH.kf_line_pieces(q, min(CH.KF_PIECE_BYTES, budget))]
    sizes = [e - a for _, a, e in units]
    if sizes and max(sizes) >= (1 << 32) - 16:
        raise ValueError("features_from_kf: {}: a single line of 4 GiB or more".format(
            paths[units[int(np.argmax(sizes))][0]]))
    batches = M._size_batches(sizes, budget)
    padded = [sum((sizes[i] + 15) // 16 * 16 for i in b) for b in batches]
    pin = device.type == "cuda"
    bufs = [torch.empty(max(padded + [16]), dtype=torch.uint8, pin_memory=pin) for _ in range(min(2, len(batches)))]

    def read(bi):
        return C.pack_ranges([(paths[units[i][0]], units[i][1], units[i][2]) for i in batches[bi]], pin=pin,
                             threads=threads, buf=bufs[bi % 2])

    file_rows = [0] * len(paths)
    parts, names = [], []
    with ThreadPoolExecutor(max_workers=1) as reader:
        nxt = reader.submit(read, 0) if batches else None
        for bi, b in enumerate(batches):
            hb = nxt.result()
            # the other buffer's last copy (batch bi - 1) ended before that batch's row counts came back, and its
            # names were taken before this turn of the loop
            nxt = reader.submit(read, bi + 1) if bi + 1 < len(batches) else None
            nbytes = int(hb.off[-1])
            d_bytes = hb.data[:max(nbytes, 16)].to(device, non_blocking=True)
            vals, row_name, unit_row0, status = parse_kf_floats(d_bytes, hb.off, nbins, scaler=scaler, dtype=dtype)
            who = [paths[units[i][0]] for i in b]
            first_of = {}                         # a file's first unit in this batch
            for x, i in enumerate(b):
                first_of.setdefault(units[i][0], x)
            first = [first_of[units[i][0]] for i in b]
            row0 = C.parsed_to_host(unit_row0, status, who, [file_rows[units[i][0]] for i in b], first,
                                    what="kf_parse_kf_floats")
            for x, i in enumerate(b):
                file_rows[units[i][0]] += int(row0[x + 1] - row0[x])
            n_rows = int(row0[-1])
            text = hb.data.numpy()
            names += names_from_spans(text, name_spans_to_host(row_name, n_rows))
            parts.append(vals[:n_rows].clone())   # the batch's rows without the slack of its cap
            del vals, d_bytes, hb, text
    values = torch.cat(parts) if parts else torch.zeros((0, nbins), dtype=dtype, device=device)
    del parts
    return FeatureStore(values.contiguous(), names, samples, np.cumsum([0] + file_rows).astype(np.int64), k)
