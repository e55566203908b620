"""Tab-separated tables of decimal floats -- the true distance matrix of a clade
and the backbone embeddings -- as tensors on the device, parsed there
(kf_parse_tsv_floats).

The reference's distance trainers read `<tree>_subtree_<c>.di_mtrx` (written by
get_distances, kf2vec/main.py:469-471, 500-502) with pd.read_csv(path, sep='\\t',
header=0, index_col=0) and reindex it into the feature matrix's order with
utils.sort_df (kf2vec/utils.py:141-192; train_model_set.py, train_model_set_chunks.py:236);
query reads `embeddings_subtree_<c>.csv` with pd.read_csv(sep='\\t', header=None,
index_col=0) and `.float()` (kf2vec/query.py:129-134).  true_distances and
backbone_embeddings give the same tables without pandas: the text goes to the
device as it is, every field becomes the correctly rounded float64 of its
decimal there (csrc/kf_decimal.h), and the kernel places the columns -- and one
index_copy_ per batch the rows -- in the order the consumer asks for.
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
from . import features as F


def parse_tsv_floats(data: torch.Tensor, off, ncols: int, col_map=None, out_cols: int | None = None,
                     cap_rows: int | None = None, dtype: torch.dtype = torch.float64, stream: int | None = None,
                     fill: float | None = None):
    """Enqueue kf_parse_tsv_floats: the rows of a tab-separated table of decimal
    floats (a name, then ncols fields, '\\t' between them) in a batch of units
    (pieces of a file cut at line starts: chunks.kf_line_pieces) parsed on the
    device into rows of out_cols values, field j of a row stored at column
    col_map[j] as `dtype` (float64, or float32: rounded once more).
    parse_tsv_floats_host states what it computes.

    data, off: as counter.parse_kf_rows takes them.  col_map: None (the identity,
    out_cols == ncols), or ncols integers (host array, or an int32 tensor on the
    device); an entry outside [0, out_cols) skips that column of the file.
    cap_rows: rows allowed for, by default (batch_bytes + n) // (2 * ncols + 1),
    which no batch can exceed.  fill: the value of the entries that no field maps
    to (None: they are not initialised).
    Returns (values [cap_rows, out_cols], row_name int32 [cap_rows, 2], unit_row0
    int64 [n + 1], status int64 [4]) on the device, as features.parse_kf_floats
    does: counter.parsed_to_host(..., what="kf_parse_tsv_floats") raises what
    status says, features.name_spans_to_host widens the name spans."""
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
    ncols = int(ncols)
    d_map = None
    if col_map is not None:
        if isinstance(col_map, torch.Tensor) and col_map.is_cuda:
            assert col_map.dtype == torch.int32 and col_map.is_contiguous() and col_map.device == dev
            d_map = col_map
        else:
            m = np.asarray(col_map.cpu() if isinstance(col_map, torch.Tensor) else col_map, dtype=np.int64)
            d_map = torch.from_numpy(np.clip(m, -1, (1 << 31) - 1).astype(np.int32)).to(dev)
        assert d_map.numel() == ncols
    out_cols = ncols if out_cols is None else int(out_cols)
    if cap_rows is None:
        cap_rows = (nbytes + n) // (2 * ncols + 1)
    cap_rows = int(cap_rows)
    if fill is None:
        vals = torch.empty((cap_rows, out_cols), dtype=dtype, device=dev)
    else:
        vals = torch.full((cap_rows, out_cols), fill, dtype=dtype, device=dev)
    row_name = torch.empty((cap_rows, 2), dtype=torch.int32, device=dev)
    unit_row0 = torch.empty(n + 1, dtype=torch.int64, device=dev)
    status = torch.empty(4, dtype=torch.int64, device=dev)
    need = int(N.lib().kf_parse_tsv_floats_scratch_bytes(nbytes, n, cap_rows))
    scratch = torch.empty(need // 8 + 1, dtype=torch.int64, device=dev)
    one = torch.empty(2, dtype=torch.int64, device=dev)   # an address for the outputs of a call that allows for no row
    s = C._stream_ptr(dev) if stream is None else stream
    with torch.cuda.device(dev):
        N.check(N.lib().kf_parse_tsv_floats(
            data.data_ptr(), d_off.data_ptr(), n, nbytes, ncols, d_map.data_ptr() if d_map is not None else None,
            out_cols, cap_rows, vals.data_ptr() if vals.numel() else one.data_ptr(), vals.element_size(),
            row_name.data_ptr() if row_name.numel() else one.data_ptr(), unit_row0.data_ptr(), status.data_ptr(),
            scratch.data_ptr(), 8 * scratch.numel(), s), "kf_parse_tsv_floats")
    return vals, row_name, unit_row0, status


# ---------------------------------------------------------------------------
# the host statement
# ---------------------------------------------------------------------------
def _tsv_field(f: bytes, convert: bool = True):
    """One field read left to right as the kernel reads it: (code, value).  A '-'
    as the first byte is the sign; what follows is features._float_field's field,
    but "nan" (a signed nan is malformed at its 'n').  convert=False (a skipped
    column): form and digit count alone, so never code 7."""
    neg = f[:1] == b"-"
    body = f[1:] if neg else f
    if neg and body[:1] == b"n":
        return 3, None
    e, x = F._float_field(body)
    if e == 7 and not convert:
        return 0, None
    if e:
        return e, None
    return 0, (-x if neg else x)


_NUM = rb"(?:-?[0-9]+(?:\.[0-9]*)?(?:[eE][+-]?[0-9]+)?|nan)"
_WELL = re.compile(rb"[^\t]*(?:\t" + _NUM + rb")*")
_ZEROS = re.compile(rb"-?0+(?:\.0*)?")


def parse_tsv_floats_host(data: bytes, ncols: int, col_map=None, out_cols: int | None = None,
                          cap_rows: int | None = None):
    """The host statement of kf_parse_tsv_floats for ONE unit of text
    (include/kf2vec_gpu.h has the contract): (values float64 [n, out_cols], names
    [n] bytes, (code, row, column)).  A line that is not empty is a row: a name
    (the bytes up to the first '\\t'), then exactly ncols fields, each [ '-' ]
    digits [ '.' digits* ] [ e|E [+|-] digits ] or "nan", of at most 19
    significant digits; a field's value is Python's float(field).  Field j goes to
    values[row, col_map[j]] (None: j); an entry outside [0, out_cols) skips the
    column, whose fields are checked for form and digit count but not for range.
    Entries that no field maps to are NaN here (the kernel leaves them as they
    were).  (0, 0, 0) and every row if the text is fine; else the code of the
    error at the lowest byte offset -- 1 too few fields, 2 too many, 3 malformed
    field, 5 a row numbered cap_rows exists, 6 more than 19 significant digits, 7
    a magnitude outside the normal float64 range -- with its row and the file's
    column, and the rows before that row.  The tests compare the kernel with it;
    no product path calls it."""
    ncols = int(ncols)
    out_cols = ncols if out_cols is None else int(out_cols)
    cmap = np.arange(ncols, dtype=np.int64) if col_map is None else np.asarray(col_map, dtype=np.int64)
    assert cmap.shape == (ncols,) and (col_map is not None or out_cols == ncols)
    placed = (cmap >= 0) & (cmap < out_cols)
    src, dst = np.flatnonzero(placed), cmap[placed]
    rows, names = [], []

    def result(status):
        return (np.stack(rows) if rows else np.zeros((0, out_cols), np.float64)), names, status

    def place(v):
        row = np.full(out_cols, np.nan)
        row[dst] = v[src]
        return row

    tiny = float.fromhex("0x1p-1021")
    for line in bytes(data).split(b"\n"):
        if not line:
            continue
        r = len(rows)
        if cap_rows is not None and r >= cap_rows:
            return result((5, r, 0))
        fields = line.split(b"\t")
        name, fields = fields[0], fields[1:]
        if _WELL.fullmatch(line) and len(fields) == ncols and not F._LONG.search(line):   # the usual row, without a loop
            v = np.asarray(fields, dtype="S").astype(np.float64)     # numpy's bytes to float64 is correctly rounded
            a = np.abs(v)
            odd = np.flatnonzero(~np.isnan(v) & ((a < tiny) | np.isinf(v)))
            if all(_ZEROS.fullmatch(fields[i]) for i in odd):
                rows.append(place(v))
                names.append(name)
                continue
        vals = []
        for j, f in enumerate(fields):
            if j >= ncols:
                return result((2, r, ncols))
            e, x = _tsv_field(f, bool(placed[j]))
            if e:
                return result((e, r, j))
            vals.append(np.nan if x is None else x)
        if len(fields) < ncols:
            return result((1, r, len(fields)))
        rows.append(place(np.asarray(vals, dtype=np.float64)))
        names.append(name)
    return result((0, 0, 0))


# ---------------------------------------------------------------------------
# names, header and the two orders (shared by the device path and its host statement)
# ---------------------------------------------------------------------------
def _text(b) -> str:
    return b if isinstance(b, str) else bytes(b).decode(errors="surrogateescape")


def _index_of(names, what: str) -> dict:
    """{name: position}; a name that comes twice is a ValueError (pandas would raise on reindexing, or mangle)."""
    index = {}
    for i, nm in enumerate(names):
        if index.setdefault(nm, i) != i:
            raise ValueError("{}: the name {!r} comes twice".format(what, nm))
    return index


def _split_header(line: bytes, path: str) -> list:
    """The column names of a header line: its cells but the first, which is the index column's."""
    cols = [_text(c) for c in line.split(b"\t")[1:]]
    _index_of(cols, "{}: header".format(path))
    return cols


def _column_map(file_cols, ncols: int, cols, path: str):
    """(col_map int32 [ncols] or None, out_cols, the output's column names) for cols= of table_from_tsv."""
    if cols is None:
        return None, ncols, (list(file_cols) if file_cols is not None else None)
    cols = [_text(c) for c in cols]
    want = _index_of(cols, "{}: cols".format(path))
    return np.asarray([want.get(c, -1) for c in file_cols], dtype=np.int32), len(cols), cols


def _first_line(path: str):
    """(the first non-empty line without its '\\n', the offset behind its '\\n'), or (None, the size)."""
    size = os.path.getsize(path)
    with open(path, "rb") as f:
        buf, base = b"", 0                    # buf = the file from base on, as far as it was read
        while True:
            blk = f.read(1 << 20)
            buf += blk
            k = len(buf) - len(buf.lstrip(b"\n"))
            buf, base = buf[k:], base + k
            i = buf.find(b"\n")
            if i >= 0:
                return buf[:i], base + i + 1
            if not blk:
                return (buf, size) if buf else (None, size)


@dataclasses.dataclass
class FloatTable:
    """A table of floats with named rows (and columns, if the file has a header) on the device."""
    values: torch.Tensor        # [R, C] float64 or float32 on the device
    row_names: list             # [R] text
    col_names: list | None      # [C] text, or None for a table without a header

    def pairs(self, labels, repeat: int = 1) -> torch.Tensor:
        """values[labels][:, labels] on the device: utils.pairwise_true_dist
        (kf2vec/utils.py:250-256) for a batch's labels, without the host's copy per
        step; repeat=2 repeats every row and column in place, as
        pairwise_true_dist_2rows' np.repeat on both axes does (utils.py:259-268)."""
        idx = torch.as_tensor(labels, dtype=torch.long, device=self.values.device).reshape(-1)
        if repeat != 1:
            idx = idx.repeat_interleave(int(repeat))
        return self.values.index_select(0, idx).index_select(1, idx)


def table_host(data: bytes, header: bool, rows=None, cols=None, path: str = "<text>"):
    """The host statement of table_from_tsv on the file's bytes: (values float64
    [R, C] numpy, row_names, col_names), by parse_tsv_floats_host and the same
    header, column map and row order.  Malformed text is a ValueError.  The tests
    compare it with pandas; no product path calls it."""
    data = bytes(data)
    body = data.lstrip(b"\n")
    first, _, rest = body.partition(b"\n")
    if not first:
        raise ValueError("{}: no line".format(path))
    file_cols = _split_header(first, path) if header else None
    ncols = first.count(b"\t")
    if ncols == 0:
        raise ValueError("{}: no column".format(path))
    if cols is not None and not header:
        raise ValueError("{}: cols= needs a header".format(path))
    col_map, out_cols, col_names = _column_map(file_cols, ncols, cols, path)
    vals, names, (code, r, c) = parse_tsv_floats_host(rest if header else body, ncols, col_map, out_cols)
    if code:
        raise ValueError("{}: row {}, column {}: {} (kf_parse_tsv_floats status {})".format(
            path, r, c, C.KF_PARSE_ERRORS[code], code))
    names = [_text(nm) for nm in names]
    if rows is None:
        return vals, names, col_names
    rows = [_text(x) for x in rows]
    want = _index_of(rows, "{}: rows".format(path))
    _index_of(names, "{}: row names".format(path))
    out = np.full((len(rows), out_cols), np.nan)
    for i, nm in enumerate(names):
        if nm in want:
            out[want[nm]] = vals[i]
    return out, rows, col_names


def table_from_tsv(path: str, device="cuda", header: bool = True, rows=None, cols=None,
                   dtype: torch.dtype = torch.float64, batch_gb: float = 1.0, p=None) -> FloatTable:
    """A tab-separated table of decimal floats with a name in the first column,
    as pd.read_csv(path, sep='\\t', index_col=0, header=0 if header else None)
    followed by .reindex(index=rows) and .reindex(columns=cols) gives it, with the
    text parsed on the device (kf_parse_tsv_floats).

    header: the first non-empty line is a header; the host reads it: its first
    cell is ignored, the others name the columns.  Without one the column count
    is the first non-empty line's count of tabs and col_names is None.
    cols= (needs a header): the output's column names in order; they become the
    kernel's column map, so columns of the file that are not asked for are
    skipped in the kernel and never stored, and columns asked for that the file
    lacks are NaN.  rows=: the output's row names in order; the output is
    allocated once, filled with NaN, and each batch's rows go to their places by
    one index_copy_: rows not asked for are dropped, rows asked for that the file
    lacks stay NaN.  Both are DataFrame.reindex semantics.
    A name that comes twice -- in the header, in rows or cols, or, with rows=,
    among the file's row names -- is a ValueError (pandas raises on some of these
    and renames on others).  Malformed text is a ValueError naming the file, the
    row (counted from 0 behind the header) and the column (counted from 0 behind
    the name column).

    Files of any size: the text behind the header goes through in
    chunks.kf_line_pieces, read in batches of about batch_gb GiB (a single line of
    4 GiB or more is refused) by pack_ranges on a reader thread, one batch ahead
    of the device, into two pinned buffers in turn, as features.features_from_kf
    reads its directory.

    Names stay text as the file holds them: pandas would turn a column of
    all-digit names into integers.  The values are the correctly rounded float64
    of every decimal; pandas' default parser is not correctly rounded (2 of the 25
    entries of the toy example's 5 x 5 matrix read differently), and
    float_precision="round_trip" is the pandas setting that agrees bit for bit."""
    from . import chunks as CH
    from . import main as M
    device = torch.device(device)
    first, behind = _first_line(path)
    if first is None:
        raise ValueError("{}: no line".format(path))
    file_cols = _split_header(first, path) if header else None
    ncols = first.count(b"\t")
    if ncols == 0:
        raise ValueError("{}: no column".format(path))
    if cols is not None and not header:
        raise ValueError("{}: cols= needs a header".format(path))
    want = None
    if rows is not None:
        rows = [_text(x) for x in rows]
        want = _index_of(rows, "{}: rows".format(path))
    col_map, out_cols, col_names = _column_map(file_cols, ncols, cols, path)
    budget = max(1, int(float(batch_gb or 1.0) * (1 << 30)))
    threads = M.host_threads(p if p is not None else os.cpu_count() or 1)
    units = CH.kf_line_pieces(path, min(CH.KF_PIECE_BYTES, budget), behind if header else 0)
    sizes = [e - a for a, e in units]
    if sizes and max(sizes) >= (1 << 32) - 16:
        raise ValueError("table_from_tsv: {}: a single line of 4 GiB or more".format(path))
    batches = M._size_batches(sizes, budget)
    padded = [sum((sizes[i] + 15) // 16 * 16 for i in b) for b in batches]
    pin = device.type == "cuda"
    bufs = [torch.empty(max(padded + [16]), dtype=torch.uint8, pin_memory=pin) for _ in range(min(2, len(batches)))]
    d_map = torch.from_numpy(col_map).to(device) if col_map is not None else None
    nan = float("nan")

    def read(bi):
        return C.pack_ranges([(path, units[i][0], units[i][1]) for i in batches[bi]], pin=pin, threads=threads,
                             buf=bufs[bi % 2])

    out = torch.full((len(rows), out_cols), nan, dtype=dtype, device=device) if want is not None else None
    seen = set()
    file_rows = 0
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
            vals, row_name, unit_row0, status = parse_tsv_floats(d_bytes, hb.off, ncols, d_map, out_cols, dtype=dtype,
                                                                 fill=nan if d_map is not None else None)
            row0 = C.parsed_to_host(unit_row0, status, [path] * len(b), [file_rows] * len(b), [0] * len(b),
                                    what="kf_parse_tsv_floats")
            n_rows = int(row0[-1])
            file_rows += n_rows
            got = F.names_from_spans(hb.data.numpy(), F.name_spans_to_host(row_name, n_rows))
            if want is None:
                names += got
                parts.append(vals[:n_rows].clone())   # the batch's rows without the slack of its cap
            else:
                for nm in got:
                    if nm in seen:
                        raise ValueError("{}: row names: the name {!r} comes twice".format(path, nm))
                    seen.add(nm)
                dest = [want.get(nm, -1) for nm in got]
                keep = [i for i, d in enumerate(dest) if d >= 0]
                if keep:
                    src = vals[:n_rows]
                    if len(keep) != n_rows:
                        src = src.index_select(0, torch.tensor(keep, dtype=torch.long, device=device))
                    out.index_copy_(0, torch.tensor([dest[i] for i in keep], dtype=torch.long, device=device), src)
            del vals, d_bytes, hb
    if want is not None:
        return FloatTable(out, rows, col_names)
    values = torch.cat(parts) if parts else torch.zeros((0, out_cols), dtype=dtype, device=device)
    return FloatTable(values.contiguous(), names, col_names)


def true_distances(path: str, order, device="cuda", dtype: torch.dtype = torch.float64) -> FloatTable:
    """The true distance matrix of a clade (`<tree>_subtree_<c>.di_mtrx` or
    `<tree>_full.di_mtrx`) in the order of the feature matrix: what
    utils.read_true_dist_mtrx and utils.sort_df (kf2vec/utils.py:141-192) leave in
    the trainers' pdf_sorted, on the device.  order: the names by row of the
    feature matrix (sort_df's `order`).  The rows are `order`; the columns are
    `order` if the file has more than one column, else the file's one column as
    it is (sort_df reindexes the columns only `if len(ddf.columns) > 1`).  Names
    of `order` that the file lacks are NaN rows and columns, as reindex leaves
    them.  FloatTable.pairs then gives every step's pairwise_true_dist."""
    first, _ = _first_line(path)
    order = list(order)
    many = first is not None and first.count(b"\t") > 1
    return table_from_tsv(path, device, header=True, rows=order, cols=order if many else None, dtype=dtype)


def backbone_embeddings(path: str, device="cuda") -> FloatTable:
    """The backbone embeddings of a clade (`embeddings_subtree_<c>.csv`: a name
    and the embedding's signed floats per line, no header) as query holds them
    after pd.read_csv(sep="\\t", header=None, index_col=0) and
    torch.from_numpy(df.values).float() (kf2vec/query.py:129-134): float32 [G, D]
    on the device, every value the correctly rounded float64 of its decimal
    rounded once more to float32, and the names as text in file order."""
    return table_from_tsv(path, device, header=False, dtype=torch.float32)


# ---------------------------------------------------------------------------
# float tables written out: the text formatted on the device (kf_format_float_rows)
# ---------------------------------------------------------------------------
KF_FLOAT_SHORTEST, KF_FLOAT_WIDENED = N.KF_FLOAT_SHORTEST, N.KF_FLOAT_WIDENED
FLOAT_TEXT_MAX = 24                  # bytes of one float's text at most


def float_row_bound(ncols: int, max_label_len: int, eol_len: int = 2) -> int:
    """Bytes that no line of format_float_rows exceeds: the label and its
    separator, 24 bytes and a separator per column, and the end of line."""
    return int(max_label_len) + 1 + (FLOAT_TEXT_MAX + 1) * int(ncols) + int(eol_len)


def quote_label(label, sep: str = "\t", eol: str = "\r\n") -> bytes:
    """A label as csv.writer(delimiter=sep, lineterminator=eol) writes it as the
    first of several fields (the csv module's own QUOTE_MINIMAL rules: quoted if it
    holds the separator, a quote or a line break); what is not text goes through
    str() as the writer does, None is the empty field."""
    import csv
    import io
    buf = io.StringIO(newline="")
    csv.writer(buf, delimiter=sep, lineterminator=eol).writerow([label, "x"])
    out = buf.getvalue()
    return out[: len(out) - len(sep) - 1 - len(eol)].encode(errors="surrogateescape")


def _float_form(values, mode: int) -> int:
    size = values.element_size() if isinstance(values, torch.Tensor) else values.dtype.itemsize
    if (size, mode) not in ((8, KF_FLOAT_SHORTEST), (4, KF_FLOAT_SHORTEST), (4, KF_FLOAT_WIDENED)):
        raise ValueError("mode {} with {}-byte values: KF_FLOAT_SHORTEST, or KF_FLOAT_WIDENED for float32".format(
            mode, size))
    return size


def _encode_labels(labels, n: int):
    """(the labels as bytes or None, the longest one's length)."""
    if labels is None:
        return None, 0
    enc = [x if isinstance(x, (bytes, bytearray)) else str(x).encode(errors="surrogateescape") for x in labels]
    if len(enc) != n:
        raise ValueError("{} labels for {} rows".format(len(enc), n))
    return enc, max([len(x) for x in enc], default=0)


def format_float_call(values: torch.Tensor, enc, mode: int, sep: str = "\t", eol: str = "\r\n",
                      nan_empty: bool = False, cap_bytes: int | None = None, stream: int | None = None):
    """Enqueue ONE kf_format_float_rows: values [n, ncols] (float32 or float64,
    contiguous, on the device) with row r's label enc[r] (bytes, already quoted;
    enc=None: no label and no leading separator).  cap_bytes: the size of the
    text buffer, by default n times float_row_bound, which must stay below 2^32.
    Returns (text uint8 [cap_bytes], row_off int64 [n + 1], status int64 [4]) on
    the device; nothing waits."""
    assert values.dim() == 2 and values.is_contiguous() and values.dtype in (torch.float32, torch.float64)
    _float_form(values, mode)
    dev = values.device
    n, ncols = int(values.shape[0]), int(values.shape[1])
    sep_b, eol_b = sep.encode(), eol.encode()
    assert len(sep_b) == 1 and len(eol_b) in (1, 2)
    if enc is None:
        pre, rpre = [b""], np.zeros(n, dtype=np.int32)
    else:
        pre, rpre = enc, np.arange(n, dtype=np.int32)
    pre_off = np.zeros(len(pre) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in pre], out=pre_off[1:])
    blob = np.frombuffer(b"".join(pre) + b"\0", dtype=np.uint8)   # never empty: an address for no prefix bytes
    d_pre = torch.from_numpy(blob.copy()).to(dev, non_blocking=True)
    d_pre_off = torch.from_numpy(pre_off).to(dev, non_blocking=True)
    d_rpre = torch.from_numpy(rpre).to(dev, non_blocking=True)
    if cap_bytes is None:
        cap_bytes = n * float_row_bound(ncols, max([len(x) for x in pre], default=0), len(eol_b))
    cap_bytes = int(cap_bytes)
    text = torch.empty(max(cap_bytes, 1), dtype=torch.uint8, device=dev)
    row_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    status = torch.empty(4, dtype=torch.int64, device=dev)
    need = int(N.lib().kf_format_float_scratch_bytes(n, ncols))
    scratch = torch.empty(need // 8 + 1, dtype=torch.int64, device=dev)
    s = C._stream_ptr(dev) if stream is None else stream
    with torch.cuda.device(dev):
        N.check(N.lib().kf_format_float_rows(
            values.data_ptr(), values.element_size(), n, ncols, int(mode), sep_b[0],
            eol_b[0] | (eol_b[1] << 8 if len(eol_b) == 2 else 0), len(eol_b), int(bool(nan_empty)), d_pre.data_ptr(),
            d_pre_off.data_ptr(), len(pre), d_rpre.data_ptr(), text.data_ptr(), cap_bytes, row_off.data_ptr(),
            status.data_ptr(), scratch.data_ptr(), 8 * scratch.numel(), s), "kf_format_float_rows")
    if stream is not None:   # the tables and the scratch are the caller's stream's until the call is done
        for t in (d_pre, d_pre_off, d_rpre, scratch):
            t.record_stream(torch.cuda.ExternalStream(stream, device=dev))
    return text[:cap_bytes], row_off, status


def float_status_check(code: int, need: int, row: int, col: int = 0, cap_bytes: int | None = None) -> None:
    """Raise what kf_format_float_rows' status words say (nothing for code 0)."""
    if code == 1:
        raise N.NativeError("kf_format_float_rows: the text needs {} bytes{} (status 1)".format(
            need, "" if cap_bytes is None else ", {} allowed for".format(cap_bytes)))
    if code == 2:
        raise ValueError("row {}: a row's prefix is out of range, or the prefix offsets decrease "
                         "(kf_format_float_rows status 2)".format(row))
    if code != 0:
        raise ValueError("row {}, column {}: a value that cannot be formatted (kf_format_float_rows status {})".format(
            row, col, code))


def format_float_rows(values: torch.Tensor, labels=None, mode: int = KF_FLOAT_SHORTEST, sep: str = "\t",
                      eol: str = "\r\n", nan_empty: bool = False):
    """The table `values` [n, ncols] (float32 or float64 on the device) as text,
    formatted there: row r is  label_r sep f sep ... f eol  (labels=None: no label
    and no leading separator; labels are written as given: quote_label quotes).
    mode KF_FLOAT_SHORTEST: a float64 as repr(float), a float32 as
    str(np.float32); KF_FLOAT_WIDENED (float32): repr of the value as a double,
    which is what .tolist() and csv.writer write.  nan_empty: NaN is an empty
    field (pandas) instead of "nan" (csv.writer).  format_float_rows_host states
    it on the host.  The rows are cut into calls whose text bound stays below
    4 GiB.  Returns (text uint8 on the device, row_off int64 numpy [n + 1])."""
    values = values.contiguous()
    n, ncols = int(values.shape[0]), int(values.shape[1])
    enc, longest = _encode_labels(labels, n)
    bound = float_row_bound(ncols, longest, len(eol.encode()))
    if bound > C.KF_FORMAT_MAX_CAP:
        raise ValueError("a row of {} columns may need {} bytes of text: 4 GiB or more".format(ncols, bound))
    per = max(1, C.KF_FORMAT_MAX_CAP // bound)
    parts, offs, base = [], [np.zeros(1, dtype=np.int64)], 0
    for r0 in range(0, max(n, 1), per):
        r1 = min(n, r0 + per)
        text, row_off, status = format_float_call(values[r0:r1], None if enc is None else enc[r0:r1], mode, sep, eol,
                                                  nan_empty)
        both = torch.cat([status, row_off]).cpu().numpy()
        float_status_check(int(both[0]), int(both[1]), r0 + int(both[2]), int(both[3]), int(text.numel()))
        off = both[4:]
        parts.append(text[: int(off[-1])])
        offs.append(off[1:] + base)
        base += int(off[-1])
    text = parts[0] if len(parts) == 1 else torch.cat(parts)
    return text, np.concatenate(offs)


def float_text_host(values, mode: int = KF_FLOAT_SHORTEST, nan_empty: bool = False) -> list:
    """Every value's text as Python and numpy print it: repr(float(v)) for a
    float64 and for a float32 in KF_FLOAT_WIDENED mode, str(np.float32(v)) for a
    float32 in KF_FLOAT_SHORTEST mode; NaN "nan" or, with nan_empty, nothing."""
    a = np.ascontiguousarray(values.cpu().numpy() if isinstance(values, torch.Tensor) else values)
    size = _float_form(a, mode)
    flat = a.reshape(-1)
    if size == 4 and mode == KF_FLOAT_SHORTEST:
        out = [str(v) for v in flat]
    else:
        with np.errstate(invalid="ignore"):    # a signalling NaN widens to a quiet one
            out = [repr(v) for v in flat.astype(np.float64).tolist()]
    if nan_empty:
        for i in np.flatnonzero(np.isnan(flat)):
            out[i] = ""
    return out


def format_float_rows_host(values, labels=None, mode: int = KF_FLOAT_SHORTEST, sep: str = "\t", eol: str = "\r\n",
                           nan_empty: bool = False):
    """The host statement of format_float_rows: (the text as bytes, row_off int64
    [n + 1]), built from Python's repr and numpy's str (float_text_host).  The
    tests compare the kernel with it; no product path calls it."""
    a = values.cpu().numpy() if isinstance(values, torch.Tensor) else np.asarray(values)
    n, ncols = a.shape
    enc, _ = _encode_labels(labels, n)
    cells = float_text_host(a, mode, nan_empty)
    sep_b, eol_b = sep.encode(), eol.encode()
    lines, off = [], np.zeros(n + 1, dtype=np.int64)
    for r in range(n):
        body = sep_b.join(x.encode() for x in cells[r * ncols: (r + 1) * ncols])
        line = (enc[r] + sep_b if enc is not None and enc[r] else b"") + body + eol_b
        lines.append(line)
        off[r + 1] = off[r] + len(line)
    return b"".join(lines), off


def header_line(header, sep: str = "\t", eol: str = "\r\n") -> bytes:
    """A header's cells as csv.writer(delimiter=sep, lineterminator=eol) writes the row."""
    import csv
    import io
    buf = io.StringIO(newline="")
    csv.writer(buf, delimiter=sep, lineterminator=eol).writerow(list(header))
    return buf.getvalue().encode(errors="surrogateescape")


class FloatTableWriter:
    """Float tables formatted on the device and written by a thread of its own, so
    a table's copy to the host and its file write overlap the device work that
    the caller enqueues next (query: the next block).  write() enqueues the
    format calls on the current stream and returns; the writer thread waits for
    each call's row offsets, copies the text it names through a pinned buffer on
    a second stream and hands it to kf_write_text_segments.  At most max_pending
    tables are in flight: write() waits for the oldest before it enqueues
    another, so the text held on the device and in pinned memory does not grow
    with the number of blocks when the disk is slower than the device.  close() (or leaving
    the with block) waits for every write and raises what one of them raised."""

    def __init__(self, device, threads: int = 1):
        self.device = torch.device(device)
        self.threads = max(1, int(threads))
        self.d2h = torch.cuda.Stream(self.device)
        self.pool = ThreadPoolExecutor(max_workers=1)
        self.pending = []
        self.max_pending = 2             # tables in flight: each holds its text on the device and a pinned copy
        self.times = {"copy_back": 0.0, "file_write": 0.0}

    def write(self, path: str, labels, values: torch.Tensor, header=None, mode: int = KF_FLOAT_SHORTEST,
              sep: str = "\t", eol: str = "\r\n", nan_empty: bool = False, append: bool = False,
              quoted: bool = False) -> None:
        """quoted: the labels are row prefixes written as given (bytes that
        quote_label has seen already, and may hold further fields: classify's
        label and class), not labels to quote."""
        while len(self.pending) >= self.max_pending:   # a slow disk holds the caller back, not memory
            self.pending.pop(0).result()
        values = values.contiguous()
        n, ncols = int(values.shape[0]), int(values.shape[1])
        enc = None if labels is None else list(labels) if quoted else [quote_label(x, sep, eol) for x in labels]
        enc, longest = _encode_labels(enc, n)
        head = header_line(header, sep, eol) if header is not None else b""
        bound = float_row_bound(ncols, longest, len(eol.encode()))
        if bound > C.KF_FORMAT_MAX_CAP:
            raise ValueError("a row of {} columns may need {} bytes of text: 4 GiB or more".format(ncols, bound))
        per = max(1, C.KF_FORMAT_MAX_CAP // bound)
        stream = torch.cuda.current_stream(self.device)
        calls = []
        for r0 in range(0, n, per):
            r1 = min(n, r0 + per)
            text, row_off, status = format_float_call(values[r0:r1], None if enc is None else enc[r0:r1], mode, sep,
                                                      eol, nan_empty)
            done = torch.cuda.Event()
            done.record(stream)
            self.d2h.wait_event(done)
            small = torch.empty(8, dtype=torch.int64, pin_memory=True)
            with torch.cuda.stream(self.d2h):
                small[:4].copy_(status, non_blocking=True)
                small[4:5].copy_(row_off[-1:], non_blocking=True)
                for t in (text, row_off, status, values):
                    t.record_stream(self.d2h)
                ev = torch.cuda.Event()
                ev.record(self.d2h)
            calls.append((r0, text, small, ev))
        self.pending.append(self.pool.submit(self._finish, path, head, calls, append))

    def _finish(self, path: str, head: bytes, calls, append: bool) -> None:
        import ctypes
        import time
        lib = N.lib()
        first = True
        if not calls:
            calls = [(0, None, None, None)]
        with torch.cuda.device(self.device):
            for r0, text, small, ev in calls:
                t0 = time.perf_counter()
                total = 0
                if text is not None:
                    ev.synchronize()
                    h = small.numpy()
                    float_status_check(int(h[0]), int(h[1]), r0 + int(h[2]), int(h[3]), int(text.numel()))
                    total = int(h[4])
                lead = head if first else b""
                host = torch.empty(max(len(lead) + total, 1), dtype=torch.uint8, pin_memory=True)
                if lead:
                    host.numpy()[: len(lead)] = np.frombuffer(lead, dtype=np.uint8)
                if total:
                    with torch.cuda.stream(self.d2h):
                        host[len(lead): len(lead) + total].copy_(text[:total], non_blocking=True)
                    self.d2h.synchronize()
                t1 = time.perf_counter()
                cp = (ctypes.c_char_p * 1)(os.fsencode(path))
                ap = np.asarray([1 if (append or not first) else 0], dtype=np.uint8)
                so = np.asarray([0, len(lead) + total], dtype=np.uint64)
                N.check(lib.kf_write_text_segments(1, cp, ap.ctypes.data, so.ctypes.data, host.data_ptr(),
                                                   self.threads), "kf_write_text_segments")
                first = False
                self.times["copy_back"] += t1 - t0
                self.times["file_write"] += time.perf_counter() - t1

    def drain(self) -> None:
        while self.pending:
            self.pending.pop(0).result()

    def close(self) -> None:
        try:
            self.drain()
        finally:
            self.pool.shutdown()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


def write_float_table(path: str, labels, values: torch.Tensor, header=None, mode: int = KF_FLOAT_SHORTEST,
                      sep: str = "\t", eol: str = "\r\n", nan_empty: bool = False, append: bool = False,
                      threads: int = 1) -> None:
    """Write the table `values` [n, ncols] (float32 or float64 on the device) to
    `path` as text formatted on the device (format_float_rows): an optional
    header row, then a line per row with its label first (labels=None: none).
    Header cells and labels are quoted on the host by the csv module's own rules
    (quote_label); the text crosses to the host through a pinned buffer and
    kf_write_text_segments writes it.  append: the file's end is where writing
    starts, else the file is truncated.
    The reference's tables: query's two files are mode=KF_FLOAT_WIDENED with the
    defaults ('\\t', '\\r\\n', "nan"); DataFrame.to_csv(sep='\\t') of a float32 frame
    is mode=KF_FLOAT_SHORTEST, eol='\\n', nan_empty=True; a `.di_mtrx` is a float64
    tensor in the same form.
    Reading back: float64 text and KF_FLOAT_WIDENED text return the same bits
    through this project's parsers.  The float32 form of KF_FLOAT_SHORTEST is the
    shortest decimal for a reader that rounds once; the parsers (like strtod and
    a cast, and like numpy) go through the nearest double, and for one float32
    and its negative, 0x15ae43fd printed 7.038531e-26, that lands one unit off
    (profiles/r20/float32_exhaustive.json)."""
    with FloatTableWriter(values.device, threads) as w:
        w.write(path, labels, values, header, mode, sep, eol, nan_empty, append)
