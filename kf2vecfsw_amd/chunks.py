"""``get_chunks`` on the device (reference kf2vec/main.py:654-929).

The reference shells out per genome to
* ``seqtk seq -l 0`` to linearise records (:732);
* ``awk gsub(/[N|n]+/,"N")`` to collapse N runs (:740-742);
* ``seqkit seq -m 10000 -g -v`` to drop gaps and contigs < 10 kbp (:753);
* ``seqkit split`` / ``seqkit sliding`` to make 10 kbp windows (:784, :824, :837);
then runs one ``get_frequencies -raw_cnt`` (a Jellyfish pair) per window
(:869-881) and concatenates the rows (:895-915).

Here the genomes are processed in batches of files:
* the files of a batch are read into one pinned buffer by a thread pool and
  their header lines indexed (``kf_index_records``);
* one H2D copy, then ONE ``kf_chunk_compact`` (csrc/kf_chunks.hip) over every
  record of every genome of the batch: linearisation, N-run collapse and gap
  removal;
* ONE device-to-host copy of the processed record bounds per batch; the host
  plans every genome's windows from them (:813-818, numpy);
* the windows are gathered into a device buffer (``kf_chunk_gather``) and
  counted by ``kf_count_batch`` in launches of at most ``max_windows`` windows
  (the count matrix is 4 x bins bytes per window: 32 KiB at k=7, 8 MiB at k=11);
* the count rows come back as uint16 on a copy stream of their own, and a
  writer thread formats and writes each launch's rows while the device counts
  the next launch (``kf_write_kf_segments16``: rows formatted by host threads,
  one file per genome written in parallel, appended when a genome's windows span
  several launches);
* at the k of ``DEVICE_FORMAT_K`` each launch's uint16 rows are instead formatted
  into `.kf` text on the device
  (``kf_format_kf_rows16``, csrc/kf_kfformat.hip); the used bytes of the text
  come back on a copy stream of their own through two pinned slabs (a copier
  thread), and a writer thread hands each slab's file ranges to
  ``kf_write_text_segments`` (pwrite in parallel, one file per genome, appended
  when a genome's windows span several slabs or launches) while the device
  counts the next launch and the copier brings its text.
  ``kf_write_kf_segments16`` (rows formatted by host threads) is the statement
  the device formatter equals byte for byte (``format_rows_host``).

``chunk_store`` runs the same pipeline without the writer and keeps the uint16
rows on the device; ``ChunkStore.batch`` draws the chunk trainer's row runs and
builds its batches there (``kf_chunk_features``, csrc/kf_chunkfeat.hip).
"""
from __future__ import annotations

import ctypes
import math
import os
import queue
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass, field

import numpy as np
import torch

from . import _native as N

CHUNK_SZ = 10000       # main.py:100
CHUNK_CNT_THR = 5      # main.py:101
assert CHUNK_SZ < 1 << 16   # window counts fit uint16 (count_and_write)
LAUNCH_WINDOWS = 4096  # windows per count launch at most (128 MiB of k=7 counts)
# bytes of `.kf` text per pinned slab (count_and_write copies through two): a k=7 launch's text (134 MB) in
# one, so that the native writer has all the launch's files to write side by side
TEXT_SLAB = 144 << 20
TEXT_SMALL = 4 << 20    # a piece of text up to this size travels in a pinned buffer of its own, not in a slab
# k at which count_and_write formats on the device: where get_chunks measured no slower than with the host
# formatter (profiles/r17: k=3 equal; k=7 0.79x and k=10 0.63x of the host writer's windows/s, whose 16
# threads format while they wait for the files anyway; other k were not measured)
DEVICE_FORMAT_K: frozenset = frozenset({3})

# KF_TRACE=1: stage timeline (host ms since the first event) for tools/chunks_bench.py
TRACE = os.environ.get("KF_TRACE") == "1"
trace: list = []


def _tr(stage: str, t0: float, **kw) -> None:
    if TRACE:
        import time
        trace.append((stage, round(t0 * 1e3, 3), round(time.perf_counter() * 1e3, 3), kw))


def window_plan(total_length: int) -> tuple[int, int]:
    """(number of windows, step) for a contig of this length (main.py:813-818;
    seqkit sliding keeps only whole windows)."""
    total_chunks = math.ceil(total_length / CHUNK_SZ)
    ovrlap = int(math.ceil((total_chunks * CHUNK_SZ - total_length) / (total_chunks - 1))) \
        if total_chunks != 1 else 0
    step = CHUNK_SZ - ovrlap
    n = 0 if total_length < CHUNK_SZ else (total_length - CHUNK_SZ) // step + 1
    return n, step


def window_name(sample: str, cid: str, s: int) -> str:
    """Row name of the window starting at s (main.py:905-915: `<sample>.part_<cid>.part_<seqkit id>`,
    ':' of seqkit's "_sliding:a-b" replaced by "__")."""
    return "{}.part_{}.part_{}_sliding__{}-{}".format(sample, cid, cid, s + 1, s + CHUNK_SZ)


def _contig_id(hdr: bytes) -> str:
    """seqtk/seqkit id: the first word of the header line ('>' and a trailing '\\r' dropped)."""
    if hdr.endswith(b"\r"):
        hdr = hdr[:-1]
    w = hdr.split()
    return w[0].decode(errors="surrogateescape") if w else ""


def records_from_index(data: np.ndarray, iv: np.ndarray, lo: int, hi: int) -> tuple[list[int], list[str]]:
    """Records of the FASTA bytes data[lo:hi] whose header lines are indexed by iv
    (kf_index_records pairs, absolute positions): [start, end) of each record's
    sequence region (the bytes after its header line, up to the next header) as
    a flat [s0, e0, s1, e1, ...] list, and the contig ids.  kf_index_records
    merges header lines that follow each other (an empty record, ">a\n>b\n..."),
    so every interval is split at its newlines: each line is one header."""
    heads: list[int] = []      # header line starts
    starts: list[int] = []     # sequence region starts
    ids: list[str] = []
    for r in range(iv.size // 2):
        hs, he = int(iv[2 * r]), int(iv[2 * r + 1])
        pos = hs
        for line in data[hs: he].tobytes().split(b"\n"):
            heads.append(pos)
            starts.append(min(pos + len(line) + 1, hi))
            ids.append(_contig_id(line[1:]))
            pos += len(line) + 1
    ends = heads[1:] + [hi]
    out = [0] * (2 * len(ids))
    out[0::2] = starts
    out[1::2] = ends
    return out, ids


def record_regions(data: np.ndarray) -> tuple[np.ndarray, list[str]]:
    """Sequence regions [start, end) of the FASTA records of one genome (the bytes
    after each header line, up to the next header) and the contig ids (first word
    of the header, seqtk/seqkit id; a trailing '\\r' of the header line is
    dropped).  Bytes before the first header belong to no record (seqtk skips them)."""
    from .counter import index_records
    data = np.ascontiguousarray(data, dtype=np.uint8)
    iv, _ = index_records(data, N.KF_FMT_FASTA, 0)
    se, ids = records_from_index(data, iv, 0, data.size)
    return np.asarray(se, dtype=np.uint64), ids


@dataclass
class Genome:
    """One input file of a batch and its fate (the log lines of main.py:761-885).
    Window w starts at starts[w] in the batch's processed sequence and at wpos[w]
    in its contig, whose name prefix is prefixes[wpre[w]]."""
    fname: str
    sample: str
    rec_lo: int = 0                  # its records in the batch's record table
    rec_hi: int = 0
    prefixes: list = field(default_factory=list)   # "<sample>.part_<cid>.part_<cid>_sliding__" per contig
    wpre: np.ndarray | None = None
    wpos: np.ndarray | None = None
    starts: np.ndarray | None = None
    excluded: str | None = None       # "none" (no contig >= 10 kbp) or "few"
    write: bool = True                # False: a later file has the same sample name
    # a file counted in record-aligned parts (main.record_pieces): its parts'
    # rows go to out_name, appended after the first part (cont); only the last
    # part is reported, with the file's windows (total_windows)
    out_name: str | None = None
    cont: bool = False
    last: bool = True
    total_windows: int | None = None

    @property
    def n_windows(self) -> int:
        return 0 if self.starts is None else int(self.starts.size)

    @property
    def names(self) -> list[str]:
        """Row names (main.py:905-915), built here only for tests: the writer builds them."""
        if self.starts is None:
            return []
        return [self.prefixes[int(p)] + "{}-{}".format(int(s) + 1, int(s) + CHUNK_SZ)
                for p, s in zip(self.wpre, self.wpos)]


def shadow(genomes: list[Genome]) -> None:
    """The reference writes genome by genome, so a later file with the same
    sample name replaces an earlier one's .kf: inside a batch, only the last
    written one is counted (across batches the in-order writer does it).  Only a
    file's last part decides: its earlier parts go to its side file anyway."""
    kept = set()
    for gm in reversed(genomes):
        gm.write = True
        if gm.excluded is None and gm.last:
            gm.write = gm.sample not in kept
            kept.add(gm.sample)


class ChunkPipeline:
    """Batched device pre-pass + window plan + count + threaded row writer."""

    def __init__(self, counter, device: torch.device, max_windows: int, threads: int,
                 pseudocount: bool = False):
        self.counter = counter
        self.device = torch.device(device)
        self.threads = max(1, int(threads))
        self.max_windows = max(1, int(max_windows))
        self.pseudocount = bool(pseudocount)
        self.writer = ThreadPoolExecutor(max_workers=1)   # launches are written in order
        self.pending = []
        self._wbuf = None
        # count rows go back on their own stream, so the next batch's H2D (on the
        # compute stream) overlaps them (PCIe is full duplex)
        self.d2h = torch.cuda.Stream(self.device)
        # the device formatter's text: a copier thread brings it to two pinned slabs, which the writer gives back
        self.copier = ThreadPoolExecutor(max_workers=1)
        self._pin, self._pin_size = [None, None], [0, 0]
        self._free = queue.SimpleQueue()
        for b in range(2):
            self._free.put(b)

    # ------------------------------------------------------------ pre-pass
    def prepare(self, hb, genomes: list[Genome]) -> torch.Tensor:
        """Compact every record of the batch on the device and plan the windows of
        every genome (one device-to-host copy).  Fills genomes[i].names/starts/
        excluded; returns the processed sequence buffer (device)."""
        import time
        t0 = time.perf_counter()
        data = hb.data.numpy()
        rec_se: list[int] = []
        rec_ids: list[str] = []
        ex = hb.excl
        # the batch's header intervals, per genome (sorted, genome by genome)
        bounds = np.searchsorted(ex[0::2], hb.off) if ex.size else np.zeros(hb.off.size, np.int64)
        for g, gm in enumerate(genomes):
            lo, hi = int(hb.off[g]), int(hb.off[g + 1])
            iv = ex[2 * int(bounds[g]): 2 * int(bounds[g + 1])]
            se, ids = records_from_index(data, iv, lo, hi)
            gm.rec_lo = len(rec_ids)
            rec_se += se
            rec_ids += ids
            gm.rec_hi = len(rec_ids)
        n_rec = len(rec_ids)
        _tr("records", t0, n_rec=n_rec)
        t0 = time.perf_counter()
        dev = self.device
        stream = torch.cuda.current_stream(dev)
        total = int(hb.off[-1])
        d_bytes = hb.data.to(dev, non_blocking=True)
        d_out = torch.empty(max(total, 16) + 16, dtype=torch.uint8, device=dev)
        if n_rec:
            host_se = torch.from_numpy(np.asarray(rec_se, dtype=np.int64))
            if hb.data.is_pinned():
                host_se = host_se.pin_memory()
            d_se_in = host_se.to(dev, non_blocking=True)
            d_se = torch.empty(2 * n_rec, dtype=torch.int64, device=dev)
            nwords = (total + 4095) // 4096 + 1
            scratch = torch.empty(nwords, dtype=torch.int32, device=dev)
            N.check(N.lib().kf_chunk_compact(d_bytes.data_ptr(), total, d_se_in.data_ptr(), n_rec, d_out.data_ptr(),
                                             d_se.data_ptr(), scratch.data_ptr(), nwords, stream.cuda_stream),
                    "kf_chunk_compact")
            out_se = d_se.cpu().numpy().view(np.uint64)      # the batch's one synchronising copy
        else:
            out_se = np.zeros(0, np.uint64)
        _tr("h2d_compact_d2h", t0, bytes=total)
        t0 = time.perf_counter()
        for gm in genomes:
            starts, pos_l, pre_l = [], [], []
            for r in range(gm.rec_lo, gm.rec_hi):
                a, b = int(out_se[2 * r]), int(out_se[2 * r + 1])
                L = b - a
                if L < CHUNK_SZ:                                   # seqkit seq -m 10000 (main.py:753)
                    continue
                n, step = window_plan(L)
                cid = rec_ids[r]
                pos = np.arange(n, dtype=np.int64) * step
                starts.append(a + pos)
                pos_l.append(pos)
                pre_l.append(np.full(n, len(gm.prefixes), np.uint32))
                gm.prefixes.append("{}.part_{}.part_{}_sliding__".format(gm.sample, cid, cid))
            cat = (lambda x, t: np.concatenate(x) if x else np.zeros(0, t))
            gm.starts, gm.wpos, gm.wpre = cat(starts, np.int64), cat(pos_l, np.int64), cat(pre_l, np.uint32)
            if not starts:
                gm.excluded = "none"                               # main.py:761-778
            elif gm.n_windows < CHUNK_CNT_THR:
                gm.excluded = "few"                                # main.py:845-860
        shadow(genomes)
        _tr("plan", t0, windows=sum(g.n_windows for g in genomes))
        return d_out

    # ------------------------------------------------------------ count
    def _count_launches(self, d_seq: torch.Tensor, work: list[Genome]):
        """Gather and count the windows of `work` (genome after genome, one flat
        window list), at most max_windows per count launch: yields (w0, w1, c16)
        per launch, c16 the rows of the windows [w0, w1) on the device."""
        dev = self.device
        starts = np.concatenate([g.starts for g in work]).astype(np.int64)
        total = int(starts.size)
        d_starts = torch.from_numpy(starts).pin_memory().to(dev, non_blocking=True)
        stream = torch.cuda.current_stream(dev)
        for w0 in range(0, total, self.max_windows):
            w1 = min(total, w0 + self.max_windows)
            nw = w1 - w0
            if self._wbuf is None or self._wbuf.numel() < nw * CHUNK_SZ:
                self._wbuf = torch.empty(nw * CHUNK_SZ, dtype=torch.uint8, device=dev)
            N.check(N.lib().kf_chunk_gather(d_seq.data_ptr(), d_starts[w0:].data_ptr(), nw, CHUNK_SZ,
                                            self._wbuf.data_ptr(), stream.cuda_stream), "kf_chunk_gather")
            from .counter import DeviceBatch
            off = torch.arange(0, (nw + 1) * CHUNK_SZ, CHUNK_SZ, dtype=torch.int64, device=dev)
            db = DeviceBatch(self._wbuf, off, torch.zeros(2, dtype=torch.int64, device=dev), nw, 0)
            counts, _ = self.counter.count(db)
            # a window has at most CHUNK_SZ - k + 1 < 2^16 k-mers: its counts are kept
            # (and cross PCIe) as uint16 bit patterns, half the bytes of the u32 rows
            c16 = counts.to(torch.int16)
            del counts
            yield w0, w1, c16
            del c16

    def count_rows(self, d_seq: torch.Tensor, genomes: list[Genome]) -> tuple[list[Genome], list[torch.Tensor]]:
        """count_and_write without the write: the batch's kept genomes and their
        window rows, int16 [windows, nbins] holding uint16 bit patterns, one tensor
        per count launch, left on the device (genome after genome, as the .kf
        files' rows would be)."""
        work = [g for g in genomes if g.excluded is None and g.write]
        return work, ([c16 for _, _, c16 in self._count_launches(d_seq, work)] if work else [])

    # ------------------------------------------------------------ count + write
    def count_and_write(self, d_seq: torch.Tensor, genomes: list[Genome], output_dir: str) -> list:
        """Gather, count and (asynchronously) write the windows of the batch's
        kept genomes, at most max_windows per count launch.  Returns the futures
        of the batch's writes."""
        work = [g for g in genomes if g.excluded is None and g.write]
        futs = []
        if not work:
            return futs
        row0 = np.cumsum([0] + [g.n_windows for g in work])
        stream = torch.cuda.current_stream(self.device)
        for w0, w1, c16 in self._count_launches(d_seq, work):
            # the segments of this launch: each genome's rows inside [w0, w1)
            segs = []
            for gi, g in enumerate(work):
                a, b = max(int(row0[gi]), w0), min(int(row0[gi + 1]), w1)
                if a >= b:
                    continue
                segs.append((os.path.join(output_dir, g.out_name or "{}.kf".format(g.sample)), a - w0, b - w0, g,
                             a - int(row0[gi]), g.cont or a > int(row0[gi])))
            args = self._write_args(segs)   # built here: the writer thread only formats or copies, and writes
            if len(self.pending) >= 2:      # at most two launches queued for the writer
                self.pending.pop(0).result()
            # the text is made on the device where that measured no slower than the
            # host formatter
            if args is not None and self.counter.k in DEVICE_FORMAT_K:
                q = queue.SimpleQueue()
                self.copier.submit(self._copy_text, self._format_launch(c16, args), q)
                futs.append(self.writer.submit(self._write_text, q, args))
            else:
                done = torch.cuda.Event()
                done.record(stream)
                self.d2h.wait_event(done)
                host = torch.empty(c16.shape, dtype=torch.int16, pin_memory=True)
                with torch.cuda.stream(self.d2h):
                    host.copy_(c16, non_blocking=True)
                    c16.record_stream(self.d2h)
                    ev = torch.cuda.Event()
                    ev.record(self.d2h)
                futs.append(self.writer.submit(self._write, ev, host, args))
            self.pending.append(futs[-1])
            del c16
        return futs

    def _write_args(self, segs):
        """kf_write_kf_segments' arguments for one launch's segments (consecutive
        row ranges): paths, row bounds, append flags and the row-name parts (the
        writer builds the names from contig prefixes and window positions)."""
        import time
        t0 = time.perf_counter()
        if not segs:
            return None
        # consecutive segments of one file (the parts of a file counted in
        # record-aligned parts) are one native segment: the writer opens each
        # segment's file once and lays its rows out from the file's end
        first = [i for i in range(len(segs)) if i == 0 or segs[i][0] != segs[i - 1][0]]
        ends = [segs[j - 1][2] for j in first[1:]] + [segs[-1][2]]
        paths = (ctypes.c_char_p * len(first))(*[os.fsencode(segs[i][0]) for i in first])
        row0 = np.asarray([0] + ends, dtype=np.int32)
        app = np.asarray([1 if segs[i][5] else 0 for i in first], dtype=np.uint8)
        pre, rpre, rpos = [], [], []
        for _, a, b, g, o, _ap in segs:
            rpre.append(g.wpre[o: o + (b - a)].astype(np.uint32) + len(pre))
            rpos.append(g.wpos[o: o + (b - a)].astype(np.uint64))
            pre += g.prefixes
        rpre = np.ascontiguousarray(np.concatenate(rpre), dtype=np.uint32)
        rpos = np.ascontiguousarray(np.concatenate(rpos), dtype=np.uint64)
        enc = [x.encode(errors="surrogateescape") for x in pre]
        arr = (ctypes.c_char_p * len(enc))(*enc)
        _tr("encode_names", t0, rows=int(rpos.size))
        return (len(first), paths, row0, app, enc, arr, rpre, rpos)

    # ------------------------------------------------------------ device formatter
    def _format_launch(self, c16: torch.Tensor, args) -> list:
        """Enqueue kf_format_kf_rows16 for one launch's rows, in as many calls as
        keep a call's text bound below 2^32, and the copy of every call's row
        offsets and status to the host on the d2h stream.  Returns per call
        (r0, r1, text, row_off + status on the host, its event)."""
        import time
        from .counter import KF_FORMAT_MAX_CAP, format_kf_row_bound, format_kf_rows
        t0 = time.perf_counter()
        _n_seg, _paths, _row0, _app, enc, _arr, rpre, rpos = args
        dev = self.device
        stream = torch.cuda.current_stream(dev)
        n, nbins = int(c16.shape[0]), int(c16.shape[1])
        bound = format_kf_row_bound(nbins, max(len(x) for x in enc), CHUNK_SZ)
        per = max(1, KF_FORMAT_MAX_CAP // bound)
        # the launch's name tables go to the device once
        d_rpre = torch.from_numpy(rpre.view(np.int32)).to(dev, non_blocking=True)
        d_rpos = torch.from_numpy(rpos.view(np.int64)).to(dev, non_blocking=True)
        calls = []
        for r0 in range(0, n, per):
            r1 = min(n, r0 + per)
            text, row_off, status = format_kf_rows(c16[r0:r1], enc, d_rpre[r0:r1], d_rpos[r0:r1], CHUNK_SZ,
                                                   self.pseudocount)
            done = torch.cuda.Event()
            done.record(stream)
            self.d2h.wait_event(done)
            small = torch.empty(4 + r1 - r0 + 1, dtype=torch.int64, pin_memory=True)
            with torch.cuda.stream(self.d2h):
                small[:4].copy_(status, non_blocking=True)
                small[4:].copy_(row_off, non_blocking=True)
                for t in (text, row_off, status):
                    t.record_stream(self.d2h)
                ev = torch.cuda.Event()
                ev.record(self.d2h)
            calls.append((r0, r1, text, small, ev))
        _tr("format_device", t0, rows=n, calls=len(calls))
        return calls

    def _copy_text(self, calls, q) -> None:
        """One launch's text to the host (copier thread): per format call, once its
        row offsets are on the host, the used bytes cross PCIe on the d2h stream
        in pieces of at most TEXT_SLAB, each into a pinned slab that the writer has
        given back (a piece of at most TEXT_SMALL bytes into a pinned buffer of its
        own); q gets (r0, r1, row offsets, lo, hi, slab, event, host buffer) per
        piece, then None (or the exception).  So the next launch's text is copied while
        the writer writes this one's."""
        import time
        from .counter import format_status_check
        try:
            with torch.cuda.device(self.device):
                for r0, r1, text, small, ev in calls:
                    t0 = time.perf_counter()
                    ev.synchronize()
                    h = small.numpy()
                    format_status_check(int(h[0]), int(h[1]), int(h[2]), int(text.numel()))
                    off = h[4:]
                    total = int(off[-1])
                    _tr("wait_format", t0, bytes=total)
                    for lo in range(0, total, TEXT_SLAB):
                        hi = min(total, lo + TEXT_SLAB)
                        if hi - lo <= TEXT_SMALL:         # (a launch's last few windows) no slab is held for it
                            b, host = None, torch.empty(hi - lo, dtype=torch.uint8, pin_memory=True)
                        else:
                            b = self._free.get()          # a slab the writer is done with
                            if self._pin[b] is None or self._pin[b].numel() < hi - lo:
                                self._pin[b] = None       # grown at least 2x, up to the slab size
                                self._pin[b] = torch.empty(min(TEXT_SLAB, max(hi - lo, 2 * self._pin_size[b])),
                                                           dtype=torch.uint8, pin_memory=True)
                                self._pin_size[b] = self._pin[b].numel()
                            host = self._pin[b]
                        done = torch.cuda.Event()
                        with torch.cuda.stream(self.d2h):
                            host[: hi - lo].copy_(text[lo:hi], non_blocking=True)
                            done.record(self.d2h)
                        q.put((r0, r1, off, lo, hi, b, done, host))
            q.put(None)
        except BaseException as e:   # the writer raises it
            q.put(e)

    def _write_text(self, q, args) -> None:
        """One launch's text to its files (writer thread): every piece that the
        copier queued, once it is on the host, goes to kf_write_text_segments as
        the byte ranges of the files it covers."""
        import time
        n_seg, paths, row0, app, _enc, _arr, _rpre, _rpos = args
        lib = N.lib()
        started = [False] * n_seg          # a file is truncated (unless appended) by its segment's first range only
        item = None
        try:
            while True:
                item = q.get()
                if item is None:
                    return
                if isinstance(item, BaseException):
                    raise item
                r0, r1, off, lo, hi, b, done, host = item
                t1 = time.perf_counter()
                done.synchronize()
                _tr("text_d2h", t1, bytes=hi - lo)
                t1 = time.perf_counter()
                # the piece's segments: (segment, first byte, end byte), back to back
                use = []
                for g in range(n_seg):
                    x, y = max(int(row0[g]), r0), min(int(row0[g + 1]), r1)
                    if x < y:                  # (a segment has rows, and a row has bytes)
                        x, y = max(int(off[x - r0]), lo), min(int(off[y - r0]), hi)
                        if x < y:
                            use.append((g, x, y))
                cp = (ctypes.c_char_p * len(use))(*[paths[g] for g, _, _ in use])
                ap = np.asarray([1 if (app[g] or started[g]) else 0 for g, _, _ in use], dtype=np.uint8)
                so = np.asarray([use[0][1] - lo] + [y - lo for _, _, y in use], dtype=np.uint64)
                for g, _, _ in use:
                    started[g] = True
                N.check(lib.kf_write_text_segments(len(use), cp, ap.ctypes.data, so.ctypes.data,
                                                   host.data_ptr(), self.threads), "kf_write_text_segments")
                if b is not None:
                    self._free.put(b)
                item = None
                _tr("write_text", t1, segs=len(use), bytes=hi - lo)
        finally:
            # after an error: give back the slabs of the pieces that were not written, or the copier waits for ever
            while item is not None and not isinstance(item, BaseException):
                if item[5] is not None:
                    self._free.put(item[5])
                item = q.get()

    def _write(self, ev, host: torch.Tensor, args) -> None:
        """Format + write one launch's rows, once its counts are on the host."""
        import time
        t0 = time.perf_counter()
        ev.synchronize()
        _tr("wait_d2h", t0)
        if args is None:
            return
        t0 = time.perf_counter()
        n_seg, paths, row0, app, _enc, arr, rpre, rpos = args
        rows = host.numpy().view(np.uint16)
        N.check(N.lib().kf_write_kf_segments16(n_seg, paths, row0.ctypes.data, app.ctypes.data, None, arr,
                                               rpre.ctypes.data, rpos.ctypes.data, CHUNK_SZ, rows.ctypes.data,
                                               rows.shape[1], int(self.pseudocount), 1, self.threads),
                "kf_write_kf_segments16")
        _tr("format_write", t0, segs=n_seg)

    def after_writes(self, fn):
        """Run fn on the writer thread once every write queued so far is done
        (the writer runs in order); returns its future."""
        f = self.writer.submit(fn)
        self.pending.append(f)
        return f

    def drain(self) -> None:
        """Wait for every queued write."""
        while self.pending:
            self.pending.pop(0).result()

    def close(self) -> None:
        self.drain()
        self.writer.shutdown()
        self.copier.shutdown()


def compact_records_host(data, se) -> tuple[bytes, np.ndarray]:
    """The host statement of kf_chunk_compact (include/kf2vec_gpu.h has the
    contract): (out, out_se uint64 [2n]) for the n sorted, disjoint ranges
    se = [a0, b0, a1, b1, ...] of `data`.  Range r is seqtk -> awk -> seqkit
    applied to data[a:b]: split at '\\n', one trailing '\\r' dropped from every
    piece (the last one included), the pieces joined, [Nn|]+ -> N, then the gap
    letters "- \\t." deleted.  `out` is the results back to back and
    out_se[2r], out_se[2r+1] the running offsets.  Regular expressions and no
    look-back, so it shares nothing with the kernel's per-byte rule.  Only
    tests call it; no product path does."""
    import re
    data = bytes(data) if isinstance(data, (bytes, bytearray, memoryview)) else \
        np.ascontiguousarray(data, dtype=np.uint8).tobytes()
    se = np.asarray(se, dtype=np.uint64).reshape(-1)
    nrun, gaps = re.compile(rb"[Nn|]+"), re.compile(rb"[- \t.]")
    parts, out_se, pos = [], np.zeros(se.size, dtype=np.uint64), 0
    for r in range(se.size // 2):
        a, b = int(se[2 * r]), int(se[2 * r + 1])
        seq = b"".join(p[:-1] if p.endswith(b"\r") else p for p in data[a:b].split(b"\n"))
        seq = gaps.sub(b"", nrun.sub(b"N", seq))
        parts.append(seq)
        out_se[2 * r] = pos
        pos += len(seq)
        out_se[2 * r + 1] = pos
    return b"".join(parts), out_se


# ---------------------------------------------------------------------------
# in-memory hand-off to the chunk trainer (kf_chunk_features)
# ---------------------------------------------------------------------------
def range_features_host(rows: np.ndarray, lo, n, scaler: float = 1.0, cap: int | None = None) -> np.ndarray:
    """The numpy statement of kf_chunk_features (float64 [S, nbins]): sample s is
    the column-wise sum of rows[lo[s]: lo[s] + n[s]] (whole-number counts, each as
    min(count, cap) if `cap` is given) over its grand total, times `scaler` --
    one view of Dataset_chunks_2rows (kf2vec/datasets.py:47-62; the numpy class
    :143-157), NaN and inf of an all-zero run replaced by 0 as there.  The tests
    compare the kernel with it; no product path calls it."""
    rows = np.asarray(rows)
    lo, n = np.asarray(lo).reshape(-1), np.asarray(n).reshape(-1)
    out = np.empty((lo.size, rows.shape[1]), dtype=np.float64)
    for s in range(lo.size):
        r = rows[int(lo[s]): int(lo[s]) + int(n[s])].astype(np.uint64)
        if cap is not None:
            r = np.minimum(r, np.uint64(cap))
        c = r.sum(axis=0)
        with np.errstate(invalid="ignore", divide="ignore"):
            x = c.astype(np.float64) / np.float64(c.sum())
        out[s] = np.nan_to_num(x, nan=0.0, posinf=0.0, neginf=0.0) * scaler
    return out


def draw_ranges(c, rng, views: int = 2) -> tuple[np.ndarray, np.ndarray]:
    """The row runs Dataset_chunks_2rows draws (kf2vec/datasets.py:47-52, :74-79)
    for items with c[i] window rows: (lo, n) int64 [len(c), views], run (i, v)
    being the rows [lo, lo + n) of item i.  `rng` is a numpy.random.RandomState
    or the numpy.random module; the draws are the reference's, item by item and
    view by view: exponential(c / 5) for the length floor(draw) + 1, a
    randint(1, c + 1) instead only if that passes c, then randint(0, c - n + 1)
    for the start -- so a stream seeded like the reference's gives its runs."""
    c = np.asarray(c, dtype=np.int64).reshape(-1)
    if c.size and int(c.min()) < 1:
        raise ValueError("draw_ranges: every item needs at least one row")
    lo = np.empty((c.size, views), dtype=np.int64)
    n = np.empty((c.size, views), dtype=np.int64)
    for i, ci in enumerate(c.tolist()):
        for v in range(views):
            m = int(np.floor(rng.exponential(ci / 5)) + 1)
            if m > ci:
                m = int(rng.randint(low=1, high=ci + 1))
            lo[i, v] = rng.randint(low=0, high=ci - m + 1)
            n[i, v] = m
    return lo, n


@dataclass
class ChunkStore:
    """A directory's window count rows on the device, as train_model_set_chunks
    holds them after my_read_csv_chunk (kf2vec/utils.py:402-405): genome g's rows
    are counts[row0[g]: row0[g + 1]]."""
    # int16 [W, nbins] holding uint16 bit patterns, the kept genomes' rows back to back; or uint8 [W, nbins], each
    # count as min(count, 255) (chunk_store_from_kf(cap8=True): utils.my_read_csv_chunk_capped's store)
    counts: torch.Tensor
    row0: np.ndarray        # int64 [G + 1], host
    samples: list           # G sample names
    excluded: dict          # sample name -> "none" (no contig >= 10 kbp) or "few" (windows)
    k: int

    @classmethod
    def from_host(cls, rows_per_genome, samples, k: int, device="cuda") -> "ChunkStore":
        """A store of uint16 [windows, nbins] arrays, one per genome (the parsed rows of its .kf file); or of
        uint8 arrays, all of them (rows capped at 255), which make a uint8 store."""
        from .counter import num_bins
        nb = num_bins(k)
        rows = [np.asarray(r) for r in rows_per_genome]
        if len(rows) != len(samples):
            raise ValueError("ChunkStore.from_host: {} genomes but {} sample names".format(len(rows), len(samples)))
        width = np.uint8 if rows and all(r.dtype == np.uint8 for r in rows) else np.uint16
        for r, name in zip(rows, samples):
            if r.dtype != width or r.ndim != 2 or r.shape[1] != nb:
                raise ValueError("ChunkStore.from_host: {}: rows must be uint16 (or all uint8) [windows, {}] at k={}, "
                                 "got {} {}".format(name, nb, k, r.dtype, r.shape))
        row0 = np.cumsum([0] + [r.shape[0] for r in rows]).astype(np.int64)
        host = np.ascontiguousarray(np.concatenate(rows) if rows else np.zeros((0, nb), np.uint16))
        counts = torch.from_numpy(host if width == np.uint8 else host.view(np.int16)).to(torch.device(device))
        return cls(counts, row0, list(samples), {}, k)

    def batch(self, idx, rng, scaler: float = 1e4, cap: int | None = None, dtype: torch.dtype = torch.float32):
        """One training batch: (Z [B, 2 * nbins], y int64 [B]) on the device for
        the genomes idx, as Dataset_chunks_2rows gives them item by item
        (kf2vec/datasets.py:91-93): Z[b] is two views of genome idx[b] side by
        side (draw_ranges from `rng`, one kf_chunk_features call over the 2 B
        runs), y = idx the label index."""
        from .counter import chunk_features
        idx = np.asarray(idx, dtype=np.int64).reshape(-1)
        lo, n = draw_ranges(self.row0[idx + 1] - self.row0[idx], rng)
        lo += self.row0[idx][:, None]
        z = chunk_features(self.counts, lo.reshape(-1), n.reshape(-1), scaler, cap, dtype)
        return z.view(idx.size, 2 * self.counts.shape[1]), torch.from_numpy(idx).to(self.counts.device)


def chunk_store(input_dir: str, k: int, device="cuda", batch_gb: float = 1.0, p=None) -> ChunkStore:
    """The store `get_chunks -k k` on input_dir and parsing its .kf files would
    give, without the files: the same input files (main.list_inputs), batches,
    pre-pass, window plan and count launches (ChunkPipeline.prepare /
    count_rows), every launch's uint16 rows kept on the device.  The genomes come
    in input order; of files that share a sample name the last kept one stands,
    at its place, as its .kf would have replaced the earlier one's; a genome
    with no contig of 10 kbp or fewer than 5 windows is listed in `excluded`.
    A file above main.SPLIT_BYTES is refused (ValueError) before anything is
    counted: files counted in record parts are out of scope here."""
    from . import main as M
    from .counter import KmerCounter, pack_files
    files_names, samples_names = M.list_inputs(input_dir)
    paths = [os.path.join(input_dir, f) for f in files_names]
    sizes = [os.path.getsize(q) for q in paths]
    big = [f for f, s in zip(files_names, sizes) if s > M.SPLIT_BYTES]
    if big:
        raise ValueError("chunk_store: input file(s) above {} bytes are not supported (get_chunks counts them in "
                         "record parts): {}".format(M.SPLIT_BYTES, ", ".join(big[:5])))
    if k not in M.supported_k:
        raise ValueError("k={} has no vocabulary: supported k are {}..{}".format(
            k, M.supported_k.start, M.supported_k.stop - 1))
    device = torch.device(device)
    counter = KmerCounter(k, device)
    budget = int(float(batch_gb or 1.0) * (1 << 30))
    max_windows = max(1, min(budget // CHUNK_SZ, budget // (4 * counter.nbins), LAUNCH_WINDOWS))   # as get_chunks
    threads = M.host_threads(p if p is not None else os.cpu_count() or 1)
    pipe = ChunkPipeline(counter, device, max_windows, threads)
    kept: dict = {}       # sample -> its rows, in the order of the files that stand
    excluded: dict = {}
    with ThreadPoolExecutor(max_workers=threads) as pool:
        for idx in M._size_batches(sizes, min(budget, 3 << 30, max(sum(sizes) // 4, 16 << 20)), ramp=True):
            hb = pack_files([paths[i] for i in idx], [samples_names[i] for i in idx], fmt=N.KF_FMT_FASTA, pool=pool)
            genomes = [Genome(files_names[i], samples_names[i]) for i in idx]
            d_seq = pipe.prepare(hb, genomes)
            work, launches = pipe.count_rows(d_seq, genomes)
            rows = torch.cat(launches) if launches else None
            w0 = 0
            for gm in work:
                kept.pop(gm.sample, None)   # a later file of the same name replaces it
                kept[gm.sample] = rows[w0: w0 + gm.n_windows]
                w0 += gm.n_windows
            for gm in genomes:
                if gm.excluded is not None:
                    excluded[gm.sample] = gm.excluded
            del hb, d_seq
    pipe.close()
    samples = list(kept)
    excluded = {s: why for s, why in excluded.items() if s not in kept}
    row0 = np.cumsum([0] + [int(kept[s].shape[0]) for s in samples]).astype(np.int64)
    counts = torch.cat([kept[s] for s in samples]) if samples else \
        torch.zeros((0, counter.nbins), dtype=torch.int16, device=device)
    return ChunkStore(counts.contiguous(), row0, samples, excluded, k)


# ---------------------------------------------------------------------------
# a get_chunks .kf directory as a ChunkStore (kf_parse_kf_rows)
# ---------------------------------------------------------------------------
KF_PIECE_BYTES = 1 << 30   # chunk_store_from_kf: .kf files above this go through in kf_line_pieces


def format_rows_host(rows: np.ndarray, prefixes, row_prefix, row_start, win_len: int, pseudocount: bool
                     ) -> tuple[bytes, np.ndarray]:
    """What kf_format_kf_rows16 computes, stated with the host formatter: the
    lines of the uint16 rows back to back, and every line's offset (n + 1).  Row
    r is main.format_kf(name, row, pseudocount, raw_cnt=True), the C++ formatter
    that tests/golden/ref_postproc pins, named as Genome.names builds names:
    prefixes[row_prefix[r]] (bytes, or str) followed, if win_len != 0, by
    "<s+1>-<s+win_len>" for s = row_start[r] (uint64 arithmetic).  No product
    path calls it."""
    from .main import format_kf
    rows = np.asarray(rows)
    rows = rows.view(np.uint16) if rows.dtype == np.int16 else rows
    pre = [x.decode(errors="surrogateescape") if isinstance(x, (bytes, bytearray)) else x for x in prefixes]
    out, off = [], [0]
    for r in range(rows.shape[0]):
        name = pre[int(row_prefix[r])]
        if win_len:
            s = int(row_start[r])
            name += "{}-{}".format((s + 1) % (1 << 64), (s + int(win_len)) % (1 << 64))
        out.append(format_kf(name, rows[r].astype(np.uint32), bool(pseudocount), raw_cnt=True))
        off.append(off[-1] + len(out[-1]))
    return b"".join(out), np.asarray(off, dtype=np.int64)


def _field_error(f: bytes) -> int:
    """The first error of one field read left to right: 0 none, 3 malformed, 4 above 65535."""
    v, st = 0, 0           # st: 0 no digit yet, 1 in the digits, 2 after the '.'
    for c in f:
        if 48 <= c <= 57:
            if st == 2:
                if c != 48:
                    return 3
                continue
            v, st = v * 10 + (c - 48), 1
            if v > 65535:
                return 4
        elif c == 46 and st == 1:
            st = 2
        else:
            return 3
    return 3 if st == 0 else 0


def parse_kf_rows_host(data: bytes, nbins: int, cap_rows: int | None = None):
    """The host statement of kf_parse_kf_rows for ONE unit of `.kf` text
    (include/kf2vec_gpu.h has the contract): (rows uint16 [n, nbins], (code, row,
    column)).  A line ends before a '\\n' or at the end of `data`; an empty line is
    no row; a row is a name (every byte up to the first ',') and exactly nbins
    fields, each one or more digits, optionally '.' and zeros, at most 65535.
    (0, 0, 0) and every row if the text is fine; else the code of the error at
    the lowest byte offset -- 1 too few fields (column: the fields there are), 2
    too many (column nbins), 3 malformed field, 4 value above 65535, 5 a row
    numbered cap_rows exists (column 0) -- with its row and column, and the rows
    before that row.  The tests compare the kernel with it; no product path calls it."""
    import re
    nbins = int(nbins)
    well = re.compile(rb"[^,]*(?:,[0-9]+(?:\.0*)?)*")
    rows = []
    for line in bytes(data).split(b"\n"):
        if not line:
            continue
        r = len(rows)
        if cap_rows is not None and r >= cap_rows:
            return _rows_array(rows, nbins), (5, r, 0)
        fields = line.split(b",")[1:]
        if well.fullmatch(line) and len(fields) == nbins:      # the usual row, without a Python loop
            v = np.asarray(fields, dtype="S").astype(np.float64) if fields else np.zeros(0)
            if not (v > 65535).any():
                rows.append(v.astype(np.uint16))
                continue
        for j, f in enumerate(fields):
            if j >= nbins:
                return _rows_array(rows, nbins), (2, r, nbins)
            e = _field_error(f)
            if e:
                return _rows_array(rows, nbins), (e, r, j)
        if len(fields) < nbins:
            return _rows_array(rows, nbins), (1, r, len(fields))
        raise AssertionError("parse_kf_rows_host: the two readings of a row disagree")
    return _rows_array(rows, nbins), (0, 0, 0)


def _rows_array(rows: list, nbins: int) -> np.ndarray:
    return np.stack(rows) if rows else np.zeros((0, nbins), np.uint16)


def kf_line_pieces(path: str, piece: int | None = None, start: int = 0) -> list[tuple[int, int]]:
    """Byte ranges [(a_i, e_i)] that cut a `.kf` file into parts of about `piece`
    bytes at line starts, as main.record_pieces cuts FASTA at records: the parts
    tile the file, every part but the first starts right after a '\\n', and a
    single line longer than `piece` stays whole.  The last line needs no '\\n'.
    `start`: a line start to begin at (the parts tile the file from there on: a
    table whose header line the caller read itself, tables.table_from_tsv)."""
    piece = KF_PIECE_BYTES if piece is None else int(piece)
    size = os.path.getsize(path)
    start = min(int(start), size)
    if size - start <= piece:
        return [(start, size)]
    cuts = [start]
    with open(path, "rb") as f:
        while cuts[-1] + piece < size:
            pos = cuts[-1] + piece          # the first line start at or after pos
            f.seek(pos - 1)
            c = size
            while True:
                blk = f.read(1 << 20)
                if not blk:
                    break
                i = blk.find(b"\n")
                if i >= 0:
                    c = f.tell() - len(blk) + i + 1
                    break
            if c >= size:
                break
            cuts.append(c)
    return [(c, cuts[i + 1] if i + 1 < len(cuts) else size) for i, c in enumerate(cuts)]


def chunk_store_from_kf(kf_dir: str, k: int, device="cuda", samples=None, batch_gb: float = 1.0, p=None,
                        cap8: bool = False) -> ChunkStore:
    """The store of a directory of get_chunks `.kf` files (this tool's or the
    reference's), as train_model_set_chunks holds them after my_read_csv_chunk
    under mp.Pool (kf2vec/train_model_set_chunks.py:251-264), with the text parsed
    on the device (kf_parse_kf_rows): what chunk_store gives for the FASTA files
    the directory was made from, without them.

    samples=None: every `*.kf` of kf_dir, sorted by name; else `<sample>.kf` for
    each name in the order given (a missing file is a ValueError before anything
    is read).  A file of no rows is listed in `excluded` as "none".  Files of any
    size: one above KF_PIECE_BYTES goes through in kf_line_pieces.  The units
    (files and pieces) are read in batches of about batch_gb GiB (a larger unit
    alone, below 4 GiB) by pack_ranges on a reader thread, one batch ahead of the
    device, into two pinned buffers in turn; each batch is copied to the device
    and parsed there, and one small copy per batch brings its units' row counts
    (and any refusal: a ValueError naming file, row and column) back.  The
    batches' rows are joined by one torch.cat at the end, so the peak device
    memory is the store plus its parts (twice the store) plus one batch.

    cap8=True: the store of utils.my_read_csv_chunk_capped (the trainers' -cap),
    every count as min(count, 255) in one byte: each batch's parsed rows go
    through kf_rows_cap8 and only the uint8 rows are kept, so the parts, their
    join and `counts` (torch.uint8) are half the bytes."""
    from . import main as M
    from .counter import num_bins, pack_ranges, parse_kf_rows, parsed_to_host, rows_cap8
    if k not in M.supported_k:
        raise ValueError("k={} has no vocabulary: supported k are {}..{}".format(
            k, M.supported_k.start, M.supported_k.stop - 1))
    if samples is None:
        samples = sorted(f[:-3] for f in os.listdir(kf_dir) if f.endswith(".kf"))
    samples = list(samples)
    paths = [os.path.join(kf_dir, s + ".kf") for s in samples]
    missing = [q for q in paths if not os.path.isfile(q)]
    if missing:
        raise ValueError("chunk_store_from_kf: no such file(s): {}".format(", ".join(missing[:5])))
    device = torch.device(device)
    nbins = num_bins(k)
    budget = max(1, int(float(batch_gb or 1.0) * (1 << 30)))
    threads = M.host_threads(p if p is not None else os.cpu_count() or 1)
    units = [(fi, a, e) for fi, q in enumerate(paths) for a, e in kf_line_pieces(q, min(KF_PIECE_BYTES, budget))]
    sizes = [e - a for _, a, e in units]
    if sizes and max(sizes) >= (1 << 32) - 16:
        raise ValueError("chunk_store_from_kf: {}: a single line of 4 GiB or more".format(
            paths[units[int(np.argmax(sizes))][0]]))
    batches = M._size_batches(sizes, budget)
    padded = [sum((sizes[i] + 15) // 16 * 16 for i in b) for b in batches]
    pin = device.type == "cuda"
    bufs = [torch.empty(max(padded + [16]), dtype=torch.uint8, pin_memory=pin) for _ in range(min(2, len(batches)))]

    def read(bi):
        return pack_ranges([(paths[units[i][0]], units[i][1], units[i][2]) for i in batches[bi]], pin=pin,
                           threads=threads, buf=bufs[bi % 2])

    file_rows = [0] * len(paths)
    parts = []
    with ThreadPoolExecutor(max_workers=1) as reader:
        nxt = reader.submit(read, 0) if batches else None
        for bi, b in enumerate(batches):
            hb = nxt.result()
            # the other buffer's last copy (batch bi - 1) ended before that batch's row counts came back
            nxt = reader.submit(read, bi + 1) if bi + 1 < len(batches) else None
            nbytes = int(hb.off[-1])
            d_bytes = hb.data[:max(nbytes, 16)].to(device, non_blocking=True)
            rows, unit_row0, status = parse_kf_rows(d_bytes, hb.off, nbins)
            names = [paths[units[i][0]] for i in b]
            first = [min(x for x, j in enumerate(b) if units[j][0] == units[i][0]) for i in b]
            row0 = parsed_to_host(unit_row0, status, names, [file_rows[units[i][0]] for i in b], first)
            for x, i in enumerate(b):
                file_rows[units[i][0]] += int(row0[x + 1] - row0[x])
            rows = rows[: int(row0[-1])]                   # the batch's rows without the slack of its cap
            parts.append(rows_cap8(rows) if cap8 else rows.clone())
            del rows, d_bytes, hb
    kept = [fi for fi in range(len(paths)) if file_rows[fi] > 0]
    excluded = {samples[fi]: "none" for fi in range(len(paths)) if file_rows[fi] == 0}
    row0 = np.cumsum([0] + [file_rows[fi] for fi in kept]).astype(np.int64)
    counts = torch.cat(parts) if parts else torch.zeros((0, nbins), dtype=torch.uint8 if cap8 else torch.int16,
                                                        device=device)
    del parts
    return ChunkStore(counts.contiguous(), row0, [samples[fi] for fi in kept], excluded, k)
