"""Host-side driver of the device k-mer counter.

Mirrors the per-file work of kf2vec's ``get_frequencies`` (reference
kf2vec/main.py:301-357) for a whole batch of genomes at once:

* :func:`pack_genomes` / :func:`pack_files` lay several FASTA/FASTQ files out
  back to back in one (pinned) host buffer and build the record index
  (``kf_index_records``) -- the device-side replacement of the ``jellyfish
  count`` input (main.py:309-311);
* :class:`KmerCounter` owns the per-k bin tables on the device (the vocab of
  main.py:278-296) and runs ``kf_count_batch`` on PyTorch-ROCm tensors, giving
  the ``n_genomes x nbins`` count matrix in vocab column order -- what the
  reference gets from ``jellyfish dump -c`` + the left-merge (main.py:317-328).

PyTorch is used for device memory and streams only.
"""
from __future__ import annotations

import ctypes
import dataclasses
import os
from typing import Sequence

import numpy as np
import torch

from . import _native as N

ALIGN = 16  # genome starts are 16-byte aligned inside a batch ('\n' padding)


def num_bins(k: int) -> int:
    return int(N.lib().kf_num_bins(k))


def tables(k: int) -> tuple[np.ndarray, np.ndarray]:
    """(code2col[4^k], col2rep[nbins]) -- see include/kf2vec_gpu.h kf_tables."""
    nb = num_bins(k)
    code2col = np.empty(1 << (2 * k), dtype=np.uint32)
    col2rep = np.empty(nb, dtype=np.uint32)
    n = ctypes.c_uint64(0)
    N.check(N.lib().kf_tables(k, code2col.ctypes.data, col2rep.ctypes.data, ctypes.byref(n)), "kf_tables")
    assert n.value == nb
    return code2col, col2rep


def vocab_text(k: int) -> bytes:
    nb = num_bins(k)
    buf = np.empty(nb * (k + 1), dtype=np.uint8)
    w = ctypes.c_uint64(0)
    N.check(N.lib().kf_vocab_text(k, buf.ctypes.data, buf.size, ctypes.byref(w)), "kf_vocab_text")
    return buf[: w.value].tobytes()


def index_records(data: np.ndarray, fmt: int = N.KF_FMT_AUTO, base: int = 0) -> tuple[np.ndarray, int]:
    """Excluded (non-sequence) byte ranges of one file, as a flat [s0,e0,s1,e1,...]
    uint64 array offset by ``base``; also returns the detected format."""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    cap = 64
    while True:
        out = np.empty(2 * cap, dtype=np.uint64)
        n = ctypes.c_uint64(0)
        f = ctypes.c_int(0)
        rc = N.lib().kf_index_records(data.ctypes.data, data.size, fmt, base, out.ctypes.data, cap,
                                      ctypes.byref(n), ctypes.byref(f))
        if rc == N.KF_ERANGE:
            cap = int(n.value)
            continue
        N.check(rc, "kf_index_records")
        return out[: 2 * n.value], int(f.value)


@dataclasses.dataclass
class HostBatch:
    """Genomes packed back to back: genome g = data[off[g]:off[g+1]]."""
    data: torch.Tensor | None   # uint8, (pinned) host
    off: np.ndarray             # uint64 [n+1]
    excl: np.ndarray | None     # uint64 [2*m] absolute [start, end) pairs; None: indexed on the device
    names: list[str]
    dev_data: torch.Tensor | None = None   # the bytes already copied to the device (maybe on another stream)
    dev_event: object = None               # ... and the event that copy recorded
    fastq: bool = False                    # excl None: every genome is FASTQ (kf_index_fastq), not FASTA

    @property
    def n(self) -> int:
        return len(self.off) - 1

    def seq_chars(self) -> int:
        """Sequence characters (excludes header/quality lines and newlines)."""
        d = self.data.numpy()
        nl = int(np.count_nonzero(d[: int(self.off[-1])] == 10))
        excl = self.excl if self.excl is not None else np.concatenate(
            [index_records(d[int(self.off[i]): int(self.off[i + 1])],
                           N.KF_FMT_FASTQ if self.fastq else N.KF_FMT_FASTA, int(self.off[i]))[0]
             for i in range(self.n)] or [np.zeros(0, np.uint64)])
        ex = int((excl[1::2] - excl[0::2]).sum()) if excl.size else 0
        return int(self.off[-1] - self.off[0]) - nl - ex


def _layout(sizes: Sequence[int]) -> np.ndarray:
    off = np.zeros(len(sizes) + 1, dtype=np.uint64)
    pos = 0
    for i, s in enumerate(sizes):
        off[i] = pos
        pos += (int(s) + ALIGN - 1) // ALIGN * ALIGN
    off[-1] = pos
    return off


def _alloc_host(nbytes: int, pin: bool) -> torch.Tensor:
    pin = pin and torch.cuda.is_available()
    return torch.empty(max(nbytes, ALIGN), dtype=torch.uint8, pin_memory=pin)


def pack_genomes(blobs: Sequence[bytes | np.ndarray], names: Sequence[str] | None = None,
                 fmt: int = N.KF_FMT_AUTO, pin: bool = True) -> HostBatch:
    sizes = [len(b) for b in blobs]
    off = _layout(sizes)
    data = _alloc_host(int(off[-1]), pin)
    d = data.numpy()
    d[: int(off[-1])] = 10  # '\n' padding between genomes is transparent
    excl = []
    for i, b in enumerate(blobs):
        a = np.frombuffer(b, dtype=np.uint8) if isinstance(b, (bytes, bytearray, memoryview)) else np.asarray(b, np.uint8)
        lo = int(off[i])
        d[lo: lo + a.size] = a
        iv, _ = index_records(d[lo: lo + a.size], fmt, lo)
        excl.append(iv)
    ex = np.concatenate(excl) if excl else np.zeros(0, np.uint64)
    return HostBatch(data, off, ex.astype(np.uint64), list(names) if names else [str(i) for i in range(len(blobs))])


def pack_files(paths: Sequence[str], names: Sequence[str] | None = None, fmt: int = N.KF_FMT_AUTO,
               pin: bool = True, threads: int = 8, pool=None, times: dict | None = None,
               buf: torch.Tensor | None = None, index: bool = True, piece: int = 1 << 20) -> HostBatch:
    """Read files straight into one (pinned) buffer and index their records.  The
    bytes come from one native call (kf_read_files: pieces of at most `piece`
    bytes read by pread on native threads, as many as `pool` has workers or
    `threads`); FASTQ files (and FASTA ones when index=True) are then indexed by
    the pool (the ctypes index calls release the GIL).
    `buf`: a caller-owned (pinned) buffer of at least the batch's bytes to read
    into instead of a fresh allocation (the caller makes sure no copy still reads it).
    index=False: a batch of FASTA files is not indexed here (excl None: to_device
    finds the header lines on the device, kf_index_fasta), nor is a batch whose
    non-empty files are all FASTQ (excl None and fastq set: kf_index_fastq); a
    batch that mixes the two is indexed on the host all the same."""
    from concurrent.futures import ThreadPoolExecutor
    import time
    t0 = time.perf_counter()
    sizes = [os.path.getsize(p) for p in paths]
    off = _layout(sizes)
    if buf is not None and buf.numel() >= max(int(off[-1]), ALIGN):
        data = buf[: max(int(off[-1]), ALIGN)]
    else:
        data = _alloc_host(int(off[-1]), pin)
    d = data.numpy()
    if times is not None:
        times["alloc_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    # the bytes: one native call (kf_read_files: pread pieces on native threads)
    nthr = getattr(pool, "_max_workers", None) or max(1, int(threads))
    if paths:
        enc = [os.fsencode(p) for p in paths]
        arr = (ctypes.c_char_p * len(enc))(*enc)
        sz = np.asarray(sizes, dtype=np.uint64)
        N.check(N.lib().kf_read_files(arr, len(enc), sz.ctypes.data, off.ctypes.data, d.ctypes.data,
                                      int(piece), int(nthr)), "kf_read_files")

    def is_fastq(i: int) -> bool:
        return fmt == N.KF_FMT_FASTQ or (fmt == N.KF_FMT_AUTO and sizes[i] > 0 and d[int(off[i])] == ord("@"))

    def on_host(i: int) -> bool:   # FASTQ (or index=True): the host index
        return index or is_fastq(i)

    def host_index(i: int):
        lo, sz = int(off[i]), sizes[i]
        return index_records(d[lo: lo + sz], fmt, lo)[0] if on_host(i) else None

    if not any(on_host(i) for i in range(len(paths))):   # FASTA only: the device indexes it
        return HostBatch(data, off, None, list(names) if names else list(paths))
    if not index and all(is_fastq(i) or sizes[i] == 0 for i in range(len(paths))):   # FASTQ only: likewise
        return HostBatch(data, off, None, list(names) if names else list(paths), fastq=True)
    if pool is not None:
        excl = list(pool.map(host_index, range(len(paths))))
    elif threads > 1 and len(paths) > 1:
        with ThreadPoolExecutor(max_workers=min(threads, len(paths))) as ex:
            excl = list(ex.map(host_index, range(len(paths))))
    else:
        excl = [host_index(i) for i in range(len(paths))]
    if not index and all(e is None for e in excl):
        return HostBatch(data, off, None, list(names) if names else list(paths))
    excl = [e if e is not None else index_records(d[int(off[i]): int(off[i]) + sizes[i]], N.KF_FMT_FASTA,
                                                  int(off[i]))[0] for i, e in enumerate(excl)]
    ex = np.concatenate(excl) if excl else np.zeros(0, np.uint64)
    return HostBatch(data, off, ex.astype(np.uint64), list(names) if names else list(paths))


def pack_ranges(ranges: Sequence[tuple[str, int, int]], names: Sequence[str] | None = None, pin: bool = True,
                threads: int = 8, chunk: int = 64 << 20, index: bool = False, buf: torch.Tensor | None = None,
                fastq: bool = False) -> HostBatch:
    """As pack_files for byte ranges [(path, start, end)] of files (the pieces of
    a file too large for one sparse call, main.fasta_pieces, get_chunks'
    record-aligned parts, main.record_pieces, or get_frequencies' pieces of a
    file above its split limit), read by os.preadv in chunks of `chunk` bytes on
    `threads` threads.  FASTA (index=False: the record index is left to the
    device; index=True: the header lines indexed here) unless `fastq`: then every
    range is FASTQ that starts at a record start (main.fastq_pieces) and the
    device indexes it (excl None and fastq set: kf_index_fastq).
    `buf`: a caller-owned (pinned) buffer to read into, as pack_files takes."""
    from concurrent.futures import ThreadPoolExecutor
    sizes = [e - a for _, a, e in ranges]
    off = _layout(sizes)
    if buf is not None and buf.numel() >= max(int(off[-1]), ALIGN):
        data = buf[: max(int(off[-1]), ALIGN)]
    else:
        data = _alloc_host(int(off[-1]), pin)
    d = data.numpy()
    for i, sz in enumerate(sizes):                # '\n' padding is transparent
        d[int(off[i]) + sz: int(off[i + 1])] = 10
    jobs = []
    for i, (p, a, e) in enumerate(ranges):
        for x in range(a, e, chunk):
            jobs.append((p, x, min(e, x + chunk), int(off[i]) + x - a))

    def read(job):
        p, x, y, dst = job
        fd = os.open(p, os.O_RDONLY)
        try:
            got = 0
            mv = memoryview(d[dst: dst + (y - x)])
            while got < y - x:
                r = os.preadv(fd, [mv[got:]], x + got)
                if r <= 0:
                    raise N.NativeError(f"short read on {p}")
                got += r
        finally:
            os.close(fd)

    with ThreadPoolExecutor(max_workers=max(1, int(threads))) as ex:
        list(ex.map(read, jobs))
        excl = None
        if index and not fastq:
            parts = list(ex.map(lambda i: index_records(d[int(off[i]): int(off[i]) + sizes[i]], N.KF_FMT_FASTA,
                                                        int(off[i]))[0], range(len(ranges))))
            excl = (np.concatenate(parts) if parts else np.zeros(0, np.uint64)).astype(np.uint64)
    return HostBatch(data, off, excl, list(names) if names else [f"{p}:{a}" for p, a, _ in ranges], fastq=fastq)


@dataclasses.dataclass
class DeviceBatch:
    data: torch.Tensor      # uint8 on device (16-byte aligned)
    off: torch.Tensor       # int64 [n+1]
    excl: torch.Tensor      # int64 [2m]
    n: int
    n_excl: int
    irregular: tuple = ()   # to_device(fallback=False): the genomes of a FASTQ batch that kf_index_fastq found
                            # not regular (their part of excl is not to be used: the caller refuses the batch)


def index_on_device(data: torch.Tensor, off: torch.Tensor, n: int, nbytes: int) -> tuple[torch.Tensor, int]:
    """FASTA header lines of a device batch (kf_index_fasta) on the current
    stream: (pairs int64[2m] on the device, m).  Reads m back (one small
    synchronising copy); a table that was too small is grown and the index run
    again, so the result is always complete."""
    dev = data.device
    s = _stream_ptr(dev)
    nb = (nbytes + 4095) // 4096
    scratch = torch.empty(nb + 1, dtype=torch.int32, device=dev)
    npairs = torch.zeros(1, dtype=torch.int64, device=dev)
    # 64 header lines per genome to start (draft assemblies with more contigs
    # re-run once with the exact count; ADVICE r04: a bytes-proportional first
    # guess allocated ~25 % of the batch)
    cap = 64 * n + 4096
    while True:
        excl = torch.empty(max(2 * cap, 2), dtype=torch.int64, device=dev)
        N.check(N.lib().kf_index_fasta(data.data_ptr(), off.data_ptr(), n, nbytes, excl.data_ptr(), cap,
                                       npairs.data_ptr(), scratch.data_ptr(), nb + 1, s), "kf_index_fasta")
        m = int(npairs.item())
        if m <= cap:
            return excl[: 2 * m], m
        cap = m


def index_fastq_on_device(data: torch.Tensor, off: torch.Tensor, n: int, nbytes: int, status_out: list | None = None
                          ) -> tuple[torch.Tensor, int, bool]:
    """FASTQ records of a device batch (kf_index_fastq) on the current stream:
    (pairs int64[2m] on the device, m, whether every genome is in the regular
    four-line form -- if not, the pairs are not to be used).  One small
    synchronising copy reads the two counts and the genomes' status words back;
    tables that were too small are grown and the index run again.  status_out: a
    list that receives the genomes' status words (uint32[n])."""
    dev = data.device
    s = _stream_ptr(dev)
    L = N.lib()
    # reads of 100 bases or more have a '\n' per ~55 bytes and a pair per ~220
    cap_lines = nbytes // 32 + 4 * n + 4096
    cap_pairs = nbytes // 128 + 2 * n + 4096
    info = torch.empty(2 + (n + 1) // 2, dtype=torch.int64, device=dev)   # d_n[2], then the status words
    while True:
        need = int(L.kf_index_fastq_scratch_bytes(nbytes, n, cap_lines))
        scratch = torch.empty(max(need // 8, 1), dtype=torch.int64, device=dev)
        excl = torch.empty(max(2 * cap_pairs, 2), dtype=torch.int64, device=dev)
        N.check(L.kf_index_fastq(data.data_ptr(), off.data_ptr(), n, nbytes, excl.data_ptr(), cap_pairs, cap_lines,
                                 info.data_ptr(), info.data_ptr() + 16, scratch.data_ptr(), need, s), "kf_index_fastq")
        h = info.cpu().numpy()
        m, lines = int(h[0]), int(h[1])
        if lines > cap_lines:   # the pairs were not counted: allow for as many as these lines can make
            cap_lines, cap_pairs = lines, max(cap_pairs, lines // 4 + 2 * n + 1)
            continue
        if m > cap_pairs:
            cap_pairs = m
            continue
        status = h[2:].view(np.uint32)[:n]
        if (status == 2).any():
            raise N.NativeError("kf_index_fastq: genome offsets must be non-decreasing and end at or below the batch")
        if status_out is not None:
            status_out.append(status.copy())
        return excl[: 2 * m], m, not status.any()


# which record index each batch without a host index took in to_device
INDEX_PATHS = {"fasta_device": 0, "fastq_device": 0, "fastq_host_fallback": 0}


def to_device(hb: HostBatch, device: torch.device | str = "cuda", fallback: bool = True) -> DeviceBatch:
    """Asynchronous H2D of a batch on the current stream.  The small offset and
    interval tables are staged through pinned memory too: a copy from pageable
    memory would block the host until the stream's earlier copies finish.  A
    batch packed without its record index (excl None) is indexed on the device
    (index_on_device, or index_fastq_on_device for a FASTQ batch: one small
    synchronising copy).  A FASTQ batch with a genome that is not in the regular
    four-line form is copied back and indexed by the host instead -- unless
    fallback=False (the pieces of a file cut by main.fastq_pieces: a piece that
    is not regular was cut at a wrong line, which the host index would read as
    if it were a record start): then the batch comes back with those genomes
    named in DeviceBatch.irregular, for the caller to refuse."""
    dev = torch.device(device)
    if hb.dev_data is not None:   # copied already (get_frequencies' readers, on a copy stream)
        cur = torch.cuda.current_stream(dev)
        if hb.dev_event is not None:
            cur.wait_event(hb.dev_event)
        data = hb.dev_data
        data.record_stream(cur)
    else:
        data = hb.data.to(dev, non_blocking=True)
    if hb.excl is None:
        pin = hb.data is None or hb.data.is_pinned()
        off = torch.from_numpy(hb.off.view(np.int64))
        off = (off.pin_memory() if pin else off).to(dev, non_blocking=pin)
        nbytes = int(hb.off[-1])
        with torch.cuda.device(dev):
            if not hb.fastq:
                excl, m = index_on_device(data, off, hb.n, nbytes)
                INDEX_PATHS["fasta_device"] += 1
            else:
                st: list = []
                excl, m, regular = index_fastq_on_device(data, off, hb.n, nbytes, st)
                INDEX_PATHS["fastq_device" if regular or not fallback else "fastq_host_fallback"] += 1
                if not regular and not fallback:
                    return DeviceBatch(data, off, excl if m else torch.zeros(2, dtype=torch.int64, device=dev), hb.n, m,
                                       tuple(int(g) for g in np.flatnonzero(st[0])))
                if not regular:
                    # from the device copy: the reader may be refilling hb.data (a pinned slot) already
                    d = data[:nbytes].cpu().numpy()
                    iv = np.concatenate([index_records(d[int(hb.off[i]): int(hb.off[i + 1])], N.KF_FMT_FASTQ,
                                                       int(hb.off[i]))[0] for i in range(hb.n)])
                    m = iv.size // 2
                    excl = torch.from_numpy(iv.view(np.int64)).to(dev)
        return DeviceBatch(data, off, excl if m else torch.zeros(2, dtype=torch.int64, device=dev), hb.n, m)
    ex = hb.excl if hb.excl.size else np.zeros(2, np.uint64)
    pin = hb.data is None or hb.data.is_pinned()
    n_off = (hb.off.size + 1) & ~1   # the interval table starts 16-byte aligned
    host = np.zeros(n_off + ex.size, np.int64)
    host[: hb.off.size] = hb.off.view(np.int64)
    host[n_off:] = ex.view(np.int64)
    small = torch.from_numpy(host)
    if pin:
        small = small.pin_memory()
    small = small.to(dev, non_blocking=pin)
    off, excl = small[: hb.off.size], small[n_off:]
    return DeviceBatch(data, off, excl, hb.n, hb.excl.size // 2)


def _stream_ptr(device: torch.device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def accumulate_rows(src: torch.Tensor, src_totals: torch.Tensor, seg: torch.Tensor, dst: torch.Tensor,
                    dst_totals: torch.Tensor, status: torch.Tensor, accumulate: bool = False,
                    stream: int | None = None) -> None:
    """Enqueue kf_rows_accumulate: dst[r] (int32[n_dst, nbins] holding uint32 bit
    patterns, as KmerCounter.count gives) receives the column-wise sum of the rows
    src[seg[r]: seg[r + 1]] (seg int32[n_dst + 1] on the device), dst_totals[r]
    the sum of their totals, added to what they hold if `accumulate`.  status
    (int32[n_dst]) bit 0: a column passed 2^32 - 1 and holds UINT32_MAX; 2: the
    segment table is bad and nothing was written.  The caller reads status back
    before it uses the rows."""
    assert src.dtype == torch.int32 and dst.dtype == torch.int32 and src.is_contiguous() and dst.is_contiguous()
    assert src.dim() == 2 and dst.dim() == 2 and src.shape[1] == dst.shape[1]
    assert src_totals.dtype == torch.int64 and src_totals.shape == (src.shape[0],) and src_totals.is_contiguous()
    assert dst_totals.dtype == torch.int64 and dst_totals.shape == (dst.shape[0],) and dst_totals.is_contiguous()
    assert seg.dtype == torch.int32 and seg.shape == (dst.shape[0] + 1,) and seg.is_contiguous()
    assert status.dtype == torch.int32 and status.shape == (dst.shape[0],) and status.is_contiguous()
    s = _stream_ptr(dst.device) if stream is None else stream
    with torch.cuda.device(dst.device):
        N.check(N.lib().kf_rows_accumulate(src.data_ptr(), src_totals.data_ptr(), src.shape[0], seg.data_ptr(),
                                           dst.shape[0], dst.shape[1], dst.data_ptr(), dst_totals.data_ptr(),
                                           status.data_ptr(), N.KF_ACCUMULATE if accumulate else 0, s),
                "kf_rows_accumulate")


_DEV_TABLES: dict = {}   # (k, device index) -> (code2col, col2rep) on the device


class KmerCounter:
    """Canonical k-mer counter for one k on one device (the ``jellyfish count -C
    -m k`` + ``dump -c`` + vocab merge of main.py:309-328)."""

    def __init__(self, k: int, device: torch.device | str = "cuda"):
        if not (N.KF_MIN_K <= k <= N.KF_MAX_K):
            raise ValueError(f"k={k} out of range [{N.KF_MIN_K}, {N.KF_MAX_K}]")
        self.k = k
        self.device = torch.device(device)
        if self.device.type != "cuda" or not torch.cuda.is_available():
            raise N.NativeError("KmerCounter needs a ROCm GPU (no CPU fallback)")
        self.nbins = num_bins(k)
        key = (k, self.device.index if self.device.index is not None else torch.cuda.current_device())
        if key not in _DEV_TABLES:   # immutable: one upload per (k, device) and process
            c2c, c2r = tables(k)
            _DEV_TABLES[key] = (torch.from_numpy(c2c.view(np.int32)).to(self.device),
                                torch.from_numpy(c2r.view(np.int32)).to(self.device))
        self.code2col, self.col2rep = _DEV_TABLES[key]

    def launch_info(self) -> tuple[int, int, int]:
        g, b, l = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        with torch.cuda.device(self.device):
            N.check(N.lib().kf_count_launch_info(self.k, ctypes.byref(g), ctypes.byref(b), ctypes.byref(l)),
                    "kf_count_launch_info")
        return g.value, b.value, l.value

    def reserve(self, max_genomes: int) -> None:
        """Allocate the library's workspace for batches of up to max_genomes now
        (kf_workspace_reserve), so that count() never allocates or synchronises."""
        with torch.cuda.device(self.device):
            N.check(N.lib().kf_workspace_reserve(self.k, int(max_genomes)), "kf_workspace_reserve")

    def alloc_out(self, n: int) -> tuple[torch.Tensor, torch.Tensor]:
        return (torch.empty((n, self.nbins), dtype=torch.int32, device=self.device),
                torch.empty(n, dtype=torch.int64, device=self.device))

    def count(self, db: DeviceBatch, counts: torch.Tensor | None = None, totals: torch.Tensor | None = None,
              accumulate: bool = False, stream: int | None = None) -> tuple[torch.Tensor, torch.Tensor]:
        """Enqueue the count kernel; returns (counts int32[n, nbins] holding uint32
        bit patterns, totals int64[n]) on the device."""
        if counts is None or totals is None:
            counts, totals = self.alloc_out(db.n)
        assert counts.shape == (db.n, self.nbins) and counts.dtype == torch.int32 and counts.is_contiguous()
        assert totals.shape == (db.n,) and totals.dtype == torch.int64
        assert db.data.data_ptr() % 16 == 0
        s = _stream_ptr(self.device) if stream is None else stream
        with torch.cuda.device(self.device):
            N.check(N.lib().kf_count_batch(
                db.data.data_ptr(), db.off.data_ptr(), db.n, db.excl.data_ptr() if db.n_excl else None,
                db.n_excl, self.code2col.data_ptr(), self.col2rep.data_ptr(), self.k,
                counts.data_ptr(), totals.data_ptr(), N.KF_ACCUMULATE if accumulate else 0, s), "kf_count_batch")
        return counts, totals


class SparseCounter:
    """Present canonical k-mers at any k = 2..31 (``kf_sparse_count``): what
    get_kmers reads from ``jellyfish count -C -m k`` + ``dump -c -t``
    (main.py:133-160) -- per genome, the distinct canonical k-mers as standard
    2-bit codes (A0 C1 G2 T3, first base most significant; ascending = the
    lexicographic order of the vocab files) and their counts."""

    def __init__(self, k: int, device: torch.device | str = "cuda"):
        if not (N.KF_MIN_K <= k <= N.KF_SPARSE_MAX_K):
            raise ValueError(f"k={k} out of range [{N.KF_MIN_K}, {N.KF_SPARSE_MAX_K}]")
        self.k = k
        self.device = torch.device(device)
        if self.device.type != "cuda" or not torch.cuda.is_available():
            raise N.NativeError("SparseCounter needs a ROCm GPU (no CPU fallback)")
        self._work = None

    def workspace_bytes(self, batch_bytes: int, n: int) -> int:
        return int(N.lib().kf_sparse_workspace_bytes(self.k, int(batch_bytes), int(n)))

    def count(self, db: DeviceBatch, batch_bytes: int):
        """Enqueue the sparse count of a batch whose genomes end at batch_bytes
        (= off[n]) on the current stream (the outputs and the reused workspace
        belong to that stream's allocator pool, so there is no stream argument);
        returns (keys int64[batch_bytes] holding uint64 codes, counts
        int32[batch_bytes] holding uint32, nuniq int64[n]) on the device: genome
        g's k-mers are keys[off[g] : off[g] + nuniq[g]]."""
        batch_bytes = int(batch_bytes)
        need = self.workspace_bytes(batch_bytes, db.n)
        if self._work is None or self._work.numel() < need:
            self._work = None
            self._work = torch.empty(max(need, 256), dtype=torch.uint8, device=self.device)
        keys = torch.empty(max(batch_bytes, 1), dtype=torch.int64, device=self.device)
        counts = torch.empty(max(batch_bytes, 1), dtype=torch.int32, device=self.device)
        nuniq = torch.zeros(max(db.n, 1), dtype=torch.int64, device=self.device)
        s = _stream_ptr(self.device)
        with torch.cuda.device(self.device):
            N.check(N.lib().kf_sparse_count(
                db.data.data_ptr(), db.off.data_ptr(), db.n, batch_bytes,
                db.excl.data_ptr() if db.n_excl else None, db.n_excl, self.k,
                self._work.data_ptr(), self._work.numel(), keys.data_ptr(), counts.data_ptr(),
                nuniq.data_ptr(), s), "kf_sparse_count")
        return keys, counts, nuniq[: db.n]

    @staticmethod
    def nuniq_to_host(nuniq: torch.Tensor) -> np.ndarray:
        """count()'s nuniq on the host (int64[n]); raises the library's error if
        the device refused the offsets or its order check failed."""
        nu = nuniq.cpu().numpy()
        if nu.size and (nu == -1).any():   # UINT64_MAX: the library refused the offsets
            raise N.NativeError("kf_sparse_count: genome offsets must be non-decreasing and end at or below "
                                "batch_bytes (nothing was counted)")
        if nu.size and (nu == -2).any():   # UINT64_MAX - 1: the device's order check failed
            raise N.NativeError("kf_sparse_count: the sorted keys failed the device's order check")
        return nu

    def to_host(self, keys: torch.Tensor, counts: torch.Tensor, nuniq: torch.Tensor,
                off: np.ndarray) -> list[tuple[np.ndarray, np.ndarray]]:
        """Per genome (keys uint64[m], counts uint32[m]) on the host: each genome's
        slice is gathered on the device and the batch copied back once."""
        nu = self.nuniq_to_host(nuniq)
        if nu.size == 0 or int(nu.sum()) == 0:
            return [(np.zeros(0, np.uint64), np.zeros(0, np.uint32)) for _ in range(nu.size)]
        idx = torch.cat([torch.arange(int(off[g]), int(off[g]) + int(nu[g]), device=keys.device)
                         for g in range(nu.size)])
        hk = keys[idx].cpu().numpy().view(np.uint64)
        hc = counts[idx].cpu().numpy().view(np.uint32)
        out, pos = [], 0
        for g in range(nu.size):
            m = int(nu[g])
            out.append((hk[pos: pos + m], hc[pos: pos + m]))
            pos += m
        return out


def merge_tile() -> int:
    """Merged positions per workgroup tile of kf_sparse_merge (a multiple of 64)."""
    return int(N.lib().kf_sparse_merge_tile())


def merge_scratch_bytes(n_a: int, n_b: int) -> int:
    return int(N.lib().kf_sparse_merge_scratch_bytes(int(n_a), int(n_b)))


def merge_sorted(keys_a: torch.Tensor, counts_a: torch.Tensor, keys_b: torch.Tensor, counts_b: torch.Tensor,
                 stream: int | None = None):
    """Enqueue kf_sparse_merge: the ascending union of two lists of (key, count)
    on the device, equal keys' counts summed -- how a piece of a large file joins
    its file's running result (main._merge_sorted_counts states what it computes).
    keys_a / keys_b: contiguous int64 holding uint64 codes, each strictly ascending
    in unsigned order (a genome's slice of SparseCounter.count); counts: int32
    holding uint32, or int64, per side.  Returns (keys int64[n_a + n_b], counts
    int64[n_a + n_b], n_out int64[1], status int32[1]) on the device: the first
    n_out entries are the result, status is 1 (and n_out 0) if an input was not
    strictly ascending.  The outputs and the scratch (16 B per tile) are allocated
    here, on the current stream's pool; merged_to_host reads n_out and status."""
    for k_, c_ in ((keys_a, counts_a), (keys_b, counts_b)):
        assert k_.dtype == torch.int64 and k_.dim() == 1 and k_.is_contiguous()
        assert c_.dtype in (torch.int32, torch.int64) and c_.shape == k_.shape and c_.is_contiguous()
        assert k_.device == keys_a.device and c_.device == keys_a.device
    dev = keys_a.device
    n_a, n_b = keys_a.numel(), keys_b.numel()
    keys = torch.empty(max(n_a + n_b, 1), dtype=torch.int64, device=dev)
    counts = torch.empty(max(n_a + n_b, 1), dtype=torch.int64, device=dev)
    n_out = torch.empty(1, dtype=torch.int64, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    need = merge_scratch_bytes(n_a, n_b)   # 0 above the library's limit: the call below says so
    scratch = torch.empty(max(need // 8, 1), dtype=torch.int64, device=dev)
    s = _stream_ptr(dev) if stream is None else stream
    with torch.cuda.device(dev):
        N.check(N.lib().kf_sparse_merge(
            keys_a.data_ptr() if n_a else None, counts_a.data_ptr() if n_a else None,
            4 if counts_a.dtype == torch.int32 else 8, n_a,
            keys_b.data_ptr() if n_b else None, counts_b.data_ptr() if n_b else None,
            4 if counts_b.dtype == torch.int32 else 8, n_b,
            keys.data_ptr(), counts.data_ptr(), n_out.data_ptr(), status.data_ptr(), scratch.data_ptr(),
            8 * scratch.numel(), s), "kf_sparse_merge")
    return keys[: n_a + n_b], counts[: n_a + n_b], n_out, status


def merged_to_host(n_out: torch.Tensor, status: torch.Tensor) -> int:
    """merge_sorted's number of entries on the host (one copy for both words);
    raises the library's error if the device's order check failed."""
    n, st = torch.cat([n_out, status.to(torch.int64)]).cpu().tolist()
    if st != 0:
        raise N.NativeError("kf_sparse_merge: an input list is not strictly ascending (nothing was merged)")
    return int(n)


def counts_to_numpy(counts: torch.Tensor) -> np.ndarray:
    return counts.cpu().numpy().view(np.uint32)


def features(counts: torch.Tensor, pseudocount: bool = False, raw_cnt: bool = False,
             scaler: float = 1.0) -> torch.Tensor:
    """In-memory hand-off: the float64 feature matrix the
    trainers build from `.kf` files -- `my_read_csv` (utils.py:436-437) then
    `* features_scaler` (train_classifier_model.py:148, train_model_set.py:291) --
    computed on the device from the count matrix, without the text round trip.

    The values are main.py:332-342 (`+0.5` pseudocount, `v / v.sum()` unless raw)
    in float64: the row sums are exact (integers or halves below 2^53) and each
    quotient is correctly rounded, so they equal the numbers the `.kf` text holds
    (`repr` round-trips float64; `pd.read_csv(..., float_precision="round_trip")`
    reads them back bit for bit).  pandas' default parser, which my_read_csv
    uses, is not correctly rounded: about half the entries of a k=7 row read
    differently, by at most ~1e-12 relative (8.7e-13 measured on the toy genomes).  An empty
    genome gives NaN rows (normalised) as the reference's "nan" strings parse.
    """
    c = counts.to(torch.int64)
    c = torch.where(c < 0, c + (1 << 32), c)          # uint32 bit patterns held in int32
    v = c.to(torch.float64)
    if pseudocount:
        v = v + 0.5
    if not raw_cnt:
        v = v / v.sum(dim=1, keepdim=True)
    return v * scaler if scaler != 1.0 else v


def chunk_features(counts: torch.Tensor, lo, n, scaler: float = 1.0, cap: int | None = None,
                   dtype: torch.dtype = torch.float32, out: torch.Tensor | None = None,
                   stream: int | None = None, check: bool = True):
    """In-memory hand-off of get_chunks to the chunk trainer (kf_chunk_features):
    [S, nbins] of `dtype` (float32 or float64), row s the column-wise sum of the
    window rows counts[lo[s]: lo[s] + n[s]] (each count as min(count, cap) if
    `cap` is given), divided by its grand total, times `scaler` -- what
    Dataset_chunks_2rows computes per view (kf2vec/datasets.py:47-62), in float64
    and rounded to float32 last; a sample with a zero total is a row of zeros.
    chunks.range_features_host states it in numpy, bit for bit.

    counts: contiguous [n_rows, nbins] on the device, int16 holding uint16 bit
    patterns (ChunkStore.counts) or int32 holding uint32 (KmerCounter.count); or
    uint8, the rows of a store that was capped at 255 as it was read
    (chunks.chunk_store_from_kf(cap8=True), rows_cap8), which go through
    kf_chunk_features8: `cap` must then be None or at least 255 (a ValueError
    otherwise), and the result is this function's with cap=255 on the uint16
    rows the store was made from, bit for bit.
    lo, n: host arrays (one staged pinned copy), or int64 tensors on the device.
    The device checks the table; its status word is read back here (the call's
    one synchronisation) and a sample outside [0, n_rows] raises N.NativeError
    with `out` untouched.  check=False (lo and n on the device): nothing waits,
    and (out, status) come back, status the int32 [1] word on the device, not
    zero where a sample lay outside -- the caller reads it with its own next
    read (the chunk trainer: once per epoch)."""
    assert counts.dtype in (torch.uint8, torch.int16, torch.int32) and counts.dim() == 2 and counts.is_contiguous()
    assert dtype in (torch.float32, torch.float64)
    rows8 = counts.dtype == torch.uint8
    if rows8 and cap is not None and int(cap) < 255:
        raise ValueError("chunk_features: cap={} with uint8 rows, which are capped at 255 already: a lower cap needs "
                         "the uint16 rows".format(cap))
    dev = counts.device
    if isinstance(lo, torch.Tensor) and lo.is_cuda:
        assert isinstance(n, torch.Tensor) and n.device == lo.device == dev and lo.shape == n.shape
        assert lo.dtype == n.dtype == torch.int64 and lo.is_contiguous() and n.is_contiguous()
        d_lo, d_n = lo, n
    else:
        def as_i64(x):   # uint64 keeps its bit pattern
            x = np.asarray(x.cpu() if isinstance(x, torch.Tensor) else x)
            return x.view(np.int64) if x.dtype == np.uint64 else x.astype(np.int64)
        t = torch.from_numpy(np.stack([as_i64(lo).reshape(-1), as_i64(n).reshape(-1)]))
        d_lo, d_n = (t.pin_memory() if t.numel() else t).to(dev, non_blocking=True)
    ns, nbins = d_lo.numel(), counts.shape[1]
    if out is None:
        out = torch.empty((ns, nbins), dtype=dtype, device=dev)
    assert out.dtype == dtype and out.shape == (ns, nbins) and out.is_contiguous() and out.device == dev
    if ns == 0:
        return out if check else (out, torch.zeros(1, dtype=torch.int32, device=dev))
    status = torch.empty(1, dtype=torch.int32, device=dev)
    need = int(N.lib().kf_chunk_features_scratch_bytes(ns))
    work = torch.empty(need // 8, dtype=torch.int64, device=dev)
    s = _stream_ptr(dev) if stream is None else stream
    with torch.cuda.device(dev):
        if rows8:
            N.check(N.lib().kf_chunk_features8(
                counts.data_ptr() if counts.shape[0] else None, counts.shape[0], nbins, d_lo.data_ptr(), d_n.data_ptr(),
                ns, float(scaler), out.data_ptr(), out.element_size(), status.data_ptr(), work.data_ptr(), need, s),
                "kf_chunk_features8")
        else:
            N.check(N.lib().kf_chunk_features(
                counts.data_ptr() if counts.shape[0] else None, counts.element_size(), counts.shape[0], nbins,
                d_lo.data_ptr(), d_n.data_ptr(), ns, 0xFFFFFFFF if cap is None else int(cap), float(scaler),
                out.data_ptr(), out.element_size(), status.data_ptr(), work.data_ptr(), need, s), "kf_chunk_features")
    if not check:
        if stream is not None:   # the work table is the caller's stream's until the call is done
            work.record_stream(torch.cuda.ExternalStream(stream, device=dev))
        return out, status
    if stream is not None:   # the read-back below is ordered on torch's current stream only
        torch.cuda.synchronize(dev)
    if int(status.item()) != 0:
        raise N.NativeError("kf_chunk_features: a sample's rows lie outside the count matrix (nothing was written)")
    return out


def rows_cap8(rows: torch.Tensor, out: torch.Tensor | None = None, stream: int | None = None) -> torch.Tensor:
    """Enqueue kf_rows_cap8: the uint8 tensor min(rows, 255) of `rows`' shape for
    int16 rows holding uint16 bit patterns (torch has no unsigned 16-bit clamp),
    contiguous and on the device -- what utils.my_read_csv_chunk_capped keeps of
    a count.  `out`: a contiguous uint8 tensor of that many elements to write
    to.  Nothing waits."""
    assert rows.dtype == torch.int16 and rows.is_contiguous()
    if out is None:
        out = torch.empty(rows.shape, dtype=torch.uint8, device=rows.device)
    assert out.dtype == torch.uint8 and out.numel() == rows.numel() and out.is_contiguous()
    assert out.device == rows.device
    n = rows.numel()
    if n:
        s = _stream_ptr(rows.device) if stream is None else stream
        with torch.cuda.device(rows.device):
            N.check(N.lib().kf_rows_cap8(rows.data_ptr(), n, out.data_ptr(), s), "kf_rows_cap8")
    return out


# ---------------------------------------------------------------------------
# get_chunks .kf text parsed on the device (kf_parse_kf_rows)
# ---------------------------------------------------------------------------
KF_PARSE_ERRORS = {1: "too few fields", 2: "too many fields", 3: "malformed field", 4: "value above 65535",
                   5: "more rows than the caller allowed for",
                   # kf_parse_kf_floats' (features.parse_kf_floats), which has no code 4
                   6: "more than 19 significant digits", 7: "magnitude outside the normal float64 range"}


def parse_kf_rows(data: torch.Tensor, off, nbins: int, cap_rows: int | None = None, stream: int | None = None):
    """Enqueue kf_parse_kf_rows: the get_chunks `.kf` text of a batch of units
    (files, or pieces cut at line starts: chunks.kf_line_pieces) parsed into
    uint16 window rows on the device, as my_read_csv_chunk leaves them
    (kf2vec/utils.py:402-405).  chunks.parse_kf_rows_host states what it computes.

    data: uint8 on the device, 16-byte aligned, the units back to back as
    pack_ranges lays them out; off: the units' offsets [n + 1] (host array, or an
    int64 tensor on the device); unit u is data[off[u]: off[u + 1]].
    cap_rows: rows allowed for; by default (batch_bytes + n) // (2 * nbins + 1),
    which no batch can exceed: a row is at least nbins times ',' and a digit, and
    its '\n' unless it is its unit's last, so the rows stay below the batch's
    own size (2 * nbins bytes of row for 2 * nbins + 1 of text).
    Returns (rows int16 [cap_rows, nbins] holding uint16 bit patterns, unit_row0
    int64 [n + 1], status int64 [4]) on the device: unit u's rows are
    rows[unit_row0[u]: unit_row0[u + 1]]; parsed_to_host brings unit_row0 to the
    host and raises what status says.  Outputs and scratch are allocated here."""
    assert data.dtype == torch.uint8 and data.dim() == 1 and data.is_contiguous()
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
    rows = torch.empty((cap_rows, nbins), dtype=torch.int16, device=dev)
    unit_row0 = torch.empty(n + 1, dtype=torch.int64, device=dev)
    status = torch.empty(4, dtype=torch.int64, device=dev)
    need = int(N.lib().kf_parse_kf_scratch_bytes(nbytes, n, cap_rows))
    scratch = torch.empty(need // 8 + 1, dtype=torch.int64, device=dev)
    one = torch.empty(8, dtype=torch.int16, device=dev)   # an address for the rows of a call that allows for none
    s = _stream_ptr(dev) if stream is None else stream
    with torch.cuda.device(dev):
        N.check(N.lib().kf_parse_kf_rows(
            data.data_ptr(), d_off.data_ptr(), n, nbytes, nbins, cap_rows,
            rows.data_ptr() if rows.numel() else one.data_ptr(), unit_row0.data_ptr(), status.data_ptr(),
            scratch.data_ptr(), 8 * scratch.numel(), s), "kf_parse_kf_rows")
    return rows, unit_row0, status


def parsed_to_host(unit_row0: torch.Tensor, status: torch.Tensor, names: Sequence[str] | None = None,
                   row_base: Sequence[int] | None = None, first_unit: Sequence[int] | None = None,
                   what: str = "kf_parse_kf_rows") -> np.ndarray:
    """parse_kf_rows' unit_row0 on the host (one copy for both tensors); raises
    ValueError if the device refused the text, naming the unit's file (names[u],
    else "unit u"), the row and the column, both counted from 0.  The row is
    counted within the file when the caller says where the file began: unit
    first_unit[u] is the first of this batch that belongs to u's file, and
    row_base[u] rows of that file lie in batches before this one.  `what` names
    the call whose status this is (features.parse_kf_floats passes its own)."""
    both = torch.cat([status, unit_row0]).cpu().numpy()
    code, unit, row, col = (int(x) for x in both[:4])
    row0 = both[4:].copy()
    if code != 0:
        who = names[unit] if names is not None else "unit {}".format(unit)
        if first_unit is not None:
            row += int(row0[unit] - row0[first_unit[unit]])
        if row_base is not None:
            row += int(row_base[unit])
        raise ValueError("{}: row {}, column {}: {} ({} status {})".format(
            who, row, col, KF_PARSE_ERRORS.get(code, "unknown error"), what, code))
    return row0


# ---------------------------------------------------------------------------
# get_chunks `.kf` text formatted on the device (kf_format_kf_rows16)
# ---------------------------------------------------------------------------
KF_FORMAT_ERRORS = {1: "the text is longer than the buffer allowed for",
                    2: "a row's prefix is out of range, or the prefix offsets decrease"}
KF_FORMAT_MAX_CAP = (1 << 32) - 1   # bytes of text per call (32-bit offsets inside a call)


def format_kf_row_bound(nbins: int, max_prefix_len: int, win_len: int) -> int:
    """Bytes that no line of format_kf_rows exceeds: the name (prefix, two uint64
    in decimal and '-' if win_len), its ',' and 8 bytes per column ("65535.0,")."""
    return int(max_prefix_len) + (41 if win_len else 0) + 1 + 8 * int(nbins)


def format_kf_rows(counts16: torch.Tensor, prefixes, row_prefix, row_start, win_len: int, pseudocount: bool,
                   stream: int | None = None, cap_bytes: int | None = None):
    """Enqueue kf_format_kf_rows16: the uint16 window rows counts16 (int16 or
    uint16 bit patterns, [n, nbins], on the device) as the `.kf` lines that
    kf_write_kf_segments16 writes for raw counts, back to back.
    chunks.format_rows_host states what it computes.

    prefixes: the name prefixes (bytes, or str encoded as the writer encodes
    them); row r is named prefixes[row_prefix[r]] followed by "<s+1>-<s+win_len>"
    for s = row_start[r], or by nothing if win_len == 0.  row_prefix (uint32) and
    row_start (uint64) are host arrays or tensors on the device.
    cap_bytes: the size of the text buffer; by default n times
    format_kf_row_bound, which no text exceeds (it must stay below 2^32: cut the
    rows into calls).
    Returns (text uint8 [cap_bytes], row_off int64 [n + 1], status int64 [4]) on
    the device: row r's line is text[row_off[r]: row_off[r + 1]]; formatted_to_host
    brings row_off to the host and raises what status says."""
    assert counts16.dim() == 2 and counts16.is_contiguous() and counts16.element_size() == 2
    dev = counts16.device
    n, nbins = int(counts16.shape[0]), int(counts16.shape[1])
    enc = [x if isinstance(x, (bytes, bytearray)) else x.encode(errors="surrogateescape") for x in prefixes]
    pre_off = np.zeros(len(enc) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in enc], out=pre_off[1:])
    blob = np.frombuffer(b"".join(enc) + b"\0", dtype=np.uint8)   # never empty: an address for no prefix bytes
    d_pre = torch.from_numpy(blob.copy()).to(dev, non_blocking=True)
    d_pre_off = torch.from_numpy(pre_off).to(dev, non_blocking=True)

    def table(x, np_t, t_t):
        if isinstance(x, torch.Tensor) and x.is_cuda:
            assert x.dtype == t_t and x.is_contiguous() and x.device == dev and x.numel() == n
            return x
        h = np.ascontiguousarray(np.asarray(x.cpu() if isinstance(x, torch.Tensor) else x), dtype=np_t)
        assert h.size == n
        return torch.from_numpy(h.view(np.dtype(np_t).str.replace("u", "i"))).to(dev, non_blocking=True)

    d_rpre = table(row_prefix, np.uint32, torch.int32)
    d_rpos = table(row_start, np.uint64, torch.int64)
    if cap_bytes is None:
        cap_bytes = n * format_kf_row_bound(nbins, max([len(x) for x in enc], default=0), win_len)
    cap_bytes = int(cap_bytes)
    text = torch.empty(max(cap_bytes, 1), dtype=torch.uint8, device=dev)
    row_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    status = torch.empty(4, dtype=torch.int64, device=dev)
    need = int(N.lib().kf_format_kf_scratch_bytes(n, nbins))
    scratch = torch.empty(need // 8 + 1, dtype=torch.int64, device=dev)
    s = _stream_ptr(dev) if stream is None else stream
    with torch.cuda.device(dev):
        N.check(N.lib().kf_format_kf_rows16(
            counts16.data_ptr(), n, nbins, d_pre.data_ptr(), d_pre_off.data_ptr(), len(enc), d_rpre.data_ptr(),
            d_rpos.data_ptr(), int(win_len), int(bool(pseudocount)), text.data_ptr(), cap_bytes, row_off.data_ptr(),
            status.data_ptr(), scratch.data_ptr(), 8 * scratch.numel(), s), "kf_format_kf_rows16")
    if stream is not None:   # the tables and the scratch are the caller's stream's until the call is done
        for t in (d_pre, d_pre_off, d_rpre, d_rpos, scratch):
            t.record_stream(torch.cuda.ExternalStream(stream, device=dev))
    return text[:cap_bytes], row_off, status


def format_status_check(code: int, need: int, row: int, cap_bytes: int | None = None) -> None:
    """Raise what kf_format_kf_rows16's status words say (nothing for code 0)."""
    if code == 1:
        raise N.NativeError("kf_format_kf_rows16: the text needs {} bytes{} (status 1)".format(
            need, "" if cap_bytes is None else ", {} allowed for".format(cap_bytes)))
    if code != 0:
        raise ValueError("row {}: {} (kf_format_kf_rows16 status {})".format(
            row, KF_FORMAT_ERRORS.get(code, "unknown error"), code))


def formatted_to_host(row_off: torch.Tensor, status: torch.Tensor, cap_bytes: int | None = None) -> np.ndarray:
    """format_kf_rows' row_off on the host (one copy for both tensors); raises
    NativeError if the text did not fit and ValueError, naming the row (counted
    from 0), if the device refused the prefix tables."""
    both = torch.cat([status, row_off]).cpu().numpy()
    format_status_check(int(both[0]), int(both[1]), int(both[2]), cap_bytes)
    return both[4:].copy()


# ---------------------------------------------------------------------------
# the get_kmers matrix on the device (kf_kmers_rows)
# ---------------------------------------------------------------------------
def kmers_tile_rows() -> int:
    """Slab rows per tile of the kf_kmers_rows kernel (a multiple of 4)."""
    return int(N.lib().kf_kmers_tile_rows())


@dataclasses.dataclass
class KmersTables:
    """kf_kmers_rows' segment tables on the device (one upload): segment s's
    k-mers are keys[src0[s] : src0[s] + n[s]], its first matrix row dst0[s]."""
    src0: torch.Tensor    # int64 [n_seg]
    n: torch.Tensor       # int64 [n_seg]
    dst0: torch.Tensor    # int64 [n_seg + 1]; dst0[n_seg] = the matrix's rows
    denom: torch.Tensor   # float32 [n_seg]
    n_seg: int
    rows: int


def kmers_tables(src0, n, dst0, denom, device: torch.device | str) -> KmersTables:
    """Upload the tables of a kf_kmers_rows call (host arrays: src0[n_seg],
    n[n_seg], dst0[n_seg + 1], denom[n_seg]) as one staged copy."""
    ns = len(n)
    dst0 = np.asarray(dst0, dtype=np.int64)
    assert len(src0) == ns and len(denom) == ns and dst0.size == ns + 1
    host = np.zeros(3 * ns + 1 + (ns + 1) // 2, dtype=np.int64)
    host[:ns] = np.asarray(src0, dtype=np.int64)
    host[ns: 2 * ns] = np.asarray(n, dtype=np.int64)
    host[2 * ns: 3 * ns + 1] = dst0
    host[3 * ns + 1:].view(np.float32)[:ns] = np.asarray(denom, dtype=np.float32)
    t = torch.from_numpy(host)
    if torch.cuda.is_available():
        t = t.pin_memory()
    t = t.to(torch.device(device), non_blocking=True)
    return KmersTables(t[:ns], t[ns: 2 * ns], t[2 * ns: 3 * ns + 1], t[3 * ns + 1:].view(torch.float32)[:ns], ns,
                       int(dst0[-1]))


def kmers_rows(keys: torch.Tensor, counts: torch.Tensor, tab: KmersTables, k: int, row_lo: int, row_hi: int,
               out: torch.Tensor, status: torch.Tensor, stream: int | None = None) -> None:
    """Enqueue kf_kmers_rows on the current stream: the rows [row_lo, row_hi) of
    the get_kmers matrix that `tab` lays out, float32 [row_hi - row_lo, k + 1],
    into `out` (element 0 = row row_lo, column 0).  keys int64 holding uint64
    standard codes; counts int32 holding uint32, or int64.  status (int32, one
    word): 2 if the device refused the tables (nothing written), else 0 -- the
    caller reads it back before it uses the rows."""
    assert keys.dtype == torch.int64 and keys.is_contiguous() and counts.is_contiguous()
    assert counts.dtype in (torch.int32, torch.int64)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() >= (row_hi - row_lo) * (k + 1)
    assert status.dtype == torch.int32 and status.numel() >= 1
    s = _stream_ptr(out.device) if stream is None else stream
    with torch.cuda.device(out.device):
        N.check(N.lib().kf_kmers_rows(keys.data_ptr(), counts.data_ptr(), 4 if counts.dtype == torch.int32 else 8,
                                      tab.src0.data_ptr(), tab.n.data_ptr(), tab.dst0.data_ptr(),
                                      tab.denom.data_ptr(), tab.n_seg, k, int(row_lo), int(row_hi), out.data_ptr(),
                                      status.data_ptr(), s), "kf_kmers_rows")


KMERS_EXACT_SUM = 1 << 24   # below this a float32 sum of whole numbers is exact in any order


def kmers_denominators(counts: torch.Tensor, src0, n) -> np.ndarray:
    """float32 [n_seg]: each segment's divisor of the get_kmers weights, equal
    bit for bit to main.kmers_matrix's `np.sum(c.astype(np.float32))` over its
    counts (counts int32 holding uint32 bit patterns, or int64; segment s is
    counts[src0[s] : src0[s] + n[s]]).  The exact integer total is summed where
    the counts are; below 2^24 every partial sum of the float32 counts is a whole
    number float32 holds, so np.sum gives float32(total) in any order.  From 2^24
    on np.sum's pairwise result depends on the rounding of its partial sums: that
    segment's counts are copied back and summed by np.sum itself."""
    u32 = counts.dtype == torch.int32
    assert u32 or counts.dtype == torch.int64
    seg = [counts[int(a): int(a) + int(m)] for a, m in zip(src0, n)]
    if not seg:
        return np.zeros(0, np.float32)
    tot = torch.stack([c.sum(dtype=torch.int64) + (((c < 0).sum(dtype=torch.int64) << 32) if u32 else 0)
                       for c in seg]).cpu().numpy()
    den = tot.astype(np.float32)
    for s in np.flatnonzero(tot >= KMERS_EXACT_SUM):
        c = seg[s].cpu().numpy()
        den[s] = np.sum((c.view(np.uint32) if u32 else c).astype(np.float32))
    return den


_std_codes: dict = {}       # k -> uint64 [nbins] on the host
_DEV_STD_CODES: dict = {}   # (k, device index) -> the same as int64 on the device


def vocab_std_codes(k: int) -> np.ndarray:
    """uint64 [nbins]: column -> the standard 2-bit code (A0 C1 G2 T3, first base
    most significant) of the vocab's k-mer for that column, from vocab_text(k).
    Not col2rep: that is the class's minimum in kf-code order, which can be the
    other strand.  The vocab is sorted, so ascending columns are ascending codes."""
    if k not in _std_codes:
        v = np.frombuffer(vocab_text(k), dtype=np.uint8).reshape(-1, k + 1)[:, :k]
        lut = np.zeros(256, dtype=np.uint64)
        for ch, d in zip(b"ACGT", range(4)):
            lut[ch] = d
        code = np.zeros(v.shape[0], dtype=np.uint64)
        for i in range(k):
            code = (code << np.uint64(2)) | lut[v[:, i]]
        _std_codes[k] = code
    return _std_codes[k]


def dense_present(counts: torch.Tensor, k: int):
    """The non-zero bins of a dense count matrix (int32 [B, nbins] holding uint32,
    as KmerCounter.count gives) in the sparse counter's form: (keys int64, counts
    int32, nuniq int64[B] on the host, off int64[B] on the host) with genome g's
    k-mers at keys[off[g] : off[g] + nuniq[g]], packed, keys ascending."""
    assert counts.dim() == 2 and counts.dtype == torch.int32 and counts.shape[1] == num_bins(k)
    dev = counts.device
    key = (k, dev.index if dev.index is not None else torch.cuda.current_device())
    if key not in _DEV_STD_CODES:   # immutable: one upload per (k, device) and process
        _DEV_STD_CODES[key] = torch.from_numpy(vocab_std_codes(k).view(np.int64)).to(dev)
    nz = counts != 0
    nu = nz.sum(dim=1).cpu().numpy().astype(np.int64)
    off = np.concatenate([[0], np.cumsum(nu)[:-1]]).astype(np.int64) if nu.size else np.zeros(0, np.int64)
    cols = nz.nonzero()[:, 1]   # row-major: ascending columns inside a row
    return _DEV_STD_CODES[key][cols], counts[nz], nu, off


def kmers_features(keys: torch.Tensor | None, counts: torch.Tensor, nuniq: torch.Tensor | None, off, k: int
                   ) -> torch.Tensor:
    """In-memory hand-off to the FSW trainer (the analogue of `features`): the
    device float32 tensor [B, Nmax, k + 1] that
    `train_model_set.pad_input([np.load(f) for f in files])` (train_model_set.py:92-94)
    builds from get_kmers' `.npy` files of the same genomes, without the files.
    Takes SparseCounter.count's (keys, counts, nuniq) with the batch's offsets
    `off`, or -- with keys, nuniq and off None -- KmerCounter.count's dense
    [B, nbins] count matrix (k <= 12).  A genome without k-mers is a row of
    zeros (get_kmers writes no file for it)."""
    if counts.dim() == 2:
        keys, counts, nu, off = dense_present(counts, k)
    else:
        nu = SparseCounter.nuniq_to_host(nuniq)
        off = np.asarray(off, dtype=np.uint64)[: nu.size].astype(np.int64)
    dev = counts.device
    B, nmax = int(nu.size), int(nu.max()) if nu.size else 0
    out = torch.empty((B, nmax, k + 1), dtype=torch.float32, device=dev)
    if B == 0 or nmax == 0:
        return out
    tab = kmers_tables(off, nu, np.arange(B + 1, dtype=np.int64) * nmax, kmers_denominators(counts, off, nu), dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    kmers_rows(keys, counts, tab, k, 0, B * nmax, out, status)
    if int(status.item()) != 0:
        raise N.NativeError("kf_kmers_rows: the device refused the segment tables")
    return out


def synth_ids(n: int, g0: int = 0, g_stride: int = 1) -> list[int]:
    return [g0 + i * g_stride for i in range(n)]


def synth_layout(n: int, seq_len: int, width: int = 80, g0: int = 0, g_stride: int = 1,
                 align: int = 256) -> np.ndarray:
    """Offsets of n synthetic genomes (kf_synth_fasta layout)."""
    L = N.lib()
    off = np.zeros(n + 1, dtype=np.uint64)
    pos = 0
    for i, g in enumerate(synth_ids(n, g0, g_stride)):
        off[i] = pos
        pos += int(L.kf_synth_genome_bytes(g, seq_len, width, align))
    off[-1] = pos
    return off


def synth_excl(off: np.ndarray, g0: int = 0, g_stride: int = 1) -> np.ndarray:
    """Record index of a synthetic batch: one header line per genome."""
    L = N.lib()
    n = len(off) - 1
    ex = np.empty(2 * n, dtype=np.uint64)
    for i, g in enumerate(synth_ids(n, g0, g_stride)):
        ex[2 * i] = off[i]
        ex[2 * i + 1] = off[i] + int(L.kf_synth_header_len(g)) - 1  # up to the header's '\n'
    return ex


def synth_fasta_bytes(seq_len: int, width: int = 80, g: int = 0) -> int:
    """Unpadded FASTA size of one synthetic genome (header + bases + newlines)."""
    return int(N.lib().kf_synth_header_len(g)) + seq_len + (seq_len + width - 1) // width


def synth_device_batch(n: int, seq_len: int, seed0: int, width: int = 80, n_period: int = 0, g0: int = 0,
                       g_stride: int = 1, device: torch.device | str = "cuda") -> DeviceBatch:
    """Generate n synthetic FASTA genomes (ids g0 + i*g_stride) directly in HBM."""
    dev = torch.device(device)
    off = synth_layout(n, seq_len, width, g0, g_stride)
    ex = synth_excl(off, g0, g_stride)
    data = torch.empty(int(off[-1]), dtype=torch.uint8, device=dev)
    doff = torch.from_numpy(off.view(np.int64)).to(dev)
    dex = torch.from_numpy(ex.view(np.int64)).to(dev)
    s = _stream_ptr(dev)
    with torch.cuda.device(dev):
        for c0 in range(0, n, 65535):
            c1 = min(n, c0 + 65535)
            N.check(N.lib().kf_synth_fasta(data.data_ptr(), doff[c0:].data_ptr(), c1 - c0, g0 + c0 * g_stride,
                                           g_stride, seed0, seq_len, width, n_period, s), "kf_synth_fasta")
    return DeviceBatch(data, doff, dex, n, n)
