"""``python -m kf2vecfsw_amd.main get_frequencies ...`` -- drop-in for the
reference's ``python -m kf2vec.main get_frequencies`` (kf2vec/main.py:250-373,
parser :1023-1038, dispatch :1489-1495).

Same flags, same stdout lines, same ``<sample>.kf`` bytes; the Jellyfish
subprocess pair per file (main.py:309-319) is replaced by one device pass per
batch of files through ``libkf2vec_gpu.so``.  Differences (DESIGN.md "Boundary"):
no ``.jf``/``.dump`` temporaries are created; a device or I/O error raises
instead of being silenced; ``-p`` sizes the host formatting/writing threads.
"""
from __future__ import annotations

import argparse
import ctypes
import multiprocessing as mp
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import _native as N

__version__ = "kf2vec 0.1.3 (kf2vecfsw_amd MI355X)"

default_k_len = 7          # main.py:80
default_seed = 28          # main.py:97
default_block_sz = 4000    # main.py:98
default_hidden_sz = 2048   # main.py:86
default_embed_sz = 1024    # main.py:87
default_batch_sz = 16      # main.py:88
default_cl_epochs = 2000   # main.py:90
default_di_epochs = 8000   # main.py:91
default_lr = 0.00001       # main.py:93
default_lr_min = 3e-6      # main.py:94
default_lr_decay = 2000    # main.py:95
min_k_len = 2              # main.py:81
max_k_len = 31             # main.py:82
supported_k = range(3, 12)  # rule-generated vocab (reference ships 3..9; 10 is a missing blob)

FORMATS = [".fq", ".fastq", ".fa", ".fna", ".fasta"]   # main.py:272
_SUFFIXES = tuple(FORMATS)


def list_inputs(input_dir: str) -> tuple[list[str], list[str]]:
    """main.py:272-275: files in os.listdir order and their sample names."""
    # (fnmatch "*" + form on POSIX is a case-sensitive suffix test)
    files_names = [f for f in os.listdir(input_dir) if f.endswith(_SUFFIXES)]
    samples_names = [f.rsplit(".f", 1)[0] for f in files_names]
    return files_names, samples_names


def write_kf_files(output_dir: str, names: list[str], counts: np.ndarray, pseudocount: bool, raw_cnt: bool,
                   threads: int) -> None:
    """Format + write ``<name>.kf`` for every row (main.py:331-357) with C++ threads."""
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    enc = [os.fsencode(n) for n in names]
    arr = (ctypes.c_char_p * len(enc))(*enc)
    N.check(N.lib().kf_write_kf_files(os.fsencode(output_dir), arr, len(enc), counts.ctypes.data,
                                      counts.shape[1] if counts.ndim == 2 else 0, int(bool(pseudocount)),
                                      int(bool(raw_cnt)), max(1, int(threads))), "kf_write_kf_files")


def format_kf(name: str, counts: np.ndarray, pseudocount: bool = False, raw_cnt: bool = False) -> bytes:
    """One ``.kf`` line (main.py:344-357), formatted by the C++ writer."""
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    nm = os.fsencode(name)
    cap = len(nm) + 2 + 26 * counts.size
    buf = ctypes.create_string_buffer(cap)
    w = ctypes.c_uint64(0)
    N.check(N.lib().kf_format_kf(nm, counts.ctypes.data, counts.size, int(pseudocount), int(raw_cnt), buf, cap,
                                 ctypes.byref(w)), "kf_format_kf")
    return buf.raw[: w.value]


def _pipeline_budget(paths: list[str], batch_gb, sizes: list[int] | None = None) -> int:
    """Bytes per batch: -batch_gb if given, else about a quarter of the input
    (so reading, copying, counting and writing overlap; 64 x 5 Mbp on two boxes,
    tools/e2e_bench.py: 4 parts 26.1 and 32.9 Gbases/s against 8 parts 22.5 and
    29.8, profiles/r05/v19_e2e_parts.json, v6_e2e_variants.json) within
    [16 MiB, 4 GiB].  KF_BATCH_PARTS overrides the part count."""
    if batch_gb:
        return int(float(batch_gb) * (1 << 30))
    total = sum(sizes) if sizes is not None else sum(os.path.getsize(p) for p in paths)
    parts = int(os.environ.get("KF_BATCH_PARTS", "4"))
    return int(min(max(total // parts, 16 << 20), 4 << 30))


COUNT_BUDGET = 2 << 30   # default count-matrix bytes per batch (device rows; as much again pinned on the host)


def _count_cap(row_bytes: int, batch_gb) -> int:
    """Genomes per batch so that the batch's count matrix (row_bytes per genome:
    4 x bins, 8 MiB at k=11, 33.6 MB at k=12) stays within -batch_gb if given,
    else COUNT_BUDGET (KF_COUNT_BUDGET_MB overrides).  The reference holds one
    genome's counts at a time (main.py:301-357); a batch of many small files must
    not hold thousands of rows."""
    env = os.environ.get("KF_COUNT_BUDGET_MB")
    b = int(float(env) * (1 << 20)) if env else int(float(batch_gb) * (1 << 30)) if batch_gb else COUNT_BUDGET
    return max(1, b // max(1, int(row_bytes)))


def _batches(paths: list[str], budget: int, ramp: bool = False, max_files: int | None = None) -> list[list[int]]:
    """Consecutive files in batches of at most `budget` bytes (a file larger than
    that alone) and at most `max_files` files.  ramp: the first two batches get a
    quarter and a half of the byte budget, so a pipeline's later stages start
    sooner."""
    return _size_batches([os.path.getsize(p) for p in paths], budget, ramp, max_files)


def _size_batches(sizes: list[int], budget: int, ramp: bool = False, max_files: int | None = None) -> list[list[int]]:
    """_batches over item sizes (files, or get_chunks' file parts)."""
    out, cur, size = [], [], 0
    for i, s in enumerate(sizes):
        lim = budget >> max(0, 2 - len(out)) if ramp else budget
        if cur and (size + s > lim or (max_files is not None and len(cur) >= max_files)):
            out.append(cur)
            cur, size = [], 0
        cur.append(i)
        size += s
    if cur:
        out.append(cur)
    return out


def _plan_units(sizes: list[int], pieces: list | None, budget: int, max_units: int | None = None,
                ramp: bool = True) -> list[list[tuple[int, int, int, str]]]:
    """get_frequencies' batches as lists of units (file index, start, end, kind):
    a whole file (kind "whole") or, for a file i with pieces[i] = (kind, [(start,
    end), ...]), kind "fasta" or "fastq", each of its pieces.  Consecutive units in
    batches as _size_batches makes them -- at most `budget` bytes (a larger unit
    alone; ramp: a quarter and a half of it for the first two) and at most
    `max_units` units, a piece counting as a genome -- and a batch holds whole
    files only or pieces of one kind only.  So a batch is at most max(budget,
    largest unit) bytes whatever the file sizes, and with no pieces the batches
    are _size_batches' own.  A pure function of its arguments."""
    out, cur, size = [], [], 0
    for fi, s in enumerate(sizes):
        pcs = pieces[fi] if pieces is not None else None
        for u in ([(fi, 0, s, "whole")] if not pcs else [(fi, a, e, pcs[0]) for a, e in pcs[1]]):
            lim = budget >> max(0, 2 - len(out)) if ramp else budget
            if cur and (size + u[2] - u[1] > lim or (max_units is not None and len(cur) >= max_units)
                        or u[3] != cur[-1][3]):
                out.append(cur)
                cur, size = [], 0
            cur.append(u)
            size += u[2] - u[1]
    if cur:
        out.append(cur)
    return out


SPLIT_GB = 4.0   # get_frequencies -split_gb: the upper clamp of _pipeline_budget


def _split_pieces(paths: list[str], sizes: list[int], k: int, split_gb) -> list | None:
    """_plan_units' `pieces` for get_frequencies: a file above -split_gb S GiB is
    cut into pieces of about min(S, 1) GiB -- fastq_pieces if its first byte is
    '@' (the sniff of KF_FMT_AUTO), else fasta_pieces -- unless no cut was found
    (one piece: the file is counted whole).  None if no file is cut."""
    s = float(SPLIT_GB if split_gb is None else split_gb)
    if s <= 0:
        return None
    limit, piece = int(s * (1 << 30)), int(min(s, 1.0) * (1 << 30))
    out: list = [None] * len(paths)
    for i, (p, sz) in enumerate(zip(paths, sizes)):
        if sz > limit:
            with open(p, "rb") as f:
                fq = f.read(1) == b"@"
            pcs = fastq_pieces(p, piece) if fq else fasta_pieces(p, k, piece)
            if len(pcs) > 1:
                out[i] = ("fastq" if fq else "fasta", pcs)
    return out if any(o is not None for o in out) else None


def shard_files(sizes: list[int], samples: list[str], world: int) -> list[list[int]]:
    """Byte-balanced shards of the input files for `world` GPUs (section 8(e): genomes
    are independent, no collective).  Files of one sample name stay in one shard,
    so the reference's last-file-wins rule for duplicate names (main.py:357 writes
    in input order) holds inside that shard; groups go largest first to the least
    loaded shard; each shard keeps the input order."""
    groups: dict[str, list[int]] = {}
    for i, s in enumerate(samples):
        groups.setdefault(s, []).append(i)
    load = [0] * world
    out: list[list[int]] = [[] for _ in range(world)]
    for g in sorted(groups.values(), key=lambda g: (-sum(sizes[i] for i in g), g[0])):
        r = min(range(world), key=lambda r: (load[r], r))
        out[r].extend(g)
        load[r] += sum(sizes[i] for i in g)
    return [sorted(o) for o in out]


def _shard_spec(args) -> tuple[int, int] | None:
    """(rank, world) when this process counts one shard: a child of `-gpus N`
    (KF_SHARD="r,N") or one rank of torchrun (RANK / WORLD_SIZE, no -gpus)."""
    e = os.environ.get("KF_SHARD")
    if e:
        r, w = (int(x) for x in e.split(","))
        return r, w
    if getattr(args, "gpus", 1) == 1 and int(os.environ.get("WORLD_SIZE", "1")) > 1:
        return int(os.environ.get("RANK", "0")), int(os.environ["WORLD_SIZE"])
    return None


def _spawn_shards(argv: list[str], world: int) -> int:
    """`-gpus N`: one child process per GPU (cuda:r), each counting shard r; no
    data crosses between them (each writes its own genomes' .kf files).  The
    parent never touches the GPU (KF_SHARD_DEVICE=cuda:0 puts every child on one
    GPU, for rehearsal on a one-GPU box)."""
    import subprocess
    procs = []
    for r in range(world):
        pkg_parent = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        env = dict(os.environ, KF_SHARD=f"{r},{world}",
                   PYTHONPATH=os.pathsep.join(filter(None, [pkg_parent, os.environ.get("PYTHONPATH")])))
        dev = os.environ.get("KF_SHARD_DEVICE") or f"cuda:{r}"
        procs.append(subprocess.Popen([sys.executable, "-m", "kf2vecfsw_amd.main"] + argv + ["-device", dev], env=env))
    return max(abs(p.wait()) for p in procs)


def visible_gpus(env=None) -> int | None:
    """GPUs this process may use, counted without initialising HIP (the -gpus
    parent forks children and must never touch the GPU itself): the GPU nodes of
    the KFD topology (nodes with SIMDs), capped by every one of
    ROCR_VISIBLE_DEVICES / HIP_VISIBLE_DEVICES / CUDA_VISIBLE_DEVICES that is set
    (HIP applies its mask on top of ROCR's, so the smallest wins).  None when the
    topology is unreadable and no mask is set: unknown."""
    topo = "/sys/class/kfd/kfd/topology/nodes"
    n_kfd = None
    try:
        n_kfd = 0
        for d in os.listdir(topo):
            try:
                props = open(os.path.join(topo, d, "properties")).read().split("\n")
            except OSError:
                continue
            if any(ln.startswith("simd_count") and ln.split()[-1] != "0" for ln in props):
                n_kfd += 1
    except OSError:
        n_kfd = None
    n = n_kfd
    env = os.environ if env is None else env
    for var in ("ROCR_VISIBLE_DEVICES", "HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        v = env.get(var)
        if v is not None:
            ids = [x for x in v.split(",") if x.strip() != ""]
            n = len(ids) if n is None else min(n, len(ids))
    return n


def usable_cpus() -> tuple[int, dict]:
    """CPUs this process may run on: the affinity mask, capped by a cgroup v2/v1
    CPU quota if one is set (a GPU box may show the whole host in the mask and
    in os.cpu_count(), e.g. 256, against a quota of 16)."""
    aff = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    quota = None
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            quota = float(q) / float(per)
    except (OSError, ValueError):
        try:
            q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0:
                quota = q / per
        except (OSError, ValueError):
            pass
    n = aff if quota is None else max(1, min(aff, int(quota)))
    return n, {"nproc": os.cpu_count(), "affinity": aff, "cgroup_cpu_quota": quota}


def host_threads(p, world: int = 1) -> int:
    """Host threads of this process (file readers, .kf formatters/writers):
    min(-p, usable CPUs), split evenly over the `world` processes that share the
    host (-gpus N children, torchrun ranks on one node).  The reference hands -p
    to Jellyfish as `-t` (main.py:309) with default mp.cpu_count()
    (main.py:1031-1033), which on a GPU box counts every host CPU, not the
    process's quota: 256 threads on a 16-CPU quota."""
    usable = usable_cpus()[0]
    return max(1, min(max(1, int(p)), usable) // max(1, int(world)))


def _procs_per_host(shard) -> int:
    """Processes of this run sharing this host's CPUs: the -gpus N children (all
    local), or torchrun's ranks on this node (LOCAL_WORLD_SIZE)."""
    if shard is None:
        return 1
    if os.environ.get("KF_SHARD"):
        return shard[1]
    return int(os.environ.get("LOCAL_WORLD_SIZE", shard[1]))


def cli_host_threads(args) -> int:
    """get_frequencies' host threads in this process: -p capped by the usable
    CPUs, shared by the processes of this run on this host."""
    return host_threads(args.p, _procs_per_host(_shard_spec(args)))


def get_frequencies(args) -> None:
    """kf2vec/main.py:250-373 on the GPU (-gpus N: byte-balanced file shards, one
    process per GPU)."""
    import time
    t_entry = time.perf_counter()
    shard = _shard_spec(args)
    lead = shard is None or shard[0] == 0
    if getattr(args, "gpus", 1) != 1 and int(os.environ.get("WORLD_SIZE", "1")) > 1 and not os.environ.get("KF_SHARD"):
        # under torchrun every rank is already one shard: a -gpus spawn per rank
        # would count the whole input on every rank and race on the same .kf files
        raise ValueError("-gpus N cannot be combined with torchrun (WORLD_SIZE > 1): each rank counts its own shard")
    if shard is None and getattr(args, "gpus", 1) != 1:
        world = args.gpus
        avail = visible_gpus()
        if world <= 0:
            if avail is None:
                raise ValueError("-gpus 0: cannot count the visible GPUs (no KFD topology, no *_VISIBLE_DEVICES)")
            world = max(1, avail)
        elif not os.environ.get("KF_SHARD_DEVICE") and avail is not None and world > avail:
            raise ValueError("-gpus {}: only {} GPU(s) visible".format(world, avail))
        if world > 1:
            print("\n==> Starting k-mer counting for {}\n".format(args.input_dir))
            for d in (args.input_dir, args.output_dir):
                if not os.path.exists(d):
                    print("No such directory '{}'".format(d), file=sys.stderr)
                    sys.exit(0)
            sys.stdout.flush()   # before the children write to the same stdout
            rc = _spawn_shards(_child_argv(args), world)
            if rc:
                sys.exit(rc)
            print("\n==> Done processing {}".format(args.input_dir))
            return
    if lead and not os.environ.get("KF_SHARD"):
        print("\n==> Starting k-mer counting for {}\n".format(args.input_dir))

    if not os.path.exists(args.input_dir):            # main.py:255-259 (exit status 0, as the reference)
        print("No such directory '{}'".format(args.input_dir), file=sys.stderr)
        sys.exit(0)
    if not os.path.exists(args.output_dir):           # main.py:262-266
        print("No such directory '{}'".format(args.output_dir), file=sys.stderr)
        sys.exit(0)

    files_names, samples_names = list_inputs(args.input_dir)
    if shard is not None:
        sizes = [os.path.getsize(os.path.join(args.input_dir, f)) for f in files_names]
        mine = shard_files(sizes, samples_names, shard[1])[shard[0]]
        files_names = [files_names[i] for i in mine]
        samples_names = [samples_names[i] for i in mine]
    if args.k not in supported_k:
        # reference: UnboundLocalError at main.py:327 for k without a vocab branch
        raise ValueError("k={} has no vocabulary: supported k are {}..{}".format(
            args.k, supported_k.start, supported_k.stop - 1))

    import torch
    from .counter import KmerCounter, accumulate_rows, pack_files, pack_ranges, to_device

    if shard is not None and not os.environ.get("KF_SHARD"):
        # torchrun: join the host-only gloo group now, before counting, so that a
        # rank that fails later drops its connections and the others' final
        # barrier errors out at once instead of waiting for a rendezvous timeout
        _join_group()
    dflt = f"cuda:{os.environ.get('LOCAL_RANK', '0')}" if shard is not None else "cuda"
    device = torch.device(getattr(args, "device", None) or dflt)
    if not files_names:   # an empty shard
        _finish(args, shard, lead)
        return
    counter = KmerCounter(args.k, device)
    paths = [os.path.join(args.input_dir, f) for f in files_names]
    # the first two batches are a quarter and a half of the others, so that the
    # first H2D and count start sooner
    # ... and at most _count_cap genomes, so the count matrix of a batch (on the
    # device, pinned for the writer, `behind` batches deep) stays bounded at any k
    batch_gb = getattr(args, "batch_gb", None)
    fsz = [os.path.getsize(p) for p in paths]
    # a file above -split_gb goes through the same stages in pieces, each piece one
    # genome of a batch, its rows summed on the device into one row per file
    # (kf_rows_accumulate): no batch, pinned slot or device block grows with a file
    batches = _plan_units(fsz, _split_pieces(paths, fsz, args.k, getattr(args, "split_gb", SPLIT_GB)),
                          _pipeline_budget(paths, batch_gb, fsz), _count_cap(4 * counter.nbins, batch_gb))
    last_unit = {u[0]: (bi, j) for bi, b in enumerate(batches) for j, u in enumerate(b)}   # a file's last piece
    # the reference processes files in order and later ones overwrite earlier
    # ones with the same sample name: keep the last occurrence only
    last = {s: i for i, s in enumerate(samples_names)}
    threads = cli_host_threads(args)
    from collections import deque
    from concurrent.futures import ThreadPoolExecutor

    files_pool = ThreadPoolExecutor(max_workers=threads)
    # KF_TRACE=1: per-batch stage timeline on stderr (host ms; device events ms
    # from the first H2D's start event), for tools/e2e_bench.py
    trace = os.environ.get("KF_TRACE") == "1"
    t_origin = time.perf_counter()
    tr: list = []

    def now_ms():
        return round((time.perf_counter() - t_origin) * 1e3, 3)

    # pinned input slots, reused round robin (a fresh pinned block per batch costs
    # ~1 ms of allocation on the reader's path): batch i reads into slot i mod
    # n_slots once the H2D that last read that slot has completed
    slot_bytes = max(sum((e - a + 15) // 16 * 16 for _, a, e, _ in b) for b in batches)   # 16-byte aligned units
    n_slots = min(len(batches), int(os.environ.get("KF_READ_AHEAD", "2")) + 2)
    slots = [torch.empty(max(slot_bytes, 16), dtype=torch.uint8, pin_memory=True) for _ in range(n_slots)]
    slot_ev: list = [None] * n_slots

    def pack(bi, units):
        t0 = now_ms()
        tm = {}
        j = bi % n_slots
        idx = [u[0] for u in units]
        if slot_ev[j] is not None:
            slot_ev[j].synchronize()
        # FASTA batches and all-FASTQ batches are indexed on the device (to_device
        # -> kf_index_fasta / kf_index_fastq): the readers only copy the files.
        # A batch that mixes the two is still indexed here, by the files' pool.
        if units[0][3] == "whole":
            hb = pack_files([paths[i] for i in idx], [samples_names[i] for i in idx], pool=files_pool, times=tm,
                            buf=slots[j], index=False)
        else:   # pieces of one kind: always indexed on the device
            hb = pack_ranges([(paths[i], a, e) for i, a, e, _ in units], [samples_names[i] for i in idx],
                             threads=threads, buf=slots[j], fastq=units[0][3] == "fastq")
        # the batch goes to the device on the copy stream as soon as it is read,
        # so its H2D overlaps the previous batch's index, count and copy-back
        # (copies issued while the batch is read, 16 MiB at a time from the
        # native readers, measured no faster: DESIGN section 8)
        with torch.cuda.stream(copy_stream):
            hb.dev_data = hb.data.to(device, non_blocking=True)
            hb.dev_event = torch.cuda.Event()
            hb.dev_event.record(copy_stream)
        slot_ev[j] = hb.dev_event   # the slot is free again once this copy has run
        if trace:
            tr.append(("read", idx[0], t0, now_ms(), tm))
        return hb

    # Three-stage pipeline over batches:
    #   readers (2)   : read the next batches into pinned memory (the native
    #                   pool's threads, pieces of 1 MiB) and put each on the copy
    #                   stream as soon as it is read; as many
    #                   batches are queued for them as there are pinned slots, so
    #                   the reads (and the copies behind them) run back to back
    #                   whatever this thread is doing (r06 KF_TRACE: with only
    #                   the next two queued, the third read started when this
    #                   thread took batch 0, after its ~2.5 ms of set-up, and the
    #                   copy stream idled 1.5 ms)
    #   this thread   : record index + count + D2H of batch i on a side stream
    #   writer thread : wait for batch i's copy-back, format + write its .kf files
    # The prints stay in the reference's per-file order (main.py:332-341).
    stream = torch.cuda.Stream(device)
    copy_stream = torch.cuda.Stream(device)
    # two readers: one read call's tail (its last pieces, the files' opens) and
    # the writer's formatting leave host threads idle that a second batch's read
    # fills
    reader = ThreadPoolExecutor(max_workers=int(os.environ.get("KF_READERS", "2")))
    writer = ThreadPoolExecutor(max_workers=1)
    ahead = n_slots   # batches queued for the readers (read, or copied, but not yet counted)
    reads = deque(reader.submit(pack, i, batches[i]) for i in range(min(ahead, len(batches))))
    # While the first batches are read: the side stream's first event and launch
    # and the device block for a batch (the caching allocator keeps it for this
    # stream) would otherwise cost ~2 ms between the first read and its H2D
    # (KF_TRACE: got 0 -> issue 0, tools/e2e_bench.py).
    big = slot_bytes
    with torch.cuda.stream(copy_stream):   # the batches' device blocks come from the copy stream's pool
        warm = torch.empty(big + 16, dtype=torch.uint8, device=device)
        warm[:16].zero_()
        del warm
    with torch.cuda.stream(stream):
        torch.cuda.Event(enable_timing=True).record(stream)
    copy_stream.synchronize()
    stream.synchronize()
    writes = []
    # batches whose .kf files may still be waiting for the writer: each holds a
    # pinned count matrix (4 x bins B per genome), so the backlog is bounded
    behind = max(1, int(os.environ.get("KF_WRITE_BEHIND", "2")))

    def write(ev, host, names, hstat=None, fnames=None):
        ev.synchronize()
        t0 = now_ms()
        c = host.numpy().view(np.uint32)
        for j in range(0 if hstat is None else len(fnames)):   # files counted in pieces: the sums' status words
            st = int(hstat[j])
            if st & 1:
                raise ValueError("{}: a k-mer count passed 2^32 - 1 when the file's pieces were summed "
                                 "(uint32 counts): nothing was written for it".format(fnames[j]))
            if st:
                raise N.NativeError("kf_rows_accumulate: bad segment table ({})".format(fnames[j]))
        write_kf_files(args.output_dir, names, c, args.pseudocount, args.raw_cnt, threads)
        if trace:
            tr.append(("write", names[0] if names else "", t0, now_ms()))

    def stop():
        """Before an error is raised from this thread: nothing more is read, and
        what was handed to the writer is written."""
        for f in reads:
            f.cancel()
        reader.shutdown()
        writer.shutdown()
        files_pool.shutdown()

    # a file counted in pieces: its row, total and status on the device from its
    # first piece until its last one is counted (its pieces may span batches)
    acc: dict = {}
    seg_of: dict = {}   # n -> the segment table [0, n] on the device

    def fold(bi, units, counts, totals):
        """Adds a piece batch's rows into their files' accumulator rows
        (kf_rows_accumulate, one call per file in the batch); returns the files
        whose last piece this batch holds."""
        done, j = [], 0
        while j < len(units):
            fi, j1 = units[j][0], j + 1
            while j1 < len(units) and units[j1][0] == fi:
                j1 += 1
            if fi not in acc:
                acc[fi] = (torch.zeros((1, counter.nbins), dtype=torch.int32, device=device),
                           torch.zeros(1, dtype=torch.int64, device=device),
                           torch.zeros(1, dtype=torch.int32, device=device))
            if j1 - j not in seg_of:
                seg_of[j1 - j] = torch.tensor([0, j1 - j], dtype=torch.int32).pin_memory().to(device, non_blocking=True)
            accumulate_rows(counts[j:j1], totals[j:j1], seg_of[j1 - j], *acc[fi], accumulate=True,
                            stream=stream.cuda_stream)
            if last_unit[fi] == (bi, j1 - 1):
                done.append(fi)
            j = j1
        return done

    evs = []
    for bi, units in enumerate(batches):
        idx = [u[0] for u in units]
        whole = units[0][3] == "whole"
        t_wait = now_ms()
        hb = reads.popleft().result()
        if trace:
            tr.append(("got", bi, t_wait, now_ms()))
        if bi + ahead < len(batches):   # its slot is batch bi's, free once bi's copy has run
            reads.append(reader.submit(pack, bi + ahead, batches[bi + ahead]))
        with torch.cuda.stream(stream):
            if trace:
                e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
                e[0].record(stream)
                evs.append((bi, now_ms(), e))
            # a FASTQ piece that is not regular was cut at a wrong line: the host
            # index would count it as if it were well cut, so it is refused instead
            db = to_device(hb, device, fallback=whole)
            del hb
            if db.irregular:
                fi, a = units[db.irregular[0]][:2]
                stop()
                raise ValueError("{}: the piece at byte {} is not FASTQ in the regular four-line form (a cut at a "
                                 "line that is no record start, or a malformed file): -split_gb 0 counts the file "
                                 "whole".format(files_names[fi], a))
            if trace:
                e[1].record(stream)
                th = [now_ms()]
            counts, totals = counter.count(db, stream=stream.cuda_stream)
            if trace:
                e[2].record(stream)
                th.append(now_ms())
            hstat = None
            if whole:
                done = idx
                keep = [j for j, i in enumerate(idx) if last[samples_names[i]] == i]
                kept = [idx[j] for j in keep]
                # (int64 named: a batch of which no file is kept -- a whole file ahead of the pieces of a
                # later file with its sample name -- gives an empty index list)
                rows = counts if len(keep) == len(idx) else counts[torch.tensor(keep, dtype=torch.int64, device=device)]
            else:
                done = fold(bi, units, counts, totals)
                kept = [fi for fi in done if last[samples_names[fi]] == fi]
                rows = torch.cat([acc[fi][0] for fi in kept]) if kept else counts[:0]
                if kept:
                    hstat = torch.empty(len(kept), dtype=torch.int32, pin_memory=True)
                    hstat.copy_(torch.cat([acc[fi][2] for fi in kept]), non_blocking=True)
                for fi in done:
                    del acc[fi]
            host = torch.empty(rows.shape, dtype=rows.dtype, pin_memory=True)
            if trace:
                th.append(now_ms())
            host.copy_(rows, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(stream)
            if trace:
                e[3].record(stream)
                th.append(now_ms())
        for i in done:   # a file counted in pieces: once, with its last piece
            if args.pseudocount:                       # main.py:332-333
                print(">>> Adding pseudocounts. Sample: {}".format(files_names[i]))
            if not args.raw_cnt:                       # main.py:340-341
                print(">>> Normalizing. Sample: {}".format(files_names[i]))
        if bi >= behind:   # backpressure: at most `behind` batches queued for the writer
            writes[bi - behind].result()
        writes.append(writer.submit(write, ev, host, [samples_names[i] for i in kept], hstat,
                                    [files_names[i] for i in kept]))
        del host, rows, counts, totals, db
        if trace:
            th.append(now_ms())
            tr.append(("issue", bi, th))   # after: to_device, count, pinned alloc, D2H, prints+submit
    for w in writes:
        w.result()
    t_written = now_ms()
    reader.shutdown()
    writer.shutdown()
    files_pool.shutdown()
    if trace and evs:
        base_cpu = evs[0][1]
        e00 = evs[0][2][0]
        for bi, t_issue, e in evs:   # device times re-based on the first start event's host time
            d = [round(base_cpu + e00.elapsed_time(x), 3) for x in e]
            tr.append(("gpu", bi, t_issue, {"h2d": d[:2], "count": d[1:3], "d2h": d[2:4]}))
        import json
        from .counter import INDEX_PATHS   # which record index the batches took (this process, so far)
        print(json.dumps({"kf_trace": tr, "total_ms": now_ms(), "written_ms": t_written,
                          "setup_ms": round((t_origin - t_entry) * 1e3, 3), "index_paths": dict(INDEX_PATHS),
                          "pinned_slots": [n_slots, slot_bytes]}),
              file=sys.stderr)

    _finish(args, shard, lead)


def _join_group() -> None:
    """Host-only gloo group of the torchrun ranks (nothing on the data path)."""
    import datetime

    import torch.distributed as dist
    if not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        # a rank may wait here for the slowest shard's counting: a long timeout
        dist.init_process_group("gloo", timeout=datetime.timedelta(hours=6))


def _finish(args, shard, lead: bool) -> None:
    """torchrun ranks meet in a gloo barrier (host only, nothing crosses) so rank 0
    prints the reference's last line after every shard is written."""
    if shard is not None and not os.environ.get("KF_SHARD"):
        import torch.distributed as dist
        _join_group()
        dist.barrier()
    if lead and not os.environ.get("KF_SHARD"):
        print("\n==> Done processing {}".format(args.input_dir))


def _child_argv(args) -> list[str]:
    """The get_frequencies command line of a -gpus child (its shard and device
    come from KF_SHARD and -device)."""
    a = ["get_frequencies", "-input_dir", args.input_dir, "-output_dir", args.output_dir, "-k", str(args.k),
         "-p", str(args.p)]
    if args.pseudocount:
        a.append("-pseudocount")
    if args.raw_cnt:
        a.append("-raw_cnt")
    if getattr(args, "batch_gb", None):
        a += ["-batch_gb", str(args.batch_gb)]
    if getattr(args, "split_gb", None) is not None:
        a += ["-split_gb", repr(float(args.split_gb))]
    return a


# ---------------------------------------------------------------------------
# get_kmers (main.py:112-184): sparse present-k-mer matrices for the FSW trainer
# ---------------------------------------------------------------------------
_GET_KMERS_DIGIT = {ord("A"): 0, ord("T"): 1, ord("C"): 2, ord("G"): 3}   # main.py:118
_digit_tables: dict = {}


def vocab_digits(k: int) -> np.ndarray:
    """uint8 [nbins, k]: the vocab k-mers as get_kmers digits (A0 T1 C2 G3)."""
    if k not in _digit_tables:
        from .counter import vocab_text
        v = np.frombuffer(vocab_text(k), dtype=np.uint8).reshape(-1, k + 1)[:, :k]
        lut = np.zeros(256, dtype=np.uint8)
        for ch, d in _GET_KMERS_DIGIT.items():
            lut[ch] = d
        _digit_tables[k] = lut[v]
    return _digit_tables[k]


def kmers_matrix(counts: np.ndarray, k: int) -> np.ndarray:
    """float32 [n_present, k+1]: digits of each present canonical k-mer + count /
    total (main.py:165-172).  Rows in vocab (sorted canonical) order; the
    reference's rows follow Jellyfish's hash order, which its FSW consumer
    (models.py:60-64) does not depend on.  While the TOTAL k-mer count (the
    float32 sum) stays below 2^24, that sum is exact in any order, so the
    weights equal the reference's bit for bit.  Above 2^24 total k-mers (genomes
    over ~17 Mbp) np.sum's pairwise float32 result depends on row order, and the
    reference's own result then depends on Jellyfish's hash order: parity there
    is unpinned (no fixture covers it)."""
    counts = np.asarray(counts)
    nz = np.nonzero(counts)[0]
    if nz.size == 0:
        return np.zeros((0, k + 1), dtype=np.float32)
    c = counts[nz].astype(np.float32)
    norm = c / np.sum(c)
    return np.column_stack((vocab_digits(k)[nz].astype(np.float32), norm))


_STD_TO_DIGIT = np.array([0, 2, 3, 1], dtype=np.uint8)   # standard code A0 C1 G2 T3 -> get_kmers digit


def sparse_kmers_matrix(keys: np.ndarray, counts: np.ndarray, k: int) -> np.ndarray:
    """kmers_matrix for the sparse counter (k up to 31): keys are the present
    canonical k-mers as ascending standard 2-bit codes, so the rows come in the
    same (lexicographic) order as kmers_matrix's vocab order."""
    if keys.size == 0:
        return np.zeros((0, k + 1), dtype=np.float32)
    shifts = (2 * np.arange(k - 1, -1, -1, dtype=np.uint64))
    digits = _STD_TO_DIGIT[((keys[:, None] >> shifts[None, :]) & np.uint64(3)).astype(np.intp)]
    c = counts.astype(np.float32)
    norm = c / np.sum(c)                                   # main.py:169
    return np.column_stack((digits.astype(np.float32), norm))


MAX_CALL_BYTES = (1 << 32) - 1   # kf_sparse_count / kf_chunk_compact: 32-bit offsets per call


def _refuse_huge_files(paths: list[str], what: str) -> None:
    """The sparse counter takes one genome per call slice with 32-bit offsets:
    a FASTQ file of 4 GiB or more (get_kmers -k 13..31 cuts only FASTA files into
    pieces) is refused up front, before any output is written, not partway
    through a directory."""
    big = [p for p in paths if os.path.getsize(p) > MAX_CALL_BYTES - 16]
    if big:
        raise ValueError("{}: input file(s) of 4 GiB or more are not supported (per-call 32-bit offsets): {}".format(
            what, ", ".join(os.path.basename(p) for p in big[:5])))


SPLIT_BYTES = 1 << 30   # get_kmers' sparse path: FASTA files above this are counted in pieces


def _line_start(f, pos: int) -> int:
    """Offset of the first byte of the line holding byte `pos`."""
    step = 1 << 16
    hi = pos
    while hi > 0:
        lo = max(0, hi - step)
        blk = os.pread(f, hi - lo, lo)
        j = blk.rfind(b"\n")
        if j >= 0:
            return lo + j + 1
        hi = lo
    return 0


def _overlap_start(fd: int, s: int, k: int) -> int:
    """The byte where a piece whose windows end at or after s must start: k-1
    sequence positions before s (newlines are transparent, every other byte is a
    position), or just after a header line, or the file start."""
    w = 1 << 12
    while True:
        lo = max(0, s - w)
        blk = os.pread(fd, s - lo, lo)
        need, q, o, short = k - 1, len(blk), s, False
        while q > 0 and need > 0:
            q -= 1
            if blk[q] == 10:                          # into the line before: a header ends the walk
                ls = blk.rfind(b"\n", 0, q) + 1
                if ls == 0 and lo > 0:
                    short = True
                    break
                if blk[ls: ls + 1] == b">":
                    return lo + q + 1
                continue
            need -= 1
            o = lo + q
        if not short and (need == 0 or lo == 0):
            o = 0 if need > 0 else o
            if o < s and os.pread(fd, 1, o) == b">":   # a '>' inside a line must not start a piece
                o -= 1                                 # (the device index would take it for a header)
            return o
        w <<= 2


def fasta_pieces(path: str, k: int, piece: int = SPLIT_BYTES) -> list[tuple[int, int]]:
    """Byte ranges [(o_i, e_i)] that count a large FASTA file in pieces (each below
    the sparse counter's 32-bit offsets) with every window counted exactly once.
    Piece i owns the windows ending in [s_i, s_{i+1}) (s_0 = 0, the last ends at
    the file end; a cut s_i lies on a sequence line, moved past a header line).
    Its bytes start k-1 sequence positions earlier, at o_i (_overlap_start):
    fewer than k positions before s_i, so no window ends there, and every window
    ending at or after s_i has its context.  Windows never span a header, so
    pieces never need more.  Jellyfish counts a file of any size in one hash
    (kf2vec/main.py:133-145); this is the device counter's way there."""
    size = os.path.getsize(path)
    if size <= piece:
        return [(0, size)]
    cuts = [0]
    fd = os.open(path, os.O_RDONLY)
    try:
        for i in range(1, -(-size // piece)):
            s = i * piece
            ls = _line_start(fd, s)
            if os.pread(fd, 1, ls) == b">":           # a header line: cut after it
                rest = s
                while True:
                    blk = os.pread(fd, 1 << 16, rest)
                    j = blk.find(b"\n")
                    if j >= 0 or not blk:
                        s = rest + (j + 1 if j >= 0 else len(blk))
                        break
                    rest += len(blk)
            if s >= size or s <= cuts[-1]:
                continue
            cuts.append(s)
        return [(_overlap_start(fd, c, k) if c else 0, cuts[i + 1] if i + 1 < len(cuts) else size)
                for i, c in enumerate(cuts)]
    finally:
        os.close(fd)


def _next_nl(fd: int, pos: int, size: int) -> int:
    """Offset of the first '\\n' at or after pos, or size if there is none."""
    step = 1 << 10
    while pos < size:
        blk = os.pread(fd, min(step, size - pos), pos)
        if not blk:
            break
        j = blk.find(b"\n")
        if j >= 0:
            return pos + j
        pos += len(blk)
        step = min(step << 2, 1 << 20)
    return size


def _fastq_cut(fd: int, s: int, limit: int, size: int) -> int | None:
    """The first line start L in [s, limit) that fastq_pieces accepts as a record
    start, or None."""
    L = s if s == 0 or os.pread(fd, 1, s - 1) == b"\n" else _next_nl(fd, s, size) + 1
    while L < min(limit, size):
        e0 = _next_nl(fd, L, size)                 # line L = [L, e0)
        if os.pread(fd, 1, L) == b"@":
            e1 = _next_nl(fd, e0 + 1, size)        # line L+1 = [e0 + 1, e1)
            if e1 + 1 < size and os.pread(fd, 1, e1 + 1) == b"+":
                s3 = _next_nl(fd, e1 + 1, size) + 1
                if s3 >= size or _next_nl(fd, s3, size) - s3 >= e1 - (e0 + 1):
                    return L
        L = e0 + 1
    return None


def fastq_pieces(path: str, piece: int = SPLIT_BYTES) -> list[tuple[int, int]]:
    """Byte ranges [(a_i, e_i)] that tile a FASTQ file in the regular four-line
    form (include/kf2vec_gpu.h, kf_index_fastq) in pieces of about `piece` bytes,
    each starting at a record's header line: k-mers never span records, so the
    pieces' counts sum to the file's and no overlap is needed.  A start other
    than 0 is the first line L at or after a multiple of `piece` (and before the
    next one: else the two pieces stay one) such that
      - L starts with '@',
      - line L+2 starts with '+',
      - line L+3 is at least as long as line L+1 (lengths without the '\\n'; not
        asked if the file ends before line L+3).
    Every header line followed by a whole record passes.  A quality line that
    starts with '@' does not: two lines on is a sequence line, which in the
    regular form never starts with '+'.  What remains is a sequence line that
    starts with '@' whose quality line starts with '+': a piece cut there starts
    with a sequence line and has its '+' line where a sequence line belongs, so
    the device index reads it as not regular and get_frequencies refuses the
    file, never counts it wrongly.
    A file with no acceptable cut (multi-line records) is one piece."""
    size = os.path.getsize(path)
    if size <= piece:
        return [(0, size)]
    cuts = [0]
    fd = os.open(path, os.O_RDONLY)
    try:
        for i in range(1, -(-size // piece)):
            c = _fastq_cut(fd, i * piece, (i + 1) * piece, size)
            if c is not None and c < size:
                cuts.append(c)
    finally:
        os.close(fd)
    return [(c, cuts[i + 1] if i + 1 < len(cuts) else size) for i, c in enumerate(cuts)]


def _next_record(fd: int, pos: int, size: int) -> int:
    """Offset of the first header line ('>' at a line start) at or after pos
    (pos > 0), or size if there is none."""
    step = 1 << 20
    q = pos - 1                       # the byte before pos: a '\n' there makes pos a line start
    while q < size:
        blk = os.pread(fd, min(step, size - q), q)
        j = blk.find(b"\n>")
        if j >= 0:
            return q + j + 1
        if len(blk) < 2:
            return size
        q += len(blk) - 1             # (a "\n>" across the block edge)
    return size


def record_pieces(path: str, piece: int | None = None) -> list[tuple[int, int]]:
    """Byte ranges [(a_i, e_i)] that cut a FASTA file into parts of about
    `piece` bytes at record starts (header lines), so every part holds whole
    records: get_chunks' windows never span a record, so its parts are counted
    independently (a part's rows follow the previous part's, in file order).
    Bytes before the first header stay in part 0 (no record: seqtk skips them).
    A single record longer than `piece` stays whole.  The reference's
    seqtk/seqkit chain reads a file of any size (kf2vec/main.py:726-760)."""
    piece = SPLIT_BYTES if piece is None else piece
    size = os.path.getsize(path)
    if size <= piece:
        return [(0, size)]
    cuts = [0]
    fd = os.open(path, os.O_RDONLY)
    try:
        while True:
            c = _next_record(fd, cuts[-1] + piece, size)
            if c >= size:
                break
            cuts.append(c)
    finally:
        os.close(fd)
    return [(c, cuts[i + 1] if i + 1 < len(cuts) else size) for i, c in enumerate(cuts)]


def _merge_sorted_counts(parts: list) -> tuple:
    """Union of per-piece (keys int64, counts) device tensors with equal keys'
    counts summed (int64: a merged count may pass 2^32); keys ascending.  The
    statement, in torch, of what kf_sparse_merge computes pair by pair
    (counter.merge_sorted; keys below 2^63, where the signed sort is the unsigned
    order): the tests compare the kernel with it, no product path calls it."""
    import torch
    keys = torch.cat([p[0] for p in parts])
    cnts = torch.cat([p[1].to(torch.int64) & 0xFFFFFFFF for p in parts])
    if keys.numel() == 0:
        return keys, cnts
    ks, order = torch.sort(keys)
    u, inv = torch.unique_consecutive(ks, return_inverse=True)
    out = torch.zeros(u.numel(), dtype=torch.int64, device=keys.device).index_add_(0, inv, cnts[order])
    return u, out


KMERS_SLAB_BYTES = 32 << 20       # get_kmers: the device slab and each of the two pinned buffers of the row stream
DENSE_PRESENT_BINS = 1 << 28      # get_kmers k <= 12: count-matrix entries whose non-zero bins are taken at once


class _KmersNpyWriter:
    """get_kmers' `.npy` files made on the device (main.py:147-176): the matrices
    of a batch's genomes, packed back to back, leave kf_kmers_rows in slabs of
    KMERS_SLAB_BYTES; a slab is copied to one of two pinned buffers and written
    to the files it covers while the device fills and copies the next one.  A
    file is the v1.0 `.npy` header for (n, k + 1) '<f4' C-order followed by its
    rows: the bytes np.save writes for the same array.  Many small genomes share
    a slab; a large one takes many."""

    def __init__(self, k: int, device, output_dir: str):
        self.k, self.device, self.output_dir = k, device, output_dir
        self.slab_rows = max(1, KMERS_SLAB_BYTES // (4 * (k + 1)))
        self._bufs, self._cap = None, 0

    def _buffers(self, rows: int):
        """The device slab, the two pinned buffers, their status words and events,
        for slabs of min(rows, slab_rows) rows: a batch of small matrices does not
        pay for pinning whole slabs (the buffers grow at least 2x up to the slab)."""
        import torch
        cap = min(self.slab_rows, rows)
        if self._bufs is None or self._cap < cap:
            self._cap = min(self.slab_rows, max(cap, 2 * self._cap))
            m = self._cap * (self.k + 1)
            self._bufs = None
            self._bufs = (torch.empty(m, dtype=torch.float32, device=self.device),
                          [torch.empty(m, dtype=torch.float32, pin_memory=True) for _ in range(2)],
                          torch.zeros(2, dtype=torch.int32, pin_memory=True),
                          [torch.cuda.Event() for _ in range(2)])
        return self._bufs

    def write(self, names: list[str], keys, counts, src0, n) -> None:
        """Genome j's k-mers are keys[src0[j] : src0[j] + n[j]] (ascending standard
        codes, int64) with `counts` (int32 holding uint32, or int64), on the
        device; src0 and n on the host.  Prints what main.py:147-176 prints."""
        import torch
        from .counter import kmers_denominators, kmers_rows, kmers_tables
        k, w = self.k, self.k + 1
        n = np.asarray(n, dtype=np.int64)
        dst0 = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
        rows = int(dst0[-1])
        g, f = 0, None

        def emit(lo: int, hi: int, h) -> None:
            """The slab rows [lo, hi) (h: its floats on the host) to their files,
            and the lines of every genome that ends at or before hi."""
            nonlocal g, f
            while g < len(names):
                a, b = int(dst0[g]), int(dst0[g + 1])
                if a == b:
                    print(f"--- Processing {names[g]} ---")
                    print(f"Warning: No valid ATCG k-mers found in {names[g]}")
                    g += 1
                    continue
                if a >= hi:
                    return
                path = os.path.join(self.output_dir, f"{names[g]}_k{k}.npy")
                if f is None:
                    print(f"--- Processing {names[g]} ---")
                    f = open(path, "wb")
                    np.lib.format.write_array_header_1_0(f, {"descr": "<f4", "fortran_order": False,
                                                             "shape": (b - a, w)})
                x0, x1 = max(a, lo), min(b, hi)
                f.write(memoryview(h[(x0 - lo) * w: (x1 - lo) * w]))
                if x1 < b:
                    return
                f.close()
                f = None
                print(f"Saved: {path} (Shape: {(b - a, w)})")
                g += 1

        try:
            if rows:
                dslab, pin, pstat, ev = self._buffers(rows)
                S = self._cap
                tab = kmers_tables(src0, n, dst0, kmers_denominators(counts, src0, n), self.device)
                nslab = -(-rows // S)
                status = torch.empty(nslab, dtype=torch.int32, device=self.device)
                prev = None

                def drain(lo, hi, b):
                    ev[b].synchronize()
                    if int(pstat[b]) != 0:
                        raise N.NativeError("kf_kmers_rows: the device refused the segment tables")
                    emit(lo, hi, pin[b].numpy())

                for i in range(nslab):
                    lo, hi, b = i * S, min(rows, (i + 1) * S), i & 1
                    kmers_rows(keys, counts, tab, k, lo, hi, dslab, status[i: i + 1])
                    pin[b][: (hi - lo) * w].copy_(dslab[: (hi - lo) * w], non_blocking=True)
                    pstat[b: b + 1].copy_(status[i: i + 1], non_blocking=True)
                    ev[b].record(torch.cuda.current_stream(self.device))
                    if prev is not None:
                        drain(*prev)   # the file write of slab i - 1 overlaps the kernel and copy of slab i
                    prev = (lo, hi, b)
                drain(*prev)
            emit(rows, rows, None)   # genomes without k-mers at the end of the batch
        finally:
            if f is not None:
                f.close()


def get_kmers(args) -> None:
    """kf2vec/main.py:112-184 on the GPU (the *.fna of input_dir in batches).
    k <= 12: the dense counter's rows, non-zero bins kept; k = 13..31 (the rest
    of the reference's 2..31): the sparse counter (device radix sort of every
    window's canonical code, kf_sparse_count); a FASTA file above SPLIT_BYTES
    goes through it in pieces (fasta_pieces) whose sorted results are merged on
    the device (kf_sparse_merge, one running result per file), so no file size
    is refused.  The matrices are built on the
    device from the keys and counts (kf_kmers_rows) and streamed into the .npy
    files (_KmersNpyWriter); sparse_kmers_matrix / kmers_matrix above are the
    host statement of what it writes."""
    import glob

    import torch
    from .counter import KmerCounter, SparseCounter, dense_present, pack_files, to_device

    if not os.path.exists(args.output_dir):             # main.py:121-122
        os.makedirs(args.output_dir)
    fasta_files = glob.glob(os.path.join(args.input_dir, "*.fna"))   # main.py:124
    if not fasta_files:
        return
    device = torch.device(getattr(args, "device", None) or "cuda")
    sparse = args.k > N.KF_MAX_K
    if sparse:   # FASTQ content (first byte '@') is not cut: its record state does not split
        fq = [p for p in fasta_files if os.path.getsize(p) > SPLIT_BYTES and open(p, "rb").read(1) == b"@"]
        _refuse_huge_files(fq, "get_kmers -k {} (kf_sparse_count, FASTQ content)".format(args.k))
    counter = SparseCounter(args.k, device) if sparse else KmerCounter(args.k, device)
    batch_gb = float(getattr(args, "batch_gb", 4.0) or 4.0)
    budget = int(batch_gb * (1 << 30))
    if sparse:   # ~21 (k <= 16) / ~29 device bytes per input byte with the outputs; 32-bit offsets
        budget = min(budget, 1 << 30)
    # dense k <= 12: the count matrix takes 4 x bins per genome whatever its size
    # (33.6 MB at k=12): at most -batch_gb of it per batch
    cap = None if sparse else _count_cap(4 * counter.nbins, batch_gb)
    writer = _KmersNpyWriter(args.k, device, args.output_dir)
    if sparse and any(os.path.getsize(p) > SPLIT_BYTES for p in fasta_files):
        _get_kmers_pieces(args, fasta_files, counter, device, budget, writer)
        return
    for idx in _batches(fasta_files, budget, max_files=cap):
        paths = [fasta_files[i] for i in idx]
        names = [os.path.basename(p).replace(".fna", "") for p in paths]   # main.py:127
        hb = pack_files(paths, names, threads=host_threads(10))   # the reference's `jellyfish count -t 10`
        if sparse:
            keys, cnts, nu = counter.count(to_device(hb, device), int(hb.off[-1]))
            nuh = SparseCounter.nuniq_to_host(nu)              # raises the library's error
            writer.write(names, keys, cnts, hb.off[: hb.n].astype(np.int64), nuh)
            del keys, cnts, nu
        else:
            counts, _ = counter.count(to_device(hb, device))
            step = max(1, DENSE_PRESENT_BINS // counter.nbins)   # genomes whose non-zero bins are taken at once
            for g0 in range(0, len(names), step):
                keys, cnts, nuh, off = dense_present(counts[g0: g0 + step], args.k)
                writer.write(names[g0: g0 + step], keys, cnts, off, nuh)
            del counts


MERGE_COPY_DOWN = 8   # a merged result is copied down when at least 1/8 of its storage is slack


def _get_kmers_pieces(args, fasta_files: list[str], counter, device, budget: int, writer) -> None:
    """get_kmers' sparse path with files above SPLIT_BYTES: every file as its
    fasta_pieces, the pieces in batches of at most `budget` bytes.  Each
    unfinished file has ONE running (keys, counts) on the device: its first
    piece's slice of the batch's result as kf_sparse_count left it (u32 counts),
    and from its second piece on the union of its pieces so far (u64 counts),
    every further piece merged into it in file order straight from the batch's
    result (counter.merge_sorted, kf_sparse_merge: two inputs and one output, no
    sort).  The device so holds one running result per unfinished file plus one
    batch, not every piece of a file plus a sort of all of them.  A merge's
    output has room for n_a + n_b entries; when the pieces shared keys and at
    least 1/MERGE_COPY_DOWN of that room is slack, the result is copied down to
    its own size, so a running result never pins more than 8/7 of what it holds.
    A file that finishes is written as main.py:147-176 does (u32 or u64 counts go
    to the row kernel as they are); a file of one piece is written from the
    batch's result with no merge.  A first piece whose file continues in the next
    batch is the only slice that is copied out of a batch's result.
    _merge_sorted_counts above states what the merges compute."""
    from .counter import merge_sorted, merged_to_host, pack_ranges, to_device
    units = []                                    # (file index, start, end)
    for fi, p in enumerate(fasta_files):
        for a, e in fasta_pieces(p, args.k, SPLIT_BYTES):
            units.append((fi, a, e))
    last = {fi: j for j, (fi, _, _) in enumerate(units)}
    running: dict = {}                            # file index -> (keys, counts) of its pieces so far
    batch, size, done = [], 0, 0

    def finish(fi):
        k_, c_ = running.pop(fi)
        base_name = os.path.basename(fasta_files[fi]).replace(".fna", "")   # main.py:127
        writer.write([base_name], k_, c_, [0], [k_.numel()])

    def run(batch, j_next):
        """Count a batch, merge its pieces into their files' running results and
        write the files whose last piece lies before unit j_next."""
        nonlocal done
        hb = pack_ranges([(fasta_files[fi], a, e) for fi, a, e in batch], threads=host_threads(10))
        db = to_device(hb, device)
        keys, cnts, nu = counter.count(db, int(hb.off[-1]))
        nuh = counter.nuniq_to_host(nu)               # raises the library's error
        views = set()                                 # files whose running result is a slice of keys / cnts
        for j, (fi, _, _) in enumerate(batch):
            lo, m = int(hb.off[j]), int(nuh[j])
            kb, cb = keys[lo: lo + m], cnts[lo: lo + m]
            if fi not in running:
                running[fi] = (kb, cb)
                views.add(fi)
                continue
            ka, ca = running.pop(fi)
            views.discard(fi)
            k_, c_, n_out, status = merge_sorted(ka, ca, kb, cb)
            del ka, ca
            n = merged_to_host(n_out, status)         # raises the library's error
            room = k_.numel()                         # n_a + n_b
            k_, c_ = k_[:n], c_[:n]
            if (room - n) * MERGE_COPY_DOWN >= room:
                k_, c_ = k_.clone(), c_.clone()
            running[fi] = (k_, c_)
        while done < len(fasta_files) and last[done] < j_next:
            finish(done)
            views.discard(done)
            done += 1
        for fi in views:                              # continues in the next batch: let go of this batch's result
            running[fi] = tuple(t.clone() for t in running[fi])
        del keys, cnts, nu, db, hb

    for j, u in enumerate(units):
        n = u[2] - u[1]
        if batch and size + n > budget:
            run(batch, j)
            batch, size = [], 0
        batch.append(u)
        size += (n + 15) // 16 * 16
    if batch:
        run(batch, len(units))


# ---------------------------------------------------------------------------
# get_chunks (main.py:654-929): raw-count rows of 10 kbp windows per genome
# ---------------------------------------------------------------------------
def _hms(seconds: float) -> tuple[int, int, int]:
    m, s = divmod(int(seconds), 60)
    h, m = divmod(m, 60)
    return h, m, s


def get_chunks(args) -> None:
    """kf2vec/main.py:654-929 in batches of genome files: each batch is read and
    header-indexed by host threads, linearised / N-collapsed / gap-filtered on the
    device in one pass (kf_chunk_compact), its windows planned from one copy of
    the record bounds, gathered and counted in launches of bounded size, and
    written by a writer thread while the device counts the next launch -- instead
    of seqtk + awk + seqkit per genome and one Jellyfish pair per window.

    Log lines: the reference's per-genome lines ("Start processing", "Done chunk
    processing" or "Excluded ...", "Done computing k-mer frequences") come in its
    order, genome by genome, once the genome's rows are written (so a genome's
    three lines are logged together, after its batch is counted)."""
    import logging
    import time

    from . import chunks as CH
    from .counter import KmerCounter, pack_files, pack_ranges

    CH.TRACE = os.environ.get("KF_TRACE") == "1"
    since = time.time()
    if not os.path.exists(args.input_dir):
        print("No such directory '{}'".format(args.input_dir), file=sys.stderr)
        sys.exit(0)
    if not os.path.exists(args.output_dir):
        print("No such directory '{}'".format(args.output_dir), file=sys.stderr)
        sys.exit(0)
    log = logging.getLogger("kf2vecfsw_amd.get_chunks")
    log.setLevel(logging.INFO)
    log.handlers[:] = [logging.FileHandler(os.path.join(args.output_dir, "get_chunks_{}.log".format(
        os.path.basename(os.path.normpath(args.input_dir)))), "w+"), logging.StreamHandler(sys.stdout)]
    for h in log.handlers:
        h.setFormatter(logging.Formatter("%(message)s"))

    def stamp(msg):
        hrs, _min, sec = _hms(time.time() - since)
        log.info(msg + " Time: {:02d}:{:02d}:{:02d}\n".format(hrs, _min, sec))

    stamp("\n==> Making a list of sample names.")
    files_names, samples_names = list_inputs(args.input_dir)
    stamp("\n==> Start processing samples.")
    if args.k not in supported_k:
        raise ValueError("k={} has no vocabulary: supported k are {}..{}".format(
            args.k, supported_k.start, supported_k.stop - 1))
    import torch
    device = torch.device(getattr(args, "device", None) or "cuda")
    counter = KmerCounter(args.k, device)
    budget = int(float(getattr(args, "batch_gb", 1.0) or 1.0) * (1 << 30))
    # windows per count launch: the window bytes AND the count matrix (4 x bins
    # per window, 8 MiB at k=11) within the budget
    # and at most CH.LAUNCH_WINDOWS, so the writer formats one launch while the
    # device counts and copies back the next
    max_windows = max(1, min(budget // CH.CHUNK_SZ, budget // (4 * counter.nbins), CH.LAUNCH_WINDOWS))
    threads = host_threads(args.p)
    pipe = CH.ChunkPipeline(counter, device, max_windows, threads, args.pseudocount)
    paths = [os.path.join(args.input_dir, f) for f in files_names]
    # units: whole files, or the record-aligned parts of a file above SPLIT_BYTES
    # (each part below kf_chunk_compact's 32-bit offsets; a single record of 4 GiB
    # or more is refused before anything is written)
    units = []   # (file index, start, end, part, parts)
    for fi, p in enumerate(paths):
        pcs = record_pieces(p)
        for j, (a, e) in enumerate(pcs):
            if e - a > MAX_CALL_BYTES - 16:
                raise ValueError("get_chunks (kf_chunk_compact): a FASTA record of 4 GiB or more is not supported "
                                 "(per-call 32-bit offsets): {} at byte {}".format(files_names[fi], a))
            units.append((fi, a, e, j, len(pcs)))
    # input batches of units: about a quarter of the input each (the first two
    # smaller, so the writer starts sooner), so that reading and preparing one
    # batch overlaps writing the previous one, within the budget (and below 4 GiB
    # of processed sequence: kf_chunk_compact's offsets)
    usz = [e - a for _, a, e, _, _ in units]
    batches = _size_batches(usz, min(budget, 3 << 30, max(sum(usz) // 4, 16 << 20)), ramp=True)
    files_pool = ThreadPoolExecutor(max_workers=threads)
    reader = ThreadPoolExecutor(max_workers=1)

    def read(idx):
        t0 = time.perf_counter()
        us = [units[u] for u in idx]
        names = [samples_names[fi] for fi, _, _, _, _ in us]
        if all(n == 1 for *_, n in us):
            hb = pack_files([paths[fi] for fi, *_ in us], names, fmt=N.KF_FMT_FASTA, pool=files_pool)
        else:
            hb = pack_ranges([(paths[fi], a, e) for fi, a, e, _, _ in us], names, threads=threads, index=True)
        CH._tr("read", t0, files=len(idx))
        return hb

    # a file in several parts: windows and long contigs so far; written to a
    # side file that replaces <sample>.kf after its last part (or is removed if
    # the file is excluded or a later file of the same name replaces it)
    acc: dict = {}

    def settle(genomes, us):
        """The parts' exclusions and names; returns the side-file steps for the
        writer: (before this batch's rows) a stale side file of a file whose first
        part is here removed, (after them) the move of a file whose last part is."""
        lasts, first = [], []
        for gm, (fi, _a, _e, j, n) in zip(genomes, us):
            if n == 1:
                continue
            if j == 0:
                first.append(os.path.join(args.output_dir, "{}.kf.parts".format(gm.sample)))
            nw, longc = acc.get(fi, (0, False))
            nw, longc = nw + gm.n_windows, longc or gm.n_windows > 0
            acc[fi] = (nw, longc)
            gm.out_name = "{}.kf.parts".format(gm.sample)
            gm.cont, gm.last = j > 0, j == n - 1
            if not gm.last:
                gm.excluded = None    # decided by the last part
                continue
            gm.total_windows = nw
            gm.excluded = "none" if not longc else ("few" if nw < CH.CHUNK_CNT_THR else None)
            lasts.append(gm)
        CH.shadow(genomes)
        moves = []
        for gm in lasts:
            side = os.path.join(args.output_dir, gm.out_name)
            final = os.path.join(args.output_dir, "{}.kf".format(gm.sample))

            def move(side=side, final=final, keep=gm.excluded is None and gm.write):
                if keep:
                    os.replace(side, final)
                elif os.path.exists(side):
                    os.remove(side)
            moves.append(move)

        def clear(paths=first):
            for p in paths:
                if os.path.exists(p):
                    os.remove(p)
        return clear, moves

    def report(genomes):
        for gm in genomes:
            if not gm.last:
                continue
            log.info("\n==> Start processing. Sample: {}".format(gm.fname))                   # main.py:703
            log.info(">>> Formatting to single line. Sample: {}".format(gm.fname))            # :728
            log.info(">>> Replacing stretches of N. Sample: {}".format(gm.fname))             # :737
            log.info(">>> Filtering contigs below threshold {}. Sample: {}".format(CH.CHUNK_SZ, gm.fname))   # :746
            if gm.excluded == "none":                                                         # :761-778
                stamp("\n==> Excluded {}. No contigs above threshold length.".format(gm.fname))
                continue
            log.info(">>> Splitting into contigs. Sample: {}".format(gm.fname))               # :783
            log.info(">>> Getting contig ids. Sample: {}".format(gm.fname))                   # :789
            log.info(">>> Computing contig statistics. Sample: {}".format(gm.fname))          # :799
            if gm.excluded == "few":                                                          # :845-860
                stamp("\n==> Excluded {}. {} chunks is too low. {} is required.".format(
                    gm.fname, gm.n_windows if gm.total_windows is None else gm.total_windows, CH.CHUNK_CNT_THR))
                continue
            stamp("\n==> Done chunk processing for {}.".format(gm.fname))                    # :866
            # the reference runs get_frequencies on the genome's chunk directory here
            # (main.py:869-881), which prints its first and last lines to stdout
            chunk_dir = os.path.join(args.output_dir, "{}_chunks".format(gm.sample))
            print("\n==> Starting k-mer counting for {}\n".format(chunk_dir))
            print("\n==> Done processing {}".format(chunk_dir))
            stamp("\n==> Done computing k-mer frequences for {}.".format(gm.fname))          # :885

    nxt = reader.submit(read, batches[0]) if batches else None
    prev = None   # (genomes, write futures) of the previous batch, logged once written
    for bi, idx in enumerate(batches):
        t0 = time.perf_counter()
        hb = nxt.result()
        CH._tr("wait_read", t0, batch=bi)
        if bi + 1 < len(batches):
            nxt = reader.submit(read, batches[bi + 1])
        genomes = [CH.Genome(files_names[units[u][0]], samples_names[units[u][0]]) for u in idx]
        d_seq = pipe.prepare(hb, genomes)
        clear, moves = settle(genomes, [units[u] for u in idx])
        t0 = time.perf_counter()
        pipe.after_writes(clear)
        futs = pipe.count_and_write(d_seq, genomes, args.output_dir)
        futs += [pipe.after_writes(f) for f in moves]   # in the writer's order: before the next batch's writes
        CH._tr("issue_counts", t0, launches=len(futs))
        del hb, d_seq
        if prev is not None:
            for f in prev[1]:
                f.result()
            report(prev[0])
        prev = (genomes, futs)
    if prev is not None:
        for f in prev[1]:
            f.result()
        report(prev[0])
    pipe.close()
    reader.shutdown()
    files_pool.shutdown()
    stamp("\n==> Done getting chunks.")
    if CH.TRACE:
        import json
        print(json.dumps({"kf_chunks_trace": CH.trace}), file=sys.stderr)
        CH.trace.clear()


def query(args) -> None:
    """`query`: distances to the backbone and embeddings of the queries, computed
    and written as text on the device (query.query_func; kf2vec/main.py:535-553)."""
    from . import query as Q
    Q.query(args)


def classify(args) -> None:
    """`classify`: the clade of every query, its probabilities computed and
    written as text on the device (classify.classify_func; kf2vec/main.py:400-411)."""
    from . import classify as CL
    CL.classify(args)


def train_model_set(args) -> None:
    """`train_model_set`: the distance model of every clade, trained on the
    device with kf_dist_loss (train.train_model_set_func; kf2vec/main.py:506-531).
    Only the NeuralNet model (-no_fsw) is trained."""
    from . import train as TR
    TR.train_model_set(args)


def train_model_set_chunks(args) -> None:
    """`train_model_set_chunks`: the distance model of every clade, trained on
    random runs of its genomes' 10-kbp windows with kf_chunk_features and
    kf_dist_loss_views (train_chunks.train_model_set_chunks_func;
    kf2vec/main.py:934-957)."""
    from . import train_chunks as TC
    TC.train_model_set_chunks(args)


def train_classifier(args) -> None:
    """`train_classifier`: the clade classifier of a library, trained on the
    device with kf_class_loss (train_classifier.train_classifier_model_func;
    kf2vec/main.py:376-397)."""
    from . import train_classifier as TC
    TC.train_classifier(args)


def train_classifier_chunks(args) -> None:
    """`train_classifier_chunks`: the clade classifier of a library, trained on
    random runs of its genomes' 10-kbp windows with kf_chunk_features (under
    -cap kf_chunk_features8 over a uint8 store) and kf_class_loss
    (train_classifier_chunks.train_classifier_model_chunks_func;
    kf2vec/main.py:960-967)."""
    from . import train_classifier_chunks as TCC
    TCC.train_classifier_chunks(args)


def process_query_data(args) -> None:
    """`process_query_data`: get_frequencies, classify and query one after
    another in this process, with the reference's banner lines and its rewiring
    of the arguments (kf2vec/main.py:626-651).  The stages hand over through the
    `.kf` files and classes.out in -output_dir."""
    print("\n==> Computing k-mer frequences\n")
    get_frequencies(args)

    print("\n==> Classifying query samples\n")
    args.input_dir = args.output_dir
    args.model = args.classifier_model
    args.seed = args.cl_seed
    args.o = args.output_dir
    classify(args)

    print("\n==> Computing model distances\n")
    args.model = args.distance_model
    args.classes = args.output_dir
    args.seed = args.di_seed
    query(args)

    print("\n==> Query processing step is completed!\n")


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description="K-mer frequency to distance\n{}".format(__version__),
                                     formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("-v", "--version", action="version", version="{}".format(__version__))
    sub = parser.add_subparsers(title="commands", dest="{commands}",
                                description="get_kmers                Extract k-mers and their frequencies from "
                                            "FASTA files\n"
                                            "get_frequencies          Extract k-mer frequency from a reference "
                                            "genome-skims or assemblies\n"
                                            "get_chunks               Extract chunks from reference assemblies\n"
                                            "train_classifier         Train classifier model based on backbone "
                                            "subtrees\n"
                                            "train_classifier_chunks  Train classifier model based on backbone "
                                            "subtrees (genomes split into chunks)\n"
                                            "train_model_set          Trains individual models for each subtree\n"
                                            "train_model_set_chunks   Trains individual models for each subtree "
                                            "using chunked genomes as input\n"
                                            "classify                 Classifies query samples using previously "
                                            "trained classifier model\n"
                                            "query                    Query models\n"
                                            "process_query_data       Wrapper command to preprocess query sequences, "
                                            "classify and compute distances to backbone species\n")
    pf = sub.add_parser("get_frequencies", description="Process a library of reference genome-skims or assemblies")
    pf.add_argument("-input_dir", help="Directory of input genomes or assemblies "
                                       "(dir of .fastq/.fq/.fa/.fna/.fasta files)")
    pf.add_argument("-output_dir", help="Directory for k-mer frequency outputs (dir for .kf files)")
    pf.add_argument("-k", type=int, choices=list(range(min_k_len, max_k_len + 1)), default=default_k_len,
                    help="K-mer length [{}-{}]. Default: {}".format(min_k_len, max_k_len, default_k_len),
                    metavar="K")
    pf.add_argument("-p", type=int, choices=list(range(1, mp.cpu_count() + 1)), default=mp.cpu_count(),
                    help="Max number of processors to use [1-{0}]. Default for this machine: {0}".format(
                        mp.cpu_count()), metavar="P")
    pf.add_argument("-pseudocount", action="store_true",
                    help="Computes k-mer counts with 0.5 pseudocount added to each frequency value")
    pf.add_argument("-raw_cnt", action="store_true", help="Computes raw k-mer counts without normalization")
    pf.add_argument("-batch_gb", type=float, default=None,
                    help="Input bytes per device batch (GiB). Default: about a quarter of the input, 16 MiB..4 GiB")
    pf.add_argument("-split_gb", type=float, default=SPLIT_GB,
                    help="A file larger than this (GiB) is counted in pieces of about min(this, 1) GiB, summed on "
                         "the device, so no batch grows with a file. 0 never splits. Default: {:g}".format(SPLIT_GB))
    pf.add_argument("-device", default=None, help="torch device (default: cuda)")
    pf.add_argument("-gpus", type=int, default=1,
                    help="GPUs to shard the files over, one process each (0 = every visible GPU). Default: 1. "
                         "Under torchrun each rank counts its own shard.")
    pf.set_defaults(func=get_frequencies)

    pk = sub.add_parser("get_kmers", description="Extract kmers and frequencies from FASTA files")
    pk.add_argument("-input_dir", help="Directory of input genomes or assemblies (dir of .fna files)")
    pk.add_argument("-output_dir", help="Directory for k-mer outputs (.npy files)")
    pk.add_argument("-k", type=int, choices=list(range(min_k_len, max_k_len + 1)), default=default_k_len,
                    help="K-mer length [{}-{}]. Default: {}".format(min_k_len, max_k_len, default_k_len),
                    metavar="K")
    pk.add_argument("-batch_gb", type=float, default=4.0, help="Input bytes per device batch (GiB)")
    pk.add_argument("-device", default=None, help="torch device (default: cuda)")
    pk.set_defaults(func=get_kmers)

    pc = sub.add_parser("get_chunks", description="Extract chunks from reference assemblies")
    pc.add_argument("-input_dir", help="Directory of input genomes or assemblies")
    pc.add_argument("-output_dir", help="Directory for chunked k-mer counts (.kf files)")
    pc.add_argument("-k", type=int, choices=list(range(min_k_len, max_k_len + 1)), default=default_k_len,
                    help="K-mer length [{}-{}]. Default: {}".format(min_k_len, max_k_len, default_k_len),
                    metavar="K")
    pc.add_argument("-p", type=int, choices=list(range(1, mp.cpu_count() + 1)), default=mp.cpu_count(),
                    help="Max number of processors to use", metavar="P")
    pc.add_argument("-pseudocount", action="store_true",
                    help="Computes k-mer counts with 0.5 pseudocount added to each frequency value")
    pc.add_argument("-batch_gb", type=float, default=1.0, help="Window bytes per device batch (GiB)")
    pc.add_argument("-device", default=None, help="torch device (default: cuda)")
    pc.set_defaults(func=get_chunks)

    pa = sub.add_parser("train_classifier", description="Train classifier model based on backbone subtrees")
    pa.add_argument("-input_dir", help="Directory of input k-mer frequencies for assemblies or reads "
                                       "(dir of .kf files for backbone)")
    pa.add_argument("-subtrees", help="Classification file with subtrees information obtained from divide_tree "
                                      "command (a .subtrees format)")
    pa.add_argument("-e", type=int, default=default_cl_epochs,
                    help="Number of epochs. Default: {}".format(default_cl_epochs))
    pa.add_argument("-hidden_sz", type=int, default=default_hidden_sz,
                    help="Hidden size. Default: {}".format(default_hidden_sz))
    pa.add_argument("-batch_sz", type=int, default=default_batch_sz,
                    help="Batch size. Default: {}".format(default_batch_sz))
    pa.add_argument("-lr", type=float, default=default_lr, help="Start learning rate. Default: {}".format(default_lr))
    pa.add_argument("-lr_min", type=float, default=default_lr_min,
                    help="Minimum learning rate. Default: {}".format(default_lr_min))
    pa.add_argument("-lr_decay", type=float, default=default_lr_decay,
                    help="Learning rate decay. Default: {}".format(default_lr_decay))
    pa.add_argument("-seed", type=int, default=default_seed, help="Random seed. Default: {}".format(default_seed))
    pa.add_argument("-mask", action="store_true", help=argparse.SUPPRESS)
    pa.add_argument("-o", help="Model output path")
    pa.add_argument("-device", default=None, help="torch device (default: cuda)")
    pa.set_defaults(func=train_classifier)

    pb = sub.add_parser("train_classifier_chunks",
                        description="Train classifier model based on backbone subtrees (genomes split into chunks)")
    pb.add_argument("-input_dir", help="Directory of input k-mer frequencies for assemblies or reads "
                                       "(dir of .kf files for backbone)")
    pb.add_argument("-input_dir_fullgenomes", help="Directory of input k-mer frequencies for full assemblies "
                                                   "(dir of .kf files for full backbone species)")
    pb.add_argument("-subtrees", help="Classification file with subtrees information obtained from divide_tree "
                                      "command (a .subtrees format)")
    pb.add_argument("-e", type=int, default=default_cl_epochs,
                    help="Number of epochs. Default: {}".format(default_cl_epochs))
    pb.add_argument("-hidden_sz", type=int, default=default_hidden_sz,
                    help="Hidden size. Default: {}".format(default_hidden_sz))
    pb.add_argument("-batch_sz", type=int, default=default_batch_sz,
                    help="Batch size. Default: {}".format(default_batch_sz))
    pb.add_argument("-lr", type=float, default=default_lr, help="Start learning rate. Default: {}".format(default_lr))
    pb.add_argument("-lr_min", type=float, default=default_lr_min,
                    help="Minimum learning rate. Default: {}".format(default_lr_min))
    pb.add_argument("-lr_decay", type=float, default=default_lr_decay,
                    help="Learning rate decay. Default: {}".format(default_lr_decay))
    pb.add_argument("-seed", type=int, default=default_seed, help="Random seed. Default: {}".format(default_seed))
    pb.add_argument("-mask", action="store_true", help=argparse.SUPPRESS)
    pb.add_argument("-cap", action="store_true",
                    help="Reduces memory consumption for input dataset (caps k-mer counts at a maximum of 255, kept "
                         "as one byte each)")
    pb.add_argument("-o", help="Model output path")
    pb.add_argument("-device", default=None, help="torch device (default: cuda)")
    pb.set_defaults(func=train_classifier_chunks)

    pt = sub.add_parser("train_model_set", description="Trains individual models for each subtree")
    pt.add_argument("-input_dir", help="Directory of input k-mer frequencies for assemblies or reads "
                                       "(dir of .kf files for backbone)")
    pt.add_argument("-test_set", help="File that contains list of filenames (no extension) to be used as a test set "
                                      "(list of .kf files for test subset)")
    pt.add_argument("-true_dist", help="Directory of distamce matrices for backbone subtrees "
                                       "(dir of *subtree_INDEX.di_mtrx files for backbone)")
    pt.add_argument("-subtrees", help="Classification file with subtrees information obtained from divide_tree "
                                      "command (a .subtrees format)")
    pt.add_argument("-e", type=int, default=default_di_epochs,
                    help="Number of epochs. Default: {}".format(default_di_epochs))
    pt.add_argument("-hidden_sz", type=int, default=default_hidden_sz,
                    help="Hidden size. Default: {}".format(default_hidden_sz))
    pt.add_argument("-embed_sz", type=int, default=default_embed_sz,
                    help="Embedding size. Default: {}".format(default_embed_sz))
    pt.add_argument("-batch_sz", type=int, default=default_batch_sz,
                    help="Batch size. Default: {}".format(default_batch_sz))
    pt.add_argument("-lr", type=float, default=default_lr, help="Start learning rate. Default: {}".format(default_lr))
    pt.add_argument("-lr_min", type=float, default=default_lr_min,
                    help="Minimum learning rate. Default: {}".format(default_lr_min))
    pt.add_argument("-lr_decay", type=float, default=default_lr_decay,
                    help="Learning rate decay. Default: {}".format(default_lr_decay))
    pt.add_argument("-clade", type=int, nargs="*", help="Clade number to train. Default: all")
    pt.add_argument("-save_interval", type=int, help="Save model after specified interval of epochs. Default: last")
    pt.add_argument("-seed", type=int, default=default_seed, help="Random seed. Default: {}".format(default_seed))
    pt.add_argument("-o", help="Model output path")
    pt.add_argument("-no_fsw", action="store_true", help="Keep original model (the only one trained here: the FSW "
                                                         "model needs fswlib)")
    pt.add_argument("-fswout_dim", type=int, default=512)
    pt.add_argument("-base_dim", type=int, default=4)
    pt.add_argument("-device", default=None, help="torch device (default: cuda)")
    pt.set_defaults(func=train_model_set)

    ph = sub.add_parser("train_model_set_chunks",
                        description="Trains individual models for each subtree using chunked genomes as input")
    ph.add_argument("-input_dir", help="Directory of input k-mer frequencies for chunked assemblies "
                                       "(dir of .kf files for chunked backbone species)")
    ph.add_argument("-input_dir_fullgenomes", help="Directory of input k-mer frequencies for full assemblies "
                                                   "(dir of .kf files for full backbone species)")
    ph.add_argument("-true_dist", help="Directory of distamce matrices for backbone subtrees "
                                       "(dir of *subtree_INDEX.di_mtrx files for backbone)")
    ph.add_argument("-subtrees", help="Classification file with subtrees information obtained from divide_tree "
                                      "command (a .subtrees format)")
    ph.add_argument("-e", type=int, default=default_di_epochs,
                    help="Number of epochs. Default: {}".format(default_di_epochs))
    ph.add_argument("-hidden_sz", type=int, default=default_hidden_sz,
                    help="Hidden size. Default: {}".format(default_hidden_sz))
    ph.add_argument("-embed_sz", type=int, default=default_embed_sz,
                    help="Embedding size. Default: {}".format(default_embed_sz))
    ph.add_argument("-batch_sz", type=int, default=default_batch_sz,
                    help="Batch size. Default: {}".format(default_batch_sz))
    ph.add_argument("-lr", type=float, default=default_lr, help="Start learning rate. Default: {}".format(default_lr))
    ph.add_argument("-lr_min", type=float, default=default_lr_min,
                    help="Minimum learning rate. Default: {}".format(default_lr_min))
    ph.add_argument("-lr_decay", type=float, default=default_lr_decay,
                    help="Learning rate decay. Default: {}".format(default_lr_decay))
    ph.add_argument("-clade", type=int, nargs="*", help="Clade number to train. Default: all")
    ph.add_argument("-seed", type=int, default=default_seed, help="Random seed. Default: {}".format(default_seed))
    ph.add_argument("-cap", action="store_true",
                    help="Caps k-mer counts of every window at a maximum of 255")
    ph.add_argument("-o", help="Model output path")
    ph.add_argument("-device", default=None, help="torch device (default: cuda)")
    ph.set_defaults(func=train_model_set_chunks)

    pq = sub.add_parser("query", description="Query models")
    pq.add_argument("-input_dir", help="Directory of input k-mer frequencies for assemblies or reads "
                                       "(dir of .kf files for queries)")
    pq.add_argument("-model", help="Directory of models and embeddings (dir of model_subtree_INDEX.ckpt and "
                                   "embeddings_subtree_INDEX.csv files for backbone)")
    pq.add_argument("-classes", help="Path to classification file with subtrees information obtained from classify "
                                     "command (classes.out file)")
    pq.add_argument("-block", type=int, default=default_block_sz,
                    help="Block size for file processing. Default: {}".format(default_block_sz))
    pq.add_argument("-seed", type=int, default=default_seed, help="Random seed. Default: {}".format(default_seed))
    pq.add_argument("-remap", help='Remap file with alternative output names ("label" and "new_label" columns in '
                                   ".tsv format)")
    pq.add_argument("-o", help="Output path")
    pq.add_argument("-device", default=None, help="torch device (default: cuda)")
    pq.set_defaults(func=query)

    pl = sub.add_parser("classify", description="Classifies query inputs using previously trained classifier model")
    pl.add_argument("-input_dir", help="Directory of input k-mer frequencies for queries samples: assemblies or reads "
                                       "(dir of .kf files for queries)")
    pl.add_argument("-model", help="Classification model")
    pl.add_argument("-block", type=int, default=default_block_sz,
                    help="Block size for file processing. Default: {}".format(default_block_sz))
    pl.add_argument("-seed", type=int, default=default_seed, help="Random seed. Default: {}".format(default_seed))
    pl.add_argument("-o", help="Output path")
    pl.add_argument("-device", default=None, help="torch device (default: cuda)")
    pl.set_defaults(func=classify)

    pp = sub.add_parser("process_query_data",
                        description="Wrapper command that combines subcommands: get_frequencies (from query samples), "
                                    "classify and query. The reference's parser defines neither -raw_cnt, -block nor "
                                    "-remap, which its get_frequencies, classify and query read, so the command "
                                    "cannot run there; here the three options exist, with the values the "
                                    "subcommands default to.")
    pp.add_argument("-input_dir", help="Directory of input genomes or assemblies "
                                       "(dir of .fastq/.fq/.fa/.fna/.fasta files)")
    pp.add_argument("-output_dir", help="Directory for outputs (dir for .kf files)")
    pp.add_argument("-k", type=int, choices=list(range(3, 11)), default=default_k_len,
                    help="K-mer length [3-10]. Default: {}".format(default_k_len), metavar="K")
    pp.add_argument("-p", type=int, choices=list(range(1, mp.cpu_count() + 1)), default=mp.cpu_count(),
                    help="Max number of processors to use [1-{0}]. Default for this machine: {0}".format(
                        mp.cpu_count()), metavar="P")
    pp.add_argument("-pseudocount", action="store_true",
                    help="Computes k-mer counts with 0.5 pseudocount added to each frequency value")
    pp.add_argument("-classifier_model", help="Classification model path")
    pp.add_argument("-cl_seed", type=int, default=default_seed,
                    help="Clssification random seed. Default: {}".format(default_seed))
    pp.add_argument("-distance_model", help="Directory of models and embeddings (dir of model_subtree_INDEX.ckpt and "
                                            "embeddings_subtree_INDEX.csv files for backbone)")
    pp.add_argument("-di_seed", type=int, default=default_seed,
                    help="Query random seed. Default: {}".format(default_seed))
    pp.add_argument("-raw_cnt", action="store_true",
                    help="Computes raw k-mer counts without normalization (not in the reference's parser, which "
                         "get_frequencies needs)")
    pp.add_argument("-block", type=int, default=default_block_sz,
                    help="Block size for file processing in classify and query (not in the reference's parser). "
                         "Default: {}".format(default_block_sz))
    pp.add_argument("-remap", help='Remap file with alternative output names for query ("label" and "new_label" '
                                   "columns in .tsv format; not in the reference's parser)")
    pp.add_argument("-device", default=None, help="torch device (default: cuda)")
    pp.set_defaults(func=process_query_data)
    return parser


_PARSER: list = []   # (mp.cpu_count() it was built for, parser)


def _parser() -> argparse.ArgumentParser:
    """build_parser(), kept for later calls in the process (a library caller that
    runs the CLI per directory; building it costs ~1-3 ms), rebuilt if the CPU
    count its -p choices were made for has changed."""
    n = mp.cpu_count()
    if not _PARSER or _PARSER[0][0] != n:
        _PARSER[:] = [(n, build_parser())]
    return _PARSER[0][1]


def main(argv=None) -> None:
    parser = _parser()
    args = parser.parse_args(argv)
    if os.environ.get("KF_SHARD"):
        # a -gpus child shares its parent's stdout with the other shards: one
        # write per line, so concurrent shards never split each other's lines
        sys.stdout.reconfigure(line_buffering=True)
    if hasattr(args, "func"):
        args.func(args)
    else:
        parser.print_help()


if __name__ == "__main__":
    main()
