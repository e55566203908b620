"""CPU side of the device FASTQ index (kf_index_fastq): the C-ABI's argument
checks, pack_files(index=False) on FASTQ batches, and the design claim the
kernels rest on -- for a genome in the regular four-line form the host state
machine (kf_index_records) excludes exactly the lines whose number mod 4 is not
1 -- checked against the host index on seeded inputs."""
import ctypes

import numpy as np

import fastq_model as M
import gen


def test_index_fastq_symbols_and_einval(native):
    """The entry points exist and refuse bad arguments before any launch (so
    this runs without a GPU): n_genomes < 0, a null count pointer, a null status
    pointer, each with a message."""
    from kf2vecfsw_amd import _native as N
    assert native.kf_index_fastq_scratch_bytes(1 << 20, 3, 1000) >= 8 * (1000 + 256 + 4 * 3)
    assert native.kf_index_fastq_scratch_bytes(1 << 20, -1, 1000) == 0
    cnt = (ctypes.c_uint64 * 2)()
    st = (ctypes.c_uint32 * 4)()
    rc = native.kf_index_fastq(None, None, -1, 0, None, 0, 0, cnt, st, None, 0, None)
    assert rc == N.KF_EINVAL and b"n_genomes" in native.kf_last_error()
    rc = native.kf_index_fastq(None, None, 1, 64, None, 0, 0, None, st, None, 0, None)
    assert rc == N.KF_EINVAL and b"null" in native.kf_last_error()
    rc = native.kf_index_fastq(None, None, 1, 64, None, 0, 0, cnt, None, None, 0, None)
    assert rc == N.KF_EINVAL and b"null" in native.kf_last_error()
    rc = native.kf_index_fastq(None, None, 1, 64, None, 0, 0, cnt, st, None, 0, None)   # no batch, no scratch
    assert rc == N.KF_EINVAL and b"null" in native.kf_last_error()


def test_pack_files_fastq_without_index(native, tmp_path):
    """pack_files(index=False): a batch whose non-empty files are all FASTQ comes
    back unindexed with the fastq flag (the device indexes it), by the sniff and
    by fmt=KF_FMT_FASTQ; seq_chars() indexes it with FASTQ rules."""
    from kf2vecfsw_amd import _native as N
    from kf2vecfsw_amd import counter as C
    rng = np.random.default_rng(7)
    paths = []
    for i, b in enumerate([gen.random_fastq(rng, 20), b"", gen.random_fastq(rng, 5)]):
        p = tmp_path / f"s{i}.fq"
        p.write_bytes(b)
        paths.append(str(p))
    ref = C.pack_files(paths, pin=False, threads=1)
    assert ref.excl is not None and not ref.fastq
    for fmt in (N.KF_FMT_AUTO, N.KF_FMT_FASTQ):
        hb = C.pack_files(paths, pin=False, threads=1, index=False, fmt=fmt)
        assert hb.excl is None and hb.fastq and hb.n == 3
        assert hb.seq_chars() == ref.seq_chars() > 0
    # positional construction keeps working and means FASTA
    assert not C.HostBatch(ref.data, ref.off, None, ref.names).fastq


def test_pack_files_mixed_batch_stays_on_host(native, tmp_path):
    """A batch that mixes FASTA and FASTQ is indexed on the host as before."""
    from kf2vecfsw_amd import counter as C
    fa = tmp_path / "a.fna"
    fa.write_bytes(b">a\nACGT\n>b\nGG\n")
    fq = tmp_path / "c.fq"
    fq.write_bytes(b"@r1\nACGT\n+\nIIII\n")
    mixed = C.pack_files([str(fa), str(fq)], pin=False, threads=1, index=False)
    ref = C.pack_files([str(fa), str(fq)], pin=False, threads=1)
    assert mixed.excl is not None and not mixed.fastq and np.array_equal(mixed.excl, ref.excl)
    only_fa = C.pack_files([str(fa)], pin=False, threads=1, index=False)
    assert only_fa.excl is None and not only_fa.fastq


def _inputs(n: int):
    """Seeded FASTQ inputs: plain four-line, multi-line, and either with 1-3
    random byte edits, a truncation or a run of trailing newlines."""
    rng = np.random.default_rng(2024)
    alphabet = b"\n\n\n@++ACGTI\r!~"
    for i in range(n):
        b = gen.random_fastq(rng, int(rng.integers(0, 7)), multiline=(i % 3 == 1))
        if i % 3 == 2 and b:
            kind = int(rng.integers(0, 3))
            if kind == 0:
                a = bytearray(b)
                for _ in range(int(rng.integers(1, 4))):
                    a[int(rng.integers(0, len(a)))] = alphabet[int(rng.integers(0, len(alphabet)))]
                b = bytes(a)
            elif kind == 1:
                b = b[: int(rng.integers(0, len(b) + 1))]
            else:
                b = b + b"\n" * int(rng.integers(1, 20))
        yield b


def test_regular_fastq_is_the_line_rule(native):
    """On every regular input the host index, the line-mod-4 rule and the pairs
    computed the way the kernels compute them exclude the same bytes (newlines
    aside); the pairs are sorted, disjoint and non-empty."""
    from kf2vecfsw_amd import _native as N
    from kf2vecfsw_amd import counter as C
    total = regular = 0
    for b in _inputs(2400):
        total += 1
        if not M.is_regular(b):
            continue
        regular += 1
        d = np.frombuffer(b, np.uint8)
        host, _ = C.index_records(d, N.KF_FMT_FASTQ, 0)
        nl = d == 10
        want = M.mask_of(host, len(b)) & ~nl
        assert np.array_equal(M.rule_mask(b) & ~nl, want), b
        pairs = M.device_pairs(b)
        assert np.array_equal(M.mask_of(pairs, len(b)) & ~nl, want), b
        p = np.asarray(pairs, np.int64)
        assert np.all(p[1::2] > p[0::2]) and np.all(p[2::2] >= p[1:-1:2]) and (not p.size or p[-1] <= len(b)), b
        records = sum(1 for j, (s, e) in enumerate(M.split_lines(b)) if j % 4 == 2)
        assert p.size // 2 == (records + 1 if M.split_lines(b) else 0), b
    assert total >= 2000 and 3 * regular >= total, (regular, total)


def test_plain_generator_is_regular_and_multiline_is_not():
    """Both sides of the device path are covered by tests/gen.py: its plain FASTQ
    is always regular, its multi-line FASTQ almost never."""
    rng = np.random.default_rng(5)
    assert all(M.is_regular(gen.random_fastq(rng, int(rng.integers(0, 30)))) for _ in range(100))
    assert sum(M.is_regular(gen.random_fastq(rng, 10, multiline=True)) for _ in range(50)) < 5
