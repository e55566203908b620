"""CPU tests of get_chunks' pre-pass, kf_chunk_compact / kf_chunk_gather
(csrc/kf_chunks.hip): the host statement chunks.compact_records_host against a
per-byte model of the kernel's rule on the whole corpus of
tests/chunk_corpus.py, the proof that the corpus tells each of nine subtly
wrong rules from the right one, the statement against the oracle's seqtk / awk /
seqkit restatement, and the entry points' refusals (all before any launch).
tests/test_gpu_chunk_compact.py compares the kernels with the same statement
on the same corpus."""
import re

import numpy as np
import pytest

import chunk_corpus as CC
import chunk_model as CM
import gen


def _records(out: bytes, out_se) -> list[bytes]:
    return [out[int(out_se[2 * r]): int(out_se[2 * r + 1])] for r in range(len(out_se) // 2)]


@pytest.mark.parametrize("g", CC.GROUPS)
def test_model_equals_statement(g):
    """The per-byte rule (look-back and all) and the regular-expression statement
    give the same bytes and the same offsets on every case of the corpus."""
    cases, exp = CC.group(g), CC.expected(g)
    assert cases
    for (name, data, se), (out, out_se) in zip(cases, exp):
        got, got_se = CM.compact_model(data, se)
        assert np.array_equal(got_se, out_se), name
        assert got == out, name
        assert out_se.dtype == np.uint64 and out_se.size == se.size and int(out_se[-1]) == len(out), name


def test_corpus_has_the_edges_it_claims():
    """The shapes the corpus is there for: the lengths of group c, touching and
    empty ranges, ranges that start and end mid-line, and no range past its buffer."""
    lens = sorted(d.size for _n, d, _se in CC.group("c"))
    assert lens == sorted(nb * 4096 - x for nb in (1, 2, 1023, 1024, 1025, 2049) for x in (4095, 0))
    assert {n.rsplit("/", 1)[1] for n, _d, _se in CC.group("c")} == {"one", "4k", "cuts"}
    for g in CC.GROUPS:
        for name, data, se in CC.group(g):
            s = se.astype(np.int64)
            assert (s[1::2] >= s[0::2]).all() and (s[2::2] >= s[1:-1:2]).all(), name    # sorted, disjoint
            assert int(s[-1]) <= data.size, name                                        # inside [0, len]
    assert len(CC.group("a")) == 32 and all(se.size == 2 * 16807 for _n, _d, se in CC.group("a"))
    _n, data, se = CC.group("e")[1]
    s = se.astype(np.int64)
    assert (data[s[0::2][1:] - 1] != 10).any() and (s[2::2] > s[1:-1:2]).any()         # mid-line starts, bytes left out
    # every kept count of group c's blocks is not the same: the scan's carry matters
    _n, data, se = CC.group("c")[-1]
    kept = (data[: data.size // 4096 * 4096].reshape(-1, 4096) != 10).sum(axis=1)
    assert (kept == 0).any() and (kept == 4096).any() and ((kept > 0) & (kept < 4096)).any()


def test_corpus_separates_every_fault():
    """Each of the nine wrong rules of chunk_model.FAULTS differs from the
    statement on at least one case of the corpus -- so a kernel with that rule
    fails tests/test_gpu_chunk_compact.py -- and the zero-pad layout of group a
    alone separates all nine.  Prints, per fault, the groups that catch it and
    the number of group a's 16,807 records that differ."""
    caught = {}
    for f in sorted(CM.FAULTS):
        groups = []
        for g in CC.GROUPS:
            for (name, data, se), (out, out_se) in zip(CC.group(g), CC.expected(g)):
                got, got_se = CM.compact_model(data, se, fault=f)
                if got != out or not np.array_equal(got_se, out_se):
                    groups.append(g)
                    break
        _name, data, se = CC.group("a")[0]
        out, out_se = CC.expected("a")[0]
        got, got_se = CM.compact_model(data, se, fault=f)
        differing = sum(x != y for x, y in zip(_records(got, got_se), _records(out, out_se)))
        caught[f] = (groups, differing)
        print("fault {} ({}): caught by group(s) {}; {} of 16807 records of a/pad0 differ".format(
            f, CM.FAULTS[f], ", ".join(groups) or "none", differing))
    assert sorted(caught) == list(range(1, 10))
    # the groups that separate each fault (group d's few ranges have no N before a range start, no '\r'
    # inside a line, no gap letter or "\r\n" between two N and no kept 'n' or '|': it misses five of them)
    assert {f: "".join(groups) for f, (groups, _) in caught.items()} == {
        1: "abce", 2: "abce", 3: "abcde", 4: "abce", 5: "abcde", 6: "abcde", 7: "abce", 8: "abcde", 9: "abce"}
    for f, (groups, differing) in caught.items():
        assert groups, "no corpus case separates fault {} ({})".format(f, CM.FAULTS[f])
        assert "a" in groups and differing > 0, (f, groups, differing)
    with pytest.raises(ValueError):
        CM.compact_model(b"N", [0, 1], fault=10)


def test_statement_small_cases():
    """compact_records_host on cases small enough to read."""
    from kf2vecfsw_amd import chunks as CH
    parts = [b"junk\n", b"AC\r\nNn|\r\n|nGT\r", b"xN-N. \tn\nA\rC\r\r\n", b"\r"]
    data = b"".join(parts)
    p = np.cumsum([len(x) for x in parts]).tolist()
    out, se = CH.compact_records_host(data, [p[0], p[1], p[1], p[2], p[2], p[2], p[2], p[3]])
    assert out == b"ACNGT" + b"xNNNA\rC\r" and se.tolist() == [0, 5, 5, 13, 13, 13, 13, 13]
    out, se = CH.compact_records_host(np.frombuffer(b"NN\nNN", np.uint8), np.array([0, 2, 2, 5], np.uint64))
    assert out == b"NN" and se.tolist() == [0, 1, 1, 2]          # touching ranges split a run: one N each
    out, se = CH.compact_records_host(b"", [0, 0, 0, 0])
    assert out == b"" and se.tolist() == [0, 0, 0, 0] and se.dtype == np.uint64


def test_statement_equals_oracle_on_chunk_genomes(native, oracle):
    """compact_records_host over record_regions == the oracle's seqtk restatement
    (fasta_records) followed by its two substitutions, record by record: the
    same number of records, the same order, the same bytes."""
    from kf2vecfsw_amd import chunks as CH
    nrun, gaps = re.compile(rb"[N|n]+"), re.compile(rb"[- \t.]")   # main.py:740, seqkit seq -g
    rng = np.random.default_rng(4040)
    datas = [gen.chunk_genome(rng, int(rng.integers(1, 12))) for _ in range(6)]
    datas += [b">a\n>b x\n" + gen.wrap(gen.random_seq(rng, 23000), 60) + b">c\n>d\n>e\n" +
              gen.wrap(gen.random_seq(rng, 12000), 80)]
    n_records = 0
    for i, data in enumerate(datas):
        se, ids = CH.record_regions(np.frombuffer(data, np.uint8))
        out, out_se = CH.compact_records_host(data, se)
        exp = [(hdr, gaps.sub(b"", nrun.sub(b"N", seq))) for hdr, seq in oracle.fasta_records(data)]
        assert len(ids) == len(exp), i
        assert ids == [(hdr.split() or [""])[0] for hdr, _ in exp], i
        assert _records(out, out_se) == [seq for _, seq in exp], i
        n_records += len(exp)
    assert n_records > 30


# ------------------------------------------------------------------ refusals
@pytest.fixture()
def bufs():
    """Host memory whose addresses stand in for the five device buffers: every
    call below returns before a kernel is launched, so none is ever read."""
    return [np.zeros(64, np.uint64) for _ in range(5)]


def _compact(lib, ptrs, length, n_rec, scratch_words):
    d_bytes, d_seq, d_out, d_out_se, d_scratch = ptrs
    return lib.kf_chunk_compact(d_bytes, length, d_seq, n_rec, d_out, d_out_se, d_scratch, scratch_words, None)


def test_chunk_compact_refusals(native, bufs):
    from kf2vecfsw_amd import _native as N
    ptrs = [b.ctypes.data for b in bufs]

    def refused(rc, code, text):
        assert rc == code
        msg = native.kf_last_error()
        assert msg and text in msg, msg

    refused(_compact(native, ptrs, 100, -1, 2), N.KF_EINVAL, b"n_rec")
    for x in range(5):
        refused(_compact(native, ptrs[:x] + [None] + ptrs[x + 1:], 100, 1, 2), N.KF_EINVAL, b"null")
    refused(_compact(native, ptrs, 1 << 32, 1, (1 << 20) + 1), N.KF_EINVAL, b"4 GiB")
    for length in (1, 4096, 4097, (1 << 32) - 1):
        nb = (length + 4095) // 4096
        refused(_compact(native, ptrs, length, 1, nb), N.KF_ERANGE, b"scratch needs %d words" % (nb + 1))
    # nothing to do: accepted whatever else is passed, nothing launched
    assert _compact(native, [None] * 5, 100, 0, 0) == N.KF_OK
    assert _compact(native, ptrs, 1 << 32, 0, 0) == N.KF_OK


def test_chunk_gather_refusals(native, bufs):
    from kf2vecfsw_amd import _native as N
    src, win, dst = [b.ctypes.data for b in bufs[:3]]
    assert native.kf_chunk_gather(src, win, -1, 16, dst, None) == N.KF_EINVAL
    assert b"n_win" in native.kf_last_error()
    for args in ((None, win, dst), (src, None, dst), (src, win, None)):
        assert native.kf_chunk_gather(args[0], args[1], 1, 16, args[2], None) == N.KF_EINVAL
        assert b"null" in native.kf_last_error()
    assert native.kf_chunk_gather(None, None, 0, 16, None, None) == N.KF_OK
