"""CPU checks of get_frequencies' piece-wise path: the FASTQ cut rule
(main.fastq_pieces), fasta_pieces at the dense counter's k, the batch planner
(main._plan_units) and kf_rows_accumulate's argument checks."""
import numpy as np
import pytest

import fastq_model as FM
import gen
from kf2vecfsw_amd import main as M
from split_inputs import fastq_reads

FA, FQ = 1, 2   # KF_FMT_FASTA, KF_FMT_FASTQ
GiB = 1 << 30


def fastq_cases():
    rng = np.random.default_rng(707)
    cases = {f"random{s}": gen.random_fastq(np.random.default_rng(s), 120, n_rate=0.01) for s in (1, 2, 3)}
    cases["qual_at_plus"] = fastq_reads(rng, 150, qual_first=b"@+")
    cases["qual_at_150"] = fastq_reads(rng, 60, length=150, qual_first=b"@@+")
    cases["crlf"] = fastq_reads(rng, 100, qual_first=b"@+I", crlf=True)
    cases["no_final_newline"] = fastq_reads(rng, 100, qual_first=b"@")[:-1]
    whole = fastq_reads(rng, 100, qual_first=b"+@")
    lines = FM.split_lines(whole)
    cases["ends_in_header"] = whole[: lines[-4][1] - 2]
    cases["ends_in_sequence"] = whole[: lines[-3][0] + 1]
    cases["ends_after_plus"] = whole[: lines[-2][1] + 1]
    cases["long_read"] = (fastq_reads(rng, 20, qual_first=b"@") + fastq_reads(rng, 1, length=9000, qual_first=b"@",
                                                                               name=b"long")
                          + fastq_reads(rng, 30, qual_first=b"+", name=b"t"))
    return cases


CASES = fastq_cases()


@pytest.mark.parametrize("case", sorted(CASES))
def test_fastq_pieces_cut_at_record_starts(tmp_path, oracle, case):
    """The ranges tile the file, every start is a header line (line number j with
    j % 4 == 0 in the four-line form), and the oracle's FASTQ counts of the
    pieces sum to those of the whole file at k = 3, 7, 11."""
    blob = CASES[case]
    assert FM.is_regular(blob)
    p = tmp_path / "r.fq"
    p.write_bytes(blob)
    line_no = {s: j for j, (s, _) in enumerate(FM.split_lines(blob))}
    whole = {k: oracle.count(blob, k, FQ) for k in (3, 7, 11)}
    for piece in (64, 100, 257, 1000, 4096):
        parts = M.fastq_pieces(str(p), piece)
        assert parts[0][0] == 0 and parts[-1][1] == len(blob)
        assert all(a < e for a, e in parts) and all(parts[i][1] == parts[i + 1][0] for i in range(len(parts) - 1))
        for i, (a, _) in enumerate(parts[1:]):
            assert line_no.get(a, 1) % 4 == 0, (piece, a)
            assert a // piece * piece > parts[i][0]   # one cut per multiple of the piece size, at or after it
        if case != "long_read":   # pieces of about `piece` bytes: reads of up to ~200 bases, ~420-byte records
            assert len(parts) >= len(blob) // (piece + 1000)
        for k, (c, t) in whole.items():
            got, gt = np.zeros_like(c), 0
            for a, e in parts:
                ci, ti = oracle.count(blob[a:e], k, FQ)
                got += ci
                gt += ti
            assert gt == t and np.array_equal(got, c), (piece, k)
    assert M.fastq_pieces(str(p), len(blob)) == [(0, len(blob))]


def test_fastq_pieces_long_read_is_not_cut(tmp_path):
    """A read longer than the piece size stays inside one piece."""
    blob = CASES["long_read"]
    p = tmp_path / "r.fq"
    p.write_bytes(blob)
    s = blob.index(b"@long0")
    for piece in (64, 1000, 4096):
        parts = M.fastq_pieces(str(p), piece)
        assert not any(s < a < s + 18000 for a, _ in parts), piece   # the record: over 18,000 bytes
        assert any(a >= s + 18000 for a, _ in parts)


def test_fastq_pieces_multi_line_is_one_piece(tmp_path):
    """A FASTQ file with two-line sequences has no line that passes the rule (two
    lines after a header comes a sequence line; a quality line starting with '@'
    has a header or a sequence line two lines on): it stays one piece and is
    counted whole."""
    rng = np.random.default_rng(5)
    recs = []
    for i in range(200):
        s = gen.random_seq(rng, 80).tobytes()
        q = bytes(rng.choice(list(b"@+I#"), size=80).tolist())
        recs.append(b"@r%d\n" % i + s[:40] + b"\n" + s[40:] + b"\n+\n" + q[:40] + b"\n" + q[40:] + b"\n")
    blob = b"".join(recs)
    assert not FM.is_regular(blob)
    p = tmp_path / "m.fq"
    p.write_bytes(blob)
    for piece in (64, 500, 4096):
        assert M.fastq_pieces(str(p), piece) == [(0, len(blob))]


@pytest.mark.parametrize("k", [8, 9, 10, 11])
def test_fasta_pieces_at_dense_k(tmp_path, oracle, k):
    """fasta_pieces as get_frequencies uses it (k up to 11): the oracle's counts of
    the pieces sum to the whole file's, with a header line exactly at a nominal
    cut and an N run across one."""
    rng = np.random.default_rng(100 + k)
    piece = 1000
    a = gen.wrap(gen.random_seq(rng, 2400), 60)
    first = (b">c0\n" + a)[: 2 * piece - 1] + b"\n"   # the next header starts exactly at byte 2 * piece
    seq = gen.random_seq(rng, 5000, lower=0.05)
    blob = first + b">c1 at a cut\n" + gen.wrap(seq, 70) + b">c2\n" + gen.wrap(gen.random_seq(rng, 3000), 0)
    arr = np.frombuffer(blob, np.uint8).copy()
    x = 4 * piece - 20                              # an N run across the cut at 4 * piece
    run = np.arange(x, x + 40)
    arr[run[arr[run] != 10]] = ord("N")
    blob = arr.tobytes()
    assert blob[2 * piece: 2 * piece + 3] == b">c1" and blob[2 * piece - 1: 2 * piece] == b"\n"
    assert blob[4 * piece - 1] in b"N\n" and blob[4 * piece + 1] in b"N\n"
    p = tmp_path / "g.fa"
    p.write_bytes(blob)
    whole, tot = oracle.count(blob, k, FA)
    for pc in (piece, 333, 4096):
        parts = M.fasta_pieces(str(p), k, pc)
        assert parts[0][0] == 0 and parts[-1][1] == len(blob) and len(parts) >= len(blob) // pc // 2
        got, gt = np.zeros_like(whole), 0
        for s, e in parts:
            c, t = oracle.count(blob[s:e], k, FA)
            got += c
            gt += t
        assert gt == tot and np.array_equal(got, whole), pc


def unit_bytes(b):
    return sum(e - a for _, a, e, _ in b)


def pieces_of(size, piece, kind):
    """A cut plan as fastq_pieces makes it: starts a record past each multiple."""
    cuts = [0] + [i * piece + 137 for i in range(1, -(-size // piece))]
    cuts = [c for c in cuts if c < size]
    return (kind, [(c, cuts[i + 1] if i + 1 < len(cuts) else size) for i, c in enumerate(cuts)])


@pytest.mark.parametrize("budget", [16 << 20, GiB, 4 * GiB])
def test_planner_bounds_batches_whatever_the_file_sizes(budget):
    """Sizes with a 300 GiB file: no batch is larger than max(budget, largest
    unit), where the units are the pieces (about 1 GiB here) and the whole files
    (below the split limit); file order is kept, a batch holds whole files only
    or pieces of one kind only, pieces count as genomes for the cap, and with no
    file cut the batches are _size_batches' own."""
    sizes = [5 << 20, 300 * GiB, 7 << 20, 3 << 20, 40 * GiB, 9 * GiB, 1 << 20, 2 * GiB, 0, 11 << 20]
    pieces = [None] * len(sizes)
    pieces[1] = pieces_of(sizes[1], GiB, "fastq")
    pieces[4] = pieces_of(sizes[4], GiB, "fastq")
    pieces[5] = pieces_of(sizes[5], GiB, "fasta")
    for cap in (None, 3, 256):
        batches = M._plan_units(sizes, pieces, budget, cap)
        units = [u for b in batches for u in b]
        largest = max(e - a for _, a, e, _ in units)
        assert largest <= 2 * GiB                                       # the whole 2 GiB file, or a piece
        assert max(unit_bytes(b) for b in batches) <= max(budget, largest)
        # every byte of every file once, files and pieces in order
        assert [u[0] for u in units] == sorted(u[0] for u in units)
        for fi, s in enumerate(sizes):
            mine = [(a, e) for f, a, e, _ in units if f == fi]
            assert mine[0][0] == 0 and mine[-1][1] == s and all(mine[i][1] == mine[i + 1][0] for i in range(len(mine) - 1))
            assert mine == (pieces[fi][1] if pieces[fi] else [(0, s)])
        for b in batches:
            assert len({u[3] for u in b}) == 1 and (cap is None or len(b) <= cap)
        if cap is not None and budget >= 4 * GiB:
            assert max(len(b) for b in batches if b[0][3] != "whole") == min(cap, 4)
    small = [s for s in sizes if s <= 2 * GiB]
    for cap in (None, 2):
        plan = M._plan_units(small, None, budget, cap)
        assert [[u[0] for u in b] for b in plan] == M._size_batches(small, budget, ramp=True, max_files=cap)
        assert all(u == (u[0], 0, small[u[0]], "whole") for b in plan for u in b)


def test_split_pieces_limit(tmp_path):
    """-split_gb S: only a file above S GiB is cut, into pieces of about min(S, 1)
    GiB by its format's rule; 0 never cuts; a file without an acceptable cut
    stays whole."""
    rng = np.random.default_rng(9)
    fq = fastq_reads(rng, 100, length=150)
    fa = gen.random_fasta(rng, 30000, max_records=3)
    small = fastq_reads(rng, 3, length=150)
    one_read = fastq_reads(rng, 1, length=20000)
    paths = []
    for name, b in (("a.fq", fq), ("b.fa", fa), ("c.fq", small), ("d.fq", one_read)):
        (tmp_path / name).write_bytes(b)
        paths.append(str(tmp_path / name))
    sizes = [len(fq), len(fa), len(small), len(one_read)]
    s = 8192 / GiB
    got = M._split_pieces(paths, sizes, 7, s)
    assert got[0] == ("fastq", M.fastq_pieces(paths[0], 8192)) and len(got[0][1]) > 2
    assert got[1] == ("fasta", M.fasta_pieces(paths[1], 7, 8192)) and len(got[1][1]) > 2
    assert got[2] is None and got[3] is None
    assert M._split_pieces(paths, sizes, 7, 0) is None and M._split_pieces(paths, sizes, 7, 4.0) is None
    assert M.build_parser().parse_args(["get_frequencies"]).split_gb == 4.0


def test_rows_accumulate_argument_checks(native):
    """Every KF_EINVAL case returns before anything touches a device."""
    from kf2vecfsw_amd import _native as N
    f = native.kf_rows_accumulate
    good = dict(src=0x1000, st=0x2000, n_src=4, seg=0x3000, n_dst=2, nbins=32, dst=0x4000, dt=0x5000, status=0x6000)

    def call(**kw):
        a = dict(good, **kw)
        return f(a["src"], a["st"], a["n_src"], a["seg"], a["n_dst"], a["nbins"], a["dst"], a["dt"], a["status"], 0,
                 None)

    for name in ("src", "st", "seg", "dst", "dt", "status"):
        assert call(**{name: None}) == N.KF_EINVAL, name
        assert b"null" in native.kf_last_error()
    assert call(n_src=-1) == N.KF_EINVAL and call(n_dst=-1) == N.KF_EINVAL
    assert call(nbins=0) == N.KF_EINVAL
    assert call(src=0x1002) == N.KF_EINVAL and call(dt=0x5004) == N.KF_EINVAL
