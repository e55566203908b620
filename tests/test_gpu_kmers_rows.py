"""GPU tests of the device-built get_kmers matrix: the kf_kmers_rows kernel, the
kmers_features hand-off and the streamed `.npy` files of the get_kmers CLI.

Expected values come from main.sparse_kmers_matrix / main.kmers_matrix (host
numpy) fed the same keys and counts, or the oracle's counts; every comparison is
bit for bit on the uint32 view of the floats, no tolerance."""
import io
import os

import numpy as np
import pytest

import gen

pytestmark = pytest.mark.gpu

GUARD = 64                 # floats on each side of an output buffer
PATTERN = 0x7FC0DEAD       # a NaN the kernel never produces
KS = [2, 3, 12, 13, 16, 17, 30, 31]   # row widths 3, 4, 13, 14, 17, 18, 31, 32 floats


@pytest.fixture(scope="module")
def torch_dev(native):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu tests need an MI355X")
    return torch.device("cuda:0")


def guarded(rows, w, dev):
    """(buffer int32 view filled with PATTERN, its float32 middle of rows x w)."""
    import torch
    buf = torch.full((2 * GUARD + rows * w,), PATTERN, dtype=torch.int32, device=dev)
    return buf, buf.view(torch.float32)[GUARD: GUARD + rows * w]


def guards_intact(buf, rows, w):
    b = buf.cpu().numpy()
    return (b[:GUARD] == PATTERN).all() and (b[GUARD + rows * w:] == PATTERN).all()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class Case:
    """Segments of {0, 1, 3, 4, 5, T-1, T, T+1, 3T+7} rows (tiles straddle
    segments), stored out of order and with gaps in the key array; keys random in
    [0, 4^k) with 0 and 4^k - 1; counts that are inexact as float32; divisors
    3, 7, 16777213 and the segments' true totals in turn."""

    def __init__(self, k, wide, dev):
        import torch
        from kf2vecfsw_amd import counter as C
        from kf2vecfsw_amd import main as M
        T = C.kmers_tile_rows()
        rng = np.random.default_rng(100 * k + wide)
        self.k, self.w, self.T = k, k + 1, T
        self.n = np.array([0, 1, 3, 4, 5, T - 1, T, T + 1, 3 * T + 7], np.int64)
        ns = self.n.size
        order = rng.permutation(ns)                       # where each segment's keys lie
        self.src0 = np.zeros(ns, np.int64)
        pos = 5
        for s in order:
            self.src0[s] = pos
            pos += int(self.n[s]) + int(rng.integers(0, 9))
        hi = 1 << (2 * k)
        keys = rng.integers(0, hi, pos, dtype=np.uint64)
        pool = [1, 3, (1 << 24) + 1, (1 << 32) - 1] + ([1 << 32, (1 << 40) + 1] if wide else [])
        cnts = rng.choice(np.array(pool, np.uint64), pos).astype(np.uint64 if wide else np.uint32)
        last = int(self.src0[-1])
        keys[last], keys[last + 1] = 0, hi - 1              # in the largest segment
        self.keys = torch.from_numpy(keys.view(np.int64)).to(dev)
        self.cnts = torch.from_numpy(cnts.view(np.int64 if wide else np.int32)).to(dev)
        true = C.kmers_denominators(self.cnts, self.src0, self.n)
        self.denom = np.array([[3, 7, 16777213, true[s]][s % 4] for s in range(ns)], np.float32)
        self.denom[-1] = true[-1]
        self.mats = []
        for s in range(ns):
            a, m = int(self.src0[s]), int(self.n[s])
            mat = M.sparse_kmers_matrix(keys[a: a + m], cnts[a: a + m], k)   # its last column: c / np.sum(c)
            if m and self.denom[s] != true[s]:
                mat[:, k] = cnts[a: a + m].astype(np.float32) / np.float32(self.denom[s])
            elif m:
                assert np.sum(cnts[a: a + m].astype(np.float32)) == true[s]
            self.mats.append(mat)
        self.packed = np.concatenate(self.mats)
        self.rows = int(self.n.sum())
        self.tab = C.kmers_tables(self.src0, self.n, np.concatenate([[0], np.cumsum(self.n)]), self.denom, dev)


_cases = {}


def case(k, wide, dev):
    if (k, wide) not in _cases:
        _cases[(k, wide)] = Case(k, wide, dev)
    return _cases[(k, wide)]


def run(c, tab, lo, hi, out, dev):
    import torch
    from kf2vecfsw_amd import counter as C
    status = torch.full((1,), 77, dtype=torch.int32, device=dev)
    C.kmers_rows(c.keys, c.cnts, tab, c.k, lo, hi, out, status)
    return int(status.item())


@pytest.mark.parametrize("wide", [0, 1])
@pytest.mark.parametrize("k", KS)
def test_kmers_rows_vs_host(torch_dev, k, wide):
    """The packed matrix of all segments in one call, u32 and u64 counts."""
    c = case(k, wide, torch_dev)
    buf, out = guarded(c.rows, c.w, torch_dev)
    assert run(c, c.tab, 0, c.rows, out, torch_dev) == 0
    got = out.cpu().numpy().reshape(c.rows, c.w)
    if not np.array_equal(bits(got), bits(c.packed)):
        bad = np.argwhere(bits(got) != bits(c.packed))[:5]
        pytest.fail(f"k={k} wide={wide}: first differing (row, col) {bad.tolist()}: got "
                    f"{[got[r, j] for r, j in bad]} want {[c.packed[r, j] for r, j in bad]}")
    assert guards_intact(buf, c.rows, c.w)


@pytest.mark.parametrize("k", [3, 16, 30])
def test_kmers_rows_padded_batch(torch_dev, k):
    """d_dst0[s] = s * Nmax: the [B, Nmax, k + 1] batch pad_sequence builds from
    the host matrices; the gap rows are zeros though d_out held garbage."""
    import torch
    from kf2vecfsw_amd import counter as C
    c = case(k, 0, torch_dev)
    B, nmax = c.n.size, int(c.n.max())
    tab = C.kmers_tables(c.src0, c.n, np.arange(B + 1, dtype=np.int64) * nmax, c.denom, torch_dev)
    buf, out = guarded(B * nmax, c.w, torch_dev)
    assert run(c, tab, 0, B * nmax, out, torch_dev) == 0
    want = torch.nn.utils.rnn.pad_sequence([torch.from_numpy(m) for m in c.mats], batch_first=True, padding_value=0)
    assert want.shape == (B, nmax, c.w)
    assert np.array_equal(bits(out.cpu().numpy().reshape(B, nmax, c.w)), bits(want.numpy()))
    assert guards_intact(buf, B * nmax, c.w)


@pytest.mark.parametrize("k", [2, 30])
def test_kmers_rows_slabs(torch_dev, k):
    """The packed matrix through slabs of 1, 5, T + 3 and 4T rows, row_lo walking
    through all of it: equal to the one-call result, and a call writes nothing
    past its row_hi (the slab buffer is re-filled with the pattern every call)."""
    import torch
    from kf2vecfsw_amd import counter as C
    c = case(k, 0, torch_dev)
    status = torch.zeros(1, dtype=torch.int32, device=torch_dev)
    for S in (1, 5, c.T + 3, 4 * c.T):
        buf, out = guarded(S, c.w, torch_dev)
        full = torch.empty(c.rows * c.w, dtype=torch.float32, device=torch_dev)
        dirty = torch.zeros((), dtype=torch.bool, device=torch_dev)
        seen = torch.zeros((), dtype=torch.int32, device=torch_dev)
        for lo in range(0, c.rows, S):
            hi = min(c.rows, lo + S)
            m = (hi - lo) * c.w
            buf.fill_(PATTERN)
            C.kmers_rows(c.keys, c.cnts, c.tab, k, lo, hi, out, status)
            seen |= status[0]
            full[lo * c.w: hi * c.w] = out[:m]
            dirty |= (buf[:GUARD] != PATTERN).any() | (buf[GUARD + m:] != PATTERN).any()
        assert int(seen.item()) == 0 and not bool(dirty.item()), S
        assert np.array_equal(bits(full.cpu().numpy().reshape(c.rows, c.w)), bits(c.packed)), S


def test_kmers_rows_refuses_bad_tables(torch_dev):
    """Checked arguments: a decreasing d_dst0, a d_n[s] larger than its gap and a
    row_hi past the total each give status 2 and leave d_out untouched; an empty
    slab of good tables gives status 0."""
    from kf2vecfsw_amd import counter as C
    c = case(13, 0, torch_dev)
    good = np.concatenate([[0], np.cumsum(c.n)])
    dec = good.copy()
    dec[5] = dec[4] - 1
    tight = good.copy()
    tight[-1] -= 1                                         # the last segment's gap is one row short
    for dst0, hi in ((dec, c.rows), (tight, c.rows - 1), (good, c.rows + 1)):
        tab = C.kmers_tables(c.src0, c.n, dst0, c.denom, torch_dev)
        buf, out = guarded(c.rows + 1, c.w, torch_dev)
        assert run(c, tab, 0, hi, out, torch_dev) == 2
        assert (buf.cpu().numpy() == PATTERN).all()
    buf, out = guarded(4, c.w, torch_dev)
    assert run(c, c.tab, 7, 7, out, torch_dev) == 0
    assert (buf.cpu().numpy() == PATTERN).all()


def pad_input(mats):
    """train_model_set.pad_input (train_model_set.py:92-94)."""
    import torch
    return torch.nn.utils.rnn.pad_sequence([torch.from_numpy(m) for m in mats], batch_first=True, padding_value=0)


@pytest.fixture(scope="module")
def genomes():
    rng = np.random.default_rng(2024)
    return [gen.random_fasta(rng, int(rng.integers(0, 30000)), n_rate=0.01, lower=0.05) for _ in range(6)] + [b""]


def test_kmers_features_dense(torch_dev, oracle, genomes):
    import torch
    from kf2vecfsw_amd import counter as C
    from kf2vecfsw_amd import main as M
    k = 7
    counts, _ = C.KmerCounter(k, torch_dev).count(C.to_device(C.pack_genomes(genomes), torch_dev))
    got = C.kmers_features(None, counts, None, None, k)
    want = pad_input([M.kmers_matrix(oracle.count(b, k)[0], k) for b in genomes])
    assert got.dtype == torch.float32 and got.device.type == "cuda" and tuple(got.shape) == tuple(want.shape)
    assert np.array_equal(bits(got.cpu().numpy()), bits(want.numpy()))


def test_kmers_features_sparse(torch_dev, oracle, genomes):
    import torch
    from kf2vecfsw_amd import counter as C
    from kf2vecfsw_amd import main as M
    k = 21
    hb = C.pack_genomes(genomes)
    keys, cnts, nu = C.SparseCounter(k, torch_dev).count(C.to_device(hb, torch_dev), int(hb.off[-1]))
    got = C.kmers_features(keys, cnts, nu, hb.off, k)
    want = pad_input([M.sparse_kmers_matrix(*oracle.sparse_count(b, k), k) for b in genomes])
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(want.shape)
    assert np.array_equal(bits(got.cpu().numpy()), bits(want.numpy()))


def npy_bytes(m):
    f = io.BytesIO()
    np.save(f, m)
    return f.getvalue()


@pytest.mark.parametrize("k", [7, 13, 31])
def test_cli_get_kmers_streams_npy_bytes(torch_dev, toy, oracle, tmp_path, monkeypatch, capsys, k):
    """get_kmers with a slab of a few hundred rows (slab edges inside genomes and
    between them): every .npy file's bytes are np.save's of the host function on
    the oracle's counts; a header-only file prints the warning and writes nothing."""
    from kf2vecfsw_amd import main as M
    monkeypatch.setattr(M, "KMERS_SLAB_BYTES", 300 * 4 * (k + 1) + 8)
    inp, out = tmp_path / "in", tmp_path / "out"
    inp.mkdir()
    small = [t for t in toy if len(t[2]) < 1_000_000]
    tiny = [(f"tiny{i}.fna", f"tiny{i}", b">t\n" + gen.random_seq(np.random.default_rng(i), 40 + 90 * i).tobytes() + b"\n",
             None) for i in range(4)]                      # several genomes inside one slab
    files = small + tiny
    for name, sample, data, _ in files:
        (inp / name).write_bytes(data)
    (inp / "hollow.fna").write_bytes(b">only a header\n")
    M.main(["get_kmers", "-input_dir", str(inp), "-output_dir", str(out), "-k", str(k)])
    printed = capsys.readouterr().out
    for name, sample, data, _ in files:
        if k <= 12:
            ref = M.kmers_matrix(oracle.count(data, k)[0], k)
        else:
            ref = M.sparse_kmers_matrix(*oracle.sparse_count(data, k), k)
        assert ref.shape[0] > 0
        path = out / f"{sample}_k{k}.npy"
        assert path.read_bytes() == npy_bytes(ref), sample
        assert f"--- Processing {sample} ---\nSaved: {path} (Shape: {ref.shape})\n" in printed
    assert "--- Processing hollow ---\nWarning: No valid ATCG k-mers found in hollow\n" in printed
    assert not (out / f"hollow_k{k}.npy").exists()
    assert len(os.listdir(out)) == len(files)


def test_get_kmers_piece_path_equals_unsplit(torch_dev, tmp_path, monkeypatch):
    """One multi-record FASTA of ~100 kB at k = 15 counted in pieces of 30,000
    bytes (merged int64 counts, count_bytes = 8): the same .npy bytes as unsplit."""
    from kf2vecfsw_amd import main as M
    rng = np.random.default_rng(15)
    inp = tmp_path / "in"
    inp.mkdir()
    data = gen.random_fasta(rng, 100_000, max_records=4, n_rate=0.001)
    (inp / "multi.fna").write_bytes(data)
    M.main(["get_kmers", "-input_dir", str(inp), "-output_dir", str(tmp_path / "whole"), "-k", "15"])
    monkeypatch.setattr(M, "SPLIT_BYTES", 30_000)
    assert len(M.fasta_pieces(str(inp / "multi.fna"), 15, M.SPLIT_BYTES)) >= 3
    M.main(["get_kmers", "-input_dir", str(inp), "-output_dir", str(tmp_path / "pieces"), "-k", "15"])
    whole = (tmp_path / "whole" / "multi_k15.npy").read_bytes()
    assert len(whole) > 128 + 50_000 * 16 * 4 and (tmp_path / "pieces" / "multi_k15.npy").read_bytes() == whole
