"""GPU tests of kf_sparse_merge (the union of two sorted (key, count) lists),
counter.merge_sorted and the get_kmers piece path that merges as it goes.

Expected values come from numpy in this file (np.union1d on the uint64 keys,
counts by np.add.at in uint64) and, for one case, from main._merge_sorted_counts;
every comparison is exact.  The kernel tests call the C-ABI with output buffers
that carry guard words on both sides, checked after every call."""
import numpy as np
import pytest

import gen

pytestmark = pytest.mark.gpu

GUARD = 64                        # u64 words on each side of an output array
PATTERN = 0x7FC0DEAD7FC0DEAD      # what they hold
KEY_HI = 1 << 62                  # 4^31


@pytest.fixture(scope="module")
def torch_dev(native):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu tests need an MI355X")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def T(native):
    return native.kf_sparse_merge_tile()


def expected(ka, ca, kb, cb):
    """(keys uint64, counts uint64) of the union, by numpy."""
    ka, kb = np.asarray(ka, np.uint64), np.asarray(kb, np.uint64)
    u = np.union1d(ka, kb)
    c = np.zeros(u.size, np.uint64)
    np.add.at(c, np.searchsorted(u, ka), np.asarray(ca).astype(np.uint64))
    np.add.at(c, np.searchsorted(u, kb), np.asarray(cb).astype(np.uint64))
    return u, c


def dev_keys(k, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(k, np.uint64).view(np.int64)).to(dev)


def dev_counts(c, dev):
    """uint32 -> int32 tensor, uint64 -> int64 tensor (the dtype chooses count_bytes)."""
    import torch
    c = np.ascontiguousarray(c)
    assert c.dtype in (np.uint32, np.uint64)
    return torch.from_numpy(c.view(np.int32 if c.dtype == np.uint32 else np.int64)).to(dev)


def raw_merge(ka, ca, kb, cb, dev):
    """kf_sparse_merge through the C-ABI into guarded outputs: (status, n_out,
    keys uint64[n_a + n_b], counts uint64[n_a + n_b]) on the host; asserts the guards."""
    import torch
    from kf2vecfsw_amd import _native as N
    from kf2vecfsw_amd.counter import _stream_ptr
    L = N.lib()
    tka, tca, tkb, tcb = dev_keys(ka, dev), dev_counts(ca, dev), dev_keys(kb, dev), dev_counts(cb, dev)
    n_a, n_b = tka.numel(), tkb.numel()
    n = n_a + n_b
    bufs = [torch.full((2 * GUARD + n,), PATTERN, dtype=torch.int64, device=dev) for _ in range(2)]
    n_out = torch.full((1,), -7, dtype=torch.int64, device=dev)
    status = torch.full((1,), 77, dtype=torch.int32, device=dev)
    need = L.kf_sparse_merge_scratch_bytes(n_a, n_b)
    scratch = torch.full((need // 8 + 2 * GUARD,), PATTERN, dtype=torch.int64, device=dev)
    N.check(L.kf_sparse_merge(tka.data_ptr() if n_a else None, tca.data_ptr() if n_a else None, tca.element_size(), n_a,
                              tkb.data_ptr() if n_b else None, tcb.data_ptr() if n_b else None, tcb.element_size(), n_b,
                              bufs[0][GUARD:].data_ptr(), bufs[1][GUARD:].data_ptr(), n_out.data_ptr(),
                              status.data_ptr(), scratch[GUARD:].data_ptr(), need, _stream_ptr(dev)),
            "kf_sparse_merge")
    out = []
    for b in bufs:
        h = b.cpu().numpy()
        assert (h[:GUARD] == PATTERN).all() and (h[GUARD + n:] == PATTERN).all(), "an output's guard words were written"
        out.append(h[GUARD: GUARD + n].view(np.uint64))
    hs = scratch.cpu().numpy()
    assert (hs[:GUARD] == PATTERN).all() and (hs[GUARD + need // 8:] == PATTERN).all(), "the scratch's guard words"
    return int(status.item()), int(n_out.item()), out[0], out[1]


def check_merge(ka, ca, kb, cb, dev):
    st, n, gk, gc = raw_merge(ka, ca, kb, cb, dev)
    ek, ec = expected(ka, ca, kb, cb)
    assert st == 0 and n == ek.size
    assert np.array_equal(gk[:n], ek), np.flatnonzero(gk[:n] != ek)[:5]
    assert np.array_equal(gc[:n], ec), np.flatnonzero(gc[:n] != ec)[:5]


def random_lists(rng, n_a, n_b, hi=KEY_HI):
    """Two strictly ascending key lists; about half of the smaller one's keys are in both."""
    small, large = min(n_a, n_b), max(n_a, n_b)
    pool = np.unique(rng.integers(0, hi, 2 * (n_a + n_b) + 8, dtype=np.uint64))
    assert pool.size >= n_a + n_b
    pool = rng.permutation(pool)
    lg = pool[:large]
    shared = lg[: small // 2]
    sm = np.concatenate([shared, pool[large: large + small - shared.size]])
    a, b = (sm, lg) if n_a <= n_b else (lg, sm)
    assert a.size == n_a and b.size == n_b
    return np.sort(a), np.sort(b)


def small_counts(rng, n):
    return rng.integers(1, 1000, n).astype(np.uint32)


SIZES_A = ["0", "1", "T-1", "T", "T+1", "3T+7"]
SIZES_B = ["0", "1", "T", "3T+7"]


def size_of(s, T):
    return {"0": 0, "1": 1, "T-1": T - 1, "T": T, "T+1": T + 1, "3T+7": 3 * T + 7}[s]


@pytest.mark.parametrize("sb", SIZES_B)
@pytest.mark.parametrize("sa", SIZES_A)
def test_merge_sizes(torch_dev, T, sa, sb):
    n_a, n_b = size_of(sa, T), size_of(sb, T)
    rng = np.random.default_rng(1000 * n_a + n_b)
    ka, kb = random_lists(rng, n_a, n_b)
    check_merge(ka, small_counts(rng, n_a), kb, small_counts(rng, n_b), torch_dev)


def test_merge_path_extremes(torch_dev, T):
    rng = np.random.default_rng(2)
    lo = np.unique(rng.integers(0, 1 << 40, 2 * T + 9, dtype=np.uint64))
    hi = np.unique(rng.integers(1 << 41, 1 << 42, 3 * T + 1, dtype=np.uint64))
    c = lambda k: small_counts(rng, k.size)
    check_merge(lo, c(lo), hi, c(hi), torch_dev)                  # all of A below all of B
    check_merge(hi, c(hi), lo, c(lo), torch_dev)                  # and the reverse
    one_hi, one_lo = np.array([1 << 50], np.uint64), np.array([0], np.uint64)
    check_merge(one_hi, c(one_hi), hi, c(hi), torch_dev)          # A of one key above all of B
    check_merge(one_lo, c(one_lo), hi, c(hi), torch_dev)          # A of one key below all of B


def test_merge_pairs_across_every_tile_edge(torch_dev, T):
    """B = 2T+5 consecutive even keys, A = the same with one smaller key in front:
    every equal pair sits at merged positions (odd, even) and one straddles each
    tile edge; without the extra key the pairs stay inside the tiles."""
    rng = np.random.default_rng(3)
    kb = (np.arange(2 * T + 5, dtype=np.uint64) + np.uint64(5)) * np.uint64(2)
    ka = np.concatenate([np.array([3], np.uint64), kb])
    assert T % 2 == 0                        # A[i], B[i-1] lie at merged positions 2i-1, 2i: one pair at (T-1, T)
    for a in (ka, kb):
        check_merge(a, small_counts(rng, a.size), kb, small_counts(rng, kb.size), torch_dev)


def test_merge_unsigned_order(torch_dev):
    ka = np.array([0, (1 << 63) - 1, 1 << 63], np.uint64)
    kb = np.array([(1 << 62) - 1, 1 << 63, (1 << 64) - 1], np.uint64)
    check_merge(ka, np.array([1, 2, 3], np.uint32), kb, np.array([10, 20, 30], np.uint32), torch_dev)
    st, n, gk, gc = raw_merge(ka, np.array([1, 2, 3], np.uint32), kb, np.array([10, 20, 30], np.uint32), torch_dev)
    assert gk[:n].tolist() == [0, (1 << 62) - 1, (1 << 63) - 1, 1 << 63, (1 << 64) - 1] and gc[:n].tolist() == [1, 10, 2, 23, 30]


@pytest.mark.parametrize("wb", [4, 8])
@pytest.mark.parametrize("wa", [4, 8])
def test_merge_count_widths(torch_dev, T, wa, wb):
    """u32 / u64 counts per side: 1 and 2^32 - 1 on both sides of shared keys (the
    sum 2^33 - 2 needs u64), and 2^40 + 1 where the side is u64."""
    rng = np.random.default_rng(10 * wa + wb)
    ka, kb = random_lists(rng, T + 3, T + 9)
    both = np.intersect1d(ka, kb)
    assert both.size >= 100
    def counts(k, w):
        c = rng.choice(np.array([1, (1 << 32) - 1], np.uint64), k.size)
        if w == 8:
            c[np.searchsorted(k, both[4:6])] = (1 << 40) + 1
            c[0] = (1 << 40) + 1
        c[np.searchsorted(k, both[:4])] = [(1 << 32) - 1, (1 << 32) - 1, 1, 1]
        return c.astype(np.uint32 if w == 4 else np.uint64)
    ca, cb = counts(ka, wa), counts(kb, wb)
    ek, ec = expected(ka, ca, kb, cb)
    assert ec[np.searchsorted(ek, both[0])] == (1 << 33) - 2
    check_merge(ka, ca, kb, cb, torch_dev)


def test_merge_equals_host_statement(torch_dev, T):
    """counter.merge_sorted == main._merge_sorted_counts == numpy on one input."""
    from kf2vecfsw_amd import counter as C
    from kf2vecfsw_amd import main as M
    rng = np.random.default_rng(4)
    ka, kb = random_lists(rng, 2 * T + 1, T + 77)
    ca, cb = rng.integers(1, 1 << 32, ka.size).astype(np.uint32), rng.integers(1, 1 << 32, kb.size).astype(np.uint32)
    ta, tb = (dev_keys(ka, torch_dev), dev_counts(ca, torch_dev)), (dev_keys(kb, torch_dev), dev_counts(cb, torch_dev))
    k_, c_, n_out, status = C.merge_sorted(*ta, *tb)
    n = C.merged_to_host(n_out, status)
    assert k_.numel() == c_.numel() == ka.size + kb.size
    hk, hc = M._merge_sorted_counts([ta, tb])
    ek, ec = expected(ka, ca, kb, cb)
    # below 2^63 the signed sort of the host statement is the unsigned order
    assert np.array_equal(hk.cpu().numpy().view(np.uint64), ek) and np.array_equal(hc.cpu().numpy().view(np.uint64), ec)
    assert n == ek.size
    assert np.array_equal(k_[:n].cpu().numpy().view(np.uint64), ek)
    assert np.array_equal(c_[:n].cpu().numpy().view(np.uint64), ec)


@pytest.mark.parametrize("case", ["a_descending_mid_tile", "a_descending_across_T", "b_equal_pair"])
def test_merge_order_check(torch_dev, T, case):
    """An input that is not strictly ascending: status 1, n_out 0, nothing outside
    the outputs written, and the next, valid call on the stream is correct."""
    from kf2vecfsw_amd import _native as N
    from kf2vecfsw_amd import counter as C
    rng = np.random.default_rng(5)
    ka, kb = random_lists(rng, 3 * T + 7, T + 5)
    good_a, good_b = ka.copy(), kb.copy()
    if case == "a_descending_mid_tile":
        i = T // 2
        ka[i], ka[i + 1] = ka[i + 1], ka[i]
    elif case == "a_descending_across_T":
        ka[T - 1], ka[T] = ka[T], ka[T - 1]
    else:
        kb[T // 3 + 1] = kb[T // 3]
    ca, cb = small_counts(rng, ka.size), small_counts(rng, kb.size)
    st, n, _, _ = raw_merge(ka, ca, kb, cb, torch_dev)
    assert (st, n) == (1, 0)
    check_merge(good_a, ca, good_b, cb, torch_dev)
    k_, c_, n_out, status = C.merge_sorted(dev_keys(ka, torch_dev), dev_counts(ca, torch_dev),
                                           dev_keys(kb, torch_dev), dev_counts(cb, torch_dev))
    with pytest.raises(N.NativeError, match="not strictly ascending"):
        C.merged_to_host(n_out, status)


def test_merge_bounded_memory(torch_dev):
    """2^20 + 2^20 keys, none shared: merge_sorted's peak allocation is its two
    outputs and the scratch (the sort-based host statement needs several times
    that: the concatenation, the sort's keys and order, unique's outputs)."""
    import torch
    from kf2vecfsw_amd import counter as C
    n = 1 << 20
    ar = torch.arange(n, dtype=torch.int64, device=torch_dev)
    ka, kb = 2 * ar, 2 * ar + 1
    ca = torch.full((n,), 3, dtype=torch.int32, device=torch_dev)
    cb = torch.full((n,), 5, dtype=torch.int32, device=torch_dev)
    del ar
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(torch_dev)
    before = torch.cuda.memory_allocated(torch_dev)
    k_, c_, n_out, status = C.merge_sorted(ka, ca, kb, cb)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated(torch_dev) - before
    bound = 16 * 2 * n + C.merge_scratch_bytes(n, n) + (1 << 20)
    print(f"merge_sorted peak rise {rise} B, bound {bound} B")
    assert rise <= bound
    assert C.merged_to_host(n_out, status) == 2 * n
    assert bool((k_ == torch.arange(2 * n, dtype=torch.int64, device=torch_dev)).all())
    assert bool((c_.view(-1, 2) == torch.tensor([3, 5], device=torch_dev)).all())


def test_merge_chaining(torch_dev, T):
    """Eight lists merged left to right: u32 + u32, then the u64 running result + u32."""
    from kf2vecfsw_amd import counter as C
    rng = np.random.default_rng(6)
    lists = []
    for i in range(8):
        k = np.unique(rng.integers(0, 3 * T, T + 5 * i, dtype=np.uint64))    # a small range: many shared keys
        lists.append((k, small_counts(rng, k.size)))
    ek, ec = np.zeros(0, np.uint64), np.zeros(0, np.uint64)
    for k, c in lists:
        ek, ec = expected(ek, ec, k, c)
    rk, rc = dev_keys(lists[0][0], torch_dev), dev_counts(lists[0][1], torch_dev)
    for k, c in lists[1:]:
        k_, c_, n_out, status = C.merge_sorted(rk, rc, dev_keys(k, torch_dev), dev_counts(c, torch_dev))
        n = C.merged_to_host(n_out, status)
        rk, rc = k_[:n], c_[:n]
    assert rc.element_size() == 8 and ek.size < sum(k.size for k, _ in lists) // 2
    assert np.array_equal(rk.cpu().numpy().view(np.uint64), ek) and np.array_equal(rc.cpu().numpy().view(np.uint64), ec)


# ---------------------------------------------------------------------------
# the get_kmers CLI: pieces merged as it goes
# ---------------------------------------------------------------------------
def fasta(records, width=80):
    return b"".join(b">r%d some text\n" % i + gen.wrap(s, width) for i, s in enumerate(records))


@pytest.mark.parametrize("k", [15, 31])
def test_get_kmers_pieces_with_shared_kmers(torch_dev, tmp_path, monkeypatch, k):
    """Four records of the SAME 25 kb sequence in pieces of 30,000 bytes: the pieces
    share almost all their k-mers (n_out far below n_a + n_b, counts reach 4)."""
    from kf2vecfsw_amd import main as M
    seq = gen.random_seq(np.random.default_rng(7), 25_000)
    inp = tmp_path / "in"
    inp.mkdir()
    (inp / "same.fna").write_bytes(fasta([seq] * 4))
    M.main(["get_kmers", "-input_dir", str(inp), "-output_dir", str(tmp_path / "whole"), "-k", str(k)])
    monkeypatch.setattr(M, "SPLIT_BYTES", 30_000)
    assert len(M.fasta_pieces(str(inp / "same.fna"), k, M.SPLIT_BYTES)) >= 3
    M.main(["get_kmers", "-input_dir", str(inp), "-output_dir", str(tmp_path / "pieces"), "-k", str(k)])
    whole = (tmp_path / "whole" / f"same_k{k}.npy").read_bytes()
    mat = np.load(tmp_path / "whole" / f"same_k{k}.npy")
    assert 20_000 < mat.shape[0] < 26_000 and mat[:, k].max() >= np.float32(4) / np.float32(4 * (25_000 - k + 1))
    assert (tmp_path / "pieces" / f"same_k{k}.npy").read_bytes() == whole


def test_get_kmers_directory_merges_once_per_extra_piece(torch_dev, tmp_path, monkeypatch):
    """A file of >= 3 pieces between two single-piece files: every .npy equals the
    unsplit run's, counter.merge_sorted runs exactly pieces - 1 times, and the
    sort-based host statement is never called."""
    from kf2vecfsw_amd import counter as C
    from kf2vecfsw_amd import main as M
    rng = np.random.default_rng(15)
    inp = tmp_path / "in"
    inp.mkdir()
    (inp / "m_large.fna").write_bytes(gen.random_fasta(rng, 100_000, max_records=4, n_rate=0.001))
    (inp / "a_small.fna").write_bytes(fasta([gen.random_seq(rng, 9_000)]))
    (inp / "z_small.fna").write_bytes(fasta([gen.random_seq(rng, 12_000), gen.random_seq(rng, 500)]))
    k = 21
    M.main(["get_kmers", "-input_dir", str(inp), "-output_dir", str(tmp_path / "whole"), "-k", str(k)])
    monkeypatch.setattr(M, "SPLIT_BYTES", 30_000)
    pieces = {f: len(M.fasta_pieces(str(inp / f"{f}.fna"), k, M.SPLIT_BYTES)) for f in ("a_small", "m_large", "z_small")}
    assert pieces["a_small"] == 1 and pieces["z_small"] == 1 and pieces["m_large"] >= 3
    calls = []
    real = C.merge_sorted

    def spy(*a, **kw):
        calls.append(tuple(t.numel() for t in a[:4]))
        return real(*a, **kw)

    def never(parts):
        raise AssertionError("_merge_sorted_counts is the host statement: no product path calls it")

    monkeypatch.setattr(C, "merge_sorted", spy)
    monkeypatch.setattr(M, "_merge_sorted_counts", never)
    M.main(["get_kmers", "-input_dir", str(inp), "-output_dir", str(tmp_path / "pieces"), "-k", str(k)])
    assert len(calls) == pieces["m_large"] - 1
    for f in pieces:
        whole = (tmp_path / "whole" / f"{f}_k{k}.npy").read_bytes()
        assert len(whole) > 128 and (tmp_path / "pieces" / f"{f}_k{k}.npy").read_bytes() == whole, f


def test_get_kmers_pieces_across_batches(torch_dev, tmp_path, monkeypatch):
    """-batch_gb of 50,000 bytes: every 30,000-byte piece is a batch of its own, so
    a file's running result lives across batches (its first piece is copied out of
    the batch's result, every later one merged from the next batch's), next to two
    single-piece files that are written from their batches' results."""
    from kf2vecfsw_amd import counter as C
    from kf2vecfsw_amd import main as M
    rng = np.random.default_rng(9)
    seq = gen.random_seq(rng, 30_000)
    inp = tmp_path / "in"
    inp.mkdir()
    (inp / "b_first.fna").write_bytes(fasta([gen.random_seq(rng, 7_000)]))
    (inp / "m_split.fna").write_bytes(fasta([seq, seq[5_000:], gen.random_seq(rng, 40_000)]))
    (inp / "y_last.fna").write_bytes(fasta([gen.random_seq(rng, 3_000)]))
    k = 17
    M.main(["get_kmers", "-input_dir", str(inp), "-output_dir", str(tmp_path / "whole"), "-k", str(k)])
    monkeypatch.setattr(M, "SPLIT_BYTES", 30_000)
    pieces = len(M.fasta_pieces(str(inp / "m_split.fna"), k, M.SPLIT_BYTES))
    assert pieces >= 3
    calls = []
    real = C.merge_sorted
    monkeypatch.setattr(C, "merge_sorted", lambda *a, **kw: calls.append(1) or real(*a, **kw))
    M.main(["get_kmers", "-input_dir", str(inp), "-output_dir", str(tmp_path / "pieces"), "-k", str(k),
            "-batch_gb", repr(50_000 / (1 << 30))])
    assert len(calls) == pieces - 1
    for f in ("b_first", "m_split", "y_last"):
        whole = (tmp_path / "whole" / f"{f}_k{k}.npy").read_bytes()
        assert len(whole) > 128 and (tmp_path / "pieces" / f"{f}_k{k}.npy").read_bytes() == whole, f
