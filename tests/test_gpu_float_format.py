"""GPU tests of the float formatter: kf_format_float_rows against its host
statement (tables.format_float_rows_host: Python's repr and numpy's str) byte
for byte -- the text, every row's offset and the status -- with d_text between
sentinel bytes and d_row_off and d_status between sentinel words that must stay
intact whatever the input; the text read back on the device by
kf_parse_tsv_floats; and kf_sq_distances against query.sq_distances_host bit
for bit."""
import numpy as np
import pytest

import test_host_float_format as H

pytestmark = pytest.mark.gpu

GUARD = 64                # sentinel bytes on either side of d_text
SENTINEL = 0xA7
SHORTEST, WIDENED = 0, 1
FORMS = [(np.float64, SHORTEST), (np.float32, SHORTEST), (np.float32, WIDENED)]
FORM_IDS = ["float64", "float32", "float32-widened"]


@pytest.fixture(scope="module")
def dev(native):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu tests need an MI355X")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def tile(native):
    return int(native.kf_format_float_tile())


def run(dev, vals, prefixes, rpre, mode, sep, eol, nan_empty, cap, shift=0, pre_off=None):
    """kf_format_float_rows with d_text (at `shift` bytes past a 256-byte boundary)
    between sentinel bytes and d_row_off, d_status between sentinel words: (text
    bytes [cap], row_off, status) on the host, after the sentinels were found intact."""
    import torch
    from kf2vecfsw_amd import _native as N
    vals = np.ascontiguousarray(vals)
    n, ncols = vals.shape
    bits = vals.view(np.int32 if vals.itemsize == 4 else np.int64)
    d_vals = torch.from_numpy(bits.copy()).to(dev) if vals.size else torch.zeros(8, dtype=torch.int64, device=dev)
    blob = b"".join(prefixes)
    if pre_off is None:
        pre_off = np.cumsum([0] + [len(p) for p in prefixes])
    d_pre = torch.from_numpy(np.frombuffer(blob + b"\0", dtype=np.uint8).copy()).to(dev)
    d_pre_off = torch.from_numpy(np.asarray(pre_off, dtype=np.int64)).to(dev)
    d_rpre = torch.from_numpy(np.asarray(list(rpre) + [0], dtype=np.uint32).view(np.int32).copy()).to(dev)
    buf = torch.full((512 + shift + cap + GUARD,), SENTINEL, dtype=torch.uint8, device=dev)
    t0 = (-buf.data_ptr()) % 256 + 256 + shift            # d_text = shift mod 256, sentinels on either side
    assert t0 >= GUARD and t0 + cap + GUARD <= buf.numel()
    row_off = torch.full((n + 3,), -7, dtype=torch.int64, device=dev)
    status = torch.full((6,), -7, dtype=torch.int64, device=dev)
    need = N.lib().kf_format_float_scratch_bytes(n, ncols)
    scratch = torch.empty(need // 8 + 1, dtype=torch.int64, device=dev)
    eol_b = eol.encode()
    N.check(N.lib().kf_format_float_rows(d_vals.data_ptr(), vals.itemsize, n, ncols, mode, ord(sep),
                                         eol_b[0] | (eol_b[1] << 8 if len(eol_b) == 2 else 0), len(eol_b),
                                         int(nan_empty), d_pre.data_ptr(), d_pre_off.data_ptr(), len(prefixes),
                                         d_rpre.data_ptr(), buf.data_ptr() + t0, cap, row_off[1:].data_ptr(),
                                         status[1:].data_ptr(), scratch.data_ptr(), need,
                                         torch.cuda.current_stream(dev).cuda_stream), "kf_format_float_rows")
    host = buf.cpu().numpy()
    assert (host[:t0] == SENTINEL).all() and (host[t0 + cap:] == SENTINEL).all(), "written outside d_text"
    row_off, status = row_off.cpu().numpy(), status.cpu().numpy()
    assert row_off[0] == row_off[-1] == -7 and status[0] == status[-1] == -7, "written outside row_off or status"
    return host[t0: t0 + cap].tobytes(), row_off[1:-1], tuple(int(x) for x in status[1:5])


def check(dev, vals, labels, mode, sep="\t", eol="\r\n", nan_empty=False, shift=0):
    """The kernel equals the statement with cap_bytes equal to the text's size; returns the text."""
    from kf2vecfsw_amd import tables as T
    n = vals.shape[0]
    exp, eoff = T.format_float_rows_host(vals, labels, mode, sep, eol, nan_empty)
    prefixes = [b""] if labels is None else [x if isinstance(x, bytes) else x.encode() for x in labels]
    rpre = [0] * n if labels is None else list(range(n))
    got, off, status = run(dev, vals, prefixes, rpre, mode, sep, eol, nan_empty, len(exp), shift)
    assert status == (0, len(exp), 0, 0)
    assert off.tolist() == eoff.tolist()
    assert got == exp
    return exp


def mixed(dtype, shape, seed):
    """Values of every kind of text: random bit patterns (any exponent), a few of magnitude one, zeros, NaN, inf."""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    if dtype == np.float32:
        a = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32).view(np.float32).copy()
    else:
        a = rng.integers(0, 1 << 64, n, dtype=np.uint64, endpoint=False).view(np.float64).copy()
    pick = rng.integers(0, 8, n)
    a[pick == 0] = rng.standard_normal(int((pick == 0).sum())).astype(dtype)
    a[pick == 1] = 0.0
    a[pick == 2] = rng.integers(-1000, 1000, int((pick == 2).sum())).astype(dtype)
    a[::97] = np.nan
    a[5::193] = np.inf
    a[7::211] = -np.inf
    return a.reshape(shape)


def labels_of(n, lo=0, hi=40):
    """Labels of lengths lo..hi in turn, so that lines start at every 16-byte phase."""
    return [("L%d_" % r + "x" * 64)[: lo + r % (hi - lo + 1)] for r in range(n)]


@pytest.mark.parametrize("dtype,mode", FORMS, ids=FORM_IDS)
def test_no_rows_and_one_row(dev, dtype, mode):
    got, off, status = run(dev, np.zeros((0, 5), dtype), [b"a"], [], mode, "\t", "\n", False, 16)
    assert status == (0, 0, 0, 0) and off.tolist() == [0]
    check(dev, mixed(dtype, (1, 1), 1), ["only"], mode)
    check(dev, mixed(dtype, (1, 9), 2), None, mode, eol="\n")


@pytest.mark.parametrize("dtype,mode", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("which", ["1", "7", "T-1", "T", "T+1"])
def test_column_counts(dev, tile, dtype, mode, which):
    ncols = {"1": 1, "7": 7, "T-1": tile - 1, "T": tile, "T+1": tile + 1}[which]
    n = 5 if ncols >= tile - 1 else 700             # more than one workgroup either way
    vals = mixed(dtype, (n, ncols), ncols)
    check(dev, vals, labels_of(n), mode, shift=ncols % 16)
    check(dev, vals, None, mode, sep=",", eol="\n", nan_empty=True, shift=3)


@pytest.mark.parametrize("dtype,mode", FORMS, ids=FORM_IDS)
def test_prefix_lengths_and_phases(dev, dtype, mode):
    n = 41 * 4
    vals = mixed(dtype, (n, 3), 41)
    text = check(dev, vals, labels_of(n), mode)
    assert text.split(b"\r\n")[0].count(b"\t") == 2          # the empty label writes no leading separator
    for shift in (1, 15):
        check(dev, vals, labels_of(n), mode, shift=shift, eol="\n")


@pytest.mark.parametrize("dtype,mode", FORMS, ids=FORM_IDS)
def test_shortest_and_longest_fields(dev, tile, dtype, mode):
    """A row of all 0.0 (3 bytes a field) and a row of the longest fields there are."""
    ncols = tile + 5
    vals = np.zeros((4, ncols), dtype)
    long_ = {(np.float64, SHORTEST): -1.2345678901234567e-308, (np.float32, SHORTEST): -1.17549435e-38,
             (np.float32, WIDENED): -1.2345678e-38}[(dtype, mode)]
    vals[1] = long_
    vals[3] = long_
    text = check(dev, vals, ["z", "l", "", "l2"], mode)
    lines = text.split(b"\r\n")
    from kf2vecfsw_amd import tables as T
    want_len = len(T.float_text_host(vals[1, :1], mode)[0])
    assert want_len == (24 if dtype == np.float64 else 23 if mode == WIDENED else 14)   # a float32 has no longer text
    assert set(len(f) for f in lines[1].split(b"\t")[1:]) == {want_len}
    assert lines[2] == b"\t".join([b"0.0"] * ncols)


@pytest.mark.parametrize("dtype,mode", FORMS, ids=FORM_IDS)
def test_cap_one_byte_short_is_status_1(dev, dtype, mode):
    from kf2vecfsw_amd import tables as T
    vals = mixed(dtype, (300, 11), 5)
    labels = labels_of(300)
    exp, eoff = T.format_float_rows_host(vals, labels, mode)
    pre = [x.encode() for x in labels]
    got, off, status = run(dev, vals, pre, range(300), mode, "\t", "\r\n", False, len(exp) - 1, shift=9)
    assert status == (1, len(exp), 0, 0)                     # and run() found nothing written past the cap
    assert off.tolist() == eoff.tolist()
    got, off, status = run(dev, vals, pre, range(300), mode, "\t", "\r\n", False, 0)
    assert status == (1, len(exp), 0, 0)


def test_bad_prefix_table_is_status_2(dev):
    vals = mixed(np.float32, (10, 4), 6)
    pre = [b"a", b"bb", b"ccc"]
    rpre = [0, 1, 2, 0, 1, 2, 3, 0, 1, 2]                    # row 6: prefix 3 of 3
    got, off, status = run(dev, vals, pre, rpre, WIDENED, "\t", "\n", False, 4096)
    assert status == (2, 0, 6, 0) and off[-1] == 0
    assert set(got) == {SENTINEL}                            # nothing is formatted
    got, off, status = run(dev, vals, pre, [0] * 10, WIDENED, "\t", "\n", False, 4096, pre_off=[0, 3, 1, 6])
    assert status[0] == 2 and off[-1] == 0 and set(got) == {SENTINEL}


@pytest.fixture(scope="module")
def value_sets():
    """The value sets of the CPU test (test_host_float_format) as one matrix per
    width.  The edges, the powers of ten and the switch neighbours are whole; the
    random patterns (2^17 of the CPU test's 2^20) and the integers (0..29,999 and
    the 40,000 below 2^24 + 2, where float32 stops holding every integer) are
    subsets: the expected text comes from Python, a microsecond a value, and the
    device runs the inline code that the CPU test puts through the whole sets."""
    f32 = np.concatenate([H.f32_edges(), H.f32_powers_of_ten(), H.f32_switch(),
                          np.arange((1 << 24) - 40000, (1 << 24) + 3, dtype=np.float64).astype(np.float32),
                          np.arange(0, 30000, dtype=np.float32), H.random_bits(np.uint32, 1 << 17)])
    f64 = np.concatenate([H.f64_edges(), H.f64_switch(), H.random_bits(np.uint64, 1 << 17),
                          np.array([0.0, -0.0, np.inf, -np.inf, np.nan])])
    return {np.float32: f32[: f32.size // 13 * 13].reshape(-1, 13), np.float64: f64[: f64.size // 13 * 13].reshape(-1, 13)}


@pytest.mark.parametrize("dtype,mode", FORMS, ids=FORM_IDS)
def test_cpu_value_sets(dev, value_sets, dtype, mode):
    check(dev, value_sets[dtype], None, mode, eol="\n", nan_empty=(mode == SHORTEST))


def test_python_wrappers(dev):
    """tables.format_float_rows (labels, the cut into calls) against the statement."""
    import torch
    from kf2vecfsw_amd import tables as T
    vals = mixed(np.float32, (50, 6), 8)
    labels = [T.quote_label(x).decode() for x in labels_of(48) + ["a\tb", 'q"']]
    exp, eoff = T.format_float_rows_host(vals, labels, T.KF_FLOAT_WIDENED)
    text, off = T.format_float_rows(torch.from_numpy(vals).to(dev), labels, T.KF_FLOAT_WIDENED)
    assert text.cpu().numpy().tobytes() == exp and off.tolist() == eoff.tolist()
    old = T.C.KF_FORMAT_MAX_CAP
    T.C.KF_FORMAT_MAX_CAP = 7 * T.float_row_bound(6, 44)     # seven rows a call
    try:
        text, off = T.format_float_rows(torch.from_numpy(vals).to(dev), labels, T.KF_FLOAT_WIDENED)
    finally:
        T.C.KF_FORMAT_MAX_CAP = old
    assert text.cpu().numpy().tobytes() == exp and off.tolist() == eoff.tolist()


# ---------------------------------------------------------------- round trip on the device
def test_round_trip_through_kf_parse_tsv_floats(dev):
    import torch
    from kf2vecfsw_amd import counter as C
    from kf2vecfsw_amd import tables as T
    rng = np.random.default_rng(12)
    a = rng.integers(0, 1 << 64, 4000 * 9, dtype=np.uint64, endpoint=False).view(np.float64).copy()
    a[~np.isfinite(a) | (np.abs(a) < np.finfo(np.float64).tiny)] = 1.5      # the parser takes normal values, zero and nan
    a[::50] = 0.0
    a[3::77] = np.nan
    a = a.reshape(4000, 9)
    labels = ["r%d" % i for i in range(4000)]
    text, off = T.format_float_rows(torch.from_numpy(a).to(dev), labels, T.KF_FLOAT_SHORTEST, eol="\n")
    data = torch.zeros((int(off[-1]) + 15) // 16 * 16, dtype=torch.uint8, device=dev)
    data[: int(off[-1])] = text
    vals, row_name, unit_row0, status = T.parse_tsv_floats(data, np.asarray([0, int(off[-1])], dtype=np.int64), 9)
    row0 = C.parsed_to_host(unit_row0, status, ["<text>"], [0], [0], what="kf_parse_tsv_floats")
    assert int(row0[-1]) == 4000
    back = vals[:4000].cpu().numpy()
    nan = np.isnan(a)
    assert np.array_equal(np.isnan(back), nan)
    assert np.array_equal(back.view(np.uint64)[~nan], a.view(np.uint64)[~nan])


# ---------------------------------------------------------------- distances
@pytest.fixture(scope="module")
def sq_tile(native):
    return int(native.kf_sq_distances_tile())


@pytest.mark.parametrize("D", [1, 3, 16, 257])
def test_sq_distances_bit_for_bit(dev, sq_tile, D):
    import torch
    from kf2vecfsw_amd import query as Q
    U = sq_tile
    sizes = [1, U - 1, U, U + 1]
    xs, ys = H.sq_inputs(U + 1, U + 1, D, seed=7)
    for q in sizes:
        for b in sizes:
            x, y = xs[:q], ys[:b]
            want = Q.sq_distances_host(x, y)
            got = Q.sq_distances(torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)).cpu().numpy()
            assert got.shape == (q, b) and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (q, b)
            if min(q, b) >= 3:
                assert got[0, 0] == 0 and got[1, 1] == 0 and got[2, 2] > 1e-6


def test_sq_distances_cut_into_calls_and_empty(dev, sq_tile):
    import torch
    from kf2vecfsw_amd import query as Q
    U = sq_tile
    x, y = H.sq_inputs(2 * U + 5, U + 9, 37, seed=9)
    dx, dy = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
    whole = Q.sq_distances(dx, dy)
    assert np.array_equal(whole.cpu().numpy().view(np.uint32), Q.sq_distances_host(x, y).view(np.uint32))
    for cut in (1, U - 3, U + 2):
        rows = torch.cat([Q.sq_distances(dx[:cut], dy), Q.sq_distances(dx[cut:], dy)], 0)
        cols = torch.cat([Q.sq_distances(dx, dy[:cut]), Q.sq_distances(dx, dy[cut:])], 1)
        assert torch.equal(rows.view(torch.int32), whole.view(torch.int32)), cut
        assert torch.equal(cols.view(torch.int32), whole.view(torch.int32)), cut
    assert Q.sq_distances(dx[:0], dy).shape == (0, U + 9) and Q.sq_distances(dx, dy[:0]).shape == (2 * U + 5, 0)


def test_sq_distances_many_tiles(dev, sq_tile):
    """A grid of 6 x 12 tiles, ragged on both sides, the whole matrix bit for bit: every workgroup's place in the
    output comes from its index over the tiles of B."""
    import torch
    from kf2vecfsw_amd import query as Q
    U = sq_tile
    x, y = H.sq_inputs(5 * U + 7, 11 * U + 3, 40, seed=11)
    got = Q.sq_distances(torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), Q.sq_distances_host(x, y).view(np.uint32))
