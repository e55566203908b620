"""CPU tests of the float formatter and of query's host halves: the shortest
digits and the text of csrc/kf_shortest.h (through kf_format_float_host and
kf_shortest_decimal_host, the same inline code the kernel runs) against Python's
repr and numpy's str, byte for byte; the reference's own float tables parsed by
the project's host parsers and formatted back; the inverse through
kf_decimal_to_double; kf_format_float_rows' and kf_sq_distances' C-ABI (every
refusal before any HIP call: fake non-null addresses, there is no device here);
query.sq_distances_host against torch.cdist on the CPU; classes.out, the remap
table and the label quoting."""
import csv
import io
import os

import numpy as np
import pytest

from conftest import GOLDEN

SHORTEST, WIDENED = 0, 1
TSV = os.path.join(GOLDEN, "tsv")
QUERY = os.path.join(GOLDEN, "query")


# ---------------------------------------------------------------- helpers
def fmt(L, a, mode, nan_empty=0):
    """kf_format_float_host of every value of `a`: a list of bytes."""
    from kf2vecfsw_amd import _native as N
    a = np.ascontiguousarray(a).reshape(-1)
    n = a.size
    out = np.full((n, 24), 0xEE, dtype=np.uint8)
    ln = np.zeros(n, dtype=np.uint8)
    N.check(L.kf_format_float_host(a.ctypes.data, a.itemsize, mode, nan_empty, n, out.ctypes.data, ln.ctypes.data))
    assert ln.max(initial=0) <= 24
    flat, ln = out.tobytes(), ln.tolist()
    return [flat[24 * i: 24 * i + ln[i]] for i in range(n)]


def want(a, mode, nan_empty=0):
    from kf2vecfsw_amd import tables as T
    return [x.encode() for x in T.float_text_host(np.ascontiguousarray(a).reshape(-1), mode, bool(nan_empty))]


def check(L, a, mode, nan_empty=0, step=1 << 20):
    a = np.ascontiguousarray(a).reshape(-1)
    for i in range(0, a.size, step):
        got, exp = fmt(L, a[i: i + step], mode, nan_empty), want(a[i: i + step], mode, nan_empty)
        if got != exp:
            bad = [(a[i + j].tobytes().hex(), g, e) for j, (g, e) in enumerate(zip(got, exp)) if g != e]
            raise AssertionError("{} of {} differ (bits little-endian, got, expected): {}".format(
                len(bad), len(got), bad[:8]))


def f32_bits(b):
    return np.asarray(b, dtype=np.uint32).view(np.float32)


def f64_bits(b):
    return np.asarray(b, dtype=np.uint64).view(np.float64)


def f32_edges():
    man = np.array([0, 1, 2, 0x400000, 0x7FFFFE, 0x7FFFFF], dtype=np.uint32)
    ex = np.arange(256, dtype=np.uint32)
    b = (ex[:, None] << 23 | man[None, :]).reshape(-1)
    return f32_bits(np.concatenate([b, b | np.uint32(1 << 31)]))


def f32_powers_of_ten():
    b = np.array([np.float32(float("1e%d" % e)) for e in range(-45, 39)], dtype=np.float32).view(np.uint32).astype(np.int64)
    b = np.concatenate([b - 1, b, b + 1])
    return f32_bits(b[(b >= 0) & (b < 0x7F800000)].astype(np.uint32))


def f32_switch():
    """Neighbours of 1e-4 and 1e16 among the float32."""
    out = []
    for v in (1e-4, 1e16):
        b = int(np.float32(v).view(np.uint32))
        out += list(range(b - 8, b + 9))
    b = np.asarray(out, dtype=np.uint32)
    return f32_bits(np.concatenate([b, b | np.uint32(1 << 31)]))


def f64_switch():
    out = []
    for v in (1e-4, 1e16):
        b = int(np.float64(v).view(np.uint64))
        out += list(range(b - 8, b + 9))
    b = np.asarray(out, dtype=np.uint64)
    return f64_bits(np.concatenate([b, b | np.uint64(1 << 63)]))


def f64_edges():
    man = np.array([0, 1, 2, 1 << 51, (1 << 52) - 2, (1 << 52) - 1], dtype=np.uint64)
    ex = np.arange(2047, dtype=np.uint64)
    b = (ex[:, None] << np.uint64(52) | man[None, :]).reshape(-1)
    return f64_bits(np.concatenate([b, b | np.uint64(1 << 63)]))


def random_bits(dtype, n=1 << 20, seed=20):
    rng = np.random.default_rng(seed)
    if dtype == np.uint32:
        return f32_bits(rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32))
    return f64_bits(rng.integers(0, 1 << 64, n, dtype=np.uint64, endpoint=False))


F32_MODES = [SHORTEST, WIDENED]


# ---------------------------------------------------------------- digits and text
@pytest.mark.parametrize("mode", F32_MODES)
def test_float32_every_exponent(native, mode):
    check(native, f32_edges(), mode)


@pytest.mark.parametrize("mode", F32_MODES)
def test_float32_powers_of_ten(native, mode):
    check(native, f32_powers_of_ten(), mode)


def test_notation_switch_at_1e_minus_4_and_1e16(native):
    """The switch between fixed and exponent notation falls at different values
    for the three forms: numpy decides by the value (float32(1e-4) is below 1e-4:
    "1e-04"), repr by the decimal exponent of the shortest digits."""
    check(native, f32_switch(), SHORTEST)
    check(native, f32_switch(), WIDENED)
    check(native, f64_switch(), SHORTEST)
    assert fmt(native, np.float32([1e-4, 1e16]), SHORTEST) == [b"1e-04", b"1e+16"]
    assert fmt(native, np.float32([1e-4, 1e16]), WIDENED) == [b"9.999999747378752e-05", b"1.0000000272564224e+16"]
    assert fmt(native, np.float64([1e-4, 1e16, 9999999999999998.0]), SHORTEST) == [b"0.0001", b"1e+16",
                                                                                   b"9999999999999998.0"]


@pytest.mark.parametrize("mode", F32_MODES)
def test_float32_integers(native, mode):
    check(native, np.arange((1 << 24) + 3, dtype=np.float64).astype(np.float32), mode)


@pytest.mark.parametrize("mode", F32_MODES)
def test_float32_random_bits(native, mode):
    check(native, random_bits(np.uint32), mode)


def test_float64_every_exponent(native):
    check(native, f64_edges(), SHORTEST)


def test_float64_random_bits(native):
    check(native, random_bits(np.uint64), SHORTEST)


def test_float64_specials(native):
    a = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan])
    assert fmt(native, a, SHORTEST) == [b"0.0", b"-0.0", b"inf", b"-inf", b"nan", b"nan"]
    check(native, a, SHORTEST)
    check(native, a.astype(np.float32), SHORTEST)
    check(native, a.astype(np.float32), WIDENED)


def test_float64_subnormals_are_formatted(native):
    """The contract allows a float64 subnormal to be refused; they are formatted, and right."""
    a = f64_bits([1, 2, 3, 0xFFFFFFFFFFFFF, 0x8000000000000001, 0x000123456789ABCD])
    assert fmt(native, a[:1], SHORTEST) == [b"5e-324"]
    check(native, a, SHORTEST)


def test_nan_flag(native):
    a = np.array([1.5, np.nan, -2.0, -np.nan])
    for arr, mode in ((a, SHORTEST), (a.astype(np.float32), SHORTEST), (a.astype(np.float32), WIDENED)):
        assert fmt(native, arr, mode, 0) == [b"1.5", b"nan", b"-2.0", b"nan"]
        assert fmt(native, arr, mode, 1) == [b"1.5", b"", b"-2.0", b""]
        check(native, arr, mode, 1)


def test_longest_texts_fit_24_bytes(native):
    a = np.array([-1.2345678901234567e-308, -1.2345678901234567e+300, -0.00012345678901234567])
    got = fmt(native, a, SHORTEST)
    assert [len(x) for x in got] == [24, 24, 23] and got == want(a, SHORTEST)


def test_mode_and_width_must_agree(native):
    from kf2vecfsw_amd import _native as N
    a = np.zeros(1)
    out, ln = np.zeros(24, np.uint8), np.zeros(1, np.uint8)
    for size, mode in ((8, WIDENED), (2, SHORTEST), (4, 2)):
        assert native.kf_format_float_host(a.ctypes.data, size, mode, 0, 1, out.ctypes.data,
                                           ln.ctypes.data) == N.KF_EINVAL


# ---------------------------------------------------------------- goldens
def native_table(L, values, names, mode, eol=b"\n", nan_empty=1):
    cells = fmt(L, values, mode, nan_empty)
    nc = values.shape[1]
    return b"".join(nm + b"\t" + b"\t".join(cells[r * nc: (r + 1) * nc]) + eol for r, nm in enumerate(names))


def read_table(path, header):
    from kf2vecfsw_amd import tables as T
    data = open(path, "rb").read()
    vals, names, _ = T.table_host(data, header, path=path)
    body = data.split(b"\n", 1)[1] if header else data
    return vals, [nm.encode() for nm in names], body


@pytest.mark.parametrize("name", sorted(f for f in os.listdir(TSV) if f.endswith(".di_mtrx")))
def test_golden_distance_matrices_float64(native, name):
    vals, names, body = read_table(os.path.join(TSV, name), True)
    assert vals.size and native_table(native, vals, names, SHORTEST) == body


@pytest.mark.parametrize("path,header", [(os.path.join(TSV, "embeddings_subtree_0.csv"), False),
                                         (os.path.join(QUERY, "embedding_query_G000196015.emb"), False),
                                         (os.path.join(QUERY, "distortions_subtree_1.csv"), True)])
def test_golden_float32_tables(native, path, header):
    """pandas' to_csv of float32 frames and numpy's str print the float32's own shortest digits."""
    vals, names, body = read_table(path, header)
    v32 = vals.astype(np.float32)
    assert vals.size and native_table(native, v32, names, SHORTEST) == body
    # the widened form of the same values is another text: the double's 17 digits
    assert native_table(native, v32, names, WIDENED) != body


# ---------------------------------------------------------------- the inverse
def decimal_of(L, a, mode):
    from kf2vecfsw_amd import _native as N
    a = np.ascontiguousarray(a)
    w, q, cls = np.zeros(a.size, np.uint64), np.zeros(a.size, np.int32), np.zeros(a.size, np.uint8)
    N.check(L.kf_shortest_decimal_host(a.ctypes.data, a.itemsize, mode, a.size, w.ctypes.data, q.ctypes.data,
                                       cls.ctypes.data))
    return w, q, cls


def to_double(L, w, q):
    from kf2vecfsw_amd import _native as N
    out, ok = np.zeros(w.size, np.float64), np.zeros(w.size, np.uint8)
    N.check(L.kf_decimal_to_double(w.ctypes.data, q.ctypes.data, w.size, out.ctypes.data, ok.ctypes.data))
    return out, ok


def test_inverse_float64(native):
    a = random_bits(np.uint64)
    w, q, cls = decimal_of(native, a, SHORTEST)
    fin = (cls & 0x7F) == 0
    assert np.array_equal(fin, np.isfinite(a) & (a != 0))
    assert w[fin].max() < 10 ** 17 and np.all(w[fin] % 10 != 0)
    back, ok = to_double(native, w, q)
    normal = fin & (np.abs(a) >= np.finfo(np.float64).tiny)      # the parser produces no subnormal
    assert np.all(ok[normal] == 1)
    assert np.array_equal(back[normal].view(np.uint64), np.abs(a[normal]).view(np.uint64))
    assert np.array_equal((cls >> 7).astype(bool), np.signbit(a))


@pytest.mark.parametrize("mode", F32_MODES)
def test_inverse_float32(native, mode):
    a = random_bits(np.uint32)
    w, q, cls = decimal_of(native, a, mode)
    fin = (cls & 0x7F) == 0
    assert np.array_equal(fin, np.isfinite(a) & (a != 0))
    assert w[fin].max() < (10 ** 9 if mode == SHORTEST else 10 ** 17)
    back, ok = to_double(native, w, q)       # every float32, subnormals too, is a normal double
    assert np.all(ok[fin] == 1)
    with np.errstate(over="ignore"):
        back32 = back.astype(np.float32)     # the decimal rounded to double, then once more: what the parsers store
    assert np.array_equal(back32[fin].view(np.uint32), np.abs(a[fin]).view(np.uint32))
    if mode == WIDENED:
        assert np.array_equal(back[fin], np.abs(a[fin]).astype(np.float64))


# ---------------------------------------------------------------- the C-ABI
def fake(i, off=0):
    """A fake device address, aligned to 4 KiB plus `off`."""
    return (0x7000_0000_0000 + (i << 32)) + off


def call(L, **kw):
    a = dict(vals=fake(1), val_bytes=4, n_rows=64, ncols=100, mode=WIDENED, sep=9, eol=0x0A0D, eol_len=2, nan_empty=0,
             pre=fake(2), pre_off=fake(3), n_pre=3, rpre=fake(4), text=fake(6), cap=1 << 20, row_off=fake(7),
             st=fake(8), scratch=fake(9), scratch_bytes=None, stream=None)
    a.update(kw)
    if a["scratch_bytes"] is None:
        a["scratch_bytes"] = L.kf_format_float_scratch_bytes(a["n_rows"], a["ncols"])
    return L.kf_format_float_rows(a["vals"], a["val_bytes"], a["n_rows"], a["ncols"], a["mode"], a["sep"], a["eol"],
                                  a["eol_len"], a["nan_empty"], a["pre"], a["pre_off"], a["n_pre"], a["rpre"],
                                  a["text"], a["cap"], a["row_off"], a["st"], a["scratch"], a["scratch_bytes"],
                                  a["stream"])


def test_symbols_exported(native):
    from kf2vecfsw_amd import _native as N
    for s in ("kf_format_float_rows", "kf_format_float_scratch_bytes", "kf_format_float_host", "kf_format_float_tile",
              "kf_shortest_decimal_host", "kf_sq_distances", "kf_sq_distances_tile"):
        assert hasattr(native, s) and s in N.SIGNATURES, s
    assert native.kf_format_float_tile() > 0 and native.kf_sq_distances_tile() > 0


def test_scratch_bytes_grow_with_every_argument(native):
    f = native.kf_format_float_scratch_bytes
    T = native.kf_format_float_tile()
    rows = [0, 1, 2, 255, 256, 257, 4096, 1 << 20, (1 << 31) - 1]
    cols = [1, 2, 7, T - 1, T, T + 1, 10000, 1 << 20]
    for c in cols:
        got = [f(n, c) for n in rows]
        assert all(x > 0 and x % 8 == 0 for x in got) and got == sorted(got), c
    for n in rows:
        got = [f(n, c) for c in cols]
        assert got == sorted(got), n
    # 8 bytes per row, 8 per tile and 16 per cell (the decimals kept between the two passes)
    assert f(4000, 10000) >= 8 * 4000 + 8 * (4000 * 10000 // T) + 16 * 4000 * 10000
    assert f(4000, 10000) < 17 * 4000 * 10000


REFUSALS = [
    ("val_bytes 2", dict(val_bytes=2), b"val_bytes"),
    ("widened float64", dict(val_bytes=8, mode=WIDENED), b"mode"),
    ("unknown mode", dict(mode=2), b"mode"),
    ("ncols 0", dict(ncols=0), b"ncols"),
    ("separator 0", dict(sep=0), b"separator"),
    ("separator 256", dict(sep=256), b"separator"),
    ("eol_len 0", dict(eol_len=0), b"eol_len"),
    ("eol_len 3", dict(eol_len=3), b"eol_len"),
    ("2^31 rows", dict(n_rows=1 << 31, ncols=1), b"fewer than 2^31"),
    ("cap of 4 GiB", dict(cap=1 << 32), b"at most 4 GiB"),
    ("cap above 4 GiB", dict(cap=(1 << 40) + 1), b"at most 4 GiB"),
    ("negative n_prefixes", dict(n_pre=-1), b"negative prefix count"),
    ("too many cells", dict(n_rows=(1 << 31) - 1, ncols=1 << 21), b"cells"),
    ("cells overflow", dict(n_rows=(1 << 31) - 1, ncols=1 << 40), b"cells"),
    ("null vals", dict(vals=None), b"null d_vals"),
    ("null prefix bytes", dict(pre=None), b"null d_prefix_bytes"),
    ("null prefix_off", dict(pre_off=None), b"null d_prefix_off"),
    ("null row_prefix", dict(rpre=None), b"null d_row_prefix"),
    ("null text", dict(text=None), b"null d_text"),
    ("null row_off", dict(row_off=None), b"null d_row_off"),
    ("null status", dict(st=None), b"null d_status"),
    ("null scratch", dict(scratch=None), b"null d_scratch"),
    ("float32 off by 2", dict(vals=fake(1, 2)), b"misaligned d_vals"),
    ("float64 off by 4", dict(vals=fake(1, 4), val_bytes=8, mode=SHORTEST), b"misaligned d_vals"),
    ("row_prefix off by 2", dict(rpre=fake(4, 2)), b"misaligned d_row_prefix"),
    ("prefix_off off by 4", dict(pre_off=fake(3, 4)), b"misaligned d_prefix_off"),
    ("row_off off by 4", dict(row_off=fake(7, 4)), b"misaligned d_row_off"),
    ("status off by 4", dict(st=fake(8, 4)), b"misaligned d_status"),
    ("scratch off by 4", dict(scratch=fake(9, 4)), b"misaligned d_scratch"),
    ("null row_off without rows", dict(n_rows=0, row_off=None), b"null d_row_off"),
    ("null status without rows", dict(n_rows=0, st=None), b"null d_status"),
]


@pytest.mark.parametrize("what,kw,msg", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_format_float_rows_refuses_before_any_hip_call(native, what, kw, msg):
    from kf2vecfsw_amd import _native as N
    assert call(native, **kw) == N.KF_EINVAL, what
    assert msg in native.kf_last_error(), native.kf_last_error()


def test_format_float_rows_small_scratch_is_erange(native):
    from kf2vecfsw_amd import _native as N
    need = native.kf_format_float_scratch_bytes(64, 100)
    assert call(native, scratch_bytes=need - 1) == N.KF_ERANGE
    assert str(need).encode() in native.kf_last_error()


SQ_REFUSALS = [
    ("D 0", dict(D=0), b"D == 0"),
    ("null x", dict(x=None), b"null d_x"),
    ("null y", dict(y=None), b"null d_y"),
    ("null out", dict(out=None), b"null d_out"),
    ("x off by 2", dict(x=fake(1, 2)), b"misaligned d_x"),
    ("y off by 1", dict(y=fake(2, 1)), b"misaligned d_y"),
    ("out off by 2", dict(out=fake(3, 2)), b"misaligned d_out"),
    ("too many tiles", dict(Q=1 << 30, B=1 << 30), b"tiles"),
]


@pytest.mark.parametrize("what,kw,msg", SQ_REFUSALS, ids=[r[0] for r in SQ_REFUSALS])
def test_sq_distances_refuses_before_any_hip_call(native, what, kw, msg):
    from kf2vecfsw_amd import _native as N
    a = dict(x=fake(1), Q=100, y=fake(2), B=100, D=16, out=fake(3))
    a.update(kw)
    assert native.kf_sq_distances(a["x"], a["Q"], a["y"], a["B"], a["D"], a["out"], None) == N.KF_EINVAL, what
    assert msg in native.kf_last_error(), native.kf_last_error()


def test_sq_distances_empty_sides_are_valid(native):
    from kf2vecfsw_amd import _native as N
    assert native.kf_sq_distances(None, 0, fake(2), 5, 16, None, None) == N.KF_OK
    assert native.kf_sq_distances(fake(1), 5, None, 0, 16, None, None) == N.KF_OK


# ---------------------------------------------------------------- distances on the host
def sq_inputs(Q, B, D, seed=0):
    """Random rows, with exact duplicates (distance 0) and rows that differ from
    a row of x by 1e-4 or by 2e-3 in one coordinate: below and above the cut at 1e-6."""
    rng = np.random.default_rng(seed + 1000 * D)
    x = rng.standard_normal((Q, D)).astype(np.float32)
    y = rng.standard_normal((B, D)).astype(np.float32)
    for j in range(min(Q, B, 3)):
        y[j] = x[j]
    if min(Q, B) >= 2:
        y[1, D // 2] += np.float32(1e-4)
    if min(Q, B) >= 3:
        y[2, D - 1] += np.float32(2e-3)
    return x, y


@pytest.mark.parametrize("D", [1, 3, 16, 257, 1024])
def test_sq_distances_host_and_cdist_within_the_bound(D):
    """Both the host statement and the reference's lines (torch.cdist in the
    direct form, squared, cut) against the float64 value of the same float32
    inputs.  The bound, relative (D + 8) * 2^-24, is one rounding each for the
    difference and the product of a term, at most D - 1 for the sum in any order,
    the square root and the square, to first order; it is not measured."""
    import torch
    from kf2vecfsw_amd import query as Q
    x, y = sq_inputs(9, 11, D)
    exact = ((x.astype(np.float64)[:, None, :] - y.astype(np.float64)[None, :, :]) ** 2).sum(-1)
    bound = (D + 8) * 2.0 ** -24
    assert not np.any(np.abs(exact - 1e-6) <= bound * 1e-6), "an exact value too close to the cut to be checked"
    expect = np.where(exact < 1e-6, 0.0, exact)
    assert (expect == 0).sum() >= 2 and (expect[2, 2] > 1e-6)
    host = Q.sq_distances_host(x, y)
    ref = torch.cdist(torch.from_numpy(x), torch.from_numpy(y), p=2, compute_mode="donot_use_mm_for_euclid_dist")
    ref = torch.square(ref)
    ref = torch.where(ref < 1.0e-6, torch.tensor(0, dtype=ref.dtype), ref).numpy()
    for name, got in (("sq_distances_host", host), ("cdist", ref)):
        assert got.dtype == np.float32
        err = np.abs(got.astype(np.float64) - expect)
        worst = float((err / np.maximum(expect, 1e-300)).max())
        print("D={} {}: worst relative error {:.3g} x 2^-24 (bound {})".format(D, name, worst * 2 ** 24, D + 8))
        assert np.all(err <= bound * expect), name


# ---------------------------------------------------------------- classes.out, remap, quoting
def test_read_classes_toy():
    from kf2vecfsw_amd import query as Q
    path = os.path.join(QUERY, "classes.out")
    got = Q.read_classes(path)
    assert [c for c, _ in got] == [0, 1] and got[0][1][0] == "G000402355sub" and sum(len(g) for _, g in got) == 5
    lines = open(path).read().splitlines()[1:]
    order, by = [], {}
    for ln in lines:
        g, c = ln.split("\t")[:2]
        c = int(float(c))
        if c not in by:
            order.append(c)
        by.setdefault(c, []).append(g)
    assert got == [(c, by[c]) for c in order]
    assert all(isinstance(c, int) for c, _ in got)
    # only the genomes asked for, clades still in order of first appearance
    some = Q.read_classes(path, ["G001020955", "G000402355sub"])
    assert some == [(0, ["G000402355sub"]), (1, ["G001020955"])]


def test_read_classes_and_remap_from_text(tmp_path):
    from kf2vecfsw_amd import query as Q
    p = tmp_path / "classes.out"
    p.write_text("genome\ttop_class\ttop_p\nb\t2.0\t0.5\na\t0.0\t0.9\nc\t2.0\t0.7\n\n")
    assert Q.read_classes(str(p)) == [(2, ["b", "c"]), (0, ["a"])]
    r = tmp_path / "remap.tsv"
    r.write_text("label\tnew_label\na\tAlpha one\nc\tC\n")
    assert Q.read_remap(str(r)) == {"a": "Alpha one", "c": "C"}
    bad = tmp_path / "bad.out"
    bad.write_text("name\tclass\nx\t1\n")
    with pytest.raises(ValueError):
        Q.read_classes(str(bad))


@pytest.mark.parametrize("sep,eol", [("\t", "\r\n"), (",", "\n")])
def test_label_quoting_is_csv_writers(sep, eol):
    from kf2vecfsw_amd import tables as T
    labels = ["plain", "", "with\ttab", "with,comma", 'a "quoted" one', "line\nbreak", "cr\rhere", " spaced ", "G0001|x", 7]
    for lab in labels:
        buf = io.StringIO(newline="")
        csv.writer(buf, delimiter=sep, lineterminator=eol).writerow([lab, 1.5])
        assert buf.getvalue().encode() == T.quote_label(lab, sep, eol) + sep.encode() + b"1.5" + eol.encode(), lab
    buf = io.StringIO(newline="")
    csv.writer(buf, delimiter=sep, lineterminator=eol).writerow([""] + labels)
    assert buf.getvalue().encode() == T.header_line([""] + labels, sep, eol)


def test_format_float_rows_host_is_csv_writer_and_to_csv():
    """The host statement against the writers it restates: .tolist() + csv.writer for the widened form."""
    from kf2vecfsw_amd import tables as T
    rng = np.random.default_rng(3)
    a = rng.standard_normal((5, 7)).astype(np.float32)
    a[1, 2], a[3, 0], a[4, 6] = np.nan, 0.0, 1e-4
    labels = ["g%d" % i for i in range(5)]
    buf = io.StringIO(newline="")
    w = csv.writer(buf, delimiter="\t")
    for lab, row in zip(labels, a.tolist()):
        w.writerow([lab] + row)
    text, off = T.format_float_rows_host(a, labels, T.KF_FLOAT_WIDENED)
    assert text == buf.getvalue().encode() and off[-1] == len(text)
    assert all(text[off[i]: off[i + 1]].startswith(labels[i].encode() + b"\t") for i in range(5))
