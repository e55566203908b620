"""GPU parity of the sparse counter (kf_sparse_count) on STRUCTURED key sets: the
branches of the chunk sort, the run fix-up, the greedy chunk plan and the
overflow sort that random DNA does not reach (tests/test_gpu_sparse.py covers
the random side).

Inputs are built key by key: a record that is exactly one k-mer followed by `N`
yields exactly one window, and a k-mer whose first and last bases are A or C (or
first A, last G) is its own canonical form, so the standard 2-bit code of the
string IS the key.  Every case is compared, bit for bit, with
  * oracle.sparse_count on the bytes, and
  * np.unique of the intended codes,
and `nuniq` must be exact.

Every case also states, through `plan_model` (a pure-Python restatement of
sp2_plan_kernel and of the chunk sort's choice of path), the structural property
it exists for ("a mixed run of 33 keys starting at slot 31", "two big buckets in
genome 0"), so a case cannot quietly stop reaching its branch.  The model and the
builder are checked without a GPU by test_structured_inputs_reach_their_paths.
"""
from __future__ import annotations

import numpy as np
import pytest

# ---- constants of kf2vecfsw_amd/csrc/kf_sparse.hip, restated (a matching
# comment sits next to each of them there)
KBD = 10                  # kBD: bucket bits, D = min(kBD, 2k)
CAP4 = 24 * 512           # kCPer4 * kCBlock: keys of a chunk, u32 keys (k <= 16)
CAP8 = 32 * 512           # kCPer8 * kCBlock: keys of a chunk, u64 keys
KDB = 10                  # kDB: bits of one LDS pass
MSD_BITS = KDB * 2        # kDB * kMsdPasses: the top bits sorted before the fix-up
KRUN = 32                 # kRun: the longest run the owner thread insertion-sorts
TILE4, TILE8 = 16384, 8192   # TileOf<u32>::tile, TileOf<u64>::tile (overflow LSD passes)

ORDERS = ("asc", "desc", "shuf")


def dims(k):
    d = min(KBD, 2 * k)
    return d, 2 * k - d


def cap_of(k):
    return CAP4 if k <= 16 else CAP8


def tile_of(k):
    return TILE4 if k <= 16 else TILE8


def ceil_log2(x):
    return 0 if x <= 1 else (x - 1).bit_length()


# ---------------------------------------------------------------- input builder
_ACGT = np.frombuffer(b"ACGT", np.uint8)
U = np.uint64


def genome(codes, k, width=None, header=b">g\n"):
    """FASTA bytes whose windows are exactly `codes` (standard 2-bit codes, in this
    order): each k-mer is a record body piece of its own, `N` between them.
    width: wrap the body so k-mers straddle lines ('\\n' is transparent)."""
    codes = np.asarray(codes, U)
    if codes.size == 0:
        return header
    assert k == 32 or not (codes >> U(2 * k)).any()
    first, last = codes >> U(2 * k - 2), codes & U(3)
    # its own canonical form: the reverse complement starts with G or T (C after A)
    assert (((first <= 1) & (last <= 1)) | ((first == 0) & (last == 2))).all(), "not self-canonical"
    sh = (2 * np.arange(k - 1, -1, -1)).astype(U)
    rows = np.full((codes.size, k + 1), ord("N"), np.uint8)
    rows[:, :k] = _ACGT[((codes[:, None] >> sh[None, :]) & U(3)).astype(np.intp)]
    body = rows.reshape(-1)[:-1]
    if width:
        n = body.size
        out = np.full(n + (n + width - 1) // width, ord("\n"), np.uint8)
        i = np.arange(n)
        out[i + i // width] = body
        return header + out.tobytes()
    return header + body.tobytes() + b"\n"


def window_codes(seq, k):
    """Canonical codes of every window of an N-free sequence (2-bit codes), in
    plain numpy: the second reference of the dense cases."""
    seq = np.asarray(seq, U)
    n = seq.size - k + 1
    fw, rc = np.zeros(n, U), np.zeros(n, U)
    for j in range(k):
        b = seq[j: j + n]
        fw = (fw << U(2)) | b
        rc |= (U(3) - b) << U(2 * j)
    return np.minimum(fw, rc)


def lows(j, first_a=False):
    """The j-th value whose last base keeps a k-mer self-canonical (monotone in
    j): last base A or C, and G too when the first base is A."""
    j = np.asarray(j, U)
    if first_a:
        return ((j // U(3)) << U(2)) | (j % U(3))
    return ((j >> U(1)) << U(2)) | (j & U(1))


def ordered(codes, how, seed=0):
    codes = np.sort(np.asarray(codes, U))
    if how == "asc":
        return codes
    if how == "desc":
        return codes[::-1].copy()
    return np.random.default_rng(seed).permutation(codes)


def distinct_idx(rng, limit, n):
    """n indices below limit, distinct while the range has room."""
    limit = int(limit)
    if limit <= (1 << 20):
        p = rng.permutation(limit).astype(U)
        return p[:n] if n <= limit else np.concatenate([p, rng.integers(0, limit, n - limit).astype(U)])
    u = np.unique(rng.integers(0, limit, 2 * n + 64).astype(U))
    assert u.size >= n
    return rng.permutation(u)[:n]


def bucket_keys(rng, k, bucket, n, dup=0.0):
    """n keys of one bucket: distinct low parts where the bucket has room, a
    share `dup` of them repeats of the others."""
    _, B = dims(k)
    fa = bucket < (1 << (KBD - 2))
    room = (3 if fa else 2) << (B - 2)
    nd = n - int(n * dup)
    idx = distinct_idx(rng, room, nd)
    if nd < n:
        idx = np.concatenate([idx, idx[rng.integers(0, nd, n - nd)]])
    return (U(bucket) << U(B)) | lows(idx, fa)


# ---------------------------------------------------------------- reachability model
class ChunkInfo:
    """One chunk of sp2_plan_kernel's plan and what sp2_chunk_kernel does with it."""

    def __init__(self, blo, nb, keys, big, B):
        self.blo, self.nb, self.nkeys, self.big = blo, nb, int(keys.size), big
        self.R = B + ceil_log2(nb)
        self.ndistinct = int(np.unique(keys).size)
        self.msd = not big and self.R > MSD_BITS
        self.run_start = self.run_len = np.zeros(0, np.int64)
        self.run_equal = np.zeros(0, bool)
        if self.msd:
            rel = keys - (U(blo) << U(B))
            top = rel >> U(self.R - MSD_BITS)
            st = np.concatenate([[0], np.flatnonzero(top[1:] != top[:-1]) + 1]).astype(np.int64)
            en = np.concatenate([st[1:], [keys.size]]).astype(np.int64)
            self.run_start, self.run_len = st, en - st
            self.run_equal = rel[st] == rel[en - 1]     # sorted: equal ends, equal run

    def runs(self, lo=2, hi=None, equal=None):
        """Lengths of the runs of lo..hi keys (equal: only all-equal / only mixed ones)."""
        m = self.run_len >= lo
        if hi is not None:
            m &= self.run_len <= hi
        if equal is not None:
            m &= self.run_equal == equal
        return sorted(self.run_len[m].tolist())

    @property
    def short(self):        # insertion-sorted by the owner thread
        return self.runs(2, KRUN)

    @property
    def mixed_long(self):   # each of these sends the chunk through the second round
        return self.runs(KRUN + 1, None, equal=False)

    @property
    def equal_long(self):
        return self.runs(KRUN + 1, None, equal=True)

    @property
    def second_round(self):
        return bool(self.mixed_long)

    def run_at(self, start):
        i = np.flatnonzero(self.run_start == start)
        assert i.size == 1, f"no run starts at slot {start}"
        return int(self.run_len[i[0]]), bool(self.run_equal[i[0]])


def plan_model(keys, counts, k):
    """The chunks of one genome, from its distinct keys and counts (the oracle's
    output): buckets by key >> B, grouped greedily as sp2_plan_kernel groups them."""
    D, B = dims(k)
    cap = cap_of(k)
    allk = np.repeat(np.asarray(keys, U), np.asarray(counts).astype(np.int64))   # ascending
    cnt = np.bincount((allk >> U(B)).astype(np.int64), minlength=1 << D)
    first = np.concatenate([[0], np.cumsum(cnt)])
    chunks = []

    def emit(lo, hi, big):
        chunks.append(ChunkInfo(lo, hi - lo, allk[first[lo]: first[hi]], big, B))

    cur_lo = cur_hi = cur_n = 0
    for b in np.flatnonzero(cnt).tolist():
        c = int(cnt[b])
        if c > cap:
            if cur_n:
                emit(cur_lo, cur_hi, False)
            cur_n = 0
            emit(b, b + 1, True)
        elif cur_n + c > cap:
            emit(cur_lo, cur_hi, False)
            cur_lo, cur_hi, cur_n = b, b + 1, c
        else:
            if not cur_n:
                cur_lo = b
            cur_hi, cur_n = b + 1, cur_n + c
    if cur_n:
        emit(cur_lo, cur_hi, False)
    assert sum(c.nkeys for c in chunks) == allk.size
    return chunks


# ---------------------------------------------------------------- case registry
class G:
    """One genome of a case: intended codes, and either the builder's wrap width
    or raw bytes (dense inputs whose windows overlap)."""

    def __init__(self, codes, width=None, raw=None):
        self.codes, self.width, self.raw = np.asarray(codes, U), width, raw


CASES = {}     # id -> (group, k, thunk -> (genomes, prop(models)))


def case(group, cid, k, thunk):
    assert cid not in CASES, cid
    CASES[cid] = (group, k, thunk)


def ids_of(group):
    return [c for c, v in CASES.items() if v[0] == group]


def one_chunk(models, g=0):
    assert len(models[g]) == 1, [(c.blo, c.nb, c.nkeys, c.big) for c in models[g]]
    return models[g][0]


# ---- chunk sort by R class ------------------------------------------------------
def _r0(k, n, kind):
    def thunk():
        if kind == "polyA":
            gs = [G(np.zeros(n, U), raw=b">a\n" + b"A" * (n + k - 1) + b"\n")]
        else:   # CAC..: one self-canonical value
            gs = [G(np.full(n, sum(1 << (4 * i) for i in range((k + 1) // 2)), U), width=61)]

        def prop(m):
            c = one_chunk(m)
            assert (c.nb, c.R, c.nkeys, c.big) == (1, 0, n, False)
        return gs, prop
    return thunk


for _k in (3, 5):
    for _n in (5000, CAP4):
        for _kind in ("polyA", "single"):
            case("rclass", f"R0-k{_k}-n{_n}-{_kind}", _k, _r0(_k, _n, _kind))


def _r5():
    rng = np.random.default_rng(50)
    # k = 5: B = 0, a bucket is one key value; buckets 64..93, first base A, last A / C / G
    vals = np.array([64 + j for j in range(30) if j & 3 != 3], U)
    codes = np.repeat(vals, rng.integers(1, 200, vals.size))

    def prop(m):
        c = one_chunk(m)
        assert (c.blo, c.nb, c.R, c.big) == (64, 30, 5, False)
    return [G(ordered(codes, "shuf", 1))], prop


case("rclass", "R5-k5-30buckets", 5, _r5)


def _k10(nb):
    def thunk():
        rng = np.random.default_rng(100 + nb)
        codes = np.concatenate([bucket_keys(rng, 10, 37 + i, 3000 - 1000 * i, dup=0.3) for i in range(nb)])

        def prop(m):
            c = one_chunk(m)
            assert (c.blo, c.nb, c.R, c.big) == (37, nb, 10 + nb - 1, False) and c.ndistinct > 500
        return [G(ordered(codes, "shuf", 2), width=61)], prop
    return thunk


case("rclass", "R10-k10-nb1", 10, _k10(1))
case("rclass", "R11-k10-nb2", 10, _k10(2))


def _pairs(rng, k, bucket, lo, n):
    """n keys of one bucket in groups of 1..3 that share everything above bit lo
    (above the last base for lo < 2: its values A and C then differ in bit 0 only)."""
    _, B = dims(k)
    fa = bucket < 256
    lo = max(lo, 2)
    h = np.repeat(distinct_idx(rng, 1 << (B - lo), n), rng.integers(1, 4, n))[:n]
    t = lows(rng.integers(0, (3 if fa else 2) << (lo - 2), n), fa)
    return (U(bucket) << U(B)) | (h << U(lo)) | t


def _edge(k, blo, nb, want_r, long_run, order):
    """The LSD / MSD edge: R = 20 stays LSD; R = 21 / 22 sorts the top 20 bits
    and leaves runs of keys equal above bit 1 / 2, with or without a mixed run of
    40 (the second round on u32 keys: three passes)."""
    def thunk():
        _, B = dims(k)
        rng = np.random.default_rng(1000 * k + nb)
        lo = max(want_r - MSD_BITS, 0)
        per = 4000 // nb
        parts = [_pairs(rng, k, blo + i, lo, per) for i in range(nb)]
        if long_run:
            # 40 keys equal above bit lo, over every value below it the builder allows
            b = blo + nb // 2
            top = (U(b) << U(B)) | (U(0x2A5) << U(max(lo, 2)))
            tails = lows(np.arange(3 if lo >= 2 else 2), True)
            parts.append(top | tails[rng.integers(0, tails.size, 40)])
            parts[-1][:tails.size] = top | tails           # every tail present
        codes = np.concatenate(parts)

        def prop(m):
            c = one_chunk(m)
            assert (c.blo, c.nb, c.R, c.big) == (blo, nb, want_r, False)
            assert c.msd == (want_r > MSD_BITS)
            if c.msd:
                assert len(c.short) > 100
                assert [x for x in c.mixed_long if x >= 40] == ([max(c.mixed_long)] if long_run else [])
                assert c.second_round == long_run
        return [G(ordered(codes, order, 3))], prop
    return thunk


case("rclass", "R20-k15-nb1", 15, _edge(15, 5, 1, 20, False, "shuf"))
for _o in ORDERS:
    for _lr in (False, True):
        _t = "mixed40" if _lr else "short"
        case("rclass", f"R21-k15-nb2-{_t}-{_o}", 15, _edge(15, 5, 2, 21, _lr, _o))
        case("rclass", f"R21-k13-nb20-{_t}-{_o}", 13, _edge(13, 40, 20, 21, _lr, _o))
        case("rclass", f"R22-k16-nb1-{_t}-{_o}", 16, _edge(16, 9, 1, 22, _lr, _o))


def _wide(k, blo, nb, long_run):
    """Chunks of 300 and 512 buckets (R = B + 9: 25 at k = 13, 61 at k = 31), a few
    keys per bucket; with a mixed run of 40 the second round takes 3 / 7 passes."""
    def thunk():
        _, B = dims(k)
        rng = np.random.default_rng(7 * k + nb)
        lo = B + ceil_log2(nb) - MSD_BITS
        parts = [_pairs(rng, k, b, lo, 3) for b in range(blo, blo + nb)]
        if long_run:
            b = blo + nb - 2
            fa = b < 256
            top = (U(b) << U(B)) | (U(0x155) << U(lo))
            parts.append(top | lows(distinct_idx(rng, (3 if fa else 2) << (lo - 2), 40), fa))
        codes = np.concatenate(parts)

        def prop(m):
            c = one_chunk(m)
            assert (c.blo, c.nb, c.R, c.big) == (blo, nb, B + 9, False)
            assert c.nkeys == 3 * nb + 40 * long_run and len(c.short) > nb // 4
            assert len(c.mixed_long) == long_run and c.second_round == long_run
        return [G(ordered(codes, "shuf", 4), width=61)], prop
    return thunk


for _k in (13, 31):
    for _lr in (False, True):
        _t = "-mixed40" if _lr else ""
        case("rclass", f"nb300-from100-k{_k}{_t}", _k, _wide(_k, 100, 300, _lr))
        case("rclass", f"nb512-k{_k}{_t}", _k, _wide(_k, 0, 512, _lr))     # (the builder reaches buckets 0..511)


# ---- fix-up runs: one bucket, R = B, runs of keys equal above bit B - 20 --------
RUN_BUCKET = 7          # first base A: last base A, C or G


def run_keys(k, h, tail_idx):
    _, B = dims(k)
    return (U(RUN_BUCKET) << U(B)) | (U(h) << U(B - MSD_BITS)) | lows(tail_idx, True)


def tail_room(k):
    return 3 << (dims(k)[1] - MSD_BITS - 2)     # k = 21: 3,072 tails; k = 31: 3 * 2^30


LENGTHS = [2, 3, KRUN - 1, KRUN, KRUN + 1, KRUN + 2, 64, 100, 1000, 5000]


def _runs(k, kind, order):
    def thunk():
        _, B = dims(k)
        rng = np.random.default_rng(31 * k + len(kind))
        room = tail_room(k)
        parts = []
        if kind == "distinct":       # (k = 21: a run has 3,072 tails, so the run of 5,000 repeats some)
            parts = [run_keys(k, 1000 * i + 5, distinct_idx(rng, room, L)) for i, L in enumerate(LENGTHS)]
        elif kind == "equal":
            parts = [run_keys(k, 1000 * i + 5, np.full(L, 17 * i, U)) for i, L in enumerate(LENGTHS)]
        elif kind in ("exfirst", "exlast"):
            for i, L in enumerate([KRUN + 1, KRUN + 2, 100, 1000]):
                t = np.full(L, 40 + i, U)
                t[0] = 40 + i + (-7 if kind == "exfirst" else 7)     # below / above the rest
                parts.append(run_keys(k, 1000 * i + 5, t))
        elif kind == "shortonly":
            parts = [run_keys(k, 97 * i + 1, distinct_idx(rng, room, 2 + i % (KRUN - 1))) for i in range(400)]
        codes = np.concatenate(parts)

        def prop(m):
            c = one_chunk(m)
            assert (c.nb, c.R, c.big, c.msd) == (1, B, False, True)
            lng = [L for L in LENGTHS if L > KRUN]
            if kind == "distinct":
                assert c.short == [L for L in LENGTHS if L <= KRUN] and c.mixed_long == lng and not c.equal_long
            elif kind == "equal":
                assert c.equal_long == lng and not c.mixed_long and not c.second_round
                assert c.runs(2, KRUN, equal=True) == [L for L in LENGTHS if L <= KRUN]
            elif kind in ("exfirst", "exlast"):
                assert c.mixed_long == [KRUN + 1, KRUN + 2, 100, 1000] and c.ndistinct == 8
            else:
                assert len(c.short) == 400 and max(c.short) == KRUN and not c.runs(KRUN + 1)
        return [G(ordered(codes, order, 5), width=61 if order == "shuf" else None)], prop
    return thunk


for _k in (21, 31):
    for _kind in ("distinct", "equal", "exfirst", "exlast", "shortonly"):
        for _o in ORDERS:
            case("runs", f"{_kind}-k{_k}-{_o}", _k, _runs(_k, _kind, _o))


DUP_TAILS = [[5, 5, 3, 3, 3, 1], [1, 1], [2, 1, 1], [0] * (KRUN - 1) + [1], [4] * (KRUN // 2) + [2] * (KRUN // 2),
             [7, 7, 7], [9, 8, 9, 8, 9]]


def _dups(k, order):
    def thunk():
        parts = [run_keys(k, 50 * i + 3, np.array(t, U)) for i, t in enumerate(DUP_TAILS)]
        codes = np.concatenate(parts)
        if order == "given":      # every run in the order written above, runs descending
            codes = np.concatenate(parts[::-1])
        else:
            codes = ordered(codes, order, 6)

        def prop(m):
            c = one_chunk(m)
            assert c.msd and c.short == sorted(len(t) for t in DUP_TAILS) and not c.runs(KRUN + 1)
            assert c.ndistinct == sum(len(set(t)) for t in DUP_TAILS) < c.nkeys
        return [G(codes)], prop
    return thunk


for _k in (21, 31):
    for _o in ORDERS + ("given",):
        case("runs", f"dups-in-short-k{_k}-{_o}", _k, _dups(_k, _o))


# ---- run position: f filler singletons below a run put it at slot f -------------
def _fill(rng, k, hs):
    return run_keys(k, 0, distinct_idx(rng, tail_room(k), len(hs))) + (np.asarray(hs, U) << U(dims(k)[1] - MSD_BITS))


def _pos(k, f, L):
    def thunk():
        rng = np.random.default_rng(k * 10000 + f * 100 + L)
        codes = np.concatenate([_fill(rng, k, np.arange(f)), run_keys(k, f + 3, distinct_idx(rng, tail_room(k), L)),
                                _fill(rng, k, f + 10 + np.arange(5))])

        def prop(m):
            c = one_chunk(m)
            assert c.msd and c.run_at(f) == (L, False) and c.runs(2) == [L]
            assert c.second_round == (L > KRUN)
        return [G(ordered(codes, "shuf", 7))], prop
    return thunk


# (k = 16: u32 keys, 384 mask words; a run there has the 3 tails of the last base)
for _k in (16, 21, 31):
    for _f in (0, 30, 31, 32, 63):
        for _L in (2, 3, KRUN, KRUN + 1):
            case("pos", f"slot{_f}-len{_L}-k{_k}", _k, _pos(_k, _f, _L))


def _tail_run(k, n, L):
    """A run that is the chunk's last keys."""
    def thunk():
        rng = np.random.default_rng(k + n + L)
        codes = np.concatenate([_fill(rng, k, np.arange(n - L)),
                                run_keys(k, (1 << MSD_BITS) - 1, distinct_idx(rng, tail_room(k), L))])

        def prop(m):
            c = one_chunk(m)
            assert (c.nkeys, c.big, c.msd) == (n, False, True)
            assert c.run_at(n - L) == (L, False) and c.runs(2) == [L]
        return [G(ordered(codes, "shuf", 8), width=61)], prop
    return thunk


for _k in (16, 21, 31):
    for _n in (cap_of(_k), cap_of(_k) - 7):       # nkeys == cap; nkeys % 32 != 0
        for _L in (3, KRUN + 1):
            case("pos", f"last-keys-n{_n}-len{_L}-k{_k}", _k, _tail_run(_k, _n, _L))


def _back_to_back(k):
    def thunk():
        rng = np.random.default_rng(k + 9)
        lens = [3, KRUN + 1, 2, KRUN]
        parts = [_fill(rng, k, np.arange(30))]
        parts += [run_keys(k, 30 + i, distinct_idx(rng, tail_room(k), L)) for i, L in enumerate(lens)]
        parts.append(_fill(rng, k, 40 + np.arange(5)))

        def prop(m):
            c = one_chunk(m)
            at = 30
            for L in lens:
                assert c.run_at(at) == (L, False)
                at += L
            assert c.runs(2) == sorted(lens)
        return [G(ordered(np.concatenate(parts), "shuf", 9))], prop
    return thunk


def _three_words(k, f, L, equal):
    def thunk():
        rng = np.random.default_rng(k + f + L)
        t = np.full(L, 11, U) if equal else distinct_idx(rng, tail_room(k), L)
        codes = np.concatenate([_fill(rng, k, np.arange(f)), run_keys(k, f + 3, t), _fill(rng, k, f + 10 + np.arange(40))])

        def prop(m):
            c = one_chunk(m)
            assert c.run_at(f) == (L, equal) and ((f + L - 1) >> 5) - (f >> 5) >= 2
            assert c.second_round == (not equal)
        return [G(ordered(codes, "shuf", 10))], prop
    return thunk


for _k in (21, 31):
    case("pos", f"back-to-back-k{_k}", _k, _back_to_back(_k))
    for _f, _L in ((31, KRUN + 2), (30, 70)):
        for _eq in (False, True):
            case("pos", f"three-words-slot{_f}-len{_L}-{'equal' if _eq else 'mixed'}-k{_k}", _k,
                 _three_words(_k, _f, _L, _eq))


# ---- plan edges ---------------------------------------------------------------------
def _one_bucket(k, delta):
    def thunk():
        cap = cap_of(k)
        n = cap + delta
        codes = bucket_keys(np.random.default_rng(k + delta + 5), k, 300, n)

        def prop(m):
            c = one_chunk(m)
            assert (c.blo, c.nb, c.nkeys, c.big) == (300, 1, n, n > cap) and c.ndistinct == n
        return [G(ordered(codes, "shuf", 11), width=61)], prop
    return thunk


def _halves(k, extra):
    def thunk():
        cap = cap_of(k)
        rng = np.random.default_rng(k + extra)
        codes = np.concatenate([bucket_keys(rng, k, 20, cap // 2), bucket_keys(rng, k, 21, cap // 2 + extra)])

        def prop(m):
            got = [(c.blo, c.nb, c.nkeys, c.big) for c in m[0]]
            want = [(20, 2, cap, False)] if not extra else [(20, 1, cap // 2, False), (21, 1, cap // 2 + 1, False)]
            assert got == want
        return [G(ordered(codes, "shuf", 12))], prop
    return thunk


def _sbsbs(k, rng):
    """small, big, small (two buckets), big, small: the big buckets flush the open chunk."""
    cap = cap_of(k)
    spec = [(10, 300), (11, cap + 1), (12, 200), (13, 150), (200, cap + 37), (400, 250)]
    return ordered(np.concatenate([bucket_keys(rng, k, b, n, dup=0.1) for b, n in spec]), "shuf", 13)


def _three_big(k, rng):
    """big, big (adjacent buckets), small, big (the last bucket the builder reaches)."""
    cap = cap_of(k)
    spec = [(0, cap + 1), (1, 2 * tile_of(k) + 1 if k <= 16 else cap + 2), (300, 100), (511, cap + 5)]
    return ordered(np.concatenate([bucket_keys(rng, k, b, n, dup=0.1) for b, n in spec]), "shuf", 14)


def _no_big(k, rng):
    return ordered(np.concatenate([bucket_keys(rng, k, b, 40) for b in range(3, 500, 7)]), "shuf", 15)


def _bigs(chunks):
    return [c.big for c in chunks]


def _plan_single(k, which):
    def thunk():
        rng = np.random.default_rng(k)
        codes = _sbsbs(k, rng) if which == "sbsbs" else _three_big(k, rng)

        def prop(m):
            if which == "sbsbs":
                assert _bigs(m[0]) == [False, True, False, True, False]
                assert [(c.blo, c.nb) for c in m[0]] == [(10, 1), (11, 1), (12, 2), (200, 1), (400, 1)]
            else:
                assert _bigs(m[0]) == [True, True, False, True] and m[0][1].nkeys > 2 * tile_of(k)
        return [G(codes)], prop
    return thunk


def _plan_batch(k):
    def thunk():
        rng = np.random.default_rng(k + 77)
        gs = [G(_sbsbs(k, rng)), G(np.zeros(0, U)), G(_no_big(k, rng), width=61), G(_three_big(k, rng))]

        def prop(m):
            assert [sum(_bigs(x)) for x in m] == [2, 0, 0, 3] and m[1] == [] and len(m[2]) >= 1
        return gs, prop
    return thunk


for _k in (13, 17, 31):
    for _d in (-1, 0, 1):
        case("plan", f"bucket-cap{_d:+d}-k{_k}", _k, _one_bucket(_k, _d))
for _k in (13, 31):
    case("plan", f"halves-share-k{_k}", _k, _halves(_k, 0))
    case("plan", f"halves-split-k{_k}", _k, _halves(_k, 1))
    case("plan", f"small-big-small-big-small-k{_k}", _k, _plan_single(_k, "sbsbs"))
    case("plan", f"three-big-alone-k{_k}", _k, _plan_single(_k, "threebig"))
    case("plan", f"batch-of-four-k{_k}", _k, _plan_batch(_k))


# ---- overflow sort with many distinct keys ------------------------------------------
def _ovf(k, size):
    def thunk():
        _, B = dims(k)
        # two LSD tiles + 1 key for u32 keys; three + 1 for u64 keys, where two tiles are the cap
        n = cap_of(k) + 1 if size == "cap+1" else (2 if k <= 16 else 3) * tile_of(k) + 1
        codes = bucket_keys(np.random.default_rng(k * 3 + n), k, 129, n, dup=0.15)
        room = 3 << (B - 2)

        def prop(m):
            c = one_chunk(m)
            assert (c.big, c.nkeys, c.blo) == (True, n, 129)
            assert c.ndistinct >= min(room, 1000) and c.ndistinct < n
        return [G(ordered(codes, "shuf", 16), width=61 if k % 2 else None)], prop
    return thunk


for _k in (9, 10, 13, 16, 17, 20, 23, 27, 31):      # 1, 2, 2, 3, 3, 4, 5, 6, 7 passes of the overflow sort
    for _s in ("cap+1", "tiles+1"):
        case("ovf", f"{_s}-k{_k}", _k, _ovf(_k, _s))


def _b0_polya(k):
    def thunk():
        n = 20000 - k + 1

        def prop(m):
            c = one_chunk(m)
            assert (c.big, c.nkeys, c.nb, c.R) == (True, n, 1, 0)
        return [G(np.zeros(n, U), raw=b"A" * 20000)], prop
    return thunk


def _b0_ac(reps):
    def thunk():
        codes = np.concatenate([np.full(reps, 1, U), np.full(reps - 1, 4, U)])     # AC; CA (< its complement TG)

        def prop(m):
            # 10,000 repeats stay under the cap: two ordinary one-value chunks (10,000 + 9,999 > cap);
            # 15,000 make two big buckets with B == 0
            assert [(c.blo, c.nkeys, c.big, c.R) for c in m[0]] == [(1, reps, reps > CAP4, 0),
                                                                    (4, reps - 1, reps - 1 > CAP4, 0)]
        return [G(codes, raw=b">r\n" + b"AC" * reps + b"\n")], prop
    return thunk


def _b0_single(k):
    def thunk():
        n = CAP4 + 1

        def prop(m):
            c = one_chunk(m)
            assert (c.big, c.nkeys, c.R) == (True, n, 0)
        return [G(np.full(n, sum(1 << (4 * i) for i in range((k + 1) // 2)), U), width=61)], prop
    return thunk


for _k in (2, 3, 5):
    case("ovf", f"B0-polyA-k{_k}", _k, _b0_polya(_k))
case("ovf", "B0-AC-x10000-k2", 2, _b0_ac(10000))
case("ovf", "B0-AC-x15000-k2", 2, _b0_ac(15000))
for _k in (3, 5):
    case("ovf", f"B0-single-value-k{_k}", _k, _b0_single(_k))


# ---- dense and skewed: overlapping windows ----------------------------------------------
def _dense(k):
    def thunk():
        import gen
        rng = np.random.default_rng(850 + k)
        skew = rng.choice(4, size=150_000, p=[0.85, 0.05, 0.05, 0.05])
        unif = rng.integers(0, 4, 100_000)
        gs = [G(window_codes(skew, k), raw=b">skewed\n" + gen.wrap(_ACGT[skew], 61)),
              G(window_codes(unif, k), raw=b">uniform\n" + gen.wrap(_ACGT[unif], 80))]

        def prop(m):
            assert any(c.big and c.ndistinct > 1000 for c in m[0]) and sum(not c.big for c in m[0]) >= 2
            assert not any(c.big for c in m[1]) and len(m[1]) >= 2
        return gs, prop
    return thunk


for _k in (16, 21, 31):
    case("dense", f"skewed-and-uniform-k{_k}", _k, _dense(_k))


# ---------------------------------------------------------------- shared per-case state
class Built:
    pass


_built = {}


def built(oracle, cid):
    """The case's bytes, the oracle's answer (checked against np.unique of the
    intended codes) and the model of every genome: made once, shared, unchanged."""
    if cid not in _built:
        _, k, thunk = CASES[cid]
        gs, prop = thunk()
        b = Built()
        b.k, b.prop = k, prop
        b.blobs = [g.raw if g.raw is not None else genome(g.codes, k, g.width) for g in gs]
        b.want, b.models = [], []
        for g, blob in zip(gs, b.blobs):
            ek, ec = oracle.sparse_count(blob, k)
            uk, uc = np.unique(g.codes, return_counts=True)
            assert np.array_equal(ek, uk) and np.array_equal(ec, uc.astype(np.uint32)), (cid, "oracle != np.unique")
            b.want.append((ek, ec))
            b.models.append(plan_model(ek, ec, k))
        assert sum(len(x) for x in b.blobs) < 3_200_000, cid
        _built[cid] = b
    return _built[cid]


@pytest.mark.parametrize("cid", list(CASES))
def test_structured_inputs_reach_their_paths(oracle, cid):
    """No GPU: the builder's bytes give the oracle exactly the intended keys, and
    the model finds the structure the case exists for."""
    b = built(oracle, cid)
    b.prop(b.models)


def test_model_recipes():
    """The model on hand-made key sets: the recipes' landing points."""
    k = 31
    keys = np.concatenate([run_keys(k, 10 * i, np.arange(L))
                           for i, L in enumerate([2, 3, 31, 32, 33, 34, 100, 1000])])
    uk, uc = np.unique(keys, return_counts=True)
    c, = plan_model(uk, uc, k)
    assert (c.R, c.short, c.mixed_long) == (52, [2, 3, 31, 32], [33, 34, 100, 1000])
    assert c.run_at(2) == (3, False) and c.run_at(2 + 3 + 31 + 32) == (33, False)
    # k = 15: one bucket is R = 20 (no MSD), two are R = 21
    for nb, r in ((1, 20), (2, 21)):
        uk = np.sort(np.concatenate([(U(5 + i) << U(20)) | lows(np.arange(10)) for i in range(nb)]))
        c, = plan_model(uk, np.ones(uk.size, np.int64), 15)
        assert (c.R, c.msd) == (r, r > MSD_BITS)
    # the greedy plan: cap stays, cap + 1 is big; a bucket that does not fit opens a chunk
    for n, big in ((CAP4, False), (CAP4 + 1, True)):
        c, = plan_model(np.array([U(3) << U(16)]), np.array([n]), 13)
        assert (c.big, c.nkeys) == (big, n)
    ch = plan_model(np.array([1 << 16, 2 << 16, 5 << 16], U), np.array([CAP4 - 1, 2, 7]), 13)
    assert [(c.blo, c.nb, c.nkeys) for c in ch] == [(1, 1, CAP4 - 1), (2, 4, 9)]
    with pytest.raises(AssertionError):
        genome(np.array([3], U), 5)        # AAAAT: first base A, last base T is outside the builder's rule


# ---------------------------------------------------------------- the device side
@pytest.fixture(scope="module")
def torch_dev(native):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu tests need an MI355X")
    return torch.device("cuda:0")


_sparse = {}


def run_case(oracle, dev, cid, alone=False):
    import torch
    from kf2vecfsw_amd import counter as C
    b = built(oracle, cid)
    b.prop(b.models)
    if b.k not in _sparse:
        _sparse[b.k] = C.SparseCounter(b.k, dev)
    sc = _sparse[b.k]
    batches = [[i] for i in range(len(b.blobs))] if alone else [list(range(len(b.blobs)))]
    for sel in batches:
        hb = C.pack_genomes([b.blobs[i] for i in sel])
        keys, cnts, nu = sc.count(C.to_device(hb, dev), int(hb.off[-1]))
        torch.cuda.synchronize()
        nuh = sc.nuniq_to_host(nu)      # raises if the device's own order check tripped
        got = sc.to_host(keys, cnts, nu, hb.off)
        for j, i in enumerate(sel):
            ek, ec = b.want[i]
            gk, gc = got[j]
            assert int(nuh[j]) == ek.size, (cid, i, int(nuh[j]), ek.size)
            if not (np.array_equal(gk, ek) and np.array_equal(gc, ec)):
                bad = np.nonzero((gk != ek) | (gc != ec))[0][:5]
                pytest.fail(f"{cid} genome {i} k={b.k}: rows differ, first {bad.tolist()}: "
                            f"got {gk[bad].tolist()}/{gc[bad].tolist()} want {ek[bad].tolist()}/{ec[bad].tolist()}")


@pytest.mark.gpu
@pytest.mark.parametrize("cid", ids_of("rclass"))
def test_chunk_sort_by_r_class(torch_dev, oracle, cid):
    """R = 0 (no pass) with many keys, one and two LSD passes, the R = 20 / 21 / 22
    edge between plain LSD and MSD + fix-up, chunks of 300 and 512 buckets."""
    run_case(oracle, torch_dev, cid)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", ids_of("runs"))
def test_fixup_runs(torch_dev, oracle, cid):
    """Runs of keys with equal top 20 bits, 2 to 5,000 long: distinct, all equal,
    equal but one, duplicates inside short runs; ascending, descending, shuffled."""
    run_case(oracle, torch_dev, cid)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", ids_of("pos"))
def test_fixup_run_positions(torch_dev, oracle, cid):
    """A run at slot 0, 30, 31, 32, 63, at the chunk's last keys, two runs back to
    back, a run over three mask words."""
    run_case(oracle, torch_dev, cid)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", ids_of("plan"))
def test_plan_edges(torch_dev, oracle, cid):
    """cap - 1 / cap / cap + 1 keys in a bucket, two buckets that fill a chunk
    exactly or by one too many, big buckets between small ones, in one genome
    and in several of a batch."""
    run_case(oracle, torch_dev, cid)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [13, 31])
def test_plan_batch_one_genome_at_a_time(torch_dev, oracle, k):
    """The batch of four again, each genome as a call of its own (the ticket order
    tables exist only for more than one genome)."""
    run_case(oracle, torch_dev, f"batch-of-four-k{k}", alone=True)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", ids_of("ovf"))
def test_overflow_sort_varied_keys(torch_dev, oracle, cid):
    """A big bucket of cap + 1 and of two LSD tiles + 1 varied keys at every pass
    count and parity of both key widths; B == 0 big buckets (gather only)."""
    run_case(oracle, torch_dev, cid)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", ids_of("dense"))
def test_dense_skewed_genome(torch_dev, oracle, cid):
    """Overlapping windows of a 150 kbp genome with P(A) = 0.85 (a big bucket of
    thousands of distinct keys next to ordinary chunks), batched with a uniform one."""
    run_case(oracle, torch_dev, cid)
