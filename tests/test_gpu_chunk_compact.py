"""GPU parity of get_chunks' pre-pass kernels with their host statements, byte
for byte and offset for offset: kf_chunk_compact against
chunks.compact_records_host on the corpus of tests/chunk_corpus.py (which
tests/test_host_chunk_compact.py shows to separate nine subtly wrong rules),
called through the library directly so that short records, the tails after the
last window, d_out_se and the bytes past the output are all looked at; and
kf_chunk_gather against numpy slices."""
import numpy as np
import pytest

import chunk_corpus as CC

pytestmark = pytest.mark.gpu

MARK = 0xA5
PAD_BYTES = 64      # marker bytes after d_out
PAD_ENTRIES = 8     # marker entries after d_out_se


@pytest.fixture(scope="module")
def torch_dev(native):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu tests need an MI355X")
    return torch.device("cuda:0")


def compact_on_device(dev, data: np.ndarray, se: np.ndarray, n_rec=None):
    """kf_chunk_compact through the library: d_bytes of exactly len bytes (16 if
    len is 0), scratch of exactly ceil(len / 4096) + 1 words, d_out of len + 64
    bytes and d_out_se of 2n + 8 entries, both filled with a marker.  Returns the
    two whole buffers on the host (uint8, uint64)."""
    import torch
    from kf2vecfsw_amd import _native as N
    n = int(data.size)
    n_rec = se.size // 2 if n_rec is None else n_rec
    host = np.zeros(n or 16, dtype=np.uint8)
    host[:n] = data
    d_bytes = torch.from_numpy(host).to(dev)
    d_se = torch.from_numpy(np.array(se, dtype=np.uint64).view(np.int64)).to(dev) if se.size else \
        torch.zeros(2, dtype=torch.int64, device=dev)
    d_out = torch.full((n + PAD_BYTES,), MARK, dtype=torch.uint8, device=dev)
    d_out_se = torch.full((8 * (se.size + PAD_ENTRIES),), MARK, dtype=torch.uint8, device=dev)
    words = (n + 4095) // 4096 + 1
    scratch = torch.empty(words, dtype=torch.int32, device=dev)
    N.check(N.lib().kf_chunk_compact(d_bytes.data_ptr(), n, d_se.data_ptr(), n_rec, d_out.data_ptr(),
                                     d_out_se.data_ptr(), scratch.data_ptr(), words,
                                     torch.cuda.current_stream(dev).cuda_stream), "kf_chunk_compact")
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), d_out_se.cpu().numpy().view(np.uint64)


def check_case(dev, name, data, se, exp):
    out, out_se = exp
    got, got_se = compact_on_device(dev, data, se)
    total = int(out_se[-1])
    assert np.array_equal(got_se[: se.size], out_se), name                              # the offsets
    assert got[:total].tobytes() == out, name                                           # the bytes
    assert (got[total:] == MARK).all(), name                                            # nothing past the output
    assert (got_se[se.size:] == np.uint64(int.from_bytes(bytes([MARK]) * 8, "little"))).all(), name
    again, again_se = compact_on_device(dev, data, se)
    assert np.array_equal(again, got) and np.array_equal(again_se, got_se), name       # the same on a second call


@pytest.mark.parametrize("half", [0, 1])
def test_compact_every_5_byte_pattern(torch_dev, half):
    """Group a: all 16,807 strings over "ANn|-\\n\\r", one range each, at every
    phase of a thread's 16 bytes; touching ranges (half 0) and ranges with a byte
    of no range between them (half 1)."""
    cases, exp = CC.group("a"), CC.expected("a")
    for x in range(16 * half, 16 * half + 16):
        check_case(torch_dev, *cases[x], exp[x])


def test_compact_motifs_across_tile_edges(torch_dev):
    """Group b: N runs, CRLF, blank lines, gap letters, a range-final '\\r',
    touching and empty ranges and bytes of no range, each byte in turn first after
    a thread, wave and workgroup edge (16, 1024, 4096, 8192, 12288)."""
    for case, exp in zip(CC.group("b"), CC.expected("b")):
        check_case(torch_dev, *case, exp)


@pytest.mark.parametrize("third", [0, 1, 2])
def test_compact_block_count_edges(torch_dev, third):
    """Group c: 1, 2, 1023, 1024, 1025 and 2049 blocks (the scan's rounds of 1,024
    and their carry), whole and with a last block of one byte, blocks of no, all
    and some kept bytes; one range, ranges of 4 KiB +- 1, random cuts."""
    cases, exp = CC.group("c"), CC.expected("c")
    for x in range(4 * third, 4 * third + 4):
        check_case(torch_dev, *cases[x], exp[x])


def test_compact_degenerate_inputs(torch_dev):
    """Group d: len == 0, only empty ranges, a range of which nothing is kept, a
    range of N-class bytes only, a look-back over 20,000 newlines; and n_rec == 0,
    which leaves both outputs untouched."""
    for case, exp in zip(CC.group("d"), CC.expected("d")):
        check_case(torch_dev, *case, exp)
    _name, data, se = CC.group("e")[0]
    got, got_se = compact_on_device(torch_dev, data, se, n_rec=0)
    assert (got == MARK).all() and (got_se.view(np.uint8) == MARK).all()


def test_compact_random_bytes_random_cuts(torch_dev):
    """Group e: all 256 byte values with the letters of the rule common, ranges
    from random cuts (mid-line starts and ends), with and without bytes left out."""
    for case, exp in zip(CC.group("e"), CC.expected("e")):
        check_case(torch_dev, *case, exp)


def test_compact_accepts_scratch_of_one_word_more(torch_dev):
    """scratch_words == ceil(len / 4096) is refused (KF_ERANGE, CPU test); one word
    more is what compact_on_device passes for every case, here at a whole number
    of blocks where blk[nb] is the word past the block counts."""
    name, data, se = CC.group("c")[1]
    assert data.size == 4096
    check_case(torch_dev, name, data, se, CC.expected("c")[1])


# ------------------------------------------------------------------ kf_chunk_gather
def gather_on_device(dev, src: np.ndarray, starts, win_len: int, n_win=None):
    import torch
    from kf2vecfsw_amd import _native as N
    n_win = len(starts) if n_win is None else n_win
    d_src = torch.from_numpy(src).to(dev)
    d_win = torch.from_numpy(np.asarray(list(starts) or [0], dtype=np.int64)).to(dev)
    d_dst = torch.full((len(starts) * win_len + PAD_BYTES,), MARK, dtype=torch.uint8, device=dev)
    N.check(N.lib().kf_chunk_gather(d_src.data_ptr(), d_win.data_ptr(), n_win, win_len, d_dst.data_ptr(),
                                    torch.cuda.current_stream(dev).cuda_stream), "kf_chunk_gather")
    torch.cuda.synchronize()
    return d_dst.cpu().numpy()


@pytest.mark.parametrize("win_len", [1, 15, 16, 255, 256, 257, 10000])
def test_gather_equals_numpy_slices(torch_dev, win_len):
    """Window w of the destination is src[s_w: s_w + win_len] for starts that are
    unaligned, overlap, repeat, come in descending order and end at src's last
    byte; the bytes after the last window are untouched, and n_win == 0 writes
    nothing."""
    rng = np.random.default_rng(6100 + win_len)
    n = 3 * win_len + 4099
    src = rng.integers(0, 256, size=n, dtype=np.uint8)
    last = n - win_len                                             # ends at the last byte of src
    starts = [1, 3, 3 + win_len // 2, 3, last, 4097, 17, 16, 0, last, 5]
    starts += sorted(rng.integers(0, last + 1, size=9).tolist(), reverse=True)
    assert max(starts) + win_len == n
    got = gather_on_device(torch_dev, src, starts, win_len)
    exp = np.concatenate([src[s: s + win_len] for s in starts])
    assert np.array_equal(got[: exp.size], exp)
    assert (got[exp.size:] == MARK).all() and got.size == exp.size + PAD_BYTES
    assert (gather_on_device(torch_dev, src, starts, win_len, n_win=0) == MARK).all()
