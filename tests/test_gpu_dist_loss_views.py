"""GPU tests of kf_dist_loss_views against train.dist_loss_host, bit for bit, the
loss and the gradient: the chunk trainer's rows (`views` rows that follow each
other share a label) and its weight 1 / (T + eps), at the smallest shapes where
the kernel can go wrong -- one genome, the last size of the one-workgroup path
and the first of the tiled one (counted in rows, not labels), three views, one
view -- each at eps = 1000 and eps = 1e-6, with the cases planted that the loss
must get right; the loss-only call; a label outside the matrix; and views = 1,
eps = 1e-6 against kf_dist_loss' own output."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (labels, views, E), S = kf_dist_loss_small_b() rows
SHAPES = [(1, 2, 1), (1, 2, 33), (8, 2, 8), ("S/2", 2, 33), ("S/2+1", 2, 33), ("S+1", 2, 64), (11, 3, 5), ("S+8", 1, 7)]
EPS = [1000.0, 1e-6]


@pytest.fixture(scope="module")
def dev(native):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu tests need an MI355X")
    return torch.device("cuda:0")


def size(native, v):
    S = native.kf_dist_loss_small_b()
    return v if isinstance(v, int) else {"S/2": S // 2, "S/2+1": S // 2 + 1, "S+1": S + 1, "S+8": S + 8}[v]


def make(G, V, E):
    """(y float32 [G V, E], P float64 [N, N], labels int64 [G]), N = G + 5: true distances in
    (50, 3000), where an eps of 1000 and one of 1e-6 both tell; embeddings whose distances are
    of the size of their square roots; P asymmetric with a diagonal that is not zero (the pairs
    of one genome's views read it); unsorted labels; with two views or more the first two rows
    equal (two identical views: d = 0 off the diagonal, c = 0); from three genomes on one
    label held by two genomes of the batch."""
    rng = np.random.default_rng(100000 * G + 1000 * V + E)
    N = G + 5
    y = (rng.standard_normal((G * V, E)) * (32.0 / np.sqrt(2.0 * E))).astype(np.float32)
    P = rng.uniform(50.0, 3000.0, size=(N, N))
    labels = rng.permutation(N)[:G].astype(np.int64)
    if G * V >= 2:
        y[1] = y[0]
    if G >= 3:
        labels[2] = labels[0]
    return y, P, labels


_HOST = {}


def host(G, V, E, eps):
    from kf2vecfsw_amd import train as TR
    key = (G, V, E, eps)
    if key not in _HOST:
        y, P, labels = make(G, V, E)
        loss, grad = TR.dist_loss_host(y, P, labels, views=V, eps=eps)
        grad.setflags(write=False)
        _HOST[key] = (y, P, labels, loss, grad)
    return _HOST[key]


def run_kernel(dev, y, P, labels, views, eps, grad=True):
    import torch
    from kf2vecfsw_amd import train as TR
    loss, g, status = TR.dist_loss(torch.from_numpy(y).to(dev), torch.from_numpy(P).to(dev),
                                   torch.from_numpy(labels).to(dev), grad=grad, views=views, eps=eps)
    return loss.cpu().numpy(), None if g is None else g.cpu().numpy(), int(status.cpu()[0])


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


@pytest.mark.parametrize("eps", EPS)
@pytest.mark.parametrize("G,V,E", SHAPES, ids=["{}x{}x{}".format(*s) for s in SHAPES])
def test_kernel_equals_the_host_statement_bit_for_bit(dev, native, G, V, E, eps):
    G = size(native, G)
    B = G * V
    y, P, labels, h_loss, h_grad = host(G, V, E, eps)
    loss, grad, status = run_kernel(dev, y, P, labels, V, eps)
    assert status == 0 and loss.dtype == np.float64 and grad.dtype == np.float32 and grad.shape == (B, E)
    print("G={} V={} E={} eps={}: loss {!r} (host {!r}), largest |grad| {:.3g}".format(
        G, V, E, eps, float(loss), float(h_loss), float(np.abs(h_grad).max())))
    assert np.isfinite(h_loss) and np.isfinite(h_grad).all()
    assert bits(loss) == bits(np.float64(h_loss))
    differ = np.flatnonzero(bits(grad).reshape(-1) != bits(h_grad).reshape(-1))
    assert differ.size == 0, "{} of {} gradient entries differ, the first at {}".format(differ.size, B * E, differ[0])
    # d_grad = NULL: the same loss bits
    loss2, grad2, status2 = run_kernel(dev, y, P, labels, V, eps, grad=False)
    assert grad2 is None and status2 == 0 and bits(loss2) == bits(loss)


def test_the_inputs_hold_the_planted_cases(native):
    from kf2vecfsw_amd import train as TR
    S = native.kf_dist_loss_small_b()
    rows = [size(native, g) * v for g, v, _ in SHAPES]
    assert S in rows and S + 2 in rows and max(r for r in rows if r <= S) == S     # both sides of the cut-over, in rows
    assert size(native, "S/2+1") <= S < size(native, "S/2+1") * 2                  # labels below it, rows above
    y, P, labels = make(8, 2, 8)
    assert np.array_equal(y[0], y[1]) and labels[2] == labels[0] and np.unique(labels).size == 7
    assert not np.array_equal(P, P.T) and np.diagonal(P).all()
    # each of them changes the result: eps, the interleaving, the asymmetry of P, its diagonal
    base = TR.dist_loss_host(y, P, labels, views=2, eps=1000.0)[0]
    assert TR.dist_loss_host(y, P, labels, views=2, eps=1e-6)[0] != base
    assert TR.dist_loss_host(y, P, np.tile(labels, 2), views=1, eps=1000.0)[0] != base
    # (the transposed matrix gives the same sums in exact arithmetic: what tells is one side read for both)
    upper = np.triu(P) + np.triu(P, 1).T
    assert TR.dist_loss_host(y, upper, labels, views=2, eps=1000.0)[1].tobytes() != \
        TR.dist_loss_host(y, P, labels, views=2, eps=1000.0)[1].tobytes()
    Q = P.copy()
    np.fill_diagonal(Q, 0.0)
    assert TR.dist_loss_host(y, Q, labels, views=2, eps=1000.0)[0] != base
    # the two equal views: a zero distance, a zero coefficient, whatever P holds there
    assert P[labels[0], labels[0]] > 0


def test_only_the_last_label_outside_the_matrix_sets_the_status(dev, native):
    """The label check walks B / views labels: the last one is read, and nothing behind it."""
    S = native.kf_dist_loss_small_b()
    for G, V, E in ((4, 2, 6), (S // 2 + 2, 2, 6), (S // 3 + 2, 3, 4)):
        y, P, labels = make(G, V, E)
        for bad in (P.shape[0], -1, 1 << 40):
            lab = labels.copy()
            lab[G - 1] = bad
            for want in (True, False):
                loss, grad, status = run_kernel(dev, y, P, lab, V, 1000.0, grad=want)
                assert status == 1 and np.isnan(loss), (G, V, bad, want)
        loss, _, status = run_kernel(dev, y, P, labels, V, 1000.0)
        assert status == 0 and np.isfinite(loss)


def test_raw_call_with_guards_and_one_view_equals_kf_dist_loss(dev, native):
    """The raw entry on both paths, guard values around every output and a labels array of
    exactly B / views entries inside a guarded buffer; and views = 1, eps = 1e-6 gives the
    bits kf_dist_loss gives."""
    import torch
    from kf2vecfsw_amd import _native as N
    from kf2vecfsw_amd import counter as CN
    from kf2vecfsw_amd import train as TR
    S = native.kf_dist_loss_small_b()
    for G, V, E in ((5, 2, 7), (S // 2 + 3, 2, 9)):
        B = G * V
        y, P, labels, h_loss, h_grad = host(G, V, E, 1000.0)
        d_y, d_P = torch.from_numpy(y).to(dev), torch.from_numpy(P).to(dev)
        d_l = torch.from_numpy(labels).to(dev)
        need = TR.dist_loss_scratch_bytes(B)
        scratch = torch.empty(need // 8 + 1, dtype=torch.int64, device=dev)
        for want in (True, False):
            out = torch.full((3,), -7.5, dtype=torch.float64, device=dev)
            st = torch.full((3,), -77, dtype=torch.int32, device=dev)
            g = torch.full((B * E + 128,), -12345.5, dtype=torch.float32, device=dev)
            N.check(native.kf_dist_loss_views(d_y.data_ptr(), B, E, d_P.data_ptr(), P.shape[0], d_l.data_ptr(), V, 1000.0,
                                              out[1:].data_ptr(), g[64:].data_ptr() if want else None, st[1:].data_ptr(),
                                              scratch.data_ptr() if need else None, need, CN._stream_ptr(dev)),
                    "kf_dist_loss_views")
            o, s, gh = out.cpu().numpy(), st.cpu().numpy(), g.cpu().numpy()
            assert o[0] == -7.5 and o[2] == -7.5 and bits(o[1:2])[0] == bits(np.float64(h_loss)), (B, want)
            assert s.tolist() == [-77, 0, -77], (B, want)
            assert np.all(gh[:64] == -12345.5) and np.all(gh[64 + B * E:] == -12345.5), (B, want)
            if want:
                assert np.array_equal(bits(gh[64: 64 + B * E]), bits(h_grad).reshape(-1)), B
            else:
                assert np.all(gh == -12345.5), B
    for G, E in ((7, 9), (S + 8, 7)):
        y, P, labels = make(G, 1, E)
        d_y, d_P, d_l = (torch.from_numpy(a).to(dev) for a in (y, P, labels))
        a = TR.dist_loss(d_y, d_P, d_l)                                   # kf_dist_loss
        B = G
        need = TR.dist_loss_scratch_bytes(B)
        scratch = torch.empty(need // 8 + 1, dtype=torch.int64, device=dev)
        loss = torch.empty((), dtype=torch.float64, device=dev)
        st = torch.empty(1, dtype=torch.int32, device=dev)
        g = torch.empty((B, E), dtype=torch.float32, device=dev)
        N.check(native.kf_dist_loss_views(d_y.data_ptr(), B, E, d_P.data_ptr(), P.shape[0], d_l.data_ptr(), 1, 1e-6,
                                          loss.data_ptr(), g.data_ptr(), st.data_ptr(),
                                          scratch.data_ptr() if need else None, need, CN._stream_ptr(dev)),
                "kf_dist_loss_views")
        assert int(st[0]) == 0 and int(a[2][0]) == 0
        assert bits(loss.cpu().numpy()) == bits(a[0].cpu().numpy())
        assert np.array_equal(bits(g.cpu().numpy()), bits(a[1].cpu().numpy()))


def test_autograd_function_with_views(dev, native):
    import torch
    from kf2vecfsw_amd import train as TR
    S = native.kf_dist_loss_small_b()
    for G, V, E in ((8, 2, 8), (S // 2 + 1, 2, 33)):
        y, P, labels, h_loss, h_grad = host(G, V, E, 1000.0)
        d_y = torch.from_numpy(y).to(dev).requires_grad_(True)
        loss, status = TR.dist_loss_fn(d_y, torch.from_numpy(P).to(dev), torch.from_numpy(labels).to(dev), V, 1000.0)
        assert bits(loss.detach().cpu().numpy()) == bits(np.float64(h_loss)) and int(status[0]) == 0
        loss.backward()
        assert np.array_equal(bits(d_y.grad.cpu().numpy()), bits(h_grad))
