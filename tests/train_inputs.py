"""Inputs of the kf_dist_loss tests, shared by test_host_train.py and
test_gpu_train.py: embeddings, a true distance matrix and labels with the cases
planted that the loss must get right."""
import numpy as np


def make(B, E, seed=0):
    """(y float32 [B, E], P float64 [N, N], labels int64 [B]) with N = B + 5:
    distances of about 1 against true distances in (0.05, 3); P is asymmetric
    with a zero diagonal; the labels are unsorted; row 0's embedding comes
    twice (B >= 3: a zero distance off the diagonal); P is 0 at one pair off
    the diagonal (B >= 2), in one direction only; and one label comes twice
    (B >= 4: a true distance of 0 between different embeddings)."""
    rng = np.random.default_rng(1000 * B + E + 7919 * seed)
    N = B + 5
    y = (rng.standard_normal((B, E)) / np.sqrt(2.0 * E)).astype(np.float32)
    P = rng.uniform(0.05, 3.0, size=(N, N))
    np.fill_diagonal(P, 0.0)
    labels = rng.permutation(N)[:B].astype(np.int64)
    if B >= 2 and labels[0] < labels[1]:
        labels[:2] = labels[1::-1].copy()
    if B >= 4:
        labels[2] = labels[0]
    if B >= 3:
        y[B - 1] = y[0]
    if B >= 2:
        P[labels[0], labels[1]] = 0.0
    return y, P, labels
