"""Inputs of the kf_class_loss tests, shared by test_host_train_classifier.py and
test_gpu_train_classifier.py: logits and classes with the cases planted that
the loss must get right."""
import numpy as np

CASES = ("spread 120", "two maxima", "-inf at the true class", "-inf elsewhere")


def make(B, C, seed=0):
    """(logits float32 [B, C], true int64 [B], {case: row}): logits spread over
    about +-8, classes drawn with repeats.  From row 1 on, as far as B and C
    allow (C >= 2), one row each with: a spread of 120, so that e underflows to
    0 (the true class at the bottom); two equal maxima (the true class the
    second of them); -inf at the true class; -inf at another class.  Which case
    comes first turns with C, so that a batch of three rows plants other cases
    at C and at C + 1."""
    rng = np.random.default_rng(100003 * B + C + 7919 * seed)
    x = rng.uniform(-8.0, 8.0, size=(B, C)).astype(np.float32)
    true = rng.integers(0, C, size=B).astype(np.int64)
    where = {}
    if C >= 2:
        for n in range(min(len(CASES), B - 1)):
            what, r = CASES[(n + C) % len(CASES)], 1 + n
            where[what] = r
            a, b = (int(v) for v in rng.permutation(C)[:2])
            if what == "spread 120":
                x[r] = rng.uniform(-2.0, 0.0, size=C).astype(np.float32)
                x[r, a] = np.float32(-120.0)
                x[r, b] = np.float32(0.0)
                true[r] = a
            elif what == "two maxima":
                lo, hi = min(a, b), max(a, b)
                x[r, lo] = x[r, hi] = np.float32(9.5)
                true[r] = hi
            elif what == "-inf at the true class":
                x[r, a] = -np.inf
                true[r] = a
            else:
                x[r, a] = -np.inf
                true[r] = b
    return x, true, where
