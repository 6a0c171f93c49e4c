"""Count tables at the edges of the RANSAC selection rule, for the CPU tests that hold the one C++ rule (rs::select_best<ROOTS,
SAMPLE>, csrc/ransac_math.h) to each estimator's own Python restatement: tests/test_ransac_cpu.py <3, 7>, test_ransac5_cpu.py
<10, 5>, test_homography_ref_cpu.py <1, 4>.  No restatement of the rule in here: only inputs."""
import numpy as np

NO_ROOT = -1
N_EDGE = 100  # correspondences of the hand-made tables


def climbing(roots):
    """The `k == bk` case: at k = 5 every root improves on the one before (100 - roots, .., 99 of 100).  The first of them
    already lowers niters to 5 or less (3 roots, 7 points: log(0.01) / log(1 - 0.97^7) = 2.8; 10 roots, 5 points: log(0.01) /
    log(1 - 0.9^5) = 5.2), not above the k being processed, and the rule still has to look at that iteration's other roots --
    and at nothing after it: the 100 at k = 6 is never read."""
    tab = np.full((8, roots), NO_ROOT, np.int32)
    tab[1, 0] = 20
    tab[5] = 100 - roots + np.arange(roots)
    tab[6, 0] = 100
    return tab, N_EDGE, 0.99


def tables(roots, no_sample=None, seed=11, n_random=300):
    """Yields (table [T, roots] int32, N, confidence).  no_sample: the table code of an iteration without a sample, or None for
    an estimator whose table never holds one (five distinct indices always exist)."""
    yield climbing(roots)
    flat = np.full((6, roots), 30, np.int32)  # ties everywhere: the first entry wins and stays
    for conf in (0.0, 0.5, 1.0):
        yield flat, N_EDGE, conf
    if no_sample is not None:
        first = np.full((4, roots), 50, np.int32)
        first[0] = no_sample  # no sample at k = 0: no model, no iteration consumed
        yield first, N_EDGE, 0.99
        later = np.full((6, roots), NO_ROOT, np.int32)
        later[1, 0], later[4, 0] = 10, 60
        later[3] = no_sample  # past the first model: the loop ends there, the 60 at k = 4 is never read
        yield later, N_EDGE, 1.0
    rng = np.random.default_rng(seed)
    for trial in range(n_random):
        N = int(rng.integers(15, 400))
        T = int(rng.integers(1, 200))
        hi = int(rng.choice([8, 12, N + 1]))  # few distinct counts: ties, and the max(best, SAMPLE - 1) floor
        tab = rng.integers(0, hi, (T, roots)).astype(np.int32)
        tab[rng.random((T, roots)) < 0.4] = NO_ROOT
        if roots > 1 and trial % 3 == 0:  # several improving roots in one iteration
            k = int(rng.integers(0, T))
            tab[k] = np.sort(rng.integers(N // 2, N + 1, roots))
        if no_sample is not None and trial % 4 == 0:
            tab[int(rng.integers(0, T))] = no_sample
        yield np.ascontiguousarray(tab), N, float(rng.choice([0.0, 0.5, 0.99, 1.0]))
