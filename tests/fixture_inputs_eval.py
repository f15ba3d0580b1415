"""Seeded INPUTS of the evaluation fixtures (tests/golden/diversity.npz), shared by the script that records scipy's results
(tools/make_golden_diversity.py) and the tests that replay them.  Inputs are regenerated from the seeds on both sides; only
recorded outputs are committed."""
import numpy as np


def body_vectors(seed, N, modes, spread):
    """Multi-modal stand-in for generated 72-D body vectors."""
    rs = np.random.RandomState(seed)
    c = rs.standard_normal((modes, 72)) * 0.6
    s = rs.uniform(0.5, 1.5, (modes, 1)) * spread
    lab = rs.randint(0, modes, N)
    return (c[lab] + rs.standard_normal((N, 72)) * s[lab]).astype(np.float32)


DIV = {'A': dict(data=(1, 2000, 12, 0.15), seed=0), 'B': dict(data=(2, 5000, 30, 0.25), seed=1), 'C': dict(data=(3, 20000, 40, 0.2), seed=2)}
K, RESTARTS, THRESH = 20, 20, 1e-5


def initial_indices(seed, N, k=K, restarts=RESTARTS):
    """The rows scipy.cluster.vq.kmeans(x, k, seed=seed) draws: `restarts` calls of RandomState(seed).choice(N, k, replace=False)."""
    rs = np.random.RandomState(seed)
    return np.stack([rs.choice(N, size=k, replace=False) for _ in range(restarts)])


def easy_case():
    """Three tight blobs; the guess rows hold a duplicate (rows 0, 0, 150, 250)."""
    rs = np.random.RandomState(0)
    return np.concatenate([rs.standard_normal((100, 72)) * 0.1 + c for c in (0, 2, -2)]).astype(np.float32)
