"""CPU checks of the evaluation feature: the recorded scipy results (tests/golden/diversity.npz) regenerate, an fp64 restatement of
scipy's k-means loop reproduces them (the arbiter the GPU tests compare with), and the histogram follows the reference's
``scipy.histogram(vecs, len(codes))`` rather than ``bincount``."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import ROOT, golden
import fixture_inputs_eval as FE


# ---- the arbiter: scipy.cluster.vq._kmeans restated in float64 numpy, squared distances in the direct form, code by code -------
def vq_f64(x, book, with_gap=False):
    """(code, dist) = nearest row of `book` per row of `x` (first minimum) in float64; with_gap: also the relative gap between the
    nearest and the second-nearest distance."""
    x = np.asarray(x, np.float64)
    d2 = np.stack([((x - np.asarray(c, np.float64)) ** 2).sum(1) for c in book], 1)
    code = d2.argmin(1)
    d = np.sqrt(d2)
    dist = d[np.arange(len(x)), code]
    if not with_gap:
        return code, dist
    if d.shape[1] < 2:
        return code, dist, np.full(len(x), np.inf)
    two = np.partition(d, 1, axis=1)[:, :2]
    return code, dist, (two[:, 1] - two[:, 0]) / np.maximum(two[:, 0], 1e-300)


def kmeans_f64(x, book, thresh=1e-5):
    """One restart: (book after the last update, avg of the last vq, iterations)."""
    x = np.asarray(x, np.float64)
    book = np.asarray(book, np.float64)
    prev, iters = np.inf, 0
    while True:
        code, dist = vq_f64(x, book)
        avg = dist.mean()
        cnt = np.bincount(code, minlength=len(book))
        book = np.stack([x[code == c].mean(0) for c in range(len(book)) if cnt[c] > 0])     # codes without members are removed
        iters += 1
        diff = abs(prev - avg)
        prev = avg
        if not diff > thresh:
            return book, avg, iters


def arbiter(x, init_rows, thresh=1e-5):
    """scipy.cluster.vq.kmeans over the given initial rows: (winner, its book, its distortion); `dist < best_dist`, strict."""
    x64 = np.asarray(x, np.float64)
    best = (None, None, np.inf)
    for r, rows in enumerate(init_rows):
        book, avg, _ = kmeans_f64(x64, x64[rows], thresh)
        if avg < best[2]:
            best = (r, book, avg)
    return best


def _maker():
    spec = importlib.util.spec_from_file_location('make_golden_diversity', os.path.join(ROOT, 'tools', 'make_golden_diversity.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_committed_initial_rows_are_what_the_seed_draws():
    g = golden('diversity')
    for name, spec in FE.DIV.items():
        N = spec['data'][1]
        init = g[name + '_init']
        assert init.shape == (FE.RESTARTS, FE.K)
        assert np.array_equal(init, FE.initial_indices(spec['seed'], N))
        # drawn as diversity_reference draws them: `restarts` choice() calls in sequence from RandomState(seed)
        rs = np.random.RandomState(spec['seed'])
        assert np.array_equal(init, np.stack([rs.choice(N, size=FE.K, replace=False) for _ in range(FE.RESTARTS)]))
        assert all(len(set(r.tolist())) == FE.K for r in init)


def test_golden_regenerates_with_scipy():
    pytest.importorskip('scipy')
    g = golden('diversity')
    new = _maker().record('A')
    assert sorted(k for k in g.files if k.startswith('A_')) == sorted(new)
    for k, v in new.items():
        if np.asarray(v).dtype.kind in 'iu':
            assert np.array_equal(g[k], v), k                                  # winner, counts, initial rows: exactly
        else:
            assert np.allclose(g[k], v, rtol=1e-6, atol=0), k                  # another scipy / BLAS build may round differently


@pytest.mark.parametrize('name', ['A', 'B'])
def test_fp64_restatement_reproduces_scipy(name):
    g = golden('diversity')
    x = FE.body_vectors(*FE.DIV[name]['data'])
    winner, book, distortion = arbiter(x, g[name + '_init'])
    assert winner == int(g[name + '_winner'])
    ref = float(g[name + '_f64_distortion'])
    assert abs(distortion - ref) <= 1e-9 * ref, (distortion, ref)
    code, dist = vq_f64(x, book)
    counts = np.histogram(code, len(book))[0]
    assert np.array_equal(counts, g[name + '_f64_counts'])
    assert book.shape == g[name + '_f64_codes'].shape and np.abs(book - g[name + '_f64_codes']).max() < 1e-9
    assert abs(dist.mean() - float(g[name + '_f64_mean_dist'])) <= 1e-9 * ref


def test_histogram_follows_the_reference_not_bincount():
    from psi_release_amd import evaluation
    code = np.array([0, 0, 1, 1, 1, 2, 2, 2, 2, 2])             # four codes, the highest (3) has no member
    counts, ent = evaluation.code_histogram(code, 4)
    ref = np.histogram(code, 4)[0]
    assert np.array_equal(counts, ref) and list(ref) == [2, 0, 3, 5]        # bins over [min, max] = [0, 2]: edges 0, .5, 1, 1.5, 2
    assert list(np.bincount(code, minlength=4)) == [2, 3, 5, 0] and not np.array_equal(ref, np.bincount(code, minlength=4))
    p = np.array([2, 3, 5]) / 10.0
    assert abs(ent - float(-(p * np.log(p)).sum())) < 1e-15
    # all codes populated: the two agree
    code = np.arange(20).repeat(3)
    assert np.array_equal(evaluation.code_histogram(code, 20)[0], np.bincount(code, minlength=20))


def test_easy_case_restatement():
    """The three-blob case of the GPU test: a duplicate guess row can never win, so k_eff drops to 3; scipy's distortion."""
    x = FE.easy_case()
    book, avg, iters = kmeans_f64(x, x[[0, 0, 150, 250]].astype(np.float64))
    assert book.shape == (3, 72) and abs(avg - 0.8335614) <= 1e-5 * 0.8335614 and iters >= 2
    far = x[[0, 150, 250, 0]].astype(np.float64)
    far[3] = 50.0
    book2, avg2, _ = kmeans_f64(x, far)
    assert np.array_equal(book, book2) and avg == avg2
