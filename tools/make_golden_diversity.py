#!/usr/bin/env python
"""Record scipy's diversity evaluation (utils/utils_eval_diversity.py:93-104) on the seeded fixtures of tests/fixture_inputs_eval.py
into tests/golden/diversity.npz: per fixture the 20 x 20 initial row indices scipy draws, and from scipy.cluster.vq.kmeans(x, 20,
seed=seed) on the float32 data and again on x.astype(float64): codebook, distortion, and from vq + np.histogram +
scipy.stats.entropy: counts, entropy, mean distance.  Outputs only; runs on a CPU.

    python tools/make_golden_diversity.py [out.npz]
"""
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import fixture_inputs_eval as FE  # noqa: E402


def record(name):
    """dict of the recorded arrays of fixture `name` (keys prefixed with the fixture's name)."""
    import scipy.cluster.vq as vq
    from scipy.stats import entropy
    spec = FE.DIV[name]
    x32 = FE.body_vectors(*spec['data'])
    out = {name + '_init': FE.initial_indices(spec['seed'], x32.shape[0]).astype(np.int64)}
    for tag, x in (('f32', x32), ('f64', x32.astype(np.float64))):
        with warnings.catch_warnings():
            warnings.simplefilter('ignore', DeprecationWarning)
            codes, distortion = vq.kmeans(x, FE.K, iter=FE.RESTARTS, thresh=FE.THRESH, seed=spec['seed'])
        vecs, dist = vq.vq(x, codes)
        counts, _ = np.histogram(vecs, len(codes))
        out['%s_%s_codes' % (name, tag)] = np.asarray(codes)
        out['%s_%s_distortion' % (name, tag)] = np.float64(distortion)
        out['%s_%s_counts' % (name, tag)] = counts.astype(np.int64)
        out['%s_%s_entropy' % (name, tag)] = np.float64(entropy(counts))
        out['%s_%s_mean_dist' % (name, tag)] = np.float64(np.mean(dist))
    # which restart won: the one whose own loop reproduces the recorded distortion (replayed from the recorded rows in float64)
    x64 = x32.astype(np.float64)
    d = [vq._kmeans(x64, x64[rows], thresh=FE.THRESH)[1] for rows in out[name + '_init']]
    out[name + '_winner'] = np.int64(int(np.argmin(d)))      # argmin = the first minimum, like `dist < best_dist`
    assert d[int(np.argmin(d))] == out[name + '_f64_distortion']
    out[name + '_runner_up_gap'] = np.float64(np.sort(d)[1] - np.sort(d)[0])
    return out


def main(path=None):
    path = path or os.path.join(ROOT, 'tests', 'golden', 'diversity.npz')
    out = {}
    for name in sorted(FE.DIV):
        out.update(record(name))
        print(name, 'winner', int(out[name + '_winner']), 'distortion f64 / f32', float(out[name + '_f64_distortion']),
              float(out[name + '_f32_distortion']), 'gap', float(out[name + '_runner_up_gap']), 'entropy',
              float(out[name + '_f64_entropy']), float(out[name + '_f32_entropy']),
              'counts equal', bool(np.array_equal(out[name + '_f64_counts'], out[name + '_f32_counts'])))
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else None)
