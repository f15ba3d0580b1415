#!/usr/bin/env python
"""python utils_eval_diversity.py GEN_PATH     (utils/utils_eval_diversity.py:56-104: k-means (k = 20) on the generated body vectors;
prints entropy: and mean distance:)"""
import argparse

import _eval_common as C

from psi_release_amd.evaluation import diversity_reference


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('gen_path', nargs='?')
    ap.add_argument('--scenes', nargs='*', default=None)
    ap.add_argument('--max_files', type=int, default=5000, help='files per scene (utils_eval_diversity.py:64)')
    ap.add_argument('--seed', type=int, default=None, help="seed of the initial codebooks (the reference passes none: numpy's global generator)")
    ap.add_argument('--synthetic', default=None)
    a = ap.parse_args(argv)
    if a.synthetic:
        scenes = a.scenes if a.scenes else C.SYNTHETIC_SCENES
        C.synthetic_tree(a.synthetic, scenes, batch=32)
        _, a.gen_path, _, _ = C.synthetic_tree(a.synthetic, scenes, batch=32, write=False)
    elif a.scenes:
        scenes = a.scenes
    elif a.gen_path and 'proxe' in a.gen_path:
        scenes = C.PROXE_SCENES
    elif a.gen_path and 'habitat' in a.gen_path:
        scenes = C.HABITAT_ROOMS
    else:
        ap.error("GEN_PATH must contain 'proxe' or 'habitat' (utils_eval_diversity.py:58-66), or pass --scenes / --synthetic DIR")
    ar = C.body_vectors(a.gen_path, scenes, a.max_files)
    res = diversity_reference(ar, k=20, n_restarts=20, seed=a.seed)
    print('entropy:' + str(res['entropy']))
    print('mean distance:' + str(res['mean_dist']))


if __name__ == '__main__':
    main()
