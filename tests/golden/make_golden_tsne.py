"""Writes g33_tsne.npz: scikit-learn's own results for the K30 tests.  No reference code is involved; the data are what
sklearn 1.7.2 returns.

  kl_seeds, kl_sklearn   TSNE(method="exact", perplexity=30, init=Y0).fit(X).kl_divergence_ for the end-to-end case of
                         tests/test_gpu_tsne.py: X = blobs(300, 10, 3, seed), Y0 = 1e-4 RandomState(100 + seed).standard_normal
  n_iter_sklearn         its n_iter_
  p96_x, p96_perplexity  a 96-row table and
  p96_joint              the dense _joint_probabilities of its float32 squared distances (sum of squared differences)

usage: make_golden_tsne.py [--seeds 0,1,...]   (PXSOM_GOLDEN_OUT overrides the output directory)
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import tsne_reference as ts  # noqa: E402


def main():
    from scipy.spatial.distance import squareform
    from sklearn.manifold import TSNE, _t_sne

    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", default="0,1,2,3,4,5")
    seeds = [int(s) for s in ap.parse_args().seeds.split(",")]
    kl, iters = [], []
    for seed in seeds:
        x, _, y0 = ts.end_to_end_case(seed)
        est = TSNE(method="exact", perplexity=30.0, init=y0.copy()).fit(x)
        kl.append(float(est.kl_divergence_))
        iters.append(int(est.n_iter_))
    x96, _ = ts.blobs(96, 5, 2, 7)
    d32 = ts.pair_sqdist_f32(x96)
    joint = squareform(_t_sne._joint_probabilities(d32, 10.0, 0))
    out = os.path.join(os.environ.get("PXSOM_GOLDEN_OUT", HERE), "g33_tsne.npz")
    np.savez_compressed(out, kl_seeds=np.asarray(seeds, np.int64), kl_sklearn=np.asarray(kl), n_iter_sklearn=np.asarray(iters, np.int64),
                        p96_x=x96, p96_perplexity=np.float64(10.0), p96_joint=joint)


if __name__ == "__main__":
    main()
