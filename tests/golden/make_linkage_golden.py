"""Records tests/golden/linkage_3000x16.npz: scipy's ward linkage of 3000 seeded Gaussian fp32 rows of 16 features --
children (int32) and heights -- the case of tests/test_linkage_gpu.py that is too long for the numpy oracle.  The seed
is the first for which the smallest relative gap between consecutive heights is at least 1e-8, the condition of an
exact comparison of children.  Needs scipy; run from the repository root: python tests/golden/make_linkage_golden.py"""
import os

import numpy as np
from scipy.cluster.hierarchy import linkage

N, D, MIN_GAP = 3000, 16, 1e-8


def centers(seed):
    return np.random.default_rng(seed).standard_normal((N, D)).astype(np.float32)


def main():
    for seed in range(100):
        Z = linkage(centers(seed).astype(np.float64), method="ward", metric="euclidean")
        h = Z[:, 2]
        assert np.all(np.diff(h) >= 0)
        gap = float(np.min((h[1:] - h[:-1]) / h[1:]))
        print(f"seed {seed}: smallest relative gap {gap:.3e}")
        if gap >= MIN_GAP:
            break
    else:
        raise SystemExit("no seed with a large enough gap")
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "linkage_3000x16.npz")
    np.savez_compressed(out, seed=np.int64(seed), n=np.int64(N), d=np.int64(D), children=Z[:, :2].astype(np.int32),
                        heights=h, smallest_relative_gap=np.float64(gap))
    print(f"wrote {out} ({os.path.getsize(out)} bytes)")


if __name__ == "__main__":
    main()
