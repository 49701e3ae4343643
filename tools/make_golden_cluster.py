"""Writes tests/golden/cluster.npz: what scipy.cluster.hierarchy gives on tie-free similarity matrices, for tests/test_cluster.py.

scipy is an independent implementation of the three linkages (a minimum spanning tree for single, nearest-neighbour chains for
average and complete) and is needed only here: the tests read the file.  Per size M the file holds the strict upper triangle of
the similarity matrix in row-major order (s_<M>), and per method scipy's linkage of the distances 1.0 - s (Z_<method>_<M>) and its
flat clusters fcluster(Z, 0.5, criterion="distance") (T_<method>_<M>).

The matrices: M points in space around max(1, M // 6) centres, s = 1 / (1 + (d / 1.5)^2).  Every case must be free of ties and clear
of the cut, or the comparison with an implementation that orders ties differently would mean nothing: consecutive heights at least
GAP apart and no height within GAP of the cut, for every method; a seed that fails is passed over.

    python tools/make_golden_cluster.py
"""
import os

import numpy as np
from scipy.cluster.hierarchy import fcluster, linkage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (2, 3, 17, 64, 130, 257)
METHODS = ("single", "average", "complete")
CUT = 0.5
GAP = 1e-6


def similarity(M, seed):
    rng = np.random.default_rng(seed)
    centres = rng.normal(size=(max(1, M // 6), 3)) * 4.0
    x = centres[rng.integers(len(centres), size=M)] + rng.normal(size=(M, 3))
    d = np.sqrt(((x[:, None] - x[None]) ** 2).sum(-1))
    return 1.0 / (1.0 + (d / 1.5) ** 2)


def margins(Z):
    h = Z[:, 2]
    gap = np.diff(h).min() if len(h) > 1 else np.inf
    return float(gap), float(np.abs(h - CUT).min())


def main():
    out = {"sizes": np.array(SIZES), "methods": np.array(METHODS), "cut": np.array(CUT)}
    for M in SIZES:
        for seed in range(1000 * M, 1000 * M + 100):
            s = similarity(M, seed)
            cond = 1.0 - s[np.triu_indices(M, 1)]           # the distances as the kernel takes them: 1.0 - s in float64
            Zs = {m: linkage(cond, method=m) for m in METHODS}
            worst = [margins(Z) for Z in Zs.values()]
            if min(g for g, _ in worst) >= GAP and min(c for _, c in worst) >= GAP:
                break
        else:
            raise SystemExit(f"M = {M}: no seed without ties")
        out[f"s_{M}"] = s[np.triu_indices(M, 1)]
        for m, Z in Zs.items():
            gap, cut = margins(Z)
            assert gap >= GAP and cut >= GAP, (M, m, gap, cut)
            assert (np.diff(Z[:, 2]) > 0).all() and (Z[:, 0] < Z[:, 1]).all()
            T = fcluster(Z, CUT, criterion="distance")
            out[f"Z_{m}_{M}"] = Z
            out[f"T_{m}_{M}"] = T.astype(np.int32)
            print(f"M {M:4d} seed {seed} {m:9s} smallest gap {gap:.2e} distance to the cut {cut:.2e} clusters {T.max()}")
    path = os.path.join(ROOT, "tests", "golden", "cluster.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
