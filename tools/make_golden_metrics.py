"""TEST INFRASTRUCTURE -- golden vectors for se3_diffusion_amd.metrics from the UNMODIFIED reference:
analysis/metrics.py ca_ca_distance (:120-125), ca_ca_clashes (:127-132), calc_aligned_rmsd (:71-73) and
data/utils.py rigid_transform_3D (:519-568), called on float32-rounded coordinates widened to float64.

Run where the reference is present (oracle/ref_loader.py), in a process of its own:
    python tools/make_golden_metrics.py
Writes tests/golden/metrics.npz: coordinates, masks and the reference's results -- data only.

Backbones ([n,5,3], atom order N, CA, C, CB, O), padded into one [6,130,5,3] call whose padding rows hold NaN and large finite
values:
  0  a 3.8 A random walk, n = 37
  1  a walk with jittered step lengths (sigma 0.15 A), n = 53, two interior residues masked out
  2  walk 0 scaled by 0.35: dozens of clashes
  3  a jittered walk, n = 130 (more than one pass of a 128-wide loop)
  4  a single residue
  5  all residues masked out
C_i -> N_{i+1} lengths are drawn around 1.329 A with sigma 0.12 A, so that c_n_bond_valid_percent lies strictly inside (0, 1).
Superposition pairs: rotated + translated + noise (n = 37); a mirror image + noise (n = 37; the reference must report a
reflection); a rotated copy (n = 53); a masked pair (n = 53); and a set of M = 5 for the all-pairs call.

Counts are compared exactly by the tests, so every distance must lie at least MARGIN from the threshold it is compared with
(3.90209737096, 1.5, 1.329 +- 0.168); a seed that misses the margin is skipped.
"""
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_loader as rl  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "metrics.npz")
CA_CA, C_N, C_N_TOL = 3.80209737096, 1.329, 12 * 0.014
MARGIN = 1e-3
NPAD = 130


def unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def walk(rng, n, jitter):
    steps = unit(rng, n) * (3.8 + jitter * rng.normal(size=(n, 1)))
    steps[0] = rng.normal(size=3) * 5.0
    return np.cumsum(steps, axis=0)


def backbone(rng, ca):
    """N, CA, C, CB, O around a CA trace; N_{i+1} sits at a drawn peptide-bond length from C_i"""
    n = len(ca)
    bb = np.zeros((n, 5, 3))
    bb[:, 1] = ca
    bb[:, 2] = ca + 1.52 * unit(rng, n)
    bb[0, 0] = ca[0] + 1.46 * unit(rng, 1)[0]
    if n > 1:
        bb[1:, 0] = bb[:-1, 2] + unit(rng, n - 1) * (C_N + 0.12 * rng.normal(size=(n - 1, 1)))
    bb[:, 3] = ca + 1.53 * unit(rng, n)
    bb[:, 4] = bb[:, 2] + 1.23 * unit(rng, n)
    return bb.astype(np.float32)


def rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def margin_ok(ca, c, nxt):
    """every compared distance keeps MARGIN from its threshold (float64 on the float32-rounded coordinates)"""
    ca, c, nxt = ca.astype(np.float64), c.astype(np.float64), nxt.astype(np.float64)
    if len(ca) < 2:
        return True
    d = np.linalg.norm(ca[1:] - ca[:-1], axis=-1)
    D = np.linalg.norm(ca[:, None] - ca[None], axis=-1)[np.triu_indices(len(ca), 1)]
    e = np.abs(np.linalg.norm(c - nxt, axis=-1) - C_N)
    return (np.abs(d - (CA_CA + 0.1)).min() >= MARGIN and np.abs(D - 1.5).min() >= MARGIN and D.min() >= MARGIN
            and np.abs(e - C_N_TOL).min() >= MARGIN)


def draw(seed):
    rng = np.random.default_rng(seed)
    w0 = walk(rng, 37, 0.0)
    bbs = [backbone(rng, w0), backbone(rng, walk(rng, 53, 0.15)), None, backbone(rng, walk(rng, 130, 0.15)),
           backbone(rng, walk(rng, 1, 0.0)), backbone(rng, walk(rng, 20, 0.15))]
    b2 = bbs[0].astype(np.float64).copy()
    b2[:, 1] *= 0.35                                            # the CA trace only: the peptide bonds keep their lengths
    bbs[2] = b2.astype(np.float32)
    masks = [np.ones(len(b), np.float32) for b in bbs]
    masks[1][[17, 40]] = 0
    masks[5][:] = 0
    bbs[1][17] = np.nan                                         # a masked-out interior row may hold anything
    atoms = np.empty((6, NPAD, 5, 3), np.float32)
    atoms[:, 0::2] = np.nan
    atoms[:, 1::2] = 3.0e30
    res_mask = np.zeros((6, NPAD), np.float32)
    for k, (b, m) in enumerate(zip(bbs, masks)):
        atoms[k, :len(b)] = b
        res_mask[k, :len(b)] = m
    # superposition pairs, padded to n = 53 with masked NaN rows
    P, NP = 4, 53
    pa = np.full((P, NP, 3), np.nan, np.float32)
    pb = np.full((P, NP, 3), np.nan, np.float32)
    pm = np.zeros((P, NP), np.float32)
    a37, a53 = walk(rng, 37, 0.15), walk(rng, 53, 0.15)
    pa[0, :37], pb[0, :37] = a37, a37 @ rotation(rng).T + rng.normal(size=3) * 10 + 0.5 * rng.normal(size=(37, 3))
    pa[1, :37], pb[1, :37] = a37, (a37 * [-1, 1, 1]) @ rotation(rng).T + 0.3 * rng.normal(size=(37, 3))
    pa[2], pb[2] = a53, a53 @ rotation(rng).T + rng.normal(size=3) * 10
    pa[3], pb[3] = a53, a53 @ rotation(rng).T + 1.0 * rng.normal(size=(53, 3))
    pm[0, :37] = pm[1, :37] = pm[2] = 1
    pm[3] = (rng.random(53) < 0.75).astype(np.float32)
    # a set of M = 5 noisy, rotated copies of one trace
    base = walk(rng, 37, 0.15)
    mset = np.stack([base @ rotation(rng).T + s * rng.normal(size=(37, 3)) for s in (0.0, 0.3, 0.6, 1.0, 2.0)]).astype(np.float32)
    return atoms, res_mask, pa, pb, pm, mset


def main():
    rl.install()
    from analysis import metrics as rm
    from data import utils as rdu
    warnings.simplefilter("ignore", RuntimeWarning)             # np.mean of an empty selection: the NaN the tests expect

    seed = 0
    while True:
        atoms, res_mask, pa, pb, pm, mset = draw(seed)
        ok = True
        for k in range(6):
            m = res_mask[k] != 0
            bb = atoms[k][m]
            ok = ok and margin_ok(bb[:, 1], bb[:-1, 2], bb[1:, 0])
        if ok:
            break
        seed += 1

    ref = np.full((6, 4), np.nan)                               # ca_ca_bond_dev, ca_ca_valid_percent, num clashes, clash percent
    for k in range(6):
        ca = atoms[k][res_mask[k] != 0][:, 1].astype(np.float64)
        dev, valid = rm.ca_ca_distance(ca)
        num, pct = rm.ca_ca_clashes(ca)
        ref[k] = dev, valid, num, pct
    assert ref[2, 2] >= 24, ref[2]                              # "dozens of clashes"
    n_mid = 0
    for k in range(6):
        bb = atoms[k][res_mask[k] != 0].astype(np.float64)
        if len(bb) > 1:
            e = np.abs(np.linalg.norm(bb[:-1, 2] - bb[1:, 0], axis=-1) - C_N) <= C_N_TOL
            n_mid += 0 < e.mean() < 1
    assert n_mid >= 2, n_mid

    P = len(pa)
    pair_mean, pair_R, pair_t, pair_refl = np.zeros(P), np.zeros((P, 3, 3)), np.zeros((P, 3)), np.zeros(P)
    for p in range(P):
        m = pm[p] != 0
        a, b = pa[p][m].astype(np.float64), pb[p][m].astype(np.float64)
        pair_mean[p] = rm.calc_aligned_rmsd(a, b)
        _, R, t, refl = rdu.rigid_transform_3D(a, b)
        pair_R[p], pair_t[p], pair_refl[p] = R, t[:, 0], float(refl)
    assert pair_refl[1] == 1.0 and pair_refl[0] == 0.0, pair_refl
    M = len(mset)
    set_mean = np.zeros((M, M))
    for i in range(M):
        for j in range(i + 1, M):
            set_mean[i, j] = set_mean[j, i] = rm.calc_aligned_rmsd(mset[i].astype(np.float64), mset[j].astype(np.float64))

    np.savez_compressed(GOLD, seed=seed, atoms=atoms, res_mask=res_mask, bb_ref=ref, pair_a=pa, pair_b=pb, pair_mask=pm,
                        pair_mean_dist=pair_mean, pair_R=pair_R, pair_t=pair_t, pair_reflection=pair_refl, set_pos=mset,
                        set_mean_dist=set_mean)
    print(f"seed {seed}: wrote {GOLD} ({os.path.getsize(GOLD)} bytes)")
    print("backbone reference rows (dev, valid, clashes, clash percent):")
    print(ref)
    print("pair mean_dist", pair_mean, "reflection", pair_refl)


if __name__ == "__main__":
    main()
