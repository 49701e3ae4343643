"""TEST INFRASTRUCTURE -- golden vectors for se3_diffusion_amd.metrics.violations from the UNMODIFIED reference:
openfold/data/data_transforms.py make_atom14_masks, make_atom14_positions and openfold/utils/loss.py find_structural_violations
(violation_tolerance_factor=12, clash_overlap_tolerance=1.5, as openfold/np/relax/amber_minimize.py:377-382 sets them),
compute_violation_metrics -- the call sequence of amber_minimize.find_violations (:354-390) on an all-alanine chain.

Run where the reference is present (oracle/ref_loader.py), in a process of its own:
    python tools/make_golden_violations.py
Writes tests/golden/violations.npz: coordinates, masks, residue numbers and the reference's results -- data only.

Every case is a backbone [n,5,3] (atom order N, CA, C, CB, O), float32, with a mask and residue numbers.  The reference is run on
the COMPACTED chain (the present residues, residue_index carrying their numbers): it would leave an absent residue at the origin,
existing.  It is run twice on the same float32-rounded coordinates: in float32, as the reference runs it (amber_minimize.py:366),
and with every floating tensor of the batch widened to float64 before find_structural_violations -- the functions follow the dtype
of what they are given.  (The masks are widened too: atom14_atom_exists is float32 whatever the coordinates are, and a float32
count + 1e-6 would round the eps of the means away.  torch's default dtype is float64 during that run for the same reason: the
reference forms the C-N length 1.329 and its tolerance as a boolean tensor times a Python float, a tensor of the default dtype, and
float32 would round the constants themselves.)

Cases:
  walk37     standard bond geometry with random torsions -- a 3.8 A walk --, C-N lengths drawn around 1.329 A with sigma 0.1 A and
             the CA-C-N and C-N-CA angles with sigma 8 and 15 degrees, so that the bond violation fraction lies strictly inside
             (0, 1) and all three means are non-zero
  removed53  the same kind, n = 53, two interior residues absent (NaN coordinates); the residue numbers keep the gap
  scaled64   the same kind, n = 64, all coordinates scaled by 0.5: dozens of clashes
  walk130    n = 130: past a 128-wide loop and two 64-residue tiles; one connection stretched to a C-N of 3.2 A, an extreme CA-CA
             distance
  single     one residue
  empty      no residue: inputs only -- the reference cannot run on it (between_residue_clash_loss takes amax over an empty
             dimension and raises)
  bonded3    n = 3, ideal geometry with C-N at 1.33 A: the bonded C-N pairs are no clash
  gapped3    the same coordinates numbered 0, 2, 4: now both C-N pairs are clashes
  repeat37   walk37's coordinates with the number 19 given twice (residues 19 and 20): the reference counts the atom pairs of two
             residues only where the first number is strictly below the second, so these two residues share no pair
  6MRR, 3HTN deposited chains of tests/golden/dssp_chains.npz with their resnum, CB placed from N, CA, C by the standard
             ideal-geometry construction: realistic inputs, losses near zero
Every hard decision must lie at least MARGIN = 1e-4 from its threshold in float64 (the three connection tolerances, the CA-CA
excess, every clash bound); a seed that misses the margin is skipped.  Prints the largest float32-against-float64 difference of
the reference per quantity: the table of tests/test_violations.py's docstring.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_loader as rl  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "violations.npz")
MARGIN = 1e-4
SCALARS = ("bonds_c_n_loss_mean", "angles_ca_c_n_loss_mean", "angles_c_n_ca_loss_mean", "clashes_mean_loss",
           "violations_extreme_ca_ca_distance", "violations_between_residue_bond", "violations_between_residue_clash",
           "violations_within_residue", "violations_per_residue")
ARRAYS = ("connections_per_residue_loss_sum", "connections_per_residue_violation_mask", "clashes_per_atom_loss_sum",
          "clashes_per_atom_clash_mask", "total_per_residue_violations_mask")
ATOM14_OF = (0, 1, 2, 4, 3)                      # alanine's atom14 order is N, CA, C, O, CB


def place(prev3, length, angle, torsion):
    """the point at `length` from c with angle (b, c, new) and torsion (a, b, c, new), degrees"""
    a, b, c = prev3
    bc = (c - b) / np.linalg.norm(c - b)
    nrm = np.cross(b - a, bc)
    nrm /= np.linalg.norm(nrm)
    m = np.cross(nrm, bc)
    ang, tor = np.radians(angle), np.radians(torsion)
    d = np.array([-np.cos(ang), np.sin(ang) * np.cos(tor), np.sin(ang) * np.sin(tor)])
    return c + length * (d[0] * bc + d[1] * m + d[2] * nrm)


def with_cb(bb4):
    """[n,4,3] N, CA, C, O -> float32 [n,5,3] N, CA, C, CB, O: the ideal CB from the frame of N, CA, C"""
    b4 = np.asarray(bb4, np.float64)
    b, c = b4[:, 1] - b4[:, 0], b4[:, 2] - b4[:, 1]
    cb = -0.58273431 * np.cross(b, c) + 0.56802827 * b - 0.54067466 * c + b4[:, 1]
    return np.stack([b4[:, 0], b4[:, 1], b4[:, 2], cb, b4[:, 3]], axis=1).astype(np.float32)


def build(phi, psi, c_n, ca_c_n=None, c_n_ca=None):
    """a backbone of standard bond geometry from its torsions (degrees), its C-N lengths c_n[i] (C of i to N of i + 1) and the two
    angles at that bond (degrees; None: the ideal 116.2 and 121.7)"""
    n = len(phi)
    ca_c_n = np.full(n, 116.2) if ca_c_n is None else ca_c_n
    c_n_ca = np.full(n, 121.7) if c_n_ca is None else c_n_ca
    N, CA, C, O = [np.zeros((n, 3)) for _ in range(4)]
    N[0], CA[0] = [0.0, 0.0, 0.0], [1.458, 0.0, 0.0]
    C[0] = CA[0] + 1.525 * np.array([-np.cos(np.radians(111.0)), np.sin(np.radians(111.0)), 0.0])
    for i in range(n):
        if i > 0:
            N[i] = place((N[i - 1], CA[i - 1], C[i - 1]), c_n[i - 1], ca_c_n[i - 1], psi[i - 1])
            CA[i] = place((CA[i - 1], C[i - 1], N[i]), 1.458, c_n_ca[i - 1], 180.0)
            C[i] = place((C[i - 1], N[i], CA[i]), 1.525, 111.0, phi[i])
        O[i] = place((N[i], CA[i], C[i]), 1.231, 120.5, psi[i] + 180.0)
    return with_cb(np.stack([N, CA, C, O], axis=1) + 3.0)       # (shifted: no coordinate is exactly zero)


def walk(rng, n, stretch=None):
    """random torsions; C-N lengths around 1.329 A (sigma 0.1 A) and the two angles at the bond around their ideal values (sigma 8
    and 15 degrees), so that each of the three tolerances is missed by some connections and met by others; stretch: one
    connection whose C-N is 3.2 A long, a CA-CA distance above 3.802 + 1.5 A"""
    k = max(n - 1, 0)
    c_n = 1.329 + 0.1 * rng.normal(size=k)
    if stretch is not None:
        c_n[stretch] = 3.2
    return build(rng.uniform(-180.0, 180.0, n), rng.uniform(-180.0, 180.0, n), c_n, 116.2 + 8.0 * rng.normal(size=k),
                 121.7 + 15.0 * rng.normal(size=k))


def margin(x, idx):
    """the smallest distance of a hard decision from its threshold, float64, on the compacted chain x [n,5,3] numbered idx"""
    x = x.astype(np.float64)
    n, m = len(x), np.inf
    if n > 1:
        ca, c, nn, can = x[:-1, 1], x[:-1, 2], x[1:, 0], x[1:, 1]
        root = lambda v: np.sqrt(1e-6 + (v ** 2).sum(-1))
        l_cn, l_cac, l_nca = root(c - nn), root(ca - c), root(nn - can)
        cos1 = (((ca - c) / l_cac[:, None]) * ((nn - c) / l_cn[:, None])).sum(-1)
        cos2 = ((-(nn - c) / l_cn[:, None]) * ((can - nn) / l_nca[:, None])).sum(-1)
        e = lambda v: np.sqrt(1e-6 + v ** 2)
        m = min(m, np.abs(e(l_cn - 1.329) - 12 * 0.014).min(), np.abs(e(cos1 + 0.4473) - 12 * 0.014).min(),
                np.abs(e(cos2 + 0.5203) - 12 * 0.0353).min(), np.abs(root(ca - can) - 3.80209737096 - 1.5).min())
        rad = np.array([1.55, 1.7, 1.7, 1.7, 1.52])
        d = np.sqrt(1e-10 + ((x[:, None, :, None] - x[None, :, None, :]) ** 2).sum(-1))
        bound = rad[None, None, :, None] + rad[None, None, None, :] - 1.5
        counted = (idx[:, None] < idx[None, :])[:, :, None, None] & np.ones((1, 1, 5, 5), bool)
        nb = idx[:, None] + 1 == idx[None, :]
        counted[:, :, 2, 0] &= ~nb
        m = min(m, np.abs(d - bound)[counted].min())
    return float(m)


def reference(x, idx, dtype):
    """the unmodified reference on the compacted chain x float32 [n,5,3] numbered idx"""
    import torch
    from openfold.data import data_transforms as dt
    from openfold.utils import loss
    n = len(x)
    pos = torch.zeros((n, 37, 3), dtype=torch.float32)
    pos[:, :5] = torch.from_numpy(np.ascontiguousarray(x))      # atom37 begins N, CA, C, CB, O
    am = torch.zeros((n, 37), dtype=torch.float32)
    am[:, :5] = 1
    batch = {"aatype": torch.zeros(n, dtype=torch.long), "all_atom_positions": pos, "all_atom_mask": am,
             "residue_index": torch.from_numpy(np.asarray(idx, np.int64)), "seq_mask": torch.ones(n, dtype=torch.float32)}
    batch = dt.make_atom14_positions(dt.make_atom14_masks(batch))
    if dtype == np.float64:
        batch = {k: (v.double() if v.is_floating_point() else v) for k, v in batch.items()}
        torch.set_default_dtype(torch.float64)                   # (bool * 1.329 is a tensor of the default dtype, loss.py:767-780)
    try:
        viol = loss.find_structural_violations(batch, batch["atom14_gt_positions"], violation_tolerance_factor=12,
                                               clash_overlap_tolerance=1.5)
        met = loss.compute_violation_metrics(batch, batch["atom14_gt_positions"], viol)
    finally:
        torch.set_default_dtype(torch.float32)
    out = {k: viol["between_residues"][k] for k in ("bonds_c_n_loss_mean", "angles_ca_c_n_loss_mean", "angles_c_n_ca_loss_mean",
                                                      "connections_per_residue_loss_sum", "connections_per_residue_violation_mask",
                                                      "clashes_mean_loss", "clashes_per_atom_loss_sum", "clashes_per_atom_clash_mask")}
    out["total_per_residue_violations_mask"] = viol["total_per_residue_violations_mask"]
    out.update(met)
    out = {k: v.numpy().astype(np.float64) for k, v in out.items()}
    for k in ("clashes_per_atom_loss_sum", "clashes_per_atom_clash_mask"):
        assert not out[k][:, 5:].any(), k                        # alanine has five atoms
        out[k] = out[k][:, list(ATOM14_OF)]
    return out


def cases(seed):
    rng = np.random.default_rng([20, seed])
    res = {}
    res["walk37"] = (walk(rng, 37), np.ones(37), np.arange(37))
    a = walk(rng, 53)
    m = np.ones(53)
    m[[17, 40]] = 0
    a[[17, 40]] = np.nan                                         # an absent row may hold anything
    res["removed53"] = (a, m, np.arange(53))
    res["scaled64"] = ((walk(rng, 64).astype(np.float64) * 0.5).astype(np.float32), np.ones(64), np.arange(64))
    res["walk130"] = (walk(rng, 130, stretch=100), np.ones(130), np.arange(130))
    res["single"] = (walk(rng, 1), np.ones(1), np.arange(1))
    res["empty"] = (np.zeros((0, 5, 3), np.float32), np.ones(0), np.arange(0))
    three = build([-120.0] * 3, [130.0] * 3, [1.33, 1.33])
    res["bonded3"] = (three, np.ones(3), np.arange(3))
    res["gapped3"] = (three, np.ones(3), np.arange(3) * 2)
    twice = np.arange(37)
    twice[20:] -= 1
    res["repeat37"] = (res["walk37"][0], np.ones(37), twice)
    G = np.load(os.path.join(ROOT, "tests", "golden", "dssp_chains.npz"))
    for name in ("6MRR", "3HTN"):
        xyz = with_cb(G[f"{name}_xyz"])
        res[name] = (xyz, np.ones(len(xyz)), G[f"{name}_resnum"].astype(np.int64))
    return res


def pack(cs, save):
    """the per-case entries joined into a few arrays (an .npz entry costs a few hundred bytes of its own): the cases' padded rows
    one after another (row_start), the reference's per-residue results over their present residues (res_start), the scalars as
    [case, SCALARS] -- NaN where the reference has no result (has_ref 0)"""
    names = list(cs)
    cat = lambda key, dt: np.concatenate([np.asarray(save[f"{c}_{key}"], dt).reshape((-1,) + np.shape(save[f"{c}_{key}"])[1:])
                                          for c in names if f"{c}_{key}" in save])
    has_ref = np.array([f"{c}_f64_{SCALARS[0]}" in save for c in names], np.uint8)
    out = {"names": save["names"], "seed": save["seed"], "margin": save["margin"], "has_ref": has_ref, "scalars": np.array(SCALARS),
           "row_start": np.cumsum([0] + [len(cs[c][0]) for c in names]),
           "res_start": np.cumsum([0] + [int((cs[c][1] != 0).sum()) * int(h) for c, h in zip(names, has_ref)]),
           "atoms": cat("atoms", np.float32), "mask": cat("mask", np.float32), "res_index": cat("res_index", np.int32)}
    for tag, dt in (("f32", np.float32), ("f64", np.float64)):
        out[f"{tag}_scalars"] = np.array([[save[f"{c}_{tag}_{k}"] if h else np.nan for k in SCALARS] for c, h in zip(names, has_ref)], dt)
        for k in ARRAYS:
            out[f"{tag}_{k}"] = cat(f"{tag}_{k}", np.uint8 if k.endswith("_mask") else dt)
    return out


def main():
    rl.install()
    seed = 0
    while True:
        cs = cases(seed)
        marg = {k: margin(a[m != 0], idx[m != 0]) for k, (a, m, idx) in cs.items()}
        fixed = min(marg[k] for k in ("bonded3", "gapped3", "6MRR", "3HTN"))
        assert fixed >= MARGIN, marg                             # (no seed moves these)
        if min(marg.values()) >= MARGIN:
            break
        seed += 1
    save = {"names": np.array(list(cs)), "seed": seed, "margin": np.array([marg[k] for k in cs])}
    gap = {}
    for name, (a, m, idx) in cs.items():
        keep = m != 0
        save[f"{name}_atoms"], save[f"{name}_mask"], save[f"{name}_res_index"] = a, m.astype(np.float32), idx.astype(np.int32)
        if not keep.any():
            continue                                             # (the reference raises on an empty chain)
        r32, r64 = reference(a[keep], idx[keep], np.float32), reference(a[keep], idx[keep], np.float64)
        for k in SCALARS + ARRAYS:
            if k.endswith("_mask"):                              # (0 or 1; the float32 run's values are float32 numbers: nothing is lost)
                save[f"{name}_f32_{k}"], save[f"{name}_f64_{k}"] = r32[k].astype(np.uint8), r64[k].astype(np.uint8)
            else:
                save[f"{name}_f32_{k}"], save[f"{name}_f64_{k}"] = r32[k].astype(np.float32), r64[k]
            if r64[k].size:
                d = np.abs(r32[k] - r64[k])
                if k in SCALARS:
                    assert (r64[k] == 0) == (r32[k] == 0), (name, k)
                    d = d / r64[k] if r64[k] != 0 else d
                gap[k] = max(gap.get(k, 0.0), float(np.max(d)))
        print(f"{name:10s} n {int(keep.sum()):4d} margin {marg[name]:.2e}  " + "  ".join(f"{r64[k]:.6g}" for k in SCALARS))
    r = {k: save[f"walk37_f64_{k}"] for k in SCALARS}
    assert 0 < r["violations_between_residue_bond"] < 1 and min(r[k] for k in SCALARS[:3]) > 0, r
    assert save["walk130_f64_violations_extreme_ca_ca_distance"] > 0
    assert save["scaled64_f64_clashes_per_atom_clash_mask"].sum() >= 24                      # "dozens of clashes"
    assert not save["bonded3_f64_clashes_per_atom_clash_mask"].any()
    assert save["gapped3_f64_clashes_per_atom_clash_mask"].sum() == 4                        # C of 0, N of 1, C of 1, N of 2
    for name in ("6MRR", "3HTN"):
        assert save[f"{name}_f64_violations_within_residue"] == 0, name                    # (what makes slot 8 the reference's there)
    np.savez_compressed(GOLD, **pack(cs, save))
    print(f"seed {seed}: wrote {GOLD} ({os.path.getsize(GOLD)} bytes)")
    print("largest float32-against-float64 difference of the reference (scalars relative, arrays absolute):")
    for k in SCALARS + ARRAYS:
        print(f"  {k:42s} {gap.get(k, 0.0):.3e}")


if __name__ == "__main__":
    main()
