"""TEST INFRASTRUCTURE -- golden vectors for se3_diffusion_amd.data.chains (fd_chain_windows, fd_chain_batch) from the UNMODIFIED
reference: data/utils.py parse_chain_feats, openfold/data/data_transforms.py atom37_to_frames and atom37_to_torsion_angles, and
Rigid.from_tensor_4x4(rigidgroups_gt_frames)[:, 0] -- the call sequence of PdbDataset._process_csv_row / __getitem__
(data/pdb_data_loader.py:133-154,240-241) on one chain.

Run where the reference is present (oracle/ref_loader.py), in a process of its own:
    python tools/make_golden_chain_batch.py
Writes tests/golden/chain_batch.npz: coordinates, masks, residue numbers and the reference's results -- data only.

Every case is a chain: atoms float32 [L,4,3] (N, CA, C, O), atom_mask uint8 [L,4], residue numbers.  Absent atoms hold zeros, as
in the files process_pdb_dataset.py writes.  The reference is run on the WINDOW of the chain -- from the first to the last residue
with N, CA and C, the reference's modeled_idx trim (pdb_data_loader.py:137-143), applied BEFORE parse_chain_feats so that the centre
is the window's, as include/fd_hip.h has it -- with its inputs widened to float64 as the reference widens them (:148-149).

Cases:
  4GYT .. 6EHB   the N, CA, C, O coordinates of the six deposited chains of tests/golden/dssp_chains.npz (68-318 residues)
  walk<n>        synthetic chains of n = 1, 2, 63, 64, 65, 255, 256, 257, 513 residues: ideal bond geometry with random torsions, every
                 coordinate jittered by 0.05 A
  single         five residues of which one is present
  empty          four residues, none present: inputs only
Every chain of more than 16 residues is modified: its first two and its last residue absent (the trim), three whole residues
removed inside, one residue without O only, one without N only.

Per case the file records the inputs, the reference's rotation matrices, translations, rigidgroups_gt_exists[:, 0] and
torsion_angles_sin_cos[:, :3] on the window, and ref_gap: the largest difference between the reference and the float64
restatement of the header (tests/test_chains.py np_chain) on the rows where the reference's frame exists, for rotation entries,
translations and torsions.  The reference rounds rotations and origins to float32 inside Rotation / Rigid; that is what the gaps show.
Asserted: on every present row |w| >= 1e-6 and |C - CA|^2, |u|^2 >= 1e-3 (the comparisons of the tests rest on these margins), and
the reference's frame exists exactly where N, CA and C are present.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import ref_loader as rl  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "chain_batch.npz")
DEPOSITED = ("4GYT", "4YOW", "6MRR", "3HTN", "5L33", "6EHB")
WALKS = (1, 2, 63, 64, 65, 255, 256, 257, 513)


def place(a, b, c, length, angle, torsion):
    """the point at `length` from c with angle (b, c, new) and torsion (a, b, c, new), degrees"""
    bc = (c - b) / np.linalg.norm(c - b)
    nrm = np.cross(b - a, bc)
    nrm /= np.linalg.norm(nrm)
    m = np.cross(nrm, bc)
    ang, tor = np.radians(angle), np.radians(torsion)
    return c + length * (-np.cos(ang) * bc + np.sin(ang) * np.cos(tor) * m + np.sin(ang) * np.sin(tor) * nrm)


def walk(rng, n):
    """N, CA, C, O of n residues, ideal bond geometry with random phi / psi, jittered by 0.05 A and shifted off the origin"""
    phi, psi = rng.uniform(-180.0, 180.0, n), rng.uniform(-180.0, 180.0, n)
    N, CA, C, O = [np.zeros((n, 3)) for _ in range(4)]
    CA[0] = [1.458, 0.0, 0.0]
    C[0] = CA[0] + 1.525 * np.array([-np.cos(np.radians(111.0)), np.sin(np.radians(111.0)), 0.0])
    for i in range(n):
        if i > 0:
            N[i] = place(N[i - 1], CA[i - 1], C[i - 1], 1.329, 116.2, psi[i - 1])
            CA[i] = place(CA[i - 1], C[i - 1], N[i], 1.458, 121.7, 180.0)
            C[i] = place(C[i - 1], N[i], CA[i], 1.525, 111.0, phi[i])
        O[i] = place(N[i], CA[i], C[i], 1.231, 120.5, psi[i] + 180.0)
    x = np.stack([N, CA, C, O], 1)
    return (x + 0.05 * rng.normal(size=x.shape) + rng.normal(size=3) * 10.0).astype(np.float32)


def modify(rng, atoms):
    """the mask of a modified chain; absent atoms are zeroed"""
    L = len(atoms)
    mask = np.ones((L, 4), np.uint8)
    if L > 16:
        mask[[0, 1, L - 1]] = 0
        inner = rng.permutation(np.arange(3, L - 2))[:5]        # (never the window's first or last residue)
        mask[inner[:3]] = 0
        mask[inner[3], 3] = 0
        mask[inner[4], 0] = 0
    atoms = atoms.copy()
    atoms[mask == 0] = 0
    return atoms, mask


def cases():
    rng = np.random.default_rng([30, 0])
    G = np.load(os.path.join(ROOT, "tests", "golden", "dssp_chains.npz"))
    res = {}
    for name in DEPOSITED:
        xyz = G[f"{name}_xyz"].astype(np.float32)
        assert np.isfinite(xyz).all() and xyz.shape[1:] == (4, 3)
        res[name] = modify(rng, xyz) + (G[f"{name}_resnum"].astype(np.int32),)
    for n in WALKS:
        res[f"walk{n}"] = modify(rng, walk(rng, n)) + (np.arange(n, dtype=np.int32) + 17,)
    a = walk(rng, 5)
    m = np.zeros((5, 4), np.uint8)
    m[2] = 1
    m[3, 1] = 1                                                  # (a CA without N and C: not present)
    a[m == 0] = 0
    res["single"] = (a, m, np.arange(5, dtype=np.int32))
    res["empty"] = (np.zeros((4, 4, 3), np.float32), np.zeros((4, 4), np.uint8), np.arange(4, dtype=np.int32))
    return res


def reference(atoms, mask):
    """the unmodified reference on a window: atoms float32 [W,4,3] (N, CA, C, O), mask [W,4]"""
    import torch
    from data import utils as du
    from openfold.data import data_transforms as dt
    from openfold.utils.rigid_utils import Rigid
    W = len(atoms)
    pos, msk = np.zeros((W, 37, 3), np.float64), np.zeros((W, 37), np.float64)
    pos[:, [0, 1, 2, 4]], msk[:, [0, 1, 2, 4]] = atoms, mask
    feats = du.parse_chain_feats({"atom_positions": pos, "atom_mask": msk})
    chain = {"aatype": torch.zeros(W, dtype=torch.long), "all_atom_positions": torch.tensor(feats["atom_positions"]).double(),
             "all_atom_mask": torch.tensor(feats["atom_mask"]).double()}
    chain = dt.atom37_to_frames(chain)
    chain = dt.atom37_to_torsion_angles()(chain)
    rig = Rigid.from_tensor_4x4(chain["rigidgroups_gt_frames"])[:, 0]
    return dict(rot=rig.get_rots().get_rot_mats().numpy(), trans=rig.get_trans().numpy(),
                exists=chain["rigidgroups_gt_exists"][:, 0].numpy(), tors=chain["torsion_angles_sin_cos"][:, :3].numpy(),
                res_mask=feats["bb_mask"])


def main():
    rl.install()
    from test_chains import np_chain, np_window
    cs = cases()
    names = list(cs)
    out = {k: [] for k in ("atoms", "mask", "res_index", "ref_rot", "ref_trans", "ref_exists", "ref_tors", "ref_gap")}
    worst = np.zeros(3)
    for name in names:
        atoms, mask, idx = cs[name]
        out["atoms"].append(atoms), out["mask"].append(mask), out["res_index"].append(idx)
        first, last, count = np_window(mask)
        W = last - first + 1
        gap = np.zeros(3)
        if W:
            ref = reference(atoms[first:last + 1], mask[first:last + 1])
            res = np_chain(atoms, mask, idx)
            ex = ref["exists"] != 0
            assert np.array_equal(ex, res["res_mask"] != 0), name       # the frame exists exactly where N, CA and C are present
            assert res["margin"]["w"] >= 1e-6 and res["margin"]["l0"] >= 1e-3 and res["margin"]["l1"] >= 1e-3, (name, res["margin"])
            gap = np.array([np.abs(ref["rot"].astype(np.float64) - res["rot"])[ex].max(),
                            np.abs(ref["trans"].astype(np.float64) - res["rigids_0"][:, 4:])[ex].max(),
                            np.abs(ref["tors"].astype(np.float64) - res["torsions"][:, :3])[ex].max()])
            out["ref_rot"].append(ref["rot"].astype(np.float32)), out["ref_trans"].append(ref["trans"].astype(np.float32))
            out["ref_exists"].append(ex.astype(np.uint8)), out["ref_tors"].append(ref["tors"].astype(np.float64))
            assert np.array_equal(out["ref_rot"][-1], ref["rot"]) and np.array_equal(out["ref_trans"][-1], ref["trans"])  # float32 as they come
            print(f"{name:8s} L {len(atoms):4d} window {first:3d}..{last:3d} present {count:4d} compared {int(ex.sum()):4d}  "
                  f"gap rot {gap[0]:.2e} trans {gap[1]:.2e} torsion {gap[2]:.2e}  margin w {res['margin']['w']:.2e} "
                  f"l0 {res['margin']['l0']:.2e} l1 {res['margin']['l1']:.2e}")
            worst = np.maximum(worst, gap)
        else:
            print(f"{name:8s} L {len(atoms):4d} no present residue: inputs only")
        out["ref_gap"].append(gap)
    lens = [len(cs[n][0]) for n in names]
    wins = [len(x) for x in out["ref_exists"]]
    it = iter(wins)
    win_len = [next(it) if np_window(cs[n][1])[2] else 0 for n in names]
    save = dict(names=np.array(names), row_start=np.cumsum([0] + lens), win_start=np.cumsum([0] + win_len),
                atoms=np.concatenate(out["atoms"]), mask=np.concatenate(out["mask"]), res_index=np.concatenate(out["res_index"]),
                ref_rot=np.concatenate(out["ref_rot"]), ref_trans=np.concatenate(out["ref_trans"]),
                ref_exists=np.concatenate(out["ref_exists"]), ref_tors=np.concatenate(out["ref_tors"]), ref_gap=np.stack(out["ref_gap"]))
    np.savez_compressed(GOLD, **save)
    print(f"wrote {GOLD} ({os.path.getsize(GOLD)} bytes)")
    print(f"largest difference of the reference from the float64 restatement: rotation entries {worst[0]:.1e}, translations "
          f"{worst[1]:.1e} A, torsions {worst[2]:.1e}")
    assert os.path.getsize(GOLD) < 1_000_000


if __name__ == "__main__":
    main()
