"""TEST INFRASTRUCTURE -- golden bytes for se3_diffusion_amd.pdb from the UNMODIFIED reference: analysis/utils.py
write_prot_to_pdb (:39-77), which formats every frame with data/protein.py to_pdb (:146-224).

Run where the reference is present (oracle/ref_loader.py), in a process of its own:
    python tools/make_golden_pdb.py
Writes tests/golden/pdb.npz -- data only: per case the inputs ({case}.x float32, {case}.aatype int64 and {case}.b float32 where
the case has them) and {case}.text, the bytes of the file the reference wrote; `cases`, the case names; `naming`, a JSON list of
scenarios {pre: names in the directory beforehand, calls: [[file name, overwrite, no_indexing], ..], chosen: the base names the
reference returned}, each run in a temporary directory of its own.

Cases (tests/test_pdb.py runs them all, on the interpreter and on the device):
  single        [1,37,3], one frame (three dimensions) of one residue, every atom present
  allatoms_k    [2,3,37,3], every atom present, aatype (3k, 3k+1, 3k+2), k = 0..6: all of 0..20, UNK last in allatoms_6
  backbone      [3,70,37,3], slots 0..4 only: serials cross 9|10 and 99|100; b-factors 100 x a 0/1 mask
  holes         [2,9,37,3], about half of the atoms exactly zero, random aatype, b-factors per atom (fractional, negative)
  empty_res     [1,5,37,3] backbone, residue 2 without an atom
  empty_ends    [1,5,37,3] backbone, residues 0 and 4 without an atom
  empty_model   [3,4,37,3] backbone, model 1 without an atom (TER with serial 1)
  strided       x[:, 1] of a [4,3,6,37,3] backbone record, stored as the contiguous copy
  numbers       the values where %.3f and %.2f can go wrong: every k/16 and k/8 tie in -4 .. 4, signed zeros, -0.0004, values that
                gain a digit (9.9996, 999.9996, -99.9996), the extremes -999.999 and 9999.999; b-factors 0, 100, ties, negative
  random        [1,24,37,3]: 2664 random float32 coordinates of mixed magnitude
"""
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_loader as rl  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "pdb.npz")
MAX_BYTES = 300_000


def backbone_only(x):
    x = x.copy()
    x[..., 5:, :] = 0.0
    return x


def number_values():
    """(coordinates, b-factors) that sit on the edges of the two formats"""
    ties3 = [k / 16 for k in range(-64, 65)]
    ties2 = [k / 8 for k in range(-32, 33)]
    coords = ties3 + [-0.0, 0.0, -0.0004, 0.0004, -0.0005, 0.0005, 0.0015, -0.0015, 9.9996, 999.9996, -99.9996, 99.9995, -9.9996,
                      -999.999, 9999.999, 9999.9990234375, -999.9990234375, 1e-8, -1e-8, 1e-4, 123.4565, 0.0625, 0.1875, 1234.5675]
    bfac = ties2 + [0.0, -0.0, 100.0, 0.005, 0.015, -0.004, -0.005, 9.996, 99.996, 999.99, -99.99, 12.345, -7.125, 54.321, 1e-8]
    return np.array(coords, np.float32), np.array(bfac, np.float32)


def cases():
    rng = np.random.default_rng(20)
    f32 = lambda a: np.asarray(a, np.float32)
    out = {}
    out["single"] = dict(x=f32(rng.normal(size=(1, 37, 3)) * 10))
    xa = f32(rng.normal(size=(2, 3, 37, 3)) * 15)
    for k in range(7):
        out[f"allatoms_{k}"] = dict(x=xa, aatype=np.arange(3 * k, 3 * k + 3))
    out["backbone"] = dict(x=backbone_only(f32(rng.normal(size=(3, 70, 37, 3)) * 20)),
                           b=np.tile(f32(100.0 * (rng.random(70) < 0.7))[:, None], (1, 37)))
    xh = f32(rng.normal(size=(2, 9, 37, 3)) * 12)
    xh[rng.random((2, 9, 37)) < 0.5] = 0.0
    out["holes"] = dict(x=xh, aatype=rng.integers(0, 21, size=9), b=np.clip(f32(rng.normal(size=(9, 37)) * 40), -99.0, 999.0))
    xe = backbone_only(f32(rng.normal(size=(1, 5, 37, 3)) * 8))
    x1, x2 = xe.copy(), xe.copy()
    x1[0, 2] = 0.0
    x2[0, [0, 4]] = 0.0
    out["empty_res"] = dict(x=x1)
    out["empty_ends"] = dict(x=x2, aatype=np.array([3, 7, 20, 11, 5]))
    xm = backbone_only(f32(rng.normal(size=(3, 4, 37, 3)) * 8))
    xm[1] = 0.0
    out["empty_model"] = dict(x=xm)
    rec = backbone_only(f32(rng.normal(size=(4, 3, 6, 37, 3)) * 25))
    out["strided"] = dict(x=np.ascontiguousarray(rec[:, 1]), b=np.tile(f32([100, 0, 100, 100, 0, 100])[:, None], (1, 37)))
    cv, bv = number_values()
    n_atoms = len(cv)
    N = -(-n_atoms // 37)
    xn = np.zeros((N * 37, 3), np.float32)
    xn[:n_atoms, 0] = cv
    xn[:n_atoms, 1] = np.roll(cv, 7)
    xn[:n_atoms, 2] = 1.5                                             # (keeps every one of them present)
    out["numbers"] = dict(x=xn.reshape(1, N, 37, 3), b=np.resize(bv, N * 37).reshape(N, 37))
    scale = np.array([0.01, 1.0, 10.0, 100.0, 1000.0])[rng.integers(0, 5, size=(1, 24, 37, 3))]
    out["random"] = dict(x=np.clip(f32(rng.normal(size=(1, 24, 37, 3)) * scale), -999.0, 9999.0),
                         b=f32(rng.uniform(-99, 999, size=(24, 37))))
    return out


NAMING = [
    dict(pre=[], calls=[["x", False, False]]),
    dict(pre=["x_1.pdb", "x_3.pdb"], calls=[["x", False, False]]),
    dict(pre=["x_1.pdb", "x_3.pdb"], calls=[["x", True, False]]),
    dict(pre=["x_1.pdb", "x_3.pdb"], calls=[["x.pdb", False, True]]),
    dict(pre=[], calls=[["y.pdb", False, False], ["y.pdb", False, False]]),
    dict(pre=[], calls=[["sample", False, False], ["bb_traj", False, False], ["x0_traj", False, False]]),
    dict(pre=[], calls=[["sample", False, False], ["bb_traj", False, False], ["x0_traj", False, False]] * 2),
    dict(pre=["x0_traj_5.pdb", "other_9.pdb"], calls=[["bb_traj", False, False], ["pdb", False, False]]),
]


def main():
    rl.install()
    from analysis import utils as au

    store, names = {}, []
    with tempfile.TemporaryDirectory() as tmp:
        for name, c in cases().items():
            x = c["x"]
            path = au.write_prot_to_pdb(x, os.path.join(tmp, name), aatype=c.get("aatype"),
                                        b_factors=c.get("b"), overwrite=True)
            with open(path, "rb") as f:
                text = np.frombuffer(f.read(), np.uint8)
            names.append(name)
            store[f"{name}.x"] = x
            if "aatype" in c:
                store[f"{name}.aatype"] = np.asarray(c["aatype"], np.int64)
            if "b" in c:
                store[f"{name}.b"] = c["b"]
            store[f"{name}.text"] = text
            print(f"{name:12s} x {x.shape}  {len(text)} bytes")
    frame = np.ones((1, 37, 3), np.float32)
    naming = []
    for sc in NAMING:
        with tempfile.TemporaryDirectory() as tmp:
            for n in sc["pre"]:
                open(os.path.join(tmp, n), "w").close()
            chosen = [os.path.relpath(au.write_prot_to_pdb(frame, os.path.join(tmp, fn), overwrite=ow, no_indexing=ni), tmp)
                      for fn, ow, ni in sc["calls"]]
        naming.append(dict(sc, chosen=chosen))
        print(sc["pre"], sc["calls"], "->", chosen)
    np.savez_compressed(GOLD, cases=np.array(names), naming=np.array(json.dumps(naming)), **store)
    size = os.path.getsize(GOLD)
    print(f"wrote {GOLD} ({size} bytes)")
    assert size < MAX_BYTES, size


if __name__ == "__main__":
    main()
