"""TEST INFRASTRUCTURE -- backbone coordinates and the files' own HELIX / SHEET records of the six coordinate files the reference
ships under ProteinMPNN/inputs/*/pdbs/, as the fixture of tests/test_dssp.py.

Run where the reference is present (oracle/ref_loader.py), never on the GPU machine:
    python tools/make_dssp_fixture.py
Writes tests/golden/dssp_chains.npz -- coordinates and labels only, nothing executable.

Per file: the first model, the first chain (the chain of the first ATOM record), alternate location blank or A, and only the
residues that have N, CA, C and O.  Per chain <name> the file holds
  <name>_xyz     float32 [n,4,3]   N, CA, C, O
  <name>_resnum  int32 [n]         the file's residue numbers
  <name>_pro     uint8 [n]         1 for a proline (no amide hydrogen: not a donor)
  <name>_ss      str               three classes from the file's own records: H inside a HELIX range of the chain, E inside a
                                   SHEET range of the chain (E wins where both claim a residue), else C
and `names`, the chain names in the order of the test's table.
"""
import glob
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_loader as rl  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "dssp_chains.npz")
ORDER = ("4GYT", "4YOW", "6MRR", "3HTN", "5L33", "6EHB")
BACKBONE = ("N", "CA", "C", "O")


def read_chain(path):
    chain, residues, order = None, {}, []
    helix, sheet = [], []
    with open(path) as f:
        for line in f:
            rec = line[:6]
            if rec == "ENDMDL":
                break
            if rec == "HELIX ":
                helix.append((line[19], int(line[21:25]), line[31], int(line[33:37])))
            elif rec == "SHEET ":
                sheet.append((line[21], int(line[22:26]), line[32], int(line[33:37])))
            elif rec == "ATOM  ":
                if chain is None:
                    chain = line[21]
                if line[21] != chain or line[16] not in " A":
                    continue
                key = (int(line[22:26]), line[26])
                if key not in residues:
                    residues[key] = dict(name=line[17:20], atoms={})
                    order.append(key)
                atom = line[12:16].strip()
                if atom in BACKBONE and atom not in residues[key]["atoms"]:
                    residues[key]["atoms"][atom] = [float(line[30:38]), float(line[38:46]), float(line[46:54])]
    keys = [k for k in order if all(a in residues[k]["atoms"] for a in BACKBONE)]
    xyz = np.array([[residues[k]["atoms"][a] for a in BACKBONE] for k in keys], np.float32)
    resnum = np.array([k[0] for k in keys], np.int32)
    pro = np.array([residues[k]["name"] == "PRO" for k in keys], np.uint8)
    ss = np.full(len(keys), "C")
    for c0, r0, c1, r1 in helix:
        if c0 == chain and c1 == chain:
            ss[(resnum >= r0) & (resnum <= r1)] = "H"
    for c0, r0, c1, r1 in sheet:
        if c0 == chain and c1 == chain:
            ss[(resnum >= r0) & (resnum <= r1)] = "E"
    return xyz, resnum, pro, "".join(ss)


def main():
    files = {os.path.basename(p)[:4]: p for p in glob.glob(os.path.join(rl.REF_ROOT, "ProteinMPNN", "inputs", "*", "pdbs", "*.pdb"))}
    out = {"names": np.array(ORDER)}
    for name in ORDER:
        xyz, resnum, pro, ss = read_chain(files[name])
        cn = np.linalg.norm(xyz[:-1, 2].astype(np.float64) - xyz[1:, 0].astype(np.float64), axis=-1)
        breaks = int(((np.diff(resnum) != 1) | (cn > 2.5)).sum())
        print(f"{name}: {len(xyz)} residues, {breaks} breaks, {int(pro.sum())} prolines, records H {ss.count('H')} E {ss.count('E')}")
        out.update({f"{name}_xyz": xyz, f"{name}_resnum": resnum, f"{name}_pro": pro, f"{name}_ss": np.array(ss)})
    np.savez_compressed(GOLD, **out)
    print(f"wrote {GOLD} ({os.path.getsize(GOLD)} bytes)")


if __name__ == "__main__":
    main()
