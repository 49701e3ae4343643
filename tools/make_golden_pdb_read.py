"""TEST INFRASTRUCTURE -- the fixture of tests/test_pdb_read.py: hand-written PDB texts, and what the UNMODIFIED reference makes of
the single-chain ones: data/parsers.py process_chain (:11-63) followed by data/utils.py parse_chain_feats (:436-445).

Run where the reference is present (oracle/ref_loader.py), in a process of its own:
    python tools/make_golden_pdb_read.py
Biopython is not installed here, so the reference's two functions run under the stub loader on duck-typed chain objects (a chain
iterates residues with .resname and .id; a residue iterates atoms with .name, .coord float32 [3] and .bfactor, a Python float)
built from the records of the test file's line reader (tests/test_pdb_read.py reference_read), as Biopython's parser would hand
them over: a residue per row, of several records with one atom name the first.

Writes tests/golden/pdb_read.npz -- data only: `cases`; per case {case}.files = F and {case}.file{k}, the bytes of its files; for
the cases of SINGLE {case}.scale and {case}.feats.{key}, the arrays of the reference's dict for chain A.

Cases:
  plain        one chain of eight residues with side chains, REMARK in front, TER and END behind
  two_chains   chains A, B and A again (a chain ID that returns), TER between them
  numbering    negative, four-digit and insertion-coded residue numbers
  altloc       alternate locations and a duplicated atom (five records lose their slot), ANISOU lines, hydrogens and an unknown
               atom name, MSE (its SE is none of the 37) and SEP
  hetatm       a chain followed by two waters and a ligand as HETATM records
  models3      three models, the second with one residue fewer
  models_same  three models of the same residues
  crlf         plain with CRLF line ends
  cut          lines cut at 54, 60 and 66 columns, no final newline
  library      five files in one call: a chain; an empty file; a file without a coordinate record; a chain that ends on residue
               A 5 without TER or END; a chain that begins with A 5
"""
import dataclasses
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import ref_loader as rl  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "pdb_read.npz")
MAX_BYTES = 100_000
SINGLE = {"plain": 1.0, "numbering": 10.0, "altloc": 1.0, "cut": 0.1}

SIDE = {"ALA": ["CB"], "GLY": [], "SER": ["CB", "OG"], "LEU": ["CB", "CG", "CD1", "CD2"], "LYS": ["CB", "CG", "CD", "CE", "NZ"],
        "TRP": ["CB", "CG", "CD1", "CD2", "NE1", "CE2", "CE3", "CZ2", "CZ3", "CH2"], "MET": ["CB", "CG", "SD", "CE"],
        "ARG": ["CB", "CG", "CD", "NE", "CZ", "NH1", "NH2"], "MSE": ["CB", "CG", "SE", "CE"], "SEP": ["CB", "OG", "P"],
        "HOH": [], "HEM": []}


class Writer:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.serial = 0
        self.lines = []

    def atom(self, name, res, chain, seq, icode=" ", alt=" ", rec="ATOM", occ=1.0, xyz=None, b=None):
        self.serial += 1
        x, y, z = self.rng.normal(size=3) * 25 if xyz is None else xyz
        b = float(self.rng.integers(0, 12000)) / 100 if b is None else b
        col = name if len(name) == 4 or name[0].isdigit() else " " + name
        self.lines.append(f"{rec:<6}{self.serial:>5} {col:<4}{alt}{res:>3} {chain}{seq:>4}{icode}   {x:8.3f}{y:8.3f}{z:8.3f}{occ:6.2f}{b:6.2f}"
                          f"          {name.lstrip('0123456789')[0]:>2}  ")

    def residue(self, res, chain, seq, icode=" ", rec="ATOM", names=None):
        for name in (["N", "CA", "C", "O"] + SIDE[res] if names is None else names):
            self.atom(name, res, chain, seq, icode, rec=rec)

    def ter(self):
        self.serial += 1
        self.lines.append(f"TER   {self.serial:>5}")

    def text(self, newline="\n", final=True):
        return (newline.join(self.lines) + (newline if final else "")).encode()


def plain(seed=1, chain="A"):
    w = Writer(seed)
    w.lines += ["HEADER    HAND WRITTEN", "REMARK   2 RESOLUTION. NOT APPLICABLE."]
    for k, res in enumerate(["MET", "ALA", "GLY", "SER", "LEU", "LYS", "TRP", "ARG"]):
        w.residue(res, chain, k + 1)
    w.atom("OXT", "ARG", chain, 8)
    w.ter()
    w.lines.append("END")
    return w


def two_chains():
    w = Writer(2)
    for k, res in enumerate(["ALA", "SER", "LEU"]):
        w.residue(res, "A", k + 1)
    w.ter()
    for k, res in enumerate(["GLY", "LYS"]):
        w.residue(res, "B", k + 1)
    w.ter()
    w.residue("TRP", "A", 4)
    w.ter()
    w.lines.append("END")
    return w


def numbering():
    w = Writer(3)
    for seq, icode, res in [(-3, " ", "ALA"), (-2, " ", "GLY"), (0, " ", "SER"), (52, " ", "LEU"), (52, "A", "LYS"), (52, "B", "ALA"),
                            (53, " ", "GLY"), (999, " ", "SER"), (1000, " ", "ALA"), (1001, " ", "ARG"), (9999, " ", "GLY")]:
        w.residue(res, "A", seq, icode)
    return w


def altloc():
    w = Writer(4)
    w.lines.append("REMARK 465 MISSING RESIDUES")
    w.residue("ALA", "A", 1, names=["N", "H", "CA", "HA", "C", "O", "CB", "1HB", "2HB"])
    for name in ["N", "CA"]:
        w.atom(name, "SER", "A", 2)
    w.lines.append(f"ANISOU{w.serial:>5}  CA  SER A   2     2406   1892   1614    198    519   -328       C  ")
    w.atom("C", "SER", "A", 2), w.atom("O", "SER", "A", 2)
    for alt, occ in (("A", 0.4), ("B", 0.6)):                                        # (the first wins here, the second in Biopython)
        w.atom("CB", "SER", "A", 2, alt=alt, occ=occ), w.atom("OG", "SER", "A", 2, alt=alt, occ=occ)
    w.residue("MSE", "A", 3)
    w.residue("LEU", "A", 4, names=["N", "CA", "C", "O", "CB", "CG", "CD1", "HD11", "CD2", "XX"])
    w.atom("CD1", "LEU", "A", 4)                                                     # a duplicated atom
    w.residue("SEP", "A", 5)
    for alt in "AB":
        w.atom("N", "GLY", "A", 6, alt=alt, occ=0.5), w.atom("CA", "GLY", "A", 6, alt=alt, occ=0.5)
    w.atom("C", "GLY", "A", 6), w.atom("O", "GLY", "A", 6)
    w.residue("ALA", "A", 7, names=["H1", "H2"])                                     # nothing but hydrogens: a row with an empty mask
    return w


def hetatm():
    w = Writer(5)
    for k, res in enumerate(["ALA", "LYS", "GLY"]):
        w.residue(res, "A", k + 1)
    w.ter()
    w.residue("HEM", "A", 201, rec="HETATM", names=["FE", "NA", "C1A", "O1A"])
    w.residue("HOH", "A", 301, rec="HETATM", names=["O"])
    w.residue("HOH", "A", 302, rec="HETATM", names=["O"])
    w.lines.append("END")
    return w


def models(counts, seed):
    w = Writer(seed)
    for m, n in enumerate(counts):
        w.serial = 0
        w.lines.append(f"MODEL     {m + 1:>4}")
        for k in range(n):
            w.residue(["ALA", "GLY", "SER", "LEU"][k % 4], "A", k + 1)
        w.ter()
        w.lines.append("ENDMDL")
    w.lines.append("END")
    return w


def cut():
    w = plain(6)
    keep = []
    for k, line in enumerate(w.lines):
        keep.append(line[:(54, 60, 66, 80)[k % 4]] if line.startswith("ATOM") else line)
    w.lines = keep[:-2]                                                              # (the last line is an ATOM record without a newline)
    return w


def library():
    ends = Writer(8)
    for k, res in enumerate(["ALA", "GLY", "SER", "LEU", "LYS"]):
        ends.residue(res, "A", k + 1)
    begins = Writer(9)
    for k, res in enumerate(["LYS", "ALA", "TRP"]):
        begins.residue(res, "A", k + 5)
    begins.lines.append("END")
    return [plain(7).text(), b"", b"HEADER    NOTHING\nREMARK   1 NO COORDINATES\nEND\n", ends.text(), begins.text()]


def cases():
    crlf = plain(1)
    return {"plain": [plain().text()], "two_chains": [two_chains().text()], "numbering": [numbering().text()],
            "altloc": [altloc().text()], "hetatm": [hetatm().text()], "models3": [models((4, 3, 4), 10).text()],
            "models_same": [models((3, 3, 3), 11).text()], "crlf": [crlf.text(newline="\r\n")], "cut": [cut().text(final=False)],
            "library": library()}


# ---- duck-typed Biopython objects ------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Atom:
    name: str
    coord: np.ndarray
    bfactor: float


class Residue(list):
    def __init__(self, resname, rid, atoms):
        super().__init__(atoms)
        self.resname, self.id = resname, rid


def chain_of(text):
    """the rows of the line reader as the residues of one Biopython chain"""
    import test_pdb_read as tr
    lines = [raw[:-1] if raw.endswith(b"\r") else raw for raw in text.split(b"\n")]
    names = [line[17:20].decode().strip() for line in lines if line[:6] == b"ATOM  "]
    read = tr.reference_read([text])
    assert set(read["chain_id"].tolist()) == {ord("A")}
    residues, at = [], 0
    for r, records in enumerate(read["records"]):
        atoms, seen = [], set()
        for name, x, y, z, b in records:
            if name.strip() not in seen:
                seen.add(name.strip())
                atoms.append(Atom(name.strip(), np.array([x, y, z], np.float32), float(b)))
        residues.append(Residue(names[at], (" ", int(read["residue_index"][r]), " "), atoms))
        at += len(records)
    return residues


def main():
    rl.install()
    from data import parsers
    from data import utils as du

    store, names = {}, []
    for name, files in cases().items():
        names.append(name)
        store[f"{name}.files"] = np.array(len(files))
        for k, blob in enumerate(files):
            store[f"{name}.file{k}"] = np.frombuffer(blob, np.uint8)
        if name in SINGLE:
            prot = parsers.process_chain(chain_of(files[0]), "A")
            feats = du.parse_chain_feats({k: dataclasses.asdict(prot)[k] for k in du.CHAIN_FEATS}, scale_factor=SINGLE[name])
            store[f"{name}.scale"] = np.array(SINGLE[name])
            for k, v in feats.items():
                store[f"{name}.feats.{k}"] = np.asarray(v)
            print(f"{name:12s} {len(files[0])} bytes, reference dict: " + ", ".join(f"{k} {np.asarray(v).dtype}{np.asarray(v).shape}" for k, v in feats.items()))
        else:
            print(f"{name:12s} {[len(b) for b in files]} bytes")
    np.savez_compressed(GOLD, cases=np.array(names), **store)
    size = os.path.getsize(GOLD)
    print(f"wrote {GOLD} ({size} bytes)")
    assert size < MAX_BYTES, size


if __name__ == "__main__":
    main()
