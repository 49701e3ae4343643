"""Writes tests/golden/mmcif_read.npz: the hand-written mmCIF texts that tests/test_mmcif_read.py reads with pdb.parse_mmcif and with
its own pure-Python reader.  Only texts are stored; what they must read as is worked out by the test's reader at run time.

    python tools/make_golden_mmcif_read.py

cases [k] names; per case `{case}.files` and `{case}.file{j}` uint8.  Every text is written by hand below, in the dialect the
wwPDB writes, and bent one way per case (the test's docstrings say which).
"""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "mmcif_read.npz")

# the wwPDB's column order
PDBX = ("group_PDB id type_symbol label_atom_id label_alt_id label_comp_id label_asym_id label_entity_id label_seq_id "
        "pdbx_PDB_ins_code Cartn_x Cartn_y Cartn_z occupancy B_iso_or_equiv pdbx_formal_charge auth_seq_id auth_comp_id auth_asym_id "
        "auth_atom_id pdbx_PDB_model_num").split()
RES3 = "ALA ARG ASN ASP CYS GLN GLU GLY HIS ILE LEU LYS MET PHE PRO SER THR TRP TYR VAL".split()
HEAD = "data_TEST\n#\n_entry.id TEST\n#\n"


def atom(rng, serial, name, comp, asym, seq, model=1, group="ATOM", alt=".", ins="?", occ="1.00", b=None, label_asym=None, label_seq=None,
         **more):
    x, y, z = (f"{v:.3f}" for v in rng.normal(size=3) * 20)
    d = dict(group_PDB=group, id=str(serial), type_symbol=name.strip("'\"")[0], label_atom_id=name, label_alt_id=alt, label_comp_id=comp,
             label_asym_id=label_asym or asym, label_entity_id="1", label_seq_id=str(seq if label_seq is None else label_seq),
             pdbx_PDB_ins_code=ins, Cartn_x=x, Cartn_y=y, Cartn_z=z, occupancy=occ,
             B_iso_or_equiv=f"{rng.integers(0, 9000) / 100:.2f}" if b is None else b, pdbx_formal_charge="?", auth_seq_id=str(seq),
             auth_comp_id=comp, auth_asym_id=asym, auth_atom_id=name, pdbx_PDB_model_num=str(model))
    d.update(more)
    return d


def residues(rng, n, asym, first=1, serial=1, names=("N", "CA", "C", "O", "CB"), **kw):
    out = []
    for r in range(n):
        for name in names:
            out.append(atom(rng, serial, name, RES3[(first + r) % 20], asym, first + r, **kw))
            serial += 1
    return out


def loop(atoms, tags=PDBX, sep=" ", lead="", tag=lambda t: "_atom_site." + t, keyword="loop_", tail=""):
    lines = [keyword] + [tag(t) for t in tags] + [lead + sep.join(a[t] for t in tags) + tail for a in atoms]
    return "\n".join(lines) + "\n"


def cases():
    rng = np.random.default_rng(2024)
    out = {}
    # columns in another order with columns nobody reads between them
    tags = ("pdbx_PDB_model_num Cartn_z junk_a B_iso_or_equiv label_comp_id auth_asym_id Cartn_x id label_alt_id junk_b occupancy "
            "auth_seq_id label_atom_id Cartn_y pdbx_PDB_ins_code group_PDB").split()
    out["permuted"] = [HEAD + loop(residues(rng, 6, "A", junk_a="x", junk_b="?"), tags) + "#\n"]
    # only the label_ ids
    out["label_only"] = [HEAD + loop(residues(rng, 5, "B", first=3), [t for t in PDBX if not t.startswith("auth_")]) + "#\n"]
    # both ids, and they differ
    both = residues(rng, 4, "H", first=101, label_asym="A", label_seq=1) + residues(rng, 3, "L", first=-2, serial=30, label_asym="B", label_seq=9)
    for k, a in enumerate(both):
        a["label_seq_id"] = str(int(a["label_seq_id"]) + k // 5 % 4)
    out["both_ids"] = [HEAD + loop(both) + "#\n"]
    # quotes: "O5'", 'CA', a quoted token with blanks in a column nobody reads, a quote inside an unquoted token
    q = residues(rng, 2, "A", note="'two words'")
    q += [atom(rng, 11, "\"O5'\"", "DA", "A", 3, note="\"it's a b\""), atom(rng, 12, "'CA'", "GLY", "A", 4, note="plain"),
          atom(rng, 13, "C", "GLY", "A", 4, note="'a  b'"), atom(rng, 14, "O5'", "GLY", "A", 4, note="''"), atom(rng, 15, "\"N\"", "'GLY'", "\"A\"", 4, note="x")]
    out["quoted"] = [HEAD + loop(q, PDBX[:10] + ["note"] + PDBX[10:]) + "#\n"]
    # tabs between the tokens, blanks in front of the rows, a comment behind them, blank lines among tags and rows
    t = loop(residues(rng, 3, "A"), sep="\t", lead="  \t", tail="  # a comment").replace("_atom_site.Cartn_x\n", "_atom_site.Cartn_x  # x\n\n  \n")
    t = t.replace("\n  \tATOM\t8\t", "\n\n \t \n  \tATOM\t8\t").replace("_atom_site.id", " \t_atom_site.id")
    out["tabs"] = [HEAD + t + "#\n"]
    # a text field in another category that looks like a loop, the real loop, an anisotrop loop behind it
    fake = "loop_\n_atom_site.Cartn_x\n_atom_site.Cartn_y\nATOM 1 N N . ALA A 1 1 ? 1.000 2.000 3.000 1.00 0.00 ? 1 ALA A N 1\n"
    field = "_struct.title\n;A title that goes on\n" + fake + ";\n_struct.pdbx_descriptor\n;second field\n  ; is no closing line here\n" + fake + ";\n#\n"
    aniso = ("loop_\n_atom_site_anisotrop.id\n_atom_site_anisotrop.U[1][1]\n_atom_site_anisotrop.pdbx_auth_seq_id\n"
             "1 0.123 1\n2 0.456 1\nATOM 3 C C . ALA A 1 1 ? 1.000 2.000 3.000 1.00 0.00 ? 1 ALA A C 1\n#\n")
    out["text_field"] = [HEAD + field + loop(residues(rng, 4, "A")) + "#\n" + aniso]
    # atom_site in key-value form, no atom_site at all, an empty file -- in the middle of a list
    a = atom(rng, 1, "CA", "GLY", "A", 1)
    keyvalue = HEAD + "".join(f"_atom_site.{t}  {a[t]}\n" for t in PDBX) + "#\n"
    nothing = HEAD + "loop_\n_citation.id\n_citation.title\nprimary 'A paper'\n2 'Another'\n#\n"
    out["library"] = [HEAD + loop(residues(rng, 3, "A")) + "#\n", keyvalue, nothing, "", HEAD + loop(residues(rng, 2, "C", first=7, junk_a="'a b'", junk_b="."), tags) + "#\n"]
    # CRLF line ends; no newline behind the last row
    out["crlf"] = [(HEAD + loop(residues(rng, 3, "A")) + "#\n").replace("\n", "\r\n"), (HEAD + loop(residues(rng, 2, "B"))).rstrip("\n"),
                   (HEAD + loop(residues(rng, 2, "C"))).replace("\n", "\r\n")[:-2], (HEAD + loop(residues(rng, 1, "D"))).replace("\n", "\r\n")[:-1]]
    # chain IDs of two bytes, one that returns; negative and five-digit residue numbers; insertion codes; alternate locations;
    # '.' and '?' for occupancy and b-factor; HETATM rows
    c = residues(rng, 2, "AA", first=-3) + residues(rng, 2, "A1", first=9999, serial=11) + residues(rng, 1, "AA", first=12345, serial=21)
    c += residues(rng, 1, "AA", first=52, serial=30, ins="A") + residues(rng, 1, "AA", first=52, serial=35, ins="B") + residues(rng, 1, "AA", first=52, serial=40)
    for k, (alt, occ, b) in enumerate([("A", "0.60", None), ("B", "0.40", None), ("A", ".", "."), ("B", "?", "?"), (".", "1", "12")]):
        c.append(atom(rng, 50 + k, ("CA", "CA", "CB", "CB", "HA")[k], "SER", "AA", 60, alt=alt, occ=occ, b=b))
    c += [atom(rng, 60, "O", "HOH", "AA", 901, group="HETATM"), atom(rng, 61, "O", "HOH", "AA", 902, group="HETATM"),
          atom(rng, 62, "SE", "MSE", "B", 1, group="HETATM"), atom(rng, 63, "CA", "MSE", "B", 1, group="HETATM"), atom(rng, 64, "CA", "ALA", "B", 1),
          atom(rng, 65, "CA", "ALA", ".", 2), atom(rng, 66, "CA", "ALA", "ABCD", 3)]
    out["chains"] = [HEAD + loop(c) + "#\n"]
    # keywords and tags in mixed case
    out["mixed_case"] = ["DATA_test\n#\n" + loop(residues(rng, 3, "A"), keyword="LOOP_",
                                                  tag=lambda t: ("_ATOM_SITE." + t.upper()) if len(t) % 2 else ("_Atom_Site." + t.lower())) + "#\n"]
    # three models that begin at model number 4, of different lengths
    m = residues(rng, 3, "A", model=4) + residues(rng, 2, "B", model=4, serial=20) + residues(rng, 4, "A", model=5) + residues(rng, 3, "A", model=7)
    out["models3"] = [HEAD + loop(m) + "#\n", HEAD + loop(residues(rng, 2, "A", model=2) + residues(rng, 2, "A", model=1)) + "#\n"]
    return out


def main():
    made = cases()
    arrays = {"cases": np.array(sorted(made))}
    for name, files in made.items():
        arrays[f"{name}.files"] = np.int64(len(files))
        for j, text in enumerate(files):
            arrays[f"{name}.file{j}"] = np.frombuffer(text.encode("latin-1"), np.uint8)
    np.savez_compressed(OUT, **arrays)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, {len(made)} cases")


if __name__ == "__main__":
    main()
