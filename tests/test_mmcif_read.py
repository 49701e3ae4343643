"""se3_diffusion_amd.pdb.parse_mmcif: the _atom_site loop of mmCIF files read into atom37 arrays on the device
(csrc/fd_cif_read.hip, fd_cif_read_lines / _marks / _header / _summary / _count / _fill).

Every comparison is == or array_equal.  Two references, neither of them Biopython's MMCIFParser, which does not exist where this
project is built:
  * pdb.parse_pdb of the same structure as PDB text: every text of tests/golden/pdb_read.npz and every file of
    tests/golden/pdb.npz (the unmodified reference writer's bytes), rewritten record by record as atom_site rows by pdb_to_cif();
  * reference_read_cif(), a pure-Python reader written from the specification in include/fd_hip.h (it splits lines, strips
    quotes and calls float()); it shares nothing with the kernel, which scans bytes and builds numbers from integers.  The
    hand-written texts of tests/golden/mmcif_read.npz (tools/make_golden_mmcif_read.py) and the boundary texts built here must
    read equal to it.
Every case runs on the interpreter and, marked gpu, on the device; the library of 200 files runs on the device only.
"""
import functools
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from se3_diffusion_amd import hip, pdb  # noqa: E402
from se3_diffusion_amd.data.chains import ChainStore  # noqa: E402

ATOMS = ("N CA C CB O CG CG1 CG2 OG OG1 SG CD CD1 CD2 ND1 ND2 OD1 OD2 SD CE CE1 CE2 CE3 NE NE1 NE2 OE1 OE2 CH2 NH1 NH2 OH CZ CZ2 "
         "CZ3 NZ OXT").split()
RES3 = "ALA ARG ASN ASP CYS GLN GLU GLY HIS ILE LEU LYS MET PHE PRO SER THR TRP TYR VAL".split()
WINDOW, CHUNK = 16, 4096                    # FD_PDB_READ_WINDOW, FD_PDB_READ_CHUNK: a thread's bytes, a block's bytes
MAX_COLS, MAX_LINE = 64, 1024               # FD_CIF_MAX_COLS, FD_CIF_MAX_LINE
TOKENS, COORD, NUMBER, RESSEQ, COLUMNS, CHAIN, MODEL = 1, 2, 3, 4, 5, 6, 7      # FD_CIF_READ_*
PDBX = ("group_PDB id type_symbol label_atom_id label_alt_id label_comp_id label_asym_id label_entity_id label_seq_id "
        "pdbx_PDB_ins_code Cartn_x Cartn_y Cartn_z occupancy B_iso_or_equiv pdbx_formal_charge auth_seq_id auth_comp_id auth_asym_id "
        "auth_atom_id pdbx_PDB_model_num").split()
FIELDS = ("atom_positions", "atom_mask", "b_factors", "aatype", "residue_index", "chain_offsets", "chain_file", "chain_model",
          "chain_id", "n_dropped")
MODES = [(h, m) for h in (False, True) for m in ("first", "all")]

WRITER = np.load(os.path.join(ROOT, "tests", "golden", "pdb.npz"))
WRITER_CASES = [str(n) for n in WRITER["cases"]]
PDB_CASES = ["plain", "two_chains", "numbering", "altloc", "hetatm", "models3", "models_same", "crlf", "cut", "library"]
CIF_CASES = ["permuted", "label_only", "both_ids", "quoted", "tabs", "text_field", "library", "crlf", "chains", "mixed_case", "models3"]


@functools.lru_cache(None)
def gold(name):
    return np.load(os.path.join(ROOT, "tests", "golden", name))


def files_of(case, name="mmcif_read.npz"):
    g = gold(name)
    return [g[f"{case}.file{k}"].tobytes() for k in range(int(g[f"{case}.files"]))]


@pytest.fixture(params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def dev(request):
    """the device the library under test runs on: the interpreter build on the CPU, or the product library on the GPU"""
    if request.param == "emu":
        request.getfixturevalue("use_emu")
        return "cpu"
    request.getfixturevalue("hip_lib")
    return "cuda"


# ---- the independent reader ------------------------------------------------------------------------------------------------------
class Refused(ValueError):
    def __init__(self, file, line, kind):
        super().__init__(f"file {file}, line {line}, kind {kind}")
        self.file, self.line, self.kind = file, line, kind


_NUMBER = re.compile(rb"[+-]?(\d+\.?\d*|\.\d+)\Z")
_INTEGER = re.compile(rb"[+-]?\d+\Z")
_BLANKS = b" \t"


def _number(tok, missing=None):
    """float(token) for an optional sign and at most 15 digits with at most one point; `missing` for no token, '.' or '?' if
    given; None for anything else"""
    if tok is None or tok in (b".", b"?"):
        return missing
    return float(tok) if _NUMBER.match(tok) and sum(c in b"0123456789" for c in tok) <= 15 else None


def _integer(tok):
    ok = tok is not None and _INTEGER.match(tok) and len(tok.lstrip(b"+-")) <= 15 and abs(int(tok)) < 2 ** 31
    return int(tok) if ok else None


def _class(raw):
    """(class, tag name) of a line as if it stood outside every text field"""
    if raw[:1] == b";":
        return "semi", None
    s = raw.lstrip(_BLANKS)
    if not s:
        return "blank", None
    parts = re.split(rb"[ \t]+", s, maxsplit=1)
    tok, rest = parts[0].lower(), (parts[1] if len(parts) > 1 else b"")
    if tok.startswith(b"#"):
        return "other", None
    if tok.startswith(b"_"):
        if tok.startswith(b"_atom_site.") and (rest == b"" or rest.startswith(b"#")):
            return "tag", tok[11:]
        return "other", None
    if tok == b"loop_":
        return "loop", None
    return ("other" if tok.startswith(b"data_") else "value"), None


def _tokens(raw):
    """(the tokens of a row up to where it ends or goes wrong, whether it went right)"""
    if len(raw) > MAX_LINE:
        return [], False
    out, q, n = [], 0, len(raw)
    while True:
        while q < n and raw[q] in _BLANKS:
            q += 1
        if q >= n or raw[q:q + 1] == b"#":
            return out, True
        c = raw[q:q + 1]
        if c in (b"'", b'"'):
            z = q + 1
            while z < n and not (raw[z:z + 1] == c and (z + 1 >= n or raw[z + 1] in _BLANKS)):
                z += 1
            if z >= n:
                return out, False
            out.append(raw[q + 1:z])
            q = z + 1
        else:
            z = q
            while z < n and raw[z] not in _BLANKS:
                z += 1
            out.append(raw[q:z])
            q = z


def _lines(blob):
    lines = blob.split(b"\n")
    if lines[-1] == b"":
        lines.pop()                                             # (a line starts behind a newline only if a byte follows)
    return [raw[:-1] if raw.endswith(b"\r") else raw for raw in lines]


def reference_read_cif(files, hetatm=False, model="first", ids="auth"):
    """include/fd_hip.h's rules for mmCIF, a line at a time.  dict of numpy arrays named as ParsedPdb's fields.  Raises
    Refused(file, line from 1, kind) for the malformed head or coordinate record of the smallest line."""
    pos, mask, bfac, aatype, resseq = [], [], [], [], []
    chain_first, chain_file, chain_model, chain_id = [], [], [], []
    dropped = np.zeros(len(files), np.int64)
    for f, blob in enumerate(files):
        lines = _lines(blob)
        classes, semis = [], 0
        for raw in lines:                                       # text fields first: they are not syntax
            c, name = _class(raw)
            classes.append(("other", None) if c == "semi" or semis % 2 else (c, name))
            semis += c == "semi"
        refused = []
        loop = tag = other = head = -1                          # the last line of each class so far
        col, width, model0, prev = None, 0, None, None          # prev: (key, model) of the coordinate record before
        for k, raw in enumerate(lines):
            c = classes[k][0]
            if c == "loop":
                loop = k
                nxt = next((j for j in range(k + 1, len(lines)) if _class(lines[j])[0] != "blank"), None)
                if nxt is not None and _class(lines[nxt])[0] == "tag":
                    if head >= 0:
                        refused.append((k, COLUMNS))
                        break
                    head, col, j = k, {}, k + 1
                    while j < len(lines) and _class(lines[j])[0] in ("tag", "blank"):
                        if _class(lines[j])[0] == "tag":
                            if width < MAX_COLS:
                                col[_class(lines[j])[1]] = width
                            width += 1
                        j += 1
                    for what in ("asym", "seq"):
                        col[what] = col.get(b"label_%s_id" % what.encode()) if ids == "label" or b"auth_%s_id" % what.encode() not in col \
                            else col[b"auth_%s_id" % what.encode()]
                    need = [b"label_atom_id", b"label_alt_id", b"label_comp_id", b"cartn_x", b"cartn_y", b"cartn_z", "asym", "seq"]
                    if width > MAX_COLS or any(col.get(n) is None for n in need):
                        refused.append((k, COLUMNS))
                        break
            elif c == "tag":
                tag = k
            elif c == "other":
                other = k
            if c != "value" or not (loop >= 0 and head == loop and tag > loop and loop > other):
                continue
            toks, ok = _tokens(raw)
            ok = ok and len(toks) == width
            get = lambda n: toks[col[n]] if col.get(n) is not None and col[n] < len(toks) else None
            het = get(b"group_pdb") == b"HETATM"
            if het and not hetatm:
                continue
            if not ok:
                refused.append((k, TOKENS))
                break
            num = _integer(get(b"pdbx_pdb_model_num")) if b"pdbx_pdb_model_num" in col else 1
            if model0 is None:
                model0 = num
            if num is not None and model == "first" and num != model0:
                prev = None
                continue
            xyz = [_number(get(n)) for n in (b"cartn_x", b"cartn_y", b"cartn_z")]
            occ, b = _number(get(b"occupancy"), 1.0), _number(get(b"b_iso_or_equiv"), 0.0)
            seq, chain = _integer(get("seq")), get("asym")
            kinds = [COORD] * any(v is None for v in xyz) + [NUMBER] * (occ is None or b is None) + [RESSEQ] * (seq is None) + \
                [CHAIN] * (not 1 <= len(chain) <= 4) + [MODEL] * (num is None)
            if kinds:
                refused.append((k, min(kinds)))
                break
            chain = b" " if chain in (b".", b"?") else chain
            ins = get(b"pdbx_pdb_ins_code")
            ins = b" " if ins is None or ins in (b".", b"?", b"") else ins[:1]
            key = (chain, seq, ins, het)
            if prev is None or prev != (key, num):
                if prev is None or prev[1] != num or prev[0][0] != chain:
                    chain_first.append(len(pos)), chain_file.append(f), chain_model.append(num - model0)
                    chain_id.append(int.from_bytes(chain.ljust(4, b"\0"), "little"))
                pos.append(np.zeros((37, 3), np.float32)), mask.append(np.zeros(37, np.uint8)), bfac.append(np.zeros(37, np.float32))
                comp = get(b"label_comp_id").decode("latin-1")
                aatype.append(RES3.index(comp) if comp in RES3 else 20)
                resseq.append(seq)
            prev = (key, num)
            name = get(b"label_atom_id").decode("latin-1")
            if name in ATOMS:
                s = ATOMS.index(name)
                if mask[-1][s]:
                    dropped[f] += 1
                else:
                    pos[-1][s], mask[-1][s], bfac[-1][s] = np.float32(xyz), 1, np.float32(b)
        if refused:
            raise Refused(f, refused[0][0] + 1, refused[0][1])
    T = len(pos)
    return {"atom_positions": np.array(pos, np.float32).reshape(T, 37, 3), "atom_mask": np.array(mask, np.uint8).reshape(T, 37),
            "b_factors": np.array(bfac, np.float32).reshape(T, 37), "aatype": np.array(aatype, np.int64),
            "residue_index": np.array(resseq, np.int64), "chain_offsets": np.array(chain_first + [T], np.int64),
            "chain_file": np.array(chain_file, np.int32), "chain_model": np.array(chain_model, np.int32),
            "chain_id": np.array(chain_id, np.int32), "n_dropped": dropped}


def assert_same(parsed, want):
    for k in FIELDS:
        got, ref = getattr(parsed, k), want[k] if isinstance(want, dict) else getattr(want, k).cpu().numpy()
        got = got.cpu().numpy()
        assert got.dtype == ref.dtype and got.shape == ref.shape, (k, got.dtype, got.shape, ref.dtype, ref.shape)
        assert np.array_equal(got, ref), k


def assert_reads_like_the_reference(files, **kw):
    """parse_mmcif gives reference_read_cif's arrays, or refuses the same file and line for the same reason"""
    try:
        want = reference_read_cif(files, **kw)
    except Refused as e:
        with pytest.raises(ValueError, match=re.escape(pdb.CIF_KINDS[e.kind]) + f" in file {e.file} .*, line {e.line}$"):
            pdb.parse_mmcif(files, **kw)
        return None
    parsed = pdb.parse_mmcif(files, **kw)
    assert_same(parsed, want)
    return parsed


# ---- the converter ---------------------------------------------------------------------------------------------------------------
def _quoted(tok, missing="?"):
    if tok == "":
        return missing
    return f'"{tok}"' if any(c in tok for c in " \t") or tok[0] in "'\"#_;" else tok


def pdb_to_cif(blob, tags=PDBX):
    """the ATOM / HETATM records of PDB text as an atom_site loop: the model number is one more than the ENDMDL records in front,
    a blank chain ID becomes '.', a blank field '?'"""
    rows, model = [], 1
    for raw in _lines(blob):
        line = raw[:80].decode("latin-1").ljust(80)
        if line[:6] == "ENDMDL":
            model += 1
        if line[:6] not in ("ATOM  ", "HETATM"):
            continue
        name, comp, seq = line[12:16].strip(" "), line[17:20].strip(" "), line[22:26].strip(" ")
        v = dict(group_PDB=line[:6].strip(), id=line[6:11].strip() or "?", type_symbol=line[76:78].strip() or "?", label_atom_id=_quoted(name),
                 label_alt_id=_quoted(line[16].strip(), "."), label_comp_id=_quoted(comp), label_asym_id=_quoted(line[21].strip(), "."),
                 label_entity_id="1", label_seq_id=seq, pdbx_PDB_ins_code=_quoted(line[26].strip()), Cartn_x=line[30:38].strip(),
                 Cartn_y=line[38:46].strip(), Cartn_z=line[46:54].strip(), occupancy=line[54:60].strip() or "?",
                 B_iso_or_equiv=line[60:66].strip() or ".", pdbx_formal_charge="?", auth_seq_id=seq, auth_comp_id=_quoted(comp),
                 auth_asym_id=_quoted(line[21].strip(), "."), auth_atom_id=_quoted(name), pdbx_PDB_model_num=str(model))
        rows.append(" ".join(v[t] for t in tags))
    if not rows:
        return b"data_none\n#\n_entry.id none\n#\n"
    return ("data_conv\n#\nloop_\n" + "".join(f"_atom_site.{t}\n" for t in tags) + "\n".join(rows) + "\n#\n").encode("latin-1")


# ---- 1. the same structure as PDB text and as mmCIF text ---------------------------------------------------------------------------
@pytest.mark.parametrize("hetatm,model", MODES)
@pytest.mark.parametrize("case", PDB_CASES)
def test_equals_parse_pdb_on_the_pdb_reader_texts(dev, case, hetatm, model):
    files = files_of(case, "pdb_read.npz")
    want = pdb.parse_pdb(files, hetatm=hetatm, model=model)
    assert_same(pdb.parse_mmcif([pdb_to_cif(b) for b in files], hetatm=hetatm, model=model), want)


@pytest.mark.parametrize("name", WRITER_CASES)
def test_equals_parse_pdb_on_the_reference_writer_files(dev, name):
    text = WRITER[f"{name}.text"].tobytes()
    cif = pdb_to_cif(text)
    for hetatm, model in MODES:
        want = pdb.parse_pdb(text, hetatm=hetatm, model=model)
        assert_same(pdb.parse_mmcif(torch.from_numpy(np.frombuffer(cif, np.uint8).copy()).to(dev), hetatm=hetatm, model=model), want)


# ---- 2. against the independent reader ---------------------------------------------------------------------------------------------
def test_fixture_holds_what_it_is_named_for():
    assert sorted(str(n) for n in gold("mmcif_read.npz")["cases"]) == sorted(CIF_CASES)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "mmcif_read.npz")) < 100_000
    one = lambda case: files_of(case)[0]
    tags = [t.split(b".")[1] for t in one("permuted").split(b"\n") if t.startswith(b"_atom_site.")]
    assert sorted(tags) != tags and tags[0] == b"pdbx_PDB_model_num" and b"junk_a" in tags and tags != [t.encode() for t in PDBX]
    assert b"auth_" not in one("label_only") and b"label_asym_id" in one("label_only")
    a, b = reference_read_cif(files_of("both_ids")), reference_read_cif(files_of("both_ids"), ids="label")
    assert [a["chain_id"].tolist(), b["chain_id"].tolist()] == [[ord("H"), ord("L")], [ord("A"), ord("B")]]
    assert not np.array_equal(a["residue_index"], b["residue_index"])
    assert b"\"O5'\"" in one("quoted") and b" 'CA' " in one("quoted") and b"'two words'" in one("quoted") and b"''" in one("quoted")
    assert _tokens(b"x \"O5'\" 'a  b' \"it's a b\" # c")[0] == [b"x", b"O5'", b"a  b", b"it's a b"]
    assert b"\tATOM\t" in one("tabs") and b"\n  \tATOM" in one("tabs") and b"  # a comment\n" in one("tabs") and b"\n \t \n" in one("tabs")
    field = one("text_field")
    assert field.count(b"\nloop_\n_atom_site.Cartn_x\n") == 2 and field.count(b"\nloop_\n_atom_site.") == 3 and field.count(b"\n;") == 4 and b"_atom_site_anisotrop." in field
    assert len(reference_read_cif([field])["aatype"]) == 4
    lib = files_of("library")
    assert len(lib) == 5 and lib[3] == b"" and b"_atom_site.Cartn_x  " in lib[1] and b"loop_" not in lib[1] and b"_atom_site" not in lib[2]
    assert reference_read_cif(lib)["chain_file"].tolist() == [0, 4]
    crlf = files_of("crlf")
    assert b"\r\n" in crlf[0] and b"\r" not in crlf[1] and not crlf[1].endswith(b"\n") and crlf[2][-1:] not in b"\r\n" and crlf[3].endswith(b"\r")
    r = reference_read_cif(files_of("chains"), hetatm=True)
    names = [int(c).to_bytes(4, "little").rstrip(b"\0").decode() for c in r["chain_id"]]
    assert names == ["AA", "A1", "AA", "B", " ", "ABCD"] and {-3, 9999, 10000, 12345} <= set(r["residue_index"].tolist())
    assert r["n_dropped"].tolist() == [2] and r["residue_index"].tolist().count(52) == 3
    assert b" . . " in one("chains") and b" ? ? " in one("chains")
    assert b"LOOP_\n" in one("mixed_case") and b"_ATOM_SITE.CARTN_X" in one("mixed_case") and b"_Atom_Site.id" in one("mixed_case")
    r = reference_read_cif(files_of("models3"), model="all")
    assert r["chain_model"].tolist() == [0, 0, 1, 3, 0, -1] and len(reference_read_cif(files_of("models3"))["chain_model"]) == 3


@pytest.mark.parametrize("ids", ["auth", "label"])
@pytest.mark.parametrize("hetatm,model", MODES)
@pytest.mark.parametrize("case", CIF_CASES)
def test_kernel_equals_the_independent_reader(dev, case, hetatm, model, ids):
    files = files_of(case)
    parsed = assert_reads_like_the_reference(files, hetatm=hetatm, model=model, ids=ids)
    if parsed is not None:                                                           # two runs give identical arrays
        again = pdb.parse_mmcif(files, hetatm=hetatm, model=model, ids=ids)
        assert all(torch.equal(getattr(parsed, k), getattr(again, k)) for k in FIELDS)
    else:
        assert ids == "label" and case in ("permuted", "library")                   # the texts without label_ ids


# ---- 3. window, chunk and file boundaries ------------------------------------------------------------------------------------------
def comment(n):
    """a comment line of n bytes, newline included"""
    assert n >= 2
    return "#".ljust(n - 1, ".") + "\n"


def blank(n):
    """a blank line of n bytes, newline included"""
    return " " * (n - 1) + "\n"


def pad_to(text, at, line=comment):
    """text with comment lines behind it so that it is `at` bytes long"""
    while at - len(text) > 300:
        text += line(200)
    if at - len(text) > 2:
        text += line(at - len(text) - 1)
    return text + "\n" * (at - len(text))


def atom_row(rng, serial, name, seq, asym="A", tags=PDBX, model=1, wide=0):
    x, y, z = (f"{v:.3f}" for v in rng.normal(size=3) * 20)
    comp = RES3[seq % 20]
    v = dict(group_PDB="ATOM", id=str(serial), type_symbol=name[0], label_atom_id=name, label_alt_id=".", label_comp_id=comp, label_asym_id=asym,
             label_entity_id="1", label_seq_id=str(seq), pdbx_PDB_ins_code="?", Cartn_x=x, Cartn_y=y, Cartn_z=z, occupancy="1.00",
             B_iso_or_equiv=f"{rng.integers(0, 9000) / 100:.2f}", pdbx_formal_charge="?", auth_seq_id=str(seq), auth_comp_id=comp,
             auth_asym_id=asym, auth_atom_id=name, pdbx_PDB_model_num=str(model))
    row = " ".join(v[t] for t in tags)
    return row + " " * max(0, wide - len(row))


def header(tags=PDBX):
    return "loop_\n" + "".join(f"_atom_site.{t}\n" for t in tags)


def rows_text(rng, n, first=1, serial=1, **kw):
    return "".join(atom_row(rng, serial + 3 * r + k, name, first + r, **kw) + "\n" for r in range(n) for k, name in enumerate(("N", "CA", "C")))


@pytest.mark.parametrize("shift", [2, 9, 15, 16, 17, 30])
def test_rows_start_at_every_place_of_a_window(dev, shift):
    """a thread owns WINDOW = 16 bytes: rows of 80 bytes and a newline behind a first line of `shift` bytes start at every offset
    of a window, and each lies across five window boundaries"""
    rng = np.random.default_rng(31)
    text = comment(shift) + header() + "".join(atom_row(rng, k, ("N", "CA", "C")[k % 3], 1 + k // 3, wide=80) + "\n" for k in range(48))
    assert {m.start() % WINDOW for m in re.finditer(b"\nATOM", text.encode())} == set(range(WINDOW))
    assert_reads_like_the_reference([text.encode()[:-1]])


def test_row_and_residue_across_a_chunk_boundary(dev):
    """a block owns CHUNK = 4096 bytes: a row begins 40 bytes in front of byte 4096 and ends behind it, its residue's other rows lie
    on both sides; the newline of another row is the last byte of chunk 1"""
    rng = np.random.default_rng(32)
    head = pad_to("data_x\n", CHUNK - 40 - 80 - len(header())) + header() + atom_row(rng, 1, "N", 1, wide=79) + "\n"
    assert len(head) == CHUNK - 40
    text = head + atom_row(rng, 2, "CA", 1) + "\n" + atom_row(rng, 3, "C", 1) + "\n" + rows_text(rng, 6, first=2, serial=4)
    text = pad_to(text, 2 * CHUNK - 80, line=blank) + atom_row(rng, 100, "N", 50, wide=79) + "\n"      # (blank lines may stand among rows)
    text += atom_row(rng, 101, "CA", 50) + "\n" + rows_text(rng, 5, first=51, serial=102) + "#\n"
    raw = text.encode()
    assert raw[CHUNK - 41:CHUNK - 36] == b"\nATOM" and raw[2 * CHUNK - 1:2 * CHUNK + 4] == b"\nATOM" and len(raw) > 2 * CHUNK
    parsed = assert_reads_like_the_reference([raw])
    assert parsed.num_residues == 13 and parsed.atom_mask.sum(1).tolist() == [3] * 7 + [2] + [3] * 5


def test_tag_lines_across_a_chunk_boundary(dev):
    rng = np.random.default_rng(33)
    text = pad_to("data_x\n", CHUNK - 150) + header() + rows_text(rng, 4) + "#\n"
    assert text[:CHUNK].count("_atom_site.") in range(3, 12)
    assert assert_reads_like_the_reference([text.encode()]).num_residues == 4


def test_a_chunk_without_a_line_start_inside_a_text_field(dev):
    """one line of a text field covers all of chunk 1; the field opens in chunk 0 and closes in chunk 2, and the lines of chunk 0
    and 2 inside it look like a loop"""
    rng = np.random.default_rng(34)
    fake = header() + atom_row(rng, 1, "CA", 1) + "\n"
    opening = "_struct.title\n;begins\n" + fake
    text = pad_to("data_x\n", CHUNK - 50 - len(opening)) + opening + "x" * (CHUNK + 100) + "\n" + fake + ";\n#\n"
    text += header() + rows_text(rng, 3) + "#\n"
    raw = text.encode()
    assert b"\n" not in raw[CHUNK:2 * CHUNK] and raw[:CHUNK].count(b"\n;") == 1 and raw[2 * CHUNK:].count(b"\n;") == 1
    assert assert_reads_like_the_reference([raw]).num_residues == 3
    # the same text without the closing line: everything behind the opening line is inside the field
    assert assert_reads_like_the_reference([raw.replace(b"\n;\n#", b"\n#")]).num_residues == 0


def test_header_in_chunk_0_and_first_row_in_chunk_2(dev):
    """blank lines may stand between the tag lines and the rows, comment lines may not: they end the loop"""
    rng = np.random.default_rng(35)
    text = pad_to("data_x\n" + header(), 2 * CHUNK + 7, line=blank) + rows_text(rng, 3) + "#\n"
    assert text[2 * CHUNK + 7:].startswith("ATOM") and "ATOM" not in text[:2 * CHUNK + 7] and text.index("pdbx_PDB_model_num") < CHUNK
    assert assert_reads_like_the_reference([text.encode()]).num_residues == 3
    ended = pad_to("data_x\n" + header(), 2 * CHUNK + 7) + rows_text(rng, 3) + "#\n"
    assert assert_reads_like_the_reference([ended.encode()]).num_residues == 0


def test_file_boundary_inside_a_chunk_with_other_columns(dev):
    """two files in one chunk whose columns stand in different orders; the first ends inside a text field that must not reach into
    the second, and its last row has no newline"""
    rng = np.random.default_rng(36)
    other = list(reversed(PDBX))
    a = "data_a\n" + header() + rows_text(rng, 3) + "#\n_struct.title\n;never closed\n"
    b = "data_b\n" + header(other) + rows_text(rng, 2, asym="B", tags=other) + rows_text(rng, 1, first=3, asym="B", tags=other)[:-1]
    assert len(a) + len(b) < CHUNK
    parsed = assert_reads_like_the_reference([a.encode(), b.encode()])
    assert parsed.chain_file.tolist() == [0, 1] and parsed.chain_names() == ["A", "B"] and parsed.num_residues == 6
    assert_reads_like_the_reference([b.encode(), a.encode(), b"", b.encode()])


def test_longest_row(dev):
    """a row of FD_CIF_MAX_LINE bytes is read, one of a byte more is refused; CRLF does not count"""
    rng = np.random.default_rng(37)
    text = lambda wide, nl="\n": ("data_x\n" + header() + rows_text(rng, 1) + atom_row(rng, 9, "N", 2, wide=wide) + "\n" + rows_text(rng, 1, first=3)).replace("\n", nl)
    assert max(len(line) for line in text(MAX_LINE).split("\n")) == MAX_LINE
    assert assert_reads_like_the_reference([text(MAX_LINE).encode()]).num_residues == 3
    assert assert_reads_like_the_reference([text(MAX_LINE, "\r\n").encode()]).num_residues == 3
    with pytest.raises(ValueError, match=f"more than 1024 bytes in file 0 .*, line {2 + len(PDBX) + 3 + 1}$"):
        pdb.parse_mmcif(text(MAX_LINE + 1).encode())
    assert assert_reads_like_the_reference([text(MAX_LINE + 1).encode()]) is None


# ---- 4. refusals -------------------------------------------------------------------------------------------------------------------
def retoken(row, *changes):
    """a row of atom_row() with the token of a tag replaced, for each (tag, token) of changes"""
    toks = row.split(" ")
    for tag, tok in zip(changes[::2], changes[1::2]):
        toks[PDBX.index(tag)] = tok
    return " ".join(toks)


def _refusals():
    rng = np.random.default_rng(38)
    good = rows_text(rng, 3).split("\n")[:-1]

    def edit(k, *changes):
        return "data_x\n#\n" + header() + "\n".join(good[:k] + [retoken(good[k], *changes)] + good[k + 1:]) + "\n#\n", 3 + len(PDBX) + k + 1

    without = lambda tag: ("data_x\n#\n" + header([t for t in PDBX if t != tag]) + "1 2 3\n#\n", 3)
    return {
        "columns_no_x": without("Cartn_x") + (COLUMNS,),
        "columns_no_alt": without("label_alt_id") + (COLUMNS,),
        "columns_65": ("data_x\n#\n" + header(PDBX + [f"more_{k}" for k in range(MAX_COLS + 1 - len(PDBX))]) + "1 2 3\n#\n", 3, COLUMNS),
        "columns_second_loop": ("data_x\n#\n" + header() + "\n".join(good) + "\n#\n" + header() + "\n".join(good) + "\n#\n", 3 + len(PDBX) + 9 + 2, COLUMNS),
        "tokens_few": ("data_x\n#\n" + header() + good[0] + "\n" + good[1].rsplit(" ", 1)[0] + "\n", 3 + len(PDBX) + 2, TOKENS),
        "tokens_many": ("data_x\n#\n" + header() + good[0] + " extra\n", 3 + len(PDBX) + 1, TOKENS),
        "tokens_quote": edit(4, "auth_atom_id", "'CA") + (TOKENS,),
        "coord_exponent": edit(7, "Cartn_y", "1.2e+1") + (COORD,),
        "coord_missing": edit(2, "Cartn_z", "?") + (COORD,),
        "coord_two_signs": edit(2, "Cartn_x", "--1.25") + (COORD,),
        "coord_16_digits": edit(2, "Cartn_x", "1.234567890123456") + (COORD,),
        "number_b": edit(5, "B_iso_or_equiv", "n/a") + (NUMBER,),
        "number_occupancy": edit(5, "occupancy", "1.0.0") + (NUMBER,),
        "resseq": edit(3, "auth_seq_id", "1.5") + (RESSEQ,),
        "resseq_missing": edit(3, "auth_seq_id", ".") + (RESSEQ,),
        "chain": edit(6, "auth_asym_id", "ABCDE") + (CHAIN,),
        "model": edit(8, "pdbx_PDB_model_num", "one") + (MODEL,),
        "smallest_kind": edit(1, "pdbx_PDB_model_num", "y", "auth_asym_id", "ABCDE", "auth_seq_id", "x") + (RESSEQ,),
    }


REFUSALS = _refusals()


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_malformed_input_is_refused(dev, name):
    text, line, kind = REFUSALS[name]
    other = ("data_o\n" + header() + rows_text(np.random.default_rng(39), 2)).encode()
    with pytest.raises(Refused) as e:
        reference_read_cif([other, b"", text.encode()])
    assert (e.value.file, e.value.line, e.value.kind) == (2, line, kind)
    with pytest.raises(ValueError, match=re.escape(pdb.CIF_KINDS[kind]) + f" in file 2 .*, line {line}$"):
        pdb.parse_mmcif([other, b"", text.encode()])
    with pytest.raises(ValueError, match=f"in file 0 .*, line {line}$"):
        pdb.parse_mmcif(torch.from_numpy(np.frombuffer(text.encode(), np.uint8).copy()).to(dev))


def test_smallest_line_of_two_offenders_and_what_is_not_refused(dev):
    rng = np.random.default_rng(40)
    other = ("data_o\n" + header() + rows_text(rng, 2)).encode()
    late, early = REFUSALS["model"], REFUSALS["coord_missing"]
    with pytest.raises(ValueError, match=f"empty or not a plain decimal.* in file 1 .*, line {early[1]}$"):
        pdb.parse_mmcif([other, early[0].encode(), late[0].encode()])
    with pytest.raises(ValueError, match=f"model number.* in file 0 .*, line {late[1]}$"):
        pdb.parse_mmcif([late[0].encode(), other, early[0].encode()])
    assert_reads_like_the_reference([late[0].encode(), other, early[0].encode()])
    # a malformed HETATM row while HETATM rows are not read; a malformed row of a model that is not read; a value line that
    # is no row
    bad_het = "HETATM 9 O O . HOH A 1 . ? what 2.000"
    second = retoken(atom_row(rng, 7, "CA", 9, model=2), "auth_seq_id", "9x")
    text = ("data_x\n1 2 3 stray values\n" + header() + rows_text(rng, 2) + bad_het + "\n" + second + "\n#\nstray again\n").encode()
    assert assert_reads_like_the_reference([text]).num_residues == 2
    for kw in (dict(hetatm=True), dict(model="all")):
        assert assert_reads_like_the_reference([text], **kw) is None
    with pytest.raises(ValueError, match="model="):
        pdb.parse_mmcif(b"", model="last")
    with pytest.raises(ValueError, match="ids="):
        pdb.parse_mmcif(b"", ids="both")


# ---- 5. properties -----------------------------------------------------------------------------------------------------------------
def test_empty_inputs(dev):
    for files in (b"", [b""], [b"", b"", b""], [b"data_x\n#\n", b""]):
        none = pdb.parse_mmcif(files)
        F = len(files) if isinstance(files, list) else 1
        assert none.num_residues == 0 and len(none) == 0 and none.n_dropped.tolist() == [0] * F and none.chain_offsets.tolist() == [0]
        assert tuple(none.atom_positions.shape) == (0, 37, 3) and tuple(none.ca_padded()[0].shape) == (0, 0, 3) and none.chain_names() == []


def test_fill_writes_only_what_records_fill(dev):
    """the six entry points called as parse_mmcif calls them, the outputs filled with a sentinel first and sized for a row and a
    segment more than there are: entries no record fills, rows >= T and segments >= C keep the sentinel"""
    lib = hip.get_lib()
    files = files_of("chains")
    want = reference_read_cif(files)
    raw = np.frombuffer(b"".join(files), np.uint8).copy()
    text = torch.from_numpy(raw).to(dev)
    n, F, nchunks = len(raw), len(files), -(-len(raw) // CHUNK)
    off = torch.tensor([0, n], dtype=torch.int64, device=dev)
    i64 = dict(dtype=torch.int64, device=dev)
    before = lambda v: torch.cat([torch.full_like(v[:, :1], -1), torch.cummax(v, 1).values[:, :-1]], 1)
    carry, lines, marks = torch.full((8, nchunks), -1, **i64), torch.empty((3, nchunks), **i64), torch.empty((4, nchunks), **i64)
    lib.call("fd_cif_read_lines", text, n, off, F, lines)
    carry[:2] = torch.cumsum(lines[:2], 1) - lines[:2]
    carry[2:3] = before(torch.where(lines[2:3] >= 0, carry[1:2] + lines[2:3], lines[2:3]))
    lib.call("fd_cif_read_marks", text, n, off, F, carry, marks)
    carry[3:7] = before(marks)
    table, first, bad = torch.zeros((F, 66), dtype=torch.int32, device=dev), torch.zeros(F, **i64), torch.empty(nchunks, **i64)
    lib.call("fd_cif_read_header", text, n, off, F, 0, 0, carry, table, first, bad)
    last, counts = torch.empty((1, nchunks), **i64), torch.empty((3, nchunks), **i64)
    lib.call("fd_cif_read_summary", text, n, off, F, 0, carry, table, last)
    carry[7:8] = before(last)
    lib.call("fd_cif_read_count", text, n, off, F, 0, 0, carry, table, counts)
    ends = torch.cumsum(counts[:2], 1)
    T, C = int(ends[0, -1]), int(ends[1, -1])
    assert (T, C) == (len(want["aatype"]), len(want["chain_id"])) and int(counts[2].min()) == pdb.STATUS_OK == int(bad.min())
    assert lines[0].sum().item() == b"".join(files).count(b"\n") and first.tolist() == [0]
    tags = [t.split(b".")[1].lower() for t in files[0].split(b"\n") if t.startswith(b"_atom_site.")]
    fields = [b"group_pdb", b"label_atom_id", b"label_alt_id", b"label_comp_id", b"auth_asym_id", b"auth_seq_id", b"pdbx_pdb_ins_code", b"cartn_x",
              b"cartn_y", b"cartn_z", b"occupancy", b"b_iso_or_equiv", b"pdbx_pdb_model_num"]
    assert table[0].tolist() == [fields.index(t) if t in fields else -1 for t in tags] + [-1] * (64 - len(tags)) + [len(tags), 1]
    bases = (ends - counts[:2]).contiguous()
    S = 77
    out = [torch.full((T + 1, 37, 3), float(S), device=dev), torch.full((T + 1, 37), S, dtype=torch.uint8, device=dev),
           torch.full((T + 1, 37), float(S), device=dev), torch.full((T + 1,), S, **i64), torch.full((T + 1,), S, **i64),
           torch.full((T + 1,), S, dtype=torch.int32, device=dev), torch.full((C + 1,), S, **i64)] + \
        [torch.full((C + 1,), S, dtype=torch.int32, device=dev) for _ in range(3)]
    lib.call("fd_cif_read_fill", text, n, off, F, 0, 0, carry, table, bases, T, C, *out)
    filled = want["atom_mask"].astype(bool)
    assert np.array_equal(out[1][:T].cpu().numpy(), np.where(filled, 1, S)) and out[1][T].tolist() == [S] * 37
    assert np.array_equal(out[0][:T].cpu().numpy(), np.where(filled[..., None], want["atom_positions"], np.float32(S)))
    assert np.array_equal(out[2][:T].cpu().numpy(), np.where(filled, want["b_factors"], np.float32(S)))
    assert bool((out[0][T] == S).all()) and bool((out[2][T] == S).all())
    for got, ref in zip(out[3:], (want["aatype"], want["residue_index"], None, want["chain_offsets"][:-1], want["chain_file"],
                                  want["chain_model"], want["chain_id"])):
        assert got[-1].item() == S and (ref is None or got[:-1].tolist() == ref.tolist())
    assert int(out[5][:T].sum()) == want["n_dropped"][0]


# ---- 6. what takes a ParsedPdb -----------------------------------------------------------------------------------------------------
def test_consumers_take_the_result(dev):
    """a text of chains AA and B in two models: the chain store builds the batch it builds from parse_pdb of the PDB form (chains A
    and B); ca_padded, models, select by a chain ID of two characters, chain_names"""
    rng = np.random.default_rng(41)
    cif = "data_x\n" + header()
    for m in (1, 2):
        cif += rows_text(rng, 7, model=m, asym="AA") + rows_text(rng, 5, first=20, serial=50, model=m, asym="B")
    cif = (cif + "#\n").encode()
    parsed = pdb.parse_mmcif(cif, model="all")
    assert_same(parsed, reference_read_cif([cif], model="all"))
    assert parsed.chain_names() == ["AA", "B", "AA", "B"] and parsed.chain_model.tolist() == [0, 0, 1, 1]
    aa = parsed.select(chain_id="AA")
    assert aa.chain_names() == ["AA", "AA"] and aa.num_residues == 14 and len(parsed.select(chain_id="A")) == 0
    assert torch.equal(aa.models(), torch.stack([parsed.chain(0).atom_positions, parsed.chain(2).atom_positions]))
    assert len(parsed.select(model=1, chain_id="B")) == 1
    with pytest.raises(ValueError, match="1 to 4 characters"):
        parsed.select(chain_id="ABCDE")
    ca, mask = parsed.ca_padded()
    assert tuple(ca.shape) == (4, 7, 3) and mask.sum(1).tolist() == [7, 5, 7, 5]
    assert torch.equal(ca[1, :5], parsed.chain(1).atom_positions[:, 1]) and not ca[1, 5:].any()
    # the same structure as PDB text: chain AA becomes A
    from_pdb, from_cif = ChainStore(dev), ChainStore(dev)
    lines = []
    for m in (0, 1):
        for c, name in ((2 * m, "A"), (2 * m + 1, "B")):
            one = parsed.chain(c)
            for r in range(one.num_residues):
                for s in (0, 1, 2):
                    x = one.atom_positions[r, s].tolist()
                    lines.append(f"ATOM  {len(lines) % 99999:>5}  {ATOMS[s]:<3} {RES3[int(one.aatype[r])]} {name}{int(one.residue_index[r]):>4}    "
                                 f"{x[0]:8.3f}{x[1]:8.3f}{x[2]:8.3f}  1.00  0.00")
        lines.append("ENDMDL")
    as_pdb = pdb.parse_pdb(("\n".join(lines) + "\n").encode(), model="all")
    assert torch.equal(as_pdb.atom_positions, parsed.atom_positions) and as_pdb.chain_id.tolist() == [65, 66, 65, 66]
    assert from_pdb.add_parsed(as_pdb) == from_cif.add_parsed(parsed) == [0, 1, 2, 3]
    from_pdb.freeze(), from_cif.freeze()
    a, b = from_pdb.build_batch([0, 1, 2, 3]), from_cif.build_batch([0, 1, 2, 3])
    assert sorted(a) == sorted(b) and all(torch.equal(a[k], b[k]) for k in a)


# ---- 7. a library, on the device only ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_library_of_200_files_gpu(hip_lib):
    """200 chains of N = 128 written by format_pdb (about 50 chunks each as mmCIF) and converted: parse_mmcif of the 200 mmCIF texts
    equals parse_pdb of the 200 PDB texts"""
    rng = np.random.default_rng(42)
    x = np.zeros((200, 128, 37, 3), np.float32)
    x[:, :, :5] = rng.normal(size=(200, 128, 5, 3)) * 15.0
    aa = torch.from_numpy(rng.integers(0, 20, size=128))
    texts = [pdb.format_pdb(torch.from_numpy(x[k]).cuda(), aatype=aa).cpu().numpy().tobytes() for k in range(200)]
    want = pdb.parse_pdb(texts)
    assert want.num_residues == 200 * 128 and len(want) == 200
    got = pdb.parse_mmcif([pdb_to_cif(t) for t in texts])
    assert_same(got, want)
    assert tuple(got.ca_padded()[0].shape) == (200, 128, 3)
