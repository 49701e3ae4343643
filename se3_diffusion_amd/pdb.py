"""PDB text of samples and trajectories, formatted on the device (csrc/fd_pdb.hip; include/fd_hip.h is the specification).

The files are byte for byte what the reference's analysis.utils.write_prot_to_pdb writes for the same float32 arrays
(data/protein.py to_pdb per frame): MODEL / ATOM / TER / ENDMDL records of 80 columns, "END" without a newline.  An atom is
present iff (|x| + |y|) + |z| > 1e-7 in float32; residues are numbered from 0, the chain is A, the occupancy 1.00.

    text = pdb.format_pdb(out["prot_traj"][:, b])             # uint8 device tensor, the whole file
    pdb.write_pdb("bb_traj.pdb", out["prot_traj"][:, b])      # one copy to the host, one write
    pdb.save_traj(out, b, output_dir)                         # the reference's sample_1 / bb_traj_1 / x0_traj_1.pdb

Input the 80 columns cannot hold (a NaN, a coordinate outside -999.999 .. 9999.999, a b-factor outside -99.99 .. 999.99, more
than 99999 atoms or 10000 residues in a model, an aatype outside 0 .. 20) raises ValueError before any file is opened; the
reference prints over-wide lines there.

Inputs are taken as float32: a float64 array is ROUNDED to float32 first, so a float64 coordinate within half a float32 ulp of a
%.3f tie may print one unit in the last place away from the reference's line for the float64 value.  The sampler's arrays are
float32.

Reading is the inverse (csrc/fd_pdb_read.hip): any number of files in one buffer, lines found, records classified by their
columns, residues numbered by an ordered scan and atoms placed, on the device.

    parsed = pdb.parse_pdb(paths_or_bytes_or_device_text)      # ParsedPdb: atom37 arrays packed over all chain segments
    pos, mask = parsed.ca_padded()                             # what metrics.novelty / tm_align_matrix / aligned_rmsd take
    frames = pdb.parse_pdb("bb_traj_1.pdb", model="all").models()
    feats = pdb.parse_pdb_feats(name, path)                    # the reference's du.parse_pdb_feats, the same dict

    parsed = pdb.parse_mmcif(paths_or_bytes_or_device_text)    # the same object from the _atom_site loop of mmCIF files

Reading back what format_pdb wrote gives float32(rint(x 1000) / 1000).  Not read: SEQRES and the other header records; of
alternate locations the first is kept, not the one of the highest occupancy (parse_pdb's note).  mmCIF is read by parse_mmcif
(csrc/fd_cif_read.hip): the _atom_site loop under the same rules, nothing else of the file.  Both readers take gzip files
(NNNN.cif.gz, pdbNNNN.ent.gz): inflate() (csrc/fd_inflate.hip) inflates one member per file on the device, a wave per file.
"""
from __future__ import annotations

import os
import re

import numpy as np
import torch

from . import hip

LINE = 81                                   # 80 columns and the newline
MAX_N = 10000                               # FD_PDB_MAX_N
STATUS_OK = 0x7FFFFFFFFFFFFFFF              # FD_PDB_STATUS_OK
KINDS = {1: "a coordinate that is NaN or infinite",
         2: "a coordinate outside -999.999 .. 9999.999 (8 columns)",
         3: "a b-factor that is not finite or outside -99.99 .. 999.99 (6 columns)",
         4: "a serial above 99999",
         5: f"a residue number above {MAX_N - 1} (N > {MAX_N})",
         6: "an aatype outside 0 .. 20"}


def _device_of(x, lib):
    if isinstance(x, torch.Tensor) and (x.is_cuda or not lib.is_device):
        return x.device
    return torch.device("cuda", torch.cuda.current_device()) if lib.is_device else torch.device("cpu")


def _atoms(atom37, dev):
    """float32 [M,N,37,3] on dev whose models are contiguous [N,37,3] blocks a fixed number of floats apart; a strided view over
    models (x[:, b] of [T,B,N,37,3]) is kept as it is."""
    a = atom37 if isinstance(atom37, torch.Tensor) else torch.from_numpy(np.asarray(atom37))
    if a.dim() == 3:
        a = a[None]
    if a.dim() != 4 or a.shape[-2:] != (37, 3):
        raise ValueError(f"Invalid positions shape {tuple(atom37.shape)}: expected [N,37,3] or [M,N,37,3]")
    a = a.to(device=dev, dtype=torch.float32)
    if a.stride()[1:] != (111, 3, 1) or (a.shape[0] > 1 and a.stride(0) < 0):
        a = a.contiguous()
    return a


def format_pdb(atom37, aatype=None, b_factors=None, first_model=1):
    """The text of the PDB file of atom37 ([N,37,3]: one model; [M,N,37,3]: models first_model, first_model + 1, ..) as a uint8
    tensor on the device.  atom37: device tensor or numpy, taken as float32 (see the module's note on float64); over models it may
    be strided.  aatype [N] integers 0 .. 20 (None: ALA), b_factors [N] or [N,37] (None: 0).  Two launches, a cumsum, and one
    read-back (the file's size and the status word)."""
    lib = hip.get_lib()
    dev = _device_of(atom37, lib)
    a = _atoms(atom37, dev)
    M, N = int(a.shape[0]), int(a.shape[1])
    if N < 1:
        raise ValueError("a model needs at least one residue")
    if first_model < 0:
        raise ValueError(f"first_model={first_model}: must not be negative")
    aa = bf = None
    if aatype is not None:
        aa = torch.as_tensor(np.asarray(aatype) if not isinstance(aatype, torch.Tensor) else aatype)
        if aa.shape != (N,):
            raise ValueError(f"aatype has shape {tuple(aa.shape)}, expected ({N},)")
        aa = aa.to(device=dev, dtype=torch.int32).contiguous()
    if b_factors is not None:
        bf = torch.as_tensor(np.asarray(b_factors) if not isinstance(b_factors, torch.Tensor) else b_factors)
        if bf.shape == (N,):
            bf = bf[:, None].expand(N, 37)
        if bf.shape != (N, 37):
            raise ValueError(f"b_factors has shape {tuple(bf.shape)}, expected ({N},) or ({N}, 37)")
        bf = bf.to(device=dev, dtype=torch.float32).contiguous()
    if M == 0:
        return torch.tensor(list(b"END"), dtype=torch.uint8, device=dev)
    stride = a.stride(0) if M > 1 else N * 111
    counts = torch.empty(M, dtype=torch.int64, device=dev)
    status = torch.empty(M, dtype=torch.int64, device=dev)
    lib.call("fd_pdb_count", a, stride, aa, bf, M, N, counts, status)
    ends = torch.cumsum(counts + 3, 0)
    lines, word = (int(v) for v in torch.stack([ends[-1], status.min()]).cpu())
    if word != STATUS_OK:
        idx, kind = divmod(word, 8)
        m, rest = divmod(idx, N * 37)
        r, s = divmod(rest, 37)
        raise ValueError(f"cannot be written as PDB text: {KINDS.get(kind, kind)} at model {m}, residue {r}, atom slot {s} "
                         f"(linear index {idx})")
    offsets = ends - (counts + 3)
    out = torch.empty(lines * LINE + 3, dtype=torch.uint8, device=dev)
    lib.call("fd_pdb_format", a, stride, aa, bf, offsets, M, N, int(first_model), out, out.numel())
    return out


def write_pdb(path, atom37, aatype=None, b_factors=None, first_model=1):
    """format_pdb's text, copied to the host once and written to path.  Nothing is opened if the input is refused."""
    return _write(format_pdb(atom37, aatype=aatype, b_factors=b_factors, first_model=first_model), path)


def _write(text, path):
    host = text.cpu().numpy()
    with open(path, "wb") as f:
        f.write(memoryview(host))
    return path


def indexed_path(file_path, overwrite=False, no_indexing=False):
    """The reference's naming rule.  no_indexing: the path itself.  Otherwise the path without every '.pdb' in it, then
    '_{k+1}.pdb', k = 0 with overwrite, else the highest index '_(digits)' + any character + 'pdb' found in the names of the
    path's directory that CONTAIN the key -- the base name with leading and trailing characters of the set {'.', 'p', 'd', 'b'}
    removed (the reference strips a character set, not a suffix: 'bb_traj' becomes '_traj', 'pdb' the empty key that every name
    contains)."""
    k = 0
    if not overwrite:
        key = os.path.basename(file_path).strip(".pdb")        # (a character set, see above)
        for name in os.listdir(os.path.dirname(file_path)):           # (an empty directory part raises, as the reference does)
            if key in name:
                found = re.findall(r"_(\d+).pdb", name)
                if found:
                    k = max(k, int(found[0]))
    if no_indexing:
        return file_path
    return file_path.replace(".pdb", "") + f"_{k + 1}.pdb"


def write_prot_to_pdb(prot_pos, file_path, aatype=None, overwrite=False, no_indexing=False, b_factors=None):
    """analysis.utils.write_prot_to_pdb with the text formatted on the device: the same signature, file name and return value
    (the path written).  prot_pos [N,37,3] or [T,N,37,3], numpy or tensor."""
    if prot_pos.ndim not in (3, 4):
        raise ValueError(f"Invalid positions shape {prot_pos.shape}")
    text = format_pdb(prot_pos, aatype=aatype, b_factors=b_factors)      # (refused input raises before the directory is read)
    return _write(text, indexed_path(file_path, overwrite=overwrite, no_indexing=no_indexing))


def save_traj(out, b, output_dir, diffuse_mask=None):
    """The three files the reference's Sampler.save_traj writes for backbone b of a sampler.sample(record="reference") result,
    straight from the recorded device tensors: sample (frame 0 of prot_traj), bb_traj (prot_traj) and x0_traj (rigid_0_traj), each
    under the reference's indexed name.  B-factors are 100 where diffuse_mask [N] is set (None: everywhere), 0 elsewhere.
    Returns {'sample_path', 'traj_path', 'x0_traj_path'}."""
    for k in ("prot_traj", "rigid_0_traj"):
        if k not in out:
            raise KeyError(f"save_traj needs {k}: call sampler.sample(record='reference')")
    prot, x0 = out["prot_traj"][:, b], out["rigid_0_traj"][:, b]
    N = prot.shape[1]
    if diffuse_mask is None:
        mask = torch.ones(N, dtype=torch.bool)
    else:
        mask = torch.as_tensor(np.asarray(diffuse_mask) if not isinstance(diffuse_mask, torch.Tensor) else diffuse_mask) != 0
    b_factors = mask.to(device=prot.device, dtype=torch.float32) * 100.0
    return {
        "sample_path": write_prot_to_pdb(prot[0], os.path.join(output_dir, "sample"), b_factors=b_factors),
        "traj_path": write_prot_to_pdb(prot, os.path.join(output_dir, "bb_traj"), b_factors=b_factors),
        "x0_traj_path": write_prot_to_pdb(x0, os.path.join(output_dir, "x0_traj"), b_factors=b_factors),
    }


# ---- reading ---------------------------------------------------------------------------------------------------------------------
READ_CHUNK = 4096                           # FD_PDB_READ_CHUNK
READ_KINDS = {1: "a coordinate record shorter than 54 columns",
              2: "a coordinate field that is empty or not a plain decimal number",
              3: "an occupancy or b-factor field that is not a plain decimal number",
              4: "a residue number that is not an integer"}
_CA = 1                                     # atom37 slot of CA


class ParsedPdb:
    """What parse_pdb read, packed over all chain segments, on the device: atom_positions [T,37,3] fp32, atom_mask [T,37] uint8,
    aatype [T] int64 (20: not one of the twenty), residue_index [T] int64 (resSeq as written), b_factors [T,37] fp32;
    chain_offsets [C+1] int64 (segment c is rows chain_offsets[c] .. chain_offsets[c+1]), chain_file, chain_model (from 0, the
    ENDMDL records in front of the segment in its file) and chain_id (a character code; from parse_mmcif up to four of them, the
    first lowest: chain_names()) [C] int32; n_dropped [F] int64, the
    records per input file that lost their slot to an earlier one; n_files = F."""

    def __init__(self, atom_positions, atom_mask, aatype, residue_index, b_factors, chain_offsets, chain_file, chain_model, chain_id,
                 n_dropped, n_files):
        self.atom_positions, self.atom_mask, self.aatype, self.residue_index, self.b_factors = \
            atom_positions, atom_mask, aatype, residue_index, b_factors
        self.chain_offsets, self.chain_file, self.chain_model, self.chain_id = chain_offsets, chain_file, chain_model, chain_id
        self.n_dropped, self.n_files = n_dropped, n_files
        self.n_lines = 0                        # lines of the whole input (set by parse_pdb)
        self._host = None

    def __len__(self):
        return int(self.chain_file.numel())

    @property
    def num_residues(self):
        return int(self.aatype.numel())

    def host_tables(self):
        """(chain_offsets, chain_file, chain_model, chain_id) as numpy; copied from the device on first use, then kept"""
        if self._host is None:
            self._host = tuple(t.cpu().numpy() for t in (self.chain_offsets, self.chain_file, self.chain_model, self.chain_id))
        return self._host

    def _rows(self, rows, chains):
        """the segments `chains` (host indices), whose rows are `rows`: a slice (views) or an index tensor (copies)"""
        off, cf, cm, ci = self.host_tables()
        new_off = np.concatenate([[0], np.cumsum(off[chains + 1] - off[chains])]).astype(np.int64)
        dev = self.aatype.device
        pick = lambda t: t[rows]
        idx = torch.from_numpy(chains).to(dev)
        out = ParsedPdb(pick(self.atom_positions), pick(self.atom_mask), pick(self.aatype), pick(self.residue_index),
                        pick(self.b_factors), torch.from_numpy(new_off).to(dev), self.chain_file[idx], self.chain_model[idx],
                        self.chain_id[idx], self.n_dropped, self.n_files)
        out._host = (new_off, cf[chains], cm[chains], ci[chains])
        return out

    def chain(self, i):
        """Segment i alone: its rows as views of this object's tensors."""
        off = self.host_tables()[0]
        if not -len(self) <= i < len(self):
            raise IndexError(f"chain {i} of {len(self)}")
        i %= len(self)
        return self._rows(slice(int(off[i]), int(off[i + 1])), np.array([i], np.int64))

    def select(self, file=None, model=None, chain_id=None):
        """The segments of input file `file`, model `model` (from 0) and chain `chain_id` (a string of 1 to 4 characters), None
        meaning any, in the order of the text.  Views of this object's tensors when the chosen segments follow one another, copies otherwise."""
        off, cf, cm, ci = self.host_tables()
        keep = np.ones(len(cf), bool)
        if file is not None:
            keep &= cf == file
        if model is not None:
            keep &= cm == model
        if chain_id is not None:
            keep &= ci == _pack_chain(chain_id)
        chains = np.flatnonzero(keep).astype(np.int64)
        if len(chains) == 0:
            return self._rows(slice(0, 0), chains)
        if chains[-1] - chains[0] + 1 == len(chains):
            return self._rows(slice(int(off[chains[0]]), int(off[chains[-1] + 1])), chains)
        rows = np.concatenate([np.arange(off[c], off[c + 1]) for c in chains])
        return self._rows(torch.from_numpy(rows).to(self.aatype.device), chains)

    def chain_names(self):
        """chain_id unpacked: per segment the chain ID as a string (parse_pdb: one character)"""
        return [int(c).to_bytes(4, "little", signed=True).rstrip(b"\0").decode("latin-1") for c in self.host_tables()[3]]

    def ca_padded(self):
        """(pos [C,Lmax,3] fp32, mask [C,Lmax] fp32): the CA atoms of every segment, padded to the longest, mask 1 where a CA was
        read -- the operands of metrics.novelty, tm_align_matrix and aligned_rmsd."""
        off = self.host_tables()[0]
        C, T = len(self), self.num_residues
        dev = self.aatype.device
        lens = off[1:] - off[:-1]
        Lmax = int(lens.max()) if C else 0
        pos = torch.zeros((C, Lmax, 3), dtype=torch.float32, device=dev)
        mask = torch.zeros((C, Lmax), dtype=torch.float32, device=dev)
        if T:
            starts = self.chain_offsets[:-1]
            seg = torch.repeat_interleave(torch.arange(C, device=dev), self.chain_offsets[1:] - starts, output_size=T)
            at = torch.arange(T, device=dev) - starts[seg]
            pos[seg, at] = self.atom_positions[:, _CA]
            mask[seg, at] = self.atom_mask[:, _CA].to(torch.float32)
        return pos, mask

    def models(self):
        """atom_positions as [M,L,37,3] when this object holds one input file whose M models each are one segment with the same
        residues (aatype and residue_index); ValueError otherwise.  Reads bb_traj / x0_traj files back."""
        off, cf, cm, _ = self.host_tables()
        M = len(cf)
        if M == 0 or len(set(cf.tolist())) != 1 or sorted(cm.tolist()) != sorted(set(cm.tolist())):
            raise ValueError("models() needs the segments of one file, one per model")
        lens = off[1:] - off[:-1]
        if len(set(lens.tolist())) != 1:
            raise ValueError(f"the models differ in their number of residues: {sorted(set(lens.tolist()))}")
        L = int(lens[0])
        aa, ri = self.aatype.reshape(M, L), self.residue_index.reshape(M, L)
        if not bool(((aa == aa[:1]).all() & (ri == ri[:1]).all()).item()):
            raise ValueError("the models differ in their residues")
        return self.atom_positions.reshape(M, L, 37, 3)


def _pack_chain(chain_id):
    """a chain ID of 1 to 4 characters as chain_id holds it: the first character lowest"""
    raw = chain_id.encode("latin-1")
    if not 1 <= len(raw) <= 4:
        raise ValueError(f"chain_id={chain_id!r}: expected 1 to 4 characters")
    return int.from_bytes(raw.ljust(4, b"\0"), "little", signed=True)


def _pieces(inputs):
    """(the entries as uint8 tensors and numpy arrays, their names)"""
    items = inputs if isinstance(inputs, (list, tuple)) else [inputs]
    pieces, names = [], []
    for k, it in enumerate(items):
        if isinstance(it, torch.Tensor):
            if it.dtype != torch.uint8 or it.dim() != 1:
                raise ValueError(f"input {k}: a tensor must be uint8 [n], got {it.dtype} {tuple(it.shape)}")
            pieces.append(it)
            names.append(f"input {k}")
        elif isinstance(it, (bytes, bytearray, memoryview)):
            pieces.append(np.frombuffer(it, np.uint8))
            names.append(f"input {k}")
        elif isinstance(it, (str, os.PathLike)):
            pieces.append(np.fromfile(os.fspath(it), np.uint8))
            names.append(os.fspath(it))
        else:
            raise TypeError(f"input {k}: expected bytes, a uint8 tensor or a path, got {type(it).__name__}")
    return pieces, names


def _gather_text(inputs, lib):
    """(text uint8 on the device, 16-byte aligned; host int64 offsets [F+1]; names): host pieces are joined and uploaded in one copy"""
    return _join(*_pieces(inputs), lib)


def _join(pieces, names, lib):
    """_gather_text's result for _pieces' entries"""
    offsets = np.concatenate([[0], np.cumsum([int(p.shape[0]) for p in pieces])]).astype(np.int64)
    on_dev = [p for p in pieces if isinstance(p, torch.Tensor) and (p.is_cuda or not lib.is_device)]
    dev = on_dev[0].device if on_dev else _device_of(None, lib)
    if len(pieces) == 1 and isinstance(pieces[0], torch.Tensor):
        text = pieces[0].to(dev).contiguous()
    elif not any(isinstance(p, torch.Tensor) for p in pieces):
        text = torch.from_numpy(np.concatenate(pieces) if pieces else np.zeros(0, np.uint8)).to(dev)
    else:
        # host pieces go up in one copy, then everything is put in order on the device
        host = [p for p in pieces if not isinstance(p, torch.Tensor)]
        up = torch.from_numpy(np.concatenate(host)).to(dev) if host else None
        parts, at = [], 0
        for p in pieces:
            if isinstance(p, torch.Tensor):
                parts.append(p.to(dev))
            else:
                parts.append(up[at:at + p.shape[0]])
                at += p.shape[0]
        text = torch.cat(parts)
    if text.data_ptr() % 16:
        text = text.clone()
    return text, offsets, names


INFLATE_KINDS = {1: "not a gzip header (magic bytes 1f 8b, CM = 8, no reserved flag)",
                 2: "the file ends before the gzip member is complete",
                 3: "block type 3, or a stored block whose LEN is not ~NLEN",
                 4: "a code-length set that is over-subscribed or incomplete",
                 5: "an invalid symbol, or a distance that reaches in front of the file's first byte",
                 6: "more or fewer bytes than ISIZE says",
                 7: "a CRC32 that is not the trailer's",
                 8: "bytes behind the trailer (several members and BGZF are not read)"}     # FD_INFLATE_*
_GZIP_MIN = 18                              # a header of 10 bytes and a trailer of 8


def inflate(inputs, gzip="auto", verify=True, max_inflated=1 << 30):
    """The texts of the input files laid end to end on the device, gzip members inflated there (csrc/fd_inflate.hip; include/fd_hip.h
    is the specification).  inputs: what parse_pdb takes -- bytes, a uint8 tensor, a path, or a list of these, each entry one
    file.  Returns (text, offsets, names): text uint8 on the device, 16-byte aligned; offsets a host int64 [F+1] array; the names.

    gzip="auto": a host entry or a path whose first two bytes are 1f 8b is a gzip file (no PDB or mmCIF text begins with 0x1f);
    a tensor that is already on the device is taken as text.  gzip=True: every entry is a gzip file; the ISIZE words of entries
    on the device are gathered there and cost one read-back.  gzip=False: nothing is inflated.  A call in which no entry is a
    gzip file does what it did before there was this function: no launch, no read-back.

    ISIZE (the last four bytes) sizes each file's place, the output is allocated once, compressed and plain host pieces go up in
    one copy, and ONE launch (a wave per file) inflates the gzip files and copies the plain ones through.  verify: the same
    launch checks each member's CRC32.  One read-back, the status.  ValueError: an entry declared gzip of fewer than 18 bytes, an
    ISIZE above max_inflated (bytes), or a file the device refuses (INFLATE_KINDS) -- the message names the file's index and
    name, the byte position in the file and the kind; the smallest index wins.

    Read: one gzip member per file (RFC 1952: FEXTRA, FNAME, FCOMMENT and FHCRC skipped, the header CRC not checked) around a
    DEFLATE stream (RFC 1951) of stored, fixed and dynamic blocks.  Not read, and refused by name, not silently cut: several
    members in one file and BGZF.  Not read at all: the zlib and raw-deflate wrappers, other compressors.  A file is inflated by
    one wave, so a single large file goes at one wave's rate, about 5 MB/s of text: 2,000 N=256 files take 26 ms, one 25 MB file
    5 s (profiles/inflate_cost.txt).  Inflate a handful of files or one large file on the host."""
    if not (gzip == "auto" or gzip is True or gzip is False):
        raise ValueError(f"gzip={gzip!r}: expected 'auto', True or False")
    lib = hip.get_lib()
    pieces, names = _pieces(inputs)
    on_dev = [isinstance(p, torch.Tensor) and (p.is_cuda or not lib.is_device) for p in pieces]
    host = lambda p, sl: bytes(p[sl].numpy()) if isinstance(p, torch.Tensor) else p[sl].tobytes()
    if gzip == "auto":
        gz = [not d and p.shape[0] >= 2 and host(p, slice(0, 2)) == b"\x1f\x8b" for p, d in zip(pieces, on_dev)]
    else:
        gz = [bool(gzip)] * len(pieces)
    if not any(gz):
        return _join(pieces, names, lib)
    F = len(pieces)
    for f in range(F):
        if gz[f] and pieces[f].shape[0] < _GZIP_MIN:
            raise ValueError(f"cannot be inflated: file {f} ({names[f]}) has {int(pieces[f].shape[0])} bytes, a gzip member has at "
                             f"least {_GZIP_MIN}")
    data, in_off, _ = _join(pieces, names, lib)
    dev = data.device
    sizes = np.diff(in_off)
    for f in range(F):
        if gz[f] and not on_dev[f]:
            sizes[f] = int.from_bytes(host(pieces[f], slice(-4, None)), "little")
    far = [f for f in range(F) if gz[f] and on_dev[f]]
    if far:
        at = torch.from_numpy((in_off[np.asarray(far) + 1, None] - 4 + np.arange(4)[None]).reshape(-1)).to(dev)
        words = data[at].cpu().numpy().reshape(-1, 4).astype(np.int64)
        sizes[far] = words[:, 0] | words[:, 1] << 8 | words[:, 2] << 16 | words[:, 3] << 24
    for f in range(F):
        # (DEFLATE gives at most 1032 bytes for one, 258 for two bits: an ISIZE above that is not the stream's, the file is cut or
        # damaged, and the device says where -- in a place no larger than the stream could fill)
        most = 1032 * int(in_off[f + 1] - in_off[f])
        if gz[f] and sizes[f] > max_inflated and sizes[f] <= most:
            raise ValueError(f"cannot be inflated: file {f} ({names[f]}) gives its inflated size (ISIZE) as {int(sizes[f])} bytes, "
                             f"above max_inflated={max_inflated}")
        if gz[f]:
            sizes[f] = min(sizes[f], most, max(max_inflated, 0))
    out_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    kinds = np.zeros(F + (F & 1), np.int32)
    kinds[:F] = gz
    meta = torch.from_numpy(np.concatenate([in_off, out_off, kinds.view(np.int64)])).to(dev)      # one upload
    text = torch.empty(int(out_off[-1]), dtype=torch.uint8, device=dev)
    if text.data_ptr() % 16:
        text = torch.empty(int(out_off[-1]) + 16, dtype=torch.uint8, device=dev)
        text = text[(-text.data_ptr()) % 16:][:int(out_off[-1])]
    status = torch.empty(F, dtype=torch.int64, device=dev)
    lib.call("fd_inflate", data, int(data.numel()), meta[:F + 1], F, meta[2 * F + 2:].view(torch.int32), text, int(text.numel()),
             meta[F + 1:2 * F + 2], int(bool(verify)), status)
    words = status.cpu().numpy()
    bad = np.flatnonzero(words)
    if len(bad):
        f = int(bad[0])
        pos, kind = divmod(int(words[f]), 16)
        raise ValueError(f"cannot be inflated: {INFLATE_KINDS.get(kind, kind)} in file {f} ({names[f]}), byte {pos} (kind {kind})")
    return text, out_off, names


def _text_of(inputs, gzip, lib):
    """_gather_text's result for the readers: through inflate unless gzip=False"""
    return _gather_text(inputs, lib) if gzip is False else inflate(inputs, gzip=gzip)


def _empty_parsed(dev, F, T, C):
    """a ParsedPdb of T rows in C segments from F files for a fill kernel to write into: zeros where no record may write"""
    i64 = dict(dtype=torch.int64, device=dev)
    return ParsedPdb(
        torch.zeros((T, 37, 3), dtype=torch.float32, device=dev), torch.zeros((T, 37), dtype=torch.uint8, device=dev),
        torch.empty(T, **i64), torch.empty(T, **i64), torch.zeros((T, 37), dtype=torch.float32, device=dev), torch.zeros(C + 1, **i64),
        torch.empty(C, dtype=torch.int32, device=dev), torch.empty(C, dtype=torch.int32, device=dev),
        torch.empty(C, dtype=torch.int32, device=dev), torch.zeros(F, **i64), F)


def _close(out, dropped):
    """behind a fill kernel: the last chain offset, and the dropped records of the rows summed per file"""
    T, C, dev = out.num_residues, len(out), out.aatype.device
    out.chain_offsets[C] = T
    seg = torch.repeat_interleave(torch.arange(C, device=dev), out.chain_offsets[1:] - out.chain_offsets[:-1], output_size=T)
    out.n_dropped.index_add_(0, out.chain_file[seg].to(torch.int64), dropped.to(torch.int64))


def parse_pdb(text_or_paths, hetatm=False, model="first", gzip="auto"):
    """Read PDB files into atom37 arrays on the device (csrc/fd_pdb_read.hip; include/fd_hip.h is the specification).

    text_or_paths: bytes, a uint8 tensor already on the device (format_pdb's result), a path, or a list of these -- each entry is
    one file; host entries are joined and uploaded in one copy.  hetatm=False: HETATM records are skipped like any other
    line, so waters and ligands never become rows (the reference's process_chain turns HOH into an UNK residue).  model="first":
    only the records in front of the first ENDMDL of each file; "all": every model, each a segment of its own.

    Returns a ParsedPdb.  Three launches and a few scans; ONE read-back (the numbers of rows, segments and lines, and the status).
    A malformed coordinate record (READ_KINDS) raises ValueError naming the file, the line in that file and the kind, before
    anything is returned; the smallest line wins.  A file without a coordinate record gives no row.

    Three differences from Biopython's object model, which the reference reads through: HETATM records (above); of several records
    for one atom of a residue (alternate locations, duplicates) the FIRST is kept and the others counted in n_dropped, where
    Biopython keeps the alternate location of the highest occupancy; a chain ID that comes back after another chain begins a
    new segment, where Biopython merges the two.  SEQRES and the other header records are not read; mmCIF is parse_mmcif's.

    gzip="auto": a host entry or a path that begins with the bytes 1f 8b (NNNN.ent.gz) is inflated on the device first, in one
    launch for all files (inflate(), which also says what gzip=True and False mean and what is refused): ONE more launch and one
    more read-back of its own, the status -- it is not folded into the read-back above.  A call without a gzip entry takes the
    path it took before there was gzip=: the same launches, the same single read-back."""
    if model not in ("first", "all"):
        raise ValueError(f"model={model!r}: expected 'first' or 'all'")
    lib = hip.get_lib()
    text, offsets, names = _text_of(text_or_paths, gzip, lib)
    dev, n, F = text.device, int(text.numel()), len(offsets) - 1
    i64 = dict(dtype=torch.int64, device=dev)
    empty = lambda T, C: _empty_parsed(dev, F, T, C)
    if n == 0:
        return empty(0, 0)
    off = torch.from_numpy(offsets).to(dev)
    nchunks = -(-n // READ_CHUNK)
    het, every = int(bool(hetatm)), int(model == "all")
    summary = torch.empty((4, nchunks), **i64)
    lib.call("fd_pdb_read_summary", text, n, off, F, het, summary)
    carry = torch.empty((4, nchunks), **i64)
    carry[:2] = torch.cumsum(summary[:2], 1) - summary[:2]
    carry[2:, 0] = -1
    carry[2:, 1:] = torch.cummax(summary[2:], 1).values[:, :-1]
    counts = torch.empty((3, nchunks), **i64)
    file_first = torch.zeros((2, F), **i64)
    lib.call("fd_pdb_read_count", text, n, off, F, het, every, carry, counts, file_first)
    ends = torch.cumsum(counts[:2], 1)
    T, C, lines, word = (int(v) for v in torch.stack([ends[0, -1], ends[1, -1], summary[0].sum(), counts[2].min()]).cpu())
    if word != STATUS_OK:
        line, kind = divmod(word, 8)
        first = file_first[0].cpu().numpy()
        f = max(g for g in range(F) if offsets[g + 1] > offsets[g] and first[g] <= line)
        raise ValueError(f"cannot be read as PDB text: {READ_KINDS.get(kind, kind)} in file {f} ({names[f]}), line {line - first[f] + 1}")
    out = empty(T, C)
    out.n_lines = lines
    if T:
        bases = (ends - counts[:2]).contiguous()
        dropped = torch.empty(T, dtype=torch.int32, device=dev)
        lib.call("fd_pdb_read_fill", text, n, off, F, het, every, carry, bases, file_first, T, C, out.atom_positions, out.atom_mask,
                 out.b_factors, out.aatype, out.residue_index, dropped, out.chain_offsets, out.chain_file, out.chain_model,
                 out.chain_id)
        _close(out, dropped)
    return out


CIF_TABLE = 66                              # FD_CIF_TABLE
CIF_KINDS = {1: "a row with a wrong number of tokens, an unclosed quote or more than 1024 bytes",
             2: "a coordinate that is empty or not a plain decimal number",
             3: "an occupancy or b-factor that is not a plain decimal number",
             4: "a residue number that is not an integer",
             5: "an atom_site loop without a needed column, with more than 64 columns, or a second one in the file",
             6: "a chain ID of more than 4 characters",
             7: "a model number that is not an integer"}


def parse_mmcif(text_or_paths, hetatm=False, model="first", ids="auth", gzip="auto"):
    """Read the _atom_site loop of mmCIF files into atom37 arrays on the device (csrc/fd_cif_read.hip; include/fd_hip.h is the
    specification).  The inputs, the result and the rules for residues, segments, slots and models are parse_pdb's, with the
    pdbx_PDB_model_num column in place of ENDMDL records: model="first" keeps the rows that carry the model number of the file's
    first coordinate record, and chain_model is a segment's model number minus that one.  All entries of one call are mmCIF.

    The columns are found by their tags in any order, per file: group_PDB, label_atom_id, label_alt_id, label_comp_id,
    auth_asym_id and auth_seq_id (ids="auth"; label_asym_id and label_seq_id where those are absent, and always with
    ids="label"), pdbx_PDB_ins_code, Cartn_x / y / z, occupancy, B_iso_or_equiv, pdbx_PDB_model_num -- Biopython's choices.  A
    chain ID has 1 to 4 characters and is packed into chain_id with the first lowest, so "A" is what parse_pdb gives;
    chain_names() unpacks, select(chain_id="AA") picks.

    Six launches and a few scans; ONE read-back.  A malformed loop head or coordinate record (CIF_KINDS) raises ValueError naming
    the file, the line in that file and the kind, before anything is returned; the smallest line wins.  A file without an
    atom_site loop, or with atom_site in key-value form, gives no row.

    Not read: _entity_poly_seq and any SEQRES-like alignment; the header items the reference's metadata uses (resolution,
    method, oligomeric state); rows that span lines and text fields inside the loop; several tags on one line.  gzip files are
    inflated on the device first, as parse_pdb's are (gzip=, pdb.inflate).  parse_pdb's three differences from Biopython's object model hold here too.  The reader is checked against
    parse_pdb on the same structures and against a pure-Python tokeniser written from the header's rules (tests/test_mmcif_read.py),
    NOT against Biopython's MMCIFParser, which does not exist where this project is built."""
    if model not in ("first", "all"):
        raise ValueError(f"model={model!r}: expected 'first' or 'all'")
    if ids not in ("auth", "label"):
        raise ValueError(f"ids={ids!r}: expected 'auth' or 'label'")
    lib = hip.get_lib()
    text, offsets, names = _text_of(text_or_paths, gzip, lib)
    dev, n, F = text.device, int(text.numel()), len(offsets) - 1
    i64 = dict(dtype=torch.int64, device=dev)
    if n == 0:
        return _empty_parsed(dev, F, 0, 0)
    off = torch.from_numpy(offsets).to(dev)
    nchunks = -(-n // READ_CHUNK)
    het, every = int(bool(hetatm)), int(model == "all")
    before = lambda v: torch.cat([torch.full_like(v[:, :1], -1), torch.cummax(v, 1).values[:, :-1]], 1)   # of the chunks in front
    carry = torch.full((8, nchunks), -1, **i64)
    lines = torch.empty((3, nchunks), **i64)
    lib.call("fd_cif_read_lines", text, n, off, F, lines)
    carry[:2] = torch.cumsum(lines[:2], 1) - lines[:2]
    carry[2:3] = before(torch.where(lines[2:3] >= 0, carry[1:2] + lines[2:3], lines[2:3]))
    marks = torch.empty((4, nchunks), **i64)
    lib.call("fd_cif_read_marks", text, n, off, F, carry, marks)
    carry[3:7] = before(marks)
    table = torch.zeros((F, CIF_TABLE), dtype=torch.int32, device=dev)
    file_first = torch.zeros(F, **i64)
    head_bad = torch.empty(nchunks, **i64)
    lib.call("fd_cif_read_header", text, n, off, F, het, int(ids == "label"), carry, table, file_first, head_bad)
    last = torch.empty((1, nchunks), **i64)
    lib.call("fd_cif_read_summary", text, n, off, F, het, carry, table, last)
    carry[7:8] = before(last)
    counts = torch.empty((3, nchunks), **i64)
    lib.call("fd_cif_read_count", text, n, off, F, het, every, carry, table, counts)
    ends = torch.cumsum(counts[:2], 1)
    T, C, n_lines, word = (int(v) for v in torch.stack([ends[0, -1], ends[1, -1], lines[0].sum(),
                                                        torch.minimum(counts[2].min(), head_bad.min())]).cpu())
    if word != STATUS_OK:
        line, kind = divmod(word, 8)
        first = file_first.cpu().numpy()
        f = max(g for g in range(F) if offsets[g + 1] > offsets[g] and first[g] <= line)
        raise ValueError(f"cannot be read as mmCIF text: {CIF_KINDS.get(kind, kind)} in file {f} ({names[f]}), line {line - first[f] + 1}")
    out = _empty_parsed(dev, F, T, C)
    out.n_lines = n_lines
    if T:
        bases = (ends - counts[:2]).contiguous()
        dropped = torch.empty(T, dtype=torch.int32, device=dev)
        lib.call("fd_cif_read_fill", text, n, off, F, het, every, carry, table, bases, T, C, out.atom_positions, out.atom_mask,
                 out.b_factors, out.aatype, out.residue_index, dropped, out.chain_offsets, out.chain_file, out.chain_model,
                 out.chain_id)
        _close(out, dropped)
    return out


def parse_pdb_feats(pdb_name, pdb_path, scale_factor=1., chain_id='A'):
    """The reference's data.utils.parse_pdb_feats with the file read on the device: the same signature and the same dict of numpy
    arrays -- atom_positions [L,37,3], atom_mask [L,37], b_factors [L,37] (float64), aatype, residue_index [L] (int64), bb_mask [L],
    bb_positions [L,3] -- for chain_id a string; a dict of those by chain for a list, or for None (every chain of the file).
    The first model is read, without HETATM records (parse_pdb's note).  Segments that share a chain ID are joined in file order,
    as Biopython's chains are.  Centring and scaling are parse_chain_feats' arithmetic in float64 numpy on the arrays read
    back.  b-factors are widened through their shortest decimal: a field of six columns survives float32 unchanged, so this is
    float(field), what Biopython stores."""
    del pdb_name
    parsed = parse_pdb(pdb_path, hetatm=False, model="first")
    _, _, _, ci = parsed.host_tables()
    ids = [chr(c) for c in ci]
    host = {}

    def _process_chain_id(x):
        if x not in ids:
            raise KeyError(x)
        if not host:
            host.update(pos=parsed.atom_positions.cpu().numpy(), mask=parsed.atom_mask.cpu().numpy(),
                        aa=parsed.aatype.cpu().numpy(), ri=parsed.residue_index.cpu().numpy(), b=parsed.b_factors.cpu().numpy())
        off = parsed.host_tables()[0]
        rows = np.concatenate([np.arange(off[c], off[c + 1]) for c, i in enumerate(ids) if i == x])
        feats = {"atom_positions": host["pos"][rows].astype(np.float64), "aatype": host["aa"][rows].astype(np.int64),
                 "atom_mask": host["mask"][rows].astype(np.float64), "residue_index": host["ri"][rows].astype(np.int64),
                 "b_factors": host["b"][rows].astype(str).astype(np.float64)}
        feats["bb_mask"] = feats["atom_mask"][:, _CA]
        bb_center = np.sum(feats["atom_positions"][:, _CA], axis=0) / (np.sum(feats["bb_mask"]) + 1e-5)
        centered = feats["atom_positions"] - bb_center[None, None, :]
        feats["atom_positions"] = (centered / scale_factor) * feats["atom_mask"][..., None]
        feats["bb_positions"] = feats["atom_positions"][:, _CA]
        return feats

    if isinstance(chain_id, str):
        return _process_chain_id(chain_id)
    if isinstance(chain_id, list):
        return {x: _process_chain_id(x) for x in chain_id}
    if chain_id is None:
        return {x: _process_chain_id(x) for x in dict.fromkeys(ids)}
    raise ValueError(f'Unrecognized chain list {chain_id}')
