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
