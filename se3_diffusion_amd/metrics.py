"""Scoring sampled backbones on the device: the coordinate arithmetic of the reference's sample evaluation
(Experiment.eval_fn -> analysis/metrics.py::protein_metrics) on the kernels of csrc/fd_metrics.hip.

From the reference: ca_ca_distance (analysis/metrics.py:120-125), ca_ca_clashes (:127-132) and calc_aligned_rmsd (:71-73) on
data/utils.py::rigid_transform_3D (:519-568) -- the columns ca_ca_bond_dev, ca_ca_valid_percent, num_ca_steric_clashes and
ca_steric_clash_percent of its metrics.csv, and the superposition of its self-consistency step.  This module's own: a peptide-bond
(C-N) check, a CA radius of gyration (in Angstrom over the CA atoms: NOT mdtraj's radius_of_gyration column, which takes all atoms
and reports nm), tm_kabsch, the TM-score formula under the one least-squares superposition -- a lower bound of the TM-score
of the given correspondence -- and tm_score, that TM-score itself: the maximum over superpositions, found by the seed-and-refine
search of Zhang & Skolnick's TM-score program (fd_tm_search; the search is spelt out in include/fd_hip.h).  It is the tm_score
column of the reference (analysis/metrics.py:44-46,104-105) for pairs whose residue-to-residue correspondence is given: sample
against ground truth, against its refolded self, against another sample of equal length.

tm_align / tm_align_matrix: TM-align's search over alignments (fd_tm_align: four initial alignments, a Needleman-Wunsch DP on the
device, the iteration between DP and superposition search; include/fd_hip.h is the specification and lists the deliberate
simplifications) -- what the reference's tmtools.tm_align performs for its tm_score column, for chains of any two lengths: sample
against sample of another length, sample against a chain of a structure library (novelty), the diversity matrix of a mixed-length
run.  Verified: a float64 restatement of the specification, analytic properties (rigid copies, deletions, identical chains) and
three pairs of deposited chains.  NOT verified: agreement with the values tmtools or the TM-score program print, for tm_score and
for tm_align alike, because neither is available to the tests.

secondary_structure: the reference's SHAPE_METRICS (analysis/metrics.py:37-42, :58-69) -- coil_percent, helix_percent,
strand_percent, non_coil_percent from Kabsch & Sander's assignment (fd_dssp_hbonds, fd_dssp_assign; include/fd_hip.h is the
specification) and radius_of_gyration as mdtraj's compute_rg defines it (all atoms, unit mass, nm) -- without the PDB file, mdtraj
and the host round trip of the reference.  NOT verified: no DSSP program and no mdtraj exists where this project is built, so
agreement with the letters md.compute_dssp prints has never been checked; the tests check a float64 restatement and its
plausibility against the HELIX / SHEET records of six deposited structures.  Two deliberate differences from the DSSP program:
the H-bond energy is not rounded to three decimals, and the gaps of a bulge must be non-negative.

violations: the reference's INTER_VIOLATION_METRICS (analysis/metrics.py:13-17) -- bonds_c_n_loss_mean, angles_ca_c_n_loss_mean,
clashes_mean_loss -- with angles_c_n_ca_loss_mean, the per-residue and per-atom arrays and compute_violation_metrics' fractions:
openfold/utils/loss.py's between_residue_bond_loss, between_residue_clash_loss and compute_violation_metrics for an all-alanine
chain, under amber_minimize.find_violations' tolerances (fd_violations; include/fd_hip.h is the specification), without the Protein
object, the atom14 arrays and the [N,N,14,14] tensors of the reference.  Verified against the unmodified reference functions, run
in float32 and in float64 on the compacted chain (tests/golden/violations.npz).  Two deliberate differences: an absent residue
takes no part (the reference would leave it at the origin, existing), and the within-residue term is left out (zero by
construction for a backbone built from ideal geometry), so violations_per_residue and num_residue_violations take the connection
and clash masks only.  Still not here: that within-residue term and the OpenMM relaxation itself, solvent
accessibility, and the sheet-label and bridge-partner columns of a DSSP record.

linkage / cluster / diversity / novelty: the two set-level figures of a sampling run.  diversity is the number of clusters over the
number of samples, from hierarchical clustering of the pairwise TM-scores at 0.5 (the paper: MaxCluster, average linkage); here
fd_cluster_linkage (single, average or complete linkage of a similarity or distance matrix where it lies in HBM, one block per
matrix) and fd_cluster_cut (flat clusters, medoids, counts; include/fd_hip.h is the specification).  novelty is the highest
TM-score of a sample against a structure library, from tm_align_matrix.  Verified: a float64 restatement of the specification,
ties included, and a recorded run of scipy.cluster.hierarchy on matrices without ties (tests/golden/cluster.npz).  NOT verified:
the reference repository holds no clustering code and MaxCluster is not available where this project is built, so agreement
with the clusters or centroids MaxCluster prints has never been checked.  The inclusive cut (similarity >= threshold merges) and
the tie rule (smallest height, then smaller id, then larger id) are this project's own choices.

Every value stays on the device as float64; only eval_rows copies to the host, once.
"""
from __future__ import annotations

import torch

from . import hip

BACKBONE_SLOTS = ("num_res", "ca_ca_bond_dev", "ca_ca_valid_percent", "num_ca_steric_clashes", "ca_steric_clash_percent",
                  "ca_radius_of_gyration", "c_n_bond_dev", "c_n_bond_valid_percent", "max_ca_ca_dist")
RMSD_SLOTS = ("num_aligned", "mean_dist", "rmsd", "tm_kabsch", "reflection", "max_dist")
TM_SLOTS = ("num_aligned", "tm_score", "tm_kabsch", "best_seed", "num_seeds", "d0", "passes")
TM_MAX_N = 2048          # fd_tm_search's limit (48 KB of LDS for the six coordinate arrays)
TM_FILL_BLOCKS = 768     # blocks resident at once on the 256 CUs of an MI355X: three per CU (164 VGPRs, 48 KB of LDS each)
TM_ALIGN_SLOTS = ("La", "Lb", "num_aligned", "tm_norm_a", "tm_norm_b", "rmsd", "d0_a", "d0_b", "best_class", "num_dp", "num_units",
                  "search_tm")
TM_ALIGN_MAX_N = 1024    # FD_TM_ALIGN_MAX_N: both chains of a pair stay in LDS (six fp32 arrays of 1024)
TM_ALIGN_FILL_BLOCKS = 256    # the seed launch keeps about 100 KB of LDS per block: one block per CU of an MI355X
SHAPE_SLOTS = ("num_res", "helix_percent", "strand_percent", "coil_percent", "non_coil_percent", "radius_of_gyration",
               "num_hbonds", "overflow")
SHAPE_COLUMNS = ("coil_percent", "helix_percent", "strand_percent", "non_coil_percent", "radius_of_gyration")    # the reference's names
DSSP_MAX_N = 2048        # FD_DSSP_MAX_N: fd_dssp_hbonds keeps C, O and CA of a whole chain in LDS (80 KB of a CU's 160 KB)
VIOLATION_SLOTS = ("num_res", "bonds_c_n_loss_mean", "angles_ca_c_n_loss_mean", "angles_c_n_ca_loss_mean", "clashes_mean_loss",
                   "violations_extreme_ca_ca_distance", "violations_between_residue_bond", "violations_between_residue_clash",
                   "violations_per_residue", "num_residue_violations", "num_bonds", "num_atom_pairs", "num_clashing_pairs")
# the reference's INTER_VIOLATION_METRICS (analysis/metrics.py:13-17) first, then the fourth mean and compute_violation_metrics' fractions
VIOLATION_COLUMNS = ("bonds_c_n_loss_mean", "angles_ca_c_n_loss_mean", "clashes_mean_loss", "angles_c_n_ca_loss_mean",
                     "violations_extreme_ca_ca_distance", "violations_between_residue_bond", "violations_between_residue_clash",
                     "violations_per_residue", "num_residue_violations")
VIOLATIONS_MAX_N = 2048  # FD_VIOLATIONS_MAX_N: fd_violations keeps the five atoms of a whole chain in LDS (140 KB of a CU's 160 KB)
VIOLATIONS_TILE = 64     # FD_VIOLATIONS_TILE
CLUSTER_SLOTS = ("num_samples", "num_clusters", "diversity", "largest_cluster", "num_singletons", "mean_within_cluster",
                 "last_height_below_cut", "first_height_above_cut")
CLUSTER_MAX_M = 4096     # FD_CLUSTER_MAX_M: the per-row caches of fd_cluster_linkage in LDS (92 KB), 128 MB of workspace per matrix
CLUSTER_METHODS = {"single": 0, "average": 1, "complete": 2}
CLUSTER_KINDS = {"distance": 0, "similarity": 1}
SS_LETTERS = " HBEGITS"  # fd_dssp_assign's codes 0..7 (-1: the residue is absent)
CA = 1                   # slot of CA in atom37 / the compact [.,5,3] order N, CA, C, CB, O


def _f32c(x):
    return x if x.dtype == torch.float32 and x.is_contiguous() else x.to(torch.float32).contiguous()


def _backbone_block(atoms, res_mask=None, out=None):
    """[B,12] float64: fd_backbone_metrics' rows for atoms [B,N,A,3] (A = 37 or 5), one launch."""
    if atoms.dim() != 4 or atoms.shape[-1] != 3 or atoms.shape[-2] not in (5, 37):
        raise ValueError(f"atoms of shape {tuple(atoms.shape)}: expected [B,N,37,3] or [B,N,5,3] (or the same without B)")
    B, N, A = atoms.shape[:3]
    atoms = _f32c(atoms)
    if res_mask is None:
        # the reference's own mask (analysis/metrics.py:86,94): a residue is present iff any of its coordinates is non-zero
        res_mask = (atoms != 0).reshape(B, N, A * 3).any(-1)
    res_mask = _f32c(res_mask.reshape(B, N))
    if out is None:
        out = torch.empty((B, 12), dtype=torch.float64, device=atoms.device)
    elif out.shape != (B, 12) or out.dtype != torch.float64 or not out.is_contiguous():
        raise ValueError(f"out: expected a contiguous float64 [{B},12] tensor")
    hip.get_lib().call("fd_backbone_metrics", atoms, A * 3, res_mask, B, N, out)
    return out


def backbone_metrics(atoms, res_mask=None, out=None):
    """Per-backbone geometry of atoms [B,N,37,3] or [B,N,5,3] (atom order N, CA, C, CB, O; or the same without B):
    dict name -> float64 device tensor [B] (0-d without B) under BACKBONE_SLOTS, the slot table of include/fd_hip.h.  res_mask [B,N]:
    a residue is present iff its value is non-zero; None derives it the reference's way (present iff any coordinate is non-zero).
    out: a float64 [B,12] tensor to write (the returned tensors are views of it).  One launch, no host synchronisation."""
    batched = atoms.dim() == 4
    if not batched:
        atoms = atoms[None]
        res_mask = None if res_mask is None else res_mask[None]
    blk = _backbone_block(atoms, res_mask, out)
    return {name: (blk[:, k] if batched else blk[0, k]) for k, name in enumerate(BACKBONE_SLOTS)}


def _dssp_call(atoms, res_mask, no_donor):
    """fd_dssp_hbonds then fd_dssp_assign on atoms [B,N,A,3]: ss int8 [B,N], out float64 [B,8], acc_idx int32 [B,N,2], acc_e float64 [B,N,2]"""
    if atoms.dim() != 4 or atoms.shape[-1] != 3 or atoms.shape[-2] not in (5, 37):
        raise ValueError(f"atoms of shape {tuple(atoms.shape)}: expected [B,N,37,3] or [B,N,5,3] (or the same without B)")
    B, N, A = atoms.shape[:3]
    if N > DSSP_MAX_N:
        raise ValueError(f"secondary_structure: N = {N} residues, at most {DSSP_MAX_N} are supported")
    atoms = _f32c(atoms)
    dev = atoms.device
    if res_mask is None:
        res_mask = (atoms != 0).reshape(B, N, A * 3).any(-1)
    res_mask = _f32c(res_mask.reshape(B, N))
    if no_donor is not None:
        no_donor = _f32c(no_donor.reshape(B, N))
    acc_idx = torch.empty((B, N, 2), dtype=torch.int32, device=dev)
    acc_e = torch.empty((B, N, 2), dtype=torch.float64, device=dev)
    ss = torch.empty((B, N), dtype=torch.int8, device=dev)
    if N == 0:
        # the entry points launch nothing on an empty chain: num_res 0, the means over no residues NaN, no bonds, no overflow
        out = torch.full((B, 8), float("nan"), dtype=torch.float64, device=dev)
        out[:, 0] = 0.0
        out[:, 6:] = 0.0
        return ss, out, acc_idx, acc_e
    out = torch.empty((B, 8), dtype=torch.float64, device=dev)
    lib = hip.get_lib()
    lib.call("fd_dssp_hbonds", atoms, A * 3, res_mask, no_donor, B, N, acc_idx, acc_e)
    lib.call("fd_dssp_assign", atoms, A * 3, A, res_mask, acc_idx, acc_e, B, N, ss, out)
    return ss, out, acc_idx, acc_e


def secondary_structure(atoms, res_mask=None, no_donor=None, return_hbonds=False):
    """Kabsch & Sander's secondary structure of atoms [B,N,37,3] or [B,N,5,3] (atom order N, CA, C, CB, O; or the same without B)
    and the reference's shape columns: dict with ss (int8 [B,N]: -1 absent, 0 blank, 1 H, 2 B, 3 E, 4 G, 5 I, 6 T, 7 S), ss3
    (int8: -1 absent, 0 C, 1 H, 2 E -- mdtraj's simplified classes) and a float64 device tensor [B] (0-d without B) per name of
    SHAPE_SLOTS (radius_of_gyration over all atoms, in nm).  res_mask as backbone_metrics; no_donor [B,N]: non-zero where the
    residue has no amide hydrogen (prolines).  return_hbonds adds acc_idx (int32 [B,N,2], each donor's two best acceptors by
    residue index, -1 if none) and acc_e (float64, kcal/mol).  include/fd_hip.h is the specification and says what is not
    verified.  N <= 2048, or ValueError before anything is launched.  Two launches, no host synchronisation."""
    batched = atoms.dim() == 4
    if not batched:
        atoms = atoms[None]
        res_mask = None if res_mask is None else res_mask[None]
        no_donor = None if no_donor is None else no_donor[None]
    ss, out, acc_idx, acc_e = _dssp_call(atoms, res_mask, no_donor)
    helix, strand = (ss == 1) | (ss == 4) | (ss == 5), (ss == 2) | (ss == 3)
    ss3 = (helix.to(torch.int8) + 2 * strand.to(torch.int8)).masked_fill_(ss < 0, -1)      # (fills on the device: nothing is uploaded)
    pick = (lambda x: x) if batched else (lambda x: x[0])
    res = {"ss": pick(ss), "ss3": pick(ss3)}
    res.update({name: pick(out[:, k]) for k, name in enumerate(SHAPE_SLOTS)})
    if return_hbonds:
        res["acc_idx"] = pick(acc_idx)
        res["acc_e"] = pick(acc_e)
    return res


def _violations_call(atoms, res_mask, res_index, per_residue):
    """fd_violations on atoms [B,N,A,3]: out float64 [B,16], then res_loss [B,N], atom_loss [B,N,5], flags uint8 [B,N] (or None)"""
    if atoms.dim() != 4 or atoms.shape[-1] != 3 or atoms.shape[-2] not in (5, 37):
        raise ValueError(f"atoms of shape {tuple(atoms.shape)}: expected [B,N,37,3] or [B,N,5,3] (or the same without B)")
    B, N, A = atoms.shape[:3]
    if N > VIOLATIONS_MAX_N:
        raise ValueError(f"violations: N = {N} residues, at most {VIOLATIONS_MAX_N} are supported")
    atoms = _f32c(atoms)
    dev = atoms.device
    if res_mask is None:
        res_mask = (atoms != 0).reshape(B, N, A * 3).any(-1)
    res_mask = _f32c(res_mask.reshape(B, N))
    if res_index is not None:
        res_index = res_index.reshape(B, N).to(torch.int32).contiguous()
    # (zeros, not empty: the entry point launches nothing on an empty chain, and zeros are what the formulas give there)
    out = torch.zeros((B, 16), dtype=torch.float64, device=dev)
    res_loss = atom_loss = flags = None
    if per_residue:
        res_loss = torch.zeros((B, N), dtype=torch.float64, device=dev)
        atom_loss = torch.zeros((B, N, 5), dtype=torch.float64, device=dev)
        flags = torch.zeros((B, N), dtype=torch.uint8, device=dev)
    ws = torch.empty((max(1, B * (-(-N // VIOLATIONS_TILE)) * 16),), dtype=torch.float64, device=dev)     # FD_VIOLATIONS_WS_DOUBLES
    hip.get_lib().call("fd_violations", atoms, A * 3, res_mask, res_index, B, N, ws, out, res_loss, atom_loss, flags)
    return out, res_loss, atom_loss, flags


def violations(atoms, res_mask=None, res_index=None, per_residue=False):
    """The reference's between-residue violation losses (openfold/utils/loss.py: between_residue_bond_loss, between_residue_clash_loss,
    compute_violation_metrics, with amber_minimize.find_violations' tolerances) of atoms [B,N,37,3] or [B,N,5,3] (atom order N, CA, C,
    CB, O; or the same without B), read as an all-alanine chain: dict name -> float64 device tensor [B] (0-d without B) under
    VIOLATION_SLOTS, the slot table of include/fd_hip.h, which also names the two deliberate differences (absent residues take no
    part; no within-residue term).  res_mask as backbone_metrics; res_index [B,N]: residue numbers (None: the position in the padded
    chain) -- a step other than 1 between consecutive present residues is a gap.  per_residue=True adds
    connections_per_residue_loss_sum (float64 [B,N]), connections_per_residue_violation_mask (bool [B,N]),
    clashes_per_atom_loss_sum (float64 [B,N,5]) and clashes_per_atom_clash_mask (bool [B,N,5]), zero at absent residues.
    N <= 2048, or ValueError before anything is launched.  One call (two launches), no host synchronisation."""
    batched = atoms.dim() == 4
    if not batched:
        atoms = atoms[None]
        res_mask = None if res_mask is None else res_mask[None]
        res_index = None if res_index is None else res_index[None]
    out, res_loss, atom_loss, flags = _violations_call(atoms, res_mask, res_index, per_residue)
    pick = (lambda x: x) if batched else (lambda x: x[0])
    res = {name: pick(out[:, k]) for k, name in enumerate(VIOLATION_SLOTS)}
    if per_residue:
        bit = torch.arange(5, device=flags.device, dtype=torch.uint8)
        res["connections_per_residue_loss_sum"] = pick(res_loss)
        res["connections_per_residue_violation_mask"] = pick((flags & 32) != 0)
        res["clashes_per_atom_loss_sum"] = pick(atom_loss)
        res["clashes_per_atom_clash_mask"] = pick(((flags[..., None] >> bit) & 1) != 0)
    return res


def ss_string(codes, classes=False):
    """Host helper (copies to the host): the usual one-letter strings of secondary_structure's ss codes, [N] -> str, [B,N] -> list
    of str: H B E G I T S, a blank for a blank residue, '-' for an absent one.  classes=True reads the codes as ss3: C H E."""
    rows = torch.as_tensor(codes).cpu().tolist()
    letters = "CHE" if classes else SS_LETTERS
    one = lambda row: "".join("-" if c < 0 else letters[c] for c in row)
    return one(rows) if rows == [] or not isinstance(rows[0], list) else [one(r) for r in rows]


def _points(pos):
    """fp32 [P,N,3] whose layout fd_aligned_rmsd can address in place: unit stride along xyz, one point stride, sets N points apart"""
    if pos.dim() != 3 or pos.shape[-1] != 3:
        raise ValueError(f"points of shape {tuple(pos.shape)}: expected [P,N,3] or [N,3]")
    P, N = pos.shape[:2]
    ok = pos.dtype == torch.float32 and pos.stride(2) == 1 and pos.stride(1) >= 3 and (P == 1 or pos.stride(0) == N * pos.stride(1))
    if not ok:
        pos = pos.to(torch.float32).contiguous()
    return pos, (pos.stride(1) if N > 1 else 3)


def _rmsd_call(pos_1, pos_2, mask, ia, ib, P, want_transform):
    a, a_stride = _points(pos_1)
    b, b_stride = _points(pos_2)
    N = a.shape[1]
    dev = a.device
    if mask is not None:
        mask = _f32c(mask.reshape(-1, N))
    out = torch.empty((P, 8), dtype=torch.float64, device=dev)
    tr = torch.empty((P, 12), dtype=torch.float64, device=dev) if want_transform else None
    hip.get_lib().call("fd_aligned_rmsd", a, a_stride, b, b_stride, ia, ib, mask, P, N, out, tr)
    return out, tr


def aligned_rmsd(pos_1, pos_2, mask=None, return_transform=False):
    """Least-squares superposition of pos_1 onto pos_2 ([P,N,3] or [N,3]; a strided view such as atom37[:, :, 1] is read in
    place) by the optimal proper rotation, rigid_transform_3D's after its reflection fix.  mask [P,N] (or [N]): the positions that
    count.  dict name -> float64 device tensor [P] (0-d without P) under RMSD_SLOTS: mean_dist is the reference's
    calc_aligned_rmsd (a mean of distances, not a root mean square), rmsd the root mean square, tm_kabsch the TM-score formula
    under this superposition, reflection 1.0 iff the reference would report reflection_detected.  return_transform adds R [P,3,3] and
    t [P,3] with aligned = R a + t.  One launch, no host synchronisation."""
    batched = pos_1.dim() == 3
    if not batched:
        pos_1, pos_2 = pos_1[None], pos_2[None]
    if pos_1.shape != pos_2.shape:
        raise ValueError(f"point sets of shapes {tuple(pos_1.shape)} and {tuple(pos_2.shape)}")
    P = pos_1.shape[0]
    out, tr = _rmsd_call(pos_1, pos_2, mask, None, None, P, return_transform)
    pick = (lambda x: x) if batched else (lambda x: x[0])
    res = {name: pick(out[:, k]) for k, name in enumerate(RMSD_SLOTS)}
    if return_transform:
        res["R"] = pick(tr[:, :9].reshape(P, 3, 3))
        res["t"] = pick(tr[:, 9:])
    return res


def pairwise_rmsd(pos, mask=None):
    """All-pairs superposed distances of M point sets pos [M,N,3] (mask [M,N]: a position counts in a pair iff it is non-zero in
    both sets): dict of float64 [M,M] device tensors mean_dist, rmsd, tm_kabsch.  tm_kabsch is only a lower bound of a pair's
    TM-score; the matrix that diversity clustering at a TM-score threshold starts from is pairwise_tm's.  One launch over the
    M (M - 1) / 2 upper pairs; the result is mirrored, the diagonal is 0, 0 and 1."""
    if pos.dim() != 3:
        raise ValueError(f"points of shape {tuple(pos.shape)}: expected [M,N,3]")
    M = pos.shape[0]
    dev = pos.device
    iu = torch.triu_indices(M, M, 1, device=dev)
    ia, ib = iu[0].to(torch.int32).contiguous(), iu[1].to(torch.int32).contiguous()
    P = ia.numel()
    out, _ = _rmsd_call(pos, pos, mask, ia, ib, P, False)
    res = {}
    for name, diag in (("mean_dist", 0.0), ("rmsd", 0.0), ("tm_kabsch", 1.0)):
        m = torch.zeros((M, M), dtype=torch.float64, device=dev)
        v = out[:, RMSD_SLOTS.index(name)]
        m[iu[0], iu[1]] = v
        m[iu[1], iu[0]] = v
        m.fill_diagonal_(diag)
        res[name] = m
    return res


def tm_num_seeds(L, seed_step=1):
    """Number of seeds fd_tm_search tries on L counting positions (include/fd_hip.h): the fragment lengths L, L >> 1, ... while above
    4 (at most six), then 4; for each the starts 0, seed_step, ... <= L - length.  0 below four positions."""
    if L < 4:
        return 0
    lens, l = [], L
    for i in range(6):
        if l <= 4:
            break
        lens.append(l)
        l = L >> (i + 1)
    lens.append(4)
    return sum((L - l) // seed_step + 1 for l in lens)


def tm_parts(P, N, seed_step=1):
    """How many blocks share the seeds of one pair when the caller does not say: enough for P * parts to reach TM_FILL_BLOCKS
    when there are few pairs, never more than ceil(seeds / 4) (a block's four waves would have nothing to do).  From N, not from
    the masks, so nothing is read back; the result does not depend on it bit for bit."""
    if P <= 0:
        return 1
    return max(1, min(-(-tm_num_seeds(N, seed_step) // 4), -(-TM_FILL_BLOCKS // P)))


def _tm_call(pos_1, pos_2, mask, ia, ib, P, seed_step, max_iter, parts, want_transform):
    a, a_stride = _points(pos_1)
    b, b_stride = _points(pos_2)
    N = a.shape[1]
    dev = a.device
    if mask is not None:
        mask = _f32c(mask.reshape(-1, N))
    if parts is None:
        parts = tm_parts(P, N, max(1, int(seed_step)))
    out = torch.empty((P, 8), dtype=torch.float64, device=dev)
    tr = torch.empty((P, 12), dtype=torch.float64, device=dev) if want_transform else None
    ws = torch.empty((P * max(1, int(parts)) * 64,), dtype=torch.float64, device=dev)      # FD_TM_WS_DOUBLES
    hip.get_lib().call("fd_tm_search", a, a_stride, b, b_stride, ia, ib, mask, P, N, seed_step, max_iter, parts, ws, out, tr)
    return out, tr


def tm_score(pos_1, pos_2, mask=None, seed_step=1, max_iter=20, return_transform=False, parts=None):
    """TM-score of pos_1 against pos_2 ([P,N,3] or [N,3]; a strided view such as atom37[:, :, 1] is read in place) under the GIVEN
    correspondence, position k to position k: the maximum over superpositions of the TM-score formula, found by the seed-and-refine
    search of the TM-score program (include/fd_hip.h spells it out), normalised by the number of counting positions.  Not
    TM-align: no search over alignments.  mask [P,N] (or [N]): the positions that count.  seed_step: distance between the starts of
    the seed fragments (1 = every start; a coarser step searches a subset of the seeds, so it can only lower the score); max_iter:
    refinements per seed; parts: blocks per pair (None: tm_parts; the result does not depend on it bit for bit).  dict name ->
    float64 device tensor [P] (0-d without P) under TM_SLOTS; return_transform adds R [P,3,3] and t [P,3] of the best superposition,
    aligned = R a + t.  N <= 2048.  Two launches (search, reduce), no host synchronisation."""
    batched = pos_1.dim() == 3
    if not batched:
        pos_1, pos_2 = pos_1[None], pos_2[None]
        mask = None if mask is None else mask[None]
    if pos_1.shape != pos_2.shape:
        raise ValueError(f"point sets of shapes {tuple(pos_1.shape)} and {tuple(pos_2.shape)}")
    P = pos_1.shape[0]
    out, tr = _tm_call(pos_1, pos_2, mask, None, None, P, seed_step, max_iter, parts, return_transform)
    pick = (lambda x: x) if batched else (lambda x: x[0])
    res = {name: pick(out[:, k]) for k, name in enumerate(TM_SLOTS)}
    if return_transform:
        res["R"] = pick(tr[:, :9].reshape(P, 3, 3))
        res["t"] = pick(tr[:, 9:])
    return res


def pairwise_tm(pos, mask=None, seed_step=1, max_iter=20):
    """All-pairs TM-scores (tm_score) of M point sets pos [M,N,3] (mask [M,N]: a position counts in a pair iff it is non-zero in both
    sets): float64 [M,M] device tensor, the matrix diversity clustering starts from.  One search over the M (M - 1) / 2 upper
    pairs; the result is mirrored (with equal lengths and a fixed correspondence the normalisation is the same both ways; the
    search itself runs set i onto set j, i < j), the diagonal is 1."""
    if pos.dim() != 3:
        raise ValueError(f"points of shape {tuple(pos.shape)}: expected [M,N,3]")
    M = pos.shape[0]
    dev = pos.device
    iu = torch.triu_indices(M, M, 1, device=dev)
    ia, ib = iu[0].to(torch.int32).contiguous(), iu[1].to(torch.int32).contiguous()
    out, _ = _tm_call(pos, pos, mask, ia, ib, ia.numel(), seed_step, max_iter, None, False)
    m = torch.zeros((M, M), dtype=torch.float64, device=dev)
    v = out[:, TM_SLOTS.index("tm_score")]
    m[iu[0], iu[1]] = v
    m[iu[1], iu[0]] = v
    m.fill_diagonal_(1.0)
    return m


def tm_align_units(La, Lb):
    """Number of units fd_tm_align's seed launch deals to its waves for chains of La and Lb counting positions (include/fd_hip.h):
    the gapless offsets plus the fragment pairs.  0 when the shorter chain has fewer than five."""
    Lmin = min(La, Lb)
    if Lmin < 5:
        return 0
    m = min(Lmin, max(Lmin // 2, 5))
    f = min(20, Lmin // 3)
    units = La + Lb - 2 * m + 1
    if f >= 4:
        starts = lambda L: (L - f) // max(f, -(-(L - f + 1) // 8)) + 1
        units += starts(La) * starts(Lb)
    return units


def tm_align_parts(P, Na, Nb):
    """How many blocks share the seed units of one pair when the caller does not say: enough for P * parts to reach
    TM_ALIGN_FILL_BLOCKS when there are few pairs, never more than ceil(units / 4).  From Na and Nb, not from the masks, so nothing
    is read back; the result does not depend on it bit for bit."""
    if P <= 0:
        return 1
    return max(1, min(-(-tm_align_units(Na, Nb) // 4), -(-TM_ALIGN_FILL_BLOCKS // P)))


def tm_align_ws_bytes(P, parts, Na, Nb):
    """FD_TM_ALIGN_WS_BYTES of include/fd_hip.h"""
    return P * parts * 4 * 32 * 8 + P * 4 * 16 * 8 + P * parts * 4 * Na * ((Nb + 31) // 32) * 8 + P * 4 * 2 * Na * 2


def _d0(L):
    """d0(L) of include/fd_hip.h on a float64 tensor of lengths"""
    return torch.where(L > 21, 1.24 * (L - 15.0).clamp_min(0.0).pow(1.0 / 3.0) - 1.8, torch.full_like(L, 0.5))


def _align_call(pos_1, pos_2, mask_1, mask_2, ia, ib, P, search_step, max_dp, parts, want_transform):
    a, a_stride = _points(pos_1)
    b, b_stride = _points(pos_2)
    Na, Nb = a.shape[1], b.shape[1]
    if Na > TM_ALIGN_MAX_N or Nb > TM_ALIGN_MAX_N:
        raise ValueError(f"tm_align: chains of {Na} and {Nb} positions, at most {TM_ALIGN_MAX_N} are supported")
    dev = a.device
    if mask_1 is not None:
        mask_1 = _f32c(mask_1.reshape(-1, Na))
    if mask_2 is not None:
        mask_2 = _f32c(mask_2.reshape(-1, Nb))
    if parts is None:
        parts = tm_align_parts(P, Na, Nb)
    out = torch.empty((P, 16), dtype=torch.float64, device=dev)
    amap = torch.empty((P, Na), dtype=torch.int32, device=dev)
    tr = torch.empty((P, 12), dtype=torch.float64, device=dev) if want_transform else None
    ws = torch.empty((max(8, tm_align_ws_bytes(P, max(1, int(parts)), Na, Nb)) + 7) // 8, dtype=torch.float64, device=dev)
    hip.get_lib().call("fd_tm_align", a, a_stride, Na, b, b_stride, Nb, ia, ib, mask_1, mask_2, P, search_step, max_dp, parts, ws,
                       out, amap, tr)
    if Na == 0 or Nb == 0:
        # the entry point launches nothing on an empty chain: the lengths, no alignment, NaN in the score slots
        def lengths(mask, idx, N):
            if mask is None or N == 0:
                return torch.full((P,), float(N), dtype=torch.float64, device=dev)
            rows = (mask != 0).sum(-1).to(torch.float64)
            return rows[:P] if idx is None else rows[idx.long()]
        out.zero_()
        out[:, 0], out[:, 1] = lengths(mask_1, ia, Na), lengths(mask_2, ib, Nb)
        out[:, 6], out[:, 7] = _d0(out[:, 0]), _d0(out[:, 1])
        out[:, 8] = -1.0
        out[:, [3, 4, 5, 11]] = float("nan")
        amap.fill_(-1)
        if tr is not None:
            tr.fill_(float("nan"))
    return out, amap, tr


def tm_align(pos_1, pos_2, mask_1=None, mask_2=None, search_step=40, max_dp=30, return_transform=False, parts=None):
    """TM-align of pos_1 [P,Na,3] against pos_2 [P,Nb,3] (or the same without P; strided views such as atom37[:, :, 1] are read in
    place): the search over residue-to-residue alignments that include/fd_hip.h specifies (fd_tm_align), for chains of any two
    lengths.  mask_1 [P,Na], mask_2 [P,Nb]: the positions that count.  search_step: distance between the seed fragments of the
    search phase; max_dp: DP iterations per gap penalty; parts: blocks per pair of the seed launch (None: tm_align_parts; the
    result does not depend on it bit for bit).  dict name -> float64 device tensor [P] (0-d without P) under TM_ALIGN_SLOTS --
    tm_norm_b is the reference's tm_score column when pos_2 is the ground truth -- plus map (int32 [P,Na]: for each position of
    pos_1 its partner in pos_2, or -1); return_transform adds R [P,3,3] and t [P,3] of tm_norm_b's superposition, aligned = R a + t.
    Agreement with tmtools is NOT verified (see the module docstring).  Na, Nb <= 1024, or ValueError before anything is launched.
    Three launches, no host synchronisation."""
    batched = pos_1.dim() == 3
    if not batched:
        pos_1, pos_2 = pos_1[None], pos_2[None]
        mask_1 = None if mask_1 is None else mask_1[None]
        mask_2 = None if mask_2 is None else mask_2[None]
    if pos_1.dim() != 3 or pos_2.dim() != 3 or pos_1.shape[0] != pos_2.shape[0]:
        raise ValueError(f"point sets of shapes {tuple(pos_1.shape)} and {tuple(pos_2.shape)}")
    P = pos_1.shape[0]
    out, amap, tr = _align_call(pos_1, pos_2, mask_1, mask_2, None, None, P, search_step, max_dp, parts, return_transform)
    pick = (lambda x: x) if batched else (lambda x: x[0])
    res = {name: pick(out[:, k]) for k, name in enumerate(TM_ALIGN_SLOTS)}
    res["map"] = pick(amap)
    if return_transform:
        res["R"] = pick(tr[:, :9].reshape(P, 3, 3))
        res["t"] = pick(tr[:, 9:])
    return res


def tm_align_matrix(pos_a, mask_a=None, pos_b=None, mask_b=None, search_step=40, max_dp=30, parts=None):
    """TM-align of every set of pos_a [Ma,Na,3] (mask_a [Ma,Na]: padding) against every set of pos_b [Mb,Nb,3]: dict of float64
    [Ma,Mb] device tensors tm_norm_a (normalised by the length of the row's chain) and tm_norm_b (by the column's) -- samples
    against a structure library for novelty.  With pos_b=None it is the mixed-length diversity matrix of one set: the upper pairs
    i < j are run (set i onto set j) and mirrored with the two normalisations swapped, so tm_norm_a[j, i] = tm_norm_b[i, j]; the
    diagonal is 1.  One call of fd_tm_align over all pairs."""
    if pos_a.dim() != 3 or (pos_b is not None and pos_b.dim() != 3):
        raise ValueError("tm_align_matrix: expected [M,N,3] point sets")
    dev = pos_a.device
    Ma = pos_a.shape[0]
    if pos_b is None:
        iu = torch.triu_indices(Ma, Ma, 1, device=dev)
        ia, ib = iu[0].to(torch.int32).contiguous(), iu[1].to(torch.int32).contiguous()
        out, _, _ = _align_call(pos_a, pos_a, mask_a, mask_a, ia, ib, ia.numel(), search_step, max_dp, parts, False)
        res = {}
        for name, other in (("tm_norm_a", "tm_norm_b"), ("tm_norm_b", "tm_norm_a")):
            m = torch.zeros((Ma, Ma), dtype=torch.float64, device=dev)
            m[iu[0], iu[1]] = out[:, TM_ALIGN_SLOTS.index(name)]
            m[iu[1], iu[0]] = out[:, TM_ALIGN_SLOTS.index(other)]
            m.fill_diagonal_(1.0)
            res[name] = m
        return res
    Mb = pos_b.shape[0]
    ia = torch.arange(Ma, device=dev, dtype=torch.int32).repeat_interleave(Mb).contiguous()
    ib = torch.arange(Mb, device=dev, dtype=torch.int32).repeat(Ma).contiguous()
    out, _, _ = _align_call(pos_a, pos_b, mask_a, mask_b, ia, ib, Ma * Mb, search_step, max_dp, parts, False)
    return {name: out[:, TM_ALIGN_SLOTS.index(name)].reshape(Ma, Mb) for name in ("tm_norm_a", "tm_norm_b")}


def eval_rows(atom37, res_mask, fixed_mask=None, gt_atom37=None, tm=False, shape=False, violations=False):
    """One dict of Python floats per backbone with the reference's column names (Experiment.eval_fn,
    experiments/train_se3_diffusion.py:475-508, and CA_VIOLATION_METRICS): ca_ca_bond_dev, ca_ca_valid_percent,
    ca_steric_clash_percent, num_ca_steric_clashes, num_res, fixed_residues, diffused_percentage -- and this module's own
    BACKBONE_SLOTS.  gt_atom37 adds aligned_rmsd_to_gt (calc_aligned_rmsd of the sample's CA onto the ground truth's) over the
    diffused present residues (analysis/metrics.py:100-102); with tm=True it also adds tm_score_to_gt, tm_score over the same
    residues, normalised by their number -- the ground truth's length under the reference's own masking (metrics.py:100-105);
    with tm="align" it adds tm_align_to_gt instead: tm_align's tm_norm_b of the sample's CA against the ground truth's over the same
    residues, the alignment search protein_metrics itself runs (tmtools.tm_align; agreement with its values is not verified).
    shape=True adds the reference's SHAPE_METRICS and non_coil_percent (SHAPE_COLUMNS; secondary_structure without a proline
    mask, as the backbone carries no sequence).  violations=True adds VIOLATION_COLUMNS: the reference's INTER_VIOLATION_METRICS
    (bonds_c_n_loss_mean, angles_ca_c_n_loss_mean, clashes_mean_loss), angles_c_n_ca_loss_mean and the violation fractions, from
    fd_violations with the position in the padded chain as the residue number.  One device-to-host copy."""
    B, N = atom37.shape[:2]
    res_mask = res_mask.reshape(B, N).to(torch.float32)
    fixed = torch.zeros_like(res_mask) if fixed_mask is None else fixed_mask.reshape(B, N).to(torch.float32)
    present = (res_mask != 0).to(torch.float64)
    cols = [_backbone_block(atom37, res_mask), (fixed.to(torch.float64) * present).sum(-1, keepdim=True)]
    if gt_atom37 is not None:
        a37, g37 = _f32c(atom37), _f32c(gt_atom37)
        diffused = (1.0 - fixed) * (res_mask != 0)
        out, _ = _rmsd_call(a37[:, :, CA], g37[:, :, CA], diffused, None, None, B, False)
        cols.append(out)
        if isinstance(tm, str):
            if tm != "align":
                raise ValueError(f"eval_rows: tm = {tm!r}, expected False, True or 'align'")
            cols.append(_align_call(a37[:, :, CA], g37[:, :, CA], diffused, diffused, None, None, B, 40, 30, None, False)[0])
        elif tm:
            cols.append(_tm_call(a37[:, :, CA], g37[:, :, CA], diffused, None, None, B, 1, 20, None, False)[0])
    if shape:
        shape_at = sum(c.shape[1] for c in cols)
        cols.append(_dssp_call(atom37, res_mask, None)[1])
    if violations:
        viol_at = sum(c.shape[1] for c in cols)
        cols.append(_violations_call(atom37, res_mask, None, False)[0])
    host = torch.cat(cols, dim=1).cpu()
    rows = []
    for b in range(B):
        v = host[b].tolist()
        row = dict(zip(BACKBONE_SLOTS, v[:len(BACKBONE_SLOTS)]))
        n = row["num_res"]
        row["fixed_residues"] = v[12]
        row["diffused_percentage"] = (n - v[12]) / n if n else float("nan")
        if gt_atom37 is not None:
            row["aligned_rmsd_to_gt"] = v[13 + RMSD_SLOTS.index("mean_dist")]
            if isinstance(tm, str):
                row["tm_align_to_gt"] = v[21 + TM_ALIGN_SLOTS.index("tm_norm_b")]
            elif tm:
                row["tm_score_to_gt"] = v[21 + TM_SLOTS.index("tm_score")]
        if shape:
            row.update({name: v[shape_at + SHAPE_SLOTS.index(name)] for name in SHAPE_COLUMNS})
        if violations:
            row.update({name: v[viol_at + VIOLATION_SLOTS.index(name)] for name in VIOLATION_COLUMNS})
        rows.append(row)
    return rows


def _cluster_operands(mat, present, method, kind, who):
    """(mat addressable in place, present uint8 [G,M] or None, G, M, ld, problem_stride, method code, kind code, batched); every
    refusal is raised here, before anything is launched or copied"""
    if method not in CLUSTER_METHODS:
        raise ValueError(f"{who}: method = {method!r}, expected one of {sorted(CLUSTER_METHODS)}")
    if kind not in CLUSTER_KINDS:
        raise ValueError(f"{who}: kind = {kind!r}, expected one of {sorted(CLUSTER_KINDS)}")
    if mat.dim() not in (2, 3) or mat.shape[-1] != mat.shape[-2]:
        raise ValueError(f"{who}: a matrix of shape {tuple(mat.shape)}: expected [M,M] or [G,M,M]")
    batched = mat.dim() == 3
    if not batched:
        mat = mat[None]
        present = None if present is None else present[None]
    G, M = mat.shape[:2]
    if M > CLUSTER_MAX_M:
        raise ValueError(f"{who}: M = {M} samples, at most {CLUSTER_MAX_M} are supported")
    if present is not None and tuple(present.shape) != (G, M):
        raise ValueError(f"{who}: present of shape {tuple(present.shape)}, expected {(G, M) if batched else (M,)}")
    in_place = mat.dtype == torch.float64 and (M <= 1 or (mat.stride(2) == 1 and mat.stride(1) >= M)) and (G <= 1 or mat.stride(0) >= 0)
    if not in_place:
        mat = mat.to(torch.float64).contiguous()
    if present is not None:
        present = (present != 0).to(torch.uint8).contiguous()
    ld = mat.stride(1) if M > 1 else max(M, 1)
    return mat, present, G, M, ld, (mat.stride(0) if G > 1 else 0), CLUSTER_METHODS[method], CLUSTER_KINDS[kind], batched


def _linkage_call(mat, present, G, M, ld, stride, method, kind):
    dev = mat.device
    Z = torch.empty((G, max(M - 1, 0), 4), dtype=torch.float64, device=dev)
    num = torch.zeros((G,), dtype=torch.int32, device=dev)          # (zeros: nothing is launched for M == 0)
    ws = torch.empty((max(1, G * M * M),), dtype=torch.float64, device=dev)      # FD_CLUSTER_WS_DOUBLES
    hip.get_lib().call("fd_cluster_linkage", mat, ld, stride, present, G, M, kind, method, ws, Z, num)
    return Z, num, ws


def linkage(mat, present=None, method="average", kind="distance"):
    """Agglomerative clustering (fd_cluster_linkage; include/fd_hip.h is the specification) of a float64 matrix mat [M,M] or of G of
    them [G,M,M], read in place at any row and problem stride with unit inner stride; only the strict upper triangle is read.
    kind "distance" or "similarity" (distance = 1 - s); method "single", "average" (UPGMA) or "complete"; present [M] / [G,M]:
    the samples that take part.  dict Z (float64 [G,M-1,4], or [M-1,4]: smaller id, larger id, height, size per merge; leaf ids are
    positions, merge s makes id M + s; rows beyond num_merges hold -1, -1, +inf, 0) and num_merges (int32 [G] or 0-d).  Ties go to
    the smallest (height, smaller id, larger id).  M <= 4096, or ValueError before anything is launched.  One launch, one block
    per matrix, no host synchronisation."""
    mat, present, G, M, ld, stride, method, kind, batched = _cluster_operands(mat, present, method, kind, "linkage")
    Z, num, _ = _linkage_call(mat, present, G, M, ld, stride, method, kind)
    return {"Z": Z if batched else Z[0], "num_merges": num if batched else num[0]}


def cluster(mat, threshold=0.5, method="average", present=None, kind="similarity"):
    """Flat clusters of mat (as linkage takes it) at a threshold: linkage, then fd_cluster_cut.  For kind "similarity" two clusters
    merge while their linkage similarity is >= threshold (the cut is 1 - threshold, inclusive); for "distance" threshold is the
    distance cut itself, inclusive.  dict: labels (int32 [G,M] or [M]: clusters numbered by their smallest member, -1 absent),
    representatives (int32, same shape: the medoid of cluster k at position k -- the member of the largest summed similarity, or
    the smallest summed distance, to the others, the smallest index on ties -- and -1 beyond the last cluster), Z and num_merges
    as linkage returns them, and a float64 tensor [G] (0-d without G) per name of CLUSTER_SLOTS; diversity is num_clusters /
    num_samples, the figure of a sampling run at similarity = TM-score and threshold 0.5.  Agreement with MaxCluster is NOT
    verified (include/fd_hip.h).  Two launches, no host synchronisation."""
    mat, present, G, M, ld, stride, method, kind, batched = _cluster_operands(mat, present, method, kind, "cluster")
    cut = 1.0 - float(threshold) if kind == 1 else float(threshold)
    if cut != cut:
        raise ValueError("cluster: the threshold is NaN")
    dev = mat.device
    Z, num, _ = _linkage_call(mat, present, G, M, ld, stride, method, kind)
    labels = torch.empty((G, M), dtype=torch.int32, device=dev)
    rep = torch.empty((G, M), dtype=torch.int32, device=dev)
    if M == 0:
        # nothing is launched without samples: no clusters, and a mean over nothing is NaN
        out = torch.full((G, 8), float("nan"), dtype=torch.float64, device=dev)
        out[:, [0, 1, 3, 4]] = 0.0
    else:
        out = torch.empty((G, 8), dtype=torch.float64, device=dev)
        hip.get_lib().call("fd_cluster_cut", Z, num, mat, ld, stride, present, G, M, kind, cut, labels, rep, out)
    pick = (lambda x: x) if batched else (lambda x: x[0])
    res = {"labels": pick(labels), "representatives": pick(rep), "Z": pick(Z), "num_merges": pick(num)}
    res.update({name: pick(out[:, k]) for k, name in enumerate(CLUSTER_SLOTS)})
    return res


def diversity(pos, mask=None, threshold=0.5, method="average", tm="given", symmetrize="min"):
    """Diversity of M sampled backbones pos [M,N,3] (mask [M,N]): cluster() of their pairwise TM-scores at `threshold`; the headline
    figure is the returned diversity = num_clusters / num_samples.  tm="given": pairwise_tm(pos, mask), the TM-score under the
    position-to-position correspondence (samples of one length).  tm="align": tm_align_matrix(pos, mask), for chains of different
    lengths (mask marks the padding); its two normalisations are combined elementwise by symmetrize: "min" (the default: the score
    normalised by the longer chain, the conservative choice), "max" or "mean".  Returns cluster's dict plus tm, the matrix that
    was clustered.  No host synchronisation."""
    if tm not in ("given", "align"):
        raise ValueError(f"diversity: tm = {tm!r}, expected 'given' or 'align'")
    if symmetrize not in ("min", "max", "mean"):
        raise ValueError(f"diversity: symmetrize = {symmetrize!r}, expected 'min', 'max' or 'mean'")
    if method not in CLUSTER_METHODS:
        raise ValueError(f"diversity: method = {method!r}, expected one of {sorted(CLUSTER_METHODS)}")
    if pos.dim() != 3 or pos.shape[0] > CLUSTER_MAX_M:
        raise ValueError(f"diversity: points of shape {tuple(pos.shape)}: expected [M,N,3] with M <= {CLUSTER_MAX_M}")
    if tm == "given":
        mat = pairwise_tm(pos, mask)
    else:
        both = tm_align_matrix(pos, mask)
        a, b = both["tm_norm_a"], both["tm_norm_b"]
        mat = torch.minimum(a, b) if symmetrize == "min" else torch.maximum(a, b) if symmetrize == "max" else 0.5 * (a + b)
    res = cluster(mat, threshold=threshold, method=method, kind="similarity")
    res["tm"] = mat
    return res


def novelty(pos, mask, lib_pos, lib_mask):
    """Novelty of M sampled backbones against a structure library: for every sample the highest TM-score, normalised by the sample's
    own length, of tm_align_matrix(pos, mask, lib_pos, lib_mask) over the library's chains.  dict max_tm_to_library (float64 [M]) and
    nearest (int64 [M], the library chain that attains it).  Plain tensor arithmetic on tm_align_matrix's result."""
    if lib_pos.dim() != 3 or lib_pos.shape[0] == 0:
        raise ValueError("novelty: the library is empty")
    best, arg = tm_align_matrix(pos, mask, lib_pos, lib_mask)["tm_norm_a"].max(dim=1)
    return {"max_tm_to_library": best, "nearest": arg}
