"""Chain store: training batches from backbone atoms, built on the device.

The reference's PdbDataset (data/pdb_data_loader.py:133-276) turns one pickled chain at a time into a training example on the
host: du.parse_chain_feats centres it on CA, the OpenFold transforms give frames and torsion angles, a scipy/numpy
forward_marginal noises it, and the DataLoader pads, collates and copies.  Here the chains are packed and uploaded ONCE
(``ChainStore.freeze``), and a batch is two launches on what lies there: fd_chain_batch (include/fd_hip.h: centre, backbone frame,
quaternion, pre-omega / phi / psi, res_mask, seq_idx, padding and the ground-truth backbone atoms of the loss) and the existing
fd_forward_marginal_batch (``SE3Diffuser.forward_marginal_batch``).  Nothing is read back from the device after ``freeze``.

    store = ChainStore("cuda")
    for feats in my_chains:                      # the dicts process_pdb_dataset.py pickles, or atoms [L,4,3] = N, CA, C, O
        store.add(feats)
    store.freeze()
    for batch, gt_atom37 in store.batches(32, 500_000, np.random.default_rng(0), diffuser, with_gt=True):
        loss = dsm_loss(batch, model(batch), gt_atom37)

What the training step reads of a chain is rigids_0, psi, res_mask, fixed_mask, seq_idx, sc_ca_t and the outputs of
forward_marginal (model/score_network.py:201, experiments/train_se3_diffusion.py:561,611-615); that is what a batch holds, under
the keys of the reference's DataLoader (those of ``train_step.synthetic_batch``).

Out of scope: entries of several chains and chain_idx; side-chain torsions and the atom14 arrays; the evaluation branch of
the dataset (t = 1, sample_ref(impute=...)); motif masks (PdbDataset._create_diffused_masks, which its own __getitem__ never
calls: fixed_mask is zero); reading pickles or mmCIF -- ``add`` takes arrays.  PDB files come in through ``pdb.parse_pdb``, which
reads them on the device, and ``add_parsed``, which takes its chain segments where they lie:

    store.add_parsed(pdb.parse_pdb(my_pdb_paths))

The store also keeps the chains' letters (``aatype``, 0 .. 20) beside the atoms, clusters them by sequence on the device
(``sequence_clusters``: se3_diffusion_amd/seqs.py) or takes clusters from elsewhere (``set_clusters``), and plans an epoch in the
reference's four sample modes (``epoch_plan``; config/base.yaml:88 trains with cluster_time_batch):

    store.sequence_clusters(min_identity=0.3, min_coverage=0.8)
    for batch in store.batches(32, 500_000, rng, diffuser, sample_mode="cluster_time_batch"):
        ...

The SEQUENCE of a chain is all of its rows in store order: a gap in the residue numbers is not a gap in the sequence, and rows
without atoms count.

Three deliberate differences from the reference (include/fd_hip.h): res_mask needs N, CA and C, not CA alone; the frame of an
absent residue and of a padding row is the identity at the origin behind res_mask = 0; quaternions have w >= 0.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import hip

_BACKBONE37 = (0, 1, 2, 4)                        # N, CA, C, O in atom37 order (residue_constants.atom_order)
SAMPLE_MODES = ("length_batch", "time_batch", "cluster_length_batch", "cluster_time_batch")
_BATCH_KEYS = ("res_mask", "fixed_mask", "seq_idx", "t", "sc_ca_t", "rigids_t", "rigids_0", "torsion_angles_sin_cos", "rot_score",
               "trans_score", "rot_score_scaling", "trans_score_scaling")


class ChainStore:
    """Backbone atoms of single chains, packed on `device`: atoms [T,4,3] fp32 (N, CA, C, O), atom_mask [T,4] uint8,
    res_index [T] int32, offsets [C+1] int64 -- the operands of fd_chain_windows / fd_chain_batch -- and aatype [T] uint8, the
    letters 0 .. 20 in the reference's restypes order (20 = X), the operand of fd_seq_align."""

    def __init__(self, device):
        self.device = torch.device(device)
        self._pending = []
        self._parsed = []                            # (atoms, atom_mask, res_index on the device, host lengths) per add_parsed call
        self._frozen = False
        self.windows = None
        self.clusters = None                         # host int64 [C] once sequence_clusters / set_clusters has run
        self.cluster_reps = None                     # host int64 [K]: the representative chain of each cluster (None: not known)

    # ------------------------------------------------------------------ building
    def add(self, chain=None, *, atoms=None, atom_mask=None, residue_index=None, aatype=None) -> int:
        """One chain; returns its id.  `chain` is the dict tools of the reference pickle (process_pdb_dataset.py: atom_positions
        [L,37,3], atom_mask [L,37], residue_index [L]; the atom37 columns 0, 1, 2, 4 are taken) or a dict / keywords with atoms
        [L,4,3] = N, CA, C, O, atom_mask [L,4] and residue_index [L] (None: 0 .. L-1).  aatype [L], integers 0 .. 20, is taken from
        the dict where it is there, else from the keyword; a chain added without letters is all X (20) and is remembered as such
        (``has_letters``)."""
        if self._frozen:
            raise RuntimeError("ChainStore.add after freeze()")
        if self._parsed:
            raise RuntimeError("ChainStore.add after add_parsed(): the chains of add come first in the store")
        if chain is not None:
            if "atom_positions" in chain:
                pos, msk = np.asarray(chain["atom_positions"]), np.asarray(chain["atom_mask"])
                if pos.ndim != 3 or pos.shape[1:] != (37, 3) or msk.shape != pos.shape[:2]:
                    raise ValueError(f"expected atom_positions [L,37,3] and atom_mask [L,37], got {pos.shape} and {msk.shape}")
                atoms, atom_mask = pos[:, _BACKBONE37], msk[:, _BACKBONE37]
            else:
                atoms, atom_mask = chain["atoms"], chain["atom_mask"]
            residue_index = chain.get("residue_index", residue_index)
            aatype = chain.get("aatype", aatype)
        atoms = np.asarray(atoms, dtype=np.float32)
        if atoms.ndim != 3 or atoms.shape[1:] != (4, 3):
            raise ValueError(f"expected atoms [L,4,3] (N, CA, C, O), got {atoms.shape}")
        L = atoms.shape[0]
        atom_mask = np.asarray(atom_mask)
        if atom_mask.shape != (L, 4):
            raise ValueError(f"expected atom_mask [{L},4], got {atom_mask.shape}")
        residue_index = np.arange(L) if residue_index is None else np.asarray(residue_index)
        if residue_index.shape != (L,):
            raise ValueError(f"expected residue_index [{L}], got {residue_index.shape}")
        if aatype is None:
            letters = np.full(L, 20, dtype=np.uint8)
        else:
            letters = np.asarray(aatype)
            if letters.shape != (L,):
                raise ValueError(f"expected aatype [{L}], got {letters.shape}")
            if L and (letters.min() < 0 or letters.max() > 20):
                raise ValueError(f"aatype must lie in 0 .. 20, got {letters.min()} .. {letters.max()}")
            letters = letters.astype(np.uint8)
        self._pending.append((atoms, (atom_mask != 0).astype(np.uint8), residue_index.astype(np.int32), letters, aatype is not None))
        return len(self._pending) - 1

    def add_parsed(self, parsed, chains=None) -> list:
        """The chain segments `chains` (indices into `parsed`, a pdb.ParsedPdb on this store's device; None: all of them) as
        chains of the store; returns their ids.  The backbone columns 0, 1, 2, 4 of atom_positions and atom_mask and the residue
        numbers, and parsed.aatype as the letters, are taken from the device arrays as they lie: nothing but the segment table
        (ParsedPdb.host_tables, read once) comes to the host.  freeze() puts these chains behind those of add(), which therefore cannot be called any more."""
        if self._frozen:
            raise RuntimeError("ChainStore.add_parsed after freeze()")
        if parsed.aatype.device.type != self.device.type:
            raise ValueError(f"parsed lies on {parsed.aatype.device}, the store on {self.device}")
        off = parsed.host_tables()[0]
        cols = list(_BACKBONE37)
        chosen = np.arange(len(parsed)) if chains is None else np.asarray(chains, dtype=np.int64).reshape(-1)
        if len(chosen) and (chosen.min() < 0 or chosen.max() >= len(parsed)):
            raise ValueError(f"chain segments must lie in [0, {len(parsed)}), got {chosen.min()} .. {chosen.max()}")
        first = len(self._pending) + sum(len(p[3]) for p in self._parsed)
        if chains is None:
            rows = slice(0, parsed.num_residues)
        else:
            rows = torch.from_numpy(np.concatenate([np.arange(off[c], off[c + 1]) for c in chosen] + [np.zeros(0, np.int64)])
                                    ).to(parsed.aatype.device)
        self._parsed.append((parsed.atom_positions[rows][:, cols].contiguous(), parsed.atom_mask[rows][:, cols].contiguous(),
                             parsed.residue_index[rows].to(torch.int32), (off[chosen + 1] - off[chosen]).astype(np.int64),
                             parsed.aatype[rows].clamp(0, 20).to(torch.uint8)))
        return list(range(first, first + len(chosen)))

    def freeze(self):
        """Pack, upload, run fd_chain_windows and copy its [C,3] table to the host: the one synchronisation of the store."""
        if self._frozen:
            return self
        C = len(self._pending)
        lens = np.array([len(p[0]) for p in self._pending], dtype=np.int64)
        has = np.array([p[4] for p in self._pending], dtype=bool)
        cat = lambda k, shape, dt: (np.concatenate([p[k] for p in self._pending]) if C else np.zeros(shape, dt))
        dev = self.device
        self.atoms = torch.from_numpy(np.ascontiguousarray(cat(0, (0, 4, 3), np.float32))).to(dev)
        self.atom_mask = torch.from_numpy(np.ascontiguousarray(cat(1, (0, 4), np.uint8))).to(dev)
        self.res_index = torch.from_numpy(np.ascontiguousarray(cat(2, (0,), np.int32))).to(dev)
        self.aatype = torch.from_numpy(np.ascontiguousarray(cat(3, (0,), np.uint8))).to(dev)
        if self._parsed:                             # the chains of add_parsed, already on the device, behind those of add
            lens = np.concatenate([lens] + [p[3] for p in self._parsed])
            C = len(lens)
            self.atoms = torch.cat([self.atoms] + [p[0] for p in self._parsed])
            self.atom_mask = torch.cat([self.atom_mask] + [p[1] for p in self._parsed])
            self.res_index = torch.cat([self.res_index] + [p[2] for p in self._parsed])
            self.aatype = torch.cat([self.aatype] + [p[4] for p in self._parsed])
            has = np.concatenate([has, np.ones(C - len(has), dtype=bool)])
        self.has_letters = has                       # host bool [C]: False for a chain that add() got without aatype (all X)
        self.offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)).to(dev)
        self._pending = None
        self._parsed = None
        window = torch.empty((C, 3), dtype=torch.int32, device=dev)
        hip.get_lib().call("fd_chain_windows", self.atoms, self.atom_mask, self.offsets, C, window)
        self._window = window
        self.windows = window.cpu().numpy()        # {first present, last present, number present} per chain
        self._frozen = True
        return self

    def __len__(self):
        if self._frozen:
            return self.windows.shape[0]
        return len(self._pending) + sum(len(p[3]) for p in self._parsed)

    @property
    def lengths(self):
        """host array [C]: residues from the first to the last present one -- the reference's modeled_seq_len; 0 for a chain
        without a present residue"""
        self._need_frozen()
        return (self.windows[:, 1] - self.windows[:, 0] + 1).astype(np.int64)

    def _need_frozen(self):
        if not self._frozen:
            raise RuntimeError("ChainStore: call freeze() first")

    # ------------------------------------------------------------------ batches
    def build_batch(self, ids, n_pad=None, with_gt=True):
        """fd_chain_batch alone: rigids_0 [B,Npad,7], torsion_angles_sin_cos [B,Npad,7,2], res_mask [B,Npad] (fp32), seq_idx
        [B,Npad] (int64) and, with_gt, gt_bb [B,Npad,5,3] (N, CA, C, CB, O of compute_backbone(rigids_0, psi)) of the chains
        `ids` (host integers, repeats allowed), padded to n_pad (None: the longest window among them)."""
        self._need_frozen()
        ids = np.asarray(ids, dtype=np.int64).reshape(-1)
        B, C = len(ids), len(self)
        if B and (ids.min() < 0 or ids.max() >= C):
            raise ValueError(f"chain ids must lie in [0, {C}), got {ids.min()} .. {ids.max()}")
        longest = int(self.lengths[ids].max()) if B else 0
        n_pad = longest if n_pad is None else int(n_pad)
        if n_pad < longest:
            raise ValueError(f"n_pad = {n_pad} is shorter than a window of {longest} residues (chain {int(ids[np.argmax(self.lengths[ids])])})")
        from .. import trunk
        dev = self.device
        out = {"rigids_0": torch.empty((B, n_pad, 7), device=dev), "torsion_angles_sin_cos": torch.empty((B, n_pad, 7, 2), device=dev),
               "res_mask": torch.empty((B, n_pad), device=dev), "seq_idx": torch.empty((B, n_pad), dtype=torch.int64, device=dev)}
        if with_gt:
            out["gt_bb"] = torch.empty((B, n_pad, 5, 3), device=dev)
        dev_ids = torch.from_numpy(ids.astype(np.int32)).to(dev)
        hip.get_lib().call("fd_chain_batch", self.atoms, self.atom_mask, self.res_index, self.offsets, self._window, dev_ids, B, n_pad,
                           trunk.head_const(), out["rigids_0"], out["torsion_angles_sin_cos"], out["res_mask"], out["seq_idx"],
                           out.get("gt_bb"))
        return out

    def training_batch(self, ids, diffuser, t=None, n_pad=None, noise=None, generator=None, rng=None, min_t=0.01):
        """(batch, gt_atom37) for the chains `ids`: fd_chain_batch, then diffuser.forward_marginal_batch(rigids_0, t,
        diffuse_mask=res_mask, noise=, generator=) as it stands (its kernel copies the frame and writes zero scores where the mask
        is 0).  batch has the keys, dtypes and shapes of train_step.synthetic_batch; fixed_mask and sc_ca_t are zero.  t [B]
        defaults to rng.uniform(min_t, 1) per entry (pdb_data_loader.py:252; data.min_t = 0.01 in config/base.yaml) -- the same id
        repeated with different t is the reference's time_batch mode.  gt_atom37 [B,Npad,37,3] holds the five backbone atoms of
        compute_backbone(rigids_0, psi), atoms 5..36 zero."""
        built = self.build_batch(ids, n_pad)
        B, N = built["res_mask"].shape
        if t is None:
            rng = np.random.default_rng() if rng is None else rng
            t = rng.uniform(min_t, 1.0, size=B)
        t = np.asarray(t, dtype=np.float64).reshape(B)
        dev = self.device
        noised = diffuser.forward_marginal_batch(built["rigids_0"], t, diffuse_mask=built["res_mask"], noise=noise, generator=generator)
        values = dict(built, fixed_mask=torch.zeros((B, N), device=dev), t=torch.tensor(t, dtype=torch.float32, device=dev),
                      sc_ca_t=torch.zeros((B, N, 3), device=dev), **noised)
        gt_atom37 = torch.zeros((B, N, 37, 3), device=dev)
        gt_atom37[:, :, :5] = built["gt_bb"]
        return {k: values[k] for k in _BATCH_KEYS}, gt_atom37

    def batch_plan(self, batch_size, max_squared_res, rng):
        """One pass over the store in the reference's length_batch mode, as host arithmetic on `lengths`: a list of id arrays, each
        of ONE length N and of at most min(batch_size, max_squared_res // N^2) chains (du.length_batching, data/utils.py:387-399),
        every chain of a length in exactly one of them, chains and batches in an order drawn from rng.  Chains without a present
        residue, and lengths with N^2 > max_squared_res, are left out."""
        lengths = self.lengths
        plan = []
        for n in np.unique(lengths[lengths > 0]):
            b = min(int(batch_size), int(max_squared_res) // int(n * n))
            if b < 1:
                continue
            ids = rng.permutation(np.flatnonzero(lengths == n))
            plan += [ids[k:k + b] for k in range(0, len(ids), b)]
        return [plan[k] for k in rng.permutation(len(plan))]

    # ------------------------------------------------------------------ clusters
    def sequence_clusters(self, min_identity=0.3, min_coverage=0.8, subst=None, gap_open=11, gap_extend=1):
        """Cluster the chains by sequence on the device (seqs.cluster_sequences on aatype and offsets as they lie: all pairs
        aligned, length-ordered greedy clustering).  Sets and returns ``clusters``, host int64 [C], numbered by ascending
        smallest member; ``cluster_reps`` [K] holds each cluster's representative, its longest chain.  Raises if a chain was
        added without letters."""
        self._need_frozen()
        if not self.has_letters.all():
            missing = np.flatnonzero(~self.has_letters)
            raise ValueError(f"ChainStore.sequence_clusters: {len(missing)} chains were added without aatype (the first: chain "
                             f"{int(missing[0])}); give add() the letters, or set_clusters() the clusters")
        from .. import seqs
        self.clusters, self.cluster_reps = seqs.cluster_sequences((self.aatype, self.offsets), min_identity, min_coverage, subst,
                                                                  gap_open, gap_extend)
        return self.clusters

    def set_clusters(self, labels):
        """Clusters from elsewhere: labels [C], any integers (equal label = same cluster), e.g. seqs.read_clusters(path) mapped
        over the caller's chain names.  Sets ``clusters``; ``cluster_reps`` is then None."""
        self._need_frozen()
        labels = np.asarray(labels)
        if labels.shape != (len(self),) or not np.issubdtype(labels.dtype, np.integer):
            raise ValueError(f"expected {len(self)} integer cluster labels, got {labels.dtype} {labels.shape}")
        self.clusters, self.cluster_reps = labels.astype(np.int64), None
        return self.clusters

    def epoch_plan(self, sample_mode, batch_size, max_squared_res, rng):
        """One epoch in one of the reference's sample modes (TrainSampler.__iter__, data/pdb_data_loader.py:328-352) as a list of
        id arrays for training_batch.  In every mode a batch of chains of length N has b = min(batch_size, max_squared_res // N^2)
        entries (what du.length_batching cuts the reference's batches to); chains without a present residue or with b < 1 are
        left out.
          'length_batch'          exactly batch_plan(batch_size, max_squared_res, rng)
          'time_batch'            the chains in rng.permutation order, each one batch of b copies of its id (training_batch then
                                  draws b different t)
          'cluster_time_batch'    one member drawn uniformly from every cluster, then as time_batch over those members
          'cluster_length_batch'  one member drawn from every cluster; per distinct length among the draws one batch of b draws
                                  WITH replacement among the drawn members of that length; the batches in rng order
        The cluster modes need ``clusters``.  Two differences from the reference: the random stream is rng's, not that of pandas'
        sample(random_state=epoch); and the clusters' members come in a shuffled order, where the reference's
        cluster_time_batch leaves them in pandas' group order."""
        if sample_mode not in SAMPLE_MODES:
            raise ValueError(f"Invalid sample mode: {sample_mode!r}; expected one of {SAMPLE_MODES}")
        if sample_mode == "length_batch":
            return self.batch_plan(batch_size, max_squared_res, rng)
        lengths = self.lengths
        cap = lambda n: min(int(batch_size), int(max_squared_res) // int(n * n)) if n > 0 else 0
        if sample_mode == "time_batch":
            members = np.arange(len(self))
        else:
            if self.clusters is None:
                raise RuntimeError(f"ChainStore.epoch_plan({sample_mode!r}): no clusters; call sequence_clusters() or set_clusters()")
            order = np.argsort(self.clusters, kind="stable")             # the members of a cluster, ascending, side by side
            first = np.flatnonzero(np.diff(self.clusters[order], prepend=self.clusters[order[0]] - 1)) if len(order) else order
            sizes = np.diff(np.append(first, len(order)))
            members = order[first + rng.integers(0, sizes)] if len(order) else order
        if sample_mode in ("time_batch", "cluster_time_batch"):
            members = members[rng.permutation(len(members))]
            return [np.full(cap(lengths[c]), c, dtype=np.int64) for c in members if cap(lengths[c]) >= 1]
        plan = []
        for n in np.unique(lengths[members]):
            if cap(n) >= 1:
                plan.append(rng.choice(members[lengths[members] == n], size=cap(n), replace=True).astype(np.int64))
        return [plan[k] for k in rng.permutation(len(plan))]

    def batches(self, batch_size, max_squared_res, rng, diffuser, with_gt=False, min_t=0.01, generator=None, sample_mode=None):
        """Iterator over one pass of batch_plan(batch_size, max_squared_res, rng) -- or, with sample_mode, of
        epoch_plan(sample_mode, ..) --: device dicts as training_batch returns them (what
        the reference's train_epoch reads from its DataLoader; its .to(device) is then a no-op), or (batch, gt_atom37) pairs
        with_gt.  t comes from the same rng, so a seeded rng fixes the whole sequence but for the noise (generator)."""
        plan = (self.batch_plan(batch_size, max_squared_res, rng) if sample_mode is None
                else self.epoch_plan(sample_mode, batch_size, max_squared_res, rng))
        for ids in plan:
            batch, gt = self.training_batch(ids, diffuser, rng=rng, min_t=min_t, generator=generator)
            yield (batch, gt) if with_gt else batch
