"""Sequence alignment and clustering on the device (csrc/fd_seq.hip: fd_seq_align, fd_seq_greedy).

The reference samples one chain per 30 %-identity sequence cluster per epoch (data/pdb_data_loader.py:279-354, sample_mode
cluster_time_batch) and takes the clusters from RCSB's clusters-by-entity-30.txt.  A set of one's own chains -- designs, domains,
predictions -- has no such file; this module makes the clusters from the sequences:

    letters, offsets = seqs.pack(["MKV...", "MRV...", ...])
    labels, reps = seqs.cluster_sequences((letters, offsets), min_identity=0.3, min_coverage=0.8)

  align             Gotoh local alignment (affine gaps) of a rectangle of chain pairs: score, matches, columns and the two
                    ranges of every pair, one wave per pair, nothing but the [Pa,Pb,8] result in memory
  relation          align over tiles of the upper triangle, thresholded into a symmetric uint8 [C,C]
  greedy_clusters   length-ordered greedy clustering of such a matrix (CD-HIT's scheme, MMseqs2's cluster-mode 2)
  cluster_sequences the three in a row
  identity_matrix   matches / columns of a rectangle, e.g. among the sequences SequenceDesigner.design returns

ALL pairs are aligned: there is no k-mer prefilter, so the cost is quadratic in the number of chains (profiles/
seq_cluster_cost.txt), and `relation` holds C^2 bytes on the device -- 400 MB at 20,000 chains, which is the memory limit of
this path; the alignment results themselves exist one tile at a time (tile^2 x 32 bytes).

Checked against: a literal pure-Python restatement of the recurrence in include/fd_hip.h and of the greedy walk, with ==
(tests/test_seq_cluster.py).  NOT checked against: MMseqs2, CD-HIT or any other aligner or clusterer (none exists where this
project is built); RCSB's cluster files were never reproduced -- their clusters come from MMseqs2 with its own prefilter,
scoring and coverage rules, and these clusters will differ from them.

BLOSUM62 below was typed from memory: neither the repository nor the machines it is built on hold a copy of the published
matrix.  It was NOT compared with NCBI's file.  What the tests vouch for is that it is symmetric, that every diagonal entry is
positive, that W-W = 11 is its largest entry and C-C = 9 the second largest.  Letter 20 (X) scores -1 against everything, itself
included: that is this module's choice.  A caller who has the file passes their own table as `subst`.
"""
from __future__ import annotations

import numpy as np
import torch

from . import hip

ALPHABET = "ARNDCQEGHILKMFPSTWYVX"           # residue_constants.restypes + X
LETTERS = 21                                  # include/fd_hip.h FD_SEQ_LETTERS
MAX_L = 2048                                  # include/fd_hip.h FD_SEQ_MAX_L
SLOTS = 8                                     # include/fd_hip.h FD_SEQ_SLOTS
MAX_SCORE = 127                               # include/fd_hip.h FD_SEQ_MAX_SCORE
MAX_GAP = 1023                                # include/fd_hip.h FD_SEQ_MAX_GAP
SCORE, MATCHES, COLUMNS, A_BEGIN, A_END, B_BEGIN, B_END = range(7)

_BLOSUM62_ROWS = """
 4 -1 -2 -2  0 -1 -1  0 -2 -1 -1 -1 -1 -2 -1  1  0 -3 -2  0
-1  5  0 -2 -3  1  0 -2  0 -3 -2  2 -1 -3 -2 -1 -1 -3 -2 -3
-2  0  6  1 -3  0  0  0  1 -3 -3  0 -2 -3 -2  1  0 -4 -2 -3
-2 -2  1  6 -3  0  2 -1 -1 -3 -4 -1 -3 -3 -1  0 -1 -4 -3 -3
 0 -3 -3 -3  9 -3 -4 -3 -3 -1 -1 -3 -1 -2 -3 -1 -1 -2 -2 -1
-1  1  0  0 -3  5  2 -2  0 -3 -2  1  0 -3 -1  0 -1 -2 -1 -2
-1  0  0  2 -4  2  5 -2  0 -3 -3  1 -2 -3 -1  0 -1 -3 -2 -2
 0 -2  0 -1 -3 -2 -2  6 -2 -4 -4 -2 -3 -3 -2  0 -2 -2 -3 -3
-2  0  1 -1 -3  0  0 -2  8 -3 -3 -1 -2 -1 -2 -1 -2 -2  2 -3
-1 -3 -3 -3 -1 -3 -3 -4 -3  4  2 -3  1  0 -3 -2 -1 -3 -1  3
-1 -2 -3 -4 -1 -2 -3 -4 -3  2  4 -2  2  0 -3 -2 -1 -2 -1  1
-1  2  0 -1 -3  1  1 -2 -1 -3 -2  5 -1 -3 -1  0 -1 -3 -2 -2
-1 -1 -2 -3 -1  0 -2 -3 -2  1  2 -1  5  0 -2 -1 -1 -1 -1  1
-2 -3 -3 -3 -2 -3 -3 -3 -1  0  0 -3  0  6 -4 -2 -2  1  3 -1
-1 -2 -2 -1 -3 -1 -1 -2 -2 -3 -3 -1 -2 -4  7 -1 -1 -4 -3 -2
 1 -1  1  0 -1  0  0  0 -1 -2 -2  0 -1 -2 -1  4  1 -3 -2 -2
 0 -1  0 -1 -1 -1 -1 -2 -2 -1 -1 -1 -1 -2 -1  1  5 -2 -2  0
-3 -3 -4 -4 -2 -2 -3 -2 -2 -3 -2 -3 -1  1 -4 -3 -2 11  2 -3
-2 -2 -2 -3 -2 -1 -2 -3  2 -1 -1 -2 -1  3 -3 -2 -2  2  7 -1
 0 -3 -3 -3 -1 -2 -2 -3 -3  3  1 -2  1 -1 -2 -2  0 -3 -1  4
"""


def _blosum62():
    t = np.full((LETTERS, LETTERS), -1, dtype=np.int32)
    t[:20, :20] = np.array(_BLOSUM62_ROWS.split(), dtype=np.int32).reshape(20, 20)
    t.setflags(write=False)
    return t


BLOSUM62 = _blosum62()                        # [21,21] int32, typed from memory, NOT compared with NCBI's file (module text)


def substitution(match, mismatch, x=-1):
    """A [21,21] int32 table: `match` on the diagonal of the twenty residues, `mismatch` off it, `x` wherever letter 20 (X)
    takes part -- X against X included."""
    t = np.full((LETTERS, LETTERS), int(mismatch), dtype=np.int32)
    t[np.arange(20), np.arange(20)] = int(match)
    t[20, :] = int(x)
    t[:, 20] = int(x)
    return t


def _device(x=None):
    lib = hip.get_lib()
    if isinstance(x, torch.Tensor) and (x.is_cuda or not lib.is_device):
        return x.device
    return torch.device("cuda", torch.cuda.current_device()) if lib.is_device else torch.device("cpu")


def pack(seqs, device=None):
    """(letters [T] uint8, offsets [C+1] int64) on the device from a list of sequences: strings over ARNDCQEGHILKMFPSTWYVX or
    integer arrays 0 .. 20 (aatype).  The ChainStore layout; an empty sequence is allowed."""
    rows = []
    for k, s in enumerate(seqs):
        if isinstance(s, str):
            a = np.frombuffer(s.encode("latin-1", "replace"), dtype=np.uint8)
            lut = np.full(256, 255, dtype=np.int64)
            lut[np.frombuffer(ALPHABET.encode(), dtype=np.uint8)] = np.arange(LETTERS)
            a = lut[a]
            if (a == 255).any():
                raise ValueError(f"sequence {k}: letter {s[int(np.argmax(a == 255))]!r} is not one of {ALPHABET}")
        else:
            a = (s.detach().cpu().numpy() if isinstance(s, torch.Tensor) else np.asarray(s)).reshape(-1).astype(np.int64)
            if len(a) and (a.min() < 0 or a.max() >= LETTERS):
                raise ValueError(f"sequence {k}: letters must lie in 0 .. 20, got {a.min()} .. {a.max()}")
        rows.append(a.astype(np.uint8))
    lens = np.array([len(a) for a in rows], dtype=np.int64)
    dev = _device() if device is None else torch.device(device)
    letters = torch.from_numpy(np.concatenate(rows + [np.zeros(0, np.uint8)])).to(dev)
    offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)).to(dev)
    return letters, offsets


def _table(subst, dev):
    t = BLOSUM62 if subst is None else subst
    t = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    if t.shape != (LETTERS, LETTERS):
        raise ValueError(f"expected a substitution table [21,21], got {t.shape}")
    if not np.issubdtype(t.dtype, np.integer):
        if not (t == np.round(t)).all():
            raise ValueError("the substitution table must hold integers")
    if np.abs(t).max() > MAX_SCORE:
        raise ValueError(f"substitution table entries must lie in -{MAX_SCORE} .. {MAX_SCORE}, got {t.min()} .. {t.max()}")
    return torch.from_numpy(np.ascontiguousarray(t.astype(np.int32))).to(dev)


def _check_gaps(gap_open, gap_extend):
    if not 0 <= int(gap_open) <= MAX_GAP:
        raise ValueError(f"gap_open must lie in 0 .. {MAX_GAP}, got {gap_open}")
    if not 1 <= int(gap_extend) <= MAX_GAP:
        raise ValueError(f"gap_extend must lie in 1 .. {MAX_GAP}, got {gap_extend}")


def _check_packed(letters, offsets):
    """host lengths [C] of a packed set whose letters are 0 .. 20 (one read-back of offsets and of the largest letter)"""
    if letters.dtype != torch.uint8 or offsets.dtype != torch.int64 or letters.dim() != 1 or offsets.dim() != 1 or len(offsets) < 1:
        raise ValueError("expected letters [T] uint8 and offsets [C+1] int64 (seqs.pack)")
    off = offsets.cpu().numpy()
    if off[0] != 0 or (np.diff(off) < 0).any() or off[-1] != len(letters):
        raise ValueError("offsets must start at 0, not decrease and end at len(letters)")
    if len(letters) and int(letters.max()) >= LETTERS:
        raise ValueError(f"letters must lie in 0 .. 20, got {int(letters.max())}")
    return np.diff(off)


def _ids(ids, C, dev, what):
    a = (ids.detach().cpu().numpy() if isinstance(ids, torch.Tensor) else np.asarray(ids)).reshape(-1).astype(np.int64)
    if len(a) and (a.min() < 0 or a.max() >= C):
        raise ValueError(f"{what} must lie in [0, {C}), got {a.min()} .. {a.max()}")
    return a, torch.from_numpy(a.astype(np.int32)).to(dev)


def _launch_align(letters, offsets, C, dev_a, dev_b, table, gap_open, gap_extend, upper_only):
    out = torch.empty((len(dev_a), len(dev_b), SLOTS), dtype=torch.int32, device=letters.device)
    hip.get_lib().call("fd_seq_align", letters, offsets, C, dev_a, len(dev_a), dev_b, len(dev_b), table, int(gap_open), int(gap_extend),
                       1 if upper_only else 0, out)
    return out


def align(letters, offsets, ids_a, ids_b, subst=None, gap_open=11, gap_extend=1, upper_only=False):
    """fd_seq_align on the rectangle ids_a x ids_b of a packed set: int32 [Pa,Pb,8] on the device = score, matches, columns,
    a_begin, a_end, b_begin, b_end, 0 (positions from 0, inclusive; -1 where the score is 0) of the local alignment of x = chain
    ids_a[ia] with y = chain ids_b[ib] under subst[letter of x][letter of y] and gap cost gap_open + k gap_extend.  The tie rules
    of include/fd_hip.h are not symmetric: align(a, b) is not the transpose of align(b, a).  upper_only: entries with
    ids_a[ia] >= ids_b[ib] are skipped and hold -1."""
    _check_gaps(gap_open, gap_extend)
    lens = _check_packed(letters, offsets)
    C, dev = len(lens), letters.device
    table = _table(subst, dev)
    a, dev_a = _ids(ids_a, C, dev, "ids_a")
    b, dev_b = _ids(ids_b, C, dev, "ids_b")
    for ids in (a, b):
        if len(ids) and lens[ids].max() > MAX_L:
            c = int(ids[np.argmax(lens[ids])])
            raise ValueError(f"chain {c} has {int(lens[c])} residues, more than the {MAX_L} an alignment takes")
    return _launch_align(letters, offsets, C, dev_a, dev_b, table, gap_open, gap_extend, upper_only)


def _check_thresholds(min_identity, min_coverage):
    for name, v in (("min_identity", min_identity), ("min_coverage", min_coverage)):
        if not 0.0 <= float(v) <= 1.0:
            raise ValueError(f"{name} must lie in [0, 1], got {v}")


def relation(letters, offsets, subst=None, min_identity=0.3, min_coverage=0.8, gap_open=11, gap_extend=1, tile=2048):
    """The symmetric relation matrix uint8 [C,C] of a packed set, on the device: chains i < j are related iff the alignment of
    x = chain i with y = chain j (x is ALWAYS the chain of the lower id) has columns > 0, matches / columns >= min_identity and
    min((a_end - a_begin + 1) / m, (b_end - b_begin + 1) / n) >= min_coverage, the quotients in float64.  The diagonal is 0.
    The upper triangle is aligned in tiles of `tile` x `tile` pairs, each thresholded with torch ops before the next is made,
    so only tile^2 x 32 bytes of alignment results exist at a time; the C^2 bytes of the result are what limits C."""
    _check_gaps(gap_open, gap_extend)
    _check_thresholds(min_identity, min_coverage)
    lens = _check_packed(letters, offsets)
    if len(lens) and lens.max() > MAX_L:
        c = int(np.argmax(lens))
        raise ValueError(f"chain {c} has {int(lens[c])} residues, more than the {MAX_L} an alignment takes")
    tile = int(tile)
    if tile < 1:
        raise ValueError(f"tile must be at least 1, got {tile}")
    C, dev = len(lens), letters.device
    table = _table(subst, dev)
    rel = torch.zeros((C, C), dtype=torch.uint8, device=dev)
    ids = torch.arange(C, dtype=torch.int32, device=dev)
    dlen = torch.from_numpy(lens.astype(np.float64)).to(dev)
    for a0 in range(0, C, tile):
        a1 = min(C, a0 + tile)
        for b0 in range(a0, C, tile):
            b1 = min(C, b0 + tile)
            out = _launch_align(letters, offsets, C, ids[a0:a1], ids[b0:b1], table, gap_open, gap_extend, True)
            cols = out[..., COLUMNS].to(torch.float64)
            ident = out[..., MATCHES].to(torch.float64) / cols
            cov_a = (out[..., A_END] - out[..., A_BEGIN] + 1).to(torch.float64) / dlen[a0:a1, None]
            cov_b = (out[..., B_END] - out[..., B_BEGIN] + 1).to(torch.float64) / dlen[None, b0:b1]
            r = ((out[..., COLUMNS] > 0) & (ident >= float(min_identity)) & (torch.minimum(cov_a, cov_b) >= float(min_coverage))
                 ).to(torch.uint8)
            rel[a0:a1, b0:b1] |= r
            rel[b0:b1, a0:a1] |= r.T
    return rel


def greedy_clusters(rel, lengths):
    """fd_seq_greedy on a relation matrix uint8 [C,C] (or [C,ld], ld >= C; only rel[min(i,j)][max(i,j)], i != j, is read) where
    it lies: the chains are walked from the longest to the shortest (`lengths`, host [C]; the lower id first among equals), an
    unlabelled chain founds a cluster and takes every unlabelled chain related to it, and the clusters are numbered by ascending
    smallest member.  Returns (labels [C] int32, rep [K] int32 -- the founders -- on the device, and the counts
    {"chains", "clusters", "largest"} from the one read-back)."""
    if rel.dtype != torch.uint8 or rel.dim() != 2 or rel.shape[1] < rel.shape[0] or rel.stride(1) != 1:
        raise ValueError(f"expected a relation matrix uint8 [C,ld >= C] with contiguous rows, got {rel.dtype} {tuple(rel.shape)}")
    C, dev = rel.shape[0], rel.device
    lengths = (lengths.detach().cpu().numpy() if isinstance(lengths, torch.Tensor) else np.asarray(lengths)).reshape(-1)
    if len(lengths) != C:
        raise ValueError(f"expected {C} lengths, got {len(lengths)}")
    order = np.lexsort((np.arange(C), -lengths.astype(np.int64))).astype(np.int32)
    labels = torch.empty(C, dtype=torch.int32, device=dev)
    rep = torch.empty(C, dtype=torch.int32, device=dev)
    if C == 0:
        return labels, rep, {"chains": 0, "clusters": 0, "largest": 0}
    out = torch.empty(4, dtype=torch.int32, device=dev)
    ws = torch.empty(2 * C, dtype=torch.int32, device=dev)
    hip.get_lib().call("fd_seq_greedy", rel, rel.stride(0), C, torch.from_numpy(order).to(dev), ws, labels, rep, out)
    n, K, largest, _ = (int(v) for v in out.cpu())
    return labels, rep[:K], {"chains": n, "clusters": K, "largest": largest}


def _packed(seqs_or_packed):
    if isinstance(seqs_or_packed, tuple) and len(seqs_or_packed) == 2 and isinstance(seqs_or_packed[0], torch.Tensor) \
            and seqs_or_packed[0].dtype == torch.uint8:
        return seqs_or_packed
    return pack(seqs_or_packed)


def cluster_sequences(seqs_or_packed, min_identity=0.3, min_coverage=0.8, subst=None, gap_open=11, gap_extend=1, tile=2048):
    """relation, then greedy_clusters, of a list of sequences (what pack takes) or of pack's (letters, offsets): host arrays
    (labels [C] int64, reps [K] int64), labels[c] = the cluster of chain c, numbered by ascending smallest member, reps[k] = the
    representative of cluster k: its longest chain, the lowest id among equals."""
    letters, offsets = _packed(seqs_or_packed)
    rel = relation(letters, offsets, subst, min_identity, min_coverage, gap_open, gap_extend, tile)
    labels, rep, _ = greedy_clusters(rel, np.diff(offsets.cpu().numpy()))
    return labels.cpu().numpy().astype(np.int64), rep.cpu().numpy().astype(np.int64)


def identity_matrix(seqs_or_packed, ids_a=None, ids_b=None, subst=None, gap_open=11, gap_extend=1):
    """matches / columns of the local alignments of ids_a x ids_b (None: all chains) as float64 [Pa,Pb] on the device; 0 where
    nothing aligns.  Entry (ia, ib) aligns x = chain ids_a[ia] with y = chain ids_b[ib], so the matrix of a set against itself
    need not be symmetric to the last pair where optimal alignments tie.  The chains may differ in length: designs against a
    native, for example."""
    letters, offsets = _packed(seqs_or_packed)
    C = len(offsets) - 1
    out = align(letters, offsets, np.arange(C) if ids_a is None else ids_a, np.arange(C) if ids_b is None else ids_b, subst,
                gap_open, gap_extend)
    cols = out[..., COLUMNS]
    return torch.where(cols > 0, out[..., MATCHES].to(torch.float64) / cols.clamp(min=1).to(torch.float64),
                       torch.zeros((), dtype=torch.float64, device=out.device))


def read_clusters(path):
    """{name: cluster} from a cluster file under the rules of the reference's TrainSampler._read_clusters
    (data/pdb_data_loader.py:319-326): the line number, from 0, is the cluster; a line's tokens are split on single spaces; of a
    token the part in front of the first '_' (RCSB writes 1ABC_1) is the name, upper-cased.  A name on several lines keeps the
    last.  The line's end is stripped and empty tokens are passed over, which the reference leaves in its table as names no
    chain has."""
    table = {}
    with open(path, "r") as f:
        for i, line in enumerate(f):
            for token in line.rstrip("\r\n").split(" "):
                if token:
                    table[token.split("_")[0].upper()] = i
    return table
