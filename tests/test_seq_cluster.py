"""se3_diffusion_amd.seqs and the cluster sampling of ChainStore: local alignment of sequence pairs (csrc/fd_seq.hip, fd_seq_align)
and length-ordered greedy clustering (fd_seq_greedy) on the device.

Every comparison is ==.  The reference is a pure-Python restatement, written from the specification in include/fd_hip.h: ref_align()
carries the tuple (score, matches, columns, i0, j0) through Gotoh's three matrices cell by cell with the tie rules spelled out,
ref_related() thresholds its results with Python floats, ref_greedy() walks the chains.  It shares nothing with the kernel, which
walks anti-diagonals with packed registers.  No other aligner or clusterer exists where this project is built: nothing here is
compared with MMseqs2, CD-HIT or RCSB's cluster files, and BLOSUM62 is only checked for the properties its module vouches for.
Every case runs on the interpreter and, marked gpu, on the device.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from se3_diffusion_amd import hip, pdb, seqs  # noqa: E402
from se3_diffusion_amd.data.chains import ChainStore  # noqa: E402

MAX_L = 2048                                # FD_SEQ_MAX_L
EMPTY_ROW = [0, 0, 0, -1, -1, -1, -1, 0]


@pytest.fixture(params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def dev(request):
    """the device the library under test runs on: the interpreter build on the CPU, or the product library on the GPU"""
    if request.param == "emu":
        request.getfixturevalue("use_emu")
        return "cpu"
    request.getfixturevalue("hip_lib")
    return "cuda"


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
EMPTY = (0, 0, 0, -1, -1)                   # score, matches, columns, i0, j0 of an empty cell


def ref_align(x, y, S, gap_open, gap_extend):
    """the output row of fd_seq_align for x, y (integer letters) -- the recurrence of include/fd_hip.h, literally"""
    m, n = len(x), len(y)
    best, best_at = EMPTY, (-1, -1)
    H_up = [EMPTY] * n                      # H(i-1, .)
    F_up = [None] * n                       # F(i-1, .); None: absent
    for i in range(m):
        H_row, F_row = [None] * n, [None] * n
        E = None                            # E(i, j-1)
        for j in range(n):
            H_left = H_row[j - 1] if j > 0 else EMPTY
            H_diag = H_up[j - 1] if i > 0 and j > 0 else EMPTY
            H_above = H_up[j] if i > 0 else EMPTY
            F_above = F_up[j] if i > 0 else None
            # E: a gap that consumes y_j
            opening = (H_left[0] - gap_open - gap_extend,) + H_left[1:]
            chosen = opening
            if E is not None:
                extension = (E[0] - gap_extend,) + E[1:]
                if extension[0] >= opening[0]:
                    chosen = extension
            E = (chosen[0], chosen[1], chosen[2] + 1, chosen[3], chosen[4])
            # F: a gap that consumes x_i
            opening = (H_above[0] - gap_open - gap_extend,) + H_above[1:]
            chosen = opening
            if F_above is not None:
                extension = (F_above[0] - gap_extend,) + F_above[1:]
                if extension[0] >= opening[0]:
                    chosen = extension
            F = (chosen[0], chosen[1], chosen[2] + 1, chosen[3], chosen[4])
            # D
            start = (H_diag[3], H_diag[4]) if H_diag[0] > 0 else (i, j)
            D = (H_diag[0] + int(S[x[i]][y[j]]), H_diag[1] + (1 if x[i] == y[j] else 0), H_diag[2] + 1, start[0], start[1])
            # H: D over E over F
            H = D
            if E[0] > H[0]:
                H = E
            if F[0] > H[0]:
                H = F
            if H[0] <= 0:
                H = EMPTY
            H_row[j], F_row[j] = H, F
            if H[0] > best[0]:              # (i, then j, ascending: the first of equal scores stays)
                best, best_at = H, (i, j)
        H_up, F_up = H_row, F_row
    if best[0] == 0:
        return list(EMPTY_ROW)
    return [best[0], best[1], best[2], best[3], best_at[0], best[4], best_at[1], 0]


def ref_related(row, m, n, min_identity, min_coverage):
    score, matches, columns, a0, a1, b0, b1, _ = row
    return columns > 0 and matches / columns >= min_identity and min((a1 - a0 + 1) / m, (b1 - b0 + 1) / n) >= min_coverage


def ref_greedy(related, lengths):
    """(labels, reps, largest) of the greedy walk from the longest chain to the shortest; related(i, j) is asked for i < j"""
    C = len(lengths)
    order = sorted(range(C), key=lambda c: (-lengths[c], c))
    return ref_greedy_order(related, order, C)


def ref_greedy_order(related, order, C):
    founder = [-1] * C
    for c in order:
        if founder[c] != -1:
            continue
        for j in range(C):
            if founder[j] == -1 and (j == c or related(min(c, j), max(c, j))):
                founder[j] = c
    number, reps, sizes = {}, [], []
    for j in range(C):
        if founder[j] not in number:
            number[founder[j]] = len(reps)
            reps.append(founder[j])
            sizes.append(0)
        sizes[number[founder[j]]] += 1
    return [number[f] for f in founder], reps, max(sizes) if sizes else 0


# ---- the set of test 1 -------------------------------------------------------------------------------------------------------------
def _mutant(rng, parent, rate):
    out = []
    for a in parent:
        if rng.random() < 0.025:            # 5 % indels: half deletions, half insertions
            continue
        if rng.random() < 0.025:
            out.append(int(rng.integers(0, 20)))
        out.append(int(rng.integers(0, 20)) if rng.random() < rate else int(a))
    return out


@functools.lru_cache(None)
def chains():
    rng = np.random.default_rng(20240607)
    out = []
    for _ in range(4):                      # four families: a parent and five mutants
        parent = [int(a) for a in rng.integers(0, 20, size=int(rng.integers(30, 71)))]
        out.append(parent)
        out += [_mutant(rng, parent, rate) for rate in (0.1, 0.3, 0.5, 0.7, 0.9)]
    out.append([7])                                              # one residue
    out.append([20] * 23)                                        # all X
    out.append(list(out[0][:17]))                                # a prefix
    out.append(list(out[6][9:31]))                               # an inner substring
    out.append(list(out[12]))                                    # two identical chains
    out.append([0] * 40)                                         # low complexity: many optimal alignments, the tie rules decide
    out.append([0] * 25)
    out.append([0, 4] * 19)
    for n in (63, 64, 65, 128, 129):                             # strip and lane boundaries
        base = out[18] * 5
        out.append([int(a) for a in np.where(rng.random(n) < 0.2, rng.integers(0, 20, size=n), np.array(base[:n]))])
    return tuple(tuple(c) for c in out)


def _random_table(rng, symmetric):
    t = rng.integers(-4, 5, size=(21, 21))
    if symmetric:
        t = np.triu(t) + np.triu(t, 1).T
    t[np.arange(21), np.arange(21)] = rng.integers(3, 10, size=21)
    return t.astype(np.int32)


@functools.lru_cache(None)
def tables():
    rng = np.random.default_rng(7)
    return {"symmetric": (_random_table(rng, True), 11, 1), "asymmetric": (_random_table(rng, False), 11, 1),
            "unit": (seqs.substitution(1, -1), 0, 1)}


@functools.lru_cache(None)
def ref_all_pairs(name):
    """{(i, j): row} for all i < j of the set under a table -- computed once, shared, never changed"""
    S, go, ge = tables()[name]
    cs = chains()
    return {(i, j): tuple(ref_align(cs[i], cs[j], S, go, ge)) for i in range(len(cs)) for j in range(i + 1, len(cs))}


def _packed(dev, cs=None):
    return seqs.pack([np.array(c, dtype=np.int64) for c in (chains() if cs is None else cs)], device=dev)


# ---- 1. alignment against the literal restatement ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["symmetric", "asymmetric", "unit"])
def test_align_all_pairs(dev, name):
    S, go, ge = tables()[name]
    letters, offsets = _packed(dev)
    C = len(chains())
    assert C >= 30
    ids = np.arange(C)
    out = seqs.align(letters, offsets, ids, ids, S, go, ge, upper_only=True).cpu().numpy()
    ref = ref_all_pairs(name)
    for i in range(C):
        for j in range(C):
            want = list(ref[(i, j)]) if i < j else [-1] * 8
            assert out[i, j].tolist() == want, (name, i, j, out[i, j].tolist(), want)


def test_set_is_not_degenerate():
    """the set exercises ties and both outcomes of every threshold: some pairs are related at (0.3, 0.8), most are not"""
    ref, cs = ref_all_pairs("symmetric"), chains()
    related = sum(ref_related(r, len(cs[i]), len(cs[j]), 0.3, 0.8) for (i, j), r in ref.items())
    assert 10 < related < len(ref) // 2


def test_transposed_pair_differs(dev):
    """the asymmetric table shows a kernel that reads subst[y][x]: the set has pairs whose two orders give different rows"""
    S, go, ge = tables()["asymmetric"]
    cs = chains()
    letters, offsets = _packed(dev)
    out = seqs.align(letters, offsets, [1, 0], [0, 1], S, go, ge).cpu().numpy()
    assert out[0, 1].tolist() == ref_align(cs[1], cs[1], S, go, ge)
    assert out[0, 0].tolist() == ref_align(cs[1], cs[0], S, go, ge)
    assert out[1, 1].tolist() == ref_align(cs[0], cs[1], S, go, ge)
    assert out[0, 0].tolist() != out[1, 1].tolist()[:3] + out[1, 1].tolist()[5:7] + out[1, 1].tolist()[3:5] + [0]


# ---- 2. sizes beyond the set --------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def big_pairs():
    rng = np.random.default_rng(11)
    a = rng.integers(0, 20, size=600)
    b = np.concatenate([rng.integers(0, 20, size=60), np.where(rng.random(560) < 0.3, rng.integers(0, 20, size=560), a[20:580]),
                        rng.integers(0, 20, size=80)])
    b = np.delete(b, [200, 201, 202, 350])[:700]
    long = rng.integers(0, 20, size=MAX_L)
    one = np.array([long[1500]])
    S = seqs.BLOSUM62
    cs = [a.tolist(), b.tolist(), long.tolist(), one.tolist()]
    return cs, ref_align(cs[0], cs[1], S, 11, 1), ref_align(cs[2], cs[3], S, 11, 1), ref_align(cs[3], cs[2], S, 11, 1)


def test_align_large(dev):
    cs, ref_ab, ref_long_one, ref_one_long = big_pairs()
    assert len(cs[1]) > 600 and ref_ab[2] > 400              # the alignment spans most of both, gaps included
    letters, offsets = _packed(dev, cs)
    out = seqs.align(letters, offsets, [0, 2, 3], [1, 3, 2]).cpu().numpy()
    assert out[0, 0].tolist() == ref_ab
    assert out[1, 1].tolist() == ref_long_one
    assert out[2, 2].tolist() == ref_one_long


# ---- 3. rectangles, sentinels, tiles ------------------------------------------------------------------------------------------------
def test_rectangles(dev):
    S, go, ge = tables()["symmetric"]
    cs, ref = chains(), ref_all_pairs("symmetric")
    letters, offsets = _packed(dev)
    lib = hip.get_lib()
    table = torch.from_numpy(S).to(dev)
    ids_a, ids_b = [3, 3, 17, 0, 30], [5, 2, 5, 31, 3, 28, 12]
    for upper in (0, 1):
        a = torch.tensor(ids_a, dtype=torch.int32, device=dev)
        b = torch.tensor(ids_b, dtype=torch.int32, device=dev)
        out = torch.full((len(ids_a), len(ids_b), 8), -77, dtype=torch.int32, device=dev)     # a sentinel: every element is written
        lib.call("fd_seq_align", letters, offsets, len(cs), a, len(ids_a), b, len(ids_b), table, go, ge, upper, out)
        out = out.cpu().numpy()
        for p, i in enumerate(ids_a):
            for q, j in enumerate(ids_b):
                if upper and i >= j:
                    want = [-1] * 8
                elif i < j:
                    want = list(ref[(i, j)])
                else:
                    want = ref_align(cs[i], cs[j], S, go, ge)
                assert out[p, q].tolist() == want, (upper, i, j)
    one = seqs.align(letters, offsets, [21], [4], S, go, ge).cpu().numpy()                    # a single pair
    assert one.shape == (1, 1, 8) and one[0, 0].tolist() == ref_align(cs[21], cs[4], S, go, ge)


def test_relation_tiles(dev):
    S, go, ge = tables()["symmetric"]
    cs, ref = chains(), ref_all_pairs("symmetric")
    C = len(cs)
    want = np.zeros((C, C), dtype=np.uint8)
    for (i, j), r in ref.items():
        want[i, j] = want[j, i] = ref_related(r, len(cs[i]), len(cs[j]), 0.3, 0.8)
    letters, offsets = _packed(dev)
    for tile in (7, C, 1):
        rel = seqs.relation(letters, offsets, S, 0.3, 0.8, go, ge, tile=tile)
        assert rel.dtype == torch.uint8 and np.array_equal(rel.cpu().numpy(), want), tile


# ---- 4. the greedy clustering kernel ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 2, 63, 64, 65, 300, 1025])
@pytest.mark.parametrize("density", [0.0, 0.02, 0.5, 1.0])
def test_greedy(dev, C, density):
    rng = np.random.default_rng(1000 * C + int(100 * density))
    ld = C + 5
    upper = np.triu(rng.random((C, C)) < density, 1)
    mat = rng.integers(0, 256, size=(C, ld)).astype(np.uint8)                 # garbage below and on the diagonal, and in the padding
    mat[:, :C][np.triu(np.ones((C, C), dtype=bool), 1)] = 0
    mat[:, :C][upper] = rng.integers(1, 256, size=int(upper.sum())).astype(np.uint8)
    lengths = rng.integers(1, 6, size=C)                                      # many equal lengths: the id breaks the tie
    labels_ref, reps_ref, largest_ref = ref_greedy(lambda i, j: bool(upper[i, j]), lengths.tolist())
    rel = torch.from_numpy(mat).to(dev)
    labels, rep, counts = seqs.greedy_clusters(rel, lengths)
    assert labels.cpu().tolist() == labels_ref
    assert rep.cpu().tolist() == reps_ref
    assert counts == {"chains": C, "clusters": len(reps_ref), "largest": largest_ref}
    # the raw outputs: rep is -1 behind the clusters
    lib = hip.get_lib()
    order = np.lexsort((np.arange(C), -lengths)).astype(np.int32)
    lab = torch.full((C,), -9, dtype=torch.int32, device=dev)
    rp = torch.full((C,), -9, dtype=torch.int32, device=dev)
    out = torch.full((4,), -9, dtype=torch.int32, device=dev)
    lib.call("fd_seq_greedy", rel, ld, C, torch.from_numpy(order).to(dev), torch.empty(2 * C, dtype=torch.int32, device=dev), lab, rp, out)
    assert lab.cpu().tolist() == labels_ref
    assert rp.cpu().tolist() == reps_ref + [-1] * (C - len(reps_ref))
    assert out.cpu().tolist() == [C, len(reps_ref), largest_ref, 0]


# ---- 5. cluster_sequences end to end --------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def ref_blosum_pairs():
    cs = chains()
    return {(i, j): tuple(ref_align(cs[i], cs[j], seqs.BLOSUM62, 11, 1)) for i in range(len(cs)) for j in range(i + 1, len(cs))}


def ref_clusters(min_identity, min_coverage):
    cs, ref = chains(), ref_blosum_pairs()
    related = lambda i, j: ref_related(ref[(i, j)], len(cs[i]), len(cs[j]), min_identity, min_coverage)
    return ref_greedy(related, [len(c) for c in cs])


@pytest.mark.parametrize("thresholds", [(0.3, 0.8), (0.5, 0.8), (0.3, 0.0), (0.9, 0.5)])
def test_cluster_sequences(dev, thresholds):
    labels_ref, reps_ref, _ = ref_clusters(*thresholds)
    labels, reps = seqs.cluster_sequences(_packed(dev), *thresholds)
    assert labels.tolist() == labels_ref and reps.tolist() == reps_ref
    first = [labels_ref.index(k) for k in range(len(reps_ref))]               # numbered by ascending smallest member
    assert first == sorted(first) and labels_ref[0] == 0
    if thresholds == (0.3, 0.8):
        assert 4 < len(reps_ref) < len(labels_ref)                            # neither one cluster nor all singletons
        strings = ["".join(seqs.ALPHABET[a] for a in c) for c in chains()]    # strings pack to the same letters
        labels_s, reps_s = seqs.cluster_sequences([s for s in strings], *thresholds)
        assert labels_s.tolist() == labels_ref and reps_s.tolist() == reps_ref


def test_identity_matrix(dev):
    cs, ref = chains(), ref_blosum_pairs()
    ident = seqs.identity_matrix(_packed(dev), [0, 1, 3], [19, 20, 25]).cpu().numpy()
    assert ident.dtype == np.float64
    for p, i in enumerate([0, 1, 3]):
        for q, j in enumerate([19, 20, 25]):
            r = ref[(i, j)]
            assert ident[p, q] == (r[1] / r[2] if r[2] else 0.0)


# ---- 6. ChainStore -----------------------------------------------------------------------------------------------------------------
def _backbone(rng, L):
    ca = np.cumsum(rng.normal(size=(L, 3)) * 2.0, axis=0)
    return (ca[:, None, :] + rng.normal(size=(L, 4, 3))).astype(np.float32)


def _store(dev, with_letters=True, sizes=None):
    """the set of test 1 as chains with random backbones; lengths repeat (the two identical chains, the family members)"""
    rng = np.random.default_rng(3)
    store = ChainStore(dev)
    for k, c in enumerate(chains()):
        L = len(c)
        kw = dict(atoms=_backbone(rng, L), atom_mask=np.ones((L, 4)))
        if with_letters or k % 2:
            kw["aatype"] = np.array(c)
        store.add(**kw)
    return store.freeze()


def test_store_letters(dev):
    store = _store(dev)
    assert store.aatype.dtype == torch.uint8 and store.aatype.cpu().tolist() == [a for c in chains() for a in c]
    assert store.has_letters.all()
    labels, reps = seqs.cluster_sequences(_packed(dev))
    got = store.sequence_clusters()
    assert got is store.clusters and got.tolist() == labels.tolist() and store.cluster_reps.tolist() == reps.tolist()
    assert got.tolist() == ref_clusters(0.3, 0.8)[0]
    # the reference's chain dict carries aatype; a chain without letters is all X and refuses to be clustered
    partial = _store(dev, with_letters=False)
    assert partial.has_letters.tolist() == [bool(k % 2) for k in range(len(chains()))]
    assert partial.aatype[: len(chains()[0])].cpu().tolist() == [20] * len(chains()[0])
    with pytest.raises(ValueError, match="without aatype"):
        partial.sequence_clusters()
    rng = np.random.default_rng(5)
    feats = {"atom_positions": rng.normal(size=(9, 37, 3)), "atom_mask": np.ones((9, 37)), "residue_index": np.arange(9),
             "aatype": np.arange(9)}
    s2 = ChainStore(dev)
    s2.add(feats)
    assert s2.freeze().aatype.cpu().tolist() == list(range(9)) and s2.has_letters.all()
    with pytest.raises(ValueError, match="aatype"):
        ChainStore(dev).add(atoms=np.zeros((3, 4, 3)), atom_mask=np.ones((3, 4)), aatype=[0, 1, 21])


def test_store_letters_from_parsed(dev):
    g = np.load(os.path.join(ROOT, "tests", "golden", "pdb_read.npz"))
    texts = [g["two_chains.file0"].tobytes(), g["plain.file0"].tobytes()]
    parsed = pdb.parse_pdb(texts)
    store = ChainStore(dev)
    ids = store.add_parsed(parsed)
    store.freeze()
    assert len(ids) == len(parsed) >= 3 and store.has_letters.all()
    assert store.aatype.dtype == torch.uint8 and store.aatype.cpu().tolist() == parsed.aatype.cpu().tolist()
    assert store.aatype.cpu().tolist()[-len(g["plain.feats.aatype"]):] == g["plain.feats.aatype"].tolist()
    labels = store.sequence_clusters()
    lens = np.diff(store.offsets.cpu().numpy())
    want, _ = seqs.cluster_sequences((store.aatype, store.offsets))
    assert labels.tolist() == want.tolist() and len(labels) == len(lens)


def _cap(batch_size, max_squared_res, n):
    return min(batch_size, max_squared_res // (n * n))


def test_epoch_plan(dev):
    store = _store(dev)
    lengths = store.lengths
    C = len(store)
    for mode in ("cluster_time_batch", "cluster_length_batch"):
        with pytest.raises(RuntimeError, match="no clusters"):
            store.epoch_plan(mode, 4, 10_000, np.random.default_rng(0))
    with pytest.raises(ValueError, match="Invalid sample mode"):
        store.epoch_plan("batch", 4, 10_000, np.random.default_rng(0))
    clusters = store.sequence_clusters()
    K = len(store.cluster_reps)
    B, MSR = 6, 16_000                        # chains of 65 residues and more get fewer than 6 entries; those above 126 none
    kept = lambda c: _cap(B, MSR, int(lengths[c])) >= 1
    assert any(not kept(c) for c in range(C)) and any(0 < _cap(B, MSR, int(lengths[c])) < B for c in range(C))

    plan = store.epoch_plan("length_batch", B, MSR, np.random.default_rng(1))
    same = store.batch_plan(B, MSR, np.random.default_rng(1))
    assert len(plan) == len(same) and all(np.array_equal(p, q) for p, q in zip(plan, same))

    plan = store.epoch_plan("time_batch", B, MSR, np.random.default_rng(2))
    assert sorted(int(p[0]) for p in plan) == [c for c in range(C) if kept(c)]
    for p in plan:
        assert len(set(p.tolist())) == 1 and len(p) == _cap(B, MSR, int(lengths[p[0]]))
    assert [int(p[0]) for p in plan] != sorted(int(p[0]) for p in plan)         # shuffled

    seen = set()
    for seed in range(8):
        plan = store.epoch_plan("cluster_time_batch", B, MSR, np.random.default_rng(seed))
        drawn = [int(p[0]) for p in plan]
        seen.update(drawn)
        for p in plan:
            assert len(set(p.tolist())) == 1 and len(p) == _cap(B, MSR, int(lengths[p[0]]))
        got = [int(clusters[c]) for c in drawn]
        assert len(set(got)) == len(got)                                         # every cluster at most once ..
        missing = set(range(K)) - set(got)                                       # .. and exactly once unless its draw is too long
        assert all(any(not kept(c) for c in np.flatnonzero(clusters == k)) for k in missing)
        assert len(got) + len(missing) == K
        again = store.epoch_plan("cluster_time_batch", B, MSR, np.random.default_rng(seed))
        assert len(again) == len(plan) and all(np.array_equal(p, q) for p, q in zip(plan, again))
    assert len(seen) > K                                                         # different members over the epochs
    plan = store.epoch_plan("cluster_time_batch", B, 10 ** 9, np.random.default_rng(3))
    assert sorted(int(clusters[p[0]]) for p in plan) == list(range(K))           # nothing too long: every cluster exactly once

    for seed in range(4):
        plan = store.epoch_plan("cluster_length_batch", B, 10 ** 9, np.random.default_rng(seed))
        members = sorted({int(c) for p in plan for c in p})
        assert len({int(clusters[c]) for c in members}) == len(members)          # members of distinct clusters
        ns = [int(lengths[p[0]]) for p in plan]
        assert len(set(ns)) == len(ns)                                           # one batch per length
        for p in plan:
            assert len(p) == B and len({int(lengths[c]) for c in p}) == 1        # one length per batch, b entries
        again = store.epoch_plan("cluster_length_batch", B, 10 ** 9, np.random.default_rng(seed))
        assert len(again) == len(plan) and all(np.array_equal(p, q) for p, q in zip(plan, again))
    plan = store.epoch_plan("cluster_length_batch", B, MSR, np.random.default_rng(0))
    assert plan and all(len(p) == _cap(B, MSR, int(lengths[p[0]])) >= 1 for p in plan)

    # clusters from elsewhere
    store.set_clusters(np.arange(C) // 2)
    assert store.cluster_reps is None
    plan = store.epoch_plan("cluster_time_batch", B, 10 ** 9, np.random.default_rng(0))
    assert sorted(int(p[0]) // 2 for p in plan) == list(range((C + 1) // 2))
    with pytest.raises(ValueError):
        store.set_clusters(np.arange(C - 1))


def test_batches_by_cluster(dev):
    from se3_diffusion_amd.data import se3_diffuser
    from test_diffuser import conf as dconf
    diff = se3_diffuser.SE3Diffuser(dconf())
    rng = np.random.default_rng(9)
    store = ChainStore(dev)
    cs = [chains()[k] for k in (26, 27, 30)]                # short chains: the batches stay small
    for c in cs:
        store.add(atoms=_backbone(rng, len(c)), atom_mask=np.ones((len(c), 4)), aatype=np.array(c))
    store.freeze()
    with pytest.raises(RuntimeError, match="no clusters"):
        next(store.batches(2, 10 ** 6, np.random.default_rng(0), diff, sample_mode="cluster_time_batch"))
    store.sequence_clusters()
    K = len(store.cluster_reps)
    plan = store.epoch_plan("cluster_time_batch", 2, 10 ** 6, np.random.default_rng(0))
    got = list(store.batches(2, 10 ** 6, np.random.default_rng(0), diff, with_gt=True, sample_mode="cluster_time_batch"))
    assert len(got) == len(plan) == K
    ref_batch, ref_gt = store.training_batch(plan[0], diff, rng=np.random.default_rng(1))
    for ids, (batch, gt) in zip(plan, got):
        n = int(store.lengths[ids[0]])
        assert set(batch) == set(ref_batch) and gt.shape == (2, n, 37, 3)
        for k, v in batch.items():
            want = (2,) + ((n,) + tuple(ref_batch[k].shape[2:]) if ref_batch[k].dim() > 1 else ())
            assert v.dtype == ref_batch[k].dtype and tuple(v.shape) == want, k
        assert len(set(batch["t"].cpu().tolist())) == 2                          # one chain at two different t
        assert torch.equal(batch["rigids_0"][0], batch["rigids_0"][1])
    plain = list(store.batches(2, 10 ** 6, np.random.default_rng(0), diff))      # sample_mode=None: what it did before
    assert len(plain) == len(store.batch_plan(2, 10 ** 6, np.random.default_rng(0)))


# ---- 7. refusals and empties -----------------------------------------------------------------------------------------------------
def test_refusals(dev):
    letters, offsets = _packed(dev, [[0, 1, 2], [3, 4]])
    ok = seqs.align(letters, offsets, [0], [1])
    assert ok.shape == (1, 1, 8)
    with pytest.raises(ValueError, match="0 .. 20"):
        seqs.align(torch.tensor([0, 21, 2, 3, 4], dtype=torch.uint8, device=dev), offsets, [0], [1])
    with pytest.raises(ValueError, match="not one of"):
        seqs.pack(["ACDB"], device=dev)
    with pytest.raises(ValueError, match="0 .. 20"):
        seqs.pack([[0, 21]], device=dev)
    long_letters, long_offsets = _packed(dev, [[1] * (MAX_L + 1), [2, 3]])
    with pytest.raises(ValueError, match="more than"):
        seqs.align(long_letters, long_offsets, [1], [0])
    with pytest.raises(ValueError, match="more than"):
        seqs.relation(long_letters, long_offsets)
    assert seqs.align(long_letters, long_offsets, [1], [1]).shape == (1, 1, 8)   # the long chain is not named
    bad = seqs.substitution(1, -1)
    bad[3, 4] = 128
    with pytest.raises(ValueError, match="-127 .. 127"):
        seqs.align(letters, offsets, [0], [1], bad)
    with pytest.raises(ValueError, match=r"\[21,21\]"):
        seqs.align(letters, offsets, [0], [1], np.zeros((20, 20), dtype=np.int32))
    for go, ge in ((11, 0), (-1, 1), (1024, 1), (11, 1024)):
        with pytest.raises(ValueError, match="gap_"):
            seqs.align(letters, offsets, [0], [1], None, go, ge)
    for ident, cov in ((-0.1, 0.5), (1.5, 0.5), (0.3, -1.0), (0.3, 1.01)):
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            seqs.relation(letters, offsets, None, ident, cov)
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            seqs.cluster_sequences((letters, offsets), ident, cov)
    with pytest.raises(ValueError, match=r"\[0, 2\)"):
        seqs.align(letters, offsets, [0], [2])
    # the library refuses the same with its error code, before any launch
    lib = hip.get_lib()
    table = torch.from_numpy(seqs.substitution(1, -1)).to(dev)
    out = torch.zeros((1, 1, 8), dtype=torch.int32, device=dev)
    one = lambda v: torch.tensor([v], dtype=torch.int32, device=dev)
    before = lib.cdll.fd_launch_count()
    cases = [(letters, offsets, 2, one(0), one(2), table, 11, 1, "chain id"),
             (letters, offsets, 2, one(-1), one(1), table, 11, 1, "chain id"),
             (torch.tensor([0, 21, 2, 3, 4], dtype=torch.uint8, device=dev), offsets, 2, one(0), one(1), table, 11, 1, "letter"),
             (long_letters, long_offsets, 2, one(0), one(1), table, 11, 1, "FD_SEQ_MAX_L"),
             (letters, offsets, 2, one(0), one(1), torch.from_numpy(bad).to(dev), 11, 1, "table entry"),
             (letters, offsets, 2, one(0), one(1), table, 11, 0, "gap_extend"),
             (letters, offsets, 2, one(0), one(1), table, 1024, 1, "gap_open")]
    for let, off, C, a, b, tab, go, ge, what in cases:
        with pytest.raises(hip.FdError, match=what):
            lib.call("fd_seq_align", let, off, C, a, 1, b, 1, tab, go, ge, 0, out)
    assert lib.cdll.fd_launch_count() == before and not out.any()


def test_empties(dev):
    lib = hip.get_lib()
    letters, offsets = _packed(dev, [[0, 1, 2], [], [17, 17]])
    before = lib.cdll.fd_launch_count()
    assert seqs.align(letters, offsets, [], [0, 1]).shape == (0, 2, 8)           # Pa = 0: nothing is launched
    assert seqs.align(letters, offsets, [0], []).shape == (1, 0, 8)
    nothing = seqs.pack([], device=dev)
    rel = seqs.relation(*nothing)
    labels, rep, counts = seqs.greedy_clusters(rel, [])                          # C = 0
    assert rel.shape == (0, 0) and labels.shape == (0,) and rep.shape == (0,) and counts["clusters"] == 0
    labels, reps = seqs.cluster_sequences(nothing)
    assert labels.shape == (0,) and reps.shape == (0,)
    e = torch.empty(0, dtype=torch.int32, device=dev)
    lib.call("fd_seq_greedy", torch.empty((0, 0), dtype=torch.uint8, device=dev), 0, 0, e, e, e, e, torch.empty(4, dtype=torch.int32, device=dev))
    assert lib.cdll.fd_launch_count() == before
    # a chain of no residues aligns with nothing and is a cluster of its own
    out = seqs.align(letters, offsets, [0, 1], [1, 2], seqs.substitution(1, -1), 0, 1).cpu().numpy()
    assert out[0, 0].tolist() == EMPTY_ROW and out[1, 0].tolist() == EMPTY_ROW and out[1, 1].tolist() == EMPTY_ROW
    labels, reps = seqs.cluster_sequences((letters, offsets), 0.0, 0.0)
    assert labels.tolist() == [0, 1, 2] and reps.tolist() == [0, 1, 2]


def test_blosum62_properties():
    """what the module vouches for -- the table was typed from memory and NOT compared with NCBI's file"""
    t = seqs.BLOSUM62
    assert t.shape == (21, 21) and t.dtype == np.int32
    assert np.array_equal(t, t.T)
    assert (np.diag(t)[:20] > 0).all()
    w, c = seqs.ALPHABET.index("W"), seqs.ALPHABET.index("C")
    flat = np.sort(t.reshape(-1))
    assert t[w, w] == 11 == flat[-1] and flat[-2] < 11
    assert t[c, c] == 9 == flat[-2] and flat[-3] < 9
    assert (t[20] == -1).all() and (t[:, 20] == -1).all()
    s = seqs.substitution(2, -3, x=-4)
    assert s[5, 5] == 2 and s[5, 6] == -3 and s[20, 20] == -4 and s[3, 20] == -4 and s[20, 3] == -4


def test_read_clusters(tmp_path):
    path = tmp_path / "clusters-by-entity-30.txt"
    path.write_text("1abc_1 2XYZ_2 3def_1\n4ghi_3\n5JKL_1 1abc_2\n")
    table = seqs.read_clusters(str(path))
    assert table == {"1ABC": 2, "2XYZ": 0, "3DEF": 0, "4GHI": 1, "5JKL": 2}
