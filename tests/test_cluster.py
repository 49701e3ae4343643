"""Clustering of sampled backbones on the device (fd_cluster_linkage, fd_cluster_cut; se3_diffusion_amd.metrics.linkage / cluster /
diversity / novelty).

Two references.  (1) _np_linkage / _np_cut: a float64 numpy restatement of include/fd_hip.h, written here: a plain greedy search of
the whole shrinking matrix per merge, with the tie key and the inclusive cut of the specification; it shares nothing with the
kernel.  Against it everything is compared bit for bit (Z, labels, representatives, all eight slots): both sides are IEEE float64
without contraction and the specification fixes the order of every operation.  (2) tests/golden/cluster.npz
(tools/make_golden_cluster.py): what scipy.cluster.hierarchy gives on tie-free matrices -- an independent implementation (a minimum
spanning tree for single linkage, nearest-neighbour chains for average and complete).  The tool asserts that consecutive heights
lie at least 1e-6 apart and no height within 1e-6 of the cut, so ids, sizes and partitions must be equal exactly; single and
complete heights are entries 1.0 - s and must be equal bit for bit; average heights may differ by the rounding of the Lance-Williams
steps: the values are in [0, 1], each of the at most M - 1 steps behind a height rounds once (a few 2^-53), and the bound is
M 2^-52 absolute.  Measured worst: 2.2e-16 (M = 64, 130, 257; bounds 1.4e-14 to 5.7e-14), on the interpreter and on the device alike.

NOT checked anywhere: agreement with MaxCluster, which the paper takes its diversity from; it is not available.

A mutation of the kernel that this file catches on the interpreter (run on a scratch copy): the minimum compared by distance
alone, ids dropped from the key -- the tie cases, the masked batch and the all-identical edge fail; the tie-free fixture cases
pass, as they must.
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
import parity_log  # noqa: E402
from se3_diffusion_amd import hip, metrics as fm  # noqa: E402
from se3_diffusion_amd.metrics import CLUSTER_MAX_M, CLUSTER_SLOTS, cluster, diversity, linkage, novelty  # noqa: E402

G = np.load(os.path.join(ROOT, "tests", "golden", "cluster.npz"))
SIZES = tuple(int(m) for m in G["sizes"])
METHODS = ("single", "average", "complete")
CUT = float(G["cut"])


# ---- the float64 restatement of include/fd_hip.h ---------------------------------------------------------------------------------------
def _np_linkage(mat, present=None, method="average", kind="distance"):
    """Z [M-1,4] and num_merges by the greedy search of the specification on the whole matrix"""
    mat = np.asarray(mat, np.float64)
    M = len(mat)
    keep = np.arange(M) if present is None else np.flatnonzero(np.asarray(present) != 0)
    n = len(keep)
    Z = np.tile(np.array([-1.0, -1.0, np.inf, 0.0]), (max(M - 1, 0), 1))
    if n < 2:
        return Z, 0
    up = np.triu(mat[np.ix_(keep, keep)], 1)
    with np.errstate(invalid="ignore"):
        D = 1.0 - up if kind == "similarity" else up.copy()
    D[np.isnan(D)] = np.inf
    D = np.triu(D, 1)
    D = D + D.T
    np.fill_diagonal(D, np.inf)
    ids, sizes = keep.astype(np.int64), np.ones(n, np.int64)
    for s in range(n - 1):
        dmin = D.min()
        p, q = np.nonzero(np.triu(D == dmin, 1))
        lo, hi = np.minimum(ids[p], ids[q]), np.maximum(ids[p], ids[q])
        e = np.lexsort((hi, lo))[0]                              # the smallest (smaller id, larger id) among the smallest distances
        x, y = (p[e], q[e]) if ids[p[e]] < ids[q[e]] else (q[e], p[e])
        nx, ny = sizes[x], sizes[y]
        Z[s] = ids[x], ids[y], dmin, nx + ny
        dx, dy = D[x], D[y]
        if method == "single":
            new = np.where(dx < dy, dx, dy)
        elif method == "complete":
            new = np.where(dx > dy, dx, dy)
        else:
            new = (float(nx) * dx + float(ny) * dy) / float(nx + ny)
        D[x, :] = new
        D[:, x] = new
        D[x, x] = np.inf
        ids[x], sizes[x] = M + s, nx + ny
        rest = np.arange(len(ids)) != y
        D, ids, sizes = D[np.ix_(rest, rest)], ids[rest], sizes[rest]
    return Z, n - 1


def _seq_sum(v):
    """the sum in the order given, one rounding per addition (np.sum adds pairwise)"""
    return float(np.cumsum(np.asarray(v, np.float64))[-1]) if len(v) else 0.0


def _np_cut(Z, num_merges, mat, present, cut, kind):
    """labels, representatives, the eight slots"""
    mat = np.asarray(mat, np.float64)
    M = len(mat)
    pres = np.ones(M, bool) if present is None else np.asarray(present) != 0
    member = {i: [i] for i in range(M) if pres[i]}               # id -> leaves, only for the merges at or below the cut
    h = Z[:num_merges, 2]
    for s in range(num_merges):
        a, b = int(Z[s, 0]), int(Z[s, 1])
        if h[s] <= cut:
            member[M + s] = sorted(member.pop(a) + member.pop(b))
    clusters = sorted(member.values(), key=lambda m: m[0])
    labels, rep = np.full(M, -1, np.int32), np.full(M, -1, np.int32)
    entry = lambda i, j: mat[min(i, j), max(i, j)]
    pairs, ups = 0, {}
    for k, mem in enumerate(clusters):
        labels[mem] = k
        best = None
        for i in mem:
            sc = _seq_sum([entry(i, j) for j in mem if j != i])
            ups[i] = _seq_sum([entry(i, j) for j in mem if j > i])
            if best is None or (sc > best[0] if kind == "similarity" else sc < best[0]):
                best = (sc, i)
        rep[k] = best[1]
        pairs += len(mem) * (len(mem) - 1) // 2
    within = _seq_sum([ups[i] for i in sorted(ups)])
    n, K = int(pres.sum()), len(clusters)
    sizes = [len(m) for m in clusters]
    nan = float("nan")
    slots = dict(num_samples=float(n), num_clusters=float(K), diversity=K / n if n else nan,
                 largest_cluster=float(max(sizes)) if sizes else 0.0, num_singletons=float(sum(m == 1 for m in sizes)),
                 mean_within_cluster=within / pairs if pairs else nan,
                 last_height_below_cut=float(h[h <= cut].max()) if (h <= cut).any() else nan,
                 first_height_above_cut=float(h[h > cut].min()) if (h > cut).any() else nan)
    return labels, rep, slots


# ---- helpers ------------------------------------------------------------------------------------------------------------------------
def _t(x, dev):
    return None if x is None else torch.as_tensor(np.ascontiguousarray(x)).to(dev)


def _bits(x):
    x = torch.as_tensor(x)
    return x.contiguous().view(torch.int64) if x.dtype == torch.float64 else x


def _same(a, b):
    a, b = torch.as_tensor(a).cpu(), torch.as_tensor(b).cpu()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _same_dict(a, b):
    return set(a) == set(b) and all(_same(a[k], b[k]) for k in a)


def _full(M, cond):
    s = np.full((M, M), np.nan)                                  # only the strict upper triangle may be read
    s[np.triu_indices(M, 1)] = cond
    return s


@functools.lru_cache(maxsize=None)
def _fixture(M):
    return _full(M, G[f"s_{M}"])


@functools.lru_cache(maxsize=None)
def _restated(key, method, kind, cut):
    """the restatement of a named matrix, computed once and shared by both tiers: (Z, num_merges, labels, rep, slots)"""
    mat, present = _matrix(key)
    Z, nm = _np_linkage(mat, present, method, kind)
    return (Z, nm) + _np_cut(Z, nm, mat, present, cut, kind)


def _slots_equal(res, p, slots):
    for k in CLUSTER_SLOTS:
        got = res[k] if p is None else res[k][p]
        want = torch.tensor(slots[k], dtype=torch.float64)
        assert got.dtype == torch.float64 and _same(got.cpu().reshape(()), want), (k, got.item(), slots[k])


def _check_restated(res, ref, p=None):
    Z, nm, labels, rep, slots = ref
    pick = (lambda x: x) if p is None else (lambda x: x[p])
    assert int(pick(res["num_merges"]).item()) == nm
    assert _same(pick(res["Z"]), torch.as_tensor(Z)), "Z differs from the restatement"
    assert np.array_equal(pick(res["labels"]).cpu().numpy(), labels)
    assert np.array_equal(pick(res["representatives"]).cpu().numpy(), rep)
    _slots_equal(res, p, slots)


def _random_similarity(M, seed):
    """tie-free by construction up to chance: the gap is asserted where it matters"""
    rng = np.random.default_rng(seed)
    centres = rng.normal(size=(max(1, M // 6), 3)) * 4.0
    x = centres[rng.integers(len(centres), size=M)] + rng.normal(size=(M, 3))
    d = np.sqrt(((x[:, None] - x[None]) ** 2).sum(-1))
    s = 1.0 / (1.0 + (d / 1.5) ** 2)
    s[np.tril_indices(M)] = np.nan
    return s


def _tie_matrix(M, seed):
    """distances that are multiples of 1/8 in [0, 1]: many exact ties, many entries equal to the cut 0.5.  The samples fall into
    M // 4 groups (sample i in group i % (M // 4)): 1/8 or 2/8 inside a group, 4/8 .. 8/8 between groups, and 4/8 everywhere between
    groups 0 and 1 -- so that each of the three linkages joins those two at a height of exactly 0.5, the cut."""
    rng = np.random.default_rng(seed)
    group = np.arange(M) % (M // 4)
    same = group[:, None] == group[None, :]
    d = np.where(same, rng.integers(1, 3, size=(M, M)), rng.integers(4, 9, size=(M, M))) / 8.0
    d[((group[:, None] == 0) & (group[None, :] == 1)) | ((group[:, None] == 1) & (group[None, :] == 0))] = 0.5
    d[np.tril_indices(M)] = np.nan
    return d


@functools.lru_cache(maxsize=None)
def _matrix(key):
    """(matrix, present) by name"""
    what, M = key.split(":")[0], int(key.split(":")[1])
    if what == "fixture":
        return _fixture(M), None
    if what == "random":
        return _random_similarity(M, 7 * M + 1), None
    if what == "ties":
        return _tie_matrix(M, M), None
    if what == "simties":
        return 1.0 - _tie_matrix(M, M + 1), None                 # (exact: multiples of 1/8)
    if what == "masked":
        present = np.ones(M, np.uint8)
        present[np.random.default_rng(M).choice(M, M // 3, replace=False)] = 0
        return _tie_matrix(M, M + 2), present
    raise KeyError(key)


# ---- 1. the recorded run of scipy ------------------------------------------------------------------------------------------------------
def _run_fixture(dev, M):
    with parity_log.case(f"cluster_fixture_{M}[{dev}]"):
        s = _fixture(M)
        one_minus = 1.0 - G[f"s_{M}"]
        for method in METHODS:
            Zs, T = G[f"Z_{method}_{M}"], G[f"T_{method}_{M}"]
            res = cluster(_t(s, dev), threshold=1.0 - CUT, method=method)
            Z = res["Z"].cpu().numpy()
            assert res["num_merges"].item() == M - 1 and Z.shape == (M - 1, 4)
            assert np.array_equal(Z[:, [0, 1, 3]], Zs[:, [0, 1, 3]]), (M, method, "ids or sizes")
            if method == "average":
                err = float(np.abs(Z[:, 2] - Zs[:, 2]).max())
                bound = M * 2.0 ** -52
                parity_log.out(f"{method}.height", err)
                print(f"  M {M} {method}: heights achieved {err:.3e} absolute (bound {bound:.1e})")
                assert err <= bound, (M, method, err, bound)
            else:
                assert np.array_equal(Z[:, 2].view(np.int64), Zs[:, 2].view(np.int64)), (M, method, "heights")
                assert np.isin(Z[:, 2], one_minus).all()         # each is 1.0 - s of an entry
            # the partition: scipy numbers its clusters otherwise; number them by their first member
            first = {}
            canon = np.array([first.setdefault(t, len(first)) for t in T], np.int32)
            assert np.array_equal(res["labels"].cpu().numpy(), canon), (M, method, "partition")
            assert res["num_clusters"].item() == len(first) and res["num_samples"].item() == M
            assert res["diversity"].item() == len(first) / M
            # the same call through linkage alone, as distances
            link = linkage(_t(1.0 - s, dev), method=method, kind="distance")
            assert _same(link["Z"], res["Z"]) and _same(link["num_merges"], res["num_merges"])
            _check_restated(res, _restated(f"fixture:{M}", method, "similarity", CUT))


@pytest.mark.parametrize("M", SIZES)
def test_fixture_emu(use_emu, M):
    _run_fixture("cpu", M)


@pytest.mark.gpu
@pytest.mark.parametrize("M", SIZES)
def test_fixture_gpu(hip_lib, M):
    _run_fixture("cuda", M)


# ---- 2. exact ties and entries on the cut: the tie key and the inclusive cut -------------------------------------------------------------
def _run_ties(dev, M):
    for key, kind in ((f"ties:{M}", "distance"), (f"simties:{M}", "similarity")):
        mat, _ = _matrix(key)
        up = mat[np.triu_indices(M, 1)]
        assert (up == 0.5).sum() >= 3 and len(np.unique(up)) <= 9          # entries on the cut, and ties everywhere
        for method in METHODS:
            ref = _restated(key, method, kind, 0.5)
            assert (ref[0][:, 2] == 0.5).any(), (key, method)               # a merge exactly at the cut: it must be replayed
            res = cluster(_t(mat, dev), threshold=0.5, method=method, kind=kind)
            _check_restated(res, ref)
            assert res["last_height_below_cut"].item() == 0.5 and not res["first_height_above_cut"].item() <= 0.5
    # the inclusive cut on its own: one pair at exactly the threshold merges, a hair above it does not
    s = np.array([[1.0, 0.5], [0.0, 1.0]])
    assert cluster(_t(s, dev), threshold=0.5)["num_clusters"].item() == 1
    assert cluster(_t(s, dev), threshold=np.nextafter(0.5, 1.0))["num_clusters"].item() == 2


@pytest.mark.parametrize("M", (12, 40))
def test_ties_emu(use_emu, M):
    _run_ties("cpu", M)


@pytest.mark.gpu
@pytest.mark.parametrize("M", (12, 40))
def test_ties_gpu(hip_lib, M):
    _run_ties("cuda", M)


# ---- 3. masks and batching ---------------------------------------------------------------------------------------------------------------
def _run_masks(dev):
    M = 40
    # one problem with absent samples against its compacted run
    mat, present = _matrix(f"masked:{M}")
    keep = np.flatnonzero(present)
    n = len(keep)
    for method in METHODS:
        res = cluster(_t(mat, dev), threshold=0.5, method=method, present=_t(present, dev), kind="distance")
        _check_restated(res, _restated(f"masked:{M}", method, "distance", 0.5))
        comp = cluster(_t(mat[np.ix_(keep, keep)], dev), threshold=0.5, method=method, kind="distance")
        Z, Zc = res["Z"].cpu().numpy(), comp["Z"].cpu().numpy()
        assert res["num_merges"].item() == n - 1 == comp["num_merges"].item()
        ids = np.concatenate([keep, M + np.arange(n - 1)]).astype(np.float64)          # compacted id -> id
        assert np.array_equal(Z[:n - 1, :2], ids[Zc[:, :2].astype(int)])
        assert np.array_equal(Z[:n - 1, 2:].view(np.int64), Zc[:, 2:].view(np.int64))
        assert (Z[n - 1:] == np.array([-1.0, -1.0, np.inf, 0.0])).all()
        labels = res["labels"].cpu().numpy()
        assert (labels[present == 0] == -1).all() and np.array_equal(labels[keep], comp["labels"].cpu().numpy())
        K = int(res["num_clusters"].item())
        rep, repc = res["representatives"].cpu().numpy(), comp["representatives"].cpu().numpy()
        assert np.array_equal(rep[:K], keep[repc[:K]]) and (rep[K:] == -1).all()
        assert all(_same(res[k], comp[k]) for k in CLUSTER_SLOTS)
    # five problems of different n in one call, in a strided view with NaN wherever nothing may be read
    ns = (0, 1, 2, 17, 40)
    rng = np.random.default_rng(5)
    buf = np.full((5, M + 3, M + 5), np.nan)
    pres = np.zeros((5, M), np.uint8)
    for g, k in enumerate(ns):
        pres[g, rng.choice(M, k, replace=False)] = 1
        d = _tie_matrix(M, 100 + g) if g % 2 else _random_similarity(M, 200 + g)
        on = np.flatnonzero(pres[g])
        upper = np.triu(np.ones((M, M), bool), 1) & pres[g][:, None].astype(bool) & pres[g][None, :].astype(bool)
        buf[g, 1:M + 1, 2:M + 2][upper] = d[upper]
        assert len(on) == k
    tb = _t(buf, dev)
    view = tb[:, 1:M + 1, 2:M + 2]
    assert not view.is_contiguous()
    for method in METHODS:
        res = cluster(view, threshold=0.5, method=method, present=_t(pres, dev), kind="distance")
        assert res["Z"].shape == (5, M - 1, 4) and res["labels"].shape == (5, M) and res["num_merges"].dtype == torch.int32
        assert res["num_merges"].tolist() == [max(k - 1, 0) for k in ns]
        assert _same_dict(res, cluster(view, threshold=0.5, method=method, present=_t(pres, dev), kind="distance"))      # again
        for g in range(5):
            clean = np.where(np.isnan(buf[g, 1:M + 1, 2:M + 2]), 0.25, buf[g, 1:M + 1, 2:M + 2])   # other garbage, contiguous
            lone = cluster(_t(clean, dev), threshold=0.5, method=method, present=_t(pres[g], dev), kind="distance")
            assert all(_same(res[k][g], lone[k]) for k in res), (method, g)
            Zr, nm = _np_linkage(clean, pres[g], method, "distance")
            _check_restated(res, (Zr, nm) + _np_cut(Zr, nm, clean, pres[g], 0.5, "distance"), g)
        assert res["num_samples"].tolist() == [float(k) for k in ns]
        assert np.isnan(res["diversity"][0].item()) and res["diversity"][1].item() == 1.0


def test_masks_emu(use_emu):
    _run_masks("cpu")


@pytest.mark.gpu
def test_masks_gpu(hip_lib):
    _run_masks("cuda")


# ---- 4. edges ----------------------------------------------------------------------------------------------------------------------------
def _run_edges(dev, lib):
    nan = float("nan")
    # no sample, one, two
    for M in (0, 1, 2):
        s = np.full((M, M), 0.75)
        res = cluster(_t(s, dev).reshape(M, M), threshold=0.5)
        assert res["Z"].shape == (max(M - 1, 0), 4) and res["labels"].shape == (M,) and res["num_merges"].item() == max(M - 1, 0)
        assert res["num_samples"].item() == M and res["num_clusters"].item() == min(M, 1)
        assert np.isnan(res["diversity"].item()) if M == 0 else res["diversity"].item() == 1.0 / M
    assert res["Z"].tolist() == [[0.0, 1.0, 0.25, 2.0]] and res["mean_within_cluster"].item() == 0.75
    assert res["representatives"].tolist() == [0, -1] and res["labels"].tolist() == [0, 0]
    assert np.isnan(res["first_height_above_cut"].item()) and res["last_height_below_cut"].item() == 0.25
    # every sample absent; one present; two present
    s = _random_similarity(9, 3)
    for on in ((), (4,), (2, 7)):
        present = np.zeros(9, np.uint8)
        present[list(on)] = 1
        res = cluster(_t(s, dev), threshold=0.0, present=_t(present, dev))
        assert res["num_merges"].item() == max(len(on) - 1, 0) and res["num_samples"].item() == len(on)
        assert (res["labels"].cpu().numpy() == np.where(present, 0, -1)).all()
        assert res["representatives"].tolist() == ([on[0]] if on else [-1]) + [-1] * 8
        assert (np.isnan(res["diversity"].item()) and res["num_clusters"].item() == 0) if not on else res["num_clusters"].item() == 1
        Z = res["Z"].cpu().numpy()
        assert (Z[max(len(on) - 1, 0):] == np.array([-1.0, -1.0, np.inf, 0.0])).all()
    assert Z[0].tolist() == [2.0, 7.0, 1.0 - s[2, 7], 2.0]
    # all samples identical: distance 0 everywhere; the tie rule alone decides the tree
    M = 11
    for method in METHODS:
        res = cluster(_t(np.zeros((M, M)), dev), threshold=0.0, method=method, kind="distance")
        Z = res["Z"].tolist()
        # (0, 1) first, then (2, 3): a pair of leaves comes before any pair with the new cluster, whose id is the largest
        assert Z[:6] == [[2.0 * k, 2.0 * k + 1, 0.0, 2.0] for k in range(5)] + [[10.0, 11.0, 0.0, 3.0]], method
        assert Z[6:] == [[12.0, 13.0, 0.0, 4.0], [14.0, 15.0, 0.0, 4.0], [16.0, 17.0, 0.0, 7.0], [18.0, 19.0, 0.0, 11.0]], method
        assert _same(res["Z"], torch.as_tensor(_np_linkage(np.zeros((M, M)), None, method, "distance")[0]))
        assert res["num_clusters"].item() == 1 and res["largest_cluster"].item() == M and res["representatives"][0].item() == 0
        assert res["mean_within_cluster"].item() == 0.0 and res["num_singletons"].item() == 0
    # a threshold above every similarity: nothing merges, every sample is its own representative
    s = _random_similarity(23, 9)
    res = cluster(_t(s, dev), threshold=2.0, method="single")
    assert res["num_clusters"].item() == 23 == res["num_singletons"].item() and res["diversity"].item() == 1.0
    assert res["labels"].tolist() == list(range(23)) == res["representatives"].tolist()
    assert np.isnan(res["mean_within_cluster"].item()) and np.isnan(res["last_height_below_cut"].item())
    assert res["first_height_above_cut"].item() == res["Z"][0, 2].item() and res["largest_cluster"].item() == 1
    # refused before any launch
    n0 = lib.cdll.fd_launch_count()
    big = torch.zeros((), dtype=torch.float64, device=dev).expand(CLUSTER_MAX_M + 1, CLUSTER_MAX_M + 1)
    for fn in (cluster, linkage):
        with pytest.raises(ValueError, match=str(CLUSTER_MAX_M)):
            fn(big)
        with pytest.raises(ValueError, match="method"):
            fn(_t(s, dev), method="ward")
        with pytest.raises(ValueError, match="kind"):
            fn(_t(s, dev), kind="affinity")
        with pytest.raises(ValueError, match="expected"):
            fn(_t(s[:, :5], dev))
    pos = torch.zeros((3, 8, 3), device=dev)
    with pytest.raises(ValueError, match="tm"):
        diversity(pos, tm="tmalign")
    with pytest.raises(ValueError, match="symmetrize"):
        diversity(pos, tm="align", symmetrize="median")
    f = lambda *shape, dt=torch.float64: torch.zeros(shape, dtype=dt, device=dev)
    with pytest.raises(hip.FdError, match="4096"):
        lib.call("fd_cluster_linkage", f(1), 4097, 0, None, 1, 4097, 0, 1, f(1), f(1), f(1, dt=torch.int32))
    with pytest.raises(hip.FdError, match="method"):
        lib.call("fd_cluster_linkage", f(4, 4), 4, 0, None, 1, 4, 0, 3, f(16), f(3, 4), f(1, dt=torch.int32))
    with pytest.raises(hip.FdError, match="4096"):
        lib.call("fd_cluster_cut", f(1), f(1, dt=torch.int32), f(1), 4097, 0, None, 1, 4097, 0, 0.5, f(1, dt=torch.int32),
                 f(1, dt=torch.int32), f(8))
    assert lib.cdll.fd_launch_count() == n0
    cluster(_t(s, dev))
    assert lib.cdll.fd_launch_count() == n0 + 2                  # one launch each


def test_edges_emu(use_emu):
    _run_edges("cpu", use_emu)


@pytest.mark.gpu
def test_edges_gpu(hip_lib):
    _run_edges("cuda", hip_lib)


# ---- 5. the shapes of the block: a wave, the block, several strides of it ---------------------------------------------------------------
def _run_boundary(dev, M):
    key = f"random:{M}"
    for method in METHODS if M <= 257 else ("average",):
        ref = _restated(key, method, "similarity", 0.5)
        h = ref[0][:, 2]
        assert np.diff(h).min() > 1e-9 and np.abs(h - 0.5).min() > 1e-9      # tie-free: the order of the merges is the data's
        res = cluster(_t(_matrix(key)[0], dev), threshold=0.5, method=method)
        _check_restated(res, ref)


@pytest.mark.parametrize("M", (63, 64, 65, 255, 256, 257))
def test_boundary_emu(use_emu, M):
    _run_boundary("cpu", M)


@pytest.mark.gpu
@pytest.mark.parametrize("M", (63, 64, 65, 255, 256, 257, 1025))
def test_boundary_gpu(hip_lib, M):
    _run_boundary("cuda", M)


# ---- 6. end to end: diversity and novelty --------------------------------------------------------------------------------------------------
def _walk(rng, N):
    step = rng.normal(size=(N, 3))
    return np.cumsum(3.8 * step / np.linalg.norm(step, axis=-1, keepdims=True), axis=0)


def _rigid(rng, x):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    q *= np.sign(np.linalg.det(q))
    return x @ q.T + rng.normal(size=3) * 10.0


def _run_planted(dev, copies):
    """four planted folds: random-walk CA chains of 48 residues, fold k copied copies[k] times under a random rigid motion and
    0.2 A of noise"""
    rng = np.random.default_rng(11)
    N = 48
    fold, pos = [], []
    for k, c in enumerate(copies):
        base = _walk(rng, N)
        for _ in range(c):
            pos.append(_rigid(rng, base + rng.normal(size=(N, 3)) * 0.2))
            fold.append(k)
    order = rng.permutation(len(pos))                            # the folds interleaved
    pos, fold = np.asarray(pos, np.float32)[order], np.asarray(fold)[order]
    tpos = _t(pos, dev)
    tm_t = fm.pairwise_tm(tpos)
    tm = tm_t.cpu().numpy()
    same = fold[:, None] == fold[None, :]
    off = ~np.eye(len(pos), dtype=bool)
    # (so that the case cannot pass by accident: the folds are what the threshold separates, with room on both sides)
    assert tm[same & off].min() > 0.5 + 0.05 and tm[~same].max() < 0.5 - 0.05, (tm[same & off].min(), tm[~same].max())
    res = diversity(tpos)
    assert res["num_clusters"].item() == 4 and res["num_samples"].item() == len(pos)
    assert res["diversity"].item() == 4 / len(pos) and res["largest_cluster"].item() == max(copies)
    labels = res["labels"].cpu().numpy()
    assert all(len(set(labels[fold == k])) == 1 for k in range(4)) and len(set(labels)) == 4
    assert fold[res["representatives"][:4].cpu().numpy()].tolist() == [fold[np.flatnonzero(labels == k)[0]] for k in range(4)]
    direct = cluster(tm_t)
    assert _same(res["tm"], tm_t) and all(_same(res[k], direct[k]) for k in direct)


def _run_align(dev, lengths, relatives, syms):
    """chains of several lengths, the first `relatives` of them prefixes of one random walk under 0.15 A of noise, the others walks
    of their own; every chain under a rigid motion"""
    rng = np.random.default_rng(13)
    M, N = len(lengths), max(lengths)
    pos, mask = np.zeros((M, N, 3), np.float32), np.zeros((M, N), np.float32)
    base = _walk(rng, N)
    for k, L in enumerate(lengths):
        x = base[:L] + rng.normal(size=(L, 3)) * 0.15 if k < relatives else _walk(rng, L)
        pos[k, :L], mask[k, :L] = _rigid(rng, x), 1
    tpos, tmask = _t(pos, dev), _t(mask, dev)
    both = fm.tm_align_matrix(tpos, tmask)
    a, b = both["tm_norm_a"], both["tm_norm_b"]
    mats = {"min": torch.minimum(a, b), "max": torch.maximum(a, b), "mean": 0.5 * (a + b)}
    for sym in syms:
        res = diversity(tpos, tmask, tm="align", symmetrize=sym) if sym != "min" else diversity(tpos, tmask, tm="align")
        direct = cluster(mats[sym])
        assert _same(res["tm"], mats[sym]) and all(_same(res[k], direct[k]) for k in direct), sym
        if sym == "min":                                         # normalised by the longer chain, the relatives still belong together
            assert res["labels"][:relatives].tolist() == [0] * relatives and res["num_clusters"].item() >= 2
    # novelty: the first chains against the last ones as a library; the last sample is the library's first chain
    h = M // 2
    nov = novelty(tpos[:h + 1], tmask[:h + 1], tpos[h:], tmask[h:])
    tm = fm.tm_align_matrix(tpos[:h + 1], tmask[:h + 1], tpos[h:], tmask[h:])["tm_norm_a"]
    assert nov["max_tm_to_library"].dtype == torch.float64 and nov["nearest"].dtype == torch.int64
    assert nov["max_tm_to_library"].shape == (h + 1,) and _same(nov["max_tm_to_library"], tm.max(dim=1).values)
    assert np.array_equal(nov["nearest"].cpu().numpy(), tm.cpu().numpy().argmax(1))
    assert nov["nearest"][h].item() == 0 and abs(nov["max_tm_to_library"][h].item() - 1.0) < 1e-6


# (the interpreter takes about a second per pair of chains: it runs a reduced set; the device runs the full one)
def test_planted_folds_emu(use_emu):
    _run_planted("cpu", (2, 1, 2, 1))


@pytest.mark.gpu
def test_planted_folds_gpu(hip_lib):
    _run_planted("cuda", (3, 5, 4, 3))


def test_align_and_novelty_emu(use_emu):
    _run_align("cpu", (24, 28, 30, 26), 2, ("min",))


@pytest.mark.gpu
def test_align_and_novelty_gpu(hip_lib):
    _run_align("cuda", (40, 44, 52, 60, 47, 56), 3, ("min", "max", "mean"))
