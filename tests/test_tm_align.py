"""TM-align on the device: the search over alignments (fd_tm_align, se3_diffusion_amd.metrics.tm_align / tm_align_matrix /
eval_rows(tm="align")).

The reference of every parity case is a float64 numpy restatement, written here, of the search that include/fd_hip.h specifies:
a textbook Kabsch superposition (SVD, determinant fix) where the kernels use Horn's quaternion, the DP filled one anti-diagonal
at a time with numpy (checked below against the cell-by-cell loop of the specification), everything else plain loops.  It
shares nothing with the kernels.  Neither tmtools nor the TM-align program is available to this suite: agreement with the values
they print is NOT checked here.

Inputs come from fixed seeds: CA traces are random walks of 3.8 A steps rounded to float32.  Bounds, the same on the interpreter
and on the device (the project's own for fp64 metrics): scalars within 1e-9 * max(1, |ref|), R and t within 1e-8 absolute; map,
num_aligned, best_class, num_dp, num_units, La, Lb exactly.  The exact comparisons are sound only under a margin, which the
restatement returns and every parity case asserts (exact ties are set aside: they are bitwise ties on both sides):
  distance part >= 1e-7 A: the smallest |sqrt(d2) - dcut| over every selection of search and quick, |d - d8| of the final filter,
      and the slack of every decisive secondary-structure threshold;
  score part >= 1e-9 (10^4 times the accumulated rounding of a DP): the smallest |h - max(v, z)| over all DP cells and |v - h| over
      the traceback, the gap between the best and the next candidate of a search, of a quick and of a class's units, |s - best.s|
      and ||s - s_old| - 1e-6| in the refinement, and the gaps between the classes' best.s.
The seeds of the inputs were chosen so that the restatement alone meets the margin.  Each case reports what it achieved through
parity_log (expected: <= 1e-11)."""
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

REL = 1e-9
MARGIN_DIST = 1e-7
MARGIN_SCORE = 1e-9
NAN = float("nan")
KINDS = ("insert", "domain", "unrelated")
SIZES = ((5, 5), (11, 12), (12, 11), (21, 22), (40, 63), (63, 64), (64, 65), (65, 130), (130, 97), (129, 128))
EXACT = ("La", "Lb", "num_aligned", "best_class", "num_dp", "num_units")
SCALARS = ("tm_norm_a", "tm_norm_b", "rmsd", "d0_a", "d0_b", "search_tm")
# input seeds, per (kind, La, Lb); 0 unless the restatement missed its margin with it (checked on the CPU, see _np_case)
SEEDS = {}


# ---- generators -------------------------------------------------------------------------------------------------------------------
def _walk(rng, n):
    steps = rng.normal(size=(n, 3))
    return np.cumsum(3.8 * steps / np.linalg.norm(steps, axis=-1, keepdims=True), axis=0)


def _rotation(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]])


def _move(rng, x, noise=0.0):
    y = x @ _rotation(rng).T + rng.normal(size=3) * 10
    return y + rng.normal(size=y.shape) * noise if noise else y


def _pair(kind, La, Lb, seed=0):
    """float32 a [La,3], b [Lb,3]: the shorter chain is derived from the longer one (insert: a moved copy with one segment deleted
    and 1 A noise; domain: a moved contiguous sub-fragment with 1 A noise) or is an unrelated walk"""
    rng = np.random.default_rng([seed, La, Lb, KINDS.index(kind)])
    Lmax, Lmin = max(La, Lb), min(La, Lb)
    long = _walk(rng, Lmax).astype(np.float32).astype(np.float64)
    cut = Lmax - Lmin
    if kind == "insert":
        at = Lmin // 2
        short = _move(rng, np.concatenate([long[:at], long[at + cut:]]), 0.6)
    elif kind == "domain":
        at = cut // 2
        short = _move(rng, long[at:at + Lmin], 0.6)
    else:
        short = _walk(rng, Lmin)
    long, short = long.astype(np.float32), short.astype(np.float32)
    return (long, short) if La >= Lb else (short, long)


# ---- the float64 restatement ------------------------------------------------------------------------------------------------------
class _Margin:
    def __init__(self):
        self.dist, self.score = np.inf, np.inf

    def d(self, x):
        x = np.asarray(x, np.float64).reshape(-1)
        if x.size:
            self.dist = min(self.dist, float(np.abs(x).min()))

    def s(self, x):
        """score differences; exact ties (zeros) are set aside"""
        x = np.abs(np.asarray(x, np.float64).reshape(-1))
        x = x[x > 0]
        if x.size:
            self.score = min(self.score, float(x.min()))

    def best_of(self, scores):
        """the gap between the greatest and every other (distinct) score"""
        s = np.asarray(scores, np.float64)
        if s.size > 1:
            self.s(s.max() - s)


def _np_d0(L):
    return float(1.24 * np.cbrt(L - 15.0) - 1.8) if L > 21 else 0.5


def _np_kabsch(a, b):
    """optimal proper rotation of a onto b (textbook Kabsch: SVD of the covariance, determinant fix)"""
    ca, cb = a.mean(0), b.mean(0)
    H = (a - ca).T @ (b - cb)
    U, S, Vt = np.linalg.svd(H)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))])
    R = Vt.T @ D @ U.T
    return R, cb - R @ ca


def _np_lens(n):
    lens, l = [], n
    for i in range(6):
        if l <= 4:
            break
        lens.append(l)
        l = n >> (i + 1)
    lens.append(4)
    return lens


def _np_search(pa, pb, Lnorm, d0, step, mg, max_iter=20):
    """search(pairs, Lnorm, d0, step): (s, R, t)"""
    n = len(pa)
    d2of = lambda R, t: ((pa @ R.T + t - pb) ** 2).sum(-1)
    if n == 0:
        return 0.0, None, None
    if n < 4:
        R, t = _np_kabsch(pa, pb)
        return float(np.sum(1.0 / (1.0 + d2of(R, t) / d0 ** 2)) / Lnorm), R, t
    d0s = min(max(d0, 4.5), 8.0)

    def score(R, t, dcut):
        d2 = d2of(R, t)
        d = np.sqrt(d2)
        while True:
            mg.d(d - dcut)
            sel = d2 < dcut * dcut
            if sel.sum() >= 3:
                break
            dcut += 0.5
        return float(np.sum(1.0 / (1.0 + d2 / d0 ** 2)) / Lnorm), sel

    cands = []
    for ln in _np_lens(n):
        for start in range(0, n - ln + 1, step):
            sel = np.zeros(n, bool)
            sel[start:start + ln] = True
            R, t = _np_kabsch(pa[sel], pb[sel])
            s, sel = score(R, t, d0s - 1.0)
            cands.append((s, R, t))
            for _ in range(max_iter):
                R, t = _np_kabsch(pa[sel], pb[sel])
                s, new = score(R, t, d0s + 1.0)
                cands.append((s, R, t))
                same = bool((new == sel).all())
                sel = new
                if same:
                    break
    best = (-1.0, None, None)
    for c in cands:
        if c[0] > best[0]:
            best = c
    mg.best_of([c[0] for c in cands])
    return best


def _np_dp_cells(S, gap):
    """DP(S, gap) of the specification, cell by cell: val, path"""
    La, Lb = S.shape
    val = np.zeros((La + 1, Lb + 1))
    path = np.zeros((La + 1, Lb + 1), bool)
    for i in range(1, La + 1):
        for j in range(1, Lb + 1):
            h = val[i - 1, j - 1] + S[i - 1, j - 1]
            v = val[i - 1, j] + (gap if path[i - 1, j] else 0.0)
            z = val[i, j - 1] + (gap if path[i, j - 1] else 0.0)
            if h >= max(v, z):
                path[i, j], val[i, j] = True, h
            else:
                path[i, j], val[i, j] = False, max(v, z)
    return val, path


def _np_dp_fill(S, gap, mg=None):
    """the same table, one anti-diagonal i + j = d at a time (the cells of a diagonal do not depend on one another)"""
    La, Lb = S.shape
    val = np.zeros((La + 1, Lb + 1))
    path = np.zeros((La + 1, Lb + 1), bool)
    for d in range(2, La + Lb + 1):
        i = np.arange(max(1, d - Lb), min(La, d - 1) + 1)
        j = d - i
        h = val[i - 1, j - 1] + S[i - 1, j - 1]
        v = val[i - 1, j] + np.where(path[i - 1, j], gap, 0.0)
        z = val[i, j - 1] + np.where(path[i, j - 1], gap, 0.0)
        m = np.maximum(v, z)
        p = h >= m
        val[i, j] = np.where(p, h, m)
        path[i, j] = p
        if mg is not None:
            mg.s(h - m)
    return val, path


def _np_dp(S, gap, mg):
    """DP(S, gap): the alignment as a list of (i, j)"""
    val, path = _np_dp_fill(S, gap, mg)
    i, j = S.shape
    pairs = []
    while i > 0 and j > 0:
        if path[i, j]:
            pairs.append((i - 1, j - 1))
            i, j = i - 1, j - 1
        else:
            h = val[i - 1, j] + (gap if path[i - 1, j] else 0.0)
            v = val[i, j - 1] + (gap if path[i, j - 1] else 0.0)
            mg.s(v - h)
            if v >= h:
                j -= 1
            else:
                i -= 1
    return pairs[::-1]


def _np_ss(x, mg):
    """CA secondary structure: 0 C, 1 H, 2 E, 3 T"""
    L = len(x)
    ss = np.zeros(L, int)
    D = lambda p, q: float(np.linalg.norm(x[p] - x[q]))
    for i in range(2, L - 2):
        d13, d14, d15, d24, d25, d35 = D(i - 2, i), D(i - 2, i + 1), D(i - 2, i + 2), D(i - 1, i + 1), D(i - 1, i + 2), D(i, i + 2)
        done = False
        for cls, tol, refs in ((1, 2.1, (6.37, 5.18, 5.18, 5.45, 5.45, 5.45)), (2, 1.42, (13.0, 10.4, 10.4, 6.1, 6.1, 6.1))):
            slack = np.array([tol - abs(d - r) for d, r in zip((d15, d14, d25, d13, d24, d35), refs)])
            if (slack > 0).all():
                mg.d(slack.min())
                ss[i], done = cls, True
                break
            mg.d(slack.min())            # robustly "not this class": the most violated condition decides
        if not done:
            mg.d(d15 - 8.0)
            ss[i] = 3 if d15 < 8.0 else 0
    return ss


def _np_align(a, b, search_step=40, max_dp=30):
    """the whole of include/fd_hip.h's fd_tm_align on the counting positions a [La,3], b [Lb,3] (float32 values)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    La, Lb = len(a), len(b)
    Lmin = min(La, Lb)
    mg = _Margin()
    res = dict(La=float(La), Lb=float(Lb), num_aligned=0.0, tm_norm_a=NAN, tm_norm_b=NAN, rmsd=NAN, d0_a=_np_d0(La), d0_b=_np_d0(Lb),
               best_class=-1.0, num_dp=0.0, num_units=0.0, search_tm=NAN, map=-np.ones(La, np.int64), R=None, t=None,
               class_s=[None] * 4)
    if Lmin < 5:
        res.update(margin_dist=np.inf, margin_score=np.inf)
        return res
    d0 = _np_d0(Lmin) + 0.8
    d0s = min(max(d0, 4.5), 8.0)
    d8 = 1.5 * Lmin ** 0.3 + 3.5

    def gather(pairs):
        ia = np.array([p[0] for p in pairs], int)
        ib = np.array([p[1] for p in pairs], int)
        return a[ia], b[ib]

    def quick(pairs):
        if len(pairs) < 3:
            return -1.0, None, None
        pa, pb = gather(pairs)
        tm = lambda d2: float(np.sum(1.0 / (1.0 + d2 / d0 ** 2)) / Lmin)
        R, t = _np_kabsch(pa, pb)
        d2 = ((pa @ R.T + t - pb) ** 2).sum(-1)
        cands = [(tm(d2), R, t)]
        for dc in (d0s, d0s + 1.0):
            mg.d(np.sqrt(d2) - dc)
            sel = d2 < dc * dc
            if sel.sum() < 3:
                break
            R, t = _np_kabsch(pa[sel], pb[sel])
            d2 = ((pa @ R.T + t - pb) ** 2).sum(-1)
            cands.append((tm(d2), R, t))
        best = cands[0]
        for c in cands[1:]:
            if c[0] > best[0]:
                best = c
        mg.best_of([c[0] for c in cands])
        return best

    def tm_matrix(R, t, dd):
        d2 = (((a @ R.T + t)[:, None, :] - b[None, :, :]) ** 2).sum(-1)
        return 1.0 / (1.0 + d2 / dd)

    maps = [None] * 4
    # class 0: gapless
    m = min(Lmin, max(Lmin // 2, 5))
    best0, scores = (-1.0, None, None, None), []
    for k in range(-(La - m), Lb - m + 1):
        pairs = [(i, i + k) for i in range(max(0, -k), min(La, Lb - k))]
        s, R, t = quick(pairs)
        scores.append(s)
        if s > best0[0]:
            best0 = (s, R, t, pairs)
    mg.best_of(scores)
    units = len(scores)
    maps[0], R0, t0 = best0[3], best0[1], best0[2]
    # classes 1, 2: secondary structure
    ssa, ssb = _np_ss(a, mg), _np_ss(b, mg)
    E = (ssa[:, None] == ssb[None, :]).astype(np.float64)
    maps[1] = _np_dp(E, -1.0, mg)
    maps[2] = _np_dp(tm_matrix(R0, t0, d0 ** 2) + 0.5 * E, -1.0, mg)
    # class 3: fragments
    f = min(20, Lmin // 3)
    if f >= 4:
        starts = lambda L: range(0, L - f + 1, max(f, -(-(L - f + 1) // 8)))
        best3, scores = (-1.0, None), []
        for sa in starts(La):
            for sb in starts(Lb):
                R, t = _np_kabsch(a[sa:sa + f], b[sb:sb + f])
                pairs = _np_dp(tm_matrix(R, t, (d0 + 1.5) ** 2), 0.0, mg)
                s = quick(pairs)[0]
                scores.append(s)
                if s > best3[0]:
                    best3 = (s, pairs)
        mg.best_of(scores)
        units += len(scores)
        maps[3] = best3[1]
    # refinement
    num_dp, results = 0, [None] * 4
    for cls, map0 in enumerate(maps):
        if map0 is None or len(map0) < 3:
            continue
        s, R, t = _np_search(*gather(map0), Lmin, d0, search_step, mg)
        best = (s, R, t, map0)
        for gap in (-0.6, 0.0):
            R, t = best[1], best[2]
            prev, s_old = map0, None
            for _ in range(max_dp):
                new = _np_dp(tm_matrix(R, t, d0 ** 2), gap, mg)
                num_dp += 1
                if new == prev:
                    break
                prev = new
                if len(new) < 3:
                    break
                s, R, t = _np_search(*gather(new), Lmin, d0, search_step, mg)
                mg.s(s - best[0])
                if s > best[0]:
                    best = (s, R, t, new)
                if s_old is not None:
                    mg.s(abs(s - s_old) - 1e-6)
                    if abs(s - s_old) < 1e-6:
                        break
                s_old = s
        results[cls] = best
    res.update(num_dp=float(num_dp), num_units=float(units), class_s=[None if r is None else r[0] for r in results])
    top, cls = -1.0, -1
    for q, r in enumerate(results):
        if r is not None and r[0] > top:
            top, cls = r[0], q
    mg.best_of([r[0] for r in results if r is not None])
    res.update(margin_dist=mg.dist, margin_score=mg.score)
    if cls < 0:
        return res
    _, R, t, pairs = results[cls]
    pa, pb = gather(pairs)
    d = np.sqrt(((pa @ R.T + t - pb) ** 2).sum(-1))
    mg.d(d - d8)
    kept = [p for p, dk in zip(pairs, d) if dk <= d8]
    pa, pb = gather(kept) if kept else (np.zeros((0, 3)), np.zeros((0, 3)))
    tm_a = _np_search(pa, pb, La, _np_d0(La), 1, mg)[0]
    tm_b, Rb, tb = _np_search(pa, pb, Lb, _np_d0(Lb), 1, mg)
    amap = -np.ones(La, np.int64)
    for i, j in kept:
        amap[i] = j
    rmsd = float(np.sqrt(np.mean(((pa @ Rb.T + tb - pb) ** 2).sum(-1)))) if kept else NAN
    res.update(num_aligned=float(len(kept)), tm_norm_a=tm_a, tm_norm_b=tm_b, rmsd=rmsd, best_class=float(cls), search_tm=top,
               map=amap, R=Rb, t=tb, search_R=R, search_t=t, d8=d8, margin_dist=mg.dist, margin_score=mg.score)
    return res


@functools.lru_cache(maxsize=None)
def _np_case(kind, La, Lb):
    a, b = _pair(kind, La, Lb, SEEDS.get((kind, La, Lb), 0))
    ref = _np_align(a, b)
    # (what makes the exact comparisons sound; no case is skipped for missing it -- the seeds above were chosen to meet it)
    assert ref["margin_dist"] >= MARGIN_DIST and ref["margin_score"] >= MARGIN_SCORE, (kind, La, Lb, ref["margin_dist"], ref["margin_score"])
    return a, b, ref


@functools.lru_cache(maxsize=None)
def _chains():
    z = np.load(os.path.join(ROOT, "tests", "golden", "dssp_chains.npz"))
    return {name: np.ascontiguousarray(z[f"{name}_xyz"][:, 1]) for name in ("6MRR", "5L33", "3HTN")}


@functools.lru_cache(maxsize=None)
def _np_chain_case(na, nb):
    ref = _np_align(_chains()[na], _chains()[nb])
    assert ref["margin_dist"] >= MARGIN_DIST and ref["margin_score"] >= MARGIN_SCORE, (na, nb, ref["margin_dist"], ref["margin_score"])
    return ref


# ---- helpers ------------------------------------------------------------------------------------------------------------------------
def _t(x, dev):
    return torch.as_tensor(np.ascontiguousarray(x)).to(dev)


def _same_bits(a, b):
    bits = lambda x: x.contiguous().view(torch.int64) if x.dtype == torch.float64 else x
    return a.keys() == b.keys() and all(torch.equal(bits(a[k]), bits(b[k])) for k in a)


def _entry(res, p):
    return {k: v[p] for k, v in res.items()}


def _err(got, ref):
    got, ref = np.asarray(got, np.float64).reshape(-1), np.asarray(ref, np.float64).reshape(-1)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (got, ref)
    ok = ~np.isnan(ref)
    return float(np.max(np.abs(got[ok] - ref[ok]) / np.maximum(1.0, np.abs(ref[ok])))) if ok.any() else 0.0


def _check(key, got, ref, bound=REL):
    e = _err(got, ref)
    parity_log.out(key, e)
    print(f"  {key}: achieved {e:.3e} (bound {bound:.0e})")
    assert e <= bound, (key, e, got, ref)


def _check_against(tag, res, ref, ridx_a=None, ridx_b=None):
    """one (unbatched) tm_align result against one restatement; ridx: compacted -> original index of a masked call"""
    print(f"  {tag}: La {ref['La']:.0f} Lb {ref['Lb']:.0f} aligned {ref['num_aligned']:.0f} tm_a {ref['tm_norm_a']:.6f} tm_b "
          f"{ref['tm_norm_b']:.6f} class {ref['best_class']:.0f} {ref['class_s']} DPs {ref['num_dp']:.0f} units {ref['num_units']:.0f} "
          f"margin {ref['margin_dist']:.2e} A / {ref['margin_score']:.2e}")
    for k in EXACT:
        assert res[k].item() == ref[k], (tag, k, res[k].item(), ref[k])
    want = ref["map"]
    if ridx_a is not None:
        full = -np.ones(res["map"].shape[-1], np.int64)
        full[ridx_a] = np.where(want >= 0, ridx_b[np.maximum(want, 0)], -1)
        want = full
    assert np.array_equal(res["map"].cpu().numpy(), want), (tag, res["map"].cpu().numpy(), want)
    for k in SCALARS:
        _check(f"{tag}.{k}", res[k].item(), ref[k])
    if "R" in res and ref["R"] is not None:
        eR = float(np.abs(res["R"].cpu().numpy() - ref["R"]).max())
        et = float(np.abs(res["t"].cpu().numpy() - ref["t"]).max())
        parity_log.out(f"{tag}.R_abs", eR)
        parity_log.out(f"{tag}.t_abs", et)
        print(f"  {tag}: R {eR:.3e} t {et:.3e} (bound 1e-08)")
        assert eR <= 1e-8 and et <= 1e-8, (tag, eR, et)


def _tm_formula(a, b, amap, R, t, L):
    """the TM formula of the pairs in amap under (R, t), normalised by L"""
    i = np.nonzero(amap >= 0)[0]
    d2 = ((a[i].astype(np.float64) @ R.T + t - b[amap[i]].astype(np.float64)) ** 2).sum(-1)
    return float(np.sum(1.0 / (1.0 + d2 / _np_d0(L) ** 2)) / L)


def _check_map_shape(amap, Lb):
    hit = amap[amap >= 0]
    assert (np.diff(hit) > 0).all() and (hit < Lb).all()          # strictly increasing, hence one-to-one


# ---- 0. the restatement's two DP fills agree (CPU only) ----------------------------------------------------------------------------
def test_restatement_dp_forms_agree():
    rng = np.random.default_rng(3)
    for La, Lb, gap in ((7, 5, -0.6), (13, 21, 0.0), (30, 17, -1.0)):
        S = rng.random((La, Lb)) if gap != -1.0 else rng.integers(0, 2, (La, Lb)).astype(np.float64)
        v0, p0 = _np_dp_cells(S, gap)
        v1, p1 = _np_dp_fill(S, gap)
        assert np.array_equal(v0, v1) and np.array_equal(p0, p1)


# ---- 1. restatement parity ----------------------------------------------------------------------------------------------------------
def _run_parity(dev, La, Lb):
    with parity_log.case(f"tm_align_parity_{La}x{Lb}[{dev}]"):
        cases = [_np_case(kind, La, Lb) for kind in KINDS]
        a = np.stack([c[0] for c in cases])
        b = np.stack([c[1] for c in cases])
        res = fm.tm_align(_t(a, dev), _t(b, dev), return_transform=True)
        assert list(res) == list(fm.TM_ALIGN_SLOTS) + ["map", "R", "t"]
        assert all(res[k].shape == (3,) and res[k].dtype == torch.float64 for k in fm.TM_ALIGN_SLOTS)
        assert res["map"].shape == (3, La) and res["map"].dtype == torch.int32
        assert res["R"].shape == (3, 3, 3) and res["t"].shape == (3, 3)
        for p, kind in enumerate(KINDS):
            _check_against(f"{kind}{La}x{Lb}", _entry(res, p), cases[p][2])
            assert res["num_units"][p].item() == fm.tm_align_units(La, Lb)


@pytest.mark.parametrize("La,Lb", SIZES)
def test_parity_emu(use_emu, La, Lb):
    _run_parity("cpu", La, Lb)


@pytest.mark.gpu
@pytest.mark.parametrize("La,Lb", SIZES)
def test_parity_gpu(hip_lib, La, Lb):
    _run_parity("cuda", La, Lb)


def test_parity_set_covers_three_classes():
    """a condition on the chosen inputs: over the parity set at least three different classes win in the restatement"""
    won = {_np_case(kind, La, Lb)[2]["best_class"] for kind in KINDS for La, Lb in SIZES}
    print(f"  winning classes over the parity set: {sorted(won)}")
    assert len(won - {-1.0}) >= 3, won


# ---- 2. real chains -----------------------------------------------------------------------------------------------------------------
CHAIN_PAIRS = (("6MRR", "5L33"), ("6MRR", "3HTN"), ("5L33", "3HTN"))


def _run_chains(dev, pairs):
    with parity_log.case(f"tm_align_chains[{dev}]"):
        for na, nb in pairs:
            ref = _np_chain_case(na, nb)
            res = fm.tm_align(_t(_chains()[na], dev), _t(_chains()[nb], dev), return_transform=True)
            _check_against(f"{na}_{nb}", res, ref)
            assert 0.2 < ref["tm_norm_a"] < 0.6            # unrelated folds of 68 to 140 residues


def test_chains_emu(use_emu):
    _run_chains("cpu", CHAIN_PAIRS)


@pytest.mark.gpu
def test_chains_gpu(hip_lib):
    _run_chains("cuda", CHAIN_PAIRS)


# ---- 3. analytic properties ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _analytic_inputs():
    rng = np.random.default_rng(23)
    a = _walk(rng, 80).astype(np.float32)
    a64 = a.astype(np.float64)
    sub = _move(rng, a64[20:55]).astype(np.float32)
    keep = np.r_[0:30, 40:80]
    cut = _move(rng, a64[keep]).astype(np.float32)
    noisy = _move(rng, a64[keep], 0.6).astype(np.float32)
    return a, sub, cut, noisy, keep


def _run_analytic(dev):
    with parity_log.case(f"tm_align_analytic[{dev}]"):
        a, sub, cut, noisy, keep = _analytic_inputs()
        run = lambda x, y: {k: (v.item() if v.dim() == 0 else v.cpu().numpy())
                            for k, v in fm.tm_align(_t(x, dev), _t(y, dev), return_transform=True).items()}
        # b is the rounded image of part of a: |b_k - (R a_k + t)| ~ 1e-5 A, so 1 - tm <= (1e-5 / d0)^2 < 1e-9
        r = run(a, sub)
        _check("sub.tm_norm_b", r["tm_norm_b"], 1.0)
        _check("sub.tm_norm_a", r["tm_norm_a"], 35.0 / 80.0)
        assert np.array_equal(r["map"], np.r_[-np.ones(20), np.arange(35), -np.ones(25)])        # the exact shift
        r = run(a, cut)
        _check("cut.tm_norm_b", r["tm_norm_b"], 1.0)
        want = -np.ones(80, np.int64)
        want[keep] = np.arange(70)
        assert np.array_equal(r["map"], want)              # the deletion is recovered exactly
        r = run(a, noisy)
        assert np.array_equal(r["map"], want) and r["num_aligned"] == 70.0
        print(f"  deletion + 1 A noise: tm_norm_b {r['tm_norm_b']:.4f}")
        assert 0.7 < r["tm_norm_b"] < 0.95
        r = run(a, a)
        _check("same.tm_norm_a", r["tm_norm_a"], 1.0)
        _check("same.tm_norm_b", r["tm_norm_b"], 1.0)
        assert np.array_equal(r["map"], np.arange(80))
        # every map is increasing and one-to-one, every kept pair lies within d8, and the formula under (R, t) gives slot 4
        for x, y in ((a, sub), (a, cut), (a, noisy), _np_case("unrelated", 40, 63)[:2], _np_case("domain", 40, 63)[:2]):
            r = run(x, y)
            _check_map_shape(r["map"], len(y))
            assert r["num_aligned"] == (r["map"] >= 0).sum()
            _check("formula.tm_norm_b", _tm_formula(x, y, r["map"], r["R"], r["t"], len(y)), r["tm_norm_b"])
            assert r["tm_norm_a"] <= 1.0 + 1e-12 and r["tm_norm_b"] <= 1.0 + 1e-12
        # ... within d8 under the SEARCH-phase superposition, which the restatement returns (the kernel's is within 1e-8 of it)
        a4, b4, ref = _np_case("unrelated", 40, 63)
        r = run(a4, b4)
        i = np.nonzero(r["map"] >= 0)[0]
        d = np.sqrt(((a4[i].astype(np.float64) @ ref["search_R"].T + ref["search_t"] - b4[r["map"][i]].astype(np.float64)) ** 2).sum(-1))
        assert (d <= ref["d8"]).all()


def test_analytic_emu(use_emu):
    _run_analytic("cpu")


@pytest.mark.gpu
def test_analytic_gpu(hip_lib):
    _run_analytic("cuda")


# ---- 4. masks and padding -----------------------------------------------------------------------------------------------------------
def _run_masks(dev):
    with parity_log.case(f"tm_align_masks[{dev}]"):
        a, b, ref = _np_case("insert", 21, 22)
        rng = np.random.default_rng(11)
        Na, Nb = 37, 30
        keep_a, keep_b = np.sort(rng.choice(Na, size=21, replace=False)), np.sort(rng.choice(Nb, size=22, replace=False))
        ma, mb = np.zeros(Na, np.float32), np.zeros(Nb, np.float32)
        ma[keep_a] = rng.choice([1.0, -2.5, 7.0], size=21)       # any non-zero value counts
        mb[keep_b] = 1.0
        A, B = rng.normal(size=(Na, 3)).astype(np.float32) * 9, rng.normal(size=(Nb, 3)).astype(np.float32) * 9
        A[keep_a], B[keep_b] = a, b
        packed = fm.tm_align(_t(a, dev), _t(b, dev), return_transform=True)
        masked = fm.tm_align(_t(A, dev), _t(B, dev), _t(ma, dev), _t(mb, dev), return_transform=True)
        assert packed["tm_norm_b"].dim() == 0 and packed["map"].shape == (21,) and masked["map"].shape == (Na,)
        no_map = lambda r: {k: v for k, v in r.items() if k != "map"}
        assert _same_bits(no_map(packed), no_map(masked))          # the results of the compacted chains, bit for bit
        _check_against("masked21x22", masked, ref, keep_a, keep_b)   # ... and the map in ORIGINAL indices
        # NaN (and infinite) bit patterns at the padded / masked-out positions change nothing
        A2, B2 = A.copy(), B.copy()
        A2[ma == 0], B2[mb == 0] = np.nan, -np.inf
        assert _same_bits(masked, fm.tm_align(_t(A2, dev), _t(B2, dev), _t(ma, dev), _t(mb, dev), return_transform=True))


def test_masks_emu(use_emu):
    _run_masks("cpu")


@pytest.mark.gpu
def test_masks_gpu(hip_lib):
    _run_masks("cuda")


# ---- 5. determinism -----------------------------------------------------------------------------------------------------------------
def _pad(x, n):
    return np.concatenate([x, np.full((n - len(x), 3), np.nan, np.float32)])


def _run_determinism(dev):
    a, b, _ = _np_case("unrelated", 21, 22)
    a2, b2, _ = _np_case("domain", 12, 11)
    ta, tb = _t(a, dev), _t(b, dev)
    runs = [fm.tm_align(ta, tb, return_transform=True, parts=parts) for parts in (1, 3, None, None, 40)]
    assert all(_same_bits(runs[0], r) for r in runs[1:])         # parts, and twice the same; 40: blocks without a unit
    # the pair alone and inside a batch of unequal pairs (padded and masked)
    A = np.stack([_pad(a2, 21), a, _pad(a[:9], 21)])
    B = np.stack([_pad(b2, 22), b, _pad(b[:17], 22)])
    ma, mb = np.zeros((3, 21), np.float32), np.zeros((3, 22), np.float32)
    ma[0, :12], ma[1], ma[2, :9] = 1, 1, 1
    mb[0, :11], mb[1], mb[2, :17] = 1, 1, 1
    batch = fm.tm_align(_t(A, dev), _t(B, dev), _t(ma, dev), _t(mb, dev), return_transform=True)
    assert _same_bits(runs[0], _entry(batch, 1))
    assert batch["La"].tolist() == [12.0, 21.0, 9.0] and batch["Lb"].tolist() == [11.0, 22.0, 17.0]
    assert fm.tm_align_parts(1, 21, 22) == -(-fm.tm_align_units(21, 22) // 4) and fm.tm_align_parts(4096, 128, 128) == 1
    assert fm.tm_align_parts(2, 3, 9) == 1 and fm.tm_align_units(4, 100) == 0 and fm.tm_align_units(5, 5) == 1


def test_determinism_emu(use_emu):
    _run_determinism("cpu")


@pytest.mark.gpu
def test_determinism_gpu(hip_lib):
    _run_determinism("cuda")


# ---- 6. short and degenerate --------------------------------------------------------------------------------------------------------
def _run_short(dev, lib):
    a, b, _ = _np_case("unrelated", 21, 22)
    ma, mb = np.zeros((3, 21), np.float32), np.ones((3, 22), np.float32)
    ma[1, 7] = 1                                                 # Lmin = 0, 1, 4
    ma[2, [2, 3, 9, 20]] = 1
    res = fm.tm_align(_t(np.stack([a] * 3), dev), _t(np.stack([b] * 3), dev), _t(ma, dev), _t(mb, dev), return_transform=True)
    assert res["La"].tolist() == [0.0, 1.0, 4.0] and res["Lb"].tolist() == [22.0] * 3
    for k in ("tm_norm_a", "tm_norm_b", "rmsd", "search_tm"):
        assert bool(torch.isnan(res[k]).all()), k
    assert res["best_class"].tolist() == [-1.0] * 3 and res["num_aligned"].tolist() == [0.0] * 3
    assert res["num_dp"].tolist() == [0.0] * 3 and res["num_units"].tolist() == [0.0] * 3
    assert res["d0_a"].tolist() == [0.5] * 3 and bool((res["map"] == -1).all())
    _check("short.d0_b", res["d0_b"][0].item(), _np_d0(22))
    # P == 0: nothing is launched
    n0 = lib.cdll.fd_launch_count()
    empty = fm.tm_align(_t(np.zeros((0, 21, 3), np.float32), dev), _t(np.zeros((0, 22, 3), np.float32), dev))
    assert empty["tm_norm_b"].shape == (0,) and empty["map"].shape == (0, 21) and lib.cdll.fd_launch_count() == n0
    # a non-finite coordinate among the counting positions: candidates that contain it never win, so the residue stays unaligned;
    # the call ends, twice with the same bits, and what it reports is a score of the remaining residues
    a2 = a.copy()
    a2[7, 1] = np.nan
    r1, r2 = (fm.tm_align(_t(a2, dev), _t(b, dev), return_transform=True) for _ in range(2))
    assert _same_bits(r1, r2) and r1["map"][7].item() == -1 and r1["La"].item() == 21.0
    tm = r1["tm_norm_b"].item()
    assert np.isnan(tm) or 0.0 <= tm <= 1.0
    if not np.isnan(tm):
        _check_map_shape(r1["map"].cpu().numpy(), 22)


def test_short_emu(use_emu):
    _run_short("cpu", use_emu)


@pytest.mark.gpu
def test_short_gpu(hip_lib):
    _run_short("cuda", hip_lib)


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------------
def _run_refusals(dev, lib):
    f32 = lambda *s: torch.zeros(s, device=dev)
    f64 = lambda *s: torch.full(s, NAN, dtype=torch.float64, device=dev)
    n0 = lib.cdll.fd_launch_count()
    with pytest.raises(ValueError, match="1024"):
        fm.tm_align(f32(1, 1025, 3), f32(1, 8, 3))
    with pytest.raises(ValueError, match="1024"):
        fm.tm_align(f32(1, 8, 3), f32(1, 1025, 3))
    with pytest.raises(hip.FdError, match="search_step"):
        fm.tm_align(f32(1, 8, 3), f32(1, 8, 3), search_step=0)
    with pytest.raises(hip.FdError, match="max_dp"):
        fm.tm_align(f32(1, 8, 3), f32(1, 8, 3), max_dp=-1)
    with pytest.raises(hip.FdError, match="parts"):
        fm.tm_align(f32(1, 8, 3), f32(1, 8, 3), parts=0)
    out, tr, ws = f64(2, 16), f64(2, 12), f64(fm.tm_align_ws_bytes(2, 1, 8, 9) // 8 + 1)
    amap = torch.full((2, 8), 7, dtype=torch.int32, device=dev)
    pts = (f32(2, 8, 3), 3, 8, f32(2, 9, 3), 3, 9)
    idx = torch.zeros(2, dtype=torch.int32, device=dev)
    call = lambda *rest: lib.call("fd_tm_align", *pts, *rest)
    with pytest.raises(hip.FdError, match="1024"):
        lib.call("fd_tm_align", f32(2, 8, 3), 3, 1025, f32(2, 9, 3), 3, 9, None, None, None, None, 2, 40, 30, 1, ws, out, amap, tr)
    with pytest.raises(hip.FdError, match="workspace"):
        call(None, None, None, None, 2, 40, 30, 1, None, out, amap, tr)
    with pytest.raises(hip.FdError, match="null out or map"):
        call(None, None, None, None, 2, 40, 30, 1, ws, None, amap, tr)
    with pytest.raises(hip.FdError, match="null out or map"):
        call(None, None, None, None, 2, 40, 30, 1, ws, out, None, tr)
    with pytest.raises(hip.FdError, match="together"):
        call(idx, None, None, None, 2, 40, 30, 1, ws, out, amap, tr)
    call(None, None, None, None, 0, 40, 30, 1, ws, out, amap, tr)                  # P == 0
    lib.call("fd_tm_align", f32(2, 8, 3), 3, 0, f32(2, 9, 3), 3, 9, None, None, None, None, 2, 40, 30, 1, ws, out, amap, tr)   # Na == 0
    lib.call("fd_tm_align", f32(2, 8, 3), 3, 8, f32(2, 9, 3), 3, 0, None, None, None, None, 2, 40, 30, 1, ws, out, amap, tr)   # Nb == 0
    assert lib.cdll.fd_launch_count() == n0                                        # refused or empty: nothing was launched
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(tr).all()) and bool((amap == 7).all())       # ... and nothing written
    # the size macro of the header and its Python mirror
    assert fm.tm_align_ws_bytes(3, 2, 100, 70) == 3 * 2 * 4 * 32 * 8 + 3 * 4 * 16 * 8 + 3 * 2 * 4 * 100 * 3 * 8 + 3 * 4 * 2 * 100 * 2


def test_refusals_emu(use_emu):
    _run_refusals("cpu", use_emu)


@pytest.mark.gpu
def test_refusals_gpu(hip_lib):
    _run_refusals("cuda", hip_lib)


# ---- 8. layouts ---------------------------------------------------------------------------------------------------------------------
def _run_layouts(dev):
    rng = np.random.default_rng(13)
    a = np.stack([_np_case(kind, 21, 22)[0] for kind in KINDS[:2]])
    b = np.stack([_np_case(kind, 21, 22)[1] for kind in KINDS[:2]])
    pa, pb = _t(a, dev), _t(b, dev)
    a37 = _t(rng.normal(size=(2, 21, 37, 3)).astype(np.float32), dev)
    b37 = _t(rng.normal(size=(2, 22, 37, 3)).astype(np.float32), dev)
    a37[:, :, 1], b37[:, :, 1] = pa, pb
    va, vb = a37[:, :, 1], b37[:, :, 1]
    assert not va.is_contiguous() and fm._points(va)[0].data_ptr() == va.data_ptr() and fm._points(va)[1] == 111
    packed = fm.tm_align(pa, pb, return_transform=True)
    assert _same_bits(packed, fm.tm_align(va, vb, return_transform=True))          # both strided, read in place
    assert _same_bits(packed, fm.tm_align(va, pb, return_transform=True))
    assert _same_bits(packed, fm.tm_align(pa, vb, return_transform=True))


def test_layouts_emu(use_emu):
    _run_layouts("cpu")


@pytest.mark.gpu
def test_layouts_gpu(hip_lib):
    _run_layouts("cuda")


# ---- 9. the matrix ------------------------------------------------------------------------------------------------------------------
def _run_matrix(dev, lengths):
    rng = np.random.default_rng(29)
    N = max(lengths)
    pos = np.stack([_pad(_walk(rng, L).astype(np.float32), N) for L in lengths])
    mask = np.stack([(np.arange(N) < L).astype(np.float32) for L in lengths])
    tp, tmk = _t(pos, dev), _t(mask, dev)
    M = len(lengths)
    both = fm.tm_align_matrix(tp, tmk)
    assert set(both) == {"tm_norm_a", "tm_norm_b"} and both["tm_norm_a"].shape == (M, M) and both["tm_norm_a"].dtype == torch.float64
    assert torch.equal(both["tm_norm_a"], both["tm_norm_b"].T)                 # the mirrored half swaps the normalisations
    assert both["tm_norm_a"].diagonal().tolist() == [1.0] * M
    bits = lambda x: x.contiguous().view(torch.int64)
    for i in range(M):
        for j in range(i + 1, M):
            one = fm.tm_align(tp[i, :lengths[i]], tp[j, :lengths[j]])            # each entry equals the pair call, bit for bit
            assert torch.equal(bits(one["tm_norm_a"][None]), bits(both["tm_norm_a"][i, j][None]))
            assert torch.equal(bits(one["tm_norm_b"][None]), bits(both["tm_norm_b"][i, j][None]))
    # two sets: rows against columns
    cross = fm.tm_align_matrix(tp[:2], tmk[:2], tp[1:], tmk[1:])
    assert cross["tm_norm_a"].shape == (2, M - 1)
    assert torch.equal(bits(cross["tm_norm_a"][0, 1:]), bits(both["tm_norm_a"][0, 2:]))
    assert torch.equal(bits(cross["tm_norm_b"][1, 1:]), bits(both["tm_norm_b"][1, 2:]))
    assert abs(cross["tm_norm_a"][1, 0].item() - 1.0) <= 1e-9                  # set 1 against itself


def test_matrix_emu(use_emu):
    _run_matrix("cpu", (40, 63, 64, 97))


@pytest.mark.gpu
def test_matrix_gpu(hip_lib):
    _run_matrix("cuda", (40, 63, 64, 97))


# ---- 10. eval_rows ------------------------------------------------------------------------------------------------------------------
def _run_eval_rows(dev):
    with parity_log.case(f"tm_align_eval_rows[{dev}]"):
        rng = np.random.default_rng(17)
        a, b, ref = _np_case("insert", 21, 22)
        s37 = rng.normal(size=(2, 24, 37, 3)).astype(np.float32)
        g37 = rng.normal(size=(2, 24, 37, 3)).astype(np.float32)
        # backbone 0: 24 random residues, all scored; backbone 1: two fixed residues and one absent, the 21 scored ones are a
        # against b[:21]
        s37[1, 2:23, 1], g37[1, 2:23, 1] = a, b[:21]
        res_mask = np.ones((2, 24), np.float32)
        res_mask[1, 23] = 0
        fixed = np.zeros((2, 24), np.float32)
        fixed[1, :2] = 1
        args = (_t(s37, dev), _t(res_mask, dev), _t(fixed, dev), _t(g37, dev))
        plain, with_tm, with_align = fm.eval_rows(*args), fm.eval_rows(*args, tm=True), fm.eval_rows(*args, tm="align")
        today = set(fm.BACKBONE_SLOTS) | {"fixed_residues", "diffused_percentage", "aligned_rmsd_to_gt"}
        same = lambda r0, r1: all(r0[k] == r1[k] or (np.isnan(r0[k]) and np.isnan(r1[k])) for k in r0)
        for r0, r1, r2 in zip(plain, with_tm, with_align):
            assert set(r0) == today and set(r1) == today | {"tm_score_to_gt"} and set(r2) == today | {"tm_align_to_gt"}
            assert same(r0, r1) and same(r0, r2)                                   # the other columns: untouched
        # eval_rows() and eval_rows(tm=True) against the existing functions
        diffused = (1 - fixed) * res_mask
        direct = fm.tm_score(_t(s37, dev)[:, :, 1], _t(g37, dev)[:, :, 1], _t(diffused, dev))
        assert [r["tm_score_to_gt"] for r in with_tm] == direct["tm_score"].tolist()
        kab = fm.aligned_rmsd(_t(s37, dev)[:, :, 1], _t(g37, dev)[:, :, 1], _t(diffused, dev))
        assert [r["aligned_rmsd_to_gt"] for r in plain] == kab["mean_dist"].tolist()
        bbm = fm.backbone_metrics(_t(s37, dev), _t(res_mask, dev))
        assert all(np.array_equal([r[k] for r in plain], bbm[k].tolist(), equal_nan=True) for k in fm.BACKBONE_SLOTS)
        # tm_align_to_gt against the restatement of a against b[:21]
        ref21 = _np_align(a, b[:21])
        assert ref21["margin_dist"] >= MARGIN_DIST and ref21["margin_score"] >= MARGIN_SCORE
        _check("eval_rows.tm_align_to_gt", with_align[1]["tm_align_to_gt"], ref21["tm_norm_b"])
        al = fm.tm_align(_t(s37, dev)[:, :, 1], _t(g37, dev)[:, :, 1], _t(diffused, dev), _t(diffused, dev))
        assert [r["tm_align_to_gt"] for r in with_align] == al["tm_norm_b"].tolist()
        no_gt = fm.eval_rows(*args[:3], tm="align")
        assert all("tm_align_to_gt" not in r for r in no_gt)


def test_eval_rows_emu(use_emu):
    _run_eval_rows("cpu")


@pytest.mark.gpu
def test_eval_rows_gpu(hip_lib):
    _run_eval_rows("cuda")
