"""Secondary structure and the shape columns on the device (fd_dssp_hbonds / fd_dssp_assign, se3_diffusion_amd.metrics
.secondary_structure / ss_string / eval_rows(shape=True), sampler.sample(metrics="shape")).

The reference of every case is a float64 numpy restatement, written here with plain loops, of the algorithm that include/fd_hip.h
specifies (Kabsch & Sander in the order the DSSP program applies it).  It shares nothing with the kernels.  Neither a DSSP
program nor mdtraj is available to this suite: agreement with the letters md.compute_dssp prints is NOT checked here.  What
stands in for it is one plausibility condition against the HELIX / SHEET records of the six deposited structures of
tests/golden/dssp_chains.npz (tools/make_dssp_fixture.py): three-class agreement >= 0.88 and a strand fraction within 0.05, on
the restatement and on the kernels' result alike -- it catches a wrong sign or an off-by-one in the specification itself.

Bounds, the same on the interpreter and on the device: acc_idx, ss, ss3, num_res, num_hbonds, overflow exactly; acc_e, the
percentages and radius_of_gyration within 1e-9 * max(1, |ref|) (the project's bound for its fp64 metrics: both sides compute in
float64 from identical float32 inputs).  The exact comparisons are sound because the restatement also returns its margin -- the
smallest of |E + 0.5|, |d_CA - 9|, |d - 0.5| over the four distances of an energy, the gaps between a donor's first, second and
third energies (exact ties of clamped energies aside: those go to the lower index on both sides), |d_CN - 2.5| and
|kappa - 70 degrees| over everything it evaluated -- and every case asserts margin >= 1e-6.  Each case reports what it achieved
through parity_log (expected: <= 1e-12)."""
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
MARGIN = 1e-6
NAN = float("nan")
G = np.load(os.path.join(ROOT, "tests", "golden", "dssp_chains.npz"))
NAMES = tuple(str(x) for x in G["names"])         # 4GYT 177, 4YOW 227, 6MRR 68, 3HTN 140 (3 breaks), 5L33 106, 6EHB 318 (1 break)
LETTERS = " HBEGITS"


# ---- the float64 restatement of include/fd_hip.h (plain loops, no cleverness) --------------------------------------------------------
def _np_dssp(atoms, mask=None, no_donor=None):
    """atoms float32 [N,A,3] (N, CA, C, CB, O first), mask [N], no_donor [N] -> dict: ss, ss3 int8 [N]; the SHAPE_SLOTS; acc_idx
    [N,2], acc_e [N,2]; margin; below (number of acceptors with E < -0.5 per donor, over ALL its candidates)"""
    N = len(atoms)
    x = atoms.astype(np.float64)
    if mask is None:
        mask = (atoms != 0).reshape(N, -1).any(-1)
    idx = [r for r in range(N) if mask[r] != 0]
    n = len(idx)
    at = lambda i, slot: x[idx[i], slot]
    Nn, CA, C, O = (lambda i: at(i, 0)), (lambda i: at(i, 1)), (lambda i: at(i, 2)), (lambda i: at(i, 4))
    dist = lambda p, q: float(np.sqrt(((p - q) ** 2).sum()))
    margin = [np.inf]

    def near(v, what=None):
        margin[0] = min(margin[0], abs(v))

    brk = []
    for a in range(n - 1):
        if idx[a + 1] != idx[a] + 1:
            brk.append(True)
        else:
            d = dist(C(a), Nn(a + 1))
            near(d - 2.5)
            brk.append(d > 2.5)

    def nobreak(a, b):
        if a < 0 or b >= n or a > b:
            return False
        return not any(brk[a:b])

    # energies and the two best acceptors
    kept = [[] for _ in range(n)]
    below = [0] * n
    for i in range(1, n):
        if brk[i - 1] or (no_donor is not None and no_donor[idx[i]] != 0):
            continue
        u = C(i - 1) - O(i - 1)
        H = Nn(i) + u / np.sqrt((u ** 2).sum())
        cands = []
        for j in range(n):
            if j == i or j == i - 1:
                continue
            dca = dist(CA(i), CA(j))
            near(dca - 9.0)
            if not dca < 9.0:
                continue
            ds = (dist(Nn(i), O(j)), dist(H, C(j)), dist(H, O(j)), dist(Nn(i), C(j)))
            for d in ds:
                near(d - 0.5)
            e = 27.888 * (1.0 / ds[0] + 1.0 / ds[1] - 1.0 / ds[2] - 1.0 / ds[3])
            if min(ds) < 0.5:
                e = -9.9
            e = max(e, -9.9)
            near(e + 0.5)
            cands.append((e, j))
        cands.sort()
        for k in range(min(2, len(cands) - 1)):
            if not (cands[k][0] == cands[k + 1][0] == -9.9):
                near(cands[k + 1][0] - cands[k][0])
        kept[i] = cands[:2]
        below[i] = sum(1 for e, _ in cands if e < -0.5)

    def hb(a, b):
        return any(j == b and e < -0.5 for e, j in kept[a])

    def turn(k, i):
        return i >= 0 and i + k < n and hb(i + k, i) and nobreak(i, i + k)

    def bridge(i, j):
        if i < 1 or j < i + 3 or j > n - 2:
            return 0
        if not (nobreak(i - 1, i + 1) and nobreak(j - 1, j + 1)):
            return 0
        if (hb(i + 1, j) and hb(j, i - 1)) or (hb(j + 1, i) and hb(i, j - 1)):
            return 1
        if (hb(i + 1, j - 1) and hb(j + 1, i - 1)) or (hb(j, i) and hb(i, j)):
            return 2
        return 0

    ladders = []                                  # (type, i-start, i-end, j-start, j-end) with start <= end on both strands
    for i in range(1, n):
        for j in range(i + 3, n - 1):
            t = bridge(i, j)
            if t == 0:
                continue
            step = 1 if t == 1 else -1
            if bridge(i - 1, j - step) == t:
                continue
            ln = 1
            while bridge(i + ln, j + step * ln) == t:
                ln += 1
            ladders.append((t, i, i + ln - 1, j, j + ln - 1) if t == 1 else (t, i, i + ln - 1, j - ln + 1, j))

    def linked(A, B):
        if A[0] != B[0]:
            return False
        if B[1] < A[1]:
            A, B = B, A
        gi = B[1] - A[2] - 1
        if A[0] == 1:
            gj, lo, hi = B[3] - A[4] - 1, A[4], B[3]
        else:
            gj, lo, hi = A[3] - B[4] - 1, B[4], A[3]
        if gi < 0 or gj < 0:
            return False
        if not ((gi <= 1 and gj <= 4) or (gi <= 4 and gj <= 1)):
            return False
        return nobreak(A[2], B[1]) and nobreak(lo, hi)

    group = list(range(len(ladders)))
    moved = True
    while moved:                                  # transitive closure, the slow way
        moved = False
        for a in range(len(ladders)):
            for b in range(len(ladders)):
                if group[a] != group[b] and linked(ladders[a], ladders[b]):
                    g = min(group[a], group[b])
                    old = max(group[a], group[b])
                    group = [g if v == old else v for v in group]
                    moved = True
    ss = [0] * n
    for want in (2, 3):                           # B first, then E over it
        for g in sorted(set(group)):
            mem = [ladders[k] for k in range(len(ladders)) if group[k] == g]
            bridges = sum(m[2] - m[1] + 1 for m in mem)
            if (3 if bridges > 1 else 2) != want:
                continue
            for r in range(min(m[1] for m in mem), max(m[2] for m in mem) + 1):
                ss[r] = want
            for r in range(min(m[3] for m in mem), max(m[4] for m in mem) + 1):
                ss[r] = want
    for i in range(1, n):
        if turn(4, i - 1) and turn(4, i):
            for k in range(4):
                ss[i + k] = 1
    for code, k in ((4, 3), (5, 5)):
        for i in range(1, n):
            if turn(k, i - 1) and turn(k, i) and all(ss[i + q] in (0, code) for q in range(k)):
                for q in range(k):
                    ss[i + q] = code
    for i in range(n):
        if ss[i] == 0 and any(turn(k, q) for k in (3, 4, 5) for q in range(i - k + 1, i)):
            ss[i] = 6
    for i in range(n):
        if nobreak(i - 2, i + 2):
            u, v = CA(i) - CA(i - 2), CA(i + 2) - CA(i)
            kappa = float(np.degrees(np.arccos(np.clip((u * v).sum() / np.sqrt((u ** 2).sum() * (v ** 2).sum()), -1.0, 1.0))))
            near(kappa - 70.0)
            if ss[i] == 0 and kappa > 70.0:
                ss[i] = 7

    full = np.full(N, -1, np.int8)
    full[idx] = ss
    ss3 = np.full(N, -1, np.int8)
    ss3[idx] = [1 if c in (1, 4, 5) else 2 if c in (2, 3) else 0 for c in ss]
    nh, ne = int((ss3 == 1).sum()), int((ss3 == 2).sum())
    pts = x[idx].reshape(-1, 3)
    pts = pts[(pts != 0).any(-1)]
    with np.errstate(invalid="ignore", divide="ignore"):
        frac = lambda c: np.float64(c) / np.float64(n)
        rg = float(np.sqrt(((pts - pts.mean(0)) ** 2).sum(-1).mean()) / 10.0) if len(pts) else NAN
        res = dict(ss=full, ss3=ss3, num_res=float(n), helix_percent=float(frac(nh)), strand_percent=float(frac(ne)),
                   coil_percent=float(frac(n - nh - ne)), non_coil_percent=float(frac(nh + ne)), radius_of_gyration=rg,
                   num_hbonds=float(sum(1 for k in kept for e, _ in k if e < -0.5)), overflow=0.0)
    acc_idx, acc_e = np.full((N, 2), -1, np.int32), np.zeros((N, 2))
    for i in range(n):
        for k, (e, j) in enumerate(kept[i]):
            acc_idx[idx[i], k], acc_e[idx[i], k] = idx[j], e
    res.update(acc_idx=acc_idx, acc_e=acc_e, margin=margin[0], below={idx[i]: below[i] for i in range(n)}, ladders=ladders)
    return res


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------
def _with_cb(bb4):
    """[n,4,3] N, CA, C, O -> float32 [n,5,3] N, CA, C, CB, O with the ideal CB (it only enters the radius of gyration)"""
    b4 = bb4.astype(np.float64)
    b, c = b4[:, 1] - b4[:, 0], b4[:, 2] - b4[:, 1]
    cb = -0.58273431 * np.cross(b, c) + 0.56802827 * b - 0.54067466 * c + b4[:, 1]
    return np.stack([b4[:, 0], b4[:, 1], b4[:, 2], cb, b4[:, 3]], axis=1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _chain(name):
    """atoms [n,5,3], residue-index mask over the file's numbering gaps, proline flags"""
    return _with_cb(G[f"{name}_xyz"]), G[f"{name}_resnum"], G[f"{name}_pro"].astype(np.float32)


def _place(prev3, length, angle, torsion):
    """the point at `length` from c with angle (b, c, new) and torsion (a, b, c, new), degrees"""
    a, b, c = prev3
    bc = (c - b) / np.linalg.norm(c - b)
    nrm = np.cross(b - a, bc)
    nrm /= np.linalg.norm(nrm)
    m = np.cross(nrm, bc)
    ang, tor = np.radians(angle), np.radians(torsion)
    d = np.array([-np.cos(ang), np.sin(ang) * np.cos(tor), np.sin(ang) * np.sin(tor)])
    return c + length * (d[0] * bc + d[1] * m + d[2] * nrm)


def _build(phi, psi):
    """a backbone of standard bond geometry from its torsions (degrees): float32 [n,5,3]"""
    n = len(phi)
    N, CA, C, O = [np.zeros((n, 3)) for _ in range(4)]
    N[0], CA[0] = [0.0, 0.0, 0.0], [1.458, 0.0, 0.0]
    C[0] = CA[0] + 1.525 * np.array([-np.cos(np.radians(111.0)), np.sin(np.radians(111.0)), 0.0])
    for i in range(n):
        if i > 0:
            N[i] = _place((N[i - 1], CA[i - 1], C[i - 1]), 1.329, 116.2, psi[i - 1])
            CA[i] = _place((CA[i - 1], C[i - 1], N[i]), 1.458, 121.7, 180.0)
            C[i] = _place((C[i - 1], N[i], CA[i]), 1.525, 111.0, phi[i])
        O[i] = _place((N[i], CA[i], C[i]), 1.231, 120.5, psi[i] + 180.0)
    return _with_cb(np.stack([N, CA, C, O], axis=1) + 3.0)       # (shifted: no coordinate is exactly zero)


@functools.lru_cache(maxsize=None)
def _helix(n):
    return _build([-57.0] * n, [-47.0] * n)


@functools.lru_cache(maxsize=None)
def _coil(n):
    rng = np.random.default_rng([5, n])
    return _build(rng.uniform(-180.0, 180.0, n), rng.uniform(-180.0, 180.0, n))


@functools.lru_cache(maxsize=None)
def _ref(kind, key, variant=""):
    """one restatement per input, computed once, shared by the interpreter and the device runs, never modified"""
    if kind == "chain":
        atoms, _, pro = _chain(key)
        mask = np.ones(len(atoms), np.float32)
        if variant == "gap":
            mask[40:45] = 0
        inp = (atoms, mask, pro)
    elif kind == "helix":
        inp = (_helix(key), None, None)
    elif kind == "coil":
        inp = (_coil(key), None, None)
    else:
        inp = _three_acceptors()
    ref = _np_dssp(*inp)
    assert ref["margin"] >= MARGIN, (kind, key, variant, ref["margin"])        # (what makes the exact comparisons sound)
    return inp, ref


def _three_acceptors(offsets=((0.05, 0.0, 0.0), (0.0, -0.05, 0.0))):
    """A beta-hairpin segment of 6MRR plus copies of one acceptor residue, each displaced by one of `offsets` (Angstrom) and each
    behind a masked-out residue: with two copies 0.05 A away the donor bonded to it has three acceptors below -0.5 and keeps two."""
    atoms, _, pro = _chain("6MRR")
    base = _np_dssp(atoms, None, pro)
    ss3 = base["ss3"]
    donor = acc = None
    for i in range(len(atoms)):                                  # a strand residue whose best acceptor is a distant strand residue
        j = base["acc_idx"][i, 0]
        if ss3[i] == 2 and j >= 0 and ss3[j] == 2 and abs(i - j) > 3 and base["acc_e"][i, 0] < -1.5:
            donor, acc = i, int(j)
            break
    assert donor is not None
    lo, hi = max(0, min(donor, acc) - 6), min(len(atoms), max(donor, acc) + 7)
    parts = [atoms[lo:hi]]
    for off in offsets:
        parts += [np.full((1, 5, 3), np.nan, np.float32), atoms[acc:acc + 1] + np.array(off, np.float32)]
    both = np.concatenate(parts)
    mask = np.ones(len(both), np.float32)
    mask[hi - lo::2] = 0
    nd = np.zeros(len(both), np.float32)
    nd[:hi - lo] = pro[lo:hi]
    return both, mask, nd


# ---- helpers ------------------------------------------------------------------------------------------------------------------------
def _t(x, dev):
    return None if x is None else torch.as_tensor(np.ascontiguousarray(x)).to(dev)


def _err(got, ref):
    got, ref = np.asarray(got, np.float64).reshape(-1), np.asarray(ref, np.float64).reshape(-1)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (got, ref)
    ok = ~np.isnan(ref)
    return float(np.max(np.abs(got[ok] - ref[ok]) / np.maximum(1.0, np.abs(ref[ok])))) if ok.any() else 0.0


def _check(key, got, ref):
    e = _err(got, ref)
    parity_log.out(key, e)
    print(f"  {key}: achieved {e:.3e} (bound {REL:.0e})")
    assert e <= REL, (key, e, got, ref)


def _string(codes):
    return "".join("-" if c < 0 else LETTERS[c] for c in codes)


def _check_against(tag, res, p, ref):
    """entry p of a batched secondary_structure(return_hbonds=True) result against one restatement (of the first len(ref) residues)"""
    N = len(ref["ss"])
    got_ss = res["ss"][p].cpu().numpy()
    print(f"  {tag}: {_string(ref['ss'])}  margin {ref['margin']:.2e}")
    assert _string(got_ss[:N]) == _string(ref["ss"]), (tag, _string(got_ss[:N]))
    assert (got_ss[N:] == -1).all() and (res["ss3"][p].cpu().numpy()[N:] == -1).all()
    assert np.array_equal(res["ss3"][p].cpu().numpy()[:N], ref["ss3"]), tag
    assert np.array_equal(res["acc_idx"][p].cpu().numpy()[:N], ref["acc_idx"]), tag
    assert (res["acc_idx"][p].cpu().numpy()[N:] == -1).all()
    for k in ("num_res", "num_hbonds", "overflow"):
        assert res[k][p].item() == ref[k], (tag, k, res[k][p].item(), ref[k])
    _check(f"{tag}.acc_e", res["acc_e"][p].cpu().numpy()[:N], ref["acc_e"])
    for k in ("helix_percent", "strand_percent", "coil_percent", "non_coil_percent", "radius_of_gyration"):
        _check(f"{tag}.{k}", res[k][p].item(), ref[k])


def _call(dev, atoms, mask, nd, **kw):
    return fm.secondary_structure(_t(atoms, dev), _t(mask, dev), _t(nd, dev), return_hbonds=True, **kw)


def _plausible(tag, name, ss3):
    """the one condition against the file's own records: agreement >= 0.88, strand fraction within 0.05"""
    rec = np.array(["CHE".index(c) for c in str(G[f"{name}_ss"])])
    agree = float((ss3 == rec).mean())
    strand, strand_rec = float((ss3 == 2).mean()), float((rec == 2).mean())
    print(f"  {tag} {name}: agreement {agree:.3f} (>= 0.88), strand fraction {strand:.3f} against the records' {strand_rec:.3f}")
    assert agree >= 0.88 and abs(strand - strand_rec) <= 0.05, (name, agree, strand, strand_rec)


# ---- 1. the six chains, each alone, with their proline masks -----------------------------------------------------------------------
def _run_chain(dev, name):
    with parity_log.case(f"dssp_chain_{name}[{dev}]"):
        (atoms, mask, pro), ref = _ref("chain", name)
        res = _call(dev, atoms[None], mask[None], pro[None])
        assert res["ss"].dtype == torch.int8 and res["ss3"].dtype == torch.int8 and res["acc_idx"].dtype == torch.int32
        assert all(res[k].dtype == torch.float64 and res[k].shape == (1,) for k in fm.SHAPE_SLOTS)
        _check_against(name, res, 0, ref)
        _plausible("restatement", name, ref["ss3"])
        _plausible("kernels", name, res["ss3"][0].cpu().numpy())
        # again: identical bits
        again = _call(dev, atoms[None], mask[None], pro[None])
        assert all(torch.equal(res[k].view(torch.int64) if res[k].dtype == torch.float64 else res[k],
                               again[k].view(torch.int64) if again[k].dtype == torch.float64 else again[k]) for k in res)
        # without B, and the letters
        one = fm.secondary_structure(_t(atoms, dev), no_donor=_t(pro, dev))
        assert one["ss"].shape == (len(atoms),) and one["helix_percent"].dim() == 0 and "acc_idx" not in one
        assert fm.ss_string(one["ss"]) == _string(ref["ss"]) and fm.ss_string(res["ss"]) == [_string(ref["ss"])]
        assert fm.ss_string(one["ss3"], classes=True) == "".join("CHE"[c] for c in ref["ss3"])


@pytest.mark.parametrize("name", NAMES)
def test_chain_emu(use_emu, name):
    _run_chain("cpu", name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_chain_gpu(hip_lib, name):
    _run_chain("cuda", name)


# ---- 2. the padded batch; 3. a gap by mask ------------------------------------------------------------------------------------------
def _run_batch(dev):
    with parity_log.case(f"dssp_batch[{dev}]"):
        atoms = np.full((7, 320, 5, 3), np.nan, np.float32)      # padding rows may hold anything
        atoms[:, 1::2] = 3.0e30
        mask, nd = np.zeros((7, 320), np.float32), np.zeros((7, 320), np.float32)
        for p, name in enumerate(NAMES + ("5L33",)):
            a, _, pro = _chain(name)
            atoms[p, :len(a)], mask[p, :len(a)], nd[p, :len(a)] = a, 1, pro
        mask[6, 40:45] = 0                                       # row 6: 5L33 with residues 40-44 masked out
        atoms[6, 40:45] = np.nan
        res = _call(dev, atoms, mask, nd)
        for p, name in enumerate(NAMES):
            (a, m, pro), ref = _ref("chain", name)
            _check_against(f"batch.{name}", res, p, ref)
            lone = _call(dev, a[None], m[None], pro[None])       # bit for bit the lone call
            n = len(a)
            for k in ("ss", "ss3", "acc_idx"):
                assert torch.equal(res[k][p, :n], lone[k][0]), (name, k)
            assert torch.equal(res["acc_e"][p, :n].contiguous().view(torch.int64), lone["acc_e"][0].contiguous().view(torch.int64))
            for k in fm.SHAPE_SLOTS:
                assert torch.equal(res[k][p:p + 1].view(torch.int64), lone[k].view(torch.int64)), (name, k)
        _, gap = _ref("chain", "5L33", "gap")
        whole = _ref("chain", "5L33")[1]
        _check_against("batch.5L33.gap", res, 6, gap)
        assert gap["num_res"] == whole["num_res"] - 5 and (gap["ss"][40:45] == -1).all()
        # nothing reaches across the gap: no kept acceptor pair of a turn spans it, and the donor behind it is none
        assert (gap["acc_idx"][45] == -1).all() and _string(gap["ss"]) != _string(whole["ss"])


def test_batch_emu(use_emu):
    _run_batch("cpu")


@pytest.mark.gpu
def test_batch_gpu(hip_lib):
    _run_batch("cuda")


# ---- 4. the ideal alpha-helix -------------------------------------------------------------------------------------------------------
HELIX_SIZES = (5, 6, 7, 20, 63, 64, 65)


def _run_helix(dev, n):
    with parity_log.case(f"dssp_helix_{n}[{dev}]"):
        (atoms, _, _), ref = _ref("helix", n)
        res = _call(dev, atoms[None], None, None)
        _check_against(f"helix{n}", res, 0, ref)
        ss = res["ss"][0].cpu().numpy()
        if n == 5:
            assert not (ss == 1).any()                           # one turn_4 only: no two consecutive ones
        if n >= 7:
            assert (ss[1:n - 1] == 1).all() and ss[0] != 1 and ss[n - 1] != 1
            assert res["helix_percent"].item() == (n - 2) / n


@pytest.mark.parametrize("n", HELIX_SIZES)
def test_helix_emu(use_emu, n):
    _run_helix("cpu", n)


@pytest.mark.gpu
@pytest.mark.parametrize("n", HELIX_SIZES)
def test_helix_gpu(hip_lib, n):
    _run_helix("cuda", n)


# ---- 5. chains without structure, and the shortest ones -----------------------------------------------------------------------------
def _run_coil(dev):
    with parity_log.case(f"dssp_coil[{dev}]"):
        for n in (1, 2, 3, 130):
            (atoms, _, _), ref = _ref("coil", n)
            res = _call(dev, atoms[None], None, None)
            _check_against(f"coil{n}", res, 0, ref)
            assert res["strand_percent"].item() == ref["strand_percent"] <= 0.05     # nothing invented
        # an empty chain and a fully masked one: num_res 0, NaN fractions, nothing else
        (atoms, _, _), _ = _ref("coil", 3)
        for res in (_call(dev, atoms[None], np.zeros((1, 3), np.float32), None), _call(dev, atoms[None, :0], None, None)):
            assert res["num_res"].tolist() == [0.0] and res["num_hbonds"].tolist() == [0.0] and res["overflow"].tolist() == [0.0]
            assert all(np.isnan(res[k].item()) for k in ("helix_percent", "strand_percent", "coil_percent", "non_coil_percent",
                                                         "radius_of_gyration"))
            assert (res["ss"] == -1).all() and (res["ss3"] == -1).all() and (res["acc_idx"] == -1).all()
        assert fm.secondary_structure(_t(atoms[None, :0], dev))["ss"].shape == (1, 0)
        assert fm.secondary_structure(_t(atoms[None][:0], dev))["helix_percent"].shape == (0,)


def test_coil_emu(use_emu):
    _run_coil("cpu")


@pytest.mark.gpu
def test_coil_gpu(hip_lib):
    _run_coil("cuda")


# ---- 6. three acceptors below -0.5: the keep-two rule -------------------------------------------------------------------------------
def _run_three(dev):
    with parity_log.case(f"dssp_three_acceptors[{dev}]"):
        (atoms, mask, nd), ref = _ref("three", 0)
        most = max(ref["below"].values())
        print(f"  most acceptors below -0.5 on one donor: {most}")
        assert most >= 3                                         # the restatement really sees three
        res = _call(dev, atoms[None], mask[None], nd[None])
        _check_against("three", res, 0, ref)
        # bitwise equal energies (one copy at zero distance): both are kept, the lower index first
        twin, tmask, tnd = _three_acceptors(((0.0, 0.0, 0.0),))
        tref = _np_dssp(twin, tmask, tnd)
        copy = len(twin) - 1
        tied = [r for r in range(len(twin)) if tref["acc_idx"][r, 1] == copy and tref["acc_e"][r, 0] == tref["acc_e"][r, 1] < -0.5]
        assert tied and all(tref["acc_idx"][r, 0] < copy for r in tied)
        tres = _call(dev, twin[None], tmask[None], tnd[None])
        assert np.array_equal(tres["acc_idx"][0].cpu().numpy(), tref["acc_idx"])
        assert np.array_equal(tres["ss"][0].cpu().numpy(), tref["ss"])


def test_three_acceptors_emu(use_emu):
    _run_three("cpu")


@pytest.mark.gpu
def test_three_acceptors_gpu(hip_lib):
    _run_three("cuda")


# ---- 7. eval_rows(shape=True); 9. the refused arguments ----------------------------------------------------------------------------
def _run_eval_rows(dev):
    a37 = np.zeros((2, 110, 37, 3), np.float32)
    mask = np.zeros((2, 110), np.float32)
    for p, name in enumerate(("5L33", "6MRR")):
        a = _chain(name)[0]
        a37[p, :len(a), :5], mask[p, :len(a)] = a, 1
    plain = fm.eval_rows(_t(a37, dev), _t(mask, dev))
    rows = fm.eval_rows(_t(a37, dev), _t(mask, dev), shape=True)
    direct = fm.secondary_structure(_t(a37, dev), _t(mask, dev))
    for p, (r0, r1) in enumerate(zip(plain, rows)):
        assert set(r1) == set(r0) | set(fm.SHAPE_COLUMNS) and all(r0[k] == r1[k] for k in r0 if r0[k] == r0[k])
        assert all(isinstance(r1[k], float) and r1[k] == direct[k][p].item() for k in fm.SHAPE_COLUMNS)
    assert fm.SHAPE_COLUMNS == ("coil_percent", "helix_percent", "strand_percent", "non_coil_percent", "radius_of_gyration")
    # atom37 with its 32 zero atoms per residue and [.,5,3] give the same radius -- atoms at exactly zero are not in the file --
    # up to the order of the sum (the threads stride over 37 n and over 5 n atom slots)
    five = fm.secondary_structure(_t(a37[:, :, :5], dev), _t(mask, dev))
    _check("eval_rows.rg_37_against_5", five["radius_of_gyration"].cpu().numpy(), direct["radius_of_gyration"].cpu().numpy())
    assert torch.equal(five["ss"], direct["ss"])


def test_eval_rows_emu(use_emu):
    _run_eval_rows("cpu")


@pytest.mark.gpu
def test_eval_rows_gpu(hip_lib):
    _run_eval_rows("cuda")


def _run_arguments(dev, lib):
    n0 = lib.cdll.fd_launch_count()
    with pytest.raises(ValueError, match="2048"):
        fm.secondary_structure(torch.zeros((1, 2049, 5, 3), device=dev))
    for shape in ((1, 8, 4, 3), (1, 8, 5, 2), (8, 3), (1, 1, 8, 5, 3)):
        with pytest.raises(ValueError, match="expected"):
            fm.secondary_structure(torch.zeros(shape, device=dev))
    f = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=dev)
    idx, e, ss, out = f(1, 2049, 2, dt=torch.int32), f(1, 2049, 2, dt=torch.float64), f(1, 2049, dt=torch.int8), f(1, 8, dt=torch.float64)
    with pytest.raises(hip.FdError, match="2048"):
        lib.call("fd_dssp_hbonds", f(1, 2049, 5, 3), 15, f(1, 2049), None, 1, 2049, idx, e)
    with pytest.raises(hip.FdError, match="2048"):
        lib.call("fd_dssp_assign", f(1, 2049, 5, 3), 15, 5, f(1, 2049), idx, e, 1, 2049, ss, out)
    with pytest.raises(hip.FdError, match="atom_stride"):
        lib.call("fd_dssp_hbonds", f(1, 8, 4, 3), 12, f(1, 8), None, 1, 8, idx, e)
    with pytest.raises(hip.FdError, match="natoms"):
        lib.call("fd_dssp_assign", f(1, 8, 5, 3), 15, 37, f(1, 8), idx, e, 1, 8, ss, out)
    assert lib.cdll.fd_launch_count() == n0                      # refused: nothing was launched
    fm.secondary_structure(f(2, 8, 5, 3))
    assert lib.cdll.fd_launch_count() == n0 + 2                  # two launches in total


def test_arguments_emu(use_emu):
    _run_arguments("cpu", use_emu)


@pytest.mark.gpu
def test_arguments_gpu(hip_lib):
    _run_arguments("cuda", hip_lib)


# ---- 7., 8. the sampler's switch -----------------------------------------------------------------------------------------------------
def _run_sampler(dev, lib):
    from oracle import framediff_oracle as fo
    from se3_diffusion_amd import sampler, train_step as ts
    from se3_diffusion_amd.data import se3_diffuser
    from se3_diffusion_amd.model.score_network import ScoreNetwork
    from test_diffuser import conf as dconf
    T = np.load(os.path.join(ROOT, "tests", "golden", "traj.npz"))        # tests/test_sampler.py's model: 2 blocks, B = 2, N = 10
    diff = se3_diffuser.SE3Diffuser(dconf())
    blocks, B, N = int(T["blocks"]), int(T["B"]), int(T["N"])
    m = ScoreNetwork(ts.base_model_conf(blocks), diff)
    m.load_state_dict(fo.synth_params(seed=int(T["seed"]), conf=dict(fo.CONF, num_blocks=blocks)), strict=True)
    m = m.to(dev).eval()
    zr, zt = T["z_rot"], T["z_trans"]

    def run(num_t=2, **kw):
        feats = sampler.init_feats(diff, B, N, dev, noise=(T["init_randn"], T["init_rand"], T["init_normal"]))
        feats["res_mask"][1, N - 2:] = 0                                   # one padded tail
        n0 = lib.cdll.fd_launch_count()
        out = sampler.sample(m, diff, feats, num_t=num_t, min_t=float(T["min_t"]), noise_scale=float(T["noise_scale"]),
                             noise_fn=lambda i, shp: (zr[i], zt[i]), **kw)
        return out, lib.cdll.fd_launch_count() - n0, feats

    run()                                                                  # (lazily built tables are launched once, here)
    off, n_off, _ = run()
    on, n_on, _ = run(metrics=True)
    shp, n_shp, feats = run(metrics="shape")
    # metrics=True: the key set and the launches of today
    assert set(on) == set(off) | {"metrics"} and tuple(on["metrics"]) == fm.BACKBONE_SLOTS and n_on == n_off + 1
    assert n_shp == n_on + 2 and set(shp) == set(on)
    assert set(shp["metrics"]) == set(fm.BACKBONE_SLOTS) | set(fm.SHAPE_SLOTS) | {"ss"}
    assert torch.equal(shp["atom37"], off["atom37"]) and torch.equal(shp["rigids"], off["rigids"])
    direct = fm.secondary_structure(shp["atom37"], feats["res_mask"])
    assert torch.equal(shp["metrics"]["ss"], direct["ss"]) and shp["metrics"]["ss"].shape == (B, N)
    for k in fm.SHAPE_SLOTS:
        assert torch.equal(shp["metrics"][k].view(torch.int64), direct[k].view(torch.int64)), k
    for k in fm.BACKBONE_SLOTS:
        assert torch.equal(shp["metrics"][k].view(torch.int64), on["metrics"][k].view(torch.int64)), k
    assert shp["metrics"]["num_res"].tolist() == [float(N), float(N - 2)]
    assert bool(torch.isfinite(shp["metrics"]["radius_of_gyration"]).all())
    with pytest.raises(ValueError, match="shape"):
        run(metrics="shapes")


def test_sampler_shape_emu(use_emu):
    _run_sampler("cpu", use_emu)


@pytest.mark.gpu
def test_sampler_shape_gpu(hip_lib):
    _run_sampler("cuda", hip_lib)
