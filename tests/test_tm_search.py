"""The TM-score of a fixed correspondence by superposition search (fd_tm_search, se3_diffusion_amd.metrics.tm_score / pairwise_tm /
eval_rows(tm=True)).

The reference of every case is a float64 numpy restatement, written here, of the search that include/fd_hip.h specifies, with
a textbook Kabsch superposition (SVD, determinant fix) where the kernel uses Horn's quaternion.  Neither tmtools nor the
TM-score program is available to this suite: agreement with the values they print is NOT checked here.

Inputs are generated from fixed seeds: CA traces are random walks of 3.8 A steps rounded to float32.  Bounds, the same on the
interpreter and on the device (the project's own, tests/test_metrics.py: both sides compute in float64 from identical float32
inputs): scalars within 1e-9 * max(1, |ref|), R and t within 1e-8 absolute, integers (num_aligned, best_seed, num_seeds, passes)
exactly.  The exact comparisons are sound because the restatement also returns its margin -- the smallest |sqrt(d2_k) - dcut| it
met over all calls of score -- and every case asserts margin >= 1e-7 A: no position sits close enough to a cutoff for rounding
to change a selection.  Each case reports what it achieved through parity_log (expected: <= 1e-11)."""
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
MARGIN = 1e-7
NAN = float("nan")
KINDS = ("noise", "hinge", "unrelated")
SIZES = (4, 5, 21, 22, 40, 63, 64, 65, 130)


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


def _pair(kind, L, seed=0):
    """float32 a, b [L,3] of one kind (the seed is fixed per case; see _np_case's margin assertion)"""
    rng = np.random.default_rng([seed, L, KINDS.index(kind)])
    a = _walk(rng, L).astype(np.float32)
    a64 = a.astype(np.float64)
    R, t = _rotation(rng), rng.normal(size=3) * 10
    if kind == "noise":
        b = a64 @ R.T + t + rng.normal(size=(L, 3)) * 1.5
    elif kind == "hinge":
        # the first floor(3L/5) residues under one rigid motion, the rest under another (about their own centroid) and 20 A away
        m = 3 * L // 5
        b = a64 @ R.T + t
        tail = a64[m:]
        c = tail.mean(0)
        u = rng.normal(size=3)
        b[m:] = (tail - c) @ _rotation(rng).T + (R @ c + t) + 20.0 * u / np.linalg.norm(u)
    else:
        b = _walk(rng, L)
    return a, b.astype(np.float32)


# ---- the float64 restatement (computed once per case, shared by both runs, never modified) ------------------------------------
def _np_kabsch(a, b):
    """optimal proper rotation of a onto b (textbook Kabsch: SVD of the covariance, determinant fix)"""
    ca, cb = a.mean(0), b.mean(0)
    H = (a - ca).T @ (b - cb)
    U, S, Vt = np.linalg.svd(H)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))])
    R = Vt.T @ D @ U.T
    return R, cb - R @ ca


def _np_lens(L):
    lens, l = [], L
    for i in range(6):
        if l <= 4:
            break
        lens.append(l)
        l = L >> (i + 1)
    lens.append(4)
    return lens


def _np_search(a, b, seed_step=1, max_iter=20):
    """the search of include/fd_hip.h on the counting positions a, b [L,3] (float32 values): dict with the TM_SLOTS, R, t, margin"""
    a, b = a.astype(np.float64), b.astype(np.float64)
    L = len(a)
    d0 = 1.24 * np.cbrt(L - 15.0) - 1.8 if L > 21 else 0.5
    res = dict(num_aligned=float(L), tm_score=NAN, tm_kabsch=NAN, best_seed=-1.0, num_seeds=0.0, d0=float(d0), passes=0.0,
               R=None, t=None, margin=np.inf)
    if L == 0:
        return res
    formula = lambda R, t: ((a @ R.T + t - b) ** 2).sum(-1)
    if L < 4:
        R, t = _np_kabsch(a, b)
        s = float(np.mean(1.0 / (1.0 + formula(R, t) / d0 ** 2)))
        res.update(tm_score=s, tm_kabsch=s, R=R, t=t)
        return res
    d0s = min(max(d0, 4.5), 8.0)

    def score(R, t, dcut):
        d2 = formula(R, t)
        d = np.sqrt(d2)
        while True:
            res["margin"] = min(res["margin"], float(np.abs(d - dcut).min()))
            sel = d2 < dcut * dcut
            if sel.sum() >= 3:
                break
            dcut += 0.5
        res["passes"] += 1.0
        return float(np.mean(1.0 / (1.0 + d2 / d0 ** 2))), sel

    best, seed = -1.0, 0
    for ln in _np_lens(L):
        for start in range(0, L - ln + 1, seed_step):
            cands = []
            sel = np.zeros(L, bool)
            sel[start:start + ln] = True
            R, t = _np_kabsch(a[sel], b[sel])
            s, sel = score(R, t, d0s - 1.0)
            cands.append((s, R, t))
            if seed == 0:
                res["tm_kabsch"] = s
            for _ in range(max_iter):
                R, t = _np_kabsch(a[sel], b[sel])
                s, new = score(R, t, d0s + 1.0)
                cands.append((s, R, t))
                same = bool((new == sel).all())
                sel = new
                if same:
                    break
            for s, R, t in cands:
                if s > best:
                    best = s
                    res.update(tm_score=s, best_seed=float(seed), R=R, t=t)
            seed += 1
    res["num_seeds"] = float(seed)
    return res


@functools.lru_cache(maxsize=None)
def _np_case(kind, L, seed_step=1):
    a, b = _pair(kind, L)
    ref = _np_search(a, b, seed_step)
    assert ref["margin"] >= MARGIN, (kind, L, ref["margin"])     # (what makes the exact comparisons below sound)
    return a, b, ref


# ---- helpers ------------------------------------------------------------------------------------------------------------------------
def _t(x, dev):
    return torch.as_tensor(np.ascontiguousarray(x)).to(dev)


def _bits(x):
    return x.contiguous().view(torch.int64)


def _same_bits(a, b):
    return a.keys() == b.keys() and all(torch.equal(_bits(a[k]), _bits(b[k])) for k in a)


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


def _check_against(tag, res, p, ref):
    """entry p of a batched tm_score result against one restatement"""
    print(f"  {tag}: tm_score {ref['tm_score']:.6f} tm_kabsch {ref['tm_kabsch']:.6f} seed {ref['best_seed']:.0f} of "
          f"{ref['num_seeds']:.0f}, passes {ref['passes']:.0f}, margin {ref['margin']:.2e}")
    for k in ("num_aligned", "best_seed", "num_seeds", "passes"):
        assert res[k][p].item() == ref[k], (tag, k, res[k][p].item(), ref[k])
    for k in ("tm_score", "tm_kabsch", "d0"):
        _check(f"{tag}.{k}", res[k][p].item(), ref[k])
    if "R" in res and ref["R"] is not None:
        eR = float(np.abs(res["R"][p].cpu().numpy() - ref["R"]).max())
        et = float(np.abs(res["t"][p].cpu().numpy() - ref["t"]).max())
        parity_log.out(f"{tag}.R_abs", eR)
        parity_log.out(f"{tag}.t_abs", et)
        print(f"  {tag}: R {eR:.3e} t {et:.3e} (bound 1e-08)")
        assert eR <= 1e-8 and et <= 1e-8, (tag, eR, et)


# ---- 1. restatement parity at seed_step = 1 ---------------------------------------------------------------------------------------
def _run_parity(dev, L):
    with parity_log.case(f"tm_search_parity_L{L}[{dev}]"):
        cases = [_np_case(kind, L) for kind in KINDS]
        a = np.stack([c[0] for c in cases])
        b = np.stack([c[1] for c in cases])
        res = fm.tm_score(_t(a, dev), _t(b, dev), return_transform=True)
        assert list(res) == list(fm.TM_SLOTS) + ["R", "t"]
        assert all(res[k].shape == (3,) and res[k].dtype == torch.float64 for k in fm.TM_SLOTS)
        assert res["R"].shape == (3, 3, 3) and res["t"].shape == (3, 3)
        for p, kind in enumerate(KINDS):
            _check_against(f"{kind}{L}", res, p, cases[p][2])
        assert np.allclose(np.linalg.det(res["R"].cpu().numpy()), 1.0, atol=1e-12)
        assert (res["tm_score"] >= res["tm_kabsch"]).all()       # seed 0's first score is a candidate


@pytest.mark.parametrize("L", SIZES)
def test_parity_emu(use_emu, L):
    _run_parity("cpu", L)


@pytest.mark.gpu
@pytest.mark.parametrize("L", SIZES)
def test_parity_gpu(hip_lib, L):
    _run_parity("cuda", L)


# ---- 2. what the search is for -----------------------------------------------------------------------------------------------------
def _run_hinge(dev):
    with parity_log.case(f"tm_search_hinge[{dev}]"):
        for L in (5, 21, 40, 130):
            a, b, _ = _np_case("hinge", L)
            tm = fm.tm_score(_t(a, dev), _t(b, dev))["tm_score"].item()
            kab = fm.aligned_rmsd(_t(a, dev), _t(b, dev))["tm_kabsch"].item()
            frac = (3 * L // 5) / L
            print(f"  hinge L={L}: tm_score {tm:.9f} (larger part {frac:.6f}), tm_kabsch {kab:.6f}, gain {tm - kab:.4f}")
            # the larger part superposes exactly, every other term is >= 0, and the fp32 rounding of the moved copy costs ~1e-10
            assert tm >= frac - 1e-6, (L, tm, frac)
            assert tm - kab >= 0.3, (L, tm, kab)


def test_hinge_emu(use_emu):
    _run_hinge("cpu")


@pytest.mark.gpu
def test_hinge_gpu(hip_lib):
    _run_hinge("cuda")


# ---- 3. rigid copies and the refused arguments ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _rigid(n):
    rng = np.random.default_rng([7, n])
    a = _walk(rng, n).astype(np.float32)
    return a, (a.astype(np.float64) @ _rotation(rng).T + rng.normal(size=3) * 10).astype(np.float32)


def _run_rigid(dev, shapes):
    with parity_log.case(f"tm_search_rigid[{dev}]"):
        for n, step in shapes:
            a, b = _rigid(n)
            res = fm.tm_score(_t(a, dev), _t(b, dev), seed_step=step)
            # b is the rounded image of a: |b_k - (R a_k + t)| <= 2^-24 * 200 A ~ 1e-5 A, so 1 - tm <= (1e-5 / d0)^2 < 1e-9 for
            # d0 >= 0.5
            gap = 1.0 - res["tm_score"].item()
            parity_log.out(f"rigid{n}.one_minus_tm", abs(gap))
            print(f"  rigid N={n} seed_step={step}: 1 - tm_score = {gap:.3e} (bound 1e-09), passes {res['passes'].item():.0f}")
            assert abs(gap) <= 1e-9 and res["num_aligned"].item() == n


RIGID = ((65, 1), (513, 16), (2048, 256))


def test_rigid_emu(use_emu):
    _run_rigid("cpu", RIGID)


@pytest.mark.gpu
def test_rigid_gpu(hip_lib):
    _run_rigid("cuda", RIGID)


def _run_arguments(dev, lib):
    f32 = lambda *s: torch.zeros(s, device=dev)
    f64 = lambda *s: torch.full(s, NAN, dtype=torch.float64, device=dev)
    n0 = lib.cdll.fd_launch_count()
    with pytest.raises(hip.FdError, match="2048"):
        fm.tm_score(f32(1, 2049, 3), f32(1, 2049, 3))
    with pytest.raises(hip.FdError, match="seed_step"):
        fm.tm_score(f32(1, 8, 3), f32(1, 8, 3), seed_step=0)
    with pytest.raises(hip.FdError, match="max_iter"):
        fm.tm_score(f32(1, 8, 3), f32(1, 8, 3), max_iter=-1)
    with pytest.raises(hip.FdError, match="parts"):
        fm.tm_score(f32(1, 8, 3), f32(1, 8, 3), parts=0)
    out, tr = f64(2, 8), f64(2, 12)
    args = (f32(2, 8, 3), 3, f32(2, 8, 3), 3, None, None, None)
    with pytest.raises(hip.FdError, match="workspace"):
        lib.call("fd_tm_search", *args, 2, 8, 1, 20, 1, None, out, tr)
    with pytest.raises(hip.FdError, match="together"):
        lib.call("fd_tm_search", *args[:4], torch.zeros(2, dtype=torch.int32, device=dev), None, None, 2, 8, 1, 20, 1, f64(128), out, tr)
    lib.call("fd_tm_search", *args, 0, 8, 1, 20, 1, f64(128), out, tr)         # P == 0
    lib.call("fd_tm_search", *args, 2, 0, 1, 20, 1, f64(128), out, tr)         # N == 0
    assert fm.tm_score(f32(0, 8, 3), f32(0, 8, 3))["tm_score"].shape == (0,)
    assert lib.cdll.fd_launch_count() == n0                                    # refused or empty: nothing was launched
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(tr).all())        # ... and nothing written


def test_arguments_emu(use_emu):
    _run_arguments("cpu", use_emu)


@pytest.mark.gpu
def test_arguments_gpu(hip_lib):
    _run_arguments("cuda", hip_lib)


# ---- 4. masks -----------------------------------------------------------------------------------------------------------------------
def _run_masks(dev):
    with parity_log.case(f"tm_search_masks[{dev}]"):
        a, b, ref = _np_case("noise", 40)
        rng = np.random.default_rng(11)
        keep = np.sort(rng.choice(64, size=40, replace=False))
        mask = np.zeros(64, np.float32)
        mask[keep] = rng.choice([1.0, -2.5, 7.0], size=40)       # any non-zero value counts
        A, B = rng.normal(size=(64, 3)).astype(np.float32) * 9, rng.normal(size=(64, 3)).astype(np.float32) * 9
        A[keep], B[keep] = a, b
        packed = fm.tm_score(_t(a, dev), _t(b, dev), return_transform=True)
        masked = fm.tm_score(_t(A, dev), _t(B, dev), _t(mask, dev), return_transform=True)
        assert packed["tm_score"].dim() == 0 and packed["R"].shape == (3, 3) and packed["t"].shape == (3,)
        assert _same_bits(packed, masked)
        _check_against("masked40", {k: v[None] for k, v in masked.items()}, 0, ref)
        # NaN (and infinite) bit patterns at the masked-out positions change nothing
        A2, B2 = A.copy(), B.copy()
        A2[mask == 0], B2[mask == 0] = np.nan, -np.inf
        assert _same_bits(masked, fm.tm_score(_t(A2, dev), _t(B2, dev), _t(mask, dev), return_transform=True))
        # a position counts only if BOTH sets' masks are non-zero: two sets, each missing some of the 40, through pairwise_tm
        m2 = np.stack([mask, mask])
        m2[0, keep[:3]], m2[1, keep[-2:]] = 0, 0
        both = fm.pairwise_tm(_t(np.stack([A2, B2]), dev), _t(m2, dev))
        inner = fm.tm_score(_t(a[3:-2], dev), _t(b[3:-2], dev))
        assert torch.equal(_bits(both[0, 1][None]), _bits(inner["tm_score"][None])) and inner["num_aligned"].item() == 35.0


def test_masks_emu(use_emu):
    _run_masks("cpu")


@pytest.mark.gpu
def test_masks_gpu(hip_lib):
    _run_masks("cuda")


# ---- 5. short sets ------------------------------------------------------------------------------------------------------------------
def _run_short(dev):
    with parity_log.case(f"tm_search_short[{dev}]"):
        a, b, _ = _np_case("noise", 40)
        mask = np.zeros((4, 40), np.float32)
        for L in (1, 2, 3):
            mask[L, [5, 17, 30][:L]] = 1
        A, B = np.stack([a] * 4), np.stack([b] * 4)
        res = fm.tm_score(_t(A, dev), _t(B, dev), _t(mask, dev), return_transform=True)
        kab = fm.aligned_rmsd(_t(A, dev), _t(B, dev), _t(mask, dev))
        assert res["num_aligned"].tolist() == [0.0, 1.0, 2.0, 3.0]
        assert res["best_seed"].tolist() == [-1.0] * 4 and res["num_seeds"].tolist() == [0.0] * 4
        assert res["passes"].tolist() == [0.0] * 4               # no seed ran: no call of score is counted
        assert res["d0"].tolist() == [0.5] * 4
        assert np.isnan(res["tm_score"][0].item()) and np.isnan(res["tm_kabsch"][0].item())
        for L in (1, 2, 3):
            ref = _np_search(a[mask[L] != 0], b[mask[L] != 0])
            _check(f"short{L}.tm_score", res["tm_score"][L].item(), kab["tm_kabsch"][L].item())
            _check(f"short{L}.tm_kabsch", res["tm_kabsch"][L].item(), kab["tm_kabsch"][L].item())
            _check(f"short{L}.np", res["tm_score"][L].item(), ref["tm_score"])


def test_short_emu(use_emu):
    _run_short("cpu")


@pytest.mark.gpu
def test_short_gpu(hip_lib):
    _run_short("cuda")


def _run_nonfinite(dev):
    """a NaN among the COUNTING positions (a diverged sample): every score is NaN, so there is no candidate -- NaN and
    best_seed -1 -- and every seed still makes between 2 and 1 + max_iter calls of score"""
    a, b, _ = _np_case("noise", 40)
    a = a.copy()
    a[7, 1] = np.nan
    res = fm.tm_score(_t(a, dev), _t(b, dev))
    assert np.isnan(res["tm_score"].item()) and np.isnan(res["tm_kabsch"].item()) and res["best_seed"].item() == -1.0
    seeds = fm.tm_num_seeds(40)
    assert res["num_seeds"].item() == seeds and 2 * seeds <= res["passes"].item() <= 21 * seeds


def test_nonfinite_emu(use_emu):
    _run_nonfinite("cpu")


@pytest.mark.gpu
def test_nonfinite_gpu(hip_lib):
    _run_nonfinite("cuda")


# ---- 6. determinism -----------------------------------------------------------------------------------------------------------------
def _run_determinism(dev):
    kinds = ("noise", "hinge")
    a = np.stack([_np_case(kind, 40)[0] for kind in kinds])
    b = np.stack([_np_case(kind, 40)[1] for kind in kinds])
    seeds = fm.tm_num_seeds(40)
    assert seeds == int(_np_case("noise", 40)[2]["num_seeds"]) == 126
    most = -(-seeds // 4)
    runs = [fm.tm_score(_t(a, dev), _t(b, dev), return_transform=True, parts=parts) for parts in (1, 3, most, most, most + 5)]
    assert all(_same_bits(runs[0], r) for r in runs[1:])         # (most + 5: blocks without a seed leave empty partials)
    assert fm.tm_parts(3, 40) == most and fm.tm_parts(4096, 40) == 1 and fm.tm_parts(2, 3) == 1 and fm.tm_parts(1, 2048) == 768


def test_determinism_emu(use_emu):
    _run_determinism("cpu")


@pytest.mark.gpu
def test_determinism_gpu(hip_lib):
    _run_determinism("cuda")


# ---- 7. seed_step -------------------------------------------------------------------------------------------------------------------
def _run_seed_step(dev):
    with parity_log.case(f"tm_search_seed_step[{dev}]"):
        for kind in KINDS:
            a, b, ref4 = _np_case(kind, 65, 4)
            fine = fm.tm_score(_t(a, dev), _t(b, dev), seed_step=1)
            coarse = fm.tm_score(_t(a, dev), _t(b, dev), seed_step=4, return_transform=True)
            _check_against(f"{kind}65.step4", {k: v[None] for k, v in coarse.items()}, 0, ref4)
            # the coarser seeds are a subset and each seed's arithmetic is identical: bitwise, no tolerance
            assert fine["tm_score"].item() >= coarse["tm_score"].item()
            assert fine["num_seeds"].item() > coarse["num_seeds"].item() == fm.tm_num_seeds(65, 4)


def test_seed_step_emu(use_emu):
    _run_seed_step("cpu")


@pytest.mark.gpu
def test_seed_step_gpu(hip_lib):
    _run_seed_step("cuda")


# ---- 8. layouts and the matrix ------------------------------------------------------------------------------------------------------
def _run_layouts(dev, lib):
    rng = np.random.default_rng(13)
    sets = np.stack([_np_case(kind, 40)[k] for kind in KINDS for k in (0, 1)][:5])          # M = 5 sets of N = 40
    pos = _t(sets, dev)
    M = 5
    # a strided CA view of atom37 is read in place and equals the packed copy
    a37 = _t(rng.normal(size=(M, 40, 37, 3)).astype(np.float32), dev)
    a37[:, :, 1] = pos
    va = a37[:, :, 1]
    assert not va.is_contiguous() and fm._points(va)[0].data_ptr() == va.data_ptr() and fm._points(va)[1] == 111
    other = pos[2:4]
    assert _same_bits(fm.tm_score(pos[:2], other, return_transform=True), fm.tm_score(va[:2], other, return_transform=True))
    assert _same_bits(fm.tm_score(other, pos[:2]), fm.tm_score(other, va[:2]))
    # the matrix: one search (two launches: search, reduce) over the 10 upper pairs through the index lists
    n0 = lib.cdll.fd_launch_count()
    tm = fm.pairwise_tm(va)
    assert lib.cdll.fd_launch_count() == n0 + 2
    assert tm.shape == (M, M) and tm.dtype == torch.float64
    assert torch.equal(tm, tm.T) and tm.diagonal().tolist() == [1.0] * M
    iu = torch.triu_indices(M, M, 1)
    pairs = fm.tm_score(pos[iu[0]], pos[iu[1]])["tm_score"]       # each entry equals the pair call, bit for bit
    assert torch.equal(_bits(pairs), _bits(tm[iu[0], iu[1]]))
    assert torch.equal(_bits(fm.tm_score(pos[1], pos[3])["tm_score"][None]), _bits(tm[1, 3][None]))
    assert 0.0 < tm.min().item() < 0.5 and tm[2, 3].item() >= 24 / 40 - 1e-6       # (unrelated walks; sets 2, 3: the hinge pair)
    n0 = lib.cdll.fd_launch_count()
    assert fm.pairwise_tm(pos[:1]).tolist() == [[1.0]]             # a lone set: no pair, nothing to launch
    assert fm.tm_score(pos[:0], pos[:0])["tm_score"].shape == (0,)
    assert lib.cdll.fd_launch_count() == n0


def test_layouts_emu(use_emu):
    _run_layouts("cpu", use_emu)


@pytest.mark.gpu
def test_layouts_gpu(hip_lib):
    _run_layouts("cuda", hip_lib)


# ---- 9. eval_rows -------------------------------------------------------------------------------------------------------------------
def _run_eval_rows(dev):
    with parity_log.case(f"tm_search_eval_rows[{dev}]"):
        rng = np.random.default_rng(17)
        s37 = rng.normal(size=(3, 40, 37, 3)).astype(np.float32)
        g37 = rng.normal(size=(3, 40, 37, 3)).astype(np.float32)
        for p, kind in enumerate(KINDS):
            s37[p, :, 1], g37[p, :, 1] = _np_case(kind, 40)[:2]
        res_mask = np.ones((3, 40), np.float32)
        res_mask[1, 36:] = 0                                     # a padded tail
        fixed = np.zeros((3, 40), np.float32)
        fixed[2, :6] = 1                                         # a fixed motif: not scored
        args = (_t(s37, dev), _t(res_mask, dev), _t(fixed, dev), _t(g37, dev))
        plain, with_tm = fm.eval_rows(*args), fm.eval_rows(*args, tm=True)
        today = set(fm.BACKBONE_SLOTS) | {"fixed_residues", "diffused_percentage", "aligned_rmsd_to_gt"}
        for r0, r1 in zip(plain, with_tm):
            assert set(r0) == today and set(r1) == today | {"tm_score_to_gt"}
            assert all(r0[k] == r1[k] or (np.isnan(r0[k]) and np.isnan(r1[k])) for k in r0)      # the other columns: untouched
        diffused = (1 - fixed) * res_mask
        direct = fm.tm_score(_t(s37, dev)[:, :, 1], _t(g37, dev)[:, :, 1], _t(diffused, dev))
        assert [r["tm_score_to_gt"] for r in with_tm] == direct["tm_score"].tolist()
        assert direct["num_aligned"].tolist() == [40.0, 36.0, 34.0]
        _check("eval_rows.tm_score_to_gt", with_tm[0]["tm_score_to_gt"], _np_case("noise", 40)[2]["tm_score"])
        no_gt = fm.eval_rows(*args[:3], tm=True)                 # without a ground truth there is nothing to score against
        assert all("tm_score_to_gt" not in r and "aligned_rmsd_to_gt" not in r for r in no_gt)


def test_eval_rows_emu(use_emu):
    _run_eval_rows("cpu")


@pytest.mark.gpu
def test_eval_rows_gpu(hip_lib):
    _run_eval_rows("cuda")
