"""Bond, angle and clash violation losses on the device (fd_violations, se3_diffusion_amd.metrics.violations /
eval_rows(violations=True), sampler.sample(metrics="violations" | "all")).

Two references.  (1) _np_violations: a float64 numpy restatement of include/fd_hip.h, written here; it shares nothing with the
kernel.  (2) tests/golden/violations.npz (tools/make_golden_violations.py): the UNMODIFIED reference -- make_atom14_masks,
make_atom14_positions, find_structural_violations(violation_tolerance_factor=12, clash_overlap_tolerance=1.5),
compute_violation_metrics -- run on the compacted chain of every case, once in float32 as the reference runs it and once with
its inputs widened to float64.  The reference cannot run on the empty chain (it raises): that case has the restatement only.

Exact: the masks, num_res, num_bonds, num_atom_pairs, num_clashing_pairs, num_residue_violations.  That is sound because every case
re-asserts its decision margin: each connection tolerance, the CA-CA excess and every clash bound lies at least 1e-4 from what it is
compared with (float64).

Against the restatement and the reference's float64 run: relative error |got - ref| / |ref| per element (an element whose
reference is zero must be zero).  Measured worst over all cases: 8.3e-16 on the interpreter and 8.3e-16 on the device (both on
walk130's connections_per_residue_loss_sum against the reference's float64 run; against the restatement 3.8e-16 and 4.8e-16).
Both sides are IEEE float64 on the same float32 inputs and the library is built without contraction, so what differs is the
order of the sums.  REL is ten times that figure.

Against the reference's float32 run -- the column it actually writes: per quantity, 4 x the largest float32-against-float64
difference of the reference itself over the cases of the fixture (the 4 is for the summation order of float32); computed from the
fixture by _gaps, never from the code under test.  The tool printed (scalars relative, arrays absolute):
    bonds_c_n_loss_mean                 9.4e-07      violations_extreme_ca_ca_distance   7.0e-08
    angles_ca_c_n_loss_mean             2.6e-07      violations_between_residue_bond     2.4e-08
    angles_c_n_ca_loss_mean             1.2e-06      violations_between_residue_clash    6.5e-08
    clashes_mean_loss                   1.0e-07      violations_per_residue              3.8e-08
    connections_per_residue_loss_sum    2.7e-07      clashes_per_atom_loss_sum           2.6e-06
violations_per_residue and num_residue_violations leave the within-residue term out (include/fd_hip.h): they are compared with
the maximum of the reference's connection and clash masks, and with the reference's own column on the two deposited chains, where
its within-residue term is zero.

Mutations of the kernel that this file catches on the interpreter (each was run on a scratch copy): no C-N exclusion; 12 * 0.0311
as the CA-C-N tolerance; <= in the res_index ordering (the kernel drops equal numbers before it compares, so the mutation is that
test reduced to j == i: repeat37 catches it; <= alone leaves the program unchanged); one triangle in the per-atom sums; no eps
inside the square root of the bond term."""
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

REL = 8.4e-15
MARGIN = 1e-4
G = np.load(os.path.join(ROOT, "tests", "golden", "violations.npz"))
NAMES = tuple(str(x) for x in G["names"])
REF_SCALARS = tuple(str(x) for x in G["scalars"])
MEANS = ("bonds_c_n_loss_mean", "angles_ca_c_n_loss_mean", "angles_c_n_ca_loss_mean", "clashes_mean_loss",
         "violations_extreme_ca_ca_distance", "violations_between_residue_bond", "violations_between_residue_clash")
COUNTS = ("num_res", "num_bonds", "num_atom_pairs", "num_clashing_pairs", "num_residue_violations")
LOSS_ARRAYS = ("connections_per_residue_loss_sum", "clashes_per_atom_loss_sum")
MASK_ARRAYS = ("connections_per_residue_violation_mask", "clashes_per_atom_clash_mask")
RADIUS = np.array([1.55, 1.7, 1.7, 1.7, 1.52])   # N, CA, C, CB, O


# ---- the float64 restatement of include/fd_hip.h ---------------------------------------------------------------------------------------
def _np_violations(atoms, mask=None, res_index=None):
    """atoms float32 [N,A,3] (N, CA, C, CB, O first), mask [N], res_index [N] -> dict: the VIOLATION_SLOTS as floats, the four
    per-residue / per-atom arrays by original index, margin"""
    N = len(atoms)
    if mask is None:
        mask = (atoms != 0).reshape(N, -1).any(-1)
    keep = np.flatnonzero(np.asarray(mask) != 0)
    n = len(keep)
    x = atoms[keep][:, :5].astype(np.float64)
    idx = (np.arange(N) if res_index is None else np.asarray(res_index))[keep].astype(np.int64)
    margin = np.inf
    pair_loss, pair_viol, bonded, far = np.zeros(max(n - 1, 0)), np.zeros(max(n - 1, 0), bool), np.zeros(max(n - 1, 0), bool), 0
    means = [0.0, 0.0, 0.0]
    if n > 1:
        ca, c, nn, can = x[:-1, 1], x[:-1, 2], x[1:, 0], x[1:, 1]
        root = lambda v: np.sqrt(1e-6 + (v ** 2).sum(-1))
        l_cn, l_cac, l_nca = root(c - nn), root(ca - c), root(nn - can)
        cos1 = (((ca - c) / l_cac[:, None]) * ((nn - c) / l_cn[:, None])).sum(-1)
        cos2 = ((-(nn - c) / l_cn[:, None]) * ((can - nn) / l_nca[:, None])).sum(-1)
        err = [np.sqrt(1e-6 + (l_cn - 1.329) ** 2), np.sqrt(1e-6 + (cos1 + 0.4473) ** 2), np.sqrt(1e-6 + (cos2 + 0.5203) ** 2)]
        tol = [12 * 0.014, 12 * 0.014, 12 * 0.0353]             # (the second: the reference's quirk, loss.py:807)
        bonded = idx[1:] - idx[:-1] == 1
        excess = root(ca - can) - 3.80209737096
        for e, t in zip(err, tol):
            margin = min(margin, np.abs(e - t).min())
            pair_loss = pair_loss + np.maximum(e - t, 0.0)
            pair_viol = pair_viol | (bonded & (e > t))
        margin = min(margin, np.abs(excess - 1.5).min())
        means = [float((bonded * np.maximum(e - t, 0.0)).sum() / (bonded.sum() + 1e-6)) for e, t in zip(err, tol)]
        far = int((bonded & (excess > 1.5)).sum())
    pad = lambda v: np.concatenate([v, v[:0] if n == 0 else np.zeros(1, v.dtype)])
    shift = lambda v: np.concatenate([v[:0] if n == 0 else np.zeros(1, v.dtype), v])
    res_loss = 0.5 * (pad(pair_loss) + shift(pair_loss)) if n else np.zeros(0)
    res_viol = pad(pair_viol) | shift(pair_viol) if n else np.zeros(0, bool)
    # clashes: [i, j, a, c] = atom a of i against atom c of j
    atom_loss, atom_clash = np.zeros((n, 5)), np.zeros((n, 5), bool)
    pairs = clashing = 0
    clash_sum = 0.0
    if n > 1:
        dist = np.sqrt(1e-10 + ((x[:, None, :, None] - x[None, :, None, :]) ** 2).sum(-1))
        bound = RADIUS[None, None, :, None] + RADIUS[None, None, None, :] - 1.5
        counted = np.broadcast_to((idx[:, None] < idx[None, :])[:, :, None, None], dist.shape).copy()
        counted[:, :, 2, 0] &= ~(idx[:, None] + 1 == idx[None, :])          # C of i, N of j, consecutive numbers: the peptide bond
        margin = min(margin, np.abs(dist - bound)[counted].min()) if counted.any() else margin
        loss = counted * np.maximum(bound - dist, 0.0)
        clash = counted & (dist < bound)
        pairs, clashing, clash_sum = int(counted.sum()), int(clash.sum()), float(loss.sum())
        atom_loss = loss.sum((1, 3)) + loss.sum((0, 2))
        atom_clash = clash.any((1, 3)) | clash.any((0, 2))
    res_any = res_viol | atom_clash.any(-1)
    nb = int(bonded.sum())
    res = dict(num_res=float(n), bonds_c_n_loss_mean=means[0], angles_ca_c_n_loss_mean=means[1], angles_c_n_ca_loss_mean=means[2],
               clashes_mean_loss=clash_sum / (1e-6 + pairs), violations_extreme_ca_ca_distance=far / (1e-4 + nb),
               violations_between_residue_bond=float(res_viol.sum()) / (1e-4 + n),
               violations_between_residue_clash=float(atom_clash.any(-1).sum()) / (1e-4 + n),
               violations_per_residue=float(res_any.sum()) / (1e-4 + n), num_residue_violations=float(res_any.sum()),
               num_bonds=float(nb), num_atom_pairs=float(pairs), num_clashing_pairs=float(clashing))

    def scatter(v, dtype):
        full = np.zeros((N,) + v.shape[1:], dtype)
        full[keep] = v
        return full
    res.update(connections_per_residue_loss_sum=scatter(res_loss, np.float64), connections_per_residue_violation_mask=scatter(res_viol, bool),
               clashes_per_atom_loss_sum=scatter(atom_loss, np.float64), clashes_per_atom_clash_mask=scatter(atom_clash, bool),
               margin=float(margin), keep=keep)
    return res


# ---- the fixture ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(name):
    """inputs (atoms [n,5,3], mask, res_index), the restatement, and the reference's float32 and float64 results (None for the
    empty chain) with the per-residue arrays scattered to original indices; computed once, shared by both tiers, never modified"""
    k = NAMES.index(name)
    rows = slice(int(G["row_start"][k]), int(G["row_start"][k + 1]))
    inp = (G["atoms"][rows], G["mask"][rows], G["res_index"][rows])
    ref = _np_violations(*inp)
    assert ref["margin"] >= MARGIN, (name, ref["margin"])        # (what makes the exact comparisons sound)
    if not G["has_ref"][k]:
        return inp, ref, None, None
    pres = slice(int(G["res_start"][k]), int(G["res_start"][k + 1]))
    both = []
    for tag in ("f32", "f64"):
        r = {s: float(G[f"{tag}_scalars"][k, i]) for i, s in enumerate(REF_SCALARS)}
        for a in LOSS_ARRAYS + MASK_ARRAYS + ("total_per_residue_violations_mask",):
            v = G[f"{tag}_{a}"][pres]
            full = np.zeros((len(inp[0]),) + v.shape[1:], np.float64)
            full[ref["keep"]] = v
            r[a] = full
        both.append(r)
    return inp, ref, both[0], both[1]


@functools.lru_cache(maxsize=None)
def _gaps():
    """per quantity the largest float32-against-float64 difference of the reference over the fixture: scalars relative, arrays
    absolute"""
    gap = {}
    for name in NAMES:
        _, _, r32, r64 = _case(name)
        if r32 is None:
            continue
        for k in REF_SCALARS:
            d = abs(r32[k] - r64[k]) / abs(r64[k]) if r64[k] != 0 else abs(r32[k])
            gap[k] = max(gap.get(k, 0.0), d)
        for k in LOSS_ARRAYS:
            gap[k] = max(gap.get(k, 0.0), float(np.abs(r32[k] - r64[k]).max()))
    return gap


# ---- helpers ------------------------------------------------------------------------------------------------------------------------
def _t(x, dev):
    return None if x is None else torch.as_tensor(np.ascontiguousarray(x)).to(dev)


def _rel(got, ref):
    """worst |got - ref| / |ref|; where the reference is zero the value must be zero"""
    got, ref = np.asarray(got, np.float64).reshape(-1), np.asarray(ref, np.float64).reshape(-1)
    zero = ref == 0
    assert (got[zero] == 0).all(), (got[zero], "expected exact zeros")
    return float(np.max(np.abs(got[~zero] - ref[~zero]) / np.abs(ref[~zero]))) if (~zero).any() else 0.0


def _check(key, got, ref, bound=None):
    e = _rel(got, ref)
    bound = REL if bound is None else bound
    parity_log.out(key, e)
    print(f"  {key}: achieved {e:.3e} (bound {bound:.1e})")
    assert e <= bound, (key, e, bound)


def _call(dev, atoms, mask, res_index, **kw):
    return fm.violations(_t(atoms, dev), _t(mask, dev), None if res_index is None else _t(np.asarray(res_index, np.int32), dev),
                         per_residue=True, **kw)


def _bits(x):
    return x.contiguous().view(torch.int64) if x.dtype == torch.float64 else x


def _same_bits(a, b, keys=None):
    return all(torch.equal(_bits(a[k]), _bits(b[k])) for k in (keys or a))


def _check_against(tag, res, p, ref, n_rows=None):
    """entry p of a batched violations(per_residue=True) result against one restatement (of the first n_rows residues)"""
    N = len(ref["connections_per_residue_loss_sum"]) if n_rows is None else n_rows
    for k in COUNTS:
        assert res[k][p].item() == ref[k], (tag, k, res[k][p].item(), ref[k])
    for k in MASK_ARRAYS:
        got = res[k][p].cpu().numpy()
        assert got.dtype == bool and np.array_equal(got[:N], ref[k]) and not got[N:].any(), (tag, k)
    for k in MEANS + ("violations_per_residue",):
        _check(f"{tag}.{k}", res[k][p].item(), ref[k])
    for k in LOSS_ARRAYS:
        got = res[k][p].cpu().numpy()
        assert not got[N:].any(), (tag, k)
        _check(f"{tag}.{k}", got[:N], ref[k])


# ---- 1. the cases of the fixture ------------------------------------------------------------------------------------------------------
def _run_case(dev, name):
    with parity_log.case(f"violations_{name}[{dev}]"):
        (atoms, mask, res_index), ref, r32, r64 = _case(name)
        n_all = len(atoms)
        print(f"  {name}: n {int(ref['num_res'])} margin {ref['margin']:.2e} bonds {ref['num_bonds']:.0f} pairs {ref['num_atom_pairs']:.0f} "
              f"clashing {ref['num_clashing_pairs']:.0f}")
        res = _call(dev, atoms[None], mask[None], res_index[None])
        assert all(res[k].dtype == torch.float64 and res[k].shape == (1,) for k in fm.VIOLATION_SLOTS)
        assert res["clashes_per_atom_loss_sum"].shape == (1, n_all, 5) and res["connections_per_residue_loss_sum"].shape == (1, n_all)
        _check_against(f"{name}.restated", res, 0, ref)
        if r64 is not None:
            # the reference's float64 run
            for k in MASK_ARRAYS:
                assert np.array_equal(res[k][0].cpu().numpy(), r64[k] != 0), (name, k)
            for k in MEANS:
                _check(f"{name}.f64.{k}", res[k][0].item(), r64[k])
            for k in LOSS_ARRAYS:
                _check(f"{name}.f64.{k}", res[k][0].cpu().numpy(), r64[k])
            # slots 8 and 9 leave the within-residue term out: the maximum of the reference's two other masks
            both = (r64["connections_per_residue_violation_mask"] != 0) | (r64["clashes_per_atom_clash_mask"] != 0).any(-1)
            assert res["num_residue_violations"].item() == float(both.sum())
            _check(f"{name}.f64.violations_per_residue", res["violations_per_residue"].item(), both.sum() / (1e-4 + ref["num_res"]))
            whole = r64["violations_within_residue"] == 0       # (the deposited chains, and chains too short to hold the term)
            if whole:
                _check(f"{name}.f64.violations_per_residue.own", res["violations_per_residue"].item(), r64["violations_per_residue"])
                assert res["num_residue_violations"].item() == r64["total_per_residue_violations_mask"].sum()
            # the reference's float32 run: 4 x the reference's own float32-against-float64 difference, per quantity
            gap = _gaps()
            for k in MASK_ARRAYS:
                assert np.array_equal(res[k][0].cpu().numpy(), r32[k] != 0), (name, k)
            for k in MEANS + (("violations_per_residue",) if whole else ()):
                _check(f"{name}.f32.{k}", res[k][0].item(), r32[k], 4 * gap[k])
            for k in LOSS_ARRAYS:
                e = float(np.abs(res[k][0].cpu().numpy() - r32[k]).max())
                print(f"  {name}.f32.{k}: achieved {e:.3e} absolute (bound {4 * gap[k]:.1e})")
                assert e <= 4 * gap[k], (name, k, e, gap[k])
        # again: identical bits
        assert _same_bits(res, _call(dev, atoms[None], mask[None], res_index[None]))
        # the compacted chain with its numbers: the same compacted chain, the same bits
        keep = ref["keep"]
        comp = _call(dev, atoms[keep][None], None if len(keep) == 0 else mask[keep][None], res_index[keep][None])
        assert _same_bits(res, comp, fm.VIOLATION_SLOTS)
        assert torch.equal(_bits(res["clashes_per_atom_loss_sum"][0, torch.as_tensor(keep, device=dev)]),
                           _bits(comp["clashes_per_atom_loss_sum"][0]))
        # without B, without the arrays
        one = fm.violations(_t(atoms, dev), _t(mask, dev), _t(res_index, dev))
        assert set(one) == set(fm.VIOLATION_SLOTS) and all(one[k].dim() == 0 for k in one)
        assert all(torch.equal(_bits(one[k].reshape(1)), _bits(res[k])) for k in one)


@pytest.mark.parametrize("name", NAMES)
def test_case_emu(use_emu, name):
    _run_case("cpu", name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_case_gpu(hip_lib, name):
    _run_case("cuda", name)


def test_fixture_is_what_the_issue_asks():
    """the properties the cases were built for, on the reference's own float64 results"""
    r = {name: _case(name) for name in NAMES}
    assert 0 < r["walk37"][3]["violations_between_residue_bond"] < 1
    assert all(r["walk37"][3][k] > 0 for k in MEANS[:3])
    assert r["removed53"][1]["num_res"] == 51 and r["removed53"][1]["num_bonds"] == 48
    assert r["scaled64"][1]["num_clashing_pairs"] >= 24
    assert r["walk130"][3]["violations_extreme_ca_ca_distance"] > 0
    assert r["single"][1]["num_res"] == 1 and r["empty"][1]["num_res"] == 0 and r["empty"][3] is None
    # the bonded C-N pair is no clash; the same coordinates with a gap in the numbering: both C-N pairs are
    assert r["bonded3"][1]["num_clashing_pairs"] == 0 and r["bonded3"][1]["num_atom_pairs"] == 3 * 25 - 2
    assert r["gapped3"][1]["num_clashing_pairs"] == 2 and r["gapped3"][1]["num_atom_pairs"] == 3 * 25
    assert r["gapped3"][3]["clashes_per_atom_clash_mask"].sum() == 4 and r["gapped3"][1]["num_bonds"] == 0
    # a number given twice: the two residues share no counted pair (24) and no bond, and 18-20 and 19-21 are now numbered
    # consecutively: their C-N pairs leave too
    assert r["repeat37"][1]["num_atom_pairs"] == r["walk37"][1]["num_atom_pairs"] - 26 and r["repeat37"][1]["num_bonds"] == 35
    for name in ("6MRR", "3HTN"):
        assert r[name][3]["violations_within_residue"] == 0 and r[name][3]["clashes_mean_loss"] == 0
    assert r["3HTN"][1]["num_bonds"] < r["3HTN"][1]["num_res"] - 1           # its numbering has gaps


# ---- 2. bits: alone, elsewhere in a batch, padded; res_index None against arange --------------------------------------------------------
def _run_bits(dev):
    (a37, _, _), ref37, _, _ = _case("walk37")
    (a64, _, _), ref64, _, _ = _case("scaled64")
    (a68, _, i68), _, _, _ = _case("6MRR")
    alone = _call(dev, a37[None], None, None)
    N = 150                                                      # three tiles: the last one holds no residue of any row
    atoms = np.full((3, N, 5, 3), np.nan, np.float32)            # padding rows may hold anything
    atoms[:, 1::2] = 3.0e30
    mask = np.zeros((3, N), np.float32)
    for p, a in enumerate((a64, a37, a68)):
        atoms[p, :len(a)], mask[p, :len(a)] = a, 1
    res = _call(dev, atoms, mask, None)
    _check_against("bits.walk37", res, 1, ref37, 37)
    _check_against("bits.scaled64", res, 0, ref64, 64)
    assert all(torch.equal(_bits(res[k][1:2]), _bits(alone[k])) for k in fm.VIOLATION_SLOTS)
    for k in LOSS_ARRAYS + MASK_ARRAYS:
        assert torch.equal(_bits(res[k][1, :37]), _bits(alone[k][0])), k
        assert not res[k][1, 37:].any(), k
    # res_index=None is the position in the padded chain
    arange = np.broadcast_to(np.arange(N, dtype=np.int32), (3, N))
    assert _same_bits(res, _call(dev, atoms, mask, arange))
    # and a shifted numbering changes nothing either
    assert _same_bits(res, _call(dev, atoms, mask, arange + 1000))


def test_bits_emu(use_emu):
    _run_bits("cpu")


@pytest.mark.gpu
def test_bits_gpu(hip_lib):
    _run_bits("cuda")


# ---- 3. the device only: more than two tiles by an odd number, B = 3, one backbone partly masked -----------------------------------
@pytest.mark.gpu
def test_three_tiles_gpu(hip_lib):
    with parity_log.case("violations_three_tiles[cuda]"):
        N = 2 * fm.VIOLATIONS_TILE + 3
        mask = np.ones((3, N), np.float32)
        mask[1, [0, 5, 6, 64, 100, N - 1]] = 0
        for seed in range(131, 195):                             # the first seed whose decisions all keep the margin (it is fixed)
            rng = np.random.default_rng(seed)
            # compact random coils of CA step 3.8 A with atoms 1.5 A around each CA: bonds, angles and clashes of every kind
            ca = np.cumsum(rng.normal(size=(3, N, 3)) * (3.8 / np.sqrt(3.0)), axis=1)
            off = rng.normal(size=(3, N, 5, 3))
            off *= 1.5 / np.linalg.norm(off, axis=-1, keepdims=True)
            off[:, :, 1] = 0
            atoms = (ca[:, :, None] + off).astype(np.float32)
            atoms[1, mask[1] == 0] = np.nan
            refs = [_np_violations(atoms[p], mask[p]) for p in range(3)]
            if min(r["margin"] for r in refs) >= MARGIN:
                break
        res = _call("cuda", atoms, mask, None)
        for p, ref in enumerate(refs):
            assert ref["margin"] >= MARGIN, (p, ref["margin"])
            assert ref["num_clashing_pairs"] > 0 and ref["bonds_c_n_loss_mean"] > 0
            _check_against(f"three_tiles.{p}", res, p, ref)


# ---- 4. eval_rows(violations=True) ----------------------------------------------------------------------------------------------------
def _run_eval_rows(dev):
    a37 = np.zeros((2, 70, 37, 3), np.float32)
    mask = np.zeros((2, 70), np.float32)
    for p, name in enumerate(("walk37", "6MRR")):
        a = _case(name)[0][0]
        a37[p, :len(a), :5], mask[p, :len(a)] = a, 1
    plain = fm.eval_rows(_t(a37, dev), _t(mask, dev))
    rows = fm.eval_rows(_t(a37, dev), _t(mask, dev), violations=True)
    direct = fm.violations(_t(a37, dev), _t(mask, dev))
    assert fm.VIOLATION_COLUMNS[:3] == ("bonds_c_n_loss_mean", "angles_ca_c_n_loss_mean", "clashes_mean_loss")   # the reference's three
    assert "angles_c_n_ca_loss_mean" in fm.VIOLATION_COLUMNS and "violations_per_residue" in fm.VIOLATION_COLUMNS
    for p, (r0, r1) in enumerate(zip(plain, rows)):
        assert set(r1) == set(r0) | set(fm.VIOLATION_COLUMNS) and all(r0[k] == r1[k] for k in r0 if r0[k] == r0[k])
        assert list(r1)[:len(r0)] == list(r0)                    # the rows are unchanged, the new columns come behind them
        assert all(isinstance(r1[k], float) and r1[k] == direct[k][p].item() for k in fm.VIOLATION_COLUMNS)
    ref = _case("walk37")[1]                                     # (numbered by position, as eval_rows numbers them)
    _check("eval_rows.bonds_c_n_loss_mean", rows[0]["bonds_c_n_loss_mean"], ref["bonds_c_n_loss_mean"])
    _check("eval_rows.clashes_mean_loss", rows[0]["clashes_mean_loss"], ref["clashes_mean_loss"])
    both = fm.eval_rows(_t(a37, dev), _t(mask, dev), shape=True, violations=True)
    assert all(both[p][k] == rows[p][k] for p in range(2) for k in fm.VIOLATION_COLUMNS) and "helix_percent" in both[0]


def test_eval_rows_emu(use_emu):
    _run_eval_rows("cpu")


@pytest.mark.gpu
def test_eval_rows_gpu(hip_lib):
    _run_eval_rows("cuda")


# ---- 5. the refused arguments ------------------------------------------------------------------------------------------------------------
def _run_arguments(dev, lib):
    n0 = lib.cdll.fd_launch_count()
    with pytest.raises(ValueError, match="2048"):
        fm.violations(torch.zeros((1, 2049, 5, 3), device=dev))
    for shape in ((1, 8, 4, 3), (1, 8, 5, 2), (8, 3), (1, 1, 8, 5, 3)):
        with pytest.raises(ValueError, match="expected"):
            fm.violations(torch.zeros(shape, device=dev))
    f = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=dev)
    ws, out = f(33 * 16, dt=torch.float64), f(1, 16, dt=torch.float64)
    with pytest.raises(hip.FdError, match="2048"):
        lib.call("fd_violations", f(1, 2049, 5, 3), 15, f(1, 2049), None, 1, 2049, ws, out, None, None, None)
    with pytest.raises(hip.FdError, match="atom_stride"):
        lib.call("fd_violations", f(1, 8, 4, 3), 12, f(1, 8), None, 1, 8, ws, out, None, None, None)
    with pytest.raises(hip.FdError, match="null"):
        lib.call("fd_violations", f(1, 8, 5, 3), 15, f(1, 8), None, 1, 8, None, out, None, None, None)
    assert lib.cdll.fd_launch_count() == n0                      # refused: nothing was launched
    res = fm.violations(f(2, 8, 5, 3))                           # all coordinates zero: no residue is present
    assert lib.cdll.fd_launch_count() == n0 + 2                  # two launches in total
    assert all(res[k].tolist() == [0.0, 0.0] for k in fm.VIOLATION_SLOTS)
    # no residues at all, no backbones at all: nothing is launched, the values are the formulas' (0)
    res = fm.violations(f(2, 0, 5, 3), per_residue=True)
    assert all(res[k].tolist() == [0.0, 0.0] for k in fm.VIOLATION_SLOTS) and res["clashes_per_atom_clash_mask"].shape == (2, 0, 5)
    assert fm.violations(f(0, 8, 5, 3))["clashes_mean_loss"].shape == (0,)
    assert lib.cdll.fd_launch_count() == n0 + 2


def test_arguments_emu(use_emu):
    _run_arguments("cpu", use_emu)


@pytest.mark.gpu
def test_arguments_gpu(hip_lib):
    _run_arguments("cuda", hip_lib)


# ---- 6. the sampler's switch -------------------------------------------------------------------------------------------------------------
def _run_sampler(dev, lib, full):
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

    def run(**kw):
        feats = sampler.init_feats(diff, B, N, dev, noise=(T["init_randn"], T["init_rand"], T["init_normal"]))
        feats["res_mask"][1, N - 2:] = 0                                   # one padded tail
        n0 = lib.cdll.fd_launch_count()
        out = sampler.sample(m, diff, feats, num_t=1, min_t=float(T["min_t"]), noise_scale=float(T["noise_scale"]),
                             noise_fn=lambda i, shp: (zr[i], zt[i]), **kw)
        return out, lib.cdll.fd_launch_count() - n0, feats

    # (one reverse step: this is about the switch.  The first run also launches the lazily built tables, so its count is not used.)
    every, _, _ = run(metrics="all")
    vio, n_vio, feats = run(metrics="violations")
    on, n_on, _ = run(metrics=True)
    assert n_vio == n_on + 2                                               # fd_violations' two launches, after the loop
    if full:                                                               # (the interpreter takes seconds per run: the device only)
        off, n_off, _ = run()
        shp, n_shp, _ = run(metrics="shape")
        _, n_all, _ = run(metrics="all")
        assert n_on == n_off + 1 and n_shp == n_on + 2                     # False, True and "shape": what they launch today
        assert n_all == n_on + 4 and set(off) | {"metrics"} == set(on) == set(vio) == set(every)
        assert set(shp["metrics"]) == set(fm.BACKBONE_SLOTS) | set(fm.SHAPE_SLOTS) | {"ss"}
    assert set(on["metrics"]) == set(fm.BACKBONE_SLOTS)
    assert set(vio["metrics"]) == set(fm.BACKBONE_SLOTS) | set(fm.VIOLATION_SLOTS)
    assert set(every["metrics"]) == set(fm.BACKBONE_SLOTS) | set(fm.SHAPE_SLOTS) | {"ss"} | set(fm.VIOLATION_SLOTS)
    assert torch.equal(vio["atom37"], on["atom37"]) and torch.equal(every["rigids"], on["rigids"])
    direct = fm.violations(vio["atom37"], feats["res_mask"])
    shape = fm.secondary_structure(vio["atom37"], feats["res_mask"])
    for k in fm.VIOLATION_SLOTS:
        assert vio["metrics"][k].shape == (B,) and torch.equal(_bits(vio["metrics"][k]), _bits(direct[k])), k
        assert torch.equal(_bits(every["metrics"][k]), _bits(direct[k])), k
    for k in fm.BACKBONE_SLOTS:
        assert torch.equal(_bits(vio["metrics"][k]), _bits(on["metrics"][k])), k
    for k in fm.SHAPE_SLOTS + ("ss",):
        assert torch.equal(_bits(every["metrics"][k]), _bits(shape[k])), k
    assert vio["metrics"]["num_res"].tolist() == [float(N), float(N - 2)]
    assert vio["metrics"]["num_bonds"].tolist() == [float(N - 1), float(N - 3)]
    ref = _np_violations(vio["atom37"][1].cpu().numpy(), feats["res_mask"][1].cpu().numpy())
    _check("sampler.clashes_mean_loss", vio["metrics"]["clashes_mean_loss"][1].item(), ref["clashes_mean_loss"])
    _check("sampler.bonds_c_n_loss_mean", vio["metrics"]["bonds_c_n_loss_mean"][1].item(), ref["bonds_c_n_loss_mean"])
    for bad in ("violation", "shapes"):
        with pytest.raises(ValueError, match="violations"):
            run(metrics=bad)


def test_sampler_violations_emu(use_emu):
    _run_sampler("cpu", use_emu, False)


@pytest.mark.gpu
def test_sampler_violations_gpu(hip_lib):
    _run_sampler("cuda", hip_lib, True)
