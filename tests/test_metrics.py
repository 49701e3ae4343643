"""Scoring sampled backbones on the device (fd_backbone_metrics / fd_aligned_rmsd, se3_diffusion_amd.metrics,
sampler.sample(metrics=True)).

Two references:
  * tests/golden/metrics.npz (tools/make_golden_metrics.py): the UNMODIFIED reference's ca_ca_distance, ca_ca_clashes,
    calc_aligned_rmsd and rigid_transform_3D on the float32-rounded coordinates widened to float64;
  * a float64 numpy restatement, written here, of every slot the reference has no function for (the slot tables of
    include/fd_hip.h), with a textbook Kabsch superposition (SVD, determinant fix) behind the pair quantities.

Bounds, the same on the interpreter and on the device: counts, num_res and reflection exactly; the other scalars within
1e-9 * max(1, |ref|); R and t within 1e-8 absolute.  They are derived, not tuned: both sides compute in float64 from identical
float32 inputs, the longest sum has 130 * 129 / 2 = 8,385 terms (n * 2^-53 ~ 1e-12), and the fixture's eigenvalue gaps are of the
order of the largest eigenvalue, so the rotation is as well conditioned as the covariance.  The generator keeps every compared
distance at least 1e-3 A from its threshold, which is what makes the exact comparison of the counts sound.  Each case reports
what it achieved through parity_log (expected: <= 1e-11)."""
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

G = np.load(os.path.join(ROOT, "tests", "golden", "metrics.npz"))
CA_CA, C_N, C_N_TOL = 3.80209737096, 1.329, 12 * 0.014
REL = 1e-9
NAN = float("nan")


# ---- float64 numpy restatements (computed once, shared, never modified) -------------------------------------------------------
def _np_backbone(bb, mask):
    """slots 0..8 of one backbone [N,A,3] by their definitions"""
    bb = bb[mask != 0].astype(np.float64)
    n = len(bb)
    ca, c, nn = bb[:, 1], bb[:, 2], bb[:, 0]
    with np.errstate(all="ignore"):
        d = np.linalg.norm(ca[1:] - ca[:-1], axis=-1)
        D = np.linalg.norm(ca[:, None] - ca[None], axis=-1)[np.triu_indices(n, 1)]
        e = np.abs(np.linalg.norm(c[:-1] - nn[1:], axis=-1) - C_N)
        mean = lambda x: float(np.mean(x)) if len(x) else NAN
        rg = float(np.sqrt(np.mean(np.sum((ca - ca.mean(0)) ** 2, axis=-1)))) if n else NAN
        clashes = float(np.sum((D > 0) & (D < 1.5)))
        pos = float(np.sum(D > 0))
        return [float(n), mean(np.abs(d - CA_CA)), mean(d < CA_CA + 0.1), clashes, clashes / pos if pos else NAN, rg,
                mean(e), mean(e <= C_N_TOL), float(d.max()) if len(d) else 0.0]


def _np_kabsch(a, b):
    """optimal proper rotation of a onto b (textbook Kabsch: SVD of the covariance, determinant fix): R, t, det(H) < 0"""
    ca, cb = a.mean(0), b.mean(0)
    H = (a - ca).T @ (b - cb)
    U, S, Vt = np.linalg.svd(H)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))])
    R = Vt.T @ D @ U.T
    return R, cb - R @ ca, bool(np.linalg.det(H) < 0)


def _np_pair(a, b, mask=None):
    """slots 0..5 of one pair by their definitions"""
    if mask is not None:
        a, b = a[mask != 0], b[mask != 0]
    a, b = a.astype(np.float64), b.astype(np.float64)
    L = len(a)
    if L == 0:
        return [0.0, NAN, NAN, NAN, 0.0, NAN]
    R, t, refl = _np_kabsch(a, b)
    d = np.linalg.norm(a @ R.T + t - b, axis=-1)
    d0 = 1.24 * np.cbrt(L - 15.0) - 1.8 if L > 21 else 0.5
    return [float(L), float(d.mean()), float(np.sqrt(np.mean(d * d))), float(np.mean(1.0 / (1.0 + (d / d0) ** 2))), float(refl),
            float(d.max())]


BB_NP = np.array([_np_backbone(G["atoms"][k], G["res_mask"][k]) for k in range(6)])
PAIR_NP = np.array([_np_pair(G["pair_a"][p], G["pair_b"][p], G["pair_mask"][p]) for p in range(4)])


def _err(got, ref):
    """max over the entries of |got - ref| / max(1, |ref|); NaN must meet NaN"""
    got, ref = np.asarray(got, np.float64).reshape(-1), np.asarray(ref, np.float64).reshape(-1)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (got, ref)
    ok = ~np.isnan(ref)
    return float(np.max(np.abs(got[ok] - ref[ok]) / np.maximum(1.0, np.abs(ref[ok])))) if ok.any() else 0.0


def _check(key, got, ref, bound=REL):
    e = _err(got, ref)
    parity_log.out(key, e)
    print(f"  {key}: achieved {e:.3e} (bound {bound:.0e})")
    assert e <= bound, (key, e, got, ref)


def _bits(x):
    return x.contiguous().view(torch.int64)


def _same_bits(a, b):
    return all(torch.equal(_bits(a[k]), _bits(b[k])) for k in a) and a.keys() == b.keys()


def _t(x, dev):
    return torch.as_tensor(np.ascontiguousarray(x)).to(dev)


def _cols(res, names):
    return np.stack([res[n].cpu().numpy() for n in names], axis=-1)


# ---- 1. backbones against the fixture and the restatement ---------------------------------------------------------------------
def _run_backbone_fixture(dev):
    with parity_log.case(f"metrics_backbone_fixture[{dev}]"):
        res = fm.backbone_metrics(_t(G["atoms"], dev), _t(G["res_mask"], dev))
        assert list(res) == list(fm.BACKBONE_SLOTS) and all(v.shape == (6,) and v.dtype == torch.float64 for v in res.values())
        ref = G["bb_ref"]                    # ca_ca_bond_dev, ca_ca_valid_percent, num clashes, clash percent (the reference's)
        assert res["num_res"].tolist() == [37.0, 51.0, 37.0, 130.0, 1.0, 0.0]
        assert res["num_ca_steric_clashes"].tolist() == ref[:, 2].tolist()
        assert ref[2, 2] >= 24                                   # (the scaled walk clashes by the dozen)
        _check("ref.ca_ca_bond_dev", res["ca_ca_bond_dev"].cpu(), ref[:, 0])
        _check("ref.ca_ca_valid_percent", res["ca_ca_valid_percent"].cpu(), ref[:, 1])
        _check("ref.ca_steric_clash_percent", res["ca_steric_clash_percent"].cpu(), ref[:, 3])
        got = _cols(res, fm.BACKBONE_SLOTS)
        for k, name in enumerate(fm.BACKBONE_SLOTS):             # every slot against its definition (5..8 have no other reference)
            _check(f"np.{name}", got[:, k], BB_NP[:, k])
        valid = BB_NP[:, 7]
        assert np.sum((valid > 0) & (valid < 1)) >= 2            # the peptide-bond check discriminates on this fixture
        # NaN / zero pattern of the single-residue and the all-masked backbone
        one, none = got[4], got[5]
        assert np.isnan(one[[1, 2, 4, 6, 7]]).all() and one[[0, 3, 5, 8]].tolist() == [1.0, 0.0, 0.0, 0.0]
        assert np.isnan(none[[1, 2, 4, 5, 6, 7]]).all() and none[[0, 3, 8]].tolist() == [0.0, 0.0, 0.0]
        # the raw block: slots 9..11 are zero; unbatched input gives 0-d tensors with the same bits
        blk = torch.full((6, 12), NAN, dtype=torch.float64, device=dev)
        res2 = fm.backbone_metrics(_t(G["atoms"], dev), _t(G["res_mask"], dev), out=blk)
        assert _same_bits(res, res2) and blk[:, 9:].abs().sum().item() == 0.0          # (two calls, equal bits)
        r1 = fm.backbone_metrics(_t(G["atoms"][3], dev), _t(G["res_mask"][3], dev))
        assert all(r1[k].dim() == 0 and torch.equal(_bits(r1[k][None]), _bits(res[k][3:4])) for k in res)


def test_backbone_fixture_emu(use_emu):
    _run_backbone_fixture("cpu")


@pytest.mark.gpu
def test_backbone_fixture_gpu(hip_lib):
    _run_backbone_fixture("cuda")


# ---- 2. padding content and strides --------------------------------------------------------------------------------------------
def _run_padding_and_strides(dev):
    with parity_log.case(f"metrics_padding_strides[{dev}]"):
        atoms, mask = G["atoms"].copy(), G["res_mask"]
        base = fm.backbone_metrics(_t(atoms, dev), _t(mask, dev))
        rng = np.random.default_rng(0)
        for fill in (0.0, np.inf, -3.0e38, None):
            other = atoms.copy()
            pad = mask == 0
            other[pad] = rng.normal(size=other[pad].shape).astype(np.float32) * 4.0 if fill is None else fill
            assert _same_bits(base, fm.backbone_metrics(_t(other, dev), _t(mask, dev))), fill
        # atom_stride 111 (atom37) and 15 (the compact buffers) give identical bits, whatever atoms 5..36 hold
        a37 = rng.normal(size=(6, 130, 37, 3)).astype(np.float32)
        a37[:, :, :5] = atoms
        assert _same_bits(base, fm.backbone_metrics(_t(a37, dev), _t(mask, dev)))
        # a mask given as any non-zero value, and the mask derived the reference's way (any coordinate non-zero)
        assert _same_bits(base, fm.backbone_metrics(_t(atoms, dev), _t(mask * -2.5, dev)))
        zero_pad = atoms.copy()
        zero_pad[mask == 0] = 0.0
        assert _same_bits(base, fm.backbone_metrics(_t(zero_pad, dev)))


def test_padding_and_strides_emu(use_emu):
    _run_padding_and_strides("cpu")


@pytest.mark.gpu
def test_padding_and_strides_gpu(hip_lib):
    _run_padding_and_strides("cuda")


# ---- 3. a backbone at the largest N, present residues on both sides of every thread's run -----------------------------------
def _run_large(dev, n):
    with parity_log.case(f"metrics_backbone_n{n}[{dev}]"):
        rng = np.random.default_rng(5)
        steps = rng.normal(size=(n, 3))
        ca = np.cumsum(3.8 * steps / np.linalg.norm(steps, axis=-1, keepdims=True), axis=0)
        bb = (ca[:, None, :] + rng.normal(size=(n, 5, 3))).astype(np.float32)
        bb[:, 1] = (0.5 * ca).astype(np.float32)                 # (half scale: clashes by the dozen)
        mask = (rng.random(n) < 0.9).astype(np.float32)
        bb[mask == 0] = np.nan
        ref = _np_backbone(bb, mask)
        # both sides are fp64 on the same fp32 inputs (distances agree to ~1e-15); the fixed draw keeps every compared distance
        # 1e-6 clear of its threshold, so the counts are compared exactly here too
        pb = bb[mask != 0].astype(np.float64)
        d = np.linalg.norm(pb[:, None, 1] - pb[None, :, 1], axis=-1)
        assert np.abs(d[np.triu_indices(len(d), 1)] - 1.5).min() > 1e-6
        assert np.abs(np.linalg.norm(pb[1:, 1] - pb[:-1, 1], axis=-1) - (CA_CA + 0.1)).min() > 1e-6
        assert np.abs(np.abs(np.linalg.norm(pb[:-1, 2] - pb[1:, 0], axis=-1) - C_N) - C_N_TOL).min() > 1e-6
        res = fm.backbone_metrics(_t(bb, dev), _t(mask, dev))
        got = _cols(res, fm.BACKBONE_SLOTS)
        assert got[0] == ref[0] and got[3] == ref[3] and ref[3] > 10, (got, ref)
        for k, name in enumerate(fm.BACKBONE_SLOTS):
            _check(f"np.{name}", got[k], ref[k])


def test_backbone_n300_emu(use_emu):
    _run_large("cpu", 300)                                       # more than one residue per thread, n not a multiple of 256


@pytest.mark.gpu
def test_backbone_n4096_gpu(hip_lib):
    _run_large("cuda", 4096)


# ---- 4. superposition against the fixture and the restatement ------------------------------------------------------------------
def _run_pairs_fixture(dev):
    with parity_log.case(f"metrics_pairs_fixture[{dev}]"):
        pa, pb, pm = G["pair_a"], G["pair_b"], G["pair_mask"]
        # a fifth pair without a common position (L = 0) and a sixth with L <= 21 (the other branch of d0)
        few = np.zeros(53, np.float32)
        few[[2, 3, 5, 8, 13, 21, 34, 40, 41, 50]] = 1
        a6 = np.concatenate([pa, pa[3:4], pa[3:4]])
        b6 = np.concatenate([pb, pb[3:4], pb[3:4]])
        m6 = np.concatenate([pm, np.zeros((1, 53), np.float32), few[None]])
        res = fm.aligned_rmsd(_t(a6, dev), _t(b6, dev), _t(m6, dev), return_transform=True)
        assert list(res) == list(fm.RMSD_SLOTS) + ["R", "t"]
        assert res["R"].shape == (6, 3, 3) and res["t"].shape == (6, 3)
        assert res["num_aligned"].tolist() == [37.0, 37.0, 53.0, float(pm[3].sum()), 0.0, 10.0]
        assert res["reflection"].tolist()[:4] == G["pair_reflection"].tolist() == [0.0, 1.0, 0.0, 0.0]
        _check("ref.mean_dist", res["mean_dist"][:4].cpu(), G["pair_mean_dist"])
        _check("ref.R", res["R"][:4].cpu(), G["pair_R"], 1e-8)
        parity_log.out("ref.t_abs", float(np.abs(res["t"][:4].cpu().numpy() - G["pair_t"]).max()))
        assert np.abs(res["R"][:4].cpu().numpy() - G["pair_R"]).max() <= 1e-8
        assert np.abs(res["t"][:4].cpu().numpy() - G["pair_t"]).max() <= 1e-8
        R = res["R"].cpu().numpy()
        assert np.allclose(np.linalg.det(R[[0, 1, 2, 3, 5]]), 1.0, atol=1e-12)       # proper rotations, the mirrored pair included
        got = _cols(res, fm.RMSD_SLOTS)
        want = np.concatenate([PAIR_NP, [_np_pair(a6[4], b6[4], m6[4]), _np_pair(a6[5], b6[5], m6[5])]])
        for k, name in enumerate(fm.RMSD_SLOTS):
            _check(f"np.{name}", got[:, k], want[:, k])
        assert np.isnan(got[4, [1, 2, 3, 5]]).all() and got[4, 0] == 0.0              # the L = 0 pattern
        # reproducible; without the transform; unbatched and unmasked on the first 37 positions
        again = fm.aligned_rmsd(_t(a6, dev), _t(b6, dev), _t(m6, dev))
        assert _same_bits({k: res[k] for k in again}, again)
        one = fm.aligned_rmsd(_t(pa[0, :37], dev), _t(pb[0, :37], dev))
        assert all(one[k].dim() == 0 for k in one)
        _check("unmasked.mean_dist", one["mean_dist"].cpu(), G["pair_mean_dist"][0])
        # padding content: masked positions may hold anything
        a7, b7 = a6.copy(), b6.copy()
        a7[m6 == 0], b7[m6 == 0] = 7.0e30, -np.inf
        assert _same_bits(again, fm.aligned_rmsd(_t(a7, dev), _t(b7, dev), _t(m6, dev)))
        # a strided CA view of atom37 is read in place and equals the packed copy
        rng = np.random.default_rng(1)
        a37 = _t(rng.normal(size=(6, 53, 37, 3)).astype(np.float32), dev)
        b37 = _t(rng.normal(size=(6, 53, 37, 3)).astype(np.float32), dev)
        a37[:, :, 1], b37[:, :, 1] = _t(a6, dev), _t(b6, dev)
        va, vb = a37[:, :, 1], b37[:, :, 1]
        assert not va.is_contiguous() and fm._points(va)[0].data_ptr() == va.data_ptr() and fm._points(va)[1] == 111
        assert _same_bits(again, fm.aligned_rmsd(va, vb, _t(m6, dev)))


def test_pairs_fixture_emu(use_emu):
    _run_pairs_fixture("cpu")


@pytest.mark.gpu
def test_pairs_fixture_gpu(hip_lib):
    _run_pairs_fixture("cuda")


def _run_pairs_large(dev, n):
    """more than one position per thread; collinear and coincident sets still give an optimal superposition's distances"""
    with parity_log.case(f"metrics_pairs_n{n}[{dev}]"):
        rng = np.random.default_rng(2)
        a = (rng.normal(size=(3, n, 3)) * 10).astype(np.float32)
        b = (a.astype(np.float64) + rng.normal(size=(3, n, 3))).astype(np.float32)
        line = np.outer(np.arange(n), [1.0, 2.0, -1.0]).astype(np.float32)
        a[1], b[1] = line, (line @ np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], np.float32)) + 3.0
        a[2], b[2] = 1.0, -2.0                                   # every point the same
        res = fm.aligned_rmsd(_t(a, dev), _t(b, dev))
        got = _cols(res, fm.RMSD_SLOTS)
        _check("np.general", got[0], _np_pair(a[0], b[0]))
        _check("np.collinear_dists", got[1, [1, 2, 5]], [0.0, 0.0, 0.0], 1e-9)
        _check("np.coincident_dists", got[2, [1, 2, 5]], [0.0, 0.0, 0.0], 1e-9)


def test_pairs_n300_emu(use_emu):
    _run_pairs_large("cpu", 300)


@pytest.mark.gpu
def test_pairs_n4096_gpu(hip_lib):
    _run_pairs_large("cuda", 4096)


# ---- 5. all pairs of a set -------------------------------------------------------------------------------------------------------
def _run_pairwise(dev, lib):
    with parity_log.case(f"metrics_pairwise[{dev}]"):
        pos = _t(G["set_pos"], dev)
        M = pos.shape[0]
        n0 = lib.cdll.fd_launch_count()
        res = fm.pairwise_rmsd(pos)
        assert lib.cdll.fd_launch_count() == n0 + 1              # one launch over the 10 upper pairs
        assert list(res) == ["mean_dist", "rmsd", "tm_kabsch"] and all(v.shape == (M, M) for v in res.values())
        for k, diag in (("mean_dist", 0.0), ("rmsd", 0.0), ("tm_kabsch", 1.0)):
            assert torch.equal(res[k], res[k].T) and res[k].diagonal().tolist() == [diag] * M
        _check("ref.set_mean_dist", res["mean_dist"].cpu(), G["set_mean_dist"])
        for i in range(M):
            for j in range(i + 1, M):
                one = fm.aligned_rmsd(pos[i], pos[j])
                assert all(torch.equal(_bits(one[k][None]), _bits(res[k][i, j][None])) for k in res), (i, j)
        # with a mask: a position counts iff it is present in both sets
        mask = np.ones((M, 37), np.float32)
        mask[1, :5], mask[3, 30:] = 0, 0
        rm = fm.pairwise_rmsd(pos, _t(mask, dev))
        want = _np_pair(G["set_pos"][1], G["set_pos"][3], mask[1] * mask[3])
        _check("np.masked_pair", [rm[k][1, 3].item() for k in res], [want[1], want[2], want[3]])
        assert fm.pairwise_rmsd(pos[:1])["tm_kabsch"].tolist() == [[1.0]]              # a lone set: nothing to launch


def test_pairwise_emu(use_emu):
    _run_pairwise("cpu", use_emu)


@pytest.mark.gpu
def test_pairwise_gpu(hip_lib):
    _run_pairwise("cuda", hip_lib)


# ---- 6. argument errors and empty inputs -------------------------------------------------------------------------------------------
def _run_arguments(dev, lib):
    f32 = lambda *s: torch.zeros(s, device=dev)
    out = torch.full((2, 12), NAN, dtype=torch.float64, device=dev)
    with pytest.raises(hip.FdError, match="atom_stride"):
        lib.call("fd_backbone_metrics", f32(2, 8, 5, 3), 14, f32(2, 8), 2, 8, out)
    with pytest.raises(hip.FdError, match="4096"):
        fm.backbone_metrics(f32(1, 4097, 5, 3), f32(1, 4097))
    with pytest.raises(hip.FdError, match="4096"):
        fm.aligned_rmsd(f32(1, 4097, 3), f32(1, 4097, 3))
    with pytest.raises(ValueError):
        fm.backbone_metrics(f32(2, 8, 4, 3))
    po = torch.full((2, 8), NAN, dtype=torch.float64, device=dev)
    tr = torch.full((2, 12), NAN, dtype=torch.float64, device=dev)
    n0 = lib.cdll.fd_launch_count()
    lib.call("fd_backbone_metrics", f32(2, 8, 5, 3), 15, f32(2, 8), 0, 8, out)         # B == 0
    lib.call("fd_backbone_metrics", f32(2, 8, 5, 3), 15, f32(2, 8), 2, 0, out)         # N == 0
    lib.call("fd_aligned_rmsd", f32(2, 8, 3), 3, f32(2, 8, 3), 3, None, None, None, 0, 8, po, tr)
    lib.call("fd_aligned_rmsd", f32(2, 8, 3), 3, f32(2, 8, 3), 3, None, None, None, 2, 0, po, tr)
    assert fm.backbone_metrics(f32(0, 8, 37, 3), f32(0, 8))["num_res"].shape == (0,)
    assert fm.aligned_rmsd(f32(0, 8, 3), f32(0, 8, 3))["rmsd"].shape == (0,)
    assert lib.cdll.fd_launch_count() == n0
    assert all(bool(torch.isnan(x).all()) for x in (out, po, tr))                     # nothing was written


def test_arguments_emu(use_emu):
    _run_arguments("cpu", use_emu)


@pytest.mark.gpu
def test_arguments_gpu(hip_lib):
    _run_arguments("cuda", hip_lib)


def test_metrics_have_no_cpu_fallback():
    if not os.path.exists(hip.LIB_PATH):
        from se3_diffusion_amd import build
        build.build(verbose=False)
    lib = hip.FdLib(hip.LIB_PATH)
    with pytest.raises(hip.FdError):
        lib.call("fd_backbone_metrics", torch.zeros(1, 4, 5, 3), 15, torch.ones(1, 4), 1, 4, torch.zeros(1, 12, dtype=torch.float64))
    with pytest.raises(hip.FdError):
        lib.call("fd_aligned_rmsd", torch.zeros(1, 4, 3), 3, torch.zeros(1, 4, 3), 3, None, None, None, 1, 4,
                 torch.zeros(1, 8, dtype=torch.float64), None)


# ---- 7. the sampler's switch ---------------------------------------------------------------------------------------------------------
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

    def run(num_t=3, **kw):
        feats = sampler.init_feats(diff, B, N, dev, noise=(T["init_randn"], T["init_rand"], T["init_normal"]))
        feats["res_mask"][1, N - 2:] = 0                                   # one padded tail
        n0 = lib.cdll.fd_launch_count()
        out = sampler.sample(m, diff, feats, num_t=num_t, min_t=float(T["min_t"]), noise_scale=float(T["noise_scale"]),
                             noise_fn=lambda i, shp: (zr[i], zt[i]), **kw)
        return out, lib.cdll.fd_launch_count() - n0, feats

    run(num_t=2)                                                           # (lazily built tables are launched once, here)
    off, n_off, _ = run()
    on, n_on, feats = run(metrics=True)
    assert "metrics" not in off and set(on) == set(off) | {"metrics"}
    assert n_on == n_off + 1, (n_on, n_off)
    assert torch.equal(on["atom37"], off["atom37"]) and torch.equal(on["rigids"], off["rigids"])
    assert _same_bits(on["metrics"], fm.backbone_metrics(on["atom37"], feats["res_mask"]))
    assert on["metrics"]["num_res"].tolist() == [float(N), float(N - 2)]
    assert bool(torch.isfinite(on["metrics"]["ca_ca_bond_dev"]).all())


def test_sampler_metrics_emu(use_emu):
    _run_sampler("cpu", use_emu)


@pytest.mark.gpu
def test_sampler_metrics_gpu(hip_lib):
    _run_sampler("cuda", hip_lib)


# ---- 8. eval_rows --------------------------------------------------------------------------------------------------------------------
def _run_eval_rows(dev):
    with parity_log.case(f"metrics_eval_rows[{dev}]"):
        a37 = np.zeros((6, 130, 37, 3), np.float32)
        a37[:, :, :5] = G["atoms"]
        mask = G["res_mask"]
        rows = fm.eval_rows(_t(a37, dev), _t(mask, dev))
        assert len(rows) == 6 and all(isinstance(v, float) for r in rows for v in r.values())
        reference_columns = {"ca_ca_bond_dev", "ca_ca_valid_percent", "ca_steric_clash_percent", "num_ca_steric_clashes", "num_res",
                             "fixed_residues", "diffused_percentage"}
        assert reference_columns <= set(rows[0]) and set(fm.BACKBONE_SLOTS) <= set(rows[0]) and "aligned_rmsd_to_gt" not in rows[0]
        for k, r in enumerate(rows):
            _check(f"row{k}", [r[n] for n in fm.BACKBONE_SLOTS], BB_NP[k])
            assert r["fixed_residues"] == 0.0
        assert rows[0]["diffused_percentage"] == 1.0 and np.isnan(rows[5]["diffused_percentage"])
        # against a ground truth: only the diffused present residues are superposed.  The sample's CA are the fixture's
        # masked pair, its mask split into "fixed" (outside the pair's mask) and one absent residue
        pa, pb, pm = G["pair_a"][3], G["pair_b"][3], G["pair_mask"][3]
        s37 = np.random.default_rng(3).normal(size=(1, 53, 37, 3)).astype(np.float32)
        g37 = s37.copy()
        s37[0, :, 1], g37[0, :, 1] = pa, pb
        res_mask = np.ones((1, 53), np.float32)
        fixed = (1 - pm)[None].copy()
        gone = int(np.flatnonzero(pm == 0)[0])
        res_mask[0, gone] = 0                                      # absent AND marked fixed: it counts in neither column
        row = fm.eval_rows(_t(s37, dev), _t(res_mask, dev), _t(fixed, dev), _t(g37, dev))[0]
        _check("aligned_rmsd_to_gt", row["aligned_rmsd_to_gt"], G["pair_mean_dist"][3])
        assert row["num_res"] == 52.0 and row["fixed_residues"] == float((1 - pm).sum() - 1)
        assert row["diffused_percentage"] == float(pm.sum()) / 52.0
        everything = fm.eval_rows(_t(s37, dev), _t(res_mask, dev), None, _t(g37, dev))[0]
        assert abs(everything["aligned_rmsd_to_gt"] - row["aligned_rmsd_to_gt"]) > 1e-3       # (the fixed residues do matter)


def test_eval_rows_emu(use_emu):
    _run_eval_rows("cpu")


@pytest.mark.gpu
def test_eval_rows_gpu(hip_lib):
    _run_eval_rows("cuda")
