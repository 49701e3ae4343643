"""se3_diffusion_amd.inference.inference_fn -- the reference's Experiment.inference_fn (experiments/train_se3_diffusion.py:718-818)
on the device-resident sampler -- against tests/golden/infer_traj.npz: everything the UNMODIFIED reference returns for
aux_traj=True at full depth, B=2 x N=64, 27 steps, backbone 1 with fixed rows and a padded tail
(tools/make_golden_infer_traj.py), the reference's numpy draws injected.  And the drop-in switch that binds it."""
import copy
import importlib
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import framediff_oracle as fo  # noqa: E402
from se3_diffusion_amd import dropin, inference, train_step as ts  # noqa: E402
from se3_diffusion_amd.data import se3_diffuser, utils as du  # noqa: E402
from se3_diffusion_amd.model.score_network import ScoreNetwork  # noqa: E402
from test_diffuser import conf as dconf  # noqa: E402
from test_parity_full import TOL_TRAJ50, TOL_TRAJ500  # noqa: E402
import parity_log  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "infer_traj.npz")
# Frames: the bounds of tests/test_parity_full.py, unchanged -- TOL_TRAJ50 (rotation matrices, translations in A) for the chained
# reverse steps, and for the final step (the network's own frame prediction, which amplifies a perturbation of its input frames
# 6-8 x) the looser bound explained beside TOL_TRAJ500, whose third entry bounds psi of that last forward.
# Atoms and trans_traj (A), worst error against the fixture over all steps, rows with res_mask == 1 (trans_traj: all rows).
# Measured on gfx950, eager and hipGraph-replayed alike: below.  On the interpreter the fixture has NOT been measured: its 28
# full-depth forwards at B=2 x N=64 take about 80 minutes there (175 s per forward), so the suite does not run it either; the
# interpreter's share of the contract is the bit-exact comparison of tests/test_sample_record.py.  Each bound is at most 4 x the
# gfx950 figure.
MEASURED = {"prot_traj": 5.91e-5, "rigid_0_traj": 4.39e-5, "trans_traj": 4.12e-5}      # gfx950
TOL = {"prot_traj": 2e-4, "rigid_0_traj": 1.5e-4, "trans_traj": 1.5e-4}


def _stub(dev, blocks, seed, num_t, min_t):
    """what inference_fn reads of the reference's Experiment"""
    diff = se3_diffuser.SE3Diffuser(dconf())
    m = ScoreNetwork(ts.base_model_conf(blocks), diff)
    m.load_state_dict(fo.synth_params(seed=seed, conf=dict(fo.CONF, num_blocks=blocks)), strict=True)
    m = m.to(dev).eval()
    return types.SimpleNamespace(model=m, diffuser=diff, _data_conf=types.SimpleNamespace(num_t=num_t, min_t=min_t),
                                 _model_conf=m._model_conf)


def _data_init(rig, res_mask, fixed_mask, dev):
    """the feature dict as the reference's Sampler.sample builds it (inference_se3_diffusion.py:427-449): numpy-born float64 masks
    and zeros, int64 seq_idx, a leading batch axis"""
    B, N = res_mask.shape
    return {"res_mask": torch.tensor(np.asarray(res_mask, dtype=np.float64)).to(dev),
            "seq_idx": torch.arange(1, N + 1)[None].repeat(B, 1).to(dev),
            "fixed_mask": torch.tensor(np.asarray(fixed_mask, dtype=np.float64)).to(dev),
            "torsion_angles_sin_cos": torch.tensor(np.zeros((B, N, 7, 2))).to(dev),
            "sc_ca_t": torch.tensor(np.zeros((B, N, 3))).to(dev),
            "rigids_t": torch.as_tensor(rig).to(dev)}


def _fixture_case(dev, use_graph):
    T = np.load(GOLD)
    B, N, num_t = int(T["B"]), int(T["N"]), int(T["num_t"])
    exp = _stub(dev, int(T["blocks"]), int(T["seed"]), num_t, float(T["min_t"]))
    data_init = _data_init(T["rig_init"], T["res_mask"], T["fixed_mask"], dev)
    # the state of numpy's global generator at the reference's first diffuser.reverse call (rotation first, then translation)
    rs = np.random.RandomState()
    rs.set_state(("MT19937", T["rng_keys"], int(T["rng_pos"]), int(T["rng_has_gauss"]), float(T["rng_cached"])))
    noise_fn = lambda i, shp: (rs.normal(size=shp), rs.normal(size=shp))
    out = inference.inference_fn(exp, data_init, aux_traj=True, noise_scale=float(T["noise_scale"]), noise_fn=noise_fn,
                                 use_graph=use_graph)
    assert sorted(out) == ["prot_traj", "psi_pred", "rigid_0_traj", "rigid_traj", "trans_traj"]
    shapes = dict(prot_traj=(num_t, B, N, 37, 3), rigid_0_traj=(num_t, B, N, 37, 3), rigid_traj=(num_t + 1, B, N, 7),
                  trans_traj=(num_t, B, N, 3))
    for k, shp in shapes.items():
        assert isinstance(out[k], np.ndarray) and out[k].dtype == np.float32 and out[k].shape == shp, k
    assert torch.is_tensor(out["psi_pred"]) and tuple(out["psi_pred"].shape) == (1, B, N, 2)
    real = T["res_mask"] == 1                                  # [B,N]
    rm = lambda q: du.quat_wxyz_to_matrix(np.asarray(q)[..., :4].astype(np.float64))
    tag = "gfx950" if dev != "cpu" else "interpreter"
    with parity_log.case(f"inference_fn infer_traj {tag} graph={use_graph}"):
        # frames, padded rows included (a padded row is not diffused: it keeps its starting frame until the final step)
        got, ref = out["rigid_traj"], T["rigid_traj"]
        assert np.array_equal(got[num_t], ref[num_t])          # the starting frames
        er = np.abs(rm(got) - rm(ref)).reshape(num_t + 1, -1).max(1)
        et = np.abs(got[..., 4:] - ref[..., 4:]).reshape(num_t + 1, -1).max(1)
        # (index 0 = the final step; the network's output on padded rows is not part of the contract)
        er0 = np.abs(rm(got[0]) - rm(ref[0]))[real].max()
        et0 = np.abs(got[0, ..., 4:] - ref[0, ..., 4:])[real].max()
        ep = np.abs(out["psi_pred"].cpu().numpy()[0] - T["psi_pred"][0])[real].max()
        parity_log.out("chain_rot_matrix_abs", er[1:].max())
        parity_log.out("chain_trans_angstrom_abs", et[1:].max())
        parity_log.out("last_rot_matrix_abs", er0)
        parity_log.out("last_trans_angstrom_abs", et0)
        parity_log.out("psi_abs", ep)
        errs = {}
        for k, fk in (("prot_traj", "prot_traj5"), ("rigid_0_traj", "rigid_0_traj5")):
            assert np.all(out[k][..., 5:, :] == 0.0), k
            errs[k] = float(np.abs(out[k][..., :5, :] - T[fk])[:, real].max())
        errs["trans_traj"] = float(np.abs(out["trans_traj"] - T["trans_traj"]).max())       # padded rows too: zeros
        for k, e in errs.items():
            parity_log.out(k + "_angstrom_abs", e)
        print(f"[parity] inference_fn {tag} graph={use_graph}: chained steps rot {er[1:].max():.2e} trans {et[1:].max():.2e} A | "
              f"final step rot {er0:.2e} trans {et0:.2e} A psi {ep:.2e} | atoms / trans_traj A { {k: float(f'{e:.2e}') for k, e in errs.items()} }")
        assert er[1:].max() < TOL_TRAJ50[0] and et[1:].max() < TOL_TRAJ50[1], (er, et)
        assert er0 < TOL_TRAJ500[0] and et0 < TOL_TRAJ500[1] and ep < TOL_TRAJ500[2], (er0, et0, ep)
        for k, e in errs.items():
            assert e < TOL[k], (k, e)
        # padding rule: zeros in trans_traj, real atoms in prot_traj
        assert np.all(out["trans_traj"][:, ~real] == 0.0) and np.abs(out["prot_traj"][:, ~real][..., :5, :]).min() > 0.0
        # the reference's stale prediction in the final step (train_se3_diffusion.py:778-790): the frames of rigid_0_traj[0] are
        # those of the previous step, psi is the fresh one -- CA identical bit for bit, O moved
        assert np.array_equal(out["rigid_0_traj"][0, ..., 1, :], out["rigid_0_traj"][1, ..., 1, :])
        assert not np.array_equal(out["rigid_0_traj"][0, ..., 4, :], out["rigid_0_traj"][1, ..., 4, :])
        assert np.array_equal(T["rigid_0_traj5"][0, ..., 1, :], T["rigid_0_traj5"][1, ..., 1, :])     # (so does the reference)


@pytest.mark.gpu
@pytest.mark.parametrize("use_graph", [False, True])
def test_inference_fn_against_reference_gpu(hip_lib, use_graph):
    _fixture_case("cuda", use_graph)


def _small(num_t=4):
    exp = _stub("cpu", 1, 3, num_t, 0.01)
    B, N = 1, 10
    rig = exp.diffuser.sample_ref_device(B * N, "cpu", generator=torch.Generator().manual_seed(1)).view(B, N, 7)
    res, fixed = np.ones((B, N)), np.zeros((B, N))
    res[0, 8:] = 0.0
    fixed[0, 1:3] = 1.0
    return exp, _data_init(rig.numpy(), res, fixed, "cpu")


def test_inference_fn_contract_emu(use_emu):
    """data_init unchanged; float64 / int64 inputs accepted; defaults from _data_conf; aux_traj=False returns prot_traj only"""
    exp, data_init = _small()
    assert data_init["res_mask"].dtype == torch.float64 and data_init["seq_idx"].dtype == torch.int64
    before = copy.deepcopy(data_init)
    gen = lambda: torch.Generator().manual_seed(5)
    out = inference.inference_fn(exp, data_init, aux_traj=True, generator=gen())
    assert sorted(data_init) == sorted(before)
    for k, v in before.items():
        assert data_init[k].dtype == v.dtype and torch.equal(data_init[k], v), k
    assert out["prot_traj"].shape == (4, 1, 10, 37, 3) and out["rigid_traj"].shape == (5, 1, 10, 7)
    assert np.array_equal(out["rigid_traj"][4], before["rigids_t"].numpy())
    assert all(out[k].dtype == np.float32 for k in ("prot_traj", "rigid_traj", "trans_traj", "rigid_0_traj"))
    assert torch.is_tensor(out["psi_pred"]) and tuple(out["psi_pred"].shape) == (1, 1, 10, 2)
    only = inference.inference_fn(exp, data_init, generator=gen())
    assert sorted(only) == ["prot_traj"] and np.array_equal(only["prot_traj"], out["prot_traj"])
    # noise_scale defaults to the reference's 1.0, not the sampler's 0.1
    low = inference.inference_fn(exp, data_init, noise_scale=0.1, generator=gen())
    assert not np.array_equal(low["prot_traj"], only["prot_traj"])
    assert inference.inference_fn(exp, data_init, num_t=3, generator=gen())["prot_traj"].shape[0] == 3


def test_inference_fn_unsupported_emu(use_emu):
    exp, data_init = _small()
    flat = dict(data_init, rigids_t=data_init["rigids_t"][0])
    with pytest.raises(ValueError, match="unbatched"):
        inference.inference_fn(exp, flat)
    with pytest.raises(ValueError, match="num_t=1"):
        inference.inference_fn(exp, data_init, num_t=1)


def _checkout(tmp_path, name):
    root = tmp_path / name
    (root / "experiments").mkdir(parents=True)
    (root / "experiments" / "__init__.py").write_text("")
    (root / "experiments" / "train_se3_diffusion.py").write_text("class Experiment:\n    pass\n")
    return str(root)


def test_dropin_device_inference_switch(tmp_path):
    """dropin.install(root, device_inference=True) rebinds Experiment.inference_fn of the checkout's experiments package;
    without the flag it does not"""
    saved_modules, saved_path = dict(sys.modules), list(sys.path)
    try:
        for flag in (False, True):
            for k in [k for k in sys.modules if k == "experiments" or k.startswith("experiments.")]:
                del sys.modules[k]
            root = _checkout(tmp_path, f"checkout_{int(flag)}")
            dropin.install(root, device_inference=flag)
            importlib.invalidate_caches()
            tr = importlib.import_module("experiments.train_se3_diffusion")
            assert os.path.dirname(os.path.dirname(tr.__file__)) == root
            if flag:
                assert tr.Experiment.inference_fn is inference.inference_fn
            else:
                assert not hasattr(tr.Experiment, "inference_fn")
            sys.path.remove(root)
    finally:
        sys.path[:] = saved_path
        for k in [k for k in sys.modules if k not in saved_modules]:
            del sys.modules[k]
        sys.modules.update(saved_modules)
