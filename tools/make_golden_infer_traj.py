"""TEST INFRASTRUCTURE -- writes tests/golden/infer_traj.npz: everything the UNMODIFIED reference's
Experiment.inference_fn(aux_traj=True) returns (experiments/train_se3_diffusion.py:718-818), on the CPU, full depth, B=2:

    backbone 0  plain
    backbone 1  a run of fixed_mask rows (both terms of trans_traj, :787-790) and padded tail rows (res_mask == 0)

Recipe of oracle/make_golden_full.py::traj_via_experiment: a recording wrapper around diffuser.reverse snapshots numpy's global
generator to learn the draws the call is about to make.  Stored: the starting frames and their draws, the generator state at the
first diffuser.reverse call (all later draws are checked to be consecutive from it), rigid_traj, trans_traj, psi_pred and atoms
0..4 (N, CA, C, CB, O) of prot_traj / rigid_0_traj -- atoms 5..36 are asserted to be exactly zero before they are dropped.

Needs a checkout of the reference (FD_REFERENCE_ROOT); the tests read only the fixture.
    python tools/make_golden_infer_traj.py [N] [num_t]
"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_loader as rl  # noqa: E402
from oracle import framediff_oracle as fo  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
CACHE = os.environ.get("FD_IGSO3_CACHE", "/tmp/fd_igso3_cache")
B, SEED, MIN_T, NOISE_SCALE = 2, 41, 0.01, 0.1
FIXED = (5, 12)        # backbone 1: rows [5, 12) carry fixed_mask = 1
N_PAD = 5              # backbone 1: the last 5 rows are padding (res_mask = 0)


def main(N=64, num_t=27):
    rl.install()
    from hydra.core.hydra_config import HydraConfig
    HydraConfig.initialized = lambda: False
    from experiments import train_se3_diffusion as tr
    torch.set_num_threads(int(os.environ.get("FD_GOLDEN_THREADS", "8")))
    base = rl.base_conf(CACHE, num_blocks=4)
    conf = rl.ns(dict(
        data=dict(min_t=MIN_T, num_t=num_t, samples_per_eval_length=1, num_eval_lengths=1),
        experiment=dict(name="golden", run_id=None, use_ddp=False, use_wandb=False, warm_start=None, use_warm_start_conf=False,
                        ckpt_dir=None, eval_dir=None, learning_rate=1e-4, num_parameters=None, batch_size=B,
                        trans_loss_weight=1.0, rot_loss_weight=0.5, rot_loss_t_threshold=0.2, separate_rot_loss=True,
                        trans_x0_threshold=1.0, coordinate_scaling=0.1, bb_atom_loss_weight=1.0, bb_atom_loss_t_filter=0.25,
                        dist_mat_loss_weight=1.0, dist_mat_loss_t_filter=0.25, aux_loss_weight=0.25, noise_scale=1.0)))
    conf.diffuser, conf.model = base.diffuser, base.model
    exp = tr.Experiment(conf=conf)
    assert type(exp.model).__module__ == "model.score_network" and type(exp.diffuser).__module__ == "data.se3_diffuser"
    exp.model.load_state_dict(fo.synth_params(seed=SEED, conf=dict(fo.CONF, num_blocks=4)), strict=True)
    exp.model.eval()
    np.random.seed(1000 + SEED)
    zr = np.random.randn(B * N, 3); ur = np.random.rand(B * N); zt = np.random.normal(size=(B * N, 3))
    np.random.seed(1000 + SEED)
    rig_init = exp.diffuser.sample_ref(n_samples=B * N, as_tensor_7=True)["rigids_t"].reshape(B, N, 7)
    # masks and zeros as Sampler.sample builds them (inference_se3_diffusion.py:427-449): numpy-born, hence float64
    res_mask = np.ones((B, N)); res_mask[1, N - N_PAD:] = 0.0
    fixed_mask = np.zeros((B, N)); fixed_mask[1, FIXED[0]:FIXED[1]] = 1.0
    feats = dict(res_mask=torch.tensor(res_mask), fixed_mask=torch.tensor(fixed_mask),
                 seq_idx=torch.arange(1, N + 1)[None].repeat(B, 1),
                 torsion_angles_sin_cos=torch.tensor(np.zeros((B, N, 7, 2))), sc_ca_t=torch.tensor(np.zeros((B, N, 3))),
                 rigids_t=rig_init.clone())
    noises, first_state = [], []
    orig_reverse = exp.diffuser.reverse

    def recording_reverse(*a, **kw):
        st = np.random.get_state()
        if not first_state:
            first_state.append(st)
        noises.append((np.random.normal(size=(B, N, 3)), np.random.normal(size=(B, N, 3))))
        np.random.set_state(st)
        return orig_reverse(*a, **kw)
    exp.diffuser.reverse = recording_reverse
    t0 = time.time()
    out = exp.inference_fn(feats, num_t=num_t, min_t=MIN_T, aux_traj=True, noise_scale=NOISE_SCALE)
    dt = time.time() - t0
    assert len(noises) == num_t - 1
    rs = np.random.RandomState()
    rs.set_state(first_state[0])
    for zr_, zt_ in noises:       # nothing but diffuser.reverse consumed the global generator: the draws are one stream
        assert np.array_equal(rs.normal(size=(B, N, 3)), zr_) and np.array_equal(rs.normal(size=(B, N, 3)), zt_)
    kind, keys, pos, has_gauss, cached = first_state[0]
    prot, rig0 = np.asarray(out["prot_traj"]), np.asarray(out["rigid_0_traj"])
    rt, tt = np.asarray(out["rigid_traj"]), np.asarray(out["trans_traj"])
    assert prot.shape == (num_t, B, N, 37, 3) and rig0.shape == prot.shape
    assert rt.shape == (num_t + 1, B, N, 7) and tt.shape == (num_t, B, N, 3) and tuple(out["psi_pred"].shape) == (1, B, N, 2)
    assert np.all(prot[..., 5:, :] == 0.0) and np.all(rig0[..., 5:, :] == 0.0)
    assert np.abs(rt[-1] - rig_init.numpy()).max() == 0.0
    path = os.path.join(GOLD, "infer_traj.npz")
    np.savez_compressed(path, B=B, N=N, num_t=num_t, min_t=MIN_T, noise_scale=NOISE_SCALE, seed=SEED, blocks=4,
                        res_mask=res_mask, fixed_mask=fixed_mask, init_randn=zr, init_rand=ur, init_normal=zt,
                        rig_init=rig_init.numpy(), rng_keys=np.asarray(keys, dtype=np.uint32), rng_pos=int(pos),
                        rng_has_gauss=int(has_gauss), rng_cached=float(cached), n_reverse=len(noises),
                        rigid_traj=rt.astype(np.float32), trans_traj=tt.astype(np.float32),
                        psi_pred=out["psi_pred"].numpy().astype(np.float32),
                        prot_traj5=prot[..., :5, :].astype(np.float32), rigid_0_traj5=rig0[..., :5, :].astype(np.float32))
    print(f"{path}: {os.path.getsize(path)} bytes, B={B} N={N} num_t={num_t}, {dt:.1f} s of reference CPU time; dtypes "
          f"{prot.dtype} {rt.dtype} {tt.dtype} {out['psi_pred'].dtype}")


if __name__ == "__main__":
    main(*[int(a) for a in sys.argv[1:3]])
