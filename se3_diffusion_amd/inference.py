"""Experiment.inference_fn of the reference (experiments/train_se3_diffusion.py:718-818) on the device-resident sampler.

The reference's loop moves both scores, the mask and the frames to numpy in every diffusion step, runs the reverse step on the
host, moves the frames back and copies two to four arrays per step for the trajectory -- each a device synchronisation, 500
times per backbone.  `inference_fn` below has the reference's signature, defaults and return value, and runs
sampler.sample(record=...) instead: the frames stay in HBM, one captured hipGraph is replayed per step, the trajectory is
recorded on the device by one launch per step (fd_sample_record) and reaches the host in ONE transfer per array at the end.

    dropin.install(reference_root, device_inference=True)      # binds it as Experiment.inference_fn

What differs from the reference's loop:
  * random stream: the reference draws every step's noise from numpy's global generator on the host; here the draws come from
    `generator` on the device, so a seed reproduces this function's trajectory, not the reference's -- same distribution, other
    numbers.  `noise_fn(step, shape) -> (z_rot, z_trans)` injects a given stream (the parity tests inject the reference's).
  * the returned arrays are float32 (the reference's follow its float64 numpy-born masks for trans_traj / psi_pred).
  * unbatched frames (rigids_t.ndim == 2) are not supported.
"""
from __future__ import annotations

import numpy as np
import torch

from . import sampler

_F32_KEYS = ("res_mask", "fixed_mask", "torsion_angles_sin_cos", "sc_ca_t", "rigids_t")


def inference_fn(self, data_init, num_t=None, min_t=None, center=True, aux_traj=False, self_condition=True, noise_scale=1.0,
                 *, generator=None, noise_fn=None, use_graph=True):
    """Drop-in for Experiment.inference_fn: `self` needs .model, .diffuser, ._data_conf.{num_t, min_t} and
    ._model_conf.embed.embed_self_conditioning.  data_init is the feature dict as the reference's Sampler.sample builds it
    (inference_se3_diffusion.py:427-449: float64 numpy-born masks and zeros, int64 seq_idx, a leading batch axis) and is not
    modified.  Returns numpy float32 arrays under the reference's keys -- prot_traj [T,B,N,37,3], and with aux_traj rigid_traj
    [T+1,B,N,7], trans_traj [T,B,N,3], rigid_0_traj [T,B,N,37,3], index 0 = the final structure -- plus psi_pred [1,B,N,2], a
    tensor as in the reference.

    Noise is drawn on the device from `generator` (torch): a seed does NOT reproduce the reference's trajectory, which consumes
    numpy's global stream on the host -- only its distribution.  noise_fn injects draws, as in sampler.sample."""
    rig = data_init["rigids_t"]
    if rig.ndim == 2:
        raise ValueError("inference_fn: unbatched rigids_t [N, 7] is not supported by the device sampler: add a batch axis "
                         "(rigids_t[None], as the reference's Sampler.sample does)")
    if num_t is None:
        num_t = self._data_conf.num_t
    if min_t is None:
        min_t = self._data_conf.min_t
    steps = np.linspace(min_t, 1.0, num_t)[::-1]
    if not (len(steps) >= 2 and steps[0] > min_t):
        raise ValueError(f"inference_fn: num_t={num_t} leaves no reverse step in front of the final one (the reference's loop "
                         "fails there with an unbound rigid_pred)")
    dev = rig.device
    feats = {k: (v.to(device=dev, dtype=torch.float32) if k in _F32_KEYS else v.to(dev)) if torch.is_tensor(v) else v
             for k, v in data_init.items()}      # (.to copies or aliases; sampler.sample clones before it writes)
    embed_sc = bool(self._model_conf.embed.embed_self_conditioning)
    out = sampler.sample(self.model, self.diffuser, feats, num_t=num_t, min_t=min_t, noise_scale=noise_scale,
                         self_condition=bool(self_condition and embed_sc), center=center, generator=generator, noise_fn=noise_fn,
                         use_graph=use_graph, record="reference" if aux_traj else "prot")
    to_np = lambda x: x.cpu().numpy()            # one device-to-host transfer per array
    ret = {"prot_traj": to_np(out["prot_traj"])}
    if aux_traj:
        ret["rigid_traj"] = to_np(out["rigid_traj"])
        ret["trans_traj"] = to_np(out["trans_traj"])
        ret["psi_pred"] = out["psi_pred"]
        ret["rigid_0_traj"] = to_np(out["rigid_0_traj"])
    return ret
