"""fd_sample_record (one launch per diffusion step writes that step's slice of the four trajectories of
Experiment.inference_fn(aux_traj=True), reference experiments/train_se3_diffusion.py:782-812) and sampler.sample(record=...).

Kernel: against a float64 numpy restatement of the four rows of the table in include/fd_hip.h.  Sampler: the recorded arrays
against what the unrecorded loop gives for the same injected noise."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import framediff_oracle as fo  # noqa: E402
from se3_diffusion_amd import hip, sampler, train_step as ts, trunk  # noqa: E402
from se3_diffusion_amd.data import se3_diffuser  # noqa: E402
from se3_diffusion_amd.model.score_network import ScoreNetwork  # noqa: E402
from test_diffuser import conf as dconf  # noqa: E402

SENTINEL = -777.0
# Atoms against float64: |coordinate| <= 30 A + 2.4 A of local geometry < 64, where a float32 ulp is 3.8e-6 A.  Each coordinate
# is a sum of three products plus the translation (4 roundings of at most half an ulp at that magnitude: 7.6e-6) of rotation
# entries that carry ~3 roundings of 6e-8 on values <= 1, times local coordinates <= 2.4 A (4e-7 each, three of them); O goes
# through two such rotations.  Bound: 2e-5 A.  Frames and masked translations are copies / products with 0 and 1: exact.
TOL_ATOMS = 2e-5


def _ref_atoms(rig, psi, hc):
    """float64: N, CA, C, CB, O of compute_backbone (all_atom.py:152-174; the arithmetic of csrc/fd_atoms.h)"""
    rig, psi = rig.astype(np.float64), psi.astype(np.float64)
    atoms = np.array(list(hc.atoms), dtype=np.float64).reshape(5, 3)
    Rd, td = np.array(list(hc.Rd), dtype=np.float64).reshape(3, 3), np.array(list(hc.td), dtype=np.float64)
    a, b, c, d = (rig[:, k] for k in range(4))
    Rm = np.stack([np.stack([a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c)], -1),
                   np.stack([2 * (b * c + a * d), a * a - b * b + c * c - d * d, 2 * (c * d - a * b)], -1),
                   np.stack([2 * (b * d - a * c), 2 * (c * d + a * b), a * a - b * b - c * c + d * d], -1)], 1)   # [R,3,3]
    t = rig[:, 4:]
    ps, pc = psi[:, 0], psi[:, 1]
    o = atoms[4]
    rot = np.stack([np.full_like(ps, o[0]), pc * o[1] - ps * o[2], ps * o[1] + pc * o[2]], -1)        # rotation about x by psi
    local = np.concatenate([np.broadcast_to(atoms[:4], (len(rig), 4, 3)), (rot @ Rd.T + td)[:, None]], 1)  # [R,5,3]
    return np.einsum("rij,rnj->rni", Rm, local) + t[:, None]


def _inputs(R, seed):
    g = np.random.RandomState(seed)
    unit = lambda u: u / np.linalg.norm(u, axis=1, keepdims=True)
    mk = lambda: np.concatenate([unit(g.normal(size=(R, 4))), g.uniform(-30, 30, size=(R, 3))], 1).astype(np.float32)
    ang = g.uniform(-np.pi, np.pi, size=R)
    return dict(rig_t=mk(), pred=mk(), psi=np.stack([np.sin(ang), np.cos(ang)], 1).astype(np.float32),
                fixed=(g.uniform(size=R) < 0.3).astype(np.float32), res=(g.uniform(size=R) < 0.8).astype(np.float32))


def _launch(lib, dev, x, T, R, aux, slot_ptr, slot, bufs):
    td = {k: torch.from_numpy(v).to(dev) for k, v in x.items()}
    lib.call("fd_sample_record", td["rig_t"], td["pred"] if aux else None, td["psi"], td["fixed"] if aux else None,
             td["res"] if aux else None, trunk.head_const(), slot_ptr, slot, T, R, int(aux),
             bufs["rigid_traj"] if aux else None, bufs["bb_t"], bufs["bb_0"] if aux else None, bufs["trans_0"] if aux else None)


def _bufs(T, R, dev):
    new = lambda *s: torch.full(s, SENTINEL, dtype=torch.float32, device=dev)
    return dict(rigid_traj=new(T + 1, R, 7), bb_t=new(T, R, 5, 3), bb_0=new(T, R, 5, 3), trans_0=new(T, R, 3))


def _check_slice(bufs, x, T, step, aux):
    """slot T-1-step holds the step, every other slot still the sentinel"""
    hc = trunk.head_const()
    idx = T - 1 - step
    got = {k: v.cpu().numpy() for k, v in bufs.items()}
    err = float(np.abs(got["bb_t"][idx] - _ref_atoms(x["rig_t"], x["psi"], hc)).max())
    assert err < TOL_ATOMS, err
    if aux:
        err0 = float(np.abs(got["bb_0"][idx] - _ref_atoms(x["pred"], x["psi"], hc)).max())
        assert err0 < TOL_ATOMS, err0
        err = max(err, err0)
        assert np.array_equal(got["rigid_traj"][idx], x["rig_t"])
        f64 = lambda k: x[k].astype(np.float64)
        dm, fm = (1 - f64("fixed")) * f64("res"), f64("fixed") * f64("res")
        want = dm[:, None] * f64("pred")[:, 4:] + fm[:, None] * f64("rig_t")[:, 4:]
        assert np.array_equal(got["trans_0"][idx].astype(np.float64), want)
        assert np.all(got["trans_0"][idx][x["res"] == 0] == 0.0)
    for k, v in got.items():
        touched = aux or k == "bb_t"
        rest = np.delete(v, idx, axis=0) if touched else v
        assert np.all(rest == SENTINEL), (k, "written outside its slot" if touched else "written with aux=0")
    return err


def _kernel_cases(lib, dev):
    worst = 0.0
    # (rows, T, step, aux, slot from the device counter?)  74: not a multiple of the block's 64 rows; 64*1024 + 1: one row above
    # what the launcher's grid cap covers in one pass
    for R, T, step, aux, counter in ((74, 5, 0, True, False), (74, 5, 4, True, True), (74, 5, 2, False, False),
                                     (74, 5, 3, False, True), (128, 3, 1, True, True), (1, 2, 1, True, False),
                                     (64 * 1024 + 1, 2, 0, True, True)):
        x, bufs = _inputs(R, seed=R + step), _bufs(T, R, dev)
        if counter:
            # as in a captured step: fd_sample_advance has already advanced the counter when the record runs (offset -1)
            cnt = torch.full((1,), step + 1, dtype=torch.int32, device=dev)
            _launch(lib, dev, x, T, R, aux, cnt, -1, bufs)
            assert int(cnt.item()) == step + 1          # the kernel only reads it
        else:
            _launch(lib, dev, x, T, R, aux, None, step, bufs)
        worst = max(worst, _check_slice(bufs, x, T, step, aux))
    print(f"[record] fd_sample_record on {dev}: worst atom error against float64 {worst:.2e} A (bound {TOL_ATOMS:.0e})")
    # a step outside [0, T): an error of the launcher where the host knows it, a skipped write where it does not
    R, T = 74, 5
    x, bufs = _inputs(R, seed=1), _bufs(T, R, dev)
    for bad in (T, -1):
        with pytest.raises(hip.FdError):
            _launch(lib, dev, x, T, R, True, None, bad, bufs)
    for bad in (T + 1, 0, 1000000):                     # counter - 1 = T, -1, far outside
        _launch(lib, dev, x, T, R, True, torch.full((1,), bad, dtype=torch.int32, device=dev), -1, bufs)
    if dev != "cpu":
        torch.cuda.synchronize()
    assert all(bool((v == SENTINEL).all()) for v in bufs.values())


def test_sample_record_kernel_emu(emu_lib):
    _kernel_cases(emu_lib, "cpu")


@pytest.mark.gpu
def test_sample_record_kernel_gpu(hip_lib):
    _kernel_cases(hip_lib, "cuda")


class _Spy(torch.nn.Module):
    """keeps a copy of what every forward returned (the sampler cannot see through it, so it behaves the same in both runs)"""

    def __init__(self, net):
        super().__init__()
        self.net, self._model_conf, self.outs = net, net._model_conf, []

    def forward(self, feats):
        out = self.net(feats)
        self.outs.append({k: out[k].clone() for k in ("rigids", "psi")})
        return out


def _small_model(dev, blocks=1, seed=3):
    diff = se3_diffuser.SE3Diffuser(dconf())
    m = ScoreNetwork(ts.base_model_conf(blocks), diff)
    m.load_state_dict(fo.synth_params(seed=seed, conf=dict(fo.CONF, num_blocks=blocks)), strict=True)
    return diff, m.to(dev).eval()


def _masked_feats(diff, B, N, dev):
    feats = sampler.init_feats(diff, B, N, dev, generator=torch.Generator(device=dev).manual_seed(1))
    feats["fixed_mask"][B - 1, 2:5] = 1.0          # both terms of trans_traj
    feats["res_mask"][B - 1, N - 3:] = 0.0         # padded rows: zeros in trans_traj, real atoms in prot_traj
    return feats


def _nan_filled_buffers(monkeypatch):
    """every slot the loop does not write stays NaN (slot T of rigid_traj is the starting frames, written at allocation)"""
    orig = sampler._record_buffers

    def filled(aux, T, *a):
        rec = orig(aux, T, *a)
        for k in ("bb_t", "bb_0", "trans_0"):
            if rec[k] is not None:
                rec[k].fill_(float("nan"))
        if rec["rigid_traj"] is not None:
            rec["rigid_traj"][:T].fill_(float("nan"))
        return rec
    monkeypatch.setattr(sampler, "_record_buffers", filled)


def test_record_matches_unrecorded_loop_emu(use_emu, monkeypatch):
    """record="reference" on the interpreter equals, slice by slice, what return_traj=True plus train_step.backbone_atoms give
    for the same injected noise -- with the reference's stale prediction in the final step (train_se3_diffusion.py:778-790)"""
    diff, net = _small_model("cpu")
    B, N, T = 2, 12, 6
    g = torch.Generator().manual_seed(0)
    z = [(torch.randn(B, N, 3, generator=g, dtype=torch.float64), torch.randn(B, N, 3, generator=g, dtype=torch.float64))
         for _ in range(T)]
    kw = dict(num_t=T, noise_fn=lambda i, shp: z[i])
    spy = _Spy(net)
    feats = _masked_feats(diff, B, N, "cpu")
    plain = sampler.sample(spy, diff, feats, return_traj=True, **kw)
    assert sorted(sampler.sample(net, diff, feats, record=None, **kw)) == ["atom37", "psi", "rigids"]      # today's keys
    assert sorted(plain) == ["atom37", "psi", "rigid_traj", "rigids"]
    _nan_filled_buffers(monkeypatch)
    rec = sampler.sample(_Spy(net), diff, feats, record="reference", **kw)
    outs = spy.outs[1:]                                 # (forward 0 is the initial self-conditioning pass)
    assert len(outs) == T and len(plain["rigid_traj"]) == T
    assert rec["prot_traj"].shape == (T, B, N, 37, 3) and rec["rigid_0_traj"].shape == (T, B, N, 37, 3)
    assert rec["rigid_traj"].shape == (T + 1, B, N, 7) and rec["trans_traj"].shape == (T, B, N, 3)
    assert rec["psi_pred"].shape == (1, B, N, 2) and torch.equal(rec["psi_pred"][0], plain["psi"])
    assert torch.equal(rec["rigid_traj"][T], feats["rigids_t"]) and torch.equal(rec["rigids"], plain["rigids"])
    dm = ((1 - feats["fixed_mask"]) * feats["res_mask"])[..., None]
    fm = (feats["fixed_mask"] * feats["res_mask"])[..., None]
    for i in range(T):
        s = T - 1 - i                                   # flipped: index 0 is the final structure
        pred = outs[min(i, T - 2)]["rigids"]            # the final step keeps the previous step's prediction
        frames = plain["rigid_traj"][i]
        assert torch.equal(rec["rigid_traj"][s], frames), i
        assert torch.equal(rec["prot_traj"][s], ts.backbone_atoms(frames, outs[i]["psi"])[0]), i
        assert torch.equal(rec["rigid_0_traj"][s], ts.backbone_atoms(pred, outs[i]["psi"])[0]), i
        assert torch.equal(rec["trans_traj"][s], dm * pred[..., 4:] + fm * frames[..., 4:]), i
    assert torch.equal(rec["rigid_0_traj"][0, ..., 1, :], rec["rigid_0_traj"][1, ..., 1, :])       # CA: stale frames
    assert not torch.equal(rec["rigid_0_traj"][0, ..., 4, :], rec["rigid_0_traj"][1, ..., 4, :])   # O: fresh psi
    assert float(rec["trans_traj"][:, B - 1, N - 3:].abs().max()) == 0.0
    assert float(rec["prot_traj"][:, B - 1, N - 3:, :5].abs().min()) > 0.0
    prot = sampler.sample(_Spy(net), diff, feats, record="prot", **kw)
    assert sorted(prot) == ["atom37", "prot_traj", "psi", "rigids"] and torch.equal(prot["prot_traj"], rec["prot_traj"])
    with pytest.raises(ValueError):
        sampler.sample(net, diff, feats, record="everything", **kw)
    with pytest.raises(ValueError):
        sampler.sample(net, diff, feats, num_t=1, record="reference")


@pytest.mark.gpu
def test_record_graph_matches_eager_gpu(hip_lib, monkeypatch):
    """the captured step with fd_sample_record inside (slot from fd_sample_advance's counter, and from the sampler's own device
    int behind host-issued steps) against the eager loop with the plain integer: the same injected noise, and no slot left
    unwritten or written by the warm-up steps alone (buffers pre-filled with NaN)"""
    from se3_diffusion_amd import options
    dev = "cuda"
    diff, net = _small_model(dev, blocks=2, seed=5)
    B, N, T = 2, 48, 12
    g = torch.Generator().manual_seed(0)
    z = [(torch.randn(B, N, 3, generator=g, dtype=torch.float64), torch.randn(B, N, 3, generator=g, dtype=torch.float64))
         for _ in range(T)]
    feats = _masked_feats(diff, B, N, dev)
    _nan_filled_buffers(monkeypatch)
    res = []
    for dev_steps, graph in ((False, False), (False, True), (True, True)):
        with options.override(sampler_device_steps=dev_steps):
            st = {}
            r = sampler.sample(net, diff, feats, num_t=T, noise_fn=lambda i, shp: z[i], use_graph=graph, record="reference", stats=st)
            assert st["captured"] == graph
            res.append({k: r[k].clone() for k in ("prot_traj", "rigid_traj", "trans_traj", "rigid_0_traj", "psi_pred")})
    for k, v in res[0].items():
        assert bool(torch.isfinite(v).all()), k
        assert torch.equal(res[1][k], res[2][k]), k
        assert float((res[1][k] - v).abs().max()) < 1e-4, k      # eager vs replayed (test_sampler.py's test_device_steps_match_host_steps_gpu holds the frames alone to 1e-5)
    for r in res:
        assert torch.equal(r["rigid_0_traj"][0, ..., 1, :], r["rigid_0_traj"][1, ..., 1, :])


@pytest.mark.gpu
def test_record_adds_one_launch_per_step_gpu(hip_lib):
    """stats["kernels_per_step"] (the library's launches inside one captured step) grows by exactly 1 when recording, and
    record=None leaves the figure of a call without the keyword"""
    dev = "cuda"
    diff = se3_diffuser.SE3Diffuser(dconf())
    m = ScoreNetwork(ts.base_model_conf(4), diff).to(dev).eval()
    n = {}
    for name, kw in (("plain", {}), ("none", dict(record=None)), ("reference", dict(record="reference")), ("prot", dict(record="prot"))):
        st = {}
        feats = sampler.init_feats(diff, 1, 128, dev, generator=torch.Generator(device=dev).manual_seed(1))
        sampler.sample(m, diff, feats, num_t=8, min_t=0.01, noise_scale=0.1, generator=torch.Generator(device=dev).manual_seed(2),
                       use_graph=True, stats=st, **kw)
        n[name] = st["kernels_per_step"]
    print(f"[record] kernels per captured step: {n}")
    assert n["none"] == n["plain"] and n["reference"] == n["plain"] + 1 and n["prot"] == n["plain"] + 1, n


@pytest.mark.gpu
def test_record_memory_is_checked_before_the_loop_gpu(hip_lib, monkeypatch):
    """buffers that do not fit raise an error that names the figure, before anything is run or captured"""
    dev = "cuda"
    diff, net = _small_model(dev)
    feats = sampler.init_feats(diff, 1, 16, dev, generator=torch.Generator(device=dev).manual_seed(1))
    assert sampler.record_bytes(True, 500, 8, 512) == 4 * (500 * 8 * 512 * 40 + 8 * 512 * 7)      # 328 MB
    monkeypatch.setattr(sampler, "record_bytes", lambda *a: 10 ** 15)
    n = hip_lib.cdll.fd_launch_count()
    with pytest.raises(RuntimeError, match="1000000000 MB"):
        sampler.sample(net, diff, feats, num_t=6, use_graph=True, record="reference")
    assert hip_lib.cdll.fd_launch_count() == n
