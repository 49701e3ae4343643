"""Per-residue frame kernels against float64 torch autograd restatements of the reference lines they cite: the backbone update
(fd_bb_update_fwd/_bwd), the score / psi / atom heads (fd_heads_fwd/_bwd), fd_split_rigids, fd_backbone_atoms, the IPA point
and o_pt kernels (fd_ipa_points_fwd/_bwd, fd_ipa_opt_fwd/_bwd/_bwd_dot) and the sequence-transformer row softmax
(fd_row_softmax_fwd/_bwd).  Kernel and reference see the same fp32 inputs (promoted to float64 for the reference); gradients
come from torch.autograd on the float64 graph.

Bounds are per element: |got - ref| <= tol * (|ref| + scale).  `scale` is the magnitude the element's round-off is relative to:
the row's max |ref| (one residue / one softmax row) unless a check names another (the sum of the magnitudes a kernel adds up,
where the result may cancel).  parity_log records max |got - ref| / (|ref| + scale) of every check; each tol is <= 4x the worst
figure measured on the host interpreter and on gfx950 (noted beside it as interpreter / gfx950)."""
import math

import numpy as np
import pytest
import torch

from oracle import framediff_oracle as fo
from se3_diffusion_amd import hip, trunk
from se3_diffusion_amd.ops import lib

import parity_log

F64 = torch.float64
DCONF = (0.1, 0.1, 20.0, 0.1, 1.5, 1000)       # coordinate_scaling, min_b, max_b, min_sigma, max_sigma, L (config/base.yaml)
CSN = 256                                      # c_s: the backbone update's input width
H, C, PQ, PV = 8, 256, 8, 12                   # IPA heads, c_hidden, query / key points, value points
LDP, QP_OFF, KVP_OFF, NQP, NKVP = 6816, 6144, 6336, 64, 160
LDF, F_PT, F_NORM = 2688, 2048, 2336


# --------------------------------------------------------------------------- helpers
def d64(t):
    return t.detach().to("cpu", F64)


def rowmax(ref, rows):
    """per-row max |ref| broadcast back over the row (rows = leading dimension)"""
    r = ref.detach().abs().reshape(rows, -1).amax(1)
    return r.reshape((rows,) + (1,) * (ref.dim() - 1)).expand_as(ref)


def check(key, got, ref, tol, scale=None, floor=None):
    """|got - ref| <= tol (|ref| + scale) elementwise; scale defaults to the row max of |ref|.  Non-finite reference entries
    (the -inf keys of a softmax row) must be matched exactly.  floor: where the float64 reference is itself only known to an
    absolute error (its own round-off), that error is taken off |got - ref| first."""
    got, ref = d64(got), d64(ref)
    assert got.shape == ref.shape, (key, got.shape, ref.shape)
    if scale is None:
        scale = rowmax(ref, ref.shape[0])
    scale = torch.as_tensor(scale, dtype=F64).detach().expand_as(ref).clone()
    fin = torch.isfinite(ref)
    assert torch.equal(torch.isfinite(got), fin), f"{key}: non-finite entries differ"
    assert torch.equal(got[~fin], ref[~fin]), f"{key}: non-finite entries differ"
    err = torch.where(fin, got - ref, torch.zeros_like(ref)).abs()
    if floor is not None:
        err = torch.clamp(err - torch.as_tensor(floor, dtype=F64).detach(), min=0.0)
    den = torch.where(fin, ref.abs() + scale, torch.ones_like(ref))
    fig = torch.where(den > 0, err / den.clamp_min(1e-300), torch.where(err > 0, math.inf, 0.0))
    worst = float(fig.max()) if fig.numel() else 0.0
    parity_log.out(key, worst)
    if worst > tol:
        i = int(fig.reshape(-1).argmax())
        raise AssertionError(f"{key}: max |got-ref|/(|ref|+scale) = {worst:.3e} > {tol:.1e} at flat index {i}: "
                             f"got {float(got.reshape(-1)[i]):.9e} ref {float(ref.reshape(-1)[i]):.9e}")


def unit_quats(g, n):
    q = torch.randn(n, 4, generator=g, dtype=F64)
    return (q / q.norm(dim=-1, keepdim=True)).float()


def grads_by_term(terms, inputs):
    """autograd of each scalar term apart: (sum of the gradients, sum of their row-max magnitudes) per input"""
    tot = [torch.zeros_like(x) for x in inputs]
    cond = [torch.zeros_like(x) for x in inputs]
    for L in terms:
        gs = torch.autograd.grad(L, inputs, retain_graph=True, allow_unused=True)
        for i, gr in enumerate(gs):
            if gr is not None:
                tot[i] = tot[i] + gr
                cond[i] = cond[i] + rowmax(gr, gr.shape[0])
    return tot, cond


def nan_like(shape, dev, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=dev)


# --------------------------------------------------------------------------- fd_split_rigids
TOL_SPLIT = 2.5e-7        # one fp32 rounding (and fp32(0.1) for 0.1): 7.1e-8 / 7.2e-8


def _split(dev, R, B, seed, with_t=True):
    g = torch.Generator().manual_seed(seed)
    rig = torch.randn(R, 7, generator=g) * 10
    t = torch.rand(B, generator=g)
    quat, trans, tsc = nan_like((R, 4), dev), nan_like((R, 3), dev), nan_like((B,), dev)
    lib().call("fd_split_rigids", rig.to(dev), DCONF[0], t.to(dev) if with_t else None, 10000.0, quat, trans,
               tsc if with_t else None, R, B)
    assert torch.equal(quat.cpu(), rig[:, :4])
    # score_network.py:190-193 scale_rigids, :38,43 t * 10000
    check("split_rigids.trans", trans, d64(rig)[:, 4:] * DCONF[0], TOL_SPLIT, scale=0.0)
    if with_t:
        check("split_rigids.tscaled", tsc, d64(t) * 10000.0, TOL_SPLIT, scale=0.0)
    else:
        assert torch.isnan(tsc).all()


# --------------------------------------------------------------------------- fd_row_softmax_fwd / _bwd
TOL_SOFTMAX = 1e-6        # probabilities against the row max: 2.0e-7 / 3.3e-7
TOL_SOFTMAX_BWD = 1.5e-6  # dA against max_j A_j (|dA_j| + |sum_k A_k dA_k|): 1.4e-7 / 4.6e-7


def _softmax(dev, rows, N, rpb, key, seed):
    """key: None, "finite" (a random additive key bias, the training-mode 1 - mask quirk generalised) or "inf" (eval
    tfmr_bool_mask: -inf on padded keys; key 0 stays finite so that no row is empty)"""
    g = torch.Generator().manual_seed(seed)
    S = torch.randn(rows, N, generator=g) * 3
    nb = (rows + rpb - 1) // rpb
    if key is None:
        ka = None
    elif key == "finite":
        ka = torch.randn(nb, N, generator=g) * 2
    else:
        ka = torch.where(torch.rand(nb, N, generator=g) < 0.3, torch.full((nb, N), float("-inf")), torch.zeros(nb, N))
        ka[:, 0] = 0.0
    A = S.to(dev).clone()
    lib().call("fd_row_softmax_fwd", A, None if ka is None else ka.to(dev), rows, N, rpb)
    S64 = d64(S).requires_grad_(True)
    logits = S64 if ka is None else S64 + d64(ka)[torch.arange(rows) // rpb]
    P = torch.softmax(logits, -1)
    check(f"row_softmax.A.N{N}", A, P, TOL_SOFTMAX)
    dA = torch.randn(rows, N, generator=g)
    dk = dA.to(dev).clone()
    lib().call("fd_row_softmax_bwd", A, dk, rows, N)
    (gS,) = torch.autograd.grad((P * d64(dA)).sum(), S64)
    dot = (P * d64(dA)).sum(-1, keepdim=True)
    cond = (P * (d64(dA).abs() + dot.abs())).amax(-1, keepdim=True)
    check(f"row_softmax.dA.N{N}", dk, gS, TOL_SOFTMAX_BWD, scale=cond)


# --------------------------------------------------------------------------- fd_bb_update_fwd / _bwd
TOL_BB_UPD = 1.5e-7       # upd against sum_c |W6_kc x_c| + |b6_k| (cs = 256 products): 2.6e-8 / 4.1e-8
TOL_BB_Q = 4e-7           # quat_out / trans_out: 5.8e-8 / 1.2e-7
TOL_BB_BWD = 6e-6         # dq, dt, dupd, dupd_s against the sum of the term magnitudes: 2.8e-7 / 1.9e-6 (dq: with |u| up to 1e3
#                           the kernel's dn + u x (d dn) cancels inside the dq' term)


def _log_scales(g, R, lo=-4.0, hi=3.0):
    return 10 ** (lo + (hi - lo) * torch.rand(R, generator=g, dtype=F64))


def _bb_fwd(dev, R, seed, pad=0):
    """ipa_pytorch.py:530-557 (upd = Linear(node * diffuse_mask)) then Rigid.compose_q_update_vec (rigid_utils.py:587-616,
    1039-1063); update vectors spread over 1e-4 .. 1e3 through the row scale of the node features; pad > 0: a strided node
    (ldn = cs + pad) whose padding is NaN"""
    g = torch.Generator().manual_seed(seed)
    ldn = CSN + pad
    node = torch.full((R, ldn), float("nan"))
    node[:, :CSN] = (torch.randn(R, CSN, generator=g, dtype=F64) * _log_scales(g, R)[:, None]).float()
    W6 = torch.randn(6, CSN, generator=g) / 16
    b6 = torch.randn(6, generator=g) * 1e-5
    dmask = (torch.rand(R, generator=g) > 0.3).float()
    quat, trans = unit_quats(g, R), torch.randn(R, 3, generator=g) * 10
    upd, q2, t2 = nan_like((R, 6), dev), nan_like((R, 4), dev), nan_like((R, 3), dev)
    lib().call("fd_bb_update_fwd", node.to(dev), ldn, CSN, dmask.to(dev), W6.to(dev), b6.to(dev), quat.to(dev),
               trans.to(dev), upd, q2, t2, R)
    x = d64(node)[:, :CSN] * d64(dmask)[:, None]
    check("bb_update.upd", upd, x @ d64(W6).T + d64(b6), TOL_BB_UPD, scale=x.abs() @ d64(W6).abs().T + d64(b6).abs())
    # the frame update of the kernel's own upd (the stage above is checked against its own condition)
    q_ref, t_ref = fo.backbone_update(d64(quat), d64(trans), d64(upd), d64(dmask))
    check("bb_update.quat_out", q2, q_ref, TOL_BB_Q)
    check("bb_update.trans_out", t2, t_ref, TOL_BB_Q,
          scale=(d64(trans).abs().amax(-1, keepdim=True) + d64(upd)[:, 3:].norm(dim=-1, keepdim=True)).expand(R, 3))


def _bb_bwd(dev, R, seed, with_dframe):
    """autograd of fo.backbone_update w.r.t. (quat, trans, upd); dframe [R,12] = dL/dR(quat) (row-major) | dL/dtrans of the
    INPUT frame, folded through quat_to_rot (rigid_utils.py:173-205)"""
    g = torch.Generator().manual_seed(seed)
    upd = (torch.randn(R, 6, generator=g, dtype=F64) * _log_scales(g, R)[:, None]).float()
    quat = unit_quats(g, R)
    dmask = (torch.rand(R, generator=g) > 0.3).float()
    dq2, dt2 = torch.randn(R, 4, generator=g), torch.randn(R, 3, generator=g)
    dframe = torch.randn(R, 12, generator=g) if with_dframe else None
    dq, dt, du, dus = (nan_like((R, k), dev) for k in (4, 3, 6, 6))
    lib().call("fd_bb_update_bwd", dq2.to(dev), dt2.to(dev), None if dframe is None else dframe.to(dev), dmask.to(dev),
               upd.to(dev), quat.to(dev), dq, dt, du, dus, R)
    q, t, u = d64(quat).requires_grad_(True), torch.zeros(R, 3, dtype=F64, requires_grad=True), d64(upd).requires_grad_(True)
    nq, nt = fo.backbone_update(q, t, u, d64(dmask))
    terms = [(nq * d64(dq2)).sum(), (nt * d64(dt2)).sum()]
    if dframe is not None:
        terms.append((fo.quat_to_rot(q).reshape(R, 9) * d64(dframe)[:, :9]).sum() + (t * d64(dframe)[:, 9:]).sum())
    (gq, gt, gu), (cq, ct, cu) = grads_by_term(terms, (q, t, u))
    tag = "dframe" if with_dframe else "no_dframe"
    check(f"bb_update.dq.{tag}", dq, gq, TOL_BB_BWD, scale=cq)
    check(f"bb_update.dt.{tag}", dt, gt, TOL_BB_BWD, scale=ct)
    check(f"bb_update.dupd.{tag}", du, gu, TOL_BB_BWD, scale=cu)
    dm = d64(dmask)[:, None]
    check(f"bb_update.dupd_s.{tag}", dus, gu * dm, TOL_BB_BWD, scale=cu * dm)


# --------------------------------------------------------------------------- fd_backbone_atoms
TOL_ATOMS = 3e-7          # atom positions against the residue's max |coordinate|: 4.9e-8 / 9.6e-8


def _atoms(dev, R, seed):
    """all_atom.py:152-174 (fo.backbone_atoms); quaternions of norm 1, 0.5 and 2 (Rigid.from_tensor_7 does not normalise)"""
    g = torch.Generator().manual_seed(seed)
    q = unit_quats(g, R) * torch.tensor([1.0, 0.5, 2.0]).repeat(R)[:R, None]
    rig = torch.cat([q, torch.randn(R, 3, generator=g) * 20], -1)
    ang = torch.rand(R, generator=g, dtype=F64) * 2 * math.pi
    psi = torch.stack([torch.sin(ang), torch.cos(ang)], -1).float()
    a37, a14 = nan_like((R, 37, 3), dev), nan_like((R, 14, 3), dev)
    lib().call("fd_backbone_atoms", rig.to(dev), psi.to(dev), trunk.head_const(), a37, a14, R)
    r37, r14 = fo.backbone_atoms(d64(rig)[None, :, :4], d64(rig)[None, :, 4:], d64(psi)[None])
    check("backbone_atoms.atom37", a37, r37[0], TOL_ATOMS)
    check("backbone_atoms.atom14", a14, r14[0], TOL_ATOMS)


# --------------------------------------------------------------------------- fd_ipa_points_fwd / _bwd
TOL_PTS = 7e-7            # global points, dproj, dframe: 1.2e-7 / 2.2e-7


def _ipa_points_ref(proj, Rm, t):
    """ipa_pytorch.py:345-374: raw [x | y | z] blocks -> Rigid.apply (rigid_utils.py:1104) -> q, k, v points"""
    Rn = proj.shape[0]
    qraw = torch.stack(proj[:, QP_OFF:KVP_OFF].split(NQP, -1), -1)                  # [R, 64, 3]
    kvraw = torch.stack(proj[:, KVP_OFF:].split(NKVP, -1), -1)                      # [R, 160, 3]
    qp = fo.rot_apply(Rm[:, None], qraw) + t[:, None]
    kv = (fo.rot_apply(Rm[:, None], kvraw) + t[:, None]).view(Rn, H, PQ + PV, 3)
    return qp.view(Rn, H, PQ, 3), kv[:, :, :PQ], kv[:, :, PQ:]


def _ipa_points(dev, B, N, seed):
    g = torch.Generator().manual_seed(seed)
    R = B * N
    proj = torch.randn(R, LDP, generator=g)
    quat, trans = unit_quats(g, R), torch.randn(R, 3, generator=g) * 10
    qp, kp, kps = nan_like((R, H, PQ, 3), dev), nan_like((R, H, PQ, 3), dev), nan_like((B, H, PQ * 3, N), dev)
    vp = nan_like((R, H, PV, 3), dev)
    lib().call("fd_ipa_points_fwd", proj.to(dev), quat.to(dev), trans.to(dev), qp, kp, vp, kps, N, R, H, C, PQ, PV)
    P64 = d64(proj).requires_grad_(True)
    Rm = fo.quat_to_rot(d64(quat)).requires_grad_(True)
    t = d64(trans).requires_grad_(True)
    rq, rk, rv = _ipa_points_ref(P64, Rm, t)
    for k, got, ref in (("qp", qp, rq), ("kp", kp, rk), ("vp", vp, rv)):
        check(f"ipa_points.{k}", got, ref, TOL_PTS)
    # kp_soa [B, H, 24, N]: the key points again, key index innermost
    assert torch.equal(kps.cpu(), kp.cpu().view(B, N, H, PQ * 3).permute(0, 2, 3, 1))
    # backward: dframe starts non-zero (the kernel accumulates); dproj outside the point columns is not touched
    dqp, dkp, dvp = torch.randn(R, H, PQ, 3, generator=g), torch.randn(R, H, PQ, 3, generator=g), torch.randn(R, H, PV, 3, generator=g)
    dproj0, dframe0 = torch.randn(R, LDP, generator=g), torch.randn(R, 12, generator=g)
    dproj, dframe = dproj0.clone().to(dev), dframe0.clone().to(dev)
    lib().call("fd_ipa_points_bwd", proj.to(dev), quat.to(dev), dqp.to(dev), dkp.to(dev), dvp.to(dev), dproj, dframe, R, H, C,
               PQ, PV)
    L = (rq * d64(dqp)).sum() + (rk * d64(dkp)).sum() + (rv * d64(dvp)).sum()
    gP, gR, gt = torch.autograd.grad(L, (P64, Rm, t))
    assert torch.equal(dproj.cpu()[:, :QP_OFF], dproj0[:, :QP_OFF])
    check("ipa_points.dproj", dproj[:, QP_OFF:], gP[:, QP_OFF:], TOL_PTS)
    check("ipa_points.dframe", dframe, d64(dframe0) + torch.cat([gR.reshape(R, 9), gt], -1), TOL_PTS)


# --------------------------------------------------------------------------- fd_ipa_opt_fwd / _bwd / _bwd_dot
TOL_OPT = 1e-6            # o_pt, |o_pt|, doptg, dframe, ptdot: 2.4e-7 / 3.4e-7


def _opt_ref(optg, Rm, t):
    """ipa_pytorch.py:432-449: o_pt = invert_apply(sum_j a v_pts) (rigid_utils.py:1118-1130), |o_pt| = sqrt(sum o^2 + 1e-8)"""
    loc = fo.rot_apply(Rm.transpose(-1, -2)[:, None], optg - t[:, None])          # [R, 96, 3]
    return loc, torch.sqrt((loc ** 2).sum(-1) + 1e-8)


def _ipa_opt(dev, R, seed):
    g = torch.Generator().manual_seed(seed)
    quat, trans = unit_quats(g, R), torch.randn(R, 3, generator=g) * 10
    optg = (trans[:, None] + torch.randn(R, H * PV, 3, generator=g) * 5).contiguous()
    optg[0, 0] = trans[0]                                                          # |o_pt| ~ 1e-4: the 1e-8 of the norm matters
    feats0 = torch.randn(R, LDF, generator=g)
    feats = feats0.clone().to(dev)
    lib().call("fd_ipa_opt_fwd", optg.to(dev), quat.to(dev), trans.to(dev), feats, R)
    Og = d64(optg).requires_grad_(True)
    Rm = fo.quat_to_rot(d64(quat)).requires_grad_(True)
    t = d64(trans).requires_grad_(True)
    loc, nrm = _opt_ref(Og, Rm, t)
    fc = feats.cpu()
    assert torch.equal(fc[:, :F_PT], feats0[:, :F_PT]) and torch.equal(fc[:, F_NORM + H * PV:], feats0[:, F_NORM + H * PV:])
    check("ipa_opt.o_pt", fc[:, F_PT:F_NORM].view(R, 3, H * PV).transpose(1, 2), loc, TOL_OPT)
    check("ipa_opt.o_norm", fc[:, F_NORM:F_NORM + H * PV], nrm, TOL_OPT)
    dfeats = torch.randn(R, LDF, generator=g)
    df = d64(dfeats)
    L = (loc * df[:, F_PT:F_NORM].view(R, 3, H * PV).transpose(1, 2)).sum() + (nrm * df[:, F_NORM:F_NORM + H * PV]).sum()
    gO, gR, gt = torch.autograd.grad(L, (Og, Rm, t))
    dframe0 = torch.randn(R, 12, generator=g)
    for dot in (False, True):
        doptg, dframe, ptdot = nan_like((R, H * PV, 3), dev), dframe0.clone().to(dev), nan_like((R, H), dev)
        if dot:
            lib().call("fd_ipa_opt_bwd_dot", dfeats.to(dev), feats, quat.to(dev), trans.to(dev), doptg, dframe, ptdot, R)
        else:
            lib().call("fd_ipa_opt_bwd", dfeats.to(dev), feats, quat.to(dev), doptg, dframe, R)
        check("ipa_opt.doptg", doptg, gO, TOL_OPT)
        check("ipa_opt.dframe", dframe, d64(dframe0) + torch.cat([gR.reshape(R, 9), gt], -1), TOL_OPT)
        if dot:
            # sum_p d(o_pt global) . (o_pt global) per head (the o_pt term of the softmax backward's row constant)
            prod = (gO * d64(optg)).sum(-1).view(R, H, PV)
            check("ipa_opt.ptdot", ptdot, prod.sum(-1), TOL_OPT, scale=rowmax(prod.abs().sum(-1), R))


# --------------------------------------------------------------------------- fd_heads_fwd / _bwd
TOL_HEADS = 1.5e-6        # rot_score, trans_score, rigids, psi, atom37, atom14: 1.6e-7 / 4.6e-7
TOL_HEADS_BWD = 2.5e-6    # dquatF, dtransF, dupsi against the sum of the incoming gradients' contributions: 1.9e-7 / 8.2e-7
# quat_to_rotvec's branch threshold as the fp32 reference (and the kernel) compares it.  The rows below stay 8 fp32 ulps clear
# of it: between 1e-3 and fp32(1e-3) the fp32 reference and a float64 restatement take different branches, and the branches
# differ by the 1e-6 inside the large-angle sine (2e-3 of the rotation vector at 1e-3)
F32_1E3 = float(np.float32(1e-3))
ULP_1E3 = float(np.spacing(np.float32(1e-3)))


def _axis_q(ang, axis=(1.0, 0.0, 0.0)):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    return [math.cos(ang / 2)] + list(math.sin(ang / 2) * a)


def _head_rows(g, B, N):
    """(q0, qF, exact): pairs whose relative rotation inv(qF) (x) q0 fp32 forms without rounding (qF a signed unit axis, or
    identity) at the places quat_to_rotvec branches or loses precision; random pairs fill each backbone"""
    I = [1.0, 0.0, 0.0, 0.0]
    special = [
        (I, I),                                                  # relative angle exactly 0
        ([0.0, 1.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0]),            # ... with a non-trivial frame
        (_axis_q(F32_1E3 - 8 * ULP_1E3), I),                     # a few ulps below / above the small-angle branch
        (_axis_q(F32_1E3 + 8 * ULP_1E3, (0, 1, 0)), I),
        (_axis_q(5e-4, (1, 2, 3)), I),                           # inside the small-angle series
        (_axis_q(1e-2, (0, 0, 1)), I),
        (_axis_q(math.pi - 1e-3, (3, -1, 2)), I),                # near 180 degrees
        (_axis_q(math.pi - 1e-2, (1, 1, 0)), I),
        ([0.0, 1.0, 0.0, 0.0], I),                               # pw exactly 0 in fp32 (180 degrees)
        ([0.0, 0.0, 0.6, 0.8], [0.0, 0.0, 0.0, 1.0]),            # pw exactly 0, qF not identity
        ([-v for v in _axis_q(1.0, (1, -2, 1))], I),             # pw < 0: the sign flip
        ([-v for v in _axis_q(2.0, (0, 1, 1))], [0.0, 1.0, 0.0, 0.0]),
        (_axis_q(0.7, (2, 1, 0)), [0.5, 0.0, 0.0, 0.0]),         # |qF| = 0.5 and 2
        (_axis_q(2.2, (1, 0, 1)), [0.0, 0.0, -2.0, 0.0]),
    ]
    ns = len(special)
    assert N >= ns
    q0 = torch.empty(B * N, 4, dtype=F64)
    qF = torch.empty(B * N, 4, dtype=F64)
    exact = torch.zeros(B * N, dtype=torch.bool)
    for b in range(B):
        r = b * N
        for k, (a, f) in enumerate(special):
            q0[r + k], qF[r + k] = torch.tensor(a, dtype=F64), torch.tensor(f, dtype=F64)
        exact[r:r + ns] = True
        q0[r + ns:r + N] = d64(unit_quats(g, N - ns))
        qF[r + ns:r + N] = d64(unit_quats(g, N - ns)) * (0.5 + 1.5 * torch.rand(N - ns, 1, generator=g, dtype=F64))
    return q0.float(), qF.float(), exact


def _heads_inputs(g, B, N, ts):
    R = B * N
    q0, qF, exact = _head_rows(g, B, N)
    rig0 = torch.cat([q0, torch.randn(R, 3, generator=g) * 10], -1)
    transF = torch.randn(R, 3, generator=g)                                  # nm
    u = torch.randn(R, 2, generator=g)
    u[5::7] = torch.tensor([3e-5, -4e-5])                                    # |u|^2 = 2.5e-9 < 1e-8: the psi clamp
    gt = torch.randn(R, 14, generator=g)
    fixed = (torch.rand(R, generator=g) < 0.2).float()
    mask = (torch.rand(R, generator=g) > 0.15).float()
    t = torch.tensor(ts, dtype=torch.float32)
    return dict(rig0=rig0, qF=qF, transF=transF, u=u, gt=gt, fixed=fixed, mask=mask, t=t, exact=exact)


def _cached_table(sg):
    """a cached score table [num_sigma, num_omega] on discrete_omega = linspace(0, pi, 1001)[1:] (so3_diffuser.py:131-180);
    the lookup semantics are what is checked, so the entries are a cheap smooth stand-in: -omega / sigma^2 (1 + 0.1 sin 7w)"""
    om = torch.linspace(0, math.pi, 1001, dtype=F64)[1:]
    tab = -om[None] / sg[:, None] ** 2 * (1 + 0.1 * torch.sin(7 * om[None]))
    return tab, om


def _heads_consts(dev, cached):
    hc0, sg = trunk.head_tables(DCONF, torch.device(dev))
    if not cached:
        return hc0, sg, None
    tab, om = _cached_table(d64(sg))
    tab_d, om_d = tab.to(dev), om.to(dev)
    hc = hip.FdHeadConst()
    for name, _ in hip.FdHeadConst._fields_:
        setattr(hc, name, getattr(hc0, name))
    hc.score_norms, hc.omega_grid, hc.n_omega = tab_d.data_ptr(), om_d.data_ptr(), om_d.numel()
    hc._tables = (tab_d, om_d)
    return hc, sg, (tab, om)


def _igso3_series64(omega, sig, L=1000):
    """f, f' of so3_diffuser.py:9-117 in float64 (fo.igso3_series) and the magnitude of the terms they sum.  Below omega =
    1e-2 the same sums in the Dirichlet-kernel form sin((l+1/2)w)/sin(w/2) = 1 + 2 sum_{k<=l} cos(kw): the quotient rule's
    numerator cancels to O(w^3) there, and at the omega = 1e-6 of an identity relative rotation fo.igso3_series is 3.2e-5
    off f'/(f + 1e-4) (against a 40-digit evaluation), the Dirichlet form 1e-15."""
    f, df = fo.igso3_series(omega, sig, L)
    ls = torch.arange(L, dtype=F64)
    om, sg = omega[:, None], sig[:, None]
    w = (2 * ls + 1) * torch.exp(-ls * (ls + 1) * sg ** 2 / 2)
    k = ls[1:]
    ratio = torch.cat([torch.ones_like(om), 1 + 2 * torch.cumsum(torch.cos(k * om), -1)], -1)
    dratio = torch.cat([torch.zeros_like(om), -2 * torch.cumsum(k * torch.sin(k * om), -1)], -1)
    small = omega < 1e-2
    f = torch.where(small, (w * ratio).sum(-1), f)
    df = torch.where(small, (w * dratio).sum(-1), df)
    with torch.no_grad():
        lh = ls + 0.5
        lo, dlo = torch.sin(om / 2), 0.5 * torch.cos(om / 2)
        big = (w * ((lo * lh).abs() + dlo.abs()) / lo ** 2 * (1 + lh * om)).sum(-1)     # sin / cos of (l+1/2) w: (l+1/2) w ulps
        sm = (w * (ls + 1) ** 3).sum(-1)
        mag = torch.where(small, sm, big)
    return f, df, mag


def _heads_ref(x, P, cached, shift=None):
    """ipa_pytorch.py:650-672 in float64: calc_rot_score (se3_diffuser.py:119-125 -> data/utils.py:582-599 ->
    so3_diffuser.py:274-305, the IGSO(3) series of so3_diffuser.py:9-117 or the cached-table lookup), calc_trans_score
    (r3_diffuser.py:148-166), the psi head's normalisation (ipa_pytorch.py:491-507, score_network.py:201-203) and the
    backbone atoms (all_atom.py:152-174).  P: the float64 leaves (qF, transF, u)."""
    R = P["qF"].shape[0]
    N = R // x["t"].numel()
    b = torch.arange(R) // N
    t = d64(x["t"])[b]
    m, fm = d64(x["mask"]), d64(x["fixed"])
    q0 = d64(x["rig0"])[:, :4]
    v = fo.quat_to_rotvec(fo.quat_multiply(fo.invert_quat(P["qF"]), q0))
    omega = torch.linalg.norm(v, dim=-1) + 1e-6
    idx = fo.so3_t_to_idx(t.numpy())
    if cached is None:
        sig = torch.tensor(fo.so3_discrete_sigma()[idx])
        f, df, mag = _igso3_series64(omega, sig)
        gs = df / (f + 1e-4)
        # the series' own round-off, 2^-52 of its terms' magnitudes
        noise = (2.0 ** -52 * mag / (f + 1e-4) * torch.linalg.norm(v, dim=-1) / (omega + 1e-6)).detach()
        (dg,) = torch.autograd.grad(gs.sum(), omega, retain_graph=True)
        alt = torch.zeros(R, dtype=torch.long)
    else:
        tab, om = cached
        edges = om[:-1]
        bk = torch.bucketize(omega.detach(), edges)
        # omega within 1e-6 of a bucket edge: the kernel's omega (which carries the fp32 rounding of inv(qF) (x) q0) may take
        # the neighbouring table entry; alt names it
        below = (bk > 0) & (omega.detach() - edges[(bk - 1).clamp(min=0)] < 1e-6)
        above = (bk < edges.numel()) & (edges[bk.clamp(max=edges.numel() - 1)] - omega.detach() < 1e-6)
        alt = torch.where(below, -1, torch.where(above, 1, 0))
        if shift is not None:
            bk = (bk + shift).clamp(0, om.numel() - 1)
        gs = tab[torch.tensor(idx), bk]                                            # a constant for autograd
        noise = torch.zeros(R, dtype=F64)
        dg = torch.zeros(R, dtype=F64)
    rot = gs[:, None] * v / (omega[:, None] + 1e-6) * m[:, None]
    ta = P["transF"] / DCONF[0]                                                    # unscale_rigids
    ts = fo.calc_trans_score(d64(x["rig0"])[:, 4:], ta, t[:, None]) * m[:, None]
    rig = torch.cat([P["qF"], ta], -1)
    un = P["u"] / torch.sqrt(torch.clamp((P["u"] ** 2).sum(-1, keepdim=True), min=1e-8))
    psi = (1 - fm[:, None]) * un + fm[:, None] * d64(x["gt"])[:, 4:6]
    a37, a14 = fo.backbone_atoms(P["qF"][None], ta[None], psi[None])
    return dict(rot_score=rot, trans_score=ts, rigids=rig, psi=psi, atom37=a37[0], atom14=a14[0], gs=gs, omega=omega, v=v,
                un=un, noise=noise * m, dg=dg.detach(), alt=alt)


def _heads(dev, B, N, ts, seed, cached=False):
    g = torch.Generator().manual_seed(seed)
    x = _heads_inputs(g, B, N, ts)
    R = B * N
    hc, sg, tabs = _heads_consts(dev, cached)
    xd = {k: v.to(dev) for k, v in x.items() if k != "exact"}
    rot = nan_like((R, 3), dev, F64)
    tsc, rig, psi, a37, a14, sca = (nan_like((R, k), dev) for k in (3, 7, 2, 111, 42, 3))
    lib().call("fd_heads_fwd", xd["rig0"], xd["qF"], xd["transF"], xd["u"], (xd["gt"], 4), 14, xd["fixed"], xd["mask"], xd["t"],
               sg, sg.numel(), hc, rot, tsc, rig, psi, a37, a14, sca, B, N)
    P = {k: d64(x[k]).requires_grad_(True) for k in ("qF", "transF", "u")}
    ref = _heads_ref(x, P, tabs)
    tag = "cached" if cached else "series"
    if cached and bool((ref["alt"] != 0).any()):
        # a table step: rows whose omega sits within 1e-6 of a bucket edge are compared with the entry the kernel took
        ref2 = _heads_ref(x, P, tabs, shift=ref["alt"])
        d1 = (d64(rot) - ref["rot_score"].detach()).abs().amax(-1)
        d2 = (d64(rot) - ref2["rot_score"].detach()).abs().amax(-1)
        ref = _heads_ref(x, P, tabs, shift=torch.where((ref["alt"] != 0) & (d2 < d1), ref["alt"], 0))
    # rot_score: rows whose relative rotation fp32 forms exactly are checked against their own magnitude.  For the random
    # pairs inv(qF) (x) q0 carries fp32 rounding of ~1e-7 absolute into v (the reference's own fp32 arithmetic, kept by the
    # kernel); where the relative rotation is tiny, or near 180 degrees where g -> 0, that is far above the row's magnitude,
    # and the scale there is the score's sensitivity to v: |g| / (omega + eps) + |g'(omega)|.  At small sigma
    # and large omega the float64 series sums terms of size ~ sum_l (2l+1)^2 w_l and cancels to f' ~ exp(-omega^2 / 2 sigma^2):
    # there the reference is its own round-off (2.0e-8 where the kernel gives -3.3e-11, t = 1e-3, a random pair), and 8x
    # that estimate is the floor.
    sens = ((ref["gs"].abs() / (ref["omega"] + 1e-6) + ref["dg"].abs()) * d64(x["mask"])).detach()[:, None].expand(R, 3)
    rm = rowmax(ref["rot_score"], R)
    sc = torch.where(x["exact"][:, None], rm, torch.maximum(rm, sens))
    check(f"heads.rot_score.{tag}", rot, ref["rot_score"], TOL_HEADS, scale=sc, floor=8 * ref["noise"][:, None].expand(R, 3))
    check(f"heads.trans_score.{tag}", tsc, ref["trans_score"], TOL_HEADS)
    check(f"heads.rigids.{tag}", rig, ref["rigids"], TOL_HEADS)
    check(f"heads.psi.{tag}", psi, ref["psi"], TOL_HEADS)
    check(f"heads.atom37.{tag}", a37.view(R, 37, 3), ref["atom37"], TOL_HEADS)
    check(f"heads.atom14.{tag}", a14.view(R, 14, 3), ref["atom14"], TOL_HEADS)
    assert torch.equal(sca.cpu(), rig.cpu()[:, 4:])
    # backward: every incoming gradient, then each one absent in turn
    dks = ("rot_score", "trans_score", "rigids", "psi", "atom37")
    gin = {"rot_score": torch.randn(R, 3, generator=g, dtype=F64), "trans_score": torch.randn(R, 3, generator=g),
           "rigids": torch.randn(R, 7, generator=g), "psi": torch.randn(R, 2, generator=g),
           "atom37": torch.randn(R, 37, 3, generator=g)}
    leaves = (P["qF"], P["transF"], P["u"], ref["un"])
    per = {}
    for k in dks:
        gs_ = torch.autograd.grad((ref[k] * d64(gin[k])).sum(), leaves, retain_graph=True, allow_unused=True)
        per[k] = [torch.zeros_like(l) if gr is None else gr for l, gr in zip(leaves, gs_)]
        # dupsi = (g - p (p . g)) / |u| removes the radial part of g = dL/d(u / |u|): its round-off is relative to |g| / |u|
        den = torch.sqrt(torch.clamp((d64(x["u"]) ** 2).sum(-1, keepdim=True), min=1e-8))
        per[k][3] = per[k][3] * (1 - d64(x["fixed"]))[:, None] / den
    # dquatF of the random pairs: inv(qF) (x) q0 is formed in fp32 (see rot_score), and the float64 gradient moves by
    # |d grad / d p| x that rounding -- 4x its spread over two random relative perturbations of q0 of 2^-23 is the floor there
    spread = torch.zeros(R, 4, dtype=F64)
    for k in range(2):
        q0p = d64(x["rig0"]).clone()
        q0p[:, :4] *= 1 + 2.0 ** -23 * (2 * torch.rand(R, 4, generator=g, dtype=F64) - 1)
        P2 = {kk: d64(x[kk]).requires_grad_(True) for kk in ("qF", "transF", "u")}
        r2 = _heads_ref(dict(x, rig0=q0p), P2, tabs)
        (g2,) = torch.autograd.grad((r2["rot_score"] * gin["rot_score"]).sum(), P2["qF"])
        spread = torch.maximum(spread, (g2 - per["rot_score"][0]).abs())
    dq_floor = torch.where(x["exact"][:, None], 0.0, 4 * rowmax(spread, R))
    for drop in (None,) + dks:
        use = [k for k in dks if k != drop]
        dq, dt, du = nan_like((R, 4), dev), nan_like((R, 3), dev), nan_like((R, 2), dev)
        a = {k: (None if k == drop else gin[k].to(dev).reshape(R, -1)) for k in dks}
        lib().call("fd_heads_bwd", xd["rig0"], xd["qF"], xd["transF"], xd["u"], psi, xd["fixed"], xd["mask"], xd["t"], sg,
                   sg.numel(), hc, a["rot_score"], a["trans_score"], a["rigids"], a["psi"], a["atom37"], dq, dt, du, B, N)
        for i, (name, got) in enumerate((("dquatF", dq), ("dtransF", dt), ("dupsi", du))):
            refg = sum(per[k][i] for k in use)
            cond = sum(rowmax(per[k][i], R) + (rowmax(per[k][3], R) if name == "dupsi" else 0) for k in use)
            check(f"heads.{name}.{tag}", got, refg, TOL_HEADS_BWD, scale=cond,
                  floor=dq_floor if (name == "dquatF" and drop != "rot_score") else None)


# --------------------------------------------------------------------------- interpreter tier
def test_split_rigids_emu(use_emu):
    with parity_log.case("frames.split_rigids_emu"):
        _split("cpu", R=1, B=1, seed=0)
        _split("cpu", R=300, B=3, seed=1)              # not a multiple of 256 threads
        _split("cpu", R=37, B=2, seed=2, with_t=False)


def test_row_softmax_emu(use_emu):
    with parity_log.case("frames.row_softmax_emu"):
        for i, N in enumerate((1, 37, 64, 65, 300, 512)):
            _softmax("cpu", rows=9, N=N, rpb=3, key=(None, "finite", "inf")[i % 3], seed=i)
            _softmax("cpu", rows=5, N=N, rpb=5, key=("inf", None, "finite")[i % 3], seed=10 + i)
        _softmax("cpu", rows=1, N=65, rpb=1, key="finite", seed=20)


def test_bb_update_emu(use_emu):
    with parity_log.case("frames.bb_update_emu"):
        _bb_fwd("cpu", R=1, seed=0)
        _bb_fwd("cpu", R=37, seed=1)                   # not a multiple of the 4 rows per block
        _bb_fwd("cpu", R=22, seed=2, pad=40)           # strided node, ldn > cs
        for s, R in enumerate((1, 37, 300)):
            _bb_bwd("cpu", R=R, seed=10 + s, with_dframe=False)
            _bb_bwd("cpu", R=R, seed=20 + s, with_dframe=True)


def test_backbone_atoms_emu(use_emu):
    with parity_log.case("frames.backbone_atoms_emu"):
        _atoms("cpu", R=1, seed=0)
        _atoms("cpu", R=301, seed=1)


def test_ipa_points_emu(use_emu):
    with parity_log.case("frames.ipa_points_emu"):
        _ipa_points("cpu", B=1, N=1, seed=0)
        _ipa_points("cpu", B=3, N=13, seed=1)          # several backbones in kp_soa


def test_ipa_opt_emu(use_emu):
    with parity_log.case("frames.ipa_opt_emu"):
        _ipa_opt("cpu", R=1, seed=0)
        _ipa_opt("cpu", R=37, seed=1)


@pytest.mark.parametrize("cached", [False, True])
def test_heads_emu(use_emu, cached):
    with parity_log.case(f"frames.heads_emu.{'cached' if cached else 'series'}"):
        _heads("cpu", B=5, N=24, ts=(0.01, 0.05, 0.3, 1.0, 1e-3), seed=3, cached=cached)
        _heads("cpu", B=1, N=14, ts=(0.5,), seed=4, cached=cached)


# --------------------------------------------------------------------------- GPU tier
# Row counts above each launcher's grid cap make every block walk more than one row: fd_split_rigids 1024 blocks x 256 rows,
# fd_bb_update_fwd 8192 x 4, fd_row_softmax_fwd / _bwd 16384 x 4 (fd_frames.hip, the launchers).
@pytest.mark.gpu
def test_split_rigids_gpu(hip_lib):
    with parity_log.case("frames.split_rigids_gpu"):
        _split("cuda", R=1, B=1, seed=0)
        _split("cuda", R=30 * 128, B=30, seed=1)
        _split("cuda", R=300_001, B=30, seed=2)


@pytest.mark.gpu
def test_row_softmax_gpu(hip_lib):
    with parity_log.case("frames.row_softmax_gpu"):
        for i, N in enumerate((1, 37, 64, 65, 300, 512)):
            _softmax("cuda", rows=4 * N + 3, N=N, rpb=N, key=(None, "finite", "inf")[i % 3], seed=i)
            _softmax("cuda", rows=4 * 2 * N, N=N, rpb=4 * N, key=("inf", None, "finite")[i % 3], seed=10 + i)
        _softmax("cuda", rows=70_001, N=65, rpb=4 * 65, key="inf", seed=20)
        _softmax("cuda", rows=66_000, N=37, rpb=4 * 37, key="finite", seed=21)


@pytest.mark.gpu
def test_bb_update_gpu(hip_lib):
    with parity_log.case("frames.bb_update_gpu"):
        _bb_fwd("cuda", R=1, seed=0)
        _bb_fwd("cuda", R=30 * 128, seed=1)
        _bb_fwd("cuda", R=40_003, seed=2, pad=40)
        for s, R in enumerate((1, 30 * 128, 40_003)):
            _bb_bwd("cuda", R=R, seed=10 + s, with_dframe=False)
            _bb_bwd("cuda", R=R, seed=20 + s, with_dframe=True)


@pytest.mark.gpu
def test_backbone_atoms_gpu(hip_lib):
    with parity_log.case("frames.backbone_atoms_gpu"):
        _atoms("cuda", R=1, seed=0)
        _atoms("cuda", R=30 * 128 + 1, seed=1)


@pytest.mark.gpu
def test_ipa_points_gpu(hip_lib):
    with parity_log.case("frames.ipa_points_gpu"):
        _ipa_points("cuda", B=1, N=1, seed=0)
        _ipa_points("cuda", B=30, N=128, seed=1)


@pytest.mark.gpu
def test_ipa_opt_gpu(hip_lib):
    with parity_log.case("frames.ipa_opt_gpu"):
        _ipa_opt("cuda", R=1, seed=0)
        _ipa_opt("cuda", R=30 * 128, seed=1)


@pytest.mark.gpu
@pytest.mark.parametrize("cached", [False, True])
def test_heads_gpu(hip_lib, cached):
    with parity_log.case(f"frames.heads_gpu.{'cached' if cached else 'series'}"):
        _heads("cuda", B=1, N=14, ts=(0.5,), seed=4, cached=cached)
        ts = tuple(float(v) for v in np.concatenate([[0.01, 0.05, 1.0, 1e-3], np.linspace(0.02, 0.98, 26)]))
        _heads("cuda", B=30, N=128, ts=ts, seed=5, cached=cached)
