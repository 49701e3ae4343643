"""The three stages of a trunk block that tests/test_stages.py leaves out, and the heads, against float64 autograd -- the same
machinery (Reference, Gates, _compare: error = max |got - ref| / max |ref| per tensor, bound of a case = min(8 max_k e32_k, 2e-5)
with e32 the same restatement in float32 torch; nothing is derived from what the code under test gives).

  ipa        network.ipa_fwd -> ipa_bwd -> ops.flush_dw / join_grad_stream against model/ipa_pytorch.py:303-471 restated here
             (`_ipa_fn`, asserted equal to fo.ipa to 1e-12): x1 = s + mask IPA(s, z, R, t, mask), the rotation as a leaf
             Rm = quat_to_rot(quat) beside trans, so that dframe [R, 12] = dL/dRm (row-major) | dL/dtrans (the convention of
             test_frames._bb_bwd), the mask literally 1e5 (m_i m_j - 1).  x1, ds and dframe over random initial values, dz
             assigned over NaN / accumulated / deferred as (dzb, W40) with the buffer still NaN, the 15 parameter gradients.
             Layouts: scattered (separate tensors: four projection GEMMs, packed W40, dW40[:H] / dW40[H:]) and flat (parameters
             and gradients back to back in the order of ScoreNetwork.flat_layout_groups(): merged GEMM, W40 a view, one dW
             launch, adjacent gW / gb).  Launch paths through options.override, each asserted through the deltas of ops.STATS:
             the fused sequence, fused_ipa_attn=False, flash forward + backward with the key side, the same with
             flash_ipa_keys=False.  zb = None or handed in as F.linear(z, W40, b40) of float32 torch.  head_weights of
             test_ipa_bwd.HW_EDGES in one case.  Forward only (save=False): the cache (one merged Wproj GEMM, a second call
             bit-identical), out_view into columns 320..575 of a NaN-filled [R, 640] buffer, the key-split kernel.
             linear_b.bias: its gradient is analytically zero (a per-head constant added to every logit of a row: softmax shift
             invariance), so a relative measure means nothing; it is held to 8 x 2^-24 x max_h sum |dzb_ref[..., h]| absolute,
             dzb_ref the float64 gradient of z W40^T + b40.
  bb_update  trunk.bb_update_fwd -> bb_update_bwd(dframe=None) -> _frame_grad_fold(dframe), as trunk._backward runs them, against
             upd = Linear(n3 * dmask), fo.backbone_update and <quat_to_rot(quat), dframe[:, :9]> + <trans, dframe[:, 9:]>:
             q2, t2, dn3 over a random initial value, dq, dt, the two parameter gradients.  dmask: zeros for fixed and padded
             residues, ones elsewhere, one example all zero -- and a second case with fractional entries: with 0 / 1 entries
             dupd * dmask = dupd exactly, so only a fractional entry tells the bias gradient's operand (dupd) from the weight
             gradient's (dupd_s); the restatement is defined for any dmask.
  heads      trunk.heads_fwd -> heads_bwd against the torsion MLP restated here (linear_1 + ReLU through Gates, linear_2 +
             residual, linear_final) in front of test_frames._heads_ref: the six outputs, dnode over a random initial value, dq,
             dt, the six torsion_pred gradients, with d_out = all five entries / the four the loss uses / psi alone (a missing
             entry is absent from the reference's loss: it must contribute nothing).
             Bounds: what passes through the MLP glue -- u (the operand the forward hands fd_heads_fwd), dnode and the six
             gradients -- takes the 8 e32 rule.  The direct outputs of fd_heads_fwd / _bwd (the six outputs, dq, dt) keep
             test_frames' element-wise bounds TOL_HEADS / TOL_HEADS_BWD with its scales and floors (a float32 IGSO(3) series is
             no noise floor), against test_frames._heads_ref at the stage's own u: those bounds are for a kernel and a reference
             that see the same float32 inputs, as in test_frames; psi, the atoms and dq would otherwise carry the MLP's float32
             noise divided by |u|, which is u's check, not theirs.

Achieved (worst tensor of the worst case of a tier; `parity_log` keys ipa.* / bb_update.* / heads.*, gradients by family):

  stage             interpreter                                     MI355X
  ipa               x1 3.4e-7  ds 7.0e-7  dframe 5.2e-7  dz 6.4e-7   x1 3.1e-7  ds 2.8e-7  dframe 9.3e-7  dz 7.6e-7
                    gradients: ipa.proj 8.8e-7, ipa.pair_proj 6.7e-7, head_weights 1.3e-6 | 8.1e-7, 9.5e-7, 1.6e-6
                    bounds 7.3e-6 | 4.7e-6 (N = 37), 8.5e-6 (N = 130)
    HW_EDGES        x1 4.8e-7  ds 3.2e-6  dframe 7.5e-6  dz 3.7e-7   x1 3.1e-6  ds 4.5e-6  dframe 7.2e-6  dz 1.2e-6
                    gradients: ipa.proj 1.1e-5 (linear_q_points.bias, flash path), ipa.pair_proj 6.8e-7, head_weights 2.6e-6
                    | 6.3e-6, 2.5e-6, 4.5e-6                         bounds 2e-5 | 2e-5: the cap (8 e32 = 3.3e-5 | 5.9e-5)
    linear_b.bias   absolute 4.6e-6 of 1.6e-5 ... 1.8e-5             absolute 1.4e-5 of 1.6e-4 (N = 130), 6.1e-6 of 8.7e-5 (N = 37; its
                                                                     last bits vary from run to run: a column sum by float atomics)
    sampling forms  x1 3.2e-7 (bounds 1.8e-6 ... 2.7e-6)             x1 2.8e-7 (bound 1.5e-6)
  bb_update         q2 9.4e-8  t2 3.2e-8  dn3 3.2e-8  dq 1.0e-7      q2 1.2e-7  t2 3.5e-8  dn3 4.3e-8  dq 1.2e-7
                    dt 4.0e-8  gradients 1.5e-7                      dt 5.0e-8  gradients 3.3e-7
                    bounds 9.4e-7 ... 1.1e-6 | 1.3e-6 ... 2.6e-6
  heads (8 e32)     u 1.5e-7  dnode 2.6e-7  gradients 8.8e-7         u 2.4e-7  dnode 5.7e-7  gradients 1.9e-6
                    bounds 1.7e-5 ... 2e-5 (8 e32 up to 2.2e-5) | 2e-5, the cap (8 e32 = 3.4e-5 ... 7.5e-5: the 1 / |u| of the psi head)
    direct          psi 4.6e-8  rot_score 1.7e-7  trans_score 4.7e-8    psi 5.2e-8  rot_score 4.4e-7  trans_score 1.2e-7
    (test_frames'   rigids 2.2e-8  atom37, atom14 4.0e-8             rigids 3.7e-8  atom37, atom14 5.4e-8
     measure)       dq 1.3e-7  dt 5.4e-8                             dq 9.6e-8  dt 6.6e-8     (TOL_HEADS 1.5e-6, TOL_HEADS_BWD 2.5e-6)
  Only the HW_EDGES cases of ipa and the heads' MLP tensors reach the 2e-5 cap; every other bound is 8 x the float32 noise of its case.
"""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import parity_log
import test_frames as tf
from oracle import framediff_oracle as fo
from se3_diffusion_amd import network as nw, ops, options, trunk
from test_ipa_bwd import HW_EDGES
from test_embed_feats import NAN, relerr
from test_stages import Gates, Reference, T, _compare, _finish, _params, _w40, _zeros_like

H, C, PQ, PV = 8, 256, 8, 12


# ------------------------------------------------------------------------------------------------ ipa
IPA = f"{T}.ipa_0"
_PROJ = ("linear_q", "linear_kv", "linear_q_points", "linear_kv_points")
IPA_PARAMS = tuple(f"{IPA}.{n}.{t}" for n in _PROJ + ("linear_b", "down_z", "linear_out") for t in ("weight", "bias")) + (
    f"{IPA}.head_weights",)
LB_BIAS = f"{IPA}.linear_b.bias"
# the groups of ScoreNetwork.flat_layout_groups() for one IPA block, in its order; every other parameter on its own
FLAT_GROUPS = ((f"{IPA}.linear_b.weight", f"{IPA}.down_z.weight"), (f"{IPA}.linear_b.bias", f"{IPA}.down_z.bias"),
               tuple(f"{IPA}.{n}.weight" for n in _PROJ), tuple(f"{IPA}.{n}.bias" for n in _PROJ))


def _ipa_fn(Lf, Cs, relu):
    """model/ipa_pytorch.py:303-471 on flat rows; leaves s [R,256], z [P,128], Rm [R,3,3], trans [R,3] and the 15 parameters"""
    B, N = Cs["B"], Cs["N"]
    lin = lambda n, x: F.linear(x, Lf[f"{IPA}.{n}.weight"], Lf[f"{IPA}.{n}.bias"])
    s = Lf["s"].view(B, N, 256)
    Rm, t = Lf["Rm"].view(B, N, 3, 3), Lf["trans"].view(B, N, 3)
    m = Cs["mask"].view(B, N)
    q = lin("linear_q", s).view(B, N, H, C)
    kv = lin("linear_kv", s).view(B, N, H, 2 * C)
    k, v = kv[..., :C], kv[..., C:]

    def pts(raw, n):                                              # [x | y | z] blocks -> Rigid.apply (:345-374)
        p = torch.stack(raw.split(raw.shape[-1] // 3, dim=-1), -1)
        return ((Rm[:, :, None] * p[..., None, :]).sum(-1) + t[:, :, None]).view(B, N, H, n, 3)

    qp = pts(lin("linear_q_points", s), PQ)
    kvp = pts(lin("linear_kv_points", s), PQ + PV)
    kp, vp = kvp[..., :PQ, :], kvp[..., PQ:, :]
    # [linear_b ; down_z] of z as one product: the same numbers as the two Linears, and one tensor whose gradient is dzb
    zb = F.linear(Lf["z"].view(B, N, N, 128), torch.cat([Lf[f"{IPA}.linear_b.weight"], Lf[f"{IPA}.down_z.weight"]], 0),
                  torch.cat([Lf[f"{IPA}.linear_b.bias"], Lf[f"{IPA}.down_z.bias"]], 0))
    zb.retain_grad()
    Cs["stash"][zb.dtype] = zb
    a = torch.einsum("bihc,bjhc->bhij", q, k) * math.sqrt(1.0 / (3 * C))
    a = a + math.sqrt(1.0 / 3) * zb[..., :H].permute(0, 3, 1, 2)
    d2 = ((qp[:, :, None] - kp[:, None, :]) ** 2).sum(-1)                                   # [B, i, j, H, Pq]
    hw = F.softplus(Lf[f"{IPA}.head_weights"]) * math.sqrt(1.0 / (3 * (PQ * 9.0 / 2)))
    a = a + ((d2 * hw[:, None]).sum(-1) * (-0.5)).permute(0, 3, 1, 2)
    a = torch.softmax(a + (1e5 * (m[:, :, None] * m[:, None, :] - 1))[:, None], dim=-1)
    o = torch.einsum("bhij,bjhc->bihc", a, v).reshape(B, N, H * C)
    og = torch.einsum("bhij,bjhpx->bihpx", a, vp) - t[:, :, None, None]
    ol = (Rm.transpose(-1, -2)[:, :, None, None] * og[..., None, :]).sum(-1)               # invert_apply (:442)
    on = torch.sqrt((ol ** 2).sum(-1) + 1e-8).reshape(B, N, H * PV)
    ol = ol.reshape(B, N, H * PV, 3)
    opair = torch.einsum("bhij,bijc->bihc", a, zb[..., H:]).reshape(B, N, -1)
    feats = torch.cat([o, ol[..., 0], ol[..., 1], ol[..., 2], on, opair], -1)
    x1 = (s + m[..., None] * lin("linear_out", feats)).reshape(B * N, 256)
    return dict(x1=x1), (x1 * Cs["dx1"]).sum()


def _unit_quats(g, n):
    q = torch.randn(n, 4, generator=g, dtype=torch.float64)
    return (q / q.norm(dim=-1, keepdim=True)).float()


@functools.lru_cache(maxsize=None)
def _ipa_case(B, N, seed, hw_edges):
    P = {k: _params(seed)[k] for k in IPA_PARAMS}
    if hw_edges:
        P[f"{IPA}.head_weights"] = torch.tensor(HW_EDGES)
    g = torch.Generator().manual_seed(seed + 1100)
    R, Pn = B * N, B * N * N
    rn = lambda *s: torch.randn(*s, generator=g)
    m = torch.ones(B, N)
    m[0, N - 3:] = 0.0                                            # a padded tail ...
    m[B - 1, N // 2] = 0.0                                        # ... and one masked residue in mid-chain
    # translations in the kernel's units, at most 1.5 per axis (the note on translations in tests/test_ipa_bwd.py)
    t = dict(s=rn(R, 256), z=rn(Pn, 128), quat=_unit_quats(g, R), trans=3.0 * torch.rand(R, 3, generator=g) - 1.5,
             mask=m.reshape(-1).contiguous(), dx1=rn(R, 256), ds0=rn(R, 256), dframe0=rn(R, 12), dz0=rn(Pn, 128))
    consts = dict(B=B, N=N, mask=t["mask"], dx1=t["dx1"], stash={})
    leaves = dict(P, s=t["s"], z=t["z"], Rm=fo.quat_to_rot(t["quat"].double()), trans=t["trans"])
    ref = Reference(_ipa_fn, leaves, consts)
    dzb_ref = consts["stash"][torch.float64].grad.reshape(Pn, 40)
    # the restatement is the oracle's IPA
    d = lambda x: x.double()
    out = fo.ipa({k: d(v) for k, v in P.items()}, IPA, d(t["s"]).view(B, N, 256), d(t["z"]).view(B, N, N, 128),
                 d(t["quat"]).view(B, N, 4), d(t["trans"]).view(B, N, 3), d(m))
    assert relerr(d(t["s"]) + d(t["mask"])[:, None] * out.reshape(R, 256), ref.r64["x1"]) < 1e-12
    return t, P, ref, dzb_ref


def _flat(dev, P):
    """parameters, and zeroed gradients in a second buffer, laid back to back group by group (64-element aligned groups)"""
    order = list(FLAT_GROUPS) + [(n,) for n in P if not any(n in grp for grp in FLAT_GROUPS)]
    place, off = {}, 0
    for grp in order:
        for n in grp:
            place[n] = off
            off += P[n].numel()
        off = (off + 63) // 64 * 64
    pbuf, gbuf = torch.zeros(off, device=dev), torch.zeros(off, device=dev)
    Pd = {n: pbuf[o:o + P[n].numel()].view(P[n].shape) for n, o in place.items()}
    for n in P:
        Pd[n].copy_(P[n])
    return Pd, {n: gbuf[o:o + P[n].numel()].view(P[n].shape) for n, o in place.items()}, pbuf


def _same_storage(a, b):
    return a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr()


_ZERO = dict(ipa_flash_fwd=0, ipa_sequence_fwd=0, ipa_flash_bwd=0, ipa_sequence_bwd=0, ipa_flash_bwd_keys=0, ipa_keys_gemms=0)
_SEQ = dict(_ZERO, ipa_sequence_fwd=1, ipa_sequence_bwd=1, ipa_keys_gemms=1)
# launch path -> (options, the counters of ops.STATS one forward + backward must add)
IPA_PATHS = dict(
    sequence=(dict(), _SEQ),
    unfused=(dict(fused_ipa_attn=False), _SEQ),
    flash=(dict(flash_ipa_min_tiles=0, flash_ipa_bwd_min_tiles=0), dict(_ZERO, ipa_flash_fwd=1, ipa_flash_bwd=1, ipa_flash_bwd_keys=1)),
    flash_gemm_keys=(dict(flash_ipa_min_tiles=0, flash_ipa_bwd_min_tiles=0, flash_ipa_keys=False),
                     dict(_ZERO, ipa_flash_fwd=1, ipa_flash_bwd=1, ipa_keys_gemms=1)))


def _stats_delta(before):
    return {k: ops.STATS[k] - before[k] for k in _ZERO}


def _ipa(dev, B, N, seed, layout, path, dz_mode="assign", zb_given=False, hw_edges=False):
    t, P, ref, dzb_ref = _ipa_case(B, N, seed, hw_edges)
    R, Pn = B * N, B * N * N
    k = {n: v.to(dev).contiguous() for n, v in t.items()}
    if layout == "flat":
        Pd, G, pbuf = _flat(dev, P)
    else:
        Pd = {n: v.to(dev) for n, v in P.items()}
        G = _zeros_like(Pd, IPA_PARAMS)
    # (handed in: the float32 product of torch, not the library's)
    zb = F.linear(t["z"], *_w40(P, IPA)).to(dev).contiguous() if zb_given else None
    ov, want = IPA_PATHS[path]
    what = f"dev={dev} B={B} N={N} {layout} {path} dz={dz_mode} zb={'given' if zb_given else 'none'}{' hw_edges' if hw_edges else ''}"
    ops.reset_dw_queue()
    before = dict(ops.STATS)
    with options.override(**ov):
        assert (nw._proj_views(Pd, IPA) is not None) == (layout == "flat") and (nw._proj_views(G, IPA) is not None) == (layout == "flat")
        x1, sv = nw.ipa_fwd(Pd, IPA, ops.mv(k["s"]), k["z"], k["quat"], k["trans"], k["mask"], B, N, zb=zb)
        # W40 is a view of the parameters in the flat layout, a pack of its own otherwise
        assert _same_storage(sv["W40"], Pd[f"{IPA}.linear_b.weight"]) == (layout == "flat")
        assert sv["fused_attn"] == (path != "unfused") and (zb is None or sv["zb"] is zb)
        ds, dframe = k["ds0"].clone(), k["dframe0"].clone()
        dz = k["dz0"].clone() if dz_mode == "accumulate" else torch.full((Pn, 128), NAN, device=dev)
        pend = nw.ipa_bwd(Pd, G, IPA, sv, k["dx1"], ops.mv(ds), dz, dframe, dz_accumulate=dz_mode == "accumulate",
                          defer_dz=dz_mode == "defer")
        _finish()
    assert _stats_delta(before) == want, ("another launch path ran", path, _stats_delta(before))
    got = dict(x1=x1, ds=ds, dframe=dframe)
    if dz_mode == "defer":
        # the buffer is left alone; the consumer's term dzb W40 is the whole gradient of z
        assert bool(torch.isnan(dz).all()), "defer_dz wrote dz"
        dzb, W40 = pend
        assert dzb.shape == (Pn, 40) and W40.shape == (40, 128)
        got["dz"] = dzb.double().cpu() @ W40.double().cpu()
    else:
        assert pend is None
        got["dz"] = dz
    got.update({"d:" + n: G[n] for n in IPA_PARAMS if n != LB_BIAS})
    dz0 = t["dz0"] if dz_mode == "accumulate" else torch.zeros(Pn, 128)
    refs = []
    for r, add in ((ref.r64, lambda a, b: a.double() + b), (ref.r32, lambda a, b: (a + b.float()).double())):
        refs.append(dict(r, ds=add(t["ds0"], r["d:s"]), dz=add(dz0, r["d:z"]),
                         dframe=add(t["dframe0"], torch.cat([r["d:Rm"].reshape(R, 9), r["d:trans"]], -1))))
    with parity_log.case(f"ipa {what} (linear_b.bias)"):
        # analytically zero (softmax shift invariance): the absolute bound of the module docstring, not a relative one
        lb = float(G[LB_BIAS].double().abs().max())
        lb_bound = 8 * 2.0 ** -24 * float(dzb_ref[:, :H].abs().sum(0).max())
        parity_log.out("ipa.linear_b.bias.abs", lb)
        parity_log.out("ipa.linear_b.bias.abs_bound", lb_bound)
        print(f"[ipa] {what}: |d linear_b.bias| {lb:.2e} bound {lb_bound:.2e} (reference {float(ref.r64['d:' + LB_BIAS].abs().max()):.1e})")
        assert float(ref.r64["d:" + LB_BIAS].abs().max()) < 1e-9 * lb_bound
        assert lb <= lb_bound, (lb, lb_bound)
    _compare("ipa", what, got, refs[0], refs[1], names={"d:" + n: n for n in IPA_PARAMS})


def _ipa_sampling(dev, B, N, seed, split_n):
    """forward only, save=False: the cache, out_view, the key-split kernel (B, N) / split_n"""
    for (b, n), form in (((B, N), "cache"), ((B, N), "out_view"), (split_n, "split")):
        t, P, ref, _ = _ipa_case(b, n, seed, False)
        R = b * n
        k = {nm: v.to(dev).contiguous() for nm, v in t.items()}
        Pd = {nm: v.to(dev) for nm, v in P.items()}
        call = lambda **kw: nw.ipa_fwd(Pd, IPA, ops.mv(k["s"]), k["z"], k["quat"], k["trans"], k["mask"], b, n, save=False, **kw)
        before = dict(ops.STATS)
        if form == "cache":
            cache = {}
            x1, sv = call(cache=cache)
            Wp, bp = cache[("Wproj", IPA)]
            assert Wp.shape == (6816, 256) and bp.shape == (6816,) and ("W40", IPA) in cache and sv["A"] is not None
            x1b, _ = call(cache=cache)
            assert cache[("Wproj", IPA)][0] is Wp and torch.equal(x1, x1b), "a second call with the same cache differs"
            want = dict(_ZERO, ipa_sequence_fwd=2)
        elif form == "out_view":
            buf = torch.full((R, 640), NAN, device=dev)
            ret, _ = call(cache={}, out_view=(buf, 320, 640))
            assert ret is buf
            x1 = buf[:, 320:576]
            assert bool(torch.isnan(buf[:, :320]).all()) and bool(torch.isnan(buf[:, 576:]).all()), "written outside columns 320..575"
            want = dict(_ZERO, ipa_sequence_fwd=1)
        else:
            assert n >= 16
            with options.override(flash_ipa_split_min_n=16):
                x1, sv = call()
            assert sv["A"] is None            # (the split kernel keeps the probabilities to itself)
            want = dict(_ZERO, ipa_flash_fwd=1)
        assert _stats_delta(before) == want, (form, _stats_delta(before))
        _compare("ipa", f"sampling dev={dev} B={b} N={n} {form}", dict(x1=x1), ref.r64, ref.r32)


# every launch path x both layouts, dz assigned
IPA_GRID = tuple((layout, path) for path in IPA_PATHS for layout in ("scattered", "flat"))
# the other two dz modes on the default path; zb handed in on the flash and the sequence path; HW_EDGES on both attention kernels
IPA_MORE = (("scattered", "sequence", dict(dz_mode="accumulate", hw_edges=True)), ("flat", "sequence", dict(dz_mode="defer")),
            ("flat", "flash", dict(zb_given=True)), ("scattered", "sequence", dict(zb_given=True)),
            ("scattered", "flash", dict(zb_given=True, dz_mode="accumulate", hw_edges=True)))
_gid = lambda c: f"{c[0]}-{c[1]}"
_mid = lambda c: f"{c[0]}-{c[1]}-" + "-".join(f"{k}={v}" for k, v in c[2].items())


@pytest.mark.parametrize("case", IPA_GRID, ids=_gid)
def test_ipa_stage_emu(use_emu, case):
    _ipa("cpu", 2, 9, 60, *case)


@pytest.mark.parametrize("case", IPA_MORE, ids=_mid)
def test_ipa_stage_more_emu(use_emu, case):
    _ipa("cpu", 2, 9, 60, case[0], case[1], **case[2])


def test_ipa_sampling_emu(use_emu):
    _ipa_sampling("cpu", 2, 9, 60, (1, 18))


@pytest.mark.gpu
@pytest.mark.parametrize("case", IPA_GRID, ids=_gid)
def test_ipa_stage_gpu(hip_lib, case):
    _ipa("cuda", 2, 37, 61, *case)
    if case in (("flat", "sequence"), ("flat", "flash")):
        _ipa("cuda", 1, 130, 62, *case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", IPA_MORE, ids=_mid)
def test_ipa_stage_more_gpu(hip_lib, case):
    _ipa("cuda", 2, 37, 61, case[0], case[1], **case[2])


@pytest.mark.gpu
def test_ipa_sampling_gpu(hip_lib):
    _ipa_sampling("cuda", 2, 37, 61, (2, 37))


# ------------------------------------------------------------------------------------------------ bb_update
BB = f"{T}.bb_update_0.linear"
BB_PARAMS = (f"{BB}.weight", f"{BB}.bias")


def _bb_fn(Lf, Cs, relu):
    R = Lf["n3"].shape[0]
    d = Cs["dmask"]
    upd = F.linear(Lf["n3"] * d[:, None], Lf[f"{BB}.weight"], Lf[f"{BB}.bias"])
    q2, t2 = fo.backbone_update(Lf["quat"], Lf["trans"], upd, d)
    loss = ((q2 * Cs["dq2"]).sum() + (t2 * Cs["dt2"]).sum() + (fo.quat_to_rot(Lf["quat"]).reshape(R, 9) * Cs["dframe"][:, :9]).sum()
            + (Lf["trans"] * Cs["dframe"][:, 9:]).sum())
    return dict(q2=q2, t2=t2), loss


@functools.lru_cache(maxsize=None)
def _bb_case(B, N, seed, soft):
    P = {k: _params(seed)[k] for k in BB_PARAMS}
    g = torch.Generator().manual_seed(seed + 1300)
    R = B * N
    rn = lambda *s: torch.randn(*s, generator=g)
    fixed = (torch.rand(B, N, generator=g) < 0.25).float()
    res = torch.ones(B, N)
    res[0, N - 2:] = 0.0
    d = (1 - fixed) * res                                         # zeros for fixed and padded residues, ones elsewhere
    d[B - 1] = 0.0                                                # one example all zero
    if soft:
        # fractional entries (module docstring): the only values at which dupd and dupd * dmask differ
        d[0, :N // 2] *= 0.25 + 0.5 * torch.rand(N // 2, generator=g)
    t = dict(n3=rn(R, 256), quat=_unit_quats(g, R), trans=1.5 * rn(R, 3), dmask=d.reshape(-1).contiguous(), dq2=rn(R, 4),
             dt2=rn(R, 3), dframe=rn(R, 12), dn30=rn(R, 256))
    consts = {n: t[n] for n in ("dmask", "dq2", "dt2", "dframe")}
    return t, P, Reference(_bb_fn, dict(P, n3=t["n3"], quat=t["quat"], trans=t["trans"]), consts)


def _bb(dev, B, N, seed, soft=False):
    t, P, ref = _bb_case(B, N, seed, soft)
    R = B * N
    k = {n: v.to(dev).contiguous() for n, v in t.items()}
    Pd = {n: v.to(dev) for n, v in P.items()}
    G = _zeros_like(Pd, BB_PARAMS)
    ops.reset_dw_queue()
    # the two steps of trunk._backward around the IPA backward: dframe = None first, the IPA's dframe folded in afterwards
    q2, t2, sv = trunk.bb_update_fwd(Pd, 0, k["n3"], k["dmask"], k["quat"], k["trans"], R)
    dn3 = k["dn30"].clone()
    dq, dt = trunk.bb_update_bwd(Pd, G, 0, sv, k["dq2"], k["dt2"], None, dn3)
    trunk._frame_grad_fold(k["quat"], k["dframe"], dq, dt, R)
    _finish()
    got = dict(q2=q2, t2=t2, dn3=dn3, dq=dq, dt=dt)
    got.update({"d:" + n: G[n] for n in BB_PARAMS})
    r64 = dict(ref.r64, dn3=t["dn30"].double() + ref.r64["d:n3"], dq=ref.r64["d:quat"], dt=ref.r64["d:trans"])
    r32 = dict(ref.r32, dn3=(t["dn30"] + ref.r32["d:n3"].float()).double(), dq=ref.r32["d:quat"], dt=ref.r32["d:trans"])
    _compare("bb_update", f"dev={dev} R={R} soft={soft}", got, r64, r32, names={"d:" + n: n for n in BB_PARAMS})


@pytest.mark.parametrize("soft", (False, True), ids=("binary", "fractional"))
def test_bb_update_stage_emu(use_emu, soft):
    _bb("cpu", 2, 9, 60, soft)


@pytest.mark.gpu
@pytest.mark.parametrize("soft", (False, True), ids=("binary", "fractional"))
def test_bb_update_stage_gpu(hip_lib, soft):
    _bb("cuda", 2, 37, 61, soft)
    _bb("cuda", 2, 150, 62, soft)


# ------------------------------------------------------------------------------------------------ heads
TP = "score_model.torsion_pred"
TP_PARAMS = tuple(f"{TP}.{n}.{t}" for n in ("linear_1", "linear_2", "linear_final") for t in ("weight", "bias"))
OUT_KEYS = ("psi", "rot_score", "trans_score", "rigids", "atom37", "atom14")
D_OUT_FORMS = dict(all=("psi", "rot_score", "trans_score", "rigids", "atom37"), loss=("rot_score", "trans_score", "rigids", "atom37"),
                   psi=("psi",))


def _heads_fn(Lf, Cs, relu):
    """the torsion MLP (ipa_pytorch.py:474-490) in front of test_frames._heads_ref; loss over the entries of d_out present"""
    node = Lf["node"]
    h1 = relu(F.linear(node, Lf[f"{TP}.linear_1.weight"], Lf[f"{TP}.linear_1.bias"]))
    h2 = F.linear(h1, Lf[f"{TP}.linear_2.weight"], Lf[f"{TP}.linear_2.bias"]) + node
    u = u_mlp = F.linear(h2, Lf[f"{TP}.linear_final.weight"], Lf[f"{TP}.linear_final.bias"])
    if Cs.get("u_stage") is not None:
        u = u + (Cs["u_stage"] - u).detach()            # the heads at the stage's own u (_heads_direct); gradients pass through
    # (test_frames' reference is float64 throughout: the float32 pass rounds the MLP and hands it u, as the stage hands fd_heads_fwd)
    ref = tf._heads_ref(Cs["x"], dict(qF=Lf["qF"].double(), transF=Lf["transF"].double(), u=u.double()), None)
    Cs["stash"][node.dtype] = dict(ref, u=u)
    # (0 x the frame: psi alone does not reach it, and every leaf needs a gradient tensor)
    loss = 0.0 * (Lf["qF"].sum() + Lf["transF"].sum())
    for kk in Cs["use"]:
        loss = loss + (ref[kk] * Cs["d_" + kk]).sum()
    return dict({kk: ref[kk] for kk in OUT_KEYS}, u=u_mlp), loss


@functools.lru_cache(maxsize=None)
def _heads_case(B, N, seed, form):
    P = {k: _params(seed)[k] for k in TP_PARAMS}
    g = torch.Generator().manual_seed(seed + 1500)
    R = B * N
    rn = lambda *s: torch.randn(*s, generator=g)
    # random frame pairs: the branch points of quat_to_rotvec and the psi clamp are test_frames' cases; qF of norm 0.5 .. 2
    qF = (tf.d64(_unit_quats(g, R)) * (0.5 + 1.5 * torch.rand(R, 1, generator=g, dtype=torch.float64))).float()
    x = dict(rig0=torch.cat([_unit_quats(g, R), rn(R, 3) * 10], -1), qF=qF, transF=rn(R, 3), gt=rn(R, 14),
             fixed=(torch.rand(R, generator=g) < 0.2).float(), mask=(torch.rand(R, generator=g) > 0.15).float(),
             t=torch.linspace(0.2, 0.8, B), exact=torch.zeros(R, dtype=torch.bool))
    t = dict(node=rn(R, 256), dnode0=rn(R, 256))
    gin = dict(psi=rn(R, 2), rot_score=torch.randn(R, 3, generator=g, dtype=torch.float64), trans_score=rn(R, 3), rigids=rn(R, 7),
               atom37=rn(R, 37, 3))
    use = D_OUT_FORMS[form]
    consts = dict({"d_" + kk: gin[kk] for kk in use}, x=x, use=use, stash={})
    leaves = dict(P, node=t["node"], qF=qF, transF=x["transF"])
    ref = Reference(_heads_fn, leaves, consts)
    # the oracle's torsion head is the restatement's (psi before the fixed-residue blend)
    un = fo.torsion_head({kk: v.double() for kk, v in P.items()}, t["node"].double())
    assert relerr(un, consts["stash"][torch.float64]["un"]) < 1e-12
    return x, t, gin, P, ref, consts


def _heads_direct(consts, leaves, relu_gates, u_stage):
    """The float64 reference of what fd_heads_fwd / _bwd give, at the stage's own u (float32, promoted): test_frames hands kernel
    and reference the same float32 inputs, and its bounds are for that; how far u itself is from float64 is the MLP's check.
    Returns the six outputs, d:qF, d:transF, and what test_frames._heads holds them to: the scale and floor of rot_score, per
    incoming gradient the magnitudes of the terms dq and dt add up, the floor of dq under the fp32 rounding of inv(qF) (x) q0."""
    x, use = consts["x"], consts["use"]
    R = x["qF"].shape[0]
    Lf = {kk: v.double().clone().requires_grad_(True) for kk, v in leaves.items()}
    Cs = {kk: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for kk, v in consts.items()}
    outs, _ = _heads_fn(Lf, dict(Cs, u_stage=u_stage.double()), Gates(fixed=relu_gates))
    aux = consts["stash"][torch.float64]
    sens = ((aux["gs"].abs() / (aux["omega"] + 1e-6) + aux["dg"].abs()) * tf.d64(x["mask"])).detach()[:, None].expand(R, 3)
    rot = dict(scale=torch.maximum(tf.rowmax(outs["rot_score"], R), sens), floor=8 * aux["noise"].detach()[:, None].expand(R, 3))
    grad = [torch.zeros(R, 4, dtype=torch.float64), torch.zeros(R, 3, dtype=torch.float64)]
    cond = [torch.zeros(R, 4, dtype=torch.float64), torch.zeros(R, 3, dtype=torch.float64)]
    grot = None
    for kk in use:
        gs = torch.autograd.grad((outs[kk] * Cs["d_" + kk]).sum(), (Lf["qF"], Lf["transF"]), retain_graph=True, allow_unused=True)
        for i, gr in enumerate(gs):
            if gr is not None:
                grad[i], cond[i] = grad[i] + gr, cond[i] + tf.rowmax(gr, R)
        if kk == "rot_score":
            grot = gs[0]
    dq_floor = None
    if grot is not None:
        gg = torch.Generator().manual_seed(77)
        spread = torch.zeros(R, 4, dtype=torch.float64)
        for _ in range(2):
            q0p = tf.d64(x["rig0"]).clone()
            q0p[:, :4] *= 1 + 2.0 ** -23 * (2 * torch.rand(R, 4, generator=gg, dtype=torch.float64) - 1)
            P2 = dict(qF=tf.d64(x["qF"]).requires_grad_(True), transF=tf.d64(x["transF"]), u=u_stage.double())
            r2 = tf._heads_ref(dict(x, rig0=q0p), P2, None)
            (g2,) = torch.autograd.grad((r2["rot_score"] * Cs["d_rot_score"]).sum(), P2["qF"])
            spread = torch.maximum(spread, (g2 - grot).abs())
        dq_floor = 4 * tf.rowmax(spread, R)
    return {kk: outs[kk].detach() for kk in OUT_KEYS}, grad, rot, cond, dq_floor


def _heads(dev, B, N, seed, form):
    x, t, gin, P, ref, consts = _heads_case(B, N, seed, form)
    R = B * N
    Pd = {n: v.to(dev) for n, v in P.items()}
    feats = dict(rigids_t=x["rig0"].view(B, N, 7), torsion_angles_sin_cos=x["gt"].view(B, N, 7, 2), fixed_mask=x["fixed"].view(B, N),
                 res_mask=x["mask"].view(B, N), t=x["t"])
    feats = {n: v.to(dev).contiguous() for n, v in feats.items()}
    shapes = dict(psi=(B, N, 2), rot_score=(B, N, 3), trans_score=(B, N, 3), rigids=(B, N, 7), atom37=(B, N, 37, 3))
    d_out = {kk: gin[kk].view(shapes[kk]).to(dev) for kk in consts["use"]}
    G = _zeros_like(Pd, TP_PARAMS)
    ops.reset_dw_queue()
    out, sv = trunk.heads_fwd(Pd, t["node"].to(dev), x["qF"].to(dev), x["transF"].to(dev), feats, B, N, tf.DCONF)
    dnode = t["dnode0"].to(dev).clone()
    dq, dt = trunk.heads_bwd(Pd, G, sv, feats, d_out, dnode)
    _finish()
    r64, r32 = ref.for_gates([sv["h1"] > 0], [sv["h1"]])
    what = f"dev={dev} B={B} N={N} d_out={form}"
    # the direct outputs of fd_heads_fwd / fd_heads_bwd: the element-wise bounds of tests/test_frames.py, not loosened
    leaves = dict(P, node=t["node"], qF=x["qF"], transF=x["transF"])
    assert sv["u"].shape == (R, 2)
    ref_out, ref_grad, rot, cond, dq_floor = _heads_direct(consts, leaves, ref.relu.used, sv["u"].cpu())
    with parity_log.case(f"heads {what} (direct)"):
        for kk in OUT_KEYS:
            kw = rot if kk == "rot_score" else {}
            tf.check(f"heads.{kk}", out[kk].reshape(ref_out[kk].shape), ref_out[kk], tf.TOL_HEADS, **kw)
        tf.check("heads.dq", dq, ref_grad[0], tf.TOL_HEADS_BWD, scale=cond[0], floor=dq_floor)
        tf.check("heads.dt", dt, ref_grad[1], tf.TOL_HEADS_BWD, scale=cond[1])
        if form == "psi":
            assert float(dq.abs().max()) == 0.0 and float(dt.abs().max()) == 0.0      # nothing reaches the frame
    # through the MLP glue (u, the operand the forward hands fd_heads_fwd, included): the 8 e32 rule
    got = dict(u=sv["u"], dnode=dnode)
    got.update({"d:" + n: G[n] for n in TP_PARAMS})
    r64 = dict(r64, dnode=t["dnode0"].double() + r64["d:node"])
    r32 = dict(r32, dnode=(t["dnode0"] + r32["d:node"].float()).double())
    _compare("heads", what, got, r64, r32, names={"d:" + n: n for n in TP_PARAMS})


@pytest.mark.parametrize("form", tuple(D_OUT_FORMS))
def test_heads_stage_emu(use_emu, form):
    _heads("cpu", 2, 9, 60, form)


@pytest.mark.gpu
@pytest.mark.parametrize("form", tuple(D_OUT_FORMS))
def test_heads_stage_gpu(hip_lib, form):
    _heads("cuda", 2, 37, 61, form)
