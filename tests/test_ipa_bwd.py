"""The backward of IPA attention (model/ipa_pytorch.py:380-457) against float64 autograd, one launch path at a time:

  flash     fd_ipa_opt_bwd_dot -> fd_ipa_flash_bwd (with dkp, and with dkp = None) -> fd_ipa_flash_bwd_keys, dQ GEMM
  attn      fd_ipa_attn_bwd: slab <= 128, slab <= 256, unaligned zb / dzb (<= 256), direct reads (> 256); kp_soa given / None
  unfused   fd_ipa_opair_bwd -> fd_ipa_softmax_bwd (<= 256 and > 256)
  kpts      fd_ipa_kpts_bwd alone
  dz_acc    fd_ipa_dz_acc against dzb W40 in float64

The reference (`_autograd`) is hermetic: torch float64 with autograd from the raw inputs; the kernels under test receive the
probabilities and the features of THAT forward, rounded to float32, so this file depends on no forward kernel and the rows of
masked residues are well defined (in float64 the uniform -1e5 of the mask shifts a row without erasing it).

Bounds: every error is max|got - ref| / max|ref| per output tensor.  The same autograd evaluated in float32 torch (mask as its
exact limit) gives the float32 noise floor e32 of a case; the bound of the case is min(8 max_k e32_k, 1e-5) over
k = dL, dzb, dqp, dkp, dhead_w -- 8 because the kernels sum sequentially and tile by tile and fd_ipa_flash_bwd expands the
distances, where torch sums pairwise.  Outputs whose reference is exactly zero (N = 1: dL, dqp, dkp, dhead_w, dQ, dK) are held to
8 * 2^-24 * max|dP| absolute.  Nothing here is derived from what the kernels give.

Achieved (worst case over the cases of a tier, relative to the tensor maximum; `parity_log` keys ipa_bwd.<path>.<output>):

  path (entry points)                       output: interpreter / MI355X (device cases include the interpreter's)
  flash (fd_ipa_flash_bwd)                  dL 2.1e-6 / 2.1e-6   dzb 1.5e-6 / 1.6e-6   dqp 1.4e-6 / 1.8e-6   dkp 1.3e-6 / 1.7e-6
                                            dhead_w 1.7e-6 / 3.9e-6 (N = 300, bound 6.8e-6)
    N = 1, absolute (bound 3.4e-5)          dL 5.7e-6   dqp, dkp 2.0e-6   dhead_w 7.1e-6   (both tiers)
  flash_keys (fd_ipa_flash_bwd_keys, GEMM)  dQ 1.6e-6 / 1.6e-6   dK 1.7e-6 / 1.7e-6   dV 5.4e-7 / 5.9e-7   dvp 4.7e-7 / 5.1e-7
  opt_bwd_dot                               doptg 1.4e-7 / 1.5e-7   ptdot 6.9e-7 / 6.9e-7
  attn, attn_kp, attn_unaligned, unfused    dL, dzb 7.7e-7 / 7.7e-7   dqp 4.1e-7 / 5.1e-7   dkp 3.7e-7 / 4.7e-7   dhead_w 7.9e-7 / 8.9e-7
    (bit-identical to each other); N = 1    dL, dqp, dkp, dhead_w exactly 0
  kpts (fd_ipa_kpts_bwd on the float64 dL)  dkp 2.5e-7 / 2.5e-7
  dz_acc                                    3.0e-7 / 3.5e-7 (bounds 0.8e-6 ... 2.4e-6)
  The bounds of the cases came out between 7.0e-7 (N = 1) and 1e-5; the tightest margins are dzb of `flash` at N = 1
  (5.1e-7 of 7.0e-7) and dhead_w of `flash` at N = 300.
"""
import functools
import math

import pytest
import torch

import parity_log
from se3_diffusion_amd import ops
from test_ipa_flash import C, CZ4, F_PAIR, H, LDF, LDP, PQ, PV, ZB, _bwd_flash, _bwd_sequence, _inputs, _points, _quat_to_rot

NAN = float("nan")
HW_EDGES = (25.0, 20.5, 3.0, 0.0, -3.0, -12.0, 0.5, -0.5)      # both sides of the softplus / sigmoid branch at 20; gamma ~ 0
FIVE = ("dL", "dzb", "dqp", "dkp", "dhw")

# (B, N, seed, spread, mask, head_w).  mask: rand = the 10 % of _inputs, last3 = the last three residues, whole = the second
# backbone entirely (the first keeps its random mask), ones.  Sizes: one ragged 16-tile (1, 5, 12), exactly one (16), N % 4 != 0
# (18, 37, 130: scalar rows of A / dL), several tiles with ragged rows and keys (37), 64-key blocks of kpts_bwd (130, 260),
# the 128 / 256 instantiation limits from both sides on the device.  Translations up to 3.0 per axis and no further: see DESIGN.md
EMU_CASES = ((1, 1, 0, 1.0, "ones", "rand"), (1, 5, 1, 1.5, "last3", "rand"), (1, 12, 2, 1.0, "rand", "rand"),
             (1, 16, 3, 3.0, "ones", "rand"), (1, 18, 4, 1.0, "rand", "edges"), (2, 37, 5, 3.0, "whole", "rand"),
             (1, 130, 6, 1.5, "rand", "rand"), (1, 260, 7, 1.0, "rand", "rand"))
GPU_CASES = EMU_CASES + ((3, 100, 8, 3.0, "rand", "rand"), (2, 128, 9, 1.0, "rand", "rand"), (1, 129, 10, 1.5, "last3", "rand"),
                         (1, 256, 11, 1.5, "rand", "edges"), (1, 257, 12, 1.0, "ones", "rand"), (1, 300, 13, 3.0, "rand", "rand"))
_id = lambda c: f"B{c[0]}N{c[1]}"


# ---------------------------------------------------------------------------------------------------------------- reference
def _autograd(c, dt, literal_mask):
    """model/ipa_pytorch.py:380-457 from the raw inputs in dtype dt, loss = sum(feats * dfeats); returns the forward's A and feats
    and every gradient the launch paths produce.  literal_mask: the reference's + 1e5 (m_i m_j - 1); else its exact limit (rows of
    masked residues unshifted, -inf on the masked keys of the others)."""
    B, N = c["B"], c["N"]
    R = B * N
    leaf = lambda t: t.to(dt).clone().requires_grad_(True)
    P = c["proj"].view(B, N, LDP)
    q = leaf(P[..., :H * C].reshape(B, N, H, C))
    kv = P[..., 2048:2048 + 2 * H * C].reshape(B, N, H, 2 * C)
    k, v = leaf(kv[..., :C]), leaf(kv[..., C:])
    qp, kp = leaf(c["qp"].view(B, N, H, PQ, 3)), leaf(c["kp"].view(B, N, H, PQ, 3))
    vp = leaf(c["vp"].view(B, N, H, PV, 3))
    zb, hw = leaf(c["zb"].view(B, N, N, ZB)), leaf(c["hw"])
    Rm = _quat_to_rot(c["quat"].to(dt)).view(B, N, 3, 3)
    t = c["trans"].to(dt).view(B, N, 3)
    m = c["mask"].to(dt).view(B, N)
    df = c["dfeats"].to(dt)
    gamma = torch.nn.functional.softplus(hw) * math.sqrt(1.0 / (3.0 * (PQ * 9.0 / 2.0)))
    lg = torch.einsum("bihc,bjhc->bhij", q, k) * math.sqrt(1.0 / (3 * C))
    lg = lg + math.sqrt(1.0 / 3) * zb[..., :H].permute(0, 3, 1, 2)
    d2 = ((qp[:, :, None] - kp[:, None]) ** 2).sum((-1, -2))                          # [B, i, j, H]
    lg = lg - 0.5 * (d2 * gamma).permute(0, 3, 1, 2)
    if literal_mask:
        lg = lg + 1e5 * (m[:, None, :, None] * m[:, None, None, :] - 1)
    else:
        add = torch.zeros(B, 1, N, N, dtype=dt)
        add.masked_fill_((m[:, None, :, None] > 0) & (m[:, None, None, :] == 0), float("-inf"))
        lg = lg + add
    lg.retain_grad()
    a = torch.softmax(lg, -1)
    o = torch.einsum("bhij,bjhc->bihc", a, v).reshape(R, H * C)
    og = torch.einsum("bhij,bjhpx->bihpx", a, vp)                                     # o_pt, global frame
    og.retain_grad()
    ol = torch.einsum("bnca,bnhpc->bnhpa", Rm, og - t[:, :, None, None, :]).reshape(R, H * PV, 3)      # R^T (o_pt - t)
    nrm = torch.sqrt((ol ** 2).sum(-1) + 1e-8)
    opair = torch.einsum("bhij,bijc->bihc", a, zb[..., H:]).reshape(R, H * CZ4)
    feats = torch.cat([o, ol[..., 0], ol[..., 1], ol[..., 2], nrm, opair], -1)
    (feats * df).sum().backward()
    d = lambda x: x.detach().double()
    dO = d(df)[:, :H * C].view(B, N, H, C)
    dout = d(df)[:, F_PAIR:].view(B, N, H, CZ4)
    dog = d(og.grad)
    dA = torch.einsum("bihc,bjhc->bhij", dO, d(v)) + torch.einsum("bihpx,bjhpx->bhij", dog, d(vp))
    dP = dA + torch.einsum("bihc,bijc->bhij", dout, d(zb)[..., H:])
    g = dict(dL=d(lg.grad), dzb=d(zb.grad).reshape(R * N, ZB), dqp=d(qp.grad).reshape(R, H, PQ * 3),
             dkp=d(kp.grad).reshape(R, H, PQ * 3), dhw=d(hw.grad), doptg=dog.reshape(R, H, PV * 3),
             ptdot=(dog * d(og)).sum((-1, -2)).reshape(R, H),                          # global frame, NOT centred on trans
             dQ=d(q.grad).reshape(R, H, C), dK=d(k.grad).reshape(R, H, C), dV=d(v.grad).reshape(R, H, C),
             dvp=d(vp.grad).reshape(R, H, PV * 3))
    return dict(A=d(a), feats=d(feats), dA=dA, dPmax=float(dP.abs().max()), g=g)


def _relerr(got, ref):
    return float((got.double().cpu() - ref).abs().max()) / float(ref.abs().max())


@functools.lru_cache(maxsize=None)
def _case(spec):
    """inputs, float64 reference, float32 noise floor and bound of one case (CPU tensors; shared by every test of the case)"""
    B, N, seed, spread, mask_mode, hw_mode = spec
    R = B * N
    proj, quat, trans, zb, hw, mask = _inputs("cpu", B, N, seed, spread, masked=mask_mode in ("rand", "whole"))
    if mask_mode == "last3":
        mask.view(B, N)[:, -3:] = 0.0
    elif mask_mode == "whole":
        mask.view(B, N)[1] = 0.0
    if hw_mode == "edges":
        hw = torch.tensor(HW_EDGES)
    dfeats = torch.randn(R, LDF, generator=torch.Generator().manual_seed(seed + 100))
    # global-frame points in float64, rounded ONCE: the same float32 values go to the kernels and (cast up) to the leaves
    P = proj.double().view(B, N, LDP)
    Rm = _quat_to_rot(quat.double()).view(B, N, 3, 3)
    t = trans.double().view(B, N, 3)
    glob = lambda x: torch.einsum("bnac,bnpc->bnpa", Rm, x) + t[:, :, None, :]
    qpg = glob(P[..., 6144:6336].view(B, N, 3, H * PQ).permute(0, 1, 3, 2)).view(B, N, H, PQ, 3)
    kvpg = glob(P[..., 6336:6816].view(B, N, 3, H * (PQ + PV)).permute(0, 1, 3, 2)).view(B, N, H, PQ + PV, 3)
    c = dict(B=B, N=N, proj=proj, quat=quat, trans=trans, zb=zb, hw=hw, mask=mask, dfeats=dfeats,
             qp=qpg.float().reshape(R, H, PQ * 3).contiguous(), kp=kvpg[..., :PQ, :].float().reshape(R, H, PQ * 3).contiguous(),
             vp=kvpg[..., PQ:, :].float().reshape(R, H, PV * 3).contiguous())
    c["kpT"] = c["kp"].view(B, N, H, PQ * 3).permute(0, 2, 3, 1).contiguous()          # fd_ipa_points_fwd's [B, 8, 24, N] copy
    r64 = _autograd(c, torch.float64, True)
    r32 = _autograd(c, torch.float32, False)
    c["ref"] = r64["g"]
    c["A"], c["feats"], c["dA"] = r64["A"].float().contiguous(), r64["feats"].float().contiguous(), r64["dA"].float().contiguous()
    c["e32"] = {k: _relerr(r32["g"][k], v) for k, v in r64["g"].items() if float(v.abs().max()) > 0.0}
    c["bound"] = min(8.0 * max(c["e32"][k] for k in FIVE if k in c["e32"]), 1e-5)
    # (the consumers' outputs and fd_ipa_opt_bwd_dot's: the same rule over every output of the case, never below the bound above)
    c["bound_all"] = min(8.0 * max(c["e32"].values()), 1e-5)
    c["abs_bound"] = 8.0 * 2.0 ** -24 * r64["dPmax"]
    if bool((mask == 0).any()) and bool((mask > 0).any()):
        assert bool((c["A"] == 0).any())                     # masked keys of valid rows: exact zeros in the probabilities
    return c


def _to(c, dev):
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in c.items() if k not in ("ref", "e32")}


def _check(c, path, got, hw_part=None):
    """every output finite and within the bound of the case; what was measured is printed and logged before it is asserted"""
    errs, bad = {}, []
    for k, gv in got.items():
        assert bool(torch.isfinite(gv).all()), (path, k)
        ref = c["ref"][k]
        sc = float(ref.abs().max())
        if sc > 0.0:
            errs[k] = float((gv.double().cpu().view_as(ref) - ref).abs().max()) / sc
            lim = c["bound"] if k in FIVE else c["bound_all"]
            parity_log.out(f"ipa_bwd.{path}.{k}", errs[k])
        else:                                                   # N = 1: the reference is exactly zero
            errs[k] = float(gv.double().cpu().abs().max())
            lim = c["abs_bound"]
            parity_log.out(f"ipa_bwd.{path}.{k}.abs", errs[k])
        if not errs[k] <= lim:
            bad.append((k, errs[k], lim))
    print(f"[ipa_bwd] {path} B={c['B']} N={c['N']}: " + " ".join(f"{k} {e:.2e}" for k, e in errs.items())
          + f" | bound {c['bound']:.2e} (consumers {c['bound_all']:.2e}, zero reference {c['abs_bound']:.2e} abs), "
          + f"e32 {max(c['e32'].values()):.1e}")
    if hw_part is not None:
        assert bool(torch.isfinite(hw_part).all()), (path, "hw_part")
    assert not bad, (path, c["B"], c["N"], bad)
    return errs


def _dhw0(c, dev, seed=0):
    """dhead_w is accumulated into (+=): it starts from random non-zero values of the gradient's own magnitude"""
    sc = float(c["ref"]["dhw"].abs().max()) or c["abs_bound"]
    return (torch.randn(H, generator=torch.Generator().manual_seed(seed)) * sc).to(dev)


def _poison(dev, *shape):
    return torch.full(shape, NAN, device=dev)


def _differ(a, b, dev):
    """the outputs that are not bit-identical between two launches.  dhead_w is the column sum of hw_part by float atomics over
    blocks of 16 rows (fd_colsum_acc): above 16 rows its last bits depend on the order in which the blocks of a launch retire, on
    the device also between two identical launches -- there the bit-identity is asserted of hw_part, its summands, instead"""
    return [k for k in a if not torch.equal(a[k], b[k]) and not (k == "dhw" and dev != "cpu")]


# --------------------------------------------------------------------------------------------------------- fd_ipa_flash_bwd path
def _path_flash(dev, spec):
    L = ops.lib()
    c = _case(spec)
    t = _to(c, dev)
    B, N = c["B"], c["N"]
    R = B * N
    doptg, ptdot, dframe = _poison(dev, R, H, PV * 3), _poison(dev, R, H), torch.zeros(R, 12, device=dev)
    L.call("fd_ipa_opt_bwd_dot", t["dfeats"], t["feats"], t["quat"], t["trans"], doptg, dframe, ptdot, R)
    _check(c, "opt_bwd_dot", dict(doptg=doptg, ptdot=ptdot))
    dhw0 = _dhw0(c, dev)

    def run(with_dkp):
        o = dict(dL=_poison(dev, B, H, N, N), dzb=_poison(dev, R * N, ZB), dqp=_poison(dev, R, H, PQ * 3), dhw=dhw0.clone())
        dkp, part = (_poison(dev, R, H, PQ * 3) if with_dkp else None), _poison(dev, R, H)
        L.call("fd_ipa_flash_bwd", t["proj"], t["A"], t["zb"], t["dfeats"], t["feats"], doptg, ptdot, t["qp"], t["kp"], t["vp"],
               t["hw"], t["trans"], o["dL"], o["dzb"], o["dqp"], dkp, o["dhw"], part, B, N)      # (raises unless FD_OK)
        return o, dkp, part

    o, dkp, part = run(True)
    o2, _, part2 = run(False)
    assert not _differ(dict(o, part=part), dict(o2, part=part2), dev), "dkp = None changed the other outputs"
    _check(c, "flash", dict(o, dkp=dkp, dhw=o["dhw"].double() - dhw0.double()), part)
    # the consumers of dL as network.ipa_bwd issues them: the key-side kernel, and dQ = sc dL K
    dproj, dvp, dkp2 = _poison(dev, R, LDP), _poison(dev, R, H, PV * 3), _poison(dev, R, H, PQ * 3)
    L.call("fd_ipa_flash_bwd_keys", t["A"], o["dL"], t["proj"], t["dfeats"], doptg, t["qp"], t["kp"], t["hw"], dproj, dvp, dkp2, B, N, 0)
    L.gemm(o["dL"], t["proj"], dproj, N, C, N, (N, 1), (LDP, 1), LDP, b_off=2048, batch=B * H, bdiv=H,
           a_bs=(H * N * N, N * N), b_bs=(N * LDP, 2 * C), c_bs=(N * LDP, C), alpha=math.sqrt(1.0 / (3 * C)))
    kvg = dproj[:, 2048:2048 + 2 * H * C].view(R, H, 2, C)
    _check(c, "flash_keys", dict(dQ=dproj[:, :H * C].reshape(R, H, C), dK=kvg[:, :, 0], dV=kvg[:, :, 1], dvp=dvp, dkp=dkp2))


# ---------------------------------------------------------------------------------- fd_ipa_attn_bwd and the unfused pair it fuses
def _path_attn(dev, spec):
    L = ops.lib()
    c = _case(spec)
    t = _to(c, dev)
    B, N = c["B"], c["N"]
    R = B * N
    dhw0 = _dhw0(c, dev, 1)

    def outs(dzb_off=0):
        buf = _poison(dev, R * N * ZB + dzb_off)
        return dict(dL=t["dA"].clone(), dzb=buf[dzb_off:].view(R * N, ZB), dqp=_poison(dev, R, H, PQ * 3),
                    dkp=_poison(dev, R, H, PQ * 3), dhw=dhw0.clone()), buf

    def attn(soa, zb_off=0, dzb_off=0):
        o, buf = outs(dzb_off)
        zbuf = torch.cat([torch.zeros(zb_off, device=dev), t["zb"].flatten()])
        part = _poison(dev, R, H)
        L.call("fd_ipa_attn_bwd", t["A"], o["dL"], (zbuf, zb_off), t["dfeats"], t["qp"], t["kp"], soa, t["hw"], (buf, dzb_off),
               o["dqp"], o["dkp"], o["dhw"], part, B, N)
        assert dzb_off == 0 or bool(torch.isnan(buf[:dzb_off]).all()), "written in front of dzb"
        return o, part

    fin = lambda o: dict(o, dhw=o["dhw"].double() - dhw0.double())
    o, part = attn(t["kpT"])                                   # N <= 128 / <= 256: the slab kernels; else direct reads
    _check(c, "attn", fin(o), part)
    o_aos, part_aos = attn(None)
    _check(c, "attn_kp", fin(o_aos), part_aos)
    if N <= 256:                                               # an unaligned zb or dzb: the direct-read kernel of <= 256
        for name, kw in (("zb", dict(zb_off=1)), ("dzb", dict(dzb_off=1))):
            ou, pu = attn(t["kpT"], **kw)
            assert not _differ(dict(o, part=part), dict(ou, part=pu), dev), f"unaligned {name}: not bit-identical to the slab kernel"
            _check(c, "attn_unaligned", fin(ou), pu)
    # fd_ipa_opair_bwd -> fd_ipa_softmax_bwd (network.ipa_bwd without sv["fused_attn"])
    u, _ = outs()
    upart = _poison(dev, R, H)
    L.call("fd_ipa_opair_bwd", t["A"], t["zb"], t["dfeats"], u["dL"], u["dzb"], B, N)
    L.call("fd_ipa_softmax_bwd", t["A"], u["dL"], t["qp"], t["kp"], t["hw"], u["dzb"], u["dqp"], u["dkp"], u["dhw"], upart, B, N)
    _check(c, "unfused", fin(u), upart)
    # (bit-identical on the interpreter and on the MI355X in every case)
    assert not _differ(dict(o_aos, part=part_aos), dict(u, part=upart), dev), "the unfused pair differs from fd_ipa_attn_bwd (kp_soa = None)"


def _path_kpts(dev, spec):
    L = ops.lib()
    c = _case(spec)
    t = _to(c, dev)
    dkp = _poison(dev, c["B"] * c["N"], H, PQ * 3)
    L.call("fd_ipa_kpts_bwd", c["ref"]["dL"].float().to(dev), t["qp"], t["kp"], t["hw"], dkp, c["B"], c["N"])
    _check(c, "kpts", dict(dkp=dkp))


@pytest.mark.parametrize("spec", EMU_CASES, ids=_id)
def test_flash_bwd_emu(use_emu, spec):
    _path_flash("cpu", spec)


@pytest.mark.parametrize("spec", EMU_CASES, ids=_id)
def test_attn_bwd_emu(use_emu, spec):
    _path_attn("cpu", spec)


@pytest.mark.parametrize("spec", EMU_CASES, ids=_id)
def test_kpts_bwd_emu(use_emu, spec):
    _path_kpts("cpu", spec)


@pytest.mark.gpu
@pytest.mark.parametrize("spec", GPU_CASES, ids=_id)
def test_flash_bwd_gpu(hip_lib, spec):
    with parity_log.case("ipa_bwd_flash"):
        _path_flash("cuda", spec)


@pytest.mark.gpu
@pytest.mark.parametrize("spec", GPU_CASES, ids=_id)
def test_attn_bwd_gpu(hip_lib, spec):
    with parity_log.case("ipa_bwd_attn"):
        _path_attn("cuda", spec)


@pytest.mark.gpu
@pytest.mark.parametrize("spec", GPU_CASES, ids=_id)
def test_kpts_bwd_gpu(hip_lib, spec):
    with parity_log.case("ipa_bwd_kpts"):
        _path_kpts("cuda", spec)


# ------------------------------------------------------------------------------------------------------------------ fd_ipa_dz_acc
def _run_dz_acc(dev, rows, seed):
    """dz[p] (+)= dzb[p] W40 over `rows` pair rows, against float64; bound 8 x the error of a float32 torch.matmul, <= 1e-5.
    dz has guard rows behind `rows` (a wave's last tile is 32 rows whatever `rows` is)."""
    L = ops.lib()
    g = torch.Generator().manual_seed(seed)
    dzb, W = torch.randn(rows, ZB, generator=g), torch.randn(ZB, 128, generator=g)
    old = torch.randn(rows, 128, generator=g)
    prod64 = dzb.double() @ W.double()
    prod32 = dzb @ W
    GUARD = 33
    for acc in (0, 1):
        ref = prod64 + old.double() if acc else prod64
        e32 = _relerr(prod32 + old if acc else prod32, ref)
        bound = min(8.0 * e32, 1e-5)
        dz = torch.full((rows + GUARD, 128), 7.0)
        dz[:rows] = old if acc else NAN
        dz = dz.to(dev)
        L.call("fd_ipa_dz_acc", dzb.to(dev), W.to(dev), dz, rows, acc)
        got = dz.cpu()
        assert bool(torch.isfinite(got).all()), (rows, acc)
        assert bool((got[rows:] == 7.0).all()), ("rows behind `rows` were written", rows, acc)
        err = _relerr(got[:rows], ref)
        parity_log.out(f"ipa_bwd.dz_acc.acc{acc}", err)
        print(f"[ipa_bwd] dz_acc rows={rows} accumulate={acc}: {err:.2e} | bound {bound:.2e} e32 {e32:.1e}")
        assert err <= bound, (rows, acc, err, bound)


@pytest.mark.parametrize("rows", [1, 31, 33, 70, 129])
def test_dz_acc_emu(use_emu, rows):
    _run_dz_acc("cpu", rows, rows)


# (2 * 400 * 400 = 320 000 > 262 144 = 2048 blocks x 4 waves x 32 rows: the only size at which the waves walk a second tile group)
@pytest.mark.gpu
@pytest.mark.parametrize("rows", [101 * 101, 2 * 400 * 400])
def test_dz_acc_gpu(hip_lib, rows):
    with parity_log.case("ipa_bwd_dz_acc"):
        _run_dz_acc("cuda", rows, rows)


# ------------------------------------------------------------------------------------------- properties at the benchmark sizes
@pytest.mark.gpu
@pytest.mark.parametrize("B,N", [(30, 128), (8, 512)])
def test_ipa_bwd_properties_full_size(hip_lib, B, N):
    """No float64 restatement at these sizes; of both backward paths on one forward:
    * sum_j dL[b, h, i, j] = 0 for every row (any softmax backward): |sum_j dL| <= 1e-5 sum_j |dL|;
    * dzb[:, :8] = sqrt(1/3) dL transposed to [b, i, j, h], within 2 ulp;
    * the columns of dL at masked keys of unmasked rows are exactly 0."""
    L = ops.lib()
    dev = "cuda"
    proj, quat, trans, zb, hw, mask = _inputs(dev, B, N, 31, 1.2)
    qp, kp, vp, kpT = _points(L, proj, quat, trans, B, N)
    R = B * N
    feats = torch.empty(R, LDF, device=dev)
    A = torch.empty(B, H, N, N, device=dev)
    L.call("fd_ipa_flash_fwd", proj, zb, qp, kp, vp, hw, mask, quat, trans, feats, A, B, N, 0)
    dfeats = torch.randn(R, LDF, generator=torch.Generator().manual_seed(131)).to(dev)
    m = mask.view(B, N) > 0
    dead = (m[:, None, :, None] & ~m[:, None, None, :]).expand(B, H, N, N)
    sq13 = torch.sqrt(torch.tensor(1.0 / 3.0, device=dev))            # sqrtf(1.0f / 3.0f), as the kernels form it
    for path, out in (("sequence", _bwd_sequence(L, proj, quat, zb, hw, qp, kp, vp, kpT, A, feats, dfeats, B, N)),
                      ("flash", _bwd_flash(L, proj, quat, trans, zb, hw, qp, kp, vp, A, feats, dfeats, B, N))):
        dL = out["dL"]
        assert bool(torch.isfinite(dL).all()), path
        d = dL.double()
        worst = float((d.sum(-1).abs() / d.abs().sum(-1).clamp_min(1e-300)).max())
        assert bool((d.sum(-1).abs() <= 1e-5 * d.abs().sum(-1)).all()), (path, worst)
        want = (dL * sq13).permute(0, 2, 3, 1).reshape(R * N, H)
        got = out["dzb"][:, :H]
        ulp = torch.nextafter(want.abs(), torch.full_like(want, float("inf"))) - want.abs()
        # (in fact bit-equal on both paths at both sizes on the MI355X: the kernels form the same fp32 product)
        exact = bool(torch.equal(got, want))
        assert bool(((got - want).abs() <= 2 * ulp).all()), path
        assert bool((dL[dead] == 0).all()), path
        print(f"[ipa_bwd] properties {path} B={B} N={N}: worst |sum dL| / sum |dL| {worst:.2e}, dzb[:, :8] bit-equal: {exact}")
