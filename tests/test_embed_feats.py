"""Kernel-level checks of the embedder's per-residue features and of the fused edge embedder's strided node terms:
fd_node_feats_ld (the [R, 65] features of score_network.py:14-47,97-126 at a row stride >= 65, zero columns behind them) against
fd_node_feats and a float64 restatement; fd_edge_embed reading p | q as the column halves of one [R, 256] buffer
(FdEdgeEmbedDesc.ld_pq) against two dense [R, 128] tensors, bit for bit.

Against references that are not the kernels themselves (model/score_network.py:67-101,129-153, data/utils.py:570-580):

  fd_edge_feats   all 120 columns against the oracle's float32 `edge_features` (the reference's own op sequence: its bin decisions,
                  its sin / cos arguments).  Distogram columns exactly equal on the constructed inputs (`edge_inputs`); on random
                  inputs at most 1e-6 of the bins may differ (sqrtf against torch.linalg.norm: one ulp), an allowance first shown
                  to cover the oracle alone: pairs whose float32 distance lies within 2 ulp of a bin edge are <= 1e-6 of the bins.
                  The other columns: 4 * 2^-24 absolute -- two float32 sin / cos of bit-identical arguments, each within 2 ulp of
                  a value <= 1.
  fd_edge_embed   out, h1, h2, h3, mean, rstd, zb against the MLP / LayerNorm / mask / W40 layer in float64 on the oracle's float32
                  features (`_ee_ref`); mask1 / mask2 bit-equal to h1 > 0 / h2 > 0 of the kernel's own saves and, fed to
                  ops.edge_embed_bwd, bit-identical to the launch that reads h1 / h2; launches without the optional outputs and
                  without zb write the same `out` bit for bit; NaN pre-fill, guard rows behind `rows` untouched.
  fd_rowscale, network.pair_mask   exactly m_i * m_j / x * s.

`edge_inputs`: B >= 2 (the batch offset of j), an index gap of +200 in mid-chain, one chain offset by +1500, seq_idx = 0 on a padded
tail, one backbone with sc_ca all zero (every distance 0 < min_bin: no bin), one with residues on the x axis at the float32
linspace(1e-5, 20, 22) edges (distances that EQUAL an edge: both strict comparisons fail), a residue 30 A away (last bin), a row
scale with zeros.

ReLU gates (`gated_tail`): a hidden unit whose float64 pre-activation lies within 1e-5 of its tensor's maximum of zero takes its
gate from what the code under test saved, every other unit uses pre > 0; the share of such units (from the float64 reference alone)
is at most 1e-4 and the code's activation there at most 1e-4 of its tensor's maximum.

Bounds: error = max |got - ref| / max |ref| per tensor; the same restatement in float32 torch (same gates) gives the float32 noise
e32 of a case, the bound is min(8 max_k e32_k, 2e-5) (the rule of tests/test_ipa_bwd.py; 2e-5: the LayerNorm bound of
tests/test_edge_mlp.py).  Nothing is derived from what the kernels give.

Achieved (worst case of a tier, `parity_log` keys edge_embed.<tensor>, edge_feats.<block>):

  tensor                       interpreter   MI355X
  fd_edge_feats                distogram bins that differ 0 / 0; columns 0..65 6.0e-8 / 6.0e-8; relative-index columns 6.0e-8 / 6.0e-8 (absolute)
  fd_edge_embed  h1            6.0e-7        2.7e-7
                 h2            7.8e-7        5.2e-7
                 h3            8.1e-7        5.5e-7
                 mean          1.0e-6        5.8e-7
                 rstd          2.8e-7        2.7e-7
                 out           8.7e-7        5.3e-7
                 zb            1.2e-6        6.4e-7
  bounds of the cases          2.6e-6 (B=1 x N=9) ... 4.5e-6   4.1e-6 ... 5.3e-6
  units on a borrowed gate     <= 4.8e-5     <= 6.6e-5 of the units of a case (cap 1e-4)
"""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import parity_log  # noqa: E402
from oracle import framediff_oracle as fo  # noqa: E402
from se3_diffusion_amd import network as nw, ops  # noqa: E402
from se3_diffusion_amd.ops import lib  # noqa: E402

NAN = float("nan")
CAP = 2e-5                                   # the LayerNorm bound of tests/test_edge_mlp.py and tests/test_edge_embed_bwd.py
GATE_MARGIN, GATE_SHARE = 1e-5, 1e-4         # (the share: the figure of tests/test_edge_mlp.py)
GUARD = 3                                    # rows behind `rows` that a launch must leave alone
SENTINEL = 0x5A5A5A5A


def _node_feats(dev, B, N, seed):
    g = torch.Generator().manual_seed(seed)
    seq = torch.arange(N).repeat(B, 1).reshape(-1).to(torch.int64).to(dev)
    t = torch.rand(B, generator=g)
    tscaled = (t * 10000).float().to(dev)
    fixed = (torch.rand(B * N, generator=g) > 0.7).float().to(dev)
    tfreq, idenom, _, _ = ops.feature_tables(torch.device(dev))
    a = torch.full((B * N, 65), float("nan"), device=dev)
    lib().call("fd_node_feats", seq, tscaled, fixed, tfreq, idenom, a, B, N)
    b = torch.full((B * N, 72), float("nan"), device=dev)
    lib().call("fd_node_feats_ld", seq, tscaled, fixed, tfreq, idenom, b, 72, B, N)
    assert torch.equal(b[:, :65], a) and float(b[:, 65:].abs().max()) == 0.0
    # float64: [sin | cos](t 1e4 freq) (32), fixed (1), [sin | cos](idx pi / denom) (32)
    tf, idn = tfreq.double().cpu().numpy(), idenom.double().cpu().numpy()
    ts = tscaled.double().cpu().numpy().repeat(N)
    arg = ts[:, None] * tf[None, :]
    idx = seq.double().cpu().numpy()
    ia = idx[:, None] * math.pi / idn[None, :]
    ref = np.concatenate([np.sin(arg), np.cos(arg), fixed.double().cpu().numpy()[:, None], np.sin(ia), np.cos(ia)], 1)
    # (float32 sin / cos of arguments up to 1e4: the argument's own rounding, 1e4 * 2^-24, bounds the agreement)
    assert float(np.abs(a.double().cpu().numpy() - ref).max()) < 2e-3
    assert float(np.abs(a.double().cpu().numpy()[:, 32:] - ref[:, 32:]).max()) < 2e-5


def _edge_embed_strided(dev, B, N, seed):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc).to(dev)
    R, P = B * N, B * N * N
    W0, W2, W4 = rn(128, 120, sc=0.1), rn(128, 128, sc=0.1), rn(128, 128, sc=0.1)
    img = ops.edge_embed_pack(W0, W2, W4)
    seq = torch.arange(N).repeat(B, 1).reshape(-1).to(torch.int64).to(dev)
    sc_ca = rn(R, 3, sc=5.0)
    _, idenom, lower, upper = ops.feature_tables(torch.device(dev))
    pq = rn(R, 256, sc=0.5)
    p, q = pq[:, :128].contiguous(), pq[:, 128:].contiguous()
    b2, b3, gm, bt = rn(128, sc=0.2), rn(128, sc=0.2), 1 + rn(128, sc=0.1), rn(128, sc=0.1)
    outs = []
    for strided in (False, True):
        out = torch.full((P, 128), float("nan"), device=dev)
        if strided:
            ops.edge_embed(seq, sc_ca, idenom, lower, upper, img, pq, pq[:, 128:], b2, b3, gm, bt, out, P, N, ld_pq=256)
        else:
            ops.edge_embed(seq, sc_ca, idenom, lower, upper, img, p, q, b2, b3, gm, bt, out, P, N)
        outs.append(out)
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])


def test_node_feats_ld_emu(use_emu):
    _node_feats("cpu", 2, 9, 0)


def test_edge_embed_ld_pq_emu(use_emu):
    _edge_embed_strided("cpu", 1, 9, 1)


@pytest.mark.gpu
def test_embed_feats_gpu(hip_lib):
    _node_feats("cuda", 3, 50, 2)
    _edge_embed_strided("cuda", 2, 40, 3)
    _edge_embed_strided("cuda", 1, 128, 4)


# ------------------------------------------------------------------------------------------------ inputs and references
def edge_inputs(B, N, seed):
    """The embedder inputs of this file and of tests/test_stages.py (CPU tensors, keys of the feature dict) -- see the docstring."""
    g = torch.Generator().manual_seed(seed)
    seq = torch.arange(1, N + 1).repeat(B, 1)
    seq[0, N // 2:] += 200                                    # a chain break in mid-chain
    seq[B - 1] += 1500                                        # large residue numbers
    mask = torch.ones(B, N)
    mask[0, N - 2:] = 0.0                                     # a padded tail: seq_idx = 0 there
    seq[0, N - 2:] = 0
    edges = torch.linspace(1e-5, 20.0, 22)
    sc = torch.zeros(B, N, 3)
    for b in range(B):
        kind = ("axis", "zero", "random")[b % 3]
        if kind == "axis":
            # residue 0 at the origin, residues 1..m ON bin edges of the x axis, one residue 30 A behind the origin (every distance
            # to it > 20: the last bin), the rest generic and far from the axis
            m = min(N - 2, 22)
            sc[b, 1:1 + m, 0] = edges[torch.linspace(0, 21, m).round().long()]
            sc[b, 1 + m, 0] = -30.0
            if N > 2 + m:
                sc[b, 2 + m:] = 6.0 * torch.randn(N - 2 - m, 3, generator=g) + torch.tensor([0.0, 15.0, 0.0])
        elif kind == "random":
            sc[b] = 5.0 * torch.randn(N, 3, generator=g)
    return dict(seq_idx=seq.contiguous(), t=(0.05 + 0.9 * torch.rand(B, generator=g)).float(), res_mask=mask,
                fixed_mask=(torch.rand(B, N, generator=g) > 0.7).float(), sc_ca_t=sc.contiguous())


def random_inputs(B, N, seed):
    """generic inputs: seq_idx = 1..N, a self-conditioning trace of independent normal positions"""
    g = torch.Generator().manual_seed(seed)
    return dict(seq_idx=torch.arange(1, N + 1).repeat(B, 1).contiguous(), t=(0.05 + 0.9 * torch.rand(B, generator=g)).float(),
                res_mask=torch.ones(B, N), fixed_mask=(torch.rand(B, N, generator=g) > 0.7).float(),
                sc_ca_t=(6.0 * torch.randn(B, N, 3, generator=g)).contiguous())


def relerr(got, ref):
    """max |got - ref| / max |ref|; an analytically zero reference is compared against an absolute floor of 1e-9 instead"""
    ref = ref.detach().double().cpu()
    return float((got.detach().double().cpu() - ref).abs().max()) / max(float(ref.abs().max()), 1e-9)


def borrow_gate(pre, kernel_gate, stats):
    """The ReLU gate of a float64 pre-activation tensor: pre > 0, except within GATE_MARGIN of the tensor maximum of zero, where
    two correct float32 implementations may differ and the gate is the code's own (kernel_gate, bool; None: nothing to borrow).
    stats collects (units inside the margin, units, the margin mask) per tensor."""
    pre = pre.detach()
    margin = pre.abs() < GATE_MARGIN * pre.abs().max()
    stats.append((int(margin.sum()), margin.numel(), margin))
    return pre > 0 if kernel_gate is None else torch.where(margin, kernel_gate.to(margin.device), pre > 0)


def check_gate_stats(stats, kernel_acts):
    """at most GATE_SHARE of the units take the borrowed gate, and the code's activation at each is <= 1e-4 of its tensor maximum"""
    inside, units = sum(s[0] for s in stats), sum(s[1] for s in stats)
    assert inside <= GATE_SHARE * units, (inside, units)
    for (n, _, margin), h in zip(stats, kernel_acts):
        h = h.detach().double().cpu()
        if n:
            assert float(h[margin].abs().max()) <= 1e-4 * float(h.abs().max()), (n, float(h[margin].abs().max()))
    return inside / max(units, 1)


def gated_tail(pre1, w, rowscale, kgates=None, gates=None, stats=None):
    """relu -> Linear -> relu -> Linear -> LayerNorm (* rowscale) behind the first layer's pre-activation pre1, in pre1's dtype
    (autograd passes through).  w = (W2, b2, W4, b4, gamma, beta).  kgates = (g1, g2): the code's own gates, borrowed inside the
    margin (float64 pass); gates = (g1, g2): fixed gates (the float32 pass reuses the float64 pass's).  Returns the tensors by name
    and the gates used."""
    W2, b2, W4, b4, gamma, beta = w
    g1 = gates[0] if gates is not None else borrow_gate(pre1, kgates[0], stats)
    h1 = pre1 * g1.to(pre1.dtype)
    pre2 = h1 @ W2.T + b2
    g2 = gates[1] if gates is not None else borrow_gate(pre2, kgates[1], stats)
    h2 = pre2 * g2.to(pre1.dtype)
    h3 = h2 @ W4.T + b4
    mean = h3.mean(-1, keepdim=True)
    var = ((h3 - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + 1e-5)
    out = ((h3 - mean) * rstd * gamma + beta) * rowscale[:, None]
    return dict(h1=h1, h2=h2, h3=h3, mean=mean[:, 0], rstd=rstd[:, 0], out=out), (g1, g2)


@functools.lru_cache(maxsize=None)
def _ee_case(B, N, seed):
    """inputs, weights and the oracle's float32 features of one fused-embedder case (CPU tensors, shared and left unchanged)"""
    f = edge_inputs(B, N, seed)
    g = torch.Generator().manual_seed(seed + 1000)
    rn = lambda *s, sc=1.0: torch.randn(*s, generator=g) * sc
    R, P = B * N, B * N * N
    c = dict(f, B=B, N=N, W0=rn(128, 120, sc=0.1), b0=rn(128, sc=0.1), W2=rn(128, 128, sc=0.1), b2=rn(128, sc=0.2),
             W4=rn(128, 128, sc=0.1), b4=rn(128, sc=0.2), gamma=1 + rn(128, sc=0.1), beta=rn(128, sc=0.1),
             W40=rn(40, 128, sc=0.1), b40=rn(40, sc=0.3), dy=rn(P, 128))
    c["ef"] = fo.edge_features(f["seq_idx"], f["t"], f["fixed_mask"], f["sc_ca_t"]).reshape(P, 120)
    pt = fo.node_features(f["seq_idx"], f["t"], f["fixed_mask"])[1].reshape(R, 33).double()
    # the per-residue halves of the first layer, rounded ONCE: the same float32 values go to the kernel and (cast up) to the reference
    c["p"] = (pt @ c["W0"][:, :33].double().T + c["b0"].double()).float().contiguous()
    c["q"] = (pt @ c["W0"][:, 33:66].double().T).float().contiguous()
    m = f["res_mask"]
    c["emask"] = (m[:, :, None] * m[:, None, :]).reshape(-1).contiguous()
    return c


def _ee_ref(c, dt, kgates=None, gates=None, stats=None):
    B, N = c["B"], c["N"]
    row = torch.arange(B * N * N)
    qi = row // N
    qj = (qi // N) * N + row % N
    d = lambda k: c[k].to(dt)
    pre1 = d("p")[qi] + d("q")[qj] + d("ef")[:, 66:] @ d("W0")[:, 66:].T
    r, g = gated_tail(pre1, tuple(d(k) for k in ("W2", "b2", "W4", "b4", "gamma", "beta")), d("emask"), kgates, gates, stats)
    r["zb"] = r["out"] @ d("W40").T + d("b40")
    return r, g


# ------------------------------------------------------------------------------------------------ fd_edge_feats
def _edge_feats(dev, B, N, seed, constructed):
    f = edge_inputs(B, N, seed) if constructed else random_inputs(B, N, seed)
    P = B * N * N
    ref = fo.edge_features(f["seq_idx"], f["t"], f["fixed_mask"], f["sc_ca_t"]).reshape(P, 120)
    nbins = P * 22
    if not constructed:
        # the allowance covers the oracle alone: float32 distances within 2 ulp of a bin edge
        sc = f["sc_ca_t"]
        dist = torch.linalg.norm(sc[:, :, None, :] - sc[:, None, :, :], dim=-1).reshape(-1, 1)
        edges = torch.linspace(1e-5, 20.0, 22)
        ulp = torch.nextafter(edges, torch.full_like(edges, float("inf"))) - edges
        near = int(((dist - edges[None]).abs() <= 2 * ulp[None]).sum())
        assert near <= 1e-6 * nbins, (near, nbins)
    tfreq, idenom, lower, upper = ops.feature_tables(torch.device(dev))
    ef = torch.full((P + GUARD, 120), NAN, device=dev)
    to = lambda x: x.to(dev).contiguous()
    lib().call("fd_edge_feats", to(f["seq_idx"]), to((f["t"] * 10000).float()), to(f["fixed_mask"]), to(f["sc_ca_t"]), tfreq, idenom,
               lower, upper, ef, B, N)
    got = ef.cpu()
    assert torch.isnan(got[P:]).all() and torch.isfinite(got[:P]).all()
    got = got[:P]
    with parity_log.case(f"edge_feats dev={dev} B={B} N={N} seed={seed} constructed={constructed}"):
        differ = int((got[:, 98:] != ref[:, 98:]).sum())
        parity_log.out("edge_feats.dgram_mismatch", differ)
        assert differ <= (0 if constructed else int(1e-6 * nbins)), (differ, nbins)
        for name, lo, hi in (("node", 0, 66), ("relpos", 66, 98)):
            err = float((got[:, lo:hi] - ref[:, lo:hi]).abs().max())
            parity_log.out(f"edge_feats.{name}", err)
            assert err <= 4 * 2.0 ** -24, (name, err)
    if constructed:
        # the cases the inputs were built for are there: a backbone without any bin, on-edge pairs without a bin beside pairs with one,
        # the last bin
        dg = ref[:, 98:].reshape(B, N, N, 22)
        assert float(dg[:, :, :, 21].sum()) > 0
        assert float(dg[0, 0, 1:min(N - 2, 22) + 1].sum()) == 0 and float(dg[0, 1, 2:4].sum()) == 2
        if B >= 2:
            assert float(dg[1].sum()) == 0


# ------------------------------------------------------------------------------------------------ fd_edge_embed
def _unpack_gates(words):
    """[rows, 4] int32 sign words -> [rows, 128] bool: bit 4 nb + e of word (row, g) is unit 16 nb + 4 g + e"""
    unit = torch.arange(128)
    nb, gg, ee = unit // 16, (unit % 16) // 4, unit % 4
    w = words.cpu().long() & 0xFFFFFFFF
    return ((w[:, gg] >> (4 * nb + ee)) & 1).bool()


def _edge_embed(dev, B, N, seed, blocks=0):
    c = _ee_case(B, N, seed)
    P = B * N * N
    to = lambda x: x.to(dev).contiguous()
    _, idenom, lower, upper = ops.feature_tables(torch.device(dev))
    k = {n: to(c[n]) for n in ("seq_idx", "sc_ca_t", "p", "q", "W0", "W2", "W4", "b2", "b4", "gamma", "beta", "W40", "b40", "emask", "dy")}
    full = lambda *cols: torch.full((P + GUARD,) + cols, NAN, device=dev)
    words = lambda: torch.full((P + GUARD, 4), SENTINEL, dtype=torch.int32, device=dev)

    def launch(zb, saves):
        o = dict(out=full(128))
        kw = {}
        if saves:
            o.update(h1=full(128), h2=full(128), h3=full(128), mean=full(), rstd=full(), mask1=words(), mask2=words())
            kw = {n: o[n] for n in ("h1", "h2", "h3", "mean", "rstd", "mask1", "mask2")}
        if zb:
            o["zb"] = full(40)
            kw.update(zb_out=o["zb"], zb_bias=k["b40"])
        img = ops.edge_embed_pack(k["W0"], k["W2"], k["W4"], W40=k["W40"] if zb else None)
        ops.edge_embed(k["seq_idx"], k["sc_ca_t"], idenom, lower, upper, img, k["p"], k["q"], k["b2"], k["b4"], k["gamma"], k["beta"],
                       o["out"], P, N, blocks=blocks, rowscale=k["emask"], **kw)
        for n, t in o.items():          # every row written, no row behind `rows` touched
            if t.dtype == torch.int32:
                assert bool((t[P:] == SENTINEL).all()), n
            else:
                assert bool(torch.isnan(t[P:]).all()) and bool(torch.isfinite(t[:P]).all()), n
        return {n: t[:P] for n, t in o.items()}

    o = launch(zb=True, saves=True)
    assert float(o["out"][k["emask"] == 0].abs().max()) == 0.0
    # packed gates = the signs of the kernel's own saves
    kg1, kg2 = (o["h1"] > 0).cpu(), (o["h2"] > 0).cpu()
    assert torch.equal(_unpack_gates(o["mask1"]), kg1) and torch.equal(_unpack_gates(o["mask2"]), kg2)
    stats = []
    ref, gates = _ee_ref(c, torch.float64, kgates=(kg1, kg2), stats=stats)
    share = check_gate_stats(stats, (o["h1"], o["h2"]))
    ref32, _ = _ee_ref(c, torch.float32, gates=gates)
    e32 = {n: relerr(ref32[n], ref[n]) for n in ref}
    bound = min(8 * max(e32.values()), CAP)
    with parity_log.case(f"edge_embed dev={dev} B={B} N={N} seed={seed} blocks={blocks}"):
        parity_log.out("edge_embed.bound", bound)
        parity_log.out("edge_embed.borrowed_share", share)
        errs = {}
        for n in ref:
            errs[n] = relerr(o[n], ref[n])
            parity_log.out(f"edge_embed.{n}", errs[n])
        print(f"[edge_embed] B={B} N={N} bound {bound:.2e} e32 {e32} errs {errs}")
        assert max(errs.values()) < bound, (errs, bound, e32)
    # the optional outputs change nothing: without the saves, and without zb
    assert torch.equal(launch(zb=True, saves=False)["out"], o["out"])
    assert torch.equal(launch(zb=False, saves=False)["out"], o["out"])
    o2 = launch(zb=False, saves=True)
    assert all(torch.equal(o2[n], o[n]) for n in o2)
    # the backward gated on the packed words against the backward that reads h1 / h2: bit-identical
    imgb = ops.edge_embed_bwd_pack(k["W2"], k["W4"])
    res = []
    for packed in (False, True):
        d3, d2, d1 = (torch.full((P, 128), NAN, device=dev) for _ in range(3))
        dg, db = torch.zeros(128, device=dev), torch.zeros(128, device=dev)
        hk = dict(gmask2=o["mask2"].contiguous(), gmask1=o["mask1"].contiguous()) if packed else {}
        ops.edge_embed_bwd(k["dy"], o["h3"].contiguous(), o["mean"].contiguous(), o["rstd"].contiguous(), k["gamma"], k["emask"],
                           None if packed else o["h2"].contiguous(), None if packed else o["h1"].contiguous(), imgb, d3, d2, d1, dg, db,
                           P, blocks=blocks, **hk)
        res.append((d3, d2, d1, dg, db))
    assert all(torch.isfinite(t).all() for t in res[0])
    assert all(torch.equal(a, b) for a, b in zip(res[0][:3], res[1][:3]))


def _pair_mask(dev, B, N, seed):
    g = torch.Generator().manual_seed(seed)
    m = (torch.rand(B, N, generator=g) > 0.3).float()
    m[0, -1] = 0.0
    assert torch.equal(nw.pair_mask(m.to(dev), B, N).cpu(), (m[:, :, None] * m[:, None, :]).reshape(-1))
    rows, cols, ld = B * N, 37, 41
    x = torch.randn(rows + GUARD, ld, generator=g)
    s = torch.randn(rows, generator=g) * (torch.rand(rows, generator=g) > 0.3)
    y = torch.full((rows + GUARD, ld), NAN, device=dev)
    lib().call("fd_rowscale", x.to(dev), ld, s.to(dev), y, ld, rows, cols)
    y = y.cpu()
    assert torch.equal(y[:rows, :cols], x[:rows, :cols] * s[:, None])
    assert torch.isnan(y[rows:]).all() and torch.isnan(y[:, cols:]).all()


EMU_EMBED = ((1, 9, 20, 0), (2, 11, 21, 1), (2, 23, 22, 3))        # (B, N, seed, blocks): the issue's shape table
GPU_EMBED = ((2, 11, 21, 1), (2, 37, 23, 0), (3, 50, 24, 5), (1, 128, 25, 0))
_eid = lambda c: f"B{c[0]}N{c[1]}"


@pytest.mark.parametrize("case", EMU_EMBED, ids=_eid)
def test_edge_embed_ref_emu(use_emu, case):
    _edge_embed("cpu", *case)


def test_edge_feats_emu(use_emu):
    _edge_feats("cpu", 2, 11, 21, constructed=True)
    _edge_feats("cpu", 3, 24, 26, constructed=True)            # all 22 edges on the axis
    _edge_feats("cpu", 2, 23, 27, constructed=False)


def test_pair_mask_emu(use_emu):
    _pair_mask("cpu", 2, 9, 30)


@pytest.mark.gpu
@pytest.mark.parametrize("case", GPU_EMBED, ids=_eid)
def test_edge_embed_ref_gpu(hip_lib, case):
    _edge_embed("cuda", *case)


@pytest.mark.gpu
def test_edge_feats_gpu(hip_lib):
    _edge_feats("cuda", 2, 11, 21, constructed=True)
    _edge_feats("cuda", 3, 50, 24, constructed=True)
    _edge_feats("cuda", 3, 50, 28, constructed=False)


@pytest.mark.gpu
def test_pair_mask_gpu(hip_lib):
    _pair_mask("cuda", 2, 9, 30)
    _pair_mask("cuda", 3, 50, 31)
