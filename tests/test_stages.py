"""The stages of network.py / trunk.py one at a time against float64 autograd: the glue around the kernels -- which operand goes to
which launch, column offsets of concat-linears, accumulate-or-assign, side-stream and grouped weight gradients -- at a bound
100-1000 x tighter than the whole-network parity tests can hold.

  embed            network.embed_fwd -> embed_regen_early -> embed_bwd -> ops.flush_dw / join_grad_stream against `_mlp3_ln` on the
                   oracle's float32 features (x node mask / pair mask): node, edge, zb, the 16 gradients of embedding_layer.*;
                   forward only: the sampling path (cache, save=False: fd_node_feats_ld at stride 72, p | q as one product)
  edge_transition  trunk.edge_transition_fwd / edge_transition_bwd against EdgeTransition.forward (x pair mask), upstream gradient
                   dz2 + dzb W40: z', zb, dz (over a NaN pre-fill), dn3 (initial value + gradient), the 10 parameter gradients, on
                   backward paths (i) / (ii) / (iii), grouped and ungrouped weight gradients, both tile shapes, the dynamic tile
                   hand-out, with / without zb_next and dzb_next, dz2 = None; forward only: folded node terms, column-split kernel
  ln_skip, tfmr_layer, post_node   the per-residue stages against fo.tfmr_layer, fo.node_transition and the Linear + LayerNorm
                   lines of ipa_pytorch.py:632-640: outputs, dx, every parameter gradient; accumulated outputs (dinit, du0[:, :256])
                   as initial value + gradient; tfmr_layer with the fused attention forced on (seq_attn_min_rows=0), with
                   fused_seq_attn=False and with fused_seq_attn_bwd=False, padded keys in key_add = 1 - mask

Inputs of the embedder: tests/test_embed_feats.py `edge_inputs` (index gaps, large residue numbers, seq_idx = 0, distances on bin
edges, 0 and beyond the last bin).

ReLU gates: the float64 restatements take the gate of a unit whose pre-activation lies within 1e-5 of its tensor maximum of zero
from what the stage saved (h > 0, or the packed sign words of the fused edge transition), pre > 0 elsewhere; at most 1e-4 of the
units may do so and the stage's activation there is at most 1e-4 of its tensor maximum (test_embed_feats.check_gate_stats).  Every
stage here saves its gates; the forward-only sampling forms compare values only, where the reference's own gate is the right one.

Bounds: error = max |got - ref| / max |ref| per tensor (floor 1e-9 for an analytically zero reference).  The same restatement
with the same gates in float32 torch gives the float32 noise e32 of every tensor of a case; the bound of the case is
min(8 max_k e32_k, 2e-5) -- the rule of tests/test_ipa_bwd.py, capped at the LayerNorm bound of tests/test_edge_mlp.py.  Nothing
is derived from what the code under test gives.

Achieved (worst tensor of the worst case of a tier; `parity_log` keys <stage>.<tensor>, gradients under their parameter family):

  stage             interpreter                      MI355X
  embed             node 3.2e-7  edge 6.9e-7  zb 1.0e-6   node 3.2e-7  edge 4.0e-7  zb 4.9e-7
                    gradients: node_embedder 3.1e-7, edge_embedder 7.1e-7 | 3.7e-7, 7.8e-7         bounds 6.0e-6 | 3.6e-6 ... 4.0e-6
    sampling path   node 2.8e-7  edge 7.2e-7  zb 9.7e-7   node 2.7e-7  edge 3.9e-7  zb 4.4e-7
  edge_transition   z' 1.0e-6  zb 7.9e-7  dz 1.6e-6       z' 6.3e-7  zb 4.8e-7  dz 1.2e-6
                    dn3 4.3e-7  gradients 9.2e-7          dn3 3.7e-7  gradients 1.7e-6             bounds 5.6e-6 ... 7.0e-6 | 4.0e-6 ... 7.2e-6
    sampling forms  z' 8.8e-7  zb 8.0e-7                  z' 6.9e-7  zb 3.6e-7
  ln_skip           u0 1.9e-7  dx1 1.6e-7  dinit 6.5e-8   u0 1.8e-7  dx1 1.2e-7  dinit 6.3e-8
                    gradients 1.0e-7                      gradients 2.4e-7                         bounds 3.5e-6 | 2.3e-6 ... 2.6e-6
  tfmr_layer        y 2.3e-7  dx 2.9e-7  gradients 3.6e-7   y 2.4e-7  dx 2.8e-7  gradients 4.7e-7    bounds 4.7e-6 | 4.7e-6 ... 4.9e-6
  post_node         n3 2.1e-7  du2 2.4e-7  du0 1.2e-7     n3 2.2e-7  du2 3.0e-7  du0 1.3e-7
                    gradients 2.8e-7                      gradients 5.6e-7                         bounds 5.2e-6 | 3.1e-6 ... 3.3e-6
  No case needs the 2e-5 cap on either tier: every bound above is 8 x the float32 noise of its case.
"""
import functools
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import parity_log  # noqa: E402
from oracle import framediff_oracle as fo  # noqa: E402
from se3_diffusion_amd import network as nw, ops, options, trunk  # noqa: E402
from test_embed_feats import CAP, NAN, borrow_gate, check_gate_stats, edge_inputs, relerr  # noqa: E402

T = "score_model.trunk"


# ------------------------------------------------------------------------------------------------ shared machinery
class Gates:
    """The ReLU of a restatement: relu(pre) = pre * gate with the gates of test_embed_feats.borrow_gate.  kernel: the stage's own
    gates in call order (None: pre > 0 everywhere); fixed: gates to reuse (the float32 pass takes the float64 pass's)."""

    def __init__(self, kernel=None, fixed=None):
        self.kernel, self.fixed, self.used, self.stats = kernel, fixed, [], []

    def __call__(self, pre):
        i = len(self.used)
        g = self.fixed[i] if self.fixed is not None else borrow_gate(pre, None if self.kernel is None else self.kernel[i], self.stats)
        self.used.append(g)
        return pre * g.to(pre.dtype)


def _autograd(fn, leaves, consts, dt, relu):
    """fn(leaves, consts, relu) -> (outputs, loss) in dtype dt; returns the outputs and `d<leaf>` for every leaf, float64"""
    Lf = {k: v.to(dt).clone().requires_grad_(True) for k, v in leaves.items()}
    Cs = {k: (v.to(dt) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in consts.items()}
    outs, loss = fn(Lf, Cs, relu)
    loss.backward()
    res = {k: v.detach().double() for k, v in outs.items()}
    res.update({"d:" + k: v.grad.detach().double() for k, v in Lf.items()})
    return res


class Reference:
    """float64 reference + float32 noise of one (case, variant), computed once with the reference's own gates and shared by every
    setting whose saved gates agree with them inside the margin (all of them, unless a unit sits there and flips); otherwise
    recomputed with the borrowed gates.  Nothing in it is modified after it is built."""

    def __init__(self, fn, leaves, consts):
        self.fn, self.leaves, self.consts = fn, leaves, consts
        self.relu = Gates()
        self.r64 = _autograd(fn, leaves, consts, torch.float64, self.relu)
        self.r32 = _autograd(fn, leaves, consts, torch.float32, Gates(fixed=self.relu.used))

    def for_gates(self, kernel_gates, kernel_acts):
        """(r64, r32) for a run that saved `kernel_gates` (bool tensors in ReLU order; kernel_acts: its activations)"""
        kernel_gates = [g.cpu() for g in kernel_gates]
        check_gate_stats(self.relu.stats, kernel_acts)
        same = all(torch.equal(kg[st[2]], rg[st[2]]) for kg, rg, st in zip(kernel_gates, self.relu.used, self.relu.stats))
        if same:
            return self.r64, self.r32
        relu = Gates(kernel=kernel_gates)
        r64 = _autograd(self.fn, self.leaves, self.consts, torch.float64, relu)
        check_gate_stats(relu.stats, kernel_acts)
        return r64, _autograd(self.fn, self.leaves, self.consts, torch.float32, Gates(fixed=relu.used))


def _compare(stage, what, got, r64, r32, names=None):
    """every tensor of `got` against r64 under the case's bound; names: key -> state_dict name of a parameter gradient"""
    keys = list(got)
    e32 = {k: relerr(r32[k], r64[k]) for k in keys}
    bound = min(8 * max(e32.values()), CAP)
    errs = {}
    with parity_log.case(f"{stage} {what}"):
        parity_log.out(f"{stage}.bound", bound)
        for k in keys:
            errs[k] = relerr(got[k], r64[k])
            if names and k in names:
                parity_log.grad(names[k], got[k].detach().double().cpu(), r64[k])
            else:
                parity_log.out(f"{stage}.{k}", errs[k])
        worst = max(errs, key=errs.get)
        print(f"[{stage}] {what}: bound {bound:.2e} worst {worst} {errs[worst]:.2e} (e32 {e32[worst]:.2e}, max e32 {max(e32.values()):.2e})")
        bad = {k: (v, e32[k]) for k, v in errs.items() if not v < bound}
        assert not bad, (stage, what, bound, bad)
    return errs


@functools.lru_cache(maxsize=None)
def _params(seed):
    return fo.synth_params(seed=seed, conf=dict(fo.CONF, num_blocks=2, tfmr_layers=1))


def _on(dev, P, prefix):
    return {k: v.to(dev) for k, v in P.items() if k.startswith(prefix)}


def _zeros_like(Pd, names):
    return {k: torch.zeros_like(Pd[k]) for k in names}


def _finish():
    ops.flush_dw()
    ops.join_grad_stream()
    if torch.cuda.is_available():
        torch.cuda.synchronize()


def _w40(P, pre):
    return (torch.cat([P[f"{pre}.linear_b.weight"], P[f"{pre}.down_z.weight"]], 0).contiguous(),
            torch.cat([P[f"{pre}.linear_b.bias"], P[f"{pre}.down_z.bias"]], 0).contiguous())


# ------------------------------------------------------------------------------------------------ embedder
NE, EE = "embedding_layer.node_embedder", "embedding_layer.edge_embedder"
EMBED_PARAMS = tuple(f"{pre}.{l}.{t}" for pre in (NE, EE) for l in (0, 2, 4, 5) for t in ("weight", "bias"))


def _embed_fn(Lf, Cs, relu):
    def mlp(pre, x, rowscale):
        h = relu(F.linear(x, Lf[f"{pre}.0.weight"], Lf[f"{pre}.0.bias"]))
        h = relu(F.linear(h, Lf[f"{pre}.2.weight"], Lf[f"{pre}.2.bias"]))
        h = F.linear(h, Lf[f"{pre}.4.weight"], Lf[f"{pre}.4.bias"])
        return F.layer_norm(h, h.shape[-1:], Lf[f"{pre}.5.weight"], Lf[f"{pre}.5.bias"]) * rowscale[:, None]
    # (ReLU order: node h1, node h2, edge h1, edge h2)
    node = mlp(NE, Cs["nf"], Cs["mask"])
    edge = mlp(EE, Cs["ef"], Cs["emask"])
    zb = edge @ Cs["W40"].T + Cs["b40"]
    return dict(node=node, edge=edge, zb=zb), (node * Cs["dnode"]).sum() + (edge * Cs["dedge"]).sum()


@functools.lru_cache(maxsize=None)
def _embed_case(B, N, seed):
    f = edge_inputs(B, N, seed)
    P = _params(seed)
    g = torch.Generator().manual_seed(seed + 500)
    R, Pn = B * N, B * N * N
    m = f["res_mask"]
    W40, b40 = _w40(P, f"{T}.ipa_0")
    consts = dict(nf=fo.node_features(f["seq_idx"], f["t"], f["fixed_mask"])[0].reshape(R, 65),
                  ef=fo.edge_features(f["seq_idx"], f["t"], f["fixed_mask"], f["sc_ca_t"]).reshape(Pn, 120),
                  mask=m.reshape(-1), emask=(m[:, :, None] * m[:, None, :]).reshape(-1), W40=W40, b40=b40,
                  dnode=torch.randn(R, 256, generator=g), dedge=torch.randn(Pn, 128, generator=g))
    return f, consts, Reference(_embed_fn, {k: P[k] for k in EMBED_PARAMS}, consts)


def _embed(dev, B, N, seed, **ov):
    f, consts, ref = _embed_case(B, N, seed)
    Pd = _on(dev, _params(seed), "embedding_layer")
    fd = {k: v.to(dev) for k, v in f.items()}
    W40, b40 = consts["W40"].to(dev), consts["b40"].to(dev)
    ops.reset_dw_queue()
    with options.override(**ov):
        node, edge, sv, zb = nw.embed_fwd(Pd, fd, B, N, zb_next=(W40, b40))
        assert (zb is not None) == bool(options.opts.fused_embed)
        G = _zeros_like(Pd, EMBED_PARAMS)
        nw.embed_regen_early(sv, G)
        nw.embed_bwd(Pd, G, sv, consts["dnode"].to(dev), consts["dedge"].to(dev))
        _finish()
    acts = [sv["node"]["h1"], sv["node"]["h2"], sv["edge"]["h1"], sv["edge"]["h2"]]
    r64, r32 = ref.for_gates([a > 0 for a in acts], acts)
    got = dict(node=node, edge=edge)
    if zb is not None:
        got["zb"] = zb
    got.update({"d:" + k: G[k] for k in EMBED_PARAMS})
    _compare("embed", f"dev={dev} B={B} N={N} {ov}", got, r64, r32, names={"d:" + k: k for k in EMBED_PARAMS})


def _embed_sampling(dev, B, N, seed):
    """forward only, as sampler.sample runs it: static-weight cache, no saves, the padded first layers (opts.embed_first_padded)"""
    f, consts, ref = _embed_case(B, N, seed)
    Pd = _on(dev, _params(seed), "embedding_layer")
    fd = {k: v.to(dev) for k, v in f.items()}
    cache = {}
    for _ in range(2):          # the second call reads the cached padded weights and image
        with options.override(embed_first_padded=True):
            node, edge, sv, zb = nw.embed_fwd(Pd, fd, B, N, cache=cache, save=False, zb_next=(consts["W40"].to(dev), consts["b40"].to(dev)))
        assert "embed_first" in cache and zb is not None and sv["edge"] is None
        _compare("embed_sampling", f"dev={dev} B={B} N={N}", dict(node=node, edge=edge, zb=zb), ref.r64, ref.r32)


EMBED_SETTINGS = (dict(), dict(fused_embed=False), dict(fused_embed_bwd=False), dict(packed_gates=False), dict(grad_stream=False))
_sid = lambda ov: "-".join(f"{k}={v}" for k, v in ov.items()) or "default"


@pytest.mark.parametrize("ov", EMBED_SETTINGS, ids=_sid)
def test_embed_stage_emu(use_emu, ov):
    _embed("cpu", 2, 11, 40, **ov)


def test_embed_stage_sampling_emu(use_emu):
    _embed_sampling("cpu", 2, 11, 40)


@pytest.mark.gpu
@pytest.mark.parametrize("ov", EMBED_SETTINGS, ids=_sid)
def test_embed_stage_gpu(hip_lib, ov):
    _embed("cuda", 2, 11, 40, **ov)
    _embed("cuda", 2, 37, 41, **ov)


@pytest.mark.gpu
def test_embed_stage_sampling_gpu(hip_lib):
    _embed_sampling("cuda", 2, 11, 40)
    _embed_sampling("cuda", 2, 37, 41)


# ------------------------------------------------------------------------------------------------ edge transition
ET = f"{T}.edge_transition_0"
ET_PARAMS = tuple(f"{ET}.{n}.{t}" for n in ("initial_embed", "trunk.0", "trunk.2", "final_layer", "layer_norm") for t in ("weight", "bias"))


def _et_fn(Lf, Cs, relu):
    """EdgeTransition.forward (ipa_pytorch.py:218-233) on flat pair rows, x pair mask; loss = <z', dz2 + dzb W40>"""
    B, N = Cs["B"], Cs["N"]
    row = torch.arange(B * N * N)
    qi = row // N
    qj = (qi // N) * N + row % N
    e = F.linear(Lf["n3"], Lf[f"{ET}.initial_embed.weight"], Lf[f"{ET}.initial_embed.bias"])
    x = torch.cat([Lf["z"], e[qi], e[qj]], -1)
    h = relu(F.linear(x, Lf[f"{ET}.trunk.0.weight"], Lf[f"{ET}.trunk.0.bias"]))
    h = relu(F.linear(h, Lf[f"{ET}.trunk.2.weight"], Lf[f"{ET}.trunk.2.bias"]))
    y = F.linear(h + x, Lf[f"{ET}.final_layer.weight"], Lf[f"{ET}.final_layer.bias"])
    z2 = F.layer_norm(y, y.shape[-1:], Lf[f"{ET}.layer_norm.weight"], Lf[f"{ET}.layer_norm.bias"]) * Cs["emask"][:, None]
    up = Cs["up"]
    return dict(z2=z2, zb=z2 @ Cs["W40"].T + Cs["b40"]), (z2 * up).sum()


@functools.lru_cache(maxsize=None)
def _et_case(B, N, seed, with_dzb, with_dz2):
    P = _params(seed)
    g = torch.Generator().manual_seed(seed + 700)
    R, Pn = B * N, B * N * N
    m = torch.ones(B, N)
    m[0, N - 2:] = 0.0
    t = dict(n3=torch.randn(R, 256, generator=g) * m.reshape(-1, 1), z=torch.randn(Pn, 128, generator=g),
             dz2=torch.randn(Pn, 128, generator=g), dzb=0.5 * torch.randn(Pn, 40, generator=g), dn3=torch.randn(R, 256, generator=g),
             emask=(m[:, :, None] * m[:, None, :]).reshape(-1).contiguous())
    W40, b40 = _w40(P, f"{T}.ipa_1")
    # the upstream gradient of z', formed in float64 and handed to both passes as a constant
    up = (t["dz2"].double() if with_dz2 else 0) + (t["dzb"].double() @ W40.double() if with_dzb else 0)
    consts = dict(B=B, N=N, emask=t["emask"], W40=W40, b40=b40, up=up)
    leaves = dict({k: P[k] for k in ET_PARAMS}, n3=t["n3"], z=t["z"])
    return t, consts, Reference(_et_fn, leaves, consts)


def _et_gates(sv):
    """the gates the forward saved: the packed sign words of the fused kernel (bit 4 nb + e of word (row, 4 c + g) is unit
    128 c + 16 nb + 4 g + e; its h2 save carries z), h > 0 of the unfused sequence"""
    if sv.get("mh1") is None:
        return [sv["h1"] > 0, sv["h2"] > 0]
    unit = torch.arange(384)
    c, nb, g, e = unit // 128, (unit % 128) // 16, (unit % 16) // 4, unit % 4
    return [((w.cpu().long() & 0xFFFFFFFF)[:, 4 * c + g] >> (4 * nb + e) & 1).bool() for w in (sv["mh1"], sv["mh2"])]


def _edge_transition(dev, B, N, seed, zb, with_dz2=True, dynamic=False, **ov):
    assert zb or with_dz2
    t, consts, ref = _et_case(B, N, seed, zb, with_dz2)
    Pd = _on(dev, _params(seed), ET)
    k = {n: v.to(dev).contiguous() for n, v in t.items()}
    W40, b40 = consts["W40"].to(dev), consts["b40"].to(dev)
    Pn = B * N * N
    ops.reset_dw_queue()
    ops.edge_sched_init(torch.device(dev))
    n_dyn = ops.STATS["edge_dynamic_launches"]
    with options.override(**ov):
        z2, sv, zbo = trunk.edge_transition_fwd(Pd, 0, k["n3"], k["z"], k["emask"], B, N, zb_next=(W40, b40) if zb else None)
        assert (zbo is not None) == bool(zb and options.opts.fused_edge)
        G = _zeros_like(Pd, ET_PARAMS)
        dz = torch.full((Pn, 128), NAN, device=dev)
        dn3 = k["dn3"].clone()
        # (the unfused paths add dzb W40 into dz2 in place: a copy per run)
        trunk.edge_transition_bwd(Pd, G, 0, sv, k["dz2"].clone() if with_dz2 else None, dz, dn3, dzb_next=(k["dzb"], W40) if zb else None)
        _finish()
    if dynamic:
        assert ops.STATS["edge_dynamic_launches"] > n_dyn, "the dynamic tile hand-out did not run"
    gates = _et_gates(sv)
    acts = [sv["h1"], sv["h2"]]
    if sv.get("h2_has_z"):
        h2 = sv["h2"].clone()
        h2[:, :128] -= k["z"]             # (exact up to the rounding of the kernel's add: only the size of the activation is read)
        acts = [sv["h1"], h2]
    r64, r32 = ref.for_gates(gates, acts)
    got = dict(z2=z2, dz=dz, dn3=dn3)
    if zbo is not None:
        got["zb"] = zbo
    got.update({"d:" + n: G[n] for n in ET_PARAMS})
    r64 = dict(r64, dz=r64["d:z"], dn3=t["dn3"].double() + r64["d:n3"])
    r32 = dict(r32, dz=r32["d:z"], dn3=(t["dn3"] + r32["d:n3"].float()).double())
    _compare("edge_transition", f"dev={dev} B={B} N={N} zb={zb} dz2={with_dz2} {ov}", got, r64, r32,
             names={"d:" + n: n for n in ET_PARAMS})


def _edge_transition_sampling(dev, B, N, seed):
    """forward only: folded node terms read at stride 1024 (cache, save=False) on the column-split kernel and on the 16-row
    kernel, and the unfolded terms without a cache"""
    t, consts, ref = _et_case(B, N, seed, True, True)
    Pd = _on(dev, _params(seed), ET)
    k = {n: v.to(dev).contiguous() for n, v in t.items()}
    W40, b40 = consts["W40"].to(dev), consts["b40"].to(dev)
    ops.edge_sched_init(torch.device(dev))
    for cache, ov in (({}, dict()), ({}, dict(edge_pair=False)), (None, dict()), ({}, dict(fold_node_terms=False))):
        with options.override(**ov):
            for again in range(2 if (cache is not None and not ov) else 1):       # (again: the folded matrix and the image from the cache)
                z2, sv, zb = trunk.edge_transition_fwd(Pd, 0, k["n3"], k["z"], k["emask"], B, N, save=False, cache=cache, zb_next=(W40, b40))
                assert sv is None and zb is not None
                assert cache is None or (("et_fold", ET) in cache) == bool(options.opts.fold_node_terms)
                _compare("edge_transition_sampling", f"dev={dev} B={B} N={N} cache={cache is not None} again={again} {ov}",
                         dict(z2=z2, zb=zb), ref.r64, ref.r32)


ET_SETTINGS = (dict(), dict(fused_ln_bwd=False), dict(fused_edge=False), dict(grouped_pair_dw=False), dict(grouped_node_dw=False),
               dict(edge_shape=8))


@pytest.mark.parametrize("zb", (False, True), ids=("plain", "zb"))
@pytest.mark.parametrize("ov", ET_SETTINGS, ids=_sid)
def test_edge_transition_stage_emu(use_emu, ov, zb):
    _edge_transition("cpu", 2, 9, 50, zb, **ov)


# dzb_next carries the whole gradient (dz2 = None) on paths (i) and (ii); 289 rows >= 4 x 64 x 1: the dynamic tile hand-out
ET_MORE_EMU = ((2, 9, 50, True, dict(with_dz2=False)), (2, 9, 50, True, dict(with_dz2=False, fused_ln_bwd=False)),
               (1, 17, 51, False, dict(dynamic=True, edge_blocks=1)), (1, 17, 51, True, dict(dynamic=True, edge_blocks=1)))


@pytest.mark.parametrize("case", ET_MORE_EMU, ids=lambda c: f"B{c[0]}N{c[1]}-{'zb' if c[3] else 'plain'}-{_sid(c[4])}")
def test_edge_transition_stage_more_emu(use_emu, case):
    _edge_transition("cpu", *case[:4], **case[4])


def test_edge_transition_sampling_emu(use_emu):
    _edge_transition_sampling("cpu", 2, 9, 50)


@pytest.mark.gpu
@pytest.mark.parametrize("zb", (False, True), ids=("plain", "zb"))
@pytest.mark.parametrize("ov", ET_SETTINGS, ids=_sid)
def test_edge_transition_stage_gpu(hip_lib, ov, zb):
    _edge_transition("cuda", 2, 9, 50, zb, **ov)
    _edge_transition("cuda", 2, 37, 52, zb, **ov)


@pytest.mark.gpu
def test_edge_transition_stage_more_gpu(hip_lib):
    for N, seed in ((9, 50), (37, 52)):
        _edge_transition("cuda", 2, N, seed, True, with_dz2=False)
        _edge_transition("cuda", 2, N, seed, True, with_dz2=False, fused_ln_bwd=False)
    for zb in (False, True):
        _edge_transition("cuda", 2, 37, 52, zb, dynamic=True, edge_blocks=2)             # 2,738 rows >= 4 x 64 x 2
        _edge_transition("cuda", 1, 128, 53, zb, dynamic=True, edge_shape=8, edge_blocks=5)   # 16,384 rows >= 4 x 128 x 5


@pytest.mark.gpu
def test_edge_transition_sampling_gpu(hip_lib):
    _edge_transition_sampling("cuda", 2, 9, 50)
    _edge_transition_sampling("cuda", 2, 37, 52)


# ------------------------------------------------------------------------------------------------ per-residue stages
LN_PARAMS = tuple(f"{T}.{n}.{t}" for n in ("ipa_ln_0", "skip_embed_0") for t in ("weight", "bias"))
TF = f"{T}.seq_tfmr_0.layers.0"
TF_PARAMS = (f"{TF}.self_attn.in_proj_weight", f"{TF}.self_attn.in_proj_bias") + tuple(
    f"{TF}.{n}.{t}" for n in ("self_attn.out_proj", "linear1", "linear2", "norm1", "norm2") for t in ("weight", "bias"))
NT = f"{T}.node_transition_0"
PN_PARAMS = tuple(f"{n}.{t}" for n in (f"{T}.post_tfmr_0", f"{NT}.linear_1", f"{NT}.linear_2", f"{NT}.linear_3", f"{NT}.ln")
                  for t in ("weight", "bias"))


def _mask(B, N):
    m = torch.ones(B, N)
    m[0, N - 3:] = 0.0                # a padded tail
    return m


def _ln_skip_fn(Lf, Cs, relu):
    u0 = torch.cat([F.layer_norm(Lf["x1"], (256,), Lf[f"{T}.ipa_ln_0.weight"], Lf[f"{T}.ipa_ln_0.bias"]),
                    F.linear(Lf["init"], Lf[f"{T}.skip_embed_0.weight"], Lf[f"{T}.skip_embed_0.bias"])], -1)
    return dict(u0=u0), (u0 * Cs["du0"]).sum()


def _tfmr_fn(Lf, Cs, relu):
    """fo.tfmr_layer with the ReLU of linear1 as an overridable gate"""
    B, N = Cs["B"], Cs["N"]
    x = Lf["x"].view(B, N, 320)
    qkv = F.linear(x, Lf[f"{TF}.self_attn.in_proj_weight"], Lf[f"{TF}.self_attn.in_proj_bias"])
    q, k, v = (t.view(B, N, 4, 80).transpose(1, 2) for t in qkv.split(320, dim=-1))
    a = torch.softmax((q @ k.transpose(-1, -2)) / math.sqrt(80) + Cs["key_add"][:, None, None, :], dim=-1)
    o = (a @ v).transpose(1, 2).reshape(B, N, 320)
    o = F.linear(o, Lf[f"{TF}.self_attn.out_proj.weight"], Lf[f"{TF}.self_attn.out_proj.bias"])
    x = F.layer_norm(x + o, (320,), Lf[f"{TF}.norm1.weight"], Lf[f"{TF}.norm1.bias"])
    x = x.reshape(B * N, 320)
    ff = F.linear(relu(F.linear(x, Lf[f"{TF}.linear1.weight"], Lf[f"{TF}.linear1.bias"])), Lf[f"{TF}.linear2.weight"], Lf[f"{TF}.linear2.bias"])
    y = F.layer_norm(x + ff, (320,), Lf[f"{TF}.norm2.weight"], Lf[f"{TF}.norm2.bias"])
    return dict(y=y), (y * Cs["dy"]).sum()


def _post_node_fn(Lf, Cs, relu):
    """n2 = u0[:, :256] + post_tfmr(u2); n3 = mask * fo.node_transition(n2) with overridable gates"""
    n2 = Lf["u0"][:, :256] + F.linear(Lf["u2"], Lf[f"{T}.post_tfmr_0.weight"], Lf[f"{T}.post_tfmr_0.bias"])
    h = relu(F.linear(n2, Lf[f"{NT}.linear_1.weight"], Lf[f"{NT}.linear_1.bias"]))
    h = relu(F.linear(h, Lf[f"{NT}.linear_2.weight"], Lf[f"{NT}.linear_2.bias"]))
    h = F.linear(h, Lf[f"{NT}.linear_3.weight"], Lf[f"{NT}.linear_3.bias"])
    n3 = F.layer_norm(h + n2, (256,), Lf[f"{NT}.ln.weight"], Lf[f"{NT}.ln.bias"]) * Cs["mask"][:, None]
    return dict(n3=n3), (n3 * Cs["dn3"]).sum()


@functools.lru_cache(maxsize=None)
def _node_case(stage, B, N, seed):
    P = _params(seed)
    g = torch.Generator().manual_seed(seed + 900)
    R = B * N
    rn = lambda *s: torch.randn(*s, generator=g)
    m = _mask(B, N)
    if stage == "ln_skip":
        t = dict(x1=rn(R, 256), init=rn(R, 256), du0=rn(R, 320), dinit=rn(R, 256))
        return t, Reference(_ln_skip_fn, dict({k: P[k] for k in LN_PARAMS}, x1=t["x1"], init=t["init"]), dict(du0=t["du0"]))
    if stage == "tfmr":
        t = dict(x=rn(R, 320), dy=rn(R, 320), key_add=(1 - m).contiguous())
        ref = Reference(_tfmr_fn, dict({k: P[k] for k in TF_PARAMS}, x=t["x"]), dict(B=B, N=N, key_add=t["key_add"], dy=t["dy"]))
        # the restatement is the oracle's layer
        y = fo.tfmr_layer({k: v.double() for k, v in P.items() if k.startswith(TF)}, TF, t["x"].double().view(B, N, 320), t["key_add"].double(), 4)
        assert relerr(y.reshape(R, 320), ref.r64["y"]) < 1e-12
        return t, ref
    t = dict(u2=rn(R, 320), u0=rn(R, 320), dn3=rn(R, 256), du0=rn(R, 320), mask=m.reshape(-1).contiguous())
    ref = Reference(_post_node_fn, dict({k: P[k] for k in PN_PARAMS}, u2=t["u2"], u0=t["u0"]), dict(mask=t["mask"], dn3=t["dn3"]))
    P64 = {k: v.double() for k, v in P.items() if k.startswith(NT) or k.startswith(f"{T}.post_tfmr_0")}
    n2 = t["u0"].double()[:, :256] + F.linear(t["u2"].double(), P64[f"{T}.post_tfmr_0.weight"], P64[f"{T}.post_tfmr_0.bias"])
    assert relerr(fo.node_transition(P64, NT, n2) * t["mask"].double()[:, None], ref.r64["n3"]) < 1e-12
    return t, ref


def _ln_skip(dev, B, N, seed):
    t, ref = _node_case("ln_skip", B, N, seed)
    Pd = _on(dev, _params(seed), T)
    k = {n: v.to(dev).contiguous() for n, v in t.items()}
    R = B * N
    ops.reset_dw_queue()
    u0, sv = nw.ln_skip_fwd(Pd, 0, k["x1"], k["init"], R)
    G = _zeros_like(Pd, LN_PARAMS)
    dx1 = torch.full((R, 256), NAN, device=dev)
    dinit = k["dinit"].clone()
    nw.ln_skip_bwd(Pd, G, 0, sv, k["du0"], dx1, dinit)
    _finish()
    got = dict(u0=u0, dx1=dx1, dinit=dinit)
    got.update({"d:" + n: G[n] for n in LN_PARAMS})
    r64 = dict(ref.r64, dx1=ref.r64["d:x1"], dinit=t["dinit"].double() + ref.r64["d:init"])
    r32 = dict(ref.r32, dx1=ref.r32["d:x1"], dinit=(t["dinit"] + ref.r32["d:init"].float()).double())
    _compare("ln_skip", f"dev={dev} B={B} N={N}", got, r64, r32, names={"d:" + n: n for n in LN_PARAMS})


def _tfmr(dev, B, N, seed, **ov):
    t, ref = _node_case("tfmr", B, N, seed)
    Pd = _on(dev, _params(seed), TF)
    k = {n: v.to(dev).contiguous() for n, v in t.items()}
    ops.reset_dw_queue()
    with options.override(seq_attn_min_rows=0, **ov):
        y, sv, pend = nw.tfmr_layer_fwd(Pd, TF, k["x"], k["key_add"].view(B, N), B, N)
        assert pend is None
        G = _zeros_like(Pd, TF_PARAMS)
        dx = nw.tfmr_layer_bwd(Pd, G, TF, sv, k["dy"])
        _finish()
    r64, r32 = ref.for_gates([sv["f"] > 0], [sv["f"]])
    got = dict(y=y, dx=dx)
    got.update({"d:" + n: G[n] for n in TF_PARAMS})
    _compare("tfmr_layer", f"dev={dev} B={B} N={N} {ov}", got, dict(r64, dx=r64["d:x"]), dict(r32, dx=r32["d:x"]),
             names={"d:" + n: n for n in TF_PARAMS})


def _post_node(dev, B, N, seed):
    t, ref = _node_case("post_node", B, N, seed)
    Pd = _on(dev, _params(seed), T)
    k = {n: v.to(dev).contiguous() for n, v in t.items()}
    R = B * N
    ops.reset_dw_queue()
    n3, sv = nw.post_node_fwd(Pd, 0, k["u2"], k["u0"], k["mask"], R)
    G = _zeros_like(Pd, PN_PARAMS)
    du0 = k["du0"].clone()
    du2 = nw.post_node_bwd(Pd, G, 0, sv, k["dn3"], du0)
    _finish()
    r64, r32 = ref.for_gates([sv["h1"] > 0, sv["h2"] > 0], [sv["h1"], sv["h2"]])
    got = dict(n3=n3, du2=du2, du0=du0)
    got.update({"d:" + n: G[n] for n in PN_PARAMS})
    # (du0's columns 256.. are untouched: the reference gradient of u0 is zero there)
    r64 = dict(r64, du2=r64["d:u2"], du0=t["du0"].double() + r64["d:u0"])
    r32 = dict(r32, du2=r32["d:u2"], du0=(t["du0"] + r32["d:u0"].float()).double())
    _compare("post_node", f"dev={dev} B={B} N={N}", got, r64, r32, names={"d:" + n: n for n in PN_PARAMS})
    assert torch.equal(du0[:, 256:], k["du0"][:, 256:])


TFMR_SETTINGS = (dict(), dict(fused_seq_attn=False), dict(fused_seq_attn_bwd=False))


def test_ln_skip_post_node_stage_emu(use_emu):
    _ln_skip("cpu", 2, 9, 60)
    _post_node("cpu", 2, 9, 60)


@pytest.mark.parametrize("ov", TFMR_SETTINGS, ids=_sid)
def test_tfmr_layer_stage_emu(use_emu, ov):
    _tfmr("cpu", 2, 9, 60, **ov)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ((2, 37, 61), (1, 300, 62)), ids=lambda s: f"B{s[0]}N{s[1]}")
def test_ln_skip_post_node_stage_gpu(hip_lib, shape):
    _ln_skip("cuda", *shape)
    _post_node("cuda", *shape)


@pytest.mark.gpu
@pytest.mark.parametrize("ov", TFMR_SETTINGS, ids=_sid)
def test_tfmr_layer_stage_gpu(hip_lib, ov):
    _tfmr("cuda", 2, 37, 61, **ov)
    _tfmr("cuda", 1, 300, 62, **ov)
