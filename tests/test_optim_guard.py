"""The guarded optimiser step (fd_adam_step_guarded / fd_grad_stats, optim.FlatAdam(max_grad_norm=, skip_nonfinite=)):
clipping by global norm, skip-on-non-finite and the step counter on the device.

Every comparison is against torch on the CPU as the independent restatement: per step, on a twin parameter list,
torch.nn.utils.clip_grad_norm_ (when clipping) and torch.optim.Adam.step() -- the latter only if every gradient element
is finite.  Parameter bound: tests/test_optim.py's, max|a-b| < 2e-6 * (1 + max|a|).  Norm bound: 1e-12 relative against the
float64 torch norm (fp32 squares are exact in fp64; a tree of per-thread runs over <= 2^25 non-negative terms has a relative
error bound of a few 1e-15 -- 1e-12 is that with margin, not a measured figure)."""
import ctypes
import os
import re

import pytest
import torch

from se3_diffusion_amd import hip
from se3_diffusion_amd.optim import FlatAdam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = float("inf"), float("nan")


def _params(dev, seed):
    g = torch.Generator().manual_seed(seed)
    shapes = [(7, 5), (6,), (128, 64), (3,), (33, 17)]          # tests/test_optim.py::_params
    return [torch.nn.Parameter(torch.randn(*s, generator=g).to(dev)) for s in shapes]


def _close(ref, mine):
    for a, b in zip(ref, mine):
        a, b = a.detach().cpu(), b.detach().cpu()
        err, bound = float((a - b).abs().max()), 2e-6 * (1 + float(a.abs().max()))
        print(f"  max|a-b| = {err:.3e}  (bound {bound:.3e})")
        assert err < bound, (err, bound)


def _norm64(grads):
    return float(torch.linalg.vector_norm(torch.cat([g.detach().double().cpu().reshape(-1) for g in grads])))


def _set_grads(mine, grads):
    for b, gr in zip(mine, grads):
        b.grad.copy_(gr)                            # into the flat buffer's views


def _twin_step(ref, topt, grads, max_norm):
    """clip_grad_norm_ + Adam.step() on the CPU twin, only if every gradient element is finite"""
    for a, gr in zip(ref, grads):
        a.grad = gr.detach().cpu().clone()
    if not all(bool(torch.isfinite(a.grad).all()) for a in ref):
        return False
    if max_norm is not None:
        torch.nn.utils.clip_grad_norm_(ref, max_norm)
    topt.step()
    return True


def _draw(ref, gen, scale):
    return [scale * torch.randn(*a.shape, generator=gen) for a in ref]


# ---- 1. clip parity ---------------------------------------------------------------------------------------------------
MAX_NORM = 5.0        # the 8797 elements of _params: |0.01 N(0,1)| ~ 0.94 stays below, |10 N(0,1)| ~ 938 is clipped


def _run_clip(dev, steps=6):
    ref, mine = _params("cpu", 1), _params(dev, 1)
    topt = torch.optim.Adam(ref, lr=1e-2)
    fopt = FlatAdam(mine, lr=1e-2, max_grad_norm=MAX_NORM, skip_nonfinite=True)
    gen = torch.Generator().manual_seed(2)
    norms = []
    for it in range(steps):
        grads = _draw(ref, gen, 0.01 if it % 2 == 0 else 10.0)
        fopt.zero_grad()
        _set_grads(mine, [g.to(dev) for g in grads])
        assert _twin_step(ref, topt, grads, MAX_NORM)
        fopt.step()
        h = fopt.health()
        want = _norm64(grads)
        print(f"  step {it}: grad_norm {h['grad_norm']!r}, float64 torch {want!r}, clip_coef {h['clip_coef']!r}")
        assert abs(h["grad_norm"] - want) <= 1e-12 * want
        assert h["step"] == it + 1 and h["skipped"] == 0 and h["nonfinite"] == 0
        coef = min(1.0, MAX_NORM / (h["grad_norm"] + 1e-6))
        assert abs(h["clip_coef"] - coef) <= 4e-16 * coef            # (the same fp64 operations: at most the last bit)
        assert h["max_abs"] == max(float(g.abs().max()) for g in grads)
        norms.append(h["grad_norm"])
    h = fopt.health()
    assert h["clipped"] == steps // 2, h                 # above max_norm on the odd steps, below on the even ones
    _close(ref, mine)
    return mine, norms


def test_clip_parity_emu(use_emu):
    _run_clip("cpu")


@pytest.mark.gpu
def test_clip_parity_gpu(hip_lib):
    _run_clip("cuda", steps=8)


# ---- 2. skip ----------------------------------------------------------------------------------------------------------
def _run_skip(dev, steps=7, bad={2: (2, 4711, INF), 4: (0, 3, NAN)}):
    """bad: step -> (gradient view, element, value).  Returns (optimiser, twin parameters, parameters, twin optimiser)."""
    ref, mine = _params("cpu", 1), _params(dev, 1)
    topt = torch.optim.Adam(ref, lr=1e-2)
    fopt = FlatAdam(mine, lr=1e-2, max_grad_norm=MAX_NORM, skip_nonfinite=True)
    gen = torch.Generator().manual_seed(3)
    applied = 0
    for it in range(steps):
        grads = _draw(ref, gen, 0.01 if it % 2 == 0 else 10.0)
        if it in bad:
            view, el, val = bad[it]
            grads[view].view(-1)[el] = val               # at the gradient buffer only
        fopt.zero_grad()
        _set_grads(mine, [g.to(dev) for g in grads])
        before = (fopt.flat_p.clone(), fopt.exp_avg.clone(), fopt.exp_avg_sq.clone())
        h0 = fopt.health()
        stepped = _twin_step(ref, topt, grads, MAX_NORM)
        fopt.step()
        h1 = fopt.health()
        if it in bad:
            assert not stepped
            assert torch.equal(fopt.flat_p, before[0]) and torch.equal(fopt.exp_avg, before[1])
            assert torch.equal(fopt.exp_avg_sq, before[2])
            assert h1["skipped"] == h0["skipped"] + 1 and h1["nonfinite"] >= 1 and h1["step"] == h0["step"]
        else:
            applied += 1
            assert not torch.equal(fopt.flat_p, before[0])
            assert h1["skipped"] == h0["skipped"] and h1["nonfinite"] == 0 and h1["step"] == h0["step"] + 1
    assert fopt.health()["step"] == applied == steps - len(bad)
    _close(ref, mine)                                    # the twin never stepped on the bad gradients
    return fopt, ref, mine, topt


def _run_no_skip(dev):
    """skip_nonfinite=False, max_grad_norm=1.0: the same gradient is NOT skipped.  The norm is taken over the finite elements,
    so the step is applied with the coefficient of the finite part and the inf element makes its own parameter and moments
    non-finite (and only those: the update is elementwise).  Tested: skipped == 0 only."""
    mine = _params(dev, 1)
    fopt = FlatAdam(mine, lr=1e-2, max_grad_norm=1.0)
    grads = _draw(mine, torch.Generator().manual_seed(3), 1.0)
    grads[2].view(-1)[4711] = INF
    _set_grads(mine, [g.to(dev) for g in grads])
    fopt.step()
    h = fopt.health()
    assert h["skipped"] == 0 and h["step"] == 1 and h["nonfinite"] == 1, h


def test_skip_nonfinite_emu(use_emu):
    _run_skip("cpu")
    _run_no_skip("cpu")


@pytest.mark.gpu
def test_skip_nonfinite_gpu(hip_lib):
    _run_skip("cuda")
    _run_no_skip("cuda")


# ---- 3. a guard that never fires equals no guard -------------------------------------------------------------------------
def _run_idle_guard(dev, steps=5):
    plain, mine = _params(dev, 1), _params(dev, 1)
    popt = FlatAdam(plain, lr=1e-2)
    fopt = FlatAdam(mine, lr=1e-2, max_grad_norm=1e30, skip_nonfinite=True)
    gen = torch.Generator().manual_seed(4)
    for it in range(steps):
        grads = [g.to(dev) for g in _draw(plain, gen, 1.0)]
        _set_grads(plain, grads)
        _set_grads(mine, grads)
        popt.step()
        fopt.step()
    h = fopt.health()
    assert h["step"] == steps and h["clipped"] == 0 and h["skipped"] == 0 and h["clip_coef"] == 1.0
    _close(plain, mine)               # (not bitwise: the bias corrections are computed on the device)


def test_idle_guard_equals_plain_emu(use_emu):
    _run_idle_guard("cpu")


@pytest.mark.gpu
def test_idle_guard_equals_plain_gpu(hip_lib):
    _run_idle_guard("cuda")


# ---- 4. reproducible ----------------------------------------------------------------------------------------------------
def _run_reproducible(dev, lib, n):
    a, na = _run_clip(dev)
    b, nb = _run_clip(dev)
    assert all(torch.equal(x.detach(), y.detach()) for x, y in zip(a, b))
    assert na == nb                                      # Python floats decoded from the same bits
    # fd_grad_stats twice on one buffer; n is not a multiple of what one block covers per trip (256 threads x 4 elements) and
    # the last float4 holds a non-finite element
    assert n % 4 == 0 and n % 1024 != 0
    g = torch.randn(n, generator=torch.Generator().manual_seed(5)).to(dev)
    g[n - 2] = NAN
    g[7] = -INF
    ws = torch.empty(hip.OPT_WS_DOUBLES, dtype=torch.float64, device=dev)
    s1 = torch.full((4,), NAN, dtype=torch.float64, device=dev)
    s2 = torch.full((4,), NAN, dtype=torch.float64, device=dev)
    lib.call("fd_grad_stats", g, n, ws, s1)
    ws.fill_(NAN)                                        # (nothing of the first call's partials may be needed)
    lib.call("fd_grad_stats", g, n, ws, s2)
    assert torch.equal(s1, s2), (s1, s2)
    fin = g.cpu()[torch.isfinite(g.cpu())].double()
    want = float((fin * fin).sum())
    got = s1.cpu().tolist()
    print(f"  sum of squares {got[0]!r}, float64 torch {want!r}")
    assert abs(got[0] - want) <= 1e-12 * want
    assert got[1] == 2.0 and got[2] == float(fin.abs().max()) and got[3] == 0.0


def test_reproducible_emu(use_emu):
    _run_reproducible("cpu", use_emu, 300_004)


@pytest.mark.gpu
def test_reproducible_gpu(hip_lib):
    _run_reproducible("cuda", hip_lib, 5_000_004)        # beyond one grid-stride trip of 4096 x 256 x 4 elements


# ---- 5. checkpoint ------------------------------------------------------------------------------------------------------
def _run_checkpoint(dev):
    # guarded FlatAdam -> torch: "step" is the number of APPLIED steps (4 attempts, one skipped)
    fopt, ref, mine, topt = _run_skip(dev, steps=4, bad={1: (2, 100, INF)})
    t2 = torch.optim.Adam(_params("cpu", 1), lr=1e-2)
    sd = fopt.state_dict()
    t2.load_state_dict(sd)
    assert float(t2.state_dict()["state"][0]["step"]) == 3.0
    assert all(float(s["step"]) == 3.0 for s in sd["state"].values())
    # torch -> guarded FlatAdam: continue from torch's state (3 applied steps) and stay within the bound
    cont = _params(dev, 1)
    for c, a in zip(cont, ref):
        c.data.copy_(a.data)
    f2 = FlatAdam(cont, lr=1e-2, max_grad_norm=MAX_NORM, skip_nonfinite=True)
    f2.load_state_dict(topt.state_dict())
    assert f2.health()["step"] == 3
    gen = torch.Generator().manual_seed(9)
    for it in range(2):
        grads = _draw(ref, gen, 10.0 if it == 0 else 0.01)
        _set_grads(cont, [g.to(dev) for g in grads])
        assert _twin_step(ref, topt, grads, MAX_NORM)
        f2.step()
    assert f2.health()["step"] == 5 and f2.health()["clipped"] == 1
    _close(ref, cont)
    assert float(f2.state_dict()["state"][0]["step"]) == 5.0


def test_checkpoint_emu(use_emu):
    _run_checkpoint("cpu")


@pytest.mark.gpu
def test_checkpoint_gpu(hip_lib):
    _run_checkpoint("cuda")


# ---- 6. ABI -------------------------------------------------------------------------------------------------------------
def test_opt_state_layout_matches_header():
    hdr = open(os.path.join(ROOT, "include", "fd_hip.h")).read()
    defs = {m.group(1): m.group(2) for m in re.finditer(r"#define (FD_[A-Z0-9_]+)\s+\(?([0-9 *L]+?)\)?\s*(?:/\*.*)?$", hdr, re.M)}
    val = lambda e: eval(e.replace("L", ""))
    assert val(defs["FD_OPT_WS_DOUBLES"]) == hip.OPT_WS_DOUBLES
    assert val(defs["FD_OPT_STATE_BYTES"]) == hip.OPT_STATE_BYTES == ctypes.sizeof(hip.FdOptState)
    # the struct itself: same fields, same order, same C types
    body = re.search(r"typedef struct FdOptState \{(.*?)\} FdOptState;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [tuple(f.split()) for f in body.split(";") if f.strip()]
    ct = {"long": ctypes.c_long, "double": ctypes.c_double, "float": ctypes.c_float, "int": ctypes.c_int}
    assert [(n, ct[t]) for t, n in fields] == list(hip.FdOptState._fields_)
    off = 0
    for t, n in fields:                                  # naturally aligned without padding: the C layout is the packed one
        assert getattr(hip.FdOptState, n).offset == off and off % ctypes.sizeof(ct[t]) == 0
        off += ctypes.sizeof(ct[t])
    assert off == hip.OPT_STATE_BYTES and off % 8 == 0


def test_guarded_step_has_no_cpu_fallback():
    if not os.path.exists(hip.LIB_PATH):
        from se3_diffusion_amd import build
        build.build(verbose=False)
    lib = hip.FdLib(hip.LIB_PATH)
    z = lambda n: torch.zeros(n)
    with pytest.raises(hip.FdError):
        lib.call("fd_adam_step_guarded", z(8), z(8), z(8), z(8), 8, 1e-2, 0.9, 0.999, 1e-8, 1.0, 1,
                 torch.zeros(hip.OPT_WS_DOUBLES, dtype=torch.float64), torch.zeros(hip.OPT_STATE_BYTES // 8, dtype=torch.int64))
    with pytest.raises(hip.FdError):
        lib.call("fd_grad_stats", z(8), 8, torch.zeros(hip.OPT_WS_DOUBLES, dtype=torch.float64),
                 torch.zeros(4, dtype=torch.float64))


def _run_empty(dev, lib):
    nan = lambda n: torch.full((n,), NAN, device=dev)
    p, g, m, v = nan(4), nan(4), nan(4), nan(4)
    ws = torch.full((hip.OPT_WS_DOUBLES,), NAN, dtype=torch.float64, device=dev)
    state = torch.full((hip.OPT_STATE_BYTES // 8,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=dev)
    stats = torch.full((4,), NAN, dtype=torch.float64, device=dev)
    n_launch = lib.cdll.fd_launch_count()
    lib.call("fd_adam_step_guarded", p, g, m, v, 0, 1e-2, 0.9, 0.999, 1e-8, 1.0, 1, ws, state)
    lib.call("fd_grad_stats", g, 0, ws, stats)
    assert lib.cdll.fd_launch_count() == n_launch
    assert all(bool(torch.isnan(t).all()) for t in (p, m, v, ws, stats))
    assert bool((state == 0x5A5A5A5A5A5A5A5A).all())
    # argument errors: a length that is not a multiple of 4, a missing state
    with pytest.raises(hip.FdError, match="multiple of 4"):
        lib.call("fd_adam_step_guarded", p, g, m, v, 3, 1e-2, 0.9, 0.999, 1e-8, 1.0, 1, ws, state)
    with pytest.raises(hip.FdError, match="null workspace or state"):
        lib.call("fd_adam_step_guarded", p, g, m, v, 4, 1e-2, 0.9, 0.999, 1e-8, 1.0, 1, ws, None)
    assert all(bool(torch.isnan(t).all()) for t in (p, m, v))


def test_empty_and_argument_errors_emu(use_emu):
    _run_empty("cpu", use_emu)


@pytest.mark.gpu
def test_empty_and_argument_errors_gpu(hip_lib):
    _run_empty("cuda", hip_lib)


# ---- 7. full size (GPU only) ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_full_size_gpu(hip_lib):
    from se3_diffusion_amd import train_step as ts
    from se3_diffusion_amd.model.score_network import ScoreNetwork
    model = ScoreNetwork(ts.base_model_conf(), diffuser=None).to("cuda").train()
    ts.perturb_final_layers(model, seed=0)
    start = [p.detach().cpu().clone() for p in model.parameters() if p.requires_grad]
    fopt = FlatAdam(model.parameters(), lr=1e-2, adjacent=model.flat_layout_groups(), max_grad_norm=1.0, skip_nonfinite=True)
    assert fopt.numel > 4096 * 256 * 4                   # more than one grid-stride trip
    ref = [torch.nn.Parameter(s.clone()) for s in start]
    topt = torch.optim.Adam(ref, lr=1e-2)
    gen = torch.Generator().manual_seed(11)
    grads = _draw(ref, gen, 1.0)
    _set_grads(fopt.params, [g.cuda() for g in grads])   # N(0,1) inside the views, the padding stays zero
    want = _norm64(grads)
    st = fopt.grad_stats().cpu().tolist()                # the stand-alone entry point on the same buffer
    assert abs(st[0] - want * want) <= 2e-12 * want * want and st[1] == 0.0
    assert _twin_step(ref, topt, grads, 1.0)
    fopt.step()                                          # one clipped step
    h = fopt.health()
    print(f"  grad_norm {h['grad_norm']!r}, float64 torch {want!r}")
    assert abs(h["grad_norm"] - want) <= 1e-12 * want
    assert h["step"] == 1 and h["clipped"] == 1 and abs(h["clip_coef"] * (h["grad_norm"] + 1e-6) - 1.0) <= 1e-15
    _close(ref, fopt.params)
    before = (fopt.flat_p.clone(), fopt.exp_avg.clone(), fopt.exp_avg_sq.clone())
    fopt.params[-1].grad.view(-1)[-1] = INF              # one element of the last view
    fopt.step()                                          # one skipped step
    h = fopt.health()
    assert h["step"] == 1 and h["skipped"] == 1 and h["nonfinite"] == 1
    assert torch.equal(fopt.flat_p, before[0]) and torch.equal(fopt.exp_avg, before[1])
    assert torch.equal(fopt.exp_avg_sq, before[2])


# ---- 8. capture (GPU only) ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_captured_step_gpu(hip_lib):
    """ONE guarded step() captured with torch.cuda.graph and replayed three times on fresh gradients equals four eager guarded
    steps (the eager warm-up step counts): the step counter, the bias corrections and the skip decision are the device's, so
    the second replay (non-finite gradient) skips and the third uses the bias correction of step 3.  Fails if either is still
    a host scalar baked into the captured launches."""
    dev = "cuda"
    mine, twin = _params(dev, 1), _params(dev, 1)
    fopt = FlatAdam(mine, lr=1e-2, max_grad_norm=MAX_NORM, skip_nonfinite=True)
    eopt = FlatAdam(twin, lr=1e-2, max_grad_norm=MAX_NORM, skip_nonfinite=True)
    gen = torch.Generator().manual_seed(6)
    flats = []
    for it in range(4):
        grads = _draw(mine, gen, 10.0 if it % 2 == 0 else 0.01)
        if it == 2:                                      # the second of the three replayed gradients
            grads[2].view(-1)[17] = NAN
        _set_grads(twin, [g.to(dev) for g in grads])
        flats.append(eopt.flat_g.clone())
        eopt.step()                                      # the eager twin: four guarded steps
    he = eopt.health()
    fopt.flat_g.copy_(flats[0])
    fopt.step()                                          # eager warm-up: it counts
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fopt.step()                                      # (recorded, not run: the counter is still 1)
    assert fopt.health()["step"] == 1
    for it in (1, 2, 3):
        fopt.flat_g.copy_(flats[it])
        graph.replay()
    torch.cuda.synchronize()
    h = fopt.health()
    assert h["step"] == 3 and h["skipped"] == 1, h
    assert he["step"] == 3 and he["skipped"] == 1, he
    assert h == he, (h, he)
    _close(twin, mine)
    # ... and both equal the CPU restatement that never stepped on the bad gradient
    ref = _params("cpu", 1)
    topt = torch.optim.Adam(ref, lr=1e-2)
    gen = torch.Generator().manual_seed(6)
    for it in range(4):
        grads = _draw(ref, gen, 10.0 if it % 2 == 0 else 0.01)
        if it == 2:
            grads[2].view(-1)[17] = NAN
        assert _twin_step(ref, topt, grads, MAX_NORM) == (it != 2)
    _close(ref, mine)


# ---- 9. through the training step -------------------------------------------------------------------------------------------
def _run_training_step(dev, B, N, blocks):
    from se3_diffusion_amd import loss as floss, train_step as ts
    from se3_diffusion_amd.model.score_network import ScoreNetwork
    model = ScoreNetwork(ts.base_model_conf(blocks), diffuser=None).to(dev).train()
    ts.perturb_final_layers(model, seed=0)
    batch = ts.synthetic_batch(B, N, dev, seed=1)
    gt37, _ = ts.backbone_atoms(batch["rigids_0"], batch["torsion_angles_sin_cos"][..., 2, :])
    fopt = FlatAdam(model.parameters(), lr=1e-3, adjacent=model.flat_layout_groups(), max_grad_norm=1.0, skip_nonfinite=True)

    def fwd_bwd():
        fopt.zero_grad()
        loss = floss.dsm_loss(batch, model(batch), gt37)
        loss.backward()
        fopt.rebind()                                    # p.grad are views of flat_g from here on
        return float(loss.detach())

    # (a) clip at half the gradient's norm
    fwd_bwd()
    n64 = float(torch.linalg.vector_norm(fopt.flat_g.double()))
    assert n64 > 0 and n64 == n64 and n64 != INF
    fopt.max_grad_norm = 0.5 * n64
    ref = [torch.nn.Parameter(p.detach().cpu().clone()) for p in fopt.params]
    topt = torch.optim.Adam(ref, lr=1e-3)
    grads = [p.grad.detach().cpu().clone() for p in fopt.params]
    assert _twin_step(ref, topt, grads, fopt.max_grad_norm)
    fopt.step()
    h = fopt.health()
    want = fopt.max_grad_norm / (n64 + 1e-6)
    print(f"  clip_coef {h['clip_coef']!r}, max_grad_norm / (n64 + 1e-6) = {want!r}")
    assert abs(h["clip_coef"] - want) <= 1e-9 * want and h["clipped"] == 1 and h["step"] == 1
    _close(ref, fopt.params)
    # (b) one inf element in one p.grad view after the backward: the step leaves the parameters alone ...
    fwd_bwd()
    victim = max(fopt.params, key=lambda p: p.numel())
    victim.grad.view(-1)[victim.numel() // 2] = INF
    before = fopt.flat_p.clone()
    fopt.step()
    assert torch.equal(fopt.flat_p, before)
    h = fopt.health()
    assert h["skipped"] == 1 and h["step"] == 1 and h["nonfinite"] == 1
    # ... and the next clean iteration trains on: a finite loss from the unchanged parameters, and an applied step
    loss = fwd_bwd()
    assert loss == loss and abs(loss) != INF
    fopt.step()
    assert not torch.equal(fopt.flat_p, before)
    assert bool(torch.isfinite(fopt.flat_p).all())
    h = fopt.health()
    assert h["skipped"] == 1 and h["step"] == 2 and h["nonfinite"] == 0


def test_training_step_emu(use_emu):
    _run_training_step("cpu", 1, 12, 1)


@pytest.mark.gpu
def test_training_step_gpu(hip_lib):
    _run_training_step("cuda", 2, 64, 2)


# ---- 10. dist.FlatGrads.grad_stats(): a buffer whose parameter count is not a multiple of 4 ---------------------------------
def _check_flat_grads_stats(params, grads, dev):
    from se3_diffusion_amd.dist import FlatGrads
    n = sum(p.numel() for p in params)
    fg = FlatGrads(params)
    assert fg.flat.numel() % 4 == 0 and 0 <= fg.flat.numel() - n < 4
    for p, gr in zip(fg.params, grads):
        p.grad.copy_(gr.to(dev))
    fg.all_reduce_mean()                                 # (single process: the rebind only) -- statistics come after it
    st = fg.grad_stats()
    got = st.cpu().tolist()
    want = _norm64(grads) ** 2
    print(f"  {n} elements: sum of squares {got[0]!r}, float64 torch {want!r}")
    assert abs(got[0] - want) <= 2e-12 * want            # (the square of a norm held to 1e-12)
    assert got[1] == 0.0 and got[2] == max(float(g.abs().max()) for g in grads) and got[3] == 0.0
    # the result tensor is the object's own, overwritten by the next call; `out=` writes elsewhere
    fg.params[0].grad.view(-1)[0] = NAN
    assert fg.grad_stats() is st and st.cpu().tolist()[1] == 1.0
    out = torch.zeros(4, dtype=torch.float64, device=dev)
    assert fg.grad_stats(out=out) is out and torch.equal(out, st)
    assert float(fg.flat[n:].abs().sum()) == 0.0         # the tail stays zero


def _run_flat_grads_stats(dev):
    ps = _params(dev, 1)
    assert sum(p.numel() for p in ps) % 4 == 1           # 8797 elements
    _check_flat_grads_stats(ps, _draw(ps, torch.Generator().manual_seed(12), 1.0), dev)


def test_flat_grads_stats_emu(use_emu):
    _run_flat_grads_stats("cpu")


@pytest.mark.gpu
def test_flat_grads_stats_gpu(hip_lib):
    _run_flat_grads_stats("cuda")


@pytest.mark.gpu
def test_flat_grads_stats_full_size_gpu(hip_lib):
    from se3_diffusion_amd import train_step as ts
    from se3_diffusion_amd.model.score_network import ScoreNetwork
    model = ScoreNetwork(ts.base_model_conf(), diffuser=None).to("cuda").train()
    ps = [p for p in model.parameters() if p.requires_grad]
    assert sum(p.numel() for p in ps) % 4 != 0           # 17,446,190 parameters
    _check_flat_grads_stats(ps, _draw(ps, torch.Generator().manual_seed(13), 1.0), "cuda")


# ---- 11. the Python surface: arguments, the step count, the statistics tensor ---------------------------------------------------
def _run_surface(dev):
    for bad in (0.0, -1.0, NAN):
        with pytest.raises(ValueError, match="max_grad_norm"):
            FlatAdam(_params(dev, 1), lr=1e-2, max_grad_norm=bad)
    mine = _params(dev, 1)
    fopt = FlatAdam(mine, lr=1e-2, skip_nonfinite=True)
    fopt.max_grad_norm = 0.0                             # changed to a refused value between steps: step() raises, launches nothing
    before = fopt.flat_p.clone()
    with pytest.raises(ValueError, match="max_grad_norm"):
        fopt.step()
    assert torch.equal(fopt.flat_p, before) and fopt.health()["step"] == 0
    fopt.max_grad_norm = None
    # the host attribute t does not exist on a guarded optimiser (it could only go stale)
    with pytest.raises(AttributeError, match="applied_steps"):
        fopt.t
    with pytest.raises(AttributeError, match="applied_steps"):
        fopt.t = 0
    _set_grads(mine, [g.to(dev) for g in _draw(mine, torch.Generator().manual_seed(14), 1.0)])
    fopt.step()
    fopt.step()
    assert fopt.applied_steps() == 2
    # a checkpoint without optimiser state leaves the device counter alone
    sd = fopt.state_dict()
    fopt.load_state_dict({"state": {}, "param_groups": sd["param_groups"]})
    assert fopt.applied_steps() == 2
    fopt.set_applied_steps(7)
    assert fopt.health()["step"] == 7
    fopt.load_state_dict(sd)
    assert fopt.applied_steps() == 2
    # unguarded: t is the host count, readable and settable as before; an empty checkpoint leaves it alone too
    popt = FlatAdam(_params(dev, 1), lr=1e-2)
    _set_grads(popt.params, [g.to(dev) for g in _draw(popt.params, torch.Generator().manual_seed(14), 1.0)])
    popt.step()
    assert popt.t == 1 and popt.applied_steps() == 1
    popt.load_state_dict({"state": {}, "param_groups": popt.state_dict()["param_groups"]})
    assert popt.t == 1
    popt.t = 0
    assert popt.applied_steps() == 0
    # grad_stats(): one tensor, overwritten; on an unguarded optimiser too
    s1 = popt.grad_stats()
    v1 = s1.clone()
    popt.flat_g.mul_(2.0)
    assert popt.grad_stats() is s1 and torch.equal(s1[0], 4.0 * v1[0]) and torch.equal(s1[2], 2.0 * v1[2])
    out = torch.full((4,), NAN, dtype=torch.float64, device=dev)
    assert popt.grad_stats(out=out) is out and torch.equal(out, s1)


def test_python_surface_emu(use_emu):
    _run_surface("cpu")


@pytest.mark.gpu
def test_python_surface_gpu(hip_lib):
    _run_surface("cuda")


def test_grad_stats_alignment_emu(use_emu):
    g = torch.zeros(8)
    ws = torch.zeros(hip.OPT_WS_DOUBLES + 1, dtype=torch.float64)
    stats = torch.zeros(5, dtype=torch.float64)
    half = lambda t: (t.view(torch.float32), 1)          # 4 bytes past an 8-byte boundary
    with pytest.raises(hip.FdError, match="8-byte aligned"):
        use_emu.call("fd_grad_stats", g, 8, half(ws), stats)
    with pytest.raises(hip.FdError, match="8-byte aligned"):
        use_emu.call("fd_grad_stats", g, 8, ws, half(stats))
