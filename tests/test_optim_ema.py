"""The moving average of the weights inside the optimiser step (fd_adam_step_ema / fd_adam_step_guarded_ema,
optim.FlatAdam(ema_decay=, ema_warmup=)): E += a (P - E) on the parameters the update kernel has just written.

Reference: after every step the device's own parameters are read back and a float64 restatement of E += a (P - E) is advanced
with a taken as the same fp32 value the kernel uses, a = (float)(1 - d_t), d_t = ema_decay or, with warm-up,
min(ema_decay, (1 + t) / (10 + t)) in double, t = applied steps including this one.
Bound (derived, not measured): one update commits at most three fp32 roundings (P - E, a * (.), E + (.)) on quantities no
larger than M = max(|E|, |P|), each of at most 2^-24 relative -- below 5 * 2^-24 * max(1, M) with the second-order terms --
and carries the earlier error with the factor 1 - a <= 1.  After K steps: |E_dev - E_64| <= 5 K 2^-24 max(1, M), M the largest
magnitude met so far.  p, exp_avg and exp_avg_sq are compared BITWISE with a twin FlatAdam that keeps no average."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from se3_diffusion_amd import hip  # noqa: E402
from se3_diffusion_amd.optim import FlatAdam  # noqa: E402

INF, NAN = float("inf"), float("nan")
DECAY = 0.9
MAX_NORM = 5.0        # tests/test_optim_guard.py: |0.01 N(0,1)| over 8797 elements stays below, |10 N(0,1)| is clipped
EPS24 = 2.0 ** -24


def _params(dev, seed):
    g = torch.Generator().manual_seed(seed)
    shapes = [(7, 5), (6,), (128, 64), (3,), (33, 17)]          # tests/test_optim_guard.py::_params: 8797 elements, five views
    return [torch.nn.Parameter(torch.randn(*s, generator=g).to(dev)) for s in shapes]


def _draw(ref, gen, scale):
    return [scale * torch.randn(*a.shape, generator=gen) for a in ref]


def _set_grads(mine, grads):
    for b, gr in zip(mine, grads):
        b.grad.copy_(gr)                            # into the flat buffer's views


def _a32(t, warmup, decay=DECAY):
    """the kernel's a: 1 - d_t in double, rounded once to fp32"""
    d = min(decay, (1.0 + t) / (10.0 + t)) if warmup else decay
    return float(torch.tensor(1.0 - d, dtype=torch.float64).to(torch.float32))


def _padding(opt):
    pad = torch.ones(opt.numel, dtype=torch.bool)
    for p, o in zip(opt.params, opt.offsets):
        pad[o:o + p.numel()] = False
    assert int(pad.sum()) > 0                        # 8797 elements in five 256-byte aligned views leave gaps
    return pad


class _Ref64:
    """float64 restatement of the average, advanced from the device's own parameters"""

    def __init__(self, opt):
        self.E = opt.ema.double().cpu()
        self.M = float(self.E.abs().max())
        self.K = 0

    def advance(self, opt, a):
        P = opt.flat_p.double().cpu()
        self.M = max(self.M, float(P.abs().max()))
        self.E = self.E + a * (P - self.E)
        self.K += 1

    def check(self, opt, what):
        err = float((opt.ema.double().cpu() - self.E).abs().max())
        bound = 5.0 * self.K * EPS24 * max(1.0, self.M)
        print(f"  {what}: max|E_dev - E_64| = {err:.3e}  (bound {bound:.3e}, K = {self.K}, M = {self.M:.3f})")
        assert err <= bound, (what, err, bound)


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _assert_twin(opt, twin):
    assert _same_bits(opt.flat_p, twin.flat_p) and _same_bits(opt.exp_avg, twin.exp_avg)
    assert _same_bits(opt.exp_avg_sq, twin.exp_avg_sq)


# ---- 1. tracking: the plain step -------------------------------------------------------------------------------------
def _run_tracking(dev, warmup, steps=6):
    mine, twin = _params(dev, 1), _params(dev, 1)
    fopt = FlatAdam(mine, lr=1e-2, ema_decay=DECAY, ema_warmup=warmup)
    topt = FlatAdam(twin, lr=1e-2)
    assert fopt.numel % 4 == 0 and fopt.numel % 1024 != 0        # a float4 tail in the last block
    assert fopt.ema.data_ptr() != fopt.flat_p.data_ptr() and _same_bits(fopt.ema, fopt.flat_p)
    assert topt.ema is None
    pad = _padding(fopt)
    ref = _Ref64(fopt)
    gen = torch.Generator().manual_seed(21)
    for it in range(steps):
        grads = [g.to(dev) for g in _draw(mine, gen, 1.0)]
        _set_grads(mine, grads)
        _set_grads(twin, grads)
        fopt.step()
        topt.step()
        ref.advance(fopt, _a32(it + 1, warmup))
        ref.check(fopt, f"step {it + 1}")
        _assert_twin(fopt, topt)
        assert float(fopt.ema.cpu()[pad].abs().max()) == 0.0
    assert fopt.t == steps
    assert not torch.equal(fopt.ema, fopt.flat_p)


@pytest.mark.parametrize("warmup", [False, True])
def test_tracking_emu(use_emu, warmup):
    _run_tracking("cpu", warmup)


@pytest.mark.gpu
@pytest.mark.parametrize("warmup", [False, True])
def test_tracking_gpu(hip_lib, warmup):
    _run_tracking("cuda", warmup)


# ---- 2. the guarded step: a skipped call leaves the average alone, the warm-up counts applied steps ---------------------
def _run_guarded(dev, warmup, steps=6, bad_step=2):
    mine, twin = _params(dev, 1), _params(dev, 1)
    fopt = FlatAdam(mine, lr=1e-2, max_grad_norm=MAX_NORM, skip_nonfinite=True, ema_decay=DECAY, ema_warmup=warmup)
    topt = FlatAdam(twin, lr=1e-2, max_grad_norm=MAX_NORM, skip_nonfinite=True)
    pad = _padding(fopt)
    ref = _Ref64(fopt)
    gen = torch.Generator().manual_seed(22)
    applied = 0
    for it in range(steps):
        grads = _draw(mine, gen, 0.01 if it % 2 == 0 else 10.0)
        if it == bad_step:
            grads[2].view(-1)[4711] = INF
        grads = [g.to(dev) for g in grads]
        _set_grads(mine, grads)
        _set_grads(twin, grads)
        before = fopt.ema.clone()
        fopt.step()
        topt.step()
        if it == bad_step:
            assert _same_bits(fopt.ema, before)
            assert fopt.health()["skipped"] == 1 and fopt.health()["step"] == applied
        else:
            applied += 1
            assert not torch.equal(fopt.ema, before)
            if warmup and it == bad_step + 1:
                # the step after the skip is where t = calls would show: that restatement misses the bound tenfold
                wrong = ref.E + _a32(it + 1, True) * (fopt.flat_p.double().cpu() - ref.E)
                assert float((fopt.ema.double().cpu() - wrong).abs().max()) > 10 * 5.0 * steps * EPS24 * max(1.0, ref.M)
            ref.advance(fopt, _a32(applied, warmup))     # t = applied steps, not calls
        ref.check(fopt, f"call {it + 1} (applied {applied})")
        _assert_twin(fopt, topt)
        assert fopt.health() == topt.health()
        assert float(fopt.ema.cpu()[pad].abs().max()) == 0.0
    h = fopt.health()
    assert h["step"] == applied == steps - 1 and h["clipped"] >= 1, h


@pytest.mark.parametrize("warmup", [False, True])
def test_guarded_emu(use_emu, warmup):
    _run_guarded("cpu", warmup)


@pytest.mark.gpu
@pytest.mark.parametrize("warmup", [False, True])
def test_guarded_gpu(hip_lib, warmup):
    _run_guarded("cuda", warmup)


# ---- 3. the entry points directly ---------------------------------------------------------------------------------------
def _adam_args():
    return 1e-2, 0.9, 0.999, 1e-8


def _run_entry_errors(dev, lib):
    nan = lambda n: torch.full((n,), NAN, device=dev)
    p, g, m, v, e = nan(8), nan(8), nan(8), nan(8), nan(8)
    ws = torch.full((hip.OPT_WS_DOUBLES,), NAN, dtype=torch.float64, device=dev)
    state = torch.full((hip.OPT_STATE_BYTES // 8,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=dev)
    lr, b1, b2, eps = _adam_args()
    n_launch = lib.cdll.fd_launch_count()
    # n == 0: FD_OK, no launch, nothing touched
    lib.call("fd_adam_step_ema", p, g, m, v, e, 0, lr, b1, b2, eps, 0.1, 0.001, 0.1)
    lib.call("fd_adam_step_guarded_ema", p, g, m, v, e, 0, lr, b1, b2, eps, 1.0, 1, ws, state, DECAY, 1)
    # a misaligned ema (4 bytes past a 16-byte boundary), a length that is no multiple of 4, a decay of 0 or 1, a null ema
    with pytest.raises(hip.FdError, match="16-byte aligned"):
        lib.call("fd_adam_step_ema", p, g, m, v, (e, 1), 4, lr, b1, b2, eps, 0.1, 0.001, 0.1)
    with pytest.raises(hip.FdError, match="16-byte aligned"):
        lib.call("fd_adam_step_guarded_ema", p, g, m, v, (e, 1), 4, lr, b1, b2, eps, 1.0, 1, ws, state, DECAY, 1)
    with pytest.raises(hip.FdError, match="multiple of 4"):
        lib.call("fd_adam_step_ema", p, g, m, v, e, 6, lr, b1, b2, eps, 0.1, 0.001, 0.1)
    with pytest.raises(hip.FdError, match="multiple of 4"):
        lib.call("fd_adam_step_guarded_ema", p, g, m, v, e, 6, lr, b1, b2, eps, 1.0, 1, ws, state, DECAY, 1)
    for decay in (0.0, 1.0):
        with pytest.raises(hip.FdError, match="strictly between 0 and 1"):
            lib.call("fd_adam_step_ema", p, g, m, v, e, 8, lr, b1, b2, eps, 0.1, 0.001, 1.0 - decay)
        with pytest.raises(hip.FdError, match="strictly between 0 and 1"):
            lib.call("fd_adam_step_guarded_ema", p, g, m, v, e, 8, lr, b1, b2, eps, 1.0, 1, ws, state, decay, 1)
    with pytest.raises(hip.FdError, match="null operand"):
        lib.call("fd_adam_step_ema", p, g, m, v, None, 8, lr, b1, b2, eps, 0.1, 0.001, 0.1)
    with pytest.raises(hip.FdError, match="null operand"):
        lib.call("fd_adam_step_guarded_ema", p, g, m, v, None, 8, lr, b1, b2, eps, 1.0, 1, ws, state, DECAY, 1)
    assert lib.cdll.fd_launch_count() == n_launch
    assert all(bool(torch.isnan(t).all()) for t in (p, g, m, v, e, ws))
    assert bool((state == 0x5A5A5A5A5A5A5A5A).all())


def _run_entry_step(dev, lib, n):
    """one step of each entry point on n elements: p, m, v bitwise as from the entry point without the average, the average
    elementwise against the formula (the module docstring's bound at K = 1)"""
    gen = torch.Generator().manual_seed(23)
    rnd = lambda: torch.randn(n, generator=gen).to(dev)
    p0, g, m0, e0 = rnd(), rnd(), 0.1 * rnd(), rnd()
    v0 = (0.1 * rnd()) ** 2
    lr, b1, b2, eps = _adam_args()
    bc1, bc2 = 1.0 - b1 ** 3, 1.0 - b2 ** 3

    def check(p, e, a, what):
        want = e0.double() + a * (p.double() - e0.double())
        err = float((e.double() - want).abs().max())
        bound = 5.0 * EPS24 * max(1.0, float(p.abs().max()), float(e0.abs().max()))
        print(f"  {what}, n = {n}: max|E_dev - E_64| = {err:.3e}  (bound {bound:.3e})")
        assert err <= bound, (what, err, bound)
        assert not torch.equal(e, e0)

    # plain
    a = _a32(0, False, 0.75)
    p, m, v, e = p0.clone(), m0.clone(), v0.clone(), e0.clone()
    pt, mt, vt = p0.clone(), m0.clone(), v0.clone()
    lib.call("fd_adam_step_ema", p, g, m, v, e, n, lr, b1, b2, eps, bc1, bc2, 1.0 - 0.75)
    lib.call("fd_adam_step", pt, g, mt, vt, n, lr, b1, b2, eps, bc1, bc2)
    assert _same_bits(p, pt) and _same_bits(m, mt) and _same_bits(v, vt)
    check(p, e, a, "fd_adam_step_ema")
    # guarded, with warm-up: the state counts 4 applied steps before the call, t = 5
    for warmup in (0, 1):
        p, m, v, e = p0.clone(), m0.clone(), v0.clone(), e0.clone()
        pt, mt, vt = p0.clone(), m0.clone(), v0.clone()
        ws = torch.zeros(hip.OPT_WS_DOUBLES, dtype=torch.float64, device=dev)
        st = torch.zeros(hip.OPT_STATE_BYTES // 8, dtype=torch.int64, device=dev)
        st[0] = 4
        stt = st.clone()
        lib.call("fd_adam_step_guarded_ema", p, g, m, v, e, n, lr, b1, b2, eps, 1.0, 1, ws, st, 0.75, warmup)
        lib.call("fd_adam_step_guarded", pt, g, mt, vt, n, lr, b1, b2, eps, 1.0, 1, ws, stt)
        assert _same_bits(p, pt) and _same_bits(m, mt) and _same_bits(v, vt) and torch.equal(st, stt)
        assert int(st[0]) == 5
        check(p, e, _a32(5, bool(warmup), 0.75), f"fd_adam_step_guarded_ema(warmup={warmup})")


def test_entry_points_emu(use_emu):
    _run_entry_errors("cpu", use_emu)
    _run_entry_step("cpu", use_emu, 4 * (256 + 3))


@pytest.mark.gpu
def test_entry_points_gpu(hip_lib):
    _run_entry_errors("cuda", hip_lib)
    _run_entry_step("cuda", hip_lib, 4 * (256 + 3))


@pytest.mark.gpu
def test_entry_points_second_grid_trip_gpu(hip_lib):
    """the smallest size at which the grid-stride loop of the capped 4096-block grid goes round twice (and ends in a partial block)"""
    _run_entry_step("cuda", hip_lib, 4 * (4096 * 256 + 259))


# ---- 4. ema_weights() ---------------------------------------------------------------------------------------------------
def _stepped(dev, steps=2, **kw):
    mine = _params(dev, 1)
    fopt = FlatAdam(mine, lr=1e-2, ema_decay=DECAY, **kw)
    gen = torch.Generator().manual_seed(24)
    for _ in range(steps):
        _set_grads(mine, [g.to(dev) for g in _draw(mine, gen, 1.0)])
        fopt.step()
    return fopt, mine


def _run_ema_weights(dev):
    fopt, mine = _stepped(dev)
    p0, e0 = fopt.flat_p.clone(), fopt.ema.clone()
    assert not torch.equal(p0, e0)
    ptrs = [p.data_ptr() for p in mine]
    bufs = (fopt.flat_p.data_ptr(), fopt.ema.data_ptr())

    def inside():
        for p, o, ptr in zip(mine, fopt.offsets, ptrs):
            assert p.data_ptr() == ptr
            assert _same_bits(p.data.reshape(-1), e0[o:o + p.numel()])
        assert _same_bits(fopt.ema, p0)
        with pytest.raises(RuntimeError, match="ema_weights"):
            fopt.step()
        with pytest.raises(RuntimeError, match="nest"):
            with fopt.ema_weights():
                pass

    def outside():
        assert _same_bits(fopt.flat_p, p0) and _same_bits(fopt.ema, e0)
        assert [p.data_ptr() for p in mine] == ptrs and (fopt.flat_p.data_ptr(), fopt.ema.data_ptr()) == bufs

    with fopt.ema_weights():
        inside()
    outside()
    with pytest.raises(ZeroDivisionError):
        with fopt.ema_weights():
            inside()
            1 / 0
    outside()
    _set_grads(mine, [g.to(dev) for g in _draw(mine, torch.Generator().manual_seed(25), 1.0)])
    fopt.step()                                          # steps again after the context
    assert fopt.t == 3 and not torch.equal(fopt.flat_p, p0)
    with pytest.raises(RuntimeError, match="no moving average"):
        with FlatAdam(_params(dev, 1), lr=1e-2).ema_weights():
            pass


def test_ema_weights_emu(use_emu):
    _run_ema_weights("cpu")


@pytest.mark.gpu
def test_ema_weights_gpu(hip_lib):
    _run_ema_weights("cuda")


# ---- 5. checkpoint ------------------------------------------------------------------------------------------------------
class _Net(torch.nn.Module):
    """the parameters of _params under a module's keys, one frozen parameter and one buffer (neither lives in flat_p)"""

    def __init__(self, dev, seed):
        super().__init__()
        self.w = torch.nn.ParameterList(_params(dev, seed))
        self.frozen = torch.nn.Parameter(torch.full((5,), 2.0, device=dev), requires_grad=False)
        self.register_buffer("table", torch.arange(7.0, device=dev))


def _run_checkpoint(dev):
    net = _Net(dev, 1)
    fopt = FlatAdam(net.parameters(), lr=1e-2, ema_decay=DECAY)
    gen = torch.Generator().manual_seed(26)
    for _ in range(2):
        _set_grads(fopt.params, [g.to(dev) for g in _draw(fopt.params, gen, 1.0)])
        fopt.step()
    e0 = fopt.ema.clone()
    sd = fopt.ema_state_dict(net)
    assert list(sd.keys()) == list(net.state_dict().keys())
    fresh = _Net(dev, 99)
    fresh.load_state_dict(sd, strict=True)
    named = dict(fresh.named_parameters())
    for i, (p, o) in enumerate(zip(fopt.params, fopt.offsets)):
        assert _same_bits(named[f"w.{i}"].data.reshape(-1), e0[o:o + p.numel()])
        assert sd[f"w.{i}"].data_ptr() != fopt.ema.data_ptr() + 4 * o      # a clone, not a view of the average
    assert torch.equal(sd["frozen"], net.frozen) and torch.equal(sd["table"], net.table)
    assert _same_bits(fopt.ema, e0)
    # reset_ema(): the average becomes the parameters; load_ema_state_dict brings the saved one back bitwise
    fopt.reset_ema()
    assert _same_bits(fopt.ema, fopt.flat_p) and not torch.equal(fopt.ema, e0)
    fopt.load_ema_state_dict(net, sd)
    assert _same_bits(fopt.ema, e0)
    # a missing key, a wrong shape: an error, and nothing written
    fopt.reset_ema()
    with pytest.raises(KeyError, match="w.4"):
        fopt.load_ema_state_dict(net, {k: v for k, v in sd.items() if k != "w.4"})
    with pytest.raises(ValueError, match="shape"):
        fopt.load_ema_state_dict(net, dict(sd, **{"w.4": sd["w.4"].reshape(17, 33)}))
    assert _same_bits(fopt.ema, fopt.flat_p)
    # an optimiser without an average
    plain = FlatAdam(_Net(dev, 1).parameters(), lr=1e-2)
    for call in (lambda: plain.ema_state_dict(net), lambda: plain.load_ema_state_dict(net, sd), plain.reset_ema):
        with pytest.raises(RuntimeError, match="no moving average"):
            call()
    # the optimiser's own state_dict is torch.optim.Adam's and carries nothing of the average
    osd = fopt.state_dict()
    assert set(osd["state"][0].keys()) == {"step", "exp_avg", "exp_avg_sq"}
    topt = torch.optim.Adam(_params("cpu", 1), lr=1e-2)
    topt.load_state_dict(osd)
    assert float(topt.state_dict()["state"][0]["step"]) == 2.0


def test_checkpoint_emu(use_emu):
    _run_checkpoint("cpu")


@pytest.mark.gpu
def test_checkpoint_gpu(hip_lib):
    _run_checkpoint("cuda")


def _run_surface(dev):
    for bad in (0.0, 1.0, -0.5, 1.5, NAN):
        with pytest.raises(ValueError, match="ema_decay"):
            FlatAdam(_params(dev, 1), lr=1e-2, ema_decay=bad)
    # changed between steps like lr; a refused value raises at step() and takes no step
    fopt, mine = _stepped(dev, steps=1, ema_warmup=False)
    ref = _Ref64(fopt)
    fopt.ema_decay = 0.5
    _set_grads(mine, [g.to(dev) for g in _draw(mine, torch.Generator().manual_seed(27), 1.0)])
    fopt.step()
    ref.advance(fopt, _a32(2, False, 0.5))
    ref.check(fopt, "decay changed to 0.5")
    fopt.ema_decay = 1.0
    before = (fopt.flat_p.clone(), fopt.ema.clone())
    with pytest.raises(ValueError, match="ema_decay"):
        fopt.step()
    assert _same_bits(fopt.flat_p, before[0]) and _same_bits(fopt.ema, before[1]) and fopt.t == 2


def test_python_surface_emu(use_emu):
    _run_surface("cpu")


@pytest.mark.gpu
def test_python_surface_gpu(hip_lib):
    _run_surface("cuda")


# ---- 6. captured step (GPU only) ------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_captured_step_gpu(hip_lib):
    """ONE guarded step with the average captured with torch.cuda.graph on a single stream (a linear graph) and replayed three
    times, the gradient buffer rewritten in place between replays, equals four eager steps (the eager warm-up step counts) in all
    five buffers, bitwise: the warm-up's t is the device counter, not a scalar baked into the captured launch, and the second
    replay (non-finite gradient) leaves the average alone."""
    dev = "cuda"
    mine, twin = _params(dev, 1), _params(dev, 1)
    kw = dict(lr=1e-2, max_grad_norm=MAX_NORM, skip_nonfinite=True, ema_decay=DECAY, ema_warmup=True)
    fopt, eopt = FlatAdam(mine, **kw), FlatAdam(twin, **kw)
    gen = torch.Generator().manual_seed(28)
    flats = []
    for it in range(4):
        grads = _draw(mine, gen, 10.0 if it % 2 == 0 else 0.01)
        if it == 2:                                      # the second of the three replayed gradients
            grads[2].view(-1)[17] = NAN
        _set_grads(twin, [g.to(dev) for g in grads])
        flats.append(eopt.flat_g.clone())
        eopt.step()
    fopt.flat_g.copy_(flats[0])
    fopt.step()                                          # eager warm-up: it counts
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fopt.step()                                      # (recorded, not run)
    assert fopt.health()["step"] == 1
    for it in (1, 2, 3):
        fopt.flat_g.copy_(flats[it])
        graph.replay()
    torch.cuda.synchronize()
    h, he = fopt.health(), eopt.health()
    assert h == he and h["step"] == 3 and h["skipped"] == 1, (h, he)
    for a, b in ((fopt.flat_p, eopt.flat_p), (fopt.flat_g, eopt.flat_g), (fopt.exp_avg, eopt.exp_avg),
                 (fopt.exp_avg_sq, eopt.exp_avg_sq), (fopt.ema, eopt.ema)):
        assert _same_bits(a, b)
    assert not torch.equal(fopt.ema, fopt.flat_p)


# ---- 7. sampling from the average -----------------------------------------------------------------------------------------
def _run_sampling(dev):
    from oracle import framediff_oracle as fo
    from se3_diffusion_amd import sampler, train_step as ts
    from se3_diffusion_amd.data import se3_diffuser
    from se3_diffusion_amd.model.score_network import ScoreNetwork
    from test_diffuser import conf as dconf
    B, N, num_t = 1, 12, 4
    diff = se3_diffuser.SE3Diffuser(dconf())

    def net():
        m = ScoreNetwork(ts.base_model_conf(1), diff)
        m.load_state_dict(fo.synth_params(seed=3, conf=dict(fo.CONF, num_blocks=1)), strict=True)
        return m.to(dev)

    model = net()
    fopt = FlatAdam(model.parameters(), lr=1e-3, ema_decay=DECAY)
    gen = torch.Generator().manual_seed(29)
    for _ in range(2):
        _set_grads(fopt.params, [g.to(dev) for g in _draw(fopt.params, gen, 1.0)])
        fopt.step()
    assert not torch.equal(fopt.ema, fopt.flat_p)
    rng = np.random.default_rng(30)
    feats = sampler.init_feats(diff, B, N, dev, noise=(rng.standard_normal((B * N, 3)), rng.random(B * N),
                                                       rng.standard_normal((B * N, 3))))
    zr, zt = rng.standard_normal((num_t, B, N, 3)), rng.standard_normal((num_t, B, N, 3))
    run = lambda m: sampler.sample(m, diff, feats, num_t=num_t, noise_fn=lambda i, shp: (zr[i], zt[i]))
    with fopt.ema_weights():
        got = run(model)
    second = net()
    second.load_state_dict(fopt.ema_state_dict(model), strict=True)
    want = run(second)
    for k in ("rigids", "atom37", "psi"):
        assert bool(torch.isfinite(got[k]).all())
        assert torch.equal(got[k], want[k]), k


def test_sampling_from_the_average_emu(use_emu):
    _run_sampling("cpu")


@pytest.mark.gpu
def test_sampling_from_the_average_gpu(hip_lib):
    _run_sampling("cuda")
