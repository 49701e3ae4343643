"""Cost of the guarded optimiser step and of the moving average at the full flat size (ScoreNetwork of config/base.yaml, 17.4 M
parameters): HIP-event times of
    plain        fd_adam_step                   (this tree's library)       28 B / parameter
    parent       fd_adam_step                   (--parent-lib: the library built from the parent commit)
    stats        fd_grad_stats                  (partials + finalize)        4 B / parameter
    guarded      fd_adam_step_guarded           (stats + decide + update)   32 B / parameter
    parent_g     fd_adam_step_guarded           (--parent-lib)
    ema          fd_adam_step_ema               (update + average)          36 B / parameter
    guarded_ema  fd_adam_step_guarded_ema       (stats + decide + update + average)  40 B / parameter
alternating per repetition (the order rotated by one each time) after a warm-up, in --rounds rounds: median and range of each over all repetitions, the range of its
round medians, the ratios and the HBM rate the bytes above imply (against 8 TB/s).  With --parent-lib one condition is judged:
the medians of plain and guarded must lie inside the range of the round medians of the parent library's same entry point, the
spread one library shows against itself in this call (templating the update kernels must cost the untemplated path nothing).
--flush (default) writes a 512 MiB buffer before every timed call, outside the event pair, so that each call finds its operands
in HBM as it does inside a training step (the 70 MB buffers would otherwise sit partly in the 256 MiB Infinity Cache between
back-to-back calls); --no-flush times them back to back.

    python tools/bench_optim.py [--parent-lib PATH] [--reps 50] [--rounds 5] [--out FILE]

Per-launch times come from a profiler run of their own: rocprofv3 --kernel-trace --stats -- python tools/bench_optim.py"""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from se3_diffusion_amd import hip, train_step as ts  # noqa: E402
from se3_diffusion_amd.model.score_network import ScoreNetwork  # noqa: E402
from se3_diffusion_amd.optim import FlatAdam  # noqa: E402

HBM_PEAK = 8.0e12


def parent_lib(path):
    """fd_adam_step and fd_adam_step_guarded of another build of the library (it predates this tree's newest entry points, so
    hip.FdLib -- which binds every symbol of this tree's header -- cannot load it)."""
    cdll = ctypes.CDLL(path)
    fns = []
    for name in ("fd_adam_step", "fd_adam_step_guarded"):
        fn = getattr(cdll, name)
        fn.restype = ctypes.c_int
        fn.argtypes = [hip._CT[c] for c in hip._SIGS[name]]
        fns.append(fn)
    return fns


BYTES_PER = {"plain": 28, "parent": 28, "stats": 4, "guarded": 32, "parent_g": 32, "ema": 36, "guarded_ema": 40}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-flush", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU (a timing taken anywhere else says nothing)"
    dev = "cuda"
    lib = hip.get_lib()
    model = ScoreNetwork(ts.base_model_conf(), diffuser=None).to(dev).train()
    opt = FlatAdam(model.parameters(), lr=1e-4, adjacent=model.flat_layout_groups(), max_grad_norm=1.0, skip_nonfinite=True,
                   ema_decay=0.999)
    n = opt.numel
    opt.flat_g.normal_(generator=torch.Generator(device=dev).manual_seed(0)).mul_(1e-3)
    stats = torch.zeros(4, dtype=torch.float64, device=dev)
    b1, b2 = opt.betas
    bc1, bc2 = 1.0 - b1 ** 10, 1.0 - b2 ** 10
    stream = torch.cuda.current_stream().cuda_stream
    bufs = (opt.flat_p, opt.flat_g, opt.exp_avg, opt.exp_avg_sq)
    calls = {
        "plain": lambda: lib.call("fd_adam_step", *bufs, n, opt.lr, b1, b2, opt.eps, bc1, bc2),
        "stats": lambda: lib.call("fd_grad_stats", opt.flat_g, n, opt._ws, stats),
        "guarded": lambda: lib.call("fd_adam_step_guarded", *bufs, n, opt.lr, b1, b2, opt.eps, 1.0, 1, opt._ws, opt._opt_state),
        "ema": lambda: lib.call("fd_adam_step_ema", *bufs, opt.ema, n, opt.lr, b1, b2, opt.eps, bc1, bc2, 1.0 - opt.ema_decay),
        "guarded_ema": lambda: lib.call("fd_adam_step_guarded_ema", *bufs, opt.ema, n, opt.lr, b1, b2, opt.eps, 1.0, 1, opt._ws,
                                        opt._opt_state, opt.ema_decay, 1),
    }
    if a.parent_lib:
        p_adam, p_guarded = parent_lib(a.parent_lib)
        ptrs = [t.data_ptr() for t in bufs]

        def parent():
            rc = p_adam(*ptrs, n, opt.lr, b1, b2, opt.eps, bc1, bc2, stream)
            assert rc == 0, rc

        def parent_g():
            rc = p_guarded(*ptrs, n, opt.lr, b1, b2, opt.eps, 1.0, 1, opt._ws.data_ptr(), opt._opt_state.data_ptr(), stream)
            assert rc == 0, rc
        calls["parent"], calls["parent_g"] = parent, parent_g
    order = [k for k in ("plain", "parent", "stats", "guarded", "parent_g", "ema", "guarded_ema") if k in calls]
    guarded_calls = sum(k in calls for k in ("guarded", "parent_g", "guarded_ema"))
    flush = None if a.no_flush else torch.empty(512 << 20, dtype=torch.uint8, device=dev)
    rounds = []                                      # per round: {call: sorted us}
    for rnd in range(a.rounds):
        events = {k: [] for k in order}
        for rep in range(a.warmup + a.reps):
            # rotated: back to back a call finds in the Infinity Cache what its predecessor left there, so every call follows
            # every other one equally often
            for k in order[rep % len(order):] + order[:rep % len(order)]:
                if flush is not None:
                    flush.fill_(rep & 0xff)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                calls[k]()
                e1.record()
                if rep >= a.warmup:
                    events[k].append((e0, e1))
        torch.cuda.synchronize()
        rounds.append({k: sorted(1e3 * e0.elapsed_time(e1) for e0, e1 in v) for k, v in events.items()})
    h = opt.health()
    assert h["skipped"] == 0 and h["step"] == a.rounds * (a.warmup + a.reps) * guarded_calls, h
    us = {k: sorted(x for r in rounds for x in r[k]) for k in order}
    med = {k: statistics.median(us[k]) for k in order}
    rmed = {k: sorted(statistics.median(r[k]) for r in rounds) for k in order}
    lines = [f"flat size {n} fp32 elements ({4 * n / 1e6:.1f} MB per buffer), {a.rounds} rounds of {a.reps} repetitions after {a.warmup} warm-up, "
             f"alternating, HIP events around each call ({'operands flushed from the Infinity Cache before each call' if flush is not None else 'back to back, no flush'})",
             f"{'call':11s} {'median us':>10s} {'min':>8s} {'max':>8s} {'round medians':>17s} {'B/param':>8s} {'TB/s at median':>15s} {'of 8 TB/s':>10s}"]
    for k in order:
        rate = BYTES_PER[k] * n / (med[k] * 1e-6)
        lines.append(f"{k:11s} {med[k]:10.1f} {us[k][0]:8.1f} {us[k][-1]:8.1f} {rmed[k][0]:8.1f} -{rmed[k][-1]:7.1f} {BYTES_PER[k]:8d} "
                     f"{rate / 1e12:15.2f} {rate / HBM_PEAK:10.2f}")
    lines.append(f"guarded / plain       = {med['guarded'] / med['plain']:.3f} (expected from bytes 32/28 = 1.143 plus two dependent launch boundaries)")
    lines.append(f"ema / plain           = {med['ema'] / med['plain']:.3f} (expected from bytes 36/28 = 1.286)")
    lines.append(f"guarded_ema / guarded = {med['guarded_ema'] / med['guarded']:.3f} (expected from bytes 40/32 = 1.250)")
    if a.parent_lib:
        for mine, par in (("plain", "parent"), ("guarded", "parent_g")):
            lo, hi = rmed[par][0], rmed[par][-1]
            verdict = "inside" if lo <= med[mine] <= hi else "below (faster than)" if med[mine] < lo else "ABOVE"
            lines.append(f"{mine} / {par} = {med[mine] / med[par]:.3f}; {mine} median {med[mine]:.1f} us against the {par} round medians "
                         f"{lo:.1f} - {hi:.1f} us: {verdict} the spread of one library against itself")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
