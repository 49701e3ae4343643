"""Cost of the guarded optimiser step at the full flat size (ScoreNetwork of config/base.yaml, 17.4 M parameters): HIP-event
times of
    plain     fd_adam_step                      (this tree's library)       28 B / parameter
    parent    fd_adam_step                      (--parent-lib: the library built from the parent commit; same kernel source)
    stats     fd_grad_stats                     (partials + finalize)        4 B / parameter
    guarded   fd_adam_step_guarded              (stats + decide + update)   32 B / parameter
alternating per repetition after a warm-up, median and range of each, the ratio guarded / plain and the HBM rate the bytes
above imply (against 8 TB/s).  --flush (default) writes a 512 MiB buffer before every timed call, outside the event pair, so
that each call finds its operands in HBM as it does inside a training step (the four 70 MB buffers would otherwise sit
partly in the 256 MiB Infinity Cache between back-to-back calls); --no-flush times them back to back.

    python tools/bench_optim.py [--parent-lib PATH] [--reps 50] [--out FILE]

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


def parent_adam(path):
    """fd_adam_step of another build of the library (it predates the guarded entry points, so hip.FdLib -- which binds every
    symbol of this tree's header -- cannot load it)."""
    cdll = ctypes.CDLL(path)
    fn = cdll.fd_adam_step
    fn.restype = ctypes.c_int
    fn.argtypes = [hip._CT[c] for c in hip._SIGS["fd_adam_step"]]
    return fn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-flush", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU (a timing taken anywhere else says nothing)"
    dev = "cuda"
    lib = hip.get_lib()
    model = ScoreNetwork(ts.base_model_conf(), diffuser=None).to(dev).train()
    opt = FlatAdam(model.parameters(), lr=1e-4, adjacent=model.flat_layout_groups(), max_grad_norm=1.0, skip_nonfinite=True)
    n = opt.numel
    opt.flat_g.normal_(generator=torch.Generator(device=dev).manual_seed(0)).mul_(1e-3)
    stats = torch.zeros(4, dtype=torch.float64, device=dev)
    b1, b2 = opt.betas
    stream = torch.cuda.current_stream().cuda_stream
    ptrs = [t.data_ptr() for t in (opt.flat_p, opt.flat_g, opt.exp_avg, opt.exp_avg_sq)]
    calls = {
        "plain": lambda: lib.call("fd_adam_step", opt.flat_p, opt.flat_g, opt.exp_avg, opt.exp_avg_sq, n, opt.lr, b1, b2, opt.eps,
                                  1.0 - b1 ** 10, 1.0 - b2 ** 10),
        "stats": lambda: lib.call("fd_grad_stats", opt.flat_g, n, opt._ws, stats),
        "guarded": lambda: lib.call("fd_adam_step_guarded", opt.flat_p, opt.flat_g, opt.exp_avg, opt.exp_avg_sq, n, opt.lr, b1, b2,
                                    opt.eps, 1.0, 1, opt._ws, opt._opt_state),
    }
    if a.parent_lib:
        pfn = parent_adam(a.parent_lib)

        def parent():
            rc = pfn(*ptrs, n, opt.lr, b1, b2, opt.eps, 1.0 - b1 ** 10, 1.0 - b2 ** 10, stream)
            assert rc == 0, rc
        calls["parent"] = parent
    order = [k for k in ("plain", "parent", "stats", "guarded") if k in calls]
    flush = None if a.no_flush else torch.empty(512 << 20, dtype=torch.uint8, device=dev)
    events = {k: [] for k in order}
    for rep in range(a.warmup + a.reps):
        for k in order:
            if flush is not None:
                flush.fill_(rep & 0xff)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            calls[k]()
            e1.record()
            if rep >= a.warmup:
                events[k].append((e0, e1))
    torch.cuda.synchronize()
    h = opt.health()
    assert h["skipped"] == 0 and h["step"] == a.warmup + a.reps, h
    bytes_per = {"plain": 28, "parent": 28, "stats": 4, "guarded": 32}
    us = {k: sorted(1e3 * e0.elapsed_time(e1) for e0, e1 in v) for k, v in events.items()}
    lines = [f"flat size {n} fp32 elements ({4 * n / 1e6:.1f} MB per buffer), {a.reps} repetitions after {a.warmup} warm-up, alternating, "
             f"HIP events around each call ({'operands flushed from the Infinity Cache before each call' if flush is not None else 'back to back, no flush'})",
             f"{'call':8s} {'median us':>10s} {'min':>8s} {'max':>8s} {'B/param':>8s} {'TB/s at median':>15s} {'of 8 TB/s':>10s}"]
    for k in order:
        med = statistics.median(us[k])
        rate = bytes_per[k] * n / (med * 1e-6)
        lines.append(f"{k:8s} {med:10.1f} {us[k][0]:8.1f} {us[k][-1]:8.1f} {bytes_per[k]:8d} {rate / 1e12:15.2f} {rate / HBM_PEAK:10.2f}")
    mp, mg = statistics.median(us["plain"]), statistics.median(us["guarded"])
    lines.append(f"guarded / plain = {mg / mp:.3f} (expected from bytes 32/28 = 1.143 plus two dependent launch boundaries)")
    if "parent" in us:
        lines.append(f"plain / parent  = {mp / statistics.median(us['parent']):.3f} (same kernel source)")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
