"""What the TM-score search costs on the device (profiles/tm_search_cost.txt).

    python tools/measure_tm_cost.py

HIP events around each call, all shapes in ONE process, alternating per repetition, 5 rounds of 10 repetitions after 3 warm-up
calls; "round medians" = the lowest and highest of the five per-round medians (the spread of one shape against itself).  Per
shape: fd_tm_search (search + reduce launches, lib.call on prepared operands, the split metrics.tm_parts picks), the mean
number of score calls per pair (slot 6, an exact integer per pair), and fd_aligned_rmsd on the same pairs in the same process.
fd_aligned_rmsd is one superposition plus one residual pass over a pair, so its time per pair is the yardstick for one pass:
    ratio = t_search / (mean passes per pair * t_rmsd)
-- below 1 the search's passes are cheaper than that launch's, above 1 dearer.  No threshold is set on it.  The Python entry points
(metrics.pairwise_tm / metrics.tm_score: allocations, index tensors and the mirroring scatter included) are timed as well.
"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    from se3_diffusion_amd import hip, metrics as fm
    assert torch.cuda.is_available(), "needs an AMD GPU (no CPU fallback)"
    dev = "cuda"
    lib = hip.get_lib()
    g = torch.Generator().manual_seed(0)

    def walk(B, N):
        steps = torch.randn(B, N, 3, generator=g)
        return torch.cumsum(3.8 * steps / steps.norm(dim=-1, keepdim=True), dim=1)

    def moved(x, sigma):
        """a rigid copy of every set of x plus N(0, sigma) per coordinate: a sample near its ground truth"""
        q, _ = torch.linalg.qr(torch.randn(x.shape[0], 3, 3, generator=g))
        q = q * torch.linalg.det(q)[:, None, None]
        return x @ q.transpose(1, 2) + 10 * torch.randn(x.shape[0], 1, 3, generator=g) + sigma * torch.randn(x.shape, generator=g)

    calls, shapes = {}, []

    def add(tag, a, b, ia, ib, P, N, seed_step, parts=None):
        parts = fm.tm_parts(P, N, seed_step) if parts is None else parts
        ws = torch.empty(P * parts * 64, dtype=torch.float64, device=dev)
        out = torch.empty(P, 8, dtype=torch.float64, device=dev)
        po = torch.empty(P, 8, dtype=torch.float64, device=dev)
        calls[f"fd_tm_search    {tag}"] = lambda: lib.call("fd_tm_search", a, 3, b, 3, ia, ib, None, P, N, seed_step, 20, parts, ws,
                                                          out, None)
        calls[f"fd_aligned_rmsd {tag}"] = lambda: lib.call("fd_aligned_rmsd", a, 3, b, 3, ia, ib, None, P, N, po, None)
        shapes.append((tag, P, parts, out))

    M, N = 64, 128
    pos = walk(M, N).to(dev)
    iu = torch.triu_indices(M, M, 1, device=dev).to(torch.int32)
    ia, ib = iu[0].contiguous(), iu[1].contiguous()
    for step in (1, 8):
        add(f"M={M} N={N} seed_step={step}", pos, pos, ia, ib, ia.numel(), N, step)
    calls[f"pairwise_tm     M={M} N={N} seed_step=1"] = lambda: fm.pairwise_tm(pos)
    gt = walk(8, 512)
    sample = moved(gt, 2.0).to(dev)
    gt = gt.to(dev)
    add("B=8 N=512 to ground truth", sample, gt, None, None, 8, 512, 1)
    for parts in (64, 128):                                  # beside the 96 of tm_parts: 512 and 1024 blocks against 768 resident
        add(f"B=8 N=512 parts={parts}", sample, gt, None, None, 8, 512, 1, parts)
    calls["tm_score        B=8 N=512 to ground truth"] = lambda: fm.tm_score(sample, gt)
    one = walk(1, 2048)
    one_b = moved(one, 2.0).to(dev)
    one = one.to(dev)
    add("P=1 N=2048 seed_step=64", one, one_b, None, None, 1, 2048, 64)

    names = list(calls)
    for n in names:
        for _ in range(3):
            calls[n]()
    torch.cuda.synchronize()
    rounds, reps = 5, 10
    times = {n: [[] for _ in range(rounds)] for n in names}
    for r in range(rounds):
        for k in range(reps):
            order = names[(r * reps + k) % len(names):] + names[:(r * reps + k) % len(names)]
            for n in order:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                calls[n]()
                e1.record()
                e1.synchronize()
                times[n][r].append(e0.elapsed_time(e1) * 1e3)
    med = {}
    print(f"{rounds} rounds of {reps} repetitions after 3 warm-up, alternating, HIP events around each call")
    print(f"{'call':<46} {'median us':>10} {'min':>10} {'max':>10}   round medians")
    for n in names:
        allt = [t for r in times[n] for t in r]
        meds = [statistics.median(r) for r in times[n]]
        med[n] = statistics.median(allt)
        print(f"{n:<46} {med[n]:10.1f} {min(allt):10.1f} {max(allt):10.1f}   {min(meds):9.1f} - {max(meds):9.1f}")
    print()
    print(f"{'shape':<30} {'pairs':>6} {'parts':>6} {'passes/pair':>12} {'mean tm':>8} {'search us':>10} {'rmsd us':>8} {'ratio':>7}")
    for tag, P, parts, out in shapes:
        o = out.cpu()
        passes = o[:, 6].mean().item()
        ts, tr = med[f"fd_tm_search    {tag}"], med[f"fd_aligned_rmsd {tag}"]
        print(f"{tag:<30} {P:6d} {parts:6d} {passes:12.1f} {o[:, 1].mean().item():8.4f} {ts:10.1f} {tr:8.1f} {ts / (passes * tr):7.3f}")


if __name__ == "__main__":
    main()
