"""What scoring sampled backbones costs on the device (profiles/sample_metrics_cost.txt).

    python tools/measure_metrics_cost.py

HIP events around each call, all shapes in ONE process, alternating per repetition, 5 rounds of 50 repetitions after 5 warm-up
calls; "round medians" = the lowest and highest of the five per-round medians (the spread of one shape against itself).  Two
figures per shape: the library launch alone (lib.call on prepared operands) and the Python entry point a user calls
(metrics.backbone_metrics / metrics.pairwise_rmsd: output allocation, index tensors and the mirroring scatter included).
Pair work from shapes: n (n - 1) / 2 distances per backbone; 3 passes over 2 N points per superposed pair.
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
        ca = torch.cumsum(3.8 * steps / steps.norm(dim=-1, keepdim=True), dim=1)
        a37 = torch.zeros(B, N, 37, 3)
        a37[:, :, :5] = ca[:, :, None, :] + torch.randn(B, N, 5, 3, generator=g)
        a37[:, :, 1] = ca
        return a37.to(dev)

    calls = {}
    for B, N in ((1, 128), (8, 512), (1, 4096)):
        a37, mask = walk(B, N), torch.ones(B, N, device=dev)
        out = torch.empty(B, 12, dtype=torch.float64, device=dev)
        calls[f"fd_backbone_metrics B={B} N={N}"] = (
            lambda a37=a37, mask=mask, out=out, B=B, N=N: lib.call("fd_backbone_metrics", a37, 111, mask, B, N, out),
            f"{B * N * (N - 1) // 2} pairs")
        calls[f"backbone_metrics    B={B} N={N}"] = (lambda a37=a37, mask=mask: fm.backbone_metrics(a37, mask), "")
    M, N = 64, 128
    pos = walk(M, N)[:, :, 1].contiguous()
    iu = torch.triu_indices(M, M, 1, device=dev).to(torch.int32)
    ia, ib = iu[0].contiguous(), iu[1].contiguous()
    po = torch.empty(ia.numel(), 8, dtype=torch.float64, device=dev)
    calls[f"fd_aligned_rmsd     M={M} N={N}"] = (
        lambda: lib.call("fd_aligned_rmsd", pos, 3, pos, 3, ia, ib, None, ia.numel(), N, po, None), f"{ia.numel()} pairs")
    calls[f"pairwise_rmsd       M={M} N={N}"] = (lambda: fm.pairwise_rmsd(pos), "")

    names = list(calls)
    for n in names:
        for _ in range(5):
            calls[n][0]()
    torch.cuda.synchronize()
    rounds, reps = 5, 50
    times = {n: [[] for _ in range(rounds)] for n in names}
    for r in range(rounds):
        for k in range(reps):
            order = names[(r * reps + k) % len(names):] + names[:(r * reps + k) % len(names)]
            for n in order:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                calls[n][0]()
                e1.record()
                e1.synchronize()
                times[n][r].append(e0.elapsed_time(e1) * 1e3)
    print(f"{rounds} rounds of {reps} repetitions after 5 warm-up, alternating, HIP events around each call")
    print(f"{'call':<34} {'median us':>9} {'min':>8} {'max':>8}   round medians      work")
    for n in names:
        allt = [t for r in times[n] for t in r]
        meds = [statistics.median(r) for r in times[n]]
        print(f"{n:<34} {statistics.median(allt):9.1f} {min(allt):8.1f} {max(allt):8.1f}   {min(meds):7.1f} - {max(meds):7.1f}   {calls[n][1]}")


if __name__ == "__main__":
    main()
