"""What TM-align's alignment search costs on the device (profiles/tm_align_cost.txt).

    python tools/measure_tm_align_cost.py

HIP events around each call, all shapes in ONE process, alternating per repetition, 3 rounds of up to 5 repetitions after 2
warm-up calls (fewer repetitions for a shape whose call takes long: about 2 s per shape and round); "round medians" = the lowest
and highest of the per-round medians (the spread of one shape against itself).  Per shape: fd_tm_align (seed, refine and final
launches, lib.call on prepared operands, the split metrics.tm_align_parts picks), the time per pair, the mean number of refinement
DPs and of seed units per pair (slots 9 and 10, exact integers) and the mean tm_norm_b; for the record fd_tm_search (the
superposition search of a GIVEN correspondence) on the same number of pairs of N = Na positions in the same process.  Chains are
unrelated random walks of 3.8 A steps: the case in which no class converges early.  No time target is set.

The DP form that shipped is the wave-systolic anti-diagonal sweep (lane l owns a row of a 64-row strip, the row above arrives by
__shfl, two bits per cell for the traceback); the block-wide form with a barrier per diagonal was not built, so there is no A/B.
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
        return torch.cumsum(3.8 * steps / steps.norm(dim=-1, keepdim=True), dim=1).to(dev)

    calls, shapes = {}, []

    def add(P, Na, Nb, search=False):
        tag = f"P={P} {Na}x{Nb}"
        M = 2
        while M * (M - 1) // 2 < P:
            M += 1
        a, b = walk(M, Na), walk(M, Nb)
        iu = torch.triu_indices(M, M, 1, device=dev).to(torch.int32)
        ia, ib = iu[0][:P].contiguous(), iu[1][:P].contiguous()
        parts = fm.tm_align_parts(P, Na, Nb)
        ws = torch.empty(fm.tm_align_ws_bytes(P, parts, Na, Nb) // 8 + 1, dtype=torch.float64, device=dev)
        out = torch.empty(P, 16, dtype=torch.float64, device=dev)
        amap = torch.empty(P, Na, dtype=torch.int32, device=dev)
        calls[f"fd_tm_align  {tag}"] = lambda: lib.call("fd_tm_align", a, 3, Na, b, 3, Nb, ia, ib, None, None, P, 40, 30, parts, ws,
                                                        out, amap, None)
        if search:
            sp = fm.tm_parts(P, Na, 1)
            sws = torch.empty(P * sp * 64, dtype=torch.float64, device=dev)
            so = torch.empty(P, 8, dtype=torch.float64, device=dev)
            a2 = walk(M, Na)
            calls[f"fd_tm_search {tag}"] = lambda: lib.call("fd_tm_search", a, 3, a2, 3, ia, ib, None, P, Na, 1, 20, sp, sws, so, None)
        shapes.append((tag, P, parts, out, search))

    for P in (1, 64, 2016):
        add(P, 128, 128, search=True)
    add(64, 128, 256)
    add(8, 512, 512)
    add(64, 512, 512)

    names = list(calls)
    reps = {}
    for n in names:
        calls[n]()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        calls[n]()
        e1.record()
        e1.synchronize()
        reps[n] = max(1, min(5, int(2000.0 / max(e0.elapsed_time(e1), 1e-3))))
    rounds = 3
    times = {n: [[] for _ in range(rounds)] for n in names}
    for r in range(rounds):
        for k in range(5):
            order = names[(r * 5 + k) % len(names):] + names[:(r * 5 + k) % len(names)]
            for n in order:
                if k >= reps[n]:
                    continue
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                calls[n]()
                e1.record()
                e1.synchronize()
                times[n][r].append(e0.elapsed_time(e1) * 1e3)
    med = {}
    print(f"{rounds} rounds of up to 5 repetitions after 2 warm-up calls, alternating, HIP events around each call")
    print(f"{'call':<30} {'reps':>5} {'median us':>12} {'min':>12} {'max':>12}   round medians")
    for n in names:
        allt = [t for r in times[n] for t in r]
        meds = [statistics.median(r) for r in times[n]]
        med[n] = statistics.median(allt)
        print(f"{n:<30} {reps[n]:5d} {med[n]:12.1f} {min(allt):12.1f} {max(allt):12.1f}   {min(meds):11.1f} - {max(meds):11.1f}")
    print()
    print(f"{'shape':<18} {'pairs':>6} {'parts':>6} {'DPs/pair':>9} {'units/pair':>11} {'mean tm_b':>10} {'align us':>12} {'us/pair':>10} "
          f"{'search us/pair':>15}")
    for tag, P, parts, out, search in shapes:
        o = out.cpu()
        t = med[f"fd_tm_align  {tag}"]
        ts = f"{med[f'fd_tm_search {tag}'] / P:15.1f}" if search else f"{'-':>15}"
        print(f"{tag:<18} {P:6d} {parts:6d} {o[:, 9].mean().item():9.1f} {o[:, 10].mean().item():11.1f} {o[:, 4].mean().item():10.4f} "
              f"{t:12.1f} {t / P:10.1f} {ts}")
    print()
    print("DP form: wave-systolic anti-diagonal sweep (the block-wide barrier-per-diagonal form was not built: no A/B).")


if __name__ == "__main__":
    main()
