"""What the secondary-structure assignment costs on the device (profiles/dssp_cost.txt).

    python tools/measure_dssp_cost.py

HIP events around each call, all shapes in ONE process, alternating per repetition, 5 rounds of 10 repetitions after 3 warm-up
calls; "round medians" = the lowest and highest of the five per-round medians (the spread of one shape against itself).  Per
shape: fd_dssp_hbonds and fd_dssp_assign (lib.call on prepared operands), fd_backbone_metrics on the same atoms in the same
process as the yardstick, and the Python entry point metrics.secondary_structure (allocations and the ss3 arithmetic included).
fd_dssp_assign is also timed on an EMPTY bonded table (acc_idx = -1 everywhere: no turn, no ladder, nothing to link): what is
left is the compaction, the all-pairs bridge sweep and the radius of gyration, so the difference to the full call is the cost of
walking, linking and labelling the ladders; and with natoms = 5 on the same atom37 (the radius then reads 5 atom slots per
residue instead of 37), so the difference to the full call is 32 / 37 of the radius of gyration's two passes.  Nothing is
replaced by these kernels, so there is no threshold: the figures are a record.

Inputs: the deposited chains of tests/golden/dssp_chains.npz, concatenated 100 A apart until N residues are reached (real
hydrogen-bond density; the joints are chain breaks by the 2.5 A rule), as atom37 with the 32 side-chain slots zero.
"""
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def chains(N):
    g = np.load(os.path.join(ROOT, "tests", "golden", "dssp_chains.npz"))
    out, k = [], 0
    while sum(len(c) for c in out) < N:
        name = str(g["names"][k % 6])
        out.append(g[f"{name}_xyz"].astype(np.float64) + 100.0 * (k + 1))
        k += 1
    bb = np.concatenate(out)[:N]
    a37 = np.zeros((N, 37, 3), np.float32)
    a37[:, 0], a37[:, 1], a37[:, 2], a37[:, 4] = bb[:, 0], bb[:, 1], bb[:, 2], bb[:, 3]
    b, c = bb[:, 1] - bb[:, 0], bb[:, 2] - bb[:, 1]
    a37[:, 3] = -0.58273431 * np.cross(b, c) + 0.56802827 * b - 0.54067466 * c + bb[:, 1]
    return a37


def main():
    import torch
    from se3_diffusion_amd import hip, metrics as fm
    assert torch.cuda.is_available(), "needs an AMD GPU (no CPU fallback)"
    dev = "cuda"
    lib = hip.get_lib()
    calls, shapes = {}, []

    def add(B, N):
        tag = f"B={B} N={N}"
        atoms = torch.from_numpy(chains(N))[None].repeat(B, 1, 1, 1).contiguous().to(dev)
        mask = torch.ones(B, N, device=dev)
        idx = torch.empty(B, N, 2, dtype=torch.int32, device=dev)
        e = torch.empty(B, N, 2, dtype=torch.float64, device=dev)
        none = torch.full((B, N, 2), -1, dtype=torch.int32, device=dev)
        ss = torch.empty(B, N, dtype=torch.int8, device=dev)
        out = torch.empty(B, 8, dtype=torch.float64, device=dev)
        bo = torch.empty(B, 12, dtype=torch.float64, device=dev)
        calls[f"fd_dssp_hbonds          {tag}"] = lambda: lib.call("fd_dssp_hbonds", atoms, 111, mask, None, B, N, idx, e)
        calls[f"fd_dssp_assign          {tag}"] = lambda: lib.call("fd_dssp_assign", atoms, 111, 37, mask, idx, e, B, N, ss, out)
        calls[f"fd_dssp_assign (empty)  {tag}"] = lambda: lib.call("fd_dssp_assign", atoms, 111, 37, mask, none, e, B, N, ss, out)
        calls[f"fd_dssp_assign (5 atoms){tag}"] = lambda: lib.call("fd_dssp_assign", atoms, 111, 5, mask, idx, e, B, N, ss, out)
        calls[f"fd_backbone_metrics     {tag}"] = lambda: lib.call("fd_backbone_metrics", atoms, 111, mask, B, N, bo)
        calls[f"secondary_structure     {tag}"] = lambda: fm.secondary_structure(atoms, mask)
        shapes.append((tag, atoms, mask))

    for B, N in ((1, 128), (32, 128), (8, 512), (1, 2048)):
        add(B, N)
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
    print(f"{'call':<40} {'median us':>10} {'min':>10} {'max':>10}   round medians")
    for n in names:
        allt = [t for r in times[n] for t in r]
        meds = [statistics.median(r) for r in times[n]]
        med[n] = statistics.median(allt)
        print(f"{n:<40} {med[n]:10.1f} {min(allt):10.1f} {max(allt):10.1f}   {min(meds):9.1f} - {max(meds):9.1f}")
    print()
    print(f"{'shape':<14} {'hbonds us':>10} {'assign us':>10} {'assign/hbonds':>14} {'empty table us':>15} {'5 atoms us':>11} "
          f"{'backbone us':>12} {'helix':>6} {'strand':>7} {'hbonds':>7} {'overflow':>9}")
    for tag, atoms, mask in shapes:
        res = fm.secondary_structure(atoms, mask)
        th, ta = med[f"fd_dssp_hbonds          {tag}"], med[f"fd_dssp_assign          {tag}"]
        print(f"{tag:<14} {th:10.1f} {ta:10.1f} {ta / th:14.2f} {med[f'fd_dssp_assign (empty)  {tag}']:15.1f} "
              f"{med[f'fd_dssp_assign (5 atoms){tag}']:11.1f} {med[f'fd_backbone_metrics     {tag}']:12.1f} {res['helix_percent'][0].item():6.3f} {res['strand_percent'][0].item():7.3f} "
              f"{res['num_hbonds'][0].item():7.0f} {res['overflow'][0].item():9.0f}")


if __name__ == "__main__":
    main()
