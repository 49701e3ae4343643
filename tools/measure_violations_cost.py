"""What the violation losses cost on the device (profiles/violations_cost.txt).

    python tools/measure_violations_cost.py

One child process per shape, one after the other (a failing child ends the run); in it HIP events around each call, 3 warm-up
calls, then 5 rounds of 10 repetitions alternating between the calls, the median over all 50 and the lowest and highest of the
five per-round medians (the spread of one call against itself).  Per shape: fd_violations without and with the optional
per-residue arrays (lib.call on prepared operands: both of its launches), the Python entry point metrics.violations (allocations
included), and for scale fd_dssp_hbonds on the same atoms -- the launch of the same form (64-residue tiles x backbones, the whole
chain staged in LDS by every block).  Nothing is replaced by this kernel, so there is no threshold: the figures are a record.

Inputs: tools/measure_dssp_cost.py's -- the deposited chains of tests/golden/dssp_chains.npz, concatenated 100 A apart until N
residues are reached, as atom37 with the 32 side-chain slots zero, every residue present.
"""
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
SHAPES = ((1, 128), (32, 128), (8, 512), (1, 2048))


def one_shape(B, N):
    import torch
    from measure_dssp_cost import chains
    from se3_diffusion_amd import hip, metrics as fm
    assert torch.cuda.is_available(), "needs an AMD GPU (no CPU fallback)"
    dev = "cuda"
    lib = hip.get_lib()
    atoms = torch.from_numpy(chains(N))[None].repeat(B, 1, 1, 1).contiguous().to(dev)
    mask = torch.ones(B, N, device=dev)
    ws = torch.empty(B * (-(-N // fm.VIOLATIONS_TILE)) * 16, dtype=torch.float64, device=dev)
    out = torch.empty(B, 16, dtype=torch.float64, device=dev)
    res_loss = torch.empty(B, N, dtype=torch.float64, device=dev)
    atom_loss = torch.empty(B, N, 5, dtype=torch.float64, device=dev)
    flags = torch.empty(B, N, dtype=torch.uint8, device=dev)
    idx = torch.empty(B, N, 2, dtype=torch.int32, device=dev)
    e = torch.empty(B, N, 2, dtype=torch.float64, device=dev)
    calls = {
        "fd_violations": lambda: lib.call("fd_violations", atoms, 111, mask, None, B, N, ws, out, None, None, None),
        "fd_violations (arrays)": lambda: lib.call("fd_violations", atoms, 111, mask, None, B, N, ws, out, res_loss, atom_loss, flags),
        "violations": lambda: fm.violations(atoms, mask),
        "fd_dssp_hbonds": lambda: lib.call("fd_dssp_hbonds", atoms, 111, mask, None, B, N, idx, e),
    }
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
    res = fm.violations(atoms, mask)
    for n in names:
        allt = [t for r in times[n] for t in r]
        meds = [statistics.median(r) for r in times[n]]
        print(f"{n + f'  B={B} N={N}':<40} {statistics.median(allt):10.1f} {min(allt):10.1f} {max(allt):10.1f}   "
              f"{min(meds):9.1f} - {max(meds):9.1f}")
    print(f"    B={B} N={N}: atom pairs {res['num_atom_pairs'][0].item():.0f}, clashing {res['num_clashing_pairs'][0].item():.0f}, "
          f"bonds {res['num_bonds'][0].item():.0f}, bonds_c_n_loss_mean {res['bonds_c_n_loss_mean'][0].item():.3e}, "
          f"clashes_mean_loss {res['clashes_mean_loss'][0].item():.3e}", flush=True)


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "--shape":
        return one_shape(int(sys.argv[2]), int(sys.argv[3]))
    print("one process per shape; 5 rounds of 10 repetitions after 3 warm-up, alternating, HIP events around each call")
    print(f"{'call':<40} {'median us':>10} {'min':>10} {'max':>10}   round medians", flush=True)
    for B, N in SHAPES:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--shape", str(B), str(N)], timeout=120)
        if r.returncode != 0:
            sys.exit(f"shape B={B} N={N} failed with status {r.returncode}: nothing further is run")


if __name__ == "__main__":
    main()
