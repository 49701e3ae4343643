"""What designing sequences for sampled backbones costs on the device (profiles/design_cost.txt).

    python tools/measure_design_cost.py [--out profiles/design_cost.txt]

--out: the table is also written to that file (the committed profile is this table between a heading and a reading written by
hand).  One child process per shape, one after the other (a failing child ends the run).  Per shape (B = 1 and 32 backbones of N = 128 and
256 residues, 8 sequences each, k_neighbors = 48, temperature 0.1): HIP events around each call, 3 warm-up calls, then 5 rounds of 6
repetitions alternating between the calls; the median over all 30 and the lowest and highest of the five per-round medians:
  fd_mpnn_graph     the launch alone on packed operands
  fd_mpnn_encoder   its eight launches alone (the three encoder layers and the decoder's per-backbone terms)
  fd_mpnn_decode    the one launch alone: B x 8 blocks, each walking its N steps -- divided by N, the latency of one decoding step
  design            SequenceDesigner.design: packing, the draws, the argsort, the three calls, the scores and the read-back of the
                    letters for the strings
beside the time the same backbones take to SAMPLE (500 steps; README: N=128 B=1 1.87-1.94 backbones/s, B=32 9.1-9.4, N=256 B=1
1.30-1.34; N=256 B=32 is not listed there).  There is no threshold: the parent commit has no such path and the reference's model
does not run where the GPU is.  Weights: tests/mpnn_weights.py (synthetic: the cost does not depend on their values).  Backbones:
CA random walks of 3.8 A steps with N, C and O at bond length.
"""
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
SHAPES = ((1, 128), (32, 128), (1, 256), (32, 256))
SAMPLING_BACKBONES_PER_S = {(1, 128): 1.90, (32, 128): 9.25, (1, 256): 1.32}      # README, middle of the stated ranges
SEQS = 8


def walk(rng, n):
    unit = lambda v: v / np.linalg.norm(v, axis=-1, keepdims=True)
    ca = np.cumsum(3.8 * unit(rng.normal(size=(n, 3))), 0)
    nn, c = ca + 1.46 * unit(rng.normal(size=(n, 3))), ca + 1.52 * unit(rng.normal(size=(n, 3)))
    return np.stack([nn, ca, c, c + 1.23 * unit(rng.normal(size=(n, 3)))], 1).astype(np.float32)


def timed(calls, rounds=5, reps=6):
    import torch
    names = list(calls)
    for n in names:
        for _ in range(3):
            calls[n]()
    torch.cuda.synchronize()
    times = {n: [[] for _ in range(rounds)] for n in names}
    for r in range(rounds):
        for k in range(reps):
            s = (r * reps + k) % len(names)
            for n in names[s:] + names[:s]:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                calls[n]()
                e1.record()
                e1.synchronize()
                times[n][r].append(e0.elapsed_time(e1) * 1e3)
    return {n: (statistics.median([t for r in times[n] for t in r]), min(t for r in times[n] for t in r),
                max(t for r in times[n] for t in r), [statistics.median(r) for r in times[n]]) for n in names}


def one_shape(B, N, dev="cuda"):
    import torch
    from mpnn_weights import make_state_dict
    from se3_diffusion_amd import hip
    from se3_diffusion_amd.design import H, NODE_SLOTS, SequenceDesigner
    assert torch.cuda.is_available(), "needs an AMD GPU (no CPU fallback)"
    lib = hip.get_lib()
    d = SequenceDesigner.from_state_dict(make_state_dict(20, 48), k_neighbors=48, device=dev)
    rng = np.random.default_rng(B * 1000 + N)
    atoms = torch.from_numpy(np.stack([walk(rng, N) for _ in range(B)])).to(dev)
    pk = d._pack(atoms, None, None)
    enc = d.encode(pk)
    T, K = pk["T"], d.k
    gen = torch.Generator(device=dev).manual_seed(0)
    order = torch.argsort(torch.rand((SEQS, B, N), generator=gen, device=dev), -1).to(torch.int32).reshape(SEQS, T).contiguous()
    uni = torch.rand((SEQS, T), generator=gen, device=dev)
    omit = torch.zeros(21, device=dev)
    omit[20] = 1.0
    bias = torch.zeros(21, device=dev)
    E2, hE2 = torch.empty_like(enc["E_idx"]), torch.empty_like(enc["h_E"])
    ws = torch.empty((T, NODE_SLOTS, H), device=dev)
    calls = {
        "fd_mpnn_graph": lambda: lib.call("fd_mpnn_graph", pk["atoms"], pk["res_index"], pk["offsets"], pk["chain_of"], T, K, d.gw,
                                          E2, hE2),
        "fd_mpnn_encoder": lambda: lib.call("fd_mpnn_encoder", enc["E_idx"], pk["offsets"], pk["chain_of"], T, K, d.ew, d.dw,
                                            enc["h_V"], hE2, enc["node"], ws, enc["EB"]),
        "fd_mpnn_decode": lambda: d._decode(pk, enc, order, None, None, uni, omit, bias, 0.1, False),
        "design": lambda: d.design(atoms, num_seqs=SEQS, generator=gen),
    }
    # (the timed encoder runs on a copy of the graph's h_E: it updates h_E in place, and `enc` keeps feeding the decoder)
    res = timed(calls)
    tag = f"B={B} N={N}"
    for n, (med, lo, hi, meds) in res.items():
        print(f"{n + '  ' + tag:<34} {med:11.1f} {lo:11.1f} {hi:11.1f}   {min(meds):10.1f} - {max(meds):10.1f}")
    dec = res["fd_mpnn_decode"][0]
    line = f"    {tag}: decode {dec / N:.1f} us per step ({B * SEQS} blocks); design {res['design'][0] / 1e3:.2f} ms for {B * SEQS} sequences"
    rate = SAMPLING_BACKBONES_PER_S.get((B, N))
    if rate:
        line += f" = {res['design'][0] / 1e6 / (B / rate) * 100:.2f} % of the {B / rate:.2f} s the {B} backbone(s) take to sample"
    else:
        line += "; the README lists no sampling time for this shape"
    out = d.design(atoms, num_seqs=SEQS, generator=gen)
    torch.cuda.synchronize()
    print(line)
    print(f"    {tag}: all finite {bool(torch.isfinite(out['log_probs']).all())}, mean score {float(out['score'].mean()):.3f}, "
          f"first sequence {out['seqs'][0][0][:32]}...", flush=True)


def main():
    if "--shape" in sys.argv:
        k = sys.argv.index("--shape")
        return one_shape(int(sys.argv[k + 1]), int(sys.argv[k + 2]))
    lines = ["one process per shape; 5 rounds of 6 repetitions after 3 warm-up, alternating, HIP events around each call",
             f"{'call':<34} {'median us':>11} {'min':>11} {'max':>11}   round medians"]
    print("\n".join(lines), flush=True)
    me = [sys.executable, os.path.abspath(__file__)]
    for B, N in SHAPES:
        r = subprocess.run(me + ["--shape", str(B), str(N)], timeout=240, stdout=subprocess.PIPE, text=True)
        print(r.stdout, end="", flush=True)
        lines.append(r.stdout.rstrip("\n"))
        if r.returncode != 0:
            sys.exit(f"shape B={B} N={N} failed with status {r.returncode}: nothing further is run")
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
