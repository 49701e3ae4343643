"""What clustering costs beside the TM matrix it consumes (profiles/cluster_cost.txt).

    python tools/measure_cluster_cost.py [--out FILE] [--max-tm-seconds S]

Per shape: the time of metrics.cluster (fd_cluster_linkage + fd_cluster_cut, average linkage, threshold 0.5) on a similarity matrix
of M samples drawn around M // 6 centres, the number of cache rows the linkage rescanned per problem, and the time of
metrics.pairwise_tm for M random-walk chains of N = 128 -- the matrix a diversity run has to compute first.  Times are device
events around the calls, after two warm-up calls, median and minimum of the repeats (pairwise_tm from M = 1024: one warm-up call,
one timed call).  pairwise_tm grows with M^2 pairs: a shape whose time, extrapolated from the previous one, exceeds
--max-tm-seconds is not run and is reported as such.
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from se3_diffusion_amd import metrics as fm  # noqa: E402

SHAPES = ((1, 64), (1, 256), (1, 1024), (1, 4096), (64, 256))     # (G, M)
N_RES = 128


def similarity(G, M, seed):
    rng = np.random.default_rng(seed)
    out = np.empty((G, M, M))
    for g in range(G):
        centres = rng.normal(size=(max(1, M // 6), 3)) * 4.0
        x = centres[rng.integers(len(centres), size=M)] + rng.normal(size=(M, 3))
        d = np.sqrt(((x[:, None] - x[None]) ** 2).sum(-1))
        out[g] = 1.0 / (1.0 + (d / 1.5) ** 2)
    return out


def chains(M, seed):
    rng = np.random.default_rng(seed)
    step = rng.normal(size=(M, N_RES, 3))
    return np.cumsum(3.8 * step / np.linalg.norm(step, axis=-1, keepdims=True), axis=1).astype(np.float32)


def timed(fn, repeats, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster_cost.txt"))
    ap.add_argument("--max-tm-seconds", type=float, default=60.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("measure_cluster_cost: no GPU; nothing here can be measured without one")
    dev = "cuda"
    lines = [f"cluster (average linkage, threshold 0.5) beside pairwise_tm (N = {N_RES}) on {torch.cuda.get_device_name(0)}",
             "times in ms: median / minimum of the repeats, device events, two warm-up calls (pairwise_tm from M = 1024: one and one)",
             f"{'G':>3} {'M':>5} {'cluster':>19} {'linkage':>19} {'rescans/problem':>16} {'merges':>7} {'pairwise_tm':>21}  cluster / tm"]
    tm_per_pair = None
    verdict = []
    for G, M in SHAPES:
        mat = torch.as_tensor(similarity(G, M, 1000 * G + M)).to(dev)
        mat = mat if G > 1 else mat[0]
        repeats = 3 if M >= 4096 else 7
        c_med, c_min = timed(lambda: fm.cluster(mat, 0.5), repeats)
        l_med, l_min = timed(lambda: fm.linkage(mat, kind="similarity"), repeats)
        ops = fm._cluster_operands(mat, None, "average", "similarity", "measure")
        _, num, ws = fm._linkage_call(*ops[:8])
        torch.cuda.synchronize()
        rescans = ws.reshape(G, M * M)[:, 0].mean().item()
        merges = num.double().mean().item()
        if G == 1:
            pairs = M * (M - 1) // 2
            if tm_per_pair is not None and tm_per_pair * pairs > args.max_tm_seconds * 1e3:
                tm_txt, ratio = f"not run (> {args.max_tm_seconds:.0f} s extrapolated)", c_med / (tm_per_pair * pairs)
                ratio_txt = f"{ratio:.2e} (against the extrapolation)"
            else:
                pos = torch.as_tensor(chains(M, M)).to(dev)
                t_med, t_min = timed(lambda: fm.pairwise_tm(pos), 1 if M >= 1024 else 3, 1 if M >= 1024 else 2)
                tm_per_pair = t_med / pairs
                tm_txt, ratio = f"{t_med:10.3f} /{t_min:10.3f}", c_med / t_med
                ratio_txt = f"{ratio:.2e}"
                del pos
            verdict.append((M, ratio))
        else:
            tm_txt, ratio_txt = "-", "-"
        lines.append(f"{G:>3} {M:>5} {c_med:9.3f} /{c_min:9.3f} {l_med:9.3f} /{l_min:9.3f} {rescans:>16.1f} {merges:>7.0f} {tm_txt:>21}  {ratio_txt}")
        print(lines[-1], flush=True)
        del mat, ws
        torch.cuda.empty_cache()
    worst = max(verdict, key=lambda v: v[1])
    lines.append("clustering costs less than the TM matrix it consumes at every measured M" if worst[1] < 1.0 else
                 f"clustering costs MORE than the TM matrix at M = {worst[0]} ({worst[1]:.2f} x)")
    lines.append(f"largest cluster / tm ratio: {worst[1]:.2e} at M = {worst[0]}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[-2:]))


if __name__ == "__main__":
    main()
