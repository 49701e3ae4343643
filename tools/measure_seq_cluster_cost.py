"""What clustering chains by sequence costs (profiles/seq_cluster_cost.txt).

    python tools/measure_seq_cluster_cost.py [--out FILE] [--chains 2000]

(a) a training set: `--chains` synthetic chains of lengths uniform in 60 .. 512 (families of ten: a random parent and mutants at
    substitution rates 0.1 .. 0.9 with 5 % indels, so that the clustering has something to find): seqs.relation -- the all-pairs
    alignment in tiles and its thresholding -- and the fd_seq_greedy launch, each after a warm-up call, host clock around a call
    that ends in a synchronise, median / min / max of the repeats; cell updates per second count the m x n cells of the pairs i < j,
    not the rows a partly filled strip computes besides.
(b) the design case: 8 sequences of 128 residues against each other (seqs.identity_matrix), device events.
(c) the restatement of tests/test_seq_cluster.py on one 128 x 128 pair on the same box: cells per second of pure Python.
(d) the VALU instructions per cell of the inner loop, counted from the compiler's assembly (hipcc -S of csrc/fd_seq.hip; per strip
    height R the loop around the exchange between lanes as a step runs it that does not change the lane's best cell, all of its
    vector instructions -- the cells and the hand-over between lanes -- over R), the issue bound that follows (256 CUs x 4 SIMDs, one wave64 vector instruction per 2 cycles at the
    2.4 GHz peak clock) and the fraction of it that (a) reached.
The projection for 20,000 chains of the same lengths is (a) times 100: the pairs grow with the square.
"""
import argparse
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from se3_diffusion_amd import build, seqs  # noqa: E402

CUS, SIMDS, CLOCK_HZ, CYCLES_PER_VALU = 256, 4, 2.4e9, 2          # MI355X: a wave64 vector instruction issues over 2 cycles


def families(C, seed):
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < C:
        parent = rng.integers(0, 20, size=int(rng.integers(60, 513)))
        out.append(parent)
        for rate in rng.uniform(0.1, 0.9, size=9):
            keep = rng.random(len(parent)) >= 0.05
            child = np.where(rng.random(len(parent)) < rate, rng.integers(0, 20, size=len(parent)), parent)[keep]
            out.append(child[:512] if len(child) >= 60 else parent)
    order = rng.permutation(C)                                     # the families do not lie side by side in a real set
    return [out[k] for k in order]


def host_timed(fn, repeats, warm=1):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms), min(ms), max(ms)


def event_timed(fn, repeats, warm=3):
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
    return statistics.median(ms), min(ms), max(ms)


def valu_per_cell():
    """{R: (vector instructions of the inner loop of align_kernel<R>, per cell)} from the compiler's assembly"""
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "fd_seq.s")
        cmd = [build.HIPCC, *build.FLAGS, "--cuda-device-only", "-S", os.path.join(build.CSRC, "fd_seq.hip"), "-o", asm]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode:
            raise SystemExit("measure_seq_cluster_cost: hipcc -S failed\n" + r.stderr[-2000:])
        text = open(asm).read()
    out = {}
    for m in re.finditer(r"^_Z\S*align_kernelILi(\d+)E\S*:.*?\n(.*?)\n\s*s_endpgm", text, re.S | re.M):
        R, lines = int(m.group(1)), m.group(2).split("\n")
        label = {mm.group(1): k for k, ln in enumerate(lines) for mm in [re.match(r"(\.LBB\d+_\d+):", ln)] if mm}
        loops = []
        for k, ln in enumerate(lines):
            mm = re.match(r"\s+s_cbranch_\w+\s+(\.LBB\d+_\d+)", ln) or re.match(r"\s+s_branch\s+(\.LBB\d+_\d+)", ln)
            if mm and mm.group(1) in label and label[mm.group(1)] < k:
                loops.append((label[mm.group(1)], k))
        # the DP loop of the strip of height R: the back edges around the exchange between lanes and R reads of the table.  The
        # innermost of them is the path of a step that does not change the lane's best cell (a step that may branches on into
        # the block behind it, which is not counted); a kernel also holds the loops of the lower strips
        inside = lambda lp, pat: sum(pat in ln for ln in lines[lp[0]:lp[1] + 1])
        dp = [lp for lp in loops if inside(lp, "ds_bpermute_b32") >= 6 and inside(lp, "ds_read_b64") >= R]
        count = lambda lp: sum(bool(re.match(r"\s+v_", ln)) for ln in lines[lp[0]:lp[1] + 1])
        best = min(dp, key=lambda lp: lp[1] - lp[0])
        out[R] = (count(best), count(best) / R)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seq_cluster_cost.txt"))
    ap.add_argument("--chains", type=int, default=2000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("measure_seq_cluster_cost: no GPU; nothing here can be measured without one")
    C = args.chains
    L = [f"tools/measure_seq_cluster_cost.py on one MI355X (gfx950; the runtime names it {torch.cuda.get_device_name(0)!r})", ""]

    def say(s=""):
        L.append(s)
        print(s, flush=True)

    # ---- (a) ----
    cs = families(C, 1)
    lens = np.array([len(c) for c in cs], dtype=np.float64)
    cells = (lens.sum() ** 2 - (lens ** 2).sum()) / 2.0
    letters, offsets = seqs.pack(cs)
    state = {}

    def run_relation():
        state["rel"] = seqs.relation(letters, offsets, None, 0.3, 0.8)

    r_med, r_min, r_max = host_timed(run_relation, 3)
    rel = state["rel"]
    g_med, g_min, g_max = host_timed(lambda: state.update(g=seqs.greedy_clusters(rel, lens)), 7, 2)
    counts = state["g"][2]
    say(f"(a) {C} chains, lengths {int(lens.min())} .. {int(lens.max())} (mean {lens.mean():.0f}), {C * (C - 1) // 2} pairs, {cells:.3e} cells; "
        f"BLOSUM62 as typed, gaps (11, 1), thresholds (0.3, 0.8)")
    say("    1 warm-up + 3 repetitions (relation), 2 + 7 (greedy); host clock around a call that ends in a synchronise; ms: median, min, max")
    say(f"    seqs.relation (all-pairs alignment in tiles of 2048 + thresholding)  {r_med:10.1f} {r_min:10.1f} {r_max:10.1f}")
    say(f"    cell updates per second                                             {cells / (r_med * 1e-3):.3e}")
    say(f"    seqs.greedy_clusters (fd_seq_greedy, one block, and its read-back)   {g_med:10.3f} {g_min:10.3f} {g_max:10.3f}")
    say(f"    {counts['clusters']} clusters, the largest of {counts['largest']}; {int(rel.sum().item()) // 2} related pairs")
    proj = r_med * 1e-3 * (20000.0 / C) ** 2
    say(f"    projected for 20,000 such chains ({(20000.0 / C) ** 2:.0f} x the pairs): {proj:.0f} s = {proj / 60:.1f} min of alignment"
        f"{' -- MORE THAN TEN MINUTES' if proj > 600 else ''}; its relation matrix holds 400 MB")
    say()
    # ---- (b) ----
    rng = np.random.default_rng(2)
    native = rng.integers(0, 20, size=128)
    designs = [np.where(rng.random(128) < 0.5, rng.integers(0, 20, size=128), native) for _ in range(8)]
    packed = seqs.pack(designs)
    d_med, d_min, d_max = event_timed(lambda: seqs.identity_matrix(packed), 15)
    say("(b) the design case: 8 sequences of 128 residues against each other, 64 pairs, 1.05e+06 cells")
    say("    3 warm-up + 15 repetitions, device events; us: median, min, max")
    say(f"    seqs.identity_matrix (checks, fd_seq_align, the quotient)            {d_med * 1e3:10.1f} {d_min * 1e3:10.1f} {d_max * 1e3:10.1f}")
    say(f"    cell updates per second                                             {64 * 128 * 128 / (d_med * 1e-3):.3e}")
    say("    at this size the call is its host side: the validation read-backs and a launch, not the arithmetic")
    say()
    # ---- (c) ----
    from test_seq_cluster import ref_align
    t0 = time.perf_counter()
    ref_align(designs[0].tolist(), designs[1].tolist(), seqs.BLOSUM62, 11, 1)
    dt = time.perf_counter() - t0
    say(f"(c) the pure-Python restatement on one 128 x 128 pair on this box: {dt:.3f} s, {128 * 128 / dt:.3e} cells per second")
    say()
    # ---- (d) ----
    say("(d) vector instructions of the inner loop, from the compiler's assembly (per step of R cells, and per cell)")
    table = valu_per_cell()
    for R in sorted(table):
        say(f"    R = {R:2d} (the tallest strip of the kernel for chains up to {64 * R:4d} rows)   {table[R][0]:5d} per step   {table[R][1]:6.1f} per cell")
    mean_need = np.mean([np.ceil(m / 64) for m in lens])
    per_cell = table[8][1] if 8 in table else max(v[1] for v in table.values())
    bound = CUS * SIMDS * CLOCK_HZ / CYCLES_PER_VALU * 64 / per_cell
    say(f"    issue bound at {per_cell:.1f} per cell: {CUS} CUs x {SIMDS} SIMDs x {CLOCK_HZ / 1e9:.1f} GHz / {CYCLES_PER_VALU} cycles x 64 lanes "
        f"= {bound:.3e} cells per second")
    say(f"    (a) reached {cells / (r_med * 1e-3) / bound:.1%} of it.  What the bound does not count: lanes without a row (a chain of m rows "
        f"fills m of the 64 R rows of its strips; mean R here {mean_need:.1f}), the skew's n + 63 steps for n columns, the six LDS-crossbar "
        f"exchanges per step, the clock under load, and the thresholding between the tiles")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(L) + "\n")


if __name__ == "__main__":
    main()
