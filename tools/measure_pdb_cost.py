"""What writing a sample's PDB files costs (se3_diffusion_amd/pdb.py on csrc/fd_pdb.hip), next to the sampling it follows.

    python tools/measure_pdb_cost.py                 # on the MI355X: T = 500, N = 128 and 512
    python tools/measure_pdb_cost.py --reference     # where the reference checkout is: its host writer on this CPU

Device run.  A synthetic record (prot_traj and rigid_0_traj [T,B=2,N,37,3], backbone atoms only, as sampler.sample(record=
"reference") leaves them) for backbone b = 1, so every call reads the strided view.  Per shape:
  fd_pdb_count, fd_pdb_format   the library calls alone on prepared operands, HIP events around each call
  to host                       text.cpu() of the formatted trajectory (pageable memory, as write_pdb does it)
  file write                    open / write / close of those bytes in a temporary directory
  format_pdb                    the two launches, the cumsum, the read-back of size and status, the allocation
  save_traj                     the three files of a sample (final frame, bb_traj, x0_traj) as a whole, wall clock
Each figure: median of REPS repetitions after WARM warm-up calls, with the lowest and highest.  Sampling times are the README's
(500 steps, B=1: N=128 1.87-1.94 backbones/s = 0.53 s; N=512 0.57 backbones/s = 1.75 s).

Reference run.  analysis.utils.write_prot_to_pdb of the unmodified reference (oracle/ref_loader.py) on the same kind of input:
one [500,128,37,3] trajectory and one [128,37,3] frame, single runs, wall clock.
"""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T = 500
SAMPLE_S = {128: 0.53, 512: 1.75}
WARM, REPS = 3, 15


def record(rng, n_frames, B, N):
    x = np.zeros((n_frames, B, N, 37, 3), np.float32)
    x[..., :5, :] = rng.normal(size=(n_frames, B, N, 5, 3)) * 15.0
    return x


def reference():
    from oracle import ref_loader as rl
    rl.install()
    from analysis import utils as au
    rng = np.random.default_rng(0)
    traj = record(rng, T, 1, 128)[:, 0]
    b = np.tile(np.full(128, 100.0)[:, None], (1, 37))
    print("reference writer (analysis.utils.write_prot_to_pdb, unmodified), this machine's CPU, single runs, wall clock")
    with tempfile.TemporaryDirectory() as tmp:
        for name, arr in (("one [128,37,3] frame", traj[0]), (f"one [{T},128,37,3] trajectory", traj)):
            t0 = time.perf_counter()
            path = au.write_prot_to_pdb(arr, os.path.join(tmp, "ref"), b_factors=b, overwrite=True)
            dt = time.perf_counter() - t0
            print(f"  {name:34s} {dt * 1e3:10.1f} ms   {os.path.getsize(path)} bytes")


def stats(xs):
    return f"{statistics.median(xs):12.1f} {min(xs):11.1f} {max(xs):11.1f}"


def device():
    import torch
    from se3_diffusion_amd import hip, pdb
    assert torch.cuda.is_available(), "the device run needs the GPU"
    lib = hip.get_lib()
    rng = np.random.default_rng(0)
    print(f"T = {T}, backbone b = 1 of B = 2, {WARM} warm-up + {REPS} repetitions; times in us: median, min, max")
    for N in (128, 512):
        out = {k: torch.from_numpy(record(rng, T, 2, N)).cuda() for k in ("prot_traj", "rigid_0_traj")}
        view = out["prot_traj"][:, 1]
        bf = torch.full((N, 37), 100.0, device="cuda")
        counts = torch.empty(T, dtype=torch.int64, device="cuda")
        status = torch.empty(T, dtype=torch.int64, device="cuda")
        text = pdb.format_pdb(view, b_factors=bf)
        offsets = torch.cumsum(torch.full((T,), 5 * N + 3, dtype=torch.int64, device="cuda"), 0) - (5 * N + 3)
        buf = torch.empty_like(text)

        def events(fn):
            ts = []
            for i in range(WARM + REPS):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                if i >= WARM:
                    ts.append(e0.elapsed_time(e1) * 1e3)
            return ts

        def wall(fn):
            ts = []
            for i in range(WARM + REPS):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if i >= WARM:
                    ts.append((time.perf_counter() - t0) * 1e6)
            return ts

        rows = {}
        rows["fd_pdb_count"] = events(lambda: lib.call("fd_pdb_count", view, view.stride(0), None, bf, T, N, counts, status))
        rows["fd_pdb_format"] = events(lambda: lib.call("fd_pdb_format", view, view.stride(0), None, bf, offsets, T, N, 1, buf,
                                                        buf.numel()))
        assert torch.equal(buf, text)
        rows["format_pdb"] = wall(lambda: pdb.format_pdb(view, b_factors=bf))
        rows["to host"] = wall(lambda: text.cpu())
        host = text.cpu().numpy()
        with tempfile.TemporaryDirectory() as tmp:
            def write():
                with open(os.path.join(tmp, "w.pdb"), "wb") as f:
                    f.write(memoryview(host))
            rows["file write"] = wall(write)
        ts = []
        for i in range(WARM + REPS):
            with tempfile.TemporaryDirectory() as tmp:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                paths = pdb.save_traj(out, 1, tmp)
                ts.append((time.perf_counter() - t0) * 1e6)
                sizes = [os.path.getsize(paths[k]) for k in ("sample_path", "traj_path", "x0_traj_path")]
        rows["save_traj (3 files)"] = ts[WARM:]
        print(f"N = {N}: trajectory text {text.numel()} bytes; the three files {sizes} bytes; sampling takes {SAMPLE_S[N]:.2f} s")
        print(f"  {'':22s} {'median us':>12s} {'min':>11s} {'max':>11s}   share of the sampling time")
        for k, v in rows.items():
            print(f"  {k:22s} {stats(v)}   {statistics.median(v) / (SAMPLE_S[N] * 1e6) * 100:8.4f} %")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", action="store_true", help="time the reference's host writer (needs the reference checkout)")
    if ap.parse_args().reference:
        reference()
    else:
        device()
