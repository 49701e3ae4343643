"""What building a training batch from the chain store costs on the device (profiles/chain_batch_cost.txt).

    python tools/measure_chain_batch_cost.py [--step-ms 21.4]

One child process per section, one after the other (a failing child ends the run).  Per batch shape (B=30 x N=128, the benchmark's
training shape, and B=8 x N=512): HIP events around each call, 3 warm-up calls, then 5 rounds of 10 repetitions alternating between
the calls, the median over all 50 and the lowest and highest of the five per-round medians (the spread of one call against itself):
  fd_chain_batch           lib.call on prepared operands: the one launch
  build_batch              the Python entry point: allocations and the upload of the ids included
  forward_marginal_batch   the existing noising on the built rigids_0 / res_mask (its draws, its launch, its casts)
  training_batch           all of it: what one batch costs
Events on one stream time the device's work when the device is the slower side and the host's enqueueing when it is not; for
launches of a few microseconds it is the latter, which is what a training loop pays too.
freeze(): 10,000 synthetic chains of 100-512 residues -- host clock around ChainStore.freeze() (it ends in the copy of the window
table to the host: pack, upload, fd_chain_windows, read-back), and fd_chain_windows alone by events.
--step-ms: the training step the share is stated against (bench.py --mode train at B=30 x N=128 on the same machine).
Nothing is replaced by these kernels, so there is no threshold: the figures are a record.

Inputs: random chains (CA walk of 3.8 A steps, N, C and O at bond length in random directions), every 17th residue absent.
"""
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = ((30, 128), (8, 512))


def walk(rng, n):
    unit = lambda v: v / np.linalg.norm(v, axis=-1, keepdims=True)
    ca = np.cumsum(3.8 * unit(rng.normal(size=(n, 3))), 0)
    nn, c = ca + 1.46 * unit(rng.normal(size=(n, 3))), ca + 1.52 * unit(rng.normal(size=(n, 3)))
    mask = np.ones((n, 4), np.uint8)
    mask[8:n - 1:17] = 0
    return np.stack([nn, ca, c, c + 1.23 * unit(rng.normal(size=(n, 3)))], 1).astype(np.float32), mask


def diffuser():
    """config/base.yaml's diffuser (the IGSO(3) tables are cached under FD_TEST_IGSO3_CACHE, as the tests keep them)"""
    from types import SimpleNamespace as ns
    from se3_diffusion_amd.data import se3_diffuser
    cache = os.environ.get("FD_TEST_IGSO3_CACHE", "/tmp/fd_test_igso3_cache")
    return se3_diffuser.SE3Diffuser(ns(diffuse_trans=True, diffuse_rot=True, r3=ns(min_b=0.1, max_b=20.0, coordinate_scaling=0.1),
                                       so3=ns(num_omega=1000, num_sigma=1000, min_sigma=0.1, max_sigma=1.5, schedule="logarithmic",
                                              cache_dir=cache, use_cached_score=False)))


def timed(calls, rounds=5, reps=10):
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


def one_shape(B, N, step_ms, dev="cuda"):
    import torch
    from se3_diffusion_amd import hip, trunk
    from se3_diffusion_amd.data.chains import ChainStore
    assert torch.cuda.is_available(), "needs an AMD GPU (no CPU fallback)"
    lib = hip.get_lib()
    diff = diffuser()
    rng = np.random.default_rng(B * 1000 + N)
    store = ChainStore(dev)
    for _ in range(64):
        a, m = walk(rng, N)
        store.add(atoms=a, atom_mask=m)
    store.freeze()
    assert (store.lengths == N).all()
    ids = rng.permutation(64)[:B]
    built = store.build_batch(ids)
    dev_ids = torch.from_numpy(ids.astype(np.int32)).to(dev)
    t = rng.uniform(0.01, 1.0, size=B)
    gen = torch.Generator(device=dev).manual_seed(0)
    calls = {
        "fd_chain_batch": lambda: lib.call("fd_chain_batch", store.atoms, store.atom_mask, store.res_index, store.offsets,
                                           store._window, dev_ids, B, N, trunk.head_const(), built["rigids_0"],
                                           built["torsion_angles_sin_cos"], built["res_mask"], built["seq_idx"], built["gt_bb"]),
        "build_batch": lambda: store.build_batch(ids),
        "forward_marginal_batch": lambda: diff.forward_marginal_batch(built["rigids_0"], t, diffuse_mask=built["res_mask"], generator=gen),
        "training_batch": lambda: store.training_batch(ids, diff, t=t, generator=gen),
    }
    res = timed(calls)
    for n, (med, lo, hi, meds) in res.items():
        print(f"{n + f'  B={B} N={N}':<42} {med:10.1f} {lo:10.1f} {hi:10.1f}   {min(meds):9.1f} - {max(meds):9.1f}")
    if (B, N) == SHAPES[0] and step_ms > 0:
        med = res["training_batch"][0]
        print(f"    training_batch is {med / (step_ms * 1e3) * 100:.2f} % of a {step_ms:.1f} ms training step at B={B} N={N}; "
              f"fd_chain_batch alone {res['fd_chain_batch'][0] / (step_ms * 1e3) * 100:.3f} %")
    batch, gt = store.training_batch(ids, diff, t=t, generator=gen)
    torch.cuda.synchronize()
    print(f"    B={B} N={N}: present {int(batch['res_mask'].sum().item())} of {B * N} rows, all finite "
          f"{all(bool(torch.isfinite(v.double()).all()) for v in batch.values()) and bool(torch.isfinite(gt).all())}", flush=True)


def freeze_section(dev="cuda", count=10000):
    import torch
    from se3_diffusion_amd import hip
    from se3_diffusion_amd.data.chains import ChainStore
    assert torch.cuda.is_available(), "needs an AMD GPU (no CPU fallback)"
    rng = np.random.default_rng(1)
    lens = rng.integers(100, 513, size=count)
    chains = [walk(rng, int(n)) for n in lens]
    torch.zeros(1, device=dev)
    torch.cuda.synchronize()
    secs = []
    for _ in range(3):
        store = ChainStore(dev)
        for a, m in chains:
            store.add(atoms=a, atom_mask=m)
        t0 = time.perf_counter()
        store.freeze()
        torch.cuda.synchronize()
        secs.append(time.perf_counter() - t0)
    T = int(lens.sum())
    print(f"freeze(): {count} chains, {T} residues ({T * 56 / 1e6:.0f} MB packed): {min(secs) * 1e3:.1f} ms (best of 3: "
          f"{', '.join(f'{s * 1e3:.1f}' for s in secs)}; the first includes the first launch of the kernel)")
    window = torch.empty_like(store._window)
    res = timed({"fd_chain_windows": lambda: hip.get_lib().call("fd_chain_windows", store.atoms, store.atom_mask, store.offsets,
                                                                len(store), window)})
    med, lo, hi, meds = res["fd_chain_windows"]
    print(f"{f'fd_chain_windows  C={count}':<42} {med:10.1f} {lo:10.1f} {hi:10.1f}   {min(meds):9.1f} - {max(meds):9.1f}")
    assert torch.equal(window, store._window)
    print(f"    lengths {store.lengths.min()} .. {store.lengths.max()}, mean {store.lengths.mean():.1f}", flush=True)


def main():
    step_ms = float(sys.argv[sys.argv.index("--step-ms") + 1]) if "--step-ms" in sys.argv else 0.0
    if "--shape" in sys.argv:
        k = sys.argv.index("--shape")
        return one_shape(int(sys.argv[k + 1]), int(sys.argv[k + 2]), step_ms)
    if "--freeze" in sys.argv:
        return freeze_section()
    print("one process per section; 5 rounds of 10 repetitions after 3 warm-up, alternating, HIP events around each call")
    print(f"{'call':<42} {'median us':>10} {'min':>10} {'max':>10}   round medians", flush=True)
    me = [sys.executable, os.path.abspath(__file__)]
    for args in [["--shape", str(B), str(N), "--step-ms", str(step_ms)] for B, N in SHAPES] + [["--freeze"]]:
        r = subprocess.run(me + args, timeout=240)
        if r.returncode != 0:
            sys.exit(f"section {' '.join(args)} failed with status {r.returncode}: nothing further is run")


if __name__ == "__main__":
    main()
