"""What inflating gzip-compressed structure files on the device costs (se3_diffusion_amd/pdb.py inflate on csrc/fd_inflate.hip, one
wave per file), next to zlib on the host of the same machine and next to the plain-text path of the same commit.

    python tools/measure_inflate_cost.py            # on the MI355X; writes profiles/inflate_cost.txt

The structures are those of tools/measure_mmcif_read_cost.py (format_pdb of backbone atoms; pdb_to_cif for the mmCIF form), each
file gzipped at level 6:
  (a) refolds     eight single-model N = 128 files in one call
  (b) trajectory  one file of 500 models of N = 128
  (c) library     2,000 single-model N = 256 files (100 distinct ones, each twenty times) in one call
Per input and format:
  upload, gzip / plain           torch.from_numpy(bytes).cuda() of the joined files (pageable memory), wall clock
  fd_inflate, verify on / off    the one library call on prepared operands, HIP events around it
  parse_*, gzip / plain bytes    the whole call from bytes on the host, wall clock
  zlib, 1 thread / 16 threads    zlib.decompress(file, 31) over the same files on the host, in a loop and in a pool of 16 threads
                                 (zlib releases the GIL), wall clock
Each figure: median of REPS repetitions after WARM warm-up calls, with the lowest and highest.  Then, over the first F files of
(c) as mmCIF, the device's way to text on the device (upload of the gzip bytes + fd_inflate with verify) against the host's (the
16-thread pool + upload of the plain text), 2 warm-up calls and 5 repetitions each.
"""
import os
import statistics
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

WARM, REPS = 3, 15
THREADS = 16
OUT = os.path.join(ROOT, "profiles", "inflate_cost.txt")


def backbone(rng, *shape):
    x = np.zeros(shape + (37, 3), np.float32)
    x[..., :5, :] = rng.normal(size=shape + (5, 3)) * 15.0
    return x


def stats(xs):
    return f"{statistics.median(xs):12.1f} {min(xs):11.1f} {max(xs):11.1f}"


def gz(data):
    c = zlib.compressobj(6, zlib.DEFLATED, 31, 9)
    return c.compress(data) + c.flush()


def main(out):
    import torch
    from se3_diffusion_amd import hip, pdb
    import test_mmcif_read as tm
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    lib = hip.get_lib()
    rng = np.random.default_rng(0)
    lines = []
    pool = ThreadPoolExecutor(THREADS)

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def events(fn, warm=WARM, reps=REPS):
        ts = []
        for i in range(warm + reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if i >= warm:
                ts.append(e0.elapsed_time(e1) * 1e3)
        return ts

    def wall(fn, warm=WARM, reps=REPS):
        ts = []
        for i in range(warm + reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if i >= warm:
                ts.append((time.perf_counter() - t0) * 1e6)
        return ts

    def operands(zipped, sizes):
        """what pdb.inflate hands to fd_inflate for these gzip files"""
        F = len(zipped)
        joined = np.frombuffer(b"".join(zipped), np.uint8)
        in_off = np.concatenate([[0], np.cumsum([len(z) for z in zipped])]).astype(np.int64)
        out_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        return (joined, torch.from_numpy(in_off).cuda(), torch.from_numpy(out_off).cuda(), torch.ones(F, dtype=torch.int32, device="cuda"),
                torch.empty(int(out_off[-1]), dtype=torch.uint8, device="cuda"), torch.empty(F, dtype=torch.int64, device="cuda"))

    def launch(data, ops, verify):
        _, in_off, out_off, kind, text, status = ops
        lib.call("fd_inflate", data, int(data.numel()), in_off, len(kind), kind, text, int(text.numel()), out_off, verify, status)

    text_of = lambda x: pdb.format_pdb(torch.from_numpy(x).cuda()).cpu().numpy().tobytes()
    inputs = {
        "(a) refolds: 8 files, N = 128": ([text_of(backbone(rng, 128)) for _ in range(8)], "first", 1),
        "(b) trajectory: 1 file, 500 models, N = 128": ([text_of(backbone(rng, 500, 128))], "all", 1),
        "(c) library: 2,000 files, N = 256": ([text_of(backbone(rng, 256)) for _ in range(100)], "first", 20),
    }
    say(f"{WARM} warm-up + {REPS} repetitions; times in us: median, min, max; gzip level 6")
    wave_rates, library = [], None
    for title, (distinct_pdb, model, repeat) in inputs.items():
        for fmt, distinct, parse in (("mmCIF", [tm.pdb_to_cif(b) for b in distinct_pdb], pdb.parse_mmcif), ("PDB", distinct_pdb, pdb.parse_pdb)):
            plain = distinct * repeat
            zipped = [gz(b) for b in distinct] * repeat
            F, n_plain, n_gzip = len(plain), sum(len(b) for b in plain), sum(len(z) for z in zipped)
            ops = operands(zipped, [len(b) for b in plain])
            data = torch.from_numpy(ops[0]).cuda()
            joined_plain = np.frombuffer(b"".join(plain), np.uint8)
            launch(data, ops, 1)
            assert not ops[5].any().item() and ops[4].cpu().numpy().tobytes() == joined_plain.tobytes()      # the device's text is zlib's
            rows = {}
            rows["upload, gzip bytes"] = wall(lambda: torch.from_numpy(ops[0]).cuda())
            rows["upload, plain bytes"] = wall(lambda: torch.from_numpy(joined_plain).cuda())
            rows["fd_inflate, verify on"] = events(lambda: launch(data, ops, 1))
            rows["fd_inflate, verify off"] = events(lambda: launch(data, ops, 0))
            rows[f"{parse.__name__}, gzip bytes"] = wall(lambda: parse(zipped, model=model))
            rows[f"{parse.__name__}, plain bytes"] = wall(lambda: parse(plain, model=model))
            rows["zlib on the host, 1 thread"] = wall(lambda: [zlib.decompress(z, 31) for z in zipped])
            rows[f"zlib on the host, {THREADS} threads"] = wall(lambda: list(pool.map(lambda z: zlib.decompress(z, 31), zipped)))
            say()
            say(f"{title}, {fmt}: {F} files, {n_gzip} bytes gzipped, {n_plain} bytes inflated (x{n_plain / n_gzip:.2f})")
            say(f"  {'':34s} {'median us':>12s} {'min':>11s} {'max':>11s}")
            for k, v in rows.items():
                say(f"  {k:34s} {stats(v)}")
            on = statistics.median(rows["fd_inflate, verify on"])
            say(f"  fd_inflate with verify: {n_plain / on:.1f} MB/s of text over all {F} waves, {n_plain / on / F:.2f} MB/s per file")
            if F == 1:
                off = statistics.median(rows["fd_inflate, verify off"])
                wave_rates.append(f"{fmt} {n_plain / on:.1f} MB/s of text with verify, {n_plain / off:.1f} MB/s without ({n_gzip / on:.1f} and "
                                  f"{n_gzip / off:.1f} MB/s of gzip bytes)")
            if fmt == "mmCIF" and repeat > 1:
                library = (plain, zipped)
    say()
    say("one wave's rate (the single file of (b), nothing else on the device): " + "; ".join(wave_rates))

    plain, zipped = library
    say()
    say(f"the first F files of (c) as mmCIF, to text on the device; median us of 5 after 2 warm-up calls")
    say(f"  {'F':>6s} {'upload gzip + fd_inflate':>26s} {'zlib x' + str(THREADS) + ' + upload plain':>26s} {'zlib x1 + upload plain':>26s}")
    ahead = None
    for F in (1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1000, 2000):
        zs, ps = zipped[:F], plain[:F]
        ops = operands(zs, [len(b) for b in ps])

        def device():
            launch(torch.from_numpy(ops[0]).cuda(), ops, 1)

        def host(threads):
            got = list(pool.map(lambda z: zlib.decompress(z, 31), zs)) if threads > 1 else [zlib.decompress(z, 31) for z in zs]
            torch.from_numpy(np.frombuffer(b"".join(got), np.uint8)).cuda()

        d = statistics.median(wall(device, 2, 5))
        h16 = statistics.median(wall(lambda: host(THREADS), 2, 5))
        h1 = statistics.median(wall(lambda: host(1), 2, 5))
        say(f"  {F:6d} {d:26.1f} {h16:26.1f} {h1:26.1f}")
        if d < h16 and ahead is None:
            ahead = F
        if d >= h16:
            ahead = None
    say(f"  the device path is ahead of the {THREADS}-thread pool from F = {ahead} on" if ahead else
        f"  the device path is not ahead of the {THREADS}-thread pool at the largest F measured")
    with open(out, "w") as f:
        f.write("tools/measure_inflate_cost.py on one MI355X (gfx950)\n" + "\n".join(lines) + "\n")
    print(f"wrote {out}")


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT, help="where the table is written")
    main(ap.parse_args().out)
