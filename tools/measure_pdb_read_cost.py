"""What reading PDB files costs (se3_diffusion_amd/pdb.py parse_pdb on csrc/fd_pdb_read.hip), next to the only host reader that
exists where this project is built: the pure-Python line reader of tests/test_pdb_read.py.  No comparison with Biopython is made.

    python tools/measure_pdb_read_cost.py            # on the MI355X; writes profiles/pdb_read_cost.txt

The texts come from format_pdb (backbone atoms only, as the sampler leaves them):
  (a) refolds     the eight single-model N = 128 files of one sample's self-consistency step, in one call
  (b) trajectory  one file of 500 models of N = 128 (a bb_traj file), model="all"
  (c) library     2,000 single-model N = 256 files (100 distinct ones, each twenty times) in one call, then ca_padded()
Per input:
  upload                         torch.from_numpy(bytes).cuda() of the joined text (pageable memory), wall clock
  fd_pdb_read_summary / _count / _fill   the library calls alone on prepared operands, HIP events around each call
  scans between                  the cumsum / cummax calls that turn per-chunk values into what each chunk needs, HIP events
  read-back                      the .cpu() of the four words (rows, segments, lines, status), wall clock, device idle before it
  parse_pdb, text on the device  the whole call on a uint8 device tensor per file, wall clock
  parse_pdb, bytes on the host   the whole call on bytes objects: joining, the upload and the above, wall clock
  ca_padded                      (c) only: the padded CA arrays for metrics.novelty, wall clock
  line reader                    tests/test_pdb_read.py reference_read on the same bytes, this machine's CPU, ONE run; for (c) on the
                                 100 distinct files only, and that time multiplied by twenty is given as an estimate
Each device figure: median of REPS repetitions after WARM warm-up calls, with the lowest and highest.
"""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

WARM, REPS = 3, 15
OUT = os.path.join(ROOT, "profiles", "pdb_read_cost.txt")


def backbone(rng, *shape):
    x = np.zeros(shape + (37, 3), np.float32)
    x[..., :5, :] = rng.normal(size=shape + (5, 3)) * 15.0
    return x


def stats(xs):
    return f"{statistics.median(xs):12.1f} {min(xs):11.1f} {max(xs):11.1f}"


def main(out):
    import torch
    from se3_diffusion_amd import hip, pdb
    import test_pdb_read as tr
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    lib = hip.get_lib()
    rng = np.random.default_rng(0)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

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

    text_of = lambda x: pdb.format_pdb(torch.from_numpy(x).cuda())
    distinct = [text_of(backbone(rng, 256)) for _ in range(100)]
    inputs = {
        "(a) refolds: 8 files, N = 128": ([text_of(backbone(rng, 128)) for _ in range(8)], "first", 1),
        "(b) trajectory: 1 file, 500 models, N = 128": ([text_of(backbone(rng, 500, 128))], "all", 1),
        "(c) library: 2,000 files, N = 256": (distinct * 20, "first", 20),
    }
    say(f"{WARM} warm-up + {REPS} repetitions; times in us: median, min, max")
    for title, (dev_files, model, repeat) in inputs.items():
        host_files = [t.cpu().numpy().tobytes() for t in dev_files[:len(dev_files) // repeat]] * repeat
        F = len(host_files)
        joined = np.frombuffer(b"".join(host_files), np.uint8)
        n = joined.size
        text = torch.from_numpy(joined).cuda()
        off = torch.from_numpy(np.concatenate([[0], np.cumsum([len(b) for b in host_files])]).astype(np.int64)).cuda()
        nchunks = -(-n // pdb.READ_CHUNK)
        every = int(model == "all")
        i64 = dict(dtype=torch.int64, device="cuda")
        summary, carry, counts = torch.empty((4, nchunks), **i64), torch.empty((4, nchunks), **i64), torch.empty((3, nchunks), **i64)
        file_first = torch.zeros((2, F), **i64)

        def scans():
            carry[:2] = torch.cumsum(summary[:2], 1) - summary[:2]
            carry[2:, 0] = -1
            carry[2:, 1:] = torch.cummax(summary[2:], 1).values[:, :-1]

        def totals():
            ends = torch.cumsum(counts[:2], 1)
            return ends, torch.stack([ends[0, -1], ends[1, -1], summary[0].sum(), counts[2].min()])

        rows = {}
        rows["upload"] = wall(lambda: torch.from_numpy(joined).cuda())
        rows["fd_pdb_read_summary"] = events(lambda: lib.call("fd_pdb_read_summary", text, n, off, F, 0, summary))
        rows["scans between (carry)"] = events(scans)
        rows["fd_pdb_read_count"] = events(lambda: lib.call("fd_pdb_read_count", text, n, off, F, 0, every, carry, counts, file_first))
        rows["scans between (bases)"] = events(totals)
        ends, words = totals()
        rows["read-back"] = wall(lambda: words.cpu())
        T, C, n_lines, word = (int(v) for v in words.cpu())
        assert word == pdb.STATUS_OK
        bases = (ends - counts[:2]).contiguous()
        parsed = pdb.parse_pdb(dev_files, model=model)
        assert (parsed.num_residues, len(parsed)) == (T, C)
        dropped = torch.empty(T, dtype=torch.int32, device="cuda")
        rows["fd_pdb_read_fill"] = events(lambda: lib.call(
            "fd_pdb_read_fill", text, n, off, F, 0, every, carry, bases, file_first, T, C, parsed.atom_positions, parsed.atom_mask,
            parsed.b_factors, parsed.aatype, parsed.residue_index, dropped, parsed.chain_offsets, parsed.chain_file,
            parsed.chain_model, parsed.chain_id))
        rows["parse_pdb, text on the device"] = wall(lambda: pdb.parse_pdb(dev_files, model=model))
        rows["parse_pdb, bytes on the host"] = wall(lambda: pdb.parse_pdb(host_files, model=model))
        if repeat > 1:
            rows["ca_padded"] = wall(lambda: pdb.parse_pdb(dev_files, model=model).ca_padded())
            rows["ca_padded"] = [a - statistics.median(rows["parse_pdb, text on the device"]) for a in rows["ca_padded"]]
        t0 = time.perf_counter()
        want = tr.reference_read(host_files[:F // repeat], model=model)
        reader_s = time.perf_counter() - t0
        assert np.array_equal(parsed.atom_positions[:len(want["aatype"])].cpu().numpy(), want["atom_positions"])
        say()
        say(f"{title}: {n} bytes, {n_lines} lines, {T} residue rows in {C} chain segments")
        say(f"  {'':32s} {'median us':>12s} {'min':>11s} {'max':>11s}")
        for k, v in rows.items():
            say(f"  {k:32s} {stats(v)}")
        if repeat > 1:
            say(f"  (ca_padded: the call behind parse_pdb, less the median of parse_pdb)")
            say(f"  line reader on the {F // repeat} distinct files, one run: {reader_s:.2f} s; times {repeat} for all {F}: about {reader_s * repeat:.0f} s")
        else:
            say(f"  line reader, one run: {reader_s:.2f} s")
    with open(out, "w") as f:
        f.write("tools/measure_pdb_read_cost.py on one MI355X (gfx950)\n" + "\n".join(lines) + "\n")
    print(f"wrote {out}")


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT, help="where the table is written")
    main(ap.parse_args().out)
