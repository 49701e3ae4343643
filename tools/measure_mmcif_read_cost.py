"""What reading mmCIF files costs (se3_diffusion_amd/pdb.py parse_mmcif on csrc/fd_cif_read.hip), next to the same structures as PDB
text through parse_pdb, and next to the only host mmCIF reader that exists where this project is built: the pure-Python reader of
tests/test_mmcif_read.py.  No comparison with Biopython or gemmi is made.

    python tools/measure_mmcif_read_cost.py            # on the MI355X; writes profiles/mmcif_read_cost.txt

The structures come from format_pdb (backbone atoms only, as the sampler leaves them); tests/test_mmcif_read.py's pdb_to_cif turns
each PDB text into an atom_site loop of the wwPDB's 21 columns:
  (a) refolds     eight single-model N = 128 files in one call
  (b) trajectory  one file of 500 models of N = 128, model="all"
  (c) library     2,000 single-model N = 256 files (100 distinct ones, each twenty times) in one call
Per input:
  upload                         torch.from_numpy(bytes).cuda() of the joined mmCIF text (pageable memory), wall clock
  fd_cif_read_*                  the six library calls alone on prepared operands, HIP events around each call
  scans between                  the cumsum / cummax calls that turn per-chunk values into what each chunk needs, HIP events
  read-back                      the .cpu() of the four words (rows, segments, lines, status), wall clock, device idle before it
  parse_mmcif, text on the device / bytes on the host      the whole call, wall clock
  parse_pdb, text on the device / bytes on the host        the whole call on the PDB text of the same structures, wall clock
  bytes/s                        the text's size over the median of the whole call with the text on the device, both formats
  pure-Python reader             reference_read_cif on the same bytes, this machine's CPU, ONE run; for (c) on the 100 distinct files
                                 only, and that time multiplied by twenty is given as an estimate
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
OUT = os.path.join(ROOT, "profiles", "mmcif_read_cost.txt")
WHY = ("  mmCIF is read at less than half of PDB's bytes/s: a PDB record is sliced at fixed columns out of five 16-byte loads, while an\n"
       "  atom_site row has to be tokenised byte by byte by the one thread that owns it, and because what a line is depends on the text\n"
       "  in front of it (text fields, the loop's header, the column table) the text is walked by six launches where PDB needs three,\n"
       "  the later ones repeating the earlier stages inside the block.")


def backbone(rng, *shape):
    x = np.zeros(shape + (37, 3), np.float32)
    x[..., :5, :] = rng.normal(size=shape + (5, 3)) * 15.0
    return x


def stats(xs):
    return f"{statistics.median(xs):12.1f} {min(xs):11.1f} {max(xs):11.1f}"


def main(out):
    import torch
    from se3_diffusion_amd import hip, pdb
    import test_mmcif_read as tm
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

    text_of = lambda x: pdb.format_pdb(torch.from_numpy(x).cuda()).cpu().numpy().tobytes()
    inputs = {
        "(a) refolds: 8 files, N = 128": ([text_of(backbone(rng, 128)) for _ in range(8)], "first", 1),
        "(b) trajectory: 1 file, 500 models, N = 128": ([text_of(backbone(rng, 500, 128))], "all", 1),
        "(c) library: 2,000 files, N = 256": ([text_of(backbone(rng, 256)) for _ in range(100)], "first", 20),
    }
    say(f"{WARM} warm-up + {REPS} repetitions; times in us: median, min, max")
    for title, (distinct_pdb, model, repeat) in inputs.items():
        distinct_cif = [tm.pdb_to_cif(b) for b in distinct_pdb]
        pdb_host, cif_host = distinct_pdb * repeat, distinct_cif * repeat
        pdb_dev = [torch.from_numpy(np.frombuffer(b, np.uint8).copy()).cuda() for b in distinct_pdb] * repeat
        cif_dev = [torch.from_numpy(np.frombuffer(b, np.uint8).copy()).cuda() for b in distinct_cif] * repeat
        F = len(cif_host)
        joined = np.frombuffer(b"".join(cif_host), np.uint8)
        n, n_pdb = joined.size, sum(len(b) for b in pdb_host)
        text = torch.from_numpy(joined).cuda()
        off = torch.from_numpy(np.concatenate([[0], np.cumsum([len(b) for b in cif_host])]).astype(np.int64)).cuda()
        nchunks = -(-n // pdb.READ_CHUNK)
        every = int(model == "all")
        i64 = dict(dtype=torch.int64, device="cuda")
        before = lambda v: torch.cat([torch.full_like(v[:, :1], -1), torch.cummax(v, 1).values[:, :-1]], 1)
        carry = torch.full((8, nchunks), -1, **i64)
        per_line, marks, last = torch.empty((3, nchunks), **i64), torch.empty((4, nchunks), **i64), torch.empty((1, nchunks), **i64)
        table, first, head_bad = torch.zeros((F, pdb.CIF_TABLE), dtype=torch.int32, device="cuda"), torch.zeros(F, **i64), torch.empty(nchunks, **i64)
        counts = torch.empty((3, nchunks), **i64)

        def scan_lines():
            carry[:2] = torch.cumsum(per_line[:2], 1) - per_line[:2]
            carry[2:3] = before(torch.where(per_line[2:3] >= 0, carry[1:2] + per_line[2:3], per_line[2:3]))

        def scan_marks():
            carry[3:7] = before(marks)

        def scan_last():
            carry[7:8] = before(last)

        def totals():
            ends = torch.cumsum(counts[:2], 1)
            return ends, torch.stack([ends[0, -1], ends[1, -1], per_line[0].sum(), torch.minimum(counts[2].min(), head_bad.min())])

        rows = {}
        rows["upload"] = wall(lambda: torch.from_numpy(joined).cuda())
        rows["fd_cif_read_lines"] = events(lambda: lib.call("fd_cif_read_lines", text, n, off, F, per_line))
        rows["scans between (lines)"] = events(scan_lines)
        rows["fd_cif_read_marks"] = events(lambda: lib.call("fd_cif_read_marks", text, n, off, F, carry, marks))
        rows["scans between (marks)"] = events(scan_marks)
        rows["fd_cif_read_header"] = events(lambda: lib.call("fd_cif_read_header", text, n, off, F, 0, 0, carry, table, first, head_bad))
        rows["fd_cif_read_summary"] = events(lambda: lib.call("fd_cif_read_summary", text, n, off, F, 0, carry, table, last))
        rows["scans between (records)"] = events(scan_last)
        rows["fd_cif_read_count"] = events(lambda: lib.call("fd_cif_read_count", text, n, off, F, 0, every, carry, table, counts))
        rows["scans between (bases)"] = events(totals)
        ends, words = totals()
        rows["read-back"] = wall(lambda: words.cpu())
        T, C, n_lines, word = (int(v) for v in words.cpu())
        assert word == pdb.STATUS_OK
        bases = (ends - counts[:2]).contiguous()
        parsed = pdb.parse_mmcif(cif_dev, model=model)
        from_pdb = pdb.parse_pdb(pdb_dev, model=model)
        assert (parsed.num_residues, len(parsed)) == (T, C)
        tm.assert_same(parsed, from_pdb)                                            # the two formats read as the same arrays
        dropped = torch.empty(T, dtype=torch.int32, device="cuda")
        rows["fd_cif_read_fill"] = events(lambda: lib.call(
            "fd_cif_read_fill", text, n, off, F, 0, every, carry, table, bases, T, C, parsed.atom_positions, parsed.atom_mask,
            parsed.b_factors, parsed.aatype, parsed.residue_index, dropped, parsed.chain_offsets, parsed.chain_file,
            parsed.chain_model, parsed.chain_id))
        rows["parse_mmcif, text on the device"] = wall(lambda: pdb.parse_mmcif(cif_dev, model=model))
        rows["parse_mmcif, bytes on the host"] = wall(lambda: pdb.parse_mmcif(cif_host, model=model))
        rows["parse_pdb, text on the device"] = wall(lambda: pdb.parse_pdb(pdb_dev, model=model))
        rows["parse_pdb, bytes on the host"] = wall(lambda: pdb.parse_pdb(pdb_host, model=model))
        t0 = time.perf_counter()
        want = tm.reference_read_cif(distinct_cif, model=model)
        reader_s = time.perf_counter() - t0
        assert np.array_equal(parsed.atom_positions[:len(want["aatype"])].cpu().numpy(), want["atom_positions"])
        rate_cif = n / statistics.median(rows["parse_mmcif, text on the device"]) * 1e6
        rate_pdb = n_pdb / statistics.median(rows["parse_pdb, text on the device"]) * 1e6
        say()
        say(f"{title}: {n} bytes of mmCIF ({n_pdb} bytes as PDB, x{n / n_pdb:.2f}), {n_lines} lines, {T} residue rows in {C} chain segments")
        say(f"  {'':34s} {'median us':>12s} {'min':>11s} {'max':>11s}")
        for k, v in rows.items():
            say(f"  {k:34s} {stats(v)}")
        say(f"  bytes/s, text on the device: mmCIF {rate_cif / 1e9:.3f} GB/s, PDB {rate_pdb / 1e9:.3f} GB/s (mmCIF / PDB = {rate_cif / rate_pdb:.2f})")
        if rate_cif < 0.5 * rate_pdb:
            say(WHY)
        if repeat > 1:
            say(f"  pure-Python reader on the {F // repeat} distinct files, one run: {reader_s:.2f} s; times {repeat} for all {F}: about {reader_s * repeat:.0f} s")
        else:
            say(f"  pure-Python reader, one run: {reader_s:.2f} s")
    with open(out, "w") as f:
        f.write("tools/measure_mmcif_read_cost.py on one MI355X (gfx950)\n" + "\n".join(lines) + "\n")
    print(f"wrote {out}")


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT, help="where the table is written")
    main(ap.parse_args().out)
