"""The input of tools/fuzz_inflate.cpp: three gzip members of a few KB (one stored, one fixed, one dynamic), each with 2,000 seeded
single-byte mutations and what zlib makes of every one of them.

    python tools/make_fuzz_inflate.py fuzz_inflate.bin

Layout, int32 little-endian: the number of streams; per stream its bytes (length first), its text (length first), the number of
mutations; per mutation the position, the new byte and 0 (zlib.decompress(mutant, 31) raises), 1 (it gives the stream's text) or 2
(it gives other bytes, which follow, length first)."""
import struct
import sys
import zlib

import numpy as np

MUTATIONS = 2000


def main(path):
    rng = np.random.default_rng(0)
    record = "ATOM  %5d  CA  %s A%4d    %8.3f%8.3f%8.3f  1.00%6.2f           C  \n"
    names = "ALA ARG ASN ASP CYS GLN GLU GLY HIS ILE".split()
    text = "".join(record % (k, names[k % 10], k // 4, *rng.normal(0, 20, 3), rng.uniform(0, 99)) for k in range(60)).encode()
    w32 = lambda v: struct.pack("<i", v)
    blob = w32(3)
    for level, strategy in ((0, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_FIXED), (9, zlib.Z_DEFAULT_STRATEGY)):
        c = zlib.compressobj(level, zlib.DEFLATED, 31, 9, strategy)
        stream = c.compress(text) + c.flush()
        blob += w32(len(stream)) + stream + w32(len(text)) + text + w32(MUTATIONS)
        counts = [0, 0, 0]
        for _ in range(MUTATIONS):
            pos = int(rng.integers(len(stream)))
            value = int((stream[pos] + rng.integers(1, 256)) % 256)
            mutant = stream[:pos] + bytes([value]) + stream[pos + 1:]
            try:
                got = zlib.decompress(mutant, 31)
                expect = 1 if got == text else 2
            except zlib.error:
                got, expect = b"", 0
            counts[expect] += 1
            blob += w32(pos) + w32(value) + w32(expect) + (w32(len(got)) + got if expect == 2 else b"")
        print(f"level {level} strategy {strategy}: {len(stream)} bytes; zlib refuses {counts[0]}, gives the text {counts[1]}, "
              f"gives other bytes {counts[2]}")
    with open(path, "wb") as f:
        f.write(blob)


if __name__ == "__main__":
    main(sys.argv[1])
