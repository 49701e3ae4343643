"""se3_diffusion_amd.pdb.inflate and the gzip= path of parse_pdb / parse_mmcif: gzip members inflated on the device, one wave per
file (csrc/fd_inflate.hip, fd_inflate).

Every comparison is == on bytes or array_equal.  The oracle is the standard library: zlib.decompress(data, 31) and zlib.crc32.
Streams come from zlib.compressobj(level, DEFLATED, 31, 9, strategy) and, for what zlib never emits (a distance of 32768, chosen
(length, distance) tokens, a single distance code, broken streams), from the small bit writer below.  read_stream() is a plain
pure-Python inflate that also reports what a stream holds (block types, longest code, largest distance, the lengths seen): every
case asserts through it that its stream reaches what the case is for, and it must agree with zlib.
Every case runs on the interpreter and, marked gpu, on the device; the library of files runs on the device only.
"""
import functools
import gzip as gzip_module
import io
import os
import sys
import zlib

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from se3_diffusion_amd import hip, pdb  # noqa: E402

FIELDS = ("atom_positions", "atom_mask", "b_factors", "aatype", "residue_index", "chain_offsets", "chain_file", "chain_model",
          "chain_id", "n_dropped")
HEADER, ENDS, BLOCK, CODES, SYMBOL, SIZE, CRC, TRAILING = 1, 2, 3, 4, 5, 6, 7, 8      # FD_INFLATE_*
RECORD = b"ATOM      1  N   ALA A   1      11.104   6.134  -6.504  1.00  0.00           N  \n"

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_BITS = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577]
DIST_BITS = [0, 0, 0, 0] + [b for b in range(1, 14) for _ in (0, 1)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


@pytest.fixture(params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def dev(request):
    """the device the library under test runs on: the interpreter build on the CPU, or the product library on the GPU"""
    if request.param == "emu":
        request.getfixturevalue("use_emu")
        return "cpu"
    request.getfixturevalue("hip_lib")
    return "cuda"


@functools.lru_cache(None)
def gold(name):
    return np.load(os.path.join(ROOT, "tests", "golden", name))


@functools.lru_cache(None)
def pdb_texts():
    g = gold("pdb.npz")
    return {str(c): g[f"{c}.text"].tobytes() for c in g["cases"]}


@functools.lru_cache(None)
def cif_texts():
    g = gold("mmcif_read.npz")
    return {k: g[k].tobytes() for k in g.files if ".file" in k and not k.endswith(".files")}


# ---- the stream maker ------------------------------------------------------------------------------------------------------------
def gz(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, 31, 9, strategy)
    return c.compress(data) + c.flush()


def member(deflate, payload, flg=0, mtime=0, extra=b"", tail=None):
    """a gzip member around a raw DEFLATE stream: `extra` is what stands between the ten fixed header bytes and the stream"""
    head = bytes([0x1f, 0x8b, 8, flg]) + mtime.to_bytes(4, "little") + bytes([0, 255]) + extra
    tail = zlib.crc32(payload).to_bytes(4, "little") + (len(payload) & 0xffffffff).to_bytes(4, "little") if tail is None else tail
    return head + deflate + tail


def canonical(lens):
    """{symbol: (code, length)} of the canonical Huffman code with these lengths (RFC 1951 3.2.2)"""
    code, out = 0, {}
    for n in range(1, 16):
        for s, l in enumerate(lens):
            if l == n:
                out[s] = (code, n)
                code += 1
        code <<= 1
    return out


class Writer:
    """DEFLATE bits: values lowest bit first, Huffman codes highest bit first"""

    def __init__(self):
        self.bits = []

    def value(self, v, n):
        self.bits += [(v >> k) & 1 for k in range(n)]

    def code(self, c):
        self.bits += [(c[0] >> k) & 1 for k in reversed(range(c[1]))]

    def align(self):
        self.bits += [0] * (-len(self.bits) % 8)

    def raw(self, data):
        self.align()
        for b in data:
            self.value(b, 8)

    def tokens(self, tokens, lit, dist):
        """literals (ints or bytes), (length, distance) pairs, ("lit", symbol) and ("dist", length symbol, distance symbol)"""
        for t in tokens:
            if isinstance(t, (bytes, bytearray)):
                for b in t:
                    self.code(lit[b])
            elif isinstance(t, int):
                self.code(lit[t])
            elif t[0] == "lit":
                self.code(lit[t[1]])
            else:
                length, distance = t
                ls = 28 if length == 258 else max(k for k in range(28) if LEN_BASE[k] <= length)
                ds = max(k for k in range(30) if DIST_BASE[k] <= distance)
                self.code(lit[257 + ls])
                self.value(length - LEN_BASE[ls], LEN_BITS[ls])
                self.code(dist[ds])
                self.value(distance - DIST_BASE[ds], DIST_BITS[ds])
        self.code(lit[256])

    def fixed(self, tokens, last=True):
        self.value(int(last), 1)
        self.value(1, 2)
        self.tokens(tokens, canonical(FIXED_LIT), canonical(FIXED_DIST))
        return self

    def dynamic(self, lit_lens, dist_lens, tokens, last=True):
        """a dynamic block whose code lengths are sent one by one with a code-length code of 16 codes of four bits"""
        self.value(int(last), 1)
        self.value(2, 2)
        self.value(len(lit_lens) - 257, 5)
        self.value(len(dist_lens) - 1, 5)
        self.value(19 - 4, 4)
        for s in CL_ORDER:
            self.value(4 if s < 16 else 0, 3)
        cl = canonical([4] * 16)
        for l in list(lit_lens) + list(dist_lens):
            self.code(cl[l])
        if tokens is not None:
            self.tokens(tokens, canonical(lit_lens), canonical(dist_lens))
        return self

    def stored(self, data, last=True, nlen=None):
        self.value(int(last), 1)
        self.value(0, 2)
        self.align()
        self.value(len(data), 16)
        self.value((len(data) ^ 0xffff) if nlen is None else nlen, 16)
        self.raw(data)
        return self

    def bytes(self):
        self.align()
        b = self.bits
        return bytes(sum(b[k + j] << j for j in range(8)) for k in range(0, len(b), 8))


def replay(tokens):
    """the bytes that literal and (length, distance) tokens stand for"""
    out = bytearray()
    for t in tokens:
        if isinstance(t, (bytes, bytearray)):
            out += t
        elif isinstance(t, int):
            out.append(t)
        else:
            for _ in range(t[0]):
                out.append(out[-t[1]])
    return bytes(out)


def hand(tokens):
    """one fixed block of these tokens as a gzip member"""
    return member(Writer().fixed(tokens).bytes(), replay(tokens))


# ---- the instrumented reader -----------------------------------------------------------------------------------------------------
class Seen:
    def __init__(self):
        self.types, self.max_code, self.max_dist, self.lengths, self.dist_codes = [], 0, 0, set(), []


def read_stream(data):
    """(the inflated bytes, what the stream holds) of one gzip member, written from RFC 1951 / 1952: plain and slow"""
    assert data[:3] == b"\x1f\x8b\x08"
    flg, p = data[3], 10
    if flg & 4:
        p += 2 + int.from_bytes(data[p:p + 2], "little")
    for bit in (8, 16):
        if flg & bit:
            p = data.index(b"\0", p) + 1
    if flg & 2:
        p += 2
    pos, seen, out = [p * 8], Seen(), bytearray()

    def take(n):
        v = 0
        for k in range(n):
            v |= ((data[pos[0] >> 3] >> (pos[0] & 7)) & 1) << k
            pos[0] += 1
        return v

    def table(lens):
        t = {(c, l): s for s, (c, l) in canonical(lens).items()}
        seen.max_code = max(seen.max_code, max(lens))
        return t

    def symbol(t):
        c = 0
        for l in range(1, 16):
            c = c << 1 | take(1)
            if (c, l) in t:
                return t[c, l]
        raise ValueError("no such code")

    last = 0
    while not last:
        last, kind = take(1), take(2)
        seen.types.append(kind)
        if kind == 0:
            pos[0] += -pos[0] % 8
            n = take(16)
            assert take(16) == n ^ 0xffff
            out += data[pos[0] >> 3:(pos[0] >> 3) + n]
            pos[0] += 8 * n
            continue
        if kind == 1:
            lit, dist = table(FIXED_LIT), table(FIXED_DIST)
            seen.max_code = max(seen.max_code, 9)
        else:
            nl, nd, nc = take(5) + 257, take(5) + 1, take(4) + 4
            cl = [0] * 19
            for k in range(nc):
                cl[CL_ORDER[k]] = take(3)
            keep, seen.max_code = seen.max_code, 0
            clt = table(cl)
            seen.max_code = keep
            lens = []
            while len(lens) < nl + nd:
                s = symbol(clt)
                if s < 16:
                    lens.append(s)
                elif s == 16:
                    lens += [lens[-1]] * (3 + take(2))
                else:
                    lens += [0] * (3 + take(3) if s == 17 else 11 + take(7))
            assert len(lens) == nl + nd
            lit = table(lens[:nl])
            dist = table(lens[nl:]) if any(lens[nl:]) else {}
            seen.dist_codes.append(sum(1 for l in lens[nl:] if l))
        while True:
            s = symbol(lit)
            if s < 256:
                out.append(s)
            elif s == 256:
                break
            else:
                n = LEN_BASE[s - 257] + take(LEN_BITS[s - 257])
                d = symbol(dist)
                d = DIST_BASE[d] + take(DIST_BITS[d])
                seen.lengths.add(n)
                seen.max_dist = max(seen.max_dist, d)
                assert d <= len(out)
                for _ in range(n):
                    out.append(out[-d])
    at = (pos[0] + 7) >> 3
    assert int.from_bytes(data[at:at + 4], "little") == zlib.crc32(out) and int.from_bytes(data[at + 4:at + 8], "little") == len(out)
    assert at + 8 == len(data)
    return bytes(out), seen


def checked(stream, text=None):
    """the stream's text by zlib; the instrumented reader agrees"""
    want = zlib.decompress(stream, 31)
    got, seen = read_stream(stream)
    assert got == want and (text is None or want == text)
    return want, seen


def inflated(inputs, dev, **kw):
    """pdb.inflate's texts as a list of bytes, one per file"""
    text, off, names = pdb.inflate(inputs, **kw)
    assert text.dtype == torch.uint8 and text.device.type == dev and text.data_ptr() % 16 == 0
    assert off.dtype == np.int64 and off[0] == 0 and off[-1] == text.numel() and len(names) == len(off) - 1
    raw = text.cpu().numpy().tobytes()
    return [raw[off[k]:off[k + 1]] for k in range(len(off) - 1)]


# ---- stored, fixed and dynamic blocks --------------------------------------------------------------------------------------------
def test_stored_blocks(dev):
    text = np.random.default_rng(0).integers(0, 256, 70000, dtype=np.uint8).tobytes()
    stream = gz(text, 0)
    _, seen = checked(stream, text)
    assert seen.types == [0, 0]                                     # 70,000 bytes do not fit one stored block
    empty_first = member(Writer().stored(b"", last=False).fixed([RECORD]).bytes(), RECORD)
    _, seen = checked(empty_first, RECORD)
    assert seen.types == [0, 1]
    assert inflated([stream, empty_first], dev) == [text, RECORD]


def test_fixed_blocks(dev):
    text = RECORD * 50
    stream = gz(text, 6, zlib.Z_FIXED)
    _, seen = checked(stream, text)
    assert seen.types == [1] and seen.lengths
    nothing = gzip_module.compress(b"")
    _, seen = checked(nothing, b"")
    assert len(nothing) == 20 and seen.types == [1]
    assert inflated([stream, nothing], dev) == [text, b""]


@pytest.mark.parametrize("level", [9, 1])
def test_dynamic_blocks_golden_texts(dev, level):
    texts = list(pdb_texts().values()) + list(cif_texts().values())
    streams = [gz(t, level) for t in texts]
    seen = [checked(s, t)[1] for s, t in zip(streams, texts)]
    assert all(2 in s.types for s, t in zip(seen, texts) if len(t) > 1000)
    assert inflated(streams, dev) == texts


def test_dynamic_blocks_full_flush(dev):
    text = max(pdb_texts().values(), key=len)
    c = zlib.compressobj(6, zlib.DEFLATED, 31, 9)
    cut = [0, len(text) // 3, 2 * len(text) // 3, len(text)]
    stream = b"".join(c.compress(text[a:z]) + c.flush(zlib.Z_FULL_FLUSH) for a, z in zip(cut, cut[1:])) + c.flush()
    _, seen = checked(stream, text)
    assert seen.types[:5] == [2, 0, 2, 0, 2]                        # an empty stored block between dynamic ones
    assert inflated(stream, dev) == [text]


# ---- long codes ------------------------------------------------------------------------------------------------------------------
def test_code_lengths_of_15(dev):
    fib = [1, 1]
    while len(fib) < 24:
        fib.append(fib[-1] + fib[-2])
    text = np.repeat(np.arange(40, 64, dtype=np.uint8), fib)
    np.random.default_rng(1).shuffle(text)
    text = text.tobytes()
    stream = gz(text, 6, zlib.Z_HUFFMAN_ONLY)
    _, seen = checked(stream, text)
    assert seen.max_code == 15 and not seen.lengths
    assert inflated(stream, dev) == [text]


def test_single_distance_code(dev):
    lit = [0] * 261
    lit[97] = lit[98] = lit[256] = lit[260] = 2                     # 'a', 'b', end of block, length 6
    tokens = [b"ab", (6, 1)]
    stream = member(Writer().dynamic(lit, [1], tokens).bytes(), replay(tokens))
    text, seen = checked(stream, b"abbbbbbb")
    assert seen.types == [2] and seen.dist_codes == [1]             # one distance code of one bit: an incomplete set zlib allows
    assert inflated(stream, dev) == [text]


# ---- match boundaries ------------------------------------------------------------------------------------------------------------
def boundary_streams():
    rng = np.random.default_rng(2)
    lead = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    cases = {"len3": [b"abc", (3, 3)], "len258": [lead(300), (258, 300)], "run": [b"a", (258, 1), (258, 1), (3, 1)],
             "first_byte": [b"abcde", (5, 5), b"x", (11, 11)]}
    for d in (2, 3, 63, 64, 65):
        for n in sorted({3, max(3, d - 1), max(3, d), d + 1, 130, 258}):      # below the distance (where 3 allows), at it, above
            cases[f"d{d}_n{n}"] = [lead(d + 7), (n, d), b"!", (n, d)]
    cases["d32768"] = [lead(32768), (258, 32768), (3, 32768)]
    return {k: (hand(t), replay(t)) for k, t in cases.items()}


def test_match_boundaries(dev):
    cases = boundary_streams()
    seen = {k: checked(s, t)[1] for k, (s, t) in cases.items()}
    assert seen["len3"].lengths == {3} and seen["len258"].lengths == {258} and seen["run"].max_dist == 1
    assert seen["d32768"].max_dist == 32768 and len(cases["d32768"][1]) == 32768 + 261
    for d in (63, 64, 65):
        assert seen[f"d{d}_n{d - 1}"].lengths == {d - 1} and seen[f"d{d}_n258"].max_dist == d
    assert inflated([s for s, _ in cases.values()], dev) == [t for _, t in cases.values()]


# ---- the header ------------------------------------------------------------------------------------------------------------------
def test_header_fields(dev):
    text = RECORD * 3
    raw = zlib.compressobj(6, zlib.DEFLATED, -15)
    deflate = raw.compress(text) + raw.flush()
    named = io.BytesIO()
    with gzip_module.GzipFile(filename="1abc.pdb", mode="wb", fileobj=named, mtime=1700000000) as f:
        f.write(text)
    named = named.getvalue()
    assert named[3] == 8 and named[4:8] != b"\0\0\0\0" and b"1abc.pdb\0" in named
    extra = b"\x05\x00hello"
    plain_head = bytes([0x1f, 0x8b, 8, 4 | 16 | 2]) + bytes(4) + bytes([0, 255]) + extra + b"a comment\0"
    full = member(deflate, text, flg=4 | 16 | 2, extra=extra + b"a comment\0" + (zlib.crc32(plain_head) & 0xffff).to_bytes(2, "little"))
    everything = member(deflate, text, flg=4 | 8 | 16, mtime=12345, extra=b"\x00\x00" + b"name\0" + b"\0")
    for s in (named, full, everything):
        checked(s, text)
    assert inflated([named, full, everything], dev) == [text] * 3


# ---- batches ---------------------------------------------------------------------------------------------------------------------
def test_batch_of_nine(dev):
    rng = np.random.default_rng(3)
    texts = pdb_texts()
    big = rng.integers(0, 256, 70000, dtype=np.uint8).tobytes()
    far = boundary_streams()["d32768"]
    c = zlib.compressobj(6, zlib.DEFLATED, 31, 9)
    flushed = c.compress(RECORD * 7) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(RECORD * 5) + c.flush()
    dynamic = texts["single"]
    files = [(gz(big, 0), big), (RECORD * 3 + b"END", None), (gz(RECORD * 50, 6, zlib.Z_FIXED), RECORD * 50), (b"", None),
             (gz(dynamic, 9), dynamic), (gzip_module.compress(b""), b""), far, (RECORD[:37], None), (flushed, RECORD * 12)]
    want = [t if t is not None else s for s, t in files]
    for s, t in files:
        if t is not None:
            checked(s, t)
    off = pdb.inflate([s for s, _ in files])[1]
    assert any(o % 16 for o in off[1:-1])
    assert inflated([s for s, _ in files], dev) == want
    assert want == [inflated(s, dev)[0] for s, _ in files]          # the per-file results
    mixed = [torch.frombuffer(bytearray(want[1]), dtype=torch.uint8).to(dev), files[2][0], want[7]]      # a device entry is text
    assert inflated(mixed, dev) == [want[1], want[2], want[7]]


def test_far_match_beside_short_files(dev):
    first = boundary_streams()["first_byte"]
    far = boundary_streams()["d32768"]
    short = (hand([b"zzz", (3, 3)]), b"zzzzzz")
    files = [short, first, short, far, first, short]
    assert inflated([s for s, _ in files] + [b"tail"], dev) == [t for _, t in files] + [b"tail"]


@pytest.mark.gpu
def test_library_of_files(hip_lib):
    """what the interpreter cannot do in seconds: 600 files in one call"""
    texts = (list(pdb_texts().values()) + list(cif_texts().values())) * 40
    texts = texts[:600]
    streams = [gz(t, 6) for t in texts]
    assert inflated(streams, "cuda") == texts


# ---- through the readers ---------------------------------------------------------------------------------------------------------
def same(a, b):
    return a.n_files == b.n_files and all(np.array_equal(getattr(a, k).cpu().numpy(), getattr(b, k).cpu().numpy()) for k in FIELDS)


def launches(fn):
    lib = hip.get_lib()
    n0 = lib.cdll.fd_launch_count()
    out = fn()
    return out, lib.cdll.fd_launch_count() - n0


def test_parse_pdb_of_gzip(dev, tmp_path):
    texts = list(pdb_texts().values())[:4]
    plain, n_plain = launches(lambda: pdb.parse_pdb(texts, model="all", gzip=False))
    assert plain.num_residues > 0
    zipped, n_zipped = launches(lambda: pdb.parse_pdb([gz(t) for t in texts], model="all"))
    assert same(plain, zipped) and n_zipped == n_plain + 1          # one more launch
    auto, n_auto = launches(lambda: pdb.parse_pdb(texts, model="all"))
    assert same(plain, auto) and n_auto == n_plain                  # no gzip entry: today's path
    paths = []
    for k, t in enumerate(texts):
        paths.append(str(tmp_path / f"pdb{k}.ent.gz"))
        with open(paths[-1], "wb") as f:
            f.write(gz(t, 9))
    assert same(plain, pdb.parse_pdb(paths, model="all"))
    on_dev = [torch.frombuffer(bytearray(gz(t)), dtype=torch.uint8).to(dev) for t in texts]
    assert same(plain, pdb.parse_pdb(on_dev, model="all", gzip=True))
    assert same(plain, pdb.parse_pdb([texts[0], gz(texts[1]), paths[2], texts[3]], model="all"))


def test_parse_mmcif_of_gzip(dev, tmp_path):
    g = gold("mmcif_read.npz")
    texts = [g[f"permuted.file{k}"].tobytes() for k in range(int(g["permuted.files"]))]
    texts += [g[f"chains.file{k}"].tobytes() for k in range(int(g["chains.files"]))]
    plain, n_plain = launches(lambda: pdb.parse_mmcif(texts, gzip=False))
    assert plain.num_residues > 0
    zipped, n_zipped = launches(lambda: pdb.parse_mmcif([gz(t) for t in texts]))
    assert same(plain, zipped) and n_zipped == n_plain + 1
    auto, n_auto = launches(lambda: pdb.parse_mmcif(texts))
    assert same(plain, auto) and n_auto == n_plain
    path = str(tmp_path / "1abc.cif.gz")
    with open(path, "wb") as f:
        f.write(gz(texts[0], 9))
    assert same(pdb.parse_mmcif(texts[0], gzip=False), pdb.parse_mmcif(path))
    on_dev = [torch.frombuffer(bytearray(gz(t)), dtype=torch.uint8).to(dev) for t in texts]
    assert same(plain, pdb.parse_mmcif(on_dev, gzip=True))


def test_parse_pdb_feats_of_gzip(dev, tmp_path):
    text = pdb_texts()["single"]
    plain, zipped = str(tmp_path / "x.pdb"), str(tmp_path / "x.pdb.gz")
    with open(plain, "wb") as f:
        f.write(text)
    with gzip_module.open(zipped, "wb") as f:
        f.write(text)
    a, b = pdb.parse_pdb_feats("x", plain), pdb.parse_pdb_feats("x", zipped)
    assert sorted(a) == sorted(b) and len(a["aatype"]) > 0 and all(np.array_equal(a[k], b[k]) for k in a)


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def refused(inputs, index, kind, **kw):
    with pytest.raises(ValueError) as e:
        pdb.inflate(inputs, **kw)
    assert f"file {index} " in str(e.value) and f"(kind {kind})" in str(e.value) and pdb.INFLATE_KINDS[kind] in str(e.value), str(e.value)
    data = inputs[index] if isinstance(inputs, list) else inputs
    oracle = zlib.decompressobj(31)                                 # the oracle refuses it too, or leaves bytes unread
    try:
        oracle.decompress(data)
        whole = oracle.eof and not oracle.unused_data
    except zlib.error:
        whole = False
    assert not whole


def cut_keeping_room(stream, at, need):
    """the first cut at or behind `at` whose last four bytes, which the caller reads as ISIZE, leave room for `need` bytes: the cut
    is then met by the stream's reader, not by the end of the output"""
    while int.from_bytes(stream[at - 4:at], "little") < need:
        at += 1
    assert at < len(stream) - 8
    return stream[:at]


def test_refused_cuts(dev):
    text = RECORD * 50
    named = io.BytesIO()
    with gzip_module.GzipFile(filename="a" * 40 + ".pdb", mode="wb", fileobj=named, mtime=0) as f:
        f.write(text)
    refused(named.getvalue()[:30], 0, ENDS, gzip=True)              # inside the header's file name
    stream = gz(text)
    refused(cut_keeping_room(stream, len(stream) // 2, len(text)), 0, ENDS)
    assert stream[-4] != 0                                          # (the cut's last four bytes read as a large ISIZE)
    refused(stream[:-3], 0, ENDS)                                   # inside the trailer
    with pytest.raises(ValueError, match="file 1 .*17 bytes"):
        pdb.inflate([stream, stream[:17]], gzip=True)


def test_refused_trailer(dev):
    text = RECORD * 50
    stream = gz(text)
    bad_crc = stream[:-8] + bytes([stream[-8] ^ 1]) + stream[-7:]
    refused(bad_crc, 0, CRC)
    assert inflated(bad_crc, dev, verify=False) == [text]
    refused(stream[:-4] + bytes([stream[-4] ^ 1]) + stream[-3:], 0, SIZE)
    refused(stream[:-4] + bytes([stream[-4] ^ 16]) + stream[-3:], 0, SIZE)
    refused(stream + b"\xff\xff\xff", 0, TRAILING)
    refused(stream + stream, 0, TRAILING)


def test_refused_streams(dev):
    type3 = Writer()
    type3.value(1, 1)
    type3.value(3, 2)
    refused(member(type3.bytes(), b""), 0, BLOCK)
    refused(member(Writer().stored(b"abcdef", nlen=0x1234).bytes(), b"abcdef"), 0, BLOCK)
    before = [b"a", (3, 2)]                                         # a distance of 2 behind one byte
    refused(member(Writer().fixed(before).bytes(), b"aaaa"), 0, SYMBOL)
    refused(member(Writer().fixed([b"ab", ("lit", 286)]).bytes(), b"ab"), 0, SYMBOL)
    over = [0] * 257
    over[97] = over[98] = over[256] = 1                             # three codes of one bit
    refused(member(Writer().dynamic(over, [1], None).bytes() + bytes(4), b""), 0, CODES)


def test_refused_headers(dev):
    text = RECORD * 50
    stream = gz(text)
    refused(stream[:3] + bytes([stream[3] | 0x20]) + stream[4:], 0, HEADER)
    refused(text, 0, HEADER, gzip=True)                             # a text file declared gzip
    refused(stream[:2] + b"\x07" + stream[3:], 0, HEADER)           # CM = 7


def test_refused_smallest_index_and_size(dev):
    text = RECORD * 50
    stream = gz(text)
    bad_crc = stream[:-8] + bytes([stream[-8] ^ 1]) + stream[-7:]
    refused([stream, text, bad_crc, stream + stream, stream], 2, CRC)
    refused([stream, text, stream + stream, bad_crc], 2, TRAILING)
    lib = hip.get_lib()
    n0 = lib.cdll.fd_launch_count()
    with pytest.raises(ValueError, match=r"file 1 .*ISIZE.* 4050 bytes, above max_inflated=4000"):
        pdb.inflate([gz(RECORD), stream], max_inflated=4000)
    assert lib.cdll.fd_launch_count() == n0                         # refused before anything is launched
    assert inflated([gz(RECORD), stream], dev, max_inflated=4050) == [RECORD, text]
    with pytest.raises(ValueError, match="gzip="):
        pdb.inflate(stream, gzip="yes")
