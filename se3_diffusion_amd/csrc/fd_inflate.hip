// fd_inflate: the texts of F files laid end to end from their gzip members (RFC 1952 around RFC 1951), or copied through.
// include/fd_hip.h is the specification; this file says how the one launch is laid out.
//
// One wave per file, one wave per block.  A DEFLATE stream is a serial bit stream, so the decode state (bit buffer, input and
// output positions, the current tables' use) is the same in all 64 lanes: every lane decodes every symbol, and the lanes differ
// only where bytes move -- a literal is stored by lane 0, the bytes of a match and of a stored block are spread over the lanes,
// the code tables are built a code length per lane, and the CRC32 is taken a slice per lane.
//
//   tables   canonical: count[len] codes of each length and the symbols in the order (length, symbol).  A symbol is decoded a bit
//            at a time, at most 15 steps.  The lengths are written to LDS by lane 0 while all lanes read the stream, then a
//            barrier, then lane len counts and places the symbols of its length, then a barrier: nobody reads what is being
//            written.
//   matches  out is the window.  A barrier in front of every match makes the bytes written so far visible to all lanes; the
//            sources of a match all lie in front of its first byte (out[p + i] = out[p - dist + i % dist]), so the lanes need
//            no order among themselves.
//   bounds   the bit reader loads in[pos] only for pos < the file's end; a store goes to out[op] only after op + count <= the
//            file's out end was checked; a match is copied only after dist <= op - the file's out start was checked.  Every
//            symbol takes at least one bit and every stored block 32, so the input length bounds the work; the header's
//            scans stop at the file's end.
#include "fd_common.h"
#include "../../include/fd_hip.h"

namespace {

constexpr int IW = 64;                            // threads of a block: one wave
constexpr int NLIT = 288, NDIST = 32, NCL = 19;   // symbols of the three codes (the fixed codes use all 288 and 32)
constexpr unsigned CRC_POLY = 0xEDB88320u;

struct Bits {
  const unsigned char* in;
  long pos, end;                                  // next byte to load, the file's end (absolute in `in`)
  unsigned long long buf;
  int cnt;
};

__device__ __forceinline__ void refill(Bits& b) {
#pragma unroll
  for (int k = 0; k < 8; ++k)
    if (b.cnt <= 56 && b.pos < b.end) {
      b.buf |= (unsigned long long)b.in[b.pos++] << b.cnt;
      b.cnt += 8;
    }
}

// the next n bits (0 .. 16), the first lowest; -1 when the file ends in front of them
__device__ __forceinline__ int take(Bits& b, int n) {
  if (b.cnt < n) {
    refill(b);
    if (b.cnt < n) return -1;
  }
  const int v = (int)(b.buf & ((1u << n) - 1u));
  b.buf >>= n;
  b.cnt -= n;
  return v;
}

// back to whole bytes: the bits of a started byte are dropped, whole bytes in the buffer are unread
__device__ __forceinline__ void to_bytes(Bits& b) {
  b.pos -= b.cnt >> 3;
  b.buf = 0;
  b.cnt = 0;
}

// one symbol of a canonical code; -1: the file ends first, -2: no such code
__device__ __forceinline__ int decode(Bits& b, const unsigned short* count, const unsigned short* sym) {
  int code = 0, first = 0, index = 0;
  for (int len = 1; len <= 15; ++len) {
    const int bit = take(b, 1);
    if (bit < 0) return -1;
    code |= bit;
    const int c = count[len];
    if (code - c < first) return sym[index + (code - first)];
    index += c;
    first = (first + c) << 1;
    code <<= 1;
  }
  return -2;
}

// count and sym of the code with lengths lens[0 .. n): lane len < 16 counts its length and places its symbols (between barriers)
__device__ void build(const unsigned char* lens, int n, unsigned short* count, unsigned short* sym, int lane) {
  if (lane >= 16) return;
  int c = 0, at = 0;
  for (int i = 0; i < n; ++i) {
    const int l = lens[i];
    c += l == lane;
    at += l > 0 && l < lane;
  }
  count[lane] = (unsigned short)c;
  if (lane == 0) return;
  for (int i = 0; i < n; ++i)
    if (lens[i] == lane) sym[at++] = (unsigned short)i;
}

// 0: a complete code; 1: codes are left over and RFC 1951 as zlib reads it allows that (no code at all, or a single code of one
// bit; never for the code-length code); -1: over-subscribed, or incomplete otherwise
__device__ int check(const unsigned short* count, int n, bool lengths_code) {
  int left = 1;
  for (int len = 1; len <= 15; ++len) {
    left = (left << 1) - count[len];
    if (left < 0) return -1;
  }
  if (left == 0) return 0;
  return (!lengths_code && count[0] + count[1] == n) ? 1 : -1;
}

// a x b mod the CRC polynomial, bit 31 being x^0 (the reflected form the CRC itself uses)
__device__ unsigned mulmod(unsigned a, unsigned b) {
  unsigned p = 0;
  for (int i = 0; i < 32; ++i) {
    if (a & (0x80000000u >> i)) p ^= b;
    b = (b >> 1) ^ ((b & 1u) ? CRC_POLY : 0u);
  }
  return p;
}

struct Tables {                                   // of one block, in LDS
  unsigned short lcount[16], lsym[NLIT], dcount[16], dsym[NDIST];
  unsigned char lens[NLIT + NDIST];               // code lengths: the literal/length code's from 0, the distance code's from NLIT
  unsigned crct[256];
};

#define FAIL(kind, at) return (long)(at) * 16 + (kind)
#define HERE (b.pos - (b.cnt >> 3) - i0)

// the member in[i0 .. i1) inflated into out[o0 .. o1); all lanes run this with the same arguments and return the same word
__device__ long inflate_member(const unsigned char* in, long i0, long i1, unsigned char* out, long o0, long o1, int verify,
                               int lane, Tables& t) {
  unsigned short *lcount = t.lcount, *lsym = t.lsym, *dcount = t.dcount, *dsym = t.dsym;
  unsigned char* lens = t.lens;
  unsigned* crct = t.crct;

  // ---- the header (RFC 1952) ----
  const long n = i1 - i0;
  if ((n >= 1 && in[i0] != 0x1f) || (n >= 2 && in[i0 + 1] != 0x8b)) FAIL(FD_INFLATE_HEADER, 0);
  if (n < 10) FAIL(FD_INFLATE_ENDS, n);
  if (in[i0 + 2] != 8) FAIL(FD_INFLATE_HEADER, 2);
  const int flg = in[i0 + 3];
  if (flg & 0xE0) FAIL(FD_INFLATE_HEADER, 3);
  long p = i0 + 10;
  if (flg & 4) {                                  // FEXTRA: XLEN and that many bytes
    if (i1 - p < 2) FAIL(FD_INFLATE_ENDS, n);
    const long xlen = in[p] | (in[p + 1] << 8);
    p += 2;
    if (i1 - p < xlen) FAIL(FD_INFLATE_ENDS, n);
    p += xlen;
  }
  for (int bit = 8; bit <= 16; bit <<= 1)         // FNAME, FCOMMENT: up to a zero byte
    if (flg & bit) {
      while (p < i1 && in[p] != 0) ++p;
      if (p >= i1) FAIL(FD_INFLATE_ENDS, n);
      ++p;
    }
  if (flg & 2) {                                  // FHCRC: skipped, not checked
    if (i1 - p < 2) FAIL(FD_INFLATE_ENDS, n);
    p += 2;
  }

  // ---- the blocks (RFC 1951) ----
  Bits b{in, p, i1, 0ull, 0};
  long op = o0;
  int last = 0;
  while (!last) {
    last = take(b, 1);
    const int type = take(b, 2);
    if (last < 0 || type < 0) FAIL(FD_INFLATE_ENDS, n);
    if (type == 3) FAIL(FD_INFLATE_BLOCK, HERE);
    if (type == 0) {
      to_bytes(b);
      if (i1 - b.pos < 4) FAIL(FD_INFLATE_ENDS, n);
      const int len = in[b.pos] | (in[b.pos + 1] << 8), nlen = in[b.pos + 2] | (in[b.pos + 3] << 8);
      if ((len ^ nlen) != 0xffff) FAIL(FD_INFLATE_BLOCK, b.pos - i0);
      b.pos += 4;
      if (i1 - b.pos < len) FAIL(FD_INFLATE_ENDS, n);
      if (o1 - op < len) FAIL(FD_INFLATE_SIZE, b.pos - i0);
      for (int i = lane; i < len; i += IW) out[op + i] = in[b.pos + i];
      b.pos += len;
      op += len;
      continue;
    }
    int nl, nd;
    if (type == 1) {
      for (int i = lane; i < NLIT; i += IW) lens[i] = i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8;
      if (lane < NDIST) lens[NLIT + lane] = 5;
      nl = NLIT;
      nd = NDIST;
    } else {
      nl = take(b, 5);
      nd = take(b, 5);
      const int nc = take(b, 4);
      if (nl < 0 || nd < 0 || nc < 0) FAIL(FD_INFLATE_ENDS, n);
      nl += 257;
      nd += 1;
      if (nl > 286 || nd > 30) FAIL(FD_INFLATE_CODES, HERE);
      // the code-length code: 3 bits each in the order of RFC 1951 3.2.7 (order[k] packed five bits apiece)
      const unsigned long long order_lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 |
                                          6ull << 35 | 10ull << 40 | 5ull << 45 | 11ull << 50 | 4ull << 55;
      const unsigned long long order_hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
      if (lane == 0)
        for (int k = 0; k < NCL; ++k) lens[k] = 0;
      for (int k = 0; k < nc + 4; ++k) {
        const int v = take(b, 3);
        if (v < 0) FAIL(FD_INFLATE_ENDS, n);
        const int s = (int)((k < 12 ? order_lo >> (5 * k) : order_hi >> (5 * (k - 12))) & 31u);
        if (lane == 0) lens[s] = (unsigned char)v;
      }
      __syncthreads();
      build(lens, NCL, lcount, lsym, lane);
      __syncthreads();
      if (check(lcount, NCL, true) != 0) FAIL(FD_INFLATE_CODES, HERE);
      // the nl + nd code lengths, run-length coded by that code
      int k = 0, prev = 0;
      while (k < nl + nd) {
        const int s = decode(b, lcount, lsym);
        if (s == -1) FAIL(FD_INFLATE_ENDS, n);
        if (s < 0) FAIL(FD_INFLATE_CODES, HERE);
        int rep = 1, val = s;
        if (s >= 16) {
          if (s == 16 && k == 0) FAIL(FD_INFLATE_CODES, HERE);
          const int extra = take(b, s == 16 ? 2 : s == 17 ? 3 : 7);
          if (extra < 0) FAIL(FD_INFLATE_ENDS, n);
          rep = extra + (s == 18 ? 11 : 3);
          val = s == 16 ? prev : 0;
          if (k + rep > nl + nd) FAIL(FD_INFLATE_CODES, HERE);
        }
        // (positions k < nl are the literal/length code's, the others the distance code's, kept at lens[NLIT ..])
        if (lane == 0)
          for (int r = 0; r < rep; ++r) lens[k + r < nl ? k + r : NLIT + (k + r - nl)] = (unsigned char)val;
        k += rep;
        prev = val;
      }
    }
    __syncthreads();                              // the lengths are written; every lane is done with the tables in front
    const bool no_end = lens[256] == 0;
    build(lens, nl, lcount, lsym, lane);
    build(lens + NLIT, nd, dcount, dsym, lane);
    __syncthreads();
    if (no_end || check(lcount, nl, false) < 0 || check(dcount, nd, false) < 0) FAIL(FD_INFLATE_CODES, HERE);

    // the symbols of the block
    for (;;) {                                    // (a symbol takes at least one bit: the input's length bounds the loop)
      int s = decode(b, lcount, lsym);
      if (s == -1) FAIL(FD_INFLATE_ENDS, n);
      if (s < 0) FAIL(FD_INFLATE_SYMBOL, HERE);
      if (s < 256) {
        if (op >= o1) FAIL(FD_INFLATE_SIZE, HERE);
        if (lane == 0) out[op] = (unsigned char)s;
        ++op;
        continue;
      }
      if (s == 256) break;
      s -= 257;
      if (s >= 29) FAIL(FD_INFLATE_SYMBOL, HERE);
      // lengths 3 .. 258: symbols 257 .. 264 have no extra bits, then four symbols share each number of extra bits
      int len, ebits = 0;
      if (s < 8) len = 3 + s;
      else if (s == 28) len = 258;
      else {
        ebits = (s >> 2) - 1;
        len = 3 + ((4 + (s & 3)) << ebits);
      }
      int e = take(b, ebits);
      if (e < 0) FAIL(FD_INFLATE_ENDS, n);
      len += e;
      int d = decode(b, dcount, dsym);
      if (d == -1) FAIL(FD_INFLATE_ENDS, n);
      if (d < 0 || d >= 30) FAIL(FD_INFLATE_SYMBOL, HERE);
      // distances 1 .. 32768: symbols 0 .. 3 have no extra bits, then two symbols share each number of extra bits
      int dist;
      ebits = 0;
      if (d < 4) dist = 1 + d;
      else {
        ebits = (d >> 1) - 1;
        dist = 1 + ((2 + (d & 1)) << ebits);
      }
      e = take(b, ebits);
      if (e < 0) FAIL(FD_INFLATE_ENDS, n);
      dist += e;
      if (dist > op - o0) FAIL(FD_INFLATE_SYMBOL, HERE);
      if (o1 - op < len) FAIL(FD_INFLATE_SIZE, HERE);
      __syncthreads();                            // the bytes in front of op are written
      const unsigned char* src = out + (op - dist);
      if (dist >= len)
        for (int i = lane; i < len; i += IW) out[op + i] = src[i];
      else
        for (int i = lane; i < len; i += IW) out[op + i] = src[i % dist];
      op += len;
    }
  }

  // ---- the trailer ----
  to_bytes(b);
  if (i1 - b.pos < 8) FAIL(FD_INFLATE_ENDS, n);
  unsigned crc = 0, isize = 0;
  for (int k = 0; k < 4; ++k) {
    crc |= (unsigned)in[b.pos + k] << (8 * k);
    isize |= (unsigned)in[b.pos + 4 + k] << (8 * k);
  }
  if (i1 - b.pos > 8) FAIL(FD_INFLATE_TRAILING, b.pos + 8 - i0);
  if (op != o1 || isize != (unsigned)((o1 - o0) & 0xffffffffL)) FAIL(FD_INFLATE_SIZE, b.pos + 4 - i0);
  if (!verify) return 0;

  // ---- CRC32: a slice per lane, joined by x^(8 bytes behind the slice) mod the polynomial ----
  __syncthreads();
  for (int i = lane; i < 256; i += IW) {
    unsigned c = (unsigned)i;
    for (int k = 0; k < 8; ++k) c = (c >> 1) ^ ((c & 1u) ? CRC_POLY : 0u);
    crct[i] = c;
  }
  __syncthreads();
  const long total = o1 - o0, slice = (total + IW - 1) / IW;
  const long a = lane * slice < total ? lane * slice : total, z = a + slice < total ? a + slice : total;
  unsigned c = 0xffffffffu;
  for (long i = a; i < z; ++i) c = crct[(c ^ out[o0 + i]) & 0xffu] ^ (c >> 8);
  c ^= 0xffffffffu;
  unsigned long long behind = (unsigned long long)(total - z);      // bytes; x^8 per byte
  unsigned shift = 0x80000000u, power = 0x00800000u;                // x^0, x^8
  for (int k = 0; k < 40; ++k) {
    if (behind & 1ull) shift = mulmod(shift, power);
    power = mulmod(power, power);
    behind >>= 1;
  }
  c = mulmod(shift, c);
  for (int o = 32; o > 0; o >>= 1) c ^= __shfl_xor(c, o);
  if (c != crc) FAIL(FD_INFLATE_CRC, b.pos - i0);
  return 0;
}

__global__ void __launch_bounds__(IW) inflate_kernel(const unsigned char* in, long n_in, const long* in_offsets, int F, const int* kind,
                                                     unsigned char* out, long n_out, const long* out_offsets, int verify,
                                                     long* status) {
  __shared__ Tables tables;
  const int f = (int)blockIdx.x, lane = (int)threadIdx.x;
  if (f >= F) return;
  const long i0 = in_offsets[f], i1 = in_offsets[f + 1], o0 = out_offsets[f], o1 = out_offsets[f + 1];
  long word;
  if (i0 < 0 || i1 < i0 || i1 > n_in || o0 < 0 || o1 < o0 || o1 > n_out) {
    word = FD_INFLATE_ENDS;                       // offsets that leave the buffers: nothing is read or written
  } else if (kind[f] == 0) {
    const long n = i1 - i0 < o1 - o0 ? i1 - i0 : o1 - o0;
    for (long i = lane; i < n; i += IW) out[o0 + i] = in[i0 + i];
    word = (i1 - i0 == o1 - o0) ? 0 : n * 16 + FD_INFLATE_SIZE;
  } else {
    word = inflate_member(in, i0, i1, out, o0, o1, verify, lane, tables);
  }
  if (lane == 0) status[f] = word;
}

}  // namespace

extern "C" int fd_inflate(const unsigned char* in, long n_in, const long* in_offsets, int F, const int* kind, unsigned char* out,
                          long n_out, const long* out_offsets, int verify, long* status, void* stream) {
  FD_CHECK_ARG(F >= 0 && n_in >= 0 && n_out >= 0, "fd_inflate: negative size");
  if (F == 0) return FD_OK;
  FD_CHECK_ARG(in_offsets && kind && out_offsets && status && (in || n_in == 0) && (out || n_out == 0), "fd_inflate: null operand");
  FD_CHECK_ARG(((((uintptr_t)in_offsets) | ((uintptr_t)out_offsets) | ((uintptr_t)status)) & 7u) == 0 && (((uintptr_t)kind) & 3u) == 0,
               "fd_inflate: misaligned operand");
  hipLaunchKernelGGL(inflate_kernel, dim3((unsigned)F), dim3(IW), 0, (hipStream_t)stream, in, n_in, in_offsets, F, kind, out, n_out,
                     out_offsets, verify, status);
  FD_CHECK_LAUNCH("fd_inflate");
  return FD_OK;
}
