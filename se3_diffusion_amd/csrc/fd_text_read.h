// What the two structure-file readers (fd_pdb_read.hip, fd_cif_read.hip) share: the text of F files end to end, a thread's window
// of 16 bytes and the line starts in it, the ordered block scan, the block minimum, the atom37 and residue name tables, and the
// digits-to-number rule.  include/fd_hip.h is the specification of both readers.
#pragma once
#include "fd_common.h"
#include "../../include/fd_hip.h"

namespace {

constexpr int RT = 256;                           // threads of a block: four waves
constexpr int RWAVES = RT / 64;
constexpr int RW = FD_PDB_READ_WINDOW;            // bytes of a thread's window
constexpr int RCHUNK = FD_PDB_READ_CHUNK;         // bytes of a block's chunk
static_assert(RT * RW == RCHUNK && RW == 16, "a window is one 16-byte load, a chunk 256 of them");
constexpr long R_OK = FD_PDB_STATUS_OK;
constexpr int R_SLOTS = 37;

constexpr unsigned pack3(const char* s) {         // a name of at most three characters, the first in the low byte
  unsigned v = 0;
  for (int k = 0; k < 3 && s[k]; ++k) v |= (unsigned)(unsigned char)s[k] << (8 * k);
  return v;
}

// the 37 atom names in atom37 order and the 20 residue names in aatype order
__device__ const unsigned kAtom[R_SLOTS] = {
    pack3("N"),   pack3("CA"),  pack3("C"),   pack3("CB"),  pack3("O"),   pack3("CG"),  pack3("CG1"), pack3("CG2"),
    pack3("OG"),  pack3("OG1"), pack3("SG"),  pack3("CD"),  pack3("CD1"), pack3("CD2"), pack3("ND1"), pack3("ND2"),
    pack3("OD1"), pack3("OD2"), pack3("SD"),  pack3("CE"),  pack3("CE1"), pack3("CE2"), pack3("CE3"), pack3("NE"),
    pack3("NE1"), pack3("NE2"), pack3("OE1"), pack3("OE2"), pack3("CH2"), pack3("NH1"), pack3("NH2"), pack3("OH"),
    pack3("CZ"),  pack3("CZ2"), pack3("CZ3"), pack3("NZ"),  pack3("OXT")};
__device__ const unsigned kRes[20] = {pack3("ALA"), pack3("ARG"), pack3("ASN"), pack3("ASP"), pack3("CYS"), pack3("GLN"), pack3("GLU"),
                                      pack3("GLY"), pack3("HIS"), pack3("ILE"), pack3("LEU"), pack3("LYS"), pack3("MET"), pack3("PHE"),
                                      pack3("PRO"), pack3("SER"), pack3("THR"), pack3("TRP"), pack3("TYR"), pack3("VAL")};
// a packed name of at most three characters -> atom37 slot or -1, aatype or 20
__device__ __forceinline__ int slot_of_name(unsigned nm) {
  int slot = -1;
  for (int s = 0; s < R_SLOTS; ++s) slot = kAtom[s] == nm ? s : slot;
  return slot;
}
__device__ __forceinline__ int aatype_of_name(unsigned nm) {
  int a = 20;
  for (int r = 0; r < 20; ++r) a = kRes[r] == nm ? r : a;
  return a;
}

struct Text {
  const unsigned char* t;                         // n bytes
  long n;
  const long* off;                                // [F+1]
  int F;
  int hetatm, model_all;
};

// The join of the threads in front of this one, in thread order, and of the whole block; every thread of the block calls it.
// R is what a thread knows of the text in front of a line: an associative join(a, b) of a in front of b, shfl_run(r, lane) and
// R::none(), the join's identity.  Shuffles in the wave, the four wave totals in wave order.
template <class R>
__device__ __forceinline__ R block_scan(const R& mine, R* wtot, R& total) {
  const int lane = fd::lane_id(), wave = fd::wave_id();
  R incl = mine;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const R u = shfl_run(incl, lane >= o ? lane - o : lane);
    if (lane >= o) incl = join(u, incl);
  }
  const R left = shfl_run(incl, lane > 0 ? lane - 1 : 0);
  if (lane == 63) wtot[wave] = incl;
  __syncthreads();
  R before = R::none();
  total = before;
  for (int w = 0; w < RWAVES; ++w) {
    if (w < wave) before = join(before, wtot[w]);
    total = join(total, wtot[w]);
  }
  __syncthreads();                                // wtot is written again by the next scan
  return lane > 0 ? join(before, left) : before;
}

__device__ __forceinline__ long block_min(long v, long* wmin) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const long u = __shfl_xor(v, o);
    v = u < v ? u : v;
  }
  if (fd::lane_id() == 0) wmin[fd::wave_id()] = v;
  __syncthreads();
  for (int w = 0; w < RWAVES; ++w) v = wmin[w] < v ? wmin[w] : v;
  __syncthreads();
  return v;
}

// the file of byte pos: the largest f < F with off[f] <= pos (an empty file holds no byte and is never the answer)
__device__ __forceinline__ int file_of(const long* __restrict__ off, int F, long pos) {
  int lo = 0, hi = F - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (off[mid] <= pos) lo = mid; else hi = mid - 1;
  }
  return lo;
}
__device__ __forceinline__ long file_end(const Text& x, int f) {
  const long e = x.off[f + 1];
  return e < x.n ? e : x.n;
}

// A thread's window: bit k of `starts` is set when a line starts at ws + k; f is the file of the window's first byte.
struct Window {
  long ws, we;
  unsigned starts;
  int f;
};
__device__ __forceinline__ Window open_window(const Text& x, long ws) {
  Window w{ws, ws + RW < x.n ? ws + RW : x.n, 0u, 0};
  if (ws >= x.n) return w;
  unsigned q[4];
  if (ws + RW <= x.n) {
    __builtin_memcpy(q, x.t + ws, 16);            // (ws is a multiple of 16 and the text 16-byte aligned)
  } else {
    for (int i = 0; i < 4; ++i) {
      unsigned v = 0;
      for (int e = 0; e < 4; ++e) v |= (ws + 4 * i + e < x.n ? (unsigned)x.t[ws + 4 * i + e] : 0u) << (8 * e);
      q[i] = v;
    }
  }
  unsigned prev = ws > 0 ? (unsigned)x.t[ws - 1] : (unsigned)'\n';
#pragma unroll
  for (int k = 0; k < RW; ++k) {
    if (prev == '\n' && ws + k < x.n) w.starts |= 1u << k;
    prev = (q[k >> 2] >> (8 * (k & 3))) & 0xffu;
  }
  w.f = file_of(x.off, x.F, ws);
  if (x.off[w.f] == ws) w.starts |= 1u;           // the first byte of a file starts a line
  for (int g = w.f + 1; g < x.F && x.off[g] < w.we; ++g)
    if (x.off[g + 1] > x.off[g] && x.off[g] > ws) w.starts |= 1u << (int)(x.off[g] - ws);
  return w;
}

// A number, one byte at a time: blanks, an optional sign, digits (POINT: with at most one '.'), blanks.  The value is the integer
// mantissa over 10^(digits behind the point) in fp64, rounded once to fp32; more than 15 digits are not a number (the mantissa
// stays exact in fp64).
struct Digits {
  int state = 0;                                  // 0 blanks in front, 1 sign, 2 digits, 3 behind the point, 4 blanks behind
  long m = 0;
  double scale = 1.0;
  int nd = 0;
  bool neg = false, bad = false;
  template <bool POINT>
  __device__ __forceinline__ void feed(unsigned c) {
    if (c == ' ') {
      if (state == 1) bad = true;
      else if (state != 0) state = 4;
    } else if (c == '+' || c == '-') {
      if (state != 0) bad = true;
      neg = c == '-';
      state = 1;
    } else if (c >= '0' && c <= '9') {
      if (state == 4 || nd == 15) bad = true;
      else m = m * 10 + (long)(c - '0');
      ++nd;
      if (state == 3) scale *= 10.0; else state = 2;
    } else if (POINT && c == '.') {
      if (state > 2) bad = true;
      state = 3;
    } else {
      bad = true;
      state = 4;
    }
  }
  // 0: a number, 1: all blank, 2: anything else
  __device__ __forceinline__ int fixed(float& value) const {
    if (state == 0 && !bad) return 1;
    if (bad || nd == 0) return 2;
    const float v = (float)((double)m / scale);
    value = neg ? -v : v;
    return 0;
  }
  // false: anything but an integer (all blank included)
  __device__ __forceinline__ bool integer(long& value) const {
    value = neg ? -m : m;
    return !bad && nd > 0;
  }
};

}  // namespace
