// fd_seq: local alignment of amino-acid sequences (Gotoh, affine gaps) for a rectangle of chain pairs, and the length-ordered
// greedy clustering of a byte relation matrix.  include/fd_hip.h is the specification; this file says how the two launches are
// laid out.
//
// align_kernel<RMAX>  one wave per pair, one pair per block.  Lane l owns the R consecutive rows l R .. l R + R - 1 of x, R the
//                  smallest of 1 .. 8, 12, 16, 24, 32 with 64 R >= m (so a pair of short chains does not pay for the longest chain
//                  of the launch; RMAX = 2, 8 or 32, by the longest x of the launch, is what the host instantiates and what sets
//                  the register budget).
//                  The wave walks the columns of y skewed by lane: at step s lane l computes column s - l of its strip, top row
//                  first.  Per row it keeps H(i, j-1) and E(i, j-1) in registers; F runs down the strip in a register; the
//                  strip's bottom H and F tuples go to lane l + 1 by six __shfl per step, which is all the communication there is.
//                  A tuple is three registers: the score, matches << 16 | columns, i0 << 16 | j0.  The table lies in LDS as
//                  {subst[x][y], (x == y) << 16 | 1}, so the diagonal move is two adds behind one 8-byte read; y lies in LDS as
//                  bytes.  The best cell of a lane is kept under the key score << 11 | (2047 - i), compared with >: the largest
//                  score, then the smallest i, then -- a lane sees the columns of a row in ascending order -- the smallest j.  A
//                  key is unique to a row, so the maximum over the lanes is the specification's cell.  A cell only adds its
//                  score to the step's maximum; the keys are looked at in the few steps whose maximum reaches the lane's best.
//                  The DP never touches memory.  No atomics, no spin, no barrier but the one behind the staging of y; every loop
//                  bound is a chain length read from offsets (and clamped to what the registers and the LDS hold).
// greedy_kernel    one block of 1024 threads.  labels is the working state (-1: unlabelled, else the founder).  The walk reads
//                  labels[order[t]] in every thread; a founder's round is: barrier (every thread has read), the row scan (thread
//                  k takes chains k, k + 1024, ..), the round's smallest member and member count by shuffles and sixteen words of
//                  LDS (two parities, so a round does not wait for the readers of the round before), barrier.  The smallest
//                  members are marked in ws; an ordered prefix count of the marks numbers the clusters.
#include "fd_common.h"
#include "../../include/fd_hip.h"

#include <climits>
#include <cstring>
#include <vector>

namespace {

constexpr int SQ_T = 64;                          // threads of an alignment block: one wave, so that a pair that ends early frees
constexpr int SQ_WAVES = SQ_T / 64;               // its slot at once (pairs of a block; a block lives as long as its longest pair)
constexpr int SQ_MAX_L = 2048;                    // FD_SEQ_MAX_L = 64 lanes x 32 rows
constexpr int SQ_LETTERS = 21;                    // FD_SEQ_LETTERS
constexpr int SQ_NEG = -(1 << 29);                // "no gap open": below any score, and 2048 extensions of 1023 do not wrap it
constexpr int SQ_IBITS = 11;                      // bits of a row number in the key
constexpr int GT = 1024;                          // threads of the clustering block
constexpr int GW = GT / 64;

struct Tup { int s, mc, ij; };                    // score, matches << 16 | columns, i0 << 16 | j0
struct alignas(8) Ent { int s, inc; };            // subst[x][y], (x == y) << 16 | 1

template <int R>
__device__ __forceinline__ void align_strip(const unsigned char* __restrict__ x, int m, const unsigned char* yl, int n,
                                            const Ent* tab, int goe, int ge, int lane, int& bkey, int& bmc, int& bij, int& bj) {
  const int nl = (m + R - 1) / R;                 // lanes that own a row
  const int steps = n + nl - 1;
  const int row0 = lane * R;
  const int nvalid = m - row0;                    // rows r < nvalid of the strip exist
  int xo[R];
  Tup Hl[R], E[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int i = row0 + r;
    const int a = i < m ? (int)x[i] : SQ_LETTERS - 1;
    xo[r] = (a < SQ_LETTERS ? a : SQ_LETTERS - 1) * SQ_LETTERS;
    Hl[r] = Tup{0, 0, 0};
    E[r] = Tup{SQ_NEG, 0, 0};
  }
  Tup botH{0, 0, 0}, botF{SQ_NEG, 0, 0}, diag_top{0, 0, 0};
  const int src = lane ? lane - 1 : 0;
  const bool top = lane == 0;
  const int ibase = row0 << 16, kbase = (1 << SQ_IBITS) - 1 - row0;
  int bthr = 1;                                   // max(1, the score of the lane's best cell)
  for (int s = 0; s < steps; ++s) {
    // what the lane above left at its column s - lane in the step before (every lane takes part in the exchange)
    Tup upH, upF;
    upH.s = __shfl(botH.s, src), upH.mc = __shfl(botH.mc, src), upH.ij = __shfl(botH.ij, src);
    upF.s = __shfl(botF.s, src), upF.mc = __shfl(botF.mc, src), upF.ij = __shfl(botF.ij, src);
    if (top) upH = Tup{0, 0, 0}, upF = Tup{SQ_NEG, 0, 0};
    const int j = s - lane;
    if (j >= 0 && j < n) {
      const int b = (int)yl[j];
      Tup diag = diag_top;                        // H(i - 1, j - 1) of the strip's top row
      diag_top = upH;
      const int ij_here = ibase + j;
      int smax = 0;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const Tup hl = Hl[r], e = E[r];
        // E: a gap that consumes y_j, from (i, j - 1); the extension on a tie
        const int es = e.s - ge, eo = hl.s - goe;
        const bool eext = es >= eo;
        const Tup En{eext ? es : eo, (eext ? e.mc : hl.mc) + 1, eext ? e.ij : hl.ij};
        // F: a gap that consumes x_i, from (i - 1, j)
        const int fs = upF.s - ge, fo = upH.s - goe;
        const bool fext = fs >= fo;
        const Tup Fn{fext ? fs : fo, (fext ? upF.mc : upH.mc) + 1, fext ? upF.ij : upH.ij};
        // D: from H(i - 1, j - 1); an empty cell (score 0: its other two words are not kept clean) starts the alignment here
        const Ent t = tab[xo[r] + b];
        const bool cont = diag.s > 0;
        const Tup Dn{diag.s + t.s, (cont ? diag.mc : 0) + t.inc, cont ? diag.ij : ij_here + (r << 16)};
        // H: D over E over F on equal scores; not positive: empty
        Tup h = Dn;
        if (En.s > h.s) h = En;
        if (Fn.s > h.s) h = Fn;
        h.s = h.s > 0 ? h.s : 0;
        smax = h.s > smax ? h.s : smax;
        diag = hl;
        Hl[r] = h, E[r] = En;
        upH = h, upF = Fn;
      }
      // the best cell: only a step that holds a score at or above the lane's best can change it (at: a smaller i wins a tie)
      if (smax >= bthr) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const int key = (Hl[r].s << SQ_IBITS) + (kbase - r);
          if (key > bkey && r < nvalid) bkey = key, bmc = Hl[r].mc, bij = Hl[r].ij, bj = j;
        }
        const int bs = bkey >> SQ_IBITS;
        bthr = bs > 1 ? bs : 1;
      }
      botH = upH, botF = upF;
    }
  }
}

template <int RMAX>
__global__ __launch_bounds__(SQ_T) void align_kernel(const unsigned char* __restrict__ letters, const long* __restrict__ offsets,
                                                     const int* __restrict__ ids_a, int Pa, const int* __restrict__ ids_b, int Pb,
                                                     const int* __restrict__ subst, int gap_open, int gap_extend, int upper_only,
                                                     int* __restrict__ out) {
  __shared__ Ent tab[SQ_LETTERS * SQ_LETTERS];
  __shared__ unsigned char ybuf[SQ_WAVES][SQ_MAX_L];
  const int tid = (int)threadIdx.x, lane = fd::lane_id(), wave = fd::wave_id();
  for (int k = tid; k < SQ_LETTERS * SQ_LETTERS; k += SQ_T)
    tab[k] = Ent{subst[k], ((k / SQ_LETTERS == k % SQ_LETTERS) << 16) | 1};
  const long p = (long)blockIdx.x * SQ_WAVES + wave;
  const bool valid = p < (long)Pa * Pb;
  int ca = 0, cb = 0, m = 0, n = 0;
  long x0 = 0, y0 = 0;
  if (valid) {
    ca = ids_a[p / Pb], cb = ids_b[p % Pb];
    x0 = offsets[ca], y0 = offsets[cb];
    const long lm = offsets[ca + 1] - x0, ln = offsets[cb + 1] - y0;
    m = (int)(lm < 0 ? 0 : lm > 64 * RMAX ? 64 * RMAX : lm);        // (the host has refused what these clamps would cut)
    n = (int)(ln < 0 ? 0 : ln > SQ_MAX_L ? SQ_MAX_L : ln);
  }
  const bool skip = upper_only != 0 && ca >= cb;
  if (valid && !skip)
    for (int k = lane; k < n; k += 64) {
      const unsigned char b = letters[y0 + k];
      ybuf[wave][k] = b < SQ_LETTERS ? b : (unsigned char)(SQ_LETTERS - 1);
    }
  __syncthreads();
  if (!valid) return;
  int* o = out + p * FD_SEQ_SLOTS;
  if (skip) {
    if (lane < FD_SEQ_SLOTS) o[lane] = -1;
    return;
  }
  int bkey = (1 << SQ_IBITS) - 1, bmc = 0, bij = 0, bj = 0;         // the key of score 0 in row 0: only a positive score beats it
  if (m > 0 && n > 0) {
    const unsigned char* x = letters + x0;
    const int goe = gap_open + gap_extend, need = (m + 63) / 64;
#define FD_SEQ_STRIP(R, LO, HI)                                                                                       \
  if constexpr (RMAX >= R)                                                                                            \
    if (need > LO && need <= HI) align_strip<R>(x, m, ybuf[wave], n, tab, goe, gap_extend, lane, bkey, bmc, bij, bj);
    FD_SEQ_STRIP(1, 0, 1) FD_SEQ_STRIP(2, 1, 2) FD_SEQ_STRIP(3, 2, 3) FD_SEQ_STRIP(4, 3, 4) FD_SEQ_STRIP(5, 4, 5) FD_SEQ_STRIP(6, 5, 6)
    FD_SEQ_STRIP(7, 6, 7) FD_SEQ_STRIP(8, 7, 8) FD_SEQ_STRIP(12, 8, 12) FD_SEQ_STRIP(16, 12, 16) FD_SEQ_STRIP(24, 16, 24)
    FD_SEQ_STRIP(32, 24, 32)
#undef FD_SEQ_STRIP
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    const int k2 = __shfl_xor(bkey, d), mc2 = __shfl_xor(bmc, d), ij2 = __shfl_xor(bij, d), j2 = __shfl_xor(bj, d);
    if (k2 > bkey) bkey = k2, bmc = mc2, bij = ij2, bj = j2;
  }
  if (lane == 0) {
    const int score = bkey >> SQ_IBITS, i = (1 << SQ_IBITS) - 1 - (bkey & ((1 << SQ_IBITS) - 1));
    int4 lo, hi;
    if (score > 0) {
      lo.x = score, lo.y = bmc >> 16, lo.z = bmc & 0xffff, lo.w = bij >> 16;
      hi.x = i, hi.y = bij & 0xffff, hi.z = bj, hi.w = 0;
    } else {
      lo.x = 0, lo.y = 0, lo.z = 0, lo.w = -1;
      hi.x = -1, hi.y = -1, hi.z = -1, hi.w = 0;
    }
    reinterpret_cast<int4*>(o)[0] = lo;
    reinterpret_cast<int4*>(o)[1] = hi;
  }
}

__global__ __launch_bounds__(GT) void greedy_kernel(const unsigned char* __restrict__ rel, long ld, int C, const int* __restrict__ order,
                                                    int* __restrict__ ws, int* labels, int* __restrict__ rep, int* __restrict__ out) {
  __shared__ int w_min[2][GW], w_cnt[2][GW], w_tot[GW];
  const int tid = (int)threadIdx.x, lane = fd::lane_id(), wave = fd::wave_id();
  int* mark = ws;                                 // [C]: founder + 1 at the smallest member of its cluster, else 0
  int* number = ws + C;                           // [C]: the cluster number of a founder
  for (int j = tid; j < C; j += GT) labels[j] = -1, rep[j] = -1, mark[j] = 0;
  __syncthreads();
  int largest = 0, par = 0;
  for (int t = 0; t < C; ++t) {
    const int c = order[t];
    if (c < 0 || c >= C) continue;                // (the same in every thread, as is what follows)
    if (labels[c] != -1) continue;
    __syncthreads();                              // every thread has read labels[c] before one of them writes it
    int mn = INT_MAX, cnt = 0;
    for (int j = tid; j < C; j += GT) {
      if (labels[j] != -1) continue;
      const bool related = j == c || (j < c ? rel[(long)j * ld + c] : rel[(long)c * ld + j]) != 0;
      if (related) {
        labels[j] = c;
        mn = j < mn ? j : mn;
        ++cnt;
      }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
      const int u = __shfl_xor(mn, d);
      mn = u < mn ? u : mn;
      cnt += __shfl_xor(cnt, d);
    }
    if (lane == 0) w_min[par][wave] = mn, w_cnt[par][wave] = cnt;
    __syncthreads();
    mn = INT_MAX, cnt = 0;
    for (int w = 0; w < GW; ++w) {
      mn = w_min[par][w] < mn ? w_min[par][w] : mn;
      cnt += w_cnt[par][w];
    }
    if (tid == 0) mark[mn] = c + 1;               // (c itself is a member, so mn <= c < C)
    largest = cnt > largest ? cnt : largest;
    par ^= 1;
  }
  __syncthreads();
  // ---- number the clusters by ascending smallest member: an ordered count of the marks ----
  const int per = (C + GT - 1) / GT;
  const int j0 = tid * per < C ? tid * per : C, j1 = j0 + per < C ? j0 + per : C;
  int mine = 0;
  for (int j = j0; j < j1; ++j) mine += mark[j] != 0;
  int incl = mine;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int u = __shfl(incl, lane >= d ? lane - d : lane);
    if (lane >= d) incl += u;
  }
  if (lane == 63) w_tot[wave] = incl;
  __syncthreads();
  int k = incl - mine, K = 0;
  for (int w = 0; w < GW; ++w) {
    if (w < wave) k += w_tot[w];
    K += w_tot[w];
  }
  for (int j = j0; j < j1; ++j)
    if (mark[j] != 0) {
      const int f = mark[j] - 1;
      number[f] = k;
      rep[k] = f;
      ++k;
    }
  __syncthreads();
  for (int j = tid; j < C; j += GT) {
    const int f = labels[j];
    if (f >= 0) labels[j] = number[f];            // (a chain that order does not name stays -1)
  }
  if (tid == 0) out[0] = C, out[1] = K, out[2] = largest, out[3] = 0;
}

// device memory as the host sees it, behind everything queued on the stream (the interpreter's device memory is host memory)
bool to_host(void* dst, const void* src, size_t bytes, hipStream_t stream) {
  if (bytes == 0) return true;
#if defined(__HIPCC__)
  return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, stream) == hipSuccess && hipStreamSynchronize(stream) == hipSuccess;
#else
  (void)stream;
  memcpy(dst, src, bytes);
  return true;
#endif
}

template <int RMAX>
void launch_align(const unsigned char* letters, const long* offsets, const int* ids_a, int Pa, const int* ids_b, int Pb,
                  const int* subst, int gap_open, int gap_extend, int upper_only, int* out, hipStream_t stream) {
  const unsigned blocks = (unsigned)(((long)Pa * Pb + SQ_WAVES - 1) / SQ_WAVES);
  hipLaunchKernelGGL(align_kernel<RMAX>, dim3(blocks), dim3(SQ_T), 0, stream, letters, offsets, ids_a, Pa, ids_b, Pb, subst, gap_open,
                     gap_extend, upper_only, out);
}

}  // namespace

extern "C" int fd_seq_align(const unsigned char* letters, const long* offsets, int C, const int* ids_a, int Pa, const int* ids_b,
                            int Pb, const int* subst, int gap_open, int gap_extend, int upper_only, int* out, void* stream) {
  static_assert(SQ_MAX_L == FD_SEQ_MAX_L && SQ_LETTERS == FD_SEQ_LETTERS && FD_SEQ_SLOTS == 8, "include/fd_hip.h");
  static_assert(FD_SEQ_MAX_L < (1 << SQ_IBITS) + 1 && FD_SEQ_MAX_SCORE * FD_SEQ_MAX_L < (1 << (30 - SQ_IBITS)), "the key of the best cell");
  FD_CHECK_ARG(C >= 0 && Pa >= 0 && Pb >= 0, "fd_seq_align: negative size");
  FD_CHECK_ARG(gap_open >= 0 && gap_open <= FD_SEQ_MAX_GAP, "fd_seq_align: gap_open must lie in 0 .. 1023");
  FD_CHECK_ARG(gap_extend >= 1 && gap_extend <= FD_SEQ_MAX_GAP, "fd_seq_align: gap_extend must lie in 1 .. 1023");
  if (Pa == 0 || Pb == 0) return FD_OK;
  FD_CHECK_ARG(letters && offsets && ids_a && ids_b && subst && out, "fd_seq_align: null operand");
  FD_CHECK_ARG((((uintptr_t)offsets) & 7u) == 0 && (((uintptr_t)ids_a) & 3u) == 0 && (((uintptr_t)ids_b) & 3u) == 0 &&
                   (((uintptr_t)subst) & 3u) == 0 && fd_aligned16(out),
               "fd_seq_align: misaligned operand");
  FD_CHECK_ARG(((long)Pa * Pb + SQ_WAVES - 1) / SQ_WAVES < (1L << 31), "fd_seq_align: Pa Pb must be below 2^31 (blocks in one grid)");
  // the operands decide what is refused, so they are read back before the launch: offsets, the ids, the table, the letters
  hipStream_t st = (hipStream_t)stream;
  std::vector<long> off((size_t)C + 1);
  std::vector<int> ia((size_t)Pa), ib((size_t)Pb), tab(SQ_LETTERS * SQ_LETTERS);
  bool ok = to_host(off.data(), offsets, off.size() * sizeof(long), st) && to_host(ia.data(), ids_a, ia.size() * sizeof(int), st) &&
            to_host(ib.data(), ids_b, ib.size() * sizeof(int), st) && to_host(tab.data(), subst, tab.size() * sizeof(int), st);
  if (!ok) {
    fd_set_error("fd_seq_align: could not read the operands back");
    return FD_ERR_LAUNCH;
  }
  FD_CHECK_ARG(off[0] == 0, "fd_seq_align: offsets[0] must be 0");
  for (int c = 0; c < C; ++c) FD_CHECK_ARG(off[c + 1] >= off[c], "fd_seq_align: offsets decrease at chain %d", c);
  for (int v : tab) FD_CHECK_ARG(v >= -FD_SEQ_MAX_SCORE && v <= FD_SEQ_MAX_SCORE, "fd_seq_align: a table entry of %d, outside -127 .. 127", v);
  long longest_a = 0;
  for (int k = 0; k < Pa + Pb; ++k) {
    const int c = k < Pa ? ia[k] : ib[k - Pa];
    FD_CHECK_ARG(c >= 0 && c < C, "fd_seq_align: chain id %d outside [0, %d)", c, C);
    const long len = off[c + 1] - off[c];
    FD_CHECK_ARG(len <= FD_SEQ_MAX_L, "fd_seq_align: chain %d has %ld residues, more than FD_SEQ_MAX_L = %d", c, len, FD_SEQ_MAX_L);
    if (k < Pa && len > longest_a) longest_a = len;
  }
  std::vector<unsigned char> let((size_t)off[C]);
  if (!to_host(let.data(), letters, let.size(), st)) {
    fd_set_error("fd_seq_align: could not read the letters back");
    return FD_ERR_LAUNCH;
  }
  for (size_t k = 0; k < let.size(); ++k)
    FD_CHECK_ARG(let[k] < SQ_LETTERS, "fd_seq_align: letter %d at row %ld, outside 0 .. 20", (int)let[k], (long)k);
  const int need = (int)((longest_a + 63) / 64);
  if (need <= 2) launch_align<2>(letters, offsets, ids_a, Pa, ids_b, Pb, subst, gap_open, gap_extend, upper_only, out, st);
  else if (need <= 8) launch_align<8>(letters, offsets, ids_a, Pa, ids_b, Pb, subst, gap_open, gap_extend, upper_only, out, st);
  else launch_align<32>(letters, offsets, ids_a, Pa, ids_b, Pb, subst, gap_open, gap_extend, upper_only, out, st);
  FD_CHECK_LAUNCH("fd_seq_align");
  return FD_OK;
}

extern "C" int fd_seq_greedy(const unsigned char* rel, long ld, int C, const int* order, int* ws, int* labels, int* rep, int* out,
                             void* stream) {
  FD_CHECK_ARG(C >= 0, "fd_seq_greedy: negative size");
  if (C == 0) return FD_OK;
  FD_CHECK_ARG(C <= FD_SEQ_GREEDY_MAX_C, "fd_seq_greedy: C must be at most 2^30");
  FD_CHECK_ARG(rel && order && ws && labels && rep && out, "fd_seq_greedy: null operand");
  FD_CHECK_ARG(ld >= C, "fd_seq_greedy: ld must be at least C");
  FD_CHECK_ARG((((uintptr_t)order) & 3u) == 0 && (((uintptr_t)ws) & 3u) == 0 && (((uintptr_t)labels) & 3u) == 0 &&
                   (((uintptr_t)rep) & 3u) == 0 && (((uintptr_t)out) & 3u) == 0,
               "fd_seq_greedy: misaligned operand");
  FD_CHECK_ARG(ws != labels && ws != rep && labels != rep, "fd_seq_greedy: ws, labels and rep must be distinct");
  hipLaunchKernelGGL(greedy_kernel, dim3(1), dim3(GT), 0, (hipStream_t)stream, rel, ld, C, order, ws, labels, rep, out);
  FD_CHECK_LAUNCH("fd_seq_greedy");
  return FD_OK;
}
