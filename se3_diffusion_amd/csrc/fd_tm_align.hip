// fd_tm_align: TM-align's search over residue-to-residue alignments (Zhang & Skolnick 2005) as include/fd_hip.h restates it:
// four initial alignments, a Needleman-Wunsch dynamic programme on the device, and the iteration between the DP and the
// superposition search of fd_tm_core.h.  Three launches, no host synchronisation, no floating-point atomics.
//
// seed    grid P x parts, four waves.  Every block compacts both chains into LDS (six fp32 arrays of 1024).  The units of a pair
//         -- the gapless offsets, then the fragment pairs -- are dealt to the waves round-robin; ONE WAVE runs a unit from end
//         to end (superposition, DP, traceback, quick score) with wave collectives only, so four units' DPs run at once and a
//         unit's arithmetic does not depend on the wave.  Each wave leaves its best gapless unit (with its superposition) and
//         its best fragment unit in the workspace.
// refine  grid P x 4, one block per candidate class.  It reduces the partials of its class in a fixed order (greatest score,
//         lowest unit), rebuilds that unit's alignment (the same arithmetic, so the same bits), or builds the secondary-structure
//         alignments, and iterates DP <-> search.  The search shares its seeds over the four waves and reduces through LDS
//         (greatest score, lowest seed); the DP runs on wave 0 while the others wait at the barrier that follows it.
// final   grid P: picks the class, drops the pairs beyond d8, runs the two full searches and writes out, map and transform.
//
// The DP is a wave-systolic anti-diagonal sweep: lane l owns row i0 + l of a strip of 64 rows and computes column s - l at step
// s; val and path of the row above come from lane l - 1 by __shfl (what that lane computed one step earlier), the diagonal is the
// value received the step before, the left neighbour is the lane's own previous result.  Lane 0 reads the row above from an
// LDS row buffer, into which the strip's last lane writes its row for the next strip -- 63 columns behind lane 0's reads, so the
// buffer is updated in place.  S(i, j) is computed on the fly from the coordinates in LDS (the lane's own point is transformed
// once per strip).  Two bits per cell are kept -- path, and the direction the traceback takes where path is false, which the
// forward pass decides from exactly the two sums the specification's traceback compares -- in words of 32 columns, in LDS
// where they fit and otherwise in the caller's workspace.  No block barrier inside a DP.  The traceback is lane 0's walk; it
// writes the pair list backwards, so the list ends at the end of its buffer ("tail-aligned").
#include "fd_common.h"
#include "fd_tm_core.h"
#include "../../include/fd_hip.h"

namespace {

using namespace fdtm;

constexpr int AT = 256;
constexpr int AW = AT / 64;
constexpr int A_MAX_N = FD_TM_ALIGN_MAX_N;
constexpr int A_PER = A_MAX_N / AT;               // positions per thread of the compaction pass
constexpr int A_PART = 32;                        // doubles per wave partial: class 0 (score, unit, R | t), class 3 at 16 (score, unit)
constexpr int A_REC = 16;                         // doubles per (pair, class) record: s, pairs, DPs, valid, R | t
constexpr int A_SEED_BITS = 1024;                 // words of LDS per wave for the DP's bits in the seed launch (128 x 128 cells)
constexpr int A_REFINE_BITS = 4096;               // ... and for the one DP wave of a refine block (256 x 256 cells)
constexpr int A_MAX_ITER = 20;

// wave-private hand-over through memory: the writes of some lanes are read by others after this point (the rendezvous is what
// the host interpreter needs, the fence what the device needs)
__device__ __forceinline__ void wave_handover() {
#if defined(__HIP_DEVICE_COMPILE__)
  __threadfence_block();
#endif
  (void)__shfl(0, 0);
}

struct Chains {
  const float *ax, *ay, *az, *bx, *by, *bz;       // compacted, in LDS
  const unsigned char *sa, *sb;                   // CA secondary-structure classes (only where a score uses them)
  int La, Lb;
};

struct List {                                     // a pair list of n pairs occupies [A_MAX_N - n, A_MAX_N) of both arrays
  unsigned short *ka, *kb;
};

struct DpScore {                                  // S(i, j) = (use_d ? 1 / (1 + d2 / dd) : 0) + we E(i, j)
  int use_d;
  double rt[12], dd, we;
};

// Compacts the present positions of one chain into LDS; returns their number.  Thread t owns the positions [t per, (t + 1) per).
__device__ int stage_chain(const float* __restrict__ src, long stride, const float* __restrict__ mask, int N, float* x, float* y,
                           float* z, unsigned short* ridx, int* wave_tot) {
  const int tid = (int)threadIdx.x, lane = fd::lane_id(), wave = fd::wave_id();
  const int per = (N + AT - 1) / AT;
  const int r0 = tid * per;
  unsigned present = 0;
#pragma unroll
  for (int k = 0; k < A_PER; ++k) {
    const int r = r0 + k;
    if (k < per && r < N && (!mask || mask[r] != 0.f)) present |= 1u << k;
  }
  const int cnt = __builtin_popcount(present);
  int incl = cnt;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl(incl, lane >= o ? lane - o : lane);
    if (lane >= o) incl += u;
  }
  __syncthreads();                                // (wave_tot may still be read from the previous chain)
  if (lane == 63) wave_tot[wave] = incl;
  __syncthreads();
  int base = incl - cnt, L = 0;
  for (int w = 0; w < AW; ++w) {
    if (w < wave) base += wave_tot[w];
    L += wave_tot[w];
  }
#pragma unroll
  for (int k = 0; k < A_PER; ++k) {
    if (present & (1u << k)) {
      const float* p = src + (long)(r0 + k) * stride;
      x[base] = p[0];
      y[base] = p[1];
      z[base] = p[2];
      if (ridx) ridx[base] = (unsigned short)(r0 + k);
      ++base;
    }
  }
  __syncthreads();
  return L;
}

// CA secondary structure of compacted residue i of a chain of L: 0 C, 1 H, 2 E, 3 T
__device__ unsigned char ca_ss(const float* x, const float* y, const float* z, int i, int L) {
  if (i < 2 || i > L - 3) return 0;
  auto D = [&](int p, int q) {
    const double dx = (double)x[p] - (double)x[q], dy = (double)y[p] - (double)y[q], dz = (double)z[p] - (double)z[q];
    return sqrt(dx * dx + dy * dy + dz * dz);
  };
  const double d13 = D(i - 2, i), d14 = D(i - 2, i + 1), d15 = D(i - 2, i + 2), d24 = D(i - 1, i + 1), d25 = D(i - 1, i + 2),
               d35 = D(i, i + 2);
  if (fabs(d15 - 6.37) < 2.1 && fabs(d14 - 5.18) < 2.1 && fabs(d25 - 5.18) < 2.1 && fabs(d13 - 5.45) < 2.1 &&
      fabs(d24 - 5.45) < 2.1 && fabs(d35 - 5.45) < 2.1)
    return 1;
  if (fabs(d15 - 13.0) < 1.42 && fabs(d14 - 10.4) < 1.42 && fabs(d25 - 10.4) < 1.42 && fabs(d13 - 6.1) < 1.42 &&
      fabs(d24 - 6.1) < 1.42 && fabs(d35 - 6.1) < 1.42)
    return 2;
  return d15 < 8.0 ? 3 : 0;
}

struct Consts {
  int Lmin, m, n0, f, ja, jb, na, nb, n3;
  double d0, d0sq, d0s, d8;
};

__device__ __forceinline__ Consts align_consts(int La, int Lb) {
  Consts c;
  c.Lmin = La < Lb ? La : Lb;
  const int half = c.Lmin / 2 > 5 ? c.Lmin / 2 : 5;
  c.m = c.Lmin < half ? c.Lmin : half;
  c.n0 = La + Lb - 2 * c.m + 1;
  c.f = c.Lmin / 3 < 20 ? c.Lmin / 3 : 20;
  const int ca = (La - c.f + 1 + 7) / 8, cb = (Lb - c.f + 1 + 7) / 8;
  c.ja = c.f > ca ? c.f : ca;
  c.jb = c.f > cb ? c.f : cb;
  c.na = c.f >= 4 ? (La - c.f) / c.ja + 1 : 0;
  c.nb = c.f >= 4 ? (Lb - c.f) / c.jb + 1 : 0;
  c.n3 = c.na * c.nb;
  c.d0 = tm_d0(c.Lmin) + 0.8;
  c.d0sq = c.d0 * c.d0;
  c.d0s = c.d0 < 4.5 ? 4.5 : (c.d0 > 8.0 ? 8.0 : c.d0);
  c.d8 = 1.5 * pow((double)c.Lmin, 0.3) + 3.5;
  return c;
}

__device__ __forceinline__ TmPairs make_pairs(const Chains& c, const unsigned short* ka, const unsigned short* kb, int n, double lnorm) {
  TmPairs q;
  q.ax = c.ax, q.ay = c.ay, q.az = c.az, q.bx = c.bx, q.by = c.by, q.bz = c.bz;
  q.ka = ka, q.kb = kb;
  q.L = n;
  q.nj = (n + 63) >> 6;
  q.lane = fd::lane_id();
  q.lnorm = lnorm;
  return q;
}

// DP(S, gap) of the header on one wave; the alignment goes to `out` tail-aligned, its number of pairs is returned (all lanes).
__device__ int dp_wave(const Chains& c, const DpScore& sc, double gap, volatile double* rowv, volatile unsigned char* rowp,
                       unsigned* bits, List out) {
  const int lane = fd::lane_id();
  const int La = c.La, Lb = c.Lb, WB = (Lb + 31) >> 5;
  for (int j = lane; j <= Lb; j += 64) {
    rowv[j] = 0.0;
    rowp[j] = 0;
  }
  wave_handover();
  for (int i0 = 0; i0 < La; i0 += 64) {
    const int rows = La - i0 < 64 ? La - i0 : 64;
    const int i = i0 + lane;
    const bool active = lane < rows;
    const bool keep_row = lane == 63 && i0 + 64 < La;
    double px = 0.0, py = 0.0, pz = 0.0;
    unsigned char si = 0;
    if (active) {
      const double ax = (double)c.ax[i], ay = (double)c.ay[i], az = (double)c.az[i];
      px = sc.rt[0] * ax + sc.rt[1] * ay + sc.rt[2] * az + sc.rt[9];
      py = sc.rt[3] * ax + sc.rt[4] * ay + sc.rt[5] * az + sc.rt[10];
      pz = sc.rt[6] * ax + sc.rt[7] * ay + sc.rt[8] * az + sc.rt[11];
      if (sc.we != 0.0) si = c.sa[i];
    }
    double cur_v = 0.0, diag = 0.0, left_v = 0.0;
    int cur_p = 0, left_p = 0;
    unsigned pw = 0, dw = 0;
    const int steps = Lb + rows - 1;
    for (int s = 0; s < steps; ++s) {
      const int j = s - lane;
      double up_v = __shfl(cur_v, lane > 0 ? lane - 1 : 0);
      int up_p = __shfl(cur_p, lane > 0 ? lane - 1 : 0);
      if (!(active && j >= 0 && j < Lb)) continue;
      if (lane == 0) {
        up_v = rowv[j + 1];
        up_p = rowp[j + 1];
      }
      double S = 0.0;
      if (sc.use_d) {
        const double dx = px - (double)c.bx[j], dy = py - (double)c.by[j], dz = pz - (double)c.bz[j];
        S = 1.0 / (1.0 + (dx * dx + dy * dy + dz * dz) / sc.dd);
      }
      if (sc.we != 0.0) S += sc.we * (si == c.sb[j] ? 1.0 : 0.0);
      const double h = (j == 0 ? 0.0 : diag) + S;
      const double v = up_v + (up_p ? gap : 0.0);
      const double z = left_v + (left_p ? gap : 0.0);
      const double mx = v > z ? v : z;
      const int p = h >= mx ? 1 : 0;
      const double val = p ? h : mx;
      pw |= (unsigned)p << (j & 31);
      dw |= (z >= v ? 1u : 0u) << (j & 31);       // the traceback's "v >= h": step to the left, else up
      if ((j & 31) == 31 || j == Lb - 1) {
        unsigned* w = bits + ((long)i * WB + (j >> 5)) * 2;
        w[0] = pw;
        w[1] = dw;
        pw = 0;
        dw = 0;
      }
      diag = up_v;
      left_v = val;
      left_p = p;
      cur_v = val;
      cur_p = p;
      if (keep_row) {
        rowv[j + 1] = val;
        rowp[j + 1] = (unsigned char)p;
      }
    }
  }
  wave_handover();
  int n = 0;
  if (lane == 0) {
    int i = La, j = Lb, pos = A_MAX_N;
    while (i > 0 && j > 0) {
      const volatile unsigned* w = bits + ((long)(i - 1) * WB + ((j - 1) >> 5)) * 2;
      const unsigned bit = 1u << ((j - 1) & 31);
      if (w[0] & bit) {
        --pos;
        out.ka[pos] = (unsigned short)(i - 1);
        out.kb[pos] = (unsigned short)(j - 1);
        --i;
        --j;
      } else if (w[1] & bit) {
        --j;
      } else {
        --i;
      }
    }
    n = A_MAX_N - pos;
  }
  wave_handover();
  return __shfl(n, 0);
}

// quick(alignment) of the header on one wave: the score (-1 below three pairs) and its superposition
__device__ double quick_wave(const TmPairs& q, double d0sq, double d0s, double (&best_rt)[12]) {
  if (q.L < 3) return -1.0;
  double rt[12];
  tm_superpose(q, tm_all(q), rt);
  double best = tm_score_pass(q, rt, d0sq, 0.0, nullptr);
#pragma unroll
  for (int k = 0; k < 12; ++k) best_rt[k] = rt[k];
  double dc = d0s;
  for (int r = 0; r < 2; ++r) {
    const unsigned sel = tm_select(q, rt, dc * dc);
    if (fd::wave_sum(__builtin_popcount(sel)) < 3) break;
    tm_superpose(q, sel, rt);
    const double s = tm_score_pass(q, rt, d0sq, 0.0, nullptr);
    if (s > best) {
      best = s;
#pragma unroll
      for (int k = 0; k < 12; ++k) best_rt[k] = rt[k];
    }
    dc = d0s + 1.0;
  }
  return best;
}

// the gapless alignment of unit u (offset k = u - (La - m)): a_i <-> b_{i + k} over the overlap; returns its length
__device__ int write_gapless(const Consts& k, int La, int Lb, int u, List l, int first, int stride) {
  const int off = u - (La - k.m);
  const int lo = off < 0 ? -off : 0;
  const int hi = La < Lb - off ? La : Lb - off;
  const int n = hi - lo;
  for (int t = first; t < n; t += stride) {
    l.ka[A_MAX_N - n + t] = (unsigned short)(lo + t);
    l.kb[A_MAX_N - n + t] = (unsigned short)(lo + off + t);
  }
  return n;
}

// the alignment of fragment unit v on one wave: superpose the two fragments, DP(1 / (1 + d2 / (d0 + 1.5)^2), 0)
__device__ int fragment_wave(const Chains& c, const Consts& k, int v, volatile double* rowv, volatile unsigned char* rowp,
                             unsigned* bits, List l) {
  const int lane = fd::lane_id();
  const int sa = (v / k.nb) * k.ja, sb = (v % k.nb) * k.jb;
  if (lane < k.f) {                               // (f <= 20: one entry per lane, at the front of the buffer)
    l.ka[lane] = (unsigned short)(sa + lane);
    l.kb[lane] = (unsigned short)(sb + lane);
  }
  wave_handover();
  const TmPairs q = make_pairs(c, l.ka, l.kb, k.f, (double)k.f);
  DpScore sc;
  sc.use_d = 1;
  sc.we = 0.0;
  sc.dd = (k.d0 + 1.5) * (k.d0 + 1.5);
  tm_superpose(q, tm_all(q), sc.rt);
  return dp_wave(c, sc, 0.0, rowv, rowp, bits, l);
}

__global__ __launch_bounds__(AT) void align_seed_kernel(const float* __restrict__ A, long a_stride, int Na, const float* __restrict__ B,
                                                        long b_stride, int Nb, const int* __restrict__ ia, const int* __restrict__ ib,
                                                        const float* __restrict__ mask_a, const float* __restrict__ mask_b, int parts,
                                                        double* __restrict__ ws_part, unsigned* __restrict__ ws_bits, long bits_stride) {
  __shared__ float xa[A_MAX_N], ya[A_MAX_N], za[A_MAX_N], xb[A_MAX_N], yb[A_MAX_N], zb[A_MAX_N];
  __shared__ unsigned short lka[AW][A_MAX_N], lkb[AW][A_MAX_N];
  __shared__ double rowv[AW][A_MAX_N + 1];
  __shared__ unsigned char rowp[AW][A_MAX_N + 8];
  __shared__ unsigned lbits[AW][A_SEED_BITS];
  __shared__ int wave_tot[AW];
  const int lane = fd::lane_id(), wave = fd::wave_id();
  const long p = (long)(blockIdx.x / (unsigned)parts);
  const int part = (int)(blockIdx.x % (unsigned)parts);
  const long sa = ia ? (long)ia[p] : p, sb = ib ? (long)ib[p] : p;
  Chains c;
  c.ax = xa, c.ay = ya, c.az = za, c.bx = xb, c.by = yb, c.bz = zb;
  c.sa = nullptr, c.sb = nullptr;
  c.La = stage_chain(A + sa * Na * a_stride, a_stride, mask_a ? mask_a + sa * Na : nullptr, Na, xa, ya, za, nullptr, wave_tot);
  c.Lb = stage_chain(B + sb * Nb * b_stride, b_stride, mask_b ? mask_b + sb * Nb : nullptr, Nb, xb, yb, zb, nullptr, wave_tot);
  const int La = c.La, Lb = c.Lb;

  // ---- the units of this wave (everything below is wave-uniform; only wave collectives) ----
  double best0 = -1.0, best3 = -1.0, rt0[12], rt[12];
  int unit0 = -1, unit3 = -1;
#pragma unroll
  for (int k = 0; k < 12; ++k) rt0[k] = 0.0;
  if ((La < Lb ? La : Lb) >= 5) {
    const Consts k = align_consts(La, Lb);
    List l;
    l.ka = lka[wave], l.kb = lkb[wave];
    const long need = (long)La * ((Lb + 31) >> 5) * 2;
    unsigned* bits = need <= A_SEED_BITS ? lbits[wave] : ws_bits + ((long)blockIdx.x * AW + wave) * bits_stride;
    for (int u = AW * part + wave; u < k.n0 + k.n3; u += AW * parts) {
      if (u < k.n0) {
        const int n = write_gapless(k, La, Lb, u, l, lane, 64);
        wave_handover();
        const TmPairs q = make_pairs(c, l.ka + A_MAX_N - n, l.kb + A_MAX_N - n, n, (double)k.Lmin);
        const double s = quick_wave(q, k.d0sq, k.d0s, rt);
        if (s > best0) {
          best0 = s;
          unit0 = u;
#pragma unroll
          for (int j = 0; j < 12; ++j) rt0[j] = rt[j];
        }
      } else {
        const int n = fragment_wave(c, k, u - k.n0, rowv[wave], rowp[wave], bits, l);
        const TmPairs q = make_pairs(c, l.ka + A_MAX_N - n, l.kb + A_MAX_N - n, n, (double)k.Lmin);
        const double s = quick_wave(q, k.d0sq, k.d0s, rt);
        if (s > best3) {
          best3 = s;
          unit3 = u;
        }
      }
      wave_handover();                            // (the next unit overwrites the list)
    }
  }
  if (lane == 0) {
    double* o = ws_part + ((long)blockIdx.x * AW + wave) * A_PART;
    o[0] = best0;
    o[1] = (double)unit0;
#pragma unroll
    for (int j = 0; j < 12; ++j) o[2 + j] = rt0[j];
    o[14] = 0.0;
    o[15] = 0.0;
    o[16] = best3;
    o[17] = (double)unit3;
#pragma unroll
    for (int j = 18; j < A_PART; ++j) o[j] = 0.0;
  }
}

// the best partial of a class in a fixed order: greatest score, lowest unit on ties (every unit ran on exactly one wave)
__device__ int reduce_partials(const double* __restrict__ w, int np, int off, double (&rt)[12]) {
  double best = -1.0;
  int unit = -1, at = 0;
  for (int k = 0; k < np; ++k) {
    const double s = w[(long)k * A_PART + off];
    const int u = (int)w[(long)k * A_PART + off + 1];
    if (s > best || (s == best && u < unit)) best = s, unit = u, at = k;
  }
#pragma unroll
  for (int j = 0; j < 12; ++j) rt[j] = off == 0 ? w[(long)at * A_PART + 2 + j] : 0.0;
  return unit;
}

// search(pairs, Lnorm, d0, step) of the header on the block: the seeds go to the waves round-robin, each wave keeps its best, the
// four are reduced through LDS (greatest score, lowest seed).  Every thread returns the same (s, rt).  Two barriers.
__device__ double block_search(const TmPairs& q, double d0, int step, double (&rt)[12], double (*part)[16]) {
  const int lane = fd::lane_id(), wave = fd::wave_id();
  const double d0sq = d0 * d0;
  const double d0s = d0 < 4.5 ? 4.5 : (d0 > 8.0 ? 8.0 : d0);
  double best = -1.0, best_rt[12], first0 = 0.0;
  int best_seed = -1;
  long passes = 0;
#pragma unroll
  for (int k = 0; k < 12; ++k) best_rt[k] = 0.0;
  if (q.L < 4) {
    if (wave == 0) {
      tm_superpose(q, tm_all(q), best_rt);
      best = tm_score_pass(q, best_rt, d0sq, 0.0, nullptr);
    }
  } else {
    const TmSeeds sd = tm_seeds(q.L, step);
    for (int seed = wave; seed < sd.total; seed += AW) {
      int start, stop;
      tm_seed_range(sd, seed, step, start, stop);
      tm_run_seed(q, start, stop, seed, d0sq, d0s, A_MAX_ITER, best, best_seed, best_rt, passes, first0);
    }
  }
  __syncthreads();
  if (lane == 0) {
    part[wave][0] = best;
    part[wave][1] = (double)best_seed;
#pragma unroll
    for (int k = 0; k < 12; ++k) part[wave][2 + k] = best_rt[k];
  }
  __syncthreads();
  double b = part[0][0], sd = part[0][1];
  int at = 0;
  for (int w = 1; w < AW; ++w) {
    const double s = part[w][0], d = part[w][1];
    if (s > b || (s == b && d < sd)) b = s, sd = d, at = w;
  }
#pragma unroll
  for (int k = 0; k < 12; ++k) rt[k] = part[at][2 + k];
  return b;
}

__device__ void copy_list(List dst, List src, int n) {
  for (int t = A_MAX_N - n + (int)threadIdx.x; t < A_MAX_N; t += AT) {
    dst.ka[t] = src.ka[t];
    dst.kb[t] = src.kb[t];
  }
  __syncthreads();
}

__global__ __launch_bounds__(AT) void align_refine_kernel(const float* __restrict__ A, long a_stride, int Na, const float* __restrict__ B,
                                                          long b_stride, int Nb, const int* __restrict__ ia, const int* __restrict__ ib,
                                                          const float* __restrict__ mask_a, const float* __restrict__ mask_b,
                                                          int search_step, int max_dp, int parts, const double* __restrict__ ws_part,
                                                          unsigned* __restrict__ ws_bits, long bits_stride, double* __restrict__ ws_rec,
                                                          unsigned short* __restrict__ ws_list) {
  __shared__ float xa[A_MAX_N], ya[A_MAX_N], za[A_MAX_N], xb[A_MAX_N], yb[A_MAX_N], zb[A_MAX_N];
  __shared__ unsigned short lka[4][A_MAX_N], lkb[4][A_MAX_N];        // map0, best, previous, current
  __shared__ unsigned char ssa[A_MAX_N], ssb[A_MAX_N];
  __shared__ double rowv[A_MAX_N + 1];
  __shared__ unsigned char rowp[A_MAX_N + 8];
  __shared__ unsigned lbits[A_REFINE_BITS];
  __shared__ double part[AW][16];
  __shared__ int wave_tot[AW], sh_n, sh_same;
  const int tid = (int)threadIdx.x, lane = fd::lane_id(), wave = fd::wave_id();
  const long p = (long)(blockIdx.x / 4u);
  const int cls = (int)(blockIdx.x % 4u);
  const long sa = ia ? (long)ia[p] : p, sb = ib ? (long)ib[p] : p;
  Chains c;
  c.ax = xa, c.ay = ya, c.az = za, c.bx = xb, c.by = yb, c.bz = zb;
  c.sa = ssa, c.sb = ssb;
  c.La = stage_chain(A + sa * Na * a_stride, a_stride, mask_a ? mask_a + sa * Na : nullptr, Na, xa, ya, za, nullptr, wave_tot);
  c.Lb = stage_chain(B + sb * Nb * b_stride, b_stride, mask_b ? mask_b + sb * Nb : nullptr, Nb, xb, yb, zb, nullptr, wave_tot);
  const int La = c.La, Lb = c.Lb;
  if ((La < Lb ? La : Lb) < 5) return;            // (the final launch writes such a pair from the lengths alone)
  const Consts k = align_consts(La, Lb);
  const List l0 = {lka[0], lkb[0]}, lbest = {lka[1], lkb[1]};
  List lprev = {lka[2], lkb[2]}, lcur = {lka[3], lkb[3]};
  const long need = (long)La * ((Lb + 31) >> 5) * 2;
  unsigned* bits = need <= A_REFINE_BITS ? lbits : ws_bits + (long)blockIdx.x * bits_stride;
  const double* wp = ws_part + p * parts * AW * A_PART;
  double* rec = ws_rec + (long)blockIdx.x * A_REC;
  double rt[12];

  // ---- the initial alignment of this class -> l0, n0 ----
  int n0 = 0;
  if (cls == 0) {
    const int u = reduce_partials(wp, parts * AW, 0, rt);
    if (u >= 0) n0 = write_gapless(k, La, Lb, u, l0, tid, AT);
    __syncthreads();
  } else if (cls == 1 || cls == 2) {
    DpScore sc;
    reduce_partials(wp, parts * AW, 0, sc.rt);    // (R0, t0) of class 0; class 1 does not use it
    sc.use_d = cls == 2;
    sc.dd = k.d0sq;
    sc.we = cls == 2 ? 0.5 : 1.0;
    for (int i = tid; i < La; i += AT) ssa[i] = ca_ss(xa, ya, za, i, La);
    for (int j = tid; j < Lb; j += AT) ssb[j] = ca_ss(xb, yb, zb, j, Lb);
    __syncthreads();
    if (wave == 0) {
      const int n = dp_wave(c, sc, -1.0, rowv, rowp, bits, l0);
      if (lane == 0) sh_n = n;
    }
    __syncthreads();
    n0 = sh_n;
  } else {
    const int u = reduce_partials(wp, parts * AW, 16, rt);
    if (u >= 0 && wave == 0) {
      const int n = fragment_wave(c, k, u - k.n0, rowv, rowp, bits, l0);
      if (lane == 0) sh_n = n;
    }
    __syncthreads();
    n0 = u >= 0 ? sh_n : 0;
  }
  if (n0 < 3) {                                   // no candidate of this class
    if (tid == 0) {
      rec[0] = -1.0;
      for (int j = 1; j < A_REC; ++j) rec[j] = 0.0;
    }
    return;
  }

  // ---- refinement ----
  const double lmin = (double)k.Lmin;
  double best_rt[12];
  double best_s = block_search(make_pairs(c, l0.ka + A_MAX_N - n0, l0.kb + A_MAX_N - n0, n0, lmin), k.d0, search_step, best_rt, part);
  int nbest = n0, num_dp = 0;
  copy_list(lbest, l0, n0);
  DpScore sc;
  sc.use_d = 1;
  sc.we = 0.0;
  sc.dd = k.d0sq;
#pragma unroll
  for (int j = 0; j < 12; ++j) rt[j] = best_rt[j];
  for (int g = 0; g < 2; ++g) {
    const double gap = g == 0 ? -0.6 : 0.0;
#pragma unroll
    for (int j = 0; j < 12; ++j) rt[j] = best_rt[j];
    copy_list(lprev, l0, n0);
    int nprev = n0;
    bool have_old = false;
    double s_old = 0.0;
    for (int it = 0; it < max_dp; ++it) {
      if (wave == 0) {
#pragma unroll
        for (int j = 0; j < 12; ++j) sc.rt[j] = rt[j];
        const int n = dp_wave(c, sc, gap, rowv, rowp, bits, lcur);
        int diff = n == nprev ? 0 : 1;
        if (!diff)
          for (int t = A_MAX_N - n + lane; t < A_MAX_N; t += 64)
            diff |= (lcur.ka[t] != lprev.ka[t] || lcur.kb[t] != lprev.kb[t]) ? 1 : 0;
        diff = fd::wave_sum(diff);
        if (lane == 0) {
          sh_n = n;
          sh_same = diff == 0 ? 1 : 0;
        }
      }
      __syncthreads();
      const int n = sh_n;
      const bool same = sh_same != 0;
      ++num_dp;
      if (same) break;
      const List tmp = lprev;
      lprev = lcur;
      lcur = tmp;
      nprev = n;
      if (n < 3) break;
      const double s = block_search(make_pairs(c, lprev.ka + A_MAX_N - n, lprev.kb + A_MAX_N - n, n, lmin), k.d0, search_step, rt, part);
      if (s > best_s) {
        best_s = s;
        nbest = n;
#pragma unroll
        for (int j = 0; j < 12; ++j) best_rt[j] = rt[j];
        copy_list(lbest, lprev, n);
      }
      if (have_old && fabs(s - s_old) < 1e-6) break;
      s_old = s;
      have_old = true;
    }
    __syncthreads();                              // (sh_n, sh_same are written again by the next gap's first DP)
  }
  if (tid == 0) {
    rec[0] = best_s;
    rec[1] = (double)nbest;
    rec[2] = (double)num_dp;
    rec[3] = 1.0;
#pragma unroll
    for (int j = 0; j < 12; ++j) rec[4 + j] = best_rt[j];
  }
  unsigned short* wl = ws_list + (long)blockIdx.x * 2 * Na;
  for (int t = tid; t < nbest; t += AT) {
    wl[t] = lbest.ka[A_MAX_N - nbest + t];
    wl[Na + t] = lbest.kb[A_MAX_N - nbest + t];
  }
}

__global__ __launch_bounds__(AT) void align_final_kernel(const float* __restrict__ A, long a_stride, int Na, const float* __restrict__ B,
                                                         long b_stride, int Nb, const int* __restrict__ ia, const int* __restrict__ ib,
                                                         const float* __restrict__ mask_a, const float* __restrict__ mask_b,
                                                         const double* __restrict__ ws_rec, const unsigned short* __restrict__ ws_list,
                                                         double* __restrict__ out, int* __restrict__ map, double* __restrict__ transform) {
  __shared__ float xa[A_MAX_N], ya[A_MAX_N], za[A_MAX_N], xb[A_MAX_N], yb[A_MAX_N], zb[A_MAX_N];
  __shared__ unsigned short ra[A_MAX_N], rb[A_MAX_N], ka[A_MAX_N], kb[A_MAX_N], ka2[A_MAX_N], kb2[A_MAX_N];
  __shared__ int full[A_MAX_N];
  __shared__ double part[AW][16];
  __shared__ int wave_tot[AW];
  const int tid = (int)threadIdx.x, lane = fd::lane_id(), wave = fd::wave_id();
  const long p = (long)blockIdx.x;
  const long sa = ia ? (long)ia[p] : p, sb = ib ? (long)ib[p] : p;
  Chains c;
  c.ax = xa, c.ay = ya, c.az = za, c.bx = xb, c.by = yb, c.bz = zb;
  c.sa = nullptr, c.sb = nullptr;
  c.La = stage_chain(A + sa * Na * a_stride, a_stride, mask_a ? mask_a + sa * Na : nullptr, Na, xa, ya, za, ra, wave_tot);
  c.Lb = stage_chain(B + sb * Nb * b_stride, b_stride, mask_b ? mask_b + sb * Nb : nullptr, Nb, xb, yb, zb, rb, wave_tot);
  const int La = c.La, Lb = c.Lb, Lmin = La < Lb ? La : Lb;
  const double nan = __builtin_nan("");
  double* o = out + p * 16;
  int* mp = map + p * Na;
  for (int r = tid; r < Na; r += AT) full[r] = -1;

  // ---- the class: greatest best.s, lowest class on ties ----
  int cls = -1, n = 0, num_dp = 0;
  double best_s = -1.0, rt[12];
#pragma unroll
  for (int j = 0; j < 12; ++j) rt[j] = 0.0;
  Consts k = align_consts(La, Lb);
  if (Lmin >= 5) {
    const double* rec = ws_rec + p * 4 * A_REC;
    for (int q = 0; q < 4; ++q) {
      if (rec[q * A_REC + 3] == 0.0) continue;
      num_dp += (int)rec[q * A_REC + 2];
      if (rec[q * A_REC] > best_s) best_s = rec[q * A_REC], cls = q;
    }
  }
  if (cls < 0) {
    __syncthreads();
    for (int r = tid; r < Na; r += AT) mp[r] = -1;
    if (tid == 0) {
      o[0] = (double)La;
      o[1] = (double)Lb;
      o[2] = 0.0;
      o[3] = nan;
      o[4] = nan;
      o[5] = nan;
      o[6] = tm_d0(La);
      o[7] = tm_d0(Lb);
      o[8] = -1.0;
      o[9] = (double)num_dp;
      o[10] = Lmin >= 5 ? (double)(k.n0 + k.n3) : 0.0;
      o[11] = nan;
      for (int j = 12; j < 16; ++j) o[j] = 0.0;
      if (transform)
        for (int j = 0; j < 12; ++j) transform[p * 12 + j] = nan;
    }
    return;
  }
  {
    const double* rec = ws_rec + (p * 4 + cls) * A_REC;
    n = (int)rec[1];
#pragma unroll
    for (int j = 0; j < 12; ++j) rt[j] = rec[4 + j];
    const unsigned short* wl = ws_list + (p * 4 + cls) * 2 * Na;
    for (int t = tid; t < n; t += AT) {
      ka[t] = wl[t];
      kb[t] = wl[Na + t];
    }
  }
  __syncthreads();

  // ---- drop the pairs beyond d8 under the search-phase superposition (ordered compaction: thread t owns the pairs [t per, ..)) ----
  const TmPairs all = make_pairs(c, ka, kb, n, 1.0);
  const int per = (n + AT - 1) / AT;
  unsigned keep = 0;
#pragma unroll
  for (int j = 0; j < A_PER; ++j) {
    const int t = tid * per + j;
    if (j < per && t < n && tm_d2(all, rt, t) <= k.d8 * k.d8) keep |= 1u << j;
  }
  const int cnt = __builtin_popcount(keep);
  int incl = cnt;
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) {
    const int u = __shfl(incl, lane >= s ? lane - s : lane);
    if (lane >= s) incl += u;
  }
  __syncthreads();
  if (lane == 63) wave_tot[wave] = incl;
  __syncthreads();
  int base = incl - cnt, nk = 0;
  for (int w = 0; w < AW; ++w) {
    if (w < wave) base += wave_tot[w];
    nk += wave_tot[w];
  }
#pragma unroll
  for (int j = 0; j < A_PER; ++j) {
    if (keep & (1u << j)) {
      const int t = tid * per + j;
      ka2[base] = ka[t];
      kb2[base] = kb[t];
      full[ra[ka[t]]] = (int)rb[kb[t]];
      ++base;
    }
  }
  __syncthreads();
  for (int r = tid; r < Na; r += AT) mp[r] = full[r];

  // ---- the two full searches ----
  double rta[12], rtb[12];
  const double tm_a = block_search(make_pairs(c, ka2, kb2, nk, (double)La), tm_d0(La), 1, rta, part);
  const double tm_b = block_search(make_pairs(c, ka2, kb2, nk, (double)Lb), tm_d0(Lb), 1, rtb, part);
  if (wave == 0) {
    const TmPairs q = make_pairs(c, ka2, kb2, nk, 1.0);
    double sum = 0.0;
    for (int j = 0; j < q.nj; ++j) {
      const int t = lane + 64 * j;
      if (t >= nk) break;
      sum += tm_d2(q, rtb, t);
    }
    sum = fd::wave_sum(sum);
    if (lane == 0) {
      o[0] = (double)La;
      o[1] = (double)Lb;
      o[2] = (double)nk;
      o[3] = tm_a >= 0.0 ? tm_a : nan;
      o[4] = tm_b >= 0.0 ? tm_b : nan;
      o[5] = sqrt(sum / (double)nk);
      o[6] = tm_d0(La);
      o[7] = tm_d0(Lb);
      o[8] = (double)cls;
      o[9] = (double)num_dp;
      o[10] = (double)(k.n0 + k.n3);
      o[11] = best_s;
      for (int j = 12; j < 16; ++j) o[j] = 0.0;
      if (transform)
        for (int j = 0; j < 12; ++j) transform[p * 12 + j] = rtb[j];
    }
  }
}

}  // namespace

extern "C" int fd_tm_align(const float* A, long a_stride, int Na, const float* B, long b_stride, int Nb, const int* ia, const int* ib,
                           const float* mask_a, const float* mask_b, int P, int search_step, int max_dp, int parts, void* ws,
                           double* out, int* map, double* transform, void* stream) {
  FD_CHECK_ARG(P >= 0 && Na >= 0 && Nb >= 0, "fd_tm_align: negative size");
  FD_CHECK_ARG(Na <= A_MAX_N && Nb <= A_MAX_N, "fd_tm_align: Na and Nb must be at most 1024");
  FD_CHECK_ARG(search_step >= 1, "fd_tm_align: search_step must be at least 1");
  FD_CHECK_ARG(max_dp >= 0, "fd_tm_align: max_dp must not be negative");
  FD_CHECK_ARG(parts >= 1, "fd_tm_align: parts must be at least 1");
  FD_CHECK_ARG((ia == nullptr) == (ib == nullptr), "fd_tm_align: ia and ib are given together or not at all");
  if (P == 0 || Na == 0 || Nb == 0) return FD_OK;
  FD_CHECK_ARG(a_stride >= 3 && b_stride >= 3, "fd_tm_align: a point stride must be at least 3 floats");
  FD_CHECK_ARG((long)P * parts < (1L << 22), "fd_tm_align: P * parts must be below 2^22");
  FD_CHECK_ARG(ws != nullptr, "fd_tm_align: null workspace (FD_TM_ALIGN_WS_BYTES)");
  FD_CHECK_ARG(out != nullptr && map != nullptr, "fd_tm_align: null out or map");
  FD_CHECK_ARG(A && B, "fd_tm_align: null operand");
  FD_CHECK_ARG((((uintptr_t)out) & 7u) == 0 && (((uintptr_t)transform) & 7u) == 0 && (((uintptr_t)ws) & 7u) == 0,
               "fd_tm_align: ws, out and transform must be 8-byte aligned");
  // the workspace, in the order of FD_TM_ALIGN_WS_BYTES: wave partials | class records | DP bits | best alignments
  const long bits_stride = (long)Na * ((Nb + 31) / 32) * 2;
  double* ws_part = (double*)ws;
  double* ws_rec = ws_part + (long)P * parts * AW * A_PART;
  unsigned* ws_bits = (unsigned*)(ws_rec + (long)P * 4 * A_REC);
  unsigned short* ws_list = (unsigned short*)(ws_bits + (long)P * parts * AW * bits_stride);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(align_seed_kernel, dim3((unsigned)((long)P * parts)), dim3(AT), 0, st, A, a_stride, Na, B, b_stride, Nb, ia, ib,
                     mask_a, mask_b, parts, ws_part, ws_bits, bits_stride);
  FD_CHECK_LAUNCH("fd_tm_align (seed)");
  hipLaunchKernelGGL(align_refine_kernel, dim3((unsigned)((long)P * 4)), dim3(AT), 0, st, A, a_stride, Na, B, b_stride, Nb, ia, ib,
                     mask_a, mask_b, search_step, max_dp, parts, ws_part, ws_bits, bits_stride, ws_rec, ws_list);
  FD_CHECK_LAUNCH("fd_tm_align (refine)");
  hipLaunchKernelGGL(align_final_kernel, dim3((unsigned)P), dim3(AT), 0, st, A, a_stride, Na, B, b_stride, Nb, ia, ib, mask_a, mask_b,
                     ws_rec, ws_list, out, map, transform);
  FD_CHECK_LAUNCH("fd_tm_align (final)");
  return FD_OK;
}
