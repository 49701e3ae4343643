// The superposition search shared by fd_tm_search (fd_metrics.hip) and fd_tm_align (fd_tm_align.hip): Horn's quaternion
// superposition in fp64 and the per-seed procedure of the TM-score program, as include/fd_hip.h specifies them, on a list of
// aligned pairs.  Everything here is WAVE-level: lanes stride over the pairs, a selection is a per-lane bit mask (bit j of a
// lane stands for pair lane + 64 j, so at most 2048 pairs), every sum is the lane's run in index order followed by the butterfly,
// whose result is the same bits in all 64 lanes -- so the eigenproblem, solved redundantly by every lane, is wave-uniform
// without a broadcast, and the arithmetic of a seed does not depend on which wave runs it.
//
// The pair list is a template parameter Q with L (pairs), nj = ceil(L / 64), lane, norm() (what the sum of a score is divided
// by) and the accessors AX(k) .. BZ(k) of pair k: TmPts reads six compacted arrays directly (pair k = position k of both sets:
// fd_tm_search, lnorm = L), TmPairs reads two chains through two index lists (fd_tm_align).
#pragma once
#include "fd_common.h"

namespace fdtm {
namespace {                                       // internal linkage: every translation unit inlines its own copy

constexpr int TM_MAX_WIDEN = 4096;                // cutoff increments of 0.5 A before a selection of < 3 positions is accepted

struct TmPts {
  const float *ax, *ay, *az, *bx, *by, *bz;       // the compacted counting positions, in LDS
  int L, nj, lane;
  __device__ __forceinline__ double norm() const { return (double)L; }
  __device__ __forceinline__ float AX(int k) const { return ax[k]; }
  __device__ __forceinline__ float AY(int k) const { return ay[k]; }
  __device__ __forceinline__ float AZ(int k) const { return az[k]; }
  __device__ __forceinline__ float BX(int k) const { return bx[k]; }
  __device__ __forceinline__ float BY(int k) const { return by[k]; }
  __device__ __forceinline__ float BZ(int k) const { return bz[k]; }
};

struct TmPairs {
  const float *ax, *ay, *az, *bx, *by, *bz;       // two compacted chains, in LDS
  const unsigned short *ka, *kb;                  // pair k = (a[ka[k]], b[kb[k]])
  int L, nj, lane;
  double lnorm;
  __device__ __forceinline__ double norm() const { return lnorm; }
  __device__ __forceinline__ float AX(int k) const { return ax[ka[k]]; }
  __device__ __forceinline__ float AY(int k) const { return ay[ka[k]]; }
  __device__ __forceinline__ float AZ(int k) const { return az[ka[k]]; }
  __device__ __forceinline__ float BX(int k) const { return bx[kb[k]]; }
  __device__ __forceinline__ float BY(int k) const { return by[kb[k]]; }
  __device__ __forceinline__ float BZ(int k) const { return bz[kb[k]]; }
};

// the at most seven fragment lengths L, L/2, L/4, ... (> 4), 4 and the number of starts 0, step, 2 step, ... <= L - len of each.
// Slot i < 6 holds L >> i while that is above 4 (the lengths only fall, so the first one at or below 4 ends them), slot 6 the
// closing 4; an unused slot has no starts and so takes no seed number.  Fixed slots: no dynamically indexed writes.
struct TmSeeds {
  int len[7], cnt[7], total;
};

__device__ __forceinline__ TmSeeds tm_seeds(int L, int seed_step) {
  TmSeeds s;
  s.total = 0;
#pragma unroll
  for (int i = 0; i < 7; ++i) {
    const int l = i < 6 ? L >> i : 4;
    const bool used = L >= 4 && (i == 6 || l > 4);
    s.len[i] = l;
    s.cnt[i] = used ? (L - l) / seed_step + 1 : 0;
    s.total += s.cnt[i];
  }
  return s;
}

// the fragment [start, stop) of seed number `seed`
__device__ __forceinline__ void tm_seed_range(const TmSeeds& sd, int seed, int seed_step, int& start, int& stop) {
  int rest = seed;
  bool found = false;
  start = 0;
  stop = 0;
#pragma unroll
  for (int i = 0; i < 7; ++i) {
    if (!found && rest < sd.cnt[i]) {
      found = true;
      start = rest * seed_step;
      stop = start + sd.len[i];
    } else if (!found) {
      rest -= sd.cnt[i];
    }
  }
}

__device__ __forceinline__ double tm_d0(int L) { return L > 21 ? 1.24 * cbrt((double)L - 15.0) - 1.8 : 0.5; }

// Largest eigenvector of the symmetric 4x4 matrix a (destroyed), by cyclic Jacobi rotations; q = (w, x, y, z), unit length.
__device__ void jacobi4_largest(double (&a)[4][4], double (&q)[4]) {
  double v[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) v[i][j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 50; ++sweep) {
    double off = 0.0;
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
      for (int r = p + 1; r < 4; ++r) off += fabs(a[p][r]);
    if (!(off > 0.0)) break;                      // (also leaves on NaN)
#pragma unroll
    for (int p = 0; p < 3; ++p) {
#pragma unroll
      for (int r = p + 1; r < 4; ++r) {
        const double apr = a[p][r];
        const double g = 100.0 * fabs(apr);
        if (sweep > 3 && fabs(a[p][p]) + g == fabs(a[p][p]) && fabs(a[r][r]) + g == fabs(a[r][r])) {
          a[p][r] = 0.0;
          a[r][p] = 0.0;
          continue;
        }
        if (apr == 0.0) continue;
        const double theta = (a[r][r] - a[p][p]) / (2.0 * apr);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
#pragma unroll
        for (int k = 0; k < 4; ++k) {             // columns p, r of a and of v
          const double akp = a[k][p], akr = a[k][r];
          a[k][p] = c * akp - sn * akr;
          a[k][r] = sn * akp + c * akr;
          const double vkp = v[k][p], vkr = v[k][r];
          v[k][p] = c * vkp - sn * vkr;
          v[k][r] = sn * vkp + c * vkr;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {             // rows p, r of a
          const double apk = a[p][k], ark = a[r][k];
          a[p][k] = c * apk - sn * ark;
          a[r][k] = sn * apk + c * ark;
        }
        a[p][r] = 0.0;
        a[r][p] = 0.0;
      }
    }
  }
  double best = a[0][0];
#pragma unroll
  for (int k = 0; k < 4; ++k) q[k] = v[k][0];
#pragma unroll
  for (int j = 1; j < 4; ++j) {
    if (a[j][j] > best) {
      best = a[j][j];
#pragma unroll
      for (int k = 0; k < 4; ++k) q[k] = v[k][j];
    }
  }
  const double nrm = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
#pragma unroll
  for (int k = 0; k < 4; ++k) q[k] /= nrm;
}

// Optimal proper rotation of the selected pairs (Horn's quaternion on the centred cross-covariance, as fd_aligned_rmsd):
// rt = R | t in every lane.
template <class Q>
__device__ void tm_superpose(const Q& q, unsigned sel, double (&rt)[12]) {
  const double n = (double)fd::wave_sum(__builtin_popcount(sel));
  double c[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int j = 0; j < q.nj; ++j) {
    if (!((sel >> j) & 1u)) continue;
    const int k = q.lane + 64 * j;
    c[0] += (double)q.AX(k);
    c[1] += (double)q.AY(k);
    c[2] += (double)q.AZ(k);
    c[3] += (double)q.BX(k);
    c[4] += (double)q.BY(k);
    c[5] += (double)q.BZ(k);
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) c[k] = fd::wave_sum(c[k]) / n;
  double s[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) s[k] = 0.0;
  for (int j = 0; j < q.nj; ++j) {
    if (!((sel >> j) & 1u)) continue;
    const int k = q.lane + 64 * j;
    const double ax = (double)q.AX(k) - c[0], ay = (double)q.AY(k) - c[1], az = (double)q.AZ(k) - c[2];
    const double bx = (double)q.BX(k) - c[3], by = (double)q.BY(k) - c[4], bz = (double)q.BZ(k) - c[5];
    s[0] += ax * bx;
    s[1] += ax * by;
    s[2] += ax * bz;
    s[3] += ay * bx;
    s[4] += ay * by;
    s[5] += ay * bz;
    s[6] += az * bx;
    s[7] += az * by;
    s[8] += az * bz;
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) s[k] = fd::wave_sum(s[k]);
  const double Sxx = s[0], Sxy = s[1], Sxz = s[2], Syx = s[3], Syy = s[4], Syz = s[5], Szx = s[6], Szy = s[7], Szz = s[8];
  double n4[4][4] = {{Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx},
                     {Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz},
                     {Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy},
                     {Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz}};
  double qn[4];
  jacobi4_largest(n4, qn);
  const double w = qn[0], x = qn[1], y = qn[2], z = qn[3];
  rt[0] = w * w + x * x - y * y - z * z;
  rt[1] = 2.0 * (x * y - w * z);
  rt[2] = 2.0 * (x * z + w * y);
  rt[3] = 2.0 * (x * y + w * z);
  rt[4] = w * w - x * x + y * y - z * z;
  rt[5] = 2.0 * (y * z - w * x);
  rt[6] = 2.0 * (x * z - w * y);
  rt[7] = 2.0 * (y * z + w * x);
  rt[8] = w * w - x * x - y * y + z * z;
  rt[9] = c[3] - (rt[0] * c[0] + rt[1] * c[1] + rt[2] * c[2]);
  rt[10] = c[4] - (rt[3] * c[0] + rt[4] * c[1] + rt[5] * c[2]);
  rt[11] = c[5] - (rt[6] * c[0] + rt[7] * c[1] + rt[8] * c[2]);
}

// d2 of pair k under rt, and the lane's selection bits for a squared cutoff
template <class Q>
__device__ __forceinline__ double tm_d2(const Q& q, const double (&rt)[12], int k) {
  const double ax = (double)q.AX(k), ay = (double)q.AY(k), az = (double)q.AZ(k);
  const double dx = (rt[0] * ax + rt[1] * ay + rt[2] * az + rt[9]) - (double)q.BX(k);
  const double dy = (rt[3] * ax + rt[4] * ay + rt[5] * az + rt[10]) - (double)q.BY(k);
  const double dz = (rt[6] * ax + rt[7] * ay + rt[8] * az + rt[11]) - (double)q.BZ(k);
  return dx * dx + dy * dy + dz * dz;
}

template <class Q>
__device__ __forceinline__ unsigned tm_select(const Q& q, const double (&rt)[12], double dc2) {
  unsigned ns = 0;
  for (int j = 0; j < q.nj; ++j) {
    const int k = q.lane + 64 * j;
    if (k >= q.L) break;
    if (tm_d2(q, rt, k) < dc2) ns |= 1u << j;
  }
  return ns;
}

// the lane's bits of all pairs
template <class Q>
__device__ __forceinline__ unsigned tm_all(const Q& q) {
  unsigned all = 0;
  for (int j = 0; j < q.nj; ++j)
    if (q.lane + 64 * j < q.L) all |= 1u << j;
  return all;
}

// score(R, t, dcut): (1/lnorm) sum 1 / (1 + d2 / d0^2) over all pairs; *sel (when asked for) = the pairs with d2 < dcut^2, dcut
// widened by 0.5 until at least three are selected.  The widening loop is wave-uniform and bounded (TM_MAX_WIDEN); a score that is
// not finite (a NaN or infinite coordinate among the pairs) can never become a candidate, so its selection is not widened at all.
template <class Q>
__device__ double tm_score_pass(const Q& q, const double (&rt)[12], double d0sq, double dcut, unsigned* sel) {
  double sum = 0.0;
  for (int j = 0; j < q.nj; ++j) {
    const int k = q.lane + 64 * j;
    if (k >= q.L) break;
    sum += 1.0 / (1.0 + tm_d2(q, rt, k) / d0sq);
  }
  sum = fd::wave_sum(sum) / q.norm();
  if (!sel) return sum;
  unsigned ns = tm_select(q, rt, dcut * dcut);
  int cnt = fd::wave_sum(__builtin_popcount(ns));
  const bool finite = sum - sum == 0.0;           // (false for NaN and for infinities; the same bits in every lane)
  for (int widen = 0; finite && cnt < 3 && widen < TM_MAX_WIDEN; ++widen) {
    dcut += 0.5;
    ns = tm_select(q, rt, dcut * dcut);
    cnt = fd::wave_sum(__builtin_popcount(ns));
  }
  *sel = ns;
  return sum;
}

// One seed, the fragment [start, stop) of the pair list: superpose it, score(d0s - 1), then up to max_iter times superpose the
// selection and score(d0s + 1) until the selection repeats.  Every call of score is a candidate for (best, best_seed, best_rt):
// strictly greater wins, so the earliest does on ties.  first0 receives the first score of seed 0; passes counts the calls of score.
template <class Q>
__device__ __forceinline__ void tm_run_seed(const Q& q, int start, int stop, int seed, double d0sq, double d0s, int max_iter, double& best,
                                            int& best_seed, double (&best_rt)[12], long& passes, double& first0) {
  double rt[12];
  const int lane = q.lane;
  unsigned sel = 0;
  for (int j = 0; j < q.nj; ++j) {
    const int k = lane + 64 * j;
    if (k >= start && k < stop) sel |= 1u << j;
  }
  tm_superpose(q, sel, rt);
  double s = tm_score_pass(q, rt, d0sq, d0s - 1.0, &sel);
  ++passes;
  if (seed == 0) first0 = s;
  bool settled = false;
  for (int it = 0;; ++it) {
    if (s > best) {                               // every call of score is a candidate; strictly greater: the earliest wins
      best = s;
      best_seed = seed;
#pragma unroll
      for (int k = 0; k < 12; ++k) best_rt[k] = rt[k];
    }
    if (settled || it >= max_iter) break;
    unsigned next;
    tm_superpose(q, sel, rt);
    s = tm_score_pass(q, rt, d0sq, d0s + 1.0, &next);
    ++passes;
    settled = fd::wave_sum(next == sel ? 0 : 1) == 0;          // "selection unchanged": in every lane of the wave
    sel = next;
  }
}

}  // namespace
}  // namespace fdtm
