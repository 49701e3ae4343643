// fd_backbone_metrics / fd_aligned_rmsd / fd_tm_search: the coordinate arithmetic of the reference's sample evaluation on the device
// (analysis/metrics.py:120-125 ca_ca_distance, :127-132 ca_ca_clashes, :71-73 calc_aligned_rmsd on
// data/utils.py:519-568 rigid_transform_3D), one launch each, the values left in HBM as fp64.
//
// fd_backbone_metrics  one block per backbone.  The present residues are compacted in index order (the reference's boolean
//                      indexing, metrics.py:94-95) by a block prefix scan of the mask; the compacted CA go to LDS as three fp32
//                      arrays together with the compacted -> original residue index.  (C and N "beside" the CA would take
//                      9 x 4096 floats = 144 KB at the largest N; the bond term reads C_i and N_{i+1} through the index from
//                      global memory instead, once.)  The pair loop gives row i to one thread, which walks j = i+1 .. n-1: the
//                      lanes of a wave read consecutive dwords of one array (or the same dword), so no LDS bank is asked twice.
//                      Rows i and n-1-i go to the same thread, which evens the triangle out to n-1 pairs per thread and trip.
// fd_aligned_rmsd      one block per pair: centroids, then the 3x3 cross-covariance, then one thread solves Horn's quaternion
//                      eigenproblem (largest eigenvector of a symmetric 4x4, cyclic Jacobi) for the optimal PROPER rotation --
//                      what rigid_transform_3D returns after its reflection fix -- then all threads take the residual distances.
// fd_tm_search        the TM-score of a given correspondence as the maximum over superpositions, by the seed-and-refine search
//                      of the TM-score program (include/fd_hip.h spells it out).  parts blocks per pair; each compacts the
//                      pair's counting positions into LDS once (six fp32 arrays, the prefix scan of fd_backbone_metrics), then
//                      ONE WAVE owns one seed at a time: lanes stride over the positions, the selection is a per-lane bit mask,
//                      and every lane solves the 4x4 eigenproblem redundantly from wave sums that are the same bits in all
//                      lanes.  Seeds take different numbers of refinements, so after the staging there is no block barrier,
//                      only wave collectives.  Each wave leaves one partial in a caller-provided workspace; a second launch,
//                      one wave per pair, takes the maximum (lowest seed on ties) and the integer sum of the pass counts.
//
// All arithmetic after the fp32 loads is fp64.  No floating-point atomics: every sum is a per-thread run in index order and a
// butterfly in the wave; the block-wide sums of the first two entry points then add the four wave results in wave order
// through LDS (fd_optim.hip::block_reduce3's pattern), the search keeps its sums inside the wave.  The results are bitwise
// reproducible for a given shape, the search's also whatever parts is.
#include "fd_common.h"
#include "fd_tm_core.h"
#include "../../include/fd_hip.h"

namespace {

using namespace fdtm;                            // jacobi4_largest and the superposition search (fd_tm_core.h)

constexpr int MT = 256;
constexpr int MW = MT / 64;
constexpr int M_MAX_N = 4096;
constexpr int M_PER = M_MAX_N / MT;               // residues per thread of the compaction pass

constexpr double CA_CA = 3.80209737096;           // openfold residue_constants.ca_ca
constexpr double CA_CA_TOL = 0.1;                 // ca_ca_distance(tol=0.1)
constexpr double CLASH_TOL = 1.5;                 // ca_ca_clashes(tol=1.5)
constexpr double C_N = 1.329;                     // openfold residue_constants.between_res_bond_length_c_n[0] (non-proline)
constexpr double C_N_TOL = 12.0 * 0.014;          // its standard deviation at the violation tolerance factor 12

// NS block-wide sums: on return every thread holds the totals.  `red` may be reused by the next call (the leading barrier).
template <int NS>
__device__ __forceinline__ void block_sums(double (&s)[NS], double (*red)[MW]) {
#pragma unroll
  for (int k = 0; k < NS; ++k) s[k] = fd::wave_sum(s[k]);
  const int lane = fd::lane_id(), wave = fd::wave_id();
  __syncthreads();
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < NS; ++k) red[k][wave] = s[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    double v = red[k][0];
    for (int w = 1; w < MW; ++w) v += red[k][w];
    s[k] = v;
  }
}

__device__ __forceinline__ double block_max(double v, double (*red)[MW]) {
  v = fd::wave_max(v);
  const int lane = fd::lane_id(), wave = fd::wave_id();
  __syncthreads();
  if (lane == 0) red[0][wave] = v;
  __syncthreads();
  v = red[0][0];
  for (int w = 1; w < MW; ++w) v = v > red[0][w] ? v : red[0][w];
  return v;
}

__device__ __forceinline__ double dist3(double ax, double ay, double az, double bx, double by, double bz) {
  const double dx = ax - bx, dy = ay - by, dz = az - bz;
  return sqrt(dx * dx + dy * dy + dz * dz);
}

__global__ __launch_bounds__(MT) void backbone_metrics_kernel(const float* __restrict__ atoms, long atom_stride,
                                                              const float* __restrict__ res_mask, int N,
                                                              double* __restrict__ out) {
  __shared__ float cx[M_MAX_N], cy[M_MAX_N], cz[M_MAX_N];
  __shared__ unsigned short ridx[M_MAX_N];
  __shared__ int wave_tot[MW];
  __shared__ double red[9][MW];
  const int tid = (int)threadIdx.x, lane = fd::lane_id(), wave = fd::wave_id();
  const long b = (long)blockIdx.x;
  const float* mask = res_mask + b * N;
  const float* bb = atoms + b * N * atom_stride;

  // ---- compaction: thread t owns the residues [t per, (t + 1) per) ----
  const int per = (N + MT - 1) / MT;
  const int r0 = tid * per;
  unsigned present = 0;                           // bit k: residue r0 + k is present
#pragma unroll
  for (int k = 0; k < M_PER; ++k) {
    const int r = r0 + k;
    if (k < per && r < N && mask[r] != 0.f) present |= 1u << k;
  }
  const int cnt = __builtin_popcount(present);
  int incl = cnt;                                 // inclusive scan within the wave, then the wave totals in wave order
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl(incl, lane >= o ? lane - o : lane);
    if (lane >= o) incl += u;
  }
  if (lane == 63) wave_tot[wave] = incl;
  __syncthreads();
  int base = incl - cnt, n = 0;
  for (int w = 0; w < MW; ++w) {
    if (w < wave) base += wave_tot[w];
    n += wave_tot[w];
  }
#pragma unroll
  for (int k = 0; k < M_PER; ++k) {
    if (present & (1u << k)) {
      const int r = r0 + k;
      const float* ca = bb + (long)r * atom_stride + 3;
      cx[base] = ca[0];
      cy[base] = ca[1];
      cz[base] = ca[2];
      ridx[base] = (unsigned short)r;
      ++base;
    }
  }
  __syncthreads();

  // ---- consecutive compacted pairs (CA-CA and C_i - N_{i+1}) and the CA sum ----
  double s[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) s[k] = 0.0;
  double mx = 0.0;
  for (int i = tid; i < n; i += MT) {
    const double ax = (double)cx[i], ay = (double)cy[i], az = (double)cz[i];
    s[4] += ax;
    s[5] += ay;
    s[6] += az;
    if (i + 1 < n) {
      const double d = dist3(ax, ay, az, (double)cx[i + 1], (double)cy[i + 1], (double)cz[i + 1]);
      s[0] += fabs(d - CA_CA);
      s[1] += d < CA_CA + CA_CA_TOL ? 1.0 : 0.0;
      mx = d > mx ? d : mx;
      const float* c = bb + (long)ridx[i] * atom_stride + 6;
      const float* nn = bb + (long)ridx[i + 1] * atom_stride;
      const double e = fabs(dist3((double)c[0], (double)c[1], (double)c[2], (double)nn[0], (double)nn[1], (double)nn[2]) - C_N);
      s[2] += e;
      s[3] += e <= C_N_TOL ? 1.0 : 0.0;
    }
  }

  // ---- all pairs i < j: rows k and n-1-k on one thread ----
  int clashes = 0, positive = 0;
  const int half = (n + 1) / 2;
  for (int k = tid; k < half; k += MT) {
    for (int pass = 0; pass < 2; ++pass) {
      const int i = pass == 0 ? k : n - 1 - k;
      if (pass == 1 && i == k) break;             // (the middle row of an odd n)
      const double ax = (double)cx[i], ay = (double)cy[i], az = (double)cz[i];
#pragma unroll 4
      for (int j = i + 1; j < n; ++j) {
        // on the squared distance: 0 < D < 1.5 iff 0 < D^2 < 2.25 (1.5^2 is exact and sqrt is monotone and correctly rounded;
        // a difference of two distinct fp32 values cannot underflow when squared in fp64)
        const double dx = ax - (double)cx[j], dy = ay - (double)cy[j], dz = az - (double)cz[j];
        const double d2 = dx * dx + dy * dy + dz * dz;
        positive += d2 > 0.0 ? 1 : 0;
        clashes += (d2 > 0.0 && d2 < CLASH_TOL * CLASH_TOL) ? 1 : 0;
      }
    }
  }
  s[7] = (double)clashes;
  s[8] = (double)positive;
  block_sums<9>(s, red);
  mx = block_max(mx, red);

  // ---- radius of gyration about the CA centroid ----
  const double dn = (double)n;
  const double mxc = s[4] / dn, myc = s[5] / dn, mzc = s[6] / dn;
  double g[1] = {0.0};
  for (int i = tid; i < n; i += MT) {
    const double dx = (double)cx[i] - mxc, dy = (double)cy[i] - myc, dz = (double)cz[i] - mzc;
    g[0] += dx * dx + dy * dy + dz * dz;
  }
  block_sums<1>(g, red);

  if (tid == 0) {
    const double np = n > 1 ? (double)(n - 1) : 0.0;    // a mean over no pairs is 0 / 0 = NaN, as np.mean gives
    double* o = out + b * 12;
    o[0] = dn;
    o[1] = s[0] / np;
    o[2] = s[1] / np;
    o[3] = s[7];
    o[4] = s[7] / s[8];
    o[5] = sqrt(g[0] / dn);
    o[6] = s[2] / np;
    o[7] = s[3] / np;
    o[8] = mx;
    o[9] = 0.0;
    o[10] = 0.0;
    o[11] = 0.0;
  }
}

__global__ __launch_bounds__(MT) void aligned_rmsd_kernel(const float* __restrict__ A, long a_stride, const float* __restrict__ B,
                                                          long b_stride, const int* __restrict__ ia, const int* __restrict__ ib,
                                                          const float* __restrict__ mask, int N, double* __restrict__ out,
                                                          double* __restrict__ transform) {
  __shared__ double red[9][MW];
  __shared__ double rt[12];
  const int tid = (int)threadIdx.x;
  const long p = (long)blockIdx.x;
  const long sa = ia ? (long)ia[p] : p, sb = ib ? (long)ib[p] : p;
  const float* a = A + sa * N * a_stride;
  const float* bq = B + sb * N * b_stride;
  const float* ma = mask ? mask + sa * N : nullptr;
  const float* mb = mask ? mask + sb * N : nullptr;
#define FD_COUNTS(k) (!mask || (ma[k] != 0.f && mb[k] != 0.f))

  // ---- count and centroids ----
  double s[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) s[k] = 0.0;
  for (int k = tid; k < N; k += MT) {
    if (!FD_COUNTS(k)) continue;
    const float* pa = a + (long)k * a_stride;
    const float* pb = bq + (long)k * b_stride;
    s[0] += 1.0;
    s[1] += (double)pa[0];
    s[2] += (double)pa[1];
    s[3] += (double)pa[2];
    s[4] += (double)pb[0];
    s[5] += (double)pb[1];
    s[6] += (double)pb[2];
  }
  block_sums<9>(s, red);
  const double L = s[0];
  const double cax = s[1] / L, cay = s[2] / L, caz = s[3] / L, cbx = s[4] / L, cby = s[5] / L, cbz = s[6] / L;

  // ---- cross-covariance H = sum (a - ca)(b - cb)^T (rigid_transform_3D's H = Am @ Bm.T) ----
#pragma unroll
  for (int k = 0; k < 9; ++k) s[k] = 0.0;
  for (int k = tid; k < N; k += MT) {
    if (!FD_COUNTS(k)) continue;
    const float* pa = a + (long)k * a_stride;
    const float* pb = bq + (long)k * b_stride;
    const double ax = (double)pa[0] - cax, ay = (double)pa[1] - cay, az = (double)pa[2] - caz;
    const double bx = (double)pb[0] - cbx, by = (double)pb[1] - cby, bz = (double)pb[2] - cbz;
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
  block_sums<9>(s, red);

  double reflection = 0.0;
  if (tid == 0) {
    const double Sxx = s[0], Sxy = s[1], Sxz = s[2], Syx = s[3], Syy = s[4], Syz = s[5], Szx = s[6], Szy = s[7], Szz = s[8];
    const double det = Sxx * (Syy * Szz - Syz * Szy) - Sxy * (Syx * Szz - Syz * Szx) + Sxz * (Syx * Szy - Syy * Szx);
    reflection = det < 0.0 ? 1.0 : 0.0;
    // Horn (1987), eq. of the matrix N: its largest eigenvector is the unit quaternion of the rotation that maximises
    // sum b . (R a) over the proper rotations
    double n4[4][4] = {{Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx},
                       {Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz},
                       {Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy},
                       {Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz}};
    double q[4];
    jacobi4_largest(n4, q);
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    double R[9] = {w * w + x * x - y * y - z * z, 2.0 * (x * y - w * z),         2.0 * (x * z + w * y),
                   2.0 * (x * y + w * z),         w * w - x * x + y * y - z * z, 2.0 * (y * z - w * x),
                   2.0 * (x * z - w * y),         2.0 * (y * z + w * x),         w * w - x * x - y * y + z * z};
#pragma unroll
    for (int k = 0; k < 9; ++k) rt[k] = R[k];
    rt[9] = cbx - (R[0] * cax + R[1] * cay + R[2] * caz);       // t = -R ca + cb
    rt[10] = cby - (R[3] * cax + R[4] * cay + R[5] * caz);
    rt[11] = cbz - (R[6] * cax + R[7] * cay + R[8] * caz);
  }
  __syncthreads();
  double R[9], t[3];
#pragma unroll
  for (int k = 0; k < 9; ++k) R[k] = rt[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) t[k] = rt[9 + k];

  // ---- residuals of aligned = R a + t against b ----
  const double d0 = L > 21.0 ? 1.24 * cbrt(L - 15.0) - 1.8 : 0.5;
  double r3[3] = {0.0, 0.0, 0.0};
  double mx = 0.0;
  for (int k = tid; k < N; k += MT) {
    if (!FD_COUNTS(k)) continue;
    const float* pa = a + (long)k * a_stride;
    const float* pb = bq + (long)k * b_stride;
    const double ax = (double)pa[0], ay = (double)pa[1], az = (double)pa[2];
    const double dx = (R[0] * ax + R[1] * ay + R[2] * az + t[0]) - (double)pb[0];
    const double dy = (R[3] * ax + R[4] * ay + R[5] * az + t[1]) - (double)pb[1];
    const double dz = (R[6] * ax + R[7] * ay + R[8] * az + t[2]) - (double)pb[2];
    const double d2 = dx * dx + dy * dy + dz * dz;
    const double d = sqrt(d2);
    const double u = d / d0;
    r3[0] += d;
    r3[1] += d2;
    r3[2] += 1.0 / (1.0 + u * u);
    mx = d > mx ? d : mx;
  }
#undef FD_COUNTS
  block_sums<3>(r3, red);
  mx = block_max(mx, red);
  if (tid == 0) {
    double* o = out + p * 8;
    o[0] = L;
    o[1] = r3[0] / L;                             // 0 / 0 = NaN for an empty pair
    o[2] = sqrt(r3[1] / L);
    o[3] = r3[2] / L;
    o[4] = reflection;
    o[5] = L > 0.0 ? mx : r3[0] / L;
    o[6] = 0.0;
    o[7] = 0.0;
    if (transform) {
#pragma unroll
      for (int k = 0; k < 12; ++k) transform[p * 12 + k] = rt[k];
    }
  }
}

// ---- fd_tm_search: the TM-score of a fixed correspondence by superposition search -----------------------------------------------
constexpr int TM_MAX_N = 2048;                    // 6 fp32 arrays of 2048 = 48 KB static LDS
constexpr int TM_PART = 16;                       // doubles per wave partial: score, seed, R | t, passes, first score of seed 0

// Block c of pair p (blockIdx.x = p parts + c) stages the pair's counting positions once; then wave w owns the seeds
// 4 c + w, + 4 parts, ...  No block barrier after the staging: the seeds take different numbers of refinements.
template <int MAXN>
__global__ __launch_bounds__(MT, 3) void tm_search_kernel(const float* __restrict__ A, long a_stride, const float* __restrict__ B,
                                                       long b_stride, const int* __restrict__ ia, const int* __restrict__ ib,
                                                       const float* __restrict__ mask, int N, int seed_step, int max_iter, int parts,
                                                       double* __restrict__ ws) {
  constexpr int PER = MAXN / MT;
  __shared__ float pax[MAXN], pay[MAXN], paz[MAXN], pbx[MAXN], pby[MAXN], pbz[MAXN];
  __shared__ int wave_tot[MW];
  const int tid = (int)threadIdx.x, lane = fd::lane_id(), wave = fd::wave_id();
  const long p = (long)(blockIdx.x / (unsigned)parts);
  const int c = (int)(blockIdx.x % (unsigned)parts);
  const long sa = ia ? (long)ia[p] : p, sb = ib ? (long)ib[p] : p;
  const float* a = A + sa * N * a_stride;
  const float* bq = B + sb * N * b_stride;
  const float* ma = mask ? mask + sa * N : nullptr;
  const float* mb = mask ? mask + sb * N : nullptr;

  // ---- staging: thread t owns the positions [t per, (t + 1) per); backbone_metrics_kernel's prefix scan ----
  const int per = (N + MT - 1) / MT;
  const int r0 = tid * per;
  unsigned present = 0;
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int r = r0 + k;
    if (k < per && r < N && (!mask || (ma[r] != 0.f && mb[r] != 0.f))) present |= 1u << k;
  }
  const int cnt = __builtin_popcount(present);
  int incl = cnt;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl(incl, lane >= o ? lane - o : lane);
    if (lane >= o) incl += u;
  }
  if (lane == 63) wave_tot[wave] = incl;
  __syncthreads();
  int base = incl - cnt, L = 0;
  for (int w = 0; w < MW; ++w) {
    if (w < wave) base += wave_tot[w];
    L += wave_tot[w];
  }
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    if (present & (1u << k)) {
      const float* pa = a + (long)(r0 + k) * a_stride;
      const float* pb = bq + (long)(r0 + k) * b_stride;
      pax[base] = pa[0];
      pay[base] = pa[1];
      paz[base] = pa[2];
      pbx[base] = pb[0];
      pby[base] = pb[1];
      pbz[base] = pb[2];
      ++base;
    }
  }
  __syncthreads();

  // ---- the seeds of this wave (everything below is wave-uniform; only wave collectives) ----
  TmPts q;
  q.ax = pax, q.ay = pay, q.az = paz, q.bx = pbx, q.by = pby, q.bz = pbz;
  q.L = L;
  q.nj = (L + 63) >> 6;
  q.lane = lane;
  const double d0 = tm_d0(L), d0sq = d0 * d0;
  const double d0s = d0 < 4.5 ? 4.5 : (d0 > 8.0 ? 8.0 : d0);
  double best = -1.0, best_rt[12], first0 = 0.0, rt[12];
  int best_seed = -1;
  long passes = 0;
#pragma unroll
  for (int k = 0; k < 12; ++k) best_rt[k] = 0.0;

  if (L < 4) {
    // no search: the formula under the whole-set superposition (NaN for an empty pair), by the first wave of the first part
    if (c == 0 && wave == 0) {
      tm_superpose(q, tm_all(q), best_rt);
      best = tm_score_pass(q, best_rt, d0sq, 0.0, nullptr);
      first0 = best;
    }
  } else {
    const TmSeeds sd = tm_seeds(L, seed_step);
    for (int seed = 4 * c + wave; seed < sd.total; seed += 4 * parts) {
      int start, stop;
      tm_seed_range(sd, seed, seed_step, start, stop);
      // fdtm::tm_run_seed, spelt out: called as that helper the kernel no longer fits the 168 VGPRs of its three-waves bound
      // (21 spilled; measured with -Rpass-analysis=kernel-resource-usage), spelt out it takes 164 as before
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
        if (s > best) {
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
        settled = fd::wave_sum(next == sel ? 0 : 1) == 0;
        sel = next;
      }
    }
  }
  if (lane == 0) {
    double* o = ws + (((long)blockIdx.x) * MW + wave) * TM_PART;
    o[0] = best;
    o[1] = (double)best_seed;
#pragma unroll
    for (int k = 0; k < 12; ++k) o[2 + k] = best_rt[k];
    o[14] = (double)passes;
    o[15] = first0;
  }
}

// One wave per pair: count L again, then the partials in a fixed order -- maximum score, lowest seed on ties; integer sum of passes.
__global__ __launch_bounds__(64) void tm_reduce_kernel(const double* __restrict__ ws, int parts, const int* __restrict__ ia,
                                                       const int* __restrict__ ib, const float* __restrict__ mask, int N,
                                                       int seed_step, double* __restrict__ out, double* __restrict__ transform) {
  const int lane = fd::lane_id();
  const long p = (long)blockIdx.x;
  int L = N;
  if (mask) {
    const long sa = ia ? (long)ia[p] : p, sb = ib ? (long)ib[p] : p;
    const float* ma = mask + sa * N;
    const float* mb = mask + sb * N;
    int n = 0;
    for (int k = lane; k < N; k += 64) n += (ma[k] != 0.f && mb[k] != 0.f) ? 1 : 0;
    L = fd::wave_sum(n);
  }
  const double* w = ws + p * parts * MW * TM_PART;
  const int np = parts * MW;
  // the lane's own partials in index order, then across the wave: the best score, then the lowest seed that has it
  double best = -1.0, seed = -1.0, passes = 0.0;
  int at = 0;
  for (int k = lane; k < np; k += 64) {
    const double s = w[(long)k * TM_PART], sd = w[(long)k * TM_PART + 1];
    passes += w[(long)k * TM_PART + 14];
    if (s > best || (s == best && sd < seed)) best = s, seed = sd, at = k;
  }
  passes = fd::wave_sum(passes);                  // (integers below 2^53: exact in any order)
  const double top = fd::wave_max(best);
  const double low = -fd::wave_max(best == top ? -seed : -4.0e9);
  const TmSeeds sd = tm_seeds(L, seed_step);
  const bool searched = L >= 4;
  // each seed ran on exactly one wave, so one lane holds (top, low) when any candidate was finite; without a search (L < 4)
  // the whole-set partial is the first one
  const bool found = searched && top >= 0.0;
  const bool mine = searched ? (found ? (best == top && seed == low) : lane == 0) : lane == 0;
  if (mine) {
    const double* b = w + (long)(found ? at : 0) * TM_PART;
    const double nan = __builtin_nan("");
    double* o = out + p * 8;
    o[0] = (double)L;
    o[1] = searched ? (found ? top : nan) : w[0];
    o[2] = w[15];
    o[3] = found ? low : -1.0;
    o[4] = (double)sd.total;
    o[5] = tm_d0(L);
    o[6] = passes;
    o[7] = 0.0;
    if (transform) {
#pragma unroll
      for (int k = 0; k < 12; ++k) transform[p * 12 + k] = b[2 + k];
    }
  }
}

}  // namespace

extern "C" int fd_backbone_metrics(const float* atoms, long atom_stride, const float* res_mask, int B, int N, double* out,
                                   void* stream) {
  FD_CHECK_ARG(B >= 0 && N >= 0, "fd_backbone_metrics: negative size");
  FD_CHECK_ARG(atom_stride >= 15, "fd_backbone_metrics: atom_stride must be at least 15 floats (N, CA, C, CB, O)");
  FD_CHECK_ARG(N <= M_MAX_N, "fd_backbone_metrics: N must be at most 4096");
  if (B == 0 || N == 0) return FD_OK;
  FD_CHECK_ARG(atoms && res_mask && out, "fd_backbone_metrics: null operand");
  FD_CHECK_ARG((((uintptr_t)out) & 7u) == 0, "fd_backbone_metrics: out must be 8-byte aligned");
  hipLaunchKernelGGL(backbone_metrics_kernel, dim3(B), dim3(MT), 0, (hipStream_t)stream, atoms, atom_stride, res_mask, N, out);
  FD_CHECK_LAUNCH("fd_backbone_metrics");
  return FD_OK;
}

extern "C" int fd_aligned_rmsd(const float* A, long a_stride, const float* B, long b_stride, const int* ia, const int* ib,
                               const float* mask, int P, int N, double* out, double* transform, void* stream) {
  FD_CHECK_ARG(P >= 0 && N >= 0, "fd_aligned_rmsd: negative size");
  FD_CHECK_ARG(a_stride >= 3 && b_stride >= 3, "fd_aligned_rmsd: a point stride must be at least 3 floats");
  FD_CHECK_ARG(N <= M_MAX_N, "fd_aligned_rmsd: N must be at most 4096");
  FD_CHECK_ARG((ia == nullptr) == (ib == nullptr), "fd_aligned_rmsd: ia and ib are given together or not at all");
  if (P == 0 || N == 0) return FD_OK;
  FD_CHECK_ARG(A && B && out, "fd_aligned_rmsd: null operand");
  FD_CHECK_ARG((((uintptr_t)out) & 7u) == 0 && (((uintptr_t)transform) & 7u) == 0,
               "fd_aligned_rmsd: out and transform must be 8-byte aligned");
  hipLaunchKernelGGL(aligned_rmsd_kernel, dim3(P), dim3(MT), 0, (hipStream_t)stream, A, a_stride, B, b_stride, ia, ib, mask, N,
                     out, transform);
  FD_CHECK_LAUNCH("fd_aligned_rmsd");
  return FD_OK;
}

extern "C" int fd_tm_search(const float* A, long a_stride, const float* B, long b_stride, const int* ia, const int* ib,
                            const float* mask, int P, int N, int seed_step, int max_iter, int parts, double* ws, double* out,
                            double* transform, void* stream) {
  FD_CHECK_ARG(P >= 0 && N >= 0, "fd_tm_search: negative size");
  FD_CHECK_ARG(a_stride >= 3 && b_stride >= 3, "fd_tm_search: a point stride must be at least 3 floats");
  FD_CHECK_ARG(N <= TM_MAX_N, "fd_tm_search: N must be at most 2048");
  FD_CHECK_ARG(seed_step >= 1, "fd_tm_search: seed_step must be at least 1");
  FD_CHECK_ARG(max_iter >= 0, "fd_tm_search: max_iter must not be negative");
  FD_CHECK_ARG(parts >= 1, "fd_tm_search: parts must be at least 1");
  FD_CHECK_ARG((ia == nullptr) == (ib == nullptr), "fd_tm_search: ia and ib are given together or not at all");
  if (P == 0 || N == 0) return FD_OK;
  FD_CHECK_ARG((long)P * parts < (1L << 24), "fd_tm_search: P * parts must be below 2^24 (blocks of 256 threads in one grid)");
  FD_CHECK_ARG(ws != nullptr, "fd_tm_search: null workspace (P * parts * 64 doubles)");
  FD_CHECK_ARG(A && B && out, "fd_tm_search: null operand");
  FD_CHECK_ARG((((uintptr_t)out) & 7u) == 0 && (((uintptr_t)transform) & 7u) == 0 && (((uintptr_t)ws) & 7u) == 0,
               "fd_tm_search: ws, out and transform must be 8-byte aligned");
  const dim3 grid((unsigned)((long)P * parts));
  // One instantiation.  The kernel is bounded to three waves per SIMD (164 VGPRs, no spill; the fp64 Jacobi sweep is what fills
  // them, and a bound of four spills), which is also what 48 KB of LDS per block admits on a 160 KB CU: a 12 KB instantiation for
  // N <= 512 could not raise the occupancy, so there is none.
  hipLaunchKernelGGL(tm_search_kernel<TM_MAX_N>, grid, dim3(MT), 0, (hipStream_t)stream, A, a_stride, B, b_stride, ia, ib, mask, N,
                     seed_step, max_iter, parts, ws);
  FD_CHECK_LAUNCH("fd_tm_search");
  hipLaunchKernelGGL(tm_reduce_kernel, dim3(P), dim3(64), 0, (hipStream_t)stream, ws, parts, ia, ib, mask, N, seed_step, out,
                     transform);
  FD_CHECK_LAUNCH("fd_tm_search (reduce)");
  return FD_OK;
}
