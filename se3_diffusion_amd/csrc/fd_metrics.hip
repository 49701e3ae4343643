// fd_backbone_metrics / fd_aligned_rmsd: the coordinate arithmetic of the reference's sample evaluation on the device
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
//
// All arithmetic after the fp32 loads is fp64.  No floating-point atomics: every sum is a per-thread run in index order, a
// butterfly in the wave, then the four wave results in wave order through LDS (fd_optim.hip::block_reduce3's pattern), so the
// results are bitwise reproducible for a given shape.
#include "fd_common.h"
#include "../../include/fd_hip.h"

namespace {

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
