// fd_chains: training batches from a packed store of backbone atoms -- the device half of the reference's PdbDataset that the
// noising kernel (fd_forward_marginal_batch) does not cover: data/utils.py:436-445 parse_chain_feats, the backbone group of
// openfold/data/data_transforms.py atom37_to_frames and slots 0..2 of atom37_to_torsion_angles, the modeled_idx trim, seq_idx and
// the padding of data/pdb_data_loader.py:133-276.  include/fd_hip.h is the specification; this file says how the two launches
// are laid out.
//
// chain_windows_kernel   one block of 256 threads per chain.  Thread t looks at the residues t, t + 256, ... of its chain and keeps
//                        the smallest and largest present index and their number; a butterfly over the wave and four words of LDS
//                        give the block's.  Integers only.
// chain_batch_kernel     one block of 256 threads per batch entry.  Pass 1: the CA sum, the CA count and the smallest res_index of
//                        the window -- thread t adds its rows t, t + 256, ... in that order, the 64 partials of a wave meet in the
//                        xor butterfly (offsets 32, 16, .., 1: every lane ends with the same bits, since a + b == b + a), and the
//                        four wave sums are added as (s0 + s1) + (s2 + s3).  Pass 2: one row per thread at a time -- the residue and
//                        the one before it come from global memory again (12 floats and 4 bytes each; the second read is an L2 hit),
//                        frame, quaternion and three torsions in fp64 registers, one rounding to fp32, and the five atoms of
//                        fd_backbone5 (fd_atoms.h) from the ROUNDED frame and psi: bit for bit what fd_backbone_atoms gives on the
//                        rows this kernel wrote.
//
// All arithmetic after the fp32 loads is fp64.  No floating-point atomics.  A row depends on its chain's window only: results are
// bitwise independent of B, of the entry's place in the batch, of Npad and of the residues outside the window.
#include "fd_atoms.h"

namespace {

constexpr int CT = 256;                           // threads of a block
constexpr int CW = CT / 64;
constexpr double C_EPS = 1e-8;                    // under every square root (rigid_utils.py:1233-1275 from_3_points, eps = 1e-8)
constexpr double C_CENTRE_EPS = 1e-5;             // data/utils.py:440

__device__ __forceinline__ int imin(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ int imax(int a, int b) { return a > b ? a : b; }

__device__ __forceinline__ int wave_imin(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = imin(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ int wave_imax(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = imax(v, __shfl_xor(v, o));
  return v;
}

__global__ __launch_bounds__(CT) void chain_windows_kernel(const unsigned char* __restrict__ atom_mask,
                                                           const long* __restrict__ offsets, int* __restrict__ window) {
  __shared__ int s_first[CW], s_last[CW], s_cnt[CW];
  const int tid = (int)threadIdx.x, lane = fd::lane_id(), wave = fd::wave_id();
  const long c = (long)blockIdx.x;
  const long off = offsets[c];
  const long L = offsets[c + 1] - off;            // (a chain has fewer than 2^31 residues: fd_hip.h)
  int first = 0x7fffffff, last = -1, cnt = 0;
  for (long i = tid; i < L; i += CT) {
    const unsigned char* m = atom_mask + (off + i) * 4;
    if (m[0] != 0 && m[1] != 0 && m[2] != 0) {
      first = imin(first, (int)i);
      last = imax(last, (int)i);
      ++cnt;
    }
  }
  first = wave_imin(first);
  last = wave_imax(last);
  cnt = fd::wave_sum(cnt);
  if (lane == 0) s_first[wave] = first, s_last[wave] = last, s_cnt[wave] = cnt;
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < CW; ++w) first = imin(first, s_first[w]), last = imax(last, s_last[w]), cnt += s_cnt[w];
    window[c * 3 + 0] = cnt == 0 ? 0 : first;
    window[c * 3 + 1] = last;
    window[c * 3 + 2] = cnt;
  }
}

// the four atoms of one residue, centred and masked: (p - c) where the atom is present, the origin where it is not (whatever
// its coordinates hold).  Returns the mask bits (bit a: atom a present).
__device__ __forceinline__ int load_residue(const float* __restrict__ atoms, const unsigned char* __restrict__ atom_mask, long r,
                                            const double ctr[3], double p[4][3]) {
  const float* a = atoms + r * 12;
  const unsigned char* m = atom_mask + r * 4;
  int bits = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const bool on = m[k] != 0;
    bits |= on ? 1 << k : 0;
#pragma unroll
    for (int d = 0; d < 3; ++d) p[k][d] = on ? (double)a[3 * k + d] - ctr[d] : 0.0;
  }
  return bits;
}

__device__ __forceinline__ double dot3(const double a[3], const double b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// e0 = unit(q - p0), e1 = unit(v - e0 (e0 . v)) with v = r - q, e2 = e0 x e1: from_3_points(p_neg_x_axis = p0, origin = q,
// p_xy_plane = r) of the reference (rigid_utils.py:1233-1275), eps under both roots
__device__ __forceinline__ void gram_schmidt(const double p0[3], const double q[3], const double r[3], double e0[3], double e1[3],
                                             double e2[3]) {
  double v[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) e0[d] = q[d] - p0[d], v[d] = r[d] - q[d];
  const double n0 = sqrt(dot3(e0, e0) + C_EPS);
#pragma unroll
  for (int d = 0; d < 3; ++d) e0[d] = e0[d] / n0;
  const double dt = dot3(e0, v);
#pragma unroll
  for (int d = 0; d < 3; ++d) e1[d] = v[d] - e0[d] * dt;
  const double n1 = sqrt(dot3(e1, e1) + C_EPS);
#pragma unroll
  for (int d = 0; d < 3; ++d) e1[d] = e1[d] / n1;
  e2[0] = e0[1] * e1[2] - e0[2] * e1[1];
  e2[1] = e0[2] * e1[0] - e0[0] * e1[2];
  e2[2] = e0[0] * e1[1] - e0[1] * e1[0];
}

// (sin, cos) of the torsion of the atoms a, b, c, d (atom37_to_torsion_angles, data_transforms.py:1037-1061)
__device__ __forceinline__ void torsion(const double a[3], const double b[3], const double c[3], const double d[3], double sign,
                                        float* out) {
  double e0[3], e1[3], e2[3], w[3];
  gram_schmidt(b, c, a, e0, e1, e2);
#pragma unroll
  for (int k = 0; k < 3; ++k) w[k] = d[k] - c[k];
  const double ry = dot3(e1, w), rz = dot3(e2, w);
  const double den = sqrt((rz * rz + ry * ry) + C_EPS);
  out[0] = (float)(sign * (rz / den));
  out[1] = (float)(sign * (ry / den));
}

__global__ __launch_bounds__(CT) void chain_batch_kernel(const float* __restrict__ atoms, const unsigned char* __restrict__ atom_mask,
                                                         const int* __restrict__ res_index, const long* __restrict__ offsets,
                                                         const int* __restrict__ window, const int* __restrict__ ids, int Npad,
                                                         AtomConst ac, float* __restrict__ rigids, float* __restrict__ torsions,
                                                         float* __restrict__ res_mask, long* __restrict__ seq_idx,
                                                         float* __restrict__ gt_bb) {
  __shared__ double s_sum[3][CW];
  __shared__ int s_cnt[CW], s_min[CW];
  const int tid = (int)threadIdx.x, lane = fd::lane_id(), wave = fd::wave_id();
  const long b = (long)blockIdx.x;
  const int c = ids[b];
  long off = 0;
  int first = 0, len = 0;
  if (c >= 0) {                                   // (the host checked ids against the store and the windows against Npad;
    off = offsets[c];                             //  what follows only keeps a wrong table from reaching past a buffer)
    const long L = offsets[c + 1] - off;
    first = window[3 * c];
    const int last = window[3 * c + 1];
    if (first >= 0 && last >= first && (long)last < L) len = imin(last - first + 1, Npad);
  }
  const long r0 = off + first;                    // residue of row 0

  // ---- pass 1: centre and smallest residue number of the window ----
  double sx = 0.0, sy = 0.0, sz = 0.0;
  int cnt = 0, lo = 0x7fffffff;
  for (int i = tid; i < len; i += CT) {
    const long r = r0 + i;
    if (atom_mask[r * 4 + 1] != 0) {
      sx += (double)atoms[r * 12 + 3], sy += (double)atoms[r * 12 + 4], sz += (double)atoms[r * 12 + 5];
      ++cnt;
    }
    lo = imin(lo, res_index[r]);
  }
  sx = fd::wave_sum(sx), sy = fd::wave_sum(sy), sz = fd::wave_sum(sz);
  cnt = fd::wave_sum(cnt);
  lo = wave_imin(lo);
  if (lane == 0) s_sum[0][wave] = sx, s_sum[1][wave] = sy, s_sum[2][wave] = sz, s_cnt[wave] = cnt, s_min[wave] = lo;
  __syncthreads();
  static_assert(CW == 4, "the combine below is written for four waves");
  const double n_ca = (double)((s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3])) + C_CENTRE_EPS;
  double ctr[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) ctr[d] = ((s_sum[d][0] + s_sum[d][1]) + (s_sum[d][2] + s_sum[d][3])) / n_ca;
  const long idx0 = (long)imin(imin(s_min[0], s_min[1]), imin(s_min[2], s_min[3]));

  // ---- pass 2: one row per thread at a time ----
  for (int i = tid; i < Npad; i += CT) {
    const long o = b * Npad + i;
    float q7[7] = {1.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float tor[14];                                // slots 3..6 (the side chain's) stay zero
#pragma unroll
    for (int k = 0; k < 14; ++k) tor[k] = 0.f;
    float present = 0.f;
    long sidx = 0;
    if (i < len) {
      const long r = r0 + i;
      double cur[4][3], prev[4][3];               // N, CA, C, O
      const int bits = load_residue(atoms, atom_mask, r, ctr, cur);
      if (i > 0) {
        load_residue(atoms, atom_mask, r - 1, ctr, prev);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) prev[k][0] = prev[k][1] = prev[k][2] = 0.0;
      }
      torsion(prev[1], prev[2], cur[0], cur[1], 1.0, tor);          // pre-omega: CA-1, C-1, N, CA
      torsion(prev[2], cur[0], cur[1], cur[2], 1.0, tor + 2);       // phi: C-1, N, CA, C
      torsion(cur[0], cur[1], cur[2], cur[3], -1.0, tor + 4);       // psi: N, CA, C, O, negated
      sidx = (long)res_index[r] - idx0 + 1;
      if ((bits & 7) == 7) {
        present = 1.f;
        // x = unit(C - CA), y = unit((N - CA) - x (x . (N - CA))), z = x x y; R = [x y z] by columns
        double x[3], y[3], z[3];
        gram_schmidt(cur[1], cur[2], cur[0], x, y, z);
        const double R00 = x[0], R10 = x[1], R20 = x[2], R01 = y[0], R11 = y[1], R21 = y[2], R02 = z[0], R12 = z[1], R22 = z[2];
        const double t0 = ((1.0 + R00) + R11) + R22, t1 = ((1.0 + R00) - R11) - R22;
        const double t2 = ((1.0 - R00) + R11) - R22, t3 = ((1.0 - R00) - R11) + R22;
        double qw, qx, qy, qz;
        if (t0 >= t1 && t0 >= t2 && t0 >= t3) {
          qw = t0, qx = R21 - R12, qy = R02 - R20, qz = R10 - R01;
        } else if (t1 >= t2 && t1 >= t3) {
          qw = R21 - R12, qx = t1, qy = R01 + R10, qz = R02 + R20;
        } else if (t2 >= t3) {
          qw = R02 - R20, qx = R01 + R10, qy = t2, qz = R12 + R21;
        } else {
          qw = R10 - R01, qx = R02 + R20, qy = R12 + R21, qz = t3;
        }
        double nq = sqrt(((qw * qw + qx * qx) + qy * qy) + qz * qz);
        if (qw < 0.0) nq = -nq;
        q7[0] = (float)(qw / nq), q7[1] = (float)(qx / nq), q7[2] = (float)(qy / nq), q7[3] = (float)(qz / nq);
        q7[4] = (float)cur[1][0], q7[5] = (float)cur[1][1], q7[6] = (float)cur[1][2];
      }
    }
#pragma unroll
    for (int k = 0; k < 7; ++k) rigids[o * 7 + k] = q7[k];
#pragma unroll
    for (int k = 0; k < 14; ++k) torsions[o * 14 + k] = tor[k];
    res_mask[o] = present;
    seq_idx[o] = sidx;
    if (gt_bb) {
      float pos[5][3];
      fd_backbone5(q7, tor[4], tor[5], ac, pos);
#pragma unroll
      for (int n = 0; n < 5; ++n)
#pragma unroll
        for (int k = 0; k < 3; ++k) gt_bb[o * 15 + n * 3 + k] = pos[n][k];
    }
  }
}

}  // namespace

extern "C" int fd_chain_windows(const float* atoms, const unsigned char* atom_mask, const long* offsets, int C, int* window,
                                void* stream) {
  (void)atoms;                                    // (presence is the mask's; the coordinates are not read)
  FD_CHECK_ARG(C >= 0, "fd_chain_windows: negative size");
  if (C == 0) return FD_OK;
  FD_CHECK_ARG(atom_mask && offsets && window, "fd_chain_windows: null operand");
  FD_CHECK_ARG((((uintptr_t)offsets) & 7u) == 0 && (((uintptr_t)window) & 3u) == 0, "fd_chain_windows: misaligned operand");
  FD_CHECK_ARG(C < (1 << 24), "fd_chain_windows: C must be below 2^24 (blocks in one grid)");
  hipLaunchKernelGGL(chain_windows_kernel, dim3((unsigned)C), dim3(CT), 0, (hipStream_t)stream, atom_mask, offsets, window);
  FD_CHECK_LAUNCH("fd_chain_windows");
  return FD_OK;
}

extern "C" int fd_chain_batch(const float* atoms, const unsigned char* atom_mask, const int* res_index, const long* offsets,
                              const int* window, const int* ids, int B, int Npad, const FdHeadConst* c, float* rigids_0,
                              float* torsions, float* res_mask, long* seq_idx, float* gt_bb, void* stream) {
  FD_CHECK_ARG(B >= 0 && Npad >= 0, "fd_chain_batch: negative size");
  if (B == 0 || Npad == 0) return FD_OK;
  FD_CHECK_ARG(atoms && atom_mask && res_index && offsets && window && ids, "fd_chain_batch: null store operand");
  FD_CHECK_ARG(rigids_0 && torsions && res_mask && seq_idx, "fd_chain_batch: null output");
  FD_CHECK_ARG(gt_bb == nullptr || c != nullptr, "fd_chain_batch: gt_bb needs the head constants");
  FD_CHECK_ARG((((uintptr_t)atoms) & 3u) == 0 && (((uintptr_t)res_index) & 3u) == 0 && (((uintptr_t)offsets) & 7u) == 0 &&
                   (((uintptr_t)window) & 3u) == 0 && (((uintptr_t)ids) & 3u) == 0 && (((uintptr_t)rigids_0) & 3u) == 0 &&
                   (((uintptr_t)torsions) & 3u) == 0 && (((uintptr_t)res_mask) & 3u) == 0 && (((uintptr_t)seq_idx) & 7u) == 0 &&
                   (((uintptr_t)gt_bb) & 3u) == 0,
               "fd_chain_batch: misaligned operand");
  FD_CHECK_ARG(B < (1 << 24), "fd_chain_batch: B must be below 2^24 (blocks in one grid)");
  AtomConst ac = {};
  if (c) ac = fd_atom_const(c);
  hipLaunchKernelGGL(chain_batch_kernel, dim3((unsigned)B), dim3(CT), 0, (hipStream_t)stream, atoms, atom_mask, res_index, offsets,
                     window, ids, Npad, ac, rigids_0, torsions, res_mask, seq_idx, gt_bb);
  FD_CHECK_LAUNCH("fd_chain_batch");
  return FD_OK;
}
