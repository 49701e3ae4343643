// fd_violations: the reference's between-residue violation losses (openfold/utils/loss.py:712-868 between_residue_bond_loss,
// :871-1015 between_residue_clash_loss, :1272-1312 compute_violation_metrics, for an all-alanine chain) from the backbone atoms
// the sampler leaves in HBM.  include/fd_hip.h is the specification; this file says how the two launches are laid out.
//
// violations_kernel   grid over (tiles of 64 COMPACTED residues x backbones), 512 threads.  Every block compacts the present
//                     residues of its chain by fd_dssp_hbonds' prefix scan and stages all five atoms of all of them as fifteen
//                     structure-of-arrays fp32 arrays of 2048 (120 KB), a bounding radius per residue (the largest distance of
//                     one of its atoms from its CA, rounded up: 8 KB), res_index (8 KB) and the index map (4 KB): 140 KB of the
//                     160 KB of a CU.  That is one block per CU, and it costs nothing here: the grid has ceil(N / 64) B blocks,
//                     below the 256 CUs at every shape this is used at, so the eight waves of a block are what fills a CU.
//                     One wave owns one residue i at a time, its atoms in registers; lanes stride over all other residues j, so a
//                     wave reads 64 consecutive dwords of one array and no LDS bank is asked twice.  A pair of residues whose CA
//                     atoms are further apart than 1.9 A + both radii cannot hold an atom pair inside the largest bound (1.7 + 1.7
//                     - 1.5) and is skipped after three loads; the pairs it does hold are counted by integer arithmetic either way.
//                     For an atom pair, 1e-10 + d2 is compared with the squared bound and the root is taken only inside it.
//                     Each lane sums its own j in index order; a butterfly over the wave gives the five per-atom sums of i (both
//                     triangles) and the upper-triangle sum of its row.  Wave 0 then does the bond and angle terms of the tile's
//                     residues, one residue per lane, and reduces the tile's scalar sums by the same butterfly into sixteen
//                     doubles of the workspace.
// violations_finish   one thread per backbone adds the tiles' partials in tile order and writes the slots.
//
// All arithmetic after the fp32 loads is fp64.  No floating-point atomics; every sum has a fixed order that depends only on the
// compacted chain: bitwise reproducible, and independent of B, of the backbone's place in the batch and of absent residues behind it
// (their tiles add +0.0).
#include "fd_common.h"
#include "../../include/fd_hip.h"

namespace {

constexpr int VT = 512;                           // threads of a block: eight waves, each owning one residue at a time
constexpr int VW = VT / 64;
constexpr int V_MAX_N = 2048;                     // FD_VIOLATIONS_MAX_N
constexpr int V_TILE = 64;                        // FD_VIOLATIONS_TILE: compacted residues per block
constexpr int V_PART = 16;                        // doubles of a block's partial

constexpr double V_TOL = 12.0;                    // violation_tolerance_factor (amber_minimize.py:379)
constexpr double V_OVERLAP = 1.5;                 // clash_overlap_tolerance (:380)
constexpr double V_EPS = 1e-6;                    // between_residue_bond_loss' eps
constexpr double V_CLASH_EPS = 1e-10;             // between_residue_clash_loss' eps
constexpr double V_CN = 1.329, V_CN_SD = 0.014;   // residue_constants.between_res_bond_length_c_n[0], ..._stddev_c_n[0]
constexpr double V_COS_CA_C_N = -0.4473;          // between_res_cos_angles_ca_c_n[0]; its tolerance is V_CN_SD's (loss.py:807)
constexpr double V_COS_C_N_CA = -0.5203, V_COS_C_N_CA_SD = 0.0353;
constexpr double V_CA_CA = 3.80209737096;         // residue_constants.ca_ca
constexpr double V_CA_EXCESS = 1.5;               // extreme_ca_ca_distance_violations' max_angstrom_tolerance
constexpr double V_MEAN_EPS = 1e-4;               // tensor_utils.masked_mean's eps
constexpr double V_REACH = 1.7 + 1.7 - V_OVERLAP + 1e-6;      // the largest bound, and room for the rounding of the test itself

// van der Waals radius of atom slot a (N, CA, C, CB, O): residue_constants.van_der_waals_radius by element
__device__ __forceinline__ double vdw(int a) { return a == 0 ? 1.55 : a == 4 ? 1.52 : 1.7; }

__device__ __forceinline__ double relu(double x) { return x > 0.0 ? x : 0.0; }

// The present residues in index order: ridx[compacted] = residue (fd_dssp.hip's compact without the inverse map).  Thread t owns
// the residues [t per, (t + 1) per).  Ends with a barrier; returns the number present.
__device__ __forceinline__ int compact(const float* __restrict__ mask, int N, unsigned short* ridx, int* wave_tot) {
  const int tid = (int)threadIdx.x, lane = fd::lane_id(), wave = fd::wave_id();
  constexpr int PER = V_MAX_N / VT;               // residues per thread at the largest N
  const int per = (N + VT - 1) / VT;
  const int r0 = tid * per;
  unsigned present = 0;
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int r = r0 + k;
    if (k < per && r < N && mask[r] != 0.f) present |= 1u << k;
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
  int base = incl - cnt, n = 0;
  for (int w = 0; w < VW; ++w) {
    if (w < wave) base += wave_tot[w];
    n += wave_tot[w];
  }
#pragma unroll
  for (int k = 0; k < PER; ++k)
    if (present & (1u << k)) ridx[base++] = (unsigned short)(r0 + k);
  __syncthreads();
  return n;
}

// The terms of the connection between the compacted residues a and a + 1 (between_residue_bond_loss on one pair).
struct Bond {
  double c_n, ca_c_n, c_n_ca;                     // the three losses, unmasked as the reference's per-residue sum takes them
  bool bonded, violated, ca_far;                  // res_index step of 1; any hard violation (masked); CA-CA excess (masked)
};

__device__ __forceinline__ Bond bond_terms(const float (*xyz)[V_MAX_N], const int* rix, int a) {
  const int b = a + 1;
  const double cax = (double)xyz[3][a], cay = (double)xyz[4][a], caz = (double)xyz[5][a];
  const double cx = (double)xyz[6][a], cy = (double)xyz[7][a], cz = (double)xyz[8][a];
  const double nx = (double)xyz[0][b], ny = (double)xyz[1][b], nz = (double)xyz[2][b];
  const double ax = (double)xyz[3][b], ay = (double)xyz[4][b], az = (double)xyz[5][b];
  const double len_c_n = sqrt(V_EPS + ((cx - nx) * (cx - nx) + (cy - ny) * (cy - ny) + (cz - nz) * (cz - nz)));
  const double len_ca_c = sqrt(V_EPS + ((cax - cx) * (cax - cx) + (cay - cy) * (cay - cy) + (caz - cz) * (caz - cz)));
  const double len_n_ca = sqrt(V_EPS + ((nx - ax) * (nx - ax) + (ny - ay) * (ny - ay) + (nz - az) * (nz - az)));
  const double ux = (cax - cx) / len_ca_c, uy = (cay - cy) / len_ca_c, uz = (caz - cz) / len_ca_c;      // C -> CA
  const double vx = (nx - cx) / len_c_n, vy = (ny - cy) / len_c_n, vz = (nz - cz) / len_c_n;            // C -> N'
  const double wx = (ax - nx) / len_n_ca, wy = (ay - ny) / len_n_ca, wz = (az - nz) / len_n_ca;         // N' -> CA'
  const double cos1 = ux * vx + uy * vy + uz * vz;
  const double cos2 = (-vx) * wx + (-vy) * wy + (-vz) * wz;
  const double e0 = sqrt(V_EPS + (len_c_n - V_CN) * (len_c_n - V_CN));
  const double e1 = sqrt(V_EPS + (cos1 - V_COS_CA_C_N) * (cos1 - V_COS_CA_C_N));
  const double e2 = sqrt(V_EPS + (cos2 - V_COS_C_N_CA) * (cos2 - V_COS_C_N_CA));
  constexpr double t0 = V_TOL * V_CN_SD, t2 = V_TOL * V_COS_C_N_CA_SD;
  const double d_ca = sqrt(V_EPS + ((cax - ax) * (cax - ax) + (cay - ay) * (cay - ay) + (caz - az) * (caz - az)));
  Bond r;
  r.c_n = relu(e0 - t0);
  r.ca_c_n = relu(e1 - t0);                       // (the reference's quirk: the bond length's tolerance on a cosine)
  r.c_n_ca = relu(e2 - t2);
  r.bonded = (long)rix[b] - (long)rix[a] == 1L;
  r.violated = r.bonded && (e0 > t0 || e1 > t0 || e2 > t2);
  r.ca_far = r.bonded && (d_ca - V_CA_CA) > V_CA_EXCESS;
  return r;
}

__global__ __launch_bounds__(VT) void violations_kernel(const float* __restrict__ atoms, long atom_stride,
                                                        const float* __restrict__ res_mask, const int* __restrict__ res_index,
                                                        int N, int tiles, double* __restrict__ ws, double* __restrict__ res_loss,
                                                        double* __restrict__ atom_loss, unsigned char* __restrict__ flags) {
  __shared__ float xyz[15][V_MAX_N];              // x, y, z of N, CA, C, CB, O of the compacted residues
  __shared__ float rad[V_MAX_N];
  __shared__ int rix[V_MAX_N];
  __shared__ unsigned short ridx[V_MAX_N];
  __shared__ int wave_tot[VW];
  __shared__ double t_upper[V_TILE];              // per residue of the tile: its row of the upper triangle
  __shared__ int t_pairs[V_TILE], t_clashes[V_TILE], t_bits[V_TILE];
  const int tid = (int)threadIdx.x, lane = fd::lane_id(), wave = fd::wave_id();
  const long b = (long)(blockIdx.x / (unsigned)tiles);
  const int tile = (int)(blockIdx.x % (unsigned)tiles);
  const float* bb = atoms + b * N * atom_stride;
  const float* mask = res_mask + b * N;
  const int n = compact(mask, N, ridx, wave_tot);
  for (int i = tid; i < n; i += VT) {
    const int r = ridx[i];
    const float* p = bb + (long)r * atom_stride;
    double far2 = 0.0;
#pragma unroll
    for (int a = 0; a < 5; ++a) {
      xyz[3 * a][i] = p[3 * a], xyz[3 * a + 1][i] = p[3 * a + 1], xyz[3 * a + 2][i] = p[3 * a + 2];
      const double dx = (double)p[3 * a] - (double)p[3], dy = (double)p[3 * a + 1] - (double)p[4],
                   dz = (double)p[3 * a + 2] - (double)p[5];
      const double d2 = dx * dx + dy * dy + dz * dz;
      far2 = d2 > far2 || d2 != d2 ? d2 : far2;                           // (NaN stays: such a residue is never skipped)
    }
    rad[i] = (float)(sqrt(far2) * (1.0 + 1e-6));                          // rounded to fp32 it is still no smaller than the distance
    rix[i] = res_index ? res_index[b * N + r] : r;
  }
  // the absent residues of this tile's range of ORIGINAL indices: zeros in the optional arrays (every element is written once)
  for (int r = tile * V_TILE + tid; r < N && r < (tile + 1) * V_TILE; r += VT) {
    if (mask[r] != 0.f) continue;
    const long o = b * N + r;
    if (res_loss) res_loss[o] = 0.0;
    if (flags) flags[o] = 0;
    if (atom_loss)
      for (int a = 0; a < 5; ++a) atom_loss[o * 5 + a] = 0.0;
  }
  __syncthreads();

  // ---- clashes: residue i on one wave, lanes over j ----
  const int i0 = tile * V_TILE;
  const int i_end = i0 + V_TILE < n ? i0 + V_TILE : n;
  for (int i = i0 + wave; i < i_end; i += VW) {                           // (everything about i is wave-uniform)
    double px[5], py[5], pz[5];
#pragma unroll
    for (int a = 0; a < 5; ++a) px[a] = (double)xyz[3 * a][i], py[a] = (double)xyz[3 * a + 1][i], pz[a] = (double)xyz[3 * a + 2][i];
    const long ri = rix[i];
    const double reach_i = V_REACH + (double)rad[i];
    double la[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, upper_sum = 0.0;
    int pairs = 0, clashes = 0, bits = 0;
    for (int j = lane; j < n; j += 64) {
      const long rj = rix[j];
      if (rj == ri) continue;                                             // the residue itself, and a repeated res_index
      const bool upper = ri < rj;                                         // the triangle the reference's mean counts
      const bool adj = upper ? rj == ri + 1 : ri == rj + 1;
      if (upper) pairs += 25 - (adj ? 1 : 0);
      const double ex = px[1] - (double)xyz[3][j], ey = py[1] - (double)xyz[4][j], ez = pz[1] - (double)xyz[5][j];
      const double reach = reach_i + (double)rad[j];
      if (ex * ex + ey * ey + ez * ez > reach * reach) continue;          // no atom pair of the two can be inside a bound
      double row = 0.0;
#pragma unroll
      for (int c = 0; c < 5; ++c) {                                       // atom c of j against the five atoms of i
        const double qx = (double)xyz[3 * c][j], qy = (double)xyz[3 * c + 1][j], qz = (double)xyz[3 * c + 2][j];
#pragma unroll
        for (int a = 0; a < 5; ++a) {
          // the peptide bond: C of the lower residue and N of the next one (loss.py:935-959)
          if (adj && ((upper && a == 2 && c == 0) || (!upper && a == 0 && c == 2))) continue;
          const double dx = px[a] - qx, dy = py[a] - qy, dz = pz[a] - qz;
          const double s = V_CLASH_EPS + (dx * dx + dy * dy + dz * dz);
          const double bound = (vdw(a) + vdw(c)) - V_OVERLAP;
          if (!(s >= bound * bound * (1.0 + 1e-12))) {                    // (beyond it the root is above the bound; NaN comes in)
            const double dist = sqrt(s);
            const double l = relu(bound - dist);
            la[a] += l;
            row += l;
            if (dist < bound) {
              bits |= 1 << a;
              clashes += upper ? 1 : 0;
            }
          }
        }
      }
      if (upper) upper_sum += row;
    }
#pragma unroll
    for (int a = 0; a < 5; ++a) la[a] = fd::wave_sum(la[a]);
    upper_sum = fd::wave_sum(upper_sum);
    pairs = fd::wave_sum(pairs);
    clashes = fd::wave_sum(clashes);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) bits |= __shfl_xor(bits, o);
    if (lane == 0) {
      t_upper[i - i0] = upper_sum;
      t_pairs[i - i0] = pairs;
      t_clashes[i - i0] = clashes;
      t_bits[i - i0] = bits;
      if (atom_loss) {
        double* o = atom_loss + (b * N + ridx[i]) * 5;
#pragma unroll
        for (int a = 0; a < 5; ++a) o[a] = la[a];
      }
    }
  }
  __syncthreads();

  // ---- bonds and angles, one residue per lane of wave 0; then the tile's sums ----
  if (wave != 0) return;
  const int i = i0 + lane;
  double s_cn = 0.0, s_cacn = 0.0, s_cnca = 0.0, s_clash = 0.0;
  int c_bonds = 0, c_far = 0, c_rbond = 0, c_rclash = 0, c_rany = 0, c_pairs = 0, c_clashes = 0;
  if (i < i_end) {
    double half = 0.0;
    bool violated = false;
    if (i > 0) {                                                          // the connection behind: its half of the per-residue values
      const Bond p = bond_terms(xyz, rix, i - 1);
      half += p.c_n + p.ca_c_n + p.c_n_ca;
      violated = p.violated;
    }
    if (i + 1 < n) {                                                      // the connection ahead: this residue owns its sums
      const Bond q = bond_terms(xyz, rix, i);
      half += q.c_n + q.ca_c_n + q.c_n_ca;
      violated = violated || q.violated;
      if (q.bonded) {
        s_cn = q.c_n, s_cacn = q.ca_c_n, s_cnca = q.c_n_ca;
        c_bonds = 1;
        c_far = q.ca_far ? 1 : 0;
      }
    }
    const int bits = t_bits[lane];
    s_clash = t_upper[lane];
    c_pairs = t_pairs[lane];
    c_clashes = t_clashes[lane];
    c_rbond = violated ? 1 : 0;
    c_rclash = bits ? 1 : 0;
    c_rany = violated || bits ? 1 : 0;
    const long o = b * N + ridx[i];
    if (res_loss) res_loss[o] = 0.5 * half;
    if (flags) flags[o] = (unsigned char)(bits | (violated ? 32 : 0));
  }
  s_cn = fd::wave_sum(s_cn), s_cacn = fd::wave_sum(s_cacn), s_cnca = fd::wave_sum(s_cnca), s_clash = fd::wave_sum(s_clash);
  c_bonds = fd::wave_sum(c_bonds), c_far = fd::wave_sum(c_far), c_rbond = fd::wave_sum(c_rbond);
  c_rclash = fd::wave_sum(c_rclash), c_rany = fd::wave_sum(c_rany), c_pairs = fd::wave_sum(c_pairs);
  c_clashes = fd::wave_sum(c_clashes);
  if (lane == 0) {
    double* o = ws + (long)blockIdx.x * V_PART;
    o[0] = s_cn, o[1] = s_cacn, o[2] = s_cnca, o[3] = s_clash;
    o[4] = (double)c_bonds, o[5] = (double)c_far, o[6] = (double)c_rbond, o[7] = (double)c_rclash, o[8] = (double)c_rany;
    o[9] = (double)c_pairs, o[10] = (double)c_clashes, o[11] = (double)n;
    o[12] = o[13] = o[14] = o[15] = 0.0;
  }
}

__global__ __launch_bounds__(64) void violations_finish(const double* __restrict__ ws, int B, int tiles, double* __restrict__ out) {
  const long b = (long)blockIdx.x * 64 + (long)threadIdx.x;
  if (b >= B) return;
  double s[11];
#pragma unroll
  for (int k = 0; k < 11; ++k) s[k] = 0.0;
  for (int t = 0; t < tiles; ++t)                                         // tile order; the counts are exact integers
#pragma unroll
    for (int k = 0; k < 11; ++k) s[k] += ws[(b * tiles + t) * V_PART + k];
  const double n = ws[b * tiles * V_PART + 11];
  double* o = out + b * FD_VIOLATION_SLOTS;
  o[0] = n;
  o[1] = s[0] / (s[4] + V_EPS);
  o[2] = s[1] / (s[4] + V_EPS);
  o[3] = s[2] / (s[4] + V_EPS);
  o[4] = s[3] / (V_EPS + s[9]);
  o[5] = s[5] / (V_MEAN_EPS + s[4]);
  o[6] = s[6] / (V_MEAN_EPS + n);
  o[7] = s[7] / (V_MEAN_EPS + n);
  o[8] = s[8] / (V_MEAN_EPS + n);
  o[9] = s[8];
  o[10] = s[4];
  o[11] = s[9];
  o[12] = s[10];
  o[13] = o[14] = o[15] = 0.0;
}

}  // namespace

extern "C" int fd_violations(const float* atoms, long atom_stride, const float* res_mask, const int* res_index, int B, int N,
                             double* ws, double* out, double* res_loss, double* atom_loss, unsigned char* flags, void* stream) {
  static_assert(V_MAX_N == FD_VIOLATIONS_MAX_N && V_TILE == FD_VIOLATIONS_TILE && V_PART == 16, "include/fd_hip.h");
  FD_CHECK_ARG(B >= 0 && N >= 0, "fd_violations: negative size");
  FD_CHECK_ARG(atom_stride >= 15, "fd_violations: atom_stride must be at least 15 floats (N, CA, C, CB, O)");
  FD_CHECK_ARG(N <= V_MAX_N, "fd_violations: N must be at most 2048");
  if (B == 0 || N == 0) return FD_OK;
  FD_CHECK_ARG(atoms && res_mask && ws && out, "fd_violations: null operand");
  FD_CHECK_ARG((((uintptr_t)ws) & 7u) == 0 && (((uintptr_t)out) & 7u) == 0 && (((uintptr_t)res_loss) & 7u) == 0 &&
                   (((uintptr_t)atom_loss) & 7u) == 0 && (((uintptr_t)res_index) & 3u) == 0,
               "fd_violations: misaligned operand");
  const int tiles = fd_cdiv(N, V_TILE);
  FD_CHECK_ARG((long)B * tiles < (1L << 24), "fd_violations: B * ceil(N / 64) must be below 2^24 (blocks in one grid)");
  hipLaunchKernelGGL(violations_kernel, dim3((unsigned)((long)B * tiles)), dim3(VT), 0, (hipStream_t)stream, atoms, atom_stride,
                     res_mask, res_index, N, tiles, ws, res_loss, atom_loss, flags);
  FD_CHECK_LAUNCH("fd_violations");
  hipLaunchKernelGGL(violations_finish, dim3((unsigned)fd_cdiv(B, 64)), dim3(64), 0, (hipStream_t)stream, ws, B, tiles, out);
  FD_CHECK_LAUNCH("fd_violations");
  return FD_OK;
}
