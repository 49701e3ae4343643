// fd_dssp_hbonds / fd_dssp_assign: Kabsch & Sander's secondary structure and the reference's shape columns (analysis/metrics.py:37-42
// SHAPE_METRICS, :58-69 calc_mdtraj_metrics) from the backbone atoms the sampler leaves in HBM.  include/fd_hip.h is the
// specification; this file says how the two launches are laid out.
//
// fd_dssp_hbonds  grid over (tiles of 64 residues x backbones).  Every block compacts the present residues of its chain by
//                 fd_backbone_metrics' prefix scan and stages the ACCEPTOR side of all of them -- C, O and CA, nine fp32 arrays
//                 of 2048 = 72 KB -- plus the two index maps (8 KB).  The donor side is wave-uniform: one wave owns one donor at
//                 a time, reads its N from global memory once and derives its H in fp64 in registers (an fp32 H in LDS would
//                 round a derived quantity the decisions are made from, and N and H of all residues would add 48 KB that only
//                 64 donors per block ever use).  Lanes stride over the acceptors, so a wave reads 64 consecutive dwords of one
//                 array: no LDS bank is asked twice.  Each lane keeps its own two lowest (energy, index) keys; a butterfly over the
//                 wave merges them -- the groups that meet in a round are disjoint, so no key is counted twice.
// fd_dssp_assign  one block of 1024 threads per backbone, everything in LDS (43 KB): the bonded table (per donor the compacted indices of its
//                 at most two acceptors below -0.5 kcal/mol), break flags, turn flags, the letters and the ladder list.  The
//                 bridge test is a function of (i, j) on the bonded table, eight lookups, never stored: row i goes to one wave,
//                 its lanes stride over j.  A pair that is a bridge and whose predecessor on the same diagonal is not one of the
//                 same type starts a ladder; the lane that finds it walks it to its end and appends it (an integer LDS counter:
//                 the ORDER of the list varies between runs, nothing that is derived from it does).  Ladders are linked by
//                 minimum-label propagation over all ladder pairs, all threads, until a sweep changes nothing; the fixed point
//                 (the smallest slot number of each connected group) does not depend on the order of the updates.  A list that
//                 would exceed its capacity raises the overflow slot.
//
// All arithmetic after the fp32 loads is fp64.  No floating-point atomics; the sums (the radius of gyration) are per-thread runs
// in index order, a butterfly in the wave, then the wave results in wave order: bitwise reproducible for a given shape.
#include "fd_common.h"
#include "../../include/fd_hip.h"

namespace {

constexpr int DT = 256;                           // threads of an H-bond block: four waves, each owning one donor at a time
constexpr int AT = 1024;                          // threads of an assignment block: the one block of a backbone sweeps all pairs
constexpr int D_MAX_N = 2048;                     // FD_DSSP_MAX_N
constexpr int D_TILE = 64;                        // residues (original index) per block of the H-bond kernel
constexpr int D_LCAP = 2048;                      // ladders per backbone
constexpr int D_NONE = 0xFFFF;                    // cpos of a residue that is not present
constexpr int D_NOJ = 0x7fffffff;                 // index of an empty acceptor slot: above every real one

constexpr double D_Q = 27.888;                    // 332 * 0.42 * 0.20 kcal/mol A
constexpr double D_EMIN = -9.9;
constexpr double D_HB = -0.5;
constexpr double D_CA_CUT = 9.0;
constexpr double D_MIN_DIST = 0.5;
constexpr double D_BREAK = 2.5;
constexpr double D_COS_70 = 0.34202014332566873;  // cos(70 degrees)

enum : signed char { SS_BLANK = 0, SS_H = 1, SS_B = 2, SS_E = 3, SS_G = 4, SS_I = 5, SS_T = 6, SS_S = 7 };

__device__ __forceinline__ double dist3(double ax, double ay, double az, double bx, double by, double bz) {
  const double dx = ax - bx, dy = ay - by, dz = az - bz;
  return sqrt(dx * dx + dy * dy + dz * dz);
}

// NS block-wide sums (fd_metrics.hip's block_sums): on return every thread holds the totals.
template <int NS, int W>
__device__ __forceinline__ void block_sums(double (&s)[NS], double (*red)[W]) {
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
    for (int w = 1; w < W; ++w) v += red[k][w];
    s[k] = v;
  }
}

// The present residues in index order: ridx[compacted] = residue, cpos[residue] = compacted (D_NONE if absent).  Thread t owns the
// residues [t per, (t + 1) per); backbone_metrics_kernel's prefix scan.  Ends with a barrier; returns the number present.
template <int T>
__device__ __forceinline__ int compact(const float* __restrict__ mask, int N, unsigned short* ridx, unsigned short* cpos,
                                       int* wave_tot) {
  const int tid = (int)threadIdx.x, lane = fd::lane_id(), wave = fd::wave_id();
  constexpr int PER = D_MAX_N / T;                // residues per thread at the largest N
  const int per = (N + T - 1) / T;
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
  for (int w = 0; w < T / 64; ++w) {
    if (w < wave) base += wave_tot[w];
    n += wave_tot[w];
  }
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int r = r0 + k;
    if (k < per && r < N) {
      if (present & (1u << k)) {
        ridx[base] = (unsigned short)r;
        cpos[r] = (unsigned short)base;
        ++base;
      } else {
        cpos[r] = (unsigned short)D_NONE;
      }
    }
  }
  __syncthreads();
  return n;
}

// ---- fd_dssp_hbonds --------------------------------------------------------------------------------------------------------------
// the ordered key (energy, index): a strictly smaller key wins, so on equal energies the lower index does
__device__ __forceinline__ bool key_less(double e, int j, double f, int k) { return e < f || (e == f && j < k); }

__global__ __launch_bounds__(DT) void dssp_hbonds_kernel(const float* __restrict__ atoms, long atom_stride,
                                                         const float* __restrict__ res_mask, const float* __restrict__ no_donor,
                                                         int N, int tiles, int* __restrict__ acc_idx, double* __restrict__ acc_e) {
  __shared__ float cx[D_MAX_N], cy[D_MAX_N], cz[D_MAX_N], ox[D_MAX_N], oy[D_MAX_N], oz[D_MAX_N], ax[D_MAX_N], ay[D_MAX_N],
      az[D_MAX_N];
  __shared__ unsigned short ridx[D_MAX_N], cpos[D_MAX_N];
  __shared__ int wave_tot[DT / 64];
  const int tid = (int)threadIdx.x, lane = fd::lane_id(), wave = fd::wave_id();
  const long b = (long)(blockIdx.x / (unsigned)tiles);
  const int tile = (int)(blockIdx.x % (unsigned)tiles);
  const float* bb = atoms + b * N * atom_stride;
  const int n = compact<DT>(res_mask + b * N, N, ridx, cpos, wave_tot);
  for (int i = tid; i < n; i += DT) {
    const float* p = bb + (long)ridx[i] * atom_stride;
    ax[i] = p[3], ay[i] = p[4], az[i] = p[5];
    cx[i] = p[6], cy[i] = p[7], cz[i] = p[8];
    ox[i] = p[12], oy[i] = p[13], oz[i] = p[14];
  }
  __syncthreads();

  const int r_end = (tile + 1) * D_TILE < N ? (tile + 1) * D_TILE : N;
  for (int r = tile * D_TILE + wave; r < r_end; r += DT / 64) {            // (everything about the donor is wave-uniform)
    const int i = (int)cpos[r];
    double e1 = 0.0, e2 = 0.0;
    int j1 = D_NOJ, j2 = D_NOJ;
    bool donor = i != D_NONE && i > 0 && (int)ridx[i > 0 ? i - 1 : 0] + 1 == r && (!no_donor || no_donor[b * N + r] == 0.f);
    double nx = 0.0, ny = 0.0, nz = 0.0;
    if (donor) {
      const float* p = bb + (long)r * atom_stride;
      nx = (double)p[0], ny = (double)p[1], nz = (double)p[2];
      // a C-N distance above 2.5 A is a chain break (NaN coordinates compare false: such a residue is left a donor and
      // every energy of it is NaN, which no comparison keeps)
      donor = !(dist3((double)cx[i - 1], (double)cy[i - 1], (double)cz[i - 1], nx, ny, nz) > D_BREAK);
    }
    if (donor) {
      const double ux = (double)cx[i - 1] - (double)ox[i - 1], uy = (double)cy[i - 1] - (double)oy[i - 1],
                   uz = (double)cz[i - 1] - (double)oz[i - 1];
      const double ul = sqrt(ux * ux + uy * uy + uz * uz);
      const double hx = nx + ux / ul, hy = ny + uy / ul, hz = nz + uz / ul;
      const double cax = (double)ax[i], cay = (double)ay[i], caz = (double)az[i];
      const double inf = __builtin_inf();
      e1 = inf, e2 = inf;
      for (int j = lane; j < n; j += 64) {
        if (j == i || j == i - 1) continue;
        if (!(dist3(cax, cay, caz, (double)ax[j], (double)ay[j], (double)az[j]) < D_CA_CUT)) continue;
        const double jcx = (double)cx[j], jcy = (double)cy[j], jcz = (double)cz[j];
        const double jox = (double)ox[j], joy = (double)oy[j], joz = (double)oz[j];
        const double dno = dist3(nx, ny, nz, jox, joy, joz), dhc = dist3(hx, hy, hz, jcx, jcy, jcz);
        const double dho = dist3(hx, hy, hz, jox, joy, joz), dnc = dist3(nx, ny, nz, jcx, jcy, jcz);
        double e = D_Q * (1.0 / dno + 1.0 / dhc - 1.0 / dho - 1.0 / dnc);
        if (dno < D_MIN_DIST || dhc < D_MIN_DIST || dho < D_MIN_DIST || dnc < D_MIN_DIST) e = D_EMIN;
        if (e < D_EMIN) e = D_EMIN;
        if (key_less(e, j, e1, j1)) {
          e2 = e1, j2 = j1;
          e1 = e, j1 = j;
        } else if (key_less(e, j, e2, j2)) {
          e2 = e, j2 = j;
        }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const double f1 = __shfl_xor(e1, o), f2 = __shfl_xor(e2, o);
        const int k1 = __shfl_xor(j1, o), k2 = __shfl_xor(j2, o);
        if (key_less(f1, k1, e1, j1)) {                               // theirs first; second: my first or their second
          if (key_less(e1, j1, f2, k2)) e2 = e1, j2 = j1; else e2 = f2, j2 = k2;
          e1 = f1, j1 = k1;
        } else if (key_less(f1, k1, e2, j2)) {                        // mine first; second: their first
          e2 = f1, j2 = k1;
        }
      }
    }
    if (lane == 0) {
      const long o = (b * N + r) * 2;
      acc_idx[o] = j1 == D_NOJ ? -1 : (int)ridx[j1];
      acc_e[o] = j1 == D_NOJ ? 0.0 : e1;
      acc_idx[o + 1] = j2 == D_NOJ ? -1 : (int)ridx[j2];
      acc_e[o + 1] = j2 == D_NOJ ? 0.0 : e2;
    }
  }
}

// ---- fd_dssp_assign --------------------------------------------------------------------------------------------------------------
struct Dssp {
  const short *a1, *a2;                           // bonded table: the donor's acceptors below -0.5 (compacted), -1 if none
  const unsigned char* brk;                       // brk[a]: chain break between a and a + 1
  int n;
};

__device__ __forceinline__ bool hb(const Dssp& d, int donor, int acc) { return (int)d.a1[donor] == acc || (int)d.a2[donor] == acc; }

__device__ __forceinline__ bool nobreak(const Dssp& d, int a, int b) {
  if (a < 0 || b >= d.n || a > b) return false;
  for (int k = a; k < b; ++k)
    if (d.brk[k]) return false;
  return true;
}

// 0 none, 1 parallel, 2 antiparallel
__device__ __forceinline__ int bridge_type(const Dssp& d, int i, int j) {
  if (i < 1 || j < i + 3 || j > d.n - 2) return 0;
  if (d.brk[i - 1] || d.brk[i] || d.brk[j - 1] || d.brk[j]) return 0;
  if ((hb(d, i + 1, j) && hb(d, j, i - 1)) || (hb(d, j + 1, i) && hb(d, i, j - 1))) return 1;
  if ((hb(d, i + 1, j - 1) && hb(d, j + 1, i - 1)) || (hb(d, j, i) && hb(d, i, j))) return 2;
  return 0;
}

struct Ladders {
  const unsigned short *i0, *jlo, *len;
  const unsigned char* type;
};

__device__ __forceinline__ bool linked(const Dssp& d, const Ladders& L, int l, int m) {
  if (L.type[l] != L.type[m]) return false;
  const int A = L.i0[l] <= L.i0[m] ? l : m, B = A == l ? m : l;       // ordered by their first strand
  const int a_i1 = (int)L.i0[A] + (int)L.len[A] - 1;
  const int gi = (int)L.i0[B] - a_i1 - 1;
  if (gi < 0 || gi > 4) return false;
  const int a_jlo = L.jlo[A], a_jhi = a_jlo + (int)L.len[A] - 1, b_jlo = L.jlo[B], b_jhi = b_jlo + (int)L.len[B] - 1;
  const int from = L.type[A] == 1 ? a_jhi : b_jhi, to = L.type[A] == 1 ? b_jlo : a_jlo;
  const int gj = to - from - 1;
  if (gj < 0 || gj > 4) return false;
  if (!((gi <= 1 && gj <= 4) || (gi <= 4 && gj <= 1))) return false;
  return nobreak(d, a_i1, L.i0[B]) && nobreak(d, from, to);
}

constexpr int AW = AT / 64;

__global__ __launch_bounds__(AT) void dssp_assign_kernel(const float* __restrict__ atoms, long atom_stride, int natoms,
                                                         const float* __restrict__ res_mask, const int* __restrict__ acc_idx,
                                                         const double* __restrict__ acc_e, int N, signed char* __restrict__ ss_out,
                                                         double* __restrict__ out) {
  __shared__ unsigned short ridx[D_MAX_N], cpos[D_MAX_N];
  __shared__ short a1[D_MAX_N], a2[D_MAX_N];
  __shared__ unsigned char brk[D_MAX_N], turn[D_MAX_N], cand[D_MAX_N];
  __shared__ signed char ss[D_MAX_N];
  __shared__ unsigned short l_i0[D_LCAP], l_jlo[D_LCAP], l_len[D_LCAP], l_grp[D_LCAP];
  __shared__ unsigned char l_type[D_LCAP];
  __shared__ int wave_tot[AW], nlad, changed;
  __shared__ double red[4][AW];
  const int tid = (int)threadIdx.x, lane = fd::lane_id(), wave = fd::wave_id();
  const long b = (long)blockIdx.x;
  const float* bb = atoms + b * N * atom_stride;
  if (tid == 0) nlad = 0;
  const int n = compact<AT>(res_mask + b * N, N, ridx, cpos, wave_tot);
  Dssp d;
  d.a1 = a1, d.a2 = a2, d.brk = brk, d.n = n;

  // ---- the bonded table and the chain breaks ----
  int nhb = 0;
  for (int i = tid; i < n; i += AT) {
    const int r = ridx[i];
    const long o = (b * N + r) * 2;
    const int k1 = acc_idx[o], k2 = acc_idx[o + 1];
    // (an index outside the chain, or of a residue that is not present -- cpos D_NONE reads as -1 --, is no acceptor)
    const bool b1 = k1 >= 0 && k1 < N && acc_e[o] < D_HB, b2 = k2 >= 0 && k2 < N && acc_e[o + 1] < D_HB;
    a1[i] = b1 ? (short)cpos[k1] : (short)-1;
    a2[i] = b2 ? (short)cpos[k2] : (short)-1;
    nhb += (b1 ? 1 : 0) + (b2 ? 1 : 0);
    bool br = false;
    if (i + 1 < n) {
      const float* c = bb + (long)r * atom_stride + 6;
      const float* nn = bb + (long)ridx[i + 1] * atom_stride;
      br = (int)ridx[i + 1] != r + 1 ||
           dist3((double)c[0], (double)c[1], (double)c[2], (double)nn[0], (double)nn[1], (double)nn[2]) > D_BREAK;
    }
    brk[i] = br ? 1 : 0;
    ss[i] = SS_BLANK;
    cand[i] = 0;
  }
  __syncthreads();

  // ---- turns: bit n - 3 of turn[i] = hb(i + n, i) and no break in i .. i + n ----
  for (int i = tid; i < n; i += AT) {
    unsigned t = 0;
#pragma unroll
    for (int k = 3; k <= 5; ++k)
      if (i + k < n && hb(d, i + k, i) && nobreak(d, i, i + k)) t |= 1u << (k - 3);
    turn[i] = (unsigned char)t;
  }

  // ---- ladders: row i on one wave, lanes over j; a bridge without a predecessor of its type starts a ladder ----
  int over = 0;
  for (int i = 1 + wave; i < n - 1; i += AW) {
    if (brk[i - 1] || brk[i]) continue;                               // (the row's half of a bridge's conditions)
    const int p1 = a1[i], p2 = a2[i], q1 = a1[i + 1], q2 = a2[i + 1]; // the acceptors of the donors i and i + 1
    for (int j = i + 3 + lane; j <= n - 2; j += 64) {
      // bridge_type(d, i, j) with its eight lookups as six independent LDS reads and no branch between them: the short-circuit
      // form waits for one LDS round trip per lookup, and this loop over all pairs is where the kernel's time goes
      const int r1 = a1[j], r2 = a2[j], s1 = a1[j + 1], s2 = a2[j + 1];
      const bool whole = !(brk[j - 1] | brk[j]);
      const bool par = (((q1 == j) | (q2 == j)) & ((r1 == i - 1) | (r2 == i - 1))) |
                       (((s1 == i) | (s2 == i)) & ((p1 == j - 1) | (p2 == j - 1)));
      const bool anti = (((q1 == j - 1) | (q2 == j - 1)) & ((s1 == i - 1) | (s2 == i - 1))) |
                        (((r1 == i) | (r2 == i)) & ((p1 == j) | (p2 == j)));
      const int t = !whole ? 0 : par ? 1 : anti ? 2 : 0;
      if (t == 0) continue;
      const int step = t == 1 ? 1 : -1;
      if (bridge_type(d, i - 1, j - step) == t) continue;
      int len = 1;
      while (bridge_type(d, i + len, j + step * len) == t) ++len;
      const int slot = atomicAdd(&nlad, 1);
      if (slot < D_LCAP) {
        l_i0[slot] = (unsigned short)i;
        l_jlo[slot] = (unsigned short)(t == 1 ? j : j - len + 1);
        l_len[slot] = (unsigned short)len;
        l_type[slot] = (unsigned char)t;
        l_grp[slot] = (unsigned short)slot;
      } else {
        over = 1;
      }
    }
  }
  __syncthreads();
  const int nl = nlad < D_LCAP ? nlad : D_LCAP;
  Ladders L;
  L.i0 = l_i0, L.jlo = l_jlo, L.len = l_len, L.type = l_type;

  // ---- bulge linking: every ladder takes the smallest label among the ladders linked to it, until nothing changes ----
  for (;;) {
    __syncthreads();
    if (tid == 0) changed = 0;
    __syncthreads();
    for (int l = tid; l < nl; l += AT) {
      int g = l_grp[l];
      for (int m = 0; m < nl; ++m) {
        const int gm = l_grp[m];
        if (gm < g && linked(d, L, l, m)) g = gm;
      }
      if (g < (int)l_grp[l]) {
        l_grp[l] = (unsigned short)g;
        changed = 1;
      }
    }
    __syncthreads();
    if (!changed) break;
  }

  // ---- sheet letters: the ladder whose slot is its group's label speaks for the group; B first, then E over it ----
  for (int pass = 0; pass < 2; ++pass) {
    for (int l = tid; l < nl; l += AT) {
      if ((int)l_grp[l] != l) continue;
      int bridges = 0, imin = D_MAX_N, imax = -1, jmin = D_MAX_N, jmax = -1;
      for (int m = 0; m < nl; ++m) {
        if ((int)l_grp[m] != l) continue;
        const int len = l_len[m], i0 = l_i0[m], j0 = l_jlo[m];
        bridges += len;
        imin = i0 < imin ? i0 : imin;
        imax = i0 + len - 1 > imax ? i0 + len - 1 : imax;
        jmin = j0 < jmin ? j0 : jmin;
        jmax = j0 + len - 1 > jmax ? j0 + len - 1 : jmax;
      }
      if ((bridges > 1) != (pass == 1)) continue;
      const signed char letter = pass == 1 ? SS_E : SS_B;
      for (int k = imin; k <= imax; ++k) ss[k] = letter;
      for (int k = jmin; k <= jmax; ++k) ss[k] = letter;
    }
    __syncthreads();
  }

  // ---- helices: H over anything; G and I only where all their residues are still blank ----
  for (int i = tid + 1; i < n; i += AT)
    if ((turn[i - 1] & 2u) && (turn[i] & 2u))
      for (int k = 0; k < 4; ++k) ss[i + k] = SS_H;                   // (turn_4(i) implies i + 4 < n)
  __syncthreads();
  for (int i = tid + 1; i < n; i += AT)
    if ((turn[i - 1] & 1u) && (turn[i] & 1u) && ss[i] == SS_BLANK && ss[i + 1] == SS_BLANK && ss[i + 2] == SS_BLANK) cand[i] = 1;
  __syncthreads();
  for (int i = tid + 1; i < n; i += AT)
    if (cand[i] & 1u)
      for (int k = 0; k < 3; ++k) ss[i + k] = SS_G;
  __syncthreads();
  for (int i = tid + 1; i < n; i += AT)
    if ((turn[i - 1] & 4u) && (turn[i] & 4u) && ss[i] == SS_BLANK && ss[i + 1] == SS_BLANK && ss[i + 2] == SS_BLANK &&
        ss[i + 3] == SS_BLANK && ss[i + 4] == SS_BLANK)
      cand[i] |= 2u;
  __syncthreads();
  for (int i = tid + 1; i < n; i += AT)
    if (cand[i] & 2u)
      for (int k = 0; k < 5; ++k) ss[i + k] = SS_I;
  __syncthreads();

  // ---- T, S, and the class counts (every thread writes and counts only its own residues) ----
  double s[4] = {0.0, 0.0, (double)nhb, (double)over};
  for (int i = tid; i < n; i += AT) {
    signed char c = ss[i];
    if (c == SS_BLANK) {
      bool t = false;
#pragma unroll
      for (int k = 3; k <= 5; ++k)
        for (int q = i - k + 1; q < i; ++q)
          if (q >= 0 && (turn[q] & (1u << (k - 3)))) t = true;
      if (t) c = SS_T;
    }
    if (c == SS_BLANK && nobreak(d, i - 2, i + 2)) {
      const float* p0 = bb + (long)ridx[i - 2] * atom_stride + 3;
      const float* p1 = bb + (long)ridx[i] * atom_stride + 3;
      const float* p2 = bb + (long)ridx[i + 2] * atom_stride + 3;
      const double ux = (double)p1[0] - (double)p0[0], uy = (double)p1[1] - (double)p0[1], uz = (double)p1[2] - (double)p0[2];
      const double vx = (double)p2[0] - (double)p1[0], vy = (double)p2[1] - (double)p1[1], vz = (double)p2[2] - (double)p1[2];
      const double ck = (ux * vx + uy * vy + uz * vz) / sqrt((ux * ux + uy * uy + uz * uz) * (vx * vx + vy * vy + vz * vz));
      if (ck < D_COS_70) c = SS_S;                                    // an angle above 70 degrees
    }
    ss[i] = c;
    s[0] += (c == SS_H || c == SS_G || c == SS_I) ? 1.0 : 0.0;
    s[1] += (c == SS_E || c == SS_B) ? 1.0 : 0.0;
  }
  block_sums<4, AW>(s, red);                                              // (its barriers also publish ss)
  for (int r = tid; r < N; r += AT) ss_out[b * N + r] = cpos[r] == D_NONE ? (signed char)-1 : ss[cpos[r]];

  // ---- radius of gyration over all atoms of the present residues whose coordinates are not all zero ----
  const int total = n * natoms;                   // (at most 2048 * 37)
  double c4[4] = {0.0, 0.0, 0.0, 0.0};
  for (int q = tid; q < total; q += AT) {
    const float* p = bb + (long)ridx[q / natoms] * atom_stride + 3 * (q % natoms);
    if (p[0] != 0.f || p[1] != 0.f || p[2] != 0.f) {
      c4[0] += 1.0;
      c4[1] += (double)p[0];
      c4[2] += (double)p[1];
      c4[3] += (double)p[2];
    }
  }
  block_sums<4, AW>(c4, red);
  const double mx = c4[1] / c4[0], my = c4[2] / c4[0], mz = c4[3] / c4[0];
  double g[1] = {0.0};
  for (int q = tid; q < total; q += AT) {
    const float* p = bb + (long)ridx[q / natoms] * atom_stride + 3 * (q % natoms);
    if (p[0] != 0.f || p[1] != 0.f || p[2] != 0.f) {
      const double dx = (double)p[0] - mx, dy = (double)p[1] - my, dz = (double)p[2] - mz;
      g[0] += dx * dx + dy * dy + dz * dz;
    }
  }
  block_sums<1, AW>(g, red);

  if (tid == 0) {
    const double dn = (double)n;                  // 0 / 0 = NaN for an empty chain, as np.mean gives
    double* o = out + b * 8;
    o[0] = dn;
    o[1] = s[0] / dn;
    o[2] = s[1] / dn;
    o[3] = (dn - s[0] - s[1]) / dn;
    o[4] = (s[0] + s[1]) / dn;
    o[5] = sqrt(g[0] / c4[0]) / 10.0;
    o[6] = s[2];
    o[7] = s[3] > 0.0 ? 1.0 : 0.0;
  }
}

}  // namespace

extern "C" int fd_dssp_hbonds(const float* atoms, long atom_stride, const float* res_mask, const float* no_donor, int B, int N,
                              int* acc_idx, double* acc_e, void* stream) {
  FD_CHECK_ARG(B >= 0 && N >= 0, "fd_dssp_hbonds: negative size");
  FD_CHECK_ARG(atom_stride >= 15, "fd_dssp_hbonds: atom_stride must be at least 15 floats (N, CA, C, CB, O)");
  FD_CHECK_ARG(N <= D_MAX_N, "fd_dssp_hbonds: N must be at most 2048");
  if (B == 0 || N == 0) return FD_OK;
  FD_CHECK_ARG(atoms && res_mask && acc_idx && acc_e, "fd_dssp_hbonds: null operand");
  FD_CHECK_ARG((((uintptr_t)acc_e) & 7u) == 0 && (((uintptr_t)acc_idx) & 3u) == 0, "fd_dssp_hbonds: misaligned output");
  const int tiles = fd_cdiv(N, D_TILE);
  FD_CHECK_ARG((long)B * tiles < (1L << 24), "fd_dssp_hbonds: B * ceil(N / 64) must be below 2^24 (blocks in one grid)");
  hipLaunchKernelGGL(dssp_hbonds_kernel, dim3((unsigned)((long)B * tiles)), dim3(DT), 0, (hipStream_t)stream, atoms, atom_stride,
                     res_mask, no_donor, N, tiles, acc_idx, acc_e);
  FD_CHECK_LAUNCH("fd_dssp_hbonds");
  return FD_OK;
}

extern "C" int fd_dssp_assign(const float* atoms, long atom_stride, int natoms, const float* res_mask, const int* acc_idx,
                              const double* acc_e, int B, int N, signed char* ss, double* out, void* stream) {
  FD_CHECK_ARG(B >= 0 && N >= 0, "fd_dssp_assign: negative size");
  FD_CHECK_ARG(atom_stride >= 15, "fd_dssp_assign: atom_stride must be at least 15 floats (N, CA, C, CB, O)");
  FD_CHECK_ARG(natoms >= 5 && 3L * natoms <= atom_stride, "fd_dssp_assign: natoms must be at least 5 and fit the atom stride");
  FD_CHECK_ARG(N <= D_MAX_N, "fd_dssp_assign: N must be at most 2048");
  if (B == 0 || N == 0) return FD_OK;
  FD_CHECK_ARG(atoms && res_mask && acc_idx && acc_e && ss && out, "fd_dssp_assign: null operand");
  FD_CHECK_ARG((((uintptr_t)acc_e) & 7u) == 0 && (((uintptr_t)out) & 7u) == 0 && (((uintptr_t)acc_idx) & 3u) == 0,
               "fd_dssp_assign: misaligned operand");
  hipLaunchKernelGGL(dssp_assign_kernel, dim3(B), dim3(AT), 0, (hipStream_t)stream, atoms, atom_stride, natoms, res_mask, acc_idx,
                     acc_e, N, ss, out);
  FD_CHECK_LAUNCH("fd_dssp_assign");
  return FD_OK;
}
