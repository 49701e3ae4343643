// fd_cluster: agglomerative clustering (single, average, complete linkage) of the similarity or distance matrices the evaluation
// kernels leave in HBM, and the flat cut of the tree with medoids and the set-level counts.  include/fd_hip.h is the specification;
// this file says how the two launches are laid out.
//
// linkage_kernel   one block of 256 threads per problem.  The present samples are compacted in index order into slots 0 .. n-1; the
//                  working matrix W [n][n] (both triangles, so that a row is contiguous) lives in the workspace in HBM.  LDS holds,
//                  per slot, the cluster's id, size and alive flag and a cache of the row's best partner -- its distance and its slot
//                  -- under the full key (distance, smaller id, larger id): 84 KB at M = 4096, and 8 KB for the list of rows to
//                  rescan.  One merge is
//                    1. a block-wide minimum over the cached entries (every comparison, in a lane, across lanes and across waves,
//                       is the full key; equal keys are the same pair seen from its two rows, and the row's slot orders those);
//                    2. the Lance-Williams update of the row and column of the slot that keeps the merged cluster, one thread per
//                       other cluster, which also compares the new distance with that cluster's cached entry (so the cache stays
//                       exact even where rounding takes an average below its operands) and lists the rows whose cached partner was
//                       one of the two merged clusters;
//                    3. a rescan of the listed rows and of the merged cluster's own row, one wave per row.
//                  Three barriers per merge, all reached by every thread: the trip count of the merge loop and the winner of step 1
//                  are the same in every thread, and the rescan loops are bounded by the number of slots.
// cut_kernel       one block of 256 threads per problem.  The merges at or below the cut set parent links (every id is a child of at
//                  most one merge); thirteen rounds of pointer jumping give every leaf its root; one thread numbers the clusters in
//                  index order; one thread per leaf sums the original entries against the other members of its cluster, in index
//                  order; one thread picks the medoids and adds the sums up, in index order.
//
// fp64 throughout, no floating-point atomics (the one atomic is the integer cursor of the rescan list in LDS; the order of the list
// changes no result), no communication between blocks: results are bitwise reproducible and independent of G and of the place of a
// problem in the batch.
#include "fd_common.h"
#include "../../include/fd_hip.h"

#include <climits>
#include <cmath>

namespace {

constexpr int CT = 256;                           // threads of a block
constexpr int CW = CT / 64;
constexpr int C_MAX_M = 4096;                     // FD_CLUSTER_MAX_M
constexpr int C_ROUNDS = 13;                      // pointer-jumping rounds: a path of 2^13 links collapses, the longest has M - 1 < 2^12

struct Key {
  double d;
  int lo, hi;                                     // the smaller and the larger id of the pair
  int i, j;                                       // the row's slot and its partner's slot (-1: no pair)
};

__device__ __forceinline__ Key no_key() { return Key{INFINITY, INT_MAX, INT_MAX, -1, -1}; }

// the order of the specification, then the row's slot: a pair appears in the caches of both of its rows under the same (d, lo, hi)
__device__ __forceinline__ bool key_less(const Key& x, const Key& y) {
  if (x.d < y.d) return true;
  if (!(x.d == y.d)) return false;
  if (x.lo != y.lo) return x.lo < y.lo;
  if (x.hi != y.hi) return x.hi < y.hi;
  return x.i < y.i;
}

__device__ __forceinline__ Key wave_min(Key k) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    Key u;
    u.d = __shfl_xor(k.d, o);
    u.lo = __shfl_xor(k.lo, o);
    u.hi = __shfl_xor(k.hi, o);
    u.i = __shfl_xor(k.i, o);
    u.j = __shfl_xor(k.j, o);
    if (key_less(u, k)) k = u;
  }
  return k;
}

__device__ __forceinline__ double first_read(double v, int kind) {
  const double d = kind ? 1.0 - v : v;
  return d == d ? d : (double)INFINITY;           // NaN is read as +inf: such a pair merges last
}

// The best partner of the cluster in slot k over the alive slots, by one wave.  `dead` is a slot to pass over and (a, id_a) the id
// to take for slot a: the two changes of the merge under way, which the arrays in LDS may or may not hold yet.  Every lane returns
// the same key.
__device__ __forceinline__ Key scan_row(const double* __restrict__ W, int n, int k, const int* cid, const unsigned char* alive,
                                        int dead, int a, int id_a) {
  const int lane = fd::lane_id();
  const int idk = k == a ? id_a : cid[k];
  const double* row = W + (long)k * n;
  Key best = no_key();
  for (int j = lane; j < n; j += 64) {
    if (j == k || j == dead || !alive[j]) continue;
    const int idj = j == a ? id_a : cid[j];
    const Key c{row[j], idk < idj ? idk : idj, idk < idj ? idj : idk, k, j};
    if (key_less(c, best)) best = c;
  }
  return wave_min(best);
}

__global__ __launch_bounds__(CT) void linkage_kernel(const double* __restrict__ mat, long ld, long problem_stride,
                                                     const unsigned char* __restrict__ present, int M, int kind, int method,
                                                     double* __restrict__ ws, double* __restrict__ Z, int* __restrict__ num_merges) {
  __shared__ double bd[C_MAX_M];                  // per slot: the distance to the best partner of its row
  __shared__ int bj[C_MAX_M];                     //           that partner's slot (-1: none)
  __shared__ int cid[C_MAX_M];                    //           the cluster's id
  __shared__ int csize[C_MAX_M];                  //           its number of leaves
  __shared__ unsigned char alive[C_MAX_M];
  __shared__ unsigned short todo[C_MAX_M];        // rows to rescan after the merge under way
  __shared__ int todo_n;
  __shared__ int wave_tot[CW];
  __shared__ double p_d[CW];                      // the waves' minima of step 1
  __shared__ int p_lo[CW], p_hi[CW], p_i[CW], p_j[CW];
  const int tid = (int)threadIdx.x, lane = fd::lane_id(), wave = fd::wave_id();
  const long g = (long)blockIdx.x;
  const double* A = mat + g * problem_stride;
  const unsigned char* pres = present ? present + g * M : nullptr;
  double* W = ws + g * (long)M * M;
  double* Zg = Z + g * (long)(M - 1) * 4;

  // ---- the present samples in index order: cid[slot] = original index (the prefix scan of fd_violations' compact) ----
  constexpr int PER = C_MAX_M / CT;
  const int per = (M + CT - 1) / CT;
  const int r0 = tid * per;
  unsigned bits = 0;
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int r = r0 + k;
    if (k < per && r < M && (!pres || pres[r] != 0)) bits |= 1u << k;
  }
  const int cnt = __builtin_popcount(bits);
  int incl = cnt;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl(incl, lane >= o ? lane - o : lane);
    if (lane >= o) incl += u;
  }
  if (lane == 63) wave_tot[wave] = incl;
  if (tid == 0) todo_n = 0;
  __syncthreads();
  int base = incl - cnt, n = 0;
  for (int w = 0; w < CW; ++w) {
    if (w < wave) base += wave_tot[w];
    n += wave_tot[w];
  }
#pragma unroll
  for (int k = 0; k < PER; ++k)
    if (bits & (1u << k)) {
      cid[base] = r0 + k;
      csize[base] = 1;
      alive[base] = 1;
      ++base;
    }
  __syncthreads();

  // ---- the distances, both triangles, from the strict upper triangle of the input ----
  for (int c = 0; c + 1 < n; ++c) {
    const double* src = A + (long)cid[c] * ld;
    for (int c2 = c + 1 + tid; c2 < n; c2 += CT) {
      const double d = first_read(src[cid[c2]], kind);
      W[(long)c * n + c2] = d;
      W[(long)c2 * n + c] = d;
    }
  }
  __syncthreads();
  for (int c = wave; c < n; c += CW) {
    const Key k = scan_row(W, n, c, cid, alive, -1, -1, 0);
    if (lane == 0) bd[c] = k.d, bj[c] = k.j;
  }
  __syncthreads();

  // ---- the merges ----
  int merges = 0;
  long rescans = 0;
  for (int s = 0; s + 1 < n; ++s) {               // (n is the same in every thread)
    Key mine = no_key();
    for (int i = tid; i < n; i += CT) {
      const int j = bj[i];
      if (!alive[i] || j < 0) continue;
      const int a = cid[i], b = cid[j];
      const Key c{bd[i], a < b ? a : b, a < b ? b : a, i, j};
      if (key_less(c, mine)) mine = c;
    }
    mine = wave_min(mine);
    if (lane == 0) p_d[wave] = mine.d, p_lo[wave] = mine.lo, p_hi[wave] = mine.hi, p_i[wave] = mine.i, p_j[wave] = mine.j;
    __syncthreads();
    Key win = no_key();
#pragma unroll
    for (int w = 0; w < CW; ++w) {
      const Key c{p_d[w], p_lo[w], p_hi[w], p_i[w], p_j[w]};
      if (key_less(c, win)) win = c;
    }
    if (win.j < 0) break;                         // (cannot happen with two alive clusters; the same in every thread)
    const int a = cid[win.i] == win.lo ? win.i : win.j;       // the slot of the smaller id: it keeps the merged cluster
    const int b = a == win.i ? win.j : win.i;
    const int na = csize[a], nb = csize[b];
    const int id_new = M + s;
    const double fa = (double)na, fb = (double)nb, fn = (double)(na + nb);
    double* row_a = W + (long)a * n;
    const double* row_b = W + (long)b * n;
    for (int k = tid; k < n; k += CT) {
      if (k == a || k == b || !alive[k]) continue;
      const double da = row_a[k], db = row_b[k];
      double dn;
      if (method == 0) dn = db < da ? db : da;
      else if (method == 2) dn = db > da ? db : da;
      else dn = (fa * da + fb * db) / fn;
      row_a[k] = dn;
      W[(long)k * n + a] = dn;
      const int pj = bj[k];
      if (pj == a || pj == b) {
        todo[atomicAdd(&todo_n, 1)] = (unsigned short)k;
      } else {
        const int idk = cid[k];
        const Key c{dn, idk, id_new, k, a};       // (the new id is above every other)
        Key old = no_key();
        if (pj >= 0) {
          const int idp = cid[pj];
          old = Key{bd[k], idk < idp ? idk : idp, idk < idp ? idp : idk, k, pj};
        }
        if (key_less(c, old)) bd[k] = dn, bj[k] = a;
      }
    }
    __syncthreads();
    const int listed = todo_n;
    if (tid == 0) {
      alive[b] = 0;
      cid[a] = id_new;
      csize[a] = na + nb;
      double* z = Zg + (long)s * 4;
      z[0] = (double)win.lo, z[1] = (double)win.hi, z[2] = win.d, z[3] = fn;
      rescans += listed + 1;
    }
    for (int e = wave; e <= listed; e += CW) {    // (listed <= n - 2)
      const int k = e == 0 ? a : (int)todo[e - 1];
      const Key r = scan_row(W, n, k, cid, alive, b, a, id_new);
      if (lane == 0) bd[k] = r.d, bj[k] = r.j;
    }
    ++merges;
    __syncthreads();
    if (tid == 0) todo_n = 0;
  }

  for (long e = (long)merges * 4 + tid; e < (long)(M - 1) * 4; e += CT) {
    const int c = (int)(e & 3);
    Zg[e] = c < 2 ? -1.0 : c == 2 ? (double)INFINITY : 0.0;
  }
  if (tid == 0) {
    num_merges[g] = merges;
    W[0] = (double)rescans;                       // (the diagonal is never read: a free place for the cost figure)
  }
}

__global__ __launch_bounds__(CT) void cut_kernel(const double* __restrict__ Z, const int* __restrict__ num_merges,
                                                 const double* __restrict__ mat, long ld, long problem_stride,
                                                 const unsigned char* __restrict__ present, int M, int kind, double cut,
                                                 int* __restrict__ labels, int* __restrict__ rep, double* __restrict__ out) {
  __shared__ int par[2 * C_MAX_M];                // by id: the merge it is a child of (-1: none at or below the cut); then towards the root
  __shared__ unsigned short clab[2 * C_MAX_M];    // by root id: the cluster's number (NONE: not met yet)
  __shared__ unsigned short lab[C_MAX_M];         // by leaf: its cluster's number (NONE: absent)
  __shared__ unsigned short medoid[C_MAX_M];      // by cluster
  __shared__ unsigned short members[C_MAX_M];     // by cluster
  __shared__ double score[C_MAX_M];               // by leaf: the sum of the entries against the other members
  __shared__ double upper[C_MAX_M];               //          the part of it with the other member behind the leaf
  __shared__ double w_below[CW], w_above[CW];
  __shared__ int n_clusters;
  constexpr unsigned short NONE = 0xffff;
  const int tid = (int)threadIdx.x, lane = fd::lane_id(), wave = fd::wave_id();
  const long g = (long)blockIdx.x;
  const double* A = mat + g * problem_stride;
  const unsigned char* pres = present ? present + g * M : nullptr;
  const double* Zg = Z + g * (long)(M - 1) * 4;
  int nm = num_merges[g];
  nm = nm < 0 ? 0 : nm > M - 1 ? M - 1 : nm;

  for (int id = tid; id < 2 * M; id += CT) par[id] = -1, clab[id] = NONE;
  for (int i = tid; i < M; i += CT) lab[i] = pres && pres[i] == 0 ? NONE : 0;
  __syncthreads();
  // the merges at or below the cut; the heights on both sides of it
  double below = -INFINITY, above = -INFINITY;    // (above: of the negated heights)
  for (int s = tid; s < nm; s += CT) {
    const double h = Zg[(long)s * 4 + 2];
    if (h <= cut) {
      const int a = (int)Zg[(long)s * 4], b = (int)Zg[(long)s * 4 + 1];
      if (a >= 0 && a < M + s && b >= 0 && b < M + s) par[a] = par[b] = M + s;
      below = h > below ? h : below;
    } else if (h > cut) {
      above = -h > above ? -h : above;
    }
  }
  below = fd::wave_max(below), above = fd::wave_max(above);
  if (lane == 0) w_below[wave] = below, w_above[wave] = above;
  __syncthreads();
  for (int round = 0; round < C_ROUNDS; ++round) {
    // (in place: whatever a racing read returns is an ancestor, so every round at least doubles the links a path has collapsed)
    for (int id = tid; id < M + nm; id += CT) {
      const int p = par[id];
      if (p >= 0) {
        const int pp = par[p];
        if (pp >= 0) par[id] = pp;
      }
    }
    __syncthreads();
  }
  // clusters numbered by their smallest member
  if (tid == 0) {
    int K = 0;
    for (int i = 0; i < M; ++i) {
      if (lab[i] == NONE) continue;
      const int r = par[i] >= 0 ? par[i] : i;
      if (clab[r] == NONE) {
        clab[r] = (unsigned short)K;
        members[K] = 0;
        ++K;
      }
      lab[i] = clab[r];
    }
    n_clusters = K;
  }
  __syncthreads();
  const int K = n_clusters;
  // every leaf against the other members of its cluster, in index order
  for (int i = tid; i < M; i += CT) {
    const unsigned short c = lab[i];
    double sum = 0.0, up = 0.0;
    if (c != NONE) {
      for (int j = 0; j < i; ++j)
        if (lab[j] == c) sum += A[(long)j * ld + i];
      const double* row = A + (long)i * ld;
      for (int j = i + 1; j < M; ++j)
        if (lab[j] == c) {
          const double v = row[j];
          sum += v;
          up += v;
        }
    }
    score[i] = sum, upper[i] = up;
    labels[g * M + i] = c == NONE ? -1 : (int)c;
  }
  __syncthreads();
  if (tid == 0) {
    int n = 0;
    double within = 0.0;
    for (int i = 0; i < M; ++i) {
      const unsigned short c = lab[i];
      if (c == NONE) continue;
      ++n;
      within += upper[i];
      if (members[c] == 0) medoid[c] = (unsigned short)i;
      else if (kind ? score[i] > score[medoid[c]] : score[i] < score[medoid[c]]) medoid[c] = (unsigned short)i;
      ++members[c];
    }
    long pairs = 0;
    int largest = 0, singletons = 0;
    for (int c = 0; c < K; ++c) {
      const int m = members[c];
      pairs += (long)m * (m - 1) / 2;
      largest = m > largest ? m : largest;
      singletons += m == 1;
    }
    double lo = -INFINITY, hi = -INFINITY;
    for (int w = 0; w < CW; ++w) lo = w_below[w] > lo ? w_below[w] : lo, hi = w_above[w] > hi ? w_above[w] : hi;
    double* o = out + g * FD_CLUSTER_SLOTS;
    o[0] = (double)n;
    o[1] = (double)K;
    o[2] = n ? (double)K / (double)n : (double)NAN;
    o[3] = (double)largest;
    o[4] = (double)singletons;
    o[5] = pairs ? within / (double)pairs : (double)NAN;
    o[6] = lo == -INFINITY ? (double)NAN : lo;
    o[7] = hi == -INFINITY ? (double)NAN : -hi;
  }
  __syncthreads();
  for (int k = tid; k < M; k += CT) rep[g * M + k] = k < K ? (int)medoid[k] : -1;
}

}  // namespace

extern "C" int fd_cluster_linkage(const double* mat, long ld, long problem_stride, const unsigned char* present, int G, int M,
                                  int kind, int method, double* ws, double* Z, int* num_merges, void* stream) {
  static_assert(C_MAX_M == FD_CLUSTER_MAX_M && FD_CLUSTER_WS_DOUBLES(3) == 9, "include/fd_hip.h");
  FD_CHECK_ARG(G >= 0 && M >= 0, "fd_cluster_linkage: negative size");
  FD_CHECK_ARG(M <= C_MAX_M, "fd_cluster_linkage: M must be at most 4096");
  FD_CHECK_ARG(kind == 0 || kind == 1, "fd_cluster_linkage: kind must be 0 (distance) or 1 (similarity)");
  FD_CHECK_ARG(method >= 0 && method <= 2, "fd_cluster_linkage: method must be 0 (single), 1 (average) or 2 (complete)");
  if (G == 0 || M == 0) return FD_OK;
  FD_CHECK_ARG(mat && ws && num_merges && (Z || M == 1), "fd_cluster_linkage: null operand");
  FD_CHECK_ARG(ld >= M && (G == 1 || problem_stride >= 0), "fd_cluster_linkage: ld must be at least M and problem_stride non-negative");
  FD_CHECK_ARG((((uintptr_t)mat) & 7u) == 0 && (((uintptr_t)ws) & 7u) == 0 && (((uintptr_t)Z) & 7u) == 0 &&
                   (((uintptr_t)num_merges) & 3u) == 0,
               "fd_cluster_linkage: misaligned operand");
  FD_CHECK_ARG(G < (1 << 24), "fd_cluster_linkage: G must be below 2^24 (blocks in one grid)");
  hipLaunchKernelGGL(linkage_kernel, dim3((unsigned)G), dim3(CT), 0, (hipStream_t)stream, mat, ld, problem_stride, present, M, kind,
                     method, ws, Z, num_merges);
  FD_CHECK_LAUNCH("fd_cluster_linkage");
  return FD_OK;
}

extern "C" int fd_cluster_cut(const double* Z, const int* num_merges, const double* mat, long ld, long problem_stride,
                              const unsigned char* present, int G, int M, int kind, double cut, int* labels, int* rep, double* out,
                              void* stream) {
  FD_CHECK_ARG(G >= 0 && M >= 0, "fd_cluster_cut: negative size");
  FD_CHECK_ARG(M <= C_MAX_M, "fd_cluster_cut: M must be at most 4096");
  FD_CHECK_ARG(kind == 0 || kind == 1, "fd_cluster_cut: kind must be 0 (distance) or 1 (similarity)");
  FD_CHECK_ARG(cut == cut, "fd_cluster_cut: the cut is NaN");
  if (G == 0 || M == 0) return FD_OK;
  FD_CHECK_ARG(mat && num_merges && labels && rep && out && (Z || M == 1), "fd_cluster_cut: null operand");
  FD_CHECK_ARG(ld >= M && (G == 1 || problem_stride >= 0), "fd_cluster_cut: ld must be at least M and problem_stride non-negative");
  FD_CHECK_ARG((((uintptr_t)mat) & 7u) == 0 && (((uintptr_t)Z) & 7u) == 0 && (((uintptr_t)out) & 7u) == 0 &&
                   (((uintptr_t)num_merges) & 3u) == 0 && (((uintptr_t)labels) & 3u) == 0 && (((uintptr_t)rep) & 3u) == 0,
               "fd_cluster_cut: misaligned operand");
  FD_CHECK_ARG(G < (1 << 24), "fd_cluster_cut: G must be below 2^24 (blocks in one grid)");
  hipLaunchKernelGGL(cut_kernel, dim3((unsigned)G), dim3(CT), 0, (hipStream_t)stream, Z, num_merges, mat, ld, problem_stride, present,
                     M, kind, cut, labels, rep, out);
  FD_CHECK_LAUNCH("fd_cluster_cut");
  return FD_OK;
}
