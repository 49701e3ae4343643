// fd_design: inference of the reference's vanilla (full-backbone) ProteinMPNN (ProteinMPNN/protein_mpnn_utils.py:574-714,
// 899-1168) on packed single chains: graph features, the three encoder layers and the autoregressive decoder with sampling and
// scoring.  include/fd_hip.h is the specification (layouts of the packed weights, the order of every sum that matters to a
// caller); this file says how the launches are laid out.
//
// Every product is an fp32 product with an fp32 sum: the per-edge 128-wide Linears run on v_mfma_f32_16x16x4_f32 (a k-ordered
// fmaf chain per output), the matrix-vector products of one node are fmaf chains on the vector ALU.  No bf16 / fp16 operand.
//
// mm_tiles             the one per-edge product: rows = the K <= 64 edges of one residue, staged in LDS with a row stride of 132
//                      floats (the sixteen rows of an A fragment then fall into distinct banks), times a transposed weight
//                      [k][128] read from L2; wave w owns the output columns 32 w .. 32 w + 31 of up to four row tiles.
// mpnn_graph_kernel    one block per residue: CA distances to its chain in LDS, the K nearest by counting the residues in front
//                      under the key (distance, index), the 416 edge features sixteen edges at a time, edge_embedding, norm_edges
//                      and W_e.
// mpnn_enc_node_kernel one block per residue: W1 as A h_i + B e_ik + C h_j (A h_i + b1 and C h_j arrive as node products of the
//                      launch before), W2, the neighbour sum in registers, W3 behind the sum, norm1, the feed-forward, norm2, and
//                      the node products the next launches need.
// mpnn_enc_edge_kernel one block per residue: W11 (same split), W12, W13, norm3, h_E in place.
// mpnn_dec_prep_kernel one block per residue: W1b h_E + b1 of the three decoder layers.
// mpnn_decode_kernel   one block per (backbone, sequence) walks the decoding order inside the kernel.  Per step and layer: the
//                      first Linear is a sum of precomputed terms, W2 is the one per-edge product, the rest are matrix-vector
//                      products of one node.  W1d h_V^l[j] of the decoded positions lives in block-private global scratch, the
//                      letters and the ranks in LDS; __syncthreads() between dependent phases, nothing crosses blocks.
//
// A row depends on its own chain only, a sequence on its own block only: results are bitwise independent of the other backbones
// of the call, of the backbone's place among them and of num_seqs.
#include "fd_common.h"
#include "../../include/fd_hip.h"

#include <cmath>

namespace {

constexpr int DT = 256;                           // threads of a block
constexpr int H = FD_MPNN_HIDDEN;
constexpr int KMAX = FD_MPNN_MAX_K;
constexpr int LMAX = FD_MPNN_MAX_L;
constexpr int LDA = 132;                          // LDS row stride of an edge tile
constexpr int NPS = FD_MPNN_NODE_SLOTS * H;       // row stride of the node products
constexpr int NF = 416, LDF = 420;                // edge features and their LDS row stride
constexpr int NL = 21;                            // letters

// ---- packed weights (include/fd_hip.h) ----
constexpr int GW_MU = 0, GW_POS = GW_MU + 16, GW_WE = GW_POS + 66 * 16, GW_LNG = GW_WE + NF * H, GW_LNB = GW_LNG + H,
              GW_WET = GW_LNB + H, GW_BE = GW_WET + H * H, GW_SIZE = GW_BE + H;
constexpr int NU_W3 = 0, NU_B3 = NU_W3 + H * H, NU_LN1G = NU_B3 + H, NU_LN1B = NU_LN1G + H, NU_WIN = NU_LN1B + H,
              NU_BIN = NU_WIN + H * 4 * H, NU_WOUT = NU_BIN + 4 * H, NU_BOUT = NU_WOUT + 4 * H * H, NU_LN2G = NU_BOUT + H,
              NU_LN2B = NU_LN2G + H, NU_SIZE = NU_LN2B + H;
constexpr int EW_W1B = 0, EW_W2 = EW_W1B + H * H, EW_B2 = EW_W2 + H * H, EW_NU = EW_B2 + H, EW_NPW = EW_NU + NU_SIZE,
              EW_NPB = EW_NPW + H * NPS, EW_W11B = EW_NPB + NPS, EW_W12 = EW_W11B + H * H, EW_B12 = EW_W12 + H * H,
              EW_W13 = EW_B12 + H, EW_B13 = EW_W13 + H * H, EW_LN3G = EW_B13 + H, EW_LN3B = EW_LN3G + H, EW_LAYER = EW_LN3B + H;
constexpr int EW_INIT = 0, EW_LAYERS = EW_INIT + H, EW_SIZE = EW_LAYERS + 3 * EW_LAYER;
constexpr int DL_W1A = 0, DL_W1D = DL_W1A + H * H, DL_TS = DL_W1D + H * H, DL_W2 = DL_TS + NL * H, DL_B2 = DL_W2 + H * H,
              DL_NU = DL_B2 + H, DL_LAYER = DL_NU + NU_SIZE;
constexpr int DW_W1B = 0, DW_B1 = DW_W1B + 3 * H * H, DW_LAYERS = DW_B1 + 3 * H, DW_WOUT = DW_LAYERS + 3 * DL_LAYER,
              DW_BOUT = DW_WOUT + H * NL, DW_SIZE = DW_BOUT + NL;
static_assert(NU_SIZE % 4 == 0 && EW_LAYERS % 4 == 0 && EW_LAYER % 4 == 0 && EW_NU % 4 == 0 && DW_LAYERS % 4 == 0 &&
                  DL_LAYER % 4 == 0 && DL_W1D % 4 == 0 && DL_NU % 4 == 0 && NU_WIN % 4 == 0 && NU_WOUT % 4 == 0,
              "the matrix-vector products read their weights by 16-byte loads");
static_assert(GW_SIZE == FD_MPNN_GRAPH_FLOATS && EW_SIZE == FD_MPNN_ENC_FLOATS && DW_SIZE == FD_MPNN_DEC_FLOATS,
              "fd_hip.h states the sizes of the packed weights");

__device__ __forceinline__ float gelu(float x) { return (0.5f * x) * (1.0f + erff(x * 0.70710678118654752f)); }

__device__ __forceinline__ f32x4 zero4() {
  f32x4 z;
  z[0] = 0.f, z[1] = 0.f, z[2] = 0.f, z[3] = 0.f;
  return z;
}

// acc[rt][c2] += A[16 rt + i][k] Wt[k][32 wave + 16 c2 + j] over k < kdim (a multiple of 4) for the row tiles rt < nrt.
// Element e of acc[rt][c2] is row 16 rt + 4 (lane >> 4) + e, column 32 wave + 16 c2 + (lane & 15).  nrt is block-uniform.
template <int RT>
__device__ __forceinline__ void mm_tiles(const float* sA, int lda, int nrt, const float* __restrict__ Wt, int kdim,
                                         f32x4 (&acc)[RT][2]) {
  const int lane = fd::lane_id(), wave = fd::wave_id();
  const int r = lane & 15, q = lane >> 4;
  const float* wp = Wt + (long)q * H + wave * 32 + r;
  const float* ap = sA + r * lda + q;
#pragma unroll 4
  for (int k = 0; k < kdim; k += 4) {      // (unrolled: the weight loads of four k-steps are in flight together)
    const float b0 = wp[(long)k * H], b1 = wp[(long)k * H + 16];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      if (rt < nrt) {
        const float a = ap[rt * 16 * lda + k];
        acc[rt][0] = fd::mfma_16x16x4(a, b0, acc[rt][0]);
        acc[rt][1] = fd::mfma_16x16x4(a, b1, acc[rt][1]);
      }
    }
  }
}

// f(row, column, value) for every element of A Wt this lane holds
template <int RT, class F>
__device__ __forceinline__ void mm_apply(const float* sA, int lda, int nrt, const float* __restrict__ Wt, int kdim, F f) {
  f32x4 acc[RT][2];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) acc[rt][0] = zero4(), acc[rt][1] = zero4();
  mm_tiles<RT>(sA, lda, nrt, Wt, kdim, acc);
  const int lane = fd::lane_id(), wave = fd::wave_id();
  const int r = lane & 15, q = lane >> 4;
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    if (rt < nrt) {
#pragma unroll
      for (int c2 = 0; c2 < 2; ++c2)
#pragma unroll
        for (int e = 0; e < 4; ++e) f(rt * 16 + 4 * q + e, wave * 32 + c2 * 16 + r, acc[rt][c2][e]);
    }
  }
}

// sum[c] = sum over the rows r < Ke of gelu((A Wt)[r][c] + bias[c]): each lane adds its rows in ascending order, then the four
// lane groups of a column meet in two butterfly steps (16, 32)
__device__ __forceinline__ void mm_gelu_colsum(const float* sA, int nrt, int Ke, const float* __restrict__ Wt,
                                               const float* __restrict__ bias, float* sum) {
  f32x4 acc[4][2];
#pragma unroll
  for (int rt = 0; rt < 4; ++rt) acc[rt][0] = zero4(), acc[rt][1] = zero4();
  mm_tiles<4>(sA, LDA, nrt, Wt, H, acc);
  const int lane = fd::lane_id(), wave = fd::wave_id();
  const int r = lane & 15, q = lane >> 4;
#pragma unroll
  for (int c2 = 0; c2 < 2; ++c2) {
    const int col = wave * 32 + c2 * 16 + r;
    const float b = bias[col];
    float s = 0.f;
#pragma unroll
    for (int rt = 0; rt < 4; ++rt) {
      if (rt < nrt) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (rt * 16 + 4 * q + e < Ke) s += gelu(acc[rt][c2][e] + b);
      }
    }
    s += __shfl_xor(s, 16);
    s += __shfl_xor(s, 32);
    if (q == 0) sum[col] = s;
  }
}

// ---- one node: W3 behind the neighbour sum, norm1, the feed-forward, norm2 ----
struct NodeLds {
  float sum[H];                                   // sum over the neighbours of the message before W3
  float hv[H];                                    // h_V of the node: input, then output
  float part[8 * H];                              // partial sums of a matrix-vector product: [slices][outputs]
  float x[H];
  float ff[4 * H];
};

// out[e] = sum over i < n of w[i ldw + e] x[i], i ascending, e < 4: four adjacent outputs over one slice of the inputs, the
// weights by 16-byte loads (w is 16-byte aligned: every block of the packed weights starts at a multiple of four floats)
__device__ __forceinline__ void dot4(const float* x, int n, const float* __restrict__ w, int ldw, float* out) {
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll 8
  for (int i = 0; i < n; ++i) {
    const float4 v = *reinterpret_cast<const float4*>(w + (long)i * ldw);
    const float xi = x[i];
    a0 = fmaf(v.x, xi, a0), a1 = fmaf(v.y, xi, a1), a2 = fmaf(v.z, xi, a2), a3 = fmaf(v.w, xi, a3);
  }
  out[0] = a0, out[1] = a1, out[2] = a2, out[3] = a3;
}

// part[s][c] = sum over the inputs i of slice s of Wt[i][c] x[i]: G groups of four outputs, 256 / G slices of the n_in inputs.
// The caller adds the slices in ascending order (slice_sum).
template <int G>
__device__ __forceinline__ void matvec_slices(const float* x, int n_in, const float* __restrict__ Wt, float* part) {
  constexpr int SL = DT / G;
  const int tid = (int)threadIdx.x, g = tid % G, sl = tid / G;
  const int n = n_in / SL;
  dot4(x + sl * n, n, Wt + (long)(sl * n) * (4 * G) + 4 * g, 4 * G, part + sl * (4 * G) + 4 * g);
}
template <int SL>
__device__ __forceinline__ float slice_sum(const float* part, int n_out, int c) {
  float v = part[c];
#pragma unroll
  for (int sl = 1; sl < SL; ++sl) v += part[sl * n_out + c];
  return v;
}

// LayerNorm over 128 values, two per lane of one wave (columns lane and lane + 64); eps = 1e-5, biased variance
__device__ __forceinline__ void wave_layernorm(float v0, float v1, const float* __restrict__ g, const float* __restrict__ b,
                                               int lane, float& y0, float& y1) {
  const float mean = fd::wave_sum(v0 + v1) * (1.0f / H);
  const float d0 = v0 - mean, d1 = v1 - mean;
  const float var = fd::wave_sum(d0 * d0 + d1 * d1) * (1.0f / H);
  const float rs = 1.0f / sqrtf(var + 1e-5f);
  y0 = (d0 * rs) * g[lane] + b[lane];
  y1 = (d1 * rs) * g[lane + 64] + b[lane + 64];
}

// nl.hv <- norm2(x + FF(x)), x = norm1(nl.hv + (W3 nl.sum + Ke b3) / 30).  Called by the whole block; ends behind a barrier.
__device__ __forceinline__ void node_update(NodeLds& nl, const float* __restrict__ nu, int Ke) {
  const int tid = (int)threadIdx.x, lane = fd::lane_id(), wave = fd::wave_id();
  matvec_slices<32>(nl.sum, H, nu + NU_W3, nl.part);
  __syncthreads();
  if (wave == 0) {
    float v[2], y0, y1;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int c = lane + 64 * u;
      const float m = slice_sum<8>(nl.part, H, c) + (float)Ke * nu[NU_B3 + c];
      v[u] = nl.hv[c] + m / 30.0f;
    }
    wave_layernorm(v[0], v[1], nu + NU_LN1G, nu + NU_LN1B, lane, y0, y1);
    nl.x[lane] = y0, nl.x[lane + 64] = y1;
  }
  __syncthreads();
  matvec_slices<128>(nl.x, H, nu + NU_WIN, nl.part);
  __syncthreads();
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int c = tid + DT * u;
    nl.ff[c] = gelu(slice_sum<2>(nl.part, 4 * H, c) + nu[NU_BIN + c]);
  }
  __syncthreads();
  matvec_slices<32>(nl.ff, 4 * H, nu + NU_WOUT, nl.part);
  __syncthreads();
  if (wave == 0) {
    float v[2], y0, y1;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int c = lane + 64 * u;
      v[u] = nl.x[c] + (slice_sum<8>(nl.part, H, c) + nu[NU_BOUT + c]);
    }
    wave_layernorm(v[0], v[1], nu + NU_LN2G, nu + NU_LN2B, lane, y0, y1);
    nl.hv[lane] = y0, nl.hv[lane + 64] = y1;
  }
  __syncthreads();
}

// the chain of a row: offset, length, neighbours in use
struct RowInfo {
  long off;
  int L, Ke, nrt;
};
__device__ __forceinline__ RowInfo row_info(const long* __restrict__ offsets, const int* __restrict__ chain_of, long row, int K) {
  RowInfo ri;
  const int b = chain_of[row];
  ri.off = offsets[b];
  const long L = offsets[b + 1] - ri.off;
  ri.L = (int)(L < LMAX ? L : LMAX);              // (the host refused longer chains; this only bounds the LDS arrays)
  ri.Ke = K < ri.L ? K : ri.L;
  ri.nrt = (ri.Ke + 15) >> 4;
  return ri;
}

// an entry of E_idx, kept inside the chain whatever the table holds
__device__ __forceinline__ int neighbour(int j, int L) { return j < 0 ? 0 : (j >= L ? L - 1 : j); }

// the edges of one residue, rows of 128, zero behind Ke
__device__ __forceinline__ void load_edges(const float* __restrict__ h_E, long row, int K, int Ke, int nrt, float* sA) {
  for (int idx = (int)threadIdx.x; idx < nrt * 16 * H; idx += DT) {
    const int r = idx >> 7, c = idx & (H - 1);
    sA[r * LDA + c] = r < Ke ? h_E[(row * K + r) * H + c] : 0.f;
  }
}

// ---- graph features ----
__device__ __forceinline__ void with_cb(const float* __restrict__ a, float* p) {
#pragma unroll
  for (int k = 0; k < 12; ++k) p[k] = a[k];
  float b[3], c[3], x[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) b[d] = p[3 + d] - p[d], c[d] = p[6 + d] - p[3 + d];
  x[0] = b[1] * c[2] - b[2] * c[1];
  x[1] = b[2] * c[0] - b[0] * c[2];
  x[2] = b[0] * c[1] - b[1] * c[0];
#pragma unroll
  for (int d = 0; d < 3; ++d) p[12 + d] = ((-0.58273431f * x[d] + 0.56802827f * b[d]) - 0.54067466f * c[d]) + p[3 + d];
}

// atom of the residue itself (high nibble) and of the neighbour (low nibble) of the 25 distance sets, in the reference's order
// (N 0, CA 1, C 2, O 3, CB 4)
__device__ const unsigned char kPairs[25] = {0x11, 0x00, 0x22, 0x33, 0x44, 0x10, 0x12, 0x13, 0x14, 0x02, 0x03, 0x04, 0x42,
                                             0x43, 0x32, 0x01, 0x21, 0x31, 0x41, 0x20, 0x30, 0x40, 0x24, 0x34, 0x23};

__global__ __launch_bounds__(DT) void mpnn_graph_kernel(const float* __restrict__ atoms, const int* __restrict__ res_index,
                                                        const long* __restrict__ offsets, const int* __restrict__ chain_of, int K,
                                                        const float* __restrict__ gw, int* __restrict__ E_idx,
                                                        float* __restrict__ h_E) {
  __shared__ float s_d[LMAX];
  __shared__ int s_idx[KMAX];
  __shared__ float s_self[15];
  __shared__ float s_at[KMAX][15];
  __shared__ int s_dres[KMAX];
  __shared__ float sF[16 * LDF];
  __shared__ float sB[KMAX * LDA];
  const int tid = (int)threadIdx.x, lane = fd::lane_id(), wave = fd::wave_id();
  const long row = (long)blockIdx.x;
  const RowInfo ri = row_info(offsets, chain_of, row, K);
  const int L = ri.L, Ke = ri.Ke, nrt = ri.nrt;
  const float* ca_i = atoms + row * 12 + 3;

  for (int j = tid; j < L; j += DT) {
    const float* ca_j = atoms + (ri.off + j) * 12 + 3;
    const float dx = ca_j[0] - ca_i[0], dy = ca_j[1] - ca_i[1], dz = ca_j[2] - ca_i[2];
    s_d[j] = sqrtf(((dx * dx + dy * dy) + dz * dz) + 1e-6f);
  }
  if (tid == 0) with_cb(atoms + row * 12, s_self);
  if (tid < KMAX) s_idx[tid] = tid < L ? tid : 0;   // (a NaN coordinate leaves places unfilled: every entry stays a residue of the chain)
  __syncthreads();
  // the place of residue j among all of them under (distance, index): the number of residues in front of it
  for (int j = tid; j < L; j += DT) {
    const float dj = s_d[j];
    int cnt = 0;
    for (int m = 0; m < L; ++m) {
      const float dm = s_d[m];
      cnt += (dm < dj || (dm == dj && m < j)) ? 1 : 0;
    }
    if (cnt < Ke) s_idx[cnt] = j;
  }
  __syncthreads();
  if (tid < K) E_idx[row * K + tid] = tid < Ke ? s_idx[tid] : -1;
  if (tid < Ke) {
    const long rj = ri.off + s_idx[tid];
    with_cb(atoms + rj * 12, s_at[tid]);
    int d = res_index[row] - res_index[rj] + 32;
    s_dres[tid] = d < 0 ? 0 : (d > 64 ? 64 : d);
  }
  for (int idx = tid; idx < (K - Ke) * H; idx += DT) h_E[(row * K + Ke) * H + idx] = 0.f;
  __syncthreads();

  for (int rt = 0; rt < nrt; ++rt) {
    for (int idx = tid; idx < 16 * 26; idx += DT) {
      const int e = idx / 26, p = idx - e * 26, k = rt * 16 + e;
      float* f = sF + e * LDF;
      if (k >= Ke) {
#pragma unroll
        for (int m = 0; m < 16; ++m) f[p * 16 + m] = 0.f;
      } else if (p == 25) {
        const float* pt = gw + GW_POS + s_dres[k] * 16;
#pragma unroll
        for (int m = 0; m < 16; ++m) f[m] = pt[m];
      } else {
        const int pa = kPairs[p] >> 4, pb = kPairs[p] & 15;
        const float* A = s_self + 3 * pa;
        const float* Bq = s_at[k] + 3 * pb;
        const float dx = A[0] - Bq[0], dy = A[1] - Bq[1], dz = A[2] - Bq[2];
        const float D = sqrtf(((dx * dx + dy * dy) + dz * dz) + 1e-6f);
#pragma unroll
        for (int m = 0; m < 16; ++m) {
          const float z = (D - gw[GW_MU + m]) / 1.25f;
          f[16 + p * 16 + m] = expf(-(z * z));
        }
      }
    }
    __syncthreads();
    mm_apply<1>(sF, LDF, 1, gw + GW_WE, NF, [&](int r, int c, float v) { sB[(rt * 16 + r) * LDA + c] = v; });
    __syncthreads();
  }
  for (int r = wave; r < Ke; r += DT / 64) {      // norm_edges
    float y0, y1;
    wave_layernorm(sB[r * LDA + lane], sB[r * LDA + lane + 64], gw + GW_LNG, gw + GW_LNB, lane, y0, y1);
    sB[r * LDA + lane] = y0, sB[r * LDA + lane + 64] = y1;
  }
  __syncthreads();
  mm_apply<4>(sB, LDA, nrt, gw + GW_WET, H, [&](int r, int c, float v) {
    if (r < Ke) h_E[(row * K + r) * H + c] = v + gw[GW_BE + c];
  });
}

// ---- encoder ----
__global__ __launch_bounds__(DT) void mpnn_enc_init_kernel(const float* __restrict__ ew, float* __restrict__ np, long T) {
  const long i = (long)blockIdx.x * DT + threadIdx.x;
  if (i >= T * 2 * H) return;
  const long row = i / (2 * H);
  const int c = (int)(i - row * 2 * H);
  np[row * NPS + 2 * H + c] = c < H ? ew[EW_INIT + c] : 0.f;      // h_V = 0: W1a h_i + b1 = b1, W1c h_j = 0
}

// node products: out[s H + c] = NPb[s H + c] + sum_i NPw[i][s H + c] hv[i], s < ns
__device__ __forceinline__ void node_products(const float* hv, const float* __restrict__ w, const float* __restrict__ b, int ns,
                                              float* __restrict__ out) {
  for (int col = (int)threadIdx.x; col < ns * H; col += DT) {
    float acc = b[col];
#pragma unroll 8
    for (int i = 0; i < H; ++i) acc = fmaf(w[(long)i * NPS + col], hv[i], acc);
    out[col] = acc;
  }
}

__global__ __launch_bounds__(DT) void mpnn_enc_node_kernel(const int* __restrict__ E_idx, const long* __restrict__ offsets,
                                                           const int* __restrict__ chain_of, int K, const float* __restrict__ w,
                                                           const float* __restrict__ np_in, float* __restrict__ np_out, int ns,
                                                           float* __restrict__ h_V, const float* __restrict__ h_E, int first) {
  __shared__ float sA[KMAX * LDA];
  __shared__ float sB[KMAX * LDA];
  __shared__ NodeLds nl;
  __shared__ long s_j[KMAX];
  const int tid = (int)threadIdx.x;
  const long row = (long)blockIdx.x;
  const RowInfo ri = row_info(offsets, chain_of, row, K);
  const int Ke = ri.Ke, nrt = ri.nrt;
  load_edges(h_E, row, K, Ke, nrt, sA);
  if (tid < KMAX) s_j[tid] = tid < Ke ? ri.off + neighbour(E_idx[row * K + tid], ri.L) : row;
  if (tid < H) nl.hv[tid] = first ? 0.f : h_V[row * H + tid];
  __syncthreads();
  const float* pa = np_in + row * NPS + 2 * H;
  mm_apply<4>(sA, LDA, nrt, w + EW_W1B, H, [&](int r, int c, float v) {
    sB[r * LDA + c] = gelu((v + pa[c]) + np_in[s_j[r] * NPS + 3 * H + c]);
  });
  __syncthreads();
  mm_gelu_colsum(sB, nrt, Ke, w + EW_W2, w + EW_B2, nl.sum);
  __syncthreads();
  node_update(nl, w + EW_NU, Ke);
  if (tid < H) h_V[row * H + tid] = nl.hv[tid];
  node_products(nl.hv, w + EW_NPW, w + EW_NPB, ns, np_out + row * NPS);
}

__global__ __launch_bounds__(DT) void mpnn_enc_edge_kernel(const int* __restrict__ E_idx, const long* __restrict__ offsets,
                                                           const int* __restrict__ chain_of, int K, const float* __restrict__ w,
                                                           const float* __restrict__ np, float* __restrict__ h_E) {
  __shared__ float sA[KMAX * LDA];
  __shared__ float sB[KMAX * LDA];
  __shared__ long s_j[KMAX];
  const int tid = (int)threadIdx.x, lane = fd::lane_id(), wave = fd::wave_id();
  const long row = (long)blockIdx.x;
  const RowInfo ri = row_info(offsets, chain_of, row, K);
  const int Ke = ri.Ke, nrt = ri.nrt;
  load_edges(h_E, row, K, Ke, nrt, sA);
  if (tid < KMAX) s_j[tid] = tid < Ke ? ri.off + neighbour(E_idx[row * K + tid], ri.L) : row;
  __syncthreads();
  const float* pa = np + row * NPS;
  mm_apply<4>(sA, LDA, nrt, w + EW_W11B, H, [&](int r, int c, float v) {
    sB[r * LDA + c] = gelu((v + pa[c]) + np[s_j[r] * NPS + H + c]);
  });
  __syncthreads();
  mm_apply<4>(sB, LDA, nrt, w + EW_W12, H, [&](int r, int c, float v) { sA[r * LDA + c] = gelu(v + w[EW_B12 + c]); });
  __syncthreads();
  mm_apply<4>(sA, LDA, nrt, w + EW_W13, H, [&](int r, int c, float v) {
    sB[r * LDA + c] = r < Ke ? h_E[(row * K + r) * H + c] + (v + w[EW_B13 + c]) : 0.f;
  });
  __syncthreads();
  for (int r = wave; r < Ke; r += DT / 64) {      // norm3
    float y0, y1;
    wave_layernorm(sB[r * LDA + lane], sB[r * LDA + lane + 64], w + EW_LN3G, w + EW_LN3B, lane, y0, y1);
    h_E[(row * K + r) * H + lane] = y0, h_E[(row * K + r) * H + lane + 64] = y1;
  }
}

__global__ __launch_bounds__(DT) void mpnn_dec_prep_kernel(const long* __restrict__ offsets, const int* __restrict__ chain_of, int K,
                                                           long T, const float* __restrict__ dw, const float* __restrict__ h_E,
                                                           float* __restrict__ EB) {
  __shared__ float sA[KMAX * LDA];
  const long row = (long)blockIdx.x;
  const RowInfo ri = row_info(offsets, chain_of, row, K);
  const int Ke = ri.Ke, nrt = ri.nrt;
  load_edges(h_E, row, K, Ke, nrt, sA);
  __syncthreads();
  for (int l = 0; l < 3; ++l) {
    float* out = EB + ((long)l * T + row) * K * H;
    const float* b = dw + DW_B1 + l * H;
    mm_apply<4>(sA, LDA, nrt, dw + DW_W1B + l * H * H, H, [&](int r, int c, float v) {
      if (r < Ke) out[r * H + c] = v + b[c];
    });
  }
}

// ---- decoder ----
__global__ __launch_bounds__(DT) void mpnn_decode_kernel(const int* __restrict__ E_idx, const long* __restrict__ offsets, int K,
                                                         long T, const float* __restrict__ dw, const float* __restrict__ h_V,
                                                         const float* __restrict__ npd, const float* __restrict__ EB,
                                                         const int* __restrict__ order, const int* __restrict__ S_in,
                                                         const unsigned char* __restrict__ fixed, const float* __restrict__ uni,
                                                         const float* __restrict__ omit, const float* __restrict__ bias,
                                                         float temperature, int forced, float* __restrict__ scratch,
                                                         int* __restrict__ S_out, float* __restrict__ log_probs,
                                                         float* __restrict__ probs) {
  __shared__ float sA[KMAX * LDA];
  __shared__ NodeLds nl;
  __shared__ float s_a[H];
  __shared__ float s_logit[32];
  __shared__ short s_rank[LMAX];
  __shared__ unsigned char s_S[LMAX];
  __shared__ int s_j[KMAX];
  __shared__ unsigned char s_bw[KMAX];
  const int tid = (int)threadIdx.x;
  const long off = offsets[blockIdx.x];
  const long Lfull = offsets[blockIdx.x + 1] - off;
  const int L = (int)(Lfull < LMAX ? Lfull : LMAX);
  const int Ke = K < L ? K : L, nrt = (Ke + 15) >> 4;
  const long sq = (long)blockIdx.y * T + off;     // this sequence's first row in the [num_seqs, T] arrays
  float* pd = scratch + sq * 2 * H;               // W1d h_V^l[j], l = 1, 2, of the decoded positions: [L][2][128]

  for (int j = tid; j < L; j += DT) s_rank[j] = 0x7fff, s_S[j] = 0;
  __syncthreads();
  for (int k = tid; k < L; k += DT) {
    const int p = order[sq + k];
    if (p >= 0 && p < L) s_rank[p] = (short)k;
  }
  __syncthreads();

  for (int step = 0; step < L; ++step) {
    const int t = order[sq + step];
    if (t < 0 || t >= L) continue;                // (not a permutation: the host's to refuse; block-uniform)
    const long row = off + t;
    if (tid < Ke) {
      const int j = neighbour(E_idx[row * K + tid], L);
      s_j[tid] = j;
      s_bw[tid] = s_rank[j] < step ? 1 : 0;
    }
    if (tid < H) nl.hv[tid] = h_V[row * H + tid], s_a[tid] = npd[row * NPS + 5 * H + tid];
    __syncthreads();
    for (int l = 0; l < 3; ++l) {
      const float* w = dw + DW_LAYERS + l * DL_LAYER;
      const float* eb = EB + ((long)l * T + row) * K * H;
      for (int idx = tid; idx < nrt * 16 * H; idx += DT) {
        const int r = idx >> 7, c = idx & (H - 1);
        float m = 0.f;
        if (r < Ke) {
          const int j = s_j[r];
          float v = s_a[c] + eb[r * H + c];
          if (s_bw[r]) {
            const float hvj = l == 0 ? npd[(off + j) * NPS + 2 * H + c] : pd[((long)j * 2 + (l - 1)) * H + c];
            v = (v + w[DL_TS + (int)s_S[j] * H + c]) + hvj;
          } else {
            v = v + npd[(off + j) * NPS + (2 + l) * H + c];
          }
          m = gelu(v);
        }
        sA[r * LDA + c] = m;
      }
      __syncthreads();
      mm_gelu_colsum(sA, nrt, Ke, w + DL_W2, w + DL_B2, nl.sum);
      __syncthreads();
      node_update(nl, w + DL_NU, Ke);
      if (l < 2) {
        // W1a h_V^{l+1}[t] for the next layer of this step, W1d h_V^{l+1}[t] for the later steps that see t as a neighbour
        // (64 groups of four outputs -- 32 of W1a, 32 of W1d -- times four slices of 32 inputs)
        const int g = tid & 63, sl = tid >> 6;
        const float* wn = dw + DW_LAYERS + (l + 1) * DL_LAYER + (g < 32 ? DL_W1A : DL_W1D) + (long)(sl * 32) * H + 4 * (g & 31);
        dot4(nl.hv + sl * 32, 32, wn, H, nl.part + sl * 2 * H + 4 * g);
        __syncthreads();
        const float acc = slice_sum<4>(nl.part, 2 * H, tid);
        if (tid < H) s_a[tid] = acc;
        else pd[((long)t * 2 + l) * H + (tid - H)] = acc;
        __syncthreads();
      }
    }
    if (tid < NL) {
      float acc = dw[DW_BOUT + tid];
      for (int i = 0; i < H; ++i) acc = fmaf(dw[DW_WOUT + i * NL + tid], nl.hv[i], acc);
      s_logit[tid] = acc;
    }
    __syncthreads();
    if (tid == 0) {
      const long o = (sq + t) * NL;
      float mx = s_logit[0];
      for (int a = 1; a < NL; ++a) mx = fmaxf(mx, s_logit[a]);
      float se = 0.f;
      for (int a = 0; a < NL; ++a) se += expf(s_logit[a] - mx);
      const float lse = logf(se);
      for (int a = 0; a < NL; ++a) log_probs[o + a] = (s_logit[a] - mx) - lse;
      float z[NL], zm = -INFINITY;
      for (int a = 0; a < NL; ++a) {
        z[a] = (s_logit[a] / temperature - omit[a] * 1e8f) + bias[a] / temperature;
        zm = fmaxf(zm, z[a]);
      }
      float zs = 0.f;
      for (int a = 0; a < NL; ++a) z[a] = expf(z[a] - zm), zs += z[a];
      const bool fix = !forced && fixed != nullptr && fixed[off + t] != 0;
      int letter = -1;
      if (forced || fix) letter = S_in[sq + t];
      const float u = (forced || fix) ? 0.f : uni[sq + t];
      float cum = 0.f;
      int last = 0;
      for (int a = 0; a < NL; ++a) {
        const float p = z[a] / zs;
        probs[o + a] = fix ? 0.f : p;
        cum += p;
        if (p > 0.f) last = a;
        if (letter < 0 && u < cum) letter = a;
      }
      if (letter < 0) letter = last;              // (u at or above the rounded total)
      letter = letter < 0 ? 0 : (letter > NL - 1 ? NL - 1 : letter);
      s_S[t] = (unsigned char)letter;
      S_out[sq + t] = letter;
    }
    __syncthreads();
  }
}

bool misaligned(const void* p, unsigned mask) { return (((uintptr_t)p) & mask) != 0; }

}  // namespace

extern "C" int fd_mpnn_graph(const float* atoms, const int* res_index, const long* offsets, const int* chain_of, long T, int K,
                             const float* gw, int* E_idx, float* h_E, void* stream) {
  FD_CHECK_ARG(T >= 0, "fd_mpnn_graph: negative size");
  FD_CHECK_ARG(K >= 1 && K <= KMAX, "fd_mpnn_graph: K must be 1..%d", KMAX);
  if (T == 0) return FD_OK;
  FD_CHECK_ARG(atoms && res_index && offsets && chain_of && gw && E_idx && h_E, "fd_mpnn_graph: null operand");
  FD_CHECK_ARG(!misaligned(atoms, 3) && !misaligned(res_index, 3) && !misaligned(offsets, 7) && !misaligned(chain_of, 3) &&
                   !misaligned(gw, 3) && !misaligned(E_idx, 3) && !misaligned(h_E, 3),
               "fd_mpnn_graph: misaligned operand");
  FD_CHECK_ARG(T < (1L << 24), "fd_mpnn_graph: T must be below 2^24 (blocks in one grid)");
  hipLaunchKernelGGL(mpnn_graph_kernel, dim3((unsigned)T), dim3(DT), 0, (hipStream_t)stream, atoms, res_index, offsets, chain_of, K,
                     gw, E_idx, h_E);
  FD_CHECK_LAUNCH("fd_mpnn_graph");
  return FD_OK;
}

extern "C" int fd_mpnn_encoder(const int* E_idx, const long* offsets, const int* chain_of, long T, int K, const float* ew,
                               const float* dw, float* h_V, float* h_E, float* node, float* node_ws, float* EB, void* stream) {
  FD_CHECK_ARG(T >= 0, "fd_mpnn_encoder: negative size");
  FD_CHECK_ARG(K >= 1 && K <= KMAX, "fd_mpnn_encoder: K must be 1..%d", KMAX);
  if (T == 0) return FD_OK;
  FD_CHECK_ARG(E_idx && offsets && chain_of && ew && dw && h_V && h_E && node && node_ws && EB, "fd_mpnn_encoder: null operand");
  FD_CHECK_ARG(node != node_ws, "fd_mpnn_encoder: node and node_ws must be two buffers");
  FD_CHECK_ARG(!misaligned(E_idx, 3) && !misaligned(offsets, 7) && !misaligned(chain_of, 3) && !misaligned(ew, 15) &&
                   !misaligned(dw, 15) && !misaligned(h_V, 3) && !misaligned(h_E, 3) && !misaligned(node, 3) &&
                   !misaligned(node_ws, 3) && !misaligned(EB, 3),
               "fd_mpnn_encoder: misaligned operand");
  FD_CHECK_ARG(T < (1L << 24), "fd_mpnn_encoder: T must be below 2^24 (blocks in one grid)");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(mpnn_enc_init_kernel, dim3((unsigned)fd_cdiv(T * 2 * H, DT)), dim3(DT), 0, st, ew, node_ws, T);
  FD_CHECK_LAUNCH("fd_mpnn_encoder");
  float* in = node_ws;
  float* out = node;
  for (int l = 0; l < 3; ++l) {
    const float* w = ew + EW_LAYERS + (long)l * EW_LAYER;
    hipLaunchKernelGGL(mpnn_enc_node_kernel, dim3((unsigned)T), dim3(DT), 0, st, E_idx, offsets, chain_of, K, w, (const float*)in,
                       out, l == 2 ? 6 : 4, h_V, (const float*)h_E, l == 0 ? 1 : 0);
    FD_CHECK_LAUNCH("fd_mpnn_encoder");
    hipLaunchKernelGGL(mpnn_enc_edge_kernel, dim3((unsigned)T), dim3(DT), 0, st, E_idx, offsets, chain_of, K, w, (const float*)out,
                       h_E);
    FD_CHECK_LAUNCH("fd_mpnn_encoder");
    float* tmp = in;
    in = out, out = tmp;
  }
  // (three layers: the last one wrote `node`)
  hipLaunchKernelGGL(mpnn_dec_prep_kernel, dim3((unsigned)T), dim3(DT), 0, st, offsets, chain_of, K, T, dw, (const float*)h_E, EB);
  FD_CHECK_LAUNCH("fd_mpnn_encoder");
  return FD_OK;
}

extern "C" int fd_mpnn_decode(const int* E_idx, const long* offsets, int B, long T, int K, int num_seqs, const float* dw,
                              const float* h_V, const float* node, const float* EB, const int* order, const int* S_in,
                              const unsigned char* fixed, const float* uniforms, const float* omit, const float* bias,
                              float temperature, int forced, float* scratch, int* S_out, float* log_probs, float* probs,
                              void* stream) {
  FD_CHECK_ARG(B >= 0 && T >= 0 && num_seqs >= 0, "fd_mpnn_decode: negative size");
  FD_CHECK_ARG(K >= 1 && K <= KMAX, "fd_mpnn_decode: K must be 1..%d", KMAX);
  if (B == 0 || T == 0 || num_seqs == 0) return FD_OK;
  FD_CHECK_ARG(E_idx && offsets && dw && h_V && node && EB && order && omit && bias && scratch && S_out && log_probs && probs,
               "fd_mpnn_decode: null operand");
  FD_CHECK_ARG(forced ? S_in != nullptr : uniforms != nullptr, "fd_mpnn_decode: forced needs S_in, sampling needs uniforms");
  FD_CHECK_ARG(forced || fixed == nullptr || S_in != nullptr, "fd_mpnn_decode: fixed positions need S_in");
  FD_CHECK_ARG(temperature > 0.f, "fd_mpnn_decode: temperature must be positive");
  FD_CHECK_ARG(!misaligned(E_idx, 3) && !misaligned(offsets, 7) && !misaligned(dw, 15) && !misaligned(h_V, 3) &&
                   !misaligned(node, 3) && !misaligned(EB, 3) && !misaligned(order, 3) && !misaligned(S_in, 3) &&
                   !misaligned(uniforms, 3) && !misaligned(omit, 3) && !misaligned(bias, 3) && !misaligned(scratch, 3) &&
                   !misaligned(S_out, 3) && !misaligned(log_probs, 3) && !misaligned(probs, 3),
               "fd_mpnn_decode: misaligned operand");
  FD_CHECK_ARG(B < (1 << 24) && num_seqs < 65536, "fd_mpnn_decode: B must be below 2^24 and num_seqs below 65536");
  hipLaunchKernelGGL(mpnn_decode_kernel, dim3((unsigned)B, (unsigned)num_seqs), dim3(DT), 0, (hipStream_t)stream, E_idx, offsets, K,
                     T, dw, h_V, node, EB, order, S_in, fixed, uniforms, omit, bias, temperature, forced, scratch, S_out, log_probs,
                     probs);
  FD_CHECK_LAUNCH("fd_mpnn_decode");
  return FD_OK;
}
