// The split-bf16 arithmetic of every fast GEMM-like kernel, defined ONCE: the exact split of fp32 values into three bf16
// planes and the order in which the six plane products are accumulated.  Uses only fd:: intrinsics (include after
// fd_intrin.h), so the interpreter build of tests/emu compiles it unchanged; header-only, in whatever namespace the
// including file stands.  tests/test_split_terms.py holds every user to the exact float64 result.
//
// x = x0 + x1 + x2 EXACTLY (round-to-nearest at every stage: 3 x (8 bits + the sign of the next residual) cover the 24-bit
// significand), so a * b = sum_{i,j} a_i * b_j with every term an exact bf16 product.  The six terms with i + j <= 2 are
// accumulated in fp32 by the bf16 MFMA, the small ones first; the three dropped terms are <= 2^-26 |a * b|.
#pragma once

// The two-value core.  A plane of a value pair (u, v) is t = fd::pack_bf16(u, v), the nearest bf16 pair (u in the low
// half); this takes it off and leaves the residuals in u, v.  pack, residual, pack, residual, pack: the three planes.
__device__ __forceinline__ void fd_split_residual(float& u, float& v, unsigned t) {
  u -= fd::bf16lo_f32(t);
  v -= fd::bf16hi_f32(t);
}

// four consecutive fp32 -> one uint2 per plane.  (Stage by stage across both pairs -- both packs, then the four
// residuals -- not pair by pair: the statement order decides the instruction order of the kernels that split on the way
// to LDS.)
__device__ __forceinline__ void fd_split4(float4 v, uint2& s0, uint2& s1, uint2& s2) {
  const unsigned h0 = fd::pack_bf16(v.x, v.y), h1 = fd::pack_bf16(v.z, v.w);
  fd_split_residual(v.x, v.y, h0);
  fd_split_residual(v.z, v.w, h1);
  const unsigned m0 = fd::pack_bf16(v.x, v.y), m1 = fd::pack_bf16(v.z, v.w);
  fd_split_residual(v.x, v.y, m0);
  fd_split_residual(v.z, v.w, m1);
  s0 = make_uint2(h0, h1);
  s1 = make_uint2(m0, m1);
  s2 = make_uint2(fd::pack_bf16(v.x, v.y), fd::pack_bf16(v.z, v.w));
}

// eight consecutive fp32 -> one uint4 (an MFMA operand's 8 k) per plane, pair by pair
__device__ __forceinline__ void fd_split8(const float (&x)[8], uint4& s0, uint4& s1, uint4& s2) {
  unsigned t0[4], t1[4], t2[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float u = x[2 * j], v = x[2 * j + 1];
    t0[j] = fd::pack_bf16(u, v);
    fd_split_residual(u, v, t0[j]);
    t1[j] = fd::pack_bf16(u, v);
    fd_split_residual(u, v, t1[j]);
    t2[j] = fd::pack_bf16(u, v);
  }
  s0 = make_uint4(t0[0], t0[1], t0[2], t0[3]);
  s1 = make_uint4(t1[0], t1[1], t1[2], t1[3]);
  s2 = make_uint4(t2[0], t2[1], t2[2], t2[3]);
}

// Product p of a k-step multiplies plane FD_PA[p] of A by plane FD_PB[p] of B: the pairs with i + j <= 2, smallest first.
// (fp32 accumulation order is observable: the grouped weight-gradient kernels walk the same six pairs plane-major,
// dw_mma6 in fd_pair_dw_common.h, and keep that order.)
constexpr int FD_PA[6] = {2, 1, 0, 1, 0, 0};
constexpr int FD_PB[6] = {0, 1, 2, 0, 1, 0};

// acc[i][j] += A_i * B_j for the TM x TN 32 x 32 blocks of a wave tile over one 16-k step (v_mfma_f32_32x32x16_bf16);
// fa[i][s] / fb[j][s] = plane s of the block's operand fragment.  The accumulators are interleaved inside a product, so
// that dependent MFMAs are TM * TN issues apart.  TRANS: transposed accumulation (B is the MFMA's row operand).
template <bool TRANS, int TM, int TN>
__device__ __forceinline__ void fd_mma6(f32x16 (&acc)[TM][TN], const uint4 (&fa)[TM][3], const uint4 (&fb)[TN][3]) {
#pragma unroll
  for (int p = 0; p < 6; ++p)
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
        acc[i][j] = TRANS ? fd::mfma_32x32x16_bf16(fb[j][FD_PB[p]], fa[i][FD_PA[p]], acc[i][j])
                          : fd::mfma_32x32x16_bf16(fa[i][FD_PA[p]], fb[j][FD_PB[p]], acc[i][j]);
}
