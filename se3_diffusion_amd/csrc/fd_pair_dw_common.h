// Shared pieces of the grouped weight-gradient kernels (fd_pair_dw.hip, fd_group_dw.hip; tools/experiments/fd_pair_dw_diag.hip):
// stage geometry, the transposed LDS operand read, the plane-major product loop of a stage.  The fp32 -> 3 x bf16 split of
// a float4 on the way to LDS is fd_split.h's fd_split4.
#pragma once
#include "fd_common.h"

namespace {

#include "fd_split.h"

constexpr int DW_THREADS = 512;
constexpr int DW_KS = 16;                          // pair rows per stage = one MFMA k-step
constexpr int DW_PSTRIDE = DW_KS * 64 + 64;        // bytes of a 32-column panel of one plane (+64: the two 8-lane halves
                                                   // of a ds_write_b64 group land on different bank halves)
constexpr int DW_PANELS = 16;                      // 12 of A (384 columns) + 4 of B (128 columns)
constexpr int DW_PLANE = DW_PANELS * DW_PSTRIDE;
constexpr int DW_STAGE = 3 * DW_PLANE;             // 52,224 B
constexpr int DW_RING = 2;
static_assert(DW_RING * DW_STAGE <= 160 * 1024, "LDS");

// the 8 consecutive k of one column: k 8kg..8kg+3 and 8kg+4..8kg+7 (four 64-byte rows further)
__device__ __forceinline__ uint4 dw_read8(const char* p) {
  const uint2 lo = fd::lds_read_tr16(p), hi = fd::lds_read_tr16(p + 256);
  return make_uint4(lo.x, lo.y, hi.x, hi.y);
}

// One 16-k stage (image st) of a wave tile of NA x 2 panels: a_rd / b_rd = this lane's read offset in the wave's first
// A / B panel of plane 0, PLANE = bytes between the planes of the image.  The six products with i + j <= 2 PLANE-MAJOR, the small
// terms first -- A plane 2, 1, 0 and under each the B planes 2 - sa .. 0, i.e. (2,0) (1,1) (1,0) (0,2) (0,1) (0,0) -- so
// that only one plane of the A fragments is live at a time.  (Not fd_split.h's order: fp32 accumulation order is
// observable, each stays as it is.)
template <bool TRANS, int NA, int PLANE>
__device__ __forceinline__ void dw_mma6(f32x16 (&acc)[NA][2], const char* st, int a_rd, int b_rd) {
  uint4 fb[2][3];
#pragma unroll
  for (int s = 0; s < 3; ++s)
#pragma unroll
    for (int j = 0; j < 2; ++j) fb[j][s] = dw_read8(st + b_rd + j * DW_PSTRIDE + s * PLANE);
#pragma unroll
  for (int sa = 2; sa >= 0; --sa) {
    uint4 fa[NA];
#pragma unroll
    for (int i = 0; i < NA; ++i) fa[i] = dw_read8(st + a_rd + i * DW_PSTRIDE + sa * PLANE);
#pragma unroll
    for (int sb = 2 - sa; sb >= 0; --sb)
#pragma unroll
      for (int i = 0; i < NA; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = TRANS ? fd::mfma_32x32x16_bf16(fb[j][sb], fa[i], acc[i][j])
                            : fd::mfma_32x32x16_bf16(fa[i], fb[j][sb], acc[i][j]);
  }
}

// the item's pointers come out of a dynamically indexed kernel-argument array: tell the compiler they are global
// (global_load / global_atomic instead of flat_*)
template <typename T>
__device__ __forceinline__ T* dw_global(T* p) {
  return (T*)(__attribute__((address_space(1))) T*)p;
}

}  // namespace
