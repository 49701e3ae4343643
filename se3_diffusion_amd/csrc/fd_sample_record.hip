// Trajectory recording of the device-resident sampler: one launch per diffusion step writes that step's slice of everything
// Experiment.inference_fn(aux_traj=True) collects (reference experiments/train_se3_diffusion.py:782-803) into preallocated
// device buffers -- the reference moves four arrays to numpy per step (du.move_to_np: a device synchronisation each) and
// calls compute_backbone twice.
//
//   rigid_traj [T+1,B,N,7]   the frames after the reverse step                                   (:782-784)
//   bb_t       [T,B,N,5,3]   N, CA, C, CB, O of compute_backbone(rigids_t, psi)                  (:801-803)
//   bb_0       [T,B,N,5,3]   the same atoms of compute_backbone(rigid_pred, psi)                 (:794-799)
//   trans_0    [T,B,N,3]     diffuse_mask * rigid_pred[4:] + fixed_mask*res_mask * rigids_t[4:]  (:787-790)
//
// The reference flips every array at the end so that index 0 is the final structure (:805-812); here step s is written at
// index T-1-s straight away (slot T of rigid_traj holds the starting frames, copied by the caller), so there is no flip pass.
//
// Stores: a thread-per-residue layout would write 60-byte records with a 60-byte stride.  A block stages TILE rows of all four
// outputs in LDS (row strides 7 / 15 / 3 dwords: odd, conflict-free) and then writes each buffer's TILE-row chunk -- contiguous
// in memory -- with consecutive lanes on consecutive dwords.
#include "fd_atoms.h"

namespace {

constexpr int TILE = 64;          // rows per block iteration
constexpr int THREADS = 256;
constexpr int MAX_BLOCKS = 1024;  // grid cap of the launcher (tiles beyond it: block-stride loop)

__device__ __forceinline__ void stream_out(float* __restrict__ dst, const float* src, int n, int tid) {
  for (int i = tid; i < n; i += THREADS) dst[i] = src[i];
}

__global__ __launch_bounds__(THREADS) void sample_record_kernel(
    const float* __restrict__ rigids_t, const float* __restrict__ rigid_pred, const float* __restrict__ psi,
    const float* __restrict__ fixed_mask, const float* __restrict__ res_mask, AtomConst ac, const int* __restrict__ slot_ptr,
    int slot_offset, int T, long R_, int aux, float* __restrict__ rigid_traj, float* __restrict__ bb_t,
    float* __restrict__ bb_0, float* __restrict__ trans_0) {
  __shared__ float s_rig[TILE * 7];
  __shared__ float s_bbt[TILE * 15];
  __shared__ float s_bb0[TILE * 15];
  __shared__ float s_tr0[TILE * 3];
  // (read-only: the counter is advanced by fd_sample_advance, an earlier launch of the same stream)
  const int step = (slot_ptr ? *slot_ptr : 0) + slot_offset;
  if (step < 0 || step >= T) return;              // uniform over the grid: never a write outside a buffer
  const long idx = (long)T - 1 - step;            // flipped: index 0 is the final structure
  const int tid = (int)threadIdx.x;
  const int row = tid & (TILE - 1), job = tid / TILE;
  const long ntiles = (R_ + TILE - 1) / TILE;
  for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long r0 = tile * TILE;
    const int nr = (int)(R_ - r0 < TILE ? R_ - r0 : TILE);
    const long r = r0 + row;
    if (row < nr) {
      if (job == 0) {                             // frames of this step and their atoms
        const float* q = rigids_t + r * 7;
        float pos[5][3];
        fd_backbone5(q, psi[r * 2], psi[r * 2 + 1], ac, pos);
#pragma unroll
        for (int n = 0; n < 5; ++n)
#pragma unroll
          for (int k = 0; k < 3; ++k) s_bbt[row * 15 + n * 3 + k] = pos[n][k];
        if (aux) {
#pragma unroll
          for (int k = 0; k < 7; ++k) s_rig[row * 7 + k] = q[k];
        }
      } else if (job == 1 && aux) {               // the network's x0 prediction: atoms and masked translations
        const float* q = rigid_pred + r * 7;
        float pos[5][3];
        fd_backbone5(q, psi[r * 2], psi[r * 2 + 1], ac, pos);
#pragma unroll
        for (int n = 0; n < 5; ++n)
#pragma unroll
          for (int k = 0; k < 3; ++k) s_bb0[row * 15 + n * 3 + k] = pos[n][k];
        const float fx = fixed_mask[r], rm = res_mask[r];
        const float dm = (1.f - fx) * rm, fm = fx * rm;
        const float* g = rigids_t + r * 7 + 4;
#pragma unroll
        for (int k = 0; k < 3; ++k) s_tr0[row * 3 + k] = dm * q[4 + k] + fm * g[k];
      }
    }
    __syncthreads();
    stream_out(bb_t + (idx * R_ + r0) * 15, s_bbt, nr * 15, tid);
    if (aux) {
      stream_out(rigid_traj + (idx * R_ + r0) * 7, s_rig, nr * 7, tid);
      stream_out(bb_0 + (idx * R_ + r0) * 15, s_bb0, nr * 15, tid);
      stream_out(trans_0 + (idx * R_ + r0) * 3, s_tr0, nr * 3, tid);
    }
    __syncthreads();                              // (the next tile reuses the staging arrays)
  }
}

}  // namespace

extern "C" int fd_sample_record(const float* rigids_t, const float* rigid_pred, const float* psi, const float* fixed_mask,
                                const float* res_mask, const FdHeadConst* c, const int* slot_ptr, int slot_offset, int T, long R_,
                                int aux, float* rigid_traj, float* bb_t, float* bb_0, float* trans_0, void* stream) {
  FD_CHECK_ARG(c != nullptr, "fd_sample_record: null constants");
  FD_CHECK_ARG(T >= 1 && R_ >= 0, "fd_sample_record: bad extents (T=%d, R=%ld)", T, R_);
  FD_CHECK_ARG(rigids_t && psi && bb_t, "fd_sample_record: null operand");
  FD_CHECK_ARG(!aux || (rigid_pred && fixed_mask && res_mask && rigid_traj && bb_0 && trans_0),
               "fd_sample_record: aux recording needs rigid_pred, both masks and all four buffers");
  // with a device counter the step is only known on the device (the kernel skips an out-of-range one)
  FD_CHECK_ARG(slot_ptr || (slot_offset >= 0 && slot_offset < T), "fd_sample_record: step %d outside [0, %d)", slot_offset, T);
  if (R_ == 0) return FD_OK;
  const long g = (R_ + TILE - 1) / TILE;
  hipLaunchKernelGGL(sample_record_kernel, dim3((unsigned)(g > MAX_BLOCKS ? MAX_BLOCKS : g)), dim3(THREADS), 0,
                     (hipStream_t)stream, rigids_t, rigid_pred, psi, fixed_mask, res_mask, fd_atom_const(c), slot_ptr, slot_offset,
                     T, R_, aux, rigid_traj, bb_t, bb_0, trans_0);
  FD_CHECK_LAUNCH("fd_sample_record");
  return FD_OK;
}
