// Stand-alone idealised backbone builder: frames (A) + psi -> N, CA, C, CB, O.
//
// Drop-in kernel behind data/all_atom.py:compute_backbone (reference all_atom.py:152-174,
// which runs torsion_angles_to_frames for all 8 rigid groups x 14 atoms with CPU-resident
// index tensors -> a device<->host round trip per call).  Here: one thread per residue,
// 5 atoms, no host involvement.  Same arithmetic as the atoms block of fd_heads_fwd.
#include "fd_atoms.h"

namespace {

__global__ __launch_bounds__(256) void backbone_atoms_kernel(const float* __restrict__ rigids,
                                                             const float* __restrict__ psi, AtomConst ac,
                                                             float* __restrict__ atom37, float* __restrict__ atom14,
                                                             long R_) {
  for (long r = (long)blockIdx.x * 256 + threadIdx.x; r < R_; r += (long)gridDim.x * 256) {
    float* a37 = atom37 + r * 111;
    float* a14 = atom14 + r * 42;
    for (int k = 0; k < 111; ++k) a37[k] = 0.f;
    for (int k = 0; k < 42; ++k) a14[k] = 0.f;
    float pos[5][3];
    fd_backbone5(rigids + r * 7, psi[r * 2], psi[r * 2 + 1], ac, pos);
    const int m14[5] = {0, 1, 2, 4, 3};
#pragma unroll
    for (int n = 0; n < 5; ++n)
#pragma unroll
      for (int k = 0; k < 3; ++k) { a37[n * 3 + k] = pos[n][k]; a14[m14[n] * 3 + k] = pos[n][k]; }
  }
}

}  // namespace

extern "C" int fd_backbone_atoms(const float* rigids, const float* psi, const FdHeadConst* c, float* atom37,
                                 float* atom14, long R_, void* stream) {
  FD_CHECK_ARG(c != nullptr, "fd_backbone_atoms: null constants");
  if (R_ == 0) return FD_OK;
  const AtomConst ac = fd_atom_const(c);
  long g = (R_ + 255) / 256;
  hipLaunchKernelGGL(backbone_atoms_kernel, dim3((unsigned)(g > 4096 ? 4096 : g)), dim3(256), 0, (hipStream_t)stream,
                     rigids, psi, ac, atom37, atom14, R_);
  FD_CHECK_LAUNCH("fd_backbone_atoms");
  return FD_OK;
}
