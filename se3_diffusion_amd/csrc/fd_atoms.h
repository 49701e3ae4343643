// Idealised backbone of one residue: frame (quaternion wxyz + translation, A) + psi (sin, cos) -> N, CA, C, CB, O
// (reference all_atom.py:152-174 restricted to the five atoms it leaves non-zero).  Shared by backbone_atoms_kernel
// (fd_atoms.hip) and sample_record_kernel (fd_sample_record.hip): one arithmetic, bit for bit.
#pragma once
#include "fd_common.h"
#include "../../include/fd_hip.h"

struct AtomConst {
  float atoms[15];
  float Rd[9];
  float td[3];
};

static inline AtomConst fd_atom_const(const FdHeadConst* c) {
  AtomConst ac;
  for (int i = 0; i < 15; ++i) ac.atoms[i] = c->atoms[i];
  for (int i = 0; i < 9; ++i) ac.Rd[i] = c->Rd[i];
  for (int i = 0; i < 3; ++i) ac.td[i] = c->td[i];
  return ac;
}

// q: 7 floats of one row; pos[n] = atom n in the order N, CA, C, CB, O
__device__ __forceinline__ void fd_backbone5(const float* __restrict__ q, float ps, float pc, const AtomConst& ac,
                                             float pos[5][3]) {
  const float a = q[0], b = q[1], c = q[2], d = q[3];
  float Rm[9];
  Rm[0] = a * a + b * b - c * c - d * d; Rm[1] = 2.f * (b * c - a * d); Rm[2] = 2.f * (b * d + a * c);
  Rm[3] = 2.f * (b * c + a * d); Rm[4] = a * a - b * b + c * c - d * d; Rm[5] = 2.f * (c * d - a * b);
  Rm[6] = 2.f * (b * d - a * c); Rm[7] = 2.f * (c * d + a * b); Rm[8] = a * a - b * b - c * c + d * d;
  const float tx = q[4], ty = q[5], tz = q[6];
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    const float lx = ac.atoms[3 * n], ly = ac.atoms[3 * n + 1], lz = ac.atoms[3 * n + 2];
    pos[n][0] = Rm[0] * lx + Rm[1] * ly + Rm[2] * lz + tx;
    pos[n][1] = Rm[3] * lx + Rm[4] * ly + Rm[5] * lz + ty;
    pos[n][2] = Rm[6] * lx + Rm[7] * ly + Rm[8] * lz + tz;
  }
  const float ox = ac.atoms[12], oy = ac.atoms[13], oz = ac.atoms[14];
  const float rx = ox, ry = pc * oy - ps * oz, rz = ps * oy + pc * oz;
  const float wx = ac.Rd[0] * rx + ac.Rd[1] * ry + ac.Rd[2] * rz + ac.td[0];
  const float wy = ac.Rd[3] * rx + ac.Rd[4] * ry + ac.Rd[5] * rz + ac.td[1];
  const float wz = ac.Rd[6] * rx + ac.Rd[7] * ry + ac.Rd[8] * rz + ac.td[2];
  pos[4][0] = Rm[0] * wx + Rm[1] * wy + Rm[2] * wz + tx;
  pos[4][1] = Rm[3] * wx + Rm[4] * wy + Rm[5] * wz + ty;
  pos[4][2] = Rm[6] * wx + Rm[7] * wy + Rm[8] * wz + tz;
}
