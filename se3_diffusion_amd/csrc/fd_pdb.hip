// fd_pdb_count / fd_pdb_format: the text of a PDB file (MODEL / ATOM / TER / ENDMDL records of 80 columns and a newline) from
// atom37 coordinates in HBM.  include/fd_hip.h is the specification; this file says how the two launches are laid out.
//
// fd_pdb_count   one block of 512 threads per model.  Threads stride over the N x 37 atom slots (a wave reads 64 consecutive
//                slots, 768 contiguous bytes), count the present ones and look for input that no 80-column record can hold.  The
//                count and the smallest offending key are reduced by shuffles in the wave and over the eight wave results in wave
//                order: one status word PER MODEL, no atomics (the caller takes the minimum over the models).
// fd_pdb_format  one block of 512 threads per model.  The block walks the model's slots 512 at a time in (residue, slot) order;
//                in each round a thread owns one slot, an ordered prefix scan of the presence flags (shuffles in the wave, the
//                eight wave totals in wave order) gives its line within the round, and the running total of the rounds before
//                gives its serial.  The thread formats its 81 bytes into LDS; the MODEL line rides in front of the first round's
//                lines, TER / ENDMDL (and END after the last model) behind the last round's.  The round's span is contiguous in
//                the file, so the block then copies it out with 16-byte stores: it is staged at the file offset's remainder
//                modulo 16, which makes LDS and HBM addresses congruent, and only the at most 15 bytes at either end are
//                written singly (they may share a 16-byte unit with the neighbouring model's block).  The placement depends on
//                the scan alone: two runs write identical bytes.
//
// A number is printed from integers: rint(|x| 10^F) in fp64 (the product of an fp32 value and 1000 or 100 is exact there, so this
// IS round-half-to-even on the exact value, what a correctly rounded %.3f prints), split into decimal digits; the sign is the
// sign bit of x, so that -0.0004f prints -0.000.  Every field writer stays inside its field whatever the value: input that does
// not fit is reported by the count pass, and a caller that formats regardless gets truncated digits, never a write outside the line.
#include "fd_common.h"
#include "../../include/fd_hip.h"

namespace {

constexpr int PT = 512;                           // threads of a block: eight waves
constexpr int PW = PT / 64;
constexpr int P_SLOTS = 37;
constexpr int P_LINE = 81;                        // 80 columns and '\n'
constexpr int P_MAX_N = FD_PDB_MAX_N;             // residue numbers 0 .. 9999 fit four columns
constexpr int P_MAX_SERIAL = 99999;
constexpr long P_OK = FD_PDB_STATUS_OK;
constexpr int P_STAGE = ((PT + 3) * P_LINE + 3 + 15 + 15) / 16 * 16;    // the shift, MODEL, 512 lines, TER, ENDMDL, END

enum {
  K_NONFINITE = FD_PDB_NONFINITE,
  K_COORD = FD_PDB_COORD,
  K_BFACTOR = FD_PDB_BFACTOR,
  K_SERIAL = FD_PDB_SERIAL,
  K_LENGTH = FD_PDB_LENGTH,
  K_AATYPE = FD_PDB_AATYPE
};

// ' ' + atom name, left-justified to four columns (the element is the name's first letter); residue names by aatype, 20 = UNK
__device__ const char kNames[P_SLOTS * 4 + 1] =
    " N   CA  C   CB  O   CG  CG1 CG2 OG  OG1 SG  CD  CD1 CD2 ND1 ND2 OD1 OD2 SD  CE  CE1 CE2 CE3 NE  NE1 NE2 OE1 OE2 CH2 NH1 "
    "NH2 OH  CZ  CZ2 CZ3 NZ  OXT";
__device__ const char kRes3[21 * 3 + 1] = "ALAARGASNASPCYSGLNGLUGLYHISILELEULYSMETPHEPROSERTHRTRPTYRVALUNK";

__device__ __forceinline__ bool finite_f(float x) { return fabsf(x) <= 3.4028234664e38f; }               // (false for NaN)
__device__ __forceinline__ bool present(float x, float y, float z) { return (fabsf(x) + fabsf(y)) + fabsf(z) > 1e-7f; }

// |rint(x scale)| for |x| < 1e5 (anything larger fits no field and is reported by the count pass), else 0
__device__ __forceinline__ long fixed_abs(float x, double scale) {
  return fabsf(x) < 1e5f ? (long)rint(fabs((double)x) * scale) : 0L;
}
// does %8.3f (scale 1000: -999.999 .. 9999.999) or %6.2f (scale 100: -99.99 .. 999.99) hold x?
__device__ __forceinline__ bool fits(float x, double scale, long lo, long hi) {
  if (!(fabsf(x) < 1e5f)) return false;
  const long u = fixed_abs(x, scale);
  return __builtin_signbit(x) ? u <= lo : u <= hi;
}

// v >= 0 right-justified in w columns
__device__ __forceinline__ void put_int(unsigned char* p, int w, long v) {
  for (int k = w - 1; k >= 0; --k) {
    if (v > 0 || k == w - 1) {
      p[k] = (unsigned char)('0' + (int)(v % 10));
      v /= 10;
    } else {
      p[k] = ' ';
    }
  }
}

// x as %W.Ff
template <int W, int F>
__device__ __forceinline__ void put_fixed(unsigned char* p, float x) {
  long u = fixed_abs(x, F == 3 ? 1000.0 : 100.0);
  int k = W - 1;
#pragma unroll
  for (int f = 0; f < F; ++f) {
    p[k--] = (unsigned char)('0' + (int)(u % 10));
    u /= 10;
  }
  p[k--] = '.';
  do {
    p[k--] = (unsigned char)('0' + (int)(u % 10));
    u /= 10;
  } while (u > 0 && k >= 0);
  if (__builtin_signbit(x) && k >= 0) p[k--] = '-';
  while (k >= 0) p[k--] = ' ';
}

__device__ __forceinline__ void put_text(unsigned char* p, const char* s, int n) {
  for (int k = 0; k < n; ++k) p[k] = (unsigned char)s[k];
}
__device__ __forceinline__ void put_spaces(unsigned char* p, int from, int to) {
  for (int k = from; k < to; ++k) p[k] = ' ';
}
__device__ __forceinline__ int res_of(const int* __restrict__ aatype, int r) {
  const int a = aatype ? aatype[r] : 0;
  return a >= 0 && a <= 20 ? a : 20;
}

__device__ __forceinline__ void atom_line(unsigned char* p, int serial, int slot, int res, int resnum, float x, float y, float z,
                                          float b) {
  put_text(p, "ATOM  ", 6);
  put_int(p + 6, 5, serial);
  p[11] = ' ';
  put_text(p + 12, kNames + 4 * slot, 4);
  p[16] = ' ';
  put_text(p + 17, kRes3 + 3 * res, 3);
  p[20] = ' ';
  p[21] = 'A';
  put_int(p + 22, 4, resnum);
  put_spaces(p, 26, 30);
  put_fixed<8, 3>(p + 30, x);
  put_fixed<8, 3>(p + 38, y);
  put_fixed<8, 3>(p + 46, z);
  put_text(p + 54, "  1.00", 6);
  put_fixed<6, 2>(p + 60, b);
  put_spaces(p, 66, 77);
  p[77] = (unsigned char)kNames[4 * slot + 1];
  p[78] = ' ';
  p[79] = ' ';
  p[80] = '\n';
}

// the model's MODEL line
__device__ __forceinline__ void model_line(unsigned char* p, long number) {
  put_text(p, "MODEL     ", 10);
  int digits = 1;
  for (long v = number; v >= 10; v /= 10) ++digits;
  put_int(p + 10, digits, number);
  put_spaces(p, 10 + digits, 80);
  p[80] = '\n';
}

// TER and ENDMDL, and END behind the last model
__device__ __forceinline__ void tail_lines(unsigned char* p, int serial, int res, int resnum, bool end) {
  put_text(p, "TER   ", 6);
  put_int(p + 6, 5, serial);
  put_spaces(p, 11, 17);
  put_text(p + 17, kRes3 + 3 * res, 3);
  p[20] = ' ';
  p[21] = 'A';
  put_int(p + 22, 4, resnum);
  put_spaces(p, 26, 80);
  p[80] = '\n';
  p += P_LINE;
  put_text(p, "ENDMDL", 6);
  put_spaces(p, 6, 80);
  p[80] = '\n';
  if (end) put_text(p + P_LINE, "END", 3);
}

// ---- fd_pdb_count ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PT) void pdb_count_kernel(const float* __restrict__ atoms, long model_stride,
                                                       const int* __restrict__ aatype, const float* __restrict__ b_factors, int N,
                                                       long* __restrict__ counts, long* __restrict__ status) {
  __shared__ int wcnt[PW];
  __shared__ long wbad[PW];
  const int tid = (int)threadIdx.x, lane = fd::lane_id(), wave = fd::wave_id();
  const long m = (long)blockIdx.x;
  const float* p = atoms + m * model_stride;
  const int total = N * P_SLOTS;
  const long key0 = m * total * 8;                // key of an entry: 8 (linear index) + kind
  int cnt = 0;
  long bad = P_OK;
  for (int a = tid; a < total; a += PT) {
    const float x = p[3 * a], y = p[3 * a + 1], z = p[3 * a + 2];
    long k = P_OK;
    if (!(finite_f(x) && finite_f(y) && finite_f(z))) {
      k = K_NONFINITE;
    } else if (present(x, y, z)) {
      if (!(fits(x, 1000.0, 999999, 9999999) && fits(y, 1000.0, 999999, 9999999) && fits(z, 1000.0, 999999, 9999999)))
        k = K_COORD;
      else if (b_factors && !fits(b_factors[a], 100.0, 9999, 99999))
        k = K_BFACTOR;
    }
    cnt += present(x, y, z) ? 1 : 0;
    if (k != P_OK) {
      k += key0 + 8L * a;
      bad = k < bad ? k : bad;
    }
  }
  if (aatype && m == 0)                           // (a residue's name does not depend on the model: reported at model 0)
    for (int r = tid; r < N; r += PT)
      if (aatype[r] < 0 || aatype[r] > 20) {
        const long k = 8L * r * P_SLOTS + K_AATYPE;
        bad = k < bad ? k : bad;
      }
  if (N > P_MAX_N && tid == 0) {                  // the first residue whose number needs a fifth column
    const long k = key0 + 8L * P_MAX_N * P_SLOTS + K_LENGTH;
    bad = k < bad ? k : bad;
  }
  cnt = fd::wave_sum(cnt);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const long u = __shfl_xor(bad, o);
    bad = u < bad ? u : bad;
  }
  if (lane == 0) wcnt[wave] = cnt, wbad[wave] = bad;
  __syncthreads();
  if (tid == 0) {
    cnt = 0;
    for (int w = 0; w < PW; ++w) {
      cnt += wcnt[w];
      bad = wbad[w] < bad ? wbad[w] : bad;
    }
    // the first line whose serial needs a sixth column: the 100000th present atom, or TER behind the 99999th (reported at the
    // model's last entry).  One thread walks the model: this is the path of a refusal.
    if (cnt >= P_MAX_SERIAL) {
      long k = key0 + 8L * (total - 1) + K_SERIAL;
      if (cnt > P_MAX_SERIAL) {
        int seen = 0;
        for (int a = 0; a < total; ++a)
          if (present(p[3 * a], p[3 * a + 1], p[3 * a + 2]) && ++seen > P_MAX_SERIAL) {
            k = key0 + 8L * a + K_SERIAL;
            break;
          }
      }
      bad = k < bad ? k : bad;
    }
    counts[m] = cnt;
    status[m] = bad;
  }
}

// ---- fd_pdb_format ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PT) void pdb_format_kernel(const float* __restrict__ atoms, long model_stride,
                                                        const int* __restrict__ aatype, const float* __restrict__ b_factors,
                                                        const long* __restrict__ line_offset, int M, int N, long first_model,
                                                        unsigned char* __restrict__ out, long out_bytes) {
  __shared__ __attribute__((aligned(16))) unsigned char stage[P_STAGE];
  __shared__ int wtot[PW];
  const int tid = (int)threadIdx.x, lane = fd::lane_id(), wave = fd::wave_id();
  const int m = (int)blockIdx.x;
  const float* p = atoms + (long)m * model_stride;
  const int total = N * P_SLOTS, rounds = (total + PT - 1) / PT;
  long g = line_offset[m] * P_LINE;               // the file offset of the next byte of this model
  int placed = 0;                                 // ATOM lines of the rounds before
  for (int it = 0; it < rounds; ++it) {
    const int a = it * PT + tid;
    float x = 0.f, y = 0.f, z = 0.f;
    if (a < total) x = p[3 * a], y = p[3 * a + 1], z = p[3 * a + 2];
    const int pres = present(x, y, z) ? 1 : 0;
    int incl = pres;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int u = __shfl(incl, lane >= o ? lane - o : lane);
      if (lane >= o) incl += u;
    }
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();
    int before = incl - pres, here = 0;
    for (int w = 0; w < PW; ++w) {
      if (w < wave) before += wtot[w];
      here += wtot[w];
    }
    const bool first = it == 0, last = it == rounds - 1, end = m == M - 1;
    const int head = first ? P_LINE : 0;
    const int span = head + here * P_LINE + (last ? 2 * P_LINE + (end ? 3 : 0) : 0);
    // (g < 0 or a span past the end: line_offset does not belong to this input; nothing is written)
    if (span > 0 && g >= 0 && g + span <= out_bytes) {
      const int sh = (int)(g & 15);
      unsigned char* s = stage + sh;
      if (first && tid == 0) model_line(s, first_model + m);
      if (last && tid == 64) tail_lines(s + head + here * P_LINE, placed + here + 1, res_of(aatype, N - 1), N - 1, end);
      if (pres) {
        const int r = a / P_SLOTS, slot = a - r * P_SLOTS;
        atom_line(s + head + before * P_LINE, placed + before + 1, slot, res_of(aatype, r), r, x, y, z,
                  b_factors ? b_factors[a] : 0.f);
      }
      __syncthreads();
      const int hb = (16 - sh) & 15, nhead = hb < span ? hb : span;
      const int nvec = (span - nhead) / 16, ntail = span - nhead - 16 * nvec;
      if (tid < nhead) out[g + tid] = s[tid];
      for (int v = tid; v < nvec; v += PT)
        *reinterpret_cast<fd::u32x4*>(out + g + nhead + 16 * v) = *reinterpret_cast<const fd::u32x4*>(s + nhead + 16 * v);
      if (tid < ntail) out[g + nhead + 16 * nvec + tid] = s[nhead + 16 * nvec + tid];
    }
    g += span;
    placed += here;
    __syncthreads();                              // stage and wtot are rewritten by the next round
  }
}

}  // namespace

extern "C" int fd_pdb_count(const float* atoms, long model_stride, const int* aatype, const float* b_factors, int M, int N,
                            long* counts, long* status, void* stream) {
  FD_CHECK_ARG(M >= 0 && N >= 1, "fd_pdb_count: M must be at least 0 and N at least 1");
  FD_CHECK_ARG((long)N * P_SLOTS * 3 < (1L << 31) / 2, "fd_pdb_count: N x 37 x 3 must be below 2^30");
  if (M == 0) return FD_OK;
  FD_CHECK_ARG(atoms && counts && status, "fd_pdb_count: null operand");
  FD_CHECK_ARG((((uintptr_t)counts) & 7u) == 0 && (((uintptr_t)status) & 7u) == 0, "fd_pdb_count: misaligned output");
  hipLaunchKernelGGL(pdb_count_kernel, dim3((unsigned)M), dim3(PT), 0, (hipStream_t)stream, atoms, model_stride, aatype, b_factors,
                     N, counts, status);
  FD_CHECK_LAUNCH("fd_pdb_count");
  return FD_OK;
}

extern "C" int fd_pdb_format(const float* atoms, long model_stride, const int* aatype, const float* b_factors,
                             const long* line_offset, int M, int N, long first_model, unsigned char* out, long out_bytes,
                             void* stream) {
  FD_CHECK_ARG(M >= 0 && N >= 1, "fd_pdb_format: M must be at least 0 and N at least 1");
  FD_CHECK_ARG((long)N * P_SLOTS * 3 < (1L << 31) / 2, "fd_pdb_format: N x 37 x 3 must be below 2^30");
  FD_CHECK_ARG(first_model >= 0 && out_bytes >= 0, "fd_pdb_format: negative model number or size");
  if (M == 0) return FD_OK;
  FD_CHECK_ARG(atoms && line_offset && out, "fd_pdb_format: null operand");
  FD_CHECK_ARG(fd_aligned16(out) && (((uintptr_t)line_offset) & 7u) == 0, "fd_pdb_format: out must be 16-byte aligned");
  hipLaunchKernelGGL(pdb_format_kernel, dim3((unsigned)M), dim3(PT), 0, (hipStream_t)stream, atoms, model_stride, aatype,
                     b_factors, line_offset, M, N, first_model, out, out_bytes);
  FD_CHECK_LAUNCH("fd_pdb_format");
  return FD_OK;
}
