// fd_pdb_read_summary / fd_pdb_read_count / fd_pdb_read_fill: atom37 arrays from the text of PDB files in HBM, the inverse of
// fd_pdb.hip.  include/fd_hip.h is the specification; this file says how the three launches are laid out.
//
// The text of F files lies end to end.  A thread owns a WINDOW of 16 bytes, a block of 256 threads a CHUNK of 4096 bytes, and a
// line belongs to the thread whose window holds its first byte.  No array is indexed by line, so nothing has to be sized by a
// count that is only known on the device: what passes between the launches is per chunk or per file.
//
//   summary  per chunk: the lines and ENDMDL records that start in it, and the position of the last ENDMDL and of the last
//            coordinate record among them.  The caller turns these into what every chunk needs to know of the text in front of
//            it (cumsum of the counts, cummax of the positions).
//   count    an ordered block scan (shuffles in the wave, the four wave totals in wave order, as fd_pdb_format's) carries the
//            same four values from thread to thread, so every thread knows for each of its lines: the line's index, the ENDMDL
//            records in front of it, and where the coordinate record before it lies.  A coordinate record is parsed and
//            checked by its thread (the <= 80 columns in five 16-byte loads), and begins a residue row when its key differs
//            from that of the record before it, which the thread reads where the scan says it lies.  Per chunk: residue
//            starts, chain starts, the smallest 8 (line index) + kind of a malformed record; per file: the index of its
//            first line and the ENDMDL records in front of it.
//   fill     the same analysis twice: once to scan the starts of a chunk into row and chain numbers, once to act on them.
//            The thread of a residue's first record walks that residue's lines in file order and places the atoms: the first
//            record of a slot wins, so the result does not depend on any order of execution.  No atomics anywhere.
#include "fd_text_read.h"                       // what this reader shares with fd_cif_read.hip

namespace {

enum { C_OTHER = 0, C_ATOM = 1, C_HETATM = 2, C_MODEL = 3, C_ENDMDL = 4 };

constexpr unsigned long pack6(const char* s) {
  unsigned long v = 0;
  for (int k = 0; k < 6; ++k) v |= (unsigned long)(unsigned char)s[k] << (8 * k);
  return v;
}
// what a thread knows of the text in front of a line: lines and ENDMDL records so far, the position of the last ENDMDL record
// and of the last coordinate record (-1: none).  Counts add, positions take the later one: an associative pair, scanned in order.
struct Run {
  long nL, nE, lastE, lastC;
  static __device__ __forceinline__ Run none() { return Run{0, 0, -1, -1}; }
};
__device__ __forceinline__ Run join(const Run& a, const Run& b) {
  return Run{a.nL + b.nL, a.nE + b.nE, b.lastE > a.lastE ? b.lastE : a.lastE, b.lastC > a.lastC ? b.lastC : a.lastC};
}
__device__ __forceinline__ Run shfl_run(const Run& r, int src) {
  return Run{__shfl(r.nL, src), __shfl(r.nE, src), __shfl(r.lastE, src), __shfl(r.lastC, src)};
}

// the record type of the line at p, from its leading six columns (a short line is padded with blanks; '\r' in front of the line's
// end is not a column)
__device__ __forceinline__ int class_of(unsigned long six) {
  return six == pack6("ATOM  ") ? C_ATOM : six == pack6("HETATM") ? C_HETATM : six == pack6("ENDMDL") ? C_ENDMDL
       : six == pack6("MODEL ") ? C_MODEL : C_OTHER;
}
__device__ __forceinline__ int classify(const unsigned char* __restrict__ t, long p, long fe) {
  unsigned long v = 0;
  int k = 0;
  for (; k < 6 && p + k < fe; ++k) {
    const unsigned char c = t[p + k];
    if (c == '\n' || (c == '\r' && (p + k + 1 >= fe || t[p + k + 1] == '\n'))) break;
    v |= (unsigned long)c << (8 * k);
  }
  for (; k < 6; ++k) v |= 0x20UL << (8 * k);
  return class_of(v);
}
__device__ __forceinline__ bool is_coord(const Text& x, int cls) { return cls == C_ATOM || (cls == C_HETATM && x.hetatm); }

// the leading 16 PIECES columns of a line in registers, blanks behind its end
template <int PIECES>
struct Line {
  unsigned w[4 * PIECES];
  int len;                                        // columns, at most 16 PIECES
  long end;                                       // the position of the line's '\n', or the file's end (NEED_END only)
};
template <int PIECES>
__device__ __forceinline__ unsigned col(const Line<PIECES>& L, int k) { return (L.w[k >> 2] >> (8 * (k & 3))) & 0xffu; }

// Reads the line at p of a file that ends at fe: a 16-byte load per piece that lies inside the file, single bytes for the last
// one; nothing at or behind fe is read.  The end of the file counts as a newline.
template <int PIECES, bool NEED_END>
__device__ __forceinline__ void load_line(const unsigned char* __restrict__ t, long p, long fe, Line<PIECES>& L) {
  int len = -1;
  bool cr = false;                                // the byte in front of the newline is '\r'
  unsigned prev = 0;
#pragma unroll
  for (int j = 0; j < PIECES; ++j) {
    unsigned q[4] = {0x20202020u, 0x20202020u, 0x20202020u, 0x20202020u};
    if (len < 0) {
      const long b = p + 16 * j;
      if (b + 16 <= fe) {
        __builtin_memcpy(q, t + b, 16);
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          unsigned v = 0;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const long a = b + 4 * i + e;
            v |= (a < fe ? (unsigned)t[a] : (unsigned)'\n') << (8 * e);
          }
          q[i] = v;
        }
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const unsigned c = (q[i] >> (8 * e)) & 0xffu;
          if (len < 0) {
            if (c == '\n') len = 16 * j + 4 * i + e, cr = prev == '\r';
            prev = c;
          }
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) L.w[4 * j + i] = q[i];
  }
  if (NEED_END) {
    long e = p + (len < 0 ? 16 * PIECES : len);
    if (len < 0)
      while (e < fe && t[e] != '\n') ++e;
    L.end = e;
  }
  len = len < 0 ? 16 * PIECES : cr ? len - 1 : len;
#pragma unroll
  for (int i = 0; i < 4 * PIECES; ++i) {
    const int nv = len - 4 * i;                   // columns of this word that belong to the line
    const unsigned keep = nv >= 4 ? 0xffffffffu : nv <= 0 ? 0u : (1u << (8 * nv)) - 1u;
    L.w[i] = (L.w[i] & keep) | (0x20202020u & ~keep);
  }
  L.len = len;
}
template <int PIECES>
__device__ __forceinline__ int class_of_line(const Line<PIECES>& L) {
  return class_of((unsigned long)L.w[0] | ((unsigned long)(L.w[1] & 0xffffu) << 32));
}

// columns [A, B): blanks, an optional sign, digits with at most one '.', blanks.  0: a number, 1: all blank, 2: anything else.
// The value is the integer mantissa over 10^(digits behind the point) in fp64, rounded once to fp32.
template <int A, int B, int PIECES>
__device__ __forceinline__ int parse_fixed(const Line<PIECES>& L, float& value) {
  Digits d;
#pragma unroll
  for (int k = A; k < B; ++k) d.feed<true>(col(L, k));
  return d.fixed(value);
}
// columns [A, B): blanks, an optional sign, digits, blanks.  false: anything else (all blank included).
template <int A, int B, int PIECES>
__device__ __forceinline__ bool parse_int(const Line<PIECES>& L, int& value) {
  Digits d;
#pragma unroll
  for (int k = A; k < B; ++k) d.feed<false>(col(L, k));
  long v;
  const bool ok = d.integer(v);
  value = (int)v;
  return ok;
}

// (chainID, resSeq, iCode, HETATM or not) of a coordinate record as one word; the chain is the top byte
template <int PIECES>
__device__ __forceinline__ unsigned long key_of(const Line<PIECES>& L) {
  static_assert(PIECES >= 2, "the key ends in column 27");
  int seq = 0;
  parse_int<22, 26>(L, seq);
  const unsigned long het = class_of_line(L) == C_HETATM ? 1UL : 0UL;
  return ((unsigned long)col(L, 21) << 56) | ((unsigned long)col(L, 26) << 48) | (het << 40) | (unsigned long)(unsigned)seq;
}
__device__ __forceinline__ int chain_of_key(unsigned long key) { return (int)(key >> 56); }

// columns 13-16 stripped of blanks -> atom37 slot, or -1 (a name with a blank inside, or of four characters, is none of the 37)
__device__ __forceinline__ int slot_of(const Line<5>& L) {
  unsigned nm = 0;
  int cnt = 0, state = 0;
  bool bad = false;
#pragma unroll
  for (int k = 12; k < 16; ++k) {
    const unsigned c = col(L, k);
    if (c == ' ') {
      if (state == 1) state = 2;
    } else {
      if (state == 2 || cnt == 3) bad = true;
      else nm |= c << (8 * cnt), ++cnt;
      state = 1;
    }
  }
  if (bad || cnt == 0) return -1;
  return slot_of_name(nm);
}
__device__ __forceinline__ int aatype_of(const Line<5>& L) {
  return aatype_of_name(col(L, 17) | (col(L, 18) << 8) | (col(L, 19) << 16));
}

// 0, or the smallest kind of what is wrong with a coordinate record
__device__ __forceinline__ int check_record(const Line<5>& L) {
  if (L.len < 54) return FD_PDB_READ_SHORT;
  float v;
  int seq;
  if (parse_fixed<30, 38>(L, v) != 0 || parse_fixed<38, 46>(L, v) != 0 || parse_fixed<46, 54>(L, v) != 0) return FD_PDB_READ_COORD;
  if (parse_fixed<54, 60>(L, v) == 2 || parse_fixed<60, 66>(L, v) == 2) return FD_PDB_READ_NUMBER;
  if (!parse_int<22, 26>(L, seq)) return FD_PDB_READ_RESSEQ;
  return 0;
}

// Calls body(p, f, fs, fe, cls, run) for every line of the window in order, run describing the text in front of that line, and
// returns run behind the window's last line.
template <class Body>
__device__ __forceinline__ Run for_each_line(const Text& x, const Window& w, Run run, Body body) {
  unsigned m = w.starts;
  int f = w.f;
  while (m) {
    const int k = __builtin_ctz(m);
    m &= m - 1;
    const long p = w.ws + k;
    while (f + 1 < x.F && p >= x.off[f + 1]) ++f;
    const long fs = x.off[f], fe = file_end(x, f);
    const int cls = classify(x.t, p, fe);
    body(p, f, fs, fe, cls, run);
    if (cls == C_ENDMDL) run.nE += 1, run.lastE = p;
    else if (is_coord(x, cls)) run.lastC = p;
    run.nL += 1;
  }
  return run;
}
__device__ __forceinline__ Run window_summary(const Text& x, const Window& w) {
  return for_each_line(x, w, Run{0, 0, -1, -1}, [](long, int, long, long, int, const Run&) {});
}

// Calls on_record(p, f, fe, L, key, new_chain, run) for every SELECTED coordinate record of the window (model "first": no ENDMDL
// between the file's start and the record) that begins a residue; CHECK: also folds 8 (line index) + kind of malformed ones
// into bad.
template <bool CHECK, class OnStart>
__device__ __forceinline__ void for_each_start(const Text& x, const Window& w, const Run& before, long& bad, OnStart on_start) {
  for_each_line(x, w, before, [&](long p, int f, long fs, long fe, int cls, const Run& run) {
    if (!is_coord(x, cls) || !(x.model_all || run.lastE < fs)) return;
    Line<5> L;
    load_line<5, true>(x.t, p, fe, L);
    if (CHECK) {
      const int kind = check_record(L);
      if (kind) {
        const long word = 8 * run.nL + kind;
        bad = word < bad ? word : bad;
      }
    }
    const unsigned long key = key_of(L);
    // the coordinate record before this one: in the same file, and no ENDMDL between the two
    const bool has_prev = run.lastC >= fs && run.lastC >= 0 && run.lastC < p && run.lastE < run.lastC;
    bool new_res = true, new_chain = true;
    if (has_prev) {
      Line<2> K;
      load_line<2, false>(x.t, run.lastC, fe, K);
      const unsigned long kp = key_of(K);
      new_res = kp != key;
      new_chain = chain_of_key(kp) != chain_of_key(key);
    }
    if (new_res) on_start(p, f, fe, L, key, new_chain, run);
  });
}

// ---- fd_pdb_read_summary -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RT) void pdb_read_summary_kernel(Text x, long nchunks, long* __restrict__ summary) {
  __shared__ Run wtot[RWAVES];
  const long chunk = (long)blockIdx.x;
  const Window w = open_window(x, chunk * RCHUNK + (long)threadIdx.x * RW);
  Run total;
  block_scan(window_summary(x, w), wtot, total);
  if (threadIdx.x == 0) {
    summary[chunk] = total.nL;
    summary[nchunks + chunk] = total.nE;
    summary[2 * nchunks + chunk] = total.lastE;
    summary[3 * nchunks + chunk] = total.lastC;
  }
}

__device__ __forceinline__ Run carry_of(const long* __restrict__ carry, long nchunks, long chunk) {
  return Run{carry[chunk], carry[nchunks + chunk], carry[2 * nchunks + chunk], carry[3 * nchunks + chunk]};
}

// ---- fd_pdb_read_count ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RT) void pdb_read_count_kernel(Text x, long nchunks, const long* __restrict__ carry,
                                                            long* __restrict__ counts, long* __restrict__ file_first) {
  __shared__ Run wtot[RWAVES];
  __shared__ long wmin[RWAVES];
  const long chunk = (long)blockIdx.x;
  const Window w = open_window(x, chunk * RCHUNK + (long)threadIdx.x * RW);
  Run total;
  const Run before = join(carry_of(carry, nchunks, chunk), block_scan(window_summary(x, w), wtot, total));
  // the first line of a file records where the file begins among the lines and the ENDMDL records
  for_each_line(x, w, before, [&](long p, int f, long fs, long, int, const Run& run) {
    if (p == fs) file_first[f] = run.nL, file_first[x.F + f] = run.nE;
  });
  Run mine{0, 0, -1, -1};                         // (nL: residue starts, nE: chain starts)
  long bad = R_OK;
  for_each_start<true>(x, w, before, bad, [&](long, int, long, const Line<5>&, unsigned long, bool new_chain, const Run&) {
    mine.nL += 1;
    mine.nE += new_chain ? 1 : 0;
  });
  block_scan(mine, wtot, total);
  bad = block_min(bad, wmin);
  if (threadIdx.x == 0) {
    counts[chunk] = total.nL;
    counts[nchunks + chunk] = total.nE;
    counts[2 * nchunks + chunk] = bad;
  }
}

// ---- fd_pdb_read_fill ----------------------------------------------------------------------------------------------------------
struct Rows {
  long T, C;
  float* pos;                                     // [T,37,3]
  unsigned char* mask;                            // [T,37]
  float* b;                                       // [T,37]
  long* aatype;                                   // [T]
  long* res_index;                                // [T]
  int* dropped;                                   // [T]
  long* chain_first;                              // [C]
  int* chain_file;                                // [C]
  int* chain_model;                               // [C]
  int* chain_id;                                  // [C]
};

// the residue whose first record is L (at p): its lines in file order, the first record of a slot wins
__device__ __forceinline__ void place_residue(const Text& x, long fe, Line<5> L, unsigned long key, const Rows& o, long row) {
  unsigned long seen = 0;
  int dropped = 0;
  for (;;) {
    const int slot = slot_of(L);
    if (slot >= 0) {
      if ((seen >> slot) & 1UL) {
        ++dropped;
      } else {
        seen |= 1UL << slot;
        float px = 0.f, py = 0.f, pz = 0.f, occ = 1.f, bf = 0.f;
        parse_fixed<30, 38>(L, px);
        parse_fixed<38, 46>(L, py);
        parse_fixed<46, 54>(L, pz);
        parse_fixed<54, 60>(L, occ);              // (read and checked; the arrays do not hold it)
        parse_fixed<60, 66>(L, bf);
        float* q = o.pos + (row * R_SLOTS + slot) * 3;
        q[0] = px, q[1] = py, q[2] = pz;
        o.mask[row * R_SLOTS + slot] = 1;
        o.b[row * R_SLOTS + slot] = bf;
      }
    }
    int cls;
    do {                                          // the next coordinate record of this file and model
      const long p = L.end + 1;
      if (p >= fe) goto done;
      load_line<5, true>(x.t, p, fe, L);
      cls = class_of_line(L);
      if (cls == C_ENDMDL) goto done;
    } while (!is_coord(x, cls));
    if (key_of(L) != key) break;
  }
done:
  o.dropped[row] = dropped;
}

__global__ __launch_bounds__(RT) void pdb_read_fill_kernel(Text x, long nchunks, const long* __restrict__ carry,
                                                           const long* __restrict__ bases, const long* __restrict__ file_first,
                                                           Rows o) {
  __shared__ Run wtot[RWAVES];
  const long chunk = (long)blockIdx.x;
  const Window w = open_window(x, chunk * RCHUNK + (long)threadIdx.x * RW);
  Run total;
  const Run before = join(carry_of(carry, nchunks, chunk), block_scan(window_summary(x, w), wtot, total));
  Run mine{0, 0, -1, -1};                         // (nL: residue starts, nE: chain starts)
  long bad = R_OK;
  for_each_start<false>(x, w, before, bad, [&](long, int, long, const Line<5>&, unsigned long, bool new_chain, const Run&) {
    mine.nL += 1;
    mine.nE += new_chain ? 1 : 0;
  });
  const Run first = block_scan(mine, wtot, total);
  long row = bases[chunk] + first.nL, chain = bases[nchunks + chunk] + first.nE;
  for_each_start<false>(x, w, before, bad, [&](long, int f, long fe, const Line<5>& L, unsigned long key, bool new_chain,
                                               const Run& run) {
    if (new_chain && chain >= 0 && chain < o.C) {
      o.chain_first[chain] = row;
      o.chain_file[chain] = f;
      o.chain_model[chain] = (int)(run.nE - file_first[x.F + f]);
      o.chain_id[chain] = chain_of_key(key);
    }
    if (row >= 0 && row < o.T) {
      int seq = 0;
      parse_int<22, 26>(L, seq);
      o.aatype[row] = aatype_of(L);
      o.res_index[row] = seq;
      place_residue(x, fe, L, key, o, row);
    }
    row += 1;
    chain += new_chain ? 1 : 0;
  });
}

int check_text(const char* who, const unsigned char* text, long n, const long* file_offsets, int F) {
  FD_CHECK_ARG(n >= 1 && n <= FD_PDB_READ_MAX_BYTES && F >= 1, "%s: n must lie in 1 .. 2^40 and F be at least 1", who);
  FD_CHECK_ARG(text && file_offsets, "%s: null operand", who);
  FD_CHECK_ARG(fd_aligned16(text) && (((uintptr_t)file_offsets) & 7u) == 0, "%s: text must be 16-byte aligned", who);
  return FD_OK;
}

}  // namespace

extern "C" int fd_pdb_read_summary(const unsigned char* text, long n, const long* file_offsets, int F, int hetatm, long* summary,
                                   void* stream) {
  if (int rc = check_text("fd_pdb_read_summary", text, n, file_offsets, F)) return rc;
  FD_CHECK_ARG(summary && (((uintptr_t)summary) & 7u) == 0, "fd_pdb_read_summary: null or misaligned output");
  const long nchunks = (n + RCHUNK - 1) / RCHUNK;
  const Text x{text, n, file_offsets, F, hetatm, 0};
  hipLaunchKernelGGL(pdb_read_summary_kernel, dim3((unsigned)nchunks), dim3(RT), 0, (hipStream_t)stream, x, nchunks, summary);
  FD_CHECK_LAUNCH("fd_pdb_read_summary");
  return FD_OK;
}

extern "C" int fd_pdb_read_count(const unsigned char* text, long n, const long* file_offsets, int F, int hetatm, int model_all,
                                 const long* carry, long* counts, long* file_first, void* stream) {
  if (int rc = check_text("fd_pdb_read_count", text, n, file_offsets, F)) return rc;
  FD_CHECK_ARG(carry && counts && file_first, "fd_pdb_read_count: null operand");
  FD_CHECK_ARG(((((uintptr_t)carry) | ((uintptr_t)counts) | ((uintptr_t)file_first)) & 7u) == 0, "fd_pdb_read_count: misaligned operand");
  const long nchunks = (n + RCHUNK - 1) / RCHUNK;
  const Text x{text, n, file_offsets, F, hetatm, model_all};
  hipLaunchKernelGGL(pdb_read_count_kernel, dim3((unsigned)nchunks), dim3(RT), 0, (hipStream_t)stream, x, nchunks, carry, counts,
                     file_first);
  FD_CHECK_LAUNCH("fd_pdb_read_count");
  return FD_OK;
}

extern "C" int fd_pdb_read_fill(const unsigned char* text, long n, const long* file_offsets, int F, int hetatm, int model_all,
                                const long* carry, const long* bases, const long* file_first, long T, long C,
                                float* atom_positions, unsigned char* atom_mask, float* b_factors, long* aatype, long* residue_index,
                                int* row_dropped, long* chain_first, int* chain_file, int* chain_model, int* chain_id, void* stream) {
  if (int rc = check_text("fd_pdb_read_fill", text, n, file_offsets, F)) return rc;
  FD_CHECK_ARG(T >= 0 && C >= 0, "fd_pdb_read_fill: negative size");
  if (T == 0) return FD_OK;
  FD_CHECK_ARG(carry && bases && file_first && atom_positions && atom_mask && b_factors && aatype && residue_index && row_dropped &&
                   chain_first && chain_file && chain_model && chain_id, "fd_pdb_read_fill: null operand");
  const long nchunks = (n + RCHUNK - 1) / RCHUNK;
  const Text x{text, n, file_offsets, F, hetatm, model_all};
  const Rows o{T, C, atom_positions, atom_mask, b_factors, aatype, residue_index, row_dropped, chain_first, chain_file, chain_model,
               chain_id};
  hipLaunchKernelGGL(pdb_read_fill_kernel, dim3((unsigned)nchunks), dim3(RT), 0, (hipStream_t)stream, x, nchunks, carry, bases,
                     file_first, o);
  FD_CHECK_LAUNCH("fd_pdb_read_fill");
  return FD_OK;
}
