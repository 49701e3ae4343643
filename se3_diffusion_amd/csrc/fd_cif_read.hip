// fd_cif_read_lines / _marks / _header / _summary / _count / _fill: atom37 arrays from the atom_site loop of mmCIF files in HBM.
// include/fd_hip.h is the specification; this file says how the six launches are laid out.  The layout is fd_pdb_read.hip's (a
// thread owns a window of 16 bytes, a block a chunk of 4096, a line belongs to the thread whose window holds its first byte and
// that thread tokenises it serially; fd_text_read.h holds what the two readers share), but what a line IS depends on more of the
// text in front of it than in PDB, so what the ordered scan carries is found in stages.  Each launch finds the next rows of
// carry [8,nchunks] per chunk, the caller turns them into "of all chunks in front" (cumsum, cummax), and every later launch
// repeats the earlier stages inside its block:
//
//   lines    per chunk: lines, ';'-lines, and the ';'-lines in front of the chunk's last file start.  With these every line
//            knows whether it lies inside a text field (the ';'-lines of its file in front of it are odd in number).
//   marks    the position of the last loop_ line, _atom_site. tag line, other non-value line and atom_site loop head (a loop_
//            line whose next non-blank line is an _atom_site. tag line).  With these every value line knows whether it is a row
//            of the atom_site loop.
//   header   the thread of a file's first head walks the tag lines and writes the file's column table, then walks on to the
//            file's first coordinate record for its model number.  No row can be parsed before this.
//   summary  the position of the last coordinate record (the rows that are not HETATM, or all with hetatm).
//   count    as fd_pdb_read_count: a coordinate record is tokenised and checked by its thread and begins a residue row when
//            its key differs from that of the record before it, which the thread tokenises where the scan says it lies.
//   fill     the same analysis; a thread remembers the starts of its window by their byte in it, the block scans their numbers
//            into row and chain numbers, and the thread of a residue's first record walks that residue's rows in file order: the
//            first record of a slot wins, so the result does not depend on any order of execution.  No atomics anywhere.
// A thread reads the text through a cursor of eight aligned bytes (Bytes): a row of 80 bytes costs about ten loads, not 80.
#include "fd_text_read.h"

namespace {

constexpr int MAXC = FD_CIF_MAX_COLS;
constexpr int MAXL = FD_CIF_MAX_LINE;
constexpr int TAB = FD_CIF_TABLE;                 // ints of a file's column table: the field of each column, columns, first model
static_assert(TAB == MAXC + 2 && MAXL < 32768, "a table is the fields, the column count and the first model; spans are shorts");

enum { L_BLANK = 0, L_VALUE, L_LOOP, L_TAG, L_OTHER, L_SEMI };
// the fields of a row that are read
enum { F_GROUP = 0, F_ATOM, F_ALT, F_COMP, F_CHAIN, F_SEQ, F_INS, F_X, F_Y, F_Z, F_OCC, F_B, F_MODEL, NFIELD };
// the tag names that are known, lower case, in the order of the fields; the two label_ ids stand behind them
enum { N_LABEL_ASYM = NFIELD, N_LABEL_SEQ, NNAME };
// a name of at most 24 bytes in three words, the first byte lowest; longer names are none of the known ones
struct Name {
  unsigned long w[3];
};
constexpr Name pack24(const char* s) {
  Name v{{0, 0, 0}};
  for (int k = 0; k < 24 && s[k]; ++k) v.w[k >> 3] |= (unsigned long)(unsigned char)s[k] << (8 * (k & 7));
  return v;
}
__device__ const Name kName[NNAME] = {pack24("group_pdb"),     pack24("label_atom_id"),      pack24("label_alt_id"),  pack24("label_comp_id"),
                                      pack24("auth_asym_id"),  pack24("auth_seq_id"),        pack24("pdbx_pdb_ins_code"), pack24("cartn_x"),
                                      pack24("cartn_y"),       pack24("cartn_z"),            pack24("occupancy"),     pack24("b_iso_or_equiv"),
                                      pack24("pdbx_pdb_model_num"), pack24("label_asym_id"), pack24("label_seq_id")};

// The text read eight aligned bytes at a time: t[q] for q < n.  The last word is put together from single bytes, so nothing outside
// the text is read (the text is 16-byte aligned).  (A cursor of 32 bytes was measured slower: the walk is bound by its
// instructions and its divergence, not by the loads.)
struct Bytes {
  const unsigned char* base;
  long n;
  long at;
  unsigned long w;
  __device__ __forceinline__ Bytes(const Text& x) : base(x.t), n(x.n), at(-1), w(0) {}
  __device__ __forceinline__ unsigned operator[](long q) {
    const long b = q & ~7L;
    if (b != at) {
      at = b;
      if (b + 8 <= n) {
        __builtin_memcpy(&w, base + b, 8);
      } else {
        w = 0;
        for (int k = 0; b + k < n; ++k) w |= (unsigned long)base[b + k] << (8 * k);
      }
    }
    return (unsigned)(w >> (8 * (q & 7))) & 0xffu;
  }
};

__device__ __forceinline__ bool is_blank(unsigned c) { return c == ' ' || c == '\t'; }
__device__ __forceinline__ unsigned lower(unsigned c) { return c >= 'A' && c <= 'Z' ? c | 0x20u : c; }
// q is at the end of its line: the file's end, a '\n', or a '\r' directly in front of either
__device__ __forceinline__ bool at_end(Bytes& t, long q, long fe) {
  if (q >= fe) return true;
  const unsigned c = t[q];
  return c == '\n' || (c == '\r' && (q + 1 >= fe || t[q + 1] == '\n'));
}
// the position of the '\n' of the line that holds q, or the file's end
__device__ __forceinline__ long line_end(Bytes& t, long q, long fe) {
  while (q < fe && t[q] != '\n') ++q;
  return q;
}
// the n bytes at q equal kw (lower case) without regard to case; the line does not end among them
__device__ __forceinline__ bool match(Bytes& t, long q, long fe, const char* kw, int n) {
  for (int k = 0; k < n; ++k)
    if (at_end(t, q + k, fe) || lower(t[q + k]) != (unsigned)(unsigned char)kw[k]) return false;
  return true;
}

// The class of the line at p as if it stood outside every text field.  A tag line: name is where the tag's name begins (behind
// "_atom_site.") and name_len its length.
__device__ __forceinline__ int classify(Bytes& t, long p, long fe, long& name, int& name_len) {
  if (t[p] == ';') return L_SEMI;
  long q = p;
  while (!at_end(t, q, fe) && is_blank(t[q])) ++q;
  if (at_end(t, q, fe)) return L_BLANK;
  const unsigned c = t[q];
  if (c == '#') return L_OTHER;
  if (c == '_') {
    if (!match(t, q, fe, "_atom_site.", 11)) return L_OTHER;
    long r = q + 11;
    name = r;
    while (!at_end(t, r, fe) && !is_blank(t[r])) ++r;
    name_len = (int)(r - name);
    while (!at_end(t, r, fe) && is_blank(t[r])) ++r;
    return at_end(t, r, fe) || t[r] == '#' ? L_TAG : L_OTHER;     // (a value behind the tag: the key-value form)
  }
  if (match(t, q, fe, "loop_", 5) && (at_end(t, q + 5, fe) || is_blank(t[q + 5]))) return L_LOOP;
  if (match(t, q, fe, "data_", 5)) return L_OTHER;
  return L_VALUE;
}
__device__ __forceinline__ int classify(Bytes& t, long p, long fe) {
  long name;
  int len;
  return classify(t, p, fe, name, len);
}
// the loop_ line at p heads an atom_site loop: the next line of its file that is not blank is an _atom_site. tag line
__device__ __forceinline__ bool is_head(Bytes& t, long p, long fe) {
  for (long q = line_end(t, p, fe) + 1; q < fe; q = line_end(t, q, fe) + 1) {
    const int c = classify(t, q, fe);
    if (c != L_BLANK) return c == L_TAG;
  }
  return false;
}

// What a thread knows of the text in front of a line.  Counts add; fileS, the ';'-lines in front of the last file start, is
// counted from where the run begins (-1: no file starts in it); positions take the later one (-1: none).
struct Run {
  long nL, nS, fileS, loop, tag, other, head, rec;
  static __device__ __forceinline__ Run none() { return Run{0, 0, -1, -1, -1, -1, -1, -1}; }
};
__device__ __forceinline__ long later(long a, long b) { return b > a ? b : a; }
__device__ __forceinline__ Run join(const Run& a, const Run& b) {
  return Run{a.nL + b.nL, a.nS + b.nS, b.fileS >= 0 ? a.nS + b.fileS : a.fileS, later(a.loop, b.loop), later(a.tag, b.tag),
             later(a.other, b.other), later(a.head, b.head), later(a.rec, b.rec)};
}
__device__ __forceinline__ Run shfl_run(const Run& r, int src) {
  return Run{__shfl(r.nL, src), __shfl(r.nS, src), __shfl(r.fileS, src), __shfl(r.loop, src),
             __shfl(r.tag, src),  __shfl(r.other, src), __shfl(r.head, src),  __shfl(r.rec, src)};
}
__device__ __forceinline__ Run positions_of(const Run& r) { return Run{0, 0, -1, r.loop, r.tag, r.other, r.head, r.rec}; }
__device__ __forceinline__ Run carry_of(const long* __restrict__ carry, long nchunks, long chunk) {
  return Run{carry[chunk], carry[nchunks + chunk], carry[2 * nchunks + chunk], carry[3 * nchunks + chunk],
             carry[4 * nchunks + chunk], carry[5 * nchunks + chunk], carry[6 * nchunks + chunk], carry[7 * nchunks + chunk]};
}
// the value line behind run, in the file that starts at fs, is a row of the atom_site loop
__device__ __forceinline__ bool is_row(const Run& run, long fs) {
  return run.loop >= fs && run.head == run.loop && run.tag > run.loop && run.loop > run.other;
}

// ---- a row ---------------------------------------------------------------------------------------------------------------------
// where the tokens of the fields lie (from the line's first byte; n < 0: none), and the row's end
struct Row {
  short a[NFIELD], n[NFIELD];
  bool ok;                                        // tokenised: not too long, every quote closed, as many tokens as tags
  long p, end;                                    // the line's first byte, and the position of its '\n' or the file's end
};
// KIND_ONLY: stops behind the group_PDB token (only is_hetatm is to be asked of r then)
template <bool KIND_ONLY = false>
__device__ __forceinline__ void tokenize(Bytes& t, long p, long fe, const int* __restrict__ tab, Row& r) {
#pragma unroll
  for (int f = 0; f < NFIELD; ++f) r.a[f] = 0, r.n[f] = -1;
  r.p = p;
  r.end = line_end(t, p, fe);
  const long ce = r.end > p && t[r.end - 1] == '\r' ? r.end - 1 : r.end;
  r.ok = false;
  if (ce - p > MAXL) return;
  long q = p;
  int k = 0;
  for (;;) {
    while (q < ce && is_blank(t[q])) ++q;
    if (q >= ce) break;
    const unsigned c = t[q];
    if (c == '#') break;
    long s = q;
    int len;
    if (c == '\'' || c == '"') {
      s = q + 1;
      long z = s;
      while (z < ce && !(t[z] == c && (z + 1 >= ce || is_blank(t[z + 1])))) ++z;
      if (z >= ce) return;                        // an unclosed quote
      len = (int)(z - s);
      q = z + 1;
    } else {
      while (q < ce && !is_blank(t[q])) ++q;
      len = (int)(q - s);
    }
    const int fld = k < MAXC ? tab[k] : -1;
#pragma unroll
    for (int f = 0; f < NFIELD; ++f)
      if (fld == f) r.a[f] = (short)(s - p), r.n[f] = (short)len;
    if (KIND_ONLY && fld == F_GROUP) return;
    ++k;
  }
  r.ok = k == tab[MAXC];
}
template <int FIELD>
__device__ __forceinline__ bool missing(Bytes& t, const Row& r) {   // none, '.' or '?'
  return r.n[FIELD] < 0 || (r.n[FIELD] == 1 && (t[r.p + r.a[FIELD]] == '.' || t[r.p + r.a[FIELD]] == '?'));
}
__device__ __forceinline__ bool is_hetatm(Bytes& t, const Row& r) {
  if (r.n[F_GROUP] != 6) return false;
  const long g = r.p + r.a[F_GROUP];
  return t[g] == 'H' && t[g + 1] == 'E' && t[g + 2] == 'T' && t[g + 3] == 'A' && t[g + 4] == 'T' && t[g + 5] == 'M';
}
// tokenises the value line at p; true: a coordinate record
__device__ __forceinline__ bool coord_row(const Text& x, Bytes& t, const int* __restrict__ tab, long p, long fe, Row& r) {
  tokenize(t, p, fe, tab, r);
  return x.hetatm || !is_hetatm(t, r);
}
// the same answer without the row: nothing is read where every row is a coordinate record
__device__ __forceinline__ bool is_coord_row(const Text& x, Bytes& t, const int* __restrict__ tab, long p, long fe) {
  if (x.hetatm) return true;
  Row r;
  tokenize<true>(t, p, fe, tab, r);
  return !is_hetatm(t, r);
}
// 0: a number, 1: none, '.' or '?', 2: anything else
template <int FIELD>
__device__ __forceinline__ int number_of(Bytes& t, const Row& r, float& value) {
  if (missing<FIELD>(t, r)) return 1;
  Digits d;
  for (int k = 0; k < r.n[FIELD]; ++k) d.feed<true>(t[r.p + r.a[FIELD] + k] == ' ' ? 'x' : t[r.p + r.a[FIELD] + k]);
  const int rc = d.fixed(value);
  return rc == 1 ? 2 : rc;
}
template <int FIELD>
__device__ __forceinline__ bool integer_of(Bytes& t, const Row& r, int& value) {
  Digits d;
  for (int k = 0; k < r.n[FIELD]; ++k) d.feed<false>(t[r.p + r.a[FIELD] + k] == ' ' ? 'x' : t[r.p + r.a[FIELD] + k]);
  long v = 0;
  const bool ok = d.integer(v) && v <= 0x7fffffffL && v >= -0x7fffffffL;
  value = ok ? (int)v : 0;
  return ok;
}
// the model number (no such column: 1); false: not an integer
__device__ __forceinline__ bool model_of(Bytes& t, const Row& r, int& model) {
  model = 1;
  return r.n[F_MODEL] < 0 || integer_of<F_MODEL>(t, r, model);
}
// the chain ID's 1 to 4 bytes, the first lowest ('.' or '?': a blank); false: none or longer
__device__ __forceinline__ bool chain_of(Bytes& t, const Row& r, int& chain) {
  chain = 32;
  if (r.n[F_CHAIN] < 1 || r.n[F_CHAIN] > 4) return false;
  if (missing<F_CHAIN>(t, r)) return true;
  unsigned v = 0;
  for (int k = 0; k < r.n[F_CHAIN]; ++k) v |= (unsigned)t[r.p + r.a[F_CHAIN] + k] << (8 * k);
  chain = (int)v;
  return true;
}
struct Key {
  int chain, seq, ins, het, model;
};
__device__ __forceinline__ bool same(const Key& a, const Key& b) {
  return a.chain == b.chain && a.seq == b.seq && a.ins == b.ins && a.het == b.het && a.model == b.model;
}
__device__ __forceinline__ Key key_of(Bytes& t, const Row& r) {
  Key k;
  chain_of(t, r, k.chain);
  integer_of<F_SEQ>(t, r, k.seq);
  k.ins = missing<F_INS>(t, r) || r.n[F_INS] < 1 ? 32 : (int)t[r.p + r.a[F_INS]];
  k.het = is_hetatm(t, r) ? 1 : 0;
  model_of(t, r, k.model);
  return k;
}
__device__ __forceinline__ unsigned name3(Bytes& t, const Row& r, int a, int n) {
  unsigned nm = 0;
  for (int k = 0; k < n; ++k) nm |= (unsigned)t[r.p + a + k] << (8 * k);
  return nm;
}
__device__ __forceinline__ int slot_of(Bytes& t, const Row& r) {
  return r.n[F_ATOM] >= 1 && r.n[F_ATOM] <= 3 ? slot_of_name(name3(t, r, r.a[F_ATOM], r.n[F_ATOM])) : -1;
}
__device__ __forceinline__ int aatype_of(Bytes& t, const Row& r) {
  return r.n[F_COMP] == 3 ? aatype_of_name(name3(t, r, r.a[F_COMP], 3)) : 20;
}
// 0, or the smallest kind of what is wrong with a coordinate record; selected: the record is of a model that is read
__device__ __forceinline__ int check_row(const Text& x, Bytes& t, const int* __restrict__ tab, const Row& r, bool& selected) {
  selected = true;
  if (!r.ok) return FD_CIF_READ_TOKENS;
  int model, v;
  const bool model_ok = model_of(t, r, model);
  if (model_ok && !x.model_all && model != tab[MAXC + 1]) {
    selected = false;
    return 0;
  }
  float w;
  if (number_of<F_X>(t, r, w) != 0 || number_of<F_Y>(t, r, w) != 0 || number_of<F_Z>(t, r, w) != 0) return FD_CIF_READ_COORD;
  if (number_of<F_OCC>(t, r, w) == 2 || number_of<F_B>(t, r, w) == 2) return FD_CIF_READ_NUMBER;
  if (!integer_of<F_SEQ>(t, r, v)) return FD_CIF_READ_RESSEQ;
  if (!chain_of(t, r, v)) return FD_CIF_READ_CHAIN;
  return model_ok ? 0 : FD_CIF_READ_MODEL;
}

// ---- lines ---------------------------------------------------------------------------------------------------------------------
// Calls body(p, f, fs, fe, cls, run, t) for every line of the window in order, run describing the text in front of that line, and
// returns run behind the window's last line.  LEVEL says how much of run is known of the text in front of the window, and so what
// cls can be trusted for: 1 nothing (cls is not to be used), 2 the lines and ';'-lines (cls is right), 3 the marks too (is_row is
// right), 4 the column tables too (the coordinate records are found).
template <int LEVEL, class Body>
__device__ __forceinline__ Run for_each_line(const Text& x, const int* __restrict__ table, const Window& w, Run run, Body body) {
  unsigned m = w.starts;
  int f = w.f;
  Bytes t(x);
  while (m) {
    const int k = __builtin_ctz(m);
    m &= m - 1;
    const long p = w.ws + k;
    while (f + 1 < x.F && p >= x.off[f + 1]) ++f;
    const long fs = x.off[f], fe = file_end(x, f);
    if (p == fs) run.fileS = run.nS;
    const int raw = LEVEL == 1 ? (t[p] == ';' ? L_SEMI : L_OTHER) : classify(t, p, fe);
    const int cls = raw == L_SEMI || ((run.nS - run.fileS) & 1) ? L_OTHER : raw;
    body(p, f, fs, fe, cls, run, t);
    run.nL += 1;
    run.nS += raw == L_SEMI ? 1 : 0;
    if (LEVEL >= 2) {
      if (cls == L_LOOP) {
        run.loop = p;
        if (is_head(t, p, fe)) run.head = p;
      } else if (cls == L_TAG) {
        run.tag = p;
      } else if (cls == L_OTHER) {
        run.other = p;
      }
    }
    if (LEVEL >= 4 && cls == L_VALUE && is_row(run, fs) && is_coord_row(x, t, table + (long)f * TAB, p, fe)) run.rec = p;
  }
  return run;
}
template <int LEVEL>
__device__ __forceinline__ Run window_summary(const Text& x, const int* __restrict__ table, const Window& w, const Run& run) {
  return for_each_line<LEVEL>(x, table, w, run, [](long, int, long, long, int, const Run&, Bytes&) {});
}
// run in front of the window, known well enough for for_each_line<LEVEL>: the earlier stages again, each scanned through the block
template <int LEVEL>
__device__ __forceinline__ Run before_window(const Text& x, const int* __restrict__ table, const Window& w, const long* __restrict__ carry,
                                             long nchunks, Run* wtot) {
  Run total;
  Run before = join(carry_of(carry, nchunks, (long)blockIdx.x), block_scan(window_summary<1>(x, table, w, Run::none()), wtot, total));
  if (LEVEL > 2) before = join(before, block_scan(positions_of(window_summary<2>(x, table, w, before)), wtot, total));
  if (LEVEL > 4) before = join(before, block_scan(positions_of(window_summary<4>(x, table, w, before)), wtot, total));
  return before;
}

// ---- fd_cif_read_lines -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RT) void cif_read_lines_kernel(Text x, long nchunks, long* __restrict__ lines) {
  __shared__ Run wtot[RWAVES];
  const long chunk = (long)blockIdx.x;
  const Window w = open_window(x, chunk * RCHUNK + (long)threadIdx.x * RW);
  Run total;
  block_scan(window_summary<1>(x, nullptr, w, Run::none()), wtot, total);
  if (threadIdx.x == 0) {
    lines[chunk] = total.nL;
    lines[nchunks + chunk] = total.nS;
    lines[2 * nchunks + chunk] = total.fileS;
  }
}

// ---- fd_cif_read_marks -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RT) void cif_read_marks_kernel(Text x, long nchunks, const long* __restrict__ carry, long* __restrict__ marks) {
  __shared__ Run wtot[RWAVES];
  const long chunk = (long)blockIdx.x;
  const Window w = open_window(x, chunk * RCHUNK + (long)threadIdx.x * RW);
  const Run before = before_window<2>(x, nullptr, w, carry, nchunks, wtot);
  Run total;
  block_scan(positions_of(window_summary<2>(x, nullptr, w, before)), wtot, total);
  if (threadIdx.x == 0) {
    marks[chunk] = total.loop;
    marks[nchunks + chunk] = total.tag;
    marks[2 * nchunks + chunk] = total.other;
    marks[3 * nchunks + chunk] = total.head;
  }
}

// ---- fd_cif_read_header ----------------------------------------------------------------------------------------------------------
// The header of the loop whose loop_ line is at p: the file's column table; 0 or FD_CIF_READ_COLUMNS.
__device__ __forceinline__ int read_header(const Text& x, Bytes& t, int ids_label, long p, long fe, int* __restrict__ tab) {
  long q = line_end(t, p, fe) + 1;
  int k = 0;
  unsigned have = 0;
  while (q < fe) {
    long name = 0;
    int len = 0;
    const int c = classify(t, q, fe, name, len);
    if (c != L_BLANK) {
      if (c != L_TAG) break;
      int id = -1;
      if (len <= 24) {
        Name nm{{0, 0, 0}};
        for (int j = 0; j < len; ++j) nm.w[j >> 3] |= (unsigned long)lower(t[name + j]) << (8 * (j & 7));
        for (int i = 0; i < NNAME; ++i)
          if (kName[i].w[0] == nm.w[0] && kName[i].w[1] == nm.w[1] && kName[i].w[2] == nm.w[2]) id = i;
      }
      if (k < MAXC) tab[k] = id;
      if (id >= 0) have |= 1u << id;
      ++k;
    }
    q = line_end(t, q, fe) + 1;
  }
  // the chain and the residue number: the auth_ columns, the label_ ones where those are absent or ids_label says so
  const int chain = !ids_label && ((have >> F_CHAIN) & 1u) ? (int)F_CHAIN : (int)N_LABEL_ASYM;
  const int seq = !ids_label && ((have >> F_SEQ) & 1u) ? (int)F_SEQ : (int)N_LABEL_SEQ;
  for (int j = 0; j < MAXC; ++j) {
    const int id = j < k ? tab[j] : -1;
    tab[j] = id == chain ? F_CHAIN : id == seq ? F_SEQ : id == F_CHAIN || id == F_SEQ || id >= NFIELD ? -1 : id;
  }
  tab[MAXC] = k;
  tab[MAXC + 1] = 0;
  const unsigned need = (1u << F_ATOM) | (1u << F_ALT) | (1u << F_COMP) | (1u << F_X) | (1u << F_Y) | (1u << F_Z) | (1u << chain) | (1u << seq);
  if (k > MAXC || (have & need) != need) return FD_CIF_READ_COLUMNS;
  // the model number of the file's first coordinate record
  while (q < fe) {
    const int c = classify(t, q, fe);
    if (c == L_BLANK) {
      q = line_end(t, q, fe) + 1;
      continue;
    }
    if (c != L_VALUE) break;
    Row r;
    if (coord_row(x, t, tab, q, fe, r)) {
      int model = 0;
      tab[MAXC + 1] = model_of(t, r, model) ? model : 0;
      break;
    }
    q = r.end + 1;
  }
  return 0;
}
__global__ __launch_bounds__(RT) void cif_read_header_kernel(Text x, long nchunks, int ids_label, const long* __restrict__ carry,
                                                             int* __restrict__ table, long* __restrict__ file_first,
                                                             long* __restrict__ bad_of) {
  __shared__ Run wtot[RWAVES];
  __shared__ long wmin[RWAVES];
  const long chunk = (long)blockIdx.x;
  const Window w = open_window(x, chunk * RCHUNK + (long)threadIdx.x * RW);
  const Run before = before_window<3>(x, nullptr, w, carry, nchunks, wtot);
  long bad = R_OK;
  for_each_line<2>(x, nullptr, w, before, [&](long p, int f, long fs, long fe, int cls, const Run& run, Bytes& t) {
    if (p == fs) file_first[f] = run.nL;
    if (cls != L_LOOP || !is_head(t, p, fe)) return;
    // a second atom_site loop of the file is refused where it begins and leaves the table alone
    const int kind = run.head >= fs ? FD_CIF_READ_COLUMNS : read_header(x, t, ids_label, p, fe, table + (long)f * TAB);
    if (kind) {
      const long word = 8 * run.nL + kind;
      bad = word < bad ? word : bad;
    }
  });
  bad = block_min(bad, wmin);
  if (threadIdx.x == 0) bad_of[chunk] = bad;
}

// ---- fd_cif_read_summary ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RT) void cif_read_summary_kernel(Text x, long nchunks, const long* __restrict__ carry,
                                                              const int* __restrict__ table, long* __restrict__ last) {
  __shared__ Run wtot[RWAVES];
  const long chunk = (long)blockIdx.x;
  const Window w = open_window(x, chunk * RCHUNK + (long)threadIdx.x * RW);
  const Run before = before_window<4>(x, table, w, carry, nchunks, wtot);
  Run total;
  block_scan(positions_of(window_summary<4>(x, table, w, before)), wtot, total);
  if (threadIdx.x == 0) last[chunk] = total.rec;
}

// Calls on_start(p, f, fe, tab, r, key, new_chain, t) for every SELECTED coordinate record of the window that begins a residue;
// CHECK: also folds 8 (line index) + kind of malformed ones into bad.
template <bool CHECK, class OnStart>
__device__ __forceinline__ void for_each_start(const Text& x, const int* __restrict__ table, const Window& w, const Run& before, long& bad,
                                               OnStart on_start) {
  for_each_line<4>(x, table, w, before, [&](long p, int f, long fs, long fe, int cls, const Run& run, Bytes& t) {
    if (cls != L_VALUE || !is_row(run, fs)) return;
    const int* tab = table + (long)f * TAB;
    Row r;
    if (!coord_row(x, t, tab, p, fe, r)) return;
    bool selected;
    const int kind = check_row(x, t, tab, r, selected);
    if (!selected) return;
    if (CHECK && kind) {
      const long word = 8 * run.nL + kind;
      bad = word < bad ? word : bad;
    }
    const Key key = key_of(t, r);
    bool new_res = true, new_chain = true;
    if (run.rec >= fs && run.rec < p) {           // the coordinate record before this one, in the same file
      Row q;
      tokenize(t, run.rec, fe, tab, q);
      const Key kp = key_of(t, q);
      new_res = !same(kp, key);
      new_chain = kp.chain != key.chain || kp.model != key.model;
    }
    if (new_res) on_start(p, f, fe, tab, r, key, new_chain, t);
  });
}

// ---- fd_cif_read_count -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RT) void cif_read_count_kernel(Text x, long nchunks, const long* __restrict__ carry,
                                                            const int* __restrict__ table, long* __restrict__ counts) {
  __shared__ Run wtot[RWAVES];
  __shared__ long wmin[RWAVES];
  const long chunk = (long)blockIdx.x;
  const Window w = open_window(x, chunk * RCHUNK + (long)threadIdx.x * RW);
  const Run before = before_window<5>(x, table, w, carry, nchunks, wtot);
  Run mine = Run::none();                         // (nL: residue starts, nS: chain starts)
  long bad = R_OK;
  for_each_start<true>(x, table, w, before, bad, [&](long, int, long, const int*, const Row&, const Key&, bool new_chain, Bytes&) {
    mine.nL += 1;
    mine.nS += new_chain ? 1 : 0;
  });
  Run total;
  block_scan(mine, wtot, total);
  bad = block_min(bad, wmin);
  if (threadIdx.x == 0) {
    counts[chunk] = total.nL;
    counts[nchunks + chunk] = total.nS;
    counts[2 * nchunks + chunk] = bad;
  }
}

// ---- fd_cif_read_fill ------------------------------------------------------------------------------------------------------------
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

// the residue whose first record is r: its rows in file order, the first record of a slot wins
__device__ __forceinline__ void place_residue(const Text& x, Bytes& t, const int* __restrict__ tab, long fe, Row r, const Key& key,
                                              const Rows& o, long row) {
  unsigned long seen = 0;
  int dropped = 0;
  for (;;) {
    const int slot = slot_of(t, r);
    if (slot >= 0) {
      if ((seen >> slot) & 1UL) {
        ++dropped;
      } else {
        seen |= 1UL << slot;
        float px = 0.f, py = 0.f, pz = 0.f, bf = 0.f;
        number_of<F_X>(t, r, px);
        number_of<F_Y>(t, r, py);
        number_of<F_Z>(t, r, pz);
        number_of<F_B>(t, r, bf);               // (the occupancy is checked; the arrays do not hold it)
        float* q = o.pos + (row * R_SLOTS + slot) * 3;
        q[0] = px, q[1] = py, q[2] = pz;
        o.mask[row * R_SLOTS + slot] = 1;
        o.b[row * R_SLOTS + slot] = bf;
      }
    }
    bool coord = false;
    long p = r.end + 1;
    while (!coord) {                              // the next coordinate record of the loop
      if (p >= fe) goto done;
      const int c = classify(t, p, fe);
      if (c == L_BLANK) {
        p = line_end(t, p, fe) + 1;
        continue;
      }
      if (c != L_VALUE) goto done;
      coord = coord_row(x, t, tab, p, fe, r);
      p = r.end + 1;
    }
    if (!same(key_of(t, r), key)) break;
  }
done:
  o.dropped[row] = dropped;
}

__global__ __launch_bounds__(RT) void cif_read_fill_kernel(Text x, long nchunks, const long* __restrict__ carry,
                                                           const int* __restrict__ table, const long* __restrict__ bases, Rows o) {
  __shared__ Run wtot[RWAVES];
  const long chunk = (long)blockIdx.x;
  const Window w = open_window(x, chunk * RCHUNK + (long)threadIdx.x * RW);
  const Run before = before_window<5>(x, table, w, carry, nchunks, wtot);
  // one analysis: the starts of the window are remembered by their byte in it, scanned into row and chain numbers, then acted on
  Run mine = Run::none();                         // (nL: residue starts, nS: chain starts)
  long bad = R_OK;
  unsigned starts = 0, chains = 0;
  for_each_start<false>(x, table, w, before, bad, [&](long p, int, long, const int*, const Row&, const Key&, bool new_chain, Bytes&) {
    mine.nL += 1;
    mine.nS += new_chain ? 1 : 0;
    starts |= 1u << (int)(p - w.ws);
    chains |= (new_chain ? 1u : 0u) << (int)(p - w.ws);
  });
  Run total;
  const Run first = block_scan(mine, wtot, total);
  long row = bases[chunk] + first.nL, chain = bases[nchunks + chunk] + first.nS;
  Bytes t(x);
  int f = w.f;
  while (starts) {
    const int k = __builtin_ctz(starts);
    starts &= starts - 1;
    const long p = w.ws + k;
    while (f + 1 < x.F && p >= x.off[f + 1]) ++f;
    const long fe = file_end(x, f);
    const int* tab = table + (long)f * TAB;
    const bool new_chain = (chains >> k) & 1u;
    Row r;
    tokenize(t, p, fe, tab, r);
    const Key key = key_of(t, r);
    if (new_chain && chain >= 0 && chain < o.C) {
      o.chain_first[chain] = row;
      o.chain_file[chain] = f;
      o.chain_model[chain] = key.model - tab[MAXC + 1];
      o.chain_id[chain] = key.chain;
    }
    if (row >= 0 && row < o.T) {
      o.aatype[row] = aatype_of(t, r);
      o.res_index[row] = key.seq;
      place_residue(x, t, tab, fe, r, key, o, row);
    }
    row += 1;
    chain += new_chain ? 1 : 0;
  }
}

int check_text(const char* who, const unsigned char* text, long n, const long* file_offsets, int F) {
  FD_CHECK_ARG(n >= 1 && n <= FD_PDB_READ_MAX_BYTES && F >= 1, "%s: n must lie in 1 .. 2^40 and F be at least 1", who);
  FD_CHECK_ARG(text && file_offsets, "%s: null operand", who);
  FD_CHECK_ARG(fd_aligned16(text) && (((uintptr_t)file_offsets) & 7u) == 0, "%s: text must be 16-byte aligned", who);
  return FD_OK;
}
bool aligned8(const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr) {
  return ((((uintptr_t)a) | ((uintptr_t)b) | ((uintptr_t)c) | ((uintptr_t)d)) & 7u) == 0;
}
long chunks_of(long n) { return (n + RCHUNK - 1) / RCHUNK; }

}  // namespace

extern "C" int fd_cif_read_lines(const unsigned char* text, long n, const long* file_offsets, int F, long* lines, void* stream) {
  if (int rc = check_text("fd_cif_read_lines", text, n, file_offsets, F)) return rc;
  FD_CHECK_ARG(lines && aligned8(lines), "fd_cif_read_lines: null or misaligned output");
  const Text x{text, n, file_offsets, F, 0, 0};
  hipLaunchKernelGGL(cif_read_lines_kernel, dim3((unsigned)chunks_of(n)), dim3(RT), 0, (hipStream_t)stream, x, chunks_of(n), lines);
  FD_CHECK_LAUNCH("fd_cif_read_lines");
  return FD_OK;
}

extern "C" int fd_cif_read_marks(const unsigned char* text, long n, const long* file_offsets, int F, const long* carry, long* marks,
                                 void* stream) {
  if (int rc = check_text("fd_cif_read_marks", text, n, file_offsets, F)) return rc;
  FD_CHECK_ARG(carry && marks && aligned8(carry, marks), "fd_cif_read_marks: null or misaligned operand");
  const Text x{text, n, file_offsets, F, 0, 0};
  hipLaunchKernelGGL(cif_read_marks_kernel, dim3((unsigned)chunks_of(n)), dim3(RT), 0, (hipStream_t)stream, x, chunks_of(n), carry, marks);
  FD_CHECK_LAUNCH("fd_cif_read_marks");
  return FD_OK;
}

extern "C" int fd_cif_read_header(const unsigned char* text, long n, const long* file_offsets, int F, int hetatm, int ids_label,
                                  const long* carry, int* table, long* file_first, long* bad, void* stream) {
  if (int rc = check_text("fd_cif_read_header", text, n, file_offsets, F)) return rc;
  FD_CHECK_ARG(carry && table && file_first && bad && aligned8(carry, file_first, bad) && (((uintptr_t)table) & 3u) == 0,
               "fd_cif_read_header: null or misaligned operand");
  const Text x{text, n, file_offsets, F, hetatm, 0};
  hipLaunchKernelGGL(cif_read_header_kernel, dim3((unsigned)chunks_of(n)), dim3(RT), 0, (hipStream_t)stream, x, chunks_of(n), ids_label,
                     carry, table, file_first, bad);
  FD_CHECK_LAUNCH("fd_cif_read_header");
  return FD_OK;
}

extern "C" int fd_cif_read_summary(const unsigned char* text, long n, const long* file_offsets, int F, int hetatm, const long* carry,
                                   const int* table, long* last, void* stream) {
  if (int rc = check_text("fd_cif_read_summary", text, n, file_offsets, F)) return rc;
  FD_CHECK_ARG(carry && table && last && aligned8(carry, last), "fd_cif_read_summary: null or misaligned operand");
  const Text x{text, n, file_offsets, F, hetatm, 0};
  hipLaunchKernelGGL(cif_read_summary_kernel, dim3((unsigned)chunks_of(n)), dim3(RT), 0, (hipStream_t)stream, x, chunks_of(n), carry, table,
                     last);
  FD_CHECK_LAUNCH("fd_cif_read_summary");
  return FD_OK;
}

extern "C" int fd_cif_read_count(const unsigned char* text, long n, const long* file_offsets, int F, int hetatm, int model_all,
                                 const long* carry, const int* table, long* counts, void* stream) {
  if (int rc = check_text("fd_cif_read_count", text, n, file_offsets, F)) return rc;
  FD_CHECK_ARG(carry && table && counts && aligned8(carry, counts), "fd_cif_read_count: null or misaligned operand");
  const Text x{text, n, file_offsets, F, hetatm, model_all};
  hipLaunchKernelGGL(cif_read_count_kernel, dim3((unsigned)chunks_of(n)), dim3(RT), 0, (hipStream_t)stream, x, chunks_of(n), carry, table,
                     counts);
  FD_CHECK_LAUNCH("fd_cif_read_count");
  return FD_OK;
}

extern "C" int fd_cif_read_fill(const unsigned char* text, long n, const long* file_offsets, int F, int hetatm, int model_all,
                                const long* carry, const int* table, const long* bases, long T, long C, float* atom_positions,
                                unsigned char* atom_mask, float* b_factors, long* aatype, long* residue_index, int* row_dropped,
                                long* chain_first, int* chain_file, int* chain_model, int* chain_id, void* stream) {
  if (int rc = check_text("fd_cif_read_fill", text, n, file_offsets, F)) return rc;
  FD_CHECK_ARG(T >= 0 && C >= 0, "fd_cif_read_fill: negative size");
  if (T == 0) return FD_OK;
  FD_CHECK_ARG(carry && table && bases && atom_positions && atom_mask && b_factors && aatype && residue_index && row_dropped &&
                   chain_first && chain_file && chain_model && chain_id, "fd_cif_read_fill: null operand");
  const Text x{text, n, file_offsets, F, hetatm, model_all};
  const Rows o{T, C, atom_positions, atom_mask, b_factors, aatype, residue_index, row_dropped, chain_first, chain_file, chain_model,
               chain_id};
  hipLaunchKernelGGL(cif_read_fill_kernel, dim3((unsigned)chunks_of(n)), dim3(RT), 0, (hipStream_t)stream, x, chunks_of(n), carry, table,
                     bases, o);
  FD_CHECK_LAUNCH("fd_cif_read_fill");
  return FD_OK;
}
