// Split-bf16 GEMM kernel (fd_gemm tile codes 4 and 6) for the pair-level GEMMs.  Included by fd_gemm.hip inside its
// anonymous namespace (uses GemmArgs, store_tile, store_tile_vec, fd_xcd_swizzle; the split fd_split8 and the six-product
// order fd_mma6 are fd_split.h's, shared with every other split-bf16 kernel).
//
// gfx950 runs the bf16 MFMA at 16x the fp32-MFMA rate.  An fp32 value splits EXACTLY into three bf16 terms
// x = x0 + x1 + x2 (round-to-nearest at every stage: 3 x (8 bits + sign of the next residual) covers the 24-bit
// significand), so  a*b = sum_{i,j} a_i*b_j  with every term an exact bf16 product.  The six terms with i+j <= 2
// are accumulated in fp32 by v_mfma_f32_32x32x16_bf16; the three dropped terms are <= 2^-26 |a*b|, below the fp32
// rounding of the product itself.  The result is an fp32-accurate GEMM (same error class as the fmaf-chain kernel;
// tests/test_gemm.py measures both against fp64) at up to 16/6 = 2.7x its peak rate.
//
// Operands stay fp32 in HBM; the split happens in registers on the way global -> LDS (11 VALU ops per element
// pair).  The block is wave-specialised so that this VALU work never sits in the instruction stream of a wave that
// feeds the matrix pipe:
//   * consumer waves (wave tile 64 x 64) issue only ds_read_b128 + MFMA;
//   * producer waves load later stages from global memory, split them and write them to LDS.
// A stage is 16 k (one MFMA step) of every row: three 32-byte bf16 planes + 16 B pad = 112 B per row (7 x 16 B:
// conflict-free ds_read_b128; the producer's row order makes every 8-lane ds_write_b128 group tile one 128-byte
// bank window).
//
// Two block shapes (BM x 128 output tile, BM/64 x 2 consumer waves, BM/64 producer waves):
//   BM = 256 (tile 4): 12 waves, LDS ring of THREE stages = 129 KB -> one block per CU.  While the consumers multiply
//     stage s out of registers they prefetch the fragments of stage s+1 (complete since the previous barrier) and
//     the producers fill stage s+2: the single barrier per stage never has an LDS read waiting behind it.
//   BM = 128 (tile 6): 6 waves, ring of TWO stages, 66 KB -> two blocks per CU, so the prologue and the (HBM-heavy)
//     epilogue of one block run under the MFMA loop of the other; the natural shape for the N_out = 128 weight
//     gradients too.
constexpr int XBK = 16;
constexpr int XROWB = 3 * XBK * 2 + 16;   // bytes per staged row
constexpr int XBN = 128;
constexpr int XBM = 256;                  // the wide shape (tile 4)

template <int BM>
struct SplitCfg {
  static constexpr int NCONS = BM * 2;           // consumer threads: (BM / 64) x 2 waves
  static constexpr int NPROD = BM;               // producer threads: BM / 64 waves
  static constexpr int NTHR = NCONS + NPROD;
  static constexpr int STAGE = (BM + XBN) * XROWB;
  static constexpr int RING = BM == 256 ? 3 : 2;
  static constexpr int EPI = BM * (XBN + 4) * 4;  // the vector epilogue transposes the C tile through LDS
  static constexpr int LDS = RING * STAGE > EPI ? RING * STAGE : EPI;
  static constexpr int BLOCKS_PER_CU = BM == 256 ? 1 : 2;
  static_assert(LDS * BLOCKS_PER_CU <= 160 * 1024, "LDS");
};

// LDS-free epilogue for the TRANSPOSED accumulation (the B fragment is the MFMA's row operand): a lane holds four
// consecutive COLUMNS of one output row per accumulator group, so bias / pair / gate / residual / old C / C move as
// float4s straight between registers and global memory -- no LDS round trip, no barrier.
template <int TM, int TN>
__device__ __forceinline__ void store_tile_t(const FdGemmDesc& d, float* __restrict__ C, f32x16 (&acc)[TM][TN],
                                             int m_base, int n_base, int h, int l31, bool vec) {
  // acc[i][j][r]: row m = m_base + 32 i + l31, column n = n_base + 32 j + 8 (r >> 2) + 4 h + (r & 3)
  const bool has_pair = d.pair_p != nullptr, has_gate = d.gate != nullptr, has_res = d.resid != nullptr;
  const bool has_rs = d.rowscale != nullptr, has_beta = d.beta != 0, has_bias = d.bias != nullptr;
  const int nres = d.nres;
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int mr = m_base + i * 32 + l31;
    const bool mok = mr < d.M;
    const int m = mok ? mr : d.M - 1;
    const float rs = has_rs ? d.rowscale[m] : 1.f;
    const float* pp = C;
    const float* pq = C;
    if (has_pair) {
      const int q = m / nres;
      const int jj = m - q * nres;
      const int bb = q / nres;
      pp = d.pair_p + (long)q * d.ld_pair;
      pq = d.pair_q + ((long)bb * nres + jj) * d.ld_pair;
    }
    float* crow = C + (long)m * d.ldc;
    const float* grow = has_gate ? d.gate + (long)m * d.ld_gate : C;
    const float* rrow = has_res ? d.resid + (long)m * d.ld_resid : C;
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int gq = 0; gq < 4; ++gq) {
        const int nr = n_base + j * 32 + 8 * gq + 4 * h;
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = d.alpha * acc[i][j][4 * gq + e];
        if (vec) {
          // N % 4 == 0: the float4 is entirely inside or outside
          const bool nok = nr < d.N;
          const int n = nok ? nr : 0;
          if (has_bias) {
            const float4 t = *reinterpret_cast<const float4*>(d.bias + n);
            v[0] += t.x; v[1] += t.y; v[2] += t.z; v[3] += t.w;
          }
          if (has_pair) {
            const float4 a = *reinterpret_cast<const float4*>(pp + n);
            const float4 b = *reinterpret_cast<const float4*>(pq + n);
            v[0] += a.x + b.x; v[1] += a.y + b.y; v[2] += a.z + b.z; v[3] += a.w + b.w;
          }
          if (d.relu) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = v[e] > 0.f ? v[e] : 0.f;
          }
          if (has_gate) {
            const float4 t = *reinterpret_cast<const float4*>(grow + n);
            v[0] = t.x > 0.f ? v[0] : 0.f; v[1] = t.y > 0.f ? v[1] : 0.f;
            v[2] = t.z > 0.f ? v[2] : 0.f; v[3] = t.w > 0.f ? v[3] : 0.f;
          }
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] *= rs;
          if (has_res) {
            const float4 t = *reinterpret_cast<const float4*>(rrow + n);
            v[0] += t.x; v[1] += t.y; v[2] += t.z; v[3] += t.w;
          }
          if (has_beta) {
            const float4 t = *reinterpret_cast<const float4*>(crow + n);
            v[0] += t.x; v[1] += t.y; v[2] += t.z; v[3] += t.w;
          }
          if (mok && nok) *reinterpret_cast<float4*>(crow + n) = make_float4(v[0], v[1], v[2], v[3]);
          fd::sched_fence();   // keep the 16 float4 groups from being software-pipelined into one register spike
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int ne = nr + e;
            const bool nok = ne < d.N;
            const int n = nok ? ne : 0;
            float x = v[e];
            if (has_bias) x += d.bias[n];
            if (has_pair) x += pp[n] + pq[n];
            if (d.relu) x = x > 0.f ? x : 0.f;
            if (has_gate) x = grow[n] > 0.f ? x : 0.f;
            x *= rs;
            if (has_res) x += rrow[n];
            if (has_beta) x += crow[n];
            if (mok && nok) crow[n] = x;
          }
        }
      }
  }
}

// Stages a ROWS x 16 operand tile with NPROD producer threads.  A slot = (row, group of 8 consecutive k).
//   KC : k contiguous in memory   -> 2 x float4 per slot, 2 lanes per row
//   !KC: row contiguous in memory -> 8 dword loads per slot (coalesced across the lanes = rows)
template <int ROWS, bool KC, int NPROD>
struct SplitStager {
  static constexpr int NS = ROWS * 2 / NPROD;
  const float* p[NS];
  int kofs[NS];   // first k of the slot inside the stage
  int lofs[NS];   // LDS byte offset of the slot (plane 0)
  long kstep, cs;

  // slot i of producer thread tid -> (row inside the tile, k group)
  static __device__ __forceinline__ void slot(int tid, int i, int& row, int& kg) {
    const int f = tid + NPROD * i;   // tid = producer thread index
    // KC: two lanes cover the 64 contiguous bytes a row contributes to a stage; the four rows of an 8-lane
    // ds_write_b128 group are taken 2 apart (2 * 112 B = 96 mod 128: the group tiles one 32-bank window)
    const int q = f >> 1;
    row = KC ? ((q & ~7) | ((q & 3) << 1) | ((q & 7) >> 2)) : (f % ROWS);
    kg = KC ? (f & 1) : (f / ROWS);
  }

  // point the slots at rows row0.. of the operand, first k = k0 (the persistent kernel calls this once per tile)
  __device__ __forceinline__ void target(const float* __restrict__ b, long rs_, int row0, int nrows, int k0, int tid) {
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      int row, kg;
      slot(tid, i, row, kg);
      // rows past the end are CLAMPED, not zero-filled: an output row/column depends only on its own operand
      // row, and the epilogue never stores rows >= M or columns >= N
      const int grow = (row0 + row < nrows) ? row0 + row : nrows - 1;
      p[i] = b + (long)grow * rs_ + (long)(k0 + 8 * kg) * cs;
    }
  }

  __device__ __forceinline__ void init(const float* __restrict__ b, long rs_, long cs_, int row0, int nrows, int k0,
                                       int tid) {
    cs = cs_;
    kstep = (long)XBK * cs_;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      int row, kg;
      slot(tid, i, row, kg);
      kofs[i] = 8 * kg;
      lofs[i] = row * XROWB + kg * 16;
    }
    target(b, rs_, row0, nrows, k0, tid);
  }

  __device__ __forceinline__ void load(float (&r)[NS][8], int k0, int K) {
    if (k0 + XBK <= K) {   // (uniform) whole stage inside the k range: unconditional loads
#pragma unroll
      for (int i = 0; i < NS; ++i) {
        if (KC) {
          const float4 v = *reinterpret_cast<const float4*>(p[i]);
          const float4 w = *reinterpret_cast<const float4*>(p[i] + 4);
          r[i][0] = v.x; r[i][1] = v.y; r[i][2] = v.z; r[i][3] = v.w;
          r[i][4] = w.x; r[i][5] = w.y; r[i][6] = w.z; r[i][7] = w.w;
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e) r[i][e] = p[i][e * cs];
        }
        p[i] += kstep;
      }
      return;
    }
    // k tail: zeros beyond K
#pragma unroll
    for (int i = 0; i < NS; ++i) {
#pragma unroll
      for (int e = 0; e < 8; ++e) r[i][e] = 0.f;
      if (KC) {
        // K % 4 == 0 (operands_vectorisable): a float4 is entirely inside or outside the k range
        if (k0 + kofs[i] < K) {
          const float4 v = *reinterpret_cast<const float4*>(p[i]);
          r[i][0] = v.x; r[i][1] = v.y; r[i][2] = v.z; r[i][3] = v.w;
        }
        if (k0 + kofs[i] + 4 < K) {
          const float4 v = *reinterpret_cast<const float4*>(p[i] + 4);
          r[i][4] = v.x; r[i][5] = v.y; r[i][6] = v.z; r[i][7] = v.w;
        }
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (k0 + kofs[i] + e < K) r[i][e] = p[i][e * cs];
      }
      p[i] += kstep;
    }
  }

  __device__ __forceinline__ void store(const float (&r)[NS][8], char* __restrict__ lds) const {
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      uint4 s0, s1, s2;
      fd_split8(r[i], s0, s1, s2);
      *reinterpret_cast<uint4*>(lds + lofs[i]) = s0;
      *reinterpret_cast<uint4*>(lds + lofs[i] + 2 * XBK) = s1;
      *reinterpret_cast<uint4*>(lds + lofs[i] + 4 * XBK) = s2;
    }
  }
};

// ---- the pieces of a block that the fresh-block kernel and the persistent kernel below share ----
// (state -- stagers, ring slots, fragment offsets -- stays in the kernels' own locals and is passed by reference)

// NSET register sets = NSET stages of global loads in flight per producer thread (stage s lives in set s % NSET).
// (Four sets were measured on the HBM-streamed pair tensor: no change against two -- 1.06 ms on the K = 384
// edge shape either way -- so the load latency is not what separates it from an L2-resident operand.)
constexpr int XNSET = 2;

// producer: one loaded register set -> (split) -> ring slot wbuf (the slot of the next LDS store, advanced here)
template <int BM, class StagerA, class StagerB>
__device__ __forceinline__ void split_put(const StagerA& sa, const StagerB& sb, char* lds, int& wbuf,
                                          const float (&xa)[StagerA::NS][8], const float (&xb)[StagerB::NS][8]) {
  char* dst = lds + wbuf * SplitCfg<BM>::STAGE;
  sa.store(xa, dst);
  sb.store(xb, dst + BM * XROWB);
  wbuf = (wbuf == SplitCfg<BM>::RING - 1) ? 0 : wbuf + 1;
}

// producer: feeds a sequence of n stages to the consumers, one barrier per stage.  issue(xa, xb) loads the NEXT stage
// of the sequence into a register set (what differs between the kernels: a fixed tile against a stream of tiles),
// put(xa, xb) moves a loaded set into the ring (split_put, or more on the way).
template <int RING, int NSA, int NSB, class Issue, class Put>
__device__ __forceinline__ void split_pump(int n, float (&ra)[XNSET][NSA][8], float (&rb)[XNSET][NSB][8], Issue& issue,
                                           Put& put) {
  constexpr int NSET = XNSET;
  // AHEAD = how many stages beyond the one being multiplied are complete in LDS at a barrier
  constexpr int AHEAD = RING - 1;
#pragma unroll
  for (int u = 0; u < NSET; ++u)
    if (u < n) issue(ra[u], rb[u]);
#pragma unroll
  for (int u = 0; u < AHEAD; ++u)
    if (u < n) {
      put(ra[u], rb[u]);
      if (u + NSET < n) issue(ra[u], rb[u]);
    }
  __syncthreads();   // the first AHEAD stages are in the ring
  // during stage `it`: stage it+AHEAD goes registers -> its ring slot (last read AHEAD barriers ago) and the loads
  // of stage it+AHEAD+NSET refill the register set
  auto step = [&](int it, float (&xa)[NSA][8], float (&xb)[NSB][8]) {
    if (it + AHEAD < n) {
      put(xa, xb);
      if (it + AHEAD + NSET < n) issue(xa, xb);
    }
    __syncthreads();
  };
  for (int it = 0; it < n; it += NSET) {
#pragma unroll
    for (int u = 0; u < NSET; ++u)
      if (it + u < n) step(it + u, ra[(AHEAD + u) % NSET], rb[(AHEAD + u) % NSET]);
  }
}

// consumer: the 2 x 2 fragments of ring slot rbuf (the slot of the next fragment read, advanced here).  a_frag / b_frag =
// per-lane fragment base: row (l31); lane-half h takes k 8h..8h+7 of the 16-k MFMA step
template <int BM>
__device__ __forceinline__ void split_read_frags(const char* lds, int& rbuf, int a_frag, int b_frag, uint4 (&xa)[2][3],
                                                 uint4 (&xb)[2][3]) {
  const char* st = lds + rbuf * SplitCfg<BM>::STAGE;
#pragma unroll
  for (int s = 0; s < 3; ++s) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
      xa[i][s] = *reinterpret_cast<const uint4*>(st + a_frag + i * 32 * XROWB + s * 2 * XBK);
#pragma unroll
    for (int j = 0; j < 2; ++j)
      xb[j][s] = *reinterpret_cast<const uint4*>(st + b_frag + j * 32 * XROWB + s * 2 * XBK);
  }
  rbuf = (rbuf == SplitCfg<BM>::RING - 1) ? 0 : rbuf + 1;
}

// consumer, ring of three, nk stages: stage it is multiplied out of registers (fd_mma6: the four accumulators interleaved,
// dependent MFMAs four issues apart) while the fragments of stage it+1 (complete in the ring since the last barrier) are
// fetched; the barrier itself carries no LDS wait on this side
template <int BM, bool TRANS>
__device__ __forceinline__ void split_multiply3(f32x16 (&acc)[2][2], int nk, const char* lds, int& rbuf, int a_frag,
                                                int b_frag) {
  uint4 fa[2][2][3], fb[2][2][3];
  auto step = [&](int it, uint4 (&ca)[2][3], uint4 (&cb)[2][3], uint4 (&na)[2][3], uint4 (&nb)[2][3]) {
    if (it + 1 < nk) split_read_frags<BM>(lds, rbuf, a_frag, b_frag, na, nb);
    fd_mma6<TRANS, 2, 2>(acc, ca, cb);
    fd::block_barrier_nofence();
  };
  split_read_frags<BM>(lds, rbuf, a_frag, b_frag, fa[0], fb[0]);
  for (int it = 0; it < nk; it += 2) {
    step(it, fa[0], fb[0], fa[1], fb[1]);
    if (it + 1 < nk) step(it + 1, fa[1], fb[1], fa[0], fb[0]);
  }
}

// TRANS: transposed accumulation + LDS-free float4 epilogue (needs ksplit == 1: its split-K atomics would touch one
// cache line per lane); !TRANS: row-major accumulation, LDS-transposed epilogue or split-K atomics.
template <int BM, bool A_KC, bool B_KC, bool TRANS>
__global__ __launch_bounds__(SplitCfg<BM>::NTHR, SplitCfg<BM>::BLOCKS_PER_CU) void gemm_bx3_kernel(GemmArgs g) {
  using Cfg = SplitCfg<BM>;
  constexpr int BN = XBN, TM = 2, TN = 2;
  constexpr int NCONS = Cfg::NCONS, NPROD = Cfg::NPROD, RING = Cfg::RING;
  constexpr int A_BYTES = BM * XROWB;
  __shared__ __attribute__((aligned(16))) char lds[Cfg::LDS];

  const FdGemmDesc& d = g.d;
  const int tid = (int)threadIdx.x;

  const int nblk = g.nblk_m * g.nblk_n;
  const int lid = fd_xcd_swizzle((int)blockIdx.x, nblk);
  const int bm = lid / g.nblk_n, bn = lid % g.nblk_n;
  const int m0 = bm * BM, n0 = bn * BN;

  const int z = (int)blockIdx.y;
  const int zo = z / d.bdiv, zi = z % d.bdiv;

  // split-K: blockIdx.z owns stages [kt0, kt0 + nk)
  const int nkt_all = (d.K + XBK - 1) / XBK;
  const int per = (nkt_all + g.ksplit - 1) / g.ksplit;
  const int kt0 = (int)blockIdx.z * per;
  const int nkt = (kt0 + per < nkt_all) ? kt0 + per : nkt_all;
  const int nk = nkt - kt0;
  if (nk <= 0) return;

  if (tid >= NCONS) {
    // ---- producer waves: global -> registers -> (split) -> LDS ring ----
    const int ptid = tid - NCONS;
    fd::raise_wave_priority();   // the producer's instruction stream must never wait for an issue slot
    const float* __restrict__ A = d.A + zo * d.a_so + zi * d.a_si;
    const float* __restrict__ B = d.B + zo * d.b_so + zi * d.b_si;
    SplitStager<BM, A_KC, NPROD> sa;
    SplitStager<BN, B_KC, NPROD> sb;
    constexpr int NSA = SplitStager<BM, A_KC, NPROD>::NS, NSB = SplitStager<BN, B_KC, NPROD>::NS;
    float ra[XNSET][NSA][8], rb[XNSET][NSB][8];
    sa.init(A, d.a_rs, d.a_cs, m0, d.M, kt0 * XBK, ptid);
    sb.init(B, d.b_cs, d.b_rs, n0, d.N, kt0 * XBK, ptid);   // the staged "row" of B is n
    int lk = kt0;   // stage of the next global load
    auto issue = [&](float (&xa)[NSA][8], float (&xb)[NSB][8]) {
      sa.load(xa, lk * XBK, d.K);
      sb.load(xb, lk * XBK, d.K);
      ++lk;
    };
    // fused bias gradient of dW = dY^T X (A = dY^T row-contiguous: producer thread t stages row m0 + t in all of
    // its slots, NPROD == BM): row sums of A over k, taken from the registers on their way to LDS
    const bool do_rowsum = !A_KC && d.a_rowsum != nullptr && bn == 0 && z == 0;
    float rsum = 0.f;
    int wbuf = 0;
    auto put = [&](float (&xa)[NSA][8], float (&xb)[NSB][8]) {
      if (!A_KC && do_rowsum) {
#pragma unroll
        for (int i = 0; i < NSA; ++i)
          rsum += ((xa[i][0] + xa[i][1]) + (xa[i][2] + xa[i][3])) + ((xa[i][4] + xa[i][5]) + (xa[i][6] + xa[i][7]));
      }
      split_put<BM>(sa, sb, lds, wbuf, xa, xb);
    };
    split_pump<RING>(nk, ra, rb, issue, put);
    if (!A_KC && do_rowsum && m0 + ptid < d.M) atomicAdd(d.a_rowsum + m0 + ptid, d.alpha * rsum);
    if (!TRANS && g.epi_vec) {   // the two barriers of the consumers' LDS-transposed epilogue
      __syncthreads();
      __syncthreads();
    }
    return;
  }

  // ---- consumer waves: LDS -> registers -> MFMA ----
  const int lane = tid & 63, wave = tid >> 6;
  const int h = lane >> 5, l31 = lane & 31;
  const int wm = wave >> 1, wn = wave & 1;
  float* __restrict__ C = d.C + zo * d.c_so + zi * d.c_si;

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int a_frag = ((wm * TM) * 32 + l31) * XROWB + h * 16;
  const int b_frag = A_BYTES + ((wn * TN) * 32 + l31) * XROWB + h * 16;
  int rbuf = 0;
  __syncthreads();   // the first stages are in the ring
  if (RING == 3) {
    split_multiply3<BM, TRANS>(acc, nk, lds, rbuf, a_frag, b_frag);
  } else {
    // two-stage ring: stage it+1 is only complete at the barrier that ends stage it, so its fragments are fetched
    // after the barrier; the co-resident second block covers that latency
    uint4 fa[TM][3], fb[TN][3];
    for (int it = 0; it < nk; ++it) {
      split_read_frags<BM>(lds, rbuf, a_frag, b_frag, fa, fb);
      fd_mma6<TRANS, TM, TN>(acc, fa, fb);
      fd::block_barrier_nofence();
    }
  }

  if (TRANS)
    store_tile_t<TM, TN>(d, C, acc, m0 + wm * TM * 32, n0 + wn * TN * 32, h, l31, g.epi_vec != 0);
  else if (g.epi_vec)
    store_tile_vec<BM, BN, TM, TN, NCONS>(d, C, acc, reinterpret_cast<float*>(lds), m0, n0, wm, wn, h, l31, tid);
  else
    store_tile<TM, TN>(d, C, acc, m0 + wm * TM * 32, n0 + wn * TN * 32, h, l31, g.ksplit > 1);
}


// Persistent form of the 256 x 128 TRANS kernel (A k-contiguous, no split-K): gridDim.x = one block per CU, block b
// walks the tiles b, b + gridDim.x, ...  The producers treat the (tile, k stage) sequence as ONE stream, so while the
// consumers store a finished tile the producers already have the next tile's first stages in the ring (and two more
// in registers): the global-load latency of a tile's prologue, the block launch and the descriptor setup no longer
// sit between two MFMA loops.  Measured on the fresh-block kernel: 10.5 us of un-overlapped prologue + epilogue per tile
// against 29 us of MFMA loop at K = 384 (52 % of a K = 128 launch); persistent: 9.3 us.  What remains is the epilogue
// itself (no epilogue: ~0; the same bytes as lane-contiguous 1 KB stores: -2.7 us): a store instruction of the
// transposed layout touches 32 different lines (a lane owns a row) and the CU retires about one line per clock.
// Re-transposing through a wave-private LDS scratch to store whole lines was measured and gives the 2.7 us back to
// the LDS round trip.  The consumers keep no fragment alive across the epilogue (stage 0 of the next tile is read from
// the ring after it), so the register budget is the fresh-block kernel's (166 VGPRs, no spills).
template <bool B_KC>
__global__ __launch_bounds__(SplitCfg<XBM>::NTHR, 1) void gemm_bx3p_kernel(GemmArgs g) {
  using Cfg = SplitCfg<XBM>;
  constexpr int BM = XBM, BN = XBN, TM = 2, TN = 2;
  constexpr int NCONS = Cfg::NCONS, NPROD = Cfg::NPROD, RING = 3;
  constexpr int A_BYTES = BM * XROWB;
  static_assert(Cfg::RING == 3, "ring");
  __shared__ __attribute__((aligned(16))) char lds[RING * Cfg::STAGE];

  const FdGemmDesc& d = g.d;
  const int tid = (int)threadIdx.x;
  const int nblk = g.nblk_m * g.nblk_n;
  const int G = (int)gridDim.x, first = (int)blockIdx.x;       // G <= nblk
  const int ntiles = (nblk - first + G - 1) / G;
  const int z = (int)blockIdx.y;
  const int zo = z / d.bdiv, zi = z % d.bdiv;
  const int nk = (d.K + XBK - 1) / XBK;
  const int total = ntiles * nk;   // the producers' stream: every stage of every tile of this block

  if (tid >= NCONS) {
    const int ptid = tid - NCONS;
    fd::raise_wave_priority();
    const float* __restrict__ A = d.A + zo * d.a_so + zi * d.a_si;
    const float* __restrict__ B = d.B + zo * d.b_so + zi * d.b_si;
    SplitStager<BM, true, NPROD> sa;
    SplitStager<BN, B_KC, NPROD> sb;
    constexpr int NSA = SplitStager<BM, true, NPROD>::NS, NSB = SplitStager<BN, B_KC, NPROD>::NS;
    float ra[XNSET][NSA][8], rb[XNSET][NSB][8];
    int lt = first, lk = 0;   // tile and k stage of the next global load
    {
      const int lid = fd_xcd_swizzle(lt, nblk);
      sa.init(A, d.a_rs, d.a_cs, (lid / g.nblk_n) * BM, d.M, 0, ptid);
      sb.init(B, d.b_cs, d.b_rs, (lid % g.nblk_n) * BN, d.N, 0, ptid);
    }
    auto issue = [&](float (&xa)[NSA][8], float (&xb)[NSB][8]) {
      sa.load(xa, lk * XBK, d.K);
      sb.load(xb, lk * XBK, d.K);
      if (++lk == nk) {
        lk = 0;
        lt += G;
        if (lt < nblk) {
          const int lid = fd_xcd_swizzle(lt, nblk);
          sa.target(A, d.a_rs, (lid / g.nblk_n) * BM, d.M, 0, ptid);
          sb.target(B, d.b_cs, (lid % g.nblk_n) * BN, d.N, 0, ptid);
        }
      }
    };
    int wbuf = 0;
    auto put = [&](float (&xa)[NSA][8], float (&xb)[NSB][8]) { split_put<BM>(sa, sb, lds, wbuf, xa, xb); };
    split_pump<RING>(total, ra, rb, issue, put);
    return;
  }

  const int lane = tid & 63, wave = tid >> 6;
  const int h = lane >> 5, l31 = lane & 31;
  const int wm = wave >> 1, wn = wave & 1;
  float* __restrict__ C = d.C + zo * d.c_so + zi * d.c_si;
  const int a_frag = ((wm * TM) * 32 + l31) * XROWB + h * 16;
  const int b_frag = A_BYTES + ((wn * TN) * 32 + l31) * XROWB + h * 16;
  int rbuf = 0;
  __syncthreads();   // the first stages are in the ring
  for (int ti = 0; ti < ntiles; ++ti) {
    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    split_multiply3<BM, true>(acc, nk, lds, rbuf, a_frag, b_frag);
    const int lid = fd_xcd_swizzle(first + ti * G, nblk);
    const int mb = (lid / g.nblk_n) * BM + wm * TM * 32, nb = (lid % g.nblk_n) * BN + wn * TN * 32;
    store_tile_t<TM, TN>(d, C, acc, mb, nb, h, l31, g.epi_vec != 0);
  }
}
