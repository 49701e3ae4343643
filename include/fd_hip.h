/* fd_hip.h -- C ABI of libfd_hip.so, the MI355X (gfx950) FrameDiff hot path.
 *
 * The reference (jasonkyuyim/se3_diffusion) has no FFI: its hot path is eager
 * PyTorch.  This header is the seam a maintainer binds (ctypes stub in
 * INTEGRATION.md) to route model/score_network.py:ScoreNetwork.forward and
 * data/se3_diffuser.py:SE3Diffuser.{calc_rot_score,calc_trans_score,reverse,
 * sample_ref,forward_marginal} through hand-written HIP kernels.
 *
 * Conventions: plain device pointers (fp32 unless stated), extents as int,
 * strides in ELEMENTS, `stream` is a hipStream_t passed as void*.  Every entry
 * point is asynchronous on `stream`, re-entrant per stream, takes no ownership,
 * and returns 0 on success or a negative FD_ERR_* code; fd_last_error() gives
 * the message of the last failure on the calling thread.
 */
#ifndef FD_HIP_H_
#define FD_HIP_H_

#ifdef __cplusplus
extern "C" {
#endif

#define FD_ABI_VERSION 2

const char* fd_last_error(void);
int fd_abi_version(void);
/* "gfx950" for the product library; "emu" for the test-only host interpreter. */
const char* fd_backend(void);
/* "" for a product build; "FD_PROBE_BUILD" when the library was built by tools/probes with the timing / ablation hooks of the
 * kernel sources enabled (csrc/fd_probe.h: those hooks do not compile in a product build). */
const char* fd_build_flags(void);
/* kernel launches this library has issued since it was loaded, including launches recorded into a hipGraph capture: the
 * difference across one captured diffusion step (experiments/train_se3_diffusion.py:746-781: one ScoreNetwork forward + one reverse
 * step) is the number of kernels a replay of that step runs. */
long fd_launch_count(void);

/* ---- dense: C = epi(alpha * A*B) --------------------------------------
 * Replaces torch Linear/matmul on the path: model/ipa_pytorch.py:101-166
 * (Linear), :169-233 (transitions), :334-374 (IPA projections), :380-386 and
 * :424-426 (qk^T, a*v); model/score_network.py:67-86 (embedder MLPs); and
 * their autograd.  A(m,k)=A[m*a_rs+k*a_cs], B(k,n)=B[k*b_rs+n*b_cs].
 * Batch index z in [0,batch): zo=z/bdiv, zi=z%bdiv; operand X is offset by
 * zo*x_so + zi*x_si.  Epilogue order: alpha, +bias[n], +pair_p/q, relu,
 * gate (zero where gate<=0), *rowscale[m], +resid, then C = v (+ C if beta). */
typedef struct FdGemmDesc {
  const float* A;
  const float* B;
  float* C;
  int M, N, K;
  long a_rs, a_cs;
  long b_rs, b_cs;
  long ldc;
  int batch, bdiv;
  long a_so, a_si, b_so, b_si, c_so, c_si;
  float alpha;
  int beta;
  const float* bias;     /* [N] */
  const float* pair_p;   /* [B*nres, ld_pair]: row (m / nres)            */
  const float* pair_q;   /* [B*nres, ld_pair]: row (m/nres^2)*nres+m%nres */
  long ld_pair;
  int nres;
  const float* resid;    /* [M, ld_resid] */
  long ld_resid;
  const float* gate;     /* [M, ld_gate] */
  long ld_gate;
  const float* rowscale; /* [M] */
  int relu;
  int tile;              /* 0 = auto; fp32 MFMA (bitwise an fmaf chain over k): 1: 128x128, 2: 64x64, 3: 128x32;
                            4: 256x128 split-bf16 (each fp32 operand = 3 exact bf16 terms, 6 bf16-MFMA products,
                            fp32 accumulate: fp32 accuracy, not bitwise the fmaf chain).  Auto picks 4 for the
                            large pair-level GEMMs unless FD_GEMM_EXACT_F32=1 is set in the environment.
                            5: latency kernel (fp32 MFMA, 32x32 tiles, K split over the waves of a block) that auto
                            picks when the problem has fewer 64x64 tiles than CUs (node-level GEMMs of sampling);
                            needs K % 8 == 0 and unit-stride 16-byte aligned operands.  A long K on few tiles (K >= 640 up
                            to 40 tiles, K >= 960 up to 80; K % 16 == 0) runs on 16x16 tiles: four times the blocks.
                            6: the split-bf16 kernel with a 128x128 block tile (two blocks per CU); never picked
                            automatically by fd_gemm (slower than 4 except for 128-row outputs), the host uses it
                            for the N_out = 128 weight gradients. */
  int ksplit;            /* >1: split K over blocks, C += alpha*A*B atomically
                            (weight gradients: tiny MxN, huge K); epilogue-free */
  int mtiles;            /* 0 = auto; >0: consecutive M tiles pipelined per block (un-batched, ksplit 1) */
  float* a_rowsum;       /* optional [M]: += alpha * sum_k A(m,k), accumulated atomically (fused bias gradient
                            of dW = dY^T X: A = dY^T, so this is sum over rows of dY) */
  const void* b_planes;  /* optional: B pre-split into its three exact bf16 planes (fd_split_planes of the buffer B lives in):
                            the address of plane 0's element of B[0]; plane p of B(k,n) is b_planes[p * b_plane_stride +
                            k * b_rs + n * b_cs] (16-bit elements).  With it fd_gemm may run the node-level layers (nn.Linear
                            forward y = x W^T and activation gradient dx = dy W, model/ipa_pytorch.py:101-166) on tiles
                            12: 128x128, 13: 64x128, 14: 64x64 -- split-bf16 arithmetic as tile 4, the weight operand moved as
                            6-byte elements with no split work in the kernel.  Needs A k-contiguous, K % 16 == 0, B unit-stride
                            along k or along n (then N % 8 == 0), un-batched, 16-byte aligned operands. */
  long b_plane_stride;   /* 16-bit elements between two planes (% 8 == 0) */
} FdGemmDesc;

int fd_gemm(const FdGemmDesc* desc, void* stream);
/* planes[p * n + e] = p-th bf16 term of x[e] (x = t0 + t1 + t2 exactly, round-to-nearest at every stage), p = 0..2: the
 * weight operand format of fd_gemm tiles 12-14.  One launch over the flat parameter buffer per optimiser step
 * (experiments/train_se3_diffusion.py:139: the parameters change once per step).  n % 8 == 0. */
int fd_split_planes(const float* x, long n, void* planes, void* stream);
/* the tile code (1..6) fd_gemm would run this descriptor with; no launch */
int fd_gemm_plan(const FdGemmDesc* desc);
/* exact != 0: every later fd_gemm runs on the fp32-MFMA kernels (as FD_GEMM_EXACT_F32=1); returns the previous mode */
int fd_gemm_set_exact_f32(int exact);
/* the split-bf16 kernel runs as `blocks` persistent blocks (default 256 = one per MI355X CU) that walk the output
 * tiles whenever a launch has at least 2 * blocks tiles; 0 = one fresh block per tile.  Returns the previous value. */
int fd_gemm_set_persistent_blocks(int blocks);

/* ---- LayerNorm / reductions (HBM-bound) -------------------------------
 * torch.nn.LayerNorm (eps 1e-5, biased variance) at score_network.py:73,85,
 * ipa_pytorch.py:189,231,577,632 and TransformerEncoderLayer.norm1/2; the
 * optional rowscale fuses the `* mask` that follows (ipa_pytorch.py:641,649). */
int fd_layernorm_fwd(const float* x, long ldx, const float* gamma, const float* beta, const float* rowscale,
                     float* y, long ldy, float* mean, float* rstd, long rows, int C, float eps, void* stream);
int fd_layernorm_bwd(const float* dy, long lddy, const float* x, long ldx, const float* gamma,
                     const float* rowscale, const float* mean, const float* rstd, float* dx, long lddx,
                     int dx_accum, float* dgamma, float* dbeta, long rows, int C, void* stream);
/* out[n] += sum_m X[m*ld+n] (bias gradients) */
int fd_colsum_acc(const float* X, long ld, long rows, int ncols, float* out, void* stream);
/* X [nbatch,n,n,C]: rowsum[b,i,:] += sum_j X[b,i,j,:], colsum[b,j,:] += sum_i X[b,i,j,:] (either may be null) */
int fd_pair_reduce_acc(const float* X, int nbatch, int n, int C, float* rowsum, float* colsum, long ld_out,
                       void* stream);
int fd_axpby(float* y, const float* x, float a, float b, long n, void* stream);
/* dst[r*ldd+c] += a*src[r*lds+c] */
int fd_add2d(float* dst, long ldd, const float* src, long lds, long rows, int cols, float a, void* stream);
int fd_rowscale(const float* x, long ldx, const float* rs, float* y, long ldy, long rows, int C, void* stream);

/* ---- edge transition, fused (model/ipa_pytorch.py:194-233 EdgeTransition.forward :218-233 and its autograd) ----
 * One kernel per direction for the whole 128 -> 384 -> 384 -> 128 chain of a pair row (se3_diffusion_amd/csrc/
 * fd_edge_mlp.hip): the hidden activations stay in the registers of the wave that owns the row, the weights stream
 * through LDS from a pre-packed bf16-plane image (fd_edge_mlp_pack, once per optimiser step, FD_EDGE_MLP_IMAGE_BYTES).
 * Split-bf16 arithmetic (fp32-accurate, as fd_gemm tile 4).  x [rows,128] = z.
 *   forward : h1 = relu(W1z x + p1[b,i] + q1[b,j]); h2 = relu(W2 h1 + bias2); y = Wf (h2 + [x | 0 | 0]) + pf[b,i] + qf[b,j]
 *             (W1z = W1[:, 0:128]; the residual through the final layer, ipa_pytorch.py:231, costs no product of its own);
 *             out = rowscale * LayerNorm(y; gamma, beta, eps).  Training outputs (all four or none): save1 = h1,
 *             save2 = h2 + [x | 0 | 0] (the operand of the final layer's weight gradient), mask1 / mask2 = the packed signs of
 *             h1 / h2 (the backward's ReLU gates); optionally y, mean, rstd of the LayerNorm.
 *   backward: x = dy; u = Wf^T x; d2 = [gmask1] u; d1 = [gmask2] (W2^T d2); out = u[0:128] + W1z^T d1, with the image packed
 *             from the transposed weights (fd_edge_mlp_pack_bwd; gmask1 / gmask2 = the forward's mask2 / mask1);
 *             save1 = d2, save2 = d1 (operands of the weight-gradient GEMMs), both required.
 * Optional fourth forward layer (zb_out != NULL): zb_out[rows,40] = W40 out + zb_bias, W40 = [linear_b.weight ; down_z.weight]
 * of the NEXT trunk block's IPA (ipa_pytorch.py:380-386,455) -- the pair bias and the down-projected pair features of its
 * attention, taken from the output while it is in registers; the image then carries four more units
 * (fd_edge_mlp_pack_zb, after fd_edge_mlp_pack). */
#define FD_EDGE_MLP_IMAGE_BYTES (124 * 12288)
int fd_edge_mlp_pack_zb(const float* W40, void* image, void* stream);
/* forward image: trunk.0.weight W1 [384,384], trunk.2.weight W2 [384,384], final_layer.weight Wf [128,384], row-major with row
 * stride ld (ipa_pytorch.py:204-216) */
int fd_edge_mlp_pack(const float* W1, const float* W2, const float* Wf, long ld, void* image, void* stream);
/* backward image (the transposed chain, hidden chunks in the order the backward kernel walks them); W40 [40,128] of the IPA block
 * BEHIND the transition or null: four leading units for the dzb term of the fused prologue (FdEdgeMlpDesc.dzb) */
int fd_edge_mlp_pack_bwd(const float* Wf, const float* W2, const float* W1, long ld, const float* W40, void* image, void* stream);
typedef struct FdEdgeMlpDesc {
  const float* x;        /* [rows,128] */
  const void* img;       /* weight image of fd_edge_mlp_pack */
  const float* p1;       /* forward: [B*nres,384] term of residue i */
  const float* q1;       /* forward: [B*nres,384] term of residue j (carries the layer-1 bias) */
  const float* bias2;    /* forward: [384] */
  float* save1;          /* [rows,384]: forward (training) h1; backward d2 */
  float* save2;          /* [rows,384]: forward (training) h2 + [x | 0 | 0]; backward d1 */
  const float* pf;       /* forward: [B*nres,128] */
  const float* qf;       /* forward: [B*nres,128] (carries the final bias) */
  const float* gamma;    /* forward: LayerNorm weight [128] */
  const float* beta;     /* forward: LayerNorm bias [128] */
  const float* rowscale; /* forward, optional: [rows] pair mask */
  float* y;              /* forward (training), optional: [rows,128] pre-LayerNorm values */
  float* mean;           /* forward (training), optional: [rows] */
  float* rstd;           /* forward (training), optional: [rows] */
  float* out;            /* [rows,128] */
  long rows;             /* B * nres * nres */
  int nres;
  int backward;
  float eps;
  int blocks;            /* 0 = persistent blocks that fill the 256 CUs (512 of shape 4, 256 of shape 8) */
  long ld_pq;            /* row stride of p1 / q1 (0 = 384) */
  long ld_pqf;           /* row stride of pf / qf (0 = 128) */
  float* zb_out;         /* forward, optional: [rows,40] (see above) */
  const float* zb_bias;  /* forward, optional: [40] */
  unsigned* mask1;       /* forward (training): [rows,12] packed signs of h1: bit 4 nb + e of word 4 c + g <-> unit 128 c + 16 nb + 4 g + e */
  unsigned* mask2;       /* forward (training): [rows,12] packed signs of h2 */
  const unsigned* gmask1; /* backward: the forward's mask2 (48 B per row instead of the 1536 B of h2) */
  const unsigned* gmask2; /* backward: the forward's mask1 */
  /* Backward, optional -- fused prologue (image from fd_edge_mlp_pack_bwd): x is then the UPSTREAM gradient of the transition's
   * output (may be null with dzb), the kernel's own input dy = LayerNorm-backward(x [+ dzb W40]; ln_y, ln_mean, ln_rstd,
   * ln_gamma, ln_rowscale) is formed in registers, written to dy_out (optional) and ln_dgamma / ln_dbeta (+=, optional). */
  const float* ln_y;        /* [rows,128] the forward's pre-LayerNorm save */
  const float* ln_mean;     /* [rows] */
  const float* ln_rstd;     /* [rows] */
  const float* ln_gamma;    /* [128] */
  const float* ln_rowscale; /* optional [rows] */
  float* dy_out;            /* optional [rows,128] */
  float* ln_dgamma;         /* optional [128], accumulated */
  float* ln_dbeta;          /* optional [128], accumulated */
  const float* dzb;         /* optional [rows,40]: adds dzb W40 to the upstream gradient (autograd of the next IPA block's linear_b /
                               down_z w.r.t. this transition's output; W40 = the four leading units of the image) */
  unsigned* sched;          /* optional: one word of device scratch -- a launch whose blocks walk four or more 64-row tiles each then
                               hands the tiles out dynamically (one atomic per tile and block); fd_edge_mlp zeroes the word on
                               the launch's stream; the words of launches that may run at the same time must differ */
  int shape;                /* 0 = by size (8 from FD_EDGE_MLP_W8_MIN_ROWS rows up; 2 for an inference forward of at most
                               FD_EDGE_MLP_PAIR_MAX_ROWS rows), 4 = 4 waves x 64-row tiles on two blocks per CU, 8 = 8 waves x 128-row
                               tiles on one block per CU (4 and 8: same results bit for bit), 2 = two waves per 16-row group, 64-row
                               tiles on one block per CU (inference forward only; equal to fp32 rounding) */
} FdEdgeMlpDesc;
#define FD_EDGE_MLP_W8_MIN_ROWS 65536L
#define FD_EDGE_MLP_PAIR_MAX_ROWS 16384L   /* 256 CUs x 4 SIMDs x 16 rows: at most one 16-row group per SIMD */
int fd_edge_mlp(const FdEdgeMlpDesc* desc, void* stream);

/* ---- edge embedder, fused (model/score_network.py:97-101,129-153 Embedder edge path, data/utils.py:570-580) ----
 * One kernel builds the 120-d pair feature on the fly and runs the MLP 120 -> 128 -> 128 -> 128 + LayerNorm + pair mask
 * in the registers of the wave that owns the pair row (se3_diffusion_amd/csrc/fd_edge_embed.hip).  The part of the first
 * layer that depends on one residue only arrives as p[b,i] = W0[:, 0:33] pt_i + b0 and q[b,j] = W0[:, 33:66] pt_j
 * (pt = [t-emb(32) | fixed]); the kernel adds W0[:, 66:120] [relpos sincos(32) | distogram(22)].  The image packs
 * W0[:, 66:120], W2, W4 ([128,120], [128,128], [128,128] row-major) as bf16 planes (FD_EDGE_EMBED_IMAGE_BYTES). */
#define FD_EDGE_EMBED_IMAGE_BYTES (24 * 12288)
/* optional fourth layer, as fd_edge_mlp's: zb_out[rows,40] = W40 out + zb_bias for the FIRST trunk block's IPA; the image then
 * carries four more units (fd_edge_embed_pack_zb after fd_edge_embed_pack) */
int fd_edge_embed_pack_zb(const float* W40, void* image, void* stream);
int fd_edge_embed_pack(const float* W0, const float* W2, const float* W4, void* image, void* stream);
typedef struct FdEdgeEmbedDesc {
  const long* seq_idx;    /* [B*nres] */
  const float* sc_ca;     /* [B*nres,3] self-conditioning CA positions (A) */
  const float* idenom;    /* [16] index-embedding denominators (host table, score_network.py:26-29) */
  const float* dg_lower;  /* [22] distogram bin edges (data/utils.py:573-578) */
  const float* dg_upper;  /* [22] */
  const void* img;
  const float* p;         /* [B*nres,128] */
  const float* q;         /* [B*nres,128] */
  const float* bias2;     /* [128] */
  const float* bias3;     /* [128] */
  const float* gamma;     /* LayerNorm weight [128] */
  const float* beta;      /* LayerNorm bias [128] */
  const float* rowscale;  /* optional [rows] pair mask */
  float* h1;              /* optional saves for the backward: [rows,128] post-ReLU layer 1 */
  float* h2;              /* ... layer 2 */
  float* h3;              /* ... layer 3 (pre-LayerNorm) */
  float* mean;            /* optional [rows] */
  float* rstd;            /* optional [rows] */
  float* out;             /* [rows,128] */
  long rows;              /* B * nres * nres */
  int nres;
  float eps;
  int blocks;             /* 0 = one persistent block per CU (256) */
  float* zb_out;          /* optional [rows,40] */
  const float* zb_bias;   /* optional [40] */
  unsigned* mask1;        /* optional [rows,4]: packed signs of h1 (bit 4 nb + e of word g <-> unit 16 nb + 4 g + e) */
  unsigned* mask2;        /* optional [rows,4]: packed signs of h2 */
  long ld_pq;             /* row stride of p / q (0 = 128): both as column blocks of one GEMM's output */
} FdEdgeEmbedDesc;
int fd_edge_embed(const FdEdgeEmbedDesc* desc, void* stream);

/* Backward dX chain of the same MLP (autograd of model/score_network.py:67-86,194-195 w.r.t. its hidden activations) in one
 * launch (se3_diffusion_amd/csrc/fd_edge_embed_bwd.hip): LayerNorm backward (dgamma / dbeta accumulated), dh2 = [h2 > 0]
 * (dh3 W4), dh1 = [h1 > 0] (dh2 W2).  h1, h2, h3, mean, rstd are fd_edge_embed's saves; dh3 / dh2 / dh1 [rows,128] are the
 * operands of the weight gradients (fd_group_dw).  Image: fd_edge_embed_bwd_pack(W2 = edge_embedder.2.weight, W4 = .4.weight). */
#define FD_EDGE_EMBED_BWD_IMAGE_BYTES (16 * 12288)
int fd_edge_embed_bwd_pack(const float* W2, const float* W4, void* image, void* stream);
typedef struct FdEdgeEmbedBwdDesc {
  const float* dy;        /* [rows,128] gradient of the embedder output */
  const float* h3;        /* [rows,128] pre-LayerNorm save */
  const float* mean;      /* [rows] */
  const float* rstd;      /* [rows] */
  const float* gamma;     /* LayerNorm weight [128] */
  const float* rowscale;  /* optional [rows] pair mask */
  const float* h2;        /* [rows,128] post-ReLU layer 2 */
  const float* h1;        /* [rows,128] post-ReLU layer 1 */
  const void* img;
  float* dh3;             /* [rows,128] out */
  float* dh2;
  float* dh1;
  float* dgamma;          /* optional [128], accumulated */
  float* dbeta;           /* optional [128], accumulated */
  long rows;
  int blocks;             /* 0 = two persistent blocks per CU (512) */
  const unsigned* gmask2; /* optional [rows,4]: fd_edge_embed's mask2 -- replaces the read of h2 (h2 may then be null) */
  const unsigned* gmask1; /* optional [rows,4]: fd_edge_embed's mask1 -- replaces the read of h1 */
  unsigned* sched;        /* optional: one word of device scratch for a dynamic tile hand-out (as FdEdgeMlpDesc.sched) */
} FdEdgeEmbedBwdDesc;
int fd_edge_embed_bwd(const FdEdgeEmbedBwdDesc* desc, void* stream);

/* ---- LayerNorm folded into the Linear that consumes it (se3_diffusion_amd/csrc/fd_ln_gemm.hip), sampling sizes (M <= ~1024) ----
 *   out[m, n] = epi( sum_k y[m, k] W[n, k] + bias[n] ),   y = ln_rowscale[m] * (LayerNorm(x[m, :]) * gamma + beta)
 *   epi: ReLU (relu != 0), then + resid[m, n].   ln_out (optional): y itself, for a later launch (a residual branch).
 * norm1 -> linear1 and norm2 -> the next consumer (self_attn.in_proj of the next layer, post_tfmr) of the sequence transformer's
 * TransformerEncoderLayer (post-norm; built at model/ipa_pytorch.py:584-595, post_tfmr :638).  LayerNorm arithmetic as
 * fd_layernorm_fwd (two-pass, eps inside the square root); exact fp32 products (v_mfma_f32_32x32x2_f32).
 * K % 8 == 0, K <= 320; x, W, gamma, beta, ln_out 16-byte aligned, row strides multiples of 4. */
typedef struct FdLnGemmDesc {
  const float* x;          /* [M, K], row stride ldx */
  long ldx;
  const float* gamma;      /* [K] */
  const float* beta;       /* [K] */
  const float* ln_rowscale;/* optional [M] */
  float* ln_out;           /* optional [M, K], row stride ld_ln_out */
  long ld_ln_out;
  const float* W;          /* [N, K], row stride ldw */
  long ldw;
  const float* bias;       /* optional [N] */
  const float* resid;      /* optional [M, N], row stride ld_resid */
  long ld_resid;
  float* out;              /* [M, N], row stride ldo */
  long ldo;
  int M, N, K;
  int relu;
  float eps;
  int ln_cols;             /* 0 = K; else only columns [0, ln_cols) of x are normalised (gamma / beta [ln_cols]), the rest pass through */
} FdLnGemmDesc;
int fd_ln_gemm(const FdLnGemmDesc* desc, void* stream);

/* ---- weight gradients of the pair-row MLPs, grouped (autograd of the Linear layers of EdgeTransition,
 * model/ipa_pytorch.py:194-233: dW = dY^T X with the B*N*N pair rows as the reduction index) ----
 * One launch for up to FD_PAIR_DW_MAX_ITEMS output tiles of 384 x 128 that share the row count
 * (se3_diffusion_amd/csrc/fd_pair_dw.hip):  C[m, n] += sum_p (A[p, m] + [m < 128] A_add[p, m]) * B[p, n].
 * Split-bf16 arithmetic (fp32-accurate, as fd_gemm tile 4); C accumulates atomically. */
#define FD_PAIR_DW_MAX_ITEMS 8
typedef struct FdPairDwItem {
  const float* A;       /* [rows, 384] ([rows, 128] when a_bands == 1), row stride lda: its columns index m */
  long lda;
  const float* A_add;   /* optional [rows, 128], row stride ld_add: added to columns 0..127 of A */
  long ld_add;
  const float* B;       /* [rows, 128] ([rows, b_cols] when b_cols > 0), row stride ldb: its columns index n */
  long ldb;
  float* C;             /* trans == 0: C[m * ldc + n] += ...; trans != 0: C[n * ldc + m] += ... */
  long ldc;
  float* a_colsum;      /* optional [384]: += sum_p A[p, :] (+ A_add) -- the bias gradient when A is dY */
  int trans;
  int a_bands;          /* 0 or 3: A has 384 columns; 1: A has 128 columns (a 128 x 128 tile; no trans / A_add) */
  int b_cols;           /* 0: B has 128 columns; else its column count (a multiple of 4, <= 128): C has b_cols columns */
} FdPairDwItem;
typedef struct FdPairDwDesc {
  FdPairDwItem item[FD_PAIR_DW_MAX_ITEMS];
  int nitems;
  long rows;            /* B * nres * nres */
  int blocks;           /* 0 = one persistent block per CU (256) */
} FdPairDwDesc;
int fd_pair_dw(const FdPairDwDesc* desc, void* stream);

/* ---- grouped node-level weight gradients (se3_diffusion_amd/csrc/fd_group_dw.hip): autograd of the per-residue nn.Linear
 * layers of a trunk block w.r.t. their weights and biases -- IPA's projections and linear_out (model/ipa_pytorch.py:236-301,
 * 455-460), skip_embed / the sequence transformer / post_tfmr (:584-595,632-638), StructureModuleTransition (:169-191),
 * the per-residue halves of EdgeTransition (:194-233), the torsion head (:560-582) and the node embedder
 * (model/score_network.py:57-66) -- as ONE launch instead of one split-K GEMM each:
 *   C_t[m * ldc_t + n] += sum_r A_t[r, m] * B_t[r, n]   (m < n_out_t, n < k_in_t, r < rows)      dW = dY^T X
 *   a_colsum_t[m]      += sum_r A_t[r, m]                (optional)                                db = sum_r dY
 * A_t = dY_t [rows, n_out_t] (row stride lda_t), B_t = X_t [rows, k_in_t] (row stride ldb_t); 16-byte aligned, strides,
 * n_out, k_in multiples of 4.  fp32 in / out, products as 3-term bf16 splits (fp32-accurate, as fd_gemm tile 4). */
#define FD_GROUP_DW_MAX_ITEMS 32
typedef struct FdGroupDwItem {
  const float* A;
  const float* B;
  float* C;
  float* a_colsum;
  int lda, ldb, ldc;
  int n_out, k_in;
} FdGroupDwItem;
typedef struct FdGroupDwDesc {
  FdGroupDwItem item[FD_GROUP_DW_MAX_ITEMS];
  int nitems;
  long rows;            /* B * nres */
  int blocks;           /* 0 = two persistent blocks per CU (512) */
} FdGroupDwDesc;
int fd_group_dw(const FdGroupDwDesc* desc, void* stream);

/* ---- sequence-transformer self-attention, fused (torch.nn.TransformerEncoderLayer.self_attn inside IpaScore,
 * model/ipa_pytorch.py:584-593; nhead 4, d_model 320): out = softmax(scale * q k^T + key_add) v per (batch, head) in one
 * launch (se3_diffusion_amd/csrc/fd_seq_attn.hip).  qkv [B*N, 960] = in_proj output [q | k | v]; key_add [B, N] additive
 * key mask or null; out [B*N, 320]; A_out [B, 4, N, N] optional (the probabilities, for the backward).  N <= 1024. */
int fd_seq_attn_fwd(const float* qkv, const float* key_add, float* out, float* A_out, float scale, int B, int N,
                    void* stream);
/* Backward of that attention in ONE launch (autograd of softmax(q k^T / sqrt(d) + mask) v, model/ipa_pytorch.py:584-593, with
 * respect to q, k, v): dqkv [B*N, 960] = [dQ | dK | dV] from qkv, the saved probabilities A [B,4,N,N], the saved output out [B*N,320]
 * and its gradient dout; replaces two batched fd_gemm launches, fd_row_softmax_bwd and two more batched fd_gemm launches; dA / dS
 * never reach HBM.  16-byte aligned tensors. */
int fd_seq_attn_bwd(const float* qkv, const float* A, const float* dout, const float* out, float* dqkv, float scale, int B, int N,
                    void* stream);

/* ---- embedder features: score_network.py:14-47,97-148; data/utils.py:570-580 ----
 * tscaled = (t*1e4) as fp32 [B]; tfreq[16], idenom[16], dg_lower[22], dg_upper[22] are the
 * host-computed tables of the reference's own op sequence. */
int fd_node_feats(const long* seq_idx, const float* tscaled, const float* fixed, const float* tfreq,
                  const float* idenom, float* out /*[B*N,65]*/, int B, int N, void* stream);
/* the same features with a row stride ld >= 65, columns 65 .. ld-1 written as zeros: K padded for the consumers' latency GEMM */
int fd_node_feats_ld(const long* seq_idx, const float* tscaled, const float* fixed, const float* tfreq,
                     const float* idenom, float* out /*[B*N,ld]*/, long ld, int B, int N, void* stream);
int fd_edge_feats(const long* seq_idx, const float* tscaled, const float* fixed, const float* sc_ca,
                  const float* tfreq, const float* idenom, const float* dg_lower, const float* dg_upper,
                  float* out /*[B*N*N,120]*/, int B, int N, void* stream);

/* ---- Invariant Point Attention, non-GEMM parts: ipa_pytorch.py:303-471 ----
 * layouts in se3_diffusion_amd/csrc/fd_ipa.hip.  Built for base.yaml dims
 * (no_heads 8, c_hidden 256, no_qk_points 8, no_v_points 12). */
/* kp_soa (may be null): a second copy of the key points as [B, 8, 24, n_res] (R = B * n_res rows), the layout the
 * attention kernels read with one lane per key */
int fd_ipa_points_fwd(const float* proj, const float* quat, const float* trans, float* qp, float* kp, float* vp,
                      float* kp_soa, int n_res, long R, int nheads, int c_hidden, int n_qk, int n_v, void* stream);
int fd_ipa_points_bwd(const float* proj, const float* quat, const float* dqp, const float* dkp, const float* dvp,
                      float* dproj, float* dframe, long R, int nheads, int c_hidden, int n_qk, int n_v,
                      void* stream);
int fd_ipa_softmax_fwd(float* S, const float* zb, const float* qp, const float* kp, const float* head_w,
                       const float* mask, int B, int N, void* stream);
/* hw_part: [B*N, 8] scratch (per-query-row partials of the head-weight gradient, column-summed into dhead_w) */
int fd_ipa_softmax_bwd(const float* A, float* dA, const float* qp, const float* kp, const float* head_w,
                       float* dzb, float* dqp, float* dkp, float* dhead_w, float* hw_part, int B, int N,
                       void* stream);
int fd_ipa_opt_fwd(const float* optg, const float* quat, const float* trans, float* feats, long R, void* stream);
int fd_ipa_opt_bwd(const float* dfeats, const float* feats, const float* quat, float* doptg, float* dframe,
                   long R, void* stream);
int fd_ipa_opair_fwd(const float* A, const float* zb, float* feats, int B, int N, void* stream);
int fd_ipa_opair_bwd(const float* A, const float* zb, const float* dfeats, float* dA, float* dzb, int B, int N,
                     void* stream);

/* softmax + o_pair of a query row in one launch (fd_ipa_softmax_fwd followed by fd_ipa_opair_fwd: the probabilities bit-identical,
 * o_pair equal to fp32 rounding -- up to 512 query rows the block is 512 threads, one wave per head, and sums o_pair in two halves
 * of the keys), and
 * their backward (fd_ipa_opair_bwd followed by fd_ipa_softmax_bwd): the probabilities / the updated dA stay in LDS.
 * kp_soa (may be null): fd_ipa_points_fwd's [B, 8, 24, N] copy of kp; when given, the key points are read from it */
int fd_ipa_attn_fwd(float* S, const float* zb, const float* qp, const float* kp, const float* kp_soa,
                    const float* head_w, const float* mask, float* feats, int B, int N, void* stream);
int fd_ipa_attn_bwd(const float* A, float* dA, const float* zb, const float* dfeats, const float* qp, const float* kp,
                    const float* kp_soa, const float* head_w, float* dzb, float* dqp, float* dkp, float* dhead_w,
                    float* hw_part, int B, int N, void* stream);

/* IPA attention of a block of the trunk in ONE launch (model/ipa_pytorch.py:380-457: logits :380-417, softmax :422,
 * o :424-428, o_pt + norm :432-449, o_pair :455-457) -- replaces  fd_gemm (q k^T) -> fd_ipa_attn_fwd -> fd_gemm (a v) ->
 * fd_gemm (a v_pts) -> fd_ipa_opt_fwd.  A block owns 16 query rows and heads_per_block heads (one wave each); keys walk in
 * tiles of 16 with a running maximum / denominator; the zb rows of the tile stream through LDS by LDS-DMA; q k^T, a v, a v_pts
 * and o_pair ride the exact-fp32 MFMA; the logits / probabilities never reach HBM.
 *   proj [R, 6816] (fd_ipa_points_fwd's input: q | kv | raw points), zb [B N N, 40], qp / kp [R, 8, 24] and vp [R, 8, 36]
 *   (global-frame points from fd_ipa_points_fwd), head_w [8], mask [R], quat [R, 4], trans [R, 3] ->
 *   feats [R, 2688] = [o 2048 | o_pt x,y,z 288 | |o_pt| 96 | o_pair 256]  (every column written).
 * A (may be null): [B, 8, N, N] receives the probabilities (training: the backward kernels read them).
 * heads_per_block: 8, 4, 2, or 0 = chosen from the number of query tiles.  All tensor arguments 16-byte aligned. */
int fd_ipa_flash_fwd(const float* proj, const float* zb, const float* qp, const float* kp, const float* vp,
                     const float* head_w, const float* mask, const float* quat, const float* trans, float* feats,
                     float* A, int B, int N, int heads_per_block, void* stream);
/* The same with the KEYS of a query tile split over key_splits blocks (inference on a lone backbone: B ceil(N/16) query tiles do
 * not fill 256 CUs): block ks walks the key tiles [ks nt / key_splits, (ks + 1) nt / key_splits) and leaves unnormalised sums
 * + (running maximum, denominator) per (split, residue, head) in `part` -- key_splits * B * N * 8 * FD_IPA_FLASH_PART_LD floats,
 * 16-byte aligned -- and a second launch (one block per residue) combines the splits and writes feats.  key_splits == 1 is
 * fd_ipa_flash_fwd; A must be null when key_splits > 1. */
#define FD_IPA_FLASH_PART_LD 328
int fd_ipa_flash_fwd_split(const float* proj, const float* zb, const float* qp, const float* kp, const float* vp,
                           const float* head_w, const float* mask, const float* quat, const float* trans, float* feats,
                           float* A, int B, int N, int heads_per_block, int key_splits, float* part, void* stream);

/* Query side of the IPA attention backward in ONE launch (autograd of model/ipa_pytorch.py:380-457 with the probabilities A
 * saved by the forward) -- replaces  fd_gemm (dA = dO V^T) -> fd_gemm (dA += dOpt vpts^T) -> fd_ipa_attn_bwd's per-row kernel;
 * dA never exists.  dL = A (dP - D) with dP = dO.v + dOpt.vpts + dout.zd on the exact-fp32 MFMA, D from the forward's outputs
 * (dO.o + dout.opair + ptdot) ->
 *   dL [B, 8, N, N] (written once: the dQ / dK GEMMs and the key-point gradient that follow read it),
 *   dzb [B N N, 40] = [sqrt(1/3) dL | sum_h A dout], dqp [R, 8, 24], dkp [R, 8, 24] (fd_ipa_kpts_bwd on dL), dhead_w [8] (+=;
 *   hw_part [R, 8] is scratch).
 * proj [R, 6816], A [B, 8, N, N], zb [B N N, 40], dfeats / feats [R, 2688], doptg [R, 8, 36] and ptdot [R, 8] from
 * fd_ipa_opt_bwd_dot, qp / kp [R, 8, 24], vp [R, 8, 36] (global frame), head_w [8], trans [R, 3].  16-byte aligned tensors. */
int fd_ipa_flash_bwd(const float* proj, const float* A, const float* zb, const float* dfeats, const float* feats,
                     const float* doptg, const float* ptdot, const float* qp, const float* kp, const float* vp,
                     const float* head_w, const float* trans, float* dL, float* dzb, float* dqp, float* dkp,
                     float* dhead_w, float* hw_part, int B, int N, void* stream);
/* KEY side of the same backward in one launch (se3_diffusion_amd/csrc/fd_ipa_flash.hip, ipa_flash_bwd_keys_kernel): autograd of
 * model/ipa_pytorch.py:380-457 with respect to keys / values and their points, from the probabilities A and the logit gradient dL
 * ([B,8,N,N] each, read once):  dproj[:, 2048 + 512 h + 256 ..] = dV = A^T dO;  dproj[:, 2048 + 512 h ..] = dK = sqrt(1/3C) dL^T Q;
 * dvp [R,8,36] = A^T doptg;  dkp [R,8,24] = gamma_h sum_i dL_ij (qp_i - kp_j).  Replaces three batched fd_gemm launches and
 * fd_ipa_kpts_bwd (pass dkp = NULL to fd_ipa_flash_bwd to skip its own fd_ipa_kpts_bwd).  heads_per_block: 0 = by size, 2 / 4 / 8. */
int fd_ipa_flash_bwd_keys(const float* A, const float* dL, const float* proj, const float* dfeats, const float* doptg,
                          const float* qp, const float* kp, const float* head_w, float* dproj, float* dvp, float* dkp,
                          int B, int N, int heads_per_block, void* stream);
/* fd_ipa_opt_bwd that also returns ptdot [R, 8] = sum_p d(o_pt, global frame) . (o_pt, global frame) per head (the o_pt term
 * of the softmax backward's row constant; model/ipa_pytorch.py:432-449) */
int fd_ipa_opt_bwd_dot(const float* dfeats, const float* feats, const float* quat, const float* trans, float* doptg,
                       float* dframe, float* ptdot, long R, void* stream);

/* dz[p, 0:128] (+)= dzb[p, 0:40] W40[0:40, 0:128] over the pair rows (autograd of linear_b / down_z w.r.t. z,
 * ipa_pytorch.py:380-386,455-457): streaming kernel, W40 resident in registers */
int fd_ipa_dz_acc(const float* dzb, const float* W40, float* dz, long rows, int accumulate, void* stream);

/* dkp[b,j,h,:] = gamma_h sum_i dLogits[b,h,i,j] (qp[b,i,h,:] - kp[b,j,h,:]) (the key-side point gradient) */
int fd_ipa_kpts_bwd(const float* dL, const float* qp, const float* kp, const float* head_w, float* dkp, int B, int N,
                    void* stream);

/* ---- sequence-transformer softmax (nn.MultiheadAttention, ipa_pytorch.py:584-593) ---- */
int fd_row_softmax_fwd(float* S, const float* key_add, long rows, int N, int rows_per_batch, void* stream);
int fd_row_softmax_bwd(const float* A, float* dA, long rows, int N, void* stream);

/* ---- input frames: rigids_t [R,7] -> quat [R,4], trans [R,3] * scale (scale_rigids, model/score_network.py:190-193) and,
 * optionally, tscaled[b] = t[b] * tscale for the B examples (the embedder's timestep argument, score_network.py:38,43) ---- */
int fd_split_rigids(const float* rig7, float scale, const float* t, float tscale, float* quat, float* trans, float* tscaled,
                    long R, int B, void* stream);

/* ---- backbone update: ipa_pytorch.py:530-557,641-644; rigid_utils.py:266-275,587-616,1039-1063 ---- */
int fd_bb_update_fwd(const float* node, long ldn, int cs, const float* dmask, const float* W6, const float* b6,
                     const float* quat, const float* trans, float* upd, float* quat_out, float* trans_out,
                     long R, void* stream);
int fd_bb_update_bwd(const float* dquat_out, const float* dtrans_out, const float* dframe, const float* dmask,
                     const float* upd, const float* quat, float* dquat, float* dtrans, float* dupd, float* dupd_s,
                     long R, void* stream);

/* ---- score heads + psi + backbone atoms: ipa_pytorch.py:650-672, se3_diffuser.py:115-125,
 * so3_diffuser.py:9-117,182-213,274-305, r3_diffuser.py:42-43,148-166, all_atom.py:152-174 ---- */
typedef struct FdHeadConst {
  float atoms[15];       /* N, CA, C, CB, O idealised local coordinates (ALA) */
  float Rd[9];           /* psi rigid-group default frame rotation */
  float td[3];           /* ... translation */
  float coord_scale;     /* 0.1 */
  double exp_max_sigma, exp_min_sigma;
  float min_b, max_b;
  int L;                 /* IGSO(3) truncation (1000) */
  /* so3.use_cached_score=True (config/icml_published.yaml; so3_diffuser.py:293-299): device table [ng, n_omega] of
   * score norms + its omega grid [n_omega]; the rotation score is then the bucketised lookup instead of the series
   * (and carries no gradient through the lookup, like torch.gather of a constant).  NULL = series. */
  const double* score_norms;
  const double* omega_grid;
  int n_omega;
} FdHeadConst;
int fd_heads_fwd(const float* rig0, const float* quatF, const float* transF, const float* upsi,
                 const float* gt_psi, long gt_stride, const float* fixed, const float* mask, const float* t,
                 const double* sigma_grid, int ng, const FdHeadConst* c, double* rot_score, float* trans_score,
                 float* rigids, float* psi_out, float* atom37, float* atom14,
                 float* sc_ca_out /* optional [R,3]: the predicted CA positions (= rigids[..., 4:7]) once more, where the sampling
                 loop keeps its self-conditioning input (experiments/train_se3_diffusion.py:763-765) */,
                 int B, int N, void* stream);
/* data/all_atom.py:152-174 compute_backbone as one kernel: rigids [R,7] (A), psi [R,2] (sin,cos) */
int fd_backbone_atoms(const float* rigids, const float* psi, const FdHeadConst* c, float* atom37, float* atom14,
                      long R, void* stream);
int fd_heads_bwd(const float* rig0, const float* quatF, const float* transF, const float* upsi,
                 const float* psi_out, const float* fixed, const float* mask, const float* t,
                 const double* sigma_grid, int ng, const FdHeadConst* c, const double* d_rot,
                 const float* d_trans_score, const float* d_rigids, const float* d_psi, const float* d_atom37,
                 float* dquatF, float* dtransF, float* dupsi, int B, int N, void* stream);

/* ---- SE(3) diffuser (fp64 arithmetic, fp32 [..,7] frames in Angstrom) ----------------
 * Random draws are inputs in the reference's call order, so identical noise gives identical frames.
 * fd_igso3_tables     data/so3_diffuser.py:122-180   pdf/cdf/score_norms [ns, no] (8 MB each at 1000^2)
 * fd_sample_ref       data/se3_diffuser.py:216-268   prior: IGSO3(t=1) x N(0, I) (scaled units -> A)
 * fd_forward_marginal data/se3_diffuser.py:43-110    noised frames + DSM score targets at time t
 * fd_se3_reverse_step data/se3_diffuser.py:160-214   one Euler-Maruyama / geodesic-random-walk step */
int fd_igso3_tables(const double* sigma, const double* omega, int ns, int no, int L, double* pdf, double* cdf,
                    double* score_norms, void* stream);
int fd_sample_ref(const double* z_axis, const double* u, const double* z_trans, const double* cdf_row,
                  const double* omega, int no, double coord_scale, float* out, long n, void* stream);
int fd_forward_marginal(const float* rig0, const double* z_axis, const double* u, const double* z_trans,
                        const double* cdf_row, const double* omega, int no,
                        const double* score_row /* optional: this sigma's score_norms row (use_cached_score) */,
                        double sigma, double beta, double coord_scale, int L, const float* mask, float* rig_t,
                        double* rot_score, double* trans_score, long n, void* stream);
/* a training batch in one launch (pdb_data_loader.py:240-262 calls forward_marginal once per example, each with its
 * own t): cdf / score_norms are the full [ns, no] tables, tparams [B,3] (device, fp64) = {sigma bin = t_to_idx(t_b),
 * discrete sigma of that bin, marginal_b_t(t_b)}; everything else is [B,N,...] as above. */
int fd_forward_marginal_batch(const float* rig0, const double* z_axis, const double* u, const double* z_trans,
                              const double* cdf, const double* omega, int no,
                              const double* score_norms /* optional, use_cached_score */, const double* tparams,
                              double coord_scale, int L, const float* mask, float* rig_t, double* rot_score,
                              double* trans_score, int B, int N, void* stream);
int fd_se3_reverse_step(const float* rig_t, const double* rot_score, const double* trans_score,
                        const double* z_rot, const double* z_trans, const float* mask, int B, int N, double g_rot,
                        double b_t, const double* tparams /* optional device {g_rot, b_t}: overrides the scalars,
                        lets one captured hipGraph serve every t */, double dt, double noise_scale,
                        double coord_scale, int center, int diffuse_rot, int diffuse_trans, float* out, void* stream);
/* the same step with the scores as the network stores them (float32, widened in registers: the same numbers the reference
 * passes after its .to(float64)); out may be rig_t (in place) in both forms */
int fd_se3_reverse_step_f32(const float* rig_t, const float* rot_score, const float* trans_score,
                        const double* z_rot, const double* z_trans, const float* mask, int B, int N, double g_rot,
                        double b_t, const double* tparams /* optional device {g_rot, b_t}: overrides the scalars,
                        lets one captured hipGraph serve every t */, double dt, double noise_scale,
                        double coord_scale, int center, int diffuse_rot, int diffuse_trans, float* out, void* stream);
/* ... and as ScoreNetwork.forward returns them: rot_score float64, trans_score float32 */
int fd_se3_reverse_step_net(const float* rig_t, const double* rot_score, const float* trans_score,
                        const double* z_rot, const double* z_trans, const float* mask, int B, int N, double g_rot,
                        double b_t, const double* tparams, double dt, double noise_scale,
                        double coord_scale, int center, int diffuse_rot, int diffuse_trans, float* out, void* stream);
/* The per-step host glue of the reverse loop (experiments/train_se3_diffusion.py:746-781: t = reverse_steps[i], the draws of
 * diffuser.reverse) as the FIRST NODE of a captured step: idx = *counter; t_out[0..B) = all_t[idx]; tparams[0..2) =
 * all_tp[2 idx ..] ({g_rot(t), b(t)} of fd_se3_reverse_step); z_out[0..nz) = z_all[(idx % K) nz ..] (K steps of normal draws,
 * rotation block then translation block per step, refilled by the caller every K steps); *counter = idx + 1.  One block. */
int fd_sample_advance(int* counter, const float* all_t, const double* all_tp, const double* z_all, int K, long nz, float* t_out,
                      int B, double* tparams, double* z_out, void* stream);
/* The trajectory bookkeeping of Experiment.inference_fn(aux_traj=True) (experiments/train_se3_diffusion.py:782-803: four
 * du.move_to_np copies and two compute_backbone calls per step, flipped at :805-812) as ONE launch per diffusion step into
 * preallocated device buffers.  Rows R = B*N, contiguous fp32.  step = (slot_ptr ? *slot_ptr : 0) + slot_offset (slot_ptr: a
 * device int the kernel only reads, e.g. the counter of fd_sample_advance with slot_offset = -1); the slice is written at the
 * FLIPPED index T-1-step of
 *   rigid_traj [T+1,R,7]  rigids_t (:782-784; index T is the starting frames, written by the caller)
 *   bb_t       [T,R,5,3]  N, CA, C, CB, O of compute_backbone(rigids_t, psi) (:801-803)
 *   bb_0       [T,R,5,3]  the same atoms of compute_backbone(rigid_pred, psi) (:794-799)
 *   trans_0    [T,R,3]    (1-fixed_mask)*res_mask * rigid_pred[4:7] + fixed_mask*res_mask * rigids_t[4:7] (:787-790)
 * aux = 0 (aux_traj=False): bb_t only; rigid_pred, the masks and the other three buffers may be NULL.  A step outside [0,T) is an
 * argument error when slot_ptr is NULL and a skipped write otherwise. */
int fd_sample_record(const float* rigids_t, const float* rigid_pred, const float* psi, const float* fixed_mask,
                     const float* res_mask, const FdHeadConst* c, const int* slot_ptr, int slot_offset, int T, long R, int aux,
                     float* rigid_traj, float* bb_t, float* bb_0, float* trans_0, void* stream);

/* ---- training loss (the step next to the hot path): experiments/train_se3_diffusion.py:524-693 ----
 * Experiment.loss_fn, both rotation branches: translation score / x0 loss, rotation axis + angle (or joint MSE) loss,
 * backbone-atom loss and the 5N x 5N distance-matrix loss with their per-example normalisers and t filters, value AND
 * gradient w.r.t. the network outputs in three launches.  loss[0] = sum_b final_b / #non-empty examples.
 * terms[b] = {trans_score_loss, trans_x0_loss, axis_loss, angle_loss (weighted), bb_atom_loss (weighted),
 * dist_mat_loss (weighted), final_b, sum of the loss mask}.  scratch: B*N*15 + 2*B floats. */
typedef struct FdLossDesc {
  int B, N;
  const float* res_mask;            /* [B,N] */
  const float* fixed_mask;          /* [B,N] */
  const float* t;                   /* [B]   */
  const float* gt_trans_score;      /* [B,N,3] */
  const double* gt_rot_score;       /* [B,N,3] */
  const float* trans_score_scaling; /* [B] */
  const float* rot_score_scaling;   /* [B] */
  const float* gt_rigids;           /* [B,N,7] rigids_0 */
  const float* gt_atom37;           /* [B,N,37,3] */
  const double* rot_score;          /* network outputs: [B,N,3] fp64 */
  const float* trans_score;         /* [B,N,3] */
  const float* rigids;              /* [B,N,7] */
  const float* atom37;              /* [B,N,37,3] */
  float coordinate_scaling, trans_x0_threshold, trans_loss_weight, rot_loss_weight, rot_loss_t_threshold;
  float bb_atom_loss_weight, bb_atom_loss_t_filter, aux_loss_weight, dist_mat_loss_weight, dist_mat_loss_t_filter;
  double* d_rot_score;              /* gradients of loss[0], same shapes as the outputs */
  float* d_trans_score;
  float* d_rigids;
  float* d_atom37;
  float* terms;                     /* [B,8] */
  float* loss;                      /* [1] */
  float* scratch;
  int joint_rot_loss;               /* 0: separate_rot_loss=True (axis + angle, base.yaml); 1: joint rot-score MSE
                                       (train_se3_diffusion.py:597-604, icml_published.yaml), reported in terms[:,3] */
} FdLossDesc;

int fd_dsm_loss(const FdLossDesc* desc, void* stream);

/* Adam (torch.optim.Adam defaults, experiments/train_se3_diffusion.py:139) over flat fp32 buffers of n elements
 * (n % 4 == 0, 16-byte aligned): m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2;
 * p -= lr/bc1 * m / (sqrt(v)/sqrt(bc2) + eps) with bc_i = 1 - b_i^t supplied by the host. */
int fd_adam_step(float* p, const float* g, float* m, float* v, long n, float lr, float b1, float b2, float eps,
                 float bc1, float bc2, void* stream);

/* fd_adam_step that also carries an exponential moving average of the parameters (the weights a diffusion model is sampled
 * from; the reference keeps none) in a fifth flat buffer of the same length and alignment: after p is updated,
 * ema += one_minus_decay * (p - ema) on the same elements, in the same launch (8 more bytes per parameter).
 * one_minus_decay = (float)(1 - d_t) strictly between 0 and 1, supplied by the host like bc_i (a warm-up schedule of d_t is
 * the caller's); p, m, v come out bit for bit as from fd_adam_step. */
int fd_adam_step_ema(float* p, const float* g, float* m, float* v, float* ema, long n, float lr, float b1, float b2, float eps,
                     float bc1, float bc2, float one_minus_decay, void* stream);

/* ---- gradient health and the guarded optimiser step (se3_diffusion_amd/csrc/fd_optim.hip) ----
 * No reference lines stand behind these two: the reference tests torch.isnan(loss) on the host once per step and aborts
 * (experiments/train_se3_diffusion.py:448-454).  The torch calls they restate are torch.nn.utils.clip_grad_norm_ followed
 * by torch.optim.Adam.step, the step taken only when every gradient element is finite -- with the norm, the decision,
 * the step counter and the bias corrections kept on the device, so the host reads nothing back and the launches can be
 * captured and replayed.  All sums are fp64 over per-block partials written with plain stores and added in a fixed order:
 * bitwise reproducible for a given n.
 *
 * workspace: FD_OPT_WS_DOUBLES doubles of device scratch (per-block partials; launches that may run at the same time need
 * workspaces of their own).  The entry points follow the empty-input rule: n == 0 returns FD_OK without a launch and
 * without touching stats / p / m / v / state. */
#define FD_OPT_WS_DOUBLES (3 * 4096)
#define FD_OPT_STATE_BYTES 72
/* The optimiser's device-resident state; zero-initialised by the caller before the first step.  Counters accumulate over
 * the calls, the remaining fields describe the latest call. */
typedef struct FdOptState {
  long step;          /* applied steps (the t of Adam's bias corrections) */
  long skipped;       /* calls that left p, m, v untouched because of a non-finite gradient element */
  long clipped;       /* applied steps whose coefficient was below 1 */
  long nonfinite;     /* non-finite elements (inf, -inf, NaN) of the latest gradient */
  double grad_norm;   /* L2 norm over the finite elements of the latest gradient */
  double clip_coef;   /* min(1, max_norm / (grad_norm + 1e-6)) of the latest call; 1 without clipping and for a skipped call */
  double max_abs;     /* max |g| over the finite elements */
  float bc1;          /* 1 - b1^step              \  of the latest applied step: computed in fp64, */
  float rsqrt_bc2;    /* 1 / sqrt(1 - b2^step)    /  rounded once to fp32                          */
  float coef;         /* clip_coef rounded to fp32: the factor the update kernel applies to g */
  int apply;          /* 1: the latest call updated p, m, v; 0: it skipped */
} FdOptState;

/* stats[4] (device) = {sum of squares over the finite elements, count of non-finite elements, max |g| over the finite elements, 0}
 * of g[0:n] (n % 4 == 0, 16-byte aligned; zero padding adds nothing); workspace and stats 8-byte aligned.  For callers that keep torch.optim.Adam over
 * dist.FlatGrads: take it after the all-reduce, so every rank sees the same figures. */
int fd_grad_stats(const float* g, long n, double* workspace, double* stats, void* stream);

/* The guarded fd_adam_step, three dependent launches: statistics of g; the decision
 *   apply = !(skip_nonfinite && nonfinite > 0);
 *   apply: step += 1, coef = max_norm > 0 ? min(1, max_norm / (norm + 1e-6)) : 1, bc_i from the new step, clipped += coef < 1
 *   else : skipped += 1 (coef = 1)
 * written into *state (FD_OPT_STATE_BYTES of DEVICE memory, 8-byte aligned); and fd_adam_step's update on coef * g with
 * lr / bc1 and 1/sqrt(bc2) read from the state, which touches neither p, m nor v when apply == 0.  g is NOT rewritten: it
 * keeps the unclipped gradient (unlike clip_grad_norm_).  max_norm <= 0: no clipping.  The norm is taken over the finite
 * elements; with skip_nonfinite == 0 a non-finite element therefore reaches its own p, m, v (and only those). */
int fd_adam_step_guarded(float* p, const float* g, float* m, float* v, long n, double lr, double b1, double b2, double eps,
                         double max_norm, int skip_nonfinite, double* workspace, void* state, void* stream);

/* fd_adam_step_guarded that also carries the moving average of fd_adam_step_ema: the update launch ends with
 * ema += a * (p - ema), a = (float)(1 - d_t), d_t = ema_warmup ? min(ema_decay, (1 + t) / (10 + t)) : ema_decay in fp64 on
 * the device, t = state->step after this call's decision (applied steps, this one included).  apply == 0 touches neither
 * p, m, v nor ema, so the average never sees a step that was not taken and the warm-up does not advance.  ema_decay strictly
 * between 0 and 1; the state keeps its layout (nothing of the average lives in it); p, m, v and *state come out bit for bit
 * as from fd_adam_step_guarded. */
int fd_adam_step_guarded_ema(float* p, const float* g, float* m, float* v, float* ema, long n, double lr, double b1, double b2,
                             double eps, double max_norm, int skip_nonfinite, double* workspace, void* state, double ema_decay,
                             int ema_warmup, void* stream);

/* ---- scoring sampled backbones (se3_diffusion_amd/csrc/fd_metrics.hip) ----
 * The coordinate arithmetic of the reference's sample evaluation (Experiment.eval_fn -> analysis/metrics.py::protein_metrics),
 * left on the device as fp64: one launch per call, no floating-point atomics, every sum in a fixed order (bitwise
 * reproducible for a given shape).  The empty-input rule holds: B == 0, P == 0 or N == 0 returns FD_OK without a launch and
 * writes nothing.  N <= 4096.
 *
 * The backbone figures, one block per backbone.  Residue r of backbone b starts at atoms + (b N + r) atom_stride floats and holds
 * N, CA, C, CB, O in slots 0..4 (three floats each): atom_stride = 111 for atom37 [B,N,37,3], 15 for [B,N,5,3]; below 15 it is
 * refused.  A residue is present iff res_mask[b,r] != 0; the present residues are compacted in index order, as the reference
 * does by boolean indexing (analysis/metrics.py:94-95), and rows that are not present are never read into a result.  With n
 * present residues, out[b][0..12) =
 *   0 num_res                  n
 *   1 ca_ca_bond_dev           mean over the n-1 consecutive compacted pairs of |d - 3.80209737096|   (metrics.py:120-125)
 *   2 ca_ca_valid_percent      mean of (d < 3.80209737096 + 0.1) on the same pairs                     (metrics.py:120-125)
 *   3 num_ca_steric_clashes    number of compacted pairs i < j with 0 < D_ij < 1.5                     (metrics.py:127-132)
 *   4 ca_steric_clash_percent  slot 3 / number of pairs i < j with D_ij > 0                            (metrics.py:127-132)
 *   5 ca_radius_of_gyration    sqrt(mean |ca - mean ca|^2) over the present CA atoms, in Angstrom (NOT mdtraj's figure of
 *                              metrics.py:62, which takes all atoms and reports nm)
 *   6 c_n_bond_dev             mean over the same consecutive pairs of | |C_i - N_{i+1}| - 1.329 |
 *   7 c_n_bond_valid_percent   mean of (| |C_i - N_{i+1}| - 1.329 | <= 12 * 0.014): openfold's non-proline peptide bond
 *                              length and standard deviation at its tolerance factor 12 (residue_constants.py:546-547)
 *   8 max_ca_ca_dist           max of the consecutive CA-CA distances (0 if there is none)
 *   9..11                      0
 * A mean over an empty set is NaN (as np.mean gives): n < 2 gives NaN in slots 1, 2, 4, 6, 7, n == 0 in slot 5 as well. */
int fd_backbone_metrics(const float* atoms, long atom_stride, const float* res_mask, int B, int N, double* out, void* stream);

/* Optimal superposition of P pairs of point sets, one block per pair (analysis/metrics.py:71-73 calc_aligned_rmsd on
 * data/utils.py:519-568 rigid_transform_3D).  Point k of set s starts at A + (s N + k) a_stride floats (B likewise, with
 * b_stride): a stride of 111 on a pointer to the CA slot reads the CA column of atom37 in place.  Pair p superposes set ia[p] of
 * A onto set ib[p] of B (ia == ib == NULL: set p of both).  mask (optional, [*,N], indexed like the sets): position k counts iff
 * it is non-zero in both sets.  The rotation is the optimal PROPER one -- what rigid_transform_3D returns after its reflection
 * fix -- from the largest eigenvector of Horn's symmetric 4x4 matrix of the fp64 cross-covariance (cyclic Jacobi).  With
 * d_k = |R a_k + t - b_k| over the L counted positions, out[p][0..8) =
 *   0 L
 *   1 mean_dist    mean d_k: what calc_aligned_rmsd returns (a mean of norms, not a root mean square; quirk and name kept)
 *   2 rmsd         sqrt(mean d_k^2)
 *   3 tm_kabsch    (1/L) sum 1 / (1 + (d_k/d0)^2), d0 = 1.24 cbrt(L - 15) - 1.8 for L > 21, else 0.5: the TM-score formula
 *                  under THIS one superposition, a lower bound of the TM-score of the given correspondence (not TM-align's value)
 *   4 reflection   1.0 iff det(covariance) < 0: rigid_transform_3D's reflection_detected
 *   5 max_dist     max d_k
 *   6, 7           0
 * L == 0 gives NaN in slots 1, 2, 3, 5.  transform (optional): [P][12] = R row-major, then t, with aligned = R a + t as in the
 * reference's return value.  With fewer than three non-collinear points the distances are those of an optimal superposition
 * and R is unspecified. */
int fd_aligned_rmsd(const float* A, long a_stride, const float* B, long b_stride, const int* ia, const int* ib,
                    const float* mask, int P, int N, double* out, double* transform, void* stream);

/* The TM-score of P pairs under their GIVEN residue-to-residue correspondence, by the superposition search of Zhang & Skolnick's
 * TM-score program: the tm_score column of the reference's EVAL_METRICS (analysis/metrics.py:44-46,104-105) for pairs whose
 * correspondence is fixed -- sample against ground truth, against its refolded self, against another sample of equal length.
 * NOT TM-align: the reference calls tmtools.tm_align, which also searches over alignments; that search is fd_tm_align below, which
 * runs this search on the pair lists it builds.  Agreement with the printed values of tmtools or of the TM-score program has not
 * been verified for either (neither is available to this project's tests; they check a float64 restatement of the search below).  Operands as fd_aligned_rmsd (strided points read in place,
 * ia / ib together or not at all, mask rows indexed like the sets, 8-byte aligned fp64 operands, P == 0 or N == 0 returns FD_OK
 * without a launch); N <= 2048, seed_step >= 1, max_iter >= 0, parts >= 1 and a non-null ws, or the call is refused.
 *
 * The search.  The counting positions (mask non-zero in both sets; all without a mask) are compacted in index order; L is their
 * number, d0 = 1.24 cbrt(L - 15) - 1.8 for L > 21, else 0.5, and d0s = min(max(d0, 4.5), 8).  All arithmetic after the fp32 loads
 * is fp64.  Fragment lengths: L, L >> 1, L >> 2, ... while above 4 (at most six), then 4.  Seeds: for each length in that order
 * the starts 0, seed_step, 2 seed_step, ... <= L - length, numbered from 0; seed 0 is the whole set.
 *   score(R, t, dcut): d2_k = |R a_k + t - b_k|^2; s = (1/L) sum_k 1 / (1 + d2_k / d0^2); selection = {k: d2_k < dcut^2}; while
 *                      fewer than 3 positions are selected, dcut += 0.5 and select again (given up after 4096 increments, which
 *                      only absurd coordinates reach; not attempted when s is not finite -- a NaN or infinite coordinate
 *                      among the counting positions -- since such a call can never be the result).
 *   per seed:          superpose the fragment (optimal proper rotation of the centred selected positions, Horn's quaternion as in
 *                      fd_aligned_rmsd); score(R, t, d0s - 1); then up to max_iter times: superpose the current selection,
 *                      score(R, t, d0s + 1), stop when the new selection equals the old one.
 * Every call of score is a candidate; the result is the candidate of the greatest s -- on ties the earliest within a seed and the
 * lowest seed number.  One wave owns one seed at a time (grid of P * parts blocks of four waves: wave w of part c of a pair takes
 * the seeds 4 c + w, + 4 parts, ...); the arithmetic of a seed does not depend on which wave ran it, each wave leaves one partial
 * in ws, and a second small launch reduces them in a fixed order: no floating-point atomics, results bitwise reproducible and
 * bitwise independent of parts.
 *   ws: caller-provided scratch of P * parts * 64 doubles (FD_TM_WS_DOUBLES), need not be initialised.
 * out[p][0..8) =
 *   0 num_aligned  L
 *   1 tm_score     the greatest s found (the TM-score of the given correspondence, normalised by L)
 *   2 tm_kabsch    the first s of seed 0: the formula under the one least-squares superposition (fd_aligned_rmsd's slot 3)
 *   3 best_seed    number of the seed that found slot 1
 *   4 num_seeds    seeds searched
 *   5 d0
 *   6 passes       calls of score over all seeds: an exact integer, the cost unit of a pair
 *   7              0
 * L == 0: slots 1, 2 NaN, best_seed -1, num_seeds 0, passes 0.  1 <= L <= 3: no search -- tm_score = tm_kabsch under the
 * whole-set superposition, best_seed -1, num_seeds 0, passes 0.  transform (optional): [P][12] = R row-major, then t, of the
 * superposition that gave slot 1, with aligned = R a + t. */
#define FD_TM_WS_DOUBLES(P, parts) ((long)(P) * (long)(parts) * 64L)
int fd_tm_search(const float* A, long a_stride, const float* B, long b_stride, const int* ia, const int* ib, const float* mask,
                 int P, int N, int seed_step, int max_iter, int parts, double* ws, double* out, double* transform, void* stream);

/* ---- TM-align: the search over alignments (se3_diffusion_amd/csrc/fd_tm_align.hip) ----
 * The alignment search of TM-align (Zhang & Skolnick 2005) as restated below, for chains of any two lengths: what the reference's
 * tm_score column (analysis/metrics.py:44-46,104-105, tmtools.tm_align) computes.  Agreement with the values tmtools prints is NOT
 * verified: tmtools does not exist where this project is built and tested.  Verified are a float64 restatement of this text,
 * analytic properties (rigid copies, deletions, identical chains) and plausibility on deposited chains.  Deliberate
 * simplifications are listed at the end.  All decisions are made in fp64 from the fp32 coordinates; distance cut-offs use strict <
 * on squared distances, as fd_tm_search does.
 *
 * Operands.  Point sets A [*,Na,3] and B [*,Nb,3] with point strides, read in place as in fd_tm_search.  mask_a [*,Na], mask_b
 * [*,Nb] (optional, indexed like the sets): the counting positions of a set are those with a non-zero mask, compacted in index
 * order; their numbers are La and Lb.  Padded positions are never read for arithmetic (NaN there does not leak).  Pair p aligns set
 * ia[p] of A to set ib[p] of B (both NULL: set p of both).  Na, Nb <= FD_TM_ALIGN_MAX_N.  Every index below is a compacted index;
 * Lmin = min(La, Lb).
 *
 * Constants.  d0(L) = 1.24 cbrt(L - 15) - 1.8 for L > 21, else 0.5.  Search phase: d0 = d0(Lmin) + 0.8, d0s = min(max(d0, 4.5), 8),
 * d8 = 1.5 Lmin^0.3 + 3.5.
 *
 *   search(pairs, Lnorm, d0, step)   fd_tm_search's per-seed procedure on the list of aligned pairs (n of them): the same fragment
 *                  lengths (n, n >> 1, ... while above 4, then 4), seeds (starts 0, step, 2 step, ... <= n - length), score with its
 *                  widening, and cut-offs d0s - 1 and d0s + 1 with d0s = min(max(d0, 4.5), 8) of the d0 GIVEN, max_iter 20; the sum is
 *                  divided by Lnorm, not by n.  n < 4: one superposition of all pairs, no seeds.  Returns the best (s, R, t); ties as
 *                  in fd_tm_search (earliest within a seed, lowest seed).
 *   quick(alignment)   n pairs; n < 3 gives -1.  Superpose all pairs: s1 = (1/Lmin) sum 1 / (1 + d2 / d0^2).  Select d2 < d0s^2; if
 *                  at least 3 pairs are selected, superpose the selection and score all pairs: s2.  From THOSE distances select
 *                  d2 < (d0s + 1)^2; if at least 3, the same again: s3.  A selection below 3 stops the chain.  The result is the
 *                  greatest of these, the earliest on ties, with its (R, t).
 *   DP(S, gap)     val[0][*] = val[*][0] = 0 and path false there.  For i = 1..La, j = 1..Lb: h = val[i-1][j-1] + S(i-1, j-1);
 *                  v = val[i-1][j] + (path[i-1][j] ? gap : 0); z = val[i][j-1] + (path[i][j-1] ? gap : 0); if h >= max(v, z) then
 *                  path = true, val = h, else path = false, val = max(v, z).  Traceback from (La, Lb) while i > 0 and j > 0: if
 *                  path[i][j], align (i-1, j-1) and step diagonally; otherwise h = val[i-1][j] + (path[i-1][j] ? gap : 0),
 *                  v = val[i][j-1] + (path[i][j-1] ? gap : 0), and j-- if v >= h, else i--.  A gap costs only where it opens after a
 *                  match; end gaps are free.
 *   CA secondary structure   for i = 2 .. L-3, with d13 = |x[i-2] - x[i]|, d14 = |x[i-2] - x[i+1]|, d15 = |x[i-2] - x[i+2]|,
 *                  d24 = |x[i-1] - x[i+1]|, d25 = |x[i-1] - x[i+2]|, d35 = |x[i] - x[i+2]|: H if |d15 - 6.37|, |d14 - 5.18|,
 *                  |d25 - 5.18|, |d13 - 5.45|, |d24 - 5.45|, |d35 - 5.45| are all < 2.1; else E if |d15 - 13|, |d14 - 10.4|,
 *                  |d25 - 10.4|, |d13 - 6.1|, |d24 - 6.1|, |d35 - 6.1| are all < 1.42; else T if d15 < 8; else C.  The two residues
 *                  at each end are C.  E(i, j) = 1 if the classes of a_i and b_j are equal, else 0.
 *
 * Four initial alignments (candidate classes):
 *   0 gapless      the offsets k, ascending, with a_i <-> b_{i+k} and an overlap >= m = min(Lmin, max(Lmin / 2, 5)) (integer
 *                  division); the one of the greatest quick wins, the lowest k on ties; its (R0, t0) is kept.
 *   1 secondary structure                   DP(E, -1).
 *   2 secondary structure + superposition   DP(1 / (1 + d2 / d0^2) under (R0, t0) + 0.5 E, -1).
 *   3 fragments    f = min(20, Lmin / 3); the class is empty if f < 4.  Starts in a: 0, ja, 2 ja, ... <= La - f with
 *                  ja = max(f, ceil((La - f + 1) / 8)); in b likewise.  For each (sa, sb) in row-major order: superpose the two
 *                  fragments, DP(1 / (1 + d2 / (d0 + 1.5)^2), 0); the alignment of the greatest quick wins, the lowest unit on ties.
 * Refinement of each candidate map0 (skipped below 3 pairs): best = (s, R, t, map0) from search(map0, Lmin, d0, search_step).  For
 * gap in (-0.6, 0): (R, t) = best's, prev = map0, s_old = none; up to max_dp times: new = DP(1 / (1 + d2 / d0^2) under (R, t), gap);
 * stop if new == prev; prev = new; stop if new has fewer than 3 pairs; (s, R, t) = search(new, Lmin, d0, search_step); if
 * s > best.s, best = (s, R, t, new); stop if s_old exists and |s - s_old| < 1e-6; s_old = s.
 * Final: the candidate of the greatest best.s (the lowest class on ties); under its (R, t) the pairs with d > d8 are dropped
 * (d2 <= d8^2 stays); then search(pairs, La, d0(La), 1) and search(pairs, Lb, d0(Lb), 1) on the rest.
 *
 * out[p][0..16) =
 *   0 La   1 Lb
 *   2 num_aligned   pairs after the d8 filter
 *   3 tm_norm_a     4 tm_norm_b (the reference's column when b is the ground truth)
 *   5 rmsd          of the kept pairs under slot 4's superposition
 *   6 d0_a = d0(La)   7 d0_b = d0(Lb)
 *   8 best_class
 *   9 num_dp        DPs run in refinement over all classes (an exact integer; the cost unit of a pair)
 *   10 num_units    gapless offsets + fragment pairs
 *   11 search_tm    best.s
 *   12..15          0
 * map [P,Na] int32: for each ORIGINAL position of a the original position in b, or -1; every element is written.  transform
 * (optional) [P][12]: slot 4's superposition, R row-major then t.  Lmin == 0 and 1 <= Lmin <= 4: no alignment is attempted -- NaN in
 * slots 3, 4, 5, 11, best_class -1, num_dp and num_units 0, map all -1.  A candidate whose score is not finite (a non-finite
 * coordinate among the counting positions) can never win, as in fd_tm_search; if no class has a candidate the pair is written like
 * a short one.
 *
 * Three launches (seed: grid P * parts, the gapless offsets and fragment pairs dealt to waves round-robin; refine: P * 4, one block
 * per class; final: P), no host synchronisation, no floating-point atomics, every reduction in a fixed order: results are bitwise
 * reproducible and bitwise independent of parts and of what else is in the batch.  ws: FD_TM_ALIGN_WS_BYTES(P, parts, Na, Nb) bytes,
 * 8-byte aligned, need not be initialised.  Refused before any launch: Na or Nb above the limit, search_step < 1, max_dp < 0,
 * parts < 1, ia without ib (or the reverse), and -- unless P == 0, Na == 0 or Nb == 0, which return FD_OK without a launch -- a
 * null ws, out or map.
 *
 * Simplifications against the TM-align program: no smoothing of the secondary-structure string; no d8 cut inside the search-phase
 * score; no fragment-threading class (get_initial_fgt); the fragment class runs on at most 8 x 8 starts; no sequence identity, no
 * circular permutation, no fast mode. */
#define FD_TM_ALIGN_MAX_N 1024
#define FD_TM_ALIGN_WS_BYTES(P, parts, Na, Nb)                                                                       \
  ((long)(P) * (long)(parts) * 4L * 32L * 8L + (long)(P) * 4L * 16L * 8L +                                           \
   (long)(P) * (long)(parts) * 4L * (long)(Na) * (((long)(Nb) + 31L) / 32L) * 8L + (long)(P) * 4L * 2L * (long)(Na) * 2L)
int fd_tm_align(const float* A, long a_stride, int Na, const float* B, long b_stride, int Nb, const int* ia, const int* ib,
                const float* mask_a, const float* mask_b, int P, int search_step, int max_dp, int parts, void* ws, double* out,
                int* map, double* transform, void* stream);

/* ---- secondary structure and the shape columns (se3_diffusion_amd/csrc/fd_dssp.hip) ----
 * Kabsch & Sander (1983) in the order the DSSP program applies it, and the reference's SHAPE_METRICS (analysis/metrics.py:37-42:
 * coil_percent, helix_percent, strand_percent, radius_of_gyration; non_coil_percent from calc_mdtraj_metrics, :58-69), which the
 * reference takes from md.compute_dssp(simplified=True) and md.compute_rg on a PDB file it writes per sample.  Two launches, one
 * per entry point; operands as fd_backbone_metrics (residue r of backbone b at atoms + (b N + r) atom_stride floats, N, CA, C, CB,
 * O in slots 0..4, read in place; present iff res_mask[b,r] != 0; B == 0 or N == 0 returns FD_OK without a launch and writes
 * nothing).  N <= FD_DSSP_MAX_N = 2048: the H-bond kernel keeps C, O and CA of a whole chain in LDS (nine fp32 arrays, 72 KB, and
 * 8 KB of index maps: 80 KB of the 160 KB of a CU); 4096 would need 160 KB and does not fit.  The assignment kernel needs 43 KB.
 * NOT verified: no DSSP program and no mdtraj is available to this project, so agreement with the letters md.compute_dssp prints
 * has never been checked; the tests check a float64 restatement of the text below and its plausibility against the HELIX / SHEET
 * records of six deposited structures.  Two deliberate differences from the DSSP program: the energy is NOT rounded to three
 * decimals, and the two gaps of a bulge must be non-negative (the program's own comparison is remembered as accepting negative
 * gaps; that form glued the strands of a meander into one stretch).
 *
 * All decisions are made in fp64 from the fp32 coordinates.
 *   residues      the present residues, compacted in index order; every index below is a compacted index, 0 .. n-1.
 *   chain break   between a and a+1 iff their original indices are not adjacent or |C(a) - N(a+1)| > 2.5 A.  nobreak(a, b): both
 *                 in 0 .. n-1, a <= b, and no break anywhere in a .. b.
 *   amide H       H(i) = N(i) + (C(i-1) - O(i-1)) / |C(i-1) - O(i-1)|.  i is a donor only if i > 0, there is no break before i and
 *                 no_donor[b,i] (optional, [B,N], by original index: prolines) is zero.
 *   energy        of donor i and acceptor j != i, j != i-1, with |CA(i) - CA(j)| < 9 A:
 *                 E = 27.888 (1/d(N,O) + 1/d(H,C) - 1/d(H,O) - 1/d(N,C)) kcal/mol, N and H of i, C and O of j;
 *                 E = -9.9 if any of the four distances is below 0.5 A, and E is clamped below at -9.9.  No rounding.
 *   acceptors     every donor keeps its two lowest energies and their acceptors; equal energies go to the lower index.
 *                 hb(a, b): b is one of a's two kept acceptors and its E < -0.5.  Nothing else of the energies is used below.
 *   turns         turn_n(i), n = 3, 4, 5: hb(i+n, i) and nobreak(i, i+n).
 *   bridges       for i >= 1, j >= i+3, j <= n-2, nobreak(i-1, i+1) and nobreak(j-1, j+1): parallel if (hb(i+1, j) and hb(j, i-1))
 *                 or (hb(j+1, i) and hb(i, j-1)); otherwise antiparallel if (hb(i+1, j-1) and hb(j+1, i-1)) or (hb(j, i) and
 *                 hb(i, j)).
 *   ladders       maximal runs of bridges of one type: (i, j), (i+1, j+1), ... parallel; (i, j), (i+1, j-1), ... antiparallel.
 *                 (The conditions of a bridge keep a run from crossing a break.)
 *   bulges        two ladders of one type, the first the one whose i-strand starts lower; a strand's start and end are its lowest
 *                 and highest residue.  gi = residues between them on the i-strand = second's i-start - first's i-end - 1; gj =
 *                 residues between them on the j-strand = second's j-start - first's j-end - 1 (parallel), first's j-start -
 *                 second's j-end - 1 (antiparallel: the second ladder's j-strand lies below the first's).  Linked iff gi >= 0,
 *                 gj >= 0, no break in either gap, and (gi <= 1 and gj <= 4) or (gi <= 4 and gj <= 1).  Linking is transitive.
 *   sheets        on each of the two strands of a group of linked ladders every residue from the strand's lowest to its highest
 *                 gets E if the group holds more than one bridge, else B.  E overrides B.
 *   helices       after the sheets: H on i .. i+3 wherever turn_4(i-1) and turn_4(i), over anything; then G on i .. i+2 wherever
 *                 turn_3(i-1) and turn_3(i) and all three are blank or G; then I on i .. i+4 wherever turn_5(i-1) and turn_5(i)
 *                 and all five are blank or I.
 *   T             blank residues i with turn_n(k) for some n and some i-n < k < i.
 *   S             remaining blank residues i with nobreak(i-2, i+2) whose angle between CA(i) - CA(i-2) and CA(i+2) - CA(i) is
 *                 above 70 degrees.
 *   classes       H, G, I -> helix; E, B -> strand; everything else coil (mdtraj's simplified=True).
 *
 * fd_dssp_hbonds(..): acc_idx [B,N,2] int32, the ORIGINAL residue indices of the two kept acceptors of the donor at original
 * index r, lowest energy first (-1: none -- not present, not a donor, or fewer candidates); acc_e [B,N,2] fp64 their energies
 * (0 where acc_idx is -1).  Every element is written. */
#define FD_DSSP_MAX_N 2048
int fd_dssp_hbonds(const float* atoms, long atom_stride, const float* res_mask, const float* no_donor, int B, int N, int* acc_idx,
                   double* acc_e, void* stream);

/* The assignment from fd_dssp_hbonds' table, one block per backbone.  natoms: atoms per residue (37 or 5; 3 natoms <= atom_stride),
 * for the radius of gyration.  ss [B,N] int8, by original index:
 *   -1 absent, 0 blank, 1 H, 2 B, 3 E, 4 G, 5 I, 6 T, 7 S
 * out[b][0..8) =
 *   0 num_res             n
 *   1 helix_percent       residues of class helix / n
 *   2 strand_percent      residues of class strand / n
 *   3 coil_percent        the rest / n
 *   4 non_coil_percent    slot 1 + slot 2
 *   5 radius_of_gyration  sqrt(mean |x - mean x|^2) over all atoms of the present residues whose three coordinates are not all
 *                         zero, in nm (Angstrom / 10): mdtraj's unit-mass compute_rg on the PDB the reference would have written
 *   6 num_hbonds          kept acceptors with E < -0.5
 *   7 overflow            1.0 iff the chain has more than 2048 ladders and some were dropped (never silently), else 0
 * n == 0 gives NaN in slots 1..5.  Chains too short for any structure (n < 6) give blank, T and S letters, not an error. */
int fd_dssp_assign(const float* atoms, long atom_stride, int natoms, const float* res_mask, const int* acc_idx, const double* acc_e,
                   int B, int N, signed char* ss, double* out, void* stream);

/* ---- bond, angle and clash violation losses (se3_diffusion_amd/csrc/fd_violations.hip) ----
 * The INTER_VIOLATION_METRICS of the reference's metrics.csv (analysis/metrics.py:13-42: bonds_c_n_loss_mean,
 * angles_ca_c_n_loss_mean, clashes_mean_loss) and what comes with them, which the reference computes per sample on the host:
 * amber_minimize.find_violations (openfold/np/relax/amber_minimize.py:354-390) builds atom14 arrays of a full-atom Protein and
 * calls openfold/utils/loss.py::find_structural_violations (:1105-1215) with violation_tolerance_factor 12 and
 * clash_overlap_tolerance 1.5 (amber_minimize.py:377-382), then compute_violation_metrics (:1272-1312).  Here: the same arithmetic
 * for an ALL-ALANINE chain -- the atoms a backbone sampler has: N, CA, C, CB, O -- so there is no proline branch and no disulfide
 * branch.  Operands as fd_backbone_metrics (residue r of backbone b at atoms + (b N + r) atom_stride floats, N, CA, C, CB, O in
 * slots 0..4, read in place; present iff res_mask[b,r] != 0; B == 0 or N == 0 returns FD_OK without a launch and writes nothing).
 * res_index (optional) [B,N] int32: the residue numbers; NULL means the position in the padded chain.  N <= FD_VIOLATIONS_MAX_N =
 * 2048: every block keeps the five atoms of a whole chain in LDS (fifteen fp32 arrays, 120 KB, and 20 KB of radii and index maps).
 *
 * All decisions are made in fp64 from the fp32 coordinates.
 *   residues      the present residues, compacted in index order: 0 .. n-1, residue k with number idx(k) = res_index of it.
 *   connections   (between_residue_bond_loss, loss.py:712-868) between k and k+1, for k = 0 .. n-2, with eps = 1e-6 INSIDE every
 *                 square root as the reference has it: l_cn = sqrt(eps + |C(k) - N(k+1)|^2), l_cac = sqrt(eps + |CA(k) - C(k)|^2),
 *                 l_nca = sqrt(eps + |N(k+1) - CA(k+1)|^2); cos1 = (CA(k) - C(k)) / l_cac . (N(k+1) - C(k)) / l_cn;
 *                 cos2 = -(N(k+1) - C(k)) / l_cn . (CA(k+1) - N(k+1)) / l_nca.
 *                   e0 = sqrt(eps + (l_cn - 1.329)^2)    tolerance t0 = 12 * 0.014
 *                   e1 = sqrt(eps + (cos1 + 0.4473)^2)   tolerance t0 AGAIN: the reference takes the C-N length's standard
 *                        deviation here (loss.py:807), not the cosine's own 0.0311.  A quirk of the reference, kept.
 *                   e2 = sqrt(eps + (cos2 + 0.5203)^2)   tolerance t2 = 12 * 0.0353
 *                 loss_x = relu(e_x - t_x).  bonded(k) = idx(k+1) - idx(k) == 1.  The three means are
 *                 sum over bonded k of loss_x / (number of bonded k + eps).  violated(k) = bonded(k) and some e_x > t_x.
 *                 connections_per_residue_loss_sum(k) = 0.5 ((loss_0 + loss_1 + loss_2)(k) + (the same)(k-1)), a missing neighbour
 *                 giving 0 -- over ALL consecutive present residues, bonded or not: the reference does not mask this sum
 *                 (loss.py:841-847).  connections_per_residue_violation_mask(k) = violated(k) or violated(k-1).
 *   clashes       (between_residue_clash_loss, loss.py:871-1015) all pairs of an atom a of residue i and an atom c of residue j
 *                 with idx(i) < idx(j), except the pair (C of i, N of j) where idx(j) == idx(i) + 1 (:935-959).  Radii: N 1.55;
 *                 CA, C, CB 1.7; O 1.52.  dist = sqrt(1e-10 + d^2), bound = r_a + r_c - 1.5, loss = relu(bound - dist), a clash
 *                 iff dist < bound.  clashes_mean_loss = sum of loss / (1e-6 + number of counted pairs).
 *                 clashes_per_atom_loss_sum(i, a): the losses of all counted pairs the atom is in, as first or as second member
 *                 (both triangles, :994-996); clashes_per_atom_clash_mask(i, a): it is in a clash.
 *   fractions     (compute_violation_metrics, loss.py:1272-1312, with tensor_utils.masked_mean's eps = 1e-4 and seq_mask = 1 on
 *                 the present residues) extreme CA-CA: bonded k with sqrt(1e-6 + |CA(k) - CA(k+1)|^2) - 3.80209737096 > 1.5, over
 *                 (1e-4 + number of bonded k); the others: residues with the mask set / (1e-4 + n).
 *
 * out[b][0..FD_VIOLATION_SLOTS) =
 *   0 num_res                            n
 *   1 bonds_c_n_loss_mean                2 angles_ca_c_n_loss_mean         3 angles_c_n_ca_loss_mean
 *   4 clashes_mean_loss
 *   5 violations_extreme_ca_ca_distance
 *   6 violations_between_residue_bond    residues with connections_per_residue_violation_mask
 *   7 violations_between_residue_clash   residues with an atom in a clash
 *   8 violations_per_residue             residues with either.  NOT the reference's value when a residue is distorted within
 *                                        itself: see the second difference below.
 *   9 num_residue_violations             the count behind slot 8 (the reference: the sum of total_per_residue_violations_mask)
 *   10 num_bonds                         bonded k
 *   11 num_atom_pairs                    counted atom pairs
 *   12 num_clashing_pairs                counted atom pairs that clash
 *   13..15                               0
 * n == 0 (and n == 1) give counts 0 and the means the formulas give with their eps: 0.
 * Optional arrays, by ORIGINAL residue index, every element written, zeros at absent residues; NULL skips one:
 *   res_loss [B,N] fp64     connections_per_residue_loss_sum
 *   atom_loss [B,N,5] fp64  clashes_per_atom_loss_sum, atoms in the order N, CA, C, CB, O
 *   flags [B,N] uint8       bit a (0..4): clashes_per_atom_clash_mask of atom a; bit 5: connections_per_residue_violation_mask
 *
 * Two deliberate differences from the reference:
 *   absent residues   a residue with res_mask == 0 takes no part, and the bond across it is a gap.  The reference leaves such a
 *                 residue at the origin with atom14_atom_exists = 1 -- atom14 existence follows the residue type, not the atom
 *                 mask -- so that every masked residue clashes with every other masked one.  What agrees with the reference is the
 *                 run on the compacted chain with residue_index carrying the original positions.
 *   within-residue term   within_residue_violations (loss.py:1018-1102) is left out: the sampler builds N, CA, C, CB and O of a
 *                 residue from ideal geometry, so the term is zero by construction for its output.  violations_per_residue and
 *                 num_residue_violations are therefore the maximum of the connection mask and the clash mask only, and
 *                 violations_within_residue is not reported.
 *
 * Two launches (a grid of ceil(N / FD_VIOLATIONS_TILE) B blocks, then one thread per backbone), no host synchronisation, no
 * floating-point atomics, every sum in a fixed order that depends only on the compacted chain: results are bitwise reproducible and
 * bitwise independent of B, of the backbone's place in the batch and of absent residues behind it.  ws: FD_VIOLATIONS_WS_DOUBLES(B, N)
 * doubles, need not be initialised.  Refused before any launch: N above the limit, atom_stride < 15, a null atoms, res_mask, ws or
 * out, a misaligned operand. */
#define FD_VIOLATION_SLOTS 16
#define FD_VIOLATIONS_MAX_N 2048
#define FD_VIOLATIONS_TILE 64
#define FD_VIOLATIONS_WS_DOUBLES(B, N) ((long)(B) * (((long)(N) + FD_VIOLATIONS_TILE - 1L) / FD_VIOLATIONS_TILE) * 16L)
int fd_violations(const float* atoms, long atom_stride, const float* res_mask, const int* res_index, int B, int N, double* ws,
                  double* out, double* res_loss, double* atom_loss, unsigned char* flags, void* stream);

/* ---- clustering of a sampled set: linkage, flat cut, diversity (se3_diffusion_amd/csrc/fd_cluster.hip) ----
 * The diversity of a FrameDiff sampling run is the number of clusters divided by the number of samples, from hierarchical
 * clustering of the pairwise TM-scores at 0.5; the paper takes it from the MaxCluster program with average linkage.  Here: the
 * agglomerative clustering of G similarity or distance matrices where they lie in HBM, one thread block per matrix, and the cut of
 * the tree into flat clusters with a representative each.  NOT verified: the reference repository holds no clustering code, and
 * MaxCluster exists on no machine this project is built on, so agreement with the clusters or centroids MaxCluster prints has never
 * been checked; the tests check a float64 restatement of the text below and a recorded run of scipy.cluster.hierarchy (an
 * independent implementation: a minimum spanning tree for single linkage, nearest-neighbour chains for the other two) on matrices
 * without ties.  The inclusive cut and the tie rule are this project's own choices; scipy defines neither.
 *
 * mat: problem g is the fp64 matrix at mat + g problem_stride, row i at + i ld doubles (ld >= M), read in place.  Only the strict
 * upper triangle (i < j) of the present samples is read; the diagonal, the lower triangle and the rows and columns of absent
 * samples may hold anything.  present (optional) [G,M] uint8: sample i of problem g takes part iff it is non-zero; NULL: all do.
 * kind 0: the entries are distances; kind 1: similarities, and the distance is 1.0 - s, taken in fp64 when the entry is first
 * read.  A NaN distance is read as +inf.  method 0 single, 1 average (UPGMA), 2 complete.
 *
 * fd_cluster_linkage(..): with n present samples, the leaves are the present samples, leaf i having id i (its ORIGINAL position),
 * size 1.  For s = 0 .. n-2:
 *   1. among the pairs of active clusters take the one with the smallest key (d, smaller id, larger id), compared in that order;
 *      x is its cluster of the smaller id, y the other;
 *   2. Z[g][s] = (id x, id y, d(x, y), size x + size y); x and y leave, and the cluster of id M + s and that size becomes active;
 *   3. its distance to every other active cluster k (Lance-Williams), n_x = size x, n_y = size y:
 *        single    d(x, k) < d(y, k) ? d(x, k) : d(y, k)      -- written so that it is min(d(x, k), d(y, k))
 *        complete  the larger of the two
 *        average   (n_x d(x, k) + n_y d(y, k)) / (n_x + n_y), each product rounded, then the sum, then the quotient
 * The three methods are monotone: up to the rounding of the average the heights Z[..][2] never decrease.  Z [G, M-1, 4] fp64;
 * rows n-1 .. M-2 (all rows if n <= 1) are filled with (-1, -1, +inf, 0); num_merges[g] (int32) = max(n - 1, 0).  Because the ids
 * of the leaves are original positions and M + s is above them all, a problem with absent samples gives bit for bit what the
 * compacted problem gives, with leaf c of the compacted problem read as the c-th present sample and n' + s as M + s.
 * ws: FD_CLUSTER_WS_DOUBLES(M) doubles per problem, G of them, 8-byte aligned, need not be initialised: the working matrix (at the
 * sizes that matter it stays in L2).  On return the first double of a problem's workspace holds the number of cache rows the
 * problem rescanned (a cost figure for tools/measure_cluster_cost.py, nothing else may be read from ws).
 * M <= FD_CLUSTER_MAX_M = 4096: the per-row caches in LDS (best partner's distance and slot, cluster size, id, alive flag) take 84 KB
 * there, the list of rows to rescan 8 KB more, and the workspace of one problem 128 MB.
 *
 * fd_cluster_cut(..): the flat clusters at height cut, from Z and num_merges as fd_cluster_linkage wrote them and the same mat, ld,
 * problem_stride, present, M and kind.  The written merges with height <= cut are replayed (INCLUSIVE: for similarities the
 * caller passes cut = 1 - threshold, so that "similarity >= threshold" merges); a cluster is what they join.
 *   labels [G,M] int32   the cluster of every sample; the clusters are numbered 0 .. K-1 in ascending order of their smallest
 *                        member; -1 for an absent sample.
 *   rep [G,M] int32      rep[g][k], k < K: the medoid of cluster k -- the member whose sum of ORIGINAL entries mat[min(i, j)][max(i, j)]
 *                        against the other members j, added in ascending j, is the largest (kind 1) or the smallest (kind 0);
 *                        equal sums go to the smallest index; a singleton is its own medoid.  -1 for k >= K.
 *   out[g][0..FD_CLUSTER_SLOTS) =
 *     0 num_samples           n
 *     1 num_clusters          K
 *     2 diversity             K / n; NaN if n == 0 (a mean over nothing is NaN, as in fd_backbone_metrics)
 *     3 largest_cluster       members of the largest cluster (0 if n == 0)
 *     4 num_singletons
 *     5 mean_within_cluster   the mean original entry over the pairs i < j of one cluster: for every sample i the entries against
 *                             the members j > i of its cluster added in ascending j, those sums added in ascending i, divided by
 *                             the number of such pairs; NaN if there is none
 *     6 last_height_below_cut   the largest written height <= cut; NaN if none
 *     7 first_height_above_cut  the smallest written height > cut; NaN if none -- the two say how close the cut came to a merge
 * Both: G == 0 or M == 0 returns FD_OK without a launch and writes nothing.  One launch each, one block per problem, no host
 * synchronisation, no communication between blocks, no floating-point atomics, every sum in a fixed order: results are bitwise
 * reproducible and bitwise independent of G and of the problem's place in the batch.  Refused before any launch: M above the limit,
 * an unknown kind or method, a NaN cut, ld < M, a null or misaligned operand. */
#define FD_CLUSTER_MAX_M 4096
#define FD_CLUSTER_SLOTS 8
#define FD_CLUSTER_WS_DOUBLES(M) ((long)(M) * (long)(M))
int fd_cluster_linkage(const double* mat, long ld, long problem_stride, const unsigned char* present, int G, int M, int kind,
                       int method, double* ws, double* Z, int* num_merges, void* stream);
int fd_cluster_cut(const double* Z, const int* num_merges, const double* mat, long ld, long problem_stride,
                   const unsigned char* present, int G, int M, int kind, double cut, int* labels, int* rep, double* out, void* stream);

/* ---- chain store: training batches from backbone atoms (se3_diffusion_amd/csrc/fd_chains.hip) ----
 * What the reference's PdbDataset does per example on the host before it noises it (data/pdb_data_loader.py:133-276:
 * du.parse_chain_feats, data/utils.py:436-445; the modeled_idx trim, :137-143; the backbone group of atom37_to_frames,
 * openfold/data/data_transforms.py:755-891, read as Rigid.from_tensor_4x4(rigidgroups_gt_frames)[:, 0], pdb_data_loader.py:240-241;
 * slots 0..2 of atom37_to_torsion_angles, data_transforms.py:922-1083; seq_idx, :156-168; du.pad_feats), for the entries of one
 * batch in one launch, from a store of single chains packed once.  The training step reads rigids_0, psi, res_mask and seq_idx of
 * this (model/score_network.py:201, experiments/train_se3_diffusion.py:561,611-615) and the ground-truth atoms, which the reference
 * recomputes from rigids_0 and psi (compute_backbone); side chains, aatype, the atom14 arrays and chain_idx are not produced.
 * NOT du.rigid_frames_from_all_atom (Rigid.from_3_points(N, CA, C)): that is another frame.
 *
 * The store (device, contiguous):
 *   atoms [T,4,3] fp32       N, CA, C, O of all chains, one after the other
 *   atom_mask [T,4] uint8    non-zero: the atom is present.  The coordinates of an absent atom may hold anything.
 *   res_index [T] int32      residue numbers
 *   offsets [C+1] int64      chain c is the residues offsets[c] .. offsets[c+1]-1; ascending, chains below 2^31 residues
 * A residue is PRESENT when N, CA and C are all present.
 *
 * fd_chain_windows(..): window [C,3] int32 = {first present residue, last present residue, number present} of every chain, as
 * positions within the chain; a chain without a present residue gets {0, -1, 0}.  [first, last] is the reference's modeled_idx
 * trim; last - first + 1 is its modeled_seq_len.  One block per chain, integer min / max / sum only.  atoms is not read.
 *
 * fd_chain_batch(..): entry b of the batch is chain ids[b] (ids [B] int32 on the device; repeats allowed).  Rows 0 .. last - first
 * of an entry are the residues first .. last of its chain (the WINDOW); the rows behind them are padding.  The caller checks, from
 * the window table it read back once, that 0 <= ids[b] < C and that no window is longer than Npad, and refuses the call otherwise:
 * the entry point cannot read device memory.  (The kernel never reads or writes past a buffer whatever the tables hold: a longer
 * window is cut at Npad, a negative id or an inconsistent window gives an entry of padding.)  All arithmetic after the fp32 loads
 * is fp64, rounded to fp32 once, where a value is stored.  Sums run left to right, ((a + b) + c) + d.
 *   centre     c = S / (n + 1e-5), S = the sum of the present CA atoms of the window, n their number (utils.py:439-441).  Thread t
 *              of 256 adds the rows t, t + 256, ... in that order; the 64 partials of a wave are combined by the butterfly
 *              v += v[lane ^ o], o = 32, 16, 8, 4, 2, 1; the four wave sums as (s0 + s1) + (s2 + s3).  n is an integer sum.
 *   atoms      every atom of the window becomes p - c if it is present and the origin if it is not (utils.py:441-443); the residue
 *              before row 0 is all origin (data_transforms.py:957-965 after the trim).
 *   gs(p, q, r)  e0 = (q - p) / sqrt(|q - p|^2 + 1e-8); v = r - q; e1' = v - e0 (e0 . v); e1 = e1' / sqrt(|e1'|^2 + 1e-8);
 *              e2 = e0 x e1  (rigid_utils.py:1233-1275 from_3_points(p_neg_x_axis = p, origin = q, p_xy_plane = r))
 *   frame      of a present residue: (x, y, z) = gs(CA, C, N), i.e. x = unit(C - CA), y = unit((N - CA) - x (x . (N - CA))),
 *              z = x x y; the rotation has the columns x, y, z and the translation is CA.  (The reference builds
 *              from_3_points(C, CA, N) and composes diag(-1, 1, -1): the same matrix.)
 *   quaternion t0 = 1 + R00 + R11 + R22, t1 = 1 + R00 - R11 - R22, t2 = 1 - R00 + R11 - R22, t3 = 1 - R00 - R11 + R22; the largest
 *              decides (the first on ties):
 *                t0: (t0, R21 - R12, R02 - R20, R10 - R01)      t1: (R21 - R12, t1, R01 + R10, R02 + R20)
 *                t2: (R02 - R20, R01 + R10, t2, R12 + R21)      t3: (R10 - R01, R02 + R20, R12 + R21, t3)
 *              divided by its norm sqrt(w^2 + x^2 + y^2 + z^2), and negated if w < 0.  No eigen-solve.
 *   torsions   of the atoms (a, b, c, d): (e0, e1, e2) = gs(b, c, a); w = d - c; ry = e1 . w, rz = e2 . w;
 *              (sin, cos) = (rz, ry) / sqrt(rz^2 + ry^2 + 1e-8).  Slot 0 pre-omega (CA-1, C-1, N, CA), slot 1 phi (C-1, N, CA, C),
 *              slot 2 psi (N, CA, C, O) with both entries negated (data_transforms.py:1063-1065); slots 3..6 zero.  Every row of the
 *              window has them, from the masked atoms, as the reference has.
 *   outputs    rigids_0 [B,Npad,7] = (w, x, y, z, CA) of a present residue and (1, 0, 0, 0, 0, 0, 0) of every other row;
 *              torsions [B,Npad,7,2], zero in the padding; res_mask [B,Npad] = 1 where the residue is present, else 0;
 *              seq_idx [B,Npad] int64 = res_index - (the smallest res_index of the window) + 1 (pdb_data_loader.py:167-168 for one
 *              chain), 0 in the padding; gt_bb [B,Npad,5,3] (optional) = N, CA, C, CB, O of fd_backbone_atoms on the rows of
 *              rigids_0 and the psi written here, bit for bit (the same device code), so the loss needs no launch of its own.
 *              head_const: the constants of fd_backbone_atoms; may be NULL without gt_bb.  Every element is written.
 * Three deliberate differences from the reference:
 *   res_mask         the reference's res_mask is the CA mask alone (utils.py:438), which leaves the degenerate frame of a residue
 *                    without N or C switched on.  Here a residue counts when N, CA and C are present.
 *   absent rows      the reference's rigids_0 of an absent residue is an arbitrary eigenvector of a zero matrix
 *                    (Rotation.get_quats -> rot_to_quat's eigh), and zeros in the padding.  Here both are the identity frame at
 *                    the origin behind res_mask = 0.
 *   quaternion sign  the reference's sign is whatever eigh returns.  Here w >= 0.
 * One block of 256 threads per entry, no host synchronisation, no floating-point atomics: results are bitwise reproducible and
 * bitwise independent of B, of the entry's place in the batch, of Npad and of the residues outside the window.  B == 0 or
 * Npad == 0 (C == 0 for the windows) returns FD_OK without a launch.  Refused before any launch: a negative size, a null or
 * misaligned operand, gt_bb without head_const. */
int fd_chain_windows(const float* atoms, const unsigned char* atom_mask, const long* offsets, int C, int* window, void* stream);
int fd_chain_batch(const float* atoms, const unsigned char* atom_mask, const int* res_index, const long* offsets, const int* window,
                   const int* ids, int B, int Npad, const FdHeadConst* head_const, float* rigids_0, float* torsions,
                   float* res_mask, long* seq_idx, float* gt_bb, void* stream);

/* ---- sequence design: ProteinMPNN inference (se3_diffusion_amd/csrc/fd_design.hip) ----
 * The reference's vanilla (full-backbone) ProteinMPNN (ProteinMPNN/protein_mpnn_utils.py: ProteinFeatures :899-994, EncLayer
 * :602-647, DecLayer :650-688, ProteinMPNN.forward :1036-1079 and .sample :1083-1168) in eval mode with augment_eps = 0, for single
 * chains with every residue present (mask = 1, one chain label), hidden_dim = node_features = edge_features = 128, three encoder
 * and three decoder layers.  Not covered: ca_only, several chains, missing residues, tied_sample, PSSM inputs, bias_by_res,
 * conditional_probs / unconditional_probs, training.
 *
 * Backbones are packed, never padded:
 *   atoms [T,4,3] fp32       N, CA, C, O of all backbones, one after the other
 *   res_index [T] int32      residue numbers
 *   offsets [B+1] int64      backbone b is the rows offsets[b] .. offsets[b+1]-1; at most FD_MPNN_MAX_L rows each (the caller
 *                            checks: the entry points cannot read device memory; a kernel only looks at the first FD_MPNN_MAX_L)
 *   chain_of [T] int32       the backbone of every row
 * K = the checkpoint's k_neighbors (1 .. FD_MPNN_MAX_K); a backbone of L rows uses Ke = min(K, L) neighbours: per-row arrays keep
 * the stride K and their entries k >= Ke are -1 (E_idx), zero (h_E) or unwritten (EB).
 * Every product is an fp32 product summed in fp32 (v_mfma_f32_16x16x4_f32 for the per-edge Linears: a k-ordered fmaf chain per
 * output; fmaf chains for the Linears of one node); exp, log, erf and sqrt are the device's fp32 functions; GELU is the exact one,
 * 0.5 x (1 + erf(x / sqrt 2)); LayerNorm has eps = 1e-5 and the biased variance.  Nothing is atomic, no sum's order depends on the
 * other backbones or sequences of the call: a row is bitwise independent of B and of its backbone's place, a sequence of num_seqs.
 *
 * The Linears of one node split their inputs into 2, 4 or 8 contiguous slices, one fmaf chain per slice and output, and add the
 * slices in ascending order.
 *
 * Packed weights (fp32, device, contiguous, ew and dw 16-byte aligned; "T" = stored transposed, [in][out], so that a column of
 * outputs is contiguous):
 *   gw [FD_MPNN_GRAPH_FLOATS]: mu[16] = linspace(2, 22, 16) | pos[66][16], pos[d] = embeddings.linear.weight[:, d] + its bias |
 *     edge_embedding.weight T [416][128] | norm_edges weight, bias | W_e.weight T [128][128] | W_e.bias.
 *   NU (one node update, 148736 floats): W3 T [128][128] | b3 | norm1 weight, bias | dense.W_in T [128][512] | its bias [512] |
 *     dense.W_out T [512][128] | its bias | norm2 weight, bias.
 *   ew [FD_MPNN_ENC_FLOATS]: W1.bias of encoder layer 0 [128] | three layers of
 *     W1[:, 128:256] T | W2 T | b2 | NU | NPW [128][6 x 128] | NPB [6 x 128] | W11[:, 128:256] T | W12 T | b12 | W13 T | b13 |
 *     norm3 weight, bias.
 *     NPW / NPB give the NODE PRODUCTS of the layer's new h_V, slots of 128: 0 = W11[:, 0:128] h + b11, 1 = W11[:, 256:384] h; then,
 *     for layers 0 and 1, 2 = (next layer's W1)[:, 0:128] h + b1, 3 = (next W1)[:, 256:384] h (slots 4, 5 unused), and for layer 2
 *     2 + l = (decoder layer l's W1)[:, 384:512] h (l = 0, 1, 2), 5 = (decoder layer 0's W1)[:, 0:128] h.
 *   dw [FD_MPNN_DEC_FLOATS]: (decoder W1)[:, 128:256] T of layers 0, 1, 2 | their three b1 | three layers of
 *     W1[:, 0:128] T | W1[:, 384:512] T | TS [21][128], TS[a] = W1[:, 256:384] W_s.weight[a] | W2 T | b2 | NU ; then
 *     W_out.weight T [128][21] | W_out.bias [21].
 *
 * fd_mpnn_graph(..): per row i the Ke nearest rows of its backbone by d(i, j) = sqrt(|CA_j - CA_i|^2 + 1e-6) in fp32
 * (((dx^2 + dy^2) + dz^2) + 1e-6), ascending under the key (d, j): E_idx [T,K] int32 holds positions WITHIN the backbone, the
 * row itself first (d = 1e-3) unless another CA coincides with it.  h_E [T,K,128] = W_e(norm_edges(edge_embedding([pos ; rbf]))):
 * pos = pos[clip(res_index[i] - res_index[j] + 32, 0, 64)]; rbf = the 25 sets of 16 exp(-((D - mu) / 1.25)^2) in the reference's
 * order (:958-982), D = sqrt(|A_i - B_j|^2 + 1e-6), with the virtual CB = -0.58273431 a + 0.56802827 b - 0.54067466 c + CA,
 * b = CA - N, c = C - CA, a = b x c (:946-949).  One block per row.
 *
 * fd_mpnn_encoder(..): the three EncLayers on h_V = 0 (h_V [T,128] is written, not read), h_E in place, and what the decoder needs
 * per backbone: node [T,6,128] = the node products of layer 2 (above), EB [3,T,K,128] = (decoder layer l's W1)[:, 128:256] h_E +
 * b1.  W1 [h_i ; e_ik ; h_j] is formed as (A h_i + b1) + B e_ik + C h_j from node products; the node update is
 * norm1(h_i + (W3 (sum_k g_k) + Ke b3) / 30) with g_k the output of the second GELU, then norm2(x + dense(x)).  node_ws [T,6,128]
 * is a workspace, distinct from node.  Eight launches (one small, seven of one block per row).
 *
 * fd_mpnn_decode(..): one block per (backbone b, sequence s), grid (B, num_seqs).  Arrays over sequences are [num_seqs, T]:
 * order int32 (order[s, offsets[b] + n] = the position within b decoded n-th; a permutation, which the caller guarantees -- an
 * entry outside 0 .. L-1 is skipped), S_in int32 letters 0..20, uniforms fp32; fixed [T] uint8 (may be NULL) is per row.  At step n,
 * position t = order[n]: for each decoder layer l the first Linear of the message of edge k (neighbour j) is
 *   W1a^l h^l[t] + EB[l][t,k] + (TS^l[S[j]] + W1d^l h^l[j])   if j was decoded before t      (h^0 = the encoder's h_V)
 *   W1a^l h^l[t] + EB[l][t,k] + W1d^l h^0[j]                  otherwise (t itself included)
 * then GELU, W2, GELU, the sum over k, W3 behind the sum as in the encoder, norm1, dense, norm2.  After layer 2:
 * logits = W_out h^3[t]; log_probs[s,t] = log_softmax(logits); p = softmax((logits / temperature - 1e8 omit) + bias / temperature)
 * (omit, bias [21] fp32).  forced = 0: the letter is the first a with uniforms[s,t] < p_0 + .. + p_a (summed in that order; the
 * last a with p_a > 0 if there is none), except at rows with fixed != 0, which take S_in and report probs = 0 as the reference's
 * all_probs does; forced = 1: every letter is S_in (the reference's forward(use_input_decoding_order=True)), uniforms may be NULL.
 * Outputs: S_out [num_seqs,T] int32, log_probs and probs [num_seqs,T,21].  scratch [num_seqs,T,2,128] fp32 is block-private
 * working memory (W1d^l h^l[j], l = 1, 2, of the decoded positions).  No barrier across blocks, no atomics.
 * T == 0 (B == 0, num_seqs == 0) returns FD_OK without a launch.  Refused before any launch: a negative size, K outside
 * 1 .. FD_MPNN_MAX_K, a null or misaligned operand, temperature <= 0, node == node_ws. */
#define FD_MPNN_HIDDEN 128
#define FD_MPNN_MAX_K 64
#define FD_MPNN_MAX_L 1024
#define FD_MPNN_NODE_SLOTS 6
#define FD_MPNN_GRAPH_FLOATS 71088
#define FD_MPNN_ENC_FLOATS 991232
#define FD_MPNN_DEC_FLOATS 654357
int fd_mpnn_graph(const float* atoms, const int* res_index, const long* offsets, const int* chain_of, long T, int K,
                  const float* gw, int* E_idx, float* h_E, void* stream);
int fd_mpnn_encoder(const int* E_idx, const long* offsets, const int* chain_of, long T, int K, const float* ew, const float* dw,
                    float* h_V, float* h_E, float* node, float* node_ws, float* EB, void* stream);
int fd_mpnn_decode(const int* E_idx, const long* offsets, int B, long T, int K, int num_seqs, const float* dw, const float* h_V,
                   const float* node, const float* EB, const int* order, const int* S_in, const unsigned char* fixed,
                   const float* uniforms, const float* omit, const float* bias, float temperature, int forced, float* scratch,
                   int* S_out, float* log_probs, float* probs, void* stream);

/* ---- PDB text (se3_diffusion_amd/csrc/fd_pdb.hip) ----
 * The text the reference's analysis/utils.py write_prot_to_pdb writes (data/protein.py to_pdb per frame), byte for byte, from
 * atom37 coordinates on the device.  M models of N residues x 37 atom slots, fp32; model m is read at atoms + m model_stride
 * (floats), [N,37,3] contiguous inside a model, so a [T,B,N,37,3] record is formatted per backbone in place.  aatype [N] int32
 * (NULL: all 0 = ALA), b_factors [N,37] fp32 (NULL: 0), both shared by all models.
 *
 * An atom is PRESENT iff (|x| + |y|) + |z| > 1e-7f in fp32.  The file is lines of 80 columns and '\n'; per model
 *   MODEL     {first_model + m}
 *   ATOM  {serial:>5} {' ' + name:<4} {res3:>3} A{resnum:>4}    {x:>8.3f}{y:>8.3f}{z:>8.3f}  1.00{b:>6.2f}          {element:>2}
 *     one per present atom in (residue, slot) order: serial from 1 in each model, name = the slot's atom37 name, res3 the residue
 *     name of aatype (20 = UNK), resnum the residue's position from 0, element the name's first letter;
 *   TER   {serial:>5}      {res3:>3} A{resnum:>4}    with the next serial and the LAST residue's name and number;
 *   ENDMDL
 * and "END" without a newline behind the last model: 81 (lines_0 + .. + lines_{M-1}) + 3 bytes with lines_m = counts[m] + 3.
 * Numbers are printed from rint(x 1000) and rint(b 100) in fp64 (exact products: round-half-to-even on the exact value) with the
 * sign of the sign bit, so -0.0004f prints -0.000.
 *
 * fd_pdb_count(..): counts [M] int64 = present atoms per model; status [M] int64 = FD_PDB_STATUS_OK, or for the model's offending
 * entry of the smallest linear index ((m N + residue) 37 + slot) the word 8 index + kind:
 *   FD_PDB_NONFINITE  a coordinate of the entry is NaN or infinite (whether or not the rule above calls the atom present);
 *   FD_PDB_COORD      a coordinate of a present atom rounds to something outside -999.999 .. 9999.999;
 *   FD_PDB_BFACTOR    the b-factor of a present atom is not finite or rounds to something outside -99.99 .. 999.99;
 *   FD_PDB_SERIAL     the atom whose serial is 100000; if the model has exactly 99999 atoms, TER's serial is, and the entry is the
 *                     model's last;
 *   FD_PDB_LENGTH     N > FD_PDB_MAX_N: entry (m, FD_PDB_MAX_N, 0), the first residue number of five digits;
 *   FD_PDB_AATYPE     aatype[residue] outside 0 .. 20: entry (0, residue, 0).
 * An entry with several kinds reports the smallest.  The minimum over status[0 .. M-1] is the file's first offender.  One block
 * per model, reductions by shuffles in a fixed order, no atomics.
 *
 * fd_pdb_format(..): line_offset [M] int64 = the exclusive prefix sum of lines_m; out [out_bytes] with out_bytes = the size
 * above, 16-byte aligned.  One block per model; the serial is an ordered prefix scan of the presence flags, so two runs write
 * the same bytes.  Meant for input whose status is OK: otherwise every field still stays inside its columns (digits that do
 * not fit are dropped, an aatype outside 0 .. 20 prints UNK), and nothing is written outside [0, out_bytes): a run of
 * lines that would cross either end is left out.  M == 0 returns FD_OK without a launch (the file is then "END", which the
 * caller writes).  Refused before any launch: N < 1, N x 111 >= 2^30, a negative first_model, a null or misaligned operand. */
#define FD_PDB_MAX_N 10000
#define FD_PDB_STATUS_OK 0x7fffffffffffffffL
#define FD_PDB_NONFINITE 1
#define FD_PDB_COORD 2
#define FD_PDB_BFACTOR 3
#define FD_PDB_SERIAL 4
#define FD_PDB_LENGTH 5
#define FD_PDB_AATYPE 6
int fd_pdb_count(const float* atoms, long model_stride, const int* aatype, const float* b_factors, int M, int N, long* counts,
                 long* status, void* stream);
int fd_pdb_format(const float* atoms, long model_stride, const int* aatype, const float* b_factors, const long* line_offset, int M,
                  int N, long first_model, unsigned char* out, long out_bytes, void* stream);

/* ---- reading PDB text (se3_diffusion_amd/csrc/fd_pdb_read.hip) ----
 * The inverse of the above: atom37 arrays from the text of F PDB files that lie end to end in text [n] uint8 (16-byte aligned),
 * file f being the bytes file_offsets[f] .. file_offsets[f+1] (int64 [F+1], 0 first, n last, not decreasing; an empty file holds
 * no line).  Nothing outside text is read.
 *
 * LINES.  A line starts at the first byte of a file and behind every '\n'; it ends in front of the next '\n' or at the end of
 * its file, and a '\r' directly in front of that end is not part of it.  Its columns are its bytes, from 1; a column behind its
 * end reads as a blank; columns behind 80 are not looked at.  Lines are numbered from 0 through all files.
 * RECORDS.  Columns 1-6 decide: "ATOM  ", "HETATM", "ENDMDL" (any other line, MODEL, TER, ANISOU, REMARK among them, only
 * counts as a line).  The COORDINATE RECORDS are the ATOM lines, and the HETATM lines iff hetatm != 0; with model_all == 0 only
 * those with no ENDMDL line between the start of their file and themselves.  A model's number is the count of ENDMDL lines
 * between the start of its file and its records; MODEL lines are not read.  Of a coordinate record (PDB v3.3):
 *   13-16 atom name: with the blanks at both ends removed, one of the 37 atom37 names gives the slot; any other name (a
 *         hydrogen, a name with a blank inside) gives none -- the record still counts for its residue;
 *   18-20 resName -> aatype 0 .. 19 in the order ALA ARG ASN ASP CYS GLN GLU GLY HIS ILE LEU LYS MET PHE PRO SER THR TRP TYR VAL,
 *         20 for anything else;      22 chainID;      23-26 resSeq, a signed integer;      27 iCode;
 *   31-38, 39-46, 47-54 x, y, z;     55-60 occupancy (all blank: 1);      61-66 tempFactor (all blank: 0).
 * NUMBERS.  A field is blanks, an optional sign, digits with at most one '.' among them, blanks; at least one digit.  Its value
 * is the integer made of the digits divided by 10^(digits behind the point) in fp64, rounded once to fp32: what
 * float32(float(field)) gives.  resSeq is the same without the point.
 * RESIDUES.  The key of a coordinate record is (chainID, resSeq, iCode, HETATM or not).  A record begins a RESIDUE ROW unless
 * the coordinate record before it lies in the same file with no ENDMDL line between the two and has the same key; it begins a
 * CHAIN SEGMENT unless that record has the same chainID.  Rows and segments are numbered in the order of the text.  A chain ID
 * that comes back after another therefore begins a new segment.  A row's atoms are those of the coordinate records from its
 * first up to the next row's first, the next ENDMDL or the end of the file: the FIRST record of a slot gives the slot's
 * position and b-factor, a later one of the same slot (an alternate location, a duplicate) is dropped and counted.
 * MALFORMED.  kind FD_PDB_READ_SHORT: a coordinate record of fewer than 54 columns; FD_PDB_READ_COORD: x, y or z is blank or
 * not a number as above (an exponent, two signs, a letter); FD_PDB_READ_NUMBER: occupancy or tempFactor is neither blank nor
 * a number; FD_PDB_READ_RESSEQ: resSeq is not an integer.  A record's word is 8 (line number) + its smallest kind.
 *
 * Three launches; a thread owns FD_PDB_READ_WINDOW bytes, a block a chunk of FD_PDB_READ_CHUNK, nchunks = ceil(n / chunk); a line
 * belongs to the window of its first byte.  All [k,nchunks] arrays are int64, row after row.
 * fd_pdb_read_summary(..): summary [4,nchunks] = per chunk the lines that start in it, the ENDMDL lines among them, the position
 *   of the last ENDMDL line and of the last ATOM (hetatm: or HETATM) line among them (-1: none).
 * fd_pdb_read_count(..): carry [4,nchunks] = the same four of ALL chunks in front of each chunk (exclusive sums, running maxima,
 *   -1 where there is none).  counts [3,nchunks] = residue rows and chain segments that begin in the chunk, and the smallest
 *   word of a malformed record in it (FD_PDB_STATUS_OK: none).  file_first [2,F] int64 = per file that holds a byte the number
 *   of its first line, and the ENDMDL lines in front of it (other entries are left alone).
 * fd_pdb_read_fill(..): bases [2,nchunks] = exclusive sums of counts' first two rows; file_first as written above; T and C
 *   their totals.  Writes, for row r: aatype [T] int64 and residue_index [T] int64 (resName and resSeq of the row's first
 *   record), row_dropped [T] int32, and for every slot a record fills atom_positions [T,37,3] fp32, atom_mask [T,37] uint8 = 1
 *   and b_factors [T,37] fp32 -- other entries are left alone (the caller zeroes them); for segment c: chain_first [C] int64
 *   (its first row), chain_file, chain_model, chain_id [C] int32 (the chainID's character code).  Rows >= T and segments >= C
 *   are not written.  Meant for text whose status is OK; a malformed field otherwise reads as 0.
 * The scans are ordered and the first record of a slot wins whatever runs first: no atomics, two runs give the same bytes.
 * Refused before any launch: n < 1, n > FD_PDB_READ_MAX_BYTES, F < 1, a null or misaligned operand. */
#define FD_PDB_READ_WINDOW 16
#define FD_PDB_READ_CHUNK 4096
#define FD_PDB_READ_MAX_BYTES (1L << 40)
#define FD_PDB_READ_SHORT 1
#define FD_PDB_READ_COORD 2
#define FD_PDB_READ_NUMBER 3
#define FD_PDB_READ_RESSEQ 4
int fd_pdb_read_summary(const unsigned char* text, long n, const long* file_offsets, int F, int hetatm, long* summary, void* stream);
int fd_pdb_read_count(const unsigned char* text, long n, const long* file_offsets, int F, int hetatm, int model_all,
                      const long* carry, long* counts, long* file_first, void* stream);
int fd_pdb_read_fill(const unsigned char* text, long n, const long* file_offsets, int F, int hetatm, int model_all, const long* carry,
                     const long* bases, const long* file_first, long T, long C, float* atom_positions, unsigned char* atom_mask,
                     float* b_factors, long* aatype, long* residue_index, int* row_dropped, long* chain_first, int* chain_file,
                     int* chain_model, int* chain_id, void* stream);

/* ---- reading mmCIF text (se3_diffusion_amd/csrc/fd_cif_read.hip) ----
 * The same arrays from the _atom_site loop of F mmCIF files that lie end to end in text, given as in the section above.
 *
 * LINES are those of the section above: a line starts at the first byte of a file and behind every '\n', a '\r' directly in
 * front of its end is not part of it, lines are numbered from 0 through all files.  There is no column limit.  Blanks and tabs
 * separate tokens.
 * TEXT FIELDS.  A line whose first byte is ';' is a ';'-line.  A line lies inside a text field when the ';'-lines of its file in
 * front of it are odd in number.  Such lines and the ';'-lines themselves are not syntax, whatever they look like: they count
 * as OTHER lines below.
 * CLASSES.  Every other line is classified by its first token behind leading blanks; keywords and tag names compare without
 * regard to ASCII case.  BLANK: no token.  LOOP: the token is "loop_" (what follows it on the line is not read).  TAG: the token
 * begins with "_atom_site." (the dot included, so _atom_site_anisotrop. is none) and nothing but blanks or a '#' comment follows
 * it on the line.  OTHER: any other token that begins with '_' (an _atom_site. tag with a value behind it, the key-value form,
 * among them), with "data_" or with '#'.  VALUE: anything else.
 * THE LOOP.  A LOOP line is a HEAD when the next line of its file that is not BLANK is a TAG line.  The head's COLUMNS are the
 * TAG lines behind it up to the first line that is neither TAG nor BLANK, numbered from 0; their number is the loop's width.  A
 * VALUE line is a ROW when, of the lines of its file in front of it, the last LOOP line is a head, a TAG line lies behind that
 * head, and no OTHER line lies behind that head.  So the rows end at the first line that is neither VALUE nor BLANK; one row per
 * line; a file without a head has no row.  A second head in one file is malformed.
 * TOKENS of a row: a run of bytes that are neither blank nor tab; or, where that run begins with ' or ", the bytes behind that
 * quote up to the next occurrence of the same quote that is followed by a blank, a tab or the line's end ("O5'" is the three
 * bytes O5').  A token that begins with '#' ends the row.  A row has as many tokens as the loop has columns and at most
 * FD_CIF_MAX_LINE bytes; a longer line is not tokenised.
 * COLUMNS that are read, by the tag's name behind "_atom_site." (of two columns of one name the later one):
 *   group_PDB            "HETATM" makes a HETATM record, anything else ATOM; no such column: every row is ATOM
 *   label_atom_id        the atom name: one of the 37 atom37 names gives the slot, any other name none
 *   label_alt_id         must be there; it is not looked at (the first record of a slot wins, as above)
 *   label_comp_id        -> aatype as above
 *   auth_asym_id         the chain ID: 1 to 4 bytes, packed into an int32 with the first byte lowest, so that a one-letter ID is
 *                        its character code; "." and "?" read as a blank (32).  label_asym_id where there is no such column,
 *                        and always with ids_label != 0
 *   auth_seq_id          the residue number, a signed integer; label_seq_id where there is no such column, and always with
 *                        ids_label != 0
 *   pdbx_PDB_ins_code    the token's first byte; ".", "?" or no such column: a blank
 *   Cartn_x, Cartn_y, Cartn_z
 *   occupancy            ".", "?" or no such column: 1 (checked, not stored)
 *   B_iso_or_equiv       ".", "?" or no such column: 0
 *   pdbx_PDB_model_num   an integer; no such column: 1
 * Every other column is tokenised and skipped.  The columns may stand in any order; the order is taken per file.
 * NUMBERS.  A token that is an optional sign and digits with at most one '.' among them, at least one and at most 15 digits, no
 * exponent; the value as in the section above.
 * RECORDS.  The COORDINATE RECORDS are the rows that are not HETATM, and all rows iff hetatm != 0; a row that cannot be tokenised
 * counts as one.  With model_all == 0 only those whose model number is that of the file's first coordinate record are SELECTED.
 * RESIDUES, CHAIN SEGMENTS, SLOTS: as in the section above with the key (chain ID, residue number, insertion code, HETATM or
 * not): a selected record begins a residue row unless the coordinate record before it lies in the same file and has the same
 * model number and key; it begins a chain segment unless that record has the same chain ID and model number.  A row's atoms are
 * those of the coordinate records from its first up to the first with another key or model number, or the end of the loop's
 * rows.  A segment's model is its model number minus that of its file's first coordinate record.
 * MALFORMED.  The word is 8 (line number) + kind.  FD_CIF_READ_COLUMNS, at a head's LOOP line: one of label_atom_id,
 * label_alt_id, label_comp_id, Cartn_x, Cartn_y, Cartn_z, the chain ID's or the residue number's column is missing; more than
 * FD_CIF_MAX_COLS columns; a second head in the file.  Of a coordinate record, the smallest of: FD_CIF_READ_TOKENS (a wrong
 * number of tokens, an unclosed quote, a line longer than FD_CIF_MAX_LINE; nothing else is checked then); and, unless the model
 * number is an integer and the record is not selected: FD_CIF_READ_COORD, FD_CIF_READ_NUMBER, FD_CIF_READ_RESSEQ as in the
 * section above, FD_CIF_READ_CHAIN (a chain ID of no or more than 4 bytes), FD_CIF_READ_MODEL (not an integer).
 *
 * Six launches with the windows and chunks of the section above.  What a line is depends on the text in front of it, so the
 * values that the ordered scan carries are found in stages: each launch writes per chunk what the next needs, and the caller
 * turns it into rows of carry [8,nchunks] int64 = for each chunk, of ALL chunks in front of it (-1 where there is none):
 *   0 the lines; 1 the ';'-lines; 2 the ';'-lines in front of the last file start; 3 .. 6 the position of the last LOOP, TAG,
 *   OTHER and head line; 7 the position of the last coordinate record.
 * A launch reads the rows that the launches in front of it made complete; the others hold -1.
 * fd_cif_read_lines(..): lines [3,nchunks] = per chunk the lines that start in it, the ';'-lines among them, and the ';'-lines of
 *   the chunk in front of its last file start (-1: no file starts in it).  Carry rows 0 and 1 are exclusive sums; row 2 is the
 *   running maximum over the chunks in front of (row 1 + lines' third row) where that row is not -1.
 * fd_cif_read_marks(..): marks [4,nchunks] = the four positions among the chunk's lines or those in front (-1: none); carry
 *   rows 3 .. 6 are running maxima over the chunks in front.
 * fd_cif_read_header(..): table [F,FD_CIF_TABLE] int32 = per file with a head: for column k < FD_CIF_MAX_COLS the field it is
 *   read as in the order of the list above (0 group_PDB .. 12 pdbx_PDB_model_num; -1: skipped), then the loop's width and the
 *   model number of the file's first coordinate record; file_first [F] int64 = per file that holds a byte the number of its
 *   first line; bad [nchunks] = the smallest word of a malformed head in the chunk (FD_PDB_STATUS_OK: none).  Other entries are
 *   left alone.
 * fd_cif_read_summary(..): last [nchunks] = the position of the last coordinate record among the chunk's lines or those in
 *   front; carry row 7 is its running maximum over the chunks in front.
 * fd_cif_read_count(..): counts [3,nchunks] as fd_pdb_read_count's.
 * fd_cif_read_fill(..): bases, T, C and the outputs as fd_pdb_read_fill's; chain_id holds the packed chain ID.  Rows >= T and
 *   segments >= C are not written, entries that no record fills are left alone.
 * The scans are ordered and the first record of a slot wins whatever runs first: no atomics, two runs give the same bytes.
 * Refused before any launch: what the section above refuses. */
#define FD_CIF_MAX_COLS 64
#define FD_CIF_MAX_LINE 1024
#define FD_CIF_TABLE 66
#define FD_CIF_READ_TOKENS 1
#define FD_CIF_READ_COORD 2
#define FD_CIF_READ_NUMBER 3
#define FD_CIF_READ_RESSEQ 4
#define FD_CIF_READ_COLUMNS 5
#define FD_CIF_READ_CHAIN 6
#define FD_CIF_READ_MODEL 7
int fd_cif_read_lines(const unsigned char* text, long n, const long* file_offsets, int F, long* lines, void* stream);
int fd_cif_read_marks(const unsigned char* text, long n, const long* file_offsets, int F, const long* carry, long* marks, void* stream);
int fd_cif_read_header(const unsigned char* text, long n, const long* file_offsets, int F, int hetatm, int ids_label,
                       const long* carry, int* table, long* file_first, long* bad, void* stream);
int fd_cif_read_summary(const unsigned char* text, long n, const long* file_offsets, int F, int hetatm, const long* carry,
                        const int* table, long* last, void* stream);
int fd_cif_read_count(const unsigned char* text, long n, const long* file_offsets, int F, int hetatm, int model_all,
                      const long* carry, const int* table, long* counts, void* stream);
int fd_cif_read_fill(const unsigned char* text, long n, const long* file_offsets, int F, int hetatm, int model_all, const long* carry,
                     const int* table, const long* bases, long T, long C, float* atom_positions, unsigned char* atom_mask,
                     float* b_factors, long* aatype, long* residue_index, int* row_dropped, long* chain_first, int* chain_file,
                     int* chain_model, int* chain_id, void* stream);

/* ---- inflating gzip members (se3_diffusion_amd/csrc/fd_inflate.hip) ----
 * The text that the two sections above read, from files that may be gzip-compressed.  F input files lie end to end in in [n_in]
 * uint8, file f being the bytes in_offsets[f] .. in_offsets[f+1] (int64 [F+1]); its text goes to out [n_out] uint8 at
 * out_offsets[f] .. out_offsets[f+1] (int64 [F+1]).  kind [F] int32: 0, a plain file, is copied through (its two sizes are equal);
 * anything else, a gzip file, is inflated, and the caller has sized its place from the ISIZE word, the file's last four bytes.
 * One launch, one wave per file; out is the window, there is no other buffer.  Nothing outside a file's own two ranges is read
 * or written, whatever the file holds, and the work is bounded by the file's length: a corrupt file ends in a status.
 *
 * A GZIP FILE is ONE member (RFC 1952): the bytes 1f 8b; CM = 8; FLG, whose bits 5 .. 7 are clear; MTIME, XFL and OS, not looked
 * at; with FEXTRA two bytes XLEN and that many bytes, with FNAME and with FCOMMENT the bytes up to a zero byte, with FHCRC two
 * bytes -- all skipped, the header CRC is NOT checked; a raw DEFLATE stream (RFC 1951); CRC32 and ISIZE, four bytes each, the
 * lowest first.  The DEFLATE stream has stored, fixed-Huffman and dynamic-Huffman blocks, lengths 3 .. 258 and distances
 * 1 .. 32768 that may reach back to the file's first output byte and no further.
 * status [F] int64 = 0, or 16 (a byte position in the input file) + kind; where a file ends early the position is its length:
 *   FD_INFLATE_HEADER    not a gzip header: other magic bytes, CM != 8, a reserved FLG bit
 *   FD_INFLATE_ENDS      the file ends before the member is complete (header, stream or trailer); also offsets that leave in or out
 *   FD_INFLATE_BLOCK     block type 3, or a stored block whose LEN is not ~NLEN
 *   FD_INFLATE_CODES     a dynamic block's code lengths: more than 286 literal/length or 30 distance codes, a repeat with nothing
 *                        to repeat or past the end, a set that is over-subscribed, or incomplete -- except, as zlib has it, a
 *                        literal/length or distance set with no code at all or with a single code of one bit -- or no code for
 *                        the end of the block
 *   FD_INFLATE_SYMBOL    a code that the set does not hold, length symbol 286 or 287, distance symbol 30 or 31, or a distance
 *                        that reaches in front of the file's first output byte
 *   FD_INFLATE_SIZE      the stream gives more or fewer bytes than the file's place holds, or ISIZE is not that size mod 2^32;
 *                        a plain file whose two sizes differ
 *   FD_INFLATE_CRC       with verify != 0: the CRC32 of the output is not the trailer's (taken by the same wave, a slice per
 *                        lane, the slices joined by x^(8 bytes) mod the polynomial)
 *   FD_INFLATE_TRAILING  bytes behind the trailer: a second member, BGZF blocks, padding.  They are named, never silently cut.
 * The first of these that the member meets in the order of its bytes is reported; TRAILING, SIZE, CRC in that order at the
 * trailer.  (Bytes behind the trailer also make the file's last four bytes something other than ISIZE: where the place sized
 * from them is too small, SIZE is met first, inside the stream.)  The output of a file with a nonzero status is unspecified
 * within its place.
 * Not read: several members in one file, BGZF, the zlib (RFC 1950) and raw-deflate wrappers, other compressors.
 * F == 0 returns FD_OK without a launch.  Refused before any launch: a negative size, a null or misaligned operand. */
#define FD_INFLATE_HEADER 1
#define FD_INFLATE_ENDS 2
#define FD_INFLATE_BLOCK 3
#define FD_INFLATE_CODES 4
#define FD_INFLATE_SYMBOL 5
#define FD_INFLATE_SIZE 6
#define FD_INFLATE_CRC 7
#define FD_INFLATE_TRAILING 8
int fd_inflate(const unsigned char* in, long n_in, const long* in_offsets, int F, const int* kind, unsigned char* out, long n_out,
               const long* out_offsets, int verify, long* status, void* stream);

/* ---- sequence alignment and clustering (se3_diffusion_amd/csrc/fd_seq.hip) ----
 * Sequences are packed as the chain store packs chains: letters [T] uint8, values 0 .. 20 in the reference's restypes order
 * (ARNDCQEGHILKMFPSTWYV, 20 = X), chain c being the rows offsets[c] .. offsets[c+1] - 1 (offsets [C+1] int64, 0 first, not
 * decreasing).
 *
 * fd_seq_align(..): Gotoh's local alignment with affine gaps of every pair of the rectangle ids_a [Pa] x ids_b [Pb] (int32 chain
 * ids, repeats allowed): for entry (ia, ib), x = chain ids_a[ia] of m residues and y = chain ids_b[ib] of n.  subst [21,21] int32
 * is indexed [letter of x][letter of y] and need not be symmetric; a gap of k residues costs gap_open + k gap_extend.  The
 * optimal path's statistics travel with its score, so no traceback is stored.  A cell state is the tuple (score, matches,
 * columns, i0, j0), and THE RECURRENCE ON THESE TUPLES IS THE SPECIFICATION (i, j from 0; H outside the matrix is empty, E and F
 * outside it are absent):
 *   E(i,j), a gap that consumes y_j: E(i,j-1) with score - gap_extend, or H(i,j-1) with score - gap_open - gap_extend; the
 *           extension where the two scores tie.  The chosen tuple keeps its matches and its start and gains one column.
 *   F(i,j), a gap that consumes x_i: the same from (i-1,j).
 *   D(i,j): H(i-1,j-1) with subst[x_i][y_j] added to the score, (x_i == y_j) to the matches and one column; from an empty cell
 *           it starts at (i0, j0) = (i, j).
 *   H(i,j): the best of D, E, F by score, D before E before F on equal scores; if that score is <= 0 the cell is EMPTY: score
 *           0, no statistics.
 *   The result is the H of the largest score; on equal scores that of the smallest i, then of the smallest j.
 * out [Pa,Pb,FD_SEQ_SLOTS] int32 (16-byte aligned) = score, matches, columns, a_begin, a_end, b_begin, b_end, 0 with positions
 * from 0, inclusive (a_begin = i0, a_end = i); a score of 0 (also m == 0 or n == 0) gives 0, 0, 0, -1, -1, -1, -1, 0.  Letter
 * 20 equals itself like any other.  align(a, b) is not the transpose of align(b, a): the tie rules are not symmetric.  With
 * upper_only != 0 the entries with ids_a[ia] >= ids_b[ib] are not computed and hold -1 in all slots.  Every element of out is
 * written.  One wave per pair, the matrix in registers; integer arithmetic only, no atomics: two runs give the same words.
 * Pa == 0 or Pb == 0 returns FD_OK without a launch.  What is refused depends on what the operands hold, so the call copies
 * offsets, the ids, the table and the letters to the host first: it waits for the stream and cannot be captured into a graph.
 * Refused before any launch (FD_ERR_ARG): a negative size, a null or misaligned operand, gap_open outside 0 .. FD_SEQ_MAX_GAP,
 * gap_extend outside 1 .. FD_SEQ_MAX_GAP, a table entry outside -FD_SEQ_MAX_SCORE .. FD_SEQ_MAX_SCORE, offsets that do not start
 * at 0 or decrease, an id outside [0, C), a named chain of more than FD_SEQ_MAX_L residues, a letter above 20.  The kernel
 * clamps the letter it uses as a table index and the lengths it uses as loop bounds regardless.
 * There is no published substitution matrix in the library: the caller passes the table (se3_diffusion_amd/seqs.py holds a
 * BLOSUM62 typed from memory that was NOT compared with NCBI's file).
 *
 * fd_seq_greedy(..): length-ordered greedy clustering (CD-HIT; MMseqs2 cluster-mode 2) on a relation matrix where it lies.
 * rel [C,ld] uint8, ld >= C: i and j are related iff rel[min(i,j)][max(i,j)] != 0 -- only the strict upper triangle is read.
 * order [C] int32 is the walk order.  Walk it: a chain that is still unlabelled founds a cluster, becomes its representative
 * and takes every still-unlabelled chain related to it.  Then the clusters are numbered 0 .. K-1 by ascending smallest member:
 * labels [C] int32 = the cluster of each chain (-1 for a chain that order does not name; entries of order outside [0, C) are
 * passed over), rep [C] int32 = the founder of cluster k, -1 for k >= K; out [4] int32 = C, K, the size of the largest
 * cluster, 0.  ws [2 C] int32 is working memory.  One block; a founder's round is a row scan by all threads between two
 * barriers; the numbering is an ordered count: no atomics, two runs give the same words.  C == 0 returns FD_OK without a launch.
 * Refused before any launch: C < 0 or above FD_SEQ_GREEDY_MAX_C, ld < C, a null or misaligned operand, ws, labels and rep not
 * distinct. */
#define FD_SEQ_MAX_L 2048
#define FD_SEQ_LETTERS 21
#define FD_SEQ_SLOTS 8
#define FD_SEQ_MAX_SCORE 127
#define FD_SEQ_MAX_GAP 1023
#define FD_SEQ_GREEDY_MAX_C (1 << 30)
int fd_seq_align(const unsigned char* letters, const long* offsets, int C, const int* ids_a, int Pa, const int* ids_b, int Pb,
                 const int* subst, int gap_open, int gap_extend, int upper_only, int* out, void* stream);
int fd_seq_greedy(const unsigned char* rel, long ld, int C, const int* order, int* ws, int* labels, int* rep, int* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FD_HIP_H_ */
