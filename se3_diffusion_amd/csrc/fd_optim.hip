// fd_grad_stats / fd_adam_step_guarded: gradient health, clipping by global norm, skip-on-non-finite and the step counter
// of the optimiser, all on the device (no reference lines stand behind these: the reference tests torch.isnan(loss) on the
// host, experiments/train_se3_diffusion.py:448-454; the torch calls restated here are torch.nn.utils.clip_grad_norm_ followed
// by torch.optim.Adam.step, the latter only when every gradient element is finite).
//
// Three dependent launches on the caller's stream:
//   K1 grad_stats_kernel     one streaming pass over g: per thread an fp64 sum of squares and the max |g| over the FINITE
//                            elements and a count of the non-finite ones; shuffles within the wave, LDS across the waves,
//                            one partial triple per block with plain stores (no floating-point atomics: the clip coefficient
//                            feeds every parameter and must come out bit for bit the same run after run)
//   K2 grad_finalize_kernel  one block: thread t adds the partials t, t + 256, ... in index order, the 256 thread sums go
//                            through the same fixed shuffle / LDS tree; thread 0 then decides the step in the FdOptState
//   K3 adam_guarded_kernel   adam_step_kernel's arithmetic (fd_loss.hip) on coef * g, with lr/bc1, 1/sqrt(bc2), coef and
//                            `apply` read from the state; returns before touching p, m, v (and ema) when apply == 0
// Every order of additions is a function of (n, grid) alone, and the grid is a function of n.
#include "fd_common.h"
#include "../../include/fd_hip.h"

static_assert(sizeof(FdOptState) == FD_OPT_STATE_BYTES, "FdOptState layout");

namespace {

constexpr int OT = 256;
constexpr int OPT_MAX_BLOCKS = 4096;                    // fd_adam_step's grid cap
constexpr int WS_STRIDE = FD_OPT_WS_DOUBLES / 3;        // workspace: [sum of squares | non-finite count | max |g|][block]
static_assert(WS_STRIDE >= OPT_MAX_BLOCKS, "workspace holds one triple per block");
constexpr int FIN_PER = OPT_MAX_BLOCKS / OT;            // partials per thread of the finalize block
static_assert(FIN_PER * OT == OPT_MAX_BLOCKS, "the finalize block covers every partial");

// the three block-wide reductions of K1 and K2: butterfly within the wave, then the four wave results in wave order
__device__ __forceinline__ void block_reduce3(double& ss, double& bad, double& mx, double (*red)[OT / 64]) {
  ss = fd::wave_sum(ss);
  bad = fd::wave_sum(bad);
  mx = fd::wave_max(mx);
  const int lane = fd::lane_id(), wave = fd::wave_id();
  if (lane == 0) {
    red[0][wave] = ss;
    red[1][wave] = bad;
    red[2][wave] = mx;
  }
  __syncthreads();
  ss = red[0][0];
  bad = red[1][0];
  mx = red[2][0];
  for (int w = 1; w < OT / 64; ++w) {
    ss += red[0][w];
    bad += red[1][w];
    mx = mx > red[2][w] ? mx : red[2][w];
  }
}

__global__ __launch_bounds__(OT) void grad_stats_kernel(const float* __restrict__ g, long n4, double* __restrict__ ws) {
  __shared__ double red[3][OT / 64];
  double ss = 0.0;
  float mx = 0.f;
  int bad = 0;
#define FD_STAT1(G, c)                                                          \
  {                                                                             \
    const bool fin = (__float_as_uint(G.c) & 0x7fffffffu) < 0x7f800000u;        \
    const float a = fin ? fabsf(G.c) : 0.f;                                     \
    ss += (double)a * (double)a;                                                \
    mx = a > mx ? a : mx;                                                       \
    bad += fin ? 0 : 1;                                                         \
  }
  for (long i = (long)blockIdx.x * OT + threadIdx.x; i < n4; i += (long)gridDim.x * OT) {
    const float4 G = reinterpret_cast<const float4*>(g)[i];
    FD_STAT1(G, x) FD_STAT1(G, y) FD_STAT1(G, z) FD_STAT1(G, w)
  }
#undef FD_STAT1
  double badd = (double)bad, mxd = (double)mx;
  block_reduce3(ss, badd, mxd, red);
  if (threadIdx.x == 0) {
    ws[blockIdx.x] = ss;
    ws[WS_STRIDE + blockIdx.x] = badd;
    ws[2 * WS_STRIDE + blockIdx.x] = mxd;
  }
}

struct OptDecide {
  double b1, b2, max_norm;
  int skip_nonfinite;
};

// stats (optional): {sum of squares, non-finite count, max |g|, 0}; st (optional): the step decision
__global__ __launch_bounds__(OT) void grad_finalize_kernel(const double* __restrict__ ws, int nblk, double* __restrict__ stats,
                                                           FdOptState* __restrict__ st, OptDecide cfg) {
  __shared__ double red[3][OT / 64];
  // thread t owns the partials t, t + 256, ...: all its loads are issued before the first addition (sixteen dependent trips to
  // memory would otherwise make this one block the longest boundary of the step), then folded in index order
  double a[FIN_PER], c[FIN_PER], x[FIN_PER];
#pragma unroll
  for (int k = 0; k < FIN_PER; ++k) {
    const int b = k * OT + (int)threadIdx.x;
    const bool in = b < nblk;
    a[k] = in ? ws[b] : 0.0;
    c[k] = in ? ws[WS_STRIDE + b] : 0.0;
    x[k] = in ? ws[2 * WS_STRIDE + b] : 0.0;
  }
  double ss = 0.0, bad = 0.0, mx = 0.0;
#pragma unroll
  for (int k = 0; k < FIN_PER; ++k) {
    ss += a[k];
    bad += c[k];
    mx = x[k] > mx ? x[k] : mx;
  }
  block_reduce3(ss, bad, mx, red);
  if (threadIdx.x != 0) return;
  if (stats) {
    stats[0] = ss;
    stats[1] = bad;
    stats[2] = mx;
    stats[3] = 0.0;
  }
  if (!st) return;
  const double norm = sqrt(ss);
  const long nonfinite = (long)bad;
  const int apply = !(cfg.skip_nonfinite && nonfinite > 0);
  double coef = 1.0;
  if (apply) {
    const long step = st->step + 1;
    if (cfg.max_norm > 0.0) {
      coef = cfg.max_norm / (norm + 1e-6);          // torch.nn.utils.clip_grad_norm_'s coefficient, clamped to 1
      coef = coef < 1.0 ? coef : 1.0;
    }
    st->step = step;
    st->bc1 = (float)(1.0 - pow(cfg.b1, (double)step));
    st->rsqrt_bc2 = (float)(1.0 / sqrt(1.0 - pow(cfg.b2, (double)step)));
    st->clipped += coef < 1.0 ? 1 : 0;
  } else {
    st->skipped += 1;
  }
  st->nonfinite = nonfinite;
  st->grad_norm = norm;
  st->clip_coef = coef;
  st->max_abs = mx;
  st->coef = (float)coef;
  st->apply = apply;
}

// EMA = true (fd_adam_step_guarded_ema): E += a (P - E) on the float4 that holds the new P, a = 1 - d_t with
// d_t = warmup ? min(decay, (1 + t) / (10 + t)) : decay in fp64 from t = st->step, which K2 has advanced for this call.  A
// skipped call returns before touching ema, and t counts applied steps only.  EMA = false reads none of the last three arguments.
template <bool EMA>
__global__ __launch_bounds__(OT) void adam_guarded_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                          float* __restrict__ m, float* __restrict__ v, long n4, float lr,
                                                          float b1, float b2, float eps, const FdOptState* __restrict__ st,
                                                          float* __restrict__ ema, double decay, int warmup) {
  if (st->apply == 0) return;
  const float coef = st->coef, rsqrt_bc2 = st->rsqrt_bc2;
  const float step = lr / st->bc1;
  float a = 0.f;
  if constexpr (EMA) {
    double d = decay;
    if (warmup) {
      const double t = (double)st->step;
      const double w = (1.0 + t) / (10.0 + t);
      d = w < d ? w : d;
    }
    a = (float)(1.0 - d);
  }
  for (long i = (long)blockIdx.x * OT + threadIdx.x; i < n4; i += (long)gridDim.x * OT) {
    float4 P = reinterpret_cast<float4*>(p)[i];
    const float4 Gd = reinterpret_cast<const float4*>(g)[i];
    float4 M = reinterpret_cast<float4*>(m)[i];
    float4 V = reinterpret_cast<float4*>(v)[i];
#define FD_ADAM1(c)                                             \
  {                                                             \
    const float gc = coef * Gd.c;                               \
    M.c = b1 * M.c + (1.f - b1) * gc;                           \
    V.c = b2 * V.c + (1.f - b2) * gc * gc;                      \
    P.c -= step * M.c / (sqrtf(V.c) * rsqrt_bc2 + eps);         \
  }
    FD_ADAM1(x) FD_ADAM1(y) FD_ADAM1(z) FD_ADAM1(w)
#undef FD_ADAM1
    reinterpret_cast<float4*>(p)[i] = P;
    reinterpret_cast<float4*>(m)[i] = M;
    reinterpret_cast<float4*>(v)[i] = V;
    if constexpr (EMA) {
      float4 E = reinterpret_cast<float4*>(ema)[i];
      E.x += a * (P.x - E.x);
      E.y += a * (P.y - E.y);
      E.z += a * (P.z - E.z);
      E.w += a * (P.w - E.w);
      reinterpret_cast<float4*>(ema)[i] = E;
    }
  }
}

int opt_grid(long n4) {
  const long gsz = (n4 + OT - 1) / OT;
  return (int)(gsz > OPT_MAX_BLOCKS ? OPT_MAX_BLOCKS : gsz);
}

}  // namespace

extern "C" int fd_grad_stats(const float* g, long n, double* workspace, double* stats, void* stream) {
  FD_CHECK_ARG(g && workspace && stats, "fd_grad_stats: null operand");
  FD_CHECK_ARG(n >= 0 && (n & 3) == 0 && fd_aligned16(g),
               "fd_grad_stats: the flat buffer must be 16-byte aligned with a length that is a multiple of 4");
  FD_CHECK_ARG((((uintptr_t)stats) & 7u) == 0 && (((uintptr_t)workspace) & 7u) == 0,
               "fd_grad_stats: workspace and stats must be 8-byte aligned");
  if (n == 0) return FD_OK;
  const long n4 = n / 4;
  const int grid = opt_grid(n4);
  hipLaunchKernelGGL(grad_stats_kernel, dim3(grid), dim3(OT), 0, (hipStream_t)stream, g, n4, workspace);
  FD_CHECK_LAUNCH("fd_grad_stats(partials)");
  const OptDecide none = {0.0, 0.0, 0.0, 0};
  FdOptState* no_state = nullptr;
  hipLaunchKernelGGL(grad_finalize_kernel, dim3(1), dim3(OT), 0, (hipStream_t)stream, (const double*)workspace, grid, stats,
                     no_state, none);
  FD_CHECK_LAUNCH("fd_grad_stats(finalize)");
  return FD_OK;
}

namespace {

// the three launches of both guarded entry points (arguments checked by the caller)
template <bool EMA>
int guarded_launch(float* p, const float* g, float* m, float* v, float* ema, long n, double lr, double b1, double b2, double eps,
                   double max_norm, int skip_nonfinite, double* workspace, void* state, double ema_decay, int ema_warmup,
                   void* stream) {
  const long n4 = n / 4;
  const int grid = opt_grid(n4);
  FdOptState* st = (FdOptState*)state;
  hipLaunchKernelGGL(grad_stats_kernel, dim3(grid), dim3(OT), 0, (hipStream_t)stream, g, n4, workspace);
  FD_CHECK_LAUNCH(EMA ? "fd_adam_step_guarded_ema(partials)" : "fd_adam_step_guarded(partials)");
  const OptDecide cfg = {b1, b2, max_norm, skip_nonfinite};
  double* no_stats = nullptr;
  hipLaunchKernelGGL(grad_finalize_kernel, dim3(1), dim3(OT), 0, (hipStream_t)stream, (const double*)workspace, grid, no_stats,
                     st, cfg);
  FD_CHECK_LAUNCH(EMA ? "fd_adam_step_guarded_ema(decide)" : "fd_adam_step_guarded(decide)");
  hipLaunchKernelGGL(HIP_KERNEL_NAME(adam_guarded_kernel<EMA>), dim3(grid), dim3(OT), 0, (hipStream_t)stream, p, g, m, v, n4,
                     (float)lr, (float)b1, (float)b2, (float)eps, (const FdOptState*)st, ema, ema_decay, ema_warmup);
  FD_CHECK_LAUNCH(EMA ? "fd_adam_step_guarded_ema(update)" : "fd_adam_step_guarded(update)");
  return FD_OK;
}

}  // namespace

extern "C" int fd_adam_step_guarded(float* p, const float* g, float* m, float* v, long n, double lr, double b1, double b2,
                                    double eps, double max_norm, int skip_nonfinite, double* workspace, void* state,
                                    void* stream) {
  FD_CHECK_ARG(p && g && m && v, "fd_adam_step_guarded: null operand");
  FD_CHECK_ARG(workspace && state, "fd_adam_step_guarded: null workspace or state");
  FD_CHECK_ARG(n >= 0 && (n & 3) == 0 && fd_aligned16(p) && fd_aligned16(g) && fd_aligned16(m) && fd_aligned16(v),
               "fd_adam_step_guarded: flat buffers must be 16-byte aligned with a length that is a multiple of 4");
  FD_CHECK_ARG((((uintptr_t)state) & 7u) == 0 && (((uintptr_t)workspace) & 7u) == 0,
               "fd_adam_step_guarded: workspace and state must be 8-byte aligned");
  if (n == 0) return FD_OK;
  return guarded_launch<false>(p, g, m, v, nullptr, n, lr, b1, b2, eps, max_norm, skip_nonfinite, workspace, state, 0.0, 0,
                               stream);
}

extern "C" int fd_adam_step_guarded_ema(float* p, const float* g, float* m, float* v, float* ema, long n, double lr, double b1,
                                        double b2, double eps, double max_norm, int skip_nonfinite, double* workspace,
                                        void* state, double ema_decay, int ema_warmup, void* stream) {
  FD_CHECK_ARG(p && g && m && v && ema, "fd_adam_step_guarded_ema: null operand");
  FD_CHECK_ARG(workspace && state, "fd_adam_step_guarded_ema: null workspace or state");
  FD_CHECK_ARG(n >= 0 && (n & 3) == 0 && fd_aligned16(p) && fd_aligned16(g) && fd_aligned16(m) && fd_aligned16(v) &&
                   fd_aligned16(ema),
               "fd_adam_step_guarded_ema: flat buffers must be 16-byte aligned with a length that is a multiple of 4");
  FD_CHECK_ARG((((uintptr_t)state) & 7u) == 0 && (((uintptr_t)workspace) & 7u) == 0,
               "fd_adam_step_guarded_ema: workspace and state must be 8-byte aligned");
  FD_CHECK_ARG(ema_decay > 0.0 && ema_decay < 1.0, "fd_adam_step_guarded_ema: ema_decay must lie strictly between 0 and 1");
  if (n == 0) return FD_OK;
  return guarded_launch<true>(p, g, m, v, ema, n, lr, b1, b2, eps, max_norm, skip_nonfinite, workspace, state, ema_decay,
                              ema_warmup, stream);
}
