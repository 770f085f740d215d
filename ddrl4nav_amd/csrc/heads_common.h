// What the head kernels share: heads.hip (Categorical actor + critic), gheads.hip (Gaussian actor + critic), gail.hip (the extra value
// head) and imit.hip (behaviour cloning).  All give a sample to one wavefront (512 features = 8 per lane), leave one row of partial sums
// per workgroup and sum the rows in a fixed order.  A head variant supplies its per-sample arithmetic, the layout of its partial row
// -- [gradient elements][statistics] -- and the reduce map that says where each of them goes; the rest is here.
#pragma once
#include "ppo_math.h"

namespace ddrl {

template <int N>
__device__ __forceinline__ float pick(const float (&a)[N], int idx) {
  // a chain of selects on registers.  Left to itself the compiler turns it into an indexed load from a private (scratch) copy of
  // the array: a dependent round trip through the vector memory path per call, four per sample in heads_loss; the empty asm keeps
  // every step a v_cndmask
  float r = a[0];
#pragma unroll
  for (int j = 1; j < N; ++j) {
    r = (idx == j) ? a[j] : r;
    asm volatile("" : "+v"(r));
  }
  return r;
}

// ---- the distributions' arithmetic that more than one head kernel evaluates ------------------------------------------------------------
// Categorical (heads.hip acting + loss, diag.hip): softmax, then torch.distributions.Categorical(probs)'s own bookkeeping; entries
// j >= A are masked.  Gaussian (gheads.hip, diag.hip): per dimension  -(a - mu)^2 / (2 var) - log(std) - LOG_SQRT_2PI.
constexpr float CAT_EPS = 1.1920928955078125e-07f;  // torch.finfo(float32).eps
constexpr float LOG_SQRT_2PI = 0.91893853320467274178f;  // math.log(math.sqrt(2 * math.pi))

template <int MAXA>
struct Dist {
  float p[MAXA];    // softmax output
  float q[MAXA];    // p / sum(p)                      (Categorical.probs)
  float lc[MAXA];   // log(clamp(q, eps, 1-eps))       (Categorical.logits)
  float ps;
};

template <int MAXA>
__device__ __forceinline__ void softmax_categorical(const float* z, int A, Dist<MAXA>& d) {
  float m = z[0];
#pragma unroll
  for (int j = 1; j < MAXA; ++j)
    if (j < A) m = fmaxf(m, z[j]);
  float s = 0.0f;
#pragma unroll
  for (int j = 0; j < MAXA; ++j) {
    d.p[j] = (j < A) ? expf(z[j] - m) : 0.0f;
    s += d.p[j];
  }
  d.ps = 0.0f;
#pragma unroll
  for (int j = 0; j < MAXA; ++j) {
    d.p[j] = d.p[j] / s;
    d.ps += d.p[j];
  }
#pragma unroll
  for (int j = 0; j < MAXA; ++j) {
    d.q[j] = d.p[j] / d.ps;
    d.lc[j] = logf(fminf(fmaxf(d.q[j], CAT_EPS), 1.0f - CAT_EPS));
  }
}

// ---- workgroup epilogue of the loss kernels: the waves add their sums into LDS one after the other (fixed order) ---------------------
//   for (w = 0; w < WAVES; ++w) { if (wave == w) { ...turn_add / turn_add_row with first = (w == 0)... } __syncthreads(); }
// turn_add: a scalar (by one lane); turn_add_row: the lane's 8 columns of a 512-wide row, at = row * 512 + lane * 8.  Where the buffer
// aliases LDS that the sample loop still reads (head weights), a __syncthreads() comes first.  (The loop stays in the kernels: passed to
// a helper as a lambda, the body moved the register allocation of heads_loss_kernel's prologue.)
__device__ __forceinline__ void turn_add(bool first, float& slot, float x) { slot = first ? x : slot + x; }
__device__ __forceinline__ void turn_add(bool first, double& slot, double x) { slot = first ? x : slot + x; }  // double partial rows (diag.hip)
__device__ __forceinline__ void turn_add_row(bool first, float* buf, int at, const float (&g)[8]) {
#pragma unroll
  for (int i = 0; i < 8; ++i) turn_add(first, buf[at + i], g[i]);
}

// ---- weight / bias gradient of a head layer of more than 8 rows, from the d(logits) its loss kernel left behind ----------------------
//   part[wg][j*512 + k] = sum_{b in the workgroup's samples} dlogits[b][j] * h[b][k],   part[wg][bias_off + j] = sum dlogits[b][j]
// (288 accumulator + weight registers do not fit a lane of the loss kernel).  Samples are dealt to workgroups round-robin, each thread
// owns columns k and k + 256 of every row; fixed order -> deterministic.
template <int MAXA>
__global__ __launch_bounds__(256) void head_wgrad_kernel(const float* __restrict__ h, int64_t ld_h, const float* __restrict__ dlogits,
                                                         int n, int A, float* __restrict__ part, int64_t pstride, int bias_off) {
  float acc[MAXA][2], bsum[MAXA];
#pragma unroll
  for (int j = 0; j < MAXA; ++j) acc[j][0] = acc[j][1] = bsum[j] = 0.0f;
  const int k = threadIdx.x;
  for (int b = blockIdx.x; b < n; b += gridDim.x) {
    const float h0 = h[(int64_t)b * ld_h + k], h1 = h[(int64_t)b * ld_h + 256 + k];
#pragma unroll
    for (int j = 0; j < MAXA; ++j) {
      const float g = (j < A) ? dlogits[(int64_t)b * A + min(j, A - 1)] : 0.0f;
      acc[j][0] = __builtin_fmaf(g, h0, acc[j][0]);
      acc[j][1] = __builtin_fmaf(g, h1, acc[j][1]);
      bsum[j] += g;
    }
  }
  float* out = part + (int64_t)blockIdx.x * pstride;
#pragma unroll
  for (int j = 0; j < MAXA; ++j) {
    if (j < A) {
      out[j * FEAT + k] = acc[j][0];
      out[j * FEAT + 256 + k] = acc[j][1];
      if (threadIdx.x == 0) out[bias_off + j] = bsum[j];
    }
  }
}

// ---- partial rows -> gradients and statistics ------------------------------------------------------------------------------------------
// Gradient element i < m.n_grad() is summed over the workgroups by ppo_math.h sum_partials8 (fixed order, in double, rounded once) and
// stored at m.dst(i) (null: dropped); the last workgroup takes the Map::N_STATS <= 4 sums behind them, one wave each
// (wave_sum_partials), and hands sum k to m.stat(k, sum).
template <class Map>
__global__ __launch_bounds__(256) void head_reduce_kernel(const float* __restrict__ part, int64_t stride, int nwg, Map m) {
  __shared__ double sh[8][RED_OUT];
  const int ng = m.n_grad();
  if (blockIdx.x == gridDim.x - 1) {
    const int k = threadIdx.x >> 6;
    if (k >= Map::N_STATS) return;
    const double s = wave_sum_partials(part, stride, nwg, ng + k);
    if ((threadIdx.x & 63) == 0) m.stat(k, s);
    return;
  }
  const int i = blockIdx.x * RED_OUT + (threadIdx.x & (RED_OUT - 1));
  const float sum = sum_partials8(part, stride, nwg, min(i, ng - 1), sh);
  if (threadIdx.x >= RED_OUT || i >= ng) return;
  if (float* d = m.dst(i)) *d = sum;
}
template <class Map>
void launch_head_reduce(const float* part, int64_t stride, int nwg, const Map& m, hipStream_t st) {
  hipLaunchKernelGGL(head_reduce_kernel<Map>, dim3((m.n_grad() + RED_OUT - 1) / RED_OUT + 1), dim3(256), 0, st, part, stride, nwg, m);
}

// the three loss statistics of PPO from their sums over the batch (ppo.py:86-108)
enum { STAT_ACTOR = 0, STAT_VALUE = 1, STAT_ENTROPY = 2 };
__device__ __forceinline__ float ppo_loss_stat(int k, double s, float inv_b, int smooth_l1) {
  if (k == STAT_ACTOR) return (float)(-s * (double)inv_b);                             // actor_loss = -mean(term)
  if (k == STAT_VALUE) return (float)(s * (double)inv_b * (smooth_l1 ? 1.0 : 0.5));  // v_loss = mean(err^2) / 2, or the smooth-L1 mean
  return (float)(s * (double)inv_b);                                                   // entropy = mean(H)
}

// Reduce map of the actor + critic heads.  Partial row: [n*512 dWa][512 dwc][n dba][dbc][n_log_std dlog_std][actor, value, entropy sums];
// the gradients go to the layers' places in the flat arena, the statistics behind its n_params gradients.
struct PpoHeadsReduce {
  HeadLayout L;
  int n_log_std;  // 0 (Categorical) or L.n (Gaussian)
  float inv_b;
  int smooth_l1;
  float* grads;
  static constexpr int N_STATS = 3;
  __host__ __device__ int n_grad() const { return (L.n + 1) * FEAT + L.n + 1 + n_log_std; }
  __device__ float* dst(int i) const {
    const int o = (L.n + 1) * FEAT;
    if (i < L.n * FEAT) return grads + L.actor_w + i;
    if (i < o) return grads + L.critic_w + (i - L.n * FEAT);
    if (i < o + L.n) return grads + L.actor_b + (i - o);
    if (i == o + L.n) return grads + L.critic_b;
    return grads + L.log_std + (i - (o + L.n + 1));
  }
  __device__ void stat(int k, double s) const { grads[L.n_params + k] = ppo_loss_stat(k, s, inv_b, smooth_l1); }
};

}  // namespace ddrl
