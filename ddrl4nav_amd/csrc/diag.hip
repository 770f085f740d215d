// Diagnostics of a PPO update on finished features (include/ddrl.h ddrl_op_heads_diag / ddrl_ppo_diag): approximate KL of the policy
// the loss was evaluated with against the one that collected the batch, the share of samples on the flat part of the clipped
// surrogate, the sums behind the critic's explained variance and the largest ratio.  The reference has no such numbers (DESIGN.md
// section 6).  A head variant in the sense of heads_common.h: its per-sample arithmetic is the forward half of heads_loss / gauss_loss
// (the same fma chains and butterflies, the same softmax_categorical / Normal log-prob text, so a ratio here is that kernel's ratio bit
// for bit), its partial row is DIAG_SLOTS doubles and its reduce map adds them up (slot 7: the larger).  It reads only.
#include "heads_common.h"
#include "kernels.h"
#include "rows.h"

namespace ddrl {

constexpr int DIAG_WAVES = 4;   // waves per workgroup: they share the LDS copy of the head weights
constexpr int DIAG_NS = 4;      // samples per wave and turn: the softmax / log / exp chain runs once per NS samples (as heads_loss)
constexpr int DIAG_MAXD = 8, DIAG_MAXA = 18;

// LDS: [MAXN actor rows][critic row][MAXN actor bias][MAXN var][MAXN log(std)][critic bias].  Rows >= L.n are neither staged nor read.
template <int MAXN, bool CONT>
__global__ __launch_bounds__(DIAG_WAVES * 64) void heads_diag_kernel(
    const float* __restrict__ h, int64_t h_es, const float* __restrict__ params, HeadLayout L, float ppo_clip, int n,
    const float* __restrict__ actions, const float* __restrict__ old_logps, const float* __restrict__ rets,
    double* __restrict__ part, float* __restrict__ logp_out, float* __restrict__ value_out) {
  constexpr int NS = DIAG_NS, WAVES = DIAG_WAVES;
  __shared__ __attribute__((aligned(16))) float wl[(MAXN + 1) * FEAT + 3 * MAXN + 4];
  __shared__ double red[DIAG_SLOTS];
  float* const sb = wl + (MAXN + 1) * FEAT;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int gw = blockIdx.x * WAVES + wave, nw = gridDim.x * WAVES;
  const int N = L.n;
  // the flat arena is only 4-byte aligned in general -> scalar loads
  for (int i = threadIdx.x; i < N * FEAT; i += WAVES * 64) wl[i] = params[L.actor_w + i];
  for (int i = threadIdx.x; i < FEAT; i += WAVES * 64) wl[MAXN * FEAT + i] = params[L.critic_w + i];
  if ((int)threadIdx.x < N) {
    sb[threadIdx.x] = params[L.actor_b + threadIdx.x];
    if constexpr (CONT) {
      const float s = expf(params[L.log_std + threadIdx.x]);  // as gheads.hip gload_weights
      sb[MAXN + threadIdx.x] = s * s;
      sb[2 * MAXN + threadIdx.x] = logf(s);
    }
  }
  if (threadIdx.x == 0) sb[3 * MAXN] = params[L.critic_b];
  __syncthreads();
  float wc[8];
  load8(wl + MAXN * FEAT + lane * 8, wc);
  const float bc = sb[3 * MAXN];
  const float lo = 1.0f - ppo_clip, hi = 1.0f + ppo_clip;  // ppo_math.h ppo_surrogate's bounds
  // a wave takes NS samples per turn: the dot products by all lanes (results in every lane), then lane i < NS works on sample i
  const int ls = lane & (NS - 1);
  const bool owner = lane < NS;
  double s_n = 0.0, s_kl = 0.0, s_clip = 0.0, s_ret = 0.0, s_ret2 = 0.0, s_e = 0.0, s_e2 = 0.0;
  float rmax = 0.0f;  // ratios are >= 0: the larger bit pattern is the larger number, and a NaN wins (ppo_math.h wave_max)
  float ha[NS][8], hc[NS][8];
  auto request = [&](int b0) {
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      const int b = min(b0 + i, n - 1);  // past the end: the last sample again, masked below
      load8(h + (int64_t)b * FEAT + lane * 8, ha[i]);
      load8(h + h_es + (int64_t)b * FEAT + lane * 8, hc[i]);
    }
  };
  if (gw * NS < n) request(gw * NS);
  for (int b0 = gw * NS; b0 < n; b0 += nw * NS) {
    const int bl = min(b0 + ls, n - 1);
    const bool live = owner && b0 + ls < n;
    const float olp = old_logps[bl], ret = rets[bl];
    // ---- the N + 1 dot products of the NS samples; a lane keeps its own sample's
    float zl[MAXN], v = 0.0f;
#pragma unroll
    for (int j = 0; j < MAXN; ++j) {
      zl[j] = 0.0f;
      if (j < N) {  // wave-uniform
        float w[8];
        load8(wl + j * FEAT + lane * 8, w);
        const float bj = sb[j];
#pragma unroll
        for (int i = 0; i < NS; ++i) {
          float s = 0.0f;
#pragma unroll
          for (int k = 0; k < 8; ++k) s = __builtin_fmaf(ha[i][k], w[k], s);
          const float zj = wave_sum(s) + bj;
          zl[j] = (ls == i) ? zj : zl[j];
        }
      }
    }
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      float sv = 0.0f;
#pragma unroll
      for (int k = 0; k < 8; ++k) sv = __builtin_fmaf(hc[i][k], wc[k], sv);
      const float vi = wave_sum(sv) + bc;
      v = (ls == i) ? vi : v;
    }
    // the next turn's samples into the registers just finished with: they arrive under the scalar chain below
    if (b0 + nw * NS < n) request(b0 + nw * NS);  // wave-uniform
    // ---- this lane's sample
    float logp;
    if constexpr (CONT) {
      logp = 0.0f;
#pragma unroll
      for (int d = 0; d < MAXN; ++d) {
        if (d < N) {
          const float diff = actions[(int64_t)bl * N + d] - zl[d];
          logp += -(diff * diff) / (2.0f * sb[MAXN + d]) - sb[2 * MAXN + d] - LOG_SQRT_2PI;
        }
      }
    } else {
      Dist<MAXN> dist;
      softmax_categorical(zl, N, dist);
      logp = pick(dist.lc, (int)actions[bl]);
    }
    const float x = logp - olp;
    const float r = expf(x);
    if (live) {
      const double xd = (double)x, rd = (double)ret, e = rd - (double)v;
      s_n += 1.0;
      s_kl += fmax(expm1(xd) - xd, 0.0);  // >= 0 in exact arithmetic; the clamp takes the last-place error of expm1 at tiny |x|
      s_clip += (r >= lo && r <= hi) ? 0.0 : 1.0;
      s_ret += rd;
      s_ret2 += rd * rd;
      s_e += e;
      s_e2 += e * e;
      rmax = __uint_as_float(max(__float_as_uint(rmax), __float_as_uint(r)));
      if (logp_out) logp_out[bl] = logp;
      if (value_out) value_out[bl] = v;
    }
  }
  // the sums live in the NS owner lanes: added in sample order into lane 0, then the waves in turn (fixed order)
  double t[DIAG_SLOTS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int i = 0; i < NS; ++i) {
    t[0] += __shfl(s_n, i, 64);
    t[1] += __shfl(s_kl, i, 64);
    t[2] += __shfl(s_clip, i, 64);
    t[3] += __shfl(s_ret, i, 64);
    t[4] += __shfl(s_ret2, i, 64);
    t[5] += __shfl(s_e, i, 64);
    t[6] += __shfl(s_e2, i, 64);
    t[7] = diag_max(t[7], (double)__shfl(rmax, i, 64));
  }
  for (int w = 0; w < WAVES; ++w) {
    if (wave == w && lane == 0) {
      const bool first = (w == 0);
#pragma unroll
      for (int k = 0; k < DIAG_SLOTS - 1; ++k) turn_add(first, red[k], t[k]);
      red[7] = first ? t[7] : diag_max(red[7], t[7]);
    }
    __syncthreads();
  }
  if (threadIdx.x < DIAG_SLOTS) part[(int64_t)blockIdx.x * DIAG_SLOTS + threadIdx.x] = red[threadIdx.x];
}

// Reduce map of the diagnostics: rows.h rows_fold_kernel adds the workgroups' rows up in a fixed order; slot 7 takes the larger.
void launch_heads_diag(const DiagCall& c, const float* actions, const float* old_logps, const float* rets, double* sums8,
                       int accumulate, float* logp_out, float* value_out, hipStream_t st) {
  const int per_wg = DIAG_WAVES * DIAG_NS;
  int wgs = (c.n + per_wg - 1) / per_wg;
  if (wgs > DIAG_MAX_WG) wgs = DIAG_MAX_WG;
  auto kern = c.continuous ? heads_diag_kernel<DIAG_MAXD, true>
                           : (c.L.n <= 8 ? heads_diag_kernel<8, false> : heads_diag_kernel<DIAG_MAXA, false>);
  hipLaunchKernelGGL(kern, dim3(wgs), dim3(DIAG_WAVES * 64), 0, st, c.h, c.h_es, c.params, c.L, c.ppo_clip, c.n, actions, old_logps,
                     rets, c.part, logp_out, value_out);
  hipLaunchKernelGGL((rows_fold_kernel<DIAG_SLOTS, DIAG_SLOTS - 1>), dim3(1), dim3(DIAG_SLOTS * 64), 0, st, (const double*)c.part, wgs, sums8,
                     accumulate);
}

}  // namespace ddrl
