// Gaussian actor head + critic head for the continuous-action nets (robot navigation), with the
// same PPO dual-clip loss block as heads.hip.  One wavefront per sample, D <= 8 action dims.
//
// Reference arithmetic replaced:
//   GaussionActor._distribution / _log_prob_from_distribution   USTC_lab/nn/actor.py:43-70
//     mu = actor_linear(h); std = exp(log_std); Normal(mu, std); log_prob(act).sum(-1)
//   torch.distributions.Normal.log_prob / entropy / sample
//     -((a-mu)^2)/(2 var) - log(std) - log(sqrt(2 pi));  0.5 + 0.5 log(2 pi) + log(std);  mu + std * eps
//   Critic.forward                                             USTC_lab/nn/critic.py:14-21
//   PPO.learn loss block + autograd                            USTC_lab/nn/ppo.py:82-129
#include "heads_common.h"
#include "kernels.h"
#include "ops.h"

namespace ddrl {

constexpr int MAXD = 8;


struct GHeadRegs {
  float wa[MAXD][8], wc[8], ba[MAXD], std[MAXD], var[MAXD], log_scale[MAXD], bc;
};

__device__ __forceinline__ void gload_weights(GHeadRegs& R, const float* params, const HeadLayout& L, int lane) {
#pragma unroll
  for (int d = 0; d < MAXD; ++d) {
    const int dd = min(d, L.n - 1);
#pragma unroll
    for (int i = 0; i < 8; ++i) R.wa[d][i] = (d < L.n) ? params[L.actor_w + (int64_t)dd * FEAT + lane * 8 + i] : 0.0f;
    R.ba[d] = (d < L.n) ? params[L.actor_b + dd] : 0.0f;
    const float s = expf(params[L.log_std + dd]);  // std = torch.exp(self.log_std)
    R.std[d] = s;
    R.var[d] = s * s;          // Normal.log_prob: var = scale ** 2
    R.log_scale[d] = logf(s);  // log_scale = scale.log()
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) R.wc[i] = params[L.critic_w + lane * 8 + i];
  R.bc = params[L.critic_b];
}

// standard normal from two counter-based uniforms (Box-Muller); u1 in (0,1]
__device__ __forceinline__ float hash_normal(uint64_t seed, uint64_t stream, uint64_t idx) {
  const float u1 = 1.0f - hash_uniform(seed, stream, 2 * idx);
  const float u2 = hash_uniform(seed, stream, 2 * idx + 1);
  return sqrtf(-2.0f * logf(u1)) * cosf(6.283185307179586f * u2);
}

__global__ __launch_bounds__(256) void gauss_act_kernel(const float* __restrict__ h_actor, const float* __restrict__ h_critic,
                                                        const float* __restrict__ params, HeadLayout L, int n,
                                                        const float* __restrict__ act_in, uint64_t seed, uint64_t stream_id,
                                                        float* __restrict__ mu_out, float* __restrict__ value,
                                                        float* __restrict__ action_out, float* __restrict__ logp_out) {
  const int lane = threadIdx.x & 63;
  const int gw = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int nw = (gridDim.x * blockDim.x) >> 6;
  GHeadRegs R;
  gload_weights(R, params, L, lane);
  for (int b = gw; b < n; b += nw) {
    float ha[8], hc[8];
    load8(h_actor + (int64_t)b * FEAT + lane * 8, ha);
    load8(h_critic + (int64_t)b * FEAT + lane * 8, hc);
    float sv = 0.0f;
#pragma unroll
    for (int i = 0; i < 8; ++i) sv = __builtin_fmaf(hc[i], R.wc[i], sv);
    const float v = wave_sum(sv) + R.bc;
    float logp = 0.0f;
#pragma unroll
    for (int d = 0; d < MAXD; ++d) {
      float s = 0.0f;
#pragma unroll
      for (int i = 0; i < 8; ++i) s = __builtin_fmaf(ha[i], R.wa[d][i], s);
      const float mu = wave_sum(s) + R.ba[d];
      if (d < L.n) {
        float a;
        if (act_in != nullptr) a = act_in[(int64_t)b * L.n + d];
        else a = mu + R.std[d] * hash_normal(seed, stream_id, (uint64_t)b * L.n + d);
        const float diff = a - mu;
        logp += -(diff * diff) / (2.0f * R.var[d]) - R.log_scale[d] - LOG_SQRT_2PI;
        if (lane == 0) {
          if (mu_out) mu_out[(int64_t)b * L.n + d] = mu;
          if (action_out) action_out[(int64_t)b * L.n + d] = a;
        }
      }
    }
    if (lane == 0) {
      value[b] = v;
      if (logp_out) logp_out[b] = logp;
    }
  }
}

// hpart per workgroup: [D*512 dWa][512 dwc][D dba][1 dbc][D dlog_std][actor_sum, v_sum, ent_sum]
// OPT / X: the update options, as heads.hip heads_loss_kernel
template <bool OPT = false, class... X>
__global__ __launch_bounds__(256) void gauss_loss_kernel(
    const float* __restrict__ h_actor, const float* __restrict__ h_critic, const float* __restrict__ params, HeadLayout L,
    ddrl_config cfg, int n, const float* __restrict__ actions, const float* __restrict__ old_logps,
    const float* __restrict__ advs, const float* __restrict__ rets, float inv_b, float* __restrict__ dh_actor,
    float* __restrict__ dh_critic, float* __restrict__ dmu_out, float* __restrict__ dvalue, float* __restrict__ hpart,
    int64_t hstride, X... x) {
  static_assert(sizeof...(X) == (OPT ? 2 : 0), "the options and old_values come with OPT only");
  __shared__ float red[(MAXD + 1) * FEAT + 3 * MAXD + 8];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int gw = blockIdx.x * 4 + wave, nw = gridDim.x * 4;
  const int D = L.n;
  const bool shared = L.shared != 0;
  const LossOptions opt = loss_options(x...);
  const float* __restrict__ old_values = loss_old_values(x...);  // OPT: never null (the launcher passes rets where the clip is off)
  bool ent_grad = shared;  // the entropy term is differentiated
  if constexpr (OPT) ent_grad = shared || opt.entropy_split != 0;
  GHeadRegs R;
  gload_weights(R, params, L, lane);
  float gwa[MAXD][8], gwc[8], gba[MAXD], gls[MAXD], gbc = 0.0f;
#pragma unroll
  for (int d = 0; d < MAXD; ++d) {
    gba[d] = gls[d] = 0.0f;
#pragma unroll
    for (int i = 0; i < 8; ++i) gwa[d][i] = 0.0f;
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) gwc[i] = 0.0f;
  double s_actor = 0.0, s_v = 0.0, s_ent = 0.0;
  float ent_b = 0.0f;  // sum_d entropy_d / D : identical for every sample
#pragma unroll
  for (int d = 0; d < MAXD; ++d)
    if (d < D) ent_b += 0.5f + LOG_SQRT_2PI + R.log_scale[d];  // 0.5 + 0.5*log(2 pi) + log(std)
  ent_b = ent_b / (float)D;

  for (int b = gw; b < n; b += nw) {
    float ha[8], hc[8];
    load8(h_actor + (int64_t)b * FEAT + lane * 8, ha);
    load8(h_critic + (int64_t)b * FEAT + lane * 8, hc);
    float sv = 0.0f;
#pragma unroll
    for (int i = 0; i < 8; ++i) sv = __builtin_fmaf(hc[i], R.wc[i], sv);
    const float v = wave_sum(sv) + R.bc;
    float diff[MAXD], logp = 0.0f;
#pragma unroll
    for (int d = 0; d < MAXD; ++d) {
      float s = 0.0f;
#pragma unroll
      for (int i = 0; i < 8; ++i) s = __builtin_fmaf(ha[i], R.wa[d][i], s);
      const float mu = wave_sum(s) + R.ba[d];
      diff[d] = (d < D) ? actions[(int64_t)b * D + min(d, D - 1)] - mu : 0.0f;
      if (d < D) logp += -(diff[d] * diff[d]) / (2.0f * R.var[d]) - R.log_scale[d] - LOG_SQRT_2PI;
    }
    const float adv = advs[b];
    const SurrogateTerm sg = ppo_surrogate(logp, old_logps[b], adv, cfg, inv_b);
    s_actor += (double)sg.term;
    const float err = rets[b] - v;
    float gv_unit;
    if constexpr (OPT) gv_unit = opt.value_clip > 0.0f ? value_loss_element_clipped(rets[b], v, old_values[b], opt.value_clip, cfg, s_v) : value_loss_element(err, cfg, s_v);
    else gv_unit = value_loss_element(err, cfg, s_v);
    s_ent += (double)ent_b;
    const float g_logp = sg.g_logp;
    const float gv = shared ? gv_unit * inv_b * cfg.v_loss_theta : gv_unit * inv_b;
    float dmu[MAXD];
#pragma unroll
    for (int d = 0; d < MAXD; ++d) {
      dmu[d] = (d < D) ? g_logp * (diff[d] / R.var[d]) : 0.0f;
      // d logp / d log_std = diff^2 / var - 1 ; entropy term only when total_loss is differentiated
      float gl = (d < D) ? g_logp * ((diff[d] * diff[d]) / R.var[d] - 1.0f) : 0.0f;
      if (ent_grad && d < D) gl += -cfg.ent_loss_theta * inv_b / (float)D;
      gls[d] += gl;
      gba[d] += dmu[d];
    }
    float da[8], dc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      float s = 0.0f;
#pragma unroll
      for (int d = 0; d < MAXD; ++d) s = __builtin_fmaf(dmu[d], R.wa[d][i], s);
      da[i] = s;
      dc[i] = gv * R.wc[i];
      gwc[i] = __builtin_fmaf(gv, hc[i], gwc[i]);
    }
#pragma unroll
    for (int d = 0; d < MAXD; ++d)
#pragma unroll
      for (int i = 0; i < 8; ++i) gwa[d][i] = __builtin_fmaf(dmu[d], ha[i], gwa[d][i]);
    gbc += gv;
    if (shared) {
#pragma unroll
      for (int i = 0; i < 8; ++i) da[i] += dc[i];
      store8(dh_actor + (int64_t)b * FEAT + lane * 8, da);
    } else {
      store8(dh_actor + (int64_t)b * FEAT + lane * 8, da);
      store8(dh_critic + (int64_t)b * FEAT + lane * 8, dc);
    }
    if (lane < D) dmu_out[(int64_t)b * D + lane] = pick(dmu, lane);
    if (lane == 0) dvalue[b] = gv;
  }

  constexpr int SCAL = (MAXD + 1) * FEAT;
  for (int w = 0; w < 4; ++w) {
    if (wave == w) {
      const bool first = (w == 0);
#pragma unroll
      for (int d = 0; d < MAXD; ++d) turn_add_row(first, red, d * FEAT + lane * 8, gwa[d]);
      turn_add_row(first, red, MAXD * FEAT + lane * 8, gwc);
      if (lane == 0) {
#pragma unroll
        for (int d = 0; d < MAXD; ++d) {
          turn_add(first, red[SCAL + d], gba[d]);
          turn_add(first, red[SCAL + MAXD + d], gls[d]);
        }
        turn_add(first, red[SCAL + 2 * MAXD], gbc);
        turn_add(first, red[SCAL + 2 * MAXD + 1], (float)s_actor);
        turn_add(first, red[SCAL + 2 * MAXD + 2], (float)s_v);
        turn_add(first, red[SCAL + 2 * MAXD + 3], (float)s_ent);
      }
    }
    __syncthreads();
  }
  float* out = hpart + (int64_t)blockIdx.x * hstride;
  for (int i = threadIdx.x; i < D * FEAT; i += 256) out[i] = red[i];
  for (int i = threadIdx.x; i < FEAT; i += 256) out[D * FEAT + i] = red[MAXD * FEAT + i];
  const int o = (D + 1) * FEAT;
  if (threadIdx.x < D) {
    out[o + threadIdx.x] = red[SCAL + threadIdx.x];
    out[o + D + 1 + threadIdx.x] = red[SCAL + MAXD + threadIdx.x];
  }
  if (threadIdx.x == 0) out[o + D] = red[SCAL + 2 * MAXD];
  if (threadIdx.x < 3) out[o + 2 * D + 1 + threadIdx.x] = red[SCAL + 2 * MAXD + 1 + threadIdx.x];
}

int64_t gauss_hpart_stride(int D) { return align_up((int64_t)(D + 1) * FEAT + 2 * D + 1 + 3, 64); }

void launch_gauss_act(const HeadLayout& L, const float* params, const float* h_actor, const float* h_critic, int n,
                      const float* act_in, uint64_t seed, uint64_t stream_id, float* mu_out, float* value, float* action_out,
                      float* logp_out, hipStream_t st) {
  int wgs = (n + 3) / 4;
  if (wgs > 1024) wgs = 1024;
  hipLaunchKernelGGL(gauss_act_kernel, dim3(wgs), dim3(256), 0, st, h_actor, h_critic, params, L, n, act_in, seed, stream_id,
                     mu_out, value, action_out, logp_out);
}

template <bool OPT, class... X>
static void launch_gauss_loss_with(const HeadLayout& L, const ddrl_config& cfg, const float* params, const float* h_actor,
                                   const float* h_critic, int n, const float* actions, const float* old_logps, const float* advs,
                                   const float* rets, float inv_b, float* dh_actor, float* dh_critic, float* dmu, float* dvalue,
                                   float* hpart, float* grads, hipStream_t st, X... x) {
  const int64_t hs = gauss_hpart_stride(L.n);
  hipLaunchKernelGGL((gauss_loss_kernel<OPT, X...>), dim3(HEAD_WG), dim3(256), 0, st, h_actor, h_critic, params, L, cfg, n, actions,
                     old_logps, advs, rets, inv_b, dh_actor, dh_critic, dmu, dvalue, hpart, hs, x...);
  launch_head_reduce(hpart, hs, HEAD_WG, PpoHeadsReduce{L, L.n, inv_b, cfg.smooth_l1_loss, grads}, st);
}

void launch_gauss_loss(const HeadLayout& L, const ddrl_config& cfg, const float* params, const float* h_actor,
                       const float* h_critic, int n, const float* actions, const float* old_logps, const float* advs,
                       const float* rets, float inv_b, float* dh_actor, float* dh_critic, float* dmu, float* dvalue,
                       float* hpart, float* grads, hipStream_t st) {
  launch_gauss_loss_with<false>(L, cfg, params, h_actor, h_critic, n, actions, old_logps, advs, rets, inv_b, dh_actor, dh_critic, dmu,
                                dvalue, hpart, grads, st);
}

void launch_gauss_loss_opt(const HeadLayout& L, const ddrl_config& cfg, const float* params, const float* h_actor,
                           const float* h_critic, int n, const float* actions, const float* old_logps, const float* advs,
                           const float* rets, const LossOptions& opt, const float* old_values, float inv_b, float* dh_actor,
                           float* dh_critic, float* dmu, float* dvalue, float* hpart, float* grads, hipStream_t st) {
  launch_gauss_loss_with<true>(L, cfg, params, h_actor, h_critic, n, actions, old_logps, advs, rets, inv_b, dh_actor, dh_critic, dmu,
                               dvalue, hpart, grads, st, opt, opt.value_clip > 0.0f ? old_values : rets);
}

}  // namespace ddrl
