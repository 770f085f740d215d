// Internal launcher interface between the translation units of libddrl_hip.so.
#pragma once
#include "common.h"

namespace ddrl {

// per-kernel HIP-event ranges (diagnostic; null when profiling is off)
struct Profiler {
  virtual void begin(const char* name, hipStream_t st) = 0;
  virtual void end(hipStream_t st) = 0;
  virtual ~Profiler() {}
};
struct ProfRange {
  Profiler* p;
  hipStream_t st;
  ProfRange(Profiler* p_, const char* name, hipStream_t s) : p(p_), st(s) {
    if (p) p->begin(name, s);
  }
  ~ProfRange() {
    if (p) p->end(st);
  }
};

// Gradient buckets of the data-parallel all-reduce, in the order the backward COMPLETES them ("bucket by layer so
// that the all-reduce of the early buckets overlaps the rest of the backward"): heads + loss tail (after heads_loss), conv1 (its
// weight gradient runs right after the data-gradient chain), dense, conv3, conv2.  launch_encoder_backward records bucket_ev[b] on
// the compute stream once bucket b's slabs are reduced into the arena; a communication stream waits for it (api.hip).
constexpr int GRAD_BUCKETS = 5, BUCKET_HEADS = 0, BUCKET_CONV1 = 1, BUCKET_FC = 2, BUCKET_CONV3 = 3, BUCKET_CONV2 = 4;

struct EncCall {
  Profiler* prof;
  const Workspace* ws;
  const ParamLayout* L;
  const Splits* splits;
  const float* params;
  const uint8_t* frames;  // [n][4][84][84]
  int n;
  hipEvent_t* bucket_ev = nullptr;  // [GRAD_BUCKETS] or null (single rank: nothing to overlap)
  bool keep_acts = false;           // acting launches: also store a1 / a2 (ddrl_debug_keep_activations; the fused kernel of act.hip keeps them on chip)
  // launches reading frames in place (ddrl_ppo_iter_indexed, ddrl_forward_indexed): tab [n][4] = index of the 7,056-byte plane behind
  // `frames` that holds channel c of sample b (entries c >= C repeat entry C - 1), n_planes = planes behind `frames`; the conv1 kernels
  // and the fused acting kernel (act.hip) clamp every entry to [0, n_planes).  null = `frames` is the contiguous [n][C][84][84]
  const int32_t* tab = nullptr;
  int64_t n_planes = 0;
};
inline void bucket_done(const EncCall& c, int b, hipStream_t st) {
  if (c.bucket_ev) (void)hipEventRecord(c.bucket_ev[b], st);
}

// encoder.hip
void launch_encoder_forward(const EncCall& c, bool acting, hipStream_t st);
void launch_encoder_backward(const EncCall& c, float* grads, hipStream_t st, bool dh_normalised = false);
void launch_backward_amax_reset(const EncCall& c, hipStream_t st);  // zeroes the gradient slots of Workspace::amax

// fc2.hip
// Split-K factor of the FC forward for a batch of n samples (1 = plain; >1 only on the acting
// path, where heads_act sums the partials).  7 k-blocks of 32 per split.
inline int fc_forward_splits(int n) { return n <= 1024 ? FC_ACT_SPLITS : 1; }
void launch_fc_forward(const EncCall& c, bool allow_split, hipStream_t st, bool per_sample_max = false);
void launch_fc_backward(const EncCall& c, float* grads, hipStream_t st, int part = 0);

// conv2.hip
void launch_conv_forward(const EncCall& c, bool acting, hipStream_t st);
void launch_conv_dgrad3(const EncCall& c, hipStream_t st);
void launch_conv_dgrad2(const EncCall& c, hipStream_t st);

// act.hip: conv1 + conv2 + conv3 of an acting forward in one launch, one workgroup per (sample, encoder); leaves a3 and every sample's
// largest |a3| (Workspace::actmax), which the dense layer's split launch takes its plane scale from
// (ACT_FUSED_MAX: common.h, next to the carve of Workspace::actmax)
void launch_act_convs(const EncCall& c, hipStream_t st);

// wgrad2.hip
void launch_conv_wgrad3(const EncCall& c, float* grads, hipStream_t st);
void launch_conv_wgrad2(const EncCall& c, float* grads, hipStream_t st);
void launch_conv_wgrad1(const EncCall& c, float* grads, hipStream_t st);

// optim.hip
void launch_pack_weights(const Workspace& w, const ParamLayout& L, const float* params, hipStream_t st);
void launch_reduce_partials(const float* part, int nsplit, int64_t count, int ne, float* grads, int64_t off0,
                            int64_t off1, hipStream_t st);
void launch_clip_adam(const ddrl_config& cfg, const ParamLayout& L, double* npart, float* params,
                      float* grads, float* m, float* v, int64_t step, hipStream_t st);
void launch_episode_returns(const float* rewards, const uint8_t* dones, int T, int N, float* rsum, float* rep, float* trace,
                            int* finished, hipStream_t st);
void launch_gae(const float* values, const float* rewards, const uint8_t* dones, int T, int N,
                float gamma, float landa, float* adv, float* ret, hipStream_t st);
void launch_gae_bootstrap(const float* values, const float* rewards, const uint8_t* dones, const int32_t* slot, const float* boot, int S,
                          int T, int N, float gamma, float landa, float* adv, float* ret, hipStream_t st);
void launch_fill_lut(float* lut, hipStream_t st);

// heads.hip: what one launch of the Categorical head kernels reads and writes.  The Atari context fills it from its workspace
// (api.hip ctx_heads_call), the operator entry points from their arguments (api_ops.hip).
struct HeadsCall {
  const ParamLayout* L;
  const ddrl_config* cfg;  // launch_heads_loss only
  const float* params;
  int n;
  // features [n][512] of the actor's encoder and their gradient; the critic's encoder's lie h_es / dh_es floats further (a difference
  // of two allocations: any value, negative included; not read with a shared prenet)
  const float* h;
  int64_t h_es;
  float* dh;
  int64_t dh_es;
  // acting on the dense layer's split-K partial sums (fc2.hip): heads_act adds them up and WRITES the finished features to h
  const float* fc_part = nullptr;
  int fc_nsplit = 0;
  float *dlogits = nullptr, *dvalue = nullptr, *hpart = nullptr;  // launch_heads_loss: [n][A], [n], [HEAD_WG][hpart_stride(A)]
  // heads_loss also normalises dh per sample (scales to gsc[e * gsc_es + b], amax slots DH / GMAX, which the caller has zeroed;
  // launch_encoder_backward is then told to skip its stand-alone dh_normalise_kernel); null = plain dh
  float* gsc = nullptr;
  int64_t gsc_es = 0;
  float* amax = nullptr;
};
void launch_heads_act(const HeadsCall& c, const float* act_in, uint64_t seed, uint64_t stream_id,
                      float* probs, float* value, float* action_out, float* logp_out, hipStream_t st);
void launch_heads_loss(const HeadsCall& c, const float* actions, const float* old_logps,
                       const float* advs, const float* rets, float inv_bglobal, float* grads,
                       hipStream_t st);
// the same with the update options (common.h LossOptions): old_values [n] is read when opt.value_clip > 0 only
void launch_heads_loss_opt(const HeadsCall& c, const float* actions, const float* old_logps, const float* advs, const float* rets,
                           const LossOptions& opt, const float* old_values, float inv_bglobal, float* grads, hipStream_t st);
void launch_categorical_sample(const float* probs, int n, int A, uint64_t seed, uint64_t stream_id, float* action,
                               float* logp, hipStream_t st);
void launch_categorical_stats(const float* probs, int n, int A, float* p_hat, float* logits,
                              float* entropy, hipStream_t st);

// diag.hip: the read-only diagnostics head of both families (include/ddrl.h ddrl_op_heads_diag).  Features as in HeadsCall: the
// critic's lie h_es floats behind the actor's (any sign; 0 with a shared prenet).  part = DIAG_MAX_WG rows of DIAG_SLOTS doubles.
constexpr int DIAG_SLOTS = 8, DIAG_MAX_WG = 1024;
struct DiagCall {
  HeadLayout L;
  bool continuous;
  float ppo_clip;
  const float* params;
  int n;
  const float* h;
  int64_t h_es;
  double* part;
};
void launch_heads_diag(const DiagCall& c, const float* actions, const float* old_logps, const float* rets, double* sums8,
                       int accumulate, float* logp_out, float* value_out, hipStream_t st);

}  // namespace ddrl
