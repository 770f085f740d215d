/*
 * ddrl.h -- C ABI of the MI355X-native DDRL4NAV actor-learner hot path (libddrl_hip.so).
 *
 * The reference has no FFI on this path: its boundary is a Python object protocol
 * (USTC_lab.nn.PPO called by USTC_lab/server/forward.py:107-182 and
 * USTC_lab/server/backward.py:168-217).  This header is what a cgo/ctypes/N-API binding of
 * that path would bind; every entry point names the reference code it replaces.
 *
 * Conventions
 *   - every function returns an int32 status (0 = DDRL_OK, negative = error); nothing throws;
 *   - all tensor pointers are DEVICE pointers owned by the caller (e.g. PyTorch-ROCm tensors)
 *     unless the name ends in _host; the library allocates no device memory after
 *     ddrl_ctx_create (it allocates none at all: the caller passes the arenas and workspace);
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); calls are
 *     asynchronous on that stream and may be captured into a hipGraph;
 *   - one caller thread per context.
 *
 * Layouts (C-contiguous):
 *   frames   uint8  [n, C, 84, 84]     C = in_channels (1..4) stacked frames exactly as the env wrapper emits them
 *                                      before the /255.0 (reference warputils.py:274-301);
 *                                      the kernels apply float32(u8/255.0) themselves.
 *   params / grads / adam_m / adam_v   float32 flat arenas in the reference's
 *                                      named_parameters() order (USTC_lab/nn/base.py:60-66):
 *                                      actor.pre.{conv1,conv2,conv3,linear}.{weight,bias},
 *                                      actor.actor_linear.{weight,bias},
 *                                      critic.critic_linear.{weight,bias},
 *                                      critic.pre.{conv1,conv2,conv3,linear}.{weight,bias}.
 *                                      `grads` has DDRL_STATS_FLOATS extra floats at its tail
 *                                      (loss partial sums) so one all-reduce covers both.
 */
#ifndef DDRL_H_
#define DDRL_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DDRL_OK 0
#define DDRL_ERR_INVALID_ARG (-1)
#define DDRL_ERR_UNSUPPORTED (-2)
#define DDRL_ERR_WORKSPACE (-3)
#define DDRL_ERR_HIP (-4)
#define DDRL_ERR_NO_DEVICE (-5)
#define DDRL_ERR_TIMEOUT (-6)
#define DDRL_ERR_NO_MEMORY (-7) /* host allocation of a handle failed */

/* 2 (round 4): ddrl_op_clip_rmsprop takes alpha as a double; ddrl_encoder_backward consumes dh (rescales its rows in place);
 * ddrl_debug_buffer 4..7 hold per-sample NORMALISED gradients.  A host built against version 1 must be rebuilt. */
#define DDRL_ABI_VERSION 3
#define DDRL_STATS_FLOATS 8 /* tail of the grad arena, see ddrl_ppo_iter */

typedef struct ddrl_ctx ddrl_ctx;
typedef struct ddrl_ring ddrl_ring;
typedef struct ddrl_comm ddrl_comm;

/* Hyper-parameters: the ConfigNN contract (USTC_lab/config/config_nn.py:19-57). */
typedef struct ddrl_config {
  int32_t n_actions;      /* ACTION_OUTPUT_DIM, 6 for Pong                       */
  int32_t in_channels;    /* int_frame_stack: 1..4 (atari.yaml: 4)                */
  int32_t max_batch;      /* largest n / B any call will pass (sizes workspace);
                             1 .. 83,886 (32-bit byte offsets into the conv1 activations);
                             larger global batches: shard, or pass B_global to ddrl_ppo_iter */
  int32_t share_cnn_net;  /* SHARE_CNN_NET: 0 = actor and critic own an encoder each (default,
                             ppo.py:118-129), 1 = one shared prenet, one Adam over every
                             parameter on total_loss (ppo.py:110-117)                */
  int32_t clip_grad;      /* CLIP_GRID                                            */
  float clip_grad_norm;   /* CLIP_GRID_NUM = 0.5                                  */
  float actor_lr;         /* ACTOR_LEARNING_RATE = 5e-5                           */
  float critic_lr;        /* CRITIC_LEARNING_RATE = 1e-3                          */
  float adam_beta1;       /* torch.optim.Adam default 0.9                         */
  float adam_beta2;       /* 0.999                                                */
  float adam_eps;         /* 1e-8                                                 */
  float ppo_clip;         /* PPO_CLIP = 0.2                                       */
  float dual_clip;        /* DUEL_PPO_CLIP = 3                                    */
  float v_loss_theta;     /* V_LOSS_THETA = 1.0                                   */
  float ent_loss_theta;   /* ENTROPY_LOSS_THETA = 0.05                            */
  float learning_rate;    /* LEARNING_RATE = 2e-4, the single Adam of the shared mode */
  int32_t smooth_l1_loss; /* SMOOTH_L1_LOSS: 0 = mean((ret-v)^2)/2, 1 = F.smooth_l1_loss (ppo.py:53-57) */
} ddrl_config;

int32_t ddrl_abi_version(void);
const char* ddrl_status_string(int32_t status);

/* Fill `cfg` with the reference defaults (config_nn.py) for Pong. */
int32_t ddrl_config_default(ddrl_config* cfg);

/* Number of fp32 parameters (3,371,847 for the default net) and of the actor-side prefix
 * (the parameters stepped with actor_lr; the remainder is stepped with critic_lr --
 * USTC_lab/nn/ppo.py:41-42). */
int32_t ddrl_param_count(const ddrl_config* cfg, int64_t* n_params, int64_t* n_actor_params);

/* Bytes of caller-provided device workspace needed for cfg->max_batch. */
int32_t ddrl_workspace_bytes(const ddrl_config* cfg, int64_t* bytes);

/* Create a context over caller-owned device arenas.  grads must hold n_params +
 * DDRL_STATS_FLOATS floats; params/adam_m/adam_v hold n_params floats.  adam_m/adam_v must be
 * zeroed by the caller for a fresh optimiser.  Replaces PPO.__init__ (ppo.py:18-59). */
int32_t ddrl_ctx_create(const ddrl_config* cfg, float* params, float* grads, float* adam_m,
                        float* adam_v, void* workspace, int64_t workspace_bytes, ddrl_ctx** out);
int32_t ddrl_ctx_destroy(ddrl_ctx* ctx);

/* Tell the context that `params` was rewritten by the caller (load_state_dict /
 * updatenn_by_redis, USTC_lab/nn/base.py:68-95): derived weight layouts are rebuilt lazily. */
int32_t ddrl_params_changed(ddrl_ctx* ctx);

/* Adam step counter (torch keeps it in optimizer state; not saved by the reference's
 * checkpoints, backward.py:208-209). */
int32_t ddrl_get_step(const ddrl_ctx* ctx, int64_t* step);
int32_t ddrl_set_step(ddrl_ctx* ctx, int64_t step);

/* PPO.forward (ppo.py:72-75) + the acting glue of ForwardThread.run (forward.py:128-149).
 *   act_in == NULL : sample  action ~ Categorical(probs)  with the counter-based stream
 *                    u = U(seed, stream, sample_index)  and inverse-CDF over p_hat; write the
 *                    action (as float, like `.to(tensortype)`) to action_out.
 *   act_in != NULL : evaluate log-prob of the given actions (PPO.forward(states, act)).
 * Outputs (any may be NULL except value/probs): probs [n,A] = softmax output (what play_mode
 * returns, actor.py:94-96); value [n]; logp_out [n] = log(clamp(p_hat[a], eps, 1-eps)). */
int32_t ddrl_forward(ddrl_ctx* ctx, const uint8_t* frames, int32_t n, const float* act_in,
                     uint64_t seed, uint64_t stream_id, float* probs, float* value,
                     float* action_out, float* logp_out, void* stream);

/* ddrl_forward on frames read where they lie (additive: ABI 3): instead of a contiguous [n][C][84][84], `planes` is a plane base
 * pointer with n_planes planes of 7,056 bytes behind it and `tab` (int32 [n][4] on the device, from ddrl_op_frame_table_planes /
 * ddrl_op_frame_table_stacks / ddrl_op_frame_slot below) names, for every sample of the call, the plane that holds each of its
 * channels.  The kernels that read the frames (the fused acting kernel up to 512 samples, the conv1 forward above) clamp every entry
 * to [0, n_planes): whatever the table holds, nothing outside [planes, planes + n_planes * 7056) is read.  Same arithmetic on the
 * same bytes: the outputs, the features ddrl_last_features returns and, with ddrl_debug_keep_activations, a1 / a2 are bit-identical to
 * ddrl_forward on the materialised stacks; the context is left as ddrl_forward leaves it.  planes 16-byte aligned, tab 4-byte aligned
 * with n * 4 entries, 1 <= n_planes <= INT64_MAX / 7056; otherwise DDRL_ERR_INVALID_ARG (checked before anything touches the context
 * or HIP). */
int32_t ddrl_forward_indexed(ddrl_ctx* ctx, const uint8_t* planes, int64_t n_planes, const int32_t* tab, int32_t n, const float* act_in,
                             uint64_t seed, uint64_t stream_id, float* probs, float* value, float* action_out, float* logp_out,
                             void* stream);

/* torch.distributions.Categorical(probs) derived quantities (actor.py:97 + forward.py:137-138,
 * ppo.py:106): p_hat = p/sum(p), logits = log(clamp(p_hat, eps, 1-eps)), entropy. */
int32_t ddrl_categorical_stats(const float* probs, int32_t n, int32_t n_actions, float* p_hat,
                               float* logits, float* entropy, void* stream);

/* dist.sample() (forward.py:137) for an existing probs tensor: fresh inverse-CDF draws with the
 * counter-based stream U(seed, stream_id, i); logp_out may be NULL. */
int32_t ddrl_categorical_sample(const float* probs, int32_t n, int32_t n_actions, uint64_t seed,
                                uint64_t stream_id, float* action_out, float* logp_out, void* stream);

/* Encoder outputs of the last ddrl_forward / ddrl_ppo_iter call: h[e][i][512], e = 0 actor,
 * 1 critic (AtariPreNet.forward, atari_encoder.py:25-32).  Copies n*512 floats each. */
int32_t ddrl_last_features(ddrl_ctx* ctx, int32_t n, float* h_actor, float* h_critic, void* stream);

/* Agents._accumulate_rewards (USTC_lab/agent/agent.py:124-140), one value head.
 *   values [T+1, N] (row T = bootstrap), rewards [T, N], dones uint8 [T, N]
 *   adv [T, N], ret [T, N]   (ret = old value + advantage; no advantage normalisation). */
int32_t ddrl_gae(const float* values, const float* rewards, const uint8_t* dones, int32_t T,
                 int32_t N, float gamma, float landa, float* adv, float* ret, void* stream);

/* Status.update_reward_status (USTC_lab/agent/statistics.py:118-123) over the T steps of one rollout, on the device: per env
 *   rewards_sum += r_t;  rewards_episode = rewards_episode * (1 - d_t) + rewards_sum * d_t;  rewards_sum *= (1 - d_t)
 * in the reference's operation order.  rewards [T, N], dones uint8 [T, N]; rewards_sum / rewards_episode [N] are read and
 * written (state across rollouts; zero them once); trace [T, N] (may be NULL) receives rewards_episode after every step;
 * episodes_finished int32 [N] (may be NULL) is increased by the number of dones. */
int32_t ddrl_episode_returns(const float* rewards, const uint8_t* dones, int32_t T, int32_t N, float* rewards_sum,
                             float* rewards_episode, float* trace, int32_t* episodes_finished, void* stream);

/* FrameStackWrapper.step / .reset (USTC_lab/env/gym_env/wrapper/warputils.py:112-131) on the device: the stacked observation of
 * the next step from the current stack, ONE new frame per env and an optional per-env reset flag, in one streaming launch:
 *   next[i][c] = newest[i]     for every c, when reset && reset[i] != 0   (.reset, :127-131, reached through NeverStopWrapper.step, :392-397)
 *              = prev[i][c+1]  for c <  channels-1                        (deque append, :118-121: the oldest plane drops out)
 *              = newest[i]     for c == channels-1                        (the newest plane is the LAST channel, :123-125)
 *   prev / next uint8 [n, channels, 84, 84], newest uint8 [n, 84, 84], reset uint8 [n] or NULL; channels 1..4 (1: next = newest,
 *   prev is not read).  prev, newest and next 16-byte aligned; next overlaps neither prev nor newest.  Needs no context, allocates
 *   nothing, asynchronous on `stream`; the argument checks run before anything touches HIP.  Added after round 6 (additive: ABI 3). */
int32_t ddrl_frame_stack_push(const uint8_t* prev, const uint8_t* newest, const uint8_t* reset, int32_t n, int32_t channels,
                              uint8_t* next, void* stream);

/* One iteration of the loss + backward half of PPO.learn (ppo.py:82-126, non-shared branch):
 * forward both encoders on B samples, dual-clip surrogate / value / entropy terms, backward
 * into the grad arena.  Gradients and loss sums are scaled by 1/B_global so that a SUM over
 * data-parallel ranks equals the full-batch mean (B_global == B on one GPU).
 * grads[n_params + 0..2] receive this rank's share of (actor_loss, v_loss, entropy). */
int32_t ddrl_ppo_iter(ddrl_ctx* ctx, const uint8_t* frames, const float* actions,
                      const float* old_logps, const float* advs, const float* rets, int32_t B,
                      int64_t B_global, void* stream);

/* ddrl_ppo_iter on frames read where they lie (additive: ABI 3): instead of a contiguous [B][C][84][84], `planes` is a plane base
 * pointer with n_planes planes of 7,056 bytes behind it and `tab` (int32 [B][4] on the device, from ddrl_op_frame_table_planes /
 * ddrl_op_frame_table_stacks below) names, for every sample of the call, the plane that holds each of its channels.  The conv1 kernels
 * clamp every entry to [0, n_planes): whatever the table holds, nothing outside [planes, planes + n_planes * 7056) is read.  Same
 * arithmetic on the same bytes: gradients, statistics, activations and sign masks are bit-identical to ddrl_ppo_iter on the materialised
 * frames, and ddrl_ppo_diag, the gradient buckets and ddrl_clip_adam_step work after it exactly as after ddrl_ppo_iter.
 * planes 16-byte aligned, tab 4-byte aligned with B * 4 entries, n_planes >= 1; otherwise DDRL_ERR_INVALID_ARG (checked before anything
 * touches the context or HIP). */
int32_t ddrl_ppo_iter_indexed(ddrl_ctx* ctx, const uint8_t* planes, int64_t n_planes, const int32_t* tab, const float* actions,
                              const float* old_logps, const float* advs, const float* rets, int32_t B, int64_t B_global, void* stream);

/* The sums of ddrl_op_heads_diag (below; sums8 = 8 doubles of device memory, overwritten) on the features the last ddrl_ppo_iter left
 * in the context, i.e. for the policy that iteration's loss was evaluated with.  Run between ddrl_ppo_iter and ddrl_clip_adam_step;
 * reads only, so gradients and statistics are untouched.  DDRL_ERR_INVALID_ARG when B is not that call's B (or no ddrl_ppo_iter
 * came last). */
int32_t ddrl_ppo_diag(ddrl_ctx* ctx, const float* actions, const float* old_logps, const float* rets, int32_t B, double* sums8,
                      void* stream);

/* clip_grad_norm_(all params, clip_grad_norm) + actor Adam + critic Adam (ppo.py:125-129).
 * Run after the (optional) all-reduce of the grad arena.  grads[n_params + 4] <- global grad
 * norm, grads[n_params + 5] <- clip coefficient, grads[n_params + 3] <- total loss. */
int32_t ddrl_clip_adam_step(ddrl_ctx* ctx, void* stream);

/* ---- multi-GPU: one process per GPU, env shards, full parameter / Adam replica per rank.
 * The reference has no such path (USTC_lab/server/backward.py:167 "TODO support mutil GPU CARD").  A communicator wraps
 * an RCCL communicator (librccl is resolved with dlopen at first use; DDRL_ERR_UNSUPPORTED when it is absent):
 * rank 0 calls ddrl_comm_unique_id and hands the 128 bytes to the other ranks by any out-of-band means (a file, a TCP
 * socket, MPI, torchrun's store), then every rank calls ddrl_comm_create.
 *   ddrl_params_broadcast : make the replicas bit-identical at start-up (weights of `root`)
 *   ddrl_grad_allreduce   : SUM all-reduce of the flat gradient arena + DDRL_STATS_FLOATS loss tail (13,487,420 B for the
 *                           default net), between ddrl_ppo_iter (which scaled everything by 1/B_global) and
 *                           ddrl_clip_adam_step: every rank then holds the full-batch mean gradient and loss shares, the clip
 *                           sees the global norm (ppo.py:126) and the replicas stay in step.
 * All calls are asynchronous on `stream`. */
int32_t ddrl_comm_unique_id(uint8_t* out128);
/* Which librccl the library resolved (file path of the ncclAllReduce symbol, NUL-terminated into path_out[cap]) and its version code
 * (ncclGetVersion); diagnostics only (bench.py --preflight), no communicator or GPU needed.  Added in round 6 (additive: ABI 3). */
int32_t ddrl_comm_info(char* path_out, int64_t cap, int32_t* version_out);
int32_t ddrl_comm_create(const uint8_t* id128, int32_t rank, int32_t world, ddrl_comm** out);
int32_t ddrl_comm_destroy(ddrl_comm* comm);
int32_t ddrl_allreduce_f32(ddrl_comm* comm, float* buf, int64_t count, void* stream);
int32_t ddrl_broadcast_f32(ddrl_comm* comm, float* buf, int64_t count, int32_t root, void* stream);
int32_t ddrl_grad_allreduce(ddrl_ctx* ctx, ddrl_comm* comm, void* stream);
/* The same reduction in LAYER BUCKETS that overlap the backward.  After ddrl_grad_buckets_enable every
 * ddrl_ppo_iter records one event per bucket on its stream, in completion order: 0 head layers + loss tail, 1 conv1, 2 dense
 * (95 % of the bytes; ready before the conv3 / conv2 weight gradients run), 3 conv3, 4 conv2.  ddrl_grad_allreduce_overlapped
 * makes `comm_stream` wait for each event and reduces the bucket's ranges there, then makes `compute_stream` wait for the last
 * one: only the small conv2 bucket is exposed.  Call it right after ddrl_ppo_iter (it does not block the host).
 * ddrl_grad_bucket_info / _wait expose the ranges (offset, count in floats; up to two per bucket) and the stream wait, for
 * hosts that reduce through another communicator (torch.distributed in the Python mirror). */
int32_t ddrl_grad_buckets_enable(ddrl_ctx* ctx);
int32_t ddrl_grad_bucket_count(const ddrl_ctx* ctx, int32_t* n);
int32_t ddrl_grad_bucket_info(const ddrl_ctx* ctx, int32_t bucket, int64_t* offsets2, int64_t* counts2, int32_t* n_ranges);
int32_t ddrl_grad_bucket_wait(ddrl_ctx* ctx, int32_t bucket, void* stream);
/* Ordering against the compute stream AT THE CALL (round 4).  ddrl_grad_buckets_begin records an event on `compute_stream`;
 * *fresh = 1 when a ddrl_ppo_iter has recorded every bucket event since the previous reduction.  Otherwise (gradients from
 * another producer, accumulation, a retried iteration) the bucket events are stale: `comm_stream` is made to wait for the
 * call-time event at once and the host must NOT rely on ddrl_grad_bucket_wait.  ddrl_grad_bucket_wait_last makes `comm_stream`
 * wait for the call-time event; hosts issue it in front of the last bucket.  ddrl_grad_allreduce_overlapped does both itself. */
int32_t ddrl_grad_buckets_begin(ddrl_ctx* ctx, void* comm_stream, void* compute_stream, int32_t* fresh);
int32_t ddrl_grad_bucket_wait_last(ddrl_ctx* ctx, void* comm_stream);
int32_t ddrl_grad_allreduce_overlapped(ddrl_ctx* ctx, ddrl_comm* comm, void* comm_stream, void* compute_stream);
int32_t ddrl_params_broadcast(ddrl_ctx* ctx, ddrl_comm* comm, int32_t root, void* stream);

/* float32(uint8/255.0) for all 256 byte values, computed with the conv1 loader's arithmetic
 * (reference: warputils.py:300 divides in float64, forward.py:102-104 casts to float32). */
int32_t ddrl_u8_table(float* out256, void* stream);

/* Diagnostic view into the workspace, for parity tests of intermediate tensors:
 * which = 0 a1, 1 a2, 2 a3, 3 h, 4 dz1, 5 dz2, 6 dz3, 7 dh (all [e][max_batch][...], e stride
 * returned in floats), 8 dlogits [B,A], 9 dvalue [B]; 10 / 11 / 12: the sign masks of a1 / a2 / a3 that
 * the forward writes for the backward's leaky-ReLU decisions (32-bit words behind the float pointer,
 * bit set = activation not positive; m1 [e][max_batch * 400 columns], bit per output channel;
 * m2 [e][max_batch][81 pixels][2], m3 [e][max_batch][49 pixels][2], bit per channel of a lane half).
 * The backward runs on per-sample NORMALISED gradients: 4..7 hold the true per-sample gradient divided by the
 * power of two g_s = 2^floor(log2 max|dh_s|); 13 = g_s [e][max_batch].  14 = the running maxima / bounds behind
 * the fp16 plane scales, [slot][encoder] (e stride 1). */
int32_t ddrl_debug_buffer(ddrl_ctx* ctx, int32_t which, float** ptr, int64_t* enc_stride);
/* ddrl_forward of at most 512 samples runs conv1-conv3 in one kernel that keeps a1 / a2 on chip (csrc/act.hip); buffers 0 and 1
 * then hold nothing of that call and ddrl_debug_buffer answers DDRL_ERR_UNSUPPORTED for them.  on = 1: the same kernel also
 * stores a1 / a2 (for tests that look at them; outputs are bit-identical either way).  Training launches always store them. */
int32_t ddrl_debug_keep_activations(ddrl_ctx* ctx, int32_t on);

/* ---- pinned-host ring: replaces the Redis LPUSH/BRPOP shuttle of frames between env workers
 * and the learner (USTC_lab/agent/multiqueue.py:83-130, server/backward.py:145-151). --------- */
int32_t ddrl_ring_create(int64_t slot_bytes, int32_t n_slots, ddrl_ring** out);
int32_t ddrl_ring_destroy(ddrl_ring* ring);
/* Producer: get the next free pinned slot (blocks up to timeout_ms, DDRL_ERR_TIMEOUT). */
int32_t ddrl_ring_acquire(ddrl_ring* ring, void** slot_host, int32_t timeout_ms);
int32_t ddrl_ring_commit(ddrl_ring* ring);
/* Consumer: hipMemcpyAsync the oldest committed slot to dst (device) on `stream`; the slot is
 * recycled when the copy has completed. */
int32_t ddrl_ring_pop_to_device(ddrl_ring* ring, void* dst, int64_t bytes, void* stream, int32_t timeout_ms);
int32_t ddrl_ring_pending(ddrl_ring* ring, int32_t* n_committed);

/* ---- EasyBytes wire codec, host memory only -------------------
 * Byte-exact with USTC_lab/data/easybytes.py: array record = >h dtype code (1 u8, 2 f16, 3 f32,
 * 4 f64), >I count, >I ndim, ndim x >I dims, raw payload (:21-26,:63-75); forward-states message =
 * >Q payload length, 4 x >H ip, >I process_env_id, arrays (:141-149); backward blob = >Q len +
 * states arrays, >Q len + other-4 arrays, marshal tail (:151-162). */
typedef struct ddrl_eb_array {
  int32_t dtype, ndim;
  int64_t dims[8];
  int64_t count;
  int64_t data_offset; /* of the raw payload inside the scanned buffer */
  int64_t nbytes;
} ddrl_eb_array;
typedef struct ddrl_eb_msg {
  int32_t ip[4];
  uint32_t process_env_id;
  int64_t payload_offset, payload_len;
} ddrl_eb_msg;
int32_t ddrl_eb_array_bytes(int32_t dtype, int32_t ndim, const int64_t* dims, int64_t* nbytes);
int32_t ddrl_eb_encode_array(int32_t dtype, int32_t ndim, const int64_t* dims, const void* data,
                             uint8_t* out, int64_t cap, int64_t* written); /* encode_data, one array */
int32_t ddrl_eb_scan(const uint8_t* buf, int64_t len, ddrl_eb_array* out, int32_t cap, int32_t* n); /* decode_data */
int32_t ddrl_eb_forward_header(const int32_t ip[4], uint32_t process_env_id, uint64_t payload_len, uint8_t* out20);
int32_t ddrl_eb_scan_forward_states(const uint8_t* buf, int64_t len, ddrl_eb_msg* out, int32_t cap, int32_t* n);
/* Frames (array `state_index`) of every message of a batched forward-states item -> contiguous
 * uint8 in dst (e.g. a pinned ring slot); float payloads hold uint8/255.0 and are mapped back
 * exactly with round(x*255).  Replaces decode_forward_states + state2tensor for the frames. */
int32_t ddrl_eb_frames_to_u8(const uint8_t* buf, int64_t len, int32_t state_index, uint8_t* dst,
                             int64_t dst_cap, int64_t* n_samples, int64_t* sample_elems);
int32_t ddrl_eb_scan_backward(const uint8_t* buf, int64_t len, int64_t* states_off, int64_t* states_len,
                              int64_t* other_off, int64_t* other_len, int64_t* tail_off);
int32_t ddrl_eb_put_u64(uint64_t v, uint8_t* out8); /* big-endian >Q */

/* ---- measurement hooks (bench.py): HIP-event timing on the caller's stream -------------- */
int32_t ddrl_timer_create(void** timer);
int32_t ddrl_timer_destroy(void* timer);
int32_t ddrl_timer_start(void* timer, void* stream);
int32_t ddrl_timer_stop(void* timer, void* stream);
int32_t ddrl_timer_elapsed_ms(void* timer, float* ms); /* synchronises on the stop event */

/* Enable per-kernel HIP-event timing (diagnostic; off by default): on = 1 inside ddrl_ppo_iter,
 * ddrl_clip_adam_step and ddrl_forward; on = 2 not inside ddrl_forward, whose launches last tens of
 * microseconds and would be slowed by about a quarter by the event records around them; on = 0 off.
 * names/ms arrays are filled up to `cap` entries; returns the count in *n. */
int32_t ddrl_profile_enable(ddrl_ctx* ctx, int32_t on);
int32_t ddrl_profile_read(ddrl_ctx* ctx, char (*names)[48], float* ms, int32_t* calls, int32_t cap, int32_t* n);

/* ------------------------------------------------------------------------------------------
 * Operator-level entry points for the encoders outside the Atari fast path.
 *
 * The reference builds its other networks from torch modules: NavPreNet / NavPedPreNet /
 * NavPreNet1D (USTC_lab/nn/nav_encoder.py:12-128: Conv2d 3x3/5x5/7x7 + ReLU + max_pool2d(2),
 * Conv1d, Linear(+ReLU), torch.cat) and MLPPreNet (USTC_lab/nn/mlp_encoder.py:12-29).  Each
 * ddrl_op_* below replaces one of those torch operators (forward and the autograd backward it
 * implies) on caller-owned device buffers; the Python host composes them exactly where the
 * reference composes the torch modules (ddrl4nav_amd/nn/generic.py).  All tensors are fp32,
 * NCHW-dense inside a sample; `*_sn` are sample strides in floats (0 = dense).
 * ------------------------------------------------------------------------------------------ */
typedef struct ddrl_conv_desc {
  int32_t n;               /* samples                                                     */
  int32_t cin, h, w;       /* input  [n][cin][h][w]   (Conv1d: h = 1)                     */
  int32_t cout, kh, kw;    /* weight [cout][cin][kh][kw]  (torch layout)                  */
  int32_t stride;          /* 1, 2 or 4, both directions                                  */
  int32_t pad_h, pad_w;    /* zero padding                                                */
  int64_t in_sn, out_sn;   /* sample strides of input / output, 0 = dense                 */
} ddrl_conv_desc;

int32_t ddrl_op_conv_out_shape(const ddrl_conv_desc* d, int32_t* oh, int32_t* ow);
/* Derived weight layouts + index tables of one layer (rebuilt whenever the weights change; the size does not depend on d->n).
 * `packed` is READ-ONLY for every later call (ABI 3; ABI 2 kept per-launch scratch inside it).  The heavy nav layers (64->128 5x5 @22,
 * 128->256 3x3 @10, 64->128 3x3 @24, 128->256 3x3 @12) run as fp16 plane products on the 16-bit matrix pipe (csrc/pconv.hip) and need
 * one float of scratch per sample for the per-sample plane scales of a launch that is not handed its scales: `scales_scratch` of
 * ddrl_op_conv_forward / _dgrad / _forward_pool / _dgrad_pooled, ddrl_op_conv_scratch_floats(d) floats for a launch of d->n samples
 * (0 for layers that need none: NULL is accepted then, and whenever in_amax / dpool_amax are given).  One launch per scratch buffer
 * at a time.  The plane kernels need 16-byte aligned tensors and sample strides that are multiples of 4 floats; other views of the same
 * layers run on the generic gather kernels (csrc/gconv.hip, f32-input MFMA) like every geometry without a specialised kernel. */
int32_t ddrl_op_conv_pack_floats(const ddrl_conv_desc* d, int64_t* floats);
int32_t ddrl_op_conv_pack(const ddrl_conv_desc* d, const float* w, float* packed, void* stream);
int32_t ddrl_op_conv_scratch_floats(const ddrl_conv_desc* d, int64_t* floats);
/* out = act(conv2d(in, w) + bias); act: 0 none, 1 ReLU        (torch.nn.Conv2d / Conv1d + F.relu) */
int32_t ddrl_op_conv_forward(const ddrl_conv_desc* d, const float* in, const float* packed, const float* bias,
                             int32_t act, float* out, float* scales_scratch, float* out_amax, void* stream);
/* din = d(loss)/d(in) given dz = d(loss)/d(pre-activation output) */
/* Conv2d + ReLU + max_pool2d(2) in ONE launch (round 4), for the layers whose kernels pool in their epilogue -- NavPreNet1D's three
 * (3->64 7x7 @48, 64->128 5x5 @22, 128->256 3x3 @10): pooled [n][cout][oh/2][ow/2] (dense) and one decision byte per window as
 * ddrl_op_maxpool2_forward_idx leaves it (ddrl_op_maxpool2_backward_idx turns d(pooled) + code into d(pre-activation)); the
 * full-resolution activations are never written.  DDRL_ERR_UNSUPPORTED for every other layer: run ddrl_op_conv_forward and
 * ddrl_op_maxpool2_forward_idx instead.  `in` 16-byte aligned, sample stride a multiple of 4 floats. */
int32_t ddrl_op_conv_forward_pool(const ddrl_conv_desc* d, const float* in, const float* packed, const float* bias, float* pooled,
                                  uint8_t* code, const float* in_amax, float* scales_scratch, float* out_amax, void* stream);
/* PER-SAMPLE MAGNITUDES (`*_amax`, ABI 3).  The fp16-plane kernels scale every sample (dense layers: every row) by a power of two taken
 * from its largest magnitude.  What travels between operators is that magnitude itself -- n floats, amax[b] >= max |x[b][:]| (any upper
 * bound is valid; the tighter, the more bits the sample keeps) --, and it comes from the PRODUCER of the tensor wherever there is one:
 *   out_amax / din_amax (outputs, may be NULL): the operator RAISES amax[b] to the largest |value| it writes for sample b (an atomic
 *     maximum on the bit pattern: deterministic, and several operators may raise the same array -- the row tiles of one launch, or
 *     the layers that fill the slices of a torch.cat buffer).  The CALLER zeroes the array before the first producer runs.
 *   in_amax / dpool_amax / dout_amax (inputs, may be NULL): the magnitudes of the tensor the operator reads; NULL = the operator runs
 *     its own pre-pass over the tensor (a full read of it: ~12 % of a robot_nav PPO iteration when every operator did that).
 * ddrl_op_sample_amax (x: n samples of `elems` floats at stride sn) and ddrl_op_row_amax (x [n][ld], `width` columns; accumulate != 0:
 * raise instead of overwrite) are the stand-alone pre-passes for tensors that arrive from elsewhere.  The magnitudes of d(pooled) bound
 * those of the routed gradient.  ddrl_op_conv_pooled_uses_scales: 1 for the layers that read in_amax / dpool_amax (the first layer of a
 * nav encoder finds its scales inside its kernels). */
int32_t ddrl_op_sample_amax(const float* x, int64_t sn, int32_t elems, int32_t n, float* amax, void* stream);
int32_t ddrl_op_conv_pooled_uses_scales(const ddrl_conv_desc* d);
int32_t ddrl_op_conv_has_forward_pool(const ddrl_conv_desc* d);  /* 1 when ddrl_op_conv_forward_pool serves the layer, else 0 (host only) */
/* The backward of the same layers straight from d(pooled) [n][cout][oh/2][ow/2] and the decision bytes: the kernels form
 * d(pre-activation) while they stage it (the pooled gradient at each window's first maximum under the ReLU's sign, zero elsewhere --
 * what ddrl_op_maxpool2_backward_idx would write), so the full-resolution gradient is neither written nor read.  Same layers as
 * ddrl_op_conv_forward_pool (the 3-channel first layer has no data gradient: DDRL_ERR_UNSUPPORTED); dpool 16-byte aligned, dense. */
int32_t ddrl_op_conv_dgrad_pooled(const ddrl_conv_desc* d, const float* dpool, const uint8_t* code, const float* packed, float* din,
                                  const float* dpool_amax, float* scales_scratch, float* din_amax, void* stream);
int32_t ddrl_op_conv_wgrad_pooled(const ddrl_conv_desc* d, const float* in, const float* dpool, const uint8_t* code, const float* packed,
                                  float* ws, float* dw, float* db, const float* in_amax, const float* dpool_amax, void* stream);
int32_t ddrl_op_conv_dgrad(const ddrl_conv_desc* d, const float* dz, const float* packed, float* din, float* scales_scratch, void* stream);
/* dw [cout][cin][kh][kw], db [cout] (overwritten); `ws` = split-K scratch of ddrl_op_conv_ws_floats.
 * Requires oh*ow >= 32. */
int32_t ddrl_op_conv_ws_floats(const ddrl_conv_desc* d, int64_t* floats);
int32_t ddrl_op_conv_wgrad(const ddrl_conv_desc* d, const float* in, const float* dz, const float* packed, float* ws,
                           float* dw, float* db, void* stream);

/* F.max_pool2d(x, 2, stride=2) over `planes` = n*c planes of h x w (both even), and its backward
 * fused with the ReLU that precedes it in the reference (`a` = relu(conv) at full resolution):
 * dz = dpool routed to the first maximum of each window (PyTorch scan order), zero where a <= 0.
 * The full-resolution pointers (in, a, dz) must be 8-byte aligned (INVALID_ARG otherwise). */
int32_t ddrl_op_maxpool2_forward(const float* in, int64_t planes, int32_t h, int32_t w, float* out, void* stream);
int32_t ddrl_op_maxpool2_relu_backward(const float* a, const float* dpool, int64_t planes, int32_t h, int32_t w,
                                       float* dz, void* stream);

/* The same pair with the decisions kept in ONE BYTE per window (round 4): the forward also writes code[planes][h/2][w/2] (bits 0-1 =
 * position of the first maximum in PyTorch's scan order, bit 2 = the maximum is positive, i.e. the ReLU in front of the pool lets the
 * gradient through); the backward reads dpool and the code instead of the full-resolution activations (1.31 instead of 2.25 tensor
 * sizes of HBM traffic) and writes the same dz as ddrl_op_maxpool2_relu_backward.  Same alignment rule for `in`; dz 16-byte aligned. */
int32_t ddrl_op_maxpool2_forward_idx(const float* in, int64_t planes, int32_t h, int32_t w, float* out, uint8_t* code, void* stream);
int32_t ddrl_op_maxpool2_backward_idx(const float* dpool, const uint8_t* code, int64_t planes, int32_t h, int32_t w, float* dz,
                                      void* stream);

/* nn.Linear(K, N) (+ReLU): out[b][:] = act(in[b][:K] W^T + bias).  Leading dimensions are
 * multiples of 4 floats (>= K rounded up to 4), pointers 16-byte aligned, N a multiple of 4.
 * Columns [K, ld_in) of `in` and [N, ld_dout) of `dout` belong to the caller: padding, or the neighbouring slices of a wider
 * torch.cat buffer.  The kernels may load them; they must hold finite values of any size, and no result depends on them (the
 * f32-input kernels multiply them by zero weights, the plane kernels keep them out of the planes, the weight gradient drops
 * the output columns they feed).  mask_src is read in columns [0, K) only.
 * wt / wn = derived layouts written by ddrl_op_linear_pack (sizes from ddrl_op_linear_pack_floats). */
int32_t ddrl_op_linear_pack_floats(int32_t K, int32_t N, int64_t* wt_floats, int64_t* wn_floats);
int32_t ddrl_op_linear_pack(const float* w, int32_t K, int32_t N, float* wt, float* wn, void* stream);
/* ws: scratch of ddrl_op_linear_ws_floats(max n, K, N) floats, shared by the three operators of a layer (they run one after the other)
 * and large enough for every launch of n <= max n rows.  Each launch lays it out from offset 0 (S = its split count):
 *   forward        f32-input kernels: S * n * N split-K partials (lets small n x N problems split K over workgroups);
 *                  plane kernels: n row scales (the pre-pass when in_amax == NULL) rounded up to 64 floats, then the partials.
 *                  NULL: the f32-input kernels in a single pass.
 *   data gradient  plane kernels: n row scales (the pre-pass when dout_amax == NULL).  NULL: the f32-input kernels.
 *   weight grad.   S slabs of N * K + N floats; plane kernels: then n + n row scales (in, dout).  Required.
 * in_amax / dout_amax: layers of K >= 128, N >= 64 in launches of n >= 128 rows (ddrl_op_linear_uses_planes: 1) run as fp16 plane
 * products and scale every ROW of `in` / `dout` by a power of two from the row's largest magnitude ("per-sample magnitudes" above: from
 * the tensor's producer, from ddrl_op_row_amax, or NULL = the operator's own pre-pass).  The forward and the weight gradient read the
 * same `in`, the data and the weight gradient the same `dout`: one array per tensor serves both. */
int32_t ddrl_op_linear_uses_planes(int32_t n, int32_t K, int32_t N);
int32_t ddrl_op_row_amax(const float* x, int64_t ld, int32_t width, int32_t n, float* amax, int32_t accumulate, void* stream);
int32_t ddrl_op_linear_forward(const float* in, int64_t ld_in, const float* wt, const float* bias, int32_t act,
                               float* out, int64_t ld_out, int32_t n, int32_t K, int32_t N, float* ws, const float* in_amax,
                               void* stream);
/* din[b][k] = [mask_src[b][k] > 0 or mask_src == NULL] * sum_n dout[b][n] W[n][k]; mask_src is the
 * (ReLU) output of the layer that produced `in`.  ws: the same scratch as the forward's (layout above).
 * din_amax (may be NULL): raised to the largest |din[b][k]| over the columns amax_lo <= k < amax_hi (amax_hi <= 0: all K columns;
 * amax_lo a multiple of 4) -- a slice when the consumer reads a slice of din (the layers behind a torch.cat). */
int32_t ddrl_op_linear_dgrad(const float* dout, int64_t ld_dout, const float* wn, const float* mask_src, int64_t ld_mask,
                             float* din, int64_t ld_din, int32_t n, int32_t K, int32_t N, float* ws, const float* dout_amax,
                             float* din_amax, int32_t amax_lo, int32_t amax_hi, void* stream);
int32_t ddrl_op_linear_ws_floats(int32_t n, int32_t K, int32_t N, int64_t* floats);
/* dw [N][K] = dout^T in, db [N] = column sums of dout (overwritten) */
int32_t ddrl_op_linear_wgrad(const float* in, int64_t ld_in, const float* dout, int64_t ld_dout, float* ws, float* dw,
                             float* db, int32_t n, int32_t K, int32_t N, const float* in_amax, const float* dout_amax, void* stream);

/* Actor / critic heads on 512-wide encoder features (AC_INPUT_DIM, config_nn.py:23) with the PPO
 * loss block and its backward, for nets assembled from the operators above.  `continuous` selects
 * GaussionActor (USTC_lab/nn/actor.py:43-70: mu = Linear(h), std = exp(log_std), Normal, log-prob
 * summed over action dims) instead of CategoricalActor (actor.py:73-101).  Offsets are positions
 * (in floats) of the head parameters inside the caller's flat parameter / gradient arenas. */
typedef struct ddrl_heads_desc {
  int32_t continuous;  /* 0 = CategoricalActor (A <= 18), 1 = GaussionActor (D <= 8)          */
  int32_t n_actions;   /* ACTION_OUTPUT_DIM                                                   */
  int32_t shared;      /* SHARE_CNN_NET: both heads read h_actor, total_loss is differentiated */
  int32_t reserved;
  int64_t actor_w, actor_b, log_std, critic_w, critic_b; /* log_std: Gaussian only             */
  int64_t n_params;    /* grads[n_params .. +8) receive the loss statistics (see ddrl_ppo_iter) */
} ddrl_heads_desc;

int32_t ddrl_op_heads_ws_floats(const ddrl_heads_desc* d, int32_t max_n, int64_t* floats);
/* h_actor / h_critic: [n][512].  dist_out: probs [n][A] (categorical) or mu [n][D] (Gaussian).
 * act_in == NULL: sample (categorical: inverse CDF on the counter-based uniform stream, as
 * ddrl_forward; Gaussian: mu + std * Box-Muller normal of the same stream); action_out is [n] or [n][D]. */
int32_t ddrl_op_heads_act(const ddrl_heads_desc* d, const float* params, const float* h_actor, const float* h_critic,
                          int32_t n, const float* act_in, uint64_t seed, uint64_t stream_id, float* dist_out, float* value,
                          float* action_out, float* logp_out, void* stream);
/* Loss terms of PPO.learn (ppo.py:82-108) for this shard scaled by 1/B_global, d(loss)/d(h) into
 * dh_actor / dh_critic (shared: both into dh_actor), head parameter gradients and the loss
 * statistics into `grads` (overwritten at the head offsets). */
int32_t ddrl_op_heads_loss(const ddrl_heads_desc* d, const ddrl_config* cfg, const float* params, const float* h_actor,
                           const float* h_critic, int32_t n, const float* actions, const float* old_logps, const float* advs,
                           const float* rets, int64_t B_global, float* dh_actor, float* dh_critic, float* grads, float* ws,
                           void* stream);
/* Diagnostics of a PPO update (the reference has none; added after round 6, additive: ABI 3): how far the policy that the loss is
 * evaluated with has moved from the one that collected the batch, how many samples sit on the flat part of the clipped surrogate, and
 * what the critic explains of the returns.  Read-only on the features / parameters the loss entry points read; per sample
 *   x = logp - old_logp (fp32; logp as ddrl_op_heads_loss differentiates it),  r = exp(x) (fp32),  e = ret - v (double)
 * and sums8[0..8) (DEVICE memory, doubles) =
 *   n,  sum(expm1(x) - x) (the "k3" KL estimator, every term in double and >= 0),  #{r outside [1 - ppo_clip, 1 + ppo_clip]} (the
 *   bounds as fp32, the test ppo_surrogate applies),  sum(ret),  sum(ret^2),  sum(e),  sum(e^2)  (terms and partial sums in double,
 *   fixed order),  max r.
 * accumulate != 0: added to what sums8 holds (slot 7: the larger), so that micro-batches build one global result.  logp_out /
 * value_out ([n], may be NULL) receive the per-sample log-prob and value.  h_critic is not read when d->shared.  ws =
 * ddrl_op_heads_diag_ws_floats floats (any max_n), 16-byte aligned like h_actor / h_critic; sums8 8-byte aligned.  The argument checks
 * run before anything touches HIP. */
int32_t ddrl_op_heads_diag_ws_floats(const ddrl_heads_desc* d, int32_t max_n, int64_t* floats);
int32_t ddrl_op_heads_diag(const ddrl_heads_desc* d, const ddrl_config* cfg, const float* params, const float* h_actor,
                           const float* h_critic, int32_t n, const float* actions, const float* old_logps, const float* rets,
                           double* sums8, int32_t accumulate, float* logp_out, float* value_out, float* ws, void* stream);
/* clip_grad_norm_ + Adam (two lr groups split at n_actor, or one when shared) on flat arenas;
 * `step` is the 1-based Adam step count; ws = ddrl_op_clip_adam_ws_bytes bytes. */
int32_t ddrl_op_clip_adam_ws_bytes(int64_t* bytes);
int32_t ddrl_op_clip_adam(const ddrl_config* cfg, float* params, float* grads, float* m, float* v, int64_t n_params,
                          int64_t n_actor, int32_t shared, int64_t step, void* ws, void* stream);
/* d[b][k] = 0 where act[b][k] <= 0: ReLU backward for an encoder whose OUTPUT is a ReLU (MLPPreNet) */
int32_t ddrl_op_relu_mask(float* d, int64_t ld_d, const float* act, int64_t ld_act, int32_t n, int32_t width, void* stream);
/* dst[i] += src[i]: gradient accumulation over micro-batches */
int32_t ddrl_op_accumulate(float* dst, const float* src, int64_t count, void* stream);

/* ------------------------------------------------------------------------------------------
 * GAIL (USTC_lab/nn/GAIL.py, nn/ppo.py:61-62,97-107).
 * ------------------------------------------------------------------------------------------ */
/* The Atari encoder on its own, for callers that compose it with other operators (the GAIL discriminator's
 * `pre`, GAIL.py:27,65-66, and a generator whose heads carry an extra critic): AtariPreNet.forward
 * (atari_encoder.py:25-32) into the context's feature buffer and its backward from the context's dh buffer into
 * the context's grad arena (encoder slots only; the head slots are not touched).  The context is created with
 * share_cnn_net = 1; `params` / `grads` point at the encoder's first parameter (prenet.conv1.weight) inside
 * the caller's arenas; adam_m / adam_v may be NULL for such a context (ddrl_clip_adam_step then fails).
 * ddrl_encoder_buffers returns the device addresses of h [max_batch][512] and dh [max_batch][512].
 * ddrl_encoder_backward CONSUMES dh: its rows are rescaled in place by per-sample powers of two (the backward
 * runs on normalised gradients); write dh again before every call. */
int32_t ddrl_encoder_forward(ddrl_ctx* ctx, const uint8_t* frames, int32_t n, void* stream);
int32_t ddrl_encoder_backward(ddrl_ctx* ctx, const uint8_t* frames, int32_t n, void* stream);
int32_t ddrl_encoder_buffers(ddrl_ctx* ctx, float** h, float** dh);

/* One more value head next to the critic (PPO.add_critic, ppo.py:61-62): value[b] = w . h[b] + bias on 512-wide
 * features (Critic.forward, critic.py:14-21).  w [512] / b [1] may sit anywhere in an fp32 arena. */
int32_t ddrl_op_value_head_forward(const float* w, const float* b, const float* h, int64_t ld_h, int32_t n, float* value,
                                   void* stream);
/* Its loss term vlossf(rets, value) (ppo.py:101-103) scaled by 1/B_global: the loss share is ADDED to vloss_accum[0]
 * (= &grads[n_params + 1], so that VLoss / PpoTotalLoss include it, ppo.py:107-108), d(loss)/d(h) is ADDED to dh
 * (run after ddrl_op_heads_loss; `shared` != 0: the gradient carries v_loss_theta, as total_loss.backward() does),
 * dw [512] / db [1] receive the head's own gradient (either may be NULL: the reference never steps this head, see
 * nn/gail.py).  ws: ddrl_op_value_head_ws_floats floats. */
int32_t ddrl_op_value_head_ws_floats(int64_t* floats);
int32_t ddrl_op_value_head_loss(const ddrl_config* cfg, int32_t shared, const float* w, const float* b, const float* h,
                                int64_t ld_h, int32_t n, const float* rets, int64_t B_global, float* dh, int64_t ld_dh, float* dw,
                                float* db, float* vloss_accum, float* ws, void* stream);
/* One term of the discriminator loss (GAIL.py:78-80): loss[0] (+)= sign * sum(score[0:n, 0]) / n_total, and the
 * gradient it seeds: dscore[i][0] = sign / n_total, dscore[i][1..width) = 0 (score / dscore rows are `ld` / `ld_d`
 * floats apart; `width` = padded output width of the last dense layer). */
int32_t ddrl_op_wgan_terms(const float* score, int64_t ld, int32_t n, int64_t n_total, float sign, float* dscore, int64_t ld_d,
                           int32_t width, float* loss, int32_t accumulate, void* stream);
/* out[c] = sum over the n rows of x[:, c] for c < width, accumulated in double and rounded once (bias gradient of a
 * narrow dense layer, e.g. the discriminator's 1-wide score layer). */
int32_t ddrl_op_colsum(const float* x, int64_t ld, int32_t n, int32_t width, float* out, void* stream);
/* torch.nn.utils.clip_grad_norm_(params, max_norm) + torch.optim.RMSprop(lr, alpha, eps).step() (GAIL.py:28,83-84)
 * on flat arenas; grads[n_params + 4] <- grad norm, grads[n_params + 5] <- clip coefficient.  ws: as ddrl_op_clip_adam.
 * alpha is a double: torch casts alpha and (1 - alpha) to float32 separately, and 1 - alpha must be formed in double. */
int32_t ddrl_op_clip_rmsprop(float* params, float* grads, float* square_avg, int64_t n_params, float lr, double alpha, float eps,
                             float max_norm, void* ws, void* stream);

/* ------------------------------------------------------------------------------------------
 * Imitation pre-training (USTC_lab/nn/base.py:109-150, called from server/backward.py:117-129,168-174).  Added after
 * round 6 (additive: ABI 3).
 * ------------------------------------------------------------------------------------------ */
/* The supervised head of Basenn._imitation_learning_classifier (USTC_lab/nn/base.py:131,143,147: CrossEntropyLoss on the
 * logits + loss.backward() through the actor's last layer), on 512-wide encoder features:
 *   logits = h W^T + b;  loss = sum_i -log_softmax(logits_i)[label_i] / n_total;  dlogit = (softmax - onehot) / n_total
 *   dh [n][ld_dh] = sum_j dlogit_j w_j;  dw [A][512] and db [A] (overwritten);
 *   stats[0] = this call's share of the loss, stats[1] = number of samples whose argmax (first maximum) equals the label.
 * h [n][ld_h] and dh are 16-byte aligned with leading dimensions that are multiples of 4 floats (>= 512); w [A][512], b [A],
 * dw, db and stats may sit anywhere in an fp32 arena.  A = n_actions in 2..18 (DDRL_ERR_UNSUPPORTED otherwise).  labels are
 * floats as the reference's reader yields them (data/mimic_exp.py:206-212); a label outside [0, A) contributes no loss and
 * no gradient and is never counted as correct.  log_softmax is z - max - log(sum exp(z - max)).  Deterministic: per-workgroup
 * partial sums in `ws` (ddrl_op_heads_bc_ws_floats(A, max n) floats), reduced in a fixed order by a second launch. */
int32_t ddrl_op_heads_bc_ws_floats(int32_t n_actions, int32_t max_n, int64_t* floats);
int32_t ddrl_op_heads_bc_loss(const float* w, const float* b, int32_t n_actions, const float* h, int64_t ld_h, int32_t n,
                              const float* labels, int64_t n_total, float* dh, int64_t ld_dh, float* dw, float* db, float* stats,
                              float* ws, void* stream);
/* The collation of one shuffled minibatch (the DataLoader of USTC_lab/nn/base.py:128,140-141) on the device:
 *   dst[i][0:row_bytes) = src[idx[i]][0:row_bytes) for i < n, and labels_dst[i] = labels_src[idx[i]] in the same launch
 *   (labels_src / labels_dst: both given or both NULL).
 * src [n_rows][row_bytes] holds the whole demonstration set (uint8 [N, C, 84, 84]: row_bytes = C * 7056); row_bytes is a
 * multiple of 16, src and dst are 16-byte aligned and do not overlap (DDRL_ERR_INVALID_ARG otherwise); idx is int32 on the
 * device.  An index outside [0, n_rows) yields a zero row and label -1; nothing is read out of bounds.  Needs no context,
 * allocates nothing, asynchronous on `stream`; the argument checks run before anything touches HIP. */
int32_t ddrl_op_gather_rows_u8(const uint8_t* src, int64_t n_rows, int64_t row_bytes, const int32_t* idx, int32_t n, uint8_t* dst,
                               const float* labels_src, float* labels_dst, void* stream);

/* ---------------------------------------------------------------------------------------------
 * PPO minibatch epochs (the reference runs full-batch iterations on raw advantages, ppo.py:77-146; added after round 6,
 * additive: ABI 3).  All four need no context, allocate nothing and are asynchronous on `stream`; their argument checks run
 * before anything touches HIP; no atomics, so a repeated call gives the same bits.
 * ------------------------------------------------------------------------------------------ */
/* sums3[0..3) (DEVICE memory, doubles, 8-byte aligned) = n, sum x, sum x^2 of the n floats of x: terms and partial sums in double,
 * per-workgroup partial rows in `ws` folded in index order by a last stage (the scheme of ddrl_op_heads_diag).  accumulate != 0:
 * added to what sums3 holds, so that micro-batches (or ranks) build one result.  ws = ddrl_op_moments_ws_floats(n) floats, 8-byte
 * aligned; x, ws and sums3 do not overlap. */
int32_t ddrl_op_moments_ws_floats(int64_t n, int64_t* floats);
int32_t ddrl_op_moments(const float* x, int64_t n, double* sums3, int32_t accumulate, float* ws, void* stream);
/* The affine pair of (x - x.mean()) / (x.std() + eps) with torch's unbiased std, from the sums of ddrl_op_moments, in double:
 *   mean = S1 / n;  var = max(0, (S2 - S1 * S1 / n) / (n - 1)) for n >= 2, 0 for n < 2;
 *   affine2[0] = (float)mean;  affine2[1] = (float)(1 / (sqrt(var) + eps))
 * sums3 and affine2 (2 floats) are DEVICE memory: the divisor never visits the host.  eps >= 0. */
int32_t ddrl_op_moments_affine(const double* sums3, double eps, float* affine2, void* stream);
/* out[i] = (x[i] - affine2[0]) * affine2[1] for i < n, in fp32: a subtract, then a multiply (never fused).  out == x is allowed;
 * any other overlap of x, affine2 and out is DDRL_ERR_INVALID_ARG. */
int32_t ddrl_op_normalize(const float* x, int64_t n, const float* affine2, float* out, void* stream);
/* The collation of one minibatch of Experience in one launch:
 *   frames_dst[i][0:row_bytes) = frames[idx[i]][0:row_bytes) for i < n   (the rules of ddrl_op_gather_rows_u8: row_bytes a multiple of
 *   16, frames / frames_dst 16-byte aligned, idx int32 on the device),
 *   X_dst[i] = X[idx[i]] for the four float columns X = actions, old_logps, advs, rets ([n_rows] -> [n]; a column is given with its
 *   destination or both are NULL),
 *   adv_affine != NULL (2 floats on the device, needs advs): advs_dst[i] = (advs[idx[i]] - adv_affine[0]) * adv_affine[1], the
 *   arithmetic of ddrl_op_normalize bit for bit.
 * An index outside [0, n_rows) reads nothing and yields a zero frame row and zeros in all four columns.  Nothing that is read (idx
 * and adv_affine included) may overlap anything that is written, nor two destinations one another: DDRL_ERR_INVALID_ARG. */
int32_t ddrl_op_gather_minibatch(const uint8_t* frames, int64_t n_rows, int64_t row_bytes, const int32_t* idx, int32_t n,
                                 uint8_t* frames_dst, const float* actions, const float* old_logps, const float* advs, const float* rets,
                                 float* actions_dst, float* old_logps_dst, float* advs_dst, float* rets_dst, const float* adv_affine,
                                 void* stream);

/* ---------------------------------------------------------------------------------------------
 * Single-frame experience pool: every Atari frame stored ONCE (additive: ABI 3).  Instead of whole stacks
 * [T+1][n_envs][C][84][84], the pool keeps
 *   planes uint8 [hist + T + 1][n_envs][84][84]   row hist + t = the one frame that arrived for step t, hist >= C - 1 history rows
 *   age    uint8 [T + 1][n_envs]                  steps since env i's stack was last reset, saturated at C - 1
 * and channel c of sample b = t * n_envs + i is pool row  hist + t - min(C - 1 - c, age[b], hist + t)  of env i: the observation of
 * FrameStackWrapper (warputils.py:112-131), what ddrl_frame_stack_push writes out.  The last term of the min is a clamp: whatever
 * bytes `age` holds, no row below 0 is read.  Both need no context, allocate nothing and are asynchronous on `stream`; their
 * argument checks run before anything touches HIP; no atomics, so a repeated call gives the same bits.  channels outside 1..4:
 * DDRL_ERR_UNSUPPORTED.
 * ------------------------------------------------------------------------------------------ */
/* age[i] = 0 where reset[i] != 0, else min(prev_age[i] + 1, channels - 1), for i < n.  reset == NULL: no env is reset.
 * prev_age == NULL (legal only together with a reset array): every env is reset.  age overlaps neither input. */
int32_t ddrl_op_frame_age(const uint8_t* prev_age, const uint8_t* reset, int32_t n, int32_t channels, uint8_t* age, void* stream);
/* stacks_dst[j] ([channels][84][84]) = the stack of sample idx[j] (idx int32 on the device), or of sample first + j when idx is NULL
 * (a contiguous minibatch; the acting slot t: first = t * n_envs, n = n_envs), assembled by the rule above, for j < n.  `rows` is
 * the number of pool rows given, rows > hist >= channels - 1; samples are valid in [0, (rows - hist) * n_envs), and `age` and
 * every column given hold that many entries.  The four float columns and adv_affine are those of ddrl_op_gather_minibatch, bit for
 * bit.  A sample outside the valid range reads nothing and yields a zero stack and zeros in all four columns.  planes and
 * stacks_dst are 16-byte aligned, n >= 1; nothing that is read (age, idx and adv_affine included) may overlap anything that is
 * written, nor two destinations one another: DDRL_ERR_INVALID_ARG. */
int32_t ddrl_op_gather_frame_stacks(const uint8_t* planes, int32_t rows, int32_t n_envs, int32_t hist, const uint8_t* age,
                                    int32_t channels, const int32_t* idx, int64_t first, int32_t n, uint8_t* stacks_dst,
                                    const float* actions, const float* old_logps, const float* advs, const float* rets,
                                    float* actions_dst, float* old_logps_dst, float* advs_dst, float* rets_dst, const float* adv_affine,
                                    void* stream);

/* ---------------------------------------------------------------------------------------------
 * Frame tables: where the frames of a training call lie, for ddrl_ppo_iter_indexed (additive: ABI 3).  tab int32 [n][4] on the device:
 * tab[j][c] = index of the 7,056-byte plane, counted from a plane base pointer, that holds channel c of sample j of the call; entries
 * c >= channels repeat entry channels - 1.  Sample j of the call is sample idx[j] (idx int32 on the device), or first + j when idx is
 * NULL.  The four float columns and adv_affine are those of ddrl_op_gather_minibatch, bit for bit: one launch collates a minibatch
 * without touching a frame.  THE ONE DIFFERENCE from the gathers: a sample index outside the valid range is CLAMPED to it before
 * anything is read -- age, the columns and the table entry all use the clamped sample -- where the gathers return zeros for such a
 * sample.  Both need no context, allocate nothing and are asynchronous on `stream`; their argument checks run before anything touches
 * HIP; no atomics, so a repeated call gives the same bits.  channels outside 1..4: DDRL_ERR_UNSUPPORTED.  tab and idx 4-byte aligned,
 * n >= 1, the plane count fits an int32; nothing that is read (age, idx and adv_affine included) may overlap anything that is written,
 * nor two destinations one another: DDRL_ERR_INVALID_ARG.
 * ------------------------------------------------------------------------------------------ */
/* The single-frame pool (above): the rule of ddrl_op_gather_frame_stacks, its clamp against a hostile `age` included:
 *   tab[j][c] = (hist + t - min(channels - 1 - c, age[b], hist + t)) * n_envs + env   for sample b = t * n_envs + env,
 * counted from the pool's `planes` pointer (rows * n_envs planes).  rows > hist >= channels - 1; samples are valid in
 * [0, (rows - hist) * n_envs), and `age` and every column given hold that many entries. */
int32_t ddrl_op_frame_table_planes(int32_t rows, int32_t n_envs, int32_t hist, const uint8_t* age, int32_t channels, const int32_t* idx,
                                   int64_t first, int32_t n, int32_t* tab, const float* actions, const float* old_logps,
                                   const float* advs, const float* rets, float* actions_dst, float* old_logps_dst, float* advs_dst,
                                   float* rets_dst, const float* adv_affine, void* stream);
/* Stacked frames uint8 [n_rows][channels][84][84]: tab[j][c] = b * channels + c, counted from the frames' pointer (n_rows * channels
 * planes); samples are valid in [0, n_rows). */
int32_t ddrl_op_frame_table_stacks(int64_t n_rows, int32_t channels, const int32_t* idx, int64_t first, int32_t n, int32_t* tab,
                                   const float* actions, const float* old_logps, const float* advs, const float* rets,
                                   float* actions_dst, float* old_logps_dst, float* advs_dst, float* rets_dst, const float* adv_affine,
                                   void* stream);
/* One acting step of the single-frame pool in one launch (additive: ABI 3), for ddrl_forward_indexed: the age row of step t and the
 * frame table of its n_envs samples,
 *   age[i]    = 0 where reset[i] != 0, else min(prev_age[i] + 1, channels - 1)            (ddrl_op_frame_age, bit for bit)
 *   tab[i][c] = (hist + t - min(channels - 1 - c, age[i], hist + t)) * n_envs + i          (ddrl_op_frame_table_planes with
 *               first = t * n_envs, n = n_envs and no columns, bit for bit; entries c >= channels repeat entry channels - 1)
 * reset == NULL: no env is reset; prev_age == NULL (legal only together with a reset array): every env is.  prev_age, reset and age
 * hold n_envs bytes, tab n_envs * 4 entries; `rows` is the number of pool rows, rows > hist + t, t >= 0, hist >= channels - 1,
 * rows * n_envs fits an int32.  tab is 16-byte aligned (an env's four entries are one store); age and tab overlap neither input nor
 * one another: DDRL_ERR_INVALID_ARG.  channels outside 1..4: DDRL_ERR_UNSUPPORTED.  Needs no context, allocates nothing, no atomics,
 * asynchronous on `stream`; the argument checks run before anything touches HIP. */
int32_t ddrl_op_frame_slot(int32_t rows, int32_t n_envs, int32_t hist, int32_t channels, int32_t t, const uint8_t* prev_age,
                           const uint8_t* reset, uint8_t* age, int32_t* tab, void* stream);

/* ---------------------------------------------------------------------------------------------
 * PPO update options (the reference has none of them, ppo.py:82-129; additive: ABI 3).  ddrl_config and every
 * entry point above are unchanged: the options arrive through entry points of their own, and with all options off those compute, bit
 * for bit, what the entry points above compute.
 * ------------------------------------------------------------------------------------------ */
typedef struct ddrl_loss_options {
  float value_clip;      /* c > 0: per sample, with e(x) the value-loss element (x^2, halved by the mean, or smooth-L1 with beta 1),
                            d = v - v_old, v_c = v_old + clamp(d, -c, c), the element is max(e(ret - v), e(ret - v_c)); its gradient
                            follows torch.max (a tie splits evenly) and torch.clamp (passes on the closed interval).  0 = off */
  int32_t entropy_split; /* != 0: with two encoders the actor side differentiates actor_loss - ent_loss_theta * entropy (the reference
                            differentiates actor_loss alone there, ppo.py:118-129): the entropy gradient reaches the actor head, the
                            actor's encoder and log_std, nothing else; with a shared prenet total_loss carries the term already and
                            the option changes nothing.  The three statistics and the total are the same either way */
  int32_t reserved[2];   /* must be 0 */
} ddrl_loss_options;

/* One training batch of the Atari context.  tab == NULL: frames_or_planes is the contiguous uint8 [B][C][84][84] of ddrl_ppo_iter and
 * n_planes is not read; otherwise it is the plane base pointer of ddrl_ppo_iter_indexed with n_planes planes behind it and tab its
 * frame table (the same rules: planes 16-byte aligned, tab 4-byte aligned with B * 4 entries, 1 <= n_planes <= INT64_MAX / 7056).
 * old_values [B] = the values the collecting policy predicted: required, 4-byte aligned, when value_clip > 0; not read otherwise. */
typedef struct ddrl_ppo_batch {
  const uint8_t* frames_or_planes;
  int64_t n_planes;
  const int32_t* tab;
  const float *actions, *old_logps, *advs, *rets, *old_values;
} ddrl_ppo_batch;

/* ddrl_ppo_iter / ddrl_ppo_iter_indexed with the options: the same launches, the loss kernel in its option form.  ddrl_ppo_diag, the
 * gradient buckets and ddrl_clip_adam_step work after it exactly as after ddrl_ppo_iter.  value_clip negative, NaN or infinite, a
 * non-zero reserved word, a missing or misaligned old_values under value_clip > 0: DDRL_ERR_INVALID_ARG (every check runs before
 * anything touches the context or HIP). */
int32_t ddrl_ppo_iter_opt(ddrl_ctx* ctx, const ddrl_ppo_batch* batch, const ddrl_loss_options* opt, int32_t B, int64_t B_global,
                          void* stream);
/* ddrl_op_heads_loss with the options, both head families (Gaussian: the entropy term's gradient is -ent_loss_theta / (B D) per
 * log_std entry); old_values [n] as above. */
int32_t ddrl_op_heads_loss_opt(const ddrl_heads_desc* d, const ddrl_config* cfg, const float* params, const float* h_actor,
                               const float* h_critic, int32_t n, const float* actions, const float* old_logps, const float* advs,
                               const float* rets, const ddrl_loss_options* opt, const float* old_values, int64_t B_global,
                               float* dh_actor, float* dh_critic, float* grads, float* ws, void* stream);
/* Overwrite actor_lr, critic_lr, learning_rate and ppo_clip of the context's configuration (learning-rate and clip schedules): the loss
 * kernels, ddrl_ppo_diag and ddrl_clip_adam_step read them at every launch, so the next call of each sees the new values.  Host only,
 * no synchronisation.  A negative or non-finite value: DDRL_ERR_INVALID_ARG, and the context is unchanged. */
int32_t ddrl_set_rates(ddrl_ctx* ctx, float actor_lr, float critic_lr, float learning_rate, float ppo_clip);
/* dst[j] = src[idx[j]] (idx int32 on the device), or src[first + j] when idx is NULL, for j < n: one more float column (old_values)
 * next to the four that the gathers and the frame tables above carry.  src holds n_rows floats; a sample outside [0, n_rows) reads
 * nothing and yields zero.  src, dst and idx 4-byte aligned, dst overlaps neither src nor idx: DDRL_ERR_INVALID_ARG.  Needs no
 * context, allocates nothing, no atomics, asynchronous on `stream`; the argument checks run before anything touches HIP. */
int32_t ddrl_op_gather_f32(const float* src, int64_t n_rows, const int32_t* idx, int64_t first, int32_t n, float* dst, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Running observation and return normalisation (the reference defines RunningMeanStd, warputils.py:83-109, and uses it nowhere;
 * additive: ABI 3).  All five need no context, allocate nothing and are asynchronous on `stream`; their argument
 * checks run before anything touches HIP: a null pointer, a misaligned one (floats 4 bytes, doubles 8), an overlap of anything read
 * with anything written, n < 1, d < 1 or ld < d is DDRL_ERR_INVALID_ARG.  No atomics; a result depends on the arguments and the data
 * alone -- not on the launch geometry, not on whether a pointer allows 16-byte loads -- and a repeated call gives the same bits.
 *   sums   double [1 + 2 d]  n, sum x_j (d entries), sum x_j^2 (d entries): a PENDING batch, additive over calls and over ranks
 *   state  double [1 + 2 d]  count, mean[d], var[d] (population variance); a fresh state is (0, 0..., 1...)
 *   affine float  [2][d]     shift[d], scale[d]
 * ------------------------------------------------------------------------------------------ */
/* sums of the columns [0, d) of x, fp32 [n][ld] (columns [d, ld) are never read): terms and partial sums in double; the rows are cut
 * into slabs whose partial rows go to `ws` (ddrl_op_column_moments_ws_floats(n, d) floats, 8-byte aligned) and are folded in slab
 * order.  accumulate != 0: added to what `sums` holds.  n <= INT64_MAX / 8 and d <= 2^28 in both. */
int32_t ddrl_op_column_moments_ws_floats(int64_t n, int32_t d, int64_t* floats);
int32_t ddrl_op_column_moments(const float* x, int64_t n, int32_t d, int64_t ld, double* sums, int32_t accumulate, float* ws, void* stream);
/* RunningMeanStd.update (warputils.py:94-109) with the pending batch of `sums`, in double, per feature j:
 *   n = sums[0];  bm = S1_j / n;  bv = max(0, S2_j / n - bm^2);  delta = bm - mean_j;  tot = count + n
 *   mean_j += delta * n / tot;  var_j = (var_j * count + bv * n + delta^2 * count * n / tot) / tot;  count = tot
 * n == 0 leaves the state unchanged.  `sums` is not modified. */
int32_t ddrl_op_running_merge(const double* sums, int32_t d, double* state, void* stream);
/* shift_j = center ? (float)mean_j : 0;  scale_j = (float)(1 / sqrt(var_j + eps)), formed in double.  eps >= 0. */
int32_t ddrl_op_running_affine(const double* state, int32_t d, double eps, int32_t center, float* affine, void* stream);
/* out[r][j] = clamp((x[r][j] - shift_j) * scale_j, -clip, clip) for r < n, j < d, in fp32: a subtract, then a multiply (never fused),
 * then v < -clip ? -clip : (v > clip ? clip : v), so that a NaN stays a NaN and an infinity goes to the clip.  clip > 0, +inf
 * allowed.  x is [n][ld_x], out [n][ld_out]; out == x with ld_out == ld_x is allowed, any other overlap is refused; the padding columns
 * [d, ld_out) of out are never written. */
int32_t ddrl_op_normalize_columns(const float* x, int64_t n, int32_t d, int64_t ld_x, const float* affine, float clip, float* out,
                                  int64_t ld_out, void* stream);
/* The discounted return that reward scaling takes its variance of, over the T steps of a rollout ([T][N], like ddrl_gae), one lane per
 * env, forward in time, never fused:  g = carry[n] * gamma + rewards[t][n];  trace[t][n] = g;  carry[n] = dones[t][n] ? 0 : g.
 * carry [N] persists between calls: two chained calls equal one call on the concatenation.  0 <= gamma <= 1. */
int32_t ddrl_op_discounted_returns(const float* rewards, const uint8_t* dones, int32_t T, int32_t N, float gamma, float* carry, float* trace,
                                   void* stream);

/* ---------------------------------------------------------------------------------------------
 * Device environments: Pong and Catch stepped and rendered on the GPU (additive: ABI 3; the rules are
 * tests/device_env_ref.py, in integers only, and the kernels reproduce them bit for bit).  Context-free, no allocation, no atomics,
 * asynchronous on `stream`; the same arguments and data give the same bits.  One launch serves all n envs.
 *   game    0 = Pong, 1 = Catch
 *   state   int32 [n][ddrl_op_env_state_ints()], 16-byte aligned: ball, velocity, paddles, scores, step and event counters
 *   env0    the global index of local env 0 (the random draws hash (seed, env0 + i, event counter)): 0 <= env0, env0 + n <= 2^32
 *   frame   uint8 [n][84][84], 16-byte aligned: background 87, objects 236; env i is written at frame + i * 7056 and nowhere else
 * A null pointer (the mask excepted), n < 1, an unknown game, a misaligned state or frame, an overlap of two arguments: DDRL_ERR_INVALID_ARG,
 * decided before anything touches HIP.
 * ------------------------------------------------------------------------------------------ */
/* the int32 words of one env's state (16) */
int32_t ddrl_op_env_state_ints(void);
/* A new first episode (all counters zero) for every env, or for those with a non-zero byte in mask (uint8 [n], NULL = all); their first
 * frames are rendered.  The state and frame of an env whose mask byte is zero are not touched. */
int32_t ddrl_op_env_reset(int32_t game, int32_t* state, int32_t n, int64_t env0, uint32_t seed, const uint8_t* mask, uint8_t* frame,
                          void* stream);
/* One step of every env: actions float32 [n] (k = (int)a % 3: stay / negative / positive direction; not finite, negative or >= n_actions:
 * stay) -> the new state, its frame, reward float32 [n] in {-1, 0, 1} and done uint8 [n].  A finished env (a score of `points` in
 * Pong, the landed ball in Catch, or max_steps steps) starts its next episode in the same launch: the frame is that episode's first and
 * done is the reset flag.  2 <= n_actions <= 18, points >= 1, max_steps >= 1; actions and reward 4-byte aligned. */
int32_t ddrl_op_env_step(int32_t game, int32_t* state, int32_t n, int64_t env0, int32_t n_actions, int32_t points, int32_t max_steps,
                         uint32_t seed, const float* actions, uint8_t* frame, float* reward, uint8_t* done, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Device navigation env: a differential-drive robot, up to 10 static circular obstacles and up to 5 walking pedestrians in a round
 * arena, stepped and observed on the GPU (additive: ABI 3; the rules are tests/nav_env_ref.py, in integers only,
 * and the kernels reproduce them bit for bit).  Context-free, no allocation, no atomics, asynchronous on `stream`; the same arguments and
 * data give the same bits.  One launch serves all n envs.  The observation is what NavPreNet1D reads:
 *   laser   float32 [n][1][960], 16-byte aligned: ranges in metres (0 .. 6), beam 0 straight ahead, counter-clockwise
 *   vector  float32 [n][5]: the goal in the robot's frame (m), the last v / 32 and w / 64, the distance to the goal (m)
 *   image   float32 [n][3][48][48], 16-byte aligned: the egocentric pedestrian map (occupancy, velocity forward / left)
 *   state   int32 [n][ddrl_op_nav_env_state_ints()], 16-byte aligned
 *   env0    the global index of local env 0 (the random draws hash (seed, env0 + i, event counter)): 0 <= env0, env0 + n <= 2^32
 * Env i is written at laser + i * 960, vector + i * 5, image + i * 6912 and nowhere else.  A null pointer (the mask excepted), n < 1,
 * n_obstacles outside 0..10, n_peds outside 0..5, a misaligned state, laser or image, an overlap of two arguments:
 * DDRL_ERR_INVALID_ARG, decided before anything touches HIP.
 * ------------------------------------------------------------------------------------------ */
/* the int32 words of one env's state (64) */
int32_t ddrl_op_nav_env_state_ints(void);
/* Host only: copies out the Q14 table the kernels index, cos[3840] then sin[3840] of 2 pi k / 3840 (7,680 words). */
int32_t ddrl_op_nav_env_trig(int32_t* cos_sin_host);
/* A new first episode (all counters zero) for every env, or for those with a non-zero byte in mask (uint8 [n], NULL = all); their first
 * observations are rendered.  The state and observation of an env whose mask byte is zero are not touched. */
int32_t ddrl_op_nav_env_reset(int32_t* state, int32_t n, int64_t env0, uint32_t seed, int32_t n_obstacles, int32_t n_peds,
                              const uint8_t* mask, float* laser, float* vector, float* image, void* stream);
/* One step of every env: actions float32 [n][2] (v = floor(clamp(a0, 0, 1) * 32) ticks of 1/256 m, w = trunc(clamp(a1, -1, 1) * 64)
 * heading steps of 2 pi / 3840; a component that is not finite counts as 0) -> the new state, its observation, reward float32 [n] (a
 * multiple of 1/256: twice the progress towards the goal in metres, -15 for a collision, +15 at the goal) and done uint8 [n].  A
 * finished env (collision, goal, or max_steps steps) starts its next episode in the same launch: the observation is that episode's first
 * and done is the reset flag.  max_steps >= 1; actions, vector and reward 4-byte aligned. */
int32_t ddrl_op_nav_env_step(int32_t* state, int32_t n, int64_t env0, uint32_t seed, int32_t n_obstacles, int32_t n_peds, int32_t max_steps,
                             const float* actions, float* laser, float* vector, float* image, float* reward, uint8_t* done, void* stream);
/* ddrl_op_nav_env_step plus one output, info int32 [n] (4-byte aligned, apart from every other argument): what the step just played
 * did, before a finished env's new episode is drawn.  State, observation, reward and done are bit-identical to ddrl_op_nav_env_step.
 *   bit 0 done   bit 1 goal   bits 2-3 collision kind (0 none, 1 static: wall or obstacle, 2 pedestrian; static wins)
 *   bit 4 truncated (max_steps reached without collision or goal)
 *   bit 5 close to a pedestrian: after the move some pedestrian's centre is within 512 ticks (2 m) of the robot's
 *   bit 6 wall hit   bit 7 obstacle hit   bits 8-13 the decoded v (0..32)   bits 16-23 the decoded w + 64 (0..128)   others zero */
int32_t ddrl_op_nav_env_step_info(int32_t* state, int32_t n, int64_t env0, uint32_t seed, int32_t n_obstacles, int32_t n_peds,
                                  int32_t max_steps, const float* actions, float* laser, float* vector, float* image, float* reward,
                                  uint8_t* done, int32_t* info, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Navigation episode statistics (additive: ABI 3): the reference's Status.update_nav_status and the sums of its
 * group_logger over the info words above, per env, on the device.  Context-free, no allocation, no atomics, asynchronous on `stream`;
 * fixed-order sums, so the same data give the same bits.  The per-env state is three buffers the caller owns (zero = a fresh Status):
 *   sums         float32 [18][N]: for every step, for the steps close to a pedestrian, for the steps in the open, six rows each:
 *                v_speeds_sum, v_speeds_episode, w_speeds_sum, w_speeds_episode, steps_sum, steps_episode
 *   episode_num  int32 [N]
 *   rings        float32 [5][100][N]: arrive_num, coll_static_num, coll_ped_num, coll_robot_num, and the truncations kept the same way
 * A null or misaligned pointer, N < 1, T < 0, an overlap of two arguments: DDRL_ERR_INVALID_ARG, decided before anything touches HIP.
 * ------------------------------------------------------------------------------------------ */
#define DDRL_NAV_STATUS_ROWS 18
#define DDRL_NAV_STATUS_RINGS 5
#define DDRL_NAV_STATUS_WINDOW 100
#define DDRL_NAV_STATUS_SUMMARY 22
/* T successive update_nav_status calls in one launch, one lane per env: info int32 [T][N] with arrive = bit 1, collision = bits 2-3,
 * all_down = bit 0, speeds = (v / 32, w / 64) from the decoded fields (w = bits 16-23 less 64), bool_get_close_to_human = bit 5,
 * is_clean = 1.  Every fp32 operation is exact, so the state equals the reference's bit for bit.  T == 0 is a no-op. */
int32_t ddrl_op_nav_status_update(const int32_t* info, int32_t T, int32_t N, float* sums, int32_t* episode_num, float* rings,
                                  void* stream);
/* summary double [DDRL_NAV_STATUS_SUMMARY] (8-byte aligned), eleven (sum, count) pairs that add across ranks: reach, static-collision,
 * pedestrian-collision and truncation rate (sum(ring) / clip(episode_num + 1, 1, 100), every env counts); linear and angular speed per
 * step of the latest finished episode (fp32 quotient per env) over all steps, over the close steps and over the open steps, counting
 * only envs whose step count is > 0; steps_episode (every env counts).  One workgroup, a fixed order. */
int32_t ddrl_op_nav_status_reduce(const float* sums, const int32_t* episode_num, const float* rings, int32_t N, double* summary,
                                  void* stream);

/* ---------------------------------------------------------------------------------------------
 * Multi-robot navigation env (additive: ABI 3; the rules are tests/fleet_env_ref.py, in integers only, and the
 * kernels reproduce them bit for bit): n_robots = 1..4 robots of the navigation env above share one arena (a world) with its obstacles
 * and pedestrians, see each other in their lidar (circles of radius 64 ticks) and in their map (under the pedestrians) and collide with
 * each other.  Context-free, no allocation, no atomics, asynchronous on `stream`; one launch serves all worlds.  A ROW is one robot: row
 * i * n_robots + r is robot r of world i, and every per-row argument has n_worlds * n_robots rows of the navigation env's shapes:
 *   laser   float32 [rows][1][960], 16-byte aligned     vector  float32 [rows][5]     image  float32 [rows][3][48][48], 16-byte aligned
 *   state   int32 [n_worlds][ddrl_op_fleet_env_state_ints()], 16-byte aligned: robot r at words 10 r .. 10 r + 8 (X, Y, H, V, W, GX, GY,
 *           DPREV, STEPS), obstacle k at 40 + 3 k, pedestrian j at 70 + 4 j, the world's event counter at 90, zeros elsewhere
 *   world0  the global index of local world 0 (the draws hash (seed, world0 + i, event counter)): 0 <= world0, world0 + n_worlds <= 2^32
 * A null pointer (mask and info excepted), n_worlds < 1, n_robots outside 1..4, n_worlds * n_robots beyond int32, n_obstacles outside
 * 0..10, n_peds outside 0..5, max_steps < 1, a misaligned state, laser or image, an overlap of two arguments: DDRL_ERR_INVALID_ARG,
 * decided before anything touches HIP.
 * ------------------------------------------------------------------------------------------ */
/* the int32 words of one world's state (96) */
int32_t ddrl_op_fleet_env_state_ints(void);
/* A new world (all counters zero; obstacles, robots with their goals and pedestrians in cells of their own) for every world, or for
 * those with a non-zero byte in mask (uint8 [n_worlds], NULL = all); the first observations of their rows are rendered.  The state and
 * the rows of a world whose mask byte is zero are not touched. */
int32_t ddrl_op_fleet_env_reset(int32_t* state, int32_t n_worlds, int32_t n_robots, int64_t world0, uint32_t seed, int32_t n_obstacles,
                                int32_t n_peds, const uint8_t* mask, float* laser, float* vector, float* image, void* stream);
/* One step of every world: actions float32 [rows][2], decoded as ddrl_op_nav_env_step's -> the new state, every row's observation,
 * reward float32 [rows] and done uint8 [rows].  The pedestrians move, then every robot; a robot's outcome is read off the positions
 * after all moves: a collision with the wall, an obstacle, a pedestrian or another robot (centres closer than 128 ticks; both partners
 * collide) costs 15, the goal pays 15, max_steps steps truncate.  Only a finished robot starts a new episode, in the same launch, at
 * the centre of a grid cell at least 300 ticks from every obstacle centre, pedestrian and other robot, with a new goal; the world is
 * never redrawn.  info int32 [rows] or NULL: the info word of ddrl_op_nav_env_step_info for the step just played, where collision kind
 * 3 is another robot (static wins, then the pedestrian); the other outputs are the same with and without it.  actions, vector, reward
 * and info 4-byte aligned. */
int32_t ddrl_op_fleet_env_step(int32_t* state, int32_t n_worlds, int32_t n_robots, int64_t world0, uint32_t seed, int32_t n_obstacles,
                               int32_t n_peds, int32_t max_steps, const float* actions, float* laser, float* vector, float* image,
                               float* reward, uint8_t* done, int32_t* info, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Bootstrapping truncated episodes (additive: ABI 3).  A time limit is not an outcome of the task: at a step
 * that max_steps ended (info bit 4) GAE should go on from the critic's value of the observation the episode ended in, not from 0.  The
 * step kernels draw the next episode in the same launch, so that observation is rendered by these two entry points, filed per env by
 * ddrl_op_file_flagged_rows and its value used by ddrl_gae_bootstrap.  Context-free, no allocation, no atomics, asynchronous on
 * `stream`; every check is decided before anything touches HIP.
 * ------------------------------------------------------------------------------------------ */
/* ddrl_op_nav_env_step_info plus the terminal observation: final_laser float32 [n][1][960], final_vector [n][5], final_image
 * [n][3][48][48], aligned like laser, vector and image and apart from every other argument.  For an env whose info word has bit 4 set,
 * row i of final_* receives the observation of the state the episode ended in (after the move and the outcome, before the new episode
 * is drawn: in the vector, v and w are the action just played and the distance is the one after the move); the rows of every other env
 * are not written.  State, observation, reward, done and info are bit-identical to ddrl_op_nav_env_step_info. */
int32_t ddrl_op_nav_env_step_final(int32_t* state, int32_t n, int64_t env0, uint32_t seed, int32_t n_obstacles, int32_t n_peds,
                                   int32_t max_steps, const float* actions, float* laser, float* vector, float* image, float* reward,
                                   uint8_t* done, int32_t* info, float* final_laser, float* final_vector, float* final_image,
                                   void* stream);
/* ddrl_op_fleet_env_step with info required, plus the terminal observation of every truncated row (final_* [rows], as above): what the
 * robot sees with every robot where it is after all moves of the step and before any respawn.  Rows without bit 4 are not written; the
 * other outputs are bit-identical to ddrl_op_fleet_env_step. */
int32_t ddrl_op_fleet_env_step_final(int32_t* state, int32_t n_worlds, int32_t n_robots, int64_t world0, uint32_t seed, int32_t n_obstacles,
                                     int32_t n_peds, int32_t max_steps, const float* actions, float* laser, float* vector, float* image,
                                     float* reward, uint8_t* done, int32_t* info, float* final_laser, float* final_vector,
                                     float* final_image, void* stream);
/* ------------------------------------------------------------------------------------------
 * The pedestrian model (tests/ped_avoid_ref.py is the rule book of "avoid").  DDRL_PED_WALK is rule 1 of the
 * entry points above: a pedestrian walks straight ahead and draws a new heading when the wall or an obstacle refuses its step.  Under
 * DDRL_PED_AVOID it also gives way to the other pedestrians and to the robots: of its step under the heading offsets 0, +30, -30, +60,
 * -60, +90, -90 degrees it takes the first that neither the wall nor an obstacle refuses and that does not bring it within 0.75 m of
 * another pedestrian or a robot while coming nearer to it; the turn persists.  A refused step straight ahead, or no step left, costs one
 * draw of a new heading, as under DDRL_PED_WALK.  No state word is added, and resets, placement, respawn and every other rule are the
 * same.  One entry point per env takes the model and every optional output of the entry points above:
 *   info     NULL or int32 [rows]: the info word, as ddrl_op_nav_env_step_info's
 *   final_*  all three NULL, or all three given (then info is required): the terminal observation, as ddrl_op_*_env_step_final's
 * With ped_model == DDRL_PED_WALK every output is bit-identical to the entry point above that takes the same outputs (the same kernels
 * are launched).  ped_model outside the two values, final_* given in part or without info, and everything the entry points above
 * refuse: DDRL_ERR_INVALID_ARG, decided before anything touches HIP.
 * ------------------------------------------------------------------------------------------ */
#define DDRL_PED_WALK 0
#define DDRL_PED_AVOID 1
int32_t ddrl_op_nav_env_step_model(int32_t* state, int32_t n, int64_t env0, uint32_t seed, int32_t n_obstacles, int32_t n_peds,
                                   int32_t max_steps, int32_t ped_model, const float* actions, float* laser, float* vector, float* image,
                                   float* reward, uint8_t* done, int32_t* info, float* final_laser, float* final_vector,
                                   float* final_image, void* stream);
int32_t ddrl_op_fleet_env_step_model(int32_t* state, int32_t n_worlds, int32_t n_robots, int64_t world0, uint32_t seed, int32_t n_obstacles,
                                     int32_t n_peds, int32_t max_steps, int32_t ped_model, const float* actions, float* laser,
                                     float* vector, float* image, float* reward, uint8_t* done, int32_t* info, float* final_laser,
                                     float* final_vector, float* final_image, void* stream);
/* Files the rows of flagged envs into a pool of S slots per env: for env n with (info[n] & mask) != 0 and 0 <= count[n] < S, row n of
 * every part's src (float32 [N][widths[k]]) is copied to dst[k] (float32 [S][N][widths[k]]) at [count[n]][n] and slot_out[n] = count[n];
 * a flagged env without room gets slot_out[n] = -1 and nothing is copied; either way count[n] (int32 [N], in/out) goes up by one, so an
 * overflow stays visible.  An env that is not flagged gets slot_out[n] = -1 and keeps its count.  src, dst and widths are HOST arrays of
 * n_parts = 1..4 entries.  One workgroup per env; a part whose width is a multiple of 4 floats on 16-byte aligned bases moves in 16-byte
 * units, any other in 4-byte units.  A null or misaligned (4 bytes) pointer, mask == 0, N < 1, S < 1, n_parts outside 1..4, a width
 * < 1, an overlap of two arguments: DDRL_ERR_INVALID_ARG. */
int32_t ddrl_op_file_flagged_rows(const int32_t* info, int32_t mask, int32_t N, int32_t S, int32_t n_parts, const float* const* src,
                                  float* const* dst, const int32_t* widths, int32_t* count, int32_t* slot_out, void* stream);
/* ddrl_gae with one change: where slot[t][n] (int32 [T][N]) is in [0, S), the successor term (gamma * V_next) * (1 - done) is
 * gamma * boot[slot[t][n]][n] (boot float32 [S][N]) -- a select, not a blend; any other slot value counts as -1, the plain term.  The
 * accumulated sum is still zeroed behind every done.  A boot entry that no slot names is never read.  With every slot -1 the results
 * equal ddrl_gae's bit for bit.  A null or misaligned pointer, S < 1, T < 0, N < 1, adv or ret overlapping an input:
 * DDRL_ERR_INVALID_ARG. */
int32_t ddrl_gae_bootstrap(const float* values, const float* rewards, const uint8_t* dones, const int32_t* slot, const float* boot,
                           int32_t S, int32_t T, int32_t N, float gamma, float landa, float* adv, float* ret, void* stream);

/* ---------------------------------------------------------------------------------------------
 * DAgger on the device (additive: ABI 3): a scripted expert for the navigation env and the cloning loss of a
 * Gaussian actor.  Context-free, no allocation, no atomics, asynchronous on `stream`; the same arguments and data give the same bits;
 * every check is decided before anything touches HIP.
 * ------------------------------------------------------------------------------------------ */
/* The expert's action for every env of ddrl_op_nav_env_*'s `state` (read, never written; words are brought into their ranges as the
 * step kernel does): the best of 51 constant-(v, w) arcs rolled 10 steps ahead against the wall, the obstacles and the pedestrians'
 * straight-line predictions (the rules are tests/nav_expert_ref.py, in integers only, and the kernel reproduces them bit for bit).
 *   label   float32 [n][2] or NULL: (v / 32, w / 64) of the winning arc, what ddrl_op_nav_env_step decodes back to (v, w)
 *   played  float32 [n][2] or NULL: label[i] where hash(seed, env0 + i, step) < threshold (the hash of the envs' draws; the env's event
 *           counter is not touched), policy[i] elsewhere; with policy NULL the label everywhere
 *   policy  float32 [n][2] or NULL: the learner's actions, copied bit for bit where they are played
 * threshold = min(2^32 - 1, floor(beta 2^32)) for DAgger's mixing rate beta.  All three of policy, played and label NULL, n < 1,
 * env0 + n beyond 2^32, n_obstacles outside 0..10, n_peds outside 0..5, a state that is not 16-byte aligned, a float pointer that is
 * not 4-byte aligned, an overlap of two arguments: DDRL_ERR_INVALID_ARG. */
int32_t ddrl_op_nav_expert(const int32_t* state, int32_t n, int64_t env0, uint32_t seed, int32_t n_obstacles, int32_t n_peds,
                           const float* policy, uint32_t step, uint32_t threshold, float* label, float* played, void* stream);
/* ddrl_op_heads_bc_loss for a Gaussian actor's mean: mu = w h + b with w [n_actions][512], 1 <= n_actions <= 8, against targets
 * float32 [n][n_actions]; loss = mean((mu - y)^2) / 2 over the n_total * n_actions elements of the whole batch (n_total >= n: the n
 * samples are a micro-batch of it).  Writes dh [n][ld_dh], dw, db and stats = (this call's share of the loss, sum |mu - y|); log_std
 * takes no part.  One wave per sample, per-workgroup partial rows summed in a fixed order by a second launch: deterministic.
 * h and dh 16-byte aligned with ld >= 512 a multiple of 4; ws = ddrl_op_heads_bc_mse_ws_floats floats. */
int32_t ddrl_op_heads_bc_mse_ws_floats(int32_t n_actions, int32_t max_n, int64_t* floats);
int32_t ddrl_op_heads_bc_mse(const float* w, const float* b, int32_t n_actions, const float* h, int64_t ld_h, int32_t n,
                             const float* targets, int64_t n_total, float* dh, int64_t ld_dh, float* dw, float* db, float* stats,
                             float* ws, void* stream);
/* dst[i][:] = src[clamp(idx[i], 0, n_rows - 1)][:] for i < n, rows of row_floats floats (any width: the 5-float vector rows of the
 * navigation env are 20 bytes).  16-byte accesses when row_floats % 4 == 0 and both bases are 16-byte aligned, 4-byte ones otherwise;
 * the result is the same.  A null or misaligned (4 bytes) pointer, n < 1, n_rows < 1, row_floats < 1, dst overlapping src or idx:
 * DDRL_ERR_INVALID_ARG. */
int32_t ddrl_op_gather_rows_f32(const float* src, int64_t n_rows, int64_t row_floats, const int32_t* idx, int32_t n, float* dst,
                                void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DDRL_H_ */
