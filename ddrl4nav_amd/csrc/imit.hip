// Imitation pre-training (behaviour cloning of the Categorical actor): the supervised loss head on 512-wide encoder features and the
// device-side minibatch gather.
//
// Reference arithmetic replaced:
//   Basenn._imitation_learning_classifier   USTC_lab/nn/base.py:120-150 (CrossEntropyLoss on the actor's logits + its autograd backward
//                                           through actor_linear; the reference's own expression cannot run on a PPO net)
//   DataLoader(dataset, batch, shuffle)     USTC_lab/nn/base.py:128,140-141 (the per-batch collation of the shuffled samples)
#include <type_traits>

#include "heads_common.h"
#include "rows.h"

namespace ddrl {

// ---- cross-entropy head ------------------------------------------------------------------------------------------------------------
// One wavefront per sample as in heads.hip: 8 features per lane, the A dot products reduced by the wave butterfly.  A wave takes NS
// samples per turn; lane i < NS then runs the softmax / log-sum-exp chain of sample i once (not 64 times on wave-uniform numbers) and
// the others read its d(logits) back with v_readlane.  The head weights sit in LDS (up to 36 KB for the 18 Atari actions).
//   GREG (A <= 8): the weight / bias gradient is accumulated in registers (64 + 8 per lane) and reduced over the workgroup's waves;
//   else (A <= 18): d(logits) is stored and head_wgrad_kernel forms the weight gradient (144 accumulators do not sit beside the rest).
// Partials per workgroup: [A*512 dw][A db][loss sum][correct count]; head_reduce_kernel sums them over BcReduce.
constexpr int BC_WAVES = 4, BC_NS = 4, BC_MAX_WG = 64;
constexpr int BC_A_SMALL = 8, BC_A_LARGE = 18;

inline int bc_workgroups(int n) {
  const int per = BC_WAVES * BC_NS;
  const int w = (n + per - 1) / per;
  return w < BC_MAX_WG ? w : BC_MAX_WG;
}
inline int64_t bc_stride(int A) { return ((int64_t)A * FEAT + A + 2 + 3) & ~(int64_t)3; }

// MSE (ddrl_op_heads_bc_mse, the Gaussian actor's mean): `labels` holds A targets per sample, d(mu) = (mu - y) / (n_total A) takes the
// place of d(logits), the loss sum is sum (mu - y)^2 and the second statistic sum |mu - y| (in double: it is no count).
template <int MAXA, bool GREG, bool MSE = false>
__global__ __launch_bounds__(BC_WAVES * 64) void bc_loss_kernel(const float* __restrict__ h, int64_t ld_h, const float* __restrict__ w,
                                                                 const float* __restrict__ bias, int A, int n,
                                                                 const float* __restrict__ labels, float inv_n, float* __restrict__ dh,
                                                                 int64_t ld_dh, float* __restrict__ dlogits, float* __restrict__ part,
                                                                 int64_t pstride) {
  __shared__ float wl[MAXA * FEAT];  // the head weights; after the sample loop the reduction buffer of the weight gradient (GREG)
  __shared__ float red[MAXA + 2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int gw = blockIdx.x * BC_WAVES + wave, nw = gridDim.x * BC_WAVES;
  // `w` / `bias` may sit anywhere in an fp32 arena (4-byte aligned): scalar loads
  for (int i = threadIdx.x; i < MAXA * FEAT; i += BC_WAVES * 64) wl[i] = (i < A * FEAT) ? w[i] : 0.0f;
  float ba[MAXA];
#pragma unroll
  for (int j = 0; j < MAXA; ++j) ba[j] = (j < A) ? bias[min(j, A - 1)] : 0.0f;
  __syncthreads();
  constexpr int NS = BC_NS, GA = GREG ? MAXA : 1;
  float gwa[GA][8], gba[GA];
#pragma unroll
  for (int j = 0; j < GA; ++j) {
    gba[j] = 0.0f;
#pragma unroll
    for (int k = 0; k < 8; ++k) gwa[j][k] = 0.0f;
  }
  double s_loss = 0.0;
  std::conditional_t<MSE, double, float> s_cnt = 0;  // a count below 2^24: exact
  const int ls = lane & (NS - 1);  // the sample of the turn this lane works on in the scalar phase
  for (int b0 = gw * NS; b0 < n; b0 += nw * NS) {
    float ha[NS][8];
#pragma unroll
    for (int i = 0; i < NS; ++i) load8(h + (int64_t)min(b0 + i, n - 1) * ld_h + lane * 8, ha[i]);  // past the end: the last sample again, masked below
    const int bl = min(b0 + ls, n - 1);
    const float lab = MSE ? 0.0f : labels[bl];
    // ---- logits: a lane keeps those of ITS sample
    float zl[MAXA];
#pragma unroll
    for (int j = 0; j < MAXA; ++j) {
      float wr[8];
      load8(wl + j * FEAT + lane * 8, wr);
      zl[j] = 0.0f;
#pragma unroll
      for (int i = 0; i < NS; ++i) {
        float s = 0.0f;
#pragma unroll
        for (int k = 0; k < 8; ++k) s = __builtin_fmaf(ha[i][k], wr[k], s);
        const float zj = wave_sum(s) + ba[j];
        zl[j] = (ls == i) ? zj : zl[j];
      }
    }
    float gzl[MAXA], nll = 0.0f;
    bool valid = true;
    int a = -1, am = 0;
    if constexpr (MSE) {
      // ---- this lane's sample: d = mu - y per dimension; d(mu) = d / (n_total A)
      float se = 0.0f;
      double sq = 0.0;
#pragma unroll
      for (int j = 0; j < MAXA; ++j) {
        const float d = (j < A) ? zl[j] - labels[(int64_t)bl * A + min(j, A - 1)] : 0.0f;
        gzl[j] = d * inv_n;
        sq += (double)d * (double)d;
        se += fabsf(d);
      }
      if (lane < NS && b0 + ls < n) {
        s_loss += sq;
        s_cnt += (double)se;
      }
    } else {
      // ---- this lane's sample: log_softmax = z - max - log sum exp(z - max); d(logits) = (softmax - onehot) / n_total
      valid = lab >= 0.0f && lab < (float)A;  // a label outside [0, A) (NaN included): no loss, no gradient
      a = valid ? (int)lab : -1;
      float m = zl[0];
#pragma unroll
      for (int j = 1; j < MAXA; ++j)
        if (j < A && zl[j] > m) {  // the first maximum, as torch.argmax
          m = zl[j];
          am = j;
        }
      float e[MAXA], se = 0.0f;
#pragma unroll
      for (int j = 0; j < MAXA; ++j) {
        e[j] = (j < A) ? expf(zl[j] - m) : 0.0f;
        se += e[j];
      }
      nll = valid ? -((pick(zl, a) - m) - logf(se)) : 0.0f;
#pragma unroll
      for (int j = 0; j < MAXA; ++j) gzl[j] = (valid && j < A) ? (e[j] / se - ((j == a) ? 1.0f : 0.0f)) * inv_n : 0.0f;
    }
    if (!MSE && lane < NS && b0 + ls < n) {
      s_loss += (double)nll;
      s_cnt += (valid && am == a) ? 1.0f : 0.0f;
      if constexpr (!GREG) {
#pragma unroll
        for (int j = 0; j < MAXA; ++j)
          if (j < A) dlogits[(int64_t)(b0 + ls) * A + j] = gzl[j];
      }
    }
    // ---- backward of the head layer: dh[b] = sum_j dlogit_j w_j (per element the j-ordered fma chain), dw += dlogit_j h[b]
    float da[NS][8];
#pragma unroll
    for (int i = 0; i < NS; ++i)
#pragma unroll
      for (int k = 0; k < 8; ++k) da[i][k] = 0.0f;
#pragma unroll
    for (int j = 0; j < MAXA; ++j) {
      float wr[8];
      load8(wl + j * FEAT + lane * 8, wr);
#pragma unroll
      for (int i = 0; i < NS; ++i) {
        // sample i's d(logit j) from its lane; samples past the end carry the last sample's numbers and are dropped here
        float g = __uint_as_float((unsigned)__builtin_amdgcn_readlane((int)__float_as_uint(gzl[j]), i));
        g = (b0 + i < n) ? g : 0.0f;
#pragma unroll
        for (int k = 0; k < 8; ++k) da[i][k] = __builtin_fmaf(g, wr[k], da[i][k]);
        if constexpr (GREG) {
          gba[j] += g;
#pragma unroll
          for (int k = 0; k < 8; ++k) gwa[j][k] = __builtin_fmaf(g, ha[i][k], gwa[j][k]);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < NS; ++i)
      if (b0 + i < n) store8(dh + (int64_t)(b0 + i) * ld_dh + lane * 8, da[i]);  // wave-uniform
  }
  // the loss sums live in lanes 0 .. NS-1 (one sample each per turn): added in sample order
  {
    double tl = 0.0;
    decltype(s_cnt) tc = 0;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      tl += __shfl(s_loss, i, 64);
      tc += __shfl(s_cnt, i, 64);
    }
    s_loss = tl, s_cnt = tc;
  }
  // ---- workgroup reduction, waves accumulate in turn (fixed order) -> part[blockIdx.x]
  __syncthreads();  // every wave is done with the weights in `wl`
  for (int wv = 0; wv < BC_WAVES; ++wv) {
    if (wave == wv) {
      const bool first = (wv == 0);
      if constexpr (GREG) {
#pragma unroll
        for (int j = 0; j < MAXA; ++j) turn_add_row(first, wl, j * FEAT + lane * 8, gwa[j]);
      }
      if (lane == 0) {
        if constexpr (GREG) {
#pragma unroll
          for (int j = 0; j < MAXA; ++j) turn_add(first, red[j], gba[j]);
        }
        turn_add(first, red[MAXA], (float)s_loss);
        turn_add(first, red[MAXA + 1], (float)s_cnt);
      }
    }
    __syncthreads();
  }
  float* out = part + (int64_t)blockIdx.x * pstride;
  if constexpr (GREG) {
    for (int i = threadIdx.x; i < A * FEAT; i += BC_WAVES * 64) out[i] = wl[i];
    if (threadIdx.x < A) out[A * FEAT + threadIdx.x] = red[threadIdx.x];
  }
  if (threadIdx.x < 2) out[A * FEAT + A + threadIdx.x] = red[MAXA + threadIdx.x];
}

// dw / db and the two statistics (loss share of the n_total samples, correct count) from the partial rows
struct BcReduce {
  int A;
  double inv_n;
  float *dw, *db, *stats;
  static constexpr int N_STATS = 2;
  __host__ __device__ int n_grad() const { return A * FEAT + A; }
  __device__ float* dst(int i) const { return i < A * FEAT ? dw + i : db + (i - A * FEAT); }
  __device__ void stat(int k, double s) const { stats[k] = (float)(k == 0 ? s * inv_n : s); }
};

// ---- minibatch gather --------------------------------------------------------------------------------------------------------------
// dst[i][:] = src[idx[i]][:] by the row mover of rows.h.  An index outside [0, n_rows) reads nothing: a zero row, label -1.
__global__ __launch_bounds__(GATHER_THREADS) void gather_rows_kernel(const uint4* __restrict__ src, int64_t n_rows, int64_t row_vecs,
                                                                      int chunks, const int32_t* __restrict__ idx, uint4* __restrict__ dst,
                                                                      const float* __restrict__ labels_src, float* __restrict__ labels_dst) {
  const int i = blockIdx.x / chunks, c = blockIdx.x % chunks;
  const int64_t r = idx[i];
  const bool ok = r >= 0 && r < n_rows;
  gather_row_chunk(src, r, ok, row_vecs, c, i, dst);
  if (labels_dst != nullptr && c == 0 && threadIdx.x == 0) labels_dst[i] = ok ? labels_src[r] : -1.0f;
}

// dst[i][:] = src[clamp(idx[i])][:] for fp32 rows of any width (ddrl_op_gather_rows_f32): VEC moves the row mover's 16-byte units, the
// other instantiation the same chunk of a row in floats (a 5-float vector row is 20 bytes)
constexpr int GATHER_F32_CHUNK = GATHER_CHUNK * 4;  // floats of a row one workgroup moves
template <bool VEC>
__global__ __launch_bounds__(GATHER_THREADS) void gather_rows_f32_kernel(const float* __restrict__ src, int64_t n_rows, int64_t row_floats,
                                                                          int chunks, const int32_t* __restrict__ idx,
                                                                          float* __restrict__ dst) {
  const int i = blockIdx.x / chunks, c = blockIdx.x % chunks;
  int64_t r = idx[i];
  r = r < 0 ? 0 : (r >= n_rows ? n_rows - 1 : r);
  if constexpr (VEC) {
    gather_row_chunk(reinterpret_cast<const uint4*>(src), r, true, row_floats / 4, c, i, reinterpret_cast<uint4*>(dst));
  } else {
    const int64_t u0 = (int64_t)c * GATHER_F32_CHUNK + threadIdx.x;
    float v[GATHER_F32_CHUNK / GATHER_THREADS];
#pragma unroll
    for (int t = 0; t < GATHER_F32_CHUNK / GATHER_THREADS; ++t) {
      const int64_t u = u0 + t * GATHER_THREADS;
      v[t] = u < row_floats ? src[r * row_floats + u] : 0.0f;
    }
#pragma unroll
    for (int t = 0; t < GATHER_F32_CHUNK / GATHER_THREADS; ++t) {
      const int64_t u = u0 + t * GATHER_THREADS;
      if (u < row_floats) dst[(int64_t)i * row_floats + u] = v[t];
    }
  }
}

}  // namespace ddrl

using namespace ddrl;

extern "C" {

int32_t ddrl_op_heads_bc_ws_floats(int32_t n_actions, int32_t max_n, int64_t* floats) {
  if (!floats || max_n < 1) return DDRL_ERR_INVALID_ARG;
  if (n_actions < 2 || n_actions > BC_A_LARGE) return DDRL_ERR_UNSUPPORTED;
  *floats = (int64_t)BC_MAX_WG * bc_stride(n_actions) + (n_actions > BC_A_SMALL ? (int64_t)max_n * n_actions : 0);
  return DDRL_OK;
}

int32_t ddrl_op_heads_bc_loss(const float* w, const float* b, int32_t n_actions, const float* h, int64_t ld_h, int32_t n,
                              const float* labels, int64_t n_total, float* dh, int64_t ld_dh, float* dw, float* db, float* stats,
                              float* ws, void* stream) {
  // every check comes before the first HIP call: a host without a GPU gets the same answers
  if (!w || !b || !h || !labels || !dh || !dw || !db || !stats || !ws || n < 1 || n_total < n) return DDRL_ERR_INVALID_ARG;
  if (n_actions < 2 || n_actions > BC_A_LARGE) return DDRL_ERR_UNSUPPORTED;
  if (ld_h < FEAT || ld_dh < FEAT || (ld_h & 3) || (ld_dh & 3) || !aligned16(h) || !aligned16(dh)) return DDRL_ERR_INVALID_ARG;
  const hipStream_t st = (hipStream_t)stream;
  const int A = n_actions, nwg = bc_workgroups(n);
  const int64_t ps = bc_stride(A);
  const double inv_n = 1.0 / (double)n_total;
  if (A <= BC_A_SMALL) {
    hipLaunchKernelGGL((bc_loss_kernel<BC_A_SMALL, true>), dim3(nwg), dim3(BC_WAVES * 64), 0, st, h, ld_h, w, b, A, n, labels,
                       (float)inv_n, dh, ld_dh, (float*)nullptr, ws, ps);
  } else {
    float* dlogits = ws + (int64_t)BC_MAX_WG * ps;
    hipLaunchKernelGGL((bc_loss_kernel<BC_A_LARGE, false>), dim3(nwg), dim3(BC_WAVES * 64), 0, st, h, ld_h, w, b, A, n, labels,
                       (float)inv_n, dh, ld_dh, dlogits, ws, ps);
    hipLaunchKernelGGL(head_wgrad_kernel<BC_A_LARGE>, dim3(nwg), dim3(256), 0, st, h, ld_h, (const float*)dlogits, n, A, ws, ps, A * FEAT);
  }
  launch_head_reduce(ws, ps, nwg, BcReduce{A, inv_n, dw, db, stats}, st);
  return launch_status();
}

int32_t ddrl_op_heads_bc_mse_ws_floats(int32_t n_actions, int32_t max_n, int64_t* floats) {
  if (!floats || max_n < 1) return DDRL_ERR_INVALID_ARG;
  if (n_actions < 1 || n_actions > BC_A_SMALL) return DDRL_ERR_UNSUPPORTED;
  *floats = (int64_t)BC_MAX_WG * bc_stride(n_actions);
  return DDRL_OK;
}

int32_t ddrl_op_heads_bc_mse(const float* w, const float* b, int32_t n_actions, const float* h, int64_t ld_h, int32_t n,
                             const float* targets, int64_t n_total, float* dh, int64_t ld_dh, float* dw, float* db, float* stats,
                             float* ws, void* stream) {
  // every check comes before the first HIP call: a host without a GPU gets the same answers
  if (!w || !b || !h || !targets || !dh || !dw || !db || !stats || !ws || n < 1 || n_total < n) return DDRL_ERR_INVALID_ARG;
  if (n_actions < 1 || n_actions > BC_A_SMALL) return DDRL_ERR_UNSUPPORTED;
  if (ld_h < FEAT || ld_dh < FEAT || (ld_h & 3) || (ld_dh & 3) || !aligned16(h) || !aligned16(dh)) return DDRL_ERR_INVALID_ARG;
  if (((uintptr_t)w & 3) || ((uintptr_t)b & 3) || ((uintptr_t)targets & 3) || ((uintptr_t)dw & 3) || ((uintptr_t)db & 3) ||
      ((uintptr_t)stats & 3) || ((uintptr_t)ws & 3) || n_total > INT64_MAX / BC_A_SMALL)
    return DDRL_ERR_INVALID_ARG;
  const hipStream_t st = (hipStream_t)stream;
  const int A = n_actions, nwg = bc_workgroups(n);
  const int64_t ps = bc_stride(A);
  const double inv_e = 1.0 / ((double)n_total * (double)A);  // one over the elements of the mean
  hipLaunchKernelGGL((bc_loss_kernel<BC_A_SMALL, true, true>), dim3(nwg), dim3(BC_WAVES * 64), 0, st, h, ld_h, w, b, A, n, targets,
                     (float)inv_e, dh, ld_dh, (float*)nullptr, ws, ps);
  launch_head_reduce(ws, ps, nwg, BcReduce{A, 0.5 * inv_e, dw, db, stats}, st);  // loss share = sum d^2 / (2 n_total A)
  return launch_status();
}

int32_t ddrl_op_gather_rows_f32(const float* src, int64_t n_rows, int64_t row_floats, const int32_t* idx, int32_t n, float* dst,
                                void* stream) {
  if (!src || !idx || !dst || n < 1 || n_rows < 1 || row_floats < 1) return DDRL_ERR_INVALID_ARG;
  if (((uintptr_t)src & 3) || ((uintptr_t)dst & 3) || ((uintptr_t)idx & 3)) return DDRL_ERR_INVALID_ARG;
  if (row_floats > INT64_MAX / 4 / n_rows || row_floats > INT64_MAX / 4 / n) return DDRL_ERR_INVALID_ARG;
  const uint64_t dst_b = (uint64_t)n * row_floats * 4;
  if (overlap(src, dst, (uint64_t)n_rows * row_floats * 4, dst_b) || overlap(idx, dst, (uint64_t)n * 4, dst_b)) return DDRL_ERR_INVALID_ARG;
  const int64_t c = (row_floats + GATHER_F32_CHUNK - 1) / GATHER_F32_CHUNK;
  if (c > INT32_MAX / n) return DDRL_ERR_INVALID_ARG;
  const dim3 grid((unsigned)(n * c)), block(GATHER_THREADS);
  if ((row_floats & 3) == 0 && aligned16(src) && aligned16(dst))
    hipLaunchKernelGGL(gather_rows_f32_kernel<true>, grid, block, 0, (hipStream_t)stream, src, n_rows, row_floats, (int)c, idx, dst);
  else
    hipLaunchKernelGGL(gather_rows_f32_kernel<false>, grid, block, 0, (hipStream_t)stream, src, n_rows, row_floats, (int)c, idx, dst);
  return launch_status();
}

int32_t ddrl_op_gather_rows_u8(const uint8_t* src, int64_t n_rows, int64_t row_bytes, const int32_t* idx, int32_t n, uint8_t* dst,
                               const float* labels_src, float* labels_dst, void* stream) {
  if (!src || !idx || !dst || n < 1 || n_rows < 1 || row_bytes < 16 || (row_bytes & 15)) return DDRL_ERR_INVALID_ARG;
  if (!aligned16(src) || !aligned16(dst) || ((uintptr_t)idx & 3)) return DDRL_ERR_INVALID_ARG;
  if ((labels_src == nullptr) != (labels_dst == nullptr)) return DDRL_ERR_INVALID_ARG;
  if (n_rows > INT64_MAX / row_bytes) return DDRL_ERR_INVALID_ARG;
  if (overlap(src, dst, (uint64_t)n_rows * row_bytes, (uint64_t)n * row_bytes)) return DDRL_ERR_INVALID_ARG;
  int64_t row_vecs;
  int chunks;
  if (!gather_grid(row_bytes, n, &row_vecs, &chunks)) return DDRL_ERR_INVALID_ARG;
  hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)(n * chunks)), dim3(GATHER_THREADS), 0, (hipStream_t)stream, (const uint4*)src,
                     n_rows, row_vecs, chunks, idx, (uint4*)dst, labels_src, labels_dst);
  return launch_status();
}

}  // extern "C"
