// Device environments: Pong and Catch stepped and rendered on the GPU (include/ddrl.h ddrl_op_env_state_ints / _env_reset / _env_step;
// DESIGN.md section 6.7).  tests/device_env_ref.py is the rule book: int32 / uint32 arithmetic only, so every state word, frame byte,
// reward and done equals the model's.  Context-free, no allocation, no atomics; the same arguments give the same bits.
//
// One 256-thread workgroup per env.  Every thread loads the env's 16 state words, the workgroup meets at a barrier, every thread
// recomputes the (workgroup-uniform) step in registers, thread 0 stores the new state, the reward and the done, and all threads render:
// a thread owns 16-byte chunks of the env's 7,056 bytes (441 chunks), decides every byte by rectangle membership of its (row, column)
// and stores the chunk whole.  Nothing is scattered: no state, however corrupted, writes outside the env's own frame, and the positions
// are clamped as they are loaded all the same.
#include "rows.h"

namespace ddrl {

constexpr int ENV_STATE_INTS = 16, ENV_THREADS = 256;
constexpr int ENV_SIZE = 84, ENV_PLANE = ENV_SIZE * ENV_SIZE, ENV_CHUNKS = ENV_PLANE / 16;
static_assert(ENV_PLANE % 16 == 0, "a frame is whole 16-byte chunks");
constexpr uint32_t ENV_BACKGROUND = 87, ENV_OBJECT = 236;
enum { ENV_PONG = 0, ENV_CATCH = 1 };
enum { S_BX = 0, S_BY, S_VX, S_VY, S_PA, S_PO, S_SA, S_SO, S_STEPS, S_EVENTS, S_USED };

// Pong: paddles 2 x 10 (opponent columns 4..5, agent columns 78..79), ball 2 x 2
constexpr int PONG_PADDLE_H = 10, PONG_PADDLE_MAX = ENV_SIZE - 10, PONG_OPP_X = 4, PONG_AGENT_X = 78, PONG_BALL = 2,
              PONG_BALL_MAX = ENV_SIZE - 2, PONG_AGENT_SPEED = 3, PONG_OPP_SPEED = 2, PONG_VX = 2, PONG_VY_MAX = 3, PONG_SERVE_X = 41,
              PONG_PADDLE_START = 37, PONG_HIT_AGENT_X = 76, PONG_HIT_OPP_X = 6;
// Catch: paddle 12 x 2 at rows 80..81, ball 4 x 4 falling 4 rows a step
constexpr int CATCH_PADDLE_W = 12, CATCH_PADDLE_MAX = ENV_SIZE - 12, CATCH_PADDLE_Y = 80, CATCH_PADDLE_H = 2, CATCH_BALL = 4,
              CATCH_BALL_MAX = ENV_SIZE - 4, CATCH_FALL = 4, CATCH_SPEED = 4, CATCH_PADDLE_START = 36;

struct EnvState {
  int w[S_USED];
};
struct EnvRect {  // inclusive
  int x0, x1, y0, y1;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ uint32_t env_hash(uint32_t seed, uint32_t env, uint32_t counter) {
  uint32_t x = seed ^ (env * 0x9E3779B1u) ^ (counter * 0x85EBCA77u);
  x ^= x >> 16;
  x *= 0x7FEB352Du;
  x ^= x >> 16;
  x *= 0x846CA68Bu;
  x ^= x >> 16;
  return x;
}

// Pong: the ball re-serves from column 41; Catch: a new ball at the top.  One hash draw.
template <int GAME>
__device__ __forceinline__ void env_serve(EnvState& s, uint32_t seed, uint32_t genv) {
  const uint32_t h = env_hash(seed, genv, (uint32_t)s.w[S_EVENTS]);
  s.w[S_EVENTS] = (int)((uint32_t)s.w[S_EVENTS] + 1u);
  if (GAME == ENV_PONG) {
    s.w[S_BX] = PONG_SERVE_X;
    s.w[S_BY] = (int)((h >> 4) % (uint32_t)(PONG_BALL_MAX + 1));
    s.w[S_VX] = (h & 1u) ? PONG_VX : -PONG_VX;
    s.w[S_VY] = (int)((h >> 1) % (uint32_t)(2 * PONG_VY_MAX + 1)) - PONG_VY_MAX;
  } else {
    s.w[S_BX] = (int)(h % (uint32_t)(CATCH_BALL_MAX + 1));
    s.w[S_BY] = 0;
    s.w[S_VX] = (int)((h >> 8) % 3u) - 1;
    s.w[S_VY] = CATCH_FALL;
  }
}

template <int GAME>
__device__ __forceinline__ void env_new_episode(EnvState& s, uint32_t seed, uint32_t genv) {
  s.w[S_PA] = GAME == ENV_PONG ? PONG_PADDLE_START : CATCH_PADDLE_START;
  s.w[S_PO] = GAME == ENV_PONG ? PONG_PADDLE_START : 0;
  s.w[S_SA] = s.w[S_SO] = s.w[S_STEPS] = 0;
  env_serve<GAME>(s, seed, genv);
}

// the loaded words brought into their ranges (a no-op on every state the rules produce); the counters pass
template <int GAME>
__device__ __forceinline__ void env_sanitize(EnvState& s) {
  if (GAME == ENV_PONG) {
    s.w[S_BX] = clampi(s.w[S_BX], 0, PONG_BALL_MAX);
    s.w[S_BY] = clampi(s.w[S_BY], 0, PONG_BALL_MAX);
    s.w[S_VX] = s.w[S_VX] > 0 ? PONG_VX : -PONG_VX;
    s.w[S_VY] = clampi(s.w[S_VY], -PONG_VY_MAX, PONG_VY_MAX);
    s.w[S_PA] = clampi(s.w[S_PA], 0, PONG_PADDLE_MAX);
    s.w[S_PO] = clampi(s.w[S_PO], 0, PONG_PADDLE_MAX);
  } else {
    s.w[S_BX] = clampi(s.w[S_BX], 0, CATCH_BALL_MAX);
    s.w[S_BY] = clampi(s.w[S_BY], 0, CATCH_BALL_MAX);
    s.w[S_VX] = clampi(s.w[S_VX], -1, 1);
    s.w[S_VY] = CATCH_FALL;
    s.w[S_PA] = clampi(s.w[S_PA], 0, CATCH_PADDLE_MAX);
    s.w[S_PO] = 0;
  }
}

// float action -> 0 stay / 1 negative direction / 2 positive direction; NaN fails both comparisons, an infinity one of them
__device__ __forceinline__ int env_decode(float a, int n_actions) {
  return (a >= 0.0f && a < (float)n_actions) ? (int)a % 3 : 0;
}

// one step of the rules (device_env_ref.py DeviceEnvRef.step), the new episode of a finished env included
template <int GAME>
__device__ __forceinline__ void env_advance(EnvState& s, int k, int points, int max_steps, uint32_t seed, uint32_t genv, int* reward,
                                            int* done) {
  const int move = k == 1 ? -1 : (k == 2 ? 1 : 0);
  int r = 0;
  bool score;
  if (GAME == ENV_PONG) {
    s.w[S_PA] = clampi(s.w[S_PA] + move * PONG_AGENT_SPEED, 0, PONG_PADDLE_MAX);
    if (s.w[S_VX] < 0) {
      const int d = clampi(s.w[S_BY] + 1 - PONG_PADDLE_H / 2 - s.w[S_PO], -PONG_OPP_SPEED, PONG_OPP_SPEED);
      s.w[S_PO] = clampi(s.w[S_PO] + d, 0, PONG_PADDLE_MAX);
    }
    int y = s.w[S_BY] + s.w[S_VY], vy = s.w[S_VY];
    if (y < 0) {
      y = -y;
      vy = -vy;
    } else if (y > PONG_BALL_MAX) {
      y = 2 * PONG_BALL_MAX - y;
      vy = -vy;
    }
    int x = s.w[S_BX] + s.w[S_VX], vx = s.w[S_VX];
    const bool at_agent = x >= PONG_AGENT_X - 1, at_opp = x <= PONG_OPP_X + 1;
    const int pad = at_agent ? s.w[S_PA] : s.w[S_PO];
    const bool over = y + PONG_BALL - 1 >= pad && y <= pad + PONG_PADDLE_H - 1;
    const bool point = (at_agent || at_opp) && !over;
    if ((at_agent || at_opp) && over) {
      const int off = y + 1 - (pad + PONG_PADDLE_H / 2);
      vy = clampi((off - (off & 1)) / 2, -PONG_VY_MAX, PONG_VY_MAX);  // floor(off / 2): the subtraction leaves an even number
      x = at_agent ? PONG_HIT_AGENT_X : PONG_HIT_OPP_X;
      vx = -vx;
    }
    s.w[S_BX] = x;
    s.w[S_BY] = y;
    s.w[S_VX] = vx;
    s.w[S_VY] = vy;
    if (point) {
      if (at_opp) {
        s.w[S_SA] += 1;
        r = 1;
      } else {
        s.w[S_SO] += 1;
        r = -1;
      }
      env_serve<GAME>(s, seed, genv);
    }
    s.w[S_STEPS] += 1;
    score = s.w[S_SA] >= points || s.w[S_SO] >= points;
  } else {
    s.w[S_PA] = clampi(s.w[S_PA] + move * CATCH_SPEED, 0, CATCH_PADDLE_MAX);
    int x = s.w[S_BX] + s.w[S_VX], vx = s.w[S_VX];
    if (x < 0) {
      x = -x;
      vx = -vx;
    } else if (x > CATCH_BALL_MAX) {
      x = 2 * CATCH_BALL_MAX - x;
      vx = -vx;
    }
    const int y = min(s.w[S_BY] + CATCH_FALL, CATCH_PADDLE_Y - CATCH_BALL);
    s.w[S_BX] = x;
    s.w[S_BY] = y;
    s.w[S_VX] = vx;
    const bool landed = y >= CATCH_PADDLE_Y - CATCH_BALL;
    if (landed) {
      const bool caught = x + CATCH_BALL - 1 >= s.w[S_PA] && x <= s.w[S_PA] + CATCH_PADDLE_W - 1;
      s.w[caught ? S_SA : S_SO] += 1;
      r = caught ? 1 : -1;
    }
    s.w[S_STEPS] += 1;
    score = landed;
  }
  const bool d = score || s.w[S_STEPS] >= max_steps;
  if (d) env_new_episode<GAME>(s, seed, genv);
  *reward = r;
  *done = d ? 1 : 0;
}

// the frame of a state: background, every byte inside a rectangle the object value; 16-byte stores into this env's 7,056 bytes only
template <int GAME>
__device__ __forceinline__ void env_render(const EnvState& s, uint4* __restrict__ frame) {
  constexpr int NR = GAME == ENV_PONG ? 3 : 2;
  EnvRect rc[NR];
  if (GAME == ENV_PONG) {
    const int pa = clampi(s.w[S_PA], 0, PONG_PADDLE_MAX), po = clampi(s.w[S_PO], 0, PONG_PADDLE_MAX);
    const int bx = clampi(s.w[S_BX], 0, PONG_BALL_MAX), by = clampi(s.w[S_BY], 0, PONG_BALL_MAX);
    rc[0] = {PONG_OPP_X, PONG_OPP_X + 1, po, po + PONG_PADDLE_H - 1};
    rc[1] = {PONG_AGENT_X, PONG_AGENT_X + 1, pa, pa + PONG_PADDLE_H - 1};
    rc[NR - 1] = {bx, bx + PONG_BALL - 1, by, by + PONG_BALL - 1};
  } else {
    const int pa = clampi(s.w[S_PA], 0, CATCH_PADDLE_MAX);
    const int bx = clampi(s.w[S_BX], 0, CATCH_BALL_MAX), by = clampi(s.w[S_BY], 0, CATCH_BALL_MAX);
    rc[0] = {pa, pa + CATCH_PADDLE_W - 1, CATCH_PADDLE_Y, CATCH_PADDLE_Y + CATCH_PADDLE_H - 1};
    rc[1] = {bx, bx + CATCH_BALL - 1, by, by + CATCH_BALL - 1};
  }
  for (int c = threadIdx.x; c < ENV_CHUNKS; c += ENV_THREADS) {
    int row = (c * 16) / ENV_SIZE, col = c * 16 - row * ENV_SIZE;
    // most chunks are background: one whose rows (two, when it wraps into the next row) or columns miss every rectangle has no byte
    // inside any and is stored without the per-byte test
    const bool wraps = col + 15 >= ENV_SIZE;
    bool touched = false;
#pragma unroll
    for (int k = 0; k < NR; ++k)
      touched = touched || (row + (wraps ? 1 : 0) >= rc[k].y0 && row <= rc[k].y1 && (wraps || (col + 15 >= rc[k].x0 && col <= rc[k].x1)));
    if (!touched) {
      constexpr uint32_t bg = ENV_BACKGROUND * 0x01010101u;
      frame[c] = make_uint4(bg, bg, bg, bg);
      continue;
    }
    uint32_t q[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      uint32_t word = 0;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        bool in = false;
#pragma unroll
        for (int k = 0; k < NR; ++k) in = in || (col >= rc[k].x0 && col <= rc[k].x1 && row >= rc[k].y0 && row <= rc[k].y1);
        word |= (in ? ENV_OBJECT : ENV_BACKGROUND) << (8 * b);
        if (++col == ENV_SIZE) {
          col = 0;
          ++row;
        }
      }
      q[j] = word;
    }
    frame[c] = make_uint4(q[0], q[1], q[2], q[3]);
  }
}

// thread 0 writes the env's 16 words (the spare ones zero) as four 16-byte stores
__device__ __forceinline__ void env_store(const EnvState& s, int32_t* __restrict__ st) {
  int4* o = reinterpret_cast<int4*>(st);
  o[0] = make_int4(s.w[0], s.w[1], s.w[2], s.w[3]);
  o[1] = make_int4(s.w[4], s.w[5], s.w[6], s.w[7]);
  o[2] = make_int4(s.w[8], s.w[9], 0, 0);
  o[3] = make_int4(0, 0, 0, 0);
}

template <int GAME>
__global__ __launch_bounds__(ENV_THREADS) void env_step_kernel(int32_t* __restrict__ state, int64_t env0, int n_actions, int points,
                                                               int max_steps, uint32_t seed, const float* __restrict__ actions,
                                                               uint8_t* __restrict__ frame, float* __restrict__ reward,
                                                               uint8_t* __restrict__ done) {
  const int64_t i = blockIdx.x;
  int32_t* st = state + i * ENV_STATE_INTS;
  EnvState s;
  {
    const int4* in = reinterpret_cast<const int4*>(st);
    const int4 a = in[0], b = in[1], c = in[2];
    s.w[0] = a.x; s.w[1] = a.y; s.w[2] = a.z; s.w[3] = a.w;
    s.w[4] = b.x; s.w[5] = b.y; s.w[6] = b.z; s.w[7] = b.w;
    s.w[8] = c.x; s.w[9] = c.y;
  }
  const int k = env_decode(actions[i], n_actions);
  __syncthreads();  // every thread of this workgroup holds the old state before thread 0 overwrites it; no other workgroup reads it
  env_sanitize<GAME>(s);
  int r, d;
  env_advance<GAME>(s, k, points, max_steps, seed, (uint32_t)(env0 + i), &r, &d);
  if (threadIdx.x == 0) {
    env_store(s, st);
    reward[i] = (float)r;
    done[i] = (uint8_t)d;
  }
  env_render<GAME>(s, reinterpret_cast<uint4*>(frame + i * ENV_PLANE));
}

template <int GAME>
__global__ __launch_bounds__(ENV_THREADS) void env_reset_kernel(int32_t* __restrict__ state, int64_t env0, uint32_t seed,
                                                                const uint8_t* __restrict__ mask, uint8_t* __restrict__ frame) {
  const int64_t i = blockIdx.x;
  if (mask != nullptr && mask[i] == 0) return;  // uniform over the workgroup; the env's state and frame stay as they are
  EnvState s;
#pragma unroll
  for (int j = 0; j < S_USED; ++j) s.w[j] = 0;
  env_new_episode<GAME>(s, seed, (uint32_t)(env0 + i));
  if (threadIdx.x == 0) env_store(s, state + i * ENV_STATE_INTS);
  env_render<GAME>(s, reinterpret_cast<uint4*>(frame + i * ENV_PLANE));
}

// game, n and env0 of both operators: a known game, 1 <= n, global env indices inside 32 bits
inline bool env_range_ok(int32_t game, int32_t n, int64_t env0) {
  return (game == ENV_PONG || game == ENV_CATCH) && n >= 1 && env0 >= 0 && env0 + (int64_t)n <= ((int64_t)1 << 32);
}

}  // namespace ddrl

using namespace ddrl;

extern "C" {

// every check comes before the first HIP call: a host without a GPU gets the same answers

int32_t ddrl_op_env_state_ints(void) { return ENV_STATE_INTS; }

int32_t ddrl_op_env_reset(int32_t game, int32_t* state, int32_t n, int64_t env0, uint32_t seed, const uint8_t* mask, uint8_t* frame,
                          void* stream) {
  if (!state || !frame || !env_range_ok(game, n, env0)) return DDRL_ERR_INVALID_ARG;
  if (!aligned16(state) || !aligned16(frame)) return DDRL_ERR_INVALID_ARG;
  const uint64_t sb = (uint64_t)n * ENV_STATE_INTS * 4, fb = (uint64_t)n * ENV_PLANE;
  if (overlap(state, frame, sb, fb) || (mask && (overlap(mask, state, (uint64_t)n, sb) || overlap(mask, frame, (uint64_t)n, fb))))
    return DDRL_ERR_INVALID_ARG;
  const hipStream_t st = (hipStream_t)stream;
  if (game == ENV_PONG)
    hipLaunchKernelGGL(env_reset_kernel<ENV_PONG>, dim3((unsigned)n), dim3(ENV_THREADS), 0, st, state, env0, seed, mask, frame);
  else
    hipLaunchKernelGGL(env_reset_kernel<ENV_CATCH>, dim3((unsigned)n), dim3(ENV_THREADS), 0, st, state, env0, seed, mask, frame);
  return launch_status();
}

int32_t ddrl_op_env_step(int32_t game, int32_t* state, int32_t n, int64_t env0, int32_t n_actions, int32_t points, int32_t max_steps,
                         uint32_t seed, const float* actions, uint8_t* frame, float* reward, uint8_t* done, void* stream) {
  if (!state || !actions || !frame || !reward || !done || !env_range_ok(game, n, env0)) return DDRL_ERR_INVALID_ARG;
  if (n_actions < 2 || n_actions > 18 || points < 1 || max_steps < 1) return DDRL_ERR_INVALID_ARG;
  if (!aligned16(state) || !aligned16(frame) || ((uintptr_t)actions & 3) || ((uintptr_t)reward & 3)) return DDRL_ERR_INVALID_ARG;
  const void* src[1] = {actions};
  const uint64_t src_b[1] = {(uint64_t)n * 4};
  void* dst[4] = {state, frame, reward, done};
  const uint64_t dst_b[4] = {(uint64_t)n * ENV_STATE_INTS * 4, (uint64_t)n * ENV_PLANE, (uint64_t)n * 4, (uint64_t)n};
  if (!reads_and_writes_apart(src, src_b, 1, dst, dst_b, 4)) return DDRL_ERR_INVALID_ARG;
  const hipStream_t st = (hipStream_t)stream;
  if (game == ENV_PONG)
    hipLaunchKernelGGL(env_step_kernel<ENV_PONG>, dim3((unsigned)n), dim3(ENV_THREADS), 0, st, state, env0, n_actions, points, max_steps,
                       seed, actions, frame, reward, done);
  else
    hipLaunchKernelGGL(env_step_kernel<ENV_CATCH>, dim3((unsigned)n), dim3(ENV_THREADS), 0, st, state, env0, n_actions, points, max_steps,
                       seed, actions, frame, reward, done);
  return launch_status();
}

}  // extern "C"
