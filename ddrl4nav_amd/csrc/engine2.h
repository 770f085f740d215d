// Two things live here:
//   (a) the pipelined f32-MFMA tile engine of the f32-input operator kernels (gconv.hip, glinear.hip): engine2_kernel and what it
//       is built from, down to launch_engine2;
//   (b) the helpers every kernel file uses: register vectors and LDS-direct loads at the top, and behind the engine the plane
//       scheme ("f16x3"), the running maxima and the per-sample magnitudes of the operator kernels.
//
// The engine:
//
//   C[row][col] = sum_k A(row,k) * B(k,col),  rows -> MFMA A operand -> accumulator registers,
//   cols -> MFMA B operand -> lanes (stores are coalesced along cols).
//
// Design points (the first build of this library gathered im2col tiles element by element and
// ran at a third of this engine's rate, profiles/README.md):
//   * operands are read from LDS as  lds[lane_base + compile-time immediate]  (one ds_read_b32
//     with an offset field per operand, zero address VALU inside the k loop);
//   * LDS is double buffered and the next k-block is prefetched global -> registers while the
//     current one feeds the matrix pipe (one barrier per k-block);
//   * ops stage RAW tensors (input planes, weight slabs) with wide coalesced loads instead of
//     gathering an im2col tile element by element (the generic gather ops of gconv.hip are the
//     exception, for layers without a specialised kernel);
//   * the order of LDS reads and MFMAs inside a k-block is pinned (compute_block); an op may ask for
//     LLVM's own interleave instead (IGLP below).
//
// An Op provides:
//   constants  THREADS, TM, TN, KSTEPS, STAGE (floats per LDS buffer)
//   struct Params, struct Regs (prefetch registers)
//   bool  init(P, tid, lds)            tile coordinates, lane bases abase[TM], bbase[TN], kb range
//   void  fetch(P, kb, regs)           issue global loads of k-block kb
//   void  commit(regs, buf)            registers -> LDS buffer
//   static constexpr int aoff(s), boff(s)   immediates of k-step s (in floats)
//   void  epilogue(P, acc)
#pragma once
#include "kernels.h"

namespace ddrl {

using f32x16 = __attribute__((ext_vector_type(16))) float;
// 16-byte register vector for staged data.  NOT HIP's float4: that is a struct, a whole-struct copy
// lowers to llvm.memcpy, and an alloca touched only by memcpys is never promoted to registers
// (the prefetch buffers then live in scratch and every load is waited for immediately).
using f4 = __attribute__((ext_vector_type(4))) float;
using f2 = __attribute__((ext_vector_type(2))) float;
__device__ __forceinline__ f4 ld4(const float* p) { return *(const f4*)p; }
__device__ __forceinline__ void st4(float* p, f4 v) { *(f4*)p = v; }
__device__ __forceinline__ f4 zero4() { return (f4){0.0f, 0.0f, 0.0f, 0.0f}; }
// LDS-direct staging: one global_load_lds_dwordx4 moves 16 bytes per lane from global memory straight into
// LDS (no staging registers, no ds_write): the 64 lanes of a wave fill the 1 KB that starts at `lds_wave_base`
// (wave-uniform) in lane order.  Completion is tracked by vmcnt: the kernel waits for it (wait_vmcnt) before the
// barrier that publishes the stage.
typedef __attribute__((address_space(1))) const void gvoid_t;
typedef __attribute__((address_space(3))) void lvoid_t;
__device__ __forceinline__ void ld16_to_lds(const void* uniform_base, uint32_t lane_bytes, float* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((gvoid_t*)((const char*)uniform_base + lane_bytes), (lvoid_t*)lds_wave_base, 16, 0, 0);
}
// Contiguous tile copy, LDS-direct: quad (tid + 256 j) of the tile comes from uniform_base + off[j]; the 64
// quads a wave moves per j land 1 KB contiguous at tile + (64 wave + 256 j) quads.  Quads >= nquads are
// skipped (the lanes are masked off).
// wave index inside the workgroup as a scalar (the LDS base of an LDS-direct load must be wave-uniform)
__device__ __forceinline__ int wave_u() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }
template <int NJ>
__device__ __forceinline__ void direct_copy(const void* uniform_base, const uint32_t (&off)[NJ], float* tile, int wave, int tid, int nquads) {
#pragma unroll
  for (int j = 0; j < NJ; ++j)
    if (256 * (j + 1) <= nquads || tid + 256 * j < nquads) ld16_to_lds(uniform_base, off[j], tile + (64 * wave + 256 * j) * 4);
}
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
// First and last statement of a rarely taken arm (ragged tails): an un-speculatable marker, so that the
// compiler keeps the arm behind its wave-uniform branch instead of hoisting / sinking its instructions
// into the common path (which costs per-lane selects or register copies there).
__device__ __forceinline__ void rare_path() { asm volatile("; rare path"); }
// a store written out in the scalar-base form (global_store_dword v_off, v_data, s[base]) measured 61 fewer vector instructions per
// ConvFwd1 workgroup but ConvFwd2 2.36 -> 2.51 ms, iteration 25.18 -> 25.40 ms: not kept
__device__ __forceinline__ void st1_so(void* uniform_base, uint32_t lane_bytes, float v) {
  *(float*)((char*)uniform_base + lane_bytes) = v;
}

// leaky_relu(v) = max(v, LEAKY * v) for a slope below one: one multiply + one max (bit-identical to the
// compare/select form, signed zeros included)
__device__ __forceinline__ float leaky_f(float v) { return __builtin_fmaxf(v, v * LEAKY); }
// the same with the decision taken from bit `bit` of a sign mask (bit SET = act is not positive): g * LEAKY or g * 1 without a
// compare (bfe, bfi, mul)
__device__ __forceinline__ float leaky_bit(unsigned mask, int bit, float g) {
  const unsigned sel = (unsigned)__builtin_amdgcn_sbfe((int)mask, bit, 1);  // 0 or ~0
  return g * __uint_as_float((__float_as_uint(LEAKY) & sel) | (0x3F800000u & ~sel));
}

// float32(u8/255.0), correctly rounded, in three vector instructions (convert, multiply, fma): 1/255 is
// split into float32 hi + lo parts and x*hi + fl(x*lo) is rounded once.  Exhaustively equal to the
// correctly rounded quotient for x = 0..255 (tests/test_gpu_parity.py checks ddrl_u8_table, which runs this
// function, bit for bit against numpy).
__device__ __forceinline__ float u8_unit(unsigned b) {
  const float x = (float)b;
  const float r_hi = 0x1.010102p-8f, r_lo = -0x1.fdfdfep-33f;
  return __builtin_fmaf(x, r_hi, x * r_lo);
}

// Ops may declare `static constexpr int IGLP = 1`: use __builtin_amdgcn_iglp_opt(0) instead of the
// pinned read-ahead order (measured per op: better for the three dense-layer kernels only).
template <class Op, class = void>
struct IglpOf {
  static constexpr bool v = false;
};
template <class Op>
struct IglpOf<Op, decltype((void)Op::IGLP)> {
  static constexpr bool v = Op::IGLP != 0;
};

template <class Op>
__device__ __forceinline__ void compute_block(const Op& op, const float* __restrict__ cur, const float* lds_base,
                                              f32x16 (&acc)[Op::TM][Op::TN]) {
  // Operand pointers of this k-block.  When the two stage buffers together exceed the 64 KB reach of the
  // DS immediate offset, the (compile-time) offset of the second buffer is folded into the lane registers
  // here, once per k-block, and hidden from the compiler; otherwise it would re-base the address with a
  // vector add in front of every far read.
  const float* pa[Op::TM];
  const float* pb[Op::TN];
  if constexpr (2 * Op::STAGE * sizeof(float) > 65536) {
    // (the pinned quantity is the byte offset from the start of LDS, not a pointer: an opaque pointer
    // would lose its LDS address space and turn the reads into flat loads)
    const unsigned cur_bytes = (unsigned)((const char*)cur - (const char*)lds_base);
#pragma unroll
    for (int i = 0; i < Op::TM; ++i) {
      unsigned o = cur_bytes + 4u * (unsigned)op.abase[i];
      asm volatile("" : "+v"(o));
      pa[i] = (const float*)((const char*)lds_base + o);
    }
#pragma unroll
    for (int j = 0; j < Op::TN; ++j) {
      unsigned o = cur_bytes + 4u * (unsigned)op.bbase[j];
      asm volatile("" : "+v"(o));
      pb[j] = (const float*)((const char*)lds_base + o);
    }
  } else {
#pragma unroll
    for (int i = 0; i < Op::TM; ++i) pa[i] = cur + op.abase[i];
#pragma unroll
    for (int j = 0; j < Op::TN; ++j) pb[j] = cur + op.bbase[j];
  }
  // operands of k-step s+1 are read from LDS before the MFMAs of k-step s are issued (measured:
  // -0.75 ms per PPO iteration over the un-pinned schedule, profiles/README.md)
  float a[Op::TM], b[Op::TN];
#pragma unroll
  for (int i = 0; i < Op::TM; ++i) a[i] = pa[i][Op::aoff(0)];
#pragma unroll
  for (int j = 0; j < Op::TN; ++j) b[j] = pb[j][Op::boff(0)];
#pragma unroll
  for (int s = 0; s < Op::KSTEPS; ++s) {
    float an[Op::TM], bn[Op::TN];
    if (s + 1 < Op::KSTEPS) {
#pragma unroll
      for (int i = 0; i < Op::TM; ++i) an[i] = pa[i][Op::aoff(s + 1 < Op::KSTEPS ? s + 1 : s)];
#pragma unroll
      for (int j = 0; j < Op::TN; ++j) bn[j] = pb[j][Op::boff(s + 1 < Op::KSTEPS ? s + 1 : s)];
    }
#pragma unroll
    for (int i = 0; i < Op::TM; ++i)
#pragma unroll
      for (int j = 0; j < Op::TN; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
    if (s + 1 < Op::KSTEPS) {
#pragma unroll
      for (int i = 0; i < Op::TM; ++i) a[i] = an[i];
#pragma unroll
      for (int j = 0; j < Op::TN; ++j) b[j] = bn[j];
    }
    // pin the order the machine scheduler would otherwise undo: the LDS reads of the NEXT k-step, then
    // this k-step's MFMAs (0x100 = DS read, 0x008 = MFMA)
    if constexpr (IglpOf<Op>::v) {
      if (s == 0) __builtin_amdgcn_iglp_opt(0);  // LLVM's built-in MFMA / DS interleave for small GEMMs
    } else {
      __builtin_amdgcn_sched_group_barrier(0x100, Op::TM + Op::TN, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, Op::TM * Op::TN, 0);
    }
  }
}

// One k-block of the pipeline with the LDS buffer index as a compile-time constant: every LDS address of
// the block is then  lane register + immediate  (no per-iteration buffer arithmetic on the vector ALU).
// BUF = -1: the buffer index is the run-time argument `rbuf` (the tail of the k loop is compiled once this way).
template <class Op, int BUF>
__device__ __forceinline__ void engine2_step(Op& op, const typename Op::Params& P, int kb, int kbe, typename Op::Regs& regs,
                                             f32x16 (&acc)[Op::TM][Op::TN], float* lds2, int rbuf = 0) {
  float* cur = lds2 + (BUF < 0 ? rbuf : BUF) * Op::STAGE;
  float* nxt = lds2 + (BUF < 0 ? rbuf ^ 1 : BUF ^ 1) * Op::STAGE;
  compute_block<Op>(op, cur, lds2, acc);
  if (kb + 1 < kbe) {
    op.commit(regs, nxt);
    if (kb + 2 < kbe) op.fetch(P, kb + 2, regs);
  }
  __syncthreads();
}

template <class Op>
__global__ __launch_bounds__(Op::THREADS, 1) void engine2_kernel(typename Op::Params P) {
  extern __shared__ __attribute__((aligned(16))) float lds2[];
  Op op;
  const int tid = threadIdx.x;
  op.init(P, tid, lds2);
  typename Op::Regs regs;
  f32x16 acc[Op::TM][Op::TN];
#pragma unroll
  for (int i = 0; i < Op::TM; ++i)
#pragma unroll
    for (int j = 0; j < Op::TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

  int kb = op.kb_begin;
  const int kbe = op.kb_end;
  if (kb < kbe) {
    op.fetch(P, kb, regs);
    op.commit(regs, lds2);
    if (kb + 1 < kbe) op.fetch(P, kb + 1, regs);
  }
  __syncthreads();
  // The loop is unrolled by the two LDS buffers (engine2_step) and leaves the last one or two k-blocks to a
  // tail with a run-time buffer index (an exit in the middle of the unrolled loop would cost a copy of every
  // accumulator register per iteration).
  for (; kb + 2 < kbe; kb += 2) {
    engine2_step<Op, 0>(op, P, kb, kbe, regs, acc, lds2);
    engine2_step<Op, 1>(op, P, kb + 1, kbe, regs, acc, lds2);
  }
  for (int rbuf = 0; kb < kbe; ++kb, rbuf ^= 1) engine2_step<Op, -1>(op, P, kb, kbe, regs, acc, lds2, rbuf);
  op.epilogue(P, acc, lds2);
}

// Raises a kernel's dynamic shared-memory limit before its first launch: once per kernel (one flag per instantiation of a template)
template <auto Kernel>
inline void lds_limit_once(int bytes) {
  static bool configured = false;
  if (!configured) {
    (void)hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    configured = true;
  }
}

template <class Op>
inline void launch_engine2(dim3 grid, const typename Op::Params& p, hipStream_t st) {
  constexpr size_t bytes = (size_t)(2 * Op::STAGE) * sizeof(float);
  if (bytes > 64 * 1024) lds_limit_once<engine2_kernel<Op>>((int)bytes);
  hipLaunchKernelGGL(engine2_kernel<Op>, grid, dim3(Op::THREADS), bytes, st, p);
}

// the value the neighbouring lane (lane ^ 1) holds: one DPP move (quad_perm [1, 0, 3, 2]), no LDS traffic
__device__ __forceinline__ float lane_swap1(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, true));
}

// accumulator element r of tile (i,j) of this lane -> (row, col) inside the wave tile
__device__ __forceinline__ int acc_row(int r, int hi) { return (r & 3) + 8 * (r >> 2) + 4 * hi; }

// ---- plane scheme of the kernels with TWO fp32 operands -----------------------------------------------------------
// "f16x3": every operand as TWO scaled fp16 planes, x S = h0 + h1 to 22 bits (h0 = fp16(x S), h1 = fp16(x S - h0),
// round-to-nearest-even; S = f16_scale(largest magnitude of the tensor), a power of two, so scaling and un-scaling are
// exact), and the three products h0 g0, h0 g1, h1 g0 on v_mfma_f32_32x32x16_f16 with fp32 accumulation.  What is left out
// (h1 g1 and the representation error) is <= 3 x 2^-22 |a b| per term with zero mean; measured against float64 it does not
// show next to the rounding of the fp32 accumulation itself (tests/test_gpu_parity.py::*_is_at_least_fp32_accurate).  Half the
// matrix instructions and two thirds of the LDS planes of "bf16x6" (three bf16 planes per operand, six products; bf16 has
// fp32's exponent range and needs no scale), which was kept for accuracy attribution only and is no longer built.
// Range: with the tensor's maximum at [2^12, 2^13) every element down to 2^-16 of it keeps its 22 bits (fp16 normal range
// 2^-14), below that the absolute error stays <= 2^-25 / S, i.e. <= 2^-38 of the maximum -- far below 2^-24 of any sum that
// the large elements take part in.
using f16x2_t = __attribute__((ext_vector_type(2))) _Float16;
using h8v = __attribute__((ext_vector_type(8))) _Float16;
constexpr int NPL = 2, NPROD = 3;
using frag8 = h8v;
// the plane products of a k-group, smallest first: h1 g0, h0 g1, h0 g0 (A plane PA[m] times B plane PB[m])
constexpr int PA[NPROD] = {1, 0, 0}, PB[NPROD] = {0, 1, 0};
// FOUR VALU instructions per PAIR: v_fma_mixlo_f16 / v_fma_mixhi_f16 compute fma(x, S, c) in fp32 and write the result as fp16 into
// the low / high half of the destination, with c an fp32 or (op_sel_hi) an fp16 source: h0 = fp16(x S + 0), h1 = fp16(x S - h0)
// straight from the h0 halves.  x S and x S - h0 are exact in fp32, so each value is rounded once, as in the plain form
// (v_pk_mul_f32, v_cvt_pk_f16_f32, two v_cvt_f32_f16, v_pk_fma_f32, v_cvt_pk_f16_f32: six; element-wise C compiled to ten).
// Bit-identical to it on 12.6 M values over 60 binades and three scales; only -0 comes out as +0.  The kernels issue 3 - 8 VALU
// instructions per MFMA, most of them this split.
using f32x2_t = __attribute__((ext_vector_type(2))) float;
// the plain form (six instructions, but visible to the scheduler): same-box A/B of the two forms per kernel -- the dense forward /
// data gradient and the one-stage conv2 weight gradient of round 5 were 1-3 % faster with it, the other six with the four-instruction form
__device__ __forceinline__ void split_planes_c(float x, float y, float scale, unsigned (&p)[NPL]) {
  const f32x2_t xs = {x * scale, y * scale};
  const f16x2_t a = __builtin_convertvector(xs, f16x2_t);
  const f32x2_t r = {__builtin_fmaf(x, scale, -(float)a[0]), __builtin_fmaf(y, scale, -(float)a[1])};
  const f16x2_t b = __builtin_convertvector(r, f16x2_t);
  p[0] = __builtin_bit_cast(unsigned, a);
  p[1] = __builtin_bit_cast(unsigned, b);
}
__device__ __forceinline__ void split_planes(float x, float y, float scale, unsigned (&p)[NPL]) {
  unsigned h0, h1;
  asm("v_fma_mixlo_f16 %0, %1, %2, 0" : "=v"(h0) : "v"(x), "v"(scale));
  asm("v_fma_mixhi_f16 %0, %1, %2, 0" : "+v"(h0) : "v"(y), "v"(scale));
  asm("v_fma_mixlo_f16 %0, %1, %2, -%3 op_sel_hi:[0,0,1]" : "=v"(h1) : "v"(x), "v"(scale), "v"(h0));
  asm("v_fma_mixhi_f16 %0, %1, %2, -%3 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "+v"(h1) : "v"(y), "v"(scale), "v"(h0));
  p[0] = h0;
  p[1] = h1;
}
__device__ __forceinline__ f32x16 mfma_planes(frag8 a, frag8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
__host__ __device__ inline float plane_scale(float amax) { return f16_scale(amax); }
// MFMA fragment through the transposing LDS read (ds_read_b64_tr_b16): the lane's 8 k-values from two 8-byte reads
using s4w = __attribute__((ext_vector_type(4))) short;
__device__ __forceinline__ frag8 tr_frag(const char* lds, int off_lo, int off_hi) {
  typedef s4w __attribute__((address_space(3))) * lds_s4;
  const s4w lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4)(lds + off_lo));
  const s4w hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4)(lds + off_hi));
  typedef __attribute__((ext_vector_type(8))) short s8w;
  return __builtin_bit_cast(frag8, (s8w)__builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}
// frame bytes 0..255 are exact in fp16: the pixel operand of conv1 is ONE plane, "f16x2" = NPL products.
// Feeding them as fp16 SUBNORMALS (0x00bb = b x 2^-24: one v_perm_b32 per pair of pixels, 2^24 folded into the epilogue's scale) was
// measured and not kept: 110 M fewer vector-ALU instructions per iteration (4 %), ConvWgrad1 2.83 -> 2.78 ms, the PPO iteration
// 25.43 -> 25.37 ms (0.2 %) -- and the results are NOT the same bits: the conv1 weight gradient's mean error against float64 grows from
// 1.0 x to 1.6 x that of an fp32 evaluation (products of a subnormal pixel with the small plane of dz1 lose bits inside the pipe), which
// breaks tests/test_gpu_parity.py::test_conv1_weight_gradient_is_at_least_fp32_accurate.  Vector-ALU count is not what bounds these kernels.
__device__ __forceinline__ unsigned pixel_pair(unsigned a, unsigned b) {
  const f16x2_t v = {(_Float16)(float)a, (_Float16)(float)b};
  return __builtin_bit_cast(unsigned, v);
}
template <int QA, int QB>
__device__ __forceinline__ unsigned pixel_pair_sel(unsigned a, unsigned b) { return pixel_pair((a >> (8 * QA)) & 255u, (b >> (8 * QB)) & 255u); }
__device__ __forceinline__ unsigned short pixel_one(unsigned a) { return __builtin_bit_cast(unsigned short, (_Float16)(float)a); }
// the four pixels of one dword as two operand pairs
__device__ __forceinline__ uint2 pixel_quad(unsigned v) { return make_uint2(pixel_pair_sel<0, 1>(v, v), pixel_pair_sel<2, 3>(v, v)); }
// Frame table (include/ddrl.h ddrl_op_frame_table_*; EncCall::tab): byte offset of the plane that holds channel ch of sample b, from the
// plane base pointer.  The clamp is part of the contract of the indirect conv1 kernels: whatever the table holds, nothing outside
// [planes, planes + n_planes * 7056) is read.
constexpr int FRAME_PLANE_BYTES = 84 * 84;
__device__ __forceinline__ int64_t frame_plane_base(const int32_t* __restrict__ tab, int b, int ch, int64_t n_planes) {
  int64_t p = tab[(int64_t)b * 4 + ch];
  p = p < 0 ? 0 : p;
  p = p > n_planes - 1 ? n_planes - 1 : p;
  return p * FRAME_PLANE_BYTES;
}
__host__ __device__ inline void planes_of(float w, float scale, unsigned short (&p)[NPL]) {
  const float ws = w * scale;
  const _Float16 h0 = (_Float16)ws;
  const _Float16 h1 = (_Float16)(ws - (float)h0);
  p[0] = __builtin_bit_cast(unsigned short, h0);
  p[1] = __builtin_bit_cast(unsigned short, h1);
}
// the largest value of the wave, in every lane (ppo_math.h's wave_max is the DPP form on unsigned bit patterns: another function)
__device__ __forceinline__ float wave_fmax(float m) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
  return m;
}
// largest magnitude of the values a thread wrote -> the tensor's running maximum (float bits of non-negative values order like
// unsigned integers; the maximum does not depend on the order of the atomics, so the result is deterministic).
// One atomic per wave on ONE address serialises in the memory system (25,600 of them cost conv1's forward 6 ms): a wave
// first LOOKS at the slot and only sends the atomic when it would raise it -- after the first few waves almost none does.
// A stale look can only be too small (the slot never decreases), i.e. it costs an atomic, never a missed maximum.
__device__ __forceinline__ void amax_update(float m, float* slot) {
  m = wave_fmax(m);
  if ((threadIdx.x & 63) == 0) {
    const unsigned bits = __float_as_uint(m);
    if (bits > __hip_atomic_load((unsigned*)slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax((unsigned*)slot, bits);
  }
}

// ---- per-sample plane scales of the operator kernels (pconv.hip, plin.hip) ----------------------------------------------------
// What travels between operators is a sample's LARGEST MAGNITUDE (any upper bound works): a producer's epilogue raises it with
// amax_raise (non-negative floats order like unsigned integers: a maximum is deterministic whatever the order of the atomics), the
// consumer turns it into the power-of-two scale of the sample's fp16 planes.  An all-zero sample (the gradient of a sample whose advantage
// is exactly 0) gets the largest scale there is -- it must not pin the batch scale of a weight gradient --; 2^60 also bounds the
// products of two scales.
__device__ __forceinline__ float scale_of_amax(float m) { return m > 0.0f ? fminf(plane_scale(m), 0x1p60f) : 0x1p60f; }
__device__ __forceinline__ void amax_raise(float m, float* slot) {  // one lane; m >= 0; the slot never decreases
  const unsigned bits = __float_as_uint(m);
  if (bits > __hip_atomic_load((unsigned*)slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax((unsigned*)slot, bits);
}
__device__ __forceinline__ void lds_amax_raise(float m, float* lds_slot) { atomicMax((unsigned*)lds_slot, __float_as_uint(m)); }

}  // namespace ddrl
