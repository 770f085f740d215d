// Filing the terminal observations of truncated episodes (include/ddrl.h ddrl_op_file_flagged_rows): the rows of
// the envs whose info word carries a flag move into a small per-env pool, dst[count[n]][n] <- src[n], without a scan, an atomic or a host
// read-back.  One 256-thread workgroup owns env n, so count[n] has one reader-writer: every thread loads it, and only behind a barrier
// does thread 0 store the new count and the slot.  A part whose rows are a multiple of 16 bytes on 16-byte aligned bases moves in 16-byte
// units (the laser's 3,840 bytes: 240 units, the map's 27,648: 1,728), any other in 4-byte units (the vector's 20 bytes).
#include "rows.h"

namespace ddrl {

constexpr int FILE_THREADS = 256, FILE_MAX_PARTS = 4;

struct FileParts {  // part k: src [N][w] -> dst [S][N][w] floats; vec: moved in 16-byte units
  const float* src[FILE_MAX_PARTS];
  float* dst[FILE_MAX_PARTS];
  int w[FILE_MAX_PARTS];
  int vec[FILE_MAX_PARTS];
  int n;
};

__global__ __launch_bounds__(FILE_THREADS) void file_flagged_rows_kernel(const int32_t* __restrict__ info, int mask, int N, int S,
                                                                         FileParts parts, int32_t* __restrict__ count,
                                                                         int32_t* __restrict__ slot_out) {
  const int n = blockIdx.x, tid = threadIdx.x;
  const bool flagged = (info[n] & mask) != 0;  // uniform over the workgroup, as everything that follows from it
  if (!flagged) {
    if (tid == 0) slot_out[n] = -1;
    return;
  }
  const int c = count[n];
  __syncthreads();  // every thread holds the old count
  const bool room = c >= 0 && c < S;
  if (tid == 0) {
    count[n] = (int)((uint32_t)c + 1u);  // keeps counting past S: an overflow stays visible
    slot_out[n] = room ? c : -1;
  }
  if (!room) return;
  const int64_t row = (int64_t)c * N + n;
#pragma unroll  // a compile-time k: the parts stay in the kernel's argument segment
  for (int k = 0; k < FILE_MAX_PARTS; ++k) {
    if (k >= parts.n) break;
    const int w = parts.w[k];
    if (parts.vec[k]) {
      const uint4* __restrict__ s = reinterpret_cast<const uint4*>(parts.src[k] + (int64_t)n * w);
      uint4* __restrict__ d = reinterpret_cast<uint4*>(parts.dst[k] + row * w);
      for (int u = tid; u < w / 4; u += FILE_THREADS) d[u] = s[u];
    } else {
      const float* __restrict__ s = parts.src[k] + (int64_t)n * w;
      float* __restrict__ d = parts.dst[k] + row * w;
      for (int u = tid; u < w; u += FILE_THREADS) d[u] = s[u];
    }
  }
}

}  // namespace ddrl

using namespace ddrl;

extern "C" {

// every check comes before the first HIP call: a host without a GPU gets the same answers
int32_t ddrl_op_file_flagged_rows(const int32_t* info, int32_t mask, int32_t N, int32_t S, int32_t n_parts, const float* const* src,
                                  float* const* dst, const int32_t* widths, int32_t* count, int32_t* slot_out, void* stream) {
  if (!info || !src || !dst || !widths || !count || !slot_out || mask == 0 || N < 1 || S < 1 || n_parts < 1 || n_parts > FILE_MAX_PARTS)
    return DDRL_ERR_INVALID_ARG;
  if (((uintptr_t)info | (uintptr_t)count | (uintptr_t)slot_out) & 3) return DDRL_ERR_INVALID_ARG;
  FileParts parts = {};
  parts.n = n_parts;
  const void* reads[1 + FILE_MAX_PARTS] = {info};
  uint64_t reads_b[1 + FILE_MAX_PARTS] = {(uint64_t)N * 4};
  void* writes[2 + FILE_MAX_PARTS] = {count, slot_out};
  uint64_t writes_b[2 + FILE_MAX_PARTS] = {(uint64_t)N * 4, (uint64_t)N * 4};
  for (int k = 0; k < n_parts; ++k) {
    if (!src[k] || !dst[k] || widths[k] < 1 || (((uintptr_t)src[k] | (uintptr_t)dst[k]) & 3)) return DDRL_ERR_INVALID_ARG;
    parts.src[k] = src[k];
    parts.dst[k] = dst[k];
    parts.w[k] = widths[k];
    parts.vec[k] = (widths[k] % 4 == 0 && aligned16(src[k]) && aligned16(dst[k])) ? 1 : 0;
    reads[1 + k] = src[k];
    reads_b[1 + k] = (uint64_t)N * widths[k] * 4;
    writes[2 + k] = dst[k];
    writes_b[2 + k] = (uint64_t)S * N * widths[k] * 4;
  }
  if (!reads_and_writes_apart(reads, reads_b, 1 + n_parts, writes, writes_b, 2 + n_parts)) return DDRL_ERR_INVALID_ARG;
  hipLaunchKernelGGL(file_flagged_rows_kernel, dim3((unsigned)N), dim3(FILE_THREADS), 0, (hipStream_t)stream, info, mask, N, S, parts, count,
                     slot_out);
  return launch_status();
}

}  // extern "C"
