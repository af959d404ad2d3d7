// The 64 x 64 FP64 tile product of the kernels that read the kept factor or the assembled S (k_selinv.hip,
// k_jointcov.hip, k_factorsolve.hip, k_pcg_panel.hip; the accumulator layout also serves k_pcg_coarse.hip): the
// loads and stores of a chunk and the pipelined K loop (accumulate_chunks).  Device only.
//
// One workgroup of 256 threads forms one output tile on v_mfma_f64_16x16x4_f64.  Wave w owns the 32 x 32 quarter
// at rows rb = 32 (w >> 1), columns cb = 32 (w & 1), as 2 x 2 MFMA blocks acc[ti][tj] of 16 x 16.  Lane l holds of
// block (ti, tj) the four elements reg = 0 .. 3 at
//     row = rb + 16 ti + (l >> 4) + 4 reg,   column = cb + 16 tj + (l & 15).
// The operands go through LDS 32 k-rows at a time, k-major ([k][index]); the callers fetch the next chunk into
// registers (Chunk) while the matrix cores work on this one.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bae {
namespace tile64 {

const int TB = 64;         // tile size
const int KCH = 32;        // k-rows per LDS chunk
const int LDS_LD = TB + 4; // LDS row stride (doubles)
typedef double double4_t __attribute__((ext_vector_type(4)));

// one chunk of 32 k-rows of both operands, k-major
struct Lds {
  double X[KCH][LDS_LD];
  double Y[KCH][LDS_LD];
};

// Thread t moves 4 double2 of a 32 x 64 chunk: element pair e = 2 t + 512 s (s < 4).
//  k-major source (rows = k, stride `ld`, 64 contiguous indices):   k = e / 64, index = e % 64
//  index-major source (rows = index, 64 contiguous k):              index = e / 32, k = e % 32
struct Chunk {
  double2 v[4];
};
__device__ __forceinline__ void load_kmajor(Chunk& c, const double* src, size_t ld, int k0) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int e = 2 * tid + 512 * s;
    c.v[s] = *reinterpret_cast<const double2*>(src + (size_t)(k0 + e / TB) * ld + (e % TB));
  }
}
__device__ __forceinline__ void load_imajor(Chunk& c, const double* src, size_t ld, int k0) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int e = 2 * tid + 512 * s;
    c.v[s] = *reinterpret_cast<const double2*>(src + (size_t)(e / KCH) * ld + k0 + (e % KCH));
  }
}
__device__ __forceinline__ void store_kmajor(const Chunk& c, double (*Z)[LDS_LD]) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int e = 2 * tid + 512 * s;
    Z[e / TB][e % TB] = c.v[s].x;
    Z[e / TB][e % TB + 1] = c.v[s].y;
  }
}
__device__ __forceinline__ void store_imajor(const Chunk& c, double (*Z)[LDS_LD]) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int e = 2 * tid + 512 * s;
    Z[e % KCH][e / KCH] = c.v[s].x;
    Z[e % KCH + 1][e / KCH] = c.v[s].y;
  }
}

__device__ __forceinline__ void zero_acc(double4_t (&acc)[2][2]) {
#pragma unroll
  for (int ti = 0; ti < 2; ++ti)
#pragma unroll
    for (int tj = 0; tj < 2; ++tj) acc[ti][tj] = (double4_t){0.0, 0.0, 0.0, 0.0};
}

// acc[i][j] += sum_k X[k][i] Y[k][j], 32 k
__device__ __forceinline__ void mma_chunk(double4_t (&acc)[2][2], const Lds& s) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int li = lane & 15, lk = lane >> 4;
  const int rb = 32 * (wave >> 1), cb = 32 * (wave & 1);
#pragma unroll
  for (int ks = 0; ks < KCH / 4; ++ks) {
    const double a0 = s.X[4 * ks + lk][rb + li];
    const double a1 = s.X[4 * ks + lk][rb + 16 + li];
    const double b0 = s.Y[4 * ks + lk][cb + li];
    const double b1 = s.Y[4 * ks + lk][cb + 16 + li];
    acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
    acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
    acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
    acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
  }
}

// The pipelined K loop of every tile product: acc += sum over nch chunks of X^T Y.  fetch(ch) loads chunk ch into the
// caller's Chunk registers, stage(ch) stores those registers to s.X and s.Y; chunk ch + 1 is fetched while the
// matrix cores work on chunk ch.  Every thread of the workgroup calls it with the same nch (it owns the barriers).
template <class Fetch, class Stage>
__device__ __forceinline__ void accumulate_chunks(double4_t (&acc)[2][2], Lds& s, uint32_t nch, Fetch fetch, Stage stage) {
  if (nch) fetch(0);
  for (uint32_t ch = 0; ch < nch; ++ch) {
    stage(ch);
    __syncthreads();
    if (ch + 1 < nch) fetch(ch + 1);
    mma_chunk(acc, s);
    __syncthreads();
  }
}

// 64 x 64 tile out of the accumulators, row stride ld
__device__ __forceinline__ void store_tile(double* __restrict__ dst, size_t ld, const double4_t (&v)[2][2]) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int li = lane & 15, lk = lane >> 4;
  const int rb = 32 * (wave >> 1), cb = 32 * (wave & 1);
#pragma unroll
  for (int ti = 0; ti < 2; ++ti)
#pragma unroll
    for (int tj = 0; tj < 2; ++tj)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int r = rb + 16 * ti + lk + 4 * reg, c = cb + 16 * tj + li;
        dst[(size_t)r * ld + c] = v[ti][tj][reg];
      }
}

// f(row, column, value) for every element of the accumulators this thread holds
template <class F>
__device__ __forceinline__ void each(const double4_t (&acc)[2][2], F f) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int li = lane & 15, lk = lane >> 4;
  const int rb = 32 * (wave >> 1), cb = 32 * (wave & 1);
#pragma unroll
  for (int ti = 0; ti < 2; ++ti)
#pragma unroll
    for (int tj = 0; tj < 2; ++tj)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) f(rb + 16 * ti + lk + 4 * reg, cb + 16 * tj + li, acc[ti][tj][reg]);
}

}  // namespace tile64
}  // namespace bae
