// Coarse space of the two-level preconditioner of the PCG solve (pcg.h has the algorithm and the host
// restatement).  Once per solve: k_pcg_coarse_assemble forms C = Z^T S Z, then C^-1 explicitly in nct + 2 launches
// (nct = tile columns of C, at most 16): k_pcg_coarse_column once per tile column (left-looking blocked Cholesky:
// every block of the column forms its own update on the FP64 matrix cores, factors and inverts the diagonal tile in
// LDS and multiplies its tile by that inverse), k_pcg_coarse_trinv (W = L^-1, one block per tile column) and
// k_pcg_coarse_ltl (C^-1 = W^T W, one block per lower tile, diagonal tiles symmetrised, upper tiles mirrored).
// Per pass: k_pcg_coarse_restrict (r_c = Z^T r) and k_pcg_coarse_apply (y_c = C^-1 r_c and the partials of r_c.y_c).
// FP64, no atomics, every sum in a fixed order.  These buffers are the solver's own: nothing of the direct solver's
// factor, selected inverse or joint-covariance work space is touched.
#include "engine.h"
#include "tile_mma.h"

namespace bae {

using tile64::double4_t;
using tile64::each;
using tile64::zero_acc;

// One thread per entry (a, b), b <= a, of the padded C: the sum of S(i, j) over the fine rows of a and of b in list
// order (ascending natural order), S read at (max, min) of the lower storage and only inside the pattern's tiles.
// Consecutive lanes own consecutive b: the unknowns of one aggregate are neighbours in memory.
__global__ __launch_bounds__(256) void k_pcg_coarse_assemble(const double* __restrict__ A, uint32_t ld, const uint8_t* __restrict__ nz,
                                                             uint32_t nt, uint32_t nc, uint32_t ncp,
                                                             const uint32_t* __restrict__ crow_ptr,
                                                             const uint32_t* __restrict__ crow_rows, double* __restrict__ C) {
  const uint32_t b = blockIdx.x * 64 + (threadIdx.x & 63u), a = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (a >= ncp || b > a) return;
  double sum = 0.0;
  bool empty = true;
  if (a < nc) {
    const uint32_t xa = crow_ptr[a], xe = crow_ptr[a + 1], ya = crow_ptr[b], ye = crow_ptr[b + 1];
    empty = xa == xe;
    for (uint32_t x = xa; x < xe; ++x) {
      const uint32_t i = crow_rows[x];
      for (uint32_t y = ya; y < ye; ++y) {
        const uint32_t j = crow_rows[y];
        const uint32_t r = i > j ? i : j, c = i > j ? j : i;
        if (r / 64 == c / 64 || nz[(size_t)(r / 64) * nt + c / 64]) sum += A[(size_t)r * ld + c];
      }
    }
  }
  if (empty && a == b) sum = 1.0;
  C[(size_t)a * ncp + b] = sum;
  C[(size_t)b * ncp + a] = sum;
}

// acc[r][c] += sum_{m < 64} X(r, m) Y(c, m) on v_mfma_f64_16x16x4_f64 into the accumulator layout of tile_mma.h
// (zero_acc, each); unlike the staging there, the operands come from the callers' lambdas and go through LDS 16
// contraction indices at a time, index-major with stride 17.  XT / YT: the source is contiguous in its first index (r or c)
// rather than in m; it only picks which threads fetch which element.
template <bool XT, bool YT, class FX, class FY>
static __device__ __forceinline__ void cc_mma64(double4_t (&acc)[2][2], double (*Xs)[17], double (*Ys)[17], FX fx, FY fy) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int li = lane & 15, lk = lane >> 4;
  const int rb = 32 * (wave >> 1), cb = 32 * (wave & 1);
  for (int h = 0; h < 4; ++h) {
    __syncthreads();
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int e = tid + 256 * s;
      { const int r = XT ? (e & 63) : (e >> 4), m = XT ? (e >> 6) : (e & 15); Xs[r][m] = fx(r, 16 * h + m); }
      { const int c = YT ? (e & 63) : (e >> 4), m = YT ? (e >> 6) : (e & 15); Ys[c][m] = fy(c, 16 * h + m); }
    }
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const double a0 = Xs[rb + li][4 * ks + lk], a1 = Xs[rb + 16 + li][4 * ks + lk];
      const double b0 = Ys[cb + li][4 * ks + lk], b1 = Ys[cb + 16 + li][4 * ks + lk];
      acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
    }
  }
}

// Tile column k of the factor, block i - k for tile row i >= k.  Every block forms D = C_kk - sum_{m<k} L_km L_km^T
// and factors it in LDS (pcg_coarse_tile_factor: L_kk in the lower triangle, W_kk^T = L_kk^-T in the strict upper
// one, dinv = the diagonal of W_kk); block 0 stores L_kk and W_kk, block i - k stores
// L_ik = (C_ik - sum_{m<k} L_im L_km^T) W_kk^T.  A pivot that is not positive and finite sets *status.
__global__ __launch_bounds__(256) void k_pcg_coarse_column(const double* __restrict__ C, uint32_t ncp, uint32_t k,
                                                           double* __restrict__ L, double* __restrict__ W,
                                                           int32_t* __restrict__ status) {
  __shared__ double Xs[64][17], Ys[64][17];
  __shared__ double d[64][65];
  __shared__ double dinv[64];
  __shared__ int bad;
  const uint32_t tid = threadIdx.x, i = k + blockIdx.x;
  const size_t N = ncp;
  const double* Lk = L + (size_t)64 * k * N;
  double* Li = L + (size_t)64 * i * N;
  if (tid == 0) bad = 0;
  double4_t accD[2][2], accT[2][2];
  zero_acc(accD);
  zero_acc(accT);
  for (uint32_t m = 0; m < k; ++m) {
    auto fk = [&](int r, int t) { return Lk[(size_t)r * N + 64 * m + t]; };
    cc_mma64<false, false>(accD, Xs, Ys, fk, fk);
    if (i != k) {
      auto fi = [&](int r, int t) { return Li[(size_t)r * N + 64 * m + t]; };
      cc_mma64<false, false>(accT, Xs, Ys, fi, fk);
    }
  }
  each(accD, [&](int r, int c, double v) { d[r][c] = C[(size_t)(64 * k + r) * N + 64 * k + c] - v; });
  // right-looking Cholesky of the lower triangle: thread (r, cq) owns the columns c = cq (mod 4) of row r
  const uint32_t r = tid & 63u, cq = tid >> 6;
  for (uint32_t j = 0; j < 64; ++j) {
    __syncthreads();
    const double p = d[j][j];
    const bool good = p > 0.0 && pcg_finite(p);
    const double l = good ? sqrt(p) : 0.0, il = good ? 1.0 / l : 0.0;
    const double drj = d[r][j] * il;
    __syncthreads();
    if (tid == 0) { d[j][j] = l; dinv[j] = il; if (!good) bad = 1; }
    if (r > j && cq == 0) d[r][j] = drj;
    __syncthreads();
    if (r > j)
      for (uint32_t c = j + 1 + ((cq + 4u - ((j + 1) & 3u)) & 3u); c <= r; c += 4) d[r][c] -= drj * d[c][j];
  }
  __syncthreads();
  // W_kk = L_kk^-1, column c by thread c; W[r][c] is kept at d[c][r]
  if (tid < 64) {
    const uint32_t c = tid;
    for (uint32_t rr = c + 1; rr < 64; ++rr) {
      double s = d[rr][c] * dinv[c];
      for (uint32_t m = c + 1; m < rr; ++m) s += d[rr][m] * d[c][m];
      d[c][rr] = -s * dinv[rr];
    }
  }
  __syncthreads();
  if (i == k) {
    for (uint32_t e = tid; e < 4096; e += 256) {
      const uint32_t rr = e >> 6, c = e & 63u;
      Li[(size_t)rr * N + 64 * k + c] = c <= rr ? d[rr][c] : 0.0;
      W[(size_t)(64 * k + rr) * N + 64 * k + c] = c < rr ? d[c][rr] : c == rr ? dinv[c] : 0.0;
    }
    if (tid == 0 && bad) *status = 1;
    return;
  }
  // T = C_ik - accT goes through the tile's own place in L
  each(accT, [&](int rr, int c, double v) { Li[(size_t)rr * N + 64 * k + c] = C[(size_t)(64 * i + rr) * N + 64 * k + c] - v; });
  __threadfence_block();
  double4_t acc[2][2];
  zero_acc(acc);
  auto fT = [&](int rr, int t) { return Li[(size_t)rr * N + 64 * k + t]; };
  auto fW = [&](int c, int t) { return t < c ? d[t][c] : t == c ? dinv[c] : 0.0; };
  cc_mma64<false, false>(acc, Xs, Ys, fT, fW);
  each(acc, [&](int rr, int c, double v) { Li[(size_t)rr * N + 64 * k + c] = v; });
}

// W = L^-1 below the diagonal tiles, block k for tile column k: for i = k + 1 ..: W_ik = - W_ii sum_{k<=m<i} L_im W_mk
// (the W_mk of the rows above were written by this block; W_ii by k_pcg_coarse_column).
__global__ __launch_bounds__(256) void k_pcg_coarse_trinv(const double* __restrict__ L, uint32_t ncp, double* __restrict__ W) {
  __shared__ double Xs[64][17], Ys[64][17];
  const uint32_t k = blockIdx.x, nct = ncp / 64;
  const size_t N = ncp;
  for (uint32_t i = k + 1; i < nct; ++i) {
    double4_t acc[2][2];
    zero_acc(acc);
    for (uint32_t m = k; m < i; ++m) {
      auto fL = [&](int r, int t) { return L[(size_t)(64 * i + r) * N + 64 * m + t]; };
      auto fW = [&](int c, int t) { return W[(size_t)(64 * m + t) * N + 64 * k + c]; };
      cc_mma64<false, true>(acc, Xs, Ys, fL, fW);
    }
    double* Wik = W + (size_t)64 * i * N + 64 * k;
    each(acc, [&](int r, int c, double v) { Wik[(size_t)r * N + c] = v; });
    __threadfence_block();
    zero_acc(acc);
    auto fD = [&](int r, int t) { return W[(size_t)(64 * i + r) * N + 64 * i + t]; };
    auto fT = [&](int c, int t) { return Wik[(size_t)t * N + c]; };
    cc_mma64<false, true>(acc, Xs, Ys, fD, fT);
    each(acc, [&](int r, int c, double v) { Wik[(size_t)r * N + c] = -v; });
    __threadfence_block();
  }
}

// C^-1 = W^T W, one block per lower tile (i, j): sum_{m >= i} W_mi^T W_mj; a diagonal tile is stored as
// (X + X^T) / 2, an off-diagonal one also as its transpose in (j, i): C^-1 is symmetric to the bit.
__global__ __launch_bounds__(256) void k_pcg_coarse_ltl(const double* __restrict__ W, uint32_t ncp, double* __restrict__ Cinv) {
  __shared__ double Xs[64][17], Ys[64][17];
  __shared__ double o[64][65];
  const uint32_t nct = ncp / 64;
  // blockIdx.x enumerates the lower tiles row by row
  uint32_t i = 0, rest = blockIdx.x;
  while (rest > i) { rest -= i + 1; ++i; }
  const uint32_t j = rest;
  const size_t N = ncp;
  double4_t acc[2][2];
  zero_acc(acc);
  for (uint32_t m = i; m < nct; ++m) {
    auto fI = [&](int r, int t) { return W[(size_t)(64 * m + t) * N + 64 * i + r]; };
    auto fJ = [&](int c, int t) { return W[(size_t)(64 * m + t) * N + 64 * j + c]; };
    cc_mma64<true, true>(acc, Xs, Ys, fI, fJ);
  }
  each(acc, [&](int r, int c, double v) { o[r][c] = v; });
  __syncthreads();
  for (uint32_t e = threadIdx.x; e < 4096; e += 256) {
    const uint32_t r = e >> 6, c = e & 63u;
    if (i == j) Cinv[(size_t)(64 * i + r) * N + 64 * i + c] = 0.5 * (o[r][c] + o[c][r]);
    else {
      Cinv[(size_t)(64 * i + r) * N + 64 * j + c] = o[r][c];
      Cinv[(size_t)(64 * j + r) * N + 64 * i + c] = o[c][r];
    }
  }
}

// r_c = Z^T r: one lane per coarse unknown over its list of fine rows; the padding of r_c is zero
__global__ __launch_bounds__(256) void k_pcg_coarse_restrict(uint32_t nc, uint32_t ncp, const PcgState* __restrict__ st,
                                                             const uint32_t* __restrict__ crow_ptr,
                                                             const uint32_t* __restrict__ crow_rows,
                                                             const double* __restrict__ r, double* __restrict__ rc) {
  if (st->done) return;
  const uint32_t c = blockIdx.x * 256 + threadIdx.x;
  if (c >= ncp) return;
  double s = 0.0;
  if (c < nc)
    for (uint32_t e = crow_ptr[c]; e < crow_ptr[c + 1]; ++e) s += r[crow_rows[e]];
  rc[c] = s;
}

// y_c = C^-1 r_c, one wavefront per row: lane t sums the columns t, t + 64, ..; the tree; the row's term of r_c.y_c
__global__ __launch_bounds__(64) void k_pcg_coarse_apply(uint32_t ncp, const PcgState* __restrict__ st,
                                                         const double* __restrict__ Cinv, const double* __restrict__ rc,
                                                         double* __restrict__ yc, double* __restrict__ ryc_part) {
  if (st->done) return;
  __shared__ double red[64];
  const uint32_t row = blockIdx.x, t = threadIdx.x;
  const double* a = Cinv + (size_t)row * ncp;
  double s = 0.0;
  for (uint32_t m = t; m < ncp; m += 64) s += a[m] * rc[m];
  red[t] = s;
  __syncthreads();
  for (int w = 32; w > 0; w >>= 1) {
    if ((int)t < w) red[t] += red[t + w];
    __syncthreads();
  }
  if (t == 0) { yc[row] = red[0]; ryc_part[row] = rc[row] * red[0]; }
}

// The coarse matrix of `plan` from the system in dA and its explicit inverse, into the work space (sized by
// pcg_solve_device); the status word w.status[1] is set on a pivot that is not positive.
int pcg_coarse_setup_device(Engine* e, const double* dA, uint32_t ld, const PcgPlan& plan) {
  Engine::PcgWork& w = e->pcg;
  hipStream_t s = e->stream;
  const uint32_t ncp = plan.ncp, nct = ncp / 64;
  hipLaunchKernelGGL(k_pcg_coarse_assemble, dim3(nct, ncp / 4), dim3(256), 0, s, dA, ld, (const uint8_t*)w.nz.p, plan.nt, plan.nc,
                     ncp, (const uint32_t*)w.crow_ptr.p, (const uint32_t*)w.crow_rows.p, w.C.p);
  for (uint32_t k = 0; k < nct; ++k)
    hipLaunchKernelGGL(k_pcg_coarse_column, dim3(nct - k), dim3(256), 0, s, (const double*)w.C.p, ncp, k, w.Lc.p, w.Wc.p,
                       w.status.p + 1);
  hipLaunchKernelGGL(k_pcg_coarse_trinv, dim3(nct), dim3(256), 0, s, (const double*)w.Lc.p, ncp, w.Wc.p);
  hipLaunchKernelGGL(k_pcg_coarse_ltl, dim3(nct * (nct + 1) / 2), dim3(256), 0, s, (const double*)w.Wc.p, ncp, w.Cinv.p);
  BAE_HIP(hipGetLastError());
  return 0;
}

void pcg_coarse_apply_device(Engine* e, const PcgPlan& plan, const PcgState* st, const double* r) {
  Engine::PcgWork& w = e->pcg;
  hipLaunchKernelGGL(k_pcg_coarse_restrict, dim3((plan.ncp + 255) / 256), dim3(256), 0, e->stream, plan.nc, plan.ncp, st,
                     (const uint32_t*)w.crow_ptr.p, (const uint32_t*)w.crow_rows.p, r, w.rc.p);
  hipLaunchKernelGGL(k_pcg_coarse_apply, dim3(plan.nc), dim3(64), 0, e->stream, plan.ncp, st, (const double*)w.Cinv.p,
                     (const double*)w.rc.p, w.yc.p, w.ryc_part.p);
}

}  // namespace bae
