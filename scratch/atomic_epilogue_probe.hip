// Probe for the C epilogue of k_update128 (k_chol.hip): read-modify-write against no-return FP64 adds.
// 512 workgroups of 256 threads, two per CU (the kernel's 73 856 B of LDS pin that), each `reps` times: a loop of
// v_mfma_f64_16x16x4_f64 into 16 accumulator tiles per wave, then the epilogue of a 128x128 block of a matrix with
// leading dimension 60 032 — 64 instructions per wave, 16 lanes contiguous (128 B), four rows per instruction.
//   form 0  no epilogue (the accumulators go to a sink once, at the end)
//   form 1  load / subtract / store as in the kernel: row 0 of MFMA tiles fetched under the last 64 MFMAs, two rows
//           in flight
//   form 2  unsafeAtomicAdd(C, -acc): global_atomic_add_f64 without return
// "duty" runs: 4096 MFMAs per wave and block (the pipe time of a 16-column block), the workgroups' first blocks
// staggered, so a CU meets one 128 KiB burst per ~110 us as in the bulk launch.  "burst" runs: no MFMAs, epilogues
// back to back on every CU: the chip-wide rate of the form.
// Per wave: cycles (s_memtime) and 100 MHz ticks from the first epilogue instruction to the issue of the last.
// Also: the memory-side add against the host's c - a, bitwise, on signed zeros, subnormals, infinities and random values.
// Build: hipcc -O3 --offload-arch=gfx950 -mllvm -amdgpu-mfma-vgpr-form atomic_epilogue_probe.hip -o atomic_epilogue_probe
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>
typedef double double4_t __attribute__((ext_vector_type(4)));

#define CHECK(x)                                                                       \
  do {                                                                                 \
    hipError_t e_ = (x);                                                               \
    if (e_ != hipSuccess) { printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); exit(2); } \
  } while (0)

static const uint32_t LD = 60032, BCOLS = LD / 128, WGS = 512;

template <int FORM>
__global__ void __launch_bounds__(256, 2)
k_probe(double* __restrict__ Cm, uint32_t ld, uint32_t bcols, uint32_t nblocks, int reps, int nmfma, int stagger,
        unsigned long long* __restrict__ rec, double* __restrict__ sink, double a0, double b0) {
  __shared__ double lds[9232];  // 73 856 B: two workgroups per CU, as k_update128
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int li = lane & 15, lk = lane >> 4;
  const int rb = 64 * (wave >> 1), cb = 64 * (wave & 1);
  lds[tid] = a0 * tid;
  __syncthreads();
  const double a = a0 + lds[(tid * 7) & 255] * 1e-12, b = b0 + lane * 1e-9;
  double4_t acc[4][4];
#pragma unroll
  for (int ti = 0; ti < 4; ++ti)
#pragma unroll
    for (int tj = 0; tj < 4; ++tj) acc[ti][tj] = (double4_t){0.0, 0.0, 0.0, 0.0};
#define P_MFMA16                                                                                   \
  _Pragma("unroll") for (int t = 0; t < 16; ++t)                                                   \
    acc[t >> 2][t & 3] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[t >> 2][t & 3], 0, 0, 0);
#define P_SB __builtin_amdgcn_sched_barrier(0)
  if (stagger) {
    const int extra = (int)((blockIdx.x * 7919u) % (uint32_t)(nmfma > 0 ? nmfma : 1)) / 16;
    for (int it = 0; it < extra; ++it) { P_MFMA16 }
  }
  for (int rep = 0; rep < reps; ++rep) {
    const uint32_t q = (uint32_t)rep * gridDim.x + blockIdx.x;
    if (q >= nblocks) break;  // (never: the host sizes the matrix for reps x grid blocks)
    double* Aic = Cm + ((size_t)(q / bcols) * 128) * ld + (size_t)(q % bcols) * 128;
    for (int it = 0; it < nmfma / 16 - 4; ++it) { P_MFMA16 }
    unsigned long long t0 = 0, w0 = 0;
    if constexpr (FORM == 1) {
      double4_t cva[4], cvb[4];
#define P_CLOAD(CV, TI)                                                              \
  _Pragma("unroll") for (int tj = 0; tj < 4; ++tj)                                   \
    _Pragma("unroll") for (int reg = 0; reg < 4; ++reg)                              \
      CV[tj][reg] = Aic[(size_t)(rb + 16 * (TI) + lk + 4 * reg) * ld + cb + 16 * tj + li];
#define P_CSTORE(CV, TI)                                                             \
  _Pragma("unroll") for (int tj = 0; tj < 4; ++tj)                                   \
    _Pragma("unroll") for (int reg = 0; reg < 4; ++reg)                              \
      Aic[(size_t)(rb + 16 * (TI) + lk + 4 * reg) * ld + cb + 16 * tj + li] = CV[tj][reg] - acc[TI][tj][reg];
      P_SB;
      t0 = __builtin_readcyclecounter(); w0 = wall_clock64();
      P_CLOAD(cva, 0);
      P_SB;
      if (nmfma > 0) for (int it = 0; it < 4; ++it) { P_MFMA16 }
      P_SB;
      P_CLOAD(cvb, 1); P_SB;
      P_CSTORE(cva, 0); P_SB;
      P_CLOAD(cva, 2); P_SB;
      P_CSTORE(cvb, 1); P_SB;
      P_CLOAD(cvb, 3); P_SB;
      P_CSTORE(cva, 2);
      P_CSTORE(cvb, 3);
      P_SB;
#undef P_CLOAD
#undef P_CSTORE
    } else {
      if (nmfma > 0) for (int it = 0; it < 4; ++it) { P_MFMA16 }
      P_SB;
      t0 = __builtin_readcyclecounter(); w0 = wall_clock64();
      if constexpr (FORM == 2) {
#pragma unroll
        for (int ti = 0; ti < 4; ++ti)
#pragma unroll
          for (int tj = 0; tj < 4; ++tj)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg)
              unsafeAtomicAdd(&Aic[(size_t)(rb + 16 * ti + lk + 4 * reg) * ld + cb + 16 * tj + li], -acc[ti][tj][reg]);
        P_SB;
      }
    }
    const unsigned long long t1 = __builtin_readcyclecounter(), w1 = wall_clock64();
    if (lane == 0) {
      rec[((size_t)q * 4 + wave) * 2] = t1 - t0;
      rec[((size_t)q * 4 + wave) * 2 + 1] = w1 - w0;
    }
  }
  if constexpr (FORM == 0) {
    double s = 0;
#pragma unroll
    for (int ti = 0; ti < 4; ++ti)
#pragma unroll
      for (int tj = 0; tj < 4; ++tj) s += acc[ti][tj][0] + acc[ti][tj][1] + acc[ti][tj][2] + acc[ti][tj][3];
    sink[blockIdx.x * 256 + tid] = s;
  }
#undef P_MFMA16
#undef P_SB
}

__global__ void k_fill(double* p, size_t n, double v) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = v;
}
__global__ void k_special(double* c, const double* a, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) unsafeAtomicAdd(&c[i], -a[i]);
}

struct Bufs { double* C; size_t c_elems; uint32_t nblocks; unsigned long long* rec; double* sink; };

template <int FORM>
static void run(const char* name, const Bufs& B, int reps, int nmfma, int stagger, std::vector<double>* block0) {
  const uint32_t nblocks = (uint32_t)reps * WGS;
  if (nblocks > B.nblocks) { printf("matrix too small\n"); exit(2); }
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
  float ms = 0;
  for (int pass = 0; pass < 2; ++pass) {  // the first pass warms up
    hipLaunchKernelGGL(k_fill, dim3(2048), dim3(256), 0, 0, B.C, B.c_elems, 1.0);
    CHECK(hipMemset(B.rec, 0, (size_t)B.nblocks * 8 * sizeof(unsigned long long)));
    CHECK(hipEventRecord(e0));
    hipLaunchKernelGGL(k_probe<FORM>, dim3(WGS), dim3(256), 0, 0, B.C, LD, BCOLS, B.nblocks, reps, nmfma, stagger, B.rec,
                       B.sink, 1.0000001, 1e-3);
    CHECK(hipEventRecord(e1));
    CHECK(hipEventSynchronize(e1));
    CHECK(hipGetLastError());
    CHECK(hipEventElapsedTime(&ms, e0, e1));
  }
  std::vector<unsigned long long> rec((size_t)nblocks * 8);
  CHECK(hipMemcpy(rec.data(), B.rec, rec.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  double sc = 0, sw = 0, mc = 0;
  for (size_t i = 0; i < (size_t)nblocks * 4; ++i) {
    sc += (double)rec[2 * i]; sw += (double)rec[2 * i + 1];
    mc = std::max(mc, (double)rec[2 * i + 1]);
  }
  const double nw = (double)nblocks * 4, bytes = (double)nblocks * 128 * 128 * 8;
  std::vector<unsigned long long> cyc((size_t)nblocks * 4);
  for (size_t i = 0; i < cyc.size(); ++i) cyc[i] = rec[2 * i];
  std::sort(cyc.begin(), cyc.end());
  printf("%-28s kernel %8.3f ms | epilogue per wave: %9.0f counter ticks mean (p10 %llu, p50 %llu, p90 %llu, p99 %llu), "
         "%7.2f us mean, %7.2f us max | C bytes %.3f GB -> %7.3f TB/s of C over the kernel\n",
         name, ms, sc / nw, cyc[cyc.size() / 10], cyc[cyc.size() / 2], cyc[cyc.size() * 9 / 10], cyc[cyc.size() * 99 / 100],
         sw / nw * 0.01, mc * 0.01, bytes * 1e-9, bytes / (ms * 1e-3) * 1e-12);
  printf("    mean ticks by block of the workgroup:");
  for (int rep = 0; rep < reps; ++rep) {
    double s = 0;
    for (size_t i = (size_t)rep * WGS * 4; i < (size_t)(rep + 1) * WGS * 4; ++i) s += (double)rec[2 * i];
    printf(" %8.0f", s / (WGS * 4.0));
  }
  printf("\n");
  if (block0) {
    block0->resize(128 * 128);
    CHECK(hipMemcpy2D(block0->data(), 128 * sizeof(double), B.C, (size_t)LD * sizeof(double), 128 * sizeof(double), 128,
                      hipMemcpyDeviceToHost));
  }
  CHECK(hipEventDestroy(e0)); CHECK(hipEventDestroy(e1));
}

static int special_values() {
  std::vector<double> c, a;
  const double dn = std::numeric_limits<double>::denorm_min(), mn = std::numeric_limits<double>::min();
  const double inf = std::numeric_limits<double>::infinity();
  const double cs[] = {0.0, -0.0, dn, -dn, 3 * dn, mn, -mn, 1.5 * mn, mn * 0.5, 1.0, -1.0, 1e308, -1e308, inf, -inf, 1e-310};
  for (double x : cs)
    for (double y : cs) { c.push_back(x); a.push_back(y); }
  srand(7);
  for (int i = 0; i < 768; ++i) {
    const double x = ldexp((double)rand() / RAND_MAX - 0.5, rand() % 80 - 40), y = ldexp((double)rand() / RAND_MAX - 0.5, rand() % 80 - 40);
    c.push_back(x); a.push_back(i % 3 == 0 ? x * (1.0 + 1e-15 * (rand() % 100)) : y);  // every third: heavy cancellation
  }
  const int n = (int)c.size();
  double *dc, *da;
  CHECK(hipMalloc(&dc, n * sizeof(double))); CHECK(hipMalloc(&da, n * sizeof(double)));
  CHECK(hipMemcpy(dc, c.data(), n * sizeof(double), hipMemcpyHostToDevice));
  CHECK(hipMemcpy(da, a.data(), n * sizeof(double), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_special, dim3((n + 255) / 256), dim3(256), 0, 0, dc, da, n);
  std::vector<double> r(n);
  CHECK(hipMemcpy(r.data(), dc, n * sizeof(double), hipMemcpyDeviceToHost));
  int bad = 0;
  for (int i = 0; i < n; ++i) {
    const volatile double want = c[i] - a[i];
    const double w = want;
    const bool both_nan = std::isnan(w) && std::isnan(r[i]);
    if (!both_nan && memcmp(&w, &r[i], 8) != 0) {
      if (bad < 8) printf("  special value mismatch: c %a a %a host %a device %a\n", c[i], a[i], w, r[i]);
      ++bad;
    }
  }
  printf("memory-side add against host c - a, bitwise: %d values, %d mismatches (NaN results compared as NaN)\n", n, bad);
  CHECK(hipFree(dc)); CHECK(hipFree(da));
  return bad;
}

int main() {
  const int reps = 6;
  Bufs B;
  B.nblocks = (uint32_t)reps * WGS;
  const uint32_t brows = (B.nblocks + BCOLS - 1) / BCOLS;
  B.c_elems = (size_t)brows * 128 * LD;
  CHECK(hipMalloc(&B.C, B.c_elems * sizeof(double)));
  CHECK(hipMalloc(&B.rec, (size_t)B.nblocks * 8 * sizeof(unsigned long long)));
  CHECK(hipMalloc(&B.sink, (size_t)WGS * 256 * sizeof(double)));
  printf("matrix %u x %u doubles (%.1f MB), %u workgroups x %d blocks of 128 x 128\n", brows * 128, LD,
         B.c_elems * 8e-6, WGS, reps);
  const int bad = special_values();
  std::vector<double> b1, b2;
  run<0>("duty  none", B, reps, 4096, 1, nullptr);
  run<1>("duty  load/subtract/store", B, reps, 4096, 1, &b1);
  run<2>("duty  no-return f64 add", B, reps, 4096, 1, &b2);
  run<1>("duty  load/subtract/store", B, reps, 4096, 1, nullptr);
  run<2>("duty  no-return f64 add", B, reps, 4096, 1, nullptr);
  printf("block 0 after one duty launch, the two forms bitwise equal: %s\n",
         memcmp(b1.data(), b2.data(), b1.size() * 8) == 0 ? "yes" : "NO");
  run<1>("burst load/subtract/store", B, reps, 0, 0, nullptr);
  run<2>("burst no-return f64 add", B, reps, 0, 0, nullptr);
  CHECK(hipFree(B.C)); CHECK(hipFree(B.rec)); CHECK(hipFree(B.sink));
  return bad ? 1 : 0;
}
