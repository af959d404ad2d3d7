// gfx950 kernels of ba_hip_refine_poses: per-pose Levenberg-Marquardt refinement with the landmarks held fixed, to
// convergence inside one launch (resect.h holds the rules).
//
// The decoupling runs across the engine's layout: observations are sorted by landmark, a pose's observations are
// scattered, and it has hundreds to thousands of them.  So: one workgroup of 256 threads per requested pose (the grid is
// the id list), reading through the per-pose list of build_pose_obs_lists.
//   slots      thread t owns list entries t, t + 256, ...  k_resect<1> and k_resect<4> keep pixel, weight, world point
//              and camera id of their 1 or 4 entries in registers across all iterations (poses of up to 256 and 1 024
//              observations); k_resect<0> streams: it re-reads through the list at every evaluation, and keeps the
//              used flag of the starting pose in one byte per list entry of the call's work space.
//   reduction  31 values (the 29 sums [H | g | E | F], the used count, the smallest depth): an xor butterfly within the
//              wave, then one LDS row per wave, double-buffered so that one __syncthreads() per evaluation suffices;
//              every thread adds the four rows in wave order.  All threads then hold identical totals, take the same
//              decision and solve the same 6 x 6 system: no broadcast, no atomics, a block-uniform loop, and an order
//              that does not depend on scheduling, so two calls give identical bits.
// T_sw of the trial pose is recomputed inside the kernel from the trial T_wp and the camera records.  FP64 throughout.
#include "engine.h"
#include "dmath.h"

using namespace bad;

namespace bae {

static constexpr int kRsThreads = 256, kRsWaves = kRsThreads / 64;

struct RsOb {
  double z[2], w0, X[4];
  uint32_t cam;
};

template <int SLOTS, bool FOV>
__global__ void __launch_bounds__(kRsThreads)
k_resect(RsOptions opt, const uint32_t* __restrict__ ids, const uint32_t* __restrict__ rows,
         const uint32_t* __restrict__ ptr, const uint32_t* __restrict__ idx, const double* __restrict__ obs_z,
         const double* __restrict__ obs_w0, const uint32_t* __restrict__ obs_cam, const uint32_t* __restrict__ obs_lm,
         const double* __restrict__ x_held, const double* __restrict__ cam, const double* __restrict__ pose_cam,
         const double* __restrict__ state, uint8_t* __restrict__ used_flag, double* __restrict__ res,
         double* __restrict__ t7, double* __restrict__ info) {
  __shared__ double red[2][kRsWaves][kRsRed];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const uint32_t p = ids[blockIdx.x], row = rows[blockIdx.x];
  const uint32_t a0 = ptr[p], k = ptr[p + 1] - a0;
  const double* ipose = pose_cam ? pose_cam + (size_t)p * 4 : nullptr;   // per-pose intrinsics, as k_linearize

  auto load = [&](uint32_t j) {
    RsOb o;
    const uint32_t a = idx[a0 + j];
    o.z[0] = obs_z[2 * (size_t)a]; o.z[1] = obs_z[2 * (size_t)a + 1];
    o.w0 = obs_w0[a];
    o.cam = obs_cam[a];
    const double* x = x_held + (size_t)obs_lm[a] * 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) o.X[i] = x[i];
    return o;
  };
  constexpr int NS = SLOTS > 0 ? SLOTS : 1;
  RsOb slot[NS];
  unsigned used_bits = 0;
  if constexpr (SLOTS > 0) {
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
      const uint32_t j = tid + kRsThreads * s;
      slot[s] = load(j < k ? j : 0);   // (k >= 1 in every launched block; entries past k are never evaluated)
    }
  }

  int buf = 0;
  // [H | g | E] (masked), used count and smallest depth at pose7; first: the starting pose, which decides what is used
  auto sums_at = [&](const double* pose7, bool first, double* tot, unsigned* used, double* depth) {
    double acc[kRsSums + 2];
#pragma unroll
    for (int i = 0; i < kRsSums + 1; ++i) acc[i] = 0.0;
    acc[kRsSums + 1] = rs_inf();
    uint32_t c_have = 0;
    Rt wp, sw;
    rs_sensor(pose7, cam + 28, &wp, &sw);
    auto one = [&](const RsOb& o, bool use) {
      if (o.cam != c_have) {
        c_have = o.cam;
        rs_sensor(pose7, cam + (size_t)c_have * kCamRec + 28, &wp, &sw);
      }
      if (first) use = rs_usable(rs_point(sw, o.X));
      if (use) {
        const double* cp = cam + (size_t)o.cam * kCamRec;
        const double* ip = ipose ? ipose : cp;
        Cam cm = {ip[0], ip[1], ip[2], ip[3], 0.0, 0};
        if constexpr (FOV) { cm.w = cp[35]; cm.model = cp[36] != 0.0 ? 1 : 0; }
        M3 R_sv;
#pragma unroll
        for (int i = 0; i < 9; ++i) R_sv.m[i] = cp[16 + i];
        double v[kRsSums];
        const double dep = rs_eval(cm, o.z, o.w0, o.X, wp, sw, R_sv, opt.huber_width, !first, v);
#pragma unroll
        for (int i = 0; i < kRsSums; ++i) acc[i] += v[i];
        acc[kRsSums] += 1.0;
        acc[kRsSums + 1] = dep < acc[kRsSums + 1] ? dep : acc[kRsSums + 1];
      }
      return use;
    };
    if constexpr (SLOTS > 0) {
#pragma unroll
      for (int s = 0; s < SLOTS; ++s)
        if ((uint32_t)(tid + kRsThreads * s) < k) {
          const bool use = one(slot[s], (used_bits >> s & 1u) != 0);
          if (first && use) used_bits |= 1u << s;
        }
    } else {
      for (uint32_t j = tid; j < k; j += kRsThreads) {
        const bool use = one(load(j), first ? false : used_flag[a0 + j] != 0);
        if (first) used_flag[a0 + j] = use ? 1 : 0;   // (read back by this thread only)
      }
    }
#pragma unroll
    for (int i = 0; i < kRsSums + 1; ++i) {
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) acc[i] += __shfl_xor(acc[i], off, 64);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const double o = __shfl_xor(acc[kRsSums + 1], off, 64);
      acc[kRsSums + 1] = o < acc[kRsSums + 1] ? o : acc[kRsSums + 1];
    }
    if (lane == 0) {
#pragma unroll
      for (int i = 0; i < kRsSums + 2; ++i) red[buf][wave][i] = acc[i];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kRsSums + 1; ++i) {
      double s = red[buf][0][i];
#pragma unroll
      for (int w = 1; w < kRsWaves; ++w) s += red[buf][w][i];
      acc[i] = s;
    }
    double dmin = red[buf][0][kRsSums + 1];
#pragma unroll
    for (int w = 1; w < kRsWaves; ++w) dmin = red[buf][w][kRsSums + 1] < dmin ? red[buf][w][kRsSums + 1] : dmin;
    buf ^= 1;
#pragma unroll
    for (int i = 0; i < kRsSums; ++i) tot[i] = acc[i];
    rs_mask_sums(tot, opt.fixed_mask);
    *used = (unsigned)acc[kRsSums];
    *depth = dmin;
  };

  double held[7];
#pragma unroll
  for (int i = 0; i < 7; ++i) held[i] = state[(size_t)p * kPoseState + i];
  // one call site of sums_at, so that it is inlined and its arrays stay in registers: the first evaluation is the
  // starting pose, every later one a trial pose.  Block-uniform: every thread holds the same state.
  RsPose m;
  double at[7];
#pragma unroll
  for (int i = 0; i < 7; ++i) at[i] = held[i];
  bool first = true;
  do {
    double tot[kRsSums], depth;
    unsigned used;
    sums_at(at, first, tot, &used, &depth);
    if (first) rs_begin(&m, opt, held, tot, used, k - used, depth);
    else rs_step(&m, opt, at, tot, depth);
    first = false;
    if (m.active) rs_apply(m.x, m.delta, opt.fixed_mask, at);
  } while (m.active);
  if (tid == 0) {
    double r[kRsResult], h[36];
    rs_result(m, r);
    rs_info(m, h);
    const bool acc = rs_accepted(m);
#pragma unroll
    for (int i = 0; i < kRsResult; ++i) res[(size_t)row * kRsResult + i] = r[i];
    // (two stores, not one store of a choice: a choice between the two arrays would keep both out of registers)
    if (acc) {
#pragma unroll
      for (int i = 0; i < 7; ++i) t7[(size_t)row * 7 + i] = m.x[i];
    } else {
#pragma unroll
      for (int i = 0; i < 7; ++i) t7[(size_t)row * 7 + i] = held[i];
    }
#pragma unroll
    for (int i = 0; i < 36; ++i) info[(size_t)row * 36 + i] = h[i];
  }
}

// a requested pose without observations: no block runs for it
__global__ void k_resect_none(uint32_t n, const uint32_t* __restrict__ ids, const uint32_t* __restrict__ rows,
                              const double* __restrict__ state, double* __restrict__ res, double* __restrict__ t7,
                              double* __restrict__ info) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t p = ids[i], row = rows[i];
  res[(size_t)row * kRsResult] = kRsTooFewObservations;
  for (int j = 1; j < kRsResult; ++j) res[(size_t)row * kRsResult + j] = 0.0;
  for (int j = 0; j < 7; ++j) t7[(size_t)row * 7 + j] = state[(size_t)p * kPoseState + j];
  for (int j = 0; j < 36; ++j) info[(size_t)row * 36 + j] = 0.0;
}

// write-back: parameters 0 .. 6 of the requested rows; rows that were not accepted hold the bits they had
__global__ void k_resect_store(uint32_t n, const uint32_t* __restrict__ ids, const uint32_t* __restrict__ rows,
                               const double* __restrict__ t7, double* __restrict__ state) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t p = ids[i], row = rows[i];
  for (int j = 0; j < 7; ++j) state[(size_t)p * kPoseState + j] = t7[(size_t)row * 7 + j];
}

// ids / rows on the device hold the requests grouped: [0, cls[0]) without observations, then the poses of up to 256,
// of up to 1 024 and of more observations, cls[1..3] of each
int launch_resect(Engine* e, const RsOptions& o, const uint32_t cls[4]) {
  Engine::Resect& w = e->resect;
  const double* x_held = e->lm_dim == 1 ? e->lm_xw.p : e->lm_x[e->cur].p;
  const double* state = e->pose_state[e->cur].p;
  if (cls[0]) {
    hipLaunchKernelGGL(k_resect_none, dim3((cls[0] + 255) / 256), dim3(256), 0, e->stream, cls[0], w.ids.p, w.rows.p, state,
                       w.res.p, w.t7.p, w.info.p);
    BAE_HIP(hipGetLastError());
  }
  uint32_t first = cls[0];
#define BAE_ARGS                                                                                                   \
  o, w.ids.p + first, w.rows.p + first, w.ptr.p, w.idx.p, e->obs_z.p, e->obs_w0.p, e->obs_cam.p, e->obs_lm.p, x_held, \
      e->cam.p, e->pose_cam_ptr(), state, w.used.p, w.res.p, w.t7.p, w.info.p
#define BAE_RS_LAUNCH(SLOTSv, count)                                                                               \
  do {                                                                                                             \
    if (count) {                                                                                                   \
      if (e->has_fov) hipLaunchKernelGGL((k_resect<SLOTSv, true>), dim3(count), dim3(kRsThreads), 0, e->stream, BAE_ARGS); \
      else hipLaunchKernelGGL((k_resect<SLOTSv, false>), dim3(count), dim3(kRsThreads), 0, e->stream, BAE_ARGS);   \
      BAE_HIP(hipGetLastError());                                                                                  \
      first += (count);                                                                                            \
    }                                                                                                              \
  } while (0)
  BAE_RS_LAUNCH(1, cls[1]);
  BAE_RS_LAUNCH(4, cls[2]);
  BAE_RS_LAUNCH(0, cls[3]);
#undef BAE_RS_LAUNCH
#undef BAE_ARGS
  return 0;
}

int launch_resect_store(Engine* e, uint32_t n) {
  Engine::Resect& w = e->resect;
  hipLaunchKernelGGL(k_resect_store, dim3((n + 255) / 256), dim3(256), 0, e->stream, n, w.ids.p, w.rows.p, w.t7.p,
                     e->pose_state[e->cur].p);
  BAE_HIP(hipGetLastError());
  return 0;
}

}  // namespace bae
