// gfx950 kernels of ba_hip_triangulate_landmarks: closed-form triangulation and per-landmark Levenberg-Marquardt
// refinement with the poses held fixed, to convergence inside one launch (triang.h holds the rules).
//
// The layout is k_linearize's (k_proj.hip): observations sorted by landmark, a wavefront owns one range of wave_rng.
//   small ranges (whole landmarks, at most 64 observations): one lane per observation.  The lane keeps its observation
//     in registers across all iterations — (R, t) of its sensor, the pixel, the weight, the intrinsics — evaluates the
//     residual and jl at the trial point of its landmark, and the sums [V | b_l | E] (10 with LmSize 3, 3 with LmSize 1)
//     go through k_linearize's segmented inclusive scan (__shfl_up within the landmark's lanes, total from its last
//     lane).  Every lane of a landmark then takes the same accept / reject decision and solves the same tiny system.
//     The loop is wave-uniform: it runs while a ballot says some landmark of the range is still iterating, finished
//     landmarks are predicated off.
//   BIG ranges (one landmark with more than 64 observations): one wave per landmark, the lanes stride over the
//     observations and reload them per iteration, the reduction is an xor butterfly.
// A wave whose range holds no selected landmark returns after reading obs_lm and the selection mask.  No atomics, no
// LDS, no order that depends on scheduling: two calls give identical bits.  FP64 throughout.
#include "engine.h"
#include "dmath.h"

using namespace bad;

namespace bae {

static constexpr int kTriWaves = 2;

struct TriSum { __device__ __forceinline__ double operator()(double a, double b) const { return a + b; } };
struct TriMax { __device__ __forceinline__ double operator()(double a, double b) const { return tri_max(a, b); } };
struct TriMin { __device__ __forceinline__ double operator()(double a, double b) const { return tri_min(a, b); } };

// v[i] of every lane -> the combination over the lanes of the lane's landmark, in every lane of it
template <int N, bool BIG, class Op>
__device__ __forceinline__ void tri_reduce(double* v, int lane, int s0, int s1, Op op) {
  if constexpr (BIG) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) v[i] = op(v[i], __shfl_xor(v[i], off, 64));
    }
  } else {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const bool take = lane - off >= s0;
#pragma unroll
      for (int i = 0; i < N; ++i) {
        const double up = __shfl_up(v[i], off, 64);
        if (take) v[i] = op(v[i], up);
      }
    }
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = __shfl(v[i], s1, 64);
  }
}

__device__ __forceinline__ Rt tri_load_rt(const double* __restrict__ p) {
  Rt t;
#pragma unroll
  for (int i = 0; i < 9; ++i) t.R.m[i] = p[i];
  t.t = v3(p[9], p[10], p[11]);
  return t;
}

template <int LM, bool BIG, bool FOV>
__global__ void __launch_bounds__(64 * kTriWaves)
k_triangulate(uint32_t n_chunks, int C, TriOptions opt, const uint2* __restrict__ wave_rng,
              const uint32_t* __restrict__ lm_ptr, const double* __restrict__ obs_z,
              const uint32_t* __restrict__ obs_pose, const uint32_t* __restrict__ obs_cam,
              const uint32_t* __restrict__ obs_lm, const double* __restrict__ obs_w0,
              const double* __restrict__ x_held, const uint32_t* __restrict__ lm_ref_pose,
              const uint32_t* __restrict__ lm_ref_cam, const double* __restrict__ cam,
              const double* __restrict__ pose_cam, const double* __restrict__ tsw, const double* __restrict__ tws,
              const uint8_t* __restrict__ mask, uint8_t* __restrict__ early, double* __restrict__ res,
              double* __restrict__ xw_out) {
  constexpr int N = TriSums<LM>::N, NL = TriSums<LM>::NL;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint32_t chunk = blockIdx.x * kTriWaves + wave;
  if (chunk >= n_chunks) return;   // waves are independent: no block-level barrier below
  const uint2 rng = wave_rng[chunk];
  const uint32_t a0 = rng.x, a1 = rng.y, nobs = a1 - a0;
  const bool valid = BIG || (uint32_t)lane < nobs;
  const uint32_t a_own = BIG ? a0 : (valid ? a0 + lane : a1 - 1);
  const uint32_t l = obs_lm[a_own];
  const bool sel = mask[l] != 0;
  if (__ballot(sel) == 0) {
    if (lane == 0) early[chunk] = 1;
    return;
  }
  if (lane == 0) early[chunk] = 0;
  const uint32_t first = lm_ptr[l], k = lm_ptr[l + 1] - first;
  const int s0 = (int)(first - a0), s1 = s0 + (int)k - 1;   // lanes of this landmark (small ranges)

  // the reference sensor (LmSize 1) and one observation as the lanes hold it
  Rt t_sw_r{}, t_ws_r{};
  if constexpr (LM == 1) {
    const size_t r = ((size_t)lm_ref_pose[l] * C + lm_ref_cam[l]) * kRt;
    t_sw_r = tri_load_rt(tsw + r);
    t_ws_r = tri_load_rt(tws + r);
  }
  auto load = [&](uint32_t a) {
    TriObs o;
    const uint32_t pm = obs_pose[a], cm = obs_cam[a];
    const double* cp = cam + (size_t)cm * kCamRec;
    const double* ip = pose_cam ? pose_cam + (size_t)pm * 4 : cp;   // per-pose intrinsics, as k_linearize
    o.cam = {ip[0], ip[1], ip[2], ip[3], 0.0, 0};
    if constexpr (FOV) { o.cam.w = cp[35]; o.cam.model = cp[36] != 0.0 ? 1 : 0; }
    const Rt t_sw_m = tri_load_rt(tsw + ((size_t)pm * C + cm) * kRt);
    if constexpr (LM == 1) o.T = compose(t_sw_m, t_ws_r);
    else o.T = t_sw_m;
    o.z[0] = obs_z[2 * (size_t)a]; o.z[1] = obs_z[2 * (size_t)a + 1];
    o.w0 = obs_w0[a];
    return o;
  };
  TriObs own;
  if constexpr (!BIG) own = load(a_own);
  // f(observation, counts) over the observations of this lane
  auto each = [&](auto&& f) {
    if constexpr (BIG) {
      for (uint32_t a = a0 + lane; a < a1; a += 64) f(load(a), true);
    } else {
      f(own, valid);
    }
  };

  double xh[4], xv[3], rho;
#pragma unroll
  for (int i = 0; i < 4; ++i) xh[i] = x_held[(size_t)l * 4 + i];
  tri_held<LM>(xh, t_sw_r, xv, &rho);

  // parallax and baseline against the first bearing
  V3 c0 = v3(0.0, 0.0, 0.0), d0 = v3(xv[0], xv[1], xv[2]);
  if constexpr (LM == 3) tri_centre_bearing(load(first), &c0, &d0);
  double pb[2] = {0.0, 0.0};
  each([&](const TriObs& o, bool ok) {
    V3 c, d;
    tri_centre_bearing(o, &c, &d);
    if (ok) { pb[0] = tri_max(pb[0], tri_angle(d0, d)); pb[1] = tri_max(pb[1], tri_dist2(c0, c)); }
  });
  tri_reduce<2, BIG>(pb, lane, s0, s1, TriMax());

  if (opt.linear_init) {
    double lin[NL];
#pragma unroll
    for (int i = 0; i < NL; ++i) lin[i] = 0.0;
    each([&](const TriObs& o, bool ok) {
      double v[NL];
      tri_linear_terms<LM>(o, xv, v);
#pragma unroll
      for (int i = 0; i < NL; ++i) lin[i] += ok ? v[i] : 0.0;
    });
    tri_reduce<NL, BIG>(lin, lane, s0, s1, TriSum());
    tri_linear_solve<LM>(lin, xv, &rho);
  }

  // [V | b_l | E] and the smallest depth at (txv, trho)
  auto sums_at = [&](const double* txv, double trho, bool guard, double* tot, double* depth) {
#pragma unroll
    for (int i = 0; i < N; ++i) tot[i] = 0.0;
    double dmin = tri_inf();
    each([&](const TriObs& o, bool ok) {
      double v[N];
      const double dep = tri_eval<LM>(o, txv, trho, opt.huber_width, guard, v);
#pragma unroll
      for (int i = 0; i < N; ++i) tot[i] += ok ? v[i] : 0.0;
      if (ok) dmin = tri_min(dmin, dep);
    });
    tri_reduce<N, BIG>(tot, lane, s0, s1, TriSum());
    if (depth) {
      tri_reduce<1, BIG>(&dmin, lane, s0, s1, TriMin());
      *depth = dmin;
    }
  };

  TriLm<LM> m;
  {
    double tot[N], depth;
    sums_at(xv, rho, false, tot, &depth);
    const double* x0 = LM == 3 ? xv : &rho;
    tri_begin<LM>(&m, opt, x0, tot, depth, pb[0], pb[1], dot(c0, c0), k);
    if (!sel) m.active = false;
  }
  while (__ballot(m.active) != 0) {
    double txv[3], trho, tot[N];
    tri_trial<LM>(m, xv, rho, txv, &trho);
    sums_at(txv, trho, true, tot, nullptr);
    if (m.active) tri_step<LM>(&m, opt, tot);
  }

  // the end point: smallest depth there, result row, coordinates
  const bool accepted = sel && tri_accepted<LM>(m, opt);
  double depth_end = m.depth;
  {
    double fxv[3], frho = LM == 3 ? rho : m.x[0];
#pragma unroll
    for (int i = 0; i < 3; ++i) fxv[i] = LM == 3 ? m.x[i] : xv[i];
    double dmin = tri_inf();
    each([&](const TriObs& o, bool ok) {
      const double dep = tri_depth<LM>(o, fxv, frho);
      if (ok) dmin = tri_min(dmin, dep);
    });
    tri_reduce<1, BIG>(&dmin, lane, s0, s1, TriMin());
    if (m.status == kTriOk || m.status == kTriNotConverged) depth_end = dmin;
    if (sel && lane == (BIG ? 0 : s1)) {
      double r[kTriResult];
      tri_result<LM>(m, k, depth_end, r);
#pragma unroll
      for (int i = 0; i < kTriResult; ++i) res[(size_t)l * kTriResult + i] = r[i];
      if (accepted) {
        double xo[4];
        tri_world<LM>(fxv, frho, t_ws_r, xo);
#pragma unroll
        for (int i = 0; i < 4; ++i) xw_out[(size_t)l * 4 + i] = xo[i];
      }
    }
  }
}

// every landmark's row before the waves run: the coordinates held, and for a selected landmark the result of one
// without observations (no wave of wave_rng reaches it)
__global__ void k_tri_prefill(uint32_t L, const double* __restrict__ x_held, const uint8_t* __restrict__ mask,
                              double* __restrict__ res, double* __restrict__ xw_out) {
  const uint32_t l = blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= L) return;
#pragma unroll
  for (int i = 0; i < 4; ++i) xw_out[(size_t)l * 4 + i] = x_held[(size_t)l * 4 + i];
  double r[kTriResult];
  tri_result_none(r);
  if (!mask[l]) r[0] = -1.0;   // not requested
#pragma unroll
  for (int i = 0; i < kTriResult; ++i) res[(size_t)l * kTriResult + i] = r[i];
}

int launch_triangulate(Engine* e, const TriOptions& o) {
  const Structure& st = e->st;
  const uint32_t L = st.L;
  if (L == 0) return 0;
  // the coordinates held: x_w (LmSize 1: lm_xw, what ba_hip_end_solve left; LmSize 3: the current landmark buffer)
  const double* x_held = e->lm_dim == 1 ? e->lm_xw.p : e->lm_x[e->cur].p;
  hipLaunchKernelGGL(k_tri_prefill, dim3((L + 255) / 256), dim3(256), 0, e->stream, L, x_held,
                     (const uint8_t*)e->tri.mask.p, e->tri.res.p, e->tri.xw.p);
  BAE_HIP(hipGetLastError());
  if (st.n_chunks == 0 || st.O == 0) return 0;
  const uint32_t n_small = st.n_chunks - st.n_big_chunks;
#define BAE_ARGS(first, count)                                                                                   \
  count, (int)st.C, o, e->wave_rng.p + (first), e->lm_ptr.p, e->obs_z.p, e->obs_pose.p, e->obs_cam.p, e->obs_lm.p, \
      e->obs_w0.p, x_held, e->lm_ref_pose.p, e->lm_ref_cam.p, e->cam.p, e->pose_cam_ptr(), e->tsw.p, e->tws.p,   \
      (const uint8_t*)e->tri.mask.p, e->tri.early.p + (first), e->tri.res.p, e->tri.xw.p
#define BAE_TRI_LAUNCH(BIGv, first, count)                                                                       \
  do {                                                                                                           \
    const dim3 grid(((count) + kTriWaves - 1) / kTriWaves), block(64 * kTriWaves);                               \
    if (e->has_fov) {                                                                                            \
      if (e->lm_dim == 1) hipLaunchKernelGGL((k_triangulate<1, BIGv, true>), grid, block, 0, e->stream, BAE_ARGS(first, count)); \
      else hipLaunchKernelGGL((k_triangulate<3, BIGv, true>), grid, block, 0, e->stream, BAE_ARGS(first, count)); \
    } else {                                                                                                     \
      if (e->lm_dim == 1) hipLaunchKernelGGL((k_triangulate<1, BIGv, false>), grid, block, 0, e->stream, BAE_ARGS(first, count)); \
      else hipLaunchKernelGGL((k_triangulate<3, BIGv, false>), grid, block, 0, e->stream, BAE_ARGS(first, count)); \
    }                                                                                                            \
  } while (0)
  if (n_small) BAE_TRI_LAUNCH(false, 0, n_small);
  if (st.n_big_chunks) BAE_TRI_LAUNCH(true, n_small, st.n_big_chunks);
#undef BAE_TRI_LAUNCH
#undef BAE_ARGS
  BAE_HIP(hipGetLastError());
  return 0;
}

}  // namespace bae
