// What the per-landmark kernels over the selected inverse share (k_selinv.hip: landmark marginals, k_lever.hip:
// leverages of projection residuals): an element of Sigma out of the compact store, the kernel arguments, and the
// incidences of a landmark.  Device code: include after engine.h, selinv.h and tile_mma.h.
#pragma once
#include "engine.h"
#include "selinv.h"
#include "tile_mma.h"

namespace bae {

using tile64::TB;

// Sigma element (r, c), either half; NaN outside the pattern
__device__ __forceinline__ double sig_at(const double* __restrict__ store, const uint32_t* __restrict__ slot,
                                         uint32_t nt, uint32_t r, uint32_t c) {
  if (r / TB < c / TB) { const uint32_t t = r; r = c; c = t; }
  const uint32_t sl = slot[(size_t)(r / TB) * nt + c / TB];
  if (sl == kNoSlot) return __builtin_nan("");
  return store[(size_t)sl * TB * TB + (size_t)(r % TB) * TB + (c % TB)];
}

struct LmArgs {
  const uint32_t* lm_ptr;
  const uint32_t* obs_pose;
  const uint32_t* obs_lm;
  const uint32_t* lm_ref_pose;
  const int32_t* pose_opt;
  const int32_t* lm_opt;
  const double* frow;
  const double* crow_lm;   // [L][6] E_l = sum w J_l^T J_k (calibration columns), or null
  const double* lm_vinv;
  const uint32_t* slot;
  const double* store;
  uint32_t nt, lrow_base, np;
  int D, K;
};

// The incidences ("entries") of landmark l: its observations (W rows of the measuring pose when the
// observation is listed and the pose active, structure.h), then (LM == 1) the reference pose's W_r row,
// then the calibration row E_l.  Same selection as k_backsub.
template <int LM>
struct LmEntry {
  bool valid;
  uint32_t base;      // first row of the block in Sigma (engine order)
  int width;          // 6 (pose rows) or K
  const double* w;    // LM rows of `width` values: w[k * 6 + i]
};
template <int LM>
__device__ __forceinline__ LmEntry<LM> lm_entry(const LmArgs& g, uint32_t l, uint32_t e, uint32_t nobs, bool any_listed) {
  constexpr int R = LM == 1 ? 6 : 8, WO = LM == 1 ? 4 : 2;
  LmEntry<LM> x;
  const uint32_t rp = g.lm_ref_pose[l];
  if (e < nobs) {
    const uint32_t a = g.lm_ptr[l] + e, pm = g.obs_pose[a];
    const int po = g.pose_opt[pm];
    x.valid = !(LM == 1 && pm == rp) && po >= 0;
    x.base = po >= 0 ? (uint32_t)po * g.D : 0;
    x.width = 6;
    x.w = g.frow + ((size_t)a * R + WO) * kRow;
  } else if (LM == 1 && e == nobs) {
    const int po = g.pose_opt[rp];
    x.valid = any_listed && po >= 0;
    x.base = po >= 0 ? (uint32_t)po * g.D : 0;
    x.width = 6;
    x.w = g.frow + ((size_t)g.lrow_base + 2 * (size_t)l) * kRow;
  } else {
    x.valid = g.K > 0 && g.crow_lm;
    x.base = g.np;
    x.width = g.K;
    x.w = g.crow_lm ? g.crow_lm + (size_t)l * kRow : nullptr;
  }
  return x;
}

// the arguments of an engine whose selected inverse is valid (marginals_compute)
inline LmArgs lm_args(const Engine* e) {
  const Structure& st = e->st;
  LmArgs g;
  g.lm_ptr = e->lm_ptr.p; g.obs_pose = e->obs_pose.p; g.obs_lm = e->obs_lm.p; g.lm_ref_pose = e->lm_ref_pose.p;
  g.pose_opt = e->pose_opt.p; g.lm_opt = e->lm_opt.p; g.frow = e->frow.p;
  g.crow_lm = st.K ? e->crow.p + 2 * (size_t)st.O * kRow : nullptr;
  g.lm_vinv = e->lm_vinv.p; g.slot = e->sig_slot.p; g.store = e->sig.p;
  g.nt = st.ld / TB; g.lrow_base = st.lrow_base; g.np = st.np; g.D = e->pose_dim; g.K = (int)st.K;
  return g;
}

}  // namespace bae
