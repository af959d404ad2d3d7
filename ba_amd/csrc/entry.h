// How a C-ABI entry point of engine.hip / engine_readers.hip begins, and how it asks requests.h.
//   BA_ENTRY_HOST    fills e->prob, copies host vectors or returns a counter: the caller's current device is left alone
//   BA_ENTRY_DEVICE  can reach a HIP call (upload, DBuf::alloc, a stream or event call, a launcher): selects e->device
//   BA_ENTRY_FINAL   ... and needs the structure of ba_hip_finalize
// Each defines `e`.  Nothing else in the two files selects a device, apart from ba_hip_create and ba_hip_destroy.
#pragma once
#include "engine.h"
#include "requests.h"

#define BA_ENTRY_HOST(h) bae::Engine* e = reinterpret_cast<bae::Engine*>(h)
#define BA_ENTRY_DEVICE(h) \
  BA_ENTRY_HOST(h);        \
  BAE_HIP(hipSetDevice(e->device))
#define BA_ENTRY_FINAL(h)                                              \
  BA_ENTRY_HOST(h);                                                    \
  if (!e->held.finalized) return e->fail_msg(bae::kNotFinalized);      \
  BAE_HIP(hipSetDevice(e->device))
// a check of requests.h: its message, if any, is the call's refusal
#define BA_ASK(check)                                                  \
  do {                                                                 \
    const std::string _m = (check);                                    \
    if (!_m.empty()) return e->fail_msg(_m.c_str());                   \
  } while (0)

namespace bae {

inline GuardFacts guard_facts(const Engine* e) {
  return {dist_solve_enabled(e), e->sharded(), e->pcg_refused(), e->opt.keep_reduced_system && e->A_keep.p,
          e->pcg_plan.nt == e->st.ld / 64 && e->pcg_blk.size() == (size_t)2 * e->st.ld, e->damp.lambda_lin > 0.0};
}
// why ba_hip_set_damping(lambda > 0) is refused on this engine, or nothing
inline std::string damping_refusal(const Engine* e) {
  if (e->calib_dim) return "ba_hip_set_damping: not offered with calibration unknowns";
  if (e->allreduce || e->coll || e->comm) return "ba_hip_set_damping: not offered on sharded engines or with the distributed solve";
  return "";
}
inline StructureView structure_view(const Engine* e) {
  const Structure& st = e->st;
  return {st.P, st.L, st.np, st.K, st.n, st.ld, (uint32_t)e->pose_dim, (uint32_t)e->lm_dim, &st.pose_opt, &st.lm_opt,
          &e->opt_of_natural};
}
inline void unpermute_vec(const Engine* e, double* v) {   // engine rows -> the caller's, in place
  if (e->opt_of_natural.empty() || !v) return;
  const StructureView sv = structure_view(e);
  std::vector<double> tmp(v, v + e->st.np);
  for (uint32_t r = 0; r < e->st.np; ++r) v[r] = tmp[int_row(sv, r)];
}

}  // namespace bae
