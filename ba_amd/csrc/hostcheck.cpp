// Host build of the device math (dmath.h) so that `-m "not gpu"` tests can compare the
// kernels' closed-form Jacobians with the oracle without a GPU.  Test hook only: the
// product never calls this library.
#include <vector>
#include "dmath.h"
using namespace bad;

static Rt rt_from7(const double* p) {
  Rt t;
  t.R = quat_to_rot(p[3], p[4], p[5], p[6]);
  t.t = v3(p[0], p[1], p[2]);
  return t;
}

// camera model of the calls below: w != 0 makes cam4 the first four parameters of a FOV camera
static double g_hostcheck_fov_w = 0.0;
extern "C" void ba_hostcheck_set_fov(double w) { g_hostcheck_fov_w = w; }
static Cam cam_from4(const double* cam4) {
  Cam c = {cam4[0], cam4[1], cam4[2], cam4[3], g_hostcheck_fov_w, g_hostcheck_fov_w != 0.0 ? 1 : 0};
  return c;
}

static int g_hostcheck_variant = 1;  // 1 = proj_linearize (what k_linearize calls), 0 = proj_jacobians
extern "C" void ba_hostcheck_set_variant(int v) { g_hostcheck_variant = v; }

extern "C" void ba_hostcheck_proj_jacobians(int lm_dim, const double* cam4, const double* z,
                                            const double* x, const double* t_wp_m7,
                                            const double* t_vs_m7, const double* t_wp_r7,
                                            const double* t_vs_r7, int same_pose, double* r2,
                                            double* jm12, double* jr12, double* jl) {
  Cam cam = cam_from4(cam4);
  const Rt t_wp_m = rt_from7(t_wp_m7), t_vs_m = rt_from7(t_vs_m7);
  const Rt t_wp_r = rt_from7(t_wp_r7), t_vs_r = rt_from7(t_vs_r7);
  const Rt t_sw_m = inverse(compose(t_wp_m, t_vs_m));
  const Rt t_ws_r = compose(t_wp_r, t_vs_r);
  const Rt t_sv_m = inverse(t_vs_m);
  // the kernels' form (proj_linearize: fewer transforms) must agree with the literal closed form
  // (proj_jacobians) — both are compared with the oracle by tests/test_hostcheck.py (variant flag)
  if (lm_dim == 1) {
    ProjJac<1> o;
    if (g_hostcheck_variant == 0) proj_jacobians<1>(cam, z, x, t_sw_m, t_ws_r, t_wp_m, t_sv_m, t_wp_r, t_vs_r, same_pose != 0, &o);
    else proj_linearize<1>(cam, z, x, t_sw_m, t_vs_m.R, t_sv_m.t, t_ws_r, t_wp_r, same_pose != 0, &o);
    for (int i = 0; i < 2; ++i) r2[i] = o.r[i];
    for (int i = 0; i < 12; ++i) { jm12[i] = o.jm[i]; jr12[i] = o.jr[i]; }
    for (int i = 0; i < 2; ++i) jl[i] = o.jl[i];
  } else {
    ProjJac<3> o;
    if (g_hostcheck_variant == 0) proj_jacobians<3>(cam, z, x, t_sw_m, t_ws_r, t_wp_m, t_sv_m, t_wp_r, t_vs_r, same_pose != 0, &o);
    else proj_linearize<3>(cam, z, x, t_sw_m, t_vs_m.R, t_sv_m.t, t_ws_r, t_wp_r, same_pose != 0, &o);
    for (int i = 0; i < 2; ++i) r2[i] = o.r[i];
    for (int i = 0; i < 12; ++i) { jm12[i] = o.jm[i]; jr12[i] = o.jr[i]; }
    for (int i = 0; i < 6; ++i) jl[i] = o.jl[i];
  }
}

// dz_dtvs rows of the DoTvs instantiations as k_linearize<.., CAL> evaluates them (LmSize 1)
extern "C" void ba_hostcheck_proj_tvs_jacobian(const double* cam4, const double* z, const double* x,
                                               const double* t_wp_m7, const double* t_vs_m7, const double* t_wp_r7,
                                               const double* t_vs_r7, int same_pose, double* jk12) {
  Cam cam = cam_from4(cam4);
  const Rt t_wp_m = rt_from7(t_wp_m7), t_vs_m = rt_from7(t_vs_m7);
  const Rt t_wp_r = rt_from7(t_wp_r7), t_vs_r = rt_from7(t_vs_r7);
  const Rt t_sw_m = inverse(compose(t_wp_m, t_vs_m));
  const Rt t_ws_r = compose(t_wp_r, t_vs_r);
  const Rt t_sv_m = inverse(t_vs_m);
  ProjJac<1> o;
  proj_linearize<1, true>(cam, z, x, t_sw_m, t_vs_m.R, t_sv_m.t, t_ws_r, t_wp_r, same_pose != 0, &o, jk12);
}

// dz_dcam_params rows of the CalibSize instantiations (proj_intrinsics_rows, what k_linearize<.., 2> calls)
extern "C" void ba_hostcheck_proj_intrinsics_jacobian(const double* cam4, const double* z_ref, double rho,
                                                      const double* t_wp_m7, const double* t_vs_m7,
                                                      const double* t_wp_r7, const double* t_vs_r7, double* jk12) {
  Cam cam = cam_from4(cam4);
  const Rt t_sw_m = inverse(compose(rt_from7(t_wp_m7), rt_from7(t_vs_m7)));
  const Rt t_ws_r = compose(rt_from7(t_wp_r7), rt_from7(t_vs_r7));
  proj_intrinsics_rows(cam, z_ref, rho, t_sw_m, t_ws_r, 1.0, jk12);
}

// the reference's chains with cached and rig extrinsics apart (proj_chain_two_tvs)
extern "C" void ba_hostcheck_proj_chain_two_tvs(const double* cam4, const double* x, const double* t_wp_m7,
                                                const double* t_wp_r7, const double* t_vs_rig7,
                                                const double* t_vs_cache7, int same_pose, double* jm12,
                                                double* jr12, double* jk12) {
  Cam cam = cam_from4(cam4);
  proj_chain_two_tvs(cam, x, t_wp_m7, t_wp_r7, t_vs_rig7, t_vs_cache7, same_pose != 0, jm12, jr12, jk12);
}

// ---- pose-pose residuals (dpose.h) ---------------------------------------------------
#include "dpose.h"

extern "C" void ba_hostcheck_unary(const double* t_wp7, const double* t_prior7, int use_rotation,
                                   double* r6, double* J36) {
  DM<6, 6> J;
  unary_residual(tq_from7(t_wp7), tq_from7(t_prior7), use_rotation, r6, &J);
  for (int i = 0; i < 36; ++i) J36[i] = J.m[i];
}

extern "C" void ba_hostcheck_binary(const double* t_w1, const double* t_w2, const double* t_12,
                                    const double* cov_inv36, const double* cov_inv_sqrt36,
                                    double weight, int use_rotation, double* h11, double* h12,
                                    double* h22, double* g1, double* g2, double* err_build,
                                    double* err_eval) {
  PPBlocks o;
  binary_blocks(tq_from7(t_w1), tq_from7(t_w2), tq_from7(t_12), cov_inv36, cov_inv_sqrt36, weight,
                use_rotation, &o, err_eval);
  for (int i = 0; i < 225; ++i) { h11[i] = o.h11.m[i]; h12[i] = o.h12.m[i]; h22[i] = o.h22.m[i]; }
  for (int i = 0; i < 15; ++i) { g1[i] = o.g1[i]; g2[i] = o.g2[i]; }
  *err_build = o.err_build;
}

extern "C" void ba_hostcheck_imu(const double* p1_16, const double* p2_16, const double* meas,
                                 int nmeas, const double* g3, const double* r6, const double* rb6,
                                 int RS, double* r15, double* dz1, double* dz2, double* cov_inv) {
  ImuOut o;
  imu_residual(p1_16, p2_16, meas, nmeas, g3, r6, rb6, RS, true, &o);
  for (int i = 0; i < 15; ++i) r15[i] = o.r[i];
  for (int i = 0; i < 225; ++i) { dz1[i] = o.dz1.m[i]; dz2[i] = o.dz2.m[i]; cov_inv[i] = o.cov_inv.m[i]; }
}

// the two-launch form of the device (k_imu_steps + k_imu): step Jacobians per sample first, then the
// sequential part — must reproduce the fused form bit for bit
extern "C" void ba_hostcheck_imu_split(const double* p1_16, const double* p2_16, const double* meas,
                                       int nmeas, const double* g3, const double* r6, const double* rb6,
                                       int RS, double* r15, double* dz1, double* dz2, double* cov_inv) {
  std::vector<double> steps((size_t)160 * (nmeas > 0 ? nmeas : 1), 0.0);
  for (int k = 1; k < nmeas; ++k) imu_step_jacobians(p1_16, meas, k, g3, &steps[(size_t)160 * k]);
  ImuOut o;
  imu_residual(p1_16, p2_16, meas, nmeas, g3, r6, rb6, RS, true, &o, nullptr, nullptr, steps.data());
  for (int i = 0; i < 15; ++i) r15[i] = o.r[i];
  for (int i = 0; i < 225; ++i) { dz1[i] = o.dz1.m[i]; dz2[i] = o.dz2.m[i]; cov_inv[i] = o.cov_inv.m[i]; }
}

// ---- static structure (structure.h) --------------------------------------------------------------
// Builds the lists of ba_hip_finalize for a graph and evaluates them on the CPU exactly as the
// device kernels do — k_linearize's row layout and landmark blocks, k_assemble_tiles' tile
// references, k_pose_blocks' per-pose terms — from per-residual Jacobians supplied by the caller.
// tests/test_structure_lists.py compares the result with a dense brute-force Schur complement, so
// the index logic is validated without a GPU.
#include "structure.h"
#include <cstring>

extern "C" int ba_hostcheck_schur_lists(
    int LM, int D, uint32_t P, const uint8_t* pose_active, uint32_t L, const uint8_t* lm_active,
    const uint32_t* lm_ref_pose, uint32_t O, const uint32_t* proj_pose, const uint32_t* proj_lm,
    const double* jm12, const double* jr12, const double* jl, const double* r2, const double* w,
    double* S_lower /* ld x ld, lower storage as on the device */, double* rhs_p, double* rhs_sc,
    double* vinv /* [L][LM*LM] */, double* bl /* [L][LM] */, uint32_t* out_ld, uint32_t* out_counts /* [8] */) {
  using namespace bae;
  Problem pb;
  pb.num_cams = 1; pb.num_poses = P; pb.num_lms = L; pb.num_proj = O;
  pb.pose_active.assign(pose_active, pose_active + P);
  pb.lm_active.assign(lm_active, lm_active + L);
  pb.lm_ref_pose.assign(lm_ref_pose, lm_ref_pose + L);
  pb.lm_ref_cam.assign(L, 0);
  pb.proj_pose.assign(proj_pose, proj_pose + O);
  pb.proj_lm.assign(proj_lm, proj_lm + O);
  pb.proj_cam.assign(O, 0);
  pb.proj_z.assign(2 * (size_t)O, 0.0);
  pb.proj_w.assign(O, 1.0);
  Lists st;
  std::string err;
  if (!build_lists(pb, LM, D, st, err)) return -1;
  const uint32_t R = st.R, WO = (uint32_t)w_row_offset(LM), ld = st.ld;
  *out_ld = ld;
  out_counts[0] = st.n_chunks; out_counts[1] = st.n_pairs; out_counts[2] = (uint32_t)st.n_pair_entries;
  out_counts[3] = (uint32_t)st.n_tile_refs; out_counts[4] = (uint32_t)st.n_pose_entries; out_counts[5] = st.n_inc;
  out_counts[6] = st.n_rows; out_counts[7] = st.Pact;
  // linearisation waves: whole landmarks, every observation covered exactly once, big ones last
  {
    std::vector<uint8_t> seen(st.O, 0);
    for (uint32_t c = 0; c < st.n_chunks; ++c) {
      const uint32_t a0 = st.wave_rng[c].x, a1 = st.wave_rng[c].y;
      if (a1 <= a0 || a1 > st.O) return -2;
      const uint32_t l0 = st.obs_lm[a0], l1 = st.obs_lm[a1 - 1];
      if (st.lm_ptr[l0] != a0 || st.lm_ptr[l1 + 1] != a1) return -3;
      const bool big = c >= st.n_chunks - st.n_big_chunks;
      if (big != (a1 - a0 > 64) || (big && l0 != l1)) return -4;
      for (uint32_t a = a0; a < a1; ++a) { if (seen[a]) return -5; seen[a] = 1; }
    }
    for (uint32_t a = 0; a < st.O; ++a) if (!seen[a]) return -5;
  }
  // ---- k_linearize, emulated per landmark ------------------------------------------------------
  std::vector<double> frow((size_t)st.n_rows * 6, 0.0), scal(st.n_scalars, 0.0);
  const int LL = LM > 0 ? LM : 1;
  for (uint32_t l = 0; l < L; ++l) {
    double V[9] = {0}, b[3] = {0}, Wr[6] = {0};
    const bool act = st.lm_opt[l] >= 0;
    for (uint32_t s = st.lm_ptr[l]; s < st.lm_ptr[l + 1]; ++s) {
      const uint32_t a = st.obs_rid[s];
      const bool same = LM == 1 && st.obs_pose[s] == lm_ref_pose[l];  // parallel_algos.h:97-99,111-113
      double Jm[12], Jr[12];
      for (int i = 0; i < 12; ++i) { Jm[i] = same ? 0.0 : jm12[12 * (size_t)a + i]; Jr[i] = (same || LM != 1) ? 0.0 : jr12[12 * (size_t)a + i]; }
      const double* Jl = jl + 2 * LL * (size_t)a;
      const double ww = w[a], sw = std::sqrt(ww);
      scal[2 * (size_t)s] = r2[2 * (size_t)a] * sw;
      scal[2 * (size_t)s + 1] = r2[2 * (size_t)a + 1] * sw;
      double* rows = &frow[(size_t)s * R * 6];
      for (int i = 0; i < 12; ++i) rows[i] = Jm[i] * sw;
      if (LM == 1) for (int i = 0; i < 12; ++i) rows[12 + i] = Jr[i] * sw;
      if (!act) continue;
      for (int p = 0; p < LM; ++p) {
        for (int q = 0; q < LM; ++q) V[p * LM + q] += (Jl[p] * Jl[q] + Jl[LM + p] * Jl[LM + q]) * ww;
        b[p] += (Jl[p] * r2[2 * (size_t)a] + Jl[LM + p] * r2[2 * (size_t)a + 1]) * ww;
      }
      for (int k = 0; k < LM; ++k)
        for (int x = 0; x < 6; ++x) rows[(WO + k) * 6 + x] = (Jm[x] * Jl[k] + Jm[6 + x] * Jl[LM + k]) * ww;
      if (LM == 1) for (int x = 0; x < 6; ++x) Wr[x] += (Jr[x] * Jl[0] + Jr[6 + x] * Jl[1]) * ww;
    }
    if (!act) continue;
    double Vi[9];
    if (LM == 1) {
      if (std::fabs(V[0]) < 1e-6) V[0] += 1e-6;
      Vi[0] = 1.0 / V[0];
    } else {
      double nrm = 0;
      for (int i = 0; i < 9; ++i) nrm += V[i] * V[i];
      if (std::sqrt(nrm) < 1e-6) { V[0] += 1e-6; V[4] += 1e-6; V[8] += 1e-6; }
      const double a = V[0], bb = V[1], c = V[2], d = V[3], e = V[4], f = V[5], g = V[6], h = V[7], i = V[8];
      const double A00 = e * i - f * h, A01 = c * h - bb * i, A02 = bb * f - c * e;
      const double A10 = f * g - d * i, A11 = a * i - c * g, A12 = c * d - a * f;
      const double A20 = d * h - e * g, A21 = bb * g - a * h, A22 = a * e - bb * d;
      const double id = 1.0 / (a * A00 + bb * A10 + c * A20);
      const double t[9] = {A00 * id, A01 * id, A02 * id, A10 * id, A11 * id, A12 * id, A20 * id, A21 * id, A22 * id};
      std::memcpy(Vi, t, sizeof(t));
    }
    for (int i = 0; i < LM * LM; ++i) vinv[(size_t)l * LM * LM + i] = Vi[i];
    for (int i = 0; i < LM; ++i) { bl[(size_t)l * LM + i] = b[i]; scal[2 * (size_t)st.O + (size_t)l * LM + i] = b[i]; }
    auto nwv = [&](const double* Wrows, double* out) {  // out[c] = -(W Vi)[:, c]
      for (int c = 0; c < LM; ++c)
        for (int x = 0; x < 6; ++x) {
          double sacc = 0;
          for (int k = 0; k < LM; ++k) sacc += Wrows[k * 6 + x] * Vi[k * LM + c];
          out[c * 6 + x] = -sacc;
        }
    };
    for (uint32_t s = st.lm_ptr[l]; s < st.lm_ptr[l + 1]; ++s) {
      double* rows = &frow[(size_t)s * R * 6];
      nwv(rows + WO * 6, rows + (WO + LM) * 6);
    }
    if (LM == 1) {
      double* lr = &frow[((size_t)st.lrow_base + 2 * l) * 6];
      for (int x = 0; x < 6; ++x) lr[x] = Wr[x];
      nwv(lr, lr + 6);
    }
  }
  // ---- k_assemble_tiles ------------------------------------------------------------------------------
  std::memset(S_lower, 0, sizeof(double) * (size_t)ld * ld);
  const uint32_t nt = ld / 64;
  uint64_t t = 0;
  for (uint32_t tr = 0; tr < nt; ++tr)
    for (uint32_t tc = 0; tc <= tr; ++tc, ++t)
      for (uint32_t q = st.tile_ptr[t]; q < st.tile_ptr[t + 1]; ++q) {
        const U2 ref = st.tile_ref[q];
        const uint32_t cnt = ref.y >> 14;
        const int ro = (int)((ref.y >> 7) & 127) - kRefBias, co = (int)(ref.y & 127) - kRefBias;
        double acc[36] = {0};
        for (uint32_t e = ref.x; e < ref.x + cnt; ++e) {
          const double* a = &frow[(size_t)st.pair_ent[e].x * 6];
          const double* bb = &frow[(size_t)st.pair_ent[e].y * 6];
          for (int x = 0; x < 6; ++x)
            for (int y = 0; y < 6; ++y) acc[x * 6 + y] += a[x] * bb[y];
        }
        for (int x = 0; x < 6; ++x)
          for (int y = 0; y < 6; ++y) {
            const int rr = ro + y, cc = co + x;  // block (i,j), i < j, is stored transposed
            if (rr < 0 || rr >= 64 || cc < 0 || cc >= 64) continue;
            double& dst = S_lower[((size_t)tr * 64 + rr) * ld + (size_t)tc * 64 + cc];
            if (dst != 0.0) return -6;  // two blocks must never overlap
            dst = acc[x * 6 + y];
          }
      }
  // ---- k_pose_blocks -----------------------------------------------------------------------------------
  for (uint32_t p = 0; p < st.Pact; ++p) {
    double blk[36] = {0}, ga[6] = {0}, gb[6] = {0};
    for (uint32_t e = st.pose_ptr[p]; e < st.pose_ptr[p + 1]; ++e) {
      const U3 en = st.pose_ent[e];
      const double* a = &frow[(size_t)en.a * 6];
      const double* bb = &frow[(size_t)en.b * 6];
      const double sc = scal[en.s];
      for (int x = 0; x < 6; ++x) {
        for (int y = 0; y < 6; ++y) blk[x * 6 + y] += a[x] * bb[y];
        (e < st.pose_mid[p] ? ga : gb)[x] += a[x] * sc;
      }
    }
    for (int x = 0; x < 6; ++x) {
      for (int y = 0; y < 6; ++y) S_lower[((size_t)p * D + x) * ld + (size_t)p * D + y] = blk[x * 6 + y];
      rhs_p[(size_t)p * D + x] = ga[x];
      rhs_sc[(size_t)p * D + x] = ga[x] + gb[x];
    }
  }
  return 0;
}

// ---- pose ordering (ordering.h) -------------------------------------------------------------------------
#include "ordering.h"

// symbolic tile elimination in place (nt x nt symmetric pattern in, lower factor pattern out); returns the
// factor's tile products
extern "C" uint64_t ba_hostcheck_tile_factor(uint32_t nt, uint8_t* nz) {
  std::vector<uint8_t> v(nz, nz + (size_t)nt * nt);
  bae::tile_symbolic_factor(v, nt);
  std::copy(v.begin(), v.end(), nz);
  return bae::factor_tile_products(v, nt);
}

// choose_pose_ordering on a group graph (CSR over ceil(Pact / G) groups); products4: per candidate
extern "C" int ba_hostcheck_pose_ordering(uint32_t Pact, int D, uint32_t K, const uint32_t* ptr, const uint32_t* adj,
                                          uint32_t* opt_of_natural, int* candidate, uint32_t* group_size,
                                          uint64_t* products4) {
  const uint32_t G = bae::pose_group_size(D), ng = (Pact + G - 1) / G;
  std::vector<uint32_t> p(ptr, ptr + ng + 1), a(adj, adj + (ng ? ptr[ng] : 0)), perm;
  bae::OrderingResult r;
  bae::choose_pose_ordering(Pact, D, K, p, a, perm, &r);
  std::copy(perm.begin(), perm.end(), opt_of_natural);
  *candidate = r.candidate;
  *group_size = r.G;
  for (int c = 0; c < bae::kOrderCandidates; ++c) products4[c] = r.products[c];
  return 0;
}

// model tile products of a group order (order[position] = group)
extern "C" uint64_t ba_hostcheck_group_order_products(uint32_t Pact, int D, uint32_t K, const uint32_t* ptr,
                                                      const uint32_t* adj, const uint32_t* order) {
  const uint32_t G = bae::pose_group_size(D), ng = (Pact + G - 1) / G;
  std::vector<uint32_t> p(ptr, ptr + ng + 1), a(adj, adj + (ng ? ptr[ng] : 0)), o(order, order + ng);
  return bae::group_order_products(Pact, D, K, p, a, o);
}

// ---- selected inverse (selinv.h) ------------------------------------------------------------------------
#include <cmath>
#include "selinv.h"

// Pattern and factor of a dense symmetric S for the two harnesses below: the closed tile pattern, L (lower
// storage, ld = 64 nt), the pivot signs and linvT; -1 on a zero pivot.  tile_map (optional, nt x nt): tiles to
// count as non-zero besides those that hold a non-zero of S
static int host_tile_factor(uint32_t n, const double* S, std::vector<uint8_t>& nz, std::vector<double>& L,
                            std::vector<double>& d, std::vector<double>& linvT, const uint8_t* tile_map = nullptr) {
  const uint32_t nt = (n + 63) / 64, ld = 64 * nt;
  nz.assign((size_t)nt * nt, 0);
  for (uint32_t r = 0; r < n; ++r)
    for (uint32_t c = 0; c < n; ++c)
      if (S[(size_t)r * n + c] != 0.0) nz[(size_t)(r / 64) * nt + c / 64] = 1;
  for (uint32_t t = 0; t < nt; ++t) nz[(size_t)t * nt + t] = 1;
  if (tile_map)
    for (uint32_t i = 0; i < nt; ++i)
      for (uint32_t k = 0; k <= i; ++k)
        if (tile_map[(size_t)i * nt + k]) nz[(size_t)i * nt + k] = nz[(size_t)k * nt + i] = 1;
  bae::tile_symbolic_factor(nz, nt);
  L.assign((size_t)ld * ld, 0.0);
  d.assign(ld, 1.0);
  for (uint32_t r = 0; r < ld; ++r)
    for (uint32_t c = 0; c <= r; ++c) L[(size_t)r * ld + c] = (r < n && c < n) ? S[(size_t)r * n + c] : (r == c ? 1.0 : 0.0);
  for (uint32_t j = 0; j < ld; ++j) {
    double p = L[(size_t)j * ld + j];
    for (uint32_t k = 0; k < j; ++k) p -= L[(size_t)j * ld + k] * L[(size_t)j * ld + k] * d[k];
    if (p == 0.0 || !std::isfinite(p)) return -1;
    d[j] = p < 0.0 ? -1.0 : 1.0;
    const double ljj = std::sqrt(std::fabs(p));
    L[(size_t)j * ld + j] = ljj;
    for (uint32_t i = j + 1; i < ld; ++i) {
      double s = L[(size_t)i * ld + j];
      for (uint32_t k = 0; k < j; ++k) s -= L[(size_t)i * ld + k] * d[k] * L[(size_t)j * ld + k];
      L[(size_t)i * ld + j] = s / (d[j] * ljj);
    }
  }
  // linvT[J] = L_JJ^-T: forward substitution on the identity, stored transposed
  linvT.assign((size_t)nt * 4096, 0.0);
  for (uint32_t J = 0; J < nt; ++J) {
    const double* Ljj = &L[(size_t)J * 64 * ld + (size_t)J * 64];
    double* G = &linvT[(size_t)J * 4096];
    for (uint32_t c = 0; c < 64; ++c)      // column c of L_JJ^-1
      for (uint32_t r = c; r < 64; ++r) {
        double s = r == c ? 1.0 : 0.0;
        for (uint32_t k = c; k < r; ++k) s -= Ljj[(size_t)r * ld + k] * G[(size_t)c * 64 + k];
        G[(size_t)c * 64 + r] = s / Ljj[(size_t)r * ld + r];  // (L^-1)[r][c] at G[c][r]
      }
  }
  return 0;
}

// The selected inverse on a dense symmetric n x n matrix S (row-major; n need not be a multiple of 64:
// the last tile is padded with an identity, as the engine pads A).  The tile pattern is that of S
// (diagonal tiles always), closed by tile_symbolic_factor.  S is factorised like the engine does —
// un-pivoted L D L^T, L carrying sqrt|pivot|, D = diag(+-1) — and selinv_host runs on the factor.
// Out: sigma (n x n, both halves, NaN outside the factor's pattern), nzL (nt x nt lower pattern), the
// tile products of the plan and its number of levels.  Returns -1 on a zero pivot.
extern "C" int ba_hostcheck_selinv(uint32_t n, const double* S, double* sigma, uint8_t* nzL_out, uint64_t* products,
                                   uint32_t* levels) {
  const uint32_t nt = (n + 63) / 64, ld = 64 * nt;
  std::vector<uint8_t> nz;
  std::vector<double> L, d, linvT;
  if (host_tile_factor(n, S, nz, L, d, linvT)) return -1;
  bae::SelinvPlan plan;
  bae::build_selinv_plan(nz, nt, plan);
  std::vector<double> store((size_t)plan.n_slots * 4096, 0.0);
  bae::selinv_host(plan, L.data(), ld, linvT.data(), d.data(), store.data());
  for (uint32_t r = 0; r < n; ++r)
    for (uint32_t c = 0; c < n; ++c) sigma[(size_t)r * n + c] = bae::selinv_element(plan, store.data(), r, c);
  std::copy(nz.begin(), nz.end(), nzL_out);
  *products = plan.products;
  *levels = (uint32_t)plan.level_ptr.size() - 1;
  return 0;
}

// the tile products formula of the plan on a lower factor pattern
extern "C" uint64_t ba_hostcheck_selinv_products(uint32_t nt, const uint8_t* nzL) {
  std::vector<uint8_t> v(nzL, nzL + (size_t)nt * nt);
  return bae::selinv_tile_products(v, nt);
}

// ---- joint covariance of a row set (jointcov.h) ---------------------------------------------------------
#include "jointcov.h"

// Sigma[sel, sel] of a dense symmetric S (as ba_hostcheck_selinv: same pattern, same factorisation) by
// build_joint_plan + jointcov_host.  Out: cov (m x m), Y (64 nt x m: the panels scattered to their tile rows,
// zero outside the reach), reach (nt flags), level_of (nt, 0xffffffff outside the reach), nzL (nt x nt), the
// tile products and the number of levels.  Returns -1 on a zero pivot, -2 on a row out of range.
extern "C" int ba_hostcheck_joint_marginals(uint32_t n, const double* S, uint32_t m, const uint32_t* sel, double* cov,
                                            double* Y_out, uint8_t* reach_out, uint32_t* level_of, uint8_t* nzL_out,
                                            uint64_t* products, uint32_t* levels) {
  const uint32_t nt = (n + 63) / 64, ld = 64 * nt;
  for (uint32_t c = 0; c < m; ++c)
    if (sel[c] >= n) return -2;
  std::vector<uint8_t> nz;
  std::vector<double> L, d, linvT;
  if (host_tile_factor(n, S, nz, L, d, linvT)) return -1;
  std::vector<uint32_t> tiles(m);
  for (uint32_t c = 0; c < m; ++c) tiles[c] = sel[c] / 64;
  bae::JointPlan p;
  bae::build_joint_plan(nz, nt, tiles, m, p);
  std::vector<double> Y(p.y_count());
  bae::jointcov_host(p, L.data(), ld, linvT.data(), d.data(), sel, Y.data(), cov);
  std::fill(Y_out, Y_out + (size_t)ld * m, 0.0);
  for (uint32_t t = 0; t < nt; ++t) {
    reach_out[t] = p.pos[t] != bae::kJointNone;
    level_of[t] = reach_out[t] ? p.level_of[p.pos[t]] : bae::kJointNone;
    if (reach_out[t])
      for (uint32_t r = 0; r < 64; ++r)
        for (uint32_t c = 0; c < m; ++c)
          Y_out[((size_t)t * 64 + r) * m + c] = Y[((size_t)p.pos[t] * 64 + r) * p.m_pad + c];
  }
  std::copy(nz.begin(), nz.end(), nzL_out);
  *products = p.products;
  *levels = p.levels();
  return 0;
}

// B^T S^-1 B for a caller's dense right-hand side B (n x m row-major), same factorisation: the plan is seeded with
// the tile rows that hold a non-zero of B, the substitution starts from B's non-zeros.  Outputs as above.
extern "C" int ba_hostcheck_joint_rhs(uint32_t n, const double* S, uint32_t m, const double* B, double* cov, double* Y_out,
                                      uint8_t* reach_out, uint32_t* level_of, uint8_t* nzL_out, uint64_t* products,
                                      uint32_t* levels) {
  const uint32_t nt = (n + 63) / 64, ld = 64 * nt;
  std::vector<uint8_t> nz;
  std::vector<double> L, d, linvT;
  if (host_tile_factor(n, S, nz, L, d, linvT)) return -1;
  std::vector<bae::JointEntry> ent;
  std::vector<uint32_t> tiles;
  for (uint32_t c = 0; c < m; ++c)
    for (uint32_t r = 0; r < n; ++r)
      if (B[(size_t)r * m + c] != 0.0) {
        ent.push_back({r, c, B[(size_t)r * m + c]});
        tiles.push_back(r / 64);
      }
  bae::JointPlan p;
  bae::build_joint_plan(nz, nt, tiles, m, p);
  std::vector<double> Y(p.y_count());
  bae::jointcov_host_rhs(p, L.data(), ld, linvT.data(), d.data(), ent.data(), ent.size(), Y.data(), cov);
  std::fill(Y_out, Y_out + (size_t)ld * m, 0.0);
  for (uint32_t t = 0; t < nt; ++t) {
    reach_out[t] = p.pos[t] != bae::kJointNone;
    level_of[t] = reach_out[t] ? p.level_of[p.pos[t]] : bae::kJointNone;
    if (reach_out[t])
      for (uint32_t r = 0; r < 64; ++r)
        for (uint32_t c = 0; c < m; ++c)
          Y_out[((size_t)t * 64 + r) * m + c] = Y[((size_t)p.pos[t] * 64 + r) * p.m_pad + c];
  }
  std::copy(nz.begin(), nz.end(), nzL_out);
  *products = p.products;
  *levels = p.levels();
  return 0;
}

// ---- solves with the kept factor (factorsolve.h) ---------------------------------------------------------
#include "factorsolve.h"

// X = S^-1 B for a dense symmetric S (n x n) and B (n x m, row-major), factorised as for ba_hostcheck_selinv on
// the pattern of S's non-zeros and the optional lower tile map (nt x nt), by build_factor_solve_plan +
// factor_solve_host.  variant: FactorSolveVariant (0 is the computation).  Out: X (n x m), nzL (nt x nt), the
// backward level of every tile column (nt), levels2 = (forward, backward) launch pairs, products2 = the tile
// products of the two passes.  Returns -1 on a zero pivot, -2 on m == 0.
extern "C" int ba_hostcheck_factor_solve(uint32_t n, const double* S, const uint8_t* tile_map, uint32_t m, const double* B,
                                         int variant, double* X, uint8_t* nzL_out, uint32_t* backward_level_of,
                                         uint32_t* levels2, uint64_t* products2) {
  const uint32_t nt = (n + 63) / 64, ld = 64 * nt;
  if (!m) return -2;
  std::vector<uint8_t> nz;
  std::vector<double> L, d, linvT;
  if (host_tile_factor(n, S, nz, L, d, linvT, tile_map)) return -1;
  bae::FactorSolvePlan p;
  bae::build_factor_solve_plan(nz, nt, m, p);
  const uint32_t mp = p.fwd.m_pad;
  std::vector<double> P(p.fwd.y_count(), 0.0);
  for (uint32_t r = 0; r < n; ++r)
    for (uint32_t c = 0; c < m; ++c) P[(size_t)r * mp + c] = B[(size_t)r * m + c];
  bae::factor_solve_host(p, L.data(), ld, linvT.data(), d.data(), P.data(), variant);
  for (uint32_t r = 0; r < n; ++r)
    for (uint32_t c = 0; c < m; ++c) X[(size_t)r * m + c] = P[(size_t)r * mp + c];
  std::copy(nz.begin(), nz.end(), nzL_out);
  for (uint32_t J = 0; J < nt; ++J) backward_level_of[J] = p.backward_level_of(J);
  levels2[0] = p.fwd.levels();
  levels2[1] = p.bwd.levels();
  products2[0] = p.fwd.products;
  products2[1] = p.bwd.products;
  return 0;
}

// The k eigenpairs of smallest magnitude of a dense symmetric S by weakest_modes_host, factorised as for
// ba_hostcheck_factor_solve.  pad_nonzero: the wrong variant of factorsolve.h.  Out: eigenvalues (k, ascending
// magnitude), modes (k x n), out_u32 = (iterations, converged, block), the largest relative residual of the k
// pairs.  Returns -1 on a zero pivot, -2 on k out of range.
extern "C" int ba_hostcheck_weakest_modes(uint32_t n, const double* S, const uint8_t* tile_map, uint32_t k, double tolerance,
                                          uint32_t max_iterations, uint32_t seed, int pad_nonzero, double* eigenvalues,
                                          double* modes, uint32_t* out_u32, double* residual_max) {
  const uint32_t nt = (n + 63) / 64, ld = 64 * nt;
  if (k == 0 || k > std::min(bae::kModeMaxK, n)) return -2;
  std::vector<uint8_t> nz;
  std::vector<double> L, d, linvT;
  if (host_tile_factor(n, S, nz, L, d, linvT, tile_map)) return -1;
  bae::ModeOptions o;
  o.tolerance = tolerance;
  o.max_iterations = max_iterations;
  o.seed = seed;
  bae::ModeResult r;
  bae::weakest_modes_host(nz, nt, L.data(), ld, linvT.data(), d.data(), n, k, o, pad_nonzero != 0, eigenvalues, modes, r);
  out_u32[0] = r.iterations;
  out_u32[1] = r.converged;
  out_u32[2] = r.block;
  *residual_max = r.residual_max;
  return 0;
}

// ---- marginalisation plan and the dense prior's error state (marg.h) ----------------------------------
#include <cstring>
#include <string>
#include "marg.h"

extern "C" void ba_hostcheck_prior_delta(const double* x0_16, const double* x16, int D, double* d, double* J) {
  bae::prior_delta(x0_16, x16, D, d, J);
}

// The plan of one marginalisation on a graph given by ids (natural pose order).  counts7: |B|, absorbed
// projection, unary, binary, inertial, prior residuals, dropped projection residuals; blanket: |B| pose ids.
// Returns 0, or -1 with the refusal in err (err_cap bytes).
extern "C" int ba_hostcheck_marg_plan(int LM, int D, uint32_t P, const uint8_t* pose_active, uint32_t L,
                                      const uint8_t* lm_active, const uint32_t* lm_ref_pose, uint32_t O,
                                      const uint32_t* proj_pose, const uint32_t* proj_lm, uint32_t nu, const uint32_t* un_pose,
                                      uint32_t nb, const uint32_t* bin_p1, const uint32_t* bin_p2, uint32_t ni,
                                      const uint32_t* imu_p1, const uint32_t* imu_p2, uint32_t nq, const uint32_t* prior_ptr,
                                      const uint32_t* prior_pose, uint32_t nm, const uint32_t* m_ids, uint32_t nl,
                                      const uint32_t* l_ids, uint32_t* counts7, uint32_t* blanket, char* err, uint32_t err_cap) {
  bae::Problem pb;
  pb.num_poses = P; pb.num_lms = L; pb.num_proj = O; pb.num_unary = nu; pb.num_binary = nb; pb.num_imu = ni;
  pb.pose_active.assign(pose_active, pose_active + P);
  pb.lm_active.assign(lm_active, lm_active + L);
  pb.lm_ref_pose.assign(lm_ref_pose, lm_ref_pose + L);
  pb.proj_pose.assign(proj_pose, proj_pose + O);
  pb.proj_lm.assign(proj_lm, proj_lm + O);
  pb.un_pose.assign(un_pose, un_pose + nu);
  pb.bin_p1.assign(bin_p1, bin_p1 + nb); pb.bin_p2.assign(bin_p2, bin_p2 + nb);
  pb.imu_p1.assign(imu_p1, imu_p1 + ni); pb.imu_p2.assign(imu_p2, imu_p2 + ni);
  std::vector<int32_t> pose_opt;
  bae::natural_pose_opt(pb, pose_opt);
  // observations sorted by landmark, stable in residual id (structure.h)
  std::vector<uint32_t> lm_ptr((size_t)L + 1, 0), obs_perm(O);
  for (uint32_t a = 0; a < O; ++a) lm_ptr[proj_lm[a] + 1]++;
  for (uint32_t l = 0; l < L; ++l) lm_ptr[l + 1] += lm_ptr[l];
  {
    std::vector<uint32_t> cur(lm_ptr.begin(), lm_ptr.end() - 1);
    for (uint32_t a = 0; a < O; ++a) obs_perm[cur[proj_lm[a]]++] = a;
  }
  bae::DensePriors pr;
  pr.ptr.assign(prior_ptr, prior_ptr + nq + 1);
  pr.pose.assign(prior_pose, prior_pose + pr.ptr.back());
  const uint32_t R = (uint32_t)bae::rows_per_obs(LM);
  bae::MargPlan pl;
  std::string e;
  if (!bae::marg_plan(pb, LM, D, pose_opt, lm_ptr, obs_perm, R, O * R, pr, m_ids, nm, l_ids, nl, pl, e)) {
    if (err && err_cap) { strncpy(err, e.c_str(), err_cap - 1); err[err_cap - 1] = 0; }
    return -1;
  }
  const uint32_t c[7] = {pl.nB, pl.n_proj, pl.n_unary, pl.n_binary, pl.n_imu, pl.n_prior, pl.n_dropped};
  for (int i = 0; i < 7; ++i) counts7[i] = c[i];
  for (uint32_t i = 0; i < pl.nB; ++i) blanket[i] = pl.local_pose[pl.nM + i];
  return 0;
}

// ---- iterative reduced solve (pcg.h) ----------------------------------------------------------------------
#include "pcg.h"

// q = S v by the tile plan on the lower storage A (row-major, 64 nt x 64 nt; tiles outside nz and the strict upper
// triangle of diagonal tiles are not read).  Returns the number of tiles visited.
extern "C" uint32_t ba_hostcheck_pcg_spmv(uint32_t nt, const uint8_t* nz, const double* A, const double* v, double* q) {
  std::vector<uint8_t> z(nz, nz + (size_t)nt * nt);
  bae::PcgPlan pl;
  bae::build_pcg_plan(z, nt, pl);
  std::vector<double> rs, cs;
  bae::pcg_spmv_host(pl, A, (size_t)64 * nt, v, q, rs, cs);
  return pl.n_tiles;
}

// pcg_host on a symmetric n x n system given by its LOWER triangle (row-major n x n): padded like the engine pads A,
// tile pattern from the nonzeros, np rows in blocks of D then one block of K = n - np.  out_u32: iterations, converged,
// residual replacements, breakdown, passes, tiles; out_f64: rel. residual of the recurrence, true, |b|.
extern "C" int ba_hostcheck_pcg(uint32_t n, const double* a_lower, const double* b, uint32_t np, uint32_t D, double rel_tolerance,
                                uint32_t max_iterations, double* x, uint32_t* out_u32, double* out_f64) {
  if (np > n || D < 1 || D > bae::kPcgMaxBlock || n - np > bae::kPcgMaxBlock) return -1;
  const uint32_t nt = (n + 63) / 64, ld = 64 * nt;
  std::vector<double> A((size_t)ld * ld, 0.0), rhs(ld, 0.0), xx(ld, 0.0);
  std::vector<uint8_t> nz((size_t)nt * nt, 0);
  for (uint32_t r = 0; r < n; ++r)
    for (uint32_t c = 0; c <= r; ++c) {
      const double v = a_lower[(size_t)r * n + c];
      A[(size_t)r * ld + c] = v;
      if (v != 0.0) nz[(size_t)(r / 64) * nt + c / 64] = 1;
    }
  for (uint32_t r = n; r < ld; ++r) A[(size_t)r * ld + r] = 1.0;
  for (uint32_t r = 0; r < n; ++r) rhs[r] = b[r];
  bae::PcgPlan pl;
  bae::build_pcg_plan(nz, nt, pl);
  std::vector<uint32_t> blk, blocks;
  bae::pcg_row_blocks(np, D, n - np, ld, blk, blocks);
  bae::PcgResult res;
  const int rc = bae::pcg_host(pl, A.data(), ld, rhs.data(), n, nz, blk, blocks, rel_tolerance, max_iterations, xx.data(), &res);
  for (uint32_t r = 0; r < n; ++r) x[r] = xx[r];
  out_u32[0] = res.iterations; out_u32[1] = res.converged; out_u32[2] = res.replacements; out_u32[3] = res.breakdown;
  out_u32[4] = res.passes; out_u32[5] = pl.n_tiles;
  out_f64[0] = res.bb > 0.0 ? std::sqrt(res.rr_recur / res.bb) : 0.0;
  out_f64[1] = res.bb > 0.0 ? std::sqrt(res.rr_true / res.bb) : 0.0;
  out_f64[2] = std::sqrt(res.bb);
  return rc;
}

// ba_hostcheck_pcg with the two-level preconditioner (coarse_aggregate = 0: the very call of ba_hostcheck_pcg).
// out_coarse (4 uint32): aggregate used, coarse unknowns, aggregates, padded coarse dimension; C / Cinv (optional):
// coarse unknowns x coarse unknowns, row-major.
extern "C" int ba_hostcheck_pcg2(uint32_t n, const double* a_lower, const double* b, uint32_t np, uint32_t D, double rel_tolerance,
                                 uint32_t max_iterations, uint32_t coarse_aggregate, double* x, uint32_t* out_u32, double* out_f64,
                                 uint32_t* out_coarse, double* C_out, double* Cinv_out) {
  if (out_coarse) out_coarse[0] = out_coarse[1] = out_coarse[2] = out_coarse[3] = 0;
  if (!coarse_aggregate) return ba_hostcheck_pcg(n, a_lower, b, np, D, rel_tolerance, max_iterations, x, out_u32, out_f64);
  if (np > n || D < 1 || D > bae::kPcgMaxBlock || n - np > bae::kPcgMaxBlock) return -1;
  const uint32_t nt = (n + 63) / 64, ld = 64 * nt;
  std::vector<double> A((size_t)ld * ld, 0.0), rhs(ld, 0.0), xx(ld, 0.0);
  std::vector<uint8_t> nz((size_t)nt * nt, 0);
  for (uint32_t r = 0; r < n; ++r)
    for (uint32_t c = 0; c <= r; ++c) {
      const double v = a_lower[(size_t)r * n + c];
      A[(size_t)r * ld + c] = v;
      if (v != 0.0) nz[(size_t)(r / 64) * nt + c / 64] = 1;
    }
  for (uint32_t r = n; r < ld; ++r) A[(size_t)r * ld + r] = 1.0;
  for (uint32_t r = 0; r < n; ++r) rhs[r] = b[r];
  bae::PcgPlan pl;
  bae::build_pcg_plan(nz, nt, pl);
  std::vector<uint32_t> blk, blocks, nat;
  bae::pcg_row_blocks(np, D, n - np, ld, blk, blocks);
  uint32_t nblk = 0;
  bae::pcg_natural_rows(np, D, n - np, ld, nat, nblk);
  bae::build_pcg_coarse(pl, nat, nblk, D, n - np, coarse_aggregate);
  bae::PcgResult res;
  std::vector<double> C, Cinv;
  const int rc = bae::pcg_host(pl, A.data(), ld, rhs.data(), n, nz, blk, blocks, rel_tolerance, max_iterations, xx.data(), &res,
                               true, &C, &Cinv);
  for (uint32_t r = 0; r < n; ++r) x[r] = xx[r];
  out_u32[0] = res.iterations; out_u32[1] = res.converged; out_u32[2] = res.replacements; out_u32[3] = res.breakdown;
  out_u32[4] = res.passes; out_u32[5] = pl.n_tiles;
  out_f64[0] = res.bb > 0.0 ? std::sqrt(res.rr_recur / res.bb) : 0.0;
  out_f64[1] = res.bb > 0.0 ? std::sqrt(res.rr_true / res.bb) : 0.0;
  out_f64[2] = std::sqrt(res.bb);
  if (out_coarse) { out_coarse[0] = pl.coarse_g; out_coarse[1] = pl.nc; out_coarse[2] = pl.naggr; out_coarse[3] = pl.ncp; }
  for (uint32_t r = 0; r < pl.nc; ++r)
    for (uint32_t c = 0; c < pl.nc; ++c) {
      if (C_out) C_out[(size_t)r * pl.nc + c] = C[(size_t)r * pl.ncp + c];
      if (Cinv_out) Cinv_out[(size_t)r * pl.nc + c] = Cinv[(size_t)r * pl.ncp + c];
    }
  return rc;
}

// C = Z^T S Z from a padded tile store (A: 64 nt x 64 nt, row-major; only the lower tiles of nz and the lower
// triangle of the diagonal tiles are read): the first n rows are np rows in blocks of D and a border of n - np.
// C_out: coarse unknowns x coarse unknowns (the caller sizes it by D ceil(ceil(np / D) / g) + n - np; the aggregate is
// not raised here: -1 if that exceeds the limit).  opt_of_natural (optional, np / D entries, np a multiple of D): the
// store holds the system under a pose ordering, block a of the natural order at block position opt_of_natural[a];
// the aggregates stay those of the natural order.  Returns the number of coarse unknowns.
extern "C" int ba_hostcheck_pcg_coarse(uint32_t nt, const uint8_t* nz, const double* A, uint32_t n, uint32_t np, uint32_t D,
                                       uint32_t coarse_aggregate, double* C_out, const uint32_t* opt_of_natural) {
  if (np > n || n > 64 * nt || D < 1 || D > bae::kPcgMaxBlock || !coarse_aggregate) return -1;
  if (opt_of_natural && np % D) return -1;
  std::vector<uint8_t> z(nz, nz + (size_t)nt * nt);
  bae::PcgPlan pl;
  bae::build_pcg_plan(z, nt, pl);
  std::vector<uint32_t> nat;
  uint32_t nblk = 0;
  bae::pcg_natural_rows(np, D, n - np, 64 * nt, nat, nblk);
  if (opt_of_natural)
    for (uint32_t a = 0; a < nblk; ++a)
      for (uint32_t d = 0; d < D; ++d) nat[(size_t)opt_of_natural[a] * D + d] = a * D + d;
  bae::build_pcg_coarse(pl, nat, nblk, D, n - np, coarse_aggregate);
  if (pl.coarse_g != coarse_aggregate) return -1;
  std::vector<double> C;
  bae::pcg_coarse_assemble_host(pl, A, (size_t)64 * nt, z, C);
  for (uint32_t r = 0; r < pl.nc; ++r)
    for (uint32_t c = 0; c < pl.nc; ++c) C_out[(size_t)r * pl.nc + c] = C[(size_t)r * pl.ncp + c];
  return (int)pl.nc;
}

// ---- leverages of projection residuals (lever.h) ---------------------------------------------------------
#include "lever.h"

// k_linearize's rows on the host, from the caller's per-residual Jacobians (unweighted) and weights: the lists of
// structure.h, the factor rows, obs_jl (sorted order) and the calibration rows
struct EmulatedRows {
  bae::Lists st;
  std::vector<double> frow, obs_jl, crow;
};
static int emulate_rows(int LM, int D, int K, uint32_t P, const uint8_t* pose_active, uint32_t L, const uint8_t* lm_active,
                        const uint32_t* lm_ref_pose, uint32_t O, const uint32_t* proj_pose, const uint32_t* proj_lm,
                        const double* jm12, const double* jr12, const double* jl, const double* jk12, const double* w,
                        EmulatedRows& er) {
  using namespace bae;
  Problem pb;
  pb.num_cams = 1; pb.num_poses = P; pb.num_lms = L; pb.num_proj = O;
  pb.pose_active.assign(pose_active, pose_active + P);
  pb.lm_active.assign(lm_active, lm_active + L);
  pb.lm_ref_pose.assign(lm_ref_pose, lm_ref_pose + L);
  pb.lm_ref_cam.assign(L, 0);
  pb.proj_pose.assign(proj_pose, proj_pose + O);
  pb.proj_lm.assign(proj_lm, proj_lm + O);
  pb.proj_cam.assign(O, 0);
  pb.proj_z.assign(2 * (size_t)O, 0.0);
  pb.proj_w.assign(O, 1.0);
  Lists& st = er.st;
  std::string err;
  if (!build_lists(pb, LM, D, st, err, nullptr, K)) return -2;
  const uint32_t R = st.R, WO = (uint32_t)w_row_offset(LM);
  std::vector<double>&frow = er.frow, &obs_jl = er.obs_jl, &crow = er.crow;
  frow.assign((size_t)st.n_rows * 6, 0.0);
  obs_jl.assign((size_t)O * 2 * LM, 0.0);
  crow.assign(K > 0 ? (2 * (size_t)O + L) * 6 : 0, 0.0);
  for (uint32_t l = 0; l < L; ++l) {
    const bool act = st.lm_opt[l] >= 0;
    for (uint32_t s = st.lm_ptr[l]; s < st.lm_ptr[l + 1]; ++s) {
      const uint32_t a = st.obs_rid[s];
      const bool same = LM == 1 && st.obs_pose[s] == lm_ref_pose[l];
      const double sw = std::sqrt(w[a]);
      const double* Jl = jl + 2 * LM * (size_t)a;
      double* rows = &frow[(size_t)s * R * 6];
      for (int i = 0; i < 12; ++i) {
        const double m = same ? 0.0 : jm12[12 * (size_t)a + i];
        rows[i] = m * sw;
        if (LM == 1) rows[12 + i] = (same ? 0.0 : jr12[12 * (size_t)a + i]) * sw;
      }
      if (K > 0)
        for (int r = 0; r < 2; ++r)
          for (int x = 0; x < K; ++x) crow[(2 * (size_t)s + r) * 6 + x] = jk12[12 * (size_t)a + 6 * r + x] * sw;
      if (!act) continue;
      for (int i = 0; i < 2 * LM; ++i) obs_jl[(size_t)s * 2 * LM + i] = Jl[i] * sw;
      for (int k = 0; k < LM; ++k)
        for (int x = 0; x < 6; ++x)
          rows[(WO + k) * 6 + x] = (rows[x] * Jl[k] + rows[6 + x] * Jl[LM + k]) * sw;
      if (LM == 1) {
        double* lr = &frow[((size_t)st.lrow_base + 2 * l) * 6];
        for (int x = 0; x < 6; ++x) lr[x] += (rows[12 + x] * Jl[0] + rows[18 + x] * Jl[1]) * sw;
      }
      if (K > 0)
        for (int x = 0; x < K; ++x)
          crow[(2 * (size_t)O + l) * 6 + x] += (crow[2 * (size_t)s * 6 + x] * Jl[0] + crow[(2 * (size_t)s + 1) * 6 + x] * Jl[1]) * sw;
    }
  }
  return 0;
}

// leverage_host on one graph: k_linearize's rows (factor rows, obs_jl, calibration rows) emulated from the
// caller's per-residual Jacobians (jk12: two rows of six per residual, or null with K == 0) and weights, then the
// device formula over the caller's dense Sigma (n x n, n = active poses * D + K, poses in id order).
// out: [O][4] by residual id.  variant: lever.h.
extern "C" int ba_hostcheck_leverages(int LM, int D, int K, uint32_t P, const uint8_t* pose_active, uint32_t L,
                                      const uint8_t* lm_active, const uint32_t* lm_ref_pose, uint32_t O,
                                      const uint32_t* proj_pose, const uint32_t* proj_lm, const double* jm12,
                                      const double* jr12, const double* jl, const double* jk12, const double* w,
                                      const double* sigma, int variant, double* out) {
  using namespace bae;
  if ((LM != 1 && LM != 3) || (K > 0 && !jk12) || K > 6) return -1;
  EmulatedRows er;
  if (int rc = emulate_rows(LM, D, K, P, pose_active, L, lm_active, lm_ref_pose, O, proj_pose, proj_lm, jm12, jr12, jl, jk12, w, er))
    return rc;
  const Lists& st = er.st;
  const std::vector<double>&frow = er.frow, &obs_jl = er.obs_jl, &crow = er.crow;
  LeverHostIn in;
  in.LM = LM; in.D = D; in.K = K; in.L = L; in.O = O; in.np = st.np; in.n = st.n; in.lrow_base = st.lrow_base;
  in.lm_ptr = st.lm_ptr.data(); in.obs_pose = st.obs_pose.data(); in.lm_ref_pose = lm_ref_pose;
  in.pose_opt = st.pose_opt.data(); in.lm_opt = st.lm_opt.data();
  in.frow = frow.data(); in.obs_jl = obs_jl.data(); in.crow = K > 0 ? crow.data() : nullptr;
  in.sigma = sigma;
  std::vector<double> sorted((size_t)O * 4, 0.0);
  leverage_host(in, variant, sorted.data());
  for (uint32_t s = 0; s < O; ++s)
    for (int i = 0; i < 4; ++i) out[4 * (size_t)st.obs_perm[s] + i] = sorted[4 * (size_t)s + i];
  return 0;
}

// ---- joint covariance of poses, calibration and landmarks (jointstate.h) -----------------------------------------
#include "jointstate.h"

// The mixed block on one graph: k_linearize's rows emulated as for ba_hostcheck_leverages, V^-1 by invert_v's rule
// from the weighted dz_dlm, the landmark columns of jointstate.h, then build_joint_plan + jointcov_host_rhs on the
// caller's dense S (n x n, n = active poses * D + K, poses in id order; factorised as for ba_hostcheck_selinv) and
// V^-1 on the diagonal landmark blocks.  Columns: poses (D each), calibration (K, when asked), landmarks (LM each),
// in the caller's order.  cov: M x M; reach_out: nt flags, or null.  variant: jointstate.h.
// Returns -1 bad arguments, -2 the lists, -3 an id out of range or inactive, -4 a zero pivot.
extern "C" int ba_hostcheck_joint_state(int LM, int D, int K, uint32_t P, const uint8_t* pose_active, uint32_t L,
                                        const uint8_t* lm_active, const uint32_t* lm_ref_pose, uint32_t O,
                                        const uint32_t* proj_pose, const uint32_t* proj_lm, const double* jm12,
                                        const double* jr12, const double* jl, const double* jk12, const double* w,
                                        uint32_t n, const double* S, uint32_t n_poses, const uint32_t* pose_ids,
                                        int include_calibration, uint32_t n_lms, const uint32_t* lm_ids, int variant,
                                        double* cov, uint8_t* reach_out) {
  using namespace bae;
  if ((LM != 1 && LM != 3) || (K > 0 && !jk12) || K > 6 || !S || !cov || (include_calibration && !K)) return -1;
  EmulatedRows er;
  if (int rc = emulate_rows(LM, D, K, P, pose_active, L, lm_active, lm_ref_pose, O, proj_pose, proj_lm, jm12, jr12, jl, jk12, w, er))
    return rc;
  const Lists& st = er.st;
  if (n != st.n) return -1;
  std::vector<double> vinv((size_t)L * LM * LM, 0.0);
  for (uint32_t l = 0; l < L; ++l) {
    if (st.lm_opt[l] < 0 || st.lm_ptr[l + 1] == st.lm_ptr[l]) continue;
    double V[9] = {0};
    for (uint32_t s = st.lm_ptr[l]; s < st.lm_ptr[l + 1]; ++s) {
      const double* B = &er.obs_jl[(size_t)s * 2 * LM];
      for (int a = 0; a < LM; ++a)
        for (int b = 0; b < LM; ++b) V[a * LM + b] += B[a] * B[b] + B[LM + a] * B[LM + b];
    }
    if (LM == 1) joint_invert_v_host<1>(V, &vinv[l]);
    else joint_invert_v_host<3>(V, &vinv[(size_t)l * 9]);
  }
  const uint32_t c0 = n_poses * (uint32_t)D + (include_calibration ? (uint32_t)K : 0), M = c0 + n_lms * (uint32_t)LM;
  std::vector<JointEntry> ent;
  std::vector<uint32_t> tiles;
  for (uint32_t i = 0; i < n_poses; ++i) {
    if (pose_ids[i] >= P || st.pose_opt[pose_ids[i]] < 0) return -3;
    for (int x = 0; x < D; ++x) ent.push_back({(uint32_t)st.pose_opt[pose_ids[i]] * D + x, i * D + x, 1.0});
  }
  if (include_calibration)
    for (int x = 0; x < K; ++x) ent.push_back({st.np + x, n_poses * D + x, 1.0});
  for (uint32_t i = 0; i < n_lms; ++i)
    if (lm_ids[i] >= L || st.lm_opt[lm_ids[i]] < 0) return -3;
  JointStateHostIn in;
  in.LM = LM; in.D = D; in.K = K; in.L = L; in.O = O; in.np = st.np; in.lrow_base = st.lrow_base;
  in.lm_ptr = st.lm_ptr.data(); in.obs_pose = st.obs_pose.data(); in.lm_ref_pose = lm_ref_pose;
  in.pose_opt = st.pose_opt.data();
  in.frow = er.frow.data(); in.crow = K > 0 ? er.crow.data() : nullptr; in.lm_vinv = vinv.data();
  joint_state_columns_host(in, n_lms, lm_ids, c0, variant, ent, nullptr);
  for (const JointEntry& x : ent) tiles.push_back(x.row / 64);
  const uint32_t nt = (n + 63) / 64, ld = 64 * nt;
  std::vector<uint8_t> nz;
  std::vector<double> Lf, d, linvT;
  if (host_tile_factor(n, S, nz, Lf, d, linvT)) return -4;
  JointPlan p;
  build_joint_plan(nz, nt, tiles, M, p);
  std::vector<double> Y(p.y_count());
  jointcov_host_rhs(p, Lf.data(), ld, linvT.data(), d.data(), ent.data(), ent.size(), Y.data(), cov);
  if (variant != 1) joint_state_add_vinv(in, n_lms, lm_ids, c0, M, cov);
  if (reach_out)
    for (uint32_t t = 0; t < nt; ++t) reach_out[t] = p.pos[t] != kJointNone;
  return 0;
}

// ---- leverages of unary, binary and inertial residuals (pplever.h) -----------------------------------------
#include "pplever.h"

// pose_pose_leverage_host on the caller's residuals: dz [nres][2][225] (dz1 | dz2, unmasked columns), info
// [nres][225] WITHOUT the weight, weight [nres] or null (Lambda = weight * info), p1 / p2 pose ids (p2 = 0xffffffff
// for a unary residual), activity and masks by pose id, dense Sigma (n x n, n = active poses * D, poses in id
// order).  cov, lam: [nres][225], lev: [nres]; any may be null.  variant: pplever.h.
extern "C" int ba_hostcheck_pose_pose_leverages(int D, uint32_t P, const uint8_t* pose_active, const uint16_t* pose_mask,
                                                uint32_t nres, const uint32_t* p1, const uint32_t* p2, const double* dz,
                                                const double* info, const double* weight, uint32_t n, const double* sigma,
                                                int variant, double* cov, double* lam, double* lev) {
  using namespace bae;
  if (D < 6 || D > kPPLevDim || !pose_active || !pose_mask || !sigma || (nres && (!p1 || !p2 || !dz || !info))) return -1;
  std::vector<int32_t> opt(P, -1);
  uint32_t k = 0;
  for (uint32_t p = 0; p < P; ++p)
    if (pose_active[p]) opt[p] = (int32_t)k++;
  if (n != k * (uint32_t)D) return -2;
  for (uint32_t q = 0; q < nres; ++q)
    if (p1[q] >= P || (p2[q] != kPPLevNoPose && p2[q] >= P)) return -3;
  PPLeverHostIn in;
  in.D = D; in.nres = nres; in.n = n; in.p1 = p1; in.p2 = p2; in.pose_opt = opt.data(); in.pose_mask = pose_mask;
  in.dz = dz; in.info = info; in.weight = weight; in.sigma = sigma;
  pose_pose_leverage_host(in, variant, cov, lam, lev);
  return 0;
}

// ---- engine lifecycle record -----------------------------------------------------------------------
#include "lifecycle.h"

// The events of lifecycle.h (HeldEvent codes) replayed in order on a fresh record: bits[i] = the flags after
// events[i], one bit per flag in HeldBit order.  Returns 0, or -(i + 1) at the first unknown code.
extern "C" int ba_hostcheck_lifecycle(uint32_t n, const int32_t* events, uint32_t* bits) {
  bae::Held h;
  for (uint32_t i = 0; i < n; ++i) {
    if (!bae::held_apply(h, events[i])) return -(int)(i + 1);
    bits[i] = bae::held_bits(h);
  }
  return 0;
}

// ---- switches and launch shapes of the LDL^T solve ---------------------------------------------------
#include "chol_launch.h"

// chol_launch.h on n rows of integers: row i reads in[i * W_in ...] and writes out[i * W_out ...]; `str` holds the
// strings of the one row of ops 0, 5 and 7 (null = variable unset).  Returns 0, or -1 for an unknown op.
//   0  switch parsing   in: nblk; str: NO128 NO_LOOKAHEAD BULK_FULL DENSE NO_DIST_SOLVE SBL BULK_FULL_M | KOUT
//                       LEFT_MIN_TILES SQUARE SQ_W DIST_LAYOUT DENSE_SCATTER TRACE_FILE; out: the 15 fields in the
//                       struct's order (the two strings as set / unset)
//   1  chain_shape      in: nblk left_min_tiles; out: left kin
//   2  rect128_shape    in: rule nblk c0 ncols G no128 rect_min_rows; out: use128 m2 rect_cols nrow64 grid
//   3  bulk_shape       in: nblk a_end full own_n own_G have_pairs npairs no128 sbl; out: kernel grid nrow64 m2 sbl swzf
//   4  FactorWork       in: nblk; out: dsgn linvT opbuf colneg total packet_stride
//   5  dist_plan_key    in: nzL_version kout pat dense_scatter; str: layout; out: key
//   7  the epilogue switch of k_update128   str: C_RMW; out: c_rmw   (6 stays unknown: tests/test_chol_launch.py)
//   8  the launch switch of the bulk update   str: BULK_GRID; out: bulk_grid
//   9  bulk_shape with a block list   in: nblk a_end full own_n own_G have_pairs npairs no128 sbl list_len bulk_grid
//                                     (list_len < 0: no list); out: as 3
extern "C" int ba_hostcheck_chol_launch(int op, uint32_t n, const int64_t* in, const char* const* str, int64_t* out) {
  using namespace bae;
  for (uint32_t i = 0; i < n; ++i) {
    CholSwitches sw;
    if (op == 0) {
      parse_process_switches(&sw, str[0], str[1], str[2], str[3], str[4], str[5], str[6]);
      parse_call_switches(&sw, (uint32_t)in[0], str[7], str[8], str[9], str[10], str[11], str[12], str[13]);
      const int64_t v[15] = {sw.no128, sw.no_lookahead, sw.bulk_full, sw.dense, sw.no_dist_solve, sw.sbl,
                             sw.rect_min_rows, sw.bulk_full_m, sw.kout, sw.left_min_tiles, sw.square, sw.sq_w,
                             sw.dist_layout != nullptr, sw.dense_scatter, sw.trace_file != nullptr};
      std::copy(v, v + 15, out);
    } else if (op == 1) {
      const int64_t* a = in + (size_t)i * 2;
      sw.left_min_tiles = (uint32_t)a[1];
      const ChainShape c = chain_shape((uint32_t)a[0], sw);
      out[(size_t)i * 2] = c.left; out[(size_t)i * 2 + 1] = c.kin;
    } else if (op == 2) {
      const int64_t* a = in + (size_t)i * 7;
      sw.no128 = a[5] != 0; sw.rect_min_rows = (uint32_t)a[6];
      const Rect128Shape r = rect128_shape(a[0] ? kRectDist : kRectSingle, (uint32_t)a[1], (uint32_t)a[2], (uint32_t)a[3],
                                           (uint32_t)a[4], sw);
      const int64_t v[5] = {r.use128, r.m2, r.rect_cols, r.nrow64, r.grid};
      std::copy(v, v + 5, out + (size_t)i * 5);
    } else if (op == 3) {
      const int64_t* a = in + (size_t)i * 9;
      sw.no128 = a[7] != 0; sw.sbl = (uint32_t)a[8];
      const BulkShape b = bulk_shape((uint32_t)a[0], (uint32_t)a[1], a[2] != 0, (uint32_t)a[3], (uint32_t)a[4], a[5] != 0,
                                     (uint32_t)a[6], sw);
      const int64_t v[6] = {b.kernel, b.grid, b.nrow64, b.m2, b.sbl, b.swzf};
      std::copy(v, v + 6, out + (size_t)i * 6);
    } else if (op == 4) {
      const FactorWork fw((uint32_t)in[i]);
      const int64_t v[6] = {(int64_t)fw.dsgn, (int64_t)fw.linvT, (int64_t)fw.opbuf, (int64_t)fw.colneg, (int64_t)fw.total,
                            kPacketStride};
      std::copy(v, v + 6, out + (size_t)i * 6);
    } else if (op == 5) {
      out[0] = (int64_t)dist_plan_key((uint64_t)in[0], (uint32_t)in[1], in[2] != 0, str[0], in[3] != 0);
    } else if (op == 7) {
      parse_process_switches(&sw, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, str[0]);
      out[0] = sw.c_rmw;
    } else if (op == 8) {
      parse_process_switches(&sw, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, str[0]);
      out[0] = sw.bulk_grid;
    } else if (op == 9) {
      const int64_t* a = in + (size_t)i * 11;
      sw.no128 = a[7] != 0; sw.sbl = (uint32_t)a[8]; sw.bulk_grid = a[10] != 0;
      const BulkShape b = bulk_shape((uint32_t)a[0], (uint32_t)a[1], a[2] != 0, (uint32_t)a[3], (uint32_t)a[4], a[5] != 0,
                                     (uint32_t)a[6], sw, a[9]);
      const int64_t v[6] = {b.kernel, b.grid, b.nrow64, b.m2, b.sbl, b.swzf};
      std::copy(v, v + 6, out + (size_t)i * 6);
    } else {
      return -1;
    }
  }
  return 0;
}

// ---- the block lists of the bulk updates (bulk_lists.h) ----------------------------------------------------------
#include "bulk_lists.h"

// build_bulk_lists on the pattern nz (nblk x nblk bytes, lower; null = none).  hdr = nblk kout no128 bulk_full_m
// full_always (BA_HIP_NO_LOOKAHEAD or BA_HIP_BULK_FULL) bulk_grid dense; budget: bytes on the device, < 0 = the default.
// out (cap entries): built nlaunches total_blocks nentries | (a_end J Jend first len blocks xcd_blocks[8]) per launch |
// (R C mask) per entry, sentinels as R = C = 2^32 - 1.  Returns the count, or -3 when out is too short.
extern "C" int64_t ba_hostcheck_bulk_lists(const uint32_t* hdr, const uint8_t* nz, int64_t budget, int64_t* out, uint64_t cap) {
  using namespace bae;
  CholSwitches sw;
  sw.no128 = hdr[2] != 0; sw.bulk_full_m = hdr[3]; sw.bulk_full = hdr[4] != 0; sw.bulk_grid = hdr[5] != 0; sw.dense = hdr[6] != 0;
  const BulkLists l = budget < 0 ? build_bulk_lists(hdr[0], hdr[1], nz, sw) : build_bulk_lists(hdr[0], hdr[1], nz, sw, (size_t)budget);
  const size_t need = 4 + 14 * l.launches.size() + 3 * l.entries.size();
  if (need > cap) return -3;
  int64_t* o = out;
  *o++ = l.built; *o++ = (int64_t)l.launches.size(); *o++ = (int64_t)l.total_blocks; *o++ = (int64_t)l.entries.size();
  for (const BulkLaunchList& b : l.launches) {
    *o++ = b.a_end; *o++ = b.J; *o++ = b.Jend; *o++ = b.first; *o++ = b.len; *o++ = b.blocks;
    for (uint32_t x = 0; x < 8; ++x) *o++ = b.xcd_blocks[x];
  }
  for (const BulkEntry& b : l.entries) { *o++ = b.R; *o++ = b.C; *o++ = (int64_t)b.mask; }
  return (int64_t)need;
}

// ---- the derived tables of the distributed solve ---------------------------------------------------------------
#include "dist_plan.h"

// dist_plan.h on one plan: hdr = nblk G nranks rank, `layout` as BA_HIP_DIST_LAYOUT, nzL the factor pattern the plan
// is built from (nblk x nblk bytes, null = dense; self messages as the engine sets them).  The result goes to out
// (cap entries) as integers; returns their count, -1 for an unknown op, -2 when the layout gives no plan, -3 when out
// is too short.
//   0  dist_owned_pairs         out: npairs | pair_first[nb + 1] | (bi bc) per pair
//   1  dist_square_rows         out: the list
//   2  dist_dense_scatter_rows  nz2: nzS or null; out: chunk nrows | off[nb N + 1] | chunk_off[nb N] | rows
//   3  dist_sparse_rects        bits: the N local patterns (dist_pattern_words(nblk) words each); arg[0]: the limit, < 0 =
//                               the default; out: refused nsend nrecv | send_first[N + 1] | recv_first[N + 1] |
//                               send_off[N + 1] | recv_off[N + 1] | (row col width off) per send, per recv rectangle;
//                               msg: the refusal
//   4  dist_assembly_need       nz2: the local pattern (nzL required); out: nblk x nblk marks
//   5  dist_staging_caps        out: usend urecv ssend srecv
//   6  bulk_update_tile_products  arg: first c0 c1 single (1: own_map_single(), the plan's map otherwise); out: the count
//   7  the plan itself          out: nb T nmsgs | tbl[T T] | (c0 c1 diag_owner) per panel | (panel src urgent ntiles
//                               ndst, the tiles, the receivers) per message
extern "C" int64_t ba_hostcheck_dist_tables(int op, const uint32_t* hdr, const char* layout, const uint8_t* nzL, const uint8_t* nz2,
                                            const uint64_t* bits, const int64_t* arg, int64_t* out, uint64_t cap, char* msg,
                                            uint32_t msg_cap) {
  using namespace bae;
  const uint32_t nblk = hdr[0], N = hdr[2], rank = hdr[3];
  OwnMap map;
  if (!build_own_map(N, layout, hdr[1], &map, nullptr)) return -2;
  map.rank = rank;
  const DistPlan pl = build_dist_plan(nblk, map, nzL, N == 1);
  std::vector<int64_t> v;
  auto put = [&](const auto& list) { v.insert(v.end(), list.begin(), list.end()); };
  if (op == 0) {
    const DistOwnedPairs o = dist_owned_pairs(pl);
    v.push_back((int64_t)o.pairs.size());
    put(o.pair_first);
    for (const DistPair& p : o.pairs) { v.push_back(p.bi); v.push_back(p.bc); }
  } else if (op == 1) {
    put(dist_square_rows(pl));
  } else if (op == 2) {
    const DistDenseRows d = dist_dense_scatter_rows(pl, nz2);
    v.push_back((int64_t)d.chunk); v.push_back((int64_t)d.rows.size());
    put(d.off); put(d.chunk_off); put(d.rows);
  } else if (op == 3) {
    const size_t words = dist_pattern_words(nblk);
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "pattern words");
    const unsigned long long* all = reinterpret_cast<const unsigned long long*>(bits);
    const DistSparseRects t = arg[0] < 0 ? dist_sparse_rects(pl, rank, all, words)
                                         : dist_sparse_rects(pl, rank, all, words, (uint64_t)arg[0]);
    v.push_back(!t.refused.empty()); v.push_back((int64_t)t.send.size()); v.push_back((int64_t)t.recv.size());
    put(t.send_first); put(t.recv_first); put(t.send_off); put(t.recv_off);
    for (const std::vector<DistRect>* l : {&t.send, &t.recv})
      for (const DistRect& r : *l) { v.push_back(r.row); v.push_back(r.col); v.push_back(r.width); v.push_back(r.off); }
    if (msg && msg_cap) {
      const size_t k = std::min<size_t>(t.refused.size(), msg_cap - 1);
      std::copy(t.refused.begin(), t.refused.begin() + k, msg);
      msg[k] = 0;
    }
  } else if (op == 4) {
    if (!nzL || !nz2) return -2;
    put(dist_assembly_need(pl, rank, nz2, nzL));
  } else if (op == 5) {
    const DistStagingCaps c = dist_staging_caps(pl, rank);
    for (size_t x : {c.usend, c.urecv, c.ssend, c.srecv}) v.push_back((int64_t)x);
  } else if (op == 6) {
    v.push_back((int64_t)bulk_update_tile_products(arg[3] ? own_map_single() : pl.map, arg[3] ? 0 : rank, nblk, (uint32_t)arg[0],
                                                   (uint32_t)arg[1], (uint32_t)arg[2], nzL));
  } else if (op == 7) {
    v.push_back(pl.nb); v.push_back(map.T); v.push_back((int64_t)pl.msgs.size());
    for (uint32_t a = 0; a < map.T; ++a)
      for (uint32_t b = 0; b < map.T; ++b) v.push_back(N > 1 ? map.tbl[a][b] : 0);
    for (const DistPanel& pn : pl.panels) { v.push_back(pn.c0); v.push_back(pn.c1); v.push_back(pn.diag_owner); }
    for (const DistMsg& m : pl.msgs) {
      v.push_back(m.panel); v.push_back(m.src); v.push_back(m.urgent); v.push_back(m.count); v.push_back((int64_t)m.dst.size());
      v.insert(v.end(), pl.tiles.begin() + m.first, pl.tiles.begin() + m.first + m.count);
      put(m.dst);
    }
  } else {
    return -1;
  }
  if (v.size() > cap) return -3;
  std::copy(v.begin(), v.end(), out);
  return (int64_t)v.size();
}

// ---- panel PCG (pcg_panel.h) --------------------------------------------------------------------------------
#include "pcg_panel.h"

// One product Q = S P by the panel plan on the lower storage A (row-major, 64 nt x 64 nt; tiles outside nz and the
// strict upper triangle of diagonal tiles are not read).  P, Q: (64 nt) x m row-major.  variant: 0, or one of the
// deliberately wrong ones of pcg_panel.h.  out_u32: sources, chunks.
extern "C" int ba_hostcheck_pcg_spmm(uint32_t nt, const uint8_t* nz, const double* A, uint32_t m, const double* P, double* Q,
                                     int variant, uint32_t* out_u32) {
  if (!nt || !m || m > bae::kPcgPanelMaxColumns) return -1;
  std::vector<uint8_t> z(nz, nz + (size_t)nt * nt);
  bae::PcgPlan pl;
  bae::build_pcg_plan(z, nt, pl);
  bae::PcgPanelPlan pp;
  bae::build_pcg_panel_plan(pl, m, pp);
  bae::pcg_panel_spmm_host(pp, A, (size_t)64 * nt, P, m, nullptr, Q, nullptr, variant);
  if (out_u32) { out_u32[0] = pp.n_src(); out_u32[1] = pp.n_chunks(); }
  return 0;
}

// pcg_panel_host on a symmetric n x n system given dense (row-major n x n; the LOWER triangle is read), padded like
// the engine pads A.  tile_map (optional, nt x nt bytes): tiles that belong to the pattern beside those of the
// nonzeros.  np rows in blocks of D, then one block of K = n - np.  B, X: n x m row-major.  Per column j: out_u32[4 j
// ..] = iterations, converged, breakdown, residual replacements; out_f64[2 j ..] = relative residual, true and of
// the recurrence.  out_scalar: passes, tiles, sources, chunks.
extern "C" int ba_hostcheck_pcg_panel(uint32_t n, const double* S, const uint8_t* tile_map, uint32_t m, const double* B,
                                      uint32_t np, uint32_t D, double rel_tolerance, uint32_t max_iterations, int variant,
                                      double* X, uint32_t* out_u32, double* out_f64, uint32_t* out_scalar) {
  if (!n || np > n || D < 1 || D > bae::kPcgMaxBlock || n - np > bae::kPcgMaxBlock || !m || m > bae::kPcgPanelMaxColumns) return -1;
  const uint32_t nt = (n + 63) / 64, ld = 64 * nt;
  std::vector<double> A((size_t)ld * ld, 0.0), Bp((size_t)ld * m, 0.0), Xp((size_t)ld * m, 0.0);
  std::vector<uint8_t> nz((size_t)nt * nt, 0);
  for (uint32_t r = 0; r < n; ++r)
    for (uint32_t c = 0; c <= r; ++c) {
      const double v = S[(size_t)r * n + c];
      A[(size_t)r * ld + c] = v;
      if (v != 0.0) nz[(size_t)(r / 64) * nt + c / 64] = 1;
    }
  if (tile_map)
    for (size_t i = 0; i < nz.size(); ++i) nz[i] |= tile_map[i] ? 1 : 0;
  for (uint32_t r = n; r < ld; ++r) A[(size_t)r * ld + r] = 1.0;
  std::copy(B, B + (size_t)n * m, Bp.begin());
  bae::PcgPlan pl;
  bae::build_pcg_plan(nz, nt, pl);
  bae::PcgPanelPlan pp;
  bae::build_pcg_panel_plan(pl, m, pp);
  std::vector<uint32_t> blk, blocks;
  bae::pcg_row_blocks(np, D, n - np, ld, blk, blocks);
  bae::PcgPanelResult res;
  const int rc = bae::pcg_panel_host(pl, pp, A.data(), ld, Bp.data(), m, n, nz, blk, blocks, rel_tolerance, max_iterations,
                                     Xp.data(), &res, variant);
  std::copy(Xp.begin(), Xp.begin() + (size_t)n * m, X);
  for (uint32_t j = 0; j < m; ++j) {
    const bae::PcgResult& c = res.col[j];
    out_u32[4 * j] = c.iterations; out_u32[4 * j + 1] = c.converged; out_u32[4 * j + 2] = c.breakdown; out_u32[4 * j + 3] = c.replacements;
    out_f64[2 * j] = c.bb > 0.0 ? std::sqrt(c.rr_true / c.bb) : 0.0;
    out_f64[2 * j + 1] = c.bb > 0.0 ? std::sqrt(c.rr_recur / c.bb) : 0.0;
  }
  if (out_scalar) { out_scalar[0] = res.passes; out_scalar[1] = pl.n_tiles; out_scalar[2] = pp.n_src(); out_scalar[3] = pp.n_chunks(); }
  return rc;
}

// ---- the request layer (requests.h) ---------------------------------------------------------------------------
#include "requests.h"

// the message into msg (cap bytes with the terminator); 0 = served, 1 = refused
static int put_message(const std::string& m, char* msg, uint32_t cap) {
  if (msg && cap) {
    const size_t k = std::min<size_t>(m.size(), cap - 1);
    std::copy(m.begin(), m.begin() + k, msg);
    msg[k] = 0;
  }
  return m.empty() ? 0 : 1;
}

// The events replayed on a fresh record as ba_hostcheck_lifecycle does, then one named guard of requests.h.
// facts: bit 0 distributed solve, 1 sharded, 2 hooked, 3 kept copy, 4 the PCG plan fits, 5 (value 32) damped.  flags: bit 0 foreign_ok
// (kept_factor), bit 1 landmarks (kept_factor, marginals), bit 2 the caller passed PCG options (pcg_panel), bit 3
// calibration unknowns (marginalize).  noun: kept_factor only, null for the calibration wording.
// Returns 0 (served), 1 (refused, the message in msg), -(i + 1) at the first unknown event code, -1000 for an
// unknown guard.
extern "C" int ba_hostcheck_guard(uint32_t n, const int32_t* events, const char* guard, const char* who, const char* noun,
                                  uint32_t facts, uint32_t flags, double rel_tolerance, uint32_t coarse_aggregate, char* msg,
                                  uint32_t cap) {
  using namespace bae;
  Held h;
  for (uint32_t i = 0; i < n; ++i)
    if (!held_apply(h, events[i])) return -(int)(i + 1);
  const GuardFacts f = {(facts & 1) != 0, (facts & 2) != 0, (facts & 4) != 0, (facts & 8) != 0, (facts & 16) != 0,
                        (facts & 32) != 0};
  const PcgAsk ask = {rel_tolerance, coarse_aggregate};
  const std::string g = guard;
  if (g == "kept_factor") return put_message(guard_kept_factor(h, f, who, noun, flags & 1, (flags & 2) != 0), msg, cap);
  if (g == "marginals") return put_message(guard_marginals(h, f, who, (flags & 2) != 0), msg, cap);
  if (g == "pcg_panel") return put_message(guard_pcg_panel(h, f, who, flags & 4 ? &ask : nullptr), msg, cap);
  if (g == "check_solve") return put_message(guard_check_solve(h, f), msg, cap);
  if (g == "get_S") return put_message(guard_get_S(h, f), msg, cap);
  if (g == "pcg_stats") return put_message(guard_pcg_stats(h), msg, cap);
  if (g == "pcg_coarse_stats") return put_message(guard_pcg_coarse_stats(h), msg, cap);
  if (g == "marginalize") return put_message(guard_marginalize(h, f, (flags & 8) != 0), msg, cap);
  return -1000;
}

// select_rows on a structure given by its tables (n = np + K; n_perm entries of opt_of_natural, 0 = no ordering).
// rows_out (room for the request's columns) and lms_out (n_lms) receive the selection, counts[0 .. 1] their sizes.
extern "C" int ba_hostcheck_selection(uint32_t P, const int32_t* pose_opt, uint32_t L, const int32_t* lm_opt, uint32_t np,
                                      uint32_t K, uint32_t D, uint32_t LM, uint32_t ld, uint32_t n_perm,
                                      const uint32_t* opt_of_natural, const char* who, uint32_t n_poses, const uint32_t* pose_ids,
                                      int include_calibration, uint32_t n_lms, const uint32_t* lm_ids, int have_out,
                                      uint64_t limit, const char* limit_name, const char* nothing, int caller_numbering,
                                      uint32_t* rows_out, uint32_t* lms_out, uint32_t* counts, char* msg, uint32_t cap) {
  using namespace bae;
  const std::vector<int32_t> po(pose_opt, pose_opt + P), lo(lm_opt, lm_opt + L);
  const std::vector<uint32_t> perm(opt_of_natural, opt_of_natural + n_perm);
  const StructureView v = {P, L, np, K, np + K, ld, D, LM, &po, &lo, &perm};
  RowSelection s;
  const int rc = put_message(select_rows(v, {who, n_poses, pose_ids, include_calibration != 0, n_lms, lm_ids, have_out != 0, limit,
                                             limit_name, nothing, caller_numbering != 0}, &s), msg, cap);
  if (rc) return rc;
  std::copy(s.rows.begin(), s.rows.end(), rows_out);
  std::copy(s.lms.begin(), s.lms.end(), lms_out);
  counts[0] = (uint32_t)s.rows.size(); counts[1] = (uint32_t)s.lms.size();
  return 0;
}

// The small checks: op 0 ids_or_all (u: have ids, n, count; name: the count's name), 1 pcg_options_ok (d: tolerance;
// u: coarse_aggregate, the PcgCoarse mode), 2 block_ok (u: block), 3 columns_ok (u: m, limit; name: the limit's).
extern "C" int ba_hostcheck_request_check(int op, const char* who, const char* name, const uint64_t* u, const double* d, char* msg,
                                          uint32_t cap) {
  using namespace bae;
  if (op == 0) return put_message(ids_or_all(who, u[0] ? who : nullptr, (uint32_t)u[1], (uint32_t)u[2], name), msg, cap);
  if (op == 1) return put_message(pcg_options_ok(who, {d[0], (uint32_t)u[0]}, (PcgCoarse)u[1]), msg, cap);
  if (op == 2) return put_message(block_ok(who, (uint32_t)u[0]), msg, cap);
  if (op == 3) return put_message(columns_ok(who, u[0], u[1], name), msg, cap);
  return -1000;
}

// natural_rowmap of np pose rows in blocks of D under opt_of_natural (n_perm entries, 0 = none) and K border rows, and
// identity_rowmap(np + K, ld): ld entries each
extern "C" void ba_hostcheck_rowmaps(uint32_t np, uint32_t K, uint32_t D, uint32_t ld, uint32_t n_perm,
                                     const uint32_t* opt_of_natural, uint32_t* natural_out, uint32_t* identity_out) {
  using namespace bae;
  const std::vector<int32_t> none;
  const std::vector<uint32_t> perm(opt_of_natural, opt_of_natural + n_perm);
  const StructureView v = {0, 0, np, K, np + K, ld, D, 0, &none, &none, &perm};
  const std::vector<uint32_t> a = natural_rowmap(v), b = identity_rowmap(np + K, ld);
  std::copy(a.begin(), a.end(), natural_out);
  std::copy(b.begin(), b.end(), identity_out);
}

#include "damping.h"
// The damping rules of damping.h.  op 0: damp_clamp(in[0]) -> out[0].  1: damp_update on (lambda, nu) = in[0 .. 1]
// with rho = in[2] -> out = (lambda, nu, accepted).  2: damp_terms_host on n parameters, in = delta | g | d -> out =
// (delta^T D delta, predicted decrease).  3: damp_v<n> on the unique entries in[0 ..] of V (n = 1 | 3) -> out = the
// damped entries, then d_l.  4: damp_pose_diag(in[0], in[1]) -> out[0].  5: damp_keep_lambda(in[0]) -> out[0].
// 6: damp_gain_ratio(in[0], in[1], in[2]) -> out[0].  Returns 0, -1000 for an unknown op.
extern "C" int ba_hostcheck_damping(int op, uint32_t n, const double* in, double lambda, double* out) {
  using namespace bae;
  if (op == 0) { out[0] = damp_clamp(in[0]); return 0; }
  if (op == 1) {
    DampState s = {in[0], in[1]};
    const bool ok = damp_update(&s, in[2]);
    out[0] = s.lambda; out[1] = s.nu; out[2] = ok ? 1.0 : 0.0;
    return 0;
  }
  if (op == 2) { damp_terms_host(n, in, in + n, in + 2 * (size_t)n, lambda, out, out + 1); return 0; }
  if (op == 3 && (n == 1 || n == 3)) {
    const uint32_t nv = n * (n + 1) / 2;
    std::copy(in, in + nv, out);
    if (n == 1) damp_v<1>(out, lambda, out + nv);
    else damp_v<3>(out, lambda, out + nv);
    return 0;
  }
  if (op == 4) { out[0] = damp_pose_diag(in[0], in[1]); return 0; }
  if (op == 5) { out[0] = damp_keep_lambda(in[0]); return 0; }
  if (op == 6) { out[0] = damp_gain_ratio(in[0], in[1], in[2]); return 0; }
  return -1000;
}

// ---- pose-pose lists and the tile pattern of the non-projection terms (structure.h) -------------------------
// The finalize steps of a graph without projections, as build_structure runs them: build_lists (opt ids under the
// optional opt_of_natural, n_perm entries or 0), build_pose_pose_lists, mark_pose_pose_tiles with the prior cliques as
// CSR.  Then k_pp_scatter restated for the host exactly as the kernel is written: block-row j of the lower storage per
// active pose, its entries in order, H11 / H22 on the diagonal block, H12 (side 1: transposed) on block (j, other) when
// other < j, g1 / g2 on the right-hand side (the kernel adds them to rhs_p and rhs_sc alike), rows and columns of masked
// parameters skipped.  pose_mask: [P] by pose id; pp_h: [nres][3][225] = H11 | H12 | H22 with row stride 15; pp_g:
// [nres][30] = g1 | g2; slots [unary | binary | imu].  The caller sizes S_lower (ld x ld), rhs (ld) and tile_nz
// ((ld / 64)^2) with ld = max(64, round_up(Pact D + K, 64)); pp_ptr takes Pact + 1 words, pp_ent 4 words for each of at
// most 2 nres entries.  counts: Pact, n, ld, n_pp_entries, nres.  Returns 0; 1 with the builder's message in msg; -2
// when ld is not the structure's.
extern "C" int ba_hostcheck_pose_pose_lists(
    int D, int K, uint32_t P, const uint8_t* pose_active, uint32_t n_perm, const uint32_t* opt_of_natural, uint32_t nu,
    const uint32_t* un_pose, uint32_t nb, const uint32_t* bin_p1, const uint32_t* bin_p2, uint32_t ni, const uint32_t* imu_p1,
    const uint32_t* imu_p2, uint32_t nq, const uint32_t* prior_ptr, const uint32_t* prior_pose, const uint16_t* pose_mask,
    const double* pp_h, const double* pp_g, uint32_t ld, double* S_lower, double* rhs, uint8_t* tile_nz, uint32_t* counts,
    uint32_t* pp_ptr, uint32_t* pp_ent, char* msg, uint32_t cap) {
  using namespace bae;
  Problem pb;
  pb.num_poses = P; pb.num_unary = nu; pb.num_binary = nb; pb.num_imu = ni;
  pb.pose_active.assign(pose_active, pose_active + P);
  pb.un_pose.assign(un_pose, un_pose + nu);
  pb.bin_p1.assign(bin_p1, bin_p1 + nb); pb.bin_p2.assign(bin_p2, bin_p2 + nb);
  pb.imu_p1.assign(imu_p1, imu_p1 + ni); pb.imu_p2.assign(imu_p2, imu_p2 + ni);
  const std::vector<uint32_t> perm(opt_of_natural, opt_of_natural + n_perm);
  Lists st;
  PosePoseLists pp;
  std::string err;
  if (!build_lists(pb, 0, D, st, err, nullptr, K, &perm) || !build_pose_pose_lists(pb, st, pp, err)) return put_message(err, msg, cap);
  for (uint32_t k = 0; k < (nq ? prior_ptr[nq] : 0); ++k)   // (priors_upload's check)
    if (prior_pose[k] >= P) return put_message("dense prior on an unknown pose", msg, cap);
  mark_pose_pose_tiles(pb, nq, prior_ptr, prior_pose, D, st);
  put_message("", msg, cap);
  const uint32_t nres = nu + nb + ni;
  counts[0] = st.Pact; counts[1] = st.n; counts[2] = st.ld; counts[3] = st.n_pp_entries; counts[4] = nres;
  if (ld != st.ld) return -2;
  std::copy(st.tile_nz.begin(), st.tile_nz.end(), tile_nz);
  std::copy(pp.pp_ptr.begin(), pp.pp_ptr.end(), pp_ptr);
  static_assert(sizeof(U4) == 4 * sizeof(uint32_t), "a scatter entry is four words");
  if (st.n_pp_entries) std::memcpy(pp_ent, pp.pp_ent.data(), (size_t)st.n_pp_entries * sizeof(U4));
  std::vector<uint16_t> mask_opt(st.Pact, 0);
  for (uint32_t p = 0; p < P; ++p)
    if (st.pose_opt[p] >= 0) mask_opt[st.pose_opt[p]] = pose_mask[p];
  // ---- k_pp_scatter ----------------------------------------------------------------------------------
  std::memset(S_lower, 0, sizeof(double) * (size_t)ld * ld);
  std::fill(rhs, rhs + ld, 0.0);
  const int kPPH = 225;
  for (uint32_t j = 0; j < st.Pact; ++j) {
    const uint16_t mj = mask_opt[j];
    for (uint32_t e = pp.pp_ptr[j]; e < pp.pp_ptr[j + 1]; ++e) {
      const U4 en = pp.pp_ent[e];
      if (en.x >= nres || en.y > 1 || (en.z != kNoPose && en.z >= st.Pact)) return -3;   // what the kernel would read
      const double* h = pp_h + (size_t)en.x * 3 * kPPH;
      const double* g = pp_g + (size_t)en.x * 30;
      for (int r = 0; r < D; ++r)
        for (int c = 0; c < D; ++c) {
          if (!(mj & (1u << r)) && !(mj & (1u << c)))
            S_lower[((size_t)j * D + r) * ld + (size_t)j * D + c] += (en.y == 0 ? h : h + 2 * kPPH)[r * 15 + c];
          if (en.z != kNoPose && en.z < j && !(mj & (1u << r)) && !(mask_opt[en.z] & (1u << c)))
            S_lower[((size_t)j * D + r) * ld + (size_t)en.z * D + c] += en.y == 0 ? h[kPPH + r * 15 + c] : h[kPPH + c * 15 + r];
        }
      for (int t = 0; t < D; ++t)
        if (!(mj & (1u << t))) rhs[(size_t)j * D + t] += g[en.y * 15 + t];
    }
  }
  return 0;
}

// coupling_group_edges of the same graph arguments: the group pairs (a << 32 | b, a < b; natural opt id / group size of
// PoseSize D) that order_poses adds to the projection part's before group_graph_csr, in enumeration order with
// duplicates.  Returns their number; fills at most cap.
extern "C" uint64_t ba_hostcheck_coupling_group_edges(int D, uint32_t P, const uint8_t* pose_active, uint32_t nb,
                                                      const uint32_t* bin_p1, const uint32_t* bin_p2, uint32_t ni,
                                                      const uint32_t* imu_p1, const uint32_t* imu_p2, uint32_t nq,
                                                      const uint32_t* prior_ptr, const uint32_t* prior_pose, uint64_t* edges,
                                                      uint64_t cap) {
  using namespace bae;
  Problem pb;
  pb.num_poses = P; pb.num_binary = nb; pb.num_imu = ni;
  pb.pose_active.assign(pose_active, pose_active + P);
  pb.bin_p1.assign(bin_p1, bin_p1 + nb); pb.bin_p2.assign(bin_p2, bin_p2 + nb);
  pb.imu_p1.assign(imu_p1, imu_p1 + ni); pb.imu_p2.assign(imu_p2, imu_p2 + ni);
  std::vector<int32_t> nat;
  natural_pose_opt(pb, nat);
  std::vector<uint64_t> out;
  coupling_group_edges(pb, nq, prior_ptr, prior_pose, nat, pose_group_size(D), out);
  std::copy(out.begin(), out.begin() + std::min<uint64_t>(out.size(), cap), edges);
  return out.size();
}

// ---- landmark triangulation (triang.h) --------------------------------------------------------------------------
#include "triang.h"

// The rules of triang.h on the host, landmark by landmark, sums in observation order.  The tables are built as
// k_pose_prep builds them: T_ws = T_wp T_vs with the quaternion product renormalised, T_sw its inverse.
//   poses7 [P][7] (t, q xyzw), cam_params4 [C][4], cam_tvs7 [C][7], cam_model [C] (0 pinhole, 1 FOV; may be NULL),
//   cam_w [C] (may be NULL), pose_cam4 [P][4] per-pose intrinsics (may be NULL)
//   lm_ptr [L + 1] over the observations sorted by landmark; obs_pose, obs_cam, obs_z [O][2], obs_w0 [O]
//   x_w [L][4], ref_pose, ref_cam [L] (read with LM == 1); mask [L] (may be NULL: every landmark)
//   opts: linear_init, max_iterations, write_back, lambda0, gradient_tolerance, step_tolerance, min_parallax, huber_width
//   res [L][8] (status -1 in rows the mask leaves out), xw_out [L][4] as ba_hip_triangulate_landmarks fills x_w4,
//   final (may be NULL) [L][10]: lambda, then the unique entries of V (LM (LM + 1) / 2) and b_l (LM) at the end point
// Returns 0, 1 with the message of requests.h (triangulation_ok on the ids of the mask's complement is the caller's
// business: ids / n are checked here when ids is not NULL), -1 for LM other than 1 or 3.
template <int LM>
static void hostcheck_triangulate_lm(uint32_t C, const std::vector<bad::Rt>& tsw, const std::vector<bad::Rt>& tws,
                                     const double* cam_params4, const int32_t* cam_model, const double* cam_w,
                                     const double* pose_cam4, uint32_t L, const uint32_t* lm_ptr, const uint32_t* obs_pose,
                                     const uint32_t* obs_cam, const double* obs_z, const double* obs_w0, const double* x_w,
                                     const uint32_t* ref_pose, const uint32_t* ref_cam, const uint8_t* mask,
                                     const bae::TriOptions& opt, double* res, double* xw_out, double* final) {
  using namespace bae;
  using namespace bad;
  constexpr int N = TriSums<LM>::N, NL = TriSums<LM>::NL;
  for (uint32_t l = 0; l < L; ++l) {
    double* r = res + (size_t)l * kTriResult;
    for (int i = 0; i < 4; ++i) xw_out[(size_t)l * 4 + i] = x_w[(size_t)l * 4 + i];
    if (final) for (int i = 0; i < 10; ++i) final[(size_t)l * 10 + i] = 0.0;
    tri_result_none(r);
    if (mask && !mask[l]) { r[0] = -1.0; continue; }
    const uint32_t a0 = lm_ptr[l], a1 = lm_ptr[l + 1], k = a1 - a0;
    if (k == 0) continue;
    Rt t_sw_r{}, t_ws_r{};
    if (LM == 1) { t_sw_r = tsw[(size_t)ref_pose[l] * C + ref_cam[l]]; t_ws_r = tws[(size_t)ref_pose[l] * C + ref_cam[l]]; }
    std::vector<TriObs> obs(k);
    for (uint32_t a = a0; a < a1; ++a) {
      TriObs& o = obs[a - a0];
      const uint32_t pm = obs_pose[a], cm = obs_cam[a];
      const double* ip = pose_cam4 ? pose_cam4 + (size_t)pm * 4 : cam_params4 + (size_t)cm * 4;
      o.cam = {ip[0], ip[1], ip[2], ip[3], cam_w ? cam_w[cm] : 0.0, cam_model && cam_model[cm] ? 1 : 0};
      const Rt& t_sw_m = tsw[(size_t)pm * C + cm];
      o.T = LM == 1 ? compose(t_sw_m, t_ws_r) : t_sw_m;
      o.z[0] = obs_z[2 * (size_t)a]; o.z[1] = obs_z[2 * (size_t)a + 1];
      o.w0 = obs_w0[a];
    }
    double xv[3], rho;
    tri_held<LM>(x_w + (size_t)l * 4, t_sw_r, xv, &rho);
    V3 c0 = v3(0.0, 0.0, 0.0), d0 = v3(xv[0], xv[1], xv[2]);
    if (LM == 3) tri_centre_bearing(obs[0], &c0, &d0);
    double par = 0.0, base2 = 0.0;
    for (const TriObs& o : obs) {
      V3 c, d;
      tri_centre_bearing(o, &c, &d);
      par = tri_max(par, tri_angle(d0, d));
      base2 = tri_max(base2, tri_dist2(c0, c));
    }
    if (opt.linear_init) {
      double lin[NL] = {};
      for (const TriObs& o : obs) {
        double v[NL];
        tri_linear_terms<LM>(o, xv, v);
        for (int i = 0; i < NL; ++i) lin[i] += v[i];
      }
      tri_linear_solve<LM>(lin, xv, &rho);
    }
    auto sums_at = [&](const double* txv, double trho, bool guard, double* tot, double* depth) {
      for (int i = 0; i < N; ++i) tot[i] = 0.0;
      double dmin = tri_inf();
      for (const TriObs& o : obs) {
        double v[N];
        const double dep = tri_eval<LM>(o, txv, trho, opt.huber_width, guard, v);
        for (int i = 0; i < N; ++i) tot[i] += v[i];
        dmin = tri_min(dmin, dep);
      }
      if (depth) *depth = dmin;
    };
    TriLm<LM> m;
    double tot[N], depth;
    sums_at(xv, rho, false, tot, &depth);
    tri_begin<LM>(&m, opt, LM == 3 ? xv : &rho, tot, depth, par, base2, dot(c0, c0), k);
    while (m.active) {
      double txv[3], trho;
      tri_trial<LM>(m, xv, rho, txv, &trho);
      sums_at(txv, trho, true, tot, nullptr);
      tri_step<LM>(&m, opt, tot);
    }
    double fxv[3], frho = LM == 3 ? rho : m.x[0];
    for (int i = 0; i < 3; ++i) fxv[i] = LM == 3 ? m.x[i] : xv[i];
    double depth_end = m.depth;
    if (m.status == kTriOk || m.status == kTriNotConverged) {
      depth_end = tri_inf();
      for (const TriObs& o : obs) depth_end = tri_min(depth_end, tri_depth<LM>(o, fxv, frho));
    }
    tri_result<LM>(m, k, depth_end, r);
    if (tri_accepted<LM>(m, opt)) tri_world<LM>(fxv, frho, t_ws_r, xw_out + (size_t)l * 4);
    if (final) {
      final[(size_t)l * 10] = m.ds.lambda;
      for (int i = 0; i < N - 1; ++i) final[(size_t)l * 10 + 1 + i] = m.cur[i];
    }
  }
}

extern "C" int ba_hostcheck_triangulate(int LM, uint32_t P, const double* poses7, uint32_t C, const double* cam_params4,
                                        const double* cam_tvs7, const int32_t* cam_model, const double* cam_w,
                                        const double* pose_cam4, uint32_t L, const uint32_t* lm_ptr, const uint32_t* obs_pose,
                                        const uint32_t* obs_cam, const double* obs_z, const double* obs_w0, const double* x_w,
                                        const uint32_t* ref_pose, const uint32_t* ref_cam, const uint8_t* mask, uint32_t n_ids,
                                        const uint32_t* ids, const double* opts8, double* res, double* xw_out, double* final,
                                        char* msg, uint32_t cap) {
  using namespace bae;
  using namespace bad;
  if (LM != 1 && LM != 3) return -1;
  TriOptions opt;
  opt.linear_init = opts8[0] != 0.0; opt.max_iterations = (int)opts8[1]; opt.write_back = opts8[2] != 0.0;
  opt.lambda0 = opts8[3]; opt.gradient_tolerance = opts8[4]; opt.step_tolerance = opts8[5]; opt.min_parallax = opts8[6];
  opt.huber_width = opts8[7];
  const std::string bad_request =
      triangulation_ok({opt.max_iterations, opt.lambda0, opt.gradient_tolerance, opt.step_tolerance, opt.min_parallax,
                        opt.huber_width}, L, ids ? n_ids : L, ids);
  if (put_message(bad_request, msg, cap)) return 1;
  std::vector<Rt> tsw((size_t)P * C), tws((size_t)P * C);
  for (uint32_t p = 0; p < P; ++p)
    for (uint32_t c = 0; c < C; ++c) {
      const double* s = poses7 + (size_t)p * 7;
      const double* cm = cam_tvs7 + (size_t)c * 7;
      Rt wp;
      wp.R = quat_to_rot(s[3], s[4], s[5], s[6]);
      wp.t = v3(s[0], s[1], s[2]);
      double qv[4] = {cm[3], cm[4], cm[5], cm[6]}, qp[4] = {s[3], s[4], s[5], s[6]}, q[4];
      quat_mul(qp, qv, q);
      quat_normalize(q);
      Rt ws;
      ws.R = quat_to_rot(q[0], q[1], q[2], q[3]);
      ws.t = mul(wp.R, v3(cm[0], cm[1], cm[2])) + wp.t;
      tws[(size_t)p * C + c] = ws;
      tsw[(size_t)p * C + c] = inverse(ws);
    }
  std::vector<uint8_t> sel;
  if (ids) {
    sel.assign(L, 0);
    for (uint32_t i = 0; i < n_ids; ++i) sel[ids[i]] = 1;
    mask = sel.data();
  }
  if (LM == 1)
    hostcheck_triangulate_lm<1>(C, tsw, tws, cam_params4, cam_model, cam_w, pose_cam4, L, lm_ptr, obs_pose, obs_cam, obs_z, obs_w0,
                                x_w, ref_pose, ref_cam, mask, opt, res, xw_out, final);
  else
    hostcheck_triangulate_lm<3>(C, tsw, tws, cam_params4, cam_model, cam_w, pose_cam4, L, lm_ptr, obs_pose, obs_cam, obs_z, obs_w0,
                                x_w, ref_pose, ref_cam, mask, opt, res, xw_out, final);
  return 0;
}

// ---- pose refinement with the landmarks held fixed (resect.h) ----------------------------------------------------
#include "resect.h"

// build_pose_obs_lists: ptr [P + 1], idx [O].  Returns 0, or 1 when an observation names a pose >= P.
extern "C" int ba_hostcheck_pose_obs_lists(uint32_t P, uint32_t O, const uint32_t* obs_pose, uint32_t* ptr, uint32_t* idx) {
  std::vector<uint32_t> p, i;
  if (!bae::build_pose_obs_lists(P, O, obs_pose, &p, &i)) return 1;
  std::copy(p.begin(), p.end(), ptr);
  std::copy(i.begin(), i.end(), idx);
  return 0;
}

// guard_refine_poses on a lifecycle record after `events` (as ba_hostcheck_guard): flags bit 0 calibration, bit 1
// hooked, bit 2 in_solve, bit 3 sharded, bit 4 distributed solve
extern "C" int ba_hostcheck_refine_poses_guard(uint32_t n, const int32_t* events, int lm_dim, uint32_t flags, char* msg,
                                               uint32_t cap) {
  using namespace bae;
  Held h;
  for (uint32_t i = 0; i < n; ++i)
    if (!held_apply(h, events[i])) return -(int)(i + 1);
  GuardFacts f = {};
  f.hooked = (flags & 2) != 0; f.sharded = (flags & 8) != 0; f.dist_solve = (flags & 16) != 0;
  return put_message(guard_refine_poses(h, f, (flags & 1) != 0, lm_dim, (flags & 4) != 0), msg, cap);
}

// The rules of resect.h on the host, pose by pose, sums in list order.
//   poses7 [P][7] (t, q xyzw), cam_params4 [C][4], cam_tvs7 [C][7], cam_model [C] (may be NULL), cam_w [C] (may be
//   NULL), pose_cam4 [P][4] per-pose intrinsics (may be NULL)
//   the observations in the engine's sorted order: obs_pose, obs_cam, obs_lm [O], obs_z [O][2], obs_w0 [O]
//   x_w [L][4] world points; ids [n] (NULL: every pose, n = P)
//   opts7: max_iterations, write_back, fixed_mask, initial_damping, gradient_tolerance, step_tolerance, huber_width
//   res [n][8], t_out [n][7], info [n][36] as ba_hip_refine_poses fills them; final (may be NULL) [n][7]: lambda, g
// Returns 0, or 1 with the message of requests.h.
extern "C" int ba_hostcheck_refine_poses(uint32_t P, const double* poses7, uint32_t C, const double* cam_params4,
                                         const double* cam_tvs7, const int32_t* cam_model, const double* cam_w,
                                         const double* pose_cam4, uint32_t O, const uint32_t* obs_pose,
                                         const uint32_t* obs_cam, const uint32_t* obs_lm, const double* obs_z,
                                         const double* obs_w0, const double* x_w, uint32_t n, const uint32_t* ids,
                                         const double* opts7, double* res, double* t_out, double* info, double* final,
                                         char* msg, uint32_t cap) {
  using namespace bae;
  using namespace bad;
  RsOptions opt;
  opt.max_iterations = (int)opts7[0]; opt.write_back = opts7[1] != 0.0; opt.fixed_mask = (unsigned)opts7[2];
  opt.lambda0 = opts7[3]; opt.gradient_tolerance = opts7[4]; opt.step_tolerance = opts7[5]; opt.huber_width = opts7[6];
  const std::string bad_request =
      refinement_ok({opt.max_iterations, opt.fixed_mask, opt.lambda0, opt.gradient_tolerance, opt.step_tolerance,
                     opt.huber_width}, P, n, ids);
  if (put_message(bad_request, msg, cap)) return 1;
  std::vector<uint32_t> ptr, idx;
  if (!build_pose_obs_lists(P, O, obs_pose, &ptr, &idx)) return put_message("an observation names a pose that does not exist", msg, cap);
  std::vector<M3> R_sv(C);
  for (uint32_t c = 0; c < C; ++c) {
    const double* t = cam_tvs7 + (size_t)c * 7;
    Rt vs;
    vs.R = quat_to_rot(t[3], t[4], t[5], t[6]);
    vs.t = v3(t[0], t[1], t[2]);
    R_sv[c] = inverse(vs).R;
  }
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t p = ids ? ids[i] : i;
    const uint32_t a0 = ptr[p], k = ptr[p + 1] - a0;
    const double* held = poses7 + (size_t)p * 7;
    std::vector<uint8_t> use(k, 0);
    auto sums_at = [&](const double* pose7, bool first, double* tot, unsigned* used, double* depth) {
      for (int j = 0; j < kRsSums; ++j) tot[j] = 0.0;
      *used = 0;
      *depth = rs_inf();
      for (uint32_t j = 0; j < k; ++j) {
        const uint32_t a = idx[a0 + j], cm = obs_cam[a];
        Rt wp, sw;
        rs_sensor(pose7, cam_tvs7 + (size_t)cm * 7, &wp, &sw);
        const double* X = x_w + (size_t)obs_lm[a] * 4;
        if (first) use[j] = rs_usable(rs_point(sw, X)) ? 1 : 0;
        if (!use[j]) continue;
        const double* ip = pose_cam4 ? pose_cam4 + (size_t)p * 4 : cam_params4 + (size_t)cm * 4;
        const Cam cam = {ip[0], ip[1], ip[2], ip[3], cam_w ? cam_w[cm] : 0.0, cam_model && cam_model[cm] ? 1 : 0};
        double v[kRsSums];
        const double dep = rs_eval(cam, obs_z + 2 * (size_t)a, obs_w0[a], X, wp, sw, R_sv[cm], opt.huber_width, !first, v);
        for (int q = 0; q < kRsSums; ++q) tot[q] += v[q];
        *used += 1;
        *depth = dep < *depth ? dep : *depth;
      }
      rs_mask_sums(tot, opt.fixed_mask);
    };
    RsPose m;
    double tot[kRsSums], depth;
    unsigned used;
    sums_at(held, true, tot, &used, &depth);
    rs_begin(&m, opt, held, tot, used, k - used, depth);
    while (m.active) {
      double trial[7];
      rs_apply(m.x, m.delta, opt.fixed_mask, trial);
      sums_at(trial, false, tot, &used, &depth);
      rs_step(&m, opt, trial, tot, depth);
    }
    rs_result(m, res + (size_t)i * kRsResult);
    const bool acc = rs_accepted(m);
    for (int j = 0; j < 7; ++j) t_out[(size_t)i * 7 + j] = acc ? m.x[j] : held[j];
    rs_info(m, info + (size_t)i * 36);
    if (final) {
      final[(size_t)i * 7] = m.ds.lambda;
      for (int j = 0; j < 6; ++j) final[(size_t)i * 7 + 1 + j] = m.cur[kRsH + j];
    }
  }
  return 0;
}
