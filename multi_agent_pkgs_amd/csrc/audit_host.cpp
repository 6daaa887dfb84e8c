// audit_host.cpp — the host form of the flight audit (audit_core.h): hdsm_flight_audit_host, which the host mirror's
// hdsm_swarm_audit calls too. Pure host C++; the device form (audit_kernels.hip) gives the same bits.
#include "../../include/hdsm_swarm.h"
#include "audit_core.h"
#include "hdsm_internal.h"

extern "C" int hdsm_internal_audit_args(int32_t n_rob, const double* plans_all, const uint8_t* has_plan, int32_t n_hor, int32_t step_plan,
                                        int32_t first, int32_t n_local, double drone_radius, double drone_z_offset, const int8_t* world,
                                        const int32_t wdim[3], const double worigin[3], double voxel_size, const hdsm_audit_round* out) {
  if (n_rob < 0 || n_local < 0 || first < 0 || (int64_t)first + n_local > n_rob) return HDSM_ERR_BAD_ARG;
  if (!(drone_radius > 0) || !(drone_z_offset > 0) || step_plan < 1 || step_plan > n_hor || n_hor > HDSM_MAX_HOR) return HDSM_ERR_BAD_ARG;
  if ((n_rob && (!plans_all || !has_plan)) || (n_local && !out)) return HDSM_ERR_BAD_ARG;
  if (world && (!wdim || !worigin || !(voxel_size > 0) || wdim[0] < 1 || wdim[1] < 1 || wdim[2] < 1)) return HDSM_ERR_BAD_ARG;
  return HDSM_OK;
}

extern "C" int hdsm_flight_audit_host(int32_t n_rob, const double* plans_all, const uint8_t* has_plan, int32_t n_hor, int32_t step_plan,
                                      int32_t first, int32_t n_local, double drone_radius, double drone_z_offset, const int8_t* world,
                                      const int32_t wdim[3], const double worigin[3], double voxel_size, hdsm_audit_round* out) {
  return hdsm_internal_audit_host_grouped(n_rob, plans_all, has_plan, n_hor, step_plan, first, n_local, drone_radius, drone_z_offset, world, wdim,
                                          worigin, voxel_size, nullptr, out);
}

extern "C" int hdsm_internal_audit_host_grouped(int32_t n_rob, const double* plans_all, const uint8_t* has_plan, int32_t n_hor, int32_t step_plan,
                                                int32_t first, int32_t n_local, double drone_radius, double drone_z_offset, const int8_t* world,
                                                const int32_t wdim[3], const double worigin[3], double voxel_size, const int32_t* range,
                                                hdsm_audit_round* out) {
  const int rc = hdsm_internal_audit_args(n_rob, plans_all, has_plan, n_hor, step_plan, first, n_local, drone_radius, drone_z_offset, world,
                                          wdim, worigin, voxel_size, out);
  if (rc) return rc;
  const hdsm_audit::Weights w = hdsm_audit::weights(drone_radius, drone_z_offset);
  hdsm_audit::World wd{};
  wd.world = world;
  if (world)
    for (int k = 0; k < 3; ++k) wd.wdim[k] = wdim[k], wd.worigin[k] = worigin[k];
  wd.voxel_size = voxel_size;
  const size_t rec = (size_t)(n_hor + 1) * 9;
  for (int k = 0; k < n_local; ++k) {
    const int a = first + k;
    hdsm_audit::empty_round(&out[k]);
    if (!has_plan[a]) continue;
    const double* pa = plans_all + (size_t)a * rec;
    hdsm_audit::Best best = hdsm_audit::no_partner();
    const int b_lo = range ? range[2 * (size_t)a] : 0, b_hi = range ? range[2 * (size_t)a + 1] : n_rob;  // partners: the subject's group
    for (int s = 0; s < step_plan; ++s)
      for (int b = b_lo; b < b_hi; ++b) {
        if (b == a || !has_plan[b]) continue;
        const double* pb = plans_all + (size_t)b * rec;
        hdsm_audit::take(best, hdsm_audit::pair_q(w, pa + 9 * s, pa + 9 * (s + 1), pb + 9 * s, pb + 9 * (s + 1)), s, b);
      }
    out[k].sep2 = best.q, out[k].partner = best.partner, out[k].substep = best.substep;
    hdsm_audit::track(wd, pa, 9, step_plan, pa + 9 * (size_t)step_plan + 3, &out[k]);
  }
  return HDSM_OK;
}
