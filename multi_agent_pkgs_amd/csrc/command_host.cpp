// command_host.cpp — the host form of the commands for the vehicle (command_core.h): hdsm_command_host, the argument checks it shares
// with hdsm_command_batch, and the own atan2 / sincos on plain arrays. Pure host C++; the device form (command_kernels.hip) gives the
// same bits.
#include <cmath>

#include "../../include/hdsm_swarm.h"
#include "command_core.h"
#include "hdsm_internal.h"

static_assert(sizeof(hdsm_command) == 128, "hdsm_command is a 128-byte record");

extern "C" int hdsm_internal_command_args(int32_t n, int32_t n_hor, int32_t step_plan, double dt, int32_t yaw_idx, double k_p_yaw, const int32_t* n_ref,
                                          const double* ref_point, const double* state_before, const double* records, const int32_t* valid_in,
                                          const double* state_after, const double* yaw) {
  if (n < 0 || n_hor < 1 || n_hor > HDSM_MAX_HOR || step_plan < 1 || step_plan > n_hor) return HDSM_ERR_BAD_ARG;
  if (!std::isfinite(dt) || !(dt > 0)) return HDSM_ERR_BAD_ARG;
  if (n > 0 && (!n_ref || !ref_point || !state_before || !records || !valid_in || !state_after || !yaw)) return HDSM_ERR_BAD_ARG;
  if (!hdsm_cmd::settings_valid(yaw_idx, n_hor, k_p_yaw, yaw, n)) return HDSM_ERR_BAD_ARG;
  for (int k = 0; k < n; ++k)
    if (valid_in[k] < 0 || valid_in[k] > 2) return HDSM_ERR_BAD_ARG;
  return HDSM_OK;
}

extern "C" int hdsm_command_host(int32_t n, int32_t n_hor, int32_t step_plan, double dt, int32_t yaw_idx, double k_p_yaw, const int32_t* n_ref,
                                 const double* ref_point, const double* state_before, const double* records, const int32_t* valid_in,
                                 const double* state_after, double* yaw, hdsm_command* setpoint, hdsm_command* pose, int64_t stats[2]) {
  const int rc = hdsm_internal_command_args(n, n_hor, step_plan, dt, yaw_idx, k_p_yaw, n_ref, ref_point, state_before, records, valid_in,
                                            state_after, yaw);
  if (rc) return rc;
  for (int k = 0; k < n; ++k) {
    int stepped = 0;
    yaw[k] = hdsm_cmd::agent_round(yaw[k], n_ref[k] > yaw_idx, ref_point + (size_t)k * 3, state_before + (size_t)k * 9,
                                   records + (size_t)k * (size_t)(n_hor + 1) * 9, state_after + (size_t)k * 9, valid_in[k], step_plan, k_p_yaw, dt,
                                   setpoint ? setpoint + (size_t)k * step_plan : nullptr, pose ? pose + k : nullptr, &stepped);
    if (stats) stats[stepped ? 0 : 1] += 1;
  }
  return HDSM_OK;
}

extern "C" int hdsm_command_atan2(int32_t n, const double* y, const double* x, double* out) {
  if (n < 0 || (n > 0 && (!y || !x || !out))) return HDSM_ERR_BAD_ARG;
  for (int k = 0; k < n; ++k) out[k] = hdsm_cmd::atan2_own(y[k], x[k]);
  return HDSM_OK;
}

extern "C" int hdsm_command_sincos(int32_t n, const double* x, double* s, double* c) {
  if (n < 0 || (n > 0 && (!x || !s || !c))) return HDSM_ERR_BAD_ARG;
  for (int k = 0; k < n; ++k) hdsm_cmd::sincos_own(x[k], s + k, c + k);
  return HDSM_OK;
}
