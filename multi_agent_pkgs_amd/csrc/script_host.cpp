// script_host.cpp — the host form of a scripted agent's published record (script_core.h): hdsm_script_records_host and the argument
// checks it shares with hdsm_script_records_batch. Pure host C++; the device form (script_kernels.hip) gives the same bits.
#include <cmath>

#include "../../include/hdsm_swarm.h"
#include "hdsm_internal.h"
#include "script_core.h"

extern "C" int hdsm_internal_script_args(int32_t n_script, int32_t n_knots, const double* knots, int32_t n_hor, int32_t step_plan, double dt,
                                         int32_t predict, int64_t round, const double* records) {
  if (n_script < 0 || n_hor < 1 || n_hor > HDSM_MAX_HOR || step_plan < 1 || step_plan > n_hor) return HDSM_ERR_BAD_ARG;
  if (!std::isfinite(dt) || !(dt > 0) || (predict != 0 && predict != 1)) return HDSM_ERR_BAD_ARG;
  if (round < 0 || round > ((int64_t)1 << 40)) return HDSM_ERR_BAD_ARG;  // (round * step_plan + i stays far inside an int64 and a double)
  if (!hdsm_script::tracks_valid(n_script, n_knots, knots) || (n_script > 0 && !records)) return HDSM_ERR_BAD_ARG;
  return HDSM_OK;
}

extern "C" int hdsm_script_records_host(int32_t n_script, int32_t n_knots, const double* knots, int32_t n_hor, int32_t step_plan, double dt,
                                        int32_t predict, int64_t round, double* records) {
  const int rc = hdsm_internal_script_args(n_script, n_knots, knots, n_hor, step_plan, dt, predict, round, records);
  if (rc) return rc;
  for (int k = 0; k < n_script; ++k)
    for (int i = 0; i <= n_hor; ++i)
      hdsm_script::record_state(knots + (size_t)k * n_knots * 4, n_knots, step_plan, dt, predict, round, i,
                                records + ((size_t)k * (n_hor + 1) + i) * 9);
  return HDSM_OK;
}
