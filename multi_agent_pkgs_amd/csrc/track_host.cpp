// track_host.cpp — the host form of imperfect tracking (track_core.h): hdsm_track_states_host and the argument checks it shares with
// hdsm_track_states_batch. Pure host C++; the device form (track_kernels.hip) gives the same bits.
#include <cmath>

#include "../../include/hdsm_swarm.h"
#include "hdsm_internal.h"
#include "track_core.h"

extern "C" int hdsm_internal_track_args(const hdsm_tracking* m, int32_t n, const int32_t* agent_id, const double* planned, double T, int64_t round,
                                        const double* flown) {
  if (!hdsm_track::model_valid(m) || n < 0 || (n > 0 && (!agent_id || !planned || !flown))) return HDSM_ERR_BAD_ARG;
  if (!std::isfinite(T) || !(T > 0)) return HDSM_ERR_BAD_ARG;
  if (round < 0 || round > hdsm_track::MAX_ROUND) return HDSM_ERR_BAD_ARG;
  return HDSM_OK;
}

extern "C" int hdsm_track_states_host(const hdsm_tracking* m, int32_t n, const int32_t* agent_id, const double* planned, double T, int64_t round,
                                      double* flown, double* dist) {
  const int rc = hdsm_internal_track_args(m, n, agent_id, planned, T, round, flown);
  if (rc) return rc;
  for (int k = 0; k < n; ++k) {
    const double* from = planned + (size_t)k * 9;
    double* to = flown + (size_t)k * 9;
    double x[9], s[9];  // (planned and flown may be the same array)
    for (int c = 0; c < 9; ++c) x[c] = from[c];
    hdsm_track::flown_state(*m, agent_id[k], round, T, x, s);
    for (int c = 0; c < 9; ++c) to[c] = s[c];
    if (dist) dist[k] = hdsm_track::pos_dist(x, s);
  }
  return HDSM_OK;
}
