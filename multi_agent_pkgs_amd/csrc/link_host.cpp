// link_host.cpp — the host form of the per-sender link model (link_core.h): hdsm_link_deliver_host (include/hdsm_swarm.h). Pure host C++.
#include "../../include/hdsm_swarm.h"
#include "link_core.h"

// One link round of the device loop's per-sender link model on host arrays: the source k_deliver runs (link_core.h).
extern "C" int hdsm_link_deliver_host(int32_t n_slots, int32_t n_rob, int32_t n_hor, int32_t step_plan, int32_t n_rounds, const int8_t* fate,
                                      int32_t max_delay, int32_t time_aware, int32_t link_round, const double* truth, double* ring, double* seen,
                                      uint8_t* seen_has, int32_t* seen_round, int32_t* shift, int32_t* counters) {
  const hdsm_link::Round a{n_slots, n_rob, n_hor, step_plan, n_rounds, max_delay, time_aware, link_round, fate, truth,
                           ring,    seen,  seen_has, seen_round, shift,  counters};
  return hdsm_link::deliver_round_host(a);
}
