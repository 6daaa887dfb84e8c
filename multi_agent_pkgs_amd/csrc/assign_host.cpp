// assign_host.cpp — the host form of the assignment (assign_core.h): hdsm_assign_host, the argument checks it shares with
// hdsm_assign_batch and hdsm_dswarm_assign, and the host mirror's hdsm_swarm_assign. Pure host C++; the device form
// (assign_kernels.hip) gives the same bits.
#include <cmath>
#include <cstdlib>
#include <vector>

#include "../../include/hdsm_swarm.h"
#include "assign_core.h"
#include "swarm_host.h"

namespace hdsm_assign {

int check_args(const hdsm_assign_setting* setting, int32_t n, int32_t n_groups, const int32_t* group_start, bool has_pos, const uint8_t* active,
               int32_t n_on, const double* slots, const int32_t* slot_of, Rule* rule, std::vector<int32_t>* gs, int* m_max) {
  const double quantum = setting ? setting->quantum : DEFAULT_QUANTUM;
  const long long max_iters = setting ? setting->max_iters : 0;
  if (n < 0 || n_groups < 0 || max_iters < 0 || !std::isfinite(quantum) || !(quantum > 0)) return HDSM_ERR_BAD_ARG;
  const double inv_q2 = 1.0 / (quantum * quantum);
  if (!std::isfinite(inv_q2) || !(inv_q2 > 0)) return HDSM_ERR_BAD_ARG;
  if (n > 0 && (!has_pos || !slots || !slot_of)) return HDSM_ERR_BAD_ARG;
  if (n_groups > 0 && group_start) {
    if (group_start[0] != 0 || group_start[n_groups] != n) return HDSM_ERR_BAD_ARG;
    for (int g = 0; g < n_groups; ++g)
      if (group_start[g + 1] <= group_start[g]) return HDSM_ERR_BAD_ARG;
    gs->assign(group_start, group_start + n_groups + 1);
  } else {
    gs->assign({0, n});
  }
  for (size_t e = 0; e < 3 * (size_t)n; ++e)
    if (!std::isfinite(slots[e])) return HDSM_ERR_BAD_ARG;
  *m_max = 0;
  for (size_t g = 0; g + 1 < gs->size(); ++g) {
    int m = 0;
    for (int k = (*gs)[g]; k < (*gs)[g + 1]; ++k) m += k < n_on && (!active || active[k] != 0);
    if (m > MAX_M) return HDSM_ERR_CAPACITY;
    *m_max = m > *m_max ? m : *m_max;
  }
  rule->inv_q2 = inv_q2, rule->max_iters = max_iters, rule->bid_limit = 1LL << BID_LIMIT_LOG2;
  if (const char* e = std::getenv("HDSM_ASSIGN_BID_LIMIT_LOG2")) {  // test hook: a lower limit (2^1 .. 2^52), for both forms alike
    const long v = std::strtol(e, nullptr, 10);
    if (v >= 1 && v <= BID_LIMIT_LOG2) rule->bid_limit = 1LL << v;
  }
  return HDSM_OK;
}

namespace {

// every group of the partition gs on the host: pos(k) is agent k's position
template <class Pos>
void solve_all(const Rule& rule, const std::vector<int32_t>& gs, Pos pos, const uint8_t* active, int32_t n_on, const double* slots, int32_t* slot_of,
               int64_t* price, hdsm_assign_stats* stats) {
  std::vector<int32_t> idx;
  for (size_t g = 0; g + 1 < gs.size(); ++g) {
    idx.clear();
    for (int k = gs[g]; k < gs[g + 1]; ++k) {
      if (k < n_on && (!active || active[k] != 0)) {
        idx.push_back(k);
      } else {
        slot_of[k] = -1;
        if (price) price[k] = 0;
      }
    }
    hdsm_assign_stats st{};
    solve_group(rule, (int)idx.size(), idx.data(), pos, slots, slot_of, price, &st);
    st.first = gs[g], st.count = gs[g + 1] - gs[g];
    if (stats) stats[g] = st;
  }
}

}  // namespace
}  // namespace hdsm_assign

extern "C" {

int hdsm_assign_host(const hdsm_assign_setting* setting, int32_t n, int32_t n_groups, const int32_t* group_start, const double* pos,
                     const uint8_t* active, const double* slots, int32_t* slot_of, int64_t* price, hdsm_assign_stats* stats) {
  using namespace hdsm_assign;
  Rule rule;
  std::vector<int32_t> gs;
  int m_max = 0;
  const int rc = check_args(setting, n, n_groups, group_start, pos != nullptr, active, n, slots, slot_of, &rule, &gs, &m_max);
  if (rc) return rc;
  solve_all(rule, gs, [pos](int k) { return pos + 3 * (size_t)k; }, active, n, slots, slot_of, price, stats);
  return HDSM_OK;
}

// The host mirror: the shard's agents on state_curr, in the shard's own groups; apply = 1 goes through hdsm_swarm_set_goals.
int hdsm_swarm_assign(void* swarm, const hdsm_assign_setting* setting, const double* slots, int32_t apply, int32_t* slot_of,
                      hdsm_assign_stats* stats) {
  using namespace hdsm_assign;
  hdsm_mirror::Swarm* sw = hdsm_mirror::as_swarm(swarm);
  if (!sw || (apply != 0 && apply != 1) || sw->n_local != sw->n_rob) return HDSM_ERR_BAD_ARG;  // (a group's agents must all be local)
  if (apply && sw->mission.on) return HDSM_ERR_BAD_ARG;                                       // (the goals are the mission's waypoints)
  const int n = sw->n_local;
  std::vector<int32_t> gs, own((size_t)n);
  Rule rule;
  int m_max = 0;
  const int rc = check_args(setting, n, sw->groups.n(), sw->groups.n() ? sw->groups.start.data() : nullptr, true, nullptr, n, slots, own.data(), &rule,
                            &gs, &m_max);
  if (rc) return rc;
  std::vector<hdsm_assign_stats> st(gs.size() - 1);
  solve_all(rule, gs, [sw](int k) { return sw->agents[(size_t)k].state_curr; }, nullptr, n, slots, own.data(), nullptr, st.data());
  if (apply) {
    std::vector<double> goals((size_t)n * 3);
    for (int k = 0; k < n; ++k)
      for (int c = 0; c < 3; ++c) goals[3 * (size_t)k + c] = own[(size_t)k] >= 0 ? slots[3 * (size_t)own[(size_t)k] + c] : sw->agents[(size_t)k].goal[c];
    if (const int rg = hdsm_swarm_set_goals(swarm, goals.data())) return rg;
  }
  if (slot_of) std::copy(own.begin(), own.end(), slot_of);
  if (stats) std::copy(st.begin(), st.end(), stats);
  return HDSM_OK;
}

}  // extern "C"
