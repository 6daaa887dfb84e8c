// assign_core.h — formations: which agent takes which slot. An exact linear assignment of the active agents of a neighbour group to the
// slots at the same indices, minimising the sum of the quantised squared distances, by the forward auction in Jacobi form with
// eps-scaling, on integers. One source for the host form (assign_host.cpp: hdsm_assign_host, the host mirror) and the device kernel
// (assign_kernels.hip: k_assign); the rule is written out in include/hdsm_swarm.h ("formations") and the order of the statements here IS
// its definition. The cost is the only floating-point arithmetic: the same IEEE operations in the same order on both sides (contraction
// off, products first, sums left to right), then one truncation. Everything behind it is int64 and independent of the order in which the
// bidders of an iteration are served, so a workgroup may serve them in any order and in parallel.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/hdsm_swarm.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define ASSIGN_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define ASSIGN_HD inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

static_assert(sizeof(hdsm_assign_setting) == 16, "hdsm_assign_setting is 16 bytes");
static_assert(sizeof(hdsm_assign_stats) == 48, "hdsm_assign_stats is 48 bytes");

namespace hdsm_assign {

constexpr int MAX_M = HDSM_ASSIGN_MAX;
constexpr long long COST_CAP = 1LL << 34;        // the largest cost: a squared distance of 2^34 quanta and beyond
constexpr int BID_LIMIT_LOG2 = 52;               // a bid of 2^52 ends the group with status 3: (bid << 10 | bidder) stays a 64-bit key
constexpr long long NONE = -(1LL << 62);         // below every value a_ij - p_j (|a| < 2^45, 0 <= p < 2^52)
constexpr double DEFAULT_QUANTUM = 0.01;
// the default budget of iterations for a group of m bidders, four times the largest count the host form recorded over
// tests/assign_cases.py and the two capacity cases (profiles/assign_iterations.json): 240 m + 256
constexpr long long BUDGET_A = 240, BUDGET_B = 256;

enum Status { OPTIMAL = 0, BUDGET = 1, NOT_FINITE = 2, BID_OVERFLOW = 3 };

// what a launch carries of the setting: 1 / quantum^2, the budget as given (0: the default) and the bid limit (2^52; a test hook of
// the host side, HDSM_ASSIGN_BID_LIMIT_LOG2, lowers it for both forms alike so that status 3 can be reached at all)
struct Rule {
  double inv_q2;
  long long max_iters, bid_limit;
};

ASSIGN_HD bool finite3(const double* p) { return p[0] - p[0] == 0.0 && p[1] - p[1] == 0.0 && p[2] - p[2] == 0.0; }

// the cost of the agent at (px, py, pz) taking the slot at (sx, sy, sz): the squared distance in quanta, truncated, capped
ASSIGN_HD long long cost(double px, double py, double pz, double sx, double sy, double sz, double inv_q2) {
  const double dx = px - sx, dy = py - sy, dz = pz - sz;
  const double d2 = (dx * dx + dy * dy) + dz * dz;
  const double t = d2 * inv_q2;
  return t >= 17179869184.0 ? COST_CAP : (long long)t;
}

ASSIGN_HD long long budget(long long max_iters, int m) { return max_iters > 0 ? max_iters : BUDGET_A * m + BUDGET_B; }
ASSIGN_HD long long eps_first(long long cmax, int m) {
  const long long e = cmax * (m + 1) / 2;
  return e > 1 ? e : 1;
}
ASSIGN_HD long long eps_next(long long eps) { return eps / 4 > 1 ? eps / 4 : 1; }

// a bidder's scan of the objects: the best value, the lowest object that has it, and the best value over the other objects
struct Scan {
  long long best, second;
  int j;
};
ASSIGN_HD Scan scan_identity() { return Scan{NONE, NONE, 0x7fffffff}; }
// object j (visited in increasing order within one scan) with the value v
ASSIGN_HD void scan_add(Scan& s, long long v, int j) {
  if (v > s.best) s.second = s.best, s.best = v, s.j = j;
  else if (v > s.second) s.second = v;
}
// two scans over disjoint sets of objects
ASSIGN_HD Scan scan_join(const Scan& a, const Scan& b) {
  const bool first = a.best > b.best || (a.best == b.best && a.j < b.j);
  const Scan &w = first ? a : b, &l = first ? b : a;
  return Scan{w.best, w.second > l.best ? w.second : l.best, w.j};
}
// the bid of a bidder with that scan for its object at price p, in a problem of m objects
ASSIGN_HD long long bid_of(const Scan& s, long long p, long long eps, int m) { return p + (s.best - (m == 1 ? s.best : s.second)) + eps; }
// a bid and its bidder as one key: the largest key on an object is the highest bid, of the lowest bidder among equals
ASSIGN_HD unsigned long long key_of(long long bid, int bidder) { return ((unsigned long long)bid << 10) | (unsigned long long)(MAX_M - 1 - bidder); }
ASSIGN_HD long long key_bid(unsigned long long k) { return (long long)(k >> 10); }
ASSIGN_HD int key_bidder(unsigned long long k) { return MAX_M - 1 - (int)(k & (MAX_M - 1)); }

// (assign_host.cpp) the argument checks every entry point shares, before anything is touched: the rule of the setting (NULL: the
// defaults), the partition as a table gs of n_groups + 1 entries (one group without one) and the largest number of active agents of a
// group; agent k is active when k < n_on and (active == NULL or active[k] != 0). HDSM_ERR_BAD_ARG / HDSM_ERR_CAPACITY as hdsm_swarm.h says.
__attribute__((visibility("hidden"))) int check_args(const hdsm_assign_setting* setting, int32_t n, int32_t n_groups, const int32_t* group_start,
                                                     bool has_pos, const uint8_t* active, int32_t n_on, const double* slots, const int32_t* slot_of,
                                                     Rule* rule, std::vector<int32_t>* gs, int* m_max);

// The host form of one group. idx [m]: the active agents of the group (ascending); bidder i is agent idx[i], object j is slot idx[j].
// pos(a) -> const double* of agent a's position; slots [n][3]. Writes slot_of / price of the active agents and *st (first and count
// are the caller's). Nothing here depends on the order in which the unassigned bidders are visited.
template <class Pos>
void solve_group(const Rule& rule, int m, const int32_t* idx, Pos pos, const double* slots, int32_t* slot_of, int64_t* price, hdsm_assign_stats* st) {
  st->active = m, st->status = OPTIMAL, st->phases = 0, st->reserved0 = 0, st->iters = st->bids = st->cost = 0;
  if (m == 0) return;
  int status = OPTIMAL;
  std::vector<long long> p((size_t)m, 0);
  std::vector<int> owner((size_t)m, -1), has((size_t)m, -1), list, next;
  std::vector<unsigned long long> key((size_t)m, 0);
  std::vector<double> P((size_t)m * 3), S((size_t)m * 3);
  for (int i = 0; i < m; ++i) {
    const double* a = pos(idx[i]);
    if (!finite3(a)) status = NOT_FINITE;
    for (int c = 0; c < 3; ++c) P[3 * (size_t)i + c] = a[c], S[3 * (size_t)i + c] = slots[3 * (size_t)idx[i] + c];
  }
  const long long M1 = m + 1;
  auto c_ij = [&](int i, int j) { return cost(P[3 * (size_t)i], P[3 * (size_t)i + 1], P[3 * (size_t)i + 2], S[3 * (size_t)j], S[3 * (size_t)j + 1], S[3 * (size_t)j + 2], rule.inv_q2); };
  if (status == OPTIMAL) {
    long long cmax = 0;
    for (int i = 0; i < m; ++i)
      for (int j = 0; j < m; ++j) {
        const long long c = c_ij(i, j);
        cmax = c > cmax ? c : cmax;
      }
    const long long max_iters = budget(rule.max_iters, m);
    for (long long eps = eps_first(cmax, m); status == OPTIMAL; eps = eps_next(eps)) {
      std::fill(owner.begin(), owner.end(), -1), std::fill(has.begin(), has.end(), -1);
      list.resize((size_t)m);
      for (int i = 0; i < m; ++i) list[(size_t)i] = i;
      while (!list.empty() && status == OPTIMAL) {
        if (st->iters == max_iters) {
          status = BUDGET;
          break;
        }
        st->iters += 1, st->bids += (long long)list.size();
        for (int i : list) {  // every bid of the iteration on the prices of its start
          Scan s = scan_identity();
          for (int j = 0; j < m; ++j) scan_add(s, -c_ij(i, j) * M1 - p[(size_t)j], j);
          const long long bid = bid_of(s, p[(size_t)s.j], eps, m);
          if (bid >= rule.bid_limit) status = BID_OVERFLOW;
          else {
            const unsigned long long k = key_of(bid, i);
            key[(size_t)s.j] = k > key[(size_t)s.j] ? k : key[(size_t)s.j];
          }
        }
        if (status != OPTIMAL) break;
        for (int j = 0; j < m; ++j) {  // the awards
          const unsigned long long k = key[(size_t)j];
          if (!k) continue;
          const int i = key_bidder(k);
          if (owner[(size_t)j] >= 0) has[(size_t)owner[(size_t)j]] = -1;
          owner[(size_t)j] = i, has[(size_t)i] = j, p[(size_t)j] = key_bid(k), key[(size_t)j] = 0;
        }
        next.clear();
        for (int i = 0; i < m; ++i)
          if (has[(size_t)i] < 0) next.push_back(i);
        list.swap(next);
      }
      if (status != OPTIMAL) break;
      st->phases += 1;
      if (eps == 1) break;
    }
  }
  st->status = status;
  for (int i = 0; i < m; ++i) {
    const int j = status == OPTIMAL ? has[(size_t)i] : i;
    slot_of[idx[i]] = idx[j];
    if (price) price[idx[i]] = status == OPTIMAL ? p[(size_t)i] : 0;
    if (status == OPTIMAL) st->cost += c_ij(i, j);
  }
}

}  // namespace hdsm_assign
