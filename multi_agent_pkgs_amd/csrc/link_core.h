// link_core.h — stale plans: the step shift of a neighbour's record and the per-sender link model of the device loop, as plain
// functions that compile for the host form (hdsm_link_deliver_host, link_host.cpp) AND for the device (k_plan_prepass, k_ref_pack,
// k_reference, k_tasc_planes, k_deliver). One source: integers and copies only, so the two forms agree bit for bit.
//
// Shift. With shift s >= 0 every instance but k's own reads record k as R'[i] = R[min(i + s, N)], i = 0..N: the plan advanced by s
// steps with its last state (v = a = 0) held. shifted_step is that index; values above N behave as N, negative ones as 0.
//
// Links. fate[n_rounds][n_rob], read cyclically: entry (q mod n_rounds, k) is the fate of the record agent k publishes in link
// round q — < 0 lost for everyone, d in 0..MAX_DELAY: it arrives d rounds late. The model is PER SENDER: every receiver, on every
// rank, sees the same thing (its limit: a link that fails for one receiver only cannot be expressed). A slot behind the table
// (k >= n_rob: the padded tail of a sharded exchange) is delivered on time. In link round r the slot's view takes the NEWEST
// record that has arrived and is newer than the one it holds (arrival): an older record that arrives after a newer one is ignored.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/hdsm_swarm.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define HDSM_LINK_HD __host__ __device__ inline
#else
#define HDSM_LINK_HD inline
#endif

namespace hdsm_link {

constexpr int MAX_DELAY = HDSM_LINK_MAX_DELAY;
constexpr int COUNTERS = 4;  // per slot: [0] records delivered, [1] broadcasts lost, [2] largest age reached (rounds), [3] link rounds

HDSM_LINK_HD int shifted_step(int st, int s, int N) {
  const int t = st + (s > 0 ? (s < N ? s : N) : 0);
  return t < N ? t : N;
}

HDSM_LINK_HD int fate_of(const int8_t* fate, int n_rounds, int n_rob, int q, int k) {
  return k < n_rob ? (int)fate[(size_t)(q % n_rounds) * (size_t)n_rob + (size_t)k] : 0;
}

// The link round whose record slot k's view takes in link round r (D: the largest delay of the table; seen_round: the round of the
// record it holds, -1 = the view of before the links), or -1: nothing new has arrived.
HDSM_LINK_HD int arrival(const int8_t* fate, int n_rounds, int n_rob, int D, int k, int r, int seen_round) {
  const int dmax = D < r ? D : r;
  for (int d = 0; d <= dmax; ++d) {  // newest first
    const int q = r - d;
    if (q <= seen_round) break;
    const int f = fate_of(fate, n_rounds, n_rob, q, k);
    if (f >= 0 && f <= d) return q;
  }
  return -1;
}

// The shift the NEXT round's launches read slot k with: its record is r - seen_round rounds older than a fresh one, and a round
// flies step_plan steps. time_aware off: the reference's behaviour, a stale plan used as it is.
HDSM_LINK_HD int shift_of(int time_aware, int r, int seen_round, int step_plan, int N) {
  if (!time_aware) return 0;
  const long long s = (long long)(r - seen_round) * (long long)step_plan;
  return s < (long long)N ? (int)s : N;
}

// The counters of slot k after link round r (seen_round: after the delivery of the round; delivered: something arrived).
HDSM_LINK_HD void count_round(int32_t* cnt, bool delivered, bool lost, int r, int seen_round) {
  cnt[0] += delivered ? 1 : 0, cnt[1] += lost ? 1 : 0;
  const int age = r - seen_round;
  cnt[2] = age > cnt[2] ? age : cnt[2];
  cnt[3] += 1;
}

// One link round over G slots of rec = (N + 1) * 9 doubles: the records published in it (truth), the ring of the last D + 1 rounds
// ([D + 1][G][rec], round q at q mod (D + 1)) and the view (seen, seen_has, seen_round, shift, cnt [G][COUNTERS]).
struct Round {
  int32_t G, n_rob, N, step_plan, n_rounds, D, time_aware, r;
  const int8_t* fate;
  const double* truth;
  double* ring;
  double* seen;
  uint8_t* seen_has;
  int32_t* seen_round;
  int32_t* shift;
  int32_t* cnt;
};

// Slot k of the round, by `lanes` cooperating lanes of which this is `lane` (a wavefront of k_deliver, or 1 on the host): the
// slot's record goes into the ring; the newest arrival, if any, into the view. Every lane takes the same decision from the same
// loads (seen_round[k] is read by all of them before lane 0 stores it: one wavefront, program order); lane 0 writes the scalars.
HDSM_LINK_HD void deliver_slot(const Round& a, int k, int lane, int lanes) {
  const size_t rec = (size_t)(a.N + 1) * 9, G = (size_t)a.G;
  const int ring_n = a.D + 1, held = a.seen_round[k];
  const int q = arrival(a.fate, a.n_rounds, a.n_rob, a.D, k, a.r, held);
  const double* tr = a.truth + (size_t)k * rec;
  double* rg = a.ring + ((size_t)(a.r % ring_n) * G + (size_t)k) * rec;
  // (q < r: a round of the ring other than this one's, r - q <= D; q == r: the record in hand)
  const double* src = (q >= 0 && q != a.r) ? a.ring + ((size_t)(q % ring_n) * G + (size_t)k) * rec : tr;
  double* sn = a.seen + (size_t)k * rec;
  const double first = src[0];
  for (size_t e = (size_t)lane; e < rec; e += (size_t)lanes) {
    const double v = tr[e];
    rg[e] = v;
    if (q >= 0) sn[e] = (q == a.r) ? v : src[e];
  }
  if (lane != 0) return;
  const int now = q >= 0 ? q : held;
  if (q >= 0) a.seen_has[k] = first == first ? 1 : 0, a.seen_round[k] = q;  // (a record without a plan carries a NaN in front)
  a.shift[k] = shift_of(a.time_aware, a.r, now, a.step_plan, a.N);
  count_round(a.cnt + (size_t)k * COUNTERS, q >= 0, fate_of(a.fate, a.n_rounds, a.n_rob, a.r, k) < 0, a.r, now);
}

// The largest delay of a table (its lost entries aside), or -1 when an entry is above MAX_DELAY.
inline int table_max_delay(int n_rounds, int n_rob, const int8_t* fate) {
  int D = 0;
  for (size_t e = 0; e < (size_t)n_rounds * (size_t)n_rob; ++e) {
    if (fate[e] > MAX_DELAY) return -1;
    D = fate[e] > D ? fate[e] : D;
  }
  return D;
}

// hdsm_link_deliver_host (include/hdsm_swarm.h): the argument checks and the round, slot by slot. Returns an hdsm_error.
inline int deliver_round_host(const Round& a) {
  if (a.G < 0 || a.n_rob < 0 || a.N < 1 || a.N > HDSM_MAX_HOR || a.step_plan < 0 || a.n_rounds < 1 || a.D < 0 || a.D > MAX_DELAY || a.r < 0)
    return HDSM_ERR_BAD_ARG;
  if (!a.fate || !a.truth || !a.ring || !a.seen || !a.seen_has || !a.seen_round || !a.shift || !a.cnt) return HDSM_ERR_BAD_ARG;
  const int tmax = table_max_delay(a.n_rounds, a.n_rob, a.fate);
  if (tmax < 0 || tmax > a.D) return HDSM_ERR_BAD_ARG;  // (a record later than the ring is long could never be delivered)
  for (int k = 0; k < a.G; ++k)
    if (a.seen_round[k] >= a.r) return HDSM_ERR_BAD_ARG;  // (a view cannot hold a record of this round or a later one)
  for (int k = 0; k < a.G; ++k) deliver_slot(a, k, 0, 1);
  return HDSM_OK;
}

}  // namespace hdsm_link
