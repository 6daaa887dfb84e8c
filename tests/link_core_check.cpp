// link_core_check.cpp — csrc/link_core.h on the host: the step shift and one flight's worth of link rounds through
// hdsm_link::deliver_round_host (what hdsm_link_deliver_host calls), with every array allocated at exactly its size so that the
// address sanitizer sees the first byte read or written outside it. Stand-alone; built with the address and undefined-behaviour
// sanitizers by tests/test_links.py. The expected view is kept by a second, history-based rule written here (no ring).
// Every property is an assertion of this program (CHECK). Exit status 0 = all held.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../multi_agent_pkgs_amd/csrc/link_core.h"

static int g_failed = 0;
#define CHECK(cond)                                                         \
  do {                                                                      \
    if (!(cond)) std::printf("line %d: %s\n", __LINE__, #cond), ++g_failed; \
  } while (0)

static unsigned g_seed = 12345u;
static unsigned rnd() { return g_seed = g_seed * 1664525u + 1013904223u, g_seed >> 8; }

// one flight: `rounds` link rounds of n_slots slots (the last n_slots - n_rob are padding) under the table `fate`
static void fly(int n_slots, int n_rob, int N, int step_plan, int n_rounds, const std::vector<int8_t>& fate, int time_aware, int rounds) {
  const size_t rec = (size_t)(N + 1) * 9, G = (size_t)n_slots;
  const int D = hdsm_link::table_max_delay(n_rounds, n_rob, fate.data());
  CHECK(D >= 0 && D <= hdsm_link::MAX_DELAY);
  std::vector<double> ring((size_t)(D + 1) * G * rec, 0.0), seen(G * rec), truth(G * rec);
  std::vector<uint8_t> seen_has(G, 1);
  std::vector<int32_t> seen_round(G, -1), shift(G, 0), cnt(G * hdsm_link::COUNTERS, 0);
  std::vector<std::vector<double>> history;
  for (size_t e = 0; e < G * rec; ++e) seen[e] = -1.0 - (double)e;
  std::vector<double> want(seen);
  std::vector<int32_t> want_round(G, -1);
  std::vector<uint8_t> want_has(G, 1);
  long delivered = 0, lost = 0;
  for (int r = 0; r < rounds; ++r) {
    for (size_t k = 0; k < G; ++k) {
      for (size_t e = 0; e < rec; ++e) truth[k * rec + e] = (double)r * 1000.0 + (double)k + (double)e * 1e-3;
      if (rnd() % 5 == 0) truth[k * rec] = std::numeric_limits<double>::quiet_NaN();  // an agent without a plan
    }
    history.push_back(truth);
    const hdsm_link::Round a{n_slots, n_rob, N, step_plan, n_rounds, D, time_aware, r, fate.data(), truth.data(), ring.data(), seen.data(),
                             seen_has.data(), seen_round.data(), shift.data(), cnt.data()};
    CHECK(hdsm_link::deliver_round_host(a) == HDSM_OK);
    for (int k = 0; k < n_slots; ++k) {
      int best = -1;
      for (int q = r > D ? r - D : 0; q <= r; ++q) {
        const int f = k < n_rob ? fate[(size_t)(q % n_rounds) * n_rob + k] : 0;
        if (f >= 0 && q + f <= r && q > want_round[k]) best = q;
      }
      if (best >= 0) {
        std::memcpy(&want[(size_t)k * rec], &history[best][(size_t)k * rec], rec * 8);
        want_round[k] = best, want_has[k] = std::isnan(history[best][(size_t)k * rec]) ? 0 : 1, ++delivered;
      }
      lost += k < n_rob && fate[(size_t)(r % n_rounds) * n_rob + k] < 0;
      const long age = r - want_round[k];
      CHECK(seen_round[k] == want_round[k] && seen_has[k] == want_has[k]);
      CHECK(shift[k] == (time_aware ? (int)(age * step_plan < N ? age * step_plan : N) : 0));
      CHECK(cnt[(size_t)k * 4 + 3] == r + 1 && cnt[(size_t)k * 4 + 2] >= age);
    }
    CHECK(std::memcmp(seen.data(), want.data(), G * rec * 8) == 0);
  }
  long got_delivered = 0, got_lost = 0;
  for (int k = 0; k < n_slots; ++k) got_delivered += cnt[(size_t)k * 4], got_lost += cnt[(size_t)k * 4 + 1];
  CHECK(got_delivered == delivered && got_lost == lost);
}

int main() {
  using hdsm_link::shifted_step;
  for (int N = 1; N <= HDSM_MAX_HOR; ++N)
    for (int s = -2; s <= N + 3; ++s)
      for (int st = 0; st <= N; ++st) {
        const int eff = s < 0 ? 0 : (s > N ? N : s);
        CHECK(shifted_step(st, s, N) == (st + eff < N ? st + eff : N));
      }
  CHECK(shifted_step(3, 2147483647, 10) == 10 && shifted_step(10, 2147483647, 10) == 10);  // (no overflow: the shift is clamped first)
  CHECK(hdsm_link::shift_of(1, 2147483000, -1, 16, 10) == 10 && hdsm_link::shift_of(0, 5, -1, 3, 10) == 0);

  // argument checks: nothing is touched on a bad argument
  {
    std::vector<int8_t> fate(4, 0);
    std::vector<double> one(18, 0.0), ring(18, 0.0);
    uint8_t has = 0;
    int32_t sr = -1, sh = 0, cnt[4] = {0, 0, 0, 0};
    hdsm_link::Round a{1, 1, 1, 1, 4, 0, 1, 0, fate.data(), one.data(), ring.data(), one.data(), &has, &sr, &sh, cnt};
    CHECK(hdsm_link::deliver_round_host(a) == HDSM_OK && sr == 0 && cnt[3] == 1);
    hdsm_link::Round b = a;
    b.r = 0;  // the view already holds round 0
    CHECK(hdsm_link::deliver_round_host(b) == HDSM_ERR_BAD_ARG);
    b = a, b.r = 1, b.n_rounds = 0;
    CHECK(hdsm_link::deliver_round_host(b) == HDSM_ERR_BAD_ARG);
    b = a, b.r = 1, b.fate = nullptr;
    CHECK(hdsm_link::deliver_round_host(b) == HDSM_ERR_BAD_ARG);
    b = a, b.r = 1, b.D = hdsm_link::MAX_DELAY + 1;
    CHECK(hdsm_link::deliver_round_host(b) == HDSM_ERR_BAD_ARG);
    fate[2] = 3;  // a delay the ring (D = 0) is too short for
    b = a, b.r = 1;
    CHECK(hdsm_link::deliver_round_host(b) == HDSM_ERR_BAD_ARG && sr == 0 && cnt[3] == 1);
    fate[2] = 8;
    CHECK(hdsm_link::table_max_delay(4, 1, fate.data()) == -1);
  }

  // crafted tables
  {
    std::vector<int8_t> ooo(6 * 3, 0);  // out of order: agent 0's record of round 0 is 3 late, that of round 1 on time
    ooo[0] = 3;
    fly(4, 3, 10, 1, 6, ooo, 1, 13);
    std::vector<int8_t> dark(14 * 3, 1);  // latency 1, agent 2 dark for nine rounds: longer than the ring of two
    for (int q = 2; q <= 10; ++q) dark[(size_t)q * 3 + 2] = -1;
    fly(3, 3, 15, 3, 14, dark, 1, 30);
    fly(3, 3, 15, 3, 14, dark, 0, 30);
    fly(5, 4, 7, 2, 3, std::vector<int8_t>(3 * 4, -1), 1, 8);  // every entry lost
    fly(2, 2, 16, 1, 1, std::vector<int8_t>{-1, 1}, 1, 6);     // n_rounds = 1
    std::vector<int8_t> late(9 * 2, 0);                        // delay 7
    for (int q = 0; q < 9; ++q) late[(size_t)q * 2] = 7;
    fly(2, 2, 10, 1, 9, late, 1, 25);
    fly(1, 1, 1, 0, 1, std::vector<int8_t>{0}, 1, 3);          // the smallest of everything
  }
  // random tables
  for (int t = 0; t < 60; ++t) {
    const int n_rob = 1 + (int)(rnd() % 9), pad = (int)(rnd() % 3), n_rounds = 1 + (int)(rnd() % 12), N = 1 + (int)(rnd() % HDSM_MAX_HOR);
    const int dmax = (int)(rnd() % (hdsm_link::MAX_DELAY + 1));
    std::vector<int8_t> fate((size_t)n_rounds * n_rob);
    for (int8_t& f : fate) f = rnd() % 4 == 0 ? (int8_t)-1 : (int8_t)(rnd() % (unsigned)(dmax + 1));
    fly(n_rob + pad, n_rob, N, 1 + (int)(rnd() % 3), n_rounds, fate, (int)(rnd() % 2), 3 * n_rounds + 5);
  }
  std::printf(g_failed ? "%d check(s) failed\n" : "link_core: all checks held\n", g_failed);
  return g_failed ? 1 : 0;
}
