// script_core_check.cpp — csrc/script_core.h on the host with every array allocated at exactly its size, so that the address
// sanitizer sees the first byte read outside a track or written outside a record. Stand-alone; built with the address and
// undefined-behaviour sanitizers by tests/test_script.py. The expected state comes from a linear scan written here (the header
// searches by bisection). Every property is an assertion of this program (CHECK). Exit status 0 = all held.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../multi_agent_pkgs_amd/csrc/script_core.h"

static int g_failed = 0;
#define CHECK(cond)                                                         \
  do {                                                                      \
    if (!(cond)) std::printf("line %d: %s\n", __LINE__, #cond), ++g_failed; \
  } while (0)

static unsigned g_seed = 2468u;
static double uni() { return g_seed = g_seed * 1664525u + 1013904223u, (double)(g_seed >> 8) / (double)(1u << 24); }

static void scan_state(const std::vector<double>& k, int n, double tau, double* s) {
  for (int c = 0; c < 9; ++c) s[c] = 0.0;
  if (tau <= k[0]) {
    for (int c = 0; c < 3; ++c) s[c] = k[1 + c];
    return;
  }
  if (tau >= k[4 * (size_t)(n - 1)]) {
    for (int c = 0; c < 3; ++c) s[c] = k[4 * (size_t)(n - 1) + 1 + c];
    return;
  }
  int j = 0;
  while (!(k[4 * (size_t)j] <= tau && tau < k[4 * (size_t)(j + 1)])) ++j;
  for (int c = 0; c < 3; ++c) {
    const double w = (k[4 * (size_t)(j + 1) + 1 + c] - k[4 * (size_t)j + 1 + c]) / (k[4 * (size_t)(j + 1)] - k[4 * (size_t)j]);
    s[c] = k[4 * (size_t)j + 1 + c] + (tau - k[4 * (size_t)j]) * w;
    s[3 + c] = w;
  }
}

static void one_track(int n) {
  std::vector<double> k((size_t)n * 4);
  double t = -1.0 + uni();
  for (int j = 0; j < n; ++j) {
    t += 0.01 + uni();
    k[4 * (size_t)j] = t;
    for (int c = 1; c < 4; ++c) k[4 * (size_t)j + c] = 40.0 * uni() - 20.0;
  }
  CHECK(hdsm_script::tracks_valid(1, n, k.data()));
  std::vector<double> taus = {k[0] - 1.0, k[0], k[4 * (size_t)(n - 1)], k[4 * (size_t)(n - 1)] + 1.0};
  for (int j = 0; j < n; ++j) {
    taus.push_back(k[4 * (size_t)j]);                                        // on the knot: the right-hand segment
    taus.push_back(std::nextafter(k[4 * (size_t)j], -1e300));
    taus.push_back(std::nextafter(k[4 * (size_t)j], 1e300));
    if (j + 1 < n) taus.push_back(k[4 * (size_t)j] + uni() * (k[4 * (size_t)(j + 1)] - k[4 * (size_t)j]));
  }
  for (double tau : taus) {
    std::vector<double> got(9, -7.0);
    double want[9];
    hdsm_script::track_state(k.data(), n, tau, got.data());
    scan_state(k, n, tau, want);
    CHECK(std::memcmp(got.data(), want, sizeof want) == 0);
  }
  // records: N + 1 states of exactly 9 doubles each, both modes; the modes agree up to step_plan, predict = 1 is a straight line behind it
  for (int N : {1, 7, 16})
    for (int sp = 1; sp <= (N < 3 ? N : 3); ++sp)
      for (long long q : {0LL, 3LL, 1000LL, 1LL << 40}) {
        std::vector<double> a((size_t)(N + 1) * 9, -7.0), b(a);
        for (int i = 0; i <= N; ++i) {
          hdsm_script::record_state(k.data(), n, sp, 0.1, 0, q, i, a.data() + 9 * (size_t)i);
          hdsm_script::record_state(k.data(), n, sp, 0.1, 1, q, i, b.data() + 9 * (size_t)i);
        }
        for (int i = 0; i <= N; ++i) {
          double want[9];
          scan_state(k, n, (double)(q * sp + i) * 0.1, want);
          CHECK(std::memcmp(a.data() + 9 * (size_t)i, want, sizeof want) == 0);
          if (i <= sp) CHECK(std::memcmp(a.data() + 9 * (size_t)i, b.data() + 9 * (size_t)i, sizeof want) == 0);
          else
            for (int c = 0; c < 3; ++c) {
              CHECK(b[9 * (size_t)i + 3 + c] == b[9 * (size_t)sp + 3 + c] && b[9 * (size_t)i + 6 + c] == 0.0);
              CHECK(b[9 * (size_t)i + c] == b[9 * (size_t)sp + c] + ((double)(i - sp) * 0.1) * b[9 * (size_t)sp + 3 + c]);
            }
        }
      }
}

int main() {
  for (int n : {1, 2, 3, 5, 64, 65, 255, 256})
    for (int rep = 0; rep < 4; ++rep) one_track(n);
  // refusals: the count, a time that does not increase, non-finite entries, no tracks at all
  std::vector<double> k = {0.0, 1, 2, 3, 1.0, 4, 5, 6, 2.0, 7, 8, 9};
  CHECK(hdsm_script::tracks_valid(1, 3, k.data()) && hdsm_script::tracks_valid(3, 1, k.data()) && hdsm_script::tracks_valid(0, 1, nullptr));
  CHECK(!hdsm_script::tracks_valid(1, 0, k.data()) && !hdsm_script::tracks_valid(1, 257, k.data()) && !hdsm_script::tracks_valid(-1, 3, k.data()));
  CHECK(!hdsm_script::tracks_valid(1, 3, nullptr));
  for (double bad : {1.0, 0.5, std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::infinity()}) {
    std::vector<double> b(k);
    b[8] = bad;
    CHECK(!hdsm_script::tracks_valid(1, 3, b.data()));
  }
  for (size_t e : {1u, 6u, 11u}) {
    std::vector<double> b(k);
    b[e] = -std::numeric_limits<double>::infinity();
    CHECK(!hdsm_script::tracks_valid(1, 3, b.data()));
  }
  std::printf(g_failed ? "%d checks failed\n" : "all checks held\n", g_failed);
  return g_failed ? 1 : 0;
}
