// track_core.h — imperfect tracking: the state an agent has flown instead of the state it planned, and the record of the difference,
// as plain functions that compile for the host forms (track_host.cpp, swarm_models.cpp) AND for the device kernel (track_kernels.hip).
// One source, the same IEEE operations in the same order (floating-point contraction off, products first, sums left to right, sqrt
// correctly rounded on both sides), so the forms agree bit for bit.
//
// Draws. A counter hash without state and without libm. mix(z) in uint64 with wrap-around:
//   z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  z ^ (z >> 31)
// h = mix(mix(mix(seed ^ 0x9E3779B97F4A7C15) + (uint64)id) + (uint64)q): id the agent's GLOBAL id, q the tracking round. Draw c of
// 0..5: s_c = 2.0 * ((double)(mix(h + c + 1) >> 11) * 0x1p-53) - 1.0 — 53 bits into a double, a power of two, a doubling and a
// difference of neighbours on the same grid: every step is exact, s_c lies in [-1, 1).
//
// Flown state of x = (p, v, a) after the interval T. Per axis: w = wind + gust * s_ax; tw = T * w; p' = (p + 0.5 * (T * tw)) + jitter *
// s_{3+ax}; v' = v + tw; a' = a.
//
// Record. d = sqrt((dx*dx + dy*dy) + dz*dz) of the STORED p' - p, the same norm of v' - v; a sample adds d and d*d to the sums and
// raises the two maxima by comparison. A model round counts in `rounds`, a state taken from outside in `external`.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <cmath>

#include "../../include/hdsm_swarm.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define TRACK_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define TRACK_HD inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace hdsm_track {

constexpr int64_t MAX_ROUND = (int64_t)1 << 40;

TRACK_HD uint64_t mix(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// the key of (seed, agent, round); draw c of 0..5 under it
TRACK_HD uint64_t key(uint64_t seed, int32_t id, long long q) {
  return mix(mix(mix(seed ^ 0x9E3779B97F4A7C15ull) + (uint64_t)id) + (uint64_t)q);
}
TRACK_HD double draw(uint64_t h, int c) { return 2.0 * ((double)(mix(h + (uint64_t)c + 1ull) >> 11) * 0x1p-53) - 1.0; }

// the state flown[9] in place of planned[9] (the two may be the same array)
TRACK_HD void flown_state(const hdsm_tracking& m, int32_t id, long long q, double T, const double* planned, double* flown) {
  const uint64_t h = key(m.seed, id, q);
#pragma unroll
  for (int ax = 0; ax < 3; ++ax) {
    const double w = m.wind[ax] + m.gust[ax] * draw(h, ax);
    const double tw = T * w;
    const double p = (planned[ax] + 0.5 * (T * tw)) + m.jitter[ax] * draw(h, 3 + ax);
    const double v = planned[3 + ax] + tw;
    const double a = planned[6 + ax];
    flown[ax] = p, flown[3 + ax] = v, flown[6 + ax] = a;
  }
}

TRACK_HD double norm3(double dx, double dy, double dz) { return sqrt((dx * dx + dy * dy) + dz * dz); }
// |p' - p| and |v' - v| of two stored states
TRACK_HD double pos_dist(const double* before, const double* after) {
  return norm3(after[0] - before[0], after[1] - before[1], after[2] - before[2]);
}
TRACK_HD double vel_dist(const double* before, const double* after) {
  return norm3(after[3] - before[3], after[4] - before[4], after[5] - before[5]);
}

// one sample into an agent's record
TRACK_HD void book(hdsm_track_record& r, double d, double dvel, bool external) {
  if (external) r.external += 1;
  else r.rounds += 1;
  r.dist_sum = r.dist_sum + d;
  r.dist_sq_sum = r.dist_sq_sum + d * d;
  if (d > r.dist_max) r.dist_max = d;
  if (dvel > r.dvel_max) r.dvel_max = dvel;
}

TRACK_HD bool finite9(const double* s) {
  bool ok = true;
#pragma unroll
  for (int c = 0; c < 9; ++c) ok = ok && (s[c] - s[c] == 0.0);  // (false for an infinity and for a NaN, without libm)
  return ok;
}

// a model as hdsm_*_set_tracking and hdsm_track_states_* accept it: every entry finite, the amplitudes not negative
inline bool model_valid(const hdsm_tracking* m) {
  if (m == nullptr) return false;
  for (int ax = 0; ax < 3; ++ax) {
    if (!std::isfinite(m->wind[ax]) || !std::isfinite(m->gust[ax]) || !std::isfinite(m->jitter[ax])) return false;
    if (m->gust[ax] < 0 || m->jitter[ax] < 0) return false;
  }
  return true;
}

}  // namespace hdsm_track
