// audit_core.h — the flight audit: what a round of published records flew, as plain functions that compile for the host form
// (audit_host.cpp, the host mirror) AND for the device kernels (audit_kernels.hip). One source, the same IEEE operations in the
// same order (floating-point contraction off, divisions and square roots correctly rounded on both sides), so the two forms
// agree bit for bit.
//
// Separation. The separating planes of the reference ask for a centre distance of 2 safety_dist along the line between two
// drones, safety_dist = the radius in that direction of the ellipse with semi-axes drone_radius / drone_z_offset (AC:1158-1170).
// That is q(d) >= 1 with q(d) = (dx^2 + dy^2) / (2 drone_radius)^2 + dz^2 / (2 drone_z_offset)^2; sigma = sqrt(q). Everything
// here works in q: no square root is taken. The two weights 1 / (2 r)^2 are formed once (weights()) and multiplied in.
//
// Pair rule. Both agents fly their records synchronously: in sub-step s < step_plan agent a moves P_a[s] -> P_a[s + 1] linearly
// while b moves P_b[s] -> P_b[s + 1]. The relative vector is d0 + t e, t in [0, 1]; q along it is a parabola whose minimum is at
// t* = clamp(-<d0, e>_w / <e, e>_w, 0, 1) (t* = 0 when <e, e>_w == 0: equal velocities, no division).
// An agent's result is the minimum over sub-steps and partners; ties go to the smaller sub-step, then the lower global id.
//
// Own track. Per sub-step: the world voxel under P[s + 1] (>= 100 occupied, < 0 unknown, 1..99 potential), the reference's
// Raycast (hdsm_sw::raycast) from P[s] to P[s + 1] over the WORLD grid (outside the world = free), the length flown, and the
// speed of the state the agent ends the round in.
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "../../include/hdsm_swarm.h"
#include "swarm_core.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace hdsm_audit {

using hdsm_sw::V3;

struct Weights {
  double wxy, wz;
};
CD_HD Weights weights(double drone_radius, double drone_z_offset) {
  const double a = 2.0 * drone_radius, b = 2.0 * drone_z_offset;
  return Weights{1.0 / (a * a), 1.0 / (b * b)};
}
CD_HD double wdot(const Weights& w, double ax, double ay, double az, double bx, double by, double bz) {
  return (ax * bx + ay * by) * w.wxy + (az * bz) * w.wz;
}

// min over t in [0, 1] of q((a0 - b0) + t ((a1 - b1) - (a0 - b0))); a0, a1, b0, b1: three doubles each. At t* >= 1 the end vector
// a1 - b1 itself is taken (not d0 + 1 e, which may differ from it in the last bit): the end of a sub-step and the start of the next
// then give the same q exactly, and the tie rule — not a rounding — decides between them.
CD_HD double pair_q(const Weights& w, const double* a0, const double* a1, const double* b0, const double* b1) {
  const double d0x = a0[0] - b0[0], d0y = a0[1] - b0[1], d0z = a0[2] - b0[2];
  const double d1x = a1[0] - b1[0], d1y = a1[1] - b1[1], d1z = a1[2] - b1[2];
  const double ex = d1x - d0x, ey = d1y - d0y, ez = d1z - d0z;
  const double ee = wdot(w, ex, ey, ez, ex, ey, ez);
  double dx = d0x, dy = d0y, dz = d0z;
  if (ee != 0.0) {
    const double t = -wdot(w, d0x, d0y, d0z, ex, ey, ez) / ee;
    if (t >= 1.0) dx = d1x, dy = d1y, dz = d1z;
    else if (t > 0.0) dx = d0x + t * ex, dy = d0y + t * ey, dz = d0z + t * ez;
  }
  return wdot(w, dx, dy, dz, dx, dy, dz);
}

struct Best {  // the running minimum of one subject
  double q;
  int32_t partner, substep;
};
CD_HD Best no_partner() { return Best{DBL_MAX, -1, 0}; }
// the total order of the tie rule: smaller q, then the smaller sub-step, then the lower global id
CD_HD bool better(double q, int substep, int partner, const Best& b) {
  return q < b.q || (q == b.q && (substep < b.substep || (substep == b.substep && partner < b.partner)));
}
CD_HD void take(Best& b, double q, int substep, int partner) {
  if (better(q, substep, partner, b)) b.q = q, b.partner = partner, b.substep = substep;
}

// the world grid as hdsm_sw::raycast wants it: raw values, every occupied value reads 100, outside = not a voxel (free)
struct WorldGrid {
  const int8_t* world;
  int dim[3];
  CD_HD bool inside(int i, int j, int k) const { return i >= 0 && j >= 0 && k >= 0 && i < dim[0] && j < dim[1] && k < dim[2]; }
  CD_HD int value(int i, int j, int k) const {
    const int v = world[(size_t)i + (size_t)j * dim[0] + (size_t)k * dim[0] * dim[1]];
    return v >= 100 ? 100 : v;
  }
};

struct World {  // NULL world = free space
  const int8_t* world;
  int32_t wdim[3];
  double worigin[3], voxel_size;
};

// The own-track rule for one agent: P(s) = pos + s * stride (three doubles each), s = 0..S; vel = the velocity of the state the
// round ends in. Fills occupied / unknown / crossed / pot / dist / speed of `out`.
CD_HD void track(const World& wd, const double* pos, int stride, int S, const double* vel, hdsm_audit_round* out) {
  int occupied = 0, unknown = 0, crossed = 0, pot = 0;
  double dist = 0.0;
  for (int s = 0; s < S; ++s) {
    const double* p0 = pos + (size_t)s * stride;
    const double* p1 = p0 + stride;
    dist += hdsm_sw::norm(V3{{p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]}});
    if (wd.world == nullptr) continue;
    const WorldGrid g{wd.world, {wd.wdim[0], wd.wdim[1], wd.wdim[2]}};
    const double vs = wd.voxel_size;
    const V3 l0 = {{(p0[0] - wd.worigin[0]) / vs, (p0[1] - wd.worigin[1]) / vs, (p0[2] - wd.worigin[2]) / vs}};
    const V3 l1 = {{(p1[0] - wd.worigin[0]) / vs, (p1[1] - wd.worigin[1]) / vs, (p1[2] - wd.worigin[2]) / vs}};
    const int i = (int)floor(l1[0]), j = (int)floor(l1[1]), k = (int)floor(l1[2]);
    if (g.inside(i, j, k)) {
      const int v = g.value(i, j, k);
      if (v >= 100) ++occupied;
      else if (v < 0) ++unknown;
      else pot += v;
    }
    V3 hit = {{-1, -1, -1}};
    if (hdsm_sw::raycast(g, l0, l1, hdsm_sw::norm(hdsm_sw::sub(l0, l1)), &hit, [](const V3&) {})) ++crossed;
  }
  out->occupied = occupied, out->unknown = unknown, out->crossed = crossed, out->pot = pot;
  out->dist = dist;
  out->speed = hdsm_sw::norm(V3{{vel[0], vel[1], vel[2]}});
}

CD_HD void empty_round(hdsm_audit_round* out) {  // an agent without a record: neither subject nor partner
  out->sep2 = DBL_MAX, out->partner = -1, out->substep = 0;
  out->occupied = out->unknown = out->crossed = out->pot = 0;
  out->dist = 0.0, out->speed = 0.0;
}

CD_HD void empty_report(hdsm_flight_report* r) {
  r->rounds = r->positions = 0;
  r->sep2_min = DBL_MAX, r->sep_partner = -1, r->sep_substep = 0, r->sep_round = -1;
  r->close_rounds = 0;
  r->occupied = r->unknown = r->crossed = r->pot_sum = 0;
  r->dist = r->speed_sum = r->speed_max = 0.0;
}

// one audited round into the flight record (warn2 = sep_warn^2: a round is close when q < sep_warn^2); sep_round counts the
// agent's audited rounds from 0. A strict '<' keeps the earliest round of a repeated minimum.
CD_HD void accumulate(hdsm_flight_report* r, const hdsm_audit_round& a, int S, double warn2) {
  if (a.sep2 < r->sep2_min) r->sep2_min = a.sep2, r->sep_partner = a.partner, r->sep_substep = a.substep, r->sep_round = r->rounds;
  if (a.sep2 < warn2) ++r->close_rounds;
  r->occupied += a.occupied, r->unknown += a.unknown, r->crossed += a.crossed, r->pot_sum += a.pot;
  r->dist += a.dist, r->speed_sum += a.speed;
  if (a.speed > r->speed_max) r->speed_max = a.speed;
  ++r->rounds, r->positions += S;
}

}  // namespace hdsm_audit
