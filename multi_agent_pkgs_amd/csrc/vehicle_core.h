// vehicle_core.h — a vehicle in the loop: a quadrotor (thrust along its z axis, first-order lags on body rates and thrust) with the
// position / attitude controller that sits on it, flying the setpoints of command_core.h, as plain functions that compile for the host
// forms (vehicle_host.cpp, swarm_models.cpp) AND for the device kernel (vehicle_kernels.hip). One source, the same IEEE operations in
// the same order (floating-point contraction off, sqrt and division correctly rounded on both sides), so the forms agree bit for bit.
// No libm call: the yaw's sine and cosine are command_core.h's sincos_own, the draws track_core.h's key / draw.
//
// THE ORDER WRITTEN HERE IS THE DEFINITION (semantics and bounds: include/hdsm_swarm.h, "a vehicle in the loop"). Throughout:
// dot(a, b) = (a0 b0 + a1 b1) + a2 b2; a x b = (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0); clamp(x, lo, hi) = lo if x < lo, hi if
// x > hi, else x (a NaN passes through); G = (0, 0, -9.81); q = (x, y, z, w).
//   frame      x_b = (1 - 2 (yy + zz), 2 (xy + zw), 2 (xz - yw)); y_b = (2 (xy - zw), 1 - 2 (xx + zz), 2 (yz + xw));
//              z_b = (2 (xz + yw), 2 (yz - xw), 1 - 2 (xx + yy)), every product of two components rounded once.
//   controller a_c[k] = ((a_r[k] + kp[k] (p_r[k] - p[k])) + kv[k] (v_r[k] - v[k])) - G[k];  n2 = dot(a_c, a_c);  z_d = a_c / sqrt(n2)
//              if n2 > 0 else z_b;  f_c = clamp(dot(a_c, z_b));  x_i = (cy, sy, 0.0);  y = z_d x x_i;  ny = sqrt(dot(y, y));  y_d = y_b
//              if ny == 0 else y / ny;  x_d = y_d x z_d;  e = 0.5 (dot(z_d, y_b) - dot(y_d, z_b), dot(x_d, z_b) - dot(z_d, x_b),
//              dot(y_d, x_b) - dot(x_d, y_b));  omega_c[k] = clamp(-(k_att[k] e[k]), -rate_max[k], rate_max[k]).
//   derivative p' = v;  v'[k] = ((f z_b[k] + G[k]) - drag[k] v[k]) + w[k];  q' = 0.5 ((w ox + y oz) - z oy, (w oy + z ox) - x oz,
//              (w oz + x oy) - y ox, -((x ox + y oy) + z oz)) with o = omega;  omega'[k] = (omega_c[k] - omega[k]) * r_rate;
//              f' = (f_c - f) * r_thrust, with r_rate = 1.0 / tau_rate and r_thrust = 1.0 / tau_thrust, each rounded once per round: the
//              two lags are the only divisors a sub-step would meet sixteen times (four stages, four elements), and a division costs
//              the device a dozen instructions of a chain that has nothing else to issue. The divisions that normalise (z_d, y_d, q)
//              stay divisions: 9.81 / 9.81 is 1, 9.81 * (1.0 / 9.81) need not be, and the hover is an exact fixed point.
//   RK4        k1 = F(Y); k2 = F(Y + (0.5 h) k1); k3 = F(Y + (0.5 h) k2); k4 = F(Y + h k3); Y = Y + (h / 6.0) (((k1 + 2.0 k2) + 2.0 k3)
//              + k4), element by element; then q = q / sqrt(((xx + yy) + zz) + ww).
//   reference  hold: (p_r, v_r, a_r) = setpoint j. along: knot (p_j, v_j, a_j), t = (double)s * h: p_r = (p_j + v_j t) + 0.5 (a_j (t t)),
//              v_r = v_j + a_j t, a_r = a_j.
//   gust       w[k] = wind[k] + gust[k] * draw(key(seed, id, q), k), once per agent and round.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <cmath>

#include "../../include/hdsm_swarm.h"
#include "command_core.h"
#include "track_core.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define VEH_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define VEH_HD inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace hdsm_veh {

constexpr int MAX_SUB = 1000;
constexpr double GZ = -9.81;  // (command_core.h's attitude subtracts the same constant)

// the integrated state, in registers
struct Y {
  double p[3], v[3], q[4], o[3], f;
};
// what a sub-step holds: the controller's outputs
struct Held {
  double oc[3], fc;
};

VEH_HD double dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
VEH_HD void cross3(const double* a, const double* b, double* c) {
  c[0] = a[1] * b[2] - a[2] * b[1], c[1] = a[2] * b[0] - a[0] * b[2], c[2] = a[0] * b[1] - a[1] * b[0];
}
VEH_HD double clamp(double x, double lo, double hi, int* hit) {
  if (x < lo) return *hit = 1, lo;
  if (x > hi) return *hit = 1, hi;
  return x;
}
VEH_HD void z_axis(const double* q, double* zb) {
  zb[0] = 2.0 * (q[0] * q[2] + q[1] * q[3]), zb[1] = 2.0 * (q[1] * q[2] - q[0] * q[3]), zb[2] = 1.0 - 2.0 * (q[0] * q[0] + q[1] * q[1]);
}
VEH_HD void frame(const double* q, double* xb, double* yb, double* zb) {
  const double xx = q[0] * q[0], yy = q[1] * q[1], zz = q[2] * q[2], xy = q[0] * q[1], xz = q[0] * q[2], yz = q[1] * q[2];
  const double xw = q[0] * q[3], yw = q[1] * q[3], zw = q[2] * q[3];
  xb[0] = 1.0 - 2.0 * (yy + zz), xb[1] = 2.0 * (xy + zw), xb[2] = 2.0 * (xz - yw);
  yb[0] = 2.0 * (xy - zw), yb[1] = 1.0 - 2.0 * (xx + zz), yb[2] = 2.0 * (yz + xw);
  zb[0] = 2.0 * (xz + yw), zb[1] = 2.0 * (yz - xw), zb[2] = 1.0 - 2.0 * (xx + yy);
}
VEH_HD void normalise(double* q) {
  const double n = sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
  q[0] = q[0] / n, q[1] = q[1] / n, q[2] = q[2] / n, q[3] = q[3] / n;
}

// the gust of agent id in vehicle round q, held over the round
VEH_HD void round_wind(const hdsm_vehicle& m, int32_t id, long long q, double* w) {
  const uint64_t h = hdsm_track::key(m.seed, id, q);
#pragma unroll
  for (int k = 0; k < 3; ++k) w[k] = m.wind[k] + m.gust[k] * hdsm_track::draw(h, k);
}

// a vehicle on the state s[9] = (p, v, a) and the yaw
VEH_HD void seat(const hdsm_vehicle& m, const double* s, double yaw, hdsm_vehicle_state& vs) {
  double sy, cy, q[4];
  hdsm_cmd::sincos_own(yaw, &sy, &cy);
  hdsm_cmd::attitude(s + 6, sy, cy, q);
  normalise(q);
  const double t[3] = {s[6] - 0.0, s[7] - 0.0, s[8] - GZ};
  int hit = 0;
#pragma unroll
  for (int k = 0; k < 3; ++k) vs.pos[k] = s[k], vs.vel[k] = s[3 + k], vs.omega[k] = 0.0;
  vs.quat[0] = q[0], vs.quat[1] = q[1], vs.quat[2] = q[2], vs.quat[3] = q[3];
  vs.thrust = clamp(sqrt(dot3(t, t)), m.thrust_min, m.thrust_max, &hit);
  vs.yaw_cmd = yaw, vs.reserved0 = 0.0;
}

// the controller: what the sub-step holds, from the state and the reference (p_r, v_r, a_r, sin and cos of the yaw)
VEH_HD Held control(const hdsm_vehicle& m, const Y& y, const double* pr, const double* vr, const double* ar, double sy, double cy, int* hit_thrust,
                    int* hit_rate) {
  double xb[3], yb[3], zb[3], ac[3], zd[3], yd[3], xd[3], e[3];
  frame(y.q, xb, yb, zb);
#pragma unroll
  for (int k = 0; k < 3; ++k) ac[k] = ((ar[k] + m.kp[k] * (pr[k] - y.p[k])) + m.kv[k] * (vr[k] - y.v[k])) - (k == 2 ? GZ : 0.0);
  const double n2 = dot3(ac, ac);
  if (n2 > 0.0) {
    const double len = sqrt(n2);
    zd[0] = ac[0] / len, zd[1] = ac[1] / len, zd[2] = ac[2] / len;
  } else {
    zd[0] = zb[0], zd[1] = zb[1], zd[2] = zb[2];
  }
  Held u;
  u.fc = clamp(dot3(ac, zb), m.thrust_min, m.thrust_max, hit_thrust);
  const double xi[3] = {cy, sy, 0.0};
  cross3(zd, xi, yd);
  const double ny = sqrt(dot3(yd, yd));
  if (ny == 0.0) yd[0] = yb[0], yd[1] = yb[1], yd[2] = yb[2];
  else yd[0] = yd[0] / ny, yd[1] = yd[1] / ny, yd[2] = yd[2] / ny;
  cross3(yd, zd, xd);
  e[0] = 0.5 * (dot3(zd, yb) - dot3(yd, zb));
  e[1] = 0.5 * (dot3(xd, zb) - dot3(zd, xb));
  e[2] = 0.5 * (dot3(yd, xb) - dot3(xd, yb));
#pragma unroll
  for (int k = 0; k < 3; ++k) u.oc[k] = clamp(-(m.k_att[k] * e[k]), -m.rate_max[k], m.rate_max[k], hit_rate);
  return u;
}

// the reciprocals of the two lags, rounded once per round
struct Lags {
  double r_rate, r_thrust;
};

// F(Y): the plant's derivative, the sub-step's holds and the round's wind given
VEH_HD Y derivative(const hdsm_vehicle& m, const Lags& lag, const Y& y, const Held& u, const double* w) {
  Y d;
  double zb[3];
  z_axis(y.q, zb);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    d.p[k] = y.v[k];
    d.v[k] = ((y.f * zb[k] + (k == 2 ? GZ : 0.0)) - m.drag[k] * y.v[k]) + w[k];
    d.o[k] = (u.oc[k] - y.o[k]) * lag.r_rate;
  }
  const double* q = y.q;
  const double* o = y.o;
  d.q[0] = 0.5 * ((q[3] * o[0] + q[1] * o[2]) - q[2] * o[1]);
  d.q[1] = 0.5 * ((q[3] * o[1] + q[2] * o[0]) - q[0] * o[2]);
  d.q[2] = 0.5 * ((q[3] * o[2] + q[0] * o[1]) - q[1] * o[0]);
  d.q[3] = 0.5 * -((q[0] * o[0] + q[1] * o[1]) + q[2] * o[2]);
  d.f = (u.fc - y.f) * lag.r_thrust;
  return d;
}

// Y + c K, element by element
VEH_HD Y advanced(const Y& y, double c, const Y& k) {
  Y r;
#pragma unroll
  for (int i = 0; i < 3; ++i) r.p[i] = y.p[i] + c * k.p[i], r.v[i] = y.v[i] + c * k.v[i], r.o[i] = y.o[i] + c * k.o[i];
#pragma unroll
  for (int i = 0; i < 4; ++i) r.q[i] = y.q[i] + c * k.q[i];
  r.f = y.f + c * k.f;
  return r;
}
VEH_HD double rk_sum(double k1, double k2, double k3, double k4) { return ((k1 + 2.0 * k2) + 2.0 * k3) + k4; }

// one sub-step: the classical RK4 step of length h, then the quaternion's norm
VEH_HD void rk4(const hdsm_vehicle& m, const Lags& lag, Y& y, const Held& u, const double* w, double h) {
  const double hh = 0.5 * h, h6 = h / 6.0;
  const Y k1 = derivative(m, lag, y, u, w);
  const Y k2 = derivative(m, lag, advanced(y, hh, k1), u, w);
  const Y k3 = derivative(m, lag, advanced(y, hh, k2), u, w);
  const Y k4 = derivative(m, lag, advanced(y, h, k3), u, w);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    y.p[i] = y.p[i] + h6 * rk_sum(k1.p[i], k2.p[i], k3.p[i], k4.p[i]);
    y.v[i] = y.v[i] + h6 * rk_sum(k1.v[i], k2.v[i], k3.v[i], k4.v[i]);
    y.o[i] = y.o[i] + h6 * rk_sum(k1.o[i], k2.o[i], k3.o[i], k4.o[i]);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) y.q[i] = y.q[i] + h6 * rk_sum(k1.q[i], k2.q[i], k3.q[i], k4.q[i]);
  y.f = y.f + h6 * rk_sum(k1.f, k2.f, k3.f, k4.f);
  normalise(y.q);
}

VEH_HD bool finite_y(const Y& y) {
  bool ok = hdsm_cmd::finite3(y.p) && hdsm_cmd::finite3(y.v) && hdsm_cmd::finite3(y.o) && hdsm_cmd::finite3(y.q);
  return ok && hdsm_cmd::finite1(y.q[3]) && hdsm_cmd::finite1(y.f);
}

// One agent's round: step_plan * n_sub sub-steps against sp[step_plan]. start[9]: knot 0 of the along feed; planned_end[9]: the state
// the commit left; vs in and out; flown[9], *d, *dvel, pose (may be NULL) out; *n_thrust, *n_rate += clamped sub-steps. Returns 1 flown,
// 0 re-seated (the end state was not finite). sp may point to device memory, everything else to registers.
VEH_HD int agent_round(const hdsm_vehicle& m, int32_t id, long long q, int step_plan, double dt, const double* start, const hdsm_command* sp,
                       const double* planned_end, hdsm_vehicle_state& vs, double* flown, double* d, double* dvel, hdsm_command* pose,
                       int* n_thrust, int* n_rate) {
  double w[3];
  round_wind(m, id, q, w);
  const double h = dt / (double)m.n_sub;
  const Lags lag{1.0 / m.tau_rate, 1.0 / m.tau_thrust};
  Y y;
#pragma unroll
  for (int k = 0; k < 3; ++k) y.p[k] = vs.pos[k], y.v[k] = vs.vel[k], y.o[k] = vs.omega[k];
#pragma unroll
  for (int k = 0; k < 4; ++k) y.q[k] = vs.quat[k];
  y.f = vs.thrust;
  double yaw_cmd = vs.yaw_cmd;
  double knot[9];
#pragma unroll
  for (int c = 0; c < 9; ++c) knot[c] = start[c];
  int valid = 0;
  hdsm_command next = sp[0];
  for (int j = 0; j < step_plan; ++j) {
    const hdsm_command c = next;
    next = sp[j + 1 < step_plan ? j + 1 : j];  // (asked for before the sub-steps of this interval: off the chain)
    valid = c.valid;
    const bool zeroed = c.valid == 0 && c.quat[0] == 0.0 && c.quat[1] == 0.0 && c.quat[2] == 0.0 && c.quat[3] == 0.0;
    const bool along = m.feed == 1 && c.valid != 0;
    double p0[3], v0[3], a0[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      p0[k] = zeroed ? y.p[k] : along ? knot[k] : c.pos[k];
      v0[k] = zeroed ? 0.0 : along ? knot[3 + k] : c.vel[k];
      a0[k] = zeroed ? 0.0 : along ? knot[6 + k] : c.acc[k];
    }
    yaw_cmd = zeroed ? yaw_cmd : c.yaw;
    double sy, cy;
    hdsm_cmd::sincos_own(yaw_cmd, &sy, &cy);
    for (int s = 0; s < m.n_sub; ++s) {
      double pr[3], vr[3];
      if (along) {
        const double t = (double)s * h;
#pragma unroll
        for (int k = 0; k < 3; ++k) pr[k] = (p0[k] + v0[k] * t) + 0.5 * (a0[k] * (t * t)), vr[k] = v0[k] + a0[k] * t;
      } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) pr[k] = p0[k], vr[k] = v0[k];
      }
      int hit_thrust = 0, hit_rate = 0;
      const Held u = control(m, y, pr, vr, a0, sy, cy, &hit_thrust, &hit_rate);
      *n_thrust += hit_thrust, *n_rate += hit_rate;
      rk4(m, lag, y, u, w, h);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) knot[k] = c.pos[k], knot[3 + k] = c.vel[k], knot[6 + k] = c.acc[k];
  }
  const bool ok = finite_y(y);
  if (ok) {
#pragma unroll
    for (int k = 0; k < 3; ++k) vs.pos[k] = y.p[k], vs.vel[k] = y.v[k], vs.omega[k] = y.o[k];
#pragma unroll
    for (int k = 0; k < 4; ++k) vs.quat[k] = y.q[k];
    vs.thrust = y.f, vs.yaw_cmd = yaw_cmd, vs.reserved0 = 0.0;
    double zb[3];
    z_axis(y.q, zb);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      flown[k] = y.p[k], flown[3 + k] = y.v[k];
      flown[6 + k] = m.acc_from == 1 ? ((y.f * zb[k] + (k == 2 ? GZ : 0.0)) - m.drag[k] * y.v[k]) + w[k] : planned_end[6 + k];
    }
    *d = hdsm_track::pos_dist(planned_end, flown), *dvel = hdsm_track::vel_dist(planned_end, flown);
  } else {
    seat(m, planned_end, hdsm_cmd::finite1(yaw_cmd) ? yaw_cmd : 0.0, vs);
#pragma unroll
    for (int c = 0; c < 9; ++c) flown[c] = planned_end[c];
    *d = 0.0, *dvel = 0.0;
  }
  if (pose != nullptr) {
    hdsm_command c;
#pragma unroll
    for (int k = 0; k < 3; ++k) c.pos[k] = vs.pos[k], c.vel[k] = vs.vel[k], c.acc[k] = flown[6 + k];
    c.quat[0] = vs.quat[0], c.quat[1] = vs.quat[1], c.quat[2] = vs.quat[2], c.quat[3] = vs.quat[3];
    c.yaw = vs.yaw_cmd, c.valid = valid, c.pad = 0, c.reserved0 = 0.0;
    *pose = c;
  }
  return ok ? 1 : 0;
}

// a setting as hdsm_*_set_vehicle and hdsm_vehicle_* accept it
inline bool settings_valid(const hdsm_vehicle* m) {
  if (m == nullptr) return false;
  if (m->n_sub < 1 || m->n_sub > MAX_SUB || m->feed < 0 || m->feed > 1 || m->acc_from < 0 || m->acc_from > 1) return false;
  const auto fin = [](double x) { return std::isfinite(x); };
  for (int k = 0; k < 3; ++k) {
    if (!fin(m->kp[k]) || !fin(m->kv[k]) || !fin(m->k_att[k]) || !fin(m->rate_max[k]) || !fin(m->drag[k]) || !fin(m->wind[k]) || !fin(m->gust[k])) return false;
    if (m->kp[k] < 0 || m->kv[k] < 0 || m->k_att[k] < 0 || !(m->rate_max[k] > 0) || m->drag[k] < 0 || m->gust[k] < 0) return false;
  }
  if (!fin(m->tau_rate) || !fin(m->tau_thrust) || !fin(m->thrust_min) || !fin(m->thrust_max)) return false;
  return m->tau_rate > 0 && m->tau_thrust > 0 && m->thrust_min >= 0 && m->thrust_min <= m->thrust_max;
}

}  // namespace hdsm_veh
