// command_core.h — what a vehicle is told after a round: the yaw step of Agent::ComputeYawAngle (AC:1025-1050), the attitude of
// Agent::ComputeAttitude (AC:1052-1069) and the full-state setpoints planner_crazyswarm_bridge takes from a plan, as plain functions
// that compile for the host forms (command_host.cpp, swarm_models.cpp) AND for the device kernel (command_kernels.hip). One source, the
// same IEEE operations in the same order (floating-point contraction off, products first, sums left to right, sqrt and division
// correctly rounded on both sides), so the forms agree bit for bit. No libm call sits in this path: host libm and the device's math
// library differ in the last bit, so atan2 and sincos are built here from +, -, *, / alone. Their constants were derived with mpmath
// at 400 bits and are written as hexadecimal doubles.
//
// atan2(y, x). r = min(|y|, |x|) / max(|y|, |x|) in [0, 1]; k = (int)(8 r + 0.5), c = k / 8; u = (r - c) / (1 + r c), |u| <= 1/16;
// atan(r) = atan(c) + atan(u), atan(c) from a table of nine entries in two doubles each, atan(u) = u - u z (1/3 - z (1/5 - ... -
// z / 15)) with z = u u (the Taylor series; the first term left out is below 2e-22). The octant is undone with pi/2 and pi in two
// doubles each. Special cases as C's atan2: a NaN in gives a NaN; y = +-0 gives +-0 for x >= +0 and +-pi for x <= -0; x = +-0 gives
// +-pi/2; one argument infinite gives +-0, +-pi, +-pi/2; both infinite +-pi/4 and +-3pi/4. Measured maximum absolute error: DESIGN §8.
//
// sincos(x). n = (int)(x 2/pi +- 0.5); r = ((x - n P1) - n P2) - n P3 with pi/2 = P1 + P2 + P3, P1 and P2 of 33 bits each (Cody and
// Waite: n P1 and n P2 are exact for |n| < 2^20, and so is x - n P1), |r| <= pi/4 + 1e-9; sin r and cos r are the Taylor series up to
// r^17 and r^18 (the first terms left out are below 1e-19 and 4e-21); the quadrant n mod 4 swaps and negates. PINNED for |x| <= 1e4 (a yaw
// grows by 2 pi per lap of a circling agent: 1500 laps). Beyond that bound: up to |x| < 2^20 the reduction stays exact and the error
// stays what it is; for |x| >= 2^20, an infinity or a NaN both results are NaN — never a wrong finite value — and a command built
// from such a yaw carries valid = 0 (every field must be finite).
//
// The yaw step, the attitude, the matrix-to-quaternion rule and the records: include/hdsm_swarm.h, "commands for the vehicle".
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <cmath>

#include "../../include/hdsm_swarm.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define CMD_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define CMD_HD inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace hdsm_cmd {

constexpr double PI_HI = 0x1.921fb54442d18p+1, PI_LO = 0x1.1a62633145c07p-53;      // pi in two doubles (PI_HI is M_PI)
constexpr double PIO2_HI = 0x1.921fb54442d18p+0, PIO2_LO = 0x1.1a62633145c07p-54;  // pi / 2
constexpr double PIO4 = 0x1.921fb54442d18p-1, PI3O4 = 0x1.2d97c7f3321d2p+1;        // pi / 4, 3 pi / 4 to nearest
constexpr double TWO_OVER_PI = 0x1.45f306dc9c883p-1;
constexpr double P1 = 0x1.921fb54400000p+0, P2 = 0x1.0b4611a600000p-34, P3 = 0x1.3198a2e037073p-69;  // pi / 2 = P1 + P2 + P3
constexpr double SINCOS_MAX = 1048576.0;  // 2^20

// (x - x == 0: false for an infinity and for a NaN, without libm)
CMD_HD bool finite1(double x) { return x - x == 0.0; }
CMD_HD bool finite3(const double* v) { return finite1(v[0]) && finite1(v[1]) && finite1(v[2]); }
CMD_HD double qnan() { return __builtin_nan(""); }

// atan(r) for 0 <= r <= 1
CMD_HD double atan_unit(double r) {
  // atan(k / 8), k = 0 .. 8, to nearest and the rest
  constexpr double T_HI[9] = {0.0,
                              0x1.fd5ba9aac2f6ep-4,
                              0x1.f5b75f92c80ddp-3,
                              0x1.6f61941e4def1p-2,
                              0x1.dac670561bb4fp-2,
                              0x1.1e00babdefeb4p-1,
                              0x1.4978fa3269ee1p-1,
                              0x1.700a7c5784634p-1,
                              0x1.921fb54442d18p-1};
  constexpr double T_LO[9] = {0.0,
                              -0x1.cd37686760c17p-59,
                              0x1.8ab6e3cf7afbdp-57,
                              -0x1.c63aae6f6e918p-56,
                              0x1.a2b7f222f65e2p-56,
                              -0x1.928df287a668fp-58,
                              0x1.2419a87f2a458p-56,
                              -0x1.8c34d25aadef6p-56,
                              0x1.1a62633145c07p-55};
  const int k = (int)(8.0 * r + 0.5);
  const double c = 0.125 * (double)k;
  const double u = k == 0 ? r : (r - c) / (1.0 + r * c);
  const double z = u * u;
  double p = 0x1.3b13b13b13b14p-4 - z * 0x1.1111111111111p-4;  // 1/13 - z / 15
  p = 0x1.745d1745d1746p-4 - z * p;                              // 1/11
  p = 0x1.c71c71c71c71cp-4 - z * p;                              // 1/9
  p = 0x1.2492492492492p-3 - z * p;                              // 1/7
  p = 0x1.999999999999ap-3 - z * p;                              // 1/5
  p = 0x1.5555555555555p-2 - z * p;                              // 1/3
  const double a = u - (u * z) * p;
  // (a select per entry, not an indexed load: the table stays in registers and immediates on the device)
  double hi = T_HI[0], lo = T_LO[0];
#pragma unroll
  for (int j = 1; j < 9; ++j) {
    hi = k == j ? T_HI[j] : hi;
    lo = k == j ? T_LO[j] : lo;
  }
  return hi + (a + lo);
}

CMD_HD double atan2_own(double y, double x) {
  if (x != x || y != y) return x + y;
  const double ax = __builtin_fabs(x), ay = __builtin_fabs(y);
  const bool xneg = __builtin_signbit(x) != 0;
  double a;
  if (ay == 0.0) {
    a = xneg ? PI_HI : 0.0;
  } else if (!finite1(ax) && !finite1(ay)) {
    a = xneg ? PI3O4 : PIO4;
  } else if (ay <= ax) {
    const double t = atan_unit(ay / ax);
    a = xneg ? (PI_HI - t) + PI_LO : t;
  } else {
    const double t = atan_unit(ax / ay);
    a = xneg ? (PIO2_HI + t) + PIO2_LO : (PIO2_HI - t) + PIO2_LO;
  }
  return __builtin_copysign(a, y);
}

CMD_HD void sincos_own(double x, double* s_out, double* c_out) {
  if (!(__builtin_fabs(x) < SINCOS_MAX)) {
    *s_out = qnan(), *c_out = qnan();
    return;
  }
  const double fn = x * TWO_OVER_PI;
  const int n = (int)(fn < 0.0 ? fn - 0.5 : fn + 0.5);
  const double dn = (double)n;
  const double r = ((x - dn * P1) - dn * P2) - dn * P3;
  const double z = r * r;
  double ps = 0x1.ae7f3e733b81fp-41 - z * 0x1.952c77030ad4ap-49;  // 1/15! - z / 17!
  ps = 0x1.6124613a86d09p-33 - z * ps;                            // 1/13!
  ps = 0x1.ae64567f544e4p-26 - z * ps;                            // 1/11!
  ps = 0x1.71de3a556c734p-19 - z * ps;                            // 1/9!
  ps = 0x1.a01a01a01a01ap-13 - z * ps;                            // 1/7!
  ps = 0x1.1111111111111p-7 - z * ps;                             // 1/5!
  ps = 0x1.5555555555555p-3 - z * ps;                             // 1/3!
  const double s = r - (r * z) * ps;
  double pc = 0x1.ae7f3e733b81fp-45 - z * 0x1.6827863b97d97p-53;  // 1/16! - z / 18!
  pc = 0x1.93974a8c07c9dp-37 - z * pc;                            // 1/14!
  pc = 0x1.1eed8eff8d898p-29 - z * pc;                            // 1/12!
  pc = 0x1.27e4fb7789f5cp-22 - z * pc;                            // 1/10!
  pc = 0x1.a01a01a01a01ap-16 - z * pc;                            // 1/8!
  pc = 0x1.6c16c16c16c17p-10 - z * pc;                            // 1/6!
  pc = 0x1.5555555555555p-5 - z * pc;                             // 1/4!
  const double c = (1.0 - 0.5 * z) + (z * z) * pc;
  const int q = n & 3;
  *s_out = q == 0 ? s : q == 1 ? c : q == 2 ? -s : -c;
  *c_out = q == 0 ? c : q == 1 ? -s : q == 2 ? -c : s;
}

// Agent::ComputeYawAngle, AC:1028-1048: the yaw after the step. has_ref: n_ref > yaw_idx; ref = traj_ref[yaw_idx][0:3], state =
// state_curr[0:3] of before the commit. *stepped: 1 a step was taken, 0 skipped (no reference point, v . v <= 0.1, v not finite).
CMD_HD double yaw_step(double yaw, bool has_ref, const double* ref, const double* state, double k_p_yaw, double dt, int* stepped) {
  *stepped = 0;
  if (!has_ref) return yaw;
  const double v[3] = {ref[0] - state[0], ref[1] - state[1], ref[2] - state[2]};
  if (!finite3(v)) return yaw;
  if (!((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2] > 0.1)) return yaw;
  const double yaw_ref = atan2_own(v[1], v[0]);  // (the projection on the x-y plane drops v[2])
  double err = yaw_ref - yaw;
  if (err > PI_HI) err = err - 2.0 * PI_HI;
  else if (err < -PI_HI) err = err + 2.0 * PI_HI;
  *stepped = 1;
  return yaw + (k_p_yaw * err) * dt;
}

// Agent::ComputeAttitude, AC:1055-1068, and Eigen's matrix-to-quaternion rule: q = (x, y, z, w) of acceleration acc[3] and the yaw
// whose sine and cosine are sy, cy
CMD_HD void attitude(const double* acc, double sy, double cy, double* q) {
  const double t[3] = {acc[0] - 0.0, acc[1] - 0.0, acc[2] - (-9.81)};
  const double tt = (t[0] * t[0] + t[1] * t[1]) + t[2] * t[2];
  double zb[3] = {t[0], t[1], t[2]};
  if (tt > 0.0) {
    const double len = sqrt(tt);
    zb[0] = t[0] / len, zb[1] = t[1] / len, zb[2] = t[2] / len;
  }
  const double xi[3] = {cy, sy, 0.0};
  const double yb[3] = {zb[1] * xi[2] - zb[2] * xi[1], zb[2] * xi[0] - zb[0] * xi[2], zb[0] * xi[1] - zb[1] * xi[0]};
  const double xb[3] = {yb[1] * zb[2] - yb[2] * zb[1], yb[2] * zb[0] - yb[0] * zb[2], yb[0] * zb[1] - yb[1] * zb[0]};
  // m[r][c], the columns x_b, y_b, z_b
  const double m00 = xb[0], m01 = yb[0], m02 = zb[0];
  const double m10 = xb[1], m11 = yb[1], m12 = zb[1];
  const double m20 = xb[2], m21 = yb[2], m22 = zb[2];
  const double T = (m00 + m11) + m22;
  if (T > 0.0) {
    double s = sqrt(T + 1.0);
    q[3] = 0.5 * s;
    s = 0.5 / s;
    q[0] = (m21 - m12) * s, q[1] = (m02 - m20) * s, q[2] = (m10 - m01) * s;
    return;
  }
  // the largest diagonal entry leads; (i, j, k) a cyclic permutation. Written out per case so that nothing is indexed at run time.
  int i = 0;
  if (m11 > m00) i = 1;
  if (m22 > (i == 0 ? m00 : m11)) i = 2;
  const double mii = i == 0 ? m00 : i == 1 ? m11 : m22;
  const double mjj = i == 0 ? m11 : i == 1 ? m22 : m00;
  const double mkk = i == 0 ? m22 : i == 1 ? m00 : m11;
  const double mkj = i == 0 ? m21 : i == 1 ? m02 : m10, mjk = i == 0 ? m12 : i == 1 ? m20 : m01;
  const double mji = i == 0 ? m10 : i == 1 ? m21 : m02, mij = i == 0 ? m01 : i == 1 ? m12 : m20;
  const double mki = i == 0 ? m20 : i == 1 ? m01 : m12, mik = i == 0 ? m02 : i == 1 ? m10 : m21;
  double s = sqrt(((mii - mjj) - mkk) + 1.0);
  const double qi = 0.5 * s;
  s = 0.5 / s;
  const double w = (mkj - mjk) * s, qj = (mji + mij) * s, qk = (mki + mik) * s;
  q[3] = w;
  q[0] = i == 0 ? qi : i == 1 ? qk : qj;
  q[1] = i == 0 ? qj : i == 1 ? qi : qk;
  q[2] = i == 0 ? qk : i == 1 ? qj : qi;
}

CMD_HD void zero(hdsm_command& c) {
#pragma unroll
  for (int k = 0; k < 3; ++k) c.pos[k] = 0.0, c.vel[k] = 0.0, c.acc[k] = 0.0;
  c.quat[0] = c.quat[1] = c.quat[2] = c.quat[3] = 0.0;
  c.yaw = 0.0, c.reserved0 = 0.0, c.valid = 0, c.pad = 0;
}

// One command from a state s[9] = (p, v, a) and the yaw (sy, cy: its sine and cosine). valid 1 / 2: the state as it is. valid 0 (no plan
// yet): the position held, v and a zero. A state, a yaw or a quaternion that is not finite: all zeros.
CMD_HD void command(const double* s, double yaw, double sy, double cy, int valid, hdsm_command& c) {
  zero(c);
  if (!(finite3(s) && finite3(s + 3) && finite3(s + 6) && finite1(yaw))) return;
  double x[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) x[k] = (valid != 0 || k < 3) ? s[k] : 0.0;
  double q[4];
  attitude(x + 6, sy, cy, q);
  if (!(finite3(q) && finite1(q[3]))) return;
#pragma unroll
  for (int k = 0; k < 3; ++k) c.pos[k] = x[k], c.vel[k] = x[3 + k], c.acc[k] = x[6 + k];
  c.quat[0] = q[0], c.quat[1] = q[1], c.quat[2] = q[2], c.quat[3] = q[3];
  c.yaw = yaw, c.valid = valid;
}

// One agent's round: the yaw step from the state of BEFORE the commit (before[0:3]) and this round's reference point, then setpoint
// [step_plan] from knots 1 .. step_plan of the record [N + 1][9] (valid 0: from `after`, the position held) and the pose from `after`
// [9], the state the round ends in. Returns the new yaw.
CMD_HD double agent_round(double yaw, bool has_ref, const double* ref, const double* before, const double* record, const double* after,
                          int valid, int step_plan, double k_p_yaw, double dt, hdsm_command* setpoint, hdsm_command* pose, int* stepped) {
  const double yaw_new = yaw_step(yaw, has_ref, ref, before, k_p_yaw, dt, stepped);
  double sy, cy;  // (one sincos per agent and round: every command of the round carries the same yaw)
  sincos_own(yaw_new, &sy, &cy);
  hdsm_command c;  // (built in registers, stored once)
  for (int j = 0; setpoint != nullptr && j < step_plan; ++j) {
    double s[9];  // (element by element, not a choice between two pointers: on the device both may be arrays held in registers)
#pragma unroll
    for (int e = 0; e < 9; ++e) s[e] = valid != 0 ? record[(size_t)(j + 1) * 9 + e] : after[e];
    command(s, yaw_new, sy, cy, valid, c);
    setpoint[j] = c;
  }
  if (pose != nullptr) {
    command(after, yaw_new, sy, cy, valid, c);
    *pose = c;
  }
  return yaw_new;
}

// what hdsm_*_set_commands accepts
inline bool settings_valid(int32_t yaw_idx, int32_t n_hor, double k_p_yaw, const double* yaw0, int32_t n) {
  if (yaw_idx < 0 || yaw_idx > n_hor || !std::isfinite(k_p_yaw)) return false;
  for (int k = 0; yaw0 != nullptr && k < n; ++k)
    if (!std::isfinite(yaw0[k])) return false;
  return true;
}

}  // namespace hdsm_cmd
