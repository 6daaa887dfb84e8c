// closed_loop.cpp — the C ABI driven from C++ (the reference's language), no Python involved: a swarm of agents on the
// circular exchange of multi_agent_planner_circle.launch.py replans in lock-step, host planner state from
// include/hdsm_swarm.h (the part of Agent::TrajPlanningIteration around the solve), solve on the GPU through hdsm_replan.
// usage: closed_loop [n_agents = 16] [rounds = 120]
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/hdsm.h"
#include "../include/hdsm_swarm.h"

int main(int argc, char** argv) {
  const int n = argc > 1 ? std::atoi(argv[1]) : 16, rounds = argc > 2 ? std::atoi(argv[2]) : 120;
  const int N = 10;
  hdsm_params prm;
  hdsm_default_params(&prm, N);  // agent_agile_config.yaml values
  prm.max_rows_static = 18;
  hdsm_swarm_config cfg;
  hdsm_swarm_default_config(&cfg);
  const int P = prm.poly_hor, RS = prm.max_rows_static;

  const double pi = std::acos(-1.0), R = std::fmax(22.0, n / (2 * pi));
  std::vector<double> starts(3 * n), goals(3 * n);
  for (int k = 0; k < n; ++k) {
    starts[3 * k] = 18.0 + R * std::cos(2 * pi * k / n), starts[3 * k + 1] = 15.0 + R * std::sin(2 * pi * k / n), starts[3 * k + 2] = 1.5;
  }
  for (int k = 0; k < n; ++k)
    for (int c = 0; c < 3; ++c) goals[3 * k + c] = starts[3 * ((k + n / 2) % n) + c];

  void *solver = nullptr, *swarm = nullptr;
  if (hdsm_create(&prm, n, n, 0, &solver) != HDSM_OK) {
    std::fprintf(stderr, "hdsm_create: %s\n", hdsm_last_error());
    return 2;
  }
  if (hdsm_swarm_create(&prm, &cfg, n, 0, n, starts.data(), goals.data(), &swarm) != HDSM_OK) return 2;
  if (hdsm_swarm_set_audit(swarm, 1, 1.0) != HDSM_OK) return 2;  // the flight audit: separation over the whole flown step

  std::vector<int32_t> id(n), n_poly(n), n_rows(n * P), status(n);
  std::vector<double> state(9 * n), ref(6 * N * n), A((size_t)n * P * RS * 3), b((size_t)n * P * RS);
  std::vector<double> plans((size_t)n * (N + 1) * 9, 0.0), traj((size_t)n * (N + 1) * 9), ctrl((size_t)n * N * 3), obj(n);
  std::vector<uint8_t> has(n, 0), used(n * P), has_new(n);
  std::vector<double> plans_new(plans.size()), pos(3 * n), dist(n);
  std::vector<int32_t> nfail(n);

  double solve_ms = 0;
  int failures = 0;
  for (int r = 0; r < rounds; ++r) {
    if (hdsm_swarm_prepare(swarm, plans.data(), has.data(), id.data(), state.data(), ref.data(), n_poly.data(), n_rows.data(),
                           A.data(), b.data()) != HDSM_OK)
      return 3;
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = hdsm_replan(solver, n, n, id.data(), state.data(), ref.data(), n_poly.data(), n_rows.data(), A.data(), b.data(),
                               plans.data(), has.data(), traj.data(), ctrl.data(), used.data(), status.data(), obj.data());
    solve_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (rc != HDSM_OK) {
      std::fprintf(stderr, "hdsm_replan: %s\n", hdsm_last_error());
      return 3;
    }
    for (int k = 0; k < n; ++k) failures += status[k] == HDSM_NO_SOLUTION;
    if (hdsm_swarm_commit(swarm, traj.data(), ctrl.data(), used.data(), status.data(), plans_new.data(), has_new.data()) != HDSM_OK)
      return 3;
    plans.swap(plans_new), has.swap(has_new);
    if (hdsm_swarm_audit(swarm, plans.data(), has.data()) != HDSM_OK) return 3;  // after the gather: the records of all agents
  }
  hdsm_swarm_state(swarm, pos.data(), dist.data(), nfail.data());
  double far = 0;
  for (int k = 0; k < n; ++k) far = std::fmax(far, dist[k]);
  // the flight report: the smallest separation ratio flown (sigma = 1: the ellipsoids of two drones touch), who and when
  std::vector<hdsm_flight_report> rep(n);
  if (hdsm_swarm_flight_report(swarm, rep.data()) != HDSM_OK) return 3;
  int worst = 0;
  long long close_rounds = 0;
  double flown = 0, speed_max = 0;
  for (int k = 0; k < n; ++k) {
    if (rep[k].sep2_min < rep[worst].sep2_min) worst = k;
    close_rounds += rep[k].close_rounds, flown += rep[k].dist, speed_max = std::fmax(speed_max, rep[k].speed_max);
  }
  // sigma of a lone agent: infinite (no partner). With the equal radii of the default parameters the safety ellipsoid is a sphere and
  // sigma * 2 * drone_radius is the centre distance in metres; with unequal radii it is no length, and only sigma is printed.
  const double sigma = rep[worst].sep_partner >= 0 ? std::sqrt(rep[worst].sep2_min) : INFINITY;
  const double approach = prm.drone_radius == prm.drone_z_offset ? sigma * 2 * prm.drone_radius : NAN;
  std::printf("closed_loop: %d agents, %d rounds, %.3f ms per replan round through hdsm_replan (host buffers), "
              "instances without solution %d, closest approach %.3f m, farthest agent %.2f m from its goal\n",
              n, rounds, solve_ms / rounds, failures, approach, far);
  std::printf("flight report: sigma_min %.4f (agents %d and %d, round %lld), agent-rounds below sigma 1: %lld, %.1f m flown, top speed %.2f m/s\n",
              sigma, worst, (int)rep[worst].sep_partner, (long long)rep[worst].sep_round, close_rounds, flown, speed_max);
  hdsm_swarm_destroy(swarm);
  hdsm_destroy(solver);
  return 0;
}
