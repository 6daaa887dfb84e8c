// local_ranks.cpp — the flight of sharded_loop.cpp in ONE process: the circular exchange sharded into `world` contiguous blocks, every
// block a device-resident loop of its own (hdsm_dswarm_*), all of them ranks of one local communicator group (hdsm_comm_create_local)
// and flown with one call per round (hdsm_dswarm_round_ranks). No launcher, no unique id, no RCCL: a rank gathers the other ranks'
// records with one kernel that reads their send buffers through plain pointers. All ranks share device 0 here; with one solver handle
// per GPU the same calls fly one rank per device (peer access is checked and enabled by hdsm_comm_create_local). No HIP headers needed.
// usage: local_ranks <world> [n_agents = 64] [rounds = 60]
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/hdsm.h"
#include "../include/hdsm_swarm.h"

#define CK(x, text)                                                   \
  do {                                                                \
    if ((x) != 0) {                                                   \
      std::fprintf(stderr, "%s failed: %s\n", #x, text());            \
      return 3;                                                       \
    }                                                                 \
  } while (0)

int main(int argc, char** argv) {
  if (argc < 2) return std::fprintf(stderr, "usage: local_ranks <world> [n_agents] [rounds]\n"), 1;
  const int world = std::atoi(argv[1]), n = argc > 2 ? std::atoi(argv[2]) : 64, rounds = argc > 3 ? std::atoi(argv[3]) : 60;
  if (world < 1 || n < 1 || rounds < 1) return std::fprintf(stderr, "world, n_agents and rounds must be positive\n"), 1;
  const int N = 10, per = (n + world - 1) / world, REC = (N + 1) * 9;
  hdsm_params prm;
  hdsm_default_params(&prm, N);
  prm.max_rows_static = 18;
  hdsm_swarm_config cfg;
  hdsm_swarm_default_config(&cfg);

  const double pi = std::acos(-1.0), R = std::fmax(22.0, n / (2 * pi));
  std::vector<double> starts(3 * n), goals(3 * n);
  for (int k = 0; k < n; ++k)
    starts[3 * k] = 18.0 + R * std::cos(2 * pi * k / n), starts[3 * k + 1] = 15.0 + R * std::sin(2 * pi * k / n), starts[3 * k + 2] = 1.5;
  for (int k = 0; k < n; ++k)
    for (int c = 0; c < 3; ++c) goals[3 * k + c] = starts[3 * ((k + n / 2) % n) + c];

  // one solver handle, one host mirror and one device loop per rank; the mirrors only hand their agents over
  std::vector<void*> solver(world, nullptr), mirror(world, nullptr), comm(world, nullptr), dswarm(world, nullptr);
  for (int r = 0; r < world; ++r) {
    const int first = std::min(r * per, n), n_local = std::min(per, n - first);  // (an empty trailing rank: first = n, no agent)
    CK(hdsm_create(&prm, per, world * per, 0, &solver[r]), hdsm_last_error);
    CK(hdsm_swarm_create(&prm, &cfg, n, first, n_local, starts.data() + 3 * first, goals.data() + 3 * first, &mirror[r]), hdsm_last_error);
  }
  CK(hdsm_comm_create_local(world, solver.data(), comm.data()), hdsm_last_error);
  for (int r = 0; r < world; ++r) CK(hdsm_dswarm_create(mirror[r], solver[r], 0, world, &dswarm[r]), hdsm_dswarm_last_error);

  const size_t G = (size_t)world * per;
  std::vector<double> plans(G * REC);
  std::vector<uint8_t> has(G);
  const auto t0 = std::chrono::steady_clock::now();
  for (int r = 0; r < rounds; ++r) CK(hdsm_dswarm_round_ranks(world, dswarm.data(), comm.data(), nullptr), hdsm_dswarm_last_error);
  // every rank holds the records of all agents: rank 0's are read (the download waits for the device)
  int32_t failures = 0;
  CK(hdsm_dswarm_download(dswarm[0], nullptr, plans.data(), has.data(), nullptr, &failures), hdsm_dswarm_last_error);
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  for (int r = 1; r < world; ++r) {
    int32_t f = 0;
    CK(hdsm_dswarm_download(dswarm[r], nullptr, nullptr, nullptr, nullptr, &f), hdsm_dswarm_last_error);
    failures += f;
  }
  int with_plan = 0;
  double checksum = 0;
  for (size_t k = 0; k < G; ++k) {
    with_plan += has[k];
    if (has[k])
      for (int e = 0; e < 3; ++e) checksum += plans[k * REC + 9 + e];
  }
  std::printf("local_ranks: %d ranks in one process, %d agents in blocks of %d, %d rounds, %.3f ms per round, instances without solution %d, "
              "agents with a plan %d, checksum of all first positions %.9f\n",
              world, n, per, rounds, ms / rounds, failures, with_plan, checksum);
  for (int r = 0; r < world; ++r) hdsm_dswarm_destroy(dswarm[r]);
  for (int r = 0; r < world; ++r) hdsm_comm_destroy(comm[r]);
  for (int r = 0; r < world; ++r) hdsm_swarm_destroy(mirror[r]), hdsm_destroy(solver[r]);
  return with_plan == n ? 0 : 7;
}
