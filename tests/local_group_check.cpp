// local_group_check.cpp — csrc/local_group.h, the shared part of a local communicator group (hdsm_comm_create_local), on the host
// (HDSM_DEVICE_MEM_HOST: events and tables are malloc'ed and counted, the k-th allocation can be made to fail). Stand-alone; built
// with the address and undefined-behaviour sanitizers by tests/test_local_ranks.py. Members stand in for the hdsm_comm objects of
// exchange_kernels.hip: a pointer to the group each, joined at creation, left in any order; the last one to leave frees the group.
// Every property is an assertion of this program (CHECK). Exit status 0 = all held.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "../multi_agent_pkgs_amd/csrc/local_group.h"

using hdsm_local::Group;
using hdsm_mem::g_fail_in;
using hdsm_mem::g_live;

static int g_failed = 0;
#define CHECK(cond)                                                         \
  do {                                                                      \
    if (!(cond)) std::printf("line %d: %s\n", __LINE__, #cond), ++g_failed; \
  } while (0)

static int g_device_calls = 0, g_refuse_device = -1;
static hipError_t on_device(int d) { return ++g_device_calls, d == g_refuse_device ? hipErrorInvalidDevice : hipSuccess; }

namespace {
struct Member {
  Group* group = nullptr;
  int rank = 0;
};
}  // namespace

// hdsm_comm_create_local's shape: the group, then one member per rank
static hipError_t create(int world, const std::vector<int>& dev, std::vector<Member>* out) {
  out->clear();
  Group* g = reinterpret_cast<Group*>(1);
  if (const hipError_t e = Group::create(world, 99, dev.data(), on_device, &g)) {
    CHECK(g == nullptr);
    return e;
  }
  for (int r = 0; r < world; ++r) g->join(), out->push_back(Member{g, r});
  return hipSuccess;
}

// two events per rank and one table per distinct device
static long expected_live(const std::vector<int>& dev) {
  std::vector<int> u(dev);
  std::sort(u.begin(), u.end());
  return 2 * (long)dev.size() + (long)(std::unique(u.begin(), u.end()) - u.begin());
}

static void check_world(const std::vector<int>& dev) {
  const int world = (int)dev.size();
  std::vector<int> order(world);
  for (int r = 0; r < world; ++r) order[r] = r;
  long allocs = 0;
  do {  // every order of leaving: the group lives exactly as long as one member does
    std::vector<Member> m;
    g_fail_in = 1 << 20;
    CHECK(create(world, dev, &m) == hipSuccess && (int)m.size() == world);
    allocs = (1 << 20) - g_fail_in;
    g_fail_in = 0;
    CHECK(allocs == expected_live(dev) && g_live == allocs);
    Group* g = m[0].group;
    CHECK(g->world == world && g->rec == 99 && g->members == world && !g->flown && g->per == 0);
    for (int r = 0; r < world; ++r) {
      const hdsm_local::Rank& k = g->ranks[r];
      CHECK(k.device == dev[r] && k.published && k.gathered && k.send == nullptr);
      CHECK(k.table_rank <= r && dev[k.table_rank] == dev[r] && (k.table_rank == r) == (bool)k.d_table);
      for (int q = 0; q < k.table_rank; ++q) CHECK(dev[q] != dev[r]);  // (the FIRST rank on the device)
      CHECK(g->table(r) != nullptr && g->table(r) == g->ranks[k.table_rank].d_table.get());
      for (int q = 0; q < world; ++q) CHECK(g->table(r)[q] == nullptr);  // zero-filled, all `world` entries there (the sanitizer watches the last)
    }
    for (int i = 0; i < world; ++i) {
      CHECK(g_live == allocs);
      const bool gone = Group::leave(m[order[i]].group);
      m[order[i]].group = nullptr;
      CHECK(gone == (i == world - 1));
    }
    CHECK(g_live == 0);
  } while (std::next_permutation(order.begin(), order.end()));
  for (long k = 1; k <= allocs; ++k) {  // the k-th allocation fails: the error comes back, nothing stays, no member was made
    std::vector<Member> m;
    g_fail_in = k;
    CHECK(create(world, dev, &m) == hipErrorOutOfMemory && m.empty() && g_fail_in == 0);
    CHECK(g_live == 0);
  }
  for (int r = 0; r < world; ++r) {  // a device that cannot be made current: the same way out
    std::vector<Member> m;
    g_refuse_device = dev[r];
    CHECK(create(world, dev, &m) == hipErrorInvalidDevice && m.empty() && g_live == 0);
    g_refuse_device = -1;
  }
}

int main() {
  {
    Group* g = reinterpret_cast<Group*>(1);
    const int dev0 = 0;
    CHECK(Group::create(0, 99, &dev0, on_device, &g) == hipErrorInvalidValue && g == nullptr);
    g = reinterpret_cast<Group*>(1);
    CHECK(Group::create(2, 99, nullptr, on_device, &g) == hipErrorInvalidValue && g == nullptr && g_live == 0);
  }
  check_world({0});           // a group of one
  check_world({0, 0, 0});     // three ranks on one device: one table
  check_world({0, 1, 2});     // one rank per device: three tables
  check_world({0, 0, 0, 0});
  check_world({1, 0, 1, 0});  // two devices, two ranks each: the tables are held by ranks 0 and 1
  CHECK(g_device_calls > 0 && g_live == 0);
  std::printf(g_failed ? "%d check(s) failed\n" : "local_group: all checks held\n", g_failed);
  return g_failed ? 1 : 0;
}
