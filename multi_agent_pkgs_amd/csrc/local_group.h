// local_group.h — the shared part of a local communicator group (hdsm_comm_create_local, ABI 1.9): the ranks of a sharded swarm held
// by ONE process, on one device or on several. Per rank: its device, the events "published" (its k_commit of this round is behind
// this point of its stream) and "gathered" (its k_gather_local of this round has read every send buffer), the address of its send
// buffer, and — once per device, held by the first rank on it — the device-resident table of the `world` send-buffer addresses that
// k_gather_local reads. Everything is held by the owners of device_mem.h; the group itself is host bookkeeping: created once, joined
// by every member (an hdsm_comm), left in any order, gone with its last member. Compiles on the host behind HDSM_DEVICE_MEM_HOST
// (tests/local_group_check.cpp): nothing of the runtime is called here but through the owners, the device is chosen by the caller's
// `on_device`.
#pragma once
#include <memory>
#include <new>

#include "device_mem.h"

namespace hdsm_local __attribute__((visibility("hidden"))) {

struct Rank {
  int device = 0;
  int table_rank = 0;  // the first rank on this device: it holds the device's copy of the table
  hdsm_mem::DevEvent published, gathered;
  const double* send = nullptr;  // [per][rec], bound by the first round of ranks (hdsm_internal_local_bind)
  hdsm_mem::DevBuf<const double*> d_table;  // [world], only in the rank that is its device's table_rank
};

struct Group {
  int world = 0, rec = 0, per = 0;
  int members = 0;     // live hdsm_comm objects of this group
  bool flown = false;  // a round has recorded the "gathered" events: the next commit waits for them
  std::unique_ptr<Rank[]> ranks;

  const double* const* table(int r) const { return ranks[ranks[r].table_rank].d_table.get(); }

  // A group of `world` ranks on devices[world], no member yet. on_device(device) makes that device current (hipSetDevice) before a
  // rank's events and table are created and returns a hipError_t. After an error nothing is left allocated and *out is null.
  template <class OnDevice>
  static hipError_t create(int world, int rec, const int* devices, OnDevice on_device, Group** out) {
    *out = nullptr;
    if (world < 1 || devices == nullptr) return hipErrorInvalidValue;
    std::unique_ptr<Group> g(new (std::nothrow) Group);
    if (!g) return hipErrorOutOfMemory;
    g->ranks.reset(new (std::nothrow) Rank[world]);
    if (!g->ranks) return hipErrorOutOfMemory;
    g->world = world, g->rec = rec;
    for (int r = 0; r < world; ++r) {
      Rank& k = g->ranks[r];
      k.device = devices[r], k.table_rank = r;
      for (int q = r - 1; q >= 0; --q)
        if (devices[q] == devices[r]) k.table_rank = q;
      if (const hipError_t e = on_device(k.device)) return e;
      // (no timing: an event that is only waited for)
      if (const hipError_t e = k.published.create(hipEventDisableTiming)) return e;
      if (const hipError_t e = k.gathered.create(hipEventDisableTiming)) return e;
      if (k.table_rank == r)
        if (const hipError_t e = k.d_table.alloc_zeroed((size_t)world)) return e;
    }
    *out = g.release();
    return hipSuccess;
  }
  void join() { ++members; }
  // a member leaves; true: it was the last one and the group is gone
  static bool leave(Group* g) {
    if (--g->members > 0) return false;
    delete g;
    return true;
  }
};

}  // namespace hdsm_local
