// hdsm_handle.h — the solver handle behind include/hdsm.h: the knobs hdsm_create settles and every device, pinned and stream resource
// of a handle as a typed member (device_mem.h), grouped by what it is for. Nothing here is released by hand: deleting the handle
// releases what it holds. No device code and nothing of the runtime beyond its types: g++ compiles this header against the host
// seam of device_mem.h (tests/device_mem_check.cpp runs alloc_fixed and SplitState::alloc with every allocation failing in turn).
#pragma once
#include "../../include/hdsm.h"
#include "device_mem.h"
#include "hdsm_shapes.h"
#include "hdsm_types.h"

namespace hdsm_handle __attribute__((visibility("hidden"))) {

using hdsm_mem::DevBuf;
using hdsm_mem::GrowBuf;
struct Handle;

// State of the split launches, allocated on the first one: the hand-over records of pass 1 with their staged rows, the item queue,
// outputs / statistics / guesses per item, snapshot scratch for the persistent workgroups of pass 2.
struct SplitState {
  DevBuf<hdsm::SplitRec> d_recs;  // hand-over records of pass 1 and their staged rows (Args::recs, rec_cand, rec_mw, rec_src)
  DevBuf<double> d_rec_cand;
  DevBuf<long long> d_rec_mw;
  DevBuf<int32_t> d_rec_src, d_rec_count, d_items;
  DevBuf<int32_t> d_slot_busy;  // [pool_cap] snapshot-scratch slots of pass 2 taken (Args::slot_busy)
  DevBuf<int32_t> d_split, d_sub_stats, d_sub_warm, d_sub_status;
  DevBuf<unsigned long long> d_inc;
  DevBuf<int32_t> d_node_pool;  // [max_inst] nodes the sub-blocks of an instance may still open (Args::node_pool)
  DevBuf<double> d_sub_traj, d_sub_ctrl, d_sub_obj, d_sub_scratch;
  DevBuf<uint8_t> d_sub_used;
  int rows_cap = 0, items_cap = 0, sub_slots_n = 0, pool_cap = 0;  // staged rows per record, queue length, persistent workgroups of pass 2, scratch slots

  bool ready() const { return pool_cap > 0; }
  // `items`: the shape of pass 2. After any failure *this is empty again (capacities 0).
  inline hipError_t alloc(const Handle& h, hdsm::Shape items);
};

// The device copies the host-pointer entry points upload into and download from, and their grow-only scratch.
struct HostStaging {
  DevBuf<int32_t> d_agent, d_npoly, d_nrows, d_status;
  DevBuf<double> d_state, d_ref, d_A, d_b, d_plans;
  DevBuf<double> d_traj, d_ctrl, d_obj;
  DevBuf<uint8_t> d_has, d_used;
  GrowBuf<double> planes, common, path, cap, full, pv;
  GrowBuf<int32_t> ncommon, np;
  hdsm_mem::PinnedBuf out;  // hdsm_replan's outputs on their way to the caller's arrays
};

// What the pre-pass kernels write for the solver, and whose pre-pass is still valid.
struct Prepass {
  DevBuf<double> d_pos;      // [n_rob_max][N][3] packed positions (pre-pass)
  DevBuf<double> d_bounds;   // [n_rob_max][4]
  DevBuf<double> d_setup;    // [max_inst][KROWS] the set-up map of every instance of a launch (Args::setup)
  DevBuf<int32_t> d_order;   // [max_inst][2] launch order: (instance, its agent id) per workgroup (k_launch_order)
  DevBuf<double> d_rpos;     // [n_rob_max][N + 1][3] packed positions of steps 0..N (k_ref_pack)
  DevBuf<double> d_rsph;     // [n_rob_max][4] their spheres
  const double* plans = nullptr;  // device loop: the plans buffer k_ref_pack has just packed for the solve as well (launch() skips its pre-pass once)
  int n_rob = 0, n_inst = 0;
  bool ordered = false;
};

struct Handle {
  int device = 0;
  int max_inst = 0, n_rob_max = 0;
  int N = 0, P = 0, RS = 0, n = 0;
  int threads = 256, cus = 256;
  int bounds_min = 256;       // swarms of at least this many agents get the sphere prefilter (HDSM_BOUNDS_MIN)
  int duo_min = 0;            // batches of at least this many instances run two workgroups per CU (HDSM_DUO_MIN; set at create: CUs + 1)
  int tri_min = 0;            // ... and of at least this many three 128-thread workgroups per CU (HDSM_TRI_MIN; 2 x CUs + 1, 0 = never)
  int quad_min = 0;           // ... and of at least this many four per CU, small LDS layout (HDSM_QUAD_MIN; 3 x CUs + 1, 0 = never)
  // subtree splitting (launch_split): 0 never, 1 always, 2 automatic (when the previous launch saw a deep tree)
  int split_mode = 2, split_budget = 0, split_ttl = 0;  // split_budget 0: by batch size, see launch()
  int rec_cap = 2048, item_budget = 32, item_min = 0, poll_sleep = 2;  // hand-over records; pass 2: see hdsm_create
  int rescue_ttl = 0;         // launches left that carry the rescue pass
  bool last_small = false;    // the last launch used a kernel shape with a reduced staging area
  hdsm::Args last_args;       // ... and its arguments (the host-buffer path adds the rescue pass at once)
  int setup_mfma = 1;         // 0 (HDSM_SETUP_MFMA=0): every instance applies the map itself (the form of rounds 1-4)
  int order_min = 0;          // batches of at least this many instances are launched most-expensive-first (0 = never)
  hdsm_params prm{};
  int64_t scratch_stride = 0;

  DevBuf<hdsm::Consts> d_consts;
  DevBuf<double> d_scratch;
  DevBuf<int32_t> d_stats;   // 8 * max_inst: iterations, nodes, sweeps, staged rows, sphere records, pairs, flags, launch-order key
  DevBuf<long long> d_prof;  // 32 * max_inst (HDSM_PROFILE / HDSM_TIMELINE builds)
  DevBuf<int32_t> d_warm;    // (MAXNV + 2) * max_inst: previous optimal working sets (params.warm_start)
  DevBuf<uint8_t> d_zero;    // n_rob_max zero bytes (has_plan of level 1)
  // neighbour groups (hdsm_set_groups): [n_rob_max][2] id range per agent, allocated by the first partition; n_total = 0: none is set.
  // group_max: the largest group (what the prefilter decision keys on instead of n_rob)
  DevBuf<int32_t> d_range;
  int n_total = 0, group_max = 0;
  const int32_t* range() const { return n_total > 0 ? d_range.get() : nullptr; }
  int prefilter_agents(int n_rob) const { return n_total > 0 ? group_max : n_rob; }
  // stale plans. shift: [n_rob] steps by which every instance but k's own reads record k advanced (last state held), read where the
  // plans are packed — d_shift (hdsm_set_plan_shift, [n_rob_max], allocated by the first call) or a borrowed device array
  // (hdsm_set_plan_shift_device); null = none. own_plans / own_has: borrowed, where instance a takes its own previous plan and flag
  // from instead of plans_all[a] / has_plan[a] (hdsm_set_own_plans_device); null = the call's arrays.
  DevBuf<int32_t> d_shift;
  const int32_t* shift = nullptr;
  const double* own_plans = nullptr;
  const uint8_t* own_has = nullptr;
  // words in mapped pinned memory the kernels raise (Args::ovf_flag, tree_flag, item_total): an instance ended on a staging overflow;
  // an instance met a deep tree; items queued by the last split launch (the merge writes it)
  hdsm_mem::MappedWord ovf_flag, tree_flag, item_total;
  SplitState sub;
  HostStaging stage;
  Prepass pre;

  hdsm_mem::DevStream stream;
  hipStream_t last_stream = nullptr;
  hdsm_mem::DevEvent ev_done;  // orders launches that arrive on different streams: recorded on last_stream when a call on ANOTHER stream joins
  bool launched = false;
  bool done_pending = false;   // launches on last_stream since ev_done was last recorded (hdsm_entry.h, mark_done / join_stream)
  bool defer_done = false;     // the device-resident loop is issuing a round on one stream (hdsm_internal_defer_done): the pre-pass rides on the reference
  hdsm_mem::TimedInterval kernel_time;  // hdsm_set_kernel_timing: around the solver kernel alone (after the pre-pass)
  bool time_kernel = false;

  // Everything a handle holds from hdsm_create on, zero-filled where the kernels rely on it. The sizes come from the members above.
  hipError_t alloc_fixed() {
    const size_t I = (size_t)max_inst, R = (size_t)n_rob_max, N = (size_t)this->N, P = (size_t)this->P, RS = (size_t)this->RS;
    hdsm_mem::FirstError ok;
    ok(d_consts.alloc(1)), ok(d_scratch.alloc(I * (size_t)scratch_stride)), ok(d_stats.alloc_zeroed(8 * I));
    ok(d_warm.alloc_zeroed((hdsm::MAXNV + 2) * I)), ok(d_zero.alloc_zeroed(R));
#if defined(HDSM_PROFILE) || defined(HDSM_TIMELINE)
    ok(d_prof.alloc(32 * I));
#endif
    HostStaging& s = stage;
    ok(s.d_agent.alloc(I)), ok(s.d_npoly.alloc(I)), ok(s.d_nrows.alloc(I * P)), ok(s.d_status.alloc(I));
    ok(s.d_state.alloc(I * 9)), ok(s.d_ref.alloc(I * N * 6));
    // (the fetch kernel of hdsm_replan uploads only the rows of the static polyhedra that exist: the rest stays finite)
    ok(s.d_A.alloc_zeroed(I * P * RS * 3)), ok(s.d_b.alloc_zeroed(I * P * RS)), ok(s.d_plans.alloc_zeroed(R * (N + 1) * 9));
    ok(s.d_traj.alloc(I * (N + 1) * 9)), ok(s.d_ctrl.alloc(I * N * 3)), ok(s.d_obj.alloc(I)), ok(s.d_has.alloc(R)), ok(s.d_used.alloc(I * P));
    ok(pre.d_pos.alloc(R * N * 3)), ok(pre.d_bounds.alloc(R * 4)), ok(pre.d_setup.alloc(I * hdsm::KROWS)), ok(pre.d_order.alloc(2 * I));
    ok(pre.d_rpos.alloc(R * (N + 1) * 3)), ok(pre.d_rsph.alloc(R * 4));
    ok(ovf_flag.create()), ok(tree_flag.create()), ok(item_total.create());
    ok(stream.create()), ok(ev_done.create(hipEventDisableTiming)), ok(kernel_time.create());
    return ok.e;
  }
};

inline hipError_t SplitState::alloc(const Handle& h, hdsm::Shape items) {
  // (resident workgroups of pass 2 per CU: per_cu of its shape, see the LDS checks at SHAPE_LAUNCH)
  sub_slots_n = hdsm::SHAPES[items].per_cu * h.cus;
  rows_cap = hdsm::SHAPES[items].cmax;
  // (rec_cap — records: one per instance that hands its search over + one per item that hands over again — set by hdsm_create)
  items_cap = h.rec_cap * 16 < 4096 ? 4096 : h.rec_cap * 16;
  // snapshot scratch of pass 2: one slot per workgroup that can be resident + one per record (an item that hands over again leaves
  // its slot to its record for the rest of the launch)
  pool_cap = sub_slots_n + h.rec_cap;
  const size_t G = (size_t)items_cap, R = (size_t)h.rec_cap, N = (size_t)h.N, I = (size_t)h.max_inst, rows = (size_t)rows_cap;
  hdsm_mem::FirstError ok;
  ok(d_recs.alloc(R)), ok(d_rec_cand.alloc(R * rows * 4)), ok(d_rec_mw.alloc(R * rows)), ok(d_rec_src.alloc(R * rows));
  ok(d_rec_count.alloc(8 + R)), ok(d_items.alloc(G)), ok(d_slot_busy.alloc((size_t)pool_cap));
  ok(d_split.alloc_zeroed(2 * I)), ok(d_inc.alloc(I)), ok(d_node_pool.alloc(I));
  ok(d_sub_stats.alloc(8 * G)), ok(d_sub_warm.alloc((hdsm::MAXNV + 2) * G)), ok(d_sub_status.alloc(G));
  ok(d_sub_traj.alloc(G * (N + 1) * 9)), ok(d_sub_ctrl.alloc(G * N * 3)), ok(d_sub_obj.alloc(G)), ok(d_sub_used.alloc(G * h.P));
  ok(d_sub_scratch.alloc((size_t)pool_cap * (size_t)h.scratch_stride));
  if (ok.ok()) ok(hdsm_mem::raw_fill(d_rec_count.get(), 0, 8 * sizeof(int32_t)));
  if (!ok.ok()) *this = SplitState{};
  return ok.e;
}

}  // namespace hdsm_handle
