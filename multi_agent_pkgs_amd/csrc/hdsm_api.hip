// hdsm_api.hip — gfx950 kernels and the extern "C" boundary declared in include/hdsm.h.
//
// One workgroup solves one agent-replan (hdsm_core.h); the launch is a plain 1-D grid of n_inst blocks.
// There is no CPU path in this library: without a HIP device hdsm_create() fails.
// The other entry points of include/hdsm.h: reference_kernels.hip (row f1), exchange_kernels.hip (RCCL), replan_host.hip (hdsm_replan).
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "../../include/hdsm.h"
#include "hdsm_consts.h"
#include "hdsm_core.h"
#include "hdsm_entry.h"
#include "hdsm_handle.h"
#include "hdsm_internal.h"
#include "hdsm_level1.h"
#include "hdsm_shapes.h"
#include "link_core.h"
#include "plan_pack.h"

using namespace hdsm_entry;

namespace {
thread_local std::string g_err;  // the one error text of the hdsm_ family (hdsm_last_error)
}
int hdsm_entry::set_err(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

namespace {

// What a workgroup works on. Ordinary launch: block b -> instance order[b] (or b). Pass 2 of a split launch (a.item_mode): the
// workgroups are PERSISTENT — each draws items from the queue pass 1 filled (Args::items: one open child of an open level of a
// handed-over instance) until the queue is empty; blockIdx only names the workgroup's snapshot scratch.
template <class Sol>
__device__ __forceinline__ void run_block(typename Sol::S* sp, const hdsm::Consts* cp, const hdsm::Args& a) {
  typename Sol::S& s = *sp;
  int inst, out, item = -1, self = -1, slot = 0;  // (ONE call site of the solver per kernel: it is a single inlined body of ~17 k instructions)
  if (a.item_mode) {
    // Pass 2 of a split launch: this workgroup takes ONE item from the queue (Args::items: an open child of an open level of a
    // handed-over instance) and a snapshot-scratch slot, and leaves. The queue can still GROW while items are running (an item
    // whose subtree turns out large hands over again), so a workgroup that finds it empty waits — on a CU that would be idle
    // anyway — until an item appears or no workgroup holds one any more (rec_count[4]). The grid is an upper bound of the items
    // of the launch (hdsm_api.hip, launch()); the workgroups beyond them find the queue empty and nothing running, and leave.
    // (the few launch arguments the loops below need, as plain values: `a` itself referenced inside a loop is kept as a private copy
    // of the whole struct — 256 bytes of scratch per lane in every kernel that shares this function)
    int32_t* const rcnt = a.rec_count;
    int32_t* const busy = a.slot_busy;
    const int icap = a.items_cap, pcap = a.pool_cap, psleep = a.poll_sleep;
    if (threadIdx.x == 0) {
      // ONE atomic per workgroup: a ticket (rcnt[2]). Ticket k is item k of the queue — when it has been published (rcnt[1] > k)
      // the workgroup takes it; until then it waits, READING only. It leaves without an item when every published item has been
      // completed (rcnt[4], raised by a workgroup after its item — and after whatever that item queued was published) and the
      // queue still ends at or before its ticket: nothing is running, so nothing can be queued any more. (Drawing with a
      // compare-and-swap on a shared counter was measured first: 512 workgroups retrying against each other cost a millisecond.)
      const int ticket = atomicAdd(&rcnt[2], 1);
      int got = -1;
      bool timed_out = ticket < icap;
      for (int spins = 0; spins < (1 << 19) && ticket < icap; ++spins) {  // (seconds: whatever holds the last items up)
        const int done = __hip_atomic_load(&rcnt[4], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        int q = __hip_atomic_load(&rcnt[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        q = q < icap ? q : icap;
        if (ticket < q) {
          got = ticket, timed_out = false;
          break;
        }
        // (read BEFORE the queue's end: all of it was completed, and only a running item can extend it) — or the launch was
        // ABORTED (rcnt[6]): a waiter ran out of patience, so its ticket will never be drawn and `done` can never reach the end
        // of the queue again; every other waiter would spin out its own seconds one after the other
        if (done >= q || __hip_atomic_load(&rcnt[6], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) {
          timed_out = false;
          break;
        }
        // (hundreds of workgroups may be waiting, and every look is a device-scope read that no L2 can serve. Letting the few whose
        // tickets come next look without sleeping was measured in round 6: no difference on cfg 3 or cfg 5 — scripts/gpu_r6_poll_ab.sh)
        for (int w = 0; w < psleep; ++w) __builtin_amdgcn_s_sleep(127);
      }
      if (timed_out) atomicExch(&rcnt[6], 1);  // (items left in the queue stay ST_PENDING: the merge reports their instances as LIMIT)
      int sl = -1;
      if (got >= 0) {  // a scratch slot: at most gridDim-resident + records slots are ever busy (a slot left to a record stays busy)
        for (int probe = 0; probe < pcap && sl < 0; ++probe) {
          const int i = (int)(((unsigned)blockIdx.x * 7u + (unsigned)probe) % (unsigned)pcap);
          if (atomicCAS(&busy[i], 0, 1) == 0) sl = i;
        }
        if (sl < 0) atomicAdd(&rcnt[4], 1), got = -2;  // (cannot happen by the count above; the item stays pending: the merge reports a limit)
      }
      s.iters_sh = got, s.rc = sl;
    }
    __syncthreads();
    const int k = hdsm::uni(s.iters_sh);
    slot = hdsm::uni(s.rc);
    __syncthreads();
    if (k < 0) return;  // (uniform: the whole workgroup leaves)
    __threadfence();    // (the item, its record and the snapshots it names were written by another workgroup)
    item = __hip_atomic_load(&a.items[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), out = k, inst = a.recs[item >> 8].inst;
  } else {
    if (a.order) {  // (instance, its agent id): one load — the own plan is requested together with the other inputs of the instance
      const int2 os = reinterpret_cast<const int2*>(a.order)[blockIdx.x];
      inst = os.x, self = os.y;
    } else {
      inst = (int)blockIdx.x;
    }
    out = inst;
    if (a.rescue && !(a.st_flags[inst] & hdsm::FLAG_STAGING_OVERFLOW)) return;  // (uniform)
  }
  // (every solver kernel has the signature (const Consts*, Args): the arguments start at byte 8 of the kernel-argument segment)
#if defined(__HIP_DEVICE_COMPILE__)
  const HDSM_KERNARG_WORD* words = (const HDSM_KERNARG_WORD*)__builtin_amdgcn_kernarg_segment_ptr() + 1;
#else
  const HDSM_KERNARG_WORD* words = nullptr;
#endif
  Sol::solve_instance(s, *cp, a, inst, out, item, self, slot, words);
  if (item >= 0 && threadIdx.x == 0) {  // (the launch arguments from the copy in LDS: the kernel's own are dead after the solver's prologue)
    if (slot >= 0) atomicExch(&s.args.slot_busy[slot], 0);  // (slot < 0: the item handed over again and its scratch stays with its record)
    __threadfence();
    atomicAdd(&s.args.rec_count[4], 1);                     // this item is completed; what it queued has been published
  }
}

// The launch shapes of these kernels: hdsm_shapes.h (HDSM_SOLVER_SHAPES). k_replan runs ONE workgroup per CU: the iteration wave
// needs > 256 registers (a 256-register budget spills 644 B/lane), so the LDS is spent on the largest staging area (staged
// neighbour rows), i.e. on fewer staging-radius retries.
template <int NV, int CMAX, int NT>
__global__ __launch_bounds__(NT) void k_replan(const hdsm::Consts* __restrict__ cp, hdsm::Args a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  using Sol = hdsm::Solver<NV, CMAX>;
  run_block<Sol>(reinterpret_cast<typename Sol::S*>(smem), cp, a);
}

// The same solver budgeted for TWO workgroups per CU (registers: 2 waves per SIMD; LDS: a staging area of CMAX_DUO
// rows makes the instance state fit twice into 160 KB). A single instance is bound by the latency of its one iterating
// wave, so when there are more instances than CUs a second resident workgroup nearly doubles the throughput. Used for
// n <= 30 only (the NV = 48 factor does not fit the halved register file).
template <int NV, int CMAX, int NT>
__global__ __launch_bounds__(NT, 2) void k_replan_duo(const hdsm::Consts* __restrict__ cp, hdsm::Args a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  using Sol = hdsm::Solver<NV, CMAX>;
  run_block<Sol>(reinterpret_cast<typename Sol::S*>(smem), cp, a);
}

// The set-up map of ALL instances of a launch as ONE dense product on the matrix cores. Everything an instance needs before its first
// iteration — x_eq, x0, the gradient at u = 0, the residual of the terminal equalities and their multipliers — is linear in
// v = (state_curr, traj_ref) (Consts::KT, built once by hdsm_create from the Hessian factor): OUT[row][inst] = sum_j KT[j][row] v[inst][j],
// (3n + 12) x (9 + 6N) times (9 + 6N) x n_inst — the one contraction of the path with matrix-matrix shape and more than a handful of
// columns. One wavefront = one 16 x 16 tile of OUT through v_mfma_f64_16x16x4_f64 (A[i = lane & 15][k = lane >> 4] = KT[4 k0 + k][row0 + i],
// B[k = lane >> 4][j = lane & 15] = v[inst0 + j][4 k0 + k], D[row = (lane >> 4) + 4 r][col = lane & 15] in register r). The solver's
// set-up then reads one number per thread instead of 23 coefficients and a 23-term dot product (hdsm_core.h, Args::setup).
struct SetupMapArgs {
  const hdsm::Consts* c;
  const double* state;  // [n_inst][9]
  const double* ref;    // [n_inst][N][6]
  double* out;          // [n_inst][KROWS]
  int32_t n_inst, N, nk, row_tiles, first_block;  // first_block: the workgroup of the pre-pass kernel at which the tiles begin
};
__device__ void setup_map_tile(const SetupMapArgs& m, int tile) {
  using v4d = double __attribute__((ext_vector_type(4)));
  const int lane = (int)threadIdx.x & 63;
  const int rt = tile % m.row_tiles, it = tile / m.row_tiles;
  if (it * 16 >= m.n_inst) return;
  const int i = lane & 15, kk = lane >> 4;
  const int row = rt * 16 + i, inst = it * 16 + i, nvt = 9 + 6 * m.N;
  const bool row_on = row < m.nk, inst_on = inst < m.n_inst;
  const double* st = m.state + (int64_t)(inst_on ? inst : 0) * 9;
  const double* rf = m.ref + (int64_t)(inst_on ? inst : 0) * 6 * m.N;
  v4d acc = {0.0, 0.0, 0.0, 0.0};
  // (the operands of NINE k-steps are requested before the first product is formed: with one step per trip the tile was a chain of 18 - 25
  // dependent round trips to memory, and the tile workgroups — not the packing ones — set the duration of the pre-pass kernel: 6.9 -> 11 us
  // in round 5; two or three trips now)
  constexpr int CH = 9;
  for (int k0 = 0; k0 < nvt; k0 += 4 * CH) {
    double av[CH], bv[CH];
#pragma unroll
    for (int u = 0; u < CH; ++u) {
      const int j = k0 + 4 * u + kk;
      av[u] = (row_on && j < nvt) ? m.c->KT[(int64_t)j * hdsm::KROWS + row] : 0.0;
      bv[u] = (inst_on && j < nvt) ? (j < 9 ? st[j] : rf[j - 9]) : 0.0;
    }
#pragma unroll
    for (int u = 0; u < CH; ++u) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u], bv[u], acc, 0, 0, 0);
  }
  const int col = lane & 15, oi = it * 16 + col;
  if (oi < m.n_inst) {
    for (int r = 0; r < 4; ++r) {
      const int orow = rt * 16 + (lane >> 4) + 4 * r;
      if (orow < m.nk) m.out[(int64_t)oi * hdsm::KROWS + orow] = acc[r];
    }
  }
}

// Pre-pass of every level-2 launch, one thread per agent of the swarm:
//   pos[n_rob][N][3]   positions of steps 1..N of every published plan, packed: the sweeps of the replan kernel read 24 B
//                      per (neighbour, step) instead of striding through 72-B state records (zeros for agents without a plan);
//   bounds[n_rob][4]   (only for swarms of at least bounds_min agents) centre of the bounding box of those positions and the
//                      radius of the sphere around it that holds them (radius -1 = no plan): the sweeps use it to skip
//                      whole neighbours (hdsm_wave_gi.h, sweep_planes).
// shift (hdsm_set_plan_shift*; null = none): record k is packed advanced by shift[k] steps with its last state held
// (hdsm_link::shifted_step) — positions AND sphere, so the sweeps, the prefilter and the warm start's rebuilt rows all see the shifted plan.
__global__ __launch_bounds__(256) void k_plan_prepass(int N, int n_rob, const double* __restrict__ plans,
                                                      const uint8_t* __restrict__ has_plan, double* __restrict__ pos,
                                                      double* __restrict__ bounds, int n_order, const int32_t* __restrict__ key_prev,
                                                      const int32_t* __restrict__ agent_id, int32_t* __restrict__ order, SetupMapArgs sm,
                                                      const int32_t* __restrict__ shift) {
  if (sm.out != nullptr && (int)blockIdx.x >= sm.first_block) {  // the workgroups behind the pre-pass proper: four tiles of the set-up map each
    setup_map_tile(sm, ((int)blockIdx.x - sm.first_block) * 4 + ((int)threadIdx.x >> 6));
    return;
  }
  if (order != nullptr && (int)blockIdx.x == (n_rob + 15) / 16) {  // one extra workgroup: the launch order of the solve that follows
    launch_order_block(n_order, key_prev, agent_id, order);
    return;
  }
  if ((int)blockIdx.x >= (n_rob + 15) / 16) return;
  // 16 lanes per agent (N <= 16 = HDSM_MAX_HOR): lane i copies the position of step i + 1, the box / sphere reductions run
  // over the 16-lane group with DPP-able shuffles — every load of a plan is issued at once instead of N dependent ones
  const int tid = (int)threadIdx.x, i = tid & 15;
  const int k = (int)blockIdx.x * 16 + (tid >> 4);
  const bool live = k < n_rob;
  const bool has = live && has_plan[k];
  const bool on = has && i < N;
  double p[3] = {0.0, 0.0, 0.0};
  if (on) {
    const double* rec = plans + ((int64_t)k * (N + 1) + hdsm_link::shifted_step(1 + i, shift != nullptr ? shift[k] : 0, N)) * 9;
    p[0] = rec[0], p[1] = rec[1], p[2] = rec[2];
  }
  if (live && i < N) {
    double* pk = pos + ((int64_t)k * N + i) * 3;
    pk[0] = p[0], pk[1] = p[1], pk[2] = p[2];
  }
  if (!bounds) return;
  plan_sphere16<false>(live && i == 0, bounds + 4 * (int64_t)k, has, p, on, p, false);
}

__global__ __launch_bounds__(256) void k_launch_order(int n_inst, const int32_t* __restrict__ key_prev, const int32_t* __restrict__ agent_id, int32_t* __restrict__ order) {
  launch_order_block(n_inst, key_prev, agent_id, order);  // level 1 has no pre-pass to ride on
}

// planes[n_inst][N][n_rob][4] for tests / level-1 callers (AC:1100-1205)
__global__ __launch_bounds__(256) void k_tasc_planes(const hdsm::Consts* __restrict__ cp, int n_inst, int n_rob,
                                                     const int32_t* agent_id, const double* state,
                                                     const double* plans, const uint8_t* has_plan,
                                                     double* planes, const int32_t* __restrict__ range, const int32_t* __restrict__ shift,
                                                     const double* own_plans, const uint8_t* own_has) {
  const hdsm::Consts& c = *cp;
  const int N = c.N;
  const int64_t total = (int64_t)n_inst * N * n_rob;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    const int k = (int)(idx % n_rob);
    const int i = (int)((idx / n_rob) % N);
    const int inst = (int)(idx / ((int64_t)n_rob * N));
    const int self = agent_id[inst];
    double row[4] = {0, 0, 0, 0};
    // (neighbour groups: an agent outside self's id range is absent; an instance whose id is not an agent has no range to take)
    const bool ranged = range != nullptr && self >= 0 && self < n_rob;
    const bool near = range == nullptr || (ranged && k >= range[2 * self] && k < range[2 * self + 1]);
    if (k != self && near && has_plan[k]) {
      double cp3[3];
      // (own_plans / own_has: the call's arrays unless hdsm_set_own_plans_device named others; the neighbour's record at its shifted step)
      const bool own = self >= 0 && self < n_rob && own_has[self];
      for (int ax = 0; ax < 3; ++ax)
        cp3[ax] = own ? own_plans[((int64_t)self * (N + 1) + (i + 1)) * 9 + ax] : state[(int64_t)inst * 9 + ax];
      double tmp[4];
      const int ik = hdsm_link::shifted_step(i + 1, shift != nullptr ? shift[k] : 0, N);
      if (hdsm::Solver<32, 16>::tasc_plane(c, cp3, plans + ((int64_t)k * (N + 1) + ik) * 9, tmp))
        row[0] = tmp[0], row[1] = tmp[1], row[2] = tmp[2], row[3] = tmp[3];
    }
    double* out = planes + idx * 4;
    out[0] = row[0], out[1] = row[1], out[2] = row[2], out[3] = row[3];
  }
}

// THREE workgroups of 128 threads (two wavefronts: the iterating one and one helper) per CU, for batches that outnumber the
// resident slots of the two-per-CU kernel. A launch lasts as long as its slowest workgroup CHAIN: with 1024 instances on 512
// slots an instance that was predicted cheap and turns out long starts late and sets the kernel time (measured: mean span
// 119 us against 107 us for the slowest instance, profiles/r03_launch_timeline.json); with 768 slots the late starters begin
// when the first instances without iterations leave (~18 us) and finish inside the slowest instance. The sweeps and the set-up
// run on half the threads (+2..3 us per instance), the staging area shrinks to 384 rows (three states in 160 KB).
template <int NV, int CMAX, int NT>
__global__ __launch_bounds__(NT, 2) void k_replan_tri(const hdsm::Consts* __restrict__ cp, hdsm::Args a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  using Sol = hdsm::Solver<NV, CMAX>;
  run_block<Sol>(reinterpret_cast<typename Sol::S*>(smem), cp, a);
}

// FOUR workgroups of 128 threads per CU: every instance of a 1024-agent round is resident at once (1024 slots), so no instance
// starts late behind a short one — in the rounds of the bench window whose instances are all of similar length (five of twenty)
// the three-per-CU launch ended 15-25 us after its slowest instance, set by a late starter. Four instance states fit 160 KB with
// the small LDS layout (Shm<.., SMALL>: 4 polyhedra of <= 20 rows, 512-neighbour chunks) and a staging area of 256 rows (the
// bench rounds stage <= 190; an overflow is re-solved by the rescue pass like for the other shared-CU kernels).
template <int NV, int CMAX, int NT>
__global__ __launch_bounds__(NT, 2) void k_replan_quad(const hdsm::Consts* __restrict__ cp, hdsm::Args a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  using Sol = hdsm::Solver<NV, CMAX, true>;
  run_block<Sol>(reinterpret_cast<typename Sol::S*>(smem), cp, a);
}

// n > 30 (H up to 16): the factor needs more than 256 registers per lane, so a wavefront must have a SIMD to itself — but a
// 128-thread workgroup has only two, and TWO such workgroups (four wavefronts, one per SIMD) fit a CU once the staging area is cut
// to 720 rows (2 x 80 KB of LDS; 736 until round 5 added the per-level child bounds; 320 rows until the butterfly layout freed the
// 19 KB transposition buffer of the old code). Batches larger than the CU count are throughput-bound at one instance per CU (cfg 5:
// 4096 instances, 16 per CU one after the other), and every instance is one latency-bound wavefront: the second one doubles the rate.
// (Until round 6 a second instantiation with 320 rows stayed selectable for the staging-overflow test, HDSM_DUO48_ROWS=320. When the
// last spilled registers of these kernels were removed, THAT instantiation — and only it — began to end feasible instances as
// "infeasible" after two operations, deterministically per build, while builds with a spill, with -O2, with -fwrapv or with device
// printf in the loop gave the oracle's answers; the CPU execution of the same source is right in either wave order. The cause was not
// found — scripts/gpu_r6_overflow_raw.py reproduces it on the sources of that commit — so the product keeps ONE instantiation per
// launch shape, each of which the whole -m gpu suite, the fuzz and the oracle check of the timed rounds run through. The 720 rows
// of this kernel are filled and overflowed on purpose by test_gpu_abi.py::test_staging_overflow_at_each_shared_cu_capacity_is_rescued
// and, in the CPU execution of the source together with the 320-row tuple, by tests/test_wave_shapes.py.)
template <int NV, int CMAX, int NT>
__global__ __launch_bounds__(NT, 1) void k_replan_duo48(const hdsm::Consts* __restrict__ cp, hdsm::Args a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  using Sol = hdsm::Solver<NV, CMAX>;
  run_block<Sol>(reinterpret_cast<typename Sol::S*>(smem), cp, a);
}

// Every row of HDSM_SOLVER_SHAPES as it is launched: the kernel, its workgroup size and its dynamic LDS (the whole instance state).
// hdsm_create raises each kernel's dynamic-LDS limit to its shm once.
using SolverKernel = void (*)(const hdsm::Consts*, hdsm::Args);
struct ShapeLaunch {
  SolverKernel kern;
  int threads;
  size_t shm;
};
#ifdef HDSM_PROFILE  // (the counters of the profile build live in LDS: that build runs at a lower occupancy)
constexpr bool LDS_FIT_CHECK = false;
#else
constexpr bool LDS_FIT_CHECK = true;
#endif
// (per_cu is what SplitState::alloc counts as resident pass-2 workgroups per CU: the state of a one-per-CU kernel, with 64 threads too, is
// held to ONE by being more than half of a CU's 160 KB)
#define HDSM_SHAPE_LAUNCH(name, kernel, nv, cmax, small, threads, per_cu)                                                               \
  static_assert(!LDS_FIT_CHECK || per_cu * sizeof(hdsm::Solver<nv, cmax, small>::S) <= 160 * 1024, #name ": per_cu instances must fit the LDS of one CU"); \
  static_assert(per_cu > 1 || sizeof(hdsm::Solver<nv, cmax, small>::S) > 80 * 1024, #name ": a one-per-CU shape must not fit a CU twice");
HDSM_SOLVER_SHAPES(HDSM_SHAPE_LAUNCH)
#undef HDSM_SHAPE_LAUNCH
#define HDSM_SHAPE_LAUNCH(name, kernel, nv, cmax, small, threads, per_cu) {kernel<nv, cmax, threads>, threads, sizeof(hdsm::Solver<nv, cmax, small>::S)},
const ShapeLaunch SHAPE_LAUNCH[hdsm::NUM_SHAPES] = {HDSM_SOLVER_SHAPES(HDSM_SHAPE_LAUNCH)};
#undef HDSM_SHAPE_LAUNCH

int launch_shape(Handle* h, hdsm::Shape s, const hdsm::Args& a, hipStream_t st, int blocks) {
  const ShapeLaunch& l = SHAPE_LAUNCH[s];
  hipLaunchKernelGGL(l.kern, dim3(blocks), dim3(l.threads), l.shm, st, h->d_consts.get(), a);
  HIP_TRY(hipGetLastError());
  return HDSM_OK;
}

// the execution knobs the choice of shape depends on (hdsm_create settles them)
hdsm::ShapeKnobs shape_knobs(const Handle* h) { return {h->n, h->threads, h->P, h->RS, h->duo_min, h->tri_min, h->quad_min}; }

// ---- subtree splitting: set-up of pass 2, merge, lazily allocated state -------------------------------------------------
// One wavefront per instance that pass 1 handed over: the best answer of its items becomes the instance's answer. `a` holds
// the instance-indexed arrays of the launch, `b` the arrays of pass 2 (indexed by the item's place in the queue).
__global__ __launch_bounds__(64) void k_split_merge(int N, int P, hdsm::Args a, hdsm::Args b) {
  if (blockIdx.x == 0 && threadIdx.x == 0 && b.item_total != nullptr) *b.item_total = a.rec_count[1];  // (sizes the grid of the next split launch)
  hdsm::split_merge(N, P, a, b, (int)blockIdx.x, (int)threadIdx.x, 64);
}

// the one-per-CU kernel (largest staging area) over the batch of `a`; only instances flagged HDSM_FLAG_STAGING_OVERFLOW work
int launch_rescue(Handle* h, const hdsm::Args& a, hipStream_t st) {
  hdsm::Args r = a;
  r.rescue = 1, r.order = nullptr, r.split_budget = 0, r.item_mode = 0, r.split_info = nullptr, r.inc_bits = nullptr, r.node_pool = nullptr;
  r.tree_flag = nullptr, r.tree_mark = 0, r.warm_out = r.warm, r.ovf_flag = nullptr;
  return launch_shape(h, hdsm::pick_shape(shape_knobs(h), r.n_inst, hdsm::PASS_RESCUE), r, st, r.n_inst);
}

}  // namespace

int hdsm_entry::rescue_if_flagged(Handle* h, hipStream_t st) {
  if (h->last_small && h->rescue_ttl == 0) {  // (a launch that already carried the rescue pass needs no second one)
    HIP_TRY(hipStreamSynchronize(st));
    if (*h->ovf_flag.host() != 0) {  // an instance ran out of staging rows in a shared-CU kernel: solve it again now, with the large area
      *h->ovf_flag.host() = 0, h->rescue_ttl = 256;
      return launch_rescue(h, h->last_args, st);
    }
  }
  return HDSM_OK;
}

namespace {

// the eight statistics of a launch, `stride` entries each, in one block
void stat_views(hdsm::Args& a, int32_t* base, size_t stride) {
  a.st_iters = base, a.st_nodes = base + stride, a.st_sweeps = base + 2 * stride, a.st_cand = base + 3 * stride;
  a.st_sph = base + 4 * stride, a.st_pairs = base + 5 * stride;
  a.st_flags = reinterpret_cast<uint32_t*>(base + 6 * stride), a.st_key = base + 7 * stride;
}

int launch(Handle* h, hdsm::Args a, hipStream_t st) {
  hdsm_handle::SplitState& sub = h->sub;
  hdsm_handle::Prepass& pp = h->pre;
  a.scratch = h->d_scratch.get();
  a.scratch_stride = h->scratch_stride;
  stat_views(a, h->d_stats.get(), (size_t)h->max_inst);
  a.prof = h->d_prof.get();
  a.warm = (h->prm.warm_start && a.l1_rows == nullptr) ? h->d_warm.get() : nullptr;
  HIP_TRY(join_stream(h, st));
  h->last_stream = st;
  a.bounds = nullptr, a.pos = nullptr, a.order = nullptr;
  a.range = a.l1_rows == nullptr ? h->range() : nullptr;
  // (the prefilter pays from a number of NEIGHBOURS on: with a partition the largest group, not the buffer. It shapes work, never answers.)
  const bool prefilter = h->prefilter_agents(a.n_rob) >= h->bounds_min;
  const bool ordered = a.warm != nullptr && h->order_min > 0 && a.n_inst >= h->order_min;
  if (ordered) a.order = pp.d_order.get();
  const bool packed = h->defer_done && a.l1_rows == nullptr && pp.plans == a.plans && pp.n_rob == a.n_rob && pp.n_inst == a.n_inst && pp.ordered == ordered;
  pp.plans = nullptr;  // (good for one solve: the plans change with the commit that follows it)
  // Stale plans. The neighbours reach the solver kernels packed (pos / bounds, shifted by the pre-pass) and `plans` is read there for the
  // instance's own record alone: the own-plan override is resolved here, the kernels only choose where the own flag comes from.
  const double* const neigh_plans = a.plans;
  const int32_t* const shift = a.l1_rows == nullptr ? h->shift : nullptr;
  if (a.l1_rows == nullptr && h->own_plans != nullptr) a.plans = h->own_plans, a.own_has = h->own_has;
  // the set-up map of every instance as one product on the matrix cores (k_plan_prepass, setup_map_tile): rides on the pre-pass launch
  SetupMapArgs sm{};
  a.setup = nullptr;
  if (a.l1_rows == nullptr && h->setup_mfma) {
    sm.c = h->d_consts.get(), sm.state = a.state, sm.ref = a.ref, sm.out = pp.d_setup.get(), sm.n_inst = a.n_inst, sm.N = h->N, sm.nk = 3 * h->n + 12;
    sm.row_tiles = (sm.nk + 15) / 16;
    a.setup = pp.d_setup.get();
  }
  const int sm_blocks = sm.out != nullptr ? (sm.row_tiles * ((a.n_inst + 15) / 16) + 3) / 4 : 0;
  if (packed) {
    a.pos = pp.d_pos.get();
    a.bounds = prefilter ? pp.d_bounds.get() : nullptr;
    if (sm_blocks > 0) {  // (the device-resident loop packs the plans elsewhere: the tiles alone)
      sm.first_block = 0;
      hipLaunchKernelGGL(k_plan_prepass, dim3(sm_blocks), dim3(256), 0, st, h->N, 0, neigh_plans, a.has_plan, pp.d_pos.get(), nullptr, 0, a.st_key, a.agent_id, nullptr, sm, shift);
      HIP_TRY(hipGetLastError());
    }
  } else if (a.l1_rows == nullptr) {
    double* const bounds = prefilter ? pp.d_bounds.get() : nullptr;
    sm.first_block = (a.n_rob + 15) / 16 + (ordered ? 1 : 0);
    hipLaunchKernelGGL(k_plan_prepass, dim3(sm.first_block + sm_blocks), dim3(256), 0, st, h->N, a.n_rob, neigh_plans, a.has_plan,
                       pp.d_pos.get(), bounds, a.n_inst, a.st_key, a.agent_id, ordered ? pp.d_order.get() : nullptr, sm, shift);
    HIP_TRY(hipGetLastError());
    a.pos = pp.d_pos.get();
    a.bounds = bounds;
  } else if (ordered) {
    hipLaunchKernelGGL(k_launch_order, dim3(1), dim3(256), 0, st, a.n_inst, a.st_key, a.agent_id, pp.d_order.get());
    HIP_TRY(hipGetLastError());
  }
  // one workgroup per agent-replan. The active-set iteration runs on wave 0 (factorisation in its registers);
  // with 256 threads the other three waves of the CU share the sweeps, the set-up and the leaf test.
  int rc;
  if (h->time_kernel) HIP_TRY(h->kernel_time.record_start(st));
  // `small`: a shape of this launch shares a CU (per_cu > 1), i.e. has a reduced staging area. It follows the shapes actually
  // launched, not the thresholds: with HDSM_DUO_MIN=0 and HDSM_QUAD_MIN / HDSM_TRI_MIN set by hand the two can disagree.
  bool small = false;
  const hdsm::ShapeKnobs knobs = shape_knobs(h);
  auto solve = [&](const hdsm::Args& x, int blocks) -> int {  // the kernel shape that suits `blocks` workgroups
    const hdsm::Shape s = hdsm::pick_shape(knobs, blocks, hdsm::PASS_ORDINARY);
    small = small || hdsm::SHAPES[s].per_cu > 1;
    return launch_shape(h, s, x, st, blocks);
  };
  a.warm_out = a.warm;
  a.tree_flag = h->tree_flag.dev();
  a.ovf_flag = h->ovf_flag.dev(), a.rescue = 0;
  // nodes after which an instance is handed over: small batches leave most CUs idle, so sub-blocks are free; in a batch that
  // fills the GPU every handed-over instance costs poly_hor set-ups and sweeps on busy CUs, so only the deep trees go
  // (measured on MI355X with the hand-over records of round 5 — a hand-over costs about one node, no search is repeated: cfg 3, 256
  // instances, 2 / 4 / 8 / 16 nodes -> 0.65 / 0.70 / 0.84 / 0.93 ms per round; cfg 5, 4096 instances, 16 / 24 / 32 / 48 / 96 nodes ->
  // 8.1 / 8.4 / 8.9 / 9.4 / 11.3 ms)
  const bool roomy = a.n_inst <= 2 * h->cus;
  // (round 6, after the dominance rule made the trees small — cfg 5: 77 k -> 23 k nodes per round: 8 / 8 instead of 16 / 16 for full
  // batches, 4.18 -> 3.51 ms on rounds 8..13 and 7.24 -> 5.86 ms on rounds 30..35, scripts/gpu_r6_cfg5_sweep.sh; cfg 3 is flat in both knobs)
  const int budget = h->split_budget > 0 ? h->split_budget : (roomy ? 2 : 8);
  a.tree_mark = budget > hdsm::TREE_MARK ? budget : hdsm::TREE_MARK;
  // Subtree splitting. A launch lasts as long as its slowest instance, and in obstacle worlds that is one agent between pillars
  // whose branch and bound needs hundreds of nodes while the other workgroups have been idle for milliseconds. When the last
  // launch met such a tree (tree_flag), this one runs in three kernels: (1) the ordinary solve with a small node budget — an
  // instance that exceeds it stops without outputs and records the step its root branched on; (2) poly_hor workgroups per
  // handed-over instance, workgroup j searching the subtree "polyhedron j at that step" (a partition of the search space that
  // does not depend on numerical noise), pruning against the best objective any of them has found (one atomicMin per
  // incumbent); (3) a merge that keeps the best answer. Same answers as the one-kernel form: the search is exact either way.
  bool split = h->split_mode == 1;
  if (h->split_mode == 2) {
    // The word is raised by kernels that may still be running when the next launch is enqueued (callers that queue dozens of
    // rounds back to back see it dozens of launches late), so a sighting keeps the split form on for the next 256 launches:
    // deep trees persist over rounds, and a split launch in which nothing is handed over costs three near-empty kernels.
    if (*h->tree_flag.host() != 0) *h->tree_flag.host() = 0, h->split_ttl = 256;
    if (h->split_ttl > 0) split = true, --h->split_ttl;
  }
  // pass 2 of a split launch: persistent workgroups, as many as fit the GPU at once (per_cu of the shape per CU)
  const hdsm::Shape items = hdsm::pick_shape(knobs, 0, hdsm::PASS_ITEMS);
  if (split && !sub.ready() && sub.alloc(*h, items) != hipSuccess) {  // (allocated by the first split launch)
    (void)hipGetLastError();  // nothing of it is left, the error is cleared: the handle goes on without split launches
    h->split_mode = 0, split = false;
  }
  if (!split) {
    rc = solve(a, a.n_inst);
  } else {
    a.split_budget = budget, a.split_info = sub.d_split.get(), a.tree_mark = 0;  // (a.tree_flag stays: k_split_merge raises it for trees that are still deep)
    a.recs = sub.d_recs.get(), a.rec_cand = sub.d_rec_cand.get(), a.rec_mw = sub.d_rec_mw.get(), a.rec_src = sub.d_rec_src.get();
    a.rec_count = sub.d_rec_count.get(), a.items = sub.d_items.get(), a.item_status = sub.d_sub_status.get();
    a.rec_cap = h->rec_cap, a.rows_cap = sub.rows_cap, a.items_cap = sub.items_cap, a.inc_bits = nullptr, a.node_pool = nullptr;
    // the node budget is the INSTANCE's: every item starts with a small share of what pass 1 left of it and hands the unused part
    // back to the instance's pool when it finishes; an item that has used its share draws from that pool (NODE_CHUNK at a time)
    const int total_nodes = h->prm.max_nodes > 0 ? h->prm.max_nodes : 2000;
    const int left_nodes = total_nodes - budget > 64 ? total_nodes - budget : 64;
    const int node_cap = left_nodes / 128 > 0 ? left_nodes / 128 : 1;
    a.nodes_pool0 = left_nodes, a.node_cap = node_cap;
    HIP_TRY(hipMemsetAsync(sub.d_rec_count.get(), 0, 8 * sizeof(int32_t), st));
    HIP_TRY(hipMemsetAsync(sub.d_slot_busy.get(), 0, (size_t)sub.pool_cap * sizeof(int32_t), st));
    hdsm::Args a1 = a;
    a1.inc_bits = sub.d_inc.get(), a1.node_pool = sub.d_node_pool.get();  // (pass 1 only WRITES them, at a hand-over: its own search runs on Consts::max_nodes)
    rc = solve(a1, a.n_inst);
    if (rc) return rc;
    hdsm::Args b = a;
    b.item_mode = 1, b.order = nullptr, b.inc_bits = sub.d_inc.get(), b.node_pool = sub.d_node_pool.get(), b.tree_flag = nullptr;
    b.traj = sub.d_sub_traj.get(), b.ctrl = sub.d_sub_ctrl.get(), b.used = sub.d_sub_used.get(), b.status = sub.d_sub_status.get(), b.obj = sub.d_sub_obj.get();
    b.scratch = sub.d_sub_scratch.get(), b.warm_out = sub.d_sub_warm.get(), b.prof = nullptr, b.pool_cap = sub.pool_cap, b.slot_busy = sub.d_slot_busy.get();
    b.item_total = h->item_total.dev();
    b.split_budget = h->item_budget;  // an item whose subtree outgrows this many nodes hands over again (0: never)
    // ... or, while workgroups are waiting for items, this many: 2 in a batch that leaves CUs idle (cfg 3: 0.84 ms against 1.14 without),
    // 16 in one that fills the GPU (every look at the queue is two device-scope reads per node: cfg 5 8.15 ms with 2 - 4, 7.5 with >= 8)
    b.split_min = h->item_min > 0 ? h->item_min : (roomy ? 2 : 8);
    b.poll_sleep = h->poll_sleep;
    stat_views(b, sub.d_sub_stats.get(), (size_t)sub.items_cap);
    small = small || hdsm::SHAPES[items].per_cu > 1;
    // the grid: an upper bound of the items of this launch — four times what the last split launch queued (the merge leaves the
    // count in pinned host memory), at least 4096; a launch that outgrows it leaves items pending and their instances end as LIMIT
    int grid = 4096;
    if (4 * *h->item_total.host() > grid) grid = 4 * *h->item_total.host();
    if (grid > sub.items_cap) grid = sub.items_cap;
    rc = launch_shape(h, items, b, st, grid);
    if (rc) return rc;
    hipLaunchKernelGGL(k_split_merge, dim3(a.n_inst), dim3(64), 0, st, h->N, h->P, a, b);
    HIP_TRY(hipGetLastError());
  }
  if (rc) return rc;
  // Staging overflow. The kernels that share a CU have a fraction of the staging rows of the one-per-CU kernel (the CMAX column of
  // hdsm_shapes.h); an instance in a very dense neighbourhood can fill them with VIOLATED rows alone and then ends with
  // HDSM_FLAG_STAGING_OVERFLOW. It raises a word in pinned host memory; while the handle has seen that word in the last 256
  // launches, every launch that used such a kernel is followed by a rescue pass — the one-per-CU kernel over the batch, in
  // which only the instances that carry the flag are solved again (the host-buffer entry point adds it at once, see hdsm_replan).
  h->last_small = small, h->last_args = a;
  if (small) {
    if (*h->ovf_flag.host() != 0) *h->ovf_flag.host() = 0, h->rescue_ttl = 256;
    if (h->rescue_ttl > 0) {
      --h->rescue_ttl;
      rc = launch_rescue(h, a, st);
      if (rc) return rc;
    }
  }
  if (h->time_kernel) HIP_TRY(h->kernel_time.record_stop(st));
  HIP_TRY(mark_done(h, st));
  return HDSM_OK;
}

int64_t scratch_stride_for(int n) {
  return n <= hdsm::SPLIT_N_MAX ? (int64_t)hdsm::Solver<32, hdsm::CMAX30>::SNAP_STRIDE * hdsm::MAXH
                 : (int64_t)hdsm::Solver<48, hdsm::CMAX48>::SNAP_STRIDE * hdsm::MAXH;
}

}  // namespace

extern "C" {

int32_t hdsm_version(void) { return (1 << 16) | 9; }  // 1.2: + hdsm_poly_octa3d_batch_wave / _device_wave, hdsm_set_kernel_timing / hdsm_last_kernel_ms; 1.3: + hdsm_host_register / _unregister; 1.4: + the path step (hdsm_swarm_set_goals / _set_path_period / _replan_paths / _path_errors, hdsm_local_path_batch / _host, hdsm_dswarm_set_goals / _path_stats / _last_path_ms); 1.5: + the path step's clearance mode (hdsm_swarm_set_path_clearance, hdsm_local_path_dmp_batch / _host); 1.6: + the flight audit and the state history (hdsm_flight_audit_host / _batch, hdsm_swarm_set_audit / _get_audit / _audit / _flight_report, hdsm_dswarm_set_audit / _flight_report / _last_audit_round / _last_audit_ms / _set_history / _download_history); 1.7: + map updates in flight (hdsm_map_region_extent / _region_scratch_bytes, hdsm_map_preprocess_region / _region_device, hdsm_swarm_update_world, hdsm_dswarm_update_world / _set_raw_world / _update_world_raw / _update_world_raw_device / _download_world / _world_stats); 1.8: + neighbour groups (hdsm_set_groups, hdsm_swarm_set_groups, hdsm_dswarm_group_report); 1.9: + local ranks (hdsm_comm_create_local, hdsm_dswarm_round_ranks, hdsm_dswarm_download_raw)

const char* hdsm_last_error(void) { return g_err.c_str(); }

void hdsm_default_params(hdsm_params* p, int32_t n_hor) {
  if (!p) return;
  std::memset(p, 0, sizeof *p);
  // multi_agent_planner/config/agent_agile_config.yaml -> InitializePlannerParameters (AC:2169-2188)
  p->n_hor = n_hor, p->poly_hor = 4, p->rk4 = 0, p->max_rows_static = 18;
  p->dt = 0.1, p->r_u = 0.01;
  const double w[9] = {100, 100, 100, 1, 1, 1, 0, 0, 0};
  for (int k = 0; k < 9; ++k) p->r_x[k] = p->r_n[k] = w[k];
  const double max_vel = 20.0, max_acc = 15.0, max_jerk = 60.0;
  for (int k = 0; k < 3; ++k) {
    p->x_lb[k] = -HDSM_INF, p->x_ub[k] = HDSM_INF;
    p->x_lb[3 + k] = -max_vel, p->x_ub[3 + k] = max_vel;
    p->x_lb[6 + k] = -max_acc, p->x_ub[6 + k] = max_acc;
    p->u_lb[k] = -max_jerk, p->u_ub[k] = max_jerk;
  }
  p->drone_radius = 0.25, p->drone_z_offset = 0.25, p->plane_perturb = 0.1;
  p->max_nodes = 0, p->max_qp_iters = 0, p->feas_tol_fixed = 1e-6, p->solver_tol = 1e-9;
  p->warm_start = 1;  // execution knobs and time_limit_s stay 0 = library defaults / no wall-clock limit
}

int hdsm_create(const hdsm_params* params, int32_t max_instances, int32_t n_rob_max, int32_t device,
                void** handle) {
  if (!params || !handle) return set_err(HDSM_ERR_BAD_ARG, "null argument");
  if (max_instances < 1 || n_rob_max < 1) return set_err(HDSM_ERR_BAD_ARG, "max_instances/n_rob_max must be >= 1");
  *handle = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return set_err(HDSM_ERR_NO_DEVICE, "no HIP device: this library has no CPU fallback");
  if (device < 0 || device >= ndev) return set_err(HDSM_ERR_NO_DEVICE, "device ordinal out of range");
  HIP_TRY(hipSetDevice(device));

  std::unique_ptr<hdsm::Consts> hc(new (std::nothrow) hdsm::Consts);
  if (!hc) return set_err(HDSM_ERR_DEVICE, "out of host memory");
  const char* msg = nullptr;
  if (int rc = hdsm::build_consts(params, hc.get(), &msg)) return set_err(rc, msg ? msg : "bad params");
  std::unique_ptr<Handle> h(new (std::nothrow) Handle);
  if (!h) return set_err(HDSM_ERR_DEVICE, "out of host memory");
  h->device = device, h->max_inst = max_instances, h->n_rob_max = n_rob_max, h->prm = *params;
  h->N = hc->N, h->P = hc->P, h->RS = hc->RS, h->n = hc->n;
  // execution knobs: hdsm_params, then the environment (scripts); out-of-range values are ignored
  auto env_int = [](const char* name, long lo, long hi, int* out) {
    if (const char* e = std::getenv(name)) {
      char* end = nullptr;
      const long v = std::strtol(e, &end, 10);
      if (end != e && *end == 0 && v >= lo && v <= hi) *out = (int)v;
    }
  };
  if (params->threads_per_instance == 64 || params->threads_per_instance == 256) h->threads = params->threads_per_instance;
  {
    int t = h->threads;
    env_int("HDSM_THREADS", 64, 256, &t);
    if (t == 64 || t == 256) h->threads = t;
  }
  h->bounds_min = params->prefilter_min_agents > 0 ? params->prefilter_min_agents : (params->prefilter_min_agents < 0 ? INT_MAX : 256);
  env_int("HDSM_BOUNDS_MIN", 1, INT_MAX, &h->bounds_min);
  {
    hipDeviceProp_t prop;
    const int cus = (hipGetDeviceProperties(&prop, device) == hipSuccess) ? prop.multiProcessorCount : 256;
    h->cus = cus;
    h->duo_min = params->duo_min_instances > 0 ? params->duo_min_instances : (params->duo_min_instances < 0 ? 0 : cus + 1);
    env_int("HDSM_DUO_MIN", 0, INT_MAX, &h->duo_min);  // 0 = never
    h->tri_min = h->duo_min > 0 ? 2 * cus + 1 : 0;     // more instances than the two-per-CU kernel has resident slots
    env_int("HDSM_TRI_MIN", 0, INT_MAX, &h->tri_min);  // 0 = never
    h->quad_min = h->tri_min > 0 ? 3 * cus + 1 : 0;    // more instances than the three-per-CU kernel has resident slots
    env_int("HDSM_QUAD_MIN", 0, INT_MAX, &h->quad_min);  // 0 = never
    env_int("HDSM_SETUP_MFMA", 0, 1, &h->setup_mfma);
    env_int("HDSM_SPLIT", 0, 2, &h->split_mode);       // subtree splitting: 0 never, 1 always, 2 (default) when the last launch met a deep tree
    env_int("HDSM_SPLIT_BUDGET", 1, 100000, &h->split_budget);  // (unset: by batch size, see launch())
    env_int("HDSM_ITEM_BUDGET", 0, 100000, &h->item_budget);    // pass 2: nodes after which an item hands over again (32; 0 = never)
    env_int("HDSM_ITEM_MIN", 1, 100000, &h->item_min);          // ... or, while workgroups wait for items, this many (unset: by batch size)
    env_int("HDSM_POLL_SLEEP", 1, 1000, &h->poll_sleep);
    h->rec_cap = 8 * max_instances < 256 ? 256 : (8 * max_instances > 2048 ? 2048 : 8 * max_instances);
    env_int("HDSM_SPLIT_RECORDS", 1, 1 << 20, &h->rec_cap);
    // more instances than can be resident at once (two workgroups per CU): launch the expensive ones first
    h->order_min = params->launch_order == 0 ? 2 * cus + 1 : (params->launch_order < 0 ? 0 : params->launch_order);
    env_int("HDSM_ORDER_MIN", 0, INT_MAX, &h->order_min);  // 0 = never
  }
  if (params->time_limit_s > 0) {
    int khz = 0;
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device) != hipSuccess || khz <= 0) khz = 100000;
    hc->time_ticks = (long long)(params->time_limit_s * 1e3 * (double)khz);
    if (hc->time_ticks < 1) hc->time_ticks = 1;
  }
  h->scratch_stride = scratch_stride_for(h->n);
  hdsm_mem::FirstError ok;
  for (const ShapeLaunch& l : SHAPE_LAUNCH)  // (the instance state of most shapes is more than the default 64 KB of dynamic LDS)
    ok(hipFuncSetAttribute(reinterpret_cast<const void*>(l.kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)l.shm));
  if (ok.ok()) ok(h->alloc_fixed());
  if (ok.ok()) ok(hipMemcpy(h->d_consts.get(), hc.get(), sizeof *hc, hipMemcpyHostToDevice));
  if (!ok.ok()) return set_err(HDSM_ERR_DEVICE, std::string("hdsm_create: ") + hipGetErrorString(ok.e));
  *handle = h.release();
  return HDSM_OK;
}

void hdsm_destroy(void* handle) {
  Handle* h = static_cast<Handle*>(handle);
  if (!h) return;
  (void)hipSetDevice(h->device);
  (void)hipDeviceSynchronize();
  delete h;
}

int hdsm_replan_device(void* handle, int32_t n_inst, int32_t n_rob, const int32_t* agent_id,
                       const double* state_curr, const double* traj_ref, const int32_t* n_poly,
                       const int32_t* n_rows_static, const double* A_static, const double* b_static,
                       const double* plans_all, const uint8_t* has_plan, double* traj_out,
                       double* ctrl_out, uint8_t* poly_used, int32_t* status, double* obj,
                       void* hip_stream) {
  Handle* h = static_cast<Handle*>(handle);
  if (int rc = check_neighbours(h, n_inst, n_rob)) return rc;
  if (n_inst == 0) return HDSM_OK;
  if (!agent_id || !state_curr || !traj_ref || !n_poly || !n_rows_static || !A_static || !b_static ||
      !plans_all || !has_plan || !traj_out || !ctrl_out || !poly_used || !status || !obj)
    return set_err(HDSM_ERR_BAD_ARG, "null array argument");
  if (traj_out == plans_all) return set_err(HDSM_ERR_BAD_ARG, "traj_out must not alias plans_all");
  HIP_TRY(hipSetDevice(h->device));
  hdsm::Args a{};
  a.n_inst = n_inst, a.n_rob = n_rob, a.agent_id = agent_id, a.state = state_curr, a.ref = traj_ref;
  a.n_poly = n_poly, a.n_rows = n_rows_static, a.A = A_static, a.b = b_static, a.plans = plans_all;
  a.has_plan = has_plan, a.traj = traj_out, a.ctrl = ctrl_out, a.used = poly_used, a.status = status;
  a.obj = obj;
  return launch(h, a, static_cast<hipStream_t>(hip_stream));
}

int hdsm_tasc_planes(void* handle, int32_t n_inst, int32_t n_rob, const int32_t* agent_id,
                     const double* state_curr, const double* plans_all, const uint8_t* has_plan,
                     double* planes) {
  Handle* h = static_cast<Handle*>(handle);
  if (int rc = check_neighbours(h, n_inst, n_rob)) return rc;
  if (n_inst == 0 || n_rob == 0) return HDSM_OK;
  if (!agent_id || !state_curr || !plans_all || !has_plan || !planes)
    return set_err(HDSM_ERR_BAD_ARG, "null array argument");
  HIP_TRY(hipSetDevice(h->device));
  const size_t I = (size_t)n_inst, N = (size_t)h->N;
  const size_t total = I * N * (size_t)n_rob * 4;
  hdsm_handle::HostStaging& s = h->stage;
  hipStream_t st = h->stream.get();
  HIP_TRY(s.planes.ensure(total, st));
  HIP_TRY(join_stream(h, st));  // staging buffers are shared
  Copies cp{st};
  cp(s.d_agent.get(), agent_id, I * 4, hipMemcpyHostToDevice);
  cp(s.d_state.get(), state_curr, I * 9 * 8, hipMemcpyHostToDevice);
  cp(s.d_plans.get(), plans_all, (size_t)n_rob * (N + 1) * 9 * 8, hipMemcpyHostToDevice);
  cp(s.d_has.get(), has_plan, (size_t)n_rob, hipMemcpyHostToDevice);
  if (cp.err.ok()) {
    const int64_t items = (int64_t)(total / 4);
    const int blocks = (int)((items + 255) / 256 > 4096 ? 4096 : (items + 255) / 256);
    hipLaunchKernelGGL(k_tasc_planes, dim3(blocks), dim3(256), 0, st, h->d_consts.get(), n_inst, n_rob, s.d_agent.get(),
                       s.d_state.get(), s.d_plans.get(), s.d_has.get(), s.planes.get(), h->range(), h->shift,
                       h->own_plans != nullptr ? h->own_plans : s.d_plans.get(),
                       h->own_plans != nullptr && h->own_has != nullptr ? h->own_has : s.d_has.get());
    cp.err(hipGetLastError());
  }
  cp(planes, s.planes.get(), total * 8, hipMemcpyDeviceToHost);
  if (cp.err.ok()) cp.err(hipStreamSynchronize(st));
  if (!cp.err.ok()) return set_err(HDSM_ERR_DEVICE, std::string("hdsm_tasc_planes: ") + hipGetErrorString(cp.err.e));
  return HDSM_OK;
}

// Neighbour groups. The partition becomes a per-agent table [n_rob_max][2] = (lo, hi) of the agent's id range, (0, 0) behind the
// partition: a workgroup reads its two bounds with the inputs of its instance (hdsm_core.h, the set-up) and the loops that run over
// the other agents run over [lo, hi) instead of [0, n_rob) (hdsm_wave_gi.h sweep_planes, k_tasc_planes, k_reference).
int hdsm_set_groups(void* handle, int32_t n_groups, const int32_t* group_start) {
  Handle* h = static_cast<Handle*>(handle);
  if (!h) return set_err(HDSM_ERR_BAD_ARG, "null handle");
  if (n_groups < 0) return set_err(HDSM_ERR_BAD_ARG, "hdsm_set_groups: negative n_groups");
  const bool none = n_groups == 0 || group_start == nullptr;
  int gmax = 0;
  if (!none) {
    if (group_start[0] != 0) return set_err(HDSM_ERR_BAD_ARG, "hdsm_set_groups: group_start[0] must be 0");
    for (int g = 0; g < n_groups; ++g) {
      if (group_start[g + 1] <= group_start[g]) return set_err(HDSM_ERR_BAD_ARG, "hdsm_set_groups: group_start must be strictly increasing");
      if (group_start[g + 1] - group_start[g] > gmax) gmax = group_start[g + 1] - group_start[g];
    }
    if (group_start[n_groups] > h->n_rob_max) return set_err(HDSM_ERR_BAD_ARG, "hdsm_set_groups: more agents than n_rob_max of the handle");
  }
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipDeviceSynchronize());
  h->pre.plans = nullptr;  // (a pre-pass of before the change is not this partition's)
  if (none) {
    h->n_total = 0, h->group_max = 0;
    return HDSM_OK;
  }
  std::vector<int32_t> table((size_t)h->n_rob_max * 2, 0);
  for (int g = 0; g < n_groups; ++g)
    for (int k = group_start[g]; k < group_start[g + 1]; ++k) table[2 * (size_t)k] = group_start[g], table[2 * (size_t)k + 1] = group_start[g + 1];
  h->n_total = 0;
  if (!h->d_range) HIP_TRY(h->d_range.alloc(table.size()));
  HIP_TRY(hipMemcpy(h->d_range.get(), table.data(), table.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  h->n_total = group_start[n_groups], h->group_max = gmax;
  return HDSM_OK;
}

// Stale plans (include/hdsm.h). The three setters only say where the launches that follow read from; each of them makes the handle's
// cached pre-pass (Prepass::plans) invalid, because what was packed before the change is not this view's.
int hdsm_set_plan_shift(void* handle, int32_t n_rob, const int32_t* shift) {
  Handle* h = static_cast<Handle*>(handle);
  if (!h) return set_err(HDSM_ERR_BAD_ARG, "null handle");
  if (n_rob < 0 || n_rob > h->n_rob_max) return set_err(HDSM_ERR_BAD_ARG, "hdsm_set_plan_shift: n_rob out of range");
  const bool none = n_rob == 0 || shift == nullptr;
  std::vector<int32_t> table((size_t)h->n_rob_max, 0);
  for (int k = 0; !none && k < n_rob; ++k) {
    if (shift[k] < 0) return set_err(HDSM_ERR_BAD_ARG, "hdsm_set_plan_shift: negative shift");
    table[(size_t)k] = shift[k] > h->N ? h->N : shift[k];
  }
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipDeviceSynchronize());
  h->pre.plans = nullptr, h->shift = nullptr;
  if (none) return HDSM_OK;
  if (!h->d_shift) HIP_TRY(h->d_shift.alloc(table.size()));
  HIP_TRY(hipMemcpy(h->d_shift.get(), table.data(), table.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  h->shift = h->d_shift.get();
  return HDSM_OK;
}

int hdsm_set_plan_shift_device(void* handle, const int32_t* d_shift) {
  Handle* h = static_cast<Handle*>(handle);
  if (!h) return set_err(HDSM_ERR_BAD_ARG, "null handle");
  h->pre.plans = nullptr, h->shift = d_shift;
  return HDSM_OK;
}

int hdsm_set_own_plans_device(void* handle, const double* d_own_plans, const uint8_t* d_own_has) {
  Handle* h = static_cast<Handle*>(handle);
  if (!h) return set_err(HDSM_ERR_BAD_ARG, "null handle");
  if (d_own_plans == nullptr && d_own_has != nullptr) return set_err(HDSM_ERR_BAD_ARG, "hdsm_set_own_plans_device: flags without plans");
  h->pre.plans = nullptr, h->own_plans = d_own_plans, h->own_has = d_own_has;
  return HDSM_OK;
}

int hdsm_reset_warm_start(void* handle) {
  Handle* h = static_cast<Handle*>(handle);
  if (!h) return set_err(HDSM_ERR_BAD_ARG, "null handle");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemset(h->d_warm.get(), 0, (size_t)(hdsm::MAXNV + 2) * h->max_inst * sizeof(int32_t)));
  return HDSM_OK;
}

// Internal (csrc/swarm_kernels.hip; not in include/): the device-resident loop issues its whole round on one stream and says so
// (defer_done: the pre-pass of its solve rides on the reference kernel); at the end of the round it names the point a later call on
// ANOTHER stream has to wait for. (Until the done event became lazy — hdsm_entry.h, join_stream — every device entry point recorded
// it, a barrier packet in front of the next kernel, and this pair existed to leave one record per round instead of one per call.)
extern "C" int hdsm_internal_defer_done(void* handle, int on) {
  Handle* h = static_cast<Handle*>(handle);
  if (!h) return HDSM_ERR_BAD_ARG;
  h->defer_done = on != 0;
  return HDSM_OK;
}
extern "C" int hdsm_internal_record_done(void* handle, void* hip_stream) {
  Handle* h = static_cast<Handle*>(handle);
  if (!h) return HDSM_ERR_BAD_ARG;
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  if (h->launched && st == h->last_stream) {  // the tail of last_stream at the next join is at or after this point
    h->done_pending = true;
    return HDSM_OK;
  }
  HIP_TRY(hipEventRecord(h->ev_done.get(), st));  // (a stream the handle has not launched on: as before)
  return HDSM_OK;
}

int hdsm_set_kernel_timing(void* handle, int32_t on) {
  Handle* h = static_cast<Handle*>(handle);
  if (!h) return set_err(HDSM_ERR_BAD_ARG, "null handle");
  h->time_kernel = on != 0;
  if (!h->time_kernel) h->kernel_time.valid = false;
  return HDSM_OK;
}

int hdsm_last_kernel_ms(void* handle, float* ms) {
  Handle* h = static_cast<Handle*>(handle);
  if (!h || !ms) return set_err(HDSM_ERR_BAD_ARG, "null argument");
  if (!h->kernel_time.valid) return set_err(HDSM_ERR_BAD_ARG, "no launch since hdsm_set_kernel_timing(handle, 1)");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(h->kernel_time.ms(ms));
  return HDSM_OK;
}

#ifdef HDSM_TIMELINE
// development aid: the launch seen from the instances (100 MHz clock): span, the slowest instance, late starters
static int print_timeline(Handle* h, int32_t n_inst) {
  std::vector<long long> pr((size_t)n_inst * 32);
  HIP_TRY(hipMemcpy(pr.data(), h->d_prof.get(), pr.size() * sizeof(long long), hipMemcpyDeviceToHost));
  long long t0 = pr[0], t1 = pr[1];
  int worst = 0, last = 0;
  double busy = 0;
  for (int k = 0; k < n_inst; ++k) {
    const long long b = pr[(size_t)k * 32], e = pr[(size_t)k * 32 + 1];
    if (b < t0) t0 = b;
    if (e > t1) t1 = e, last = k;
    if (e - b > pr[(size_t)worst * 32 + 1] - pr[(size_t)worst * 32]) worst = k;
    busy += (double)(e - b);
  }
  int late = 0;
  for (int k = 0; k < n_inst; ++k) late += pr[(size_t)k * 32] - t0 > 200;  // started more than 2 us after the first
  if (const char* path = std::getenv("HDSM_TIMELINE_DUMP")) {  // raw rows for offline analysis, one block per launch
    if (FILE* f = std::fopen(path, "ab")) {
      const long long head[2] = {0x54494d454c494e33LL, n_inst};  // ("TIMELIN3": 32 entries per instance)
      std::fwrite(head, sizeof(long long), 2, f);
      for (int k = 0; k < n_inst; ++k) std::fwrite(&pr[(size_t)k * 32], sizeof(long long), 32, f);
      std::fclose(f);
    }
  }
  auto us = [](long long ticks) { return (double)ticks * 0.01; };
  const long long *w = &pr[(size_t)worst * 32], *l = &pr[(size_t)last * 32];
  std::fprintf(stderr,
               "HDSM_TIMELINE span %.2f us | slowest inst %d: %.2f us, start +%.2f, block %lld, iters %lld nodes %lld sweeps %lld staged %lld+%lld flags %lld status %lld | last to finish inst %d: "
               "start +%.2f dur %.2f block %lld iters %lld | %d of %d started > 2 us late | sum of instance times %.1f us (%.2f per span-slot of 512)\n",
               us(t1 - t0), worst, us(w[1] - w[0]), us(w[0] - t0), w[2], w[4], w[5], w[6], w[7], w[9], w[8], w[10], last, us(l[0] - t0), us(l[1] - l[0]), l[2], l[4], late,
               n_inst, us((long long)busy), busy / (double)(t1 - t0) / 512.0);
  return HDSM_OK;
}
#endif
#ifdef HDSM_PROFILE
// development aid: phase cycle counters of the slowest instance and the batch mean
static int print_profile(Handle* h, int32_t n_inst) {
  std::vector<long long> pr((size_t)n_inst * 32);
  HIP_TRY(hipMemcpy(pr.data(), h->d_prof.get(), pr.size() * sizeof(long long), hipMemcpyDeviceToHost));
  int worst = 0;
  double mean[32] = {0};
  for (int k = 0; k < n_inst; ++k) {
    if (pr[(size_t)k * 32 + 11] > pr[(size_t)worst * 32 + 11]) worst = k;
    for (int j = 0; j < 32; ++j) mean[j] += (double)pr[(size_t)k * 32 + j] / n_inst;
  }
  static const char* nm[32] = {"states", "select", "normal", "d", "sums", "upd", "add", "drop", "setup", "sweep",
                               "leaf", "TOTAL", "iters", "sweeps", "warm_ops", "warm_cycles", "sw_cull", "sw_filter",
                               "sw_load", "sw_body", "sw_tail", "su_stage", "su_grad", "su_fact",
                               "w_prep", "w_fetch", "w_normal", "w_dir", "w_add", "w_pair", "w_drop", "w_7"};
#ifdef HDSM_PROF_OP  // record 16..31 = slots 8..23: the inside of a regular operation (OP_PROF in hdsm_wave_gi.h / hdsm_wave_gib.h)
  static const char* op_nm[16] = {"sel_boxes", "sel_rows", "w0_wait_done", "normal_entry", "d_reduce", "d_sums", "d_gather_z", "d_urow", "add_scalars", "add_gather",
                                  "add_update", "sc_states", "sc_rows", "sc_max", "sc_normal", "sc_wait_go"};
  for (int j = 0; j < 16; ++j) nm[16 + j] = op_nm[j];
#endif
  std::fprintf(stderr, "HDSM_PROFILE worst inst %d:", worst);
  for (int j = 0; j < 32; ++j) std::fprintf(stderr, " %s=%lld", nm[j], pr[(size_t)worst * 32 + j]);
  std::fprintf(stderr, "\nHDSM_PROFILE mean:");
  for (int j = 0; j < 32; ++j) std::fprintf(stderr, " %s=%.0f", nm[j], mean[j]);
  std::fprintf(stderr, "\n");
  return HDSM_OK;
}
#endif

int hdsm_last_stats(void* handle, int32_t n_inst, int32_t* qp_iters, int32_t* nodes, int32_t* sweeps,
                    int32_t* cand) {
  Handle* h = static_cast<Handle*>(handle);
  if (int rc = check_common(h, n_inst, 0)) return rc;
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipStreamSynchronize(h->last_stream));
#ifdef HDSM_TIMELINE
  if (int rc = print_timeline(h, n_inst)) return rc;
#endif
#ifdef HDSM_PROFILE
  if (int rc = print_profile(h, n_inst)) return rc;
#endif
  int32_t* dst[4] = {qp_iters, nodes, sweeps, cand};
  for (int k = 0; k < 4; ++k)
    if (dst[k])
      HIP_TRY(hipMemcpy(dst[k], h->d_stats.get() + (size_t)k * h->max_inst, (size_t)n_inst * 4, hipMemcpyDeviceToHost));
  return HDSM_OK;
}

int hdsm_solve(void* handle, int32_t n_inst, int32_t r_max, const double* state_curr,
               const double* traj_ref, const int32_t* n_poly, const int32_t* n_rows, const double* A,
               const double* b, double* traj_out, double* ctrl_out, uint8_t* poly_used, int32_t* status,
               double* obj) {
  Handle* h = static_cast<Handle*>(handle);
  if (int rc = check_common(h, n_inst, 0)) return rc;
  if (n_inst == 0) return HDSM_OK;
  if (!state_curr || !traj_ref || !n_poly || !n_rows || !A || !b || !traj_out || !ctrl_out || !poly_used || !status || !obj)
    return set_err(HDSM_ERR_BAD_ARG, "null array argument");
  hdsm::Level1Split sp;
  const char* msg = nullptr;
  if (int rc = hdsm::level1_split(h->prm, n_inst, r_max, n_poly, n_rows, A, b, &sp, &msg))
    return set_err(rc, msg ? msg : "bad level-1 input");
  HIP_TRY(hipSetDevice(h->device));
  const size_t I = (size_t)n_inst, N = (size_t)h->N, P = (size_t)h->P, RS = (size_t)h->RS;
  hdsm_handle::HostStaging& s = h->stage;
  hipStream_t st = h->stream.get();
  HIP_TRY(s.common.ensure(sp.common.size(), st));
  Copies cp{st};
  cp.err(s.ncommon.ensure(sp.n_common.size(), st));
  if (cp.err.ok()) cp.err(join_stream(h, st));
  const auto H2D = hipMemcpyHostToDevice;
  const auto D2H = hipMemcpyDeviceToHost;
  std::vector<int32_t> ids(I, -1);
  cp(s.common.get(), sp.common.data(), sp.common.size() * 8, H2D);
  cp(s.ncommon.get(), sp.n_common.data(), sp.n_common.size() * 4, H2D);
  cp(s.d_agent.get(), ids.data(), I * 4, H2D);
  cp(s.d_state.get(), state_curr, I * 9 * 8, H2D);
  cp(s.d_ref.get(), traj_ref, I * N * 6 * 8, H2D);
  cp(s.d_npoly.get(), sp.n_poly.data(), I * 4, H2D);
  cp(s.d_nrows.get(), sp.n_rows_static.data(), I * P * 4, H2D);
  cp(s.d_A.get(), sp.A_static.data(), I * P * RS * 3 * 8, H2D);
  cp(s.d_b.get(), sp.b_static.data(), I * P * RS * 8, H2D);
  cp(s.d_traj.get(), traj_out, I * (N + 1) * 9 * 8, H2D);
  cp(s.d_ctrl.get(), ctrl_out, I * N * 3 * 8, H2D);
  cp(s.d_used.get(), poly_used, I * P, H2D);
  cp(s.d_obj.get(), obj, I * 8, H2D);
  int rc = HDSM_OK;
  if (cp.err.ok()) {
    hdsm::Args a{};
    a.n_inst = n_inst, a.n_rob = 0, a.agent_id = s.d_agent.get(), a.state = s.d_state.get(), a.ref = s.d_ref.get();
    a.n_poly = s.d_npoly.get(), a.n_rows = s.d_nrows.get(), a.A = s.d_A.get(), a.b = s.d_b.get(), a.plans = s.d_plans.get();
    a.has_plan = h->d_zero.get(), a.traj = s.d_traj.get(), a.ctrl = s.d_ctrl.get(), a.used = s.d_used.get(), a.status = s.d_status.get();
    a.obj = s.d_obj.get(), a.l1_rows = s.common.get(), a.l1_nrows = s.ncommon.get(), a.l1_rmax = sp.rc_max;
    rc = launch(h, a, st);
  }
  cp(traj_out, s.d_traj.get(), I * (N + 1) * 9 * 8, D2H);
  cp(ctrl_out, s.d_ctrl.get(), I * N * 3 * 8, D2H);
  cp(poly_used, s.d_used.get(), I * P, D2H);
  cp(status, s.d_status.get(), I * 4, D2H);
  cp(obj, s.d_obj.get(), I * 8, D2H);
  if (cp.err.ok()) cp.err(hipStreamSynchronize(st));
  if (rc) return rc;
  if (!cp.err.ok()) return set_err(HDSM_ERR_DEVICE, std::string("hdsm_solve: ") + hipGetErrorString(cp.err.e));
  return HDSM_OK;
}

int hdsm_last_sweep_stats(void* handle, int32_t n_inst, int32_t* sphere_records, int32_t* pairs, uint32_t* flags) {
  Handle* h = static_cast<Handle*>(handle);
  if (int rc = check_common(h, n_inst, 0)) return rc;
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipStreamSynchronize(h->last_stream));
  void* dst[3] = {sphere_records, pairs, flags};
  for (int k = 0; k < 3; ++k)
    if (dst[k])
      HIP_TRY(hipMemcpy(dst[k], h->d_stats.get() + (size_t)(4 + k) * h->max_inst, (size_t)n_inst * 4, hipMemcpyDeviceToHost));
  return HDSM_OK;
}

}  // extern "C"
