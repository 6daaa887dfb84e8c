// assign_kernels.hip — formations (assign_core.h) on the device, for hdsm_assign_batch and hdsm_dswarm_assign:
//   k_assign   one workgroup per neighbour group, one thread per bidder and per object (64 .. 1024 threads, from the launch's largest
//              m). Slot coordinates, bidder positions, prices, the bids' keys, owners and the list of unassigned bidders live in LDS
//              (82 KB at any size; one workgroup per CU). An iteration: every unassigned bidder is served by ONE wavefront — its 64
//              lanes scan the objects strided, each keeping its best value, index and second best, a butterfly joins them with the tie
//              rule, and lane 0 lands the bid with one 64-bit LDS max of (bid << 10 | 1023 - bidder); behind a barrier the thread of
//              every object that received bids awards and unseats; behind another the unassigned bidders are compacted by ballot and
//              prefix count, so the long tail of iterations with a few bidders costs one short wavefront each and the other
//              wavefronts only meet the barriers. Costs are recomputed from the coordinates at every visit (a cache of m * m int64 has
//              no room on chip). No scratch, no global atomics; the loop is bounded by the budget of iterations.
// The arithmetic is assign_core.h's, the same source as the host form; nothing depends on which wavefront serves which bidder.
#include <hip/hip_runtime.h>

#include "../../include/hdsm_swarm.h"
#include "assign_core.h"
#include "assign_device.h"
#include "device_mem.h"
#include "hdsm_internal.h"

namespace hdsm_assign {
namespace {

__device__ inline Scan scan_shfl_xor(const Scan& s, int mask) {
  return Scan{__shfl_xor(s.best, mask, 64), __shfl_xor(s.second, mask, 64), __shfl_xor(s.j, mask, 64)};
}

__global__ __launch_bounds__(1024) void k_assign(Launch a) {
  __shared__ double sx[MAX_M], sy[MAX_M], sz[MAX_M], bx[MAX_M], by[MAX_M], bz[MAX_M];
  __shared__ long long price[MAX_M];
  __shared__ unsigned long long key[MAX_M];
  __shared__ int owner[MAX_M], has[MAX_M], ulist[MAX_M], aidx[MAX_M];
  __shared__ int wcnt[16];
  __shared__ unsigned long long cmax_s, cost_s;
  __shared__ int flag_s;

  const int g = (int)blockIdx.x, t = (int)threadIdx.x, T = (int)blockDim.x, lane = t & 63, wave = t >> 6, W = T >> 6;
  const int lo = a.gstart[g], hi = a.gstart[g + 1];
  const unsigned long long below = (1ull << lane) - 1ull;
  if (t == 0) cmax_s = 0, cost_s = 0, flag_s = OPTIMAL;

  // the group's active agents, in ascending order; the others are told so
  int m = 0;
  for (int base = lo; base < hi; base += T) {
    const int k = base + t;
    const bool in = k < hi, act = in && k < a.n_on && (a.active == nullptr || a.active[k] != 0);
    const unsigned long long mask = __ballot(act);
    if (lane == 0) wcnt[wave] = __popcll(mask);
    __syncthreads();
    int before = 0, total = 0;
    for (int w = 0; w < W; ++w) {
      const int c = wcnt[w];
      before += w < wave ? c : 0, total += c;
    }
    const int at = m + before + __popcll(mask & below);
    if (act && at < MAX_M) aidx[at] = k;
    if (in && !act) {
      a.slot_of[k] = -1;
      if (a.price != nullptr) a.price[k] = 0;
    }
    m += total;
    __syncthreads();
  }
  m = m < MAX_M ? m : MAX_M;  // (the host refuses a larger group before the launch)

  if (t < m) {
    const int k = aidx[t];
    double p[3];
    const double* src = a.agents != nullptr ? a.agents[k].state_curr : a.pos + 3 * (size_t)k;
    p[0] = src[0], p[1] = src[1], p[2] = src[2];
    if (!finite3(p)) flag_s = NOT_FINITE;
    bx[t] = p[0], by[t] = p[1], bz[t] = p[2];
    sx[t] = a.slots[3 * (size_t)k], sy[t] = a.slots[3 * (size_t)k + 1], sz[t] = a.slots[3 * (size_t)k + 2];
    price[t] = 0, key[t] = 0, has[t] = t;
  }
  __syncthreads();
  int status = flag_s;
  const double inv_q2 = a.rule.inv_q2;
  const long long M1 = m + 1;
  long long iters = 0, bids = 0;
  int phases = 0;

  if (status == OPTIMAL && m > 0) {
    {  // the largest cost: thread i over the objects, one LDS max per wavefront
      long long c = 0;
      if (t < m) {
        const double px = bx[t], py = by[t], pz = bz[t];
        for (int j = 0; j < m; ++j) {
          const long long cj = cost(px, py, pz, sx[j], sy[j], sz[j], inv_q2);
          c = cj > c ? cj : c;
        }
      }
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) {
        const long long o = __shfl_xor(c, off, 64);
        c = o > c ? o : c;
      }
      if (lane == 0 && c > 0) atomicMax(&cmax_s, (unsigned long long)c);
      __syncthreads();
    }
    const long long max_iters = budget(a.rule.max_iters, m), limit = a.rule.bid_limit;
    for (long long eps = eps_first((long long)cmax_s, m);; eps = eps_next(eps)) {
      if (t < m) owner[t] = -1, has[t] = -1, ulist[t] = t;
      int nb = m;
      __syncthreads();
      while (nb > 0) {
        if (iters == max_iters) {
          status = BUDGET;
          break;
        }
        iters += 1, bids += nb;
        for (int b = wave; b < nb; b += W) {  // one wavefront per unassigned bidder, on the prices of the iteration's start
          const int i = ulist[b];
          const double px = bx[i], py = by[i], pz = bz[i];
          Scan s = scan_identity();
          for (int j = lane; j < m; j += 64) scan_add(s, -cost(px, py, pz, sx[j], sy[j], sz[j], inv_q2) * M1 - price[j], j);
#pragma unroll
          for (int off = 32; off >= 1; off >>= 1) s = scan_join(s, scan_shfl_xor(s, off));
          if (lane == 0) {
            const long long bid = bid_of(s, price[s.j], eps, m);
            if (bid >= limit) flag_s = BID_OVERFLOW;
            else atomicMax(&key[s.j], key_of(bid, i));
          }
        }
        __syncthreads();
        if (t < m) {  // the awards: object t takes its highest bid and unseats its owner
          const unsigned long long k = key[t];
          if (k != 0) {
            const int i = key_bidder(k), prev = owner[t];
            if (prev >= 0) has[prev] = -1;
            owner[t] = i, has[i] = t, price[t] = key_bid(k), key[t] = 0;
          }
        }
        __syncthreads();
        const bool un = t < m && has[t] < 0;
        const unsigned long long mask = __ballot(un);
        if (lane == 0) wcnt[wave] = __popcll(mask);
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < W; ++w) {
          const int c = wcnt[w];
          before += w < wave ? c : 0, total += c;
        }
        if (un) ulist[before + __popcll(mask & below)] = t;
        status = flag_s, nb = total;
        __syncthreads();
        if (status != OPTIMAL) break;
      }
      if (status != OPTIMAL) break;
      phases += 1;
      if (eps == 1) break;
    }
  }

  // the assignment (the identity and zero prices unless optimal), its cost, the group's figures
  long long c = 0;
  if (t < m) {
    const int j = status == OPTIMAL ? has[t] : t, k = aidx[t];
    a.slot_of[k] = aidx[j];
    if (a.price != nullptr) a.price[k] = status == OPTIMAL ? price[t] : 0;
    if (status == OPTIMAL) c = cost(bx[t], by[t], bz[t], sx[j], sy[j], sz[j], inv_q2);
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) c += __shfl_xor(c, off, 64);
  if (lane == 0 && c != 0) atomicAdd(&cost_s, (unsigned long long)c);
  __syncthreads();
  if (t == 0) {
    hdsm_assign_stats r;
    r.first = lo, r.count = hi - lo, r.active = m, r.status = status;
    r.phases = phases, r.reserved0 = 0;
    r.iters = iters, r.bids = bids, r.cost = (long long)cost_s;
    a.stats[g] = r;
  }
}

}  // namespace

hipError_t launch(const Launch& a, int m_max, hipStream_t st) {
  if (a.n_groups <= 0) return hipSuccess;
  int threads = (m_max + 63) / 64 * 64;
  threads = threads < 64 ? 64 : threads > MAX_M ? MAX_M : threads;
  hipLaunchKernelGGL(k_assign, dim3((unsigned)a.n_groups), dim3((unsigned)threads), 0, st, a);
  return hipGetLastError();
}

}  // namespace hdsm_assign

namespace {

// hdsm_assign_batch; with reps > 0 the launch is repeated reps times on the same inputs, each between two HIP events: ms [reps]
int batch(int32_t device, const hdsm_assign_setting* setting, int32_t n, int32_t n_groups, const int32_t* group_start, const double* pos,
          const uint8_t* active, const double* slots, int32_t* slot_of, int64_t* price, hdsm_assign_stats* stats, int reps, float* ms) {
  using namespace hdsm_assign;
  Rule rule;
  std::vector<int32_t> gs;
  int m_max = 0;
  const int rc = check_args(setting, n, n_groups, group_start, pos != nullptr, active, n, slots, slot_of, &rule, &gs, &m_max);
  if (rc) return rc;
  const int G = (int)gs.size() - 1;
  if (n == 0) {
    if (stats) stats[0] = hdsm_assign_stats{};
    return HDSM_OK;
  }
  if (hipSetDevice(device) != hipSuccess) return HDSM_ERR_NO_DEVICE;
  const size_t N = (size_t)n;
  hdsm_mem::DevBuf<double> d_pos, d_slots;
  hdsm_mem::DevBuf<uint8_t> d_active;
  hdsm_mem::DevBuf<int32_t> d_gs, d_slot_of;
  hdsm_mem::DevBuf<int64_t> d_price;
  hdsm_mem::DevBuf<hdsm_assign_stats> d_stats;
  hdsm_mem::FirstError ok;
  ok(d_pos.alloc(N * 3)), ok(d_slots.alloc(N * 3)), ok(d_gs.alloc(gs.size())), ok(d_slot_of.alloc(N)), ok(d_price.alloc(N)), ok(d_stats.alloc((size_t)G));
  if (active) ok(d_active.alloc(N));
  if (ok.ok()) {
    ok(hipMemcpy(d_pos.get(), pos, N * 3 * sizeof(double), hipMemcpyHostToDevice));
    ok(hipMemcpy(d_slots.get(), slots, N * 3 * sizeof(double), hipMemcpyHostToDevice));
    ok(hipMemcpy(d_gs.get(), gs.data(), gs.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    if (active) ok(hipMemcpy(d_active.get(), active, N, hipMemcpyHostToDevice));
  }
  const Launch args{rule, G, n, d_gs.get(), nullptr, d_pos.get(), active ? d_active.get() : nullptr, d_slots.get(), d_slot_of.get(), d_price.get(),
                    d_stats.get()};
  if (ok.ok() && reps <= 0) {
    ok(launch(args, m_max, nullptr));
    ok(hipDeviceSynchronize());
  }
  hdsm_mem::DevEvent t0, t1;
  if (ok.ok() && reps > 0) ok(t0.create(hipEventDefault)), ok(t1.create(hipEventDefault));
  for (int r = 0; r < reps && ok.ok(); ++r) {
    ok(hipEventRecord(t0.get(), nullptr)), ok(launch(args, m_max, nullptr)), ok(hipEventRecord(t1.get(), nullptr));
    ok(hipEventSynchronize(t1.get()));
    if (ok.ok()) ok(hipEventElapsedTime(&ms[r], t0.get(), t1.get()));
  }
  std::vector<int32_t> h_slot(N);
  std::vector<int64_t> h_price(N);
  std::vector<hdsm_assign_stats> h_stats((size_t)G);
  if (ok.ok()) {  // (into the caller's arrays only once everything has arrived)
    ok(hipMemcpy(h_slot.data(), d_slot_of.get(), N * sizeof(int32_t), hipMemcpyDeviceToHost));
    ok(hipMemcpy(h_price.data(), d_price.get(), N * sizeof(int64_t), hipMemcpyDeviceToHost));
    ok(hipMemcpy(h_stats.data(), d_stats.get(), (size_t)G * sizeof(hdsm_assign_stats), hipMemcpyDeviceToHost));
  }
  if (!ok.ok()) return HDSM_ERR_DEVICE;
  std::copy(h_slot.begin(), h_slot.end(), slot_of);
  if (price) std::copy(h_price.begin(), h_price.end(), price);
  if (stats) std::copy(h_stats.begin(), h_stats.end(), stats);
  return HDSM_OK;
}

}  // namespace

extern "C" int hdsm_assign_batch(int32_t device, const hdsm_assign_setting* setting, int32_t n, int32_t n_groups, const int32_t* group_start,
                                 const double* pos, const uint8_t* active, const double* slots, int32_t* slot_of, int64_t* price,
                                 hdsm_assign_stats* stats) {
  return batch(device, setting, n, n_groups, group_start, pos, active, slots, slot_of, price, stats, 0, nullptr);
}

extern "C" int hdsm_internal_assign_batch_timed(int32_t device, const hdsm_assign_setting* setting, int32_t n, int32_t n_groups,
                                                const int32_t* group_start, const double* pos, const uint8_t* active, const double* slots,
                                                int32_t* slot_of, int64_t* price, hdsm_assign_stats* stats, int32_t reps, float* ms) {
  if (reps < 1 || !ms) return HDSM_ERR_BAD_ARG;
  return batch(device, setting, n, n_groups, group_start, pos, active, slots, slot_of, price, stats, reps, ms);
}
