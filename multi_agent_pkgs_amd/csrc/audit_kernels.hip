// audit_kernels.hip — the flight audit (audit_core.h) on the device, for hdsm_flight_audit_batch and the device-resident loop:
//   k_audit_pack   the (step_plan + 1) x 3 positions that matter out of the [n_hor + 1][9] records into a compact [G][S + 1][3]
//                  array (cfg 5: 4.7 MB of records -> 200 KB), so that the pair sweep reads contiguous tiles
//   k_audit        the dense pair sweep: a workgroup = one wavefront of 64 subjects (one per lane) x one chunk of at most 64 partners.
//                  The chunk's positions and flags are staged through LDS once and read as broadcasts; every lane keeps its
//                  minimum over the chunk in three registers and stores it as a partial [chunk][subject]. n_local = G = 4096:
//                  64 x 64 workgroups (audit_device.h: why the tiles are small).
//   k_audit_track  one lane per subject: the partials merged in chunk order with the tie rule (smaller sub-step, lower id: a total
//                  order, so the result does not depend on how the partners were chunked), the own-track rule, the round's record,
//                  the flight record, and the history row (state_curr after the commit).
// No atomics, no scratch; the arithmetic is audit_core.h's, the same source as the host form.
#include <hip/hip_runtime.h>

#include "../../include/hdsm_swarm.h"
#include "audit_core.h"
#include "audit_device.h"
#include "hdsm_internal.h"

namespace hdsm_audit {
namespace {

__global__ __launch_bounds__(256) void k_audit_pack(int G, int S, int rec, const double* plans, double* pos) {
  const int per = (S + 1) * 3;
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long long)G * per) return;
  const int g = (int)(e / per), r = (int)(e % per);
  pos[e] = plans[(size_t)g * rec + (size_t)(r / 3) * 9 + (r % 3)];
}

__global__ __launch_bounds__(SWEEP_THREADS) void k_audit(int G, int n_local, int S, int first, int tile, Weights w, const double* pos,
                                                         const uint8_t* has, const int32_t* __restrict__ range, Partial* part) {
  __shared__ double t_pos[TILE_DOUBLES];
  __shared__ uint8_t t_has[TILE_PARTNERS];
  const int tid = (int)threadIdx.x, k = (int)blockIdx.x * SWEEP_THREADS + tid, chunk = (int)blockIdx.y;
  const int per = (S + 1) * 3, p0 = chunk * tile;
  const int cnt = G - p0 < tile ? G - p0 : tile;  // (>= 1: the grid has ceil(G / tile) chunks)
  // neighbour groups: a lane takes a partner only inside its subject's id range [lo, hi). A workgroup (ONE wavefront) none of whose
  // subjects' ranges meets the chunk has nothing to read: "no partner" partials, the tile is not staged.
  static_assert(SWEEP_THREADS == 64, "the vote below is the whole workgroup's");
  int lo = 0, hi = G;
  if (range != nullptr) {
    lo = k < n_local ? range[2 * (size_t)(first + k)] : 0, hi = k < n_local ? range[2 * (size_t)(first + k) + 1] : 0;
    if (!__any(lo < p0 + cnt && hi > p0)) {
      if (k < n_local) part[(size_t)chunk * n_local + k] = Partial{DBL_MAX, -1, 0};
      return;
    }
  }
  for (int e = tid; e < cnt * per; e += SWEEP_THREADS) t_pos[e] = pos[(size_t)p0 * per + e];
  for (int e = tid; e < cnt; e += SWEEP_THREADS) t_has[e] = has[p0 + e];
  __syncthreads();
  if (k >= n_local) return;
  const int a = first + k;
  Best best = no_partner();
  if (has[a]) {
    const double* pa = pos + (size_t)a * per;
    for (int s = 0; s < S; ++s) {
      const double a0[3] = {pa[3 * s], pa[3 * s + 1], pa[3 * s + 2]};
      const double a1[3] = {pa[3 * s + 3], pa[3 * s + 4], pa[3 * s + 5]};
      for (int j = 0; j < cnt; ++j) {
        if (!t_has[j]) continue;  // (the same for every lane)
        if (p0 + j < lo || p0 + j >= hi) continue;  // (not of this subject's group)
        const double* pb = t_pos + j * per + 3 * s;
        const double q = pair_q(w, a0, a1, pb, pb + 3);
        if (p0 + j != a) take(best, q, s, p0 + j);
      }
    }
  }
  part[(size_t)chunk * n_local + k] = Partial{best.q, best.partner, best.substep};
}

__global__ __launch_bounds__(64) void k_audit_track(int n_local, int S, int first, int chunks, int audit, World wd, const double* pos,
                                                    const double* plans, int rec, const uint8_t* has, const Partial* part,
                                                    hdsm_audit_round* round, hdsm_flight_report* report, double warn2, const double* state0,
                                                    size_t state_stride, double* hist_row) {
  const int k = (int)blockIdx.x * 64 + (int)threadIdx.x;
  if (k >= n_local) return;
  if (hist_row != nullptr) {
    const double* sc = reinterpret_cast<const double*>(reinterpret_cast<const char*>(state0) + (size_t)k * state_stride);
    for (int c = 0; c < 9; ++c) hist_row[(size_t)k * 9 + c] = sc[c];
  }
  if (!audit) return;
  const int a = first + k;
  hdsm_audit_round out;
  empty_round(&out);
  if (has[a]) {
    Best best = no_partner();
    for (int c = 0; c < chunks; ++c) {
      const Partial p = part[(size_t)c * n_local + k];
      if (p.partner >= 0) take(best, p.q, p.substep, p.partner);
    }
    out.sep2 = best.q, out.partner = best.partner, out.substep = best.substep;
    track(wd, pos + (size_t)a * (S + 1) * 3, 3, S, plans + (size_t)a * rec + (size_t)S * 9 + 3, &out);
    if (report != nullptr) accumulate(&report[k], out, S, warn2);
  }
  round[k] = out;
}

}  // namespace

hipError_t device_alloc(DeviceBufs* b, int G, int n_local, int S) {
  *b = DeviceBufs{};
  b->G = G, b->n_local = n_local, b->S = S, b->tile = tile_partners(S);
  b->chunks = G > 0 ? (G + b->tile - 1) / b->tile : 1;
  hipError_t e = b->d_pos.alloc((size_t)G * (S + 1) * 3 + 1);
  if (e == hipSuccess) e = b->d_part.alloc((size_t)b->chunks * n_local + 1);
  if (e == hipSuccess) e = b->d_round.alloc((size_t)n_local + 1);
  if (e != hipSuccess) *b = DeviceBufs{};
  return e;
}

hipError_t launch(const DeviceBufs& b, bool audit, const double* d_plans, const uint8_t* d_has, const int32_t* d_range, int n_hor, int first, const Weights& w,
                  const World& wd, hdsm_flight_report* d_report, double warn2, const double* state0, size_t state_stride, double* hist_row,
                  hipStream_t st) {
  if (b.n_local <= 0) return hipSuccess;
  const int rec = (n_hor + 1) * 9;
  if (audit) {
    const long long elems = (long long)b.G * (b.S + 1) * 3;
    hipLaunchKernelGGL(k_audit_pack, dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, st, b.G, b.S, rec, d_plans, b.d_pos.get());
    hipLaunchKernelGGL(k_audit, dim3((unsigned)((b.n_local + SWEEP_THREADS - 1) / SWEEP_THREADS), (unsigned)b.chunks), dim3(SWEEP_THREADS), 0, st,
                       b.G, b.n_local, b.S, first, b.tile, w, b.d_pos.get(), d_has, d_range, b.d_part.get());
  }
  hipLaunchKernelGGL(k_audit_track, dim3((unsigned)((b.n_local + 63) / 64)), dim3(64), 0, st, b.n_local, b.S, first, b.chunks, audit ? 1 : 0, wd,
                     b.d_pos.get(), d_plans, rec, d_has, b.d_part.get(), b.d_round.get(), d_report, warn2, state0, state_stride, hist_row);
  return hipGetLastError();
}

}  // namespace hdsm_audit

extern "C" int hdsm_flight_audit_batch(int32_t device, int32_t n_rob, const double* plans_all, const uint8_t* has_plan, int32_t n_hor,
                                       int32_t step_plan, int32_t first, int32_t n_local, double drone_radius, double drone_z_offset,
                                       const int8_t* world, const int32_t wdim[3], const double worigin[3], double voxel_size,
                                       hdsm_audit_round* out) {
  const int rc = hdsm_internal_audit_args(n_rob, plans_all, has_plan, n_hor, step_plan, first, n_local, drone_radius, drone_z_offset, world,
                                          wdim, worigin, voxel_size, out);
  if (rc) return rc;
  if (n_local == 0) return HDSM_OK;
  if (hipSetDevice(device) != hipSuccess) return HDSM_ERR_NO_DEVICE;
  hdsm_audit::DeviceBufs b;
  hdsm_mem::DevBuf<double> d_plans;
  hdsm_mem::DevBuf<uint8_t> d_has;
  hdsm_mem::DevBuf<int8_t> d_world;
  const size_t pcount = (size_t)n_rob * (n_hor + 1) * 9, wbytes = world ? (size_t)wdim[0] * wdim[1] * wdim[2] : 0;
  hdsm_mem::FirstError ok;
  ok(hdsm_audit::device_alloc(&b, n_rob, n_local, step_plan));
  ok(d_plans.alloc(pcount)), ok(d_has.alloc((size_t)n_rob));
  if (world) ok(d_world.alloc(wbytes));
  if (ok.ok()) {
    ok(hipMemcpy(d_plans.get(), plans_all, pcount * sizeof(double), hipMemcpyHostToDevice));
    ok(hipMemcpy(d_has.get(), has_plan, (size_t)n_rob, hipMemcpyHostToDevice));
    if (world) ok(hipMemcpy(d_world.get(), world, wbytes, hipMemcpyHostToDevice));
  }
  if (ok.ok()) {
    hdsm_audit::World wd{};
    wd.world = d_world.get(), wd.voxel_size = voxel_size;
    if (world)
      for (int k = 0; k < 3; ++k) wd.wdim[k] = wdim[k], wd.worigin[k] = worigin[k];
    ok(hdsm_audit::launch(b, true, d_plans.get(), d_has.get(), nullptr, n_hor, first, hdsm_audit::weights(drone_radius, drone_z_offset), wd, nullptr, 0.0, nullptr, 0,
                          nullptr, nullptr));
    ok(hipDeviceSynchronize());
  }
  if (ok.ok()) ok(hipMemcpy(out, b.d_round.get(), (size_t)n_local * sizeof(hdsm_audit_round), hipMemcpyDeviceToHost));
  return ok.ok() ? HDSM_OK : HDSM_ERR_DEVICE;
}
