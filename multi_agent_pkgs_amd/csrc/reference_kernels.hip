// reference_kernels.hip — row f1, the reference trajectory of every agent of a round (GenerateReferenceTrajectory AC:1449-1553,
// SamplePath AC:1591-1663, the velocity limit AC:1769-1817): k_ref_pack, k_reference<64|256>, hdsm_reference_device / hdsm_reference.
// In the device-resident loop k_ref_pack also leaves the solver's pre-pass (plan_pack.h).
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <string>

#include "../../include/hdsm.h"
#include "hdsm_core.h"
#include "hdsm_entry.h"
#include "link_core.h"
#include "plan_pack.h"

using namespace hdsm_entry;

namespace {

// ---- next row f1: reference trajectory (AC:1449-1553). One workgroup per agent: the neighbour term of
// ComputePathVelocity is a min-reduction over (step, neighbour) streamed from the all-gathered plans buffer
// (thread <-> neighbour, all N+1 positions of that neighbour read back to back), SamplePath is a short sequential
// walk done by one thread, the velocity references are elementwise.
struct RefArgs {
  int32_t n_inst, n_rob, pmax, N;
  double dt;
  hdsm_ref_config cfg;
  const int32_t* agent_id;
  const double* path;
  const int32_t* n_path;
  const double* vel_cap;
  const double* plans;
  const uint8_t* has_plan;
  double* ref_full;
  double* ref;
  double* path_vel;
  const double* rpos;  // [n_rob][N + 1][3] positions of steps 0..N, packed (k_ref_pack)
  const double* rsph;  // [n_rob][4] enclosing sphere of those positions (radius < 0: no plan)
  const int32_t* range;  // neighbour groups (hdsm_set_groups): [.][2] id range per agent, null = [0, n_rob)
  // stale plans, resolved by the host: where the instance's OWN plan and flag come from (hdsm_set_own_plans_device, else plans / has_plan)
  // and the step shift of the neighbours' records (hdsm_set_plan_shift*, null = none) for the scan that reads them directly
  const double* own_plans;
  const uint8_t* own_has;
  const int32_t* shift;
  int32_t own_local;  // a shift or an override is set: rsph[self] is not the sphere of the instance's own plan (k_reference forms it)
  double wocc[hdsm::MAXH + 1];  // GetVelocityLimit's weight of step i (AC:1791-1795, 1805-1817): config only, evaluated by the host's libm
};

// Positions of steps 0..N of every published plan, packed, and their enclosing sphere: 16 lanes per agent (N + 1 <= 17: lane
// 15 also takes step 16). The velocity limit reads 24 B per (neighbour, step) from here instead of a 72-B stride of the
// records, and skips a neighbour whose sphere is further away than the closest one found.
// In the device-resident loop (one stream, same plans buffer for the reference and the solve of a round) this kernel also leaves
// what k_plan_prepass would compute a few microseconds later from the same records — positions of steps 1..N (`pos`), their
// bounding sphere (`bounds`, may be null), the launch order of the solve (one extra workgroup) — and the solve skips its pre-pass.
// shift (null = none): record k is packed advanced by shift[k] steps, last state held (hdsm_link::shifted_step); the spheres are
// those of the shifted positions.
__global__ __launch_bounds__(256) void k_ref_pack(int N, int n_rob, const double* __restrict__ plans,
                                                   const uint8_t* __restrict__ has_plan, double* __restrict__ rpos,
                                                   double* __restrict__ rsph, double* __restrict__ pos, double* __restrict__ bounds,
                                                   int n_order, const int32_t* __restrict__ key_prev, const int32_t* __restrict__ agent_id,
                                                   int32_t* __restrict__ order, const int32_t* __restrict__ shift) {
  if (order != nullptr && blockIdx.x == gridDim.x - 1) {
    launch_order_block(n_order, key_prev, agent_id, order);
    return;
  }
  const int tid = (int)threadIdx.x, i = tid & 15;
  const int k = (int)blockIdx.x * 16 + (tid >> 4);
  const bool live = k < n_rob;
  const bool has = live && has_plan[k];
  const int sk = (has && shift != nullptr) ? shift[k] : 0;
  double p[2][3] = {{0, 0, 0}, {0, 0, 0}};
  bool on[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int st = i + 16 * u;
    on[u] = has && st <= N && (u == 0 || i == 0);
    if (on[u]) {
      const double* rec = plans + ((int64_t)k * (N + 1) + hdsm_link::shifted_step(st, sk, N)) * 9;
      p[u][0] = rec[0], p[u][1] = rec[1], p[u][2] = rec[2];
    }
    if (live && st <= N && (u == 0 || i == 0)) {
      double* pk = rpos + ((int64_t)k * (N + 1) + st) * 3;
      pk[0] = p[u][0], pk[1] = p[u][1], pk[2] = p[u][2];
      if (pos != nullptr && st >= 1) {
        double* pq = pos + ((int64_t)k * N + st - 1) * 3;
        pq[0] = p[u][0], pq[1] = p[u][1], pq[2] = p[u][2];
      }
    }
  }
  if (bounds != nullptr) {  // the sphere of steps 1..N: the record k_plan_prepass forms
    plan_sphere16<true>(live && i == 0, bounds + 4 * (int64_t)k, has, p[0], on[0] && i >= 1, p[1], on[1]);
  }
  plan_sphere16<true>(live && i == 0, rsph + (int64_t)k * 4, has, p[0], on[0], p[1], on[1]);  // steps 0..N
}

// wave reductions of k_reference: DPP row rotations + v_readlane (hdsm_wave_gi.h) — a __shfl_xor stage on a double is two
// ds_bpermute round trips, and the kernel reduces 14 values per instance
__device__ __forceinline__ double ref_wave_min(double v) { return -hdsm::wave_max64(-v); }

// NT threads per instance: 256 for small batches (more lanes on the one instance's neighbour scans), 64 — one wavefront, every
// instance of a 1024-agent round resident at once, the workgroup barriers of the reductions cost nothing — for large ones
// (46 -> ~20 us per 1024-agent round).
template <int NT>
__global__ __launch_bounds__(NT) void k_reference(RefArgs a) {
  __shared__ double own[hdsm::MAXH + 1][3];
  __shared__ double wocc[hdsm::MAXH + 1];
  __shared__ double red[NT];
  __shared__ double d2w[NT / 64][hdsm::MAXH + 1];
  __shared__ int idx[NT];
  constexpr int PATH_LDS = 64;
  __shared__ double spath[PATH_LDS * 3];
  __shared__ double pts[hdsm::MAXH + 1][3];
  __shared__ int cnt_s;
  constexpr int SURV_CAP = 2048;
  __shared__ int surv[SURV_CAP];
  __shared__ int surv_n;
  const int inst = blockIdx.x, tid = threadIdx.x, N = a.N;
  const int self = a.agent_id[inst];
  const int np = min(max(a.n_path[inst], 1), a.pmax);  // the host wrapper rejects counts outside [1, pmax]; device callers are clamped
  const bool own_has = self >= 0 && self < a.n_rob && a.own_has[self];
  // the ids the three neighbour scans below run over (the same for the whole workgroup: scalar loads, scalar loop bounds)
  int g_lo = 0, g_hi = a.n_rob;
  if (a.range != nullptr) {
    const bool agent = self >= 0 && self < a.n_rob;
    g_lo = agent ? a.range[2 * self] : 0, g_hi = agent ? min(a.range[2 * self + 1], a.n_rob) : 0;
  }
  // the polyline goes through LDS: the sampling walk below is one thread's chain, and every global read in it was a
  // dependent round trip
  const double* pth_g = a.path + (int64_t)inst * a.pmax * 3;
  const bool path_fits = np <= PATH_LDS;
  if (path_fits)
    for (int e = tid; e < np * 3; e += NT) spath[e] = pth_g[e];
  const double* pth = path_fits ? spath : pth_g;
  if (tid <= N) {
    for (int c = 0; c < 3; ++c) own[tid][c] = own_has ? a.own_plans[((int64_t)self * (N + 1) + tid) * 9 + c] : 0.0;
    wocc[tid] = a.wocc[tid];
  }
  __syncthreads();
  double pv = a.vel_cap ? a.vel_cap[inst] : a.cfg.path_vel_max;
  if (pv > a.cfg.path_vel_max) pv = a.cfg.path_vel_max;
  // The limit of one (neighbour, step) pair, v = v_min + (v_max - v_min) (1 - w_i / exp(k d)), does not decrease with the
  // distance d (k >= 0, w_i >= 0, v_max >= v_min; every operation of the chain is monotone), so the minimum over the
  // neighbours is taken on the SQUARED distances — three subtractions and three multiply-adds per pair — and the square root,
  // the exponential and the division are evaluated once per step on the closest neighbour instead of once per pair.
  const bool monotone = a.cfg.sens_dist >= 0 && a.cfg.path_vel_max >= a.cfg.path_vel_min;
  if (own_has && np >= 2 && monotone) {
    // (1) the neighbour whose sphere is closest: its exact squared distances bound the minima from above
    double4 ss;
    if (a.own_local) {
      // Stale plans: rsph[self] is the sphere of the record the OTHERS read (shifted, or the stale copy of an own-plan override), not
      // of the plan this instance flies. Wave 0 forms the own one from `own` (box centre, largest distance, as plan_sphere16 does;
      // any sphere that holds the N + 1 points gives the same minima). A non-finite plan gets the never-culling radius.
      if (tid < 64) {
        const bool in = tid <= N;
        double c3[3], r2 = 0.0;
        for (int ax = 0; ax < 3; ++ax) {
          const double v = in ? own[tid][ax] : 0.0;
          const bool fin = v - v == 0.0;
          const double lo = ref_wave_min((in && fin) ? v : DBL_MAX), hi = hdsm::wave_max64((in && fin) ? v : -DBL_MAX);
          c3[ax] = 0.5 * (lo + hi);
          r2 += fin ? (v - c3[ax]) * (v - c3[ax]) : DBL_MAX;
        }
        r2 = hdsm::wave_max64((in && r2 == r2) ? r2 : (in ? DBL_MAX : 0.0));
        if (tid == 0) {
          double w = sqrt(r2) * (1.0 + 1e-9);
          if (!(w >= 0.0) || !(w < 1e299)) w = 1e300;
          red[0] = c3[0], red[1] = c3[1], red[2] = c3[2], red[3] = w;
        }
      }
      __syncthreads();
      ss = double4{red[0], red[1], red[2], red[3]};
      __syncthreads();  // (red is reused by the reductions below)
    } else {
      ss = *reinterpret_cast<const double4*>(a.rsph + (int64_t)self * 4);
    }
    // Only a FINITE gap is a candidate (g < +inf, false for a NaN): the centre of a non-finite plan's sphere may be infinite (g = +inf)
    // or NaN (a plan with +inf and -inf on one axis). Taken as a lane's first candidate, a NaN lost to nobody, and every neighbour
    // the lane met after it was missing from the bound: with no other candidate the bound became 0 and neighbours whose sphere did
    // not touch ours were culled. Such a sphere needs no bound: its radius is 1e300 and pass (2) keeps it whatever umax is.
    double gbest = HUGE_VAL;
    int jbest = -1;
    constexpr int UB = 8;  // sphere records in flight per thread: the scans are chains of L2 round trips otherwise
    for (int j0 = g_lo + tid; j0 < g_hi; j0 += UB * NT) {
      double4 sj[UB];
#pragma unroll
      for (int u = 0; u < UB; ++u) {
        const int j = j0 + u * NT;
        sj[u] = *reinterpret_cast<const double4*>(a.rsph + (int64_t)(j < g_hi ? j : self) * 4);
      }
#pragma unroll
      for (int u = 0; u < UB; ++u) {
        const int j = j0 + u * NT;
        if (j >= g_hi || j == self || sj[u].w < 0) continue;  // (w < 0: no plan)
        const double cx = sj[u].x - ss.x, cy = sj[u].y - ss.y, cz = sj[u].z - ss.z;
        const double g = sqrt(cx * cx + cy * cy + cz * cz) - sj[u].w - ss.w;  // every step of j is at least this far (g may be < 0)
        if (g < gbest) gbest = g, jbest = j;
      }
    }
    {  // (which of several equally close spheres wins only moves the bound below)
      const double key = jbest >= 0 ? gbest : DBL_MAX;
      const double m = ref_wave_min(key);
      const unsigned long long who = __ballot(jbest >= 0 && key == m);
      const int src = who != 0ull ? __ffsll((long long)who) - 1 : 0;
      jbest = who != 0ull ? __builtin_amdgcn_readlane(jbest, src) : -1;
      gbest = m;
    }
    if constexpr (NT > 64) {
      if ((tid & 63) == 0) red[tid >> 6] = gbest, idx[tid >> 6] = jbest;
      __syncthreads();
      gbest = red[0], jbest = idx[0];
#pragma unroll
      for (int w = 1; w < NT / 64; ++w)
        if (idx[w] >= 0 && (jbest < 0 || red[w] < gbest)) gbest = red[w], jbest = idx[w];
      __syncthreads();
    }
    const int jstar = jbest;
    double umax = 0.0;
    {
      const int lane = tid & 63;
      double u = 0.0;
      if (lane <= N && jstar >= 0) {
        const double* rp = a.rpos + ((int64_t)jstar * (N + 1) + lane) * 3;
        const double dx = own[lane][0] - rp[0], dy = own[lane][1] - rp[1], dz = own[lane][2] - rp[2];
        u = dx * dx + dy * dy + dz * dz;
        u = (u == u) ? u : DBL_MAX;  // (a non-finite plan bounds nothing)
      }
      u = hdsm::wave_max64(u);
      umax = u;
    }
    // (2) minima of the squared distances over the neighbours that can still lower one of them
    double d2min[hdsm::MAXH + 1];
#pragma unroll
    for (int i = 0; i <= hdsm::MAXH; ++i) d2min[i] = DBL_MAX;
    // The neighbours that pass the sphere test are first LISTED (LDS) and then shared out evenly, one per thread and trip: taken
    // where they are found, a trip of the scan cost a full round trip to memory for the whole wavefront whenever ANY lane had a
    // survivor in it — 16 round trips per instance in a dense ring, half of this kernel's time.
    auto drain = [&]() {
      __syncthreads();
      const int cnt = surv_n < SURV_CAP ? surv_n : SURV_CAP;
      for (int k = tid; k < cnt; k += NT) {
        const double* rp = a.rpos + (int64_t)surv[k] * (N + 1) * 3;
#pragma unroll
        for (int i = 0; i <= hdsm::MAXH; ++i)
          if (i <= N) {
            const double dx = own[i][0] - rp[3 * i], dy = own[i][1] - rp[3 * i + 1], dz = own[i][2] - rp[3 * i + 2];
            d2min[i] = fmin(d2min[i], dx * dx + dy * dy + dz * dz);
          }
      }
      __syncthreads();
      if (tid == 0) surv_n = 0;
      __syncthreads();
    };
    if (tid == 0) surv_n = 0;
    __syncthreads();
    int listed = 0;  // (an upper bound of surv_n, the same in every thread)
    for (int j0 = g_lo + tid; j0 - tid < g_hi; j0 += UB * NT) {
      if (listed + UB * NT > SURV_CAP) drain(), listed = 0;
      double4 sj[UB];
#pragma unroll
      for (int u = 0; u < UB; ++u) {
        const int j = j0 + u * NT;
        sj[u] = *reinterpret_cast<const double4*>(a.rsph + (int64_t)(j < g_hi ? j : self) * 4);
      }
#pragma unroll
      for (int u = 0; u < UB; ++u) {
        const int j = j0 + u * NT;
        if (j >= g_hi || j == self || sj[u].w < 0) continue;
        const double cx = sj[u].x - ss.x, cy = sj[u].y - ss.y, cz = sj[u].z - ss.z;
        // (squared: all its steps are further than the closest neighbour's when the gap between the spheres is)
        const double c2 = cx * cx + cy * cy + cz * cz, reach = sj[u].w + ss.w + sqrt(umax) * (1.0 + 1e-9);
        if (c2 > reach * reach * (1.0 + 1e-9)) continue;
        surv[atomicAdd(&surv_n, 1)] = j;
      }
      listed += UB * NT;
    }
    drain();
#pragma unroll
    for (int i = 0; i <= hdsm::MAXH; ++i)
      if (i <= N) {
        double m = d2min[i];
        m = ref_wave_min(m);
        if ((tid & 63) == 0) d2w[tid >> 6][i] = m;
      }
    __syncthreads();
    if (tid <= N) {
      double m = d2w[0][tid];
#pragma unroll
      for (int w = 1; w < NT / 64; ++w) m = fmin(m, d2w[w][tid]);
      if (m < DBL_MAX) {
        const double d = sqrt(m);
        const double alpha = (1 - wocc[tid] * (1 / exp(a.cfg.sens_dist * d)));
        const double v = a.cfg.path_vel_min + (a.cfg.path_vel_max - a.cfg.path_vel_min) * alpha;
        if (v < pv) pv = v;
      }
    }
  } else if (own_has && np >= 2) {  // (a configuration whose limit is not monotone in the distance: every pair is evaluated)
    for (int j = g_lo + tid; j < g_hi; j += NT) {
      if (j == self || !a.has_plan[j]) continue;
      const double* rec0 = a.plans + (int64_t)j * (N + 1) * 9;
      const int sj = a.shift != nullptr ? a.shift[j] : 0;
      for (int i = 0; i <= N; ++i) {
        const double* rec = rec0 + 9 * (hdsm_link::shifted_step(i, sj, N) - i);  // (rec[9 i] is the neighbour's shifted step i)
        const double dx = own[i][0] - rec[9 * i], dy = own[i][1] - rec[9 * i + 1], dz = own[i][2] - rec[9 * i + 2];
        const double d = sqrt(dx * dx + dy * dy + dz * dz);
        const double alpha = (1 - wocc[i] * (1 / exp(a.cfg.sens_dist * d)));
        const double v = a.cfg.path_vel_min + (a.cfg.path_vel_max - a.cfg.path_vel_min) * alpha;
        if (v < pv) pv = v;
      }
    }
  }
  pv = ref_wave_min(pv);
  if constexpr (NT > 64) {
    if ((tid & 63) == 0) red[tid >> 6] = pv;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) pv = fmin(pv, red[w]);
  }
  pv = (np < 2) ? 0.0 : pv;
  if (tid == 0) {  // SamplePath, AC:1591-1663
    int cnt = 0;
    if (np < 2) {
      for (int i = 0; i < N; ++i, ++cnt)
        for (int c = 0; c < 3; ++c) pts[cnt][c] = pth[c];
    } else {
      const double samp = pv * a.dt;
      int path_idx = 1, ref_idx = 0;
      double cur[3] = {pth[0], pth[1], pth[2]};
      for (int c = 0; c < 3; ++c) pts[0][c] = cur[c];
      cnt = 1;
      double limit = samp;
      while (ref_idx < N) {
        const double* nx = pth + 3 * path_idx;
        const double d0 = nx[0] - cur[0], d1 = nx[1] - cur[1], d2 = nx[2] - cur[2];
        const double dist_next = sqrt(d0 * d0 + d1 * d1 + d2 * d2);
        if (dist_next > limit) {
          cur[0] = cur[0] + limit * d0 / dist_next, cur[1] = cur[1] + limit * d1 / dist_next;
          cur[2] = cur[2] + limit * d2 / dist_next;
          for (int c = 0; c < 3; ++c) pts[cnt][c] = cur[c];
          ++cnt, ++ref_idx;
          limit = fmax(0.0, samp - a.cfg.path_vel_dec * a.dt);
        } else {
          cur[0] = nx[0], cur[1] = nx[1], cur[2] = nx[2];
          if (++path_idx == np) {
            for (int i = ref_idx; i < N; ++i, ++cnt)
              for (int c = 0; c < 3; ++c) pts[cnt][c] = pth[3 * (np - 1) + c];
            break;
          }
          limit -= dist_next;
        }
      }
    }
    cnt_s = cnt;
    a.path_vel[inst] = pv;
  }
  __syncthreads();
  const int cnt = cnt_s;
  if (tid <= N) {  // velocity reference AC:1527-1547: row i looks back from i+1; the last row copies the previous one
    const int i = tid < cnt ? tid : cnt - 1;
    const int ii = (i + 1 < cnt) ? i : (cnt >= 2 ? cnt - 2 : 0);  // pair used by row i
    double v[3] = {0, 0, 0};
    if (cnt > 1) {
      const double d0 = pts[ii][0] - pts[ii + 1][0], d1 = pts[ii][1] - pts[ii + 1][1], d2 = pts[ii][2] - pts[ii + 1][2];
      const double dist = sqrt(d0 * d0 + d1 * d1 + d2 * d2);
      if (dist > 1e-2) v[0] = pv * d0 / dist, v[1] = pv * d1 / dist, v[2] = pv * d2 / dist;
    }
    double* out = a.ref_full + ((int64_t)inst * (N + 1) + tid) * 6;
    for (int c = 0; c < 3; ++c) out[c] = pts[i][c], out[3 + c] = v[c];
    if (a.ref && tid < N) {
      double* o2 = a.ref + ((int64_t)inst * N + tid) * 6;
      for (int c = 0; c < 6; ++c) o2[c] = out[c];
    }
  }
}

}  // namespace

extern "C" {

int hdsm_reference_device(void* handle, const hdsm_ref_config* cfg, int32_t n_inst, int32_t n_rob,
                          const int32_t* agent_id, const double* path, const int32_t* n_path, int32_t pmax,
                          const double* vel_cap, const double* plans_all, const uint8_t* has_plan,
                          double* ref_full, double* ref, double* path_vel, void* hip_stream) {
  Handle* h = static_cast<Handle*>(handle);
  if (int rc = check_neighbours(h, n_inst, n_rob)) return rc;
  if (n_inst == 0) return HDSM_OK;
  if (!cfg || !agent_id || !path || !n_path || !plans_all || !has_plan || !ref_full || !path_vel || pmax < 1)
    return set_err(HDSM_ERR_BAD_ARG, "null or empty argument");
  HIP_TRY(hipSetDevice(h->device));
  RefArgs a{};
  a.n_inst = n_inst, a.n_rob = n_rob, a.pmax = pmax, a.N = h->N, a.dt = h->prm.dt, a.cfg = *cfg;
  a.agent_id = agent_id, a.path = path, a.n_path = n_path, a.vel_cap = vel_cap, a.plans = plans_all;
  a.has_plan = has_plan, a.ref_full = ref_full, a.ref = ref, a.path_vel = path_vel;
  hdsm_handle::Prepass& pp = h->pre;
  a.rpos = pp.d_rpos.get(), a.rsph = pp.d_rsph.get(), a.range = h->range();
  a.own_plans = h->own_plans != nullptr ? h->own_plans : plans_all;
  a.own_has = h->own_plans != nullptr && h->own_has != nullptr ? h->own_has : has_plan;
  a.shift = h->shift, a.own_local = (h->shift != nullptr || h->own_plans != nullptr) ? 1 : 0;
  for (int i = 0; i <= hdsm::MAXH; ++i) {
    double occ = 100 * std::pow(cfg->sens_other_agents, (double)i);  // AC:1791-1795
    occ = occ < 0 ? 0 : (occ > 100 ? 100 : occ);
    a.wocc[i] = std::pow(occ / 100, cfg->sens_pot);  // GetVelocityLimit AC:1805-1817
  }
  // d_rpos / d_rsph are scratch of the HANDLE: a call that arrives on another stream than the previous launch waits for it
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  HIP_TRY(join_stream(h, st));
  h->last_stream = st;
  {
    // device-resident loop (defer_done: one stream, the solve of this round follows on the same plans): the pre-pass rides along
    const bool with_pre = h->defer_done;
    const bool ordered = with_pre && h->prm.warm_start && h->order_min > 0 && n_inst >= h->order_min;
    const bool pre = h->prefilter_agents(n_rob) >= h->bounds_min;
    hipLaunchKernelGGL(k_ref_pack, dim3((n_rob + 15) / 16 + (ordered ? 1 : 0)), dim3(256), 0, st, h->N, n_rob, plans_all, has_plan, pp.d_rpos.get(), pp.d_rsph.get(),
                       with_pre ? pp.d_pos.get() : nullptr, with_pre && pre ? pp.d_bounds.get() : nullptr, n_inst, h->d_stats.get() + 7 * h->max_inst, agent_id,
                       ordered ? pp.d_order.get() : nullptr, h->shift);
    pp.plans = with_pre ? plans_all : nullptr, pp.n_rob = n_rob, pp.n_inst = n_inst, pp.ordered = ordered;
  }
  HIP_TRY(hipGetLastError());
  if (n_inst >= 256) hipLaunchKernelGGL(k_reference<64>, dim3(n_inst), dim3(64), 0, st, a);
  else hipLaunchKernelGGL(k_reference<256>, dim3(n_inst), dim3(256), 0, st, a);
  HIP_TRY(hipGetLastError());
  HIP_TRY(mark_done(h, st));
  return HDSM_OK;
}

int hdsm_reference(void* handle, const hdsm_ref_config* cfg, int32_t n_inst, int32_t n_rob, const int32_t* agent_id,
                   const double* path, const int32_t* n_path, int32_t pmax, const double* vel_cap,
                   const double* plans_all, const uint8_t* has_plan, double* ref_full, double* ref, double* path_vel) {
  Handle* h = static_cast<Handle*>(handle);
  if (int rc = check_neighbours(h, n_inst, n_rob)) return rc;
  if (n_inst == 0) return HDSM_OK;
  if (!cfg || !agent_id || !path || !n_path || !plans_all || !has_plan || !ref_full || !path_vel || pmax < 1)
    return set_err(HDSM_ERR_BAD_ARG, "null or empty argument");
  for (int32_t k = 0; k < n_inst; ++k)
    if (n_path[k] < 1 || n_path[k] > pmax) return set_err(HDSM_ERR_BAD_ARG, "n_path[k] must be in [1, pmax]");
  HIP_TRY(hipSetDevice(h->device));
  const size_t I = (size_t)n_inst, N = (size_t)h->N;
  hdsm_handle::HostStaging& s = h->stage;
  hipStream_t st = h->stream.get();
  hipError_t e = s.path.ensure(I * pmax * 3, st);
  if (e == hipSuccess) e = s.cap.ensure(I, st);
  if (e == hipSuccess) e = s.full.ensure(I * (N + 1) * 6, st);
  if (e == hipSuccess) e = s.pv.ensure(I, st);
  if (e == hipSuccess) e = s.np.ensure(I, st);
  if (e != hipSuccess) return set_err(HDSM_ERR_DEVICE, std::string("hdsm_reference: ") + hipGetErrorString(e));
  HIP_TRY(join_stream(h, st));
  Copies cp{st};
  cp(s.path.get(), path, I * pmax * 3 * 8, hipMemcpyHostToDevice);
  cp(s.np.get(), n_path, I * 4, hipMemcpyHostToDevice);
  if (vel_cap) cp(s.cap.get(), vel_cap, I * 8, hipMemcpyHostToDevice);
  cp(s.d_agent.get(), agent_id, I * 4, hipMemcpyHostToDevice);
  cp(s.d_plans.get(), plans_all, (size_t)n_rob * (N + 1) * 9 * 8, hipMemcpyHostToDevice);
  cp(s.d_has.get(), has_plan, (size_t)n_rob, hipMemcpyHostToDevice);
  int rc = HDSM_OK;
  if (cp.err.ok())
    rc = hdsm_reference_device(handle, cfg, n_inst, n_rob, s.d_agent.get(), s.path.get(), s.np.get(), pmax, vel_cap ? s.cap.get() : nullptr,
                               s.d_plans.get(), s.d_has.get(), s.full.get(), ref ? s.d_ref.get() : nullptr, s.pv.get(), st);
  cp(ref_full, s.full.get(), I * (N + 1) * 6 * 8, hipMemcpyDeviceToHost);
  if (ref) cp(ref, s.d_ref.get(), I * N * 6 * 8, hipMemcpyDeviceToHost);
  cp(path_vel, s.pv.get(), I * 8, hipMemcpyDeviceToHost);
  if (cp.err.ok()) cp.err(hipStreamSynchronize(st));
  if (rc) return rc;
  if (!cp.err.ok()) return set_err(HDSM_ERR_DEVICE, std::string("hdsm_reference: ") + hipGetErrorString(cp.err.e));
  return HDSM_OK;
}

}  // extern "C"
