// plan_pack.h — device header: what the kernels that pack the published plans for the solver share across translation units
// (k_plan_prepass and k_launch_order in hdsm_api.hip, k_ref_pack in reference_kernels.hip): the enclosing sphere of a plan and the
// launch order. The build has no relocatable device code, so they are inline functions of a header.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// The enclosing sphere of one plan, formed by the 16 lanes of its group: every lane brings up to two points of the plan (p0 if on0,
// p1 if on1; TWO = false: there is no second slot), the group reduces their bounding box with shuffles, takes its centre and the
// largest squared distance of a point from it, and keeps whether every point was finite. The lane with `lead` (one of the group)
// writes the record rec[4]: centre and radius sqrt(r2) (1 + 1e-9); radius -1 for an agent without a plan (`has`), 1e300 for a
// non-finite or out-of-range one. (Written here, not returned: a record formed in every lane costs k_ref_pack three registers.)
template <bool TWO>
__device__ __forceinline__ void plan_sphere16(bool lead, double* rec, bool has, const double* p0, bool on0, const double* p1, bool on1) {
  double lo[3], hi[3];
  for (int ax = 0; ax < 3; ++ax) {
    lo[ax] = on0 ? p0[ax] : 1e300, hi[ax] = on0 ? p0[ax] : -1e300;
    if (TWO && on1) lo[ax] = fmin(lo[ax], p1[ax]), hi[ax] = fmax(hi[ax], p1[ax]);
  }
  for (int off = 8; off > 0; off >>= 1)
    for (int ax = 0; ax < 3; ++ax) {
      lo[ax] = fmin(lo[ax], __shfl_xor(lo[ax], off, 16));
      hi[ax] = fmax(hi[ax], __shfl_xor(hi[ax], off, 16));
    }
  const double cx = 0.5 * (lo[0] + hi[0]), cy = 0.5 * (lo[1] + hi[1]), cz = 0.5 * (lo[2] + hi[2]);
  double r2 = 0.0;
  if (on0) {
    const double ux = p0[0] - cx, uy = p0[1] - cy, uz = p0[2] - cz;
    r2 = ux * ux + uy * uy + uz * uz;
  }
  bool finite = r2 == r2;
  if (TWO && on1) {
    const double vx = p1[0] - cx, vy = p1[1] - cy, vz = p1[2] - cz;
    const double q2 = vx * vx + vy * vy + vz * vz;
    finite = finite && (q2 == q2);
    r2 = fmax(r2, q2);
  }
  for (int off = 8; off > 0; off >>= 1) {
    r2 = fmax(r2, __shfl_xor(r2, off, 16));
    finite = finite && __shfl_xor((int)finite, off, 16);
  }
  if (!lead) return;
  double4 out = {0.0, 0.0, 0.0, -1.0};
  if (has) {
    out.x = cx, out.y = cy, out.z = cz;
    out.w = sqrt(r2) * (1.0 + 1e-9);
    if (!finite || !(out.w >= 0.0) || !(out.w < 1e299)) out.w = 1e300;  // non-finite plan: never culled, the step-by-step test decides
  }
  *reinterpret_cast<double4*>(rec) = out;
}

// Longest-processing-time-first launch order. A launch lasts as long as its slowest workgroup chain: with more instances than
// resident workgroups (2 per CU) an expensive instance that happens to start late sets the kernel time. Workgroups are
// dispatched in index order, so workgroup w takes instance order[w], the instances sorted by the key they left in the
// PREVIOUS launch on this handle (largest first; a counting sort on 256 values): the time the instance took, or the maximum if it
// found no solution (hdsm_core.h, st_key). The previous replan of the same agent is a good predictor (gridlocked neighbourhoods
// persist); the answer of an instance does not depend on the order. An entry is the pair (instance, its agent id): the workgroup
// then needs no second, dependent load (agent_id[instance]) before it can ask for the agent's own plan.
__device__ inline void launch_order_block(int n_inst, const int32_t* __restrict__ key_prev, const int32_t* __restrict__ agent_id, int32_t* __restrict__ order) {
  __shared__ int bucket[256];
  __shared__ int wave_total[4];
  const int tid = (int)threadIdx.x, nt = (int)blockDim.x;
  // The block is ONE chain of dependent steps (histogram, scan, scatter), and it sits in a launch whose other workgroups need two or three
  // memory round trips: so every thread asks for all its keys and agent ids at once, before the first LDS operation, and keeps them in
  // registers for both passes — one round trip for batches of up to LB x 256 instances. (Walking the keys once per pass, a load and an LDS
  // atomic at a time, was eight dependent trips at 1024 instances.) The instances beyond the first batch take a batch-wide trip per pass.
  constexpr int LB = 4;
  int bk[LB], ag[LB];
#pragma unroll
  for (int u = 0; u < LB; ++u) {
    const int k = tid + u * nt;
    const int it = k < n_inst ? key_prev[k] : 0;
    ag[u] = k < n_inst ? agent_id[k] : 0;
    bk[u] = 255 - (it < 0 ? 0 : (it > 255 ? 255 : it));
  }
  for (int b = tid; b < 256; b += nt) bucket[b] = 0;
  __syncthreads();
#pragma unroll
  for (int u = 0; u < LB; ++u)
    if (tid + u * nt < n_inst) atomicAdd(&bucket[bk[u]], 1);
  for (int k0 = LB * nt + tid; k0 - tid < n_inst; k0 += LB * nt) {
    int it[LB];
#pragma unroll
    for (int u = 0; u < LB; ++u) it[u] = k0 + u * nt < n_inst ? key_prev[k0 + u * nt] : 0;
#pragma unroll
    for (int u = 0; u < LB; ++u)
      if (k0 + u * nt < n_inst) atomicAdd(&bucket[255 - (it[u] < 0 ? 0 : (it[u] > 255 ? 255 : it[u]))], 1);
  }
  __syncthreads();
  // exclusive prefix over the 256 buckets, a bucket per thread (every launch of this block has 256 threads): scan inside the wavefront,
  // then the totals of the wavefronts before. (One thread walked the buckets before round 6, 256 dependent LDS round trips.)
  {
    const int c = bucket[tid & 255];
    int incl = c;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int v = __shfl_up(incl, off, 64);
      if ((tid & 63) >= off) incl += v;
    }
    if ((tid & 63) == 63) wave_total[(tid >> 6) & 3] = incl;
    __syncthreads();
    int base = 0;
    for (int w = 0; w < ((tid >> 6) & 3); ++w) base += wave_total[w];
    if (tid < 256) bucket[tid] = base + incl - c;
  }
  __syncthreads();
  int2* const pairs = reinterpret_cast<int2*>(order);  // (read as int2 by the solver's workgroups too)
#pragma unroll
  for (int u = 0; u < LB; ++u)
    if (tid + u * nt < n_inst) pairs[atomicAdd(&bucket[bk[u]], 1)] = make_int2(tid + u * nt, ag[u]);
  for (int k0 = LB * nt + tid; k0 - tid < n_inst; k0 += LB * nt) {
    int it[LB], id[LB];
#pragma unroll
    for (int u = 0; u < LB; ++u) {
      const int k = k0 + u * nt;
      it[u] = k < n_inst ? key_prev[k] : 0, id[u] = k < n_inst ? agent_id[k] : 0;
    }
#pragma unroll
    for (int u = 0; u < LB; ++u)
      if (k0 + u * nt < n_inst) pairs[atomicAdd(&bucket[255 - (it[u] < 0 ? 0 : (it[u] > 255 ? 255 : it[u]))], 1)] = make_int2(k0 + u * nt, id[u]);
  }
}
