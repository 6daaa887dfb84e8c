// path_kernels.hip — the path step of path_core.h as a stand-alone batch on the device (hdsm_local_path_batch): one workgroup per
// case, the same block planner (hdsm_path::plan_block) as the device-resident loop's k_path, host pointers in and out.
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/hdsm_swarm.h"
#include "device_mem.h"
#include "path_core.h"

namespace {

struct BatchArgs {
  const int8_t* world;
  int32_t wdim[3], ldim[3];
  const int32_t *off, *ground_k;
  const double *origin, *start, *goal;
  double res;
  int32_t pmax;
  double* paths;
  int32_t *n_path, *status;
};

__global__ __launch_bounds__(hdsm_path::THREADS) void k_path_batch(BatchArgs a) {
  __shared__ hdsm_path::PathLds lds;
  const int t = (int)blockIdx.x, tid = (int)threadIdx.x;
  hdsm_path::PathIn in;
  in.g.world = a.world;
  for (int ax = 0; ax < 3; ++ax) {
    in.g.wdim[ax] = a.world ? a.wdim[ax] : 0, in.g.dim[ax] = a.ldim[ax], in.g.off[ax] = a.off[3 * (size_t)t + ax];
    in.origin[ax] = a.origin[3 * (size_t)t + ax], in.start[ax] = a.start[3 * (size_t)t + ax], in.goal[ax] = a.goal[3 * (size_t)t + ax];
  }
  in.g.ground_k = a.ground_k[t];
  in.res = a.res;
  const int st = hdsm_path::plan_block(in, lds, tid);
  const int np = st == hdsm_path::PATH_OK ? lds.n_out : 0;
  if (tid == 0) a.status[t] = st, a.n_path[t] = np;
  for (int e = tid; e < 3 * a.pmax; e += hdsm_path::THREADS) {
    const int i = e / 3;
    a.paths[(size_t)t * a.pmax * 3 + e] = np ? lds.out[i < np ? i : np - 1][e % 3] : 0.0;
  }
}

// the clearance mode (path_core.h, 6a-7'): the same arguments, the tunnel's mask as a table, the cost and the chain's length out
__global__ __launch_bounds__(hdsm_path::THREADS) void k_dmp_batch(BatchArgs a, int rn, const uint32_t* rows, int32_t* cost, int32_t* n_raw) {
  __shared__ hdsm_path::DmpLds lds;
  const int t = (int)blockIdx.x, tid = (int)threadIdx.x;
  hdsm_path::PathIn in;
  in.g.world = a.world;
  for (int ax = 0; ax < 3; ++ax) {
    in.g.wdim[ax] = a.world ? a.wdim[ax] : 0, in.g.dim[ax] = a.ldim[ax], in.g.off[ax] = a.off[3 * (size_t)t + ax];
    in.origin[ax] = a.origin[3 * (size_t)t + ax], in.start[ax] = a.start[3 * (size_t)t + ax], in.goal[ax] = a.goal[3 * (size_t)t + ax];
  }
  in.g.ground_k = a.ground_k[t];
  in.res = a.res;
  const int st = hdsm_path::plan_dmp_block(in, rn, rows, lds, tid);
  const int np = st == hdsm_path::PATH_OK ? lds.p.n_out : 0;
  if (tid == 0) a.status[t] = st, a.n_path[t] = np, cost[t] = np ? lds.cost : -1, n_raw[t] = np ? lds.n_raw : 0;
  for (int e = tid; e < 3 * a.pmax; e += hdsm_path::THREADS) {
    const int i = e / 3;
    a.paths[(size_t)t * a.pmax * 3 + e] = np ? lds.p.out[i < np ? i : np - 1][e % 3] : 0.0;
  }
}

// hdsm_local_path_batch (mask == nullptr) and hdsm_local_path_dmp_batch
int run_batch(int32_t device, int32_t n, const int8_t* world, const int32_t wdim[3], const int32_t ldim[3], const int32_t* off,
              const int32_t* ground_k, const double* origin, const double* start, const double* goal, double res, int32_t pmax, double* paths,
              int32_t* n_path, int32_t* status, const hdsm_path::DmpMask* mask, int32_t* cost, int32_t* n_raw) {
  if (n == 0) return HDSM_OK;
  if (pmax > hdsm_sw::PATH_PTS) {  // (the device keeps PATH_PTS points: the rows beyond repeat the last point, as on the host)
    std::vector<double> tmp((size_t)n * hdsm_sw::PATH_PTS * 3);
    const int rc = run_batch(device, n, world, wdim, ldim, off, ground_k, origin, start, goal, res, hdsm_sw::PATH_PTS, tmp.data(), n_path, status,
                             mask, cost, n_raw);
    if (rc) return rc;
    for (int t = 0; t < n; ++t)
      for (int i = 0; i < pmax; ++i)
        for (int c = 0; c < 3; ++c)
          paths[((size_t)t * pmax + i) * 3 + c] = tmp[((size_t)t * hdsm_sw::PATH_PTS + (i < hdsm_sw::PATH_PTS ? i : hdsm_sw::PATH_PTS - 1)) * 3 + c];
    return HDSM_OK;
  }
  if (hipSetDevice(device) != hipSuccess) return HDSM_ERR_NO_DEVICE;
  const size_t wbytes = world ? (size_t)wdim[0] * wdim[1] * wdim[2] : 0;
  BatchArgs a{};
  a.res = res, a.pmax = pmax;
  for (int ax = 0; ax < 3; ++ax) a.wdim[ax] = world ? wdim[ax] : 0, a.ldim[ax] = ldim[ax];
  hdsm_mem::DevBuf<int8_t> d_world;
  hdsm_mem::DevBuf<int32_t> d_off, d_gk, d_np, d_st, d_cost, d_raw;
  hdsm_mem::DevBuf<uint32_t> d_rows;
  hdsm_mem::DevBuf<double> d_org, d_s, d_g, d_paths;
  hdsm_mem::FirstError ok;
  const size_t N = (size_t)n;
  if (world) ok(d_world.alloc(wbytes));
  ok(d_off.alloc(N * 3)), ok(d_gk.alloc(N)), ok(d_np.alloc(N)), ok(d_st.alloc(N));
  ok(d_org.alloc(N * 3)), ok(d_s.alloc(N * 3)), ok(d_g.alloc(N * 3)), ok(d_paths.alloc(N * pmax * 3));
  if (mask) ok(d_cost.alloc(N)), ok(d_raw.alloc(N)), ok(d_rows.alloc(sizeof mask->rows / sizeof mask->rows[0]));
  if (ok.ok()) {
    if (world) ok(hipMemcpy(d_world.get(), world, wbytes, hipMemcpyHostToDevice));
    ok(hipMemcpy(d_off.get(), off, N * 12, hipMemcpyHostToDevice)), ok(hipMemcpy(d_gk.get(), ground_k, N * 4, hipMemcpyHostToDevice));
    ok(hipMemcpy(d_org.get(), origin, N * 24, hipMemcpyHostToDevice)), ok(hipMemcpy(d_s.get(), start, N * 24, hipMemcpyHostToDevice));
    ok(hipMemcpy(d_g.get(), goal, N * 24, hipMemcpyHostToDevice));
    if (mask) ok(hipMemcpy(d_rows.get(), mask->rows, sizeof mask->rows, hipMemcpyHostToDevice));
  }
  if (ok.ok()) {
    a.world = d_world.get(), a.off = d_off.get(), a.ground_k = d_gk.get(), a.origin = d_org.get(), a.start = d_s.get(), a.goal = d_g.get();
    a.paths = d_paths.get(), a.n_path = d_np.get(), a.status = d_st.get();
    if (mask) hipLaunchKernelGGL(k_dmp_batch, dim3((unsigned)n), dim3(hdsm_path::THREADS), 0, 0, a, mask->rn, d_rows.get(), d_cost.get(), d_raw.get());
    else hipLaunchKernelGGL(k_path_batch, dim3((unsigned)n), dim3(hdsm_path::THREADS), 0, 0, a);
    ok(hipGetLastError());
    ok(hipDeviceSynchronize());
  }
  if (ok.ok()) {
    ok(hipMemcpy(paths, d_paths.get(), N * pmax * 24, hipMemcpyDeviceToHost));
    ok(hipMemcpy(n_path, d_np.get(), N * 4, hipMemcpyDeviceToHost)), ok(hipMemcpy(status, d_st.get(), N * 4, hipMemcpyDeviceToHost));
    if (mask) ok(hipMemcpy(cost, d_cost.get(), N * 4, hipMemcpyDeviceToHost)), ok(hipMemcpy(n_raw, d_raw.get(), N * 4, hipMemcpyDeviceToHost));
  }
  return ok.ok() ? HDSM_OK : HDSM_ERR_DEVICE;
}

}  // namespace

extern "C" int hdsm_local_path_batch(int32_t device, int32_t n, const int8_t* world, const int32_t wdim[3], const int32_t ldim[3],
                                     const int32_t* off, const int32_t* ground_k, const double* origin, const double* start, const double* goal,
                                     double res, int32_t pmax, double* paths, int32_t* n_path, int32_t* status) {
  if (n < 0 || !ldim || !off || !ground_k || !origin || !start || !goal || !(res > 0) || pmax < 2 || !paths || !n_path || !status ||
      (world && !wdim))
    return HDSM_ERR_BAD_ARG;
  return run_batch(device, n, world, wdim, ldim, off, ground_k, origin, start, goal, res, pmax, paths, n_path, status, nullptr, nullptr, nullptr);
}

extern "C" int hdsm_local_path_dmp_batch(int32_t device, int32_t n, const int8_t* world, const int32_t wdim[3], const int32_t ldim[3],
                                         const int32_t* off, const int32_t* ground_k, const double* origin, const double* start,
                                         const double* goal, double res, double search_rad, int32_t pmax, double* paths, int32_t* n_path,
                                         int32_t* status, int32_t* cost, int32_t* n_raw) {
  if (n < 0 || !ldim || !off || !ground_k || !origin || !start || !goal || !(res > 0) || !(search_rad == search_rad) || pmax < 2 || !paths ||
      !n_path || !status || !cost || !n_raw || (world && !wdim))
    return HDSM_ERR_BAD_ARG;
  hdsm_path::DmpMask mask;
  hdsm_path::dmp_build_mask(search_rad, res, &mask);  // (a radius over DMP_MAX_RN voxels: status 4 for every case in a world)
  return run_batch(device, n, world, wdim, ldim, off, ground_k, origin, start, goal, res, pmax, paths, n_path, status, &mask, cost, n_raw);
}
