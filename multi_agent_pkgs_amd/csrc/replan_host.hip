// replan_host.hip — hdsm_replan, the host-pointer form of a replan round: upload, hdsm_replan_device, download of the instances
// that have a solution; for arrays registered with hdsm_host_register one fetch and one deliver kernel instead of the copies.
// (The drop-in call shape for AC:1086-1215 fused with AC:858-1023: the caller's arrays are host memory.)
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/hdsm.h"
#include "hdsm_entry.h"

using namespace hdsm_entry;

namespace {

// hdsm_replan with page-locked input arrays: ONE kernel reads them from mapped host memory (coalesced reads over PCIe) into the
// handle's device arrays instead of nine stream-ordered copies, and of the static polyhedra only the rows that exist
// (n_rows_static of max_rows_static; the rest of the device array is never read by the solver). Blocks 0 .. n_inst - 1 take one
// instance each, the blocks after them the plans of every agent.
struct FetchArgs {
  int32_t n_inst, n_rob, N, P, RS, plan_blocks;
  const int32_t *agent_id, *n_poly, *n_rows;
  const double *state, *ref, *A, *b, *plans;
  const uint8_t* has;
  int32_t *d_agent, *d_npoly, *d_nrows;
  double *d_state, *d_ref, *d_A, *d_b, *d_plans;
  uint8_t* d_has;
};
__global__ __launch_bounds__(256) void k_fetch(FetchArgs a) {
  const int tid = (int)threadIdx.x, blk = (int)blockIdx.x;
  if (blk >= a.n_inst) {
    const int64_t total = (int64_t)a.n_rob * (a.N + 1) * 9;
    for (int64_t e = (int64_t)(blk - a.n_inst) * 256 + tid; e < total; e += (int64_t)a.plan_blocks * 256) a.d_plans[e] = a.plans[e];
    for (int e = (blk - a.n_inst) * 256 + tid; e < a.n_rob; e += a.plan_blocks * 256) a.d_has[e] = a.has[e];
    return;
  }
  const int k = blk, P = a.P, RS = a.RS;
  __shared__ int32_t rows_s[HDSM_MAX_POLY];  // (read once over PCIe, not once per entry)
  if (tid == 0) a.d_agent[k] = a.agent_id[k];
  const int np = a.n_poly[k];
  if (tid == 1) a.d_npoly[k] = np;
  if (tid < 9) a.d_state[(int64_t)k * 9 + tid] = a.state[(int64_t)k * 9 + tid];
  if (tid < P) {
    const int32_t nr = a.n_rows[(int64_t)k * P + tid];
    rows_s[tid] = nr, a.d_nrows[(int64_t)k * P + tid] = nr;
  }
  for (int e = tid; e < 6 * a.N; e += 256) a.d_ref[(int64_t)k * 6 * a.N + e] = a.ref[(int64_t)k * 6 * a.N + e];
  __syncthreads();
  for (int e = tid; e < P * RS * 4; e += 256) {  // entry (polyhedron j, row r, component c): c < 3 -> A, c = 3 -> b
    const int c = e & 3, jr = e >> 2, j = jr / RS, r = jr % RS;
    if (j >= np || r >= rows_s[j]) continue;
    const int64_t row = ((int64_t)k * P + j) * RS + r;
    if (c < 3) a.d_A[row * 3 + c] = a.A[row * 3 + c];
    else a.d_b[row] = a.b[row];
  }
}

// hdsm_replan with page-locked output arrays (hdsm_host_register): the results go from HBM straight into the caller's arrays —
// mapped host memory, written over PCIe by the device — and only for instances that HAVE a solution ("outputs are left
// untouched" otherwise): no staging download, no host-side filter copy. One 64-lane group per instance.
__global__ __launch_bounds__(256) void k_deliver(int n_inst, int trj, int ctl, int P, const double* __restrict__ traj, const double* __restrict__ ctrl,
                                                 const double* __restrict__ obj, const int32_t* __restrict__ status, const uint8_t* __restrict__ used,
                                                 double* o_traj, double* o_ctrl, double* o_obj, int32_t* o_status, uint8_t* o_used) {
  const int k = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6), lane = (int)threadIdx.x & 63;
  if (k >= n_inst) return;
  const int stt = status[k];
  if (lane == 0) o_status[k] = stt;
  if (stt == HDSM_NO_SOLUTION) return;
  for (int e = lane; e < trj; e += 64) o_traj[(int64_t)k * trj + e] = traj[(int64_t)k * trj + e];
  for (int e = lane; e < ctl; e += 64) o_ctrl[(int64_t)k * ctl + e] = ctrl[(int64_t)k * ctl + e];
  if (lane < P) o_used[(int64_t)k * P + lane] = used[(int64_t)k * P + lane];
  if (lane == 0) o_obj[k] = obj[k];
}

// Registered (page-locked, mapped) host memory. hdsm_host_register records every range it maps — base, length, device-side
// address — and hdsm_replan takes the kernel paths (k_fetch / k_deliver) only for arrays that lie INSIDE a recorded range with all
// the bytes the call will touch (an array that merely starts in one, or memory page-locked by somebody else, goes through the copy
// path like pageable memory). While nothing is registered the look-up is one load: no runtime query per array and call.
struct HostRange {
  char* base;
  size_t bytes;
  char* dev;
};
std::mutex g_reg_mutex;
std::vector<HostRange> g_reg;
std::atomic<int> g_reg_count{0};

bool mapped_host_range(const void* p, size_t bytes, void** dev) {
  if (g_reg_count.load(std::memory_order_acquire) == 0) return false;
  std::lock_guard<std::mutex> lock(g_reg_mutex);
  const char* c = static_cast<const char*>(p);
  for (const HostRange& r : g_reg)
    if (c >= r.base && bytes <= r.bytes && (size_t)(c - r.base) <= r.bytes - bytes) {
      *dev = r.dev + (c - r.base);
      return true;
    }
  return false;
}

}  // namespace

extern "C" {

int hdsm_host_register(void* ptr, size_t bytes) {
  if (!ptr || bytes == 0) return set_err(HDSM_ERR_BAD_ARG, "hdsm_host_register: null or empty range");
  hipError_t e = hipHostRegister(ptr, bytes, hipHostRegisterMapped | hipHostRegisterPortable);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return set_err(HDSM_ERR_DEVICE, std::string("hdsm_host_register: ") + hipGetErrorString(e));
  }
  void* dev = nullptr;
  e = hipHostGetDevicePointer(&dev, ptr, 0);
  if (e != hipSuccess || dev == nullptr) {
    (void)hipGetLastError();
    (void)hipHostUnregister(ptr);
    return set_err(HDSM_ERR_DEVICE, std::string("hdsm_host_register: no device address for the range: ") + hipGetErrorString(e));
  }
  std::lock_guard<std::mutex> lock(g_reg_mutex);
  g_reg.push_back(HostRange{static_cast<char*>(ptr), bytes, static_cast<char*>(dev)});
  g_reg_count.store((int)g_reg.size(), std::memory_order_release);
  return HDSM_OK;
}

int hdsm_host_unregister(void* ptr) {
  if (!ptr) return set_err(HDSM_ERR_BAD_ARG, "hdsm_host_unregister: null pointer");
  {
    std::lock_guard<std::mutex> lock(g_reg_mutex);
    for (size_t k = 0; k < g_reg.size(); ++k)
      if (g_reg[k].base == static_cast<char*>(ptr)) {
        g_reg.erase(g_reg.begin() + (long)k);
        break;
      }
    g_reg_count.store((int)g_reg.size(), std::memory_order_release);
  }
  const hipError_t e = hipHostUnregister(ptr);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return set_err(HDSM_ERR_DEVICE, std::string("hdsm_host_unregister: ") + hipGetErrorString(e));
  }
  return HDSM_OK;
}

int hdsm_replan(void* handle, int32_t n_inst, int32_t n_rob, const int32_t* agent_id,
                const double* state_curr, const double* traj_ref, const int32_t* n_poly,
                const int32_t* n_rows_static, const double* A_static, const double* b_static,
                const double* plans_all, const uint8_t* has_plan, double* traj_out, double* ctrl_out,
                uint8_t* poly_used, int32_t* status, double* obj) {
  Handle* h = static_cast<Handle*>(handle);
  if (int rc = check_neighbours(h, n_inst, n_rob)) return rc;
  if (n_inst == 0) return HDSM_OK;
  if (!agent_id || !state_curr || !traj_ref || !n_poly || !n_rows_static || !A_static || !b_static ||
      !plans_all || !has_plan || !traj_out || !ctrl_out || !poly_used || !status || !obj)
    return set_err(HDSM_ERR_BAD_ARG, "null array argument");
  HIP_TRY(hipSetDevice(h->device));
  const size_t I = (size_t)n_inst, N = (size_t)h->N, P = (size_t)h->P, RS = (size_t)h->RS;
  hdsm_handle::HostStaging& s = h->stage;
  hipStream_t st = h->stream.get();
  const auto H2D = hipMemcpyHostToDevice;
  const auto D2H = hipMemcpyDeviceToHost;
  HIP_TRY(join_stream(h, st));
  bool in_mapped = true;
  {
    const void* hp[9] = {agent_id, state_curr, traj_ref, n_poly, n_rows_static, A_static, b_static, plans_all, has_plan};
    const size_t hb[9] = {I * 4, I * 9 * 8, I * N * 6 * 8, I * 4, I * P * 4, I * P * RS * 3 * 8, I * P * RS * 8, (size_t)n_rob * (N + 1) * 9 * 8, (size_t)n_rob};
    void* dp[9];
    for (int k = 0; k < 9 && in_mapped; ++k) in_mapped = mapped_host_range(hp[k], hb[k], &dp[k]);
    if (in_mapped) {  // page-locked arrays of the caller (hdsm_host_register): one fetch kernel
      FetchArgs f{};
      f.n_inst = n_inst, f.n_rob = n_rob, f.N = (int)N, f.P = (int)P, f.RS = (int)RS;
      const int64_t plan_items = (int64_t)n_rob * (int64_t)(N + 1) * 9;
      f.plan_blocks = (int)((plan_items + 1023) / 1024 < 1 ? 1 : ((plan_items + 1023) / 1024 > 1024 ? 1024 : (plan_items + 1023) / 1024));
      f.agent_id = static_cast<const int32_t*>(dp[0]), f.state = static_cast<const double*>(dp[1]), f.ref = static_cast<const double*>(dp[2]);
      f.n_poly = static_cast<const int32_t*>(dp[3]), f.n_rows = static_cast<const int32_t*>(dp[4]), f.A = static_cast<const double*>(dp[5]);
      f.b = static_cast<const double*>(dp[6]), f.plans = static_cast<const double*>(dp[7]), f.has = static_cast<const uint8_t*>(dp[8]);
      f.d_agent = s.d_agent.get(), f.d_state = s.d_state.get(), f.d_ref = s.d_ref.get(), f.d_npoly = s.d_npoly.get(), f.d_nrows = s.d_nrows.get();
      f.d_A = s.d_A.get(), f.d_b = s.d_b.get(), f.d_plans = s.d_plans.get(), f.d_has = s.d_has.get();
      hipLaunchKernelGGL(k_fetch, dim3((unsigned)(n_inst + f.plan_blocks)), dim3(256), 0, st, f);
      HIP_TRY(hipGetLastError());
    }
  }
  if (!in_mapped) {
    HIP_TRY(hipMemcpyAsync(s.d_agent.get(), agent_id, I * 4, H2D, st));
    HIP_TRY(hipMemcpyAsync(s.d_state.get(), state_curr, I * 9 * 8, H2D, st));
    HIP_TRY(hipMemcpyAsync(s.d_ref.get(), traj_ref, I * N * 6 * 8, H2D, st));
    HIP_TRY(hipMemcpyAsync(s.d_npoly.get(), n_poly, I * 4, H2D, st));
    HIP_TRY(hipMemcpyAsync(s.d_nrows.get(), n_rows_static, I * P * 4, H2D, st));
    HIP_TRY(hipMemcpyAsync(s.d_A.get(), A_static, I * P * RS * 3 * 8, H2D, st));
    HIP_TRY(hipMemcpyAsync(s.d_b.get(), b_static, I * P * RS * 8, H2D, st));
    HIP_TRY(hipMemcpyAsync(s.d_plans.get(), plans_all, (size_t)n_rob * (N + 1) * 9 * 8, H2D, st));
    HIP_TRY(hipMemcpyAsync(s.d_has.get(), has_plan, (size_t)n_rob, H2D, st));
  }
  int rc = hdsm_replan_device(handle, n_inst, n_rob, s.d_agent.get(), s.d_state.get(), s.d_ref.get(), s.d_npoly.get(), s.d_nrows.get(),
                              s.d_A.get(), s.d_b.get(), s.d_plans.get(), s.d_has.get(), s.d_traj.get(), s.d_ctrl.get(), s.d_used.get(),
                              s.d_status.get(), s.d_obj.get(), st);
  if (rc) return rc;
  rc = rescue_if_flagged(h, st);
  if (rc) return rc;
  // Outputs are "left untouched" for instances without a solution. The caller's arrays are not uploaded to seed the device
  // copies (a megabyte each way per 1024 agents): the results come back into a pinned staging block of the handle and only
  // the instances that HAVE a solution are copied into the caller's arrays.
  const size_t trj = (N + 1) * 9, ctl = N * 3;
  void* dp[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  {  // page-locked output arrays (hdsm_host_register, every array inside a registered range): delivered by the device, filtered there
    void* hp[5] = {traj_out, ctrl_out, obj, status, poly_used};
    const size_t hb[5] = {I * trj * 8, I * ctl * 8, I * 8, I * 4, I * P};
    bool mapped = true;
    for (int k = 0; k < 5 && mapped; ++k) mapped = mapped_host_range(hp[k], hb[k], &dp[k]);
    if (!mapped) dp[0] = nullptr;
  }
  if (dp[0] != nullptr) {
    hipLaunchKernelGGL(k_deliver, dim3((unsigned)((I + 3) / 4)), dim3(256), 0, st, n_inst, (int)trj, (int)ctl, (int)P, s.d_traj.get(), s.d_ctrl.get(), s.d_obj.get(),
                       s.d_status.get(), s.d_used.get(), static_cast<double*>(dp[0]), static_cast<double*>(dp[1]), static_cast<double*>(dp[2]),
                       static_cast<int32_t*>(dp[3]), static_cast<uint8_t*>(dp[4]));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
  } else {
    HIP_TRY(s.out.ensure(I * (trj * 8 + ctl * 8 + 8 + 4 + P)));
    double* o_traj = static_cast<double*>(s.out.get());
    double* o_ctrl = o_traj + I * trj;
    double* o_obj = o_ctrl + I * ctl;
    int32_t* o_status = reinterpret_cast<int32_t*>(o_obj + I);
    uint8_t* o_used = reinterpret_cast<uint8_t*>(o_status + I);
    HIP_TRY(hipMemcpyAsync(o_traj, s.d_traj.get(), I * trj * 8, D2H, st));
    HIP_TRY(hipMemcpyAsync(o_ctrl, s.d_ctrl.get(), I * ctl * 8, D2H, st));
    HIP_TRY(hipMemcpyAsync(o_obj, s.d_obj.get(), I * 8, D2H, st));
    HIP_TRY(hipMemcpyAsync(o_status, s.d_status.get(), I * 4, D2H, st));
    HIP_TRY(hipMemcpyAsync(o_used, s.d_used.get(), I * P, D2H, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (size_t k = 0; k < I; ++k) {
      status[k] = o_status[k];
      if (o_status[k] == HDSM_NO_SOLUTION) continue;
      std::memcpy(traj_out + k * trj, o_traj + k * trj, trj * 8);
      std::memcpy(ctrl_out + k * ctl, o_ctrl + k * ctl, ctl * 8);
      std::memcpy(poly_used + k * P, o_used + k * P, P);
      obj[k] = o_obj[k];
    }
  }
  // (one exit for both delivery paths: anything added after the download applies to registered callers too)
  return HDSM_OK;
}

}  // extern "C"
