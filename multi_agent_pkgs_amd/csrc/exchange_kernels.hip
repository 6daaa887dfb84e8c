// exchange_kernels.hip — the multi-GPU exchange of the published plans: one RCCL all-gather per replan round in place of the
// reference's DDS all-to-all (AC:46-48, 610-677), the has_plan flag travelling inside the record. The only file that includes RCCL.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <cstring>
#include <new>
#include <string>

#include "../../include/hdsm.h"
#include "hdsm_entry.h"

using namespace hdsm_entry;

namespace {

// hdsm_publish_device / hdsm_exchange_device: the has_plan flag travels inside the record (first entry NaN = no plan)
__global__ __launch_bounds__(256) void k_publish(int rec, int per, int n_local, const double* __restrict__ traj,
                                                 const uint8_t* __restrict__ has_local, double* __restrict__ out) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)per * rec) return;
  const int k = (int)(idx / rec), e = (int)(idx % rec);
  const bool has = k < n_local && has_local[k];
  double v = has ? traj[idx] : 0.0;
  if (!has && e == 0) v = __longlong_as_double(0x7ff8000000000000LL);
  out[idx] = v;
}
__global__ __launch_bounds__(256) void k_has_from_sentinel(int rec, int n, const double* __restrict__ plans,
                                                           uint8_t* __restrict__ has) {
  const int k = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (k >= n) return;
  const double v = plans[(int64_t)k * rec];
  has[k] = (v == v) ? 1 : 0;
}

}  // namespace

extern "C" {

// ---- multi-GPU exchange (RCCL) -------------------------------------------------------------------------------------
struct Comm {
  ncclComm_t nccl = nullptr;
  int rank = 0, world = 1, device = 0, rec = 0;  // rec = doubles per published record, (N + 1) * 9
};

#define NCCL_TRY(expr)                                                                                 \
  do {                                                                                                  \
    ncclResult_t r_ = (expr);                                                                           \
    if (r_ != ncclSuccess) return set_err(HDSM_ERR_COMM, std::string(#expr) + ": " + ncclGetErrorString(r_)); \
  } while (0)

int hdsm_comm_unique_id(uint8_t id[HDSM_COMM_ID_BYTES]) {
  static_assert(sizeof(ncclUniqueId) <= HDSM_COMM_ID_BYTES, "ncclUniqueId does not fit HDSM_COMM_ID_BYTES");
  if (!id) return set_err(HDSM_ERR_BAD_ARG, "null id");
  ncclUniqueId u;
  NCCL_TRY(ncclGetUniqueId(&u));
  std::memset(id, 0, HDSM_COMM_ID_BYTES);
  std::memcpy(id, &u, sizeof u);
  return HDSM_OK;
}

int hdsm_comm_create(void* handle, const uint8_t id[HDSM_COMM_ID_BYTES], int32_t rank, int32_t world, void** comm) {
  Handle* h = static_cast<Handle*>(handle);
  if (!h || !id || !comm || world < 1 || rank < 0 || rank >= world) return set_err(HDSM_ERR_BAD_ARG, "bad hdsm_comm_create argument");
  *comm = nullptr;
  HIP_TRY(hipSetDevice(h->device));
  Comm* c = new (std::nothrow) Comm;
  if (!c) return set_err(HDSM_ERR_DEVICE, "out of host memory");
  c->rank = rank, c->world = world, c->device = h->device, c->rec = (h->N + 1) * 9;
  ncclUniqueId u;
  std::memcpy(&u, id, sizeof u);
  ncclResult_t r = ncclCommInitRank(&c->nccl, world, u, rank);
  if (r != ncclSuccess) {
    delete c;
    return set_err(HDSM_ERR_COMM, std::string("ncclCommInitRank: ") + ncclGetErrorString(r));
  }
  *comm = c;
  return HDSM_OK;
}

int hdsm_comm_info(void* comm, int32_t* rank, int32_t* world) {
  Comm* c = static_cast<Comm*>(comm);
  if (!c) return set_err(HDSM_ERR_BAD_ARG, "null comm");
  int r = -1, w = -1;
  NCCL_TRY(ncclCommUserRank(c->nccl, &r));   // what RCCL itself says, not what the caller passed
  NCCL_TRY(ncclCommCount(c->nccl, &w));
  if (rank) *rank = r;
  if (world) *world = w;
  return HDSM_OK;
}

void hdsm_comm_destroy(void* comm) {
  Comm* c = static_cast<Comm*>(comm);
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->nccl) (void)ncclCommDestroy(c->nccl);
  delete c;
}

int hdsm_publish_device(void* handle, int32_t per, int32_t n_local, const double* traj, const uint8_t* has_plan_local,
                        double* plans_local, void* hip_stream) {
  Handle* h = static_cast<Handle*>(handle);
  if (!h || per < 0 || n_local < 0 || n_local > per) return set_err(HDSM_ERR_BAD_ARG, "bad hdsm_publish_device argument");
  if (per == 0) return HDSM_OK;
  if (!traj || !has_plan_local || !plans_local) return set_err(HDSM_ERR_BAD_ARG, "null array argument");
  HIP_TRY(hipSetDevice(h->device));
  const int rec = (h->N + 1) * 9;
  const int64_t tot = (int64_t)per * rec;
  hipLaunchKernelGGL(k_publish, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(hip_stream), rec, per,
                     n_local, traj, has_plan_local, plans_local);
  HIP_TRY(hipGetLastError());
  return HDSM_OK;
}

int hdsm_exchange_device(void* comm, int32_t per, const double* plans_local, double* plans_all, uint8_t* has_plan_all,
                         void* hip_stream) {
  Comm* c = static_cast<Comm*>(comm);
  if (!c || per < 0) return set_err(HDSM_ERR_BAD_ARG, "bad hdsm_exchange_device argument");
  if (per == 0) return HDSM_OK;
  if (!plans_local || !plans_all || !has_plan_all) return set_err(HDSM_ERR_BAD_ARG, "null array argument");
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  // ONE collective per replan round: rank r's shard lands at plans_all + r * per * rec (in place if it already is there)
  NCCL_TRY(ncclAllGather(plans_local, plans_all, (size_t)per * c->rec, ncclDouble, c->nccl, st));
  const int n = per * c->world;
  hipLaunchKernelGGL(k_has_from_sentinel, dim3((n + 255) / 256), dim3(256), 0, st, c->rec, n, plans_all, has_plan_all);
  HIP_TRY(hipGetLastError());
  return HDSM_OK;
}

}  // extern "C"
