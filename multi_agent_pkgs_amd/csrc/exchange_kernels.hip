// exchange_kernels.hip — the multi-GPU exchange of the published plans: one RCCL all-gather per replan round in place of the
// reference's DDS all-to-all (AC:46-48, 610-677), the has_plan flag travelling inside the record. The only file that includes RCCL.
// Local ranks (hdsm_comm_create_local): the ranks of one process gather with ONE kernel per rank, k_gather_local, that reads the other
// ranks' send buffers through plain pointers — the same code on one device and, with peer access, on several.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/hdsm.h"
#include "hdsm_entry.h"
#include "hdsm_internal.h"
#include "local_group.h"

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


// The all-gather of local ranks and the flags from the sentinel in one pass (hdsm_dswarm_round_ranks: one launch per rank and round
// in place of ncclAllGather + k_has_from_sentinel). Slot s = r * per + k of the plans buffer is record k of rank r's send buffer
// send[r]; a shard is ONE contiguous run of len = per * rec doubles, so it is moved as such: thread j of a shard takes the doubles
// 2j - h and 2j - h + 1, h = 1 when the destination starts on an odd double. Where source and destination agree modulo 16 bytes the
// pair is one 16-byte access on both sides and the ragged head (h) and tail go as single doubles; where they do not, as two 8-byte
// accesses. Nothing but 8-byte alignment is assumed (a record is 792 B at H = 10). Whoever moves element 0 of a record sets the
// slot's flag. No LDS, no scratch, no atomics; the grid follows the bytes (launch_gather_local), grid-stride beyond 2048 blocks.
// (A send-buffer address comes out of the table, so the compiler cannot see that it is global memory: said here, or every read of a
// record is a flat load.)
typedef double pair_t __attribute__((ext_vector_type(2)));
#define HDSM_GLOBAL_AS __attribute__((address_space(1)))
__global__ __launch_bounds__(256) void k_gather_local(int world, int per, int rec, const double* const* __restrict__ send,
                                                      double* __restrict__ plans, uint8_t* __restrict__ has) {
  const int64_t len = (int64_t)per * rec, chunks = len / 2 + 1, total = chunks * world;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int r = (int)(t / chunks);
    const int64_t j = t - r * chunks;
    const HDSM_GLOBAL_AS double* src = (const HDSM_GLOBAL_AS double*)send[r];
    double* dst = plans + r * len;
    const bool wide = (((uintptr_t)src ^ (uintptr_t)dst) & 8) == 0;
    const int h = wide ? (int)(((uintptr_t)dst >> 3) & 1) : 0;
    const int64_t e0 = 2 * j - h, e1 = e0 + 1;
    const bool in0 = e0 >= 0 && e0 < len, in1 = e1 < len;
    double v0 = 0.0, v1 = 0.0;
    if (wide && in0 && in1) {
      const pair_t v = *(const HDSM_GLOBAL_AS pair_t*)(src + e0);
      *reinterpret_cast<pair_t*>(dst + e0) = v;
      v0 = v.x, v1 = v.y;
    } else {
      if (in0) v0 = src[e0], dst[e0] = v0;
      if (in1) v1 = src[e1], dst[e1] = v1;
    }
    if (in0 && e0 % rec == 0) has[(int64_t)r * per + e0 / rec] = (v0 == v0) ? 1 : 0;
    if (in1 && e1 % rec == 0) has[(int64_t)r * per + e1 / rec] = (v1 == v1) ? 1 : 0;
  }
}
#undef HDSM_GLOBAL_AS

}  // namespace

extern "C" {

// ---- multi-GPU exchange (RCCL), and local ranks ---------------------------------------------------------------------
enum CommKind { COMM_RCCL = 0, COMM_LOCAL = 1 };
struct Comm {
  ncclComm_t nccl = nullptr;
  int rank = 0, world = 1, device = 0, rec = 0;  // rec = doubles per published record, (N + 1) * 9
  CommKind kind = COMM_RCCL;
  hdsm_local::Group* group = nullptr;  // COMM_LOCAL: what the ranks of the group share (local_group.h); gone with its last member
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
  if (c->kind == COMM_LOCAL) {
    if (rank) *rank = c->rank;
    if (world) *world = c->world;
    return HDSM_OK;
  }
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
  if (c->kind == COMM_LOCAL) {
    if (c->group && c->group->members == 1)  // the last member: a round in flight may still read the tables and wait for the events
      for (int r = 0; r < c->group->world; ++r)
        if (hipSetDevice(c->group->ranks[r].device) == hipSuccess) (void)hipDeviceSynchronize();
    if (c->group) (void)hdsm_local::Group::leave(c->group);
  } else if (c->nccl) {
    (void)ncclCommDestroy(c->nccl);
  }
  delete c;
}

int hdsm_comm_create_local(int32_t world, void* const* handles, void** comms) {
  if (world < 1 || !handles || !comms) return set_err(HDSM_ERR_BAD_ARG, "bad hdsm_comm_create_local argument");
  for (int r = 0; r < world; ++r) comms[r] = nullptr;
  std::vector<int> dev((size_t)world), uniq;
  for (int r = 0; r < world; ++r) {
    const Handle* h = static_cast<const Handle*>(handles[r]);
    if (!h) return set_err(HDSM_ERR_BAD_ARG, "hdsm_comm_create_local: null handle of rank " + std::to_string(r));
    if (h->N != static_cast<const Handle*>(handles[0])->N)
      return set_err(HDSM_ERR_BAD_ARG, "hdsm_comm_create_local: the handles of ranks 0 and " + std::to_string(r) + " differ in n_hor");
    dev[(size_t)r] = h->device;
    bool seen = false;
    for (int d : uniq) seen = seen || d == h->device;
    if (!seen) uniq.push_back(h->device);
  }
  // ranks on different devices read each other's send buffers: every pair of devices, both directions, checked before one is enabled
  for (size_t a = 0; a < uniq.size(); ++a)
    for (size_t b = 0; b < uniq.size(); ++b) {
      if (a == b) continue;
      int can = 0;
      HIP_TRY(hipDeviceCanAccessPeer(&can, uniq[a], uniq[b]));
      if (!can)
        return set_err(HDSM_ERR_COMM, "hdsm_comm_create_local: device " + std::to_string(uniq[a]) + " cannot access the memory of device " +
                                          std::to_string(uniq[b]) + " (no peer access between the two)");
    }
  for (size_t a = 0; a < uniq.size(); ++a)
    for (size_t b = 0; b < uniq.size(); ++b) {
      if (a == b) continue;
      HIP_TRY(hipSetDevice(uniq[a]));
      const hipError_t e = hipDeviceEnablePeerAccess(uniq[b], 0);
      if (e == hipErrorPeerAccessAlreadyEnabled) (void)hipGetLastError();
      else HIP_TRY(e);
    }
  const int rec = (static_cast<const Handle*>(handles[0])->N + 1) * 9;
  hdsm_local::Group* g = nullptr;
  const hipError_t e = hdsm_local::Group::create(world, rec, dev.data(), [](int d) { return hipSetDevice(d); }, &g);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return set_err(HDSM_ERR_DEVICE, std::string("hdsm_comm_create_local: ") + hipGetErrorString(e));
  }
  for (int r = 0; r < world; ++r) {
    Comm* c = new (std::nothrow) Comm;
    if (!c) {
      for (int q = 0; q < r; ++q) delete static_cast<Comm*>(comms[q]), comms[q] = nullptr;
      delete g;
      return set_err(HDSM_ERR_DEVICE, "out of host memory");
    }
    c->rank = r, c->world = world, c->device = dev[(size_t)r], c->rec = rec, c->kind = COMM_LOCAL, c->group = g;
    g->join();
    comms[r] = c;
  }
  return HDSM_OK;
}

// ---- local ranks: what hdsm_dswarm_round_ranks needs of the group (hdsm_internal.h) ----
int hdsm_internal_comm_kind(void* comm, int32_t* device) {
  const Comm* c = static_cast<const Comm*>(comm);
  if (!c) return -1;
  if (device) *device = c->device;
  return c->kind == COMM_LOCAL ? 1 : 0;
}

int hdsm_internal_local_check(int32_t world, void* const* comms, int32_t rec) {
  if (world < 1 || !comms) return set_err(HDSM_ERR_BAD_ARG, "bad argument");
  const hdsm_local::Group* g = nullptr;
  for (int r = 0; r < world; ++r) {
    const Comm* c = static_cast<const Comm*>(comms[r]);
    if (!c) return set_err(HDSM_ERR_BAD_ARG, "null communicator of rank " + std::to_string(r));
    if (c->kind != COMM_LOCAL) return set_err(HDSM_ERR_BAD_ARG, "the communicator given for rank " + std::to_string(r) + " is not a local one (hdsm_comm_create_local)");
    if (r == 0) g = c->group;
    if (c->group != g) return set_err(HDSM_ERR_BAD_ARG, "the communicators of ranks 0 and " + std::to_string(r) + " belong to different local groups");
    if (c->world != world) return set_err(HDSM_ERR_BAD_ARG, "the local group has " + std::to_string(c->world) + " ranks, the call names " + std::to_string(world));
    if (c->rank != r)  // (with the two checks above: every rank of the group exactly once)
      return set_err(HDSM_ERR_BAD_ARG, "position " + std::to_string(r) + " holds the communicator of rank " + std::to_string(c->rank) + ": every rank once, in rank order");
    if (c->rec != rec) return set_err(HDSM_ERR_BAD_ARG, "the local group was made for another n_hor than the shards'");
  }
  return HDSM_OK;
}

int hdsm_internal_local_bind(int32_t world, void* const* comms, const double* const* send, int32_t per) {
  if (world < 1 || !comms || !send || per < 0) return set_err(HDSM_ERR_BAD_ARG, "bad argument");
  hdsm_local::Group* g = static_cast<Comm*>(comms[0])->group;
  bool same = g->per == per;
  for (int r = 0; r < world; ++r) same = same && g->ranks[r].send == send[r];
  if (same) return HDSM_OK;
  // other shards than the round before (or the first round): a gather in flight may still read the old table
  for (int r = 0; r < world && g->flown; ++r) {
    HIP_TRY(hipSetDevice(g->ranks[r].device));
    HIP_TRY(hipDeviceSynchronize());
  }
  for (int r = 0; r < world; ++r) {
    if (g->ranks[r].table_rank != r) continue;
    HIP_TRY(hipSetDevice(g->ranks[r].device));
    HIP_TRY(hipMemcpy(g->ranks[r].d_table.get(), send, (size_t)world * sizeof(const double*), hipMemcpyHostToDevice));
  }
  for (int r = 0; r < world; ++r) g->ranks[r].send = send[r];
  g->per = per;
  return HDSM_OK;
}

int hdsm_internal_local_commit_gate(void* comm, void* hip_stream) {
  const Comm* c = static_cast<const Comm*>(comm);
  if (!c || c->kind != COMM_LOCAL) return set_err(HDSM_ERR_BAD_ARG, "not a local communicator");
  if (!c->group->flown) return HDSM_OK;  // (no gather yet: nobody reads the send buffer)
  for (int q = 0; q < c->world; ++q) HIP_TRY(hipStreamWaitEvent(static_cast<hipStream_t>(hip_stream), c->group->ranks[q].gathered.get(), 0));
  return HDSM_OK;
}

int hdsm_internal_local_published(void* comm, void* hip_stream) {
  const Comm* c = static_cast<const Comm*>(comm);
  if (!c || c->kind != COMM_LOCAL) return set_err(HDSM_ERR_BAD_ARG, "not a local communicator");
  HIP_TRY(hipEventRecord(c->group->ranks[c->rank].published.get(), static_cast<hipStream_t>(hip_stream)));
  return HDSM_OK;
}

int hdsm_internal_gather_local_launch(int32_t world, int32_t per, int32_t rec, const double* const* d_send, double* plans_all,
                                      uint8_t* has_plan_all, void* hip_stream) {
  if (world < 1 || per < 0 || rec < 1) return set_err(HDSM_ERR_BAD_ARG, "bad argument");
  if (per == 0) return HDSM_OK;
  if (!d_send || !plans_all || !has_plan_all) return set_err(HDSM_ERR_BAD_ARG, "null array argument");
  const int64_t threads = ((int64_t)per * rec / 2 + 1) * world;  // one per 16 bytes of the plans buffer (and a ragged end per shard)
  const int64_t blocks = (threads + 255) / 256;
  hipLaunchKernelGGL(k_gather_local, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, static_cast<hipStream_t>(hip_stream), world, per, rec,
                     d_send, plans_all, has_plan_all);
  HIP_TRY(hipGetLastError());
  return HDSM_OK;
}

int hdsm_internal_local_gather(void* comm, double* plans_all, uint8_t* has_plan_all, void* hip_stream, void* mark) {
  const Comm* c = static_cast<const Comm*>(comm);
  if (!c || c->kind != COMM_LOCAL) return set_err(HDSM_ERR_BAD_ARG, "not a local communicator");
  hdsm_local::Group* g = c->group;
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  for (int q = 0; q < c->world; ++q) HIP_TRY(hipStreamWaitEvent(st, g->ranks[q].published.get(), 0));
  if (mark) HIP_TRY(hipEventRecord(static_cast<hipEvent_t>(mark), st));
  if (int rc = hdsm_internal_gather_local_launch(c->world, g->per, c->rec, g->table(c->rank), plans_all, has_plan_all, st)) return rc;
  HIP_TRY(hipEventRecord(g->ranks[c->rank].gathered.get(), st));
  g->flown = true;
  return HDSM_OK;
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
  if (c->kind == COMM_LOCAL) return set_err(HDSM_ERR_BAD_ARG, HDSM_LOCAL_COMM_REFUSED);
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
