// dswarm_world.hip — map updates in flight for the device-resident loop (ABI 1.7; semantics in hdsm_swarm.h): boxes of values into the
// device world or the resident raw grid (k_box_put), the region pre-processing of map_kernels.hip behind a raw box, and the
// polyhedron cache of k_corridor (swarm_kernels.hip) kept honest (k_cache_invalidate) — with the downloads and counters that go with them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <string>
#include <vector>

#include "dswarm.h"

using namespace hdsm_dswarm;

namespace {

// values [bdim[2]][bdim[1]][bdim[0]] into the box lo .. lo + bdim of a grid [.][ny][nx]: thread <-> up to four voxels of one row
__global__ __launch_bounds__(256) void k_box_put(const int8_t* __restrict__ vals, int8_t* __restrict__ grid, int nx, int ny, int lx, int ly, int lz,
                                                 int bx, int by, int bz) {
  const int qpr = (bx + 3) / 4, rows = by * bz;
  for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < qpr * rows; q += gridDim.x * blockDim.x) {
    const int row = q / qpr, x0 = (q - row * qpr) * 4, z = row / by, y = row - z * by;
    const int n = bx - x0 < 4 ? bx - x0 : 4;
    const int8_t* in = vals + (size_t)row * bx + x0;
    int8_t* out = grid + ((size_t)(lz + z) * ny + (ly + y)) * nx + (lx + x0);
    if (n == 4) __builtin_memcpy(out, in, 4);
    else
      for (int k = 0; k < n; ++k) out[k] = in[k];
  }
}

// The polyhedron cache after voxels lo .. hi (inclusive, world voxels) were written: one lane per (agent, entry). An entry whose
// decomposition could have looked at a written voxel — its seed +- (rad + 1): wave_map_radius and one voxel of margin — is dropped,
// the others stay. A dropped entry becomes a hole: its seed voxel is set to kCacheHole, so it is never found again, and the agent's
// n / next are left as they are; the next polyhedron k_corridor records goes into the first hole, so the agent keeps its six slots.
// (An entry is read only through the comparison of its seed voxel, so nothing else of it needs clearing.)
__global__ __launch_bounds__(256) void k_cache_invalidate(PolyCache* cache, int n_agents, int rad, int lx, int ly, int lz, int hx, int hy, int hz,
                                                          unsigned long long* dropped) {
  const int t = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (t >= n_agents * CACHE_POLYS) return;
  PolyCache& pc = cache[t / CACHE_POLYS];
  const int e = t % CACHE_POLYS;
  if (e >= pc.n || pc.seed_w[e][0] == kCacheHole) return;
  const int sx = pc.seed_w[e][0], sy = pc.seed_w[e][1], sz = pc.seed_w[e][2];
  const bool meets = sx + rad >= lx && sx - rad <= hx && sy + rad >= ly && sy - rad <= hy && sz + rad >= lz && sz - rad <= hz;
  if (!meets) return;
  pc.seed_w[e][0] = kCacheHole;
  atomicAdd(dropped, 1ull);
}

// the two refusals more than one entry point gives
int no_world() { return fail(HDSM_ERR_BAD_ARG, "the dswarm has no world (hdsm_swarm_set_world before hdsm_dswarm_create)"); }
int no_raw_world() { return fail(HDSM_ERR_BAD_ARG, "no raw world is resident (hdsm_dswarm_set_raw_world)"); }

// the box lo .. lo + bdim inside the device world? (0 empty, 1 yes, < 0 an error)
int world_box(DSwarm* d, const int32_t* lo, const int32_t* bdim) {
  if (!d || !lo || !bdim) return fail(HDSM_ERR_BAD_ARG, "null argument");
  if (!d->c.has_world) return no_world();
  for (int ax = 0; ax < 3; ++ax)
    if (bdim[ax] < 0 || lo[ax] < 0 || lo[ax] > d->c.wdim[ax] || bdim[ax] > d->c.wdim[ax] - lo[ax])
      return fail(HDSM_ERR_BAD_ARG, "the box does not lie inside the world");
  return (bdim[0] == 0 || bdim[1] == 0 || bdim[2] == 0) ? 0 : 1;
}

// values (device) into the box of `grid` (the device world or the resident raw grid), on st
int put_box(DSwarm* d, const int8_t* d_vals, int8_t* grid, const int32_t lo[3], const int32_t bdim[3], hipStream_t st) {
  const int quads = ((bdim[0] + 3) / 4) * bdim[1] * bdim[2];
  hipLaunchKernelGGL(k_box_put, dim3((unsigned)std::min((quads + 255) / 256, 4096)), dim3(256), 0, st, d_vals, grid, d->c.wdim[0], d->c.wdim[1], lo[0],
                     lo[1], lo[2], bdim[0], bdim[1], bdim[2]);
  HIP_TRY(hipGetLastError());
  return HDSM_OK;
}

// drops the cache entries that could have looked at the written voxels wlo .. wlo + wdim (NULL: every entry), on st, and books the update
int invalidate(DSwarm* d, const int32_t* wlo, const int32_t* wdim, hipStream_t st) {
  if (!d->edits.d_dropped) HIP_TRY(d->edits.d_dropped.alloc_zeroed(1));
  if (!d->d_cache || d->n_local == 0) return HDSM_OK;
  const int rad = hdsm_cd::wave_map_radius(d->c.n_it_decomp) + 1;
  const int big = 1 << 29;
  const int l[3] = {wlo ? wlo[0] : -big, wlo ? wlo[1] : -big, wlo ? wlo[2] : -big};
  const int h[3] = {wlo ? wlo[0] + wdim[0] - 1 : big, wlo ? wlo[1] + wdim[1] - 1 : big, wlo ? wlo[2] + wdim[2] - 1 : big};
  hipLaunchKernelGGL(k_cache_invalidate, dim3((unsigned)((d->n_local * CACHE_POLYS + 255) / 256)), dim3(256), 0, st, d->d_cache.get(), d->n_local, rad, l[0],
                     l[1], l[2], h[0], h[1], h[2], d->edits.d_dropped.get());
  HIP_TRY(hipGetLastError());
  return HDSM_OK;
}

// the host values of a box into the staging buffer (the device is idle: the callers have synchronised)
int stage_box(DSwarm* d, const int8_t* values, const int32_t bdim[3]) {
  WorldEdits& w = d->edits;
  const size_t bytes = (size_t)bdim[0] * bdim[1] * bdim[2];
  if (bytes > w.edit_cap) {
    w.edit_cap = 0;
    HIP_TRY(w.d_edit.alloc(bytes));
    w.edit_cap = bytes;
  }
  HIP_TRY(hipMemcpy(w.d_edit.get(), values, bytes, hipMemcpyHostToDevice));
  return HDSM_OK;
}

}  // namespace

extern "C" {

int hdsm_dswarm_update_world(void* dswarm, const int8_t* values, const int32_t lo[3], const int32_t bdim[3]) {
  DSwarm* d = as_dswarm(dswarm);
  const int k = world_box(d, lo, bdim);
  if (k <= 0) return k;
  if (!values) return fail(HDSM_ERR_BAD_ARG, "null values");
  if (int rc = device_idle(d)) return rc;
  if (int rc = stage_box(d, values, bdim)) return rc;
  if (int rc = put_box(d, d->edits.d_edit.get(), d->d_world.get(), lo, bdim, nullptr)) return rc;
  if (int rc = invalidate(d, lo, bdim, nullptr)) return rc;
  HIP_TRY(hipDeviceSynchronize());
  ++d->edits.updates, d->edits.voxels += (long long)bdim[0] * bdim[1] * bdim[2];
  return HDSM_OK;
}

int hdsm_dswarm_set_raw_world(void* dswarm, const hdsm_map_config* map_cfg, const int8_t* raw_full) {
  DSwarm* d = as_dswarm(dswarm);
  if (!d || !map_cfg || !raw_full) return fail(HDSM_ERR_BAD_ARG, "null argument");
  if (!d->c.has_world) return no_world();
  const size_t vox = d->voxels();
  for (size_t i = 0; i < vox; ++i)
    if (raw_full[i] != -1 && raw_full[i] != 0 && raw_full[i] != 100) return fail(HDSM_ERR_BAD_ARG, "a raw grid holds -1, 0 and 100 only");
  if (vox < 4 || vox >= ((size_t)1 << 30)) return fail(HDSM_ERR_BAD_ARG, "a raw world needs 4 .. 2^30 - 1 voxels");
  const int32_t zero[3] = {0, 0, 0};
  const size_t scr = hdsm_map_region_scratch_bytes(map_cfg, d->c.wdim, zero, d->c.wdim);  // the largest box; >= the full form's 2 vox
  if (scr == 0) return fail(HDSM_ERR_BAD_ARG, std::string("map configuration: ") + hdsm_map_last_error());
  if (int rc = device_idle(d)) return rc;
  WorldEdits& w = d->edits;
  {  // out of the dswarm until the new grid is in it: an allocation or a copy that fails leaves no raw world resident
    DevBuf<int8_t> raw = std::move(w.d_raw);
    DevBuf<uint8_t> map_scr = std::move(w.d_map_scr);
    if (!raw) HIP_TRY(raw.alloc(vox));
    if (!map_scr) HIP_TRY(map_scr.alloc(scr));
    HIP_TRY(hipMemcpy(raw.get(), raw_full, vox, hipMemcpyHostToDevice));
    w.d_raw = std::move(raw), w.d_map_scr = std::move(map_scr);
  }
  // (the arguments were checked above: what can still fail is a launch, and then the device world is no longer the old one —
  // the cache is emptied on that way out too)
  const int rc = hdsm_map_preprocess_device(d->device, map_cfg, 1, d->c.wdim, w.d_raw.get(), d->d_world.get(), w.d_map_scr.get(), nullptr);
  if (rc == HDSM_OK) w.mcfg = *map_cfg;
  const int rc2 = invalidate(d, nullptr, nullptr, nullptr);
  if (rc) {
    w.d_raw.reset();  // (no raw world is resident: the raw update calls keep refusing)
    return fail(rc, std::string("hdsm_map_preprocess_device: ") + hdsm_map_last_error());
  }
  if (rc2) return rc2;
  HIP_TRY(hipDeviceSynchronize());
  return HDSM_OK;
}

int hdsm_dswarm_update_world_raw_device(void* dswarm, const int8_t* d_raw_values, const int32_t lo[3], const int32_t bdim[3], void* hip_stream) {
  DSwarm* d = as_dswarm(dswarm);
  const int k = world_box(d, lo, bdim);
  if (k < 0) return k;
  WorldEdits& w = d->edits;
  if (!w.d_raw) return no_raw_world();
  if (k == 0) return HDSM_OK;
  if (!d_raw_values) return fail(HDSM_ERR_BAD_ARG, "null values");
  HIP_TRY(hipSetDevice(d->device));
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  int32_t wlo[3], wdim[3];
  if (int rc = hdsm_map_region_extent(&w.mcfg, d->c.wdim, lo, bdim, wlo, wdim, nullptr, nullptr)) return fail(rc, hdsm_map_last_error());
  if (int rc = put_box(d, d_raw_values, w.d_raw.get(), lo, bdim, st)) return rc;
  if (int rc = hdsm_map_preprocess_region_device(d->device, &w.mcfg, d->c.wdim, w.d_raw.get(), d->d_world.get(), lo, bdim, w.d_map_scr.get(), st))
    return fail(rc, std::string("hdsm_map_preprocess_region_device: ") + hdsm_map_last_error());
  if (int rc = invalidate(d, wlo, wdim, st)) return rc;
  ++w.updates, w.voxels += (long long)wdim[0] * wdim[1] * wdim[2];
  return HDSM_OK;
}

int hdsm_dswarm_update_world_raw(void* dswarm, const int8_t* raw_values, const int32_t lo[3], const int32_t bdim[3]) {
  DSwarm* d = as_dswarm(dswarm);
  const int k = world_box(d, lo, bdim);
  if (k < 0) return k;
  if (!d->edits.d_raw) return no_raw_world();
  if (k == 0) return HDSM_OK;
  if (!raw_values) return fail(HDSM_ERR_BAD_ARG, "null values");
  if (int rc = device_idle(d)) return rc;
  if (int rc = stage_box(d, raw_values, bdim)) return rc;
  if (int rc = hdsm_dswarm_update_world_raw_device(dswarm, d->edits.d_edit.get(), lo, bdim, nullptr)) return rc;
  HIP_TRY(hipDeviceSynchronize());
  return HDSM_OK;
}

int hdsm_dswarm_download_world(void* dswarm, int8_t* world) {
  DSwarm* d = as_dswarm(dswarm);
  if (!d || !world) return fail(HDSM_ERR_BAD_ARG, "null argument");
  if (!d->c.has_world) return fail(HDSM_ERR_BAD_ARG, "the dswarm has no world");
  if (int rc = device_idle(d)) return rc;
  HIP_TRY(hipMemcpy(world, d->d_world.get(), d->voxels(), hipMemcpyDeviceToHost));
  return HDSM_OK;
}

int hdsm_dswarm_world_stats(void* dswarm, int64_t out[4]) {
  DSwarm* d = as_dswarm(dswarm);
  if (!d || !out) return fail(HDSM_ERR_BAD_ARG, "null argument");
  out[0] = d->edits.updates, out[1] = d->edits.voxels, out[2] = 0, out[3] = d->edits.d_raw ? 1 : 0;
  if (!d->edits.d_dropped) return HDSM_OK;
  if (int rc = device_idle(d)) return rc;
  unsigned long long n = 0;
  HIP_TRY(hipMemcpy(&n, d->edits.d_dropped.get(), sizeof n, hipMemcpyDeviceToHost));
  out[2] = (int64_t)n;
  return HDSM_OK;
}

// The polyhedron cache of the device corridor (k_corridor, PolyCache), summed over the shard's agents since hdsm_dswarm_create:
// out[0] polyhedra asked for, out[1] formed from a cached structure recorded in the same local grid, out[2] formed from one recorded in
// ANOTHER grid at the same height (the interior rule), out[3] = 1 if the cache is on (HDSM_POLY_CACHE, a world is set), else 0.
int hdsm_dswarm_cache_stats(void* dswarm, int64_t out[4]) {
  DSwarm* d = as_dswarm(dswarm);
  if (!d || !out) return fail(HDSM_ERR_BAD_ARG, "null argument");
  out[0] = out[1] = out[2] = out[3] = 0;
  if (!d->d_cache || d->n_local == 0) return HDSM_OK;
  if (int rc = device_idle(d)) return rc;
  out[3] = 1;
  // (only the four counters of every entry travel: one strided 2-D copy)
  std::vector<int32_t> cnt((size_t)d->n_local * 4);
  HIP_TRY(hipMemcpy2D(cnt.data(), 16, reinterpret_cast<const char*>(d->d_cache.get()) + offsetof(PolyCache, asked), sizeof(PolyCache), 16,
                      (size_t)d->n_local, hipMemcpyDeviceToHost));
  for (int k = 0; k < d->n_local; ++k) out[0] += cnt[4 * (size_t)k], out[1] += cnt[4 * (size_t)k + 1], out[2] += cnt[4 * (size_t)k + 2];
  return HDSM_OK;
}

}  // extern "C"
