// map_kernels.hip — next row f4: the map pre-processing stencils of mapping_util's MapBuilder (map_builder.cpp:209-216)
// on a batch of int8 voxel grids: SetUncertainToUnknown (MB:331-362), InflateObstacles and CreatePotentialField
// (voxel_grid.cpp:252-297, "VG"). See include/hdsm.h.
//
// The reference stamps a mask around every occupied voxel (scatter). Both masks are RADIAL — membership and value of
// an offset depend on its length only (CreateMask, VG:192-226) and the value decreases with the length — so
//   inflated(v)  <=>  the nearest occupied voxel, searched in the cube |d| <= rn per axis, is at a length the mask holds
//   potential(v)  =   mask value at the length of the nearest occupied voxel in that cube
// and the nearest length comes from an exact, windowed, separable squared distance transform: three 1-D min-plus
// passes (x, y, z) of 2 rn + 1 taps each instead of (2 rn + 1)^3 stamps — 33 taps for the shipped potential field
// instead of ~1200. Squared lengths are small integers (<= 3 rn^2 <= 255 for rn <= 9), kept in one byte; the mask
// becomes a table indexed by squared length, built on the host with the reference's own double arithmetic
// (hypot, pow, the int8 cast) and checked to be the same for every offset of equal squared length.
// Byte work, HBM/L2-bound: thread <-> voxel, x fastest, so every tap of every pass is a coalesced byte stream.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/hdsm.h"
#include "device_mem.h"

namespace {

constexpr int kRnMax = 9;        // 3 * 9^2 = 243 < 255
constexpr uint8_t kFar = 255;    // "no occupied voxel in the window"

struct MapTables {
  int rn0, rn1, rn2;             // cube of SetUncertainToUnknown, window of the inflation / potential masks
  uint8_t in1[256];              // squared length -> inflation mask holds it
  int8_t val2[256];              // squared length -> potential value (0 = not in the mask or no effect)
};

struct Dims {
  int nx, ny, nz;
  int vox;                       // voxels per grid (< 2^31); the grid of the batch is blockIdx.y
};

// Every thread owns FOUR consecutive voxels of one grid (x fastest): taps are fetched as one (unaligned) 32-bit load
// per row instead of four byte loads, and the index arithmetic is 32-bit and shared by the four.
constexpr int VPT = 4;

__device__ __forceinline__ uint32_t load4(const void* p) {  // 4 bytes at any alignment
  uint32_t v;
  __builtin_memcpy(&v, p, 4);
  return v;
}
__device__ __forceinline__ void store4(void* p, uint32_t v) { __builtin_memcpy(p, &v, 4); }
__device__ __forceinline__ int byte_of(uint32_t w, int k) { return (int)((w >> (8 * k)) & 0xffu); }

// Packed arithmetic on the four voxels of a quad: two registers of 2 x u16 (v_pk_add_u16 / v_pk_min_u16), bytes moved
// in and out with v_perm_b32. A tap then costs 7 instructions for four voxels instead of ~40 scalar ones.
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ u16x2 as_pk(uint32_t w) { return __builtin_bit_cast(u16x2, w); }
__device__ __forceinline__ uint32_t as_u32(u16x2 v) { return __builtin_bit_cast(uint32_t, v); }
__device__ __forceinline__ u16x2 widen_lo(uint32_t w) { return as_pk(__builtin_amdgcn_perm(0u, w, 0x0c010c00u)); }  // bytes 0, 1
__device__ __forceinline__ u16x2 widen_hi(uint32_t w) { return as_pk(__builtin_amdgcn_perm(0u, w, 0x0c030c02u)); }  // bytes 2, 3
__device__ __forceinline__ uint32_t narrow(u16x2 lo, u16x2 hi) {  // values already <= 255
  return __builtin_amdgcn_perm(as_u32(hi), as_u32(lo), 0x06040200u);
}
// per byte: 0x00 where the byte of w equals `key`, 0xff elsewhere
__device__ __forceinline__ uint32_t far_unless(uint32_t w, uint32_t key4) {
  const uint32_t x = w ^ key4;                                                 // zero byte <=> match
  const uint32_t nz = (((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u;   // bit 7 set <=> byte non-zero
  return (nz >> 7) * 255u;
}

struct Pos {  // coordinates of voxel p + k for k < VPT (a quad may run over the end of a row / slice)
  int x[VPT], y[VPT], z[VPT];
};
__device__ __forceinline__ Pos coords(const Dims& d, int p) {
  Pos c;
  const unsigned slice = (unsigned)d.nx * (unsigned)d.ny;
  int z = (int)((unsigned)p / slice);
  const unsigned r = (unsigned)p - (unsigned)z * slice;
  int y = (int)(r / (unsigned)d.nx), x = (int)(r - (unsigned)y * (unsigned)d.nx);
#pragma unroll
  for (int k = 0; k < VPT; ++k) {
    c.x[k] = x, c.y[k] = y, c.z[k] = z;
    if (++x == d.nx) {
      x = 0;
      if (++y == d.ny) y = 0, ++z;
    }
  }
  return c;
}

// One pass of a windowed, separable min-plus transform along AXIS (0 x, 1 y, 2 z), 2 rn + 1 taps.
//   SRC 0: taps read the byte field of the previous pass          cost = src + w(t)
//   SRC 1: taps read the int8 grid, occupied voxels (== 100)       cost = w(t)            (distance transforms)
//   SRC 2: taps read the int8 grid, unknown voxels (== -1) that lie at least rn voxels inside the grid (x pass only)
//   SQ   : w(t) = t^2 (Euclidean: squared distance to the nearest source voxel in the cube |d| <= rn), else w = 0
//          (Chebyshev: is there a source voxel in the cube)
//   LAST : 0 write the byte field; otherwise merge into the grid read at the voxel itself and write the grid:
//          1 inflation (VG:252-278): nearest occupied voxel at a length the mask holds -> occupied, unknown voxels too
//          2 potential field (VG:280-297): known voxels take max(own value, mask value at the nearest occupied voxel)
//          3 SetUncertainToUnknown (MB:331-362): not occupied and an inner unknown voxel in the cube -> unknown
template <int AXIS, int SRC, int LAST, bool SQ>
__global__ __launch_bounds__(256) void k_pass(Dims d, int rn, MapTables tb, const int8_t* __restrict__ grid,
                                              const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int8_t* __restrict__ out) {
  const size_t g0 = (size_t)blockIdx.y * d.vox;
  const int stride = (AXIS == 0) ? 1 : (AXIS == 1 ? d.nx : d.nx * d.ny);
  const int len = (AXIS == 0) ? d.nx : (AXIS == 1 ? d.ny : d.nz);
  const uint8_t* taps = (SRC == 0) ? src + g0 : reinterpret_cast<const uint8_t*>(grid) + g0;
  for (int p = (blockIdx.x * blockDim.x + threadIdx.x) * VPT; p < d.vox; p += gridDim.x * blockDim.x * VPT) {
    const int nq = (d.vox - p < VPT) ? d.vox - p : VPT;
    const Pos c = coords(d, p);
    // per voxel: the taps t in [lo, hi] stay inside the grid (and, SRC 2, land on an inner voxel of an inner row)
    int lo[VPT], hi[VPT], lo_all = -rn, hi_all = rn;
#pragma unroll
    for (int k = 0; k < VPT; ++k) {
      const int pos = (AXIS == 0) ? c.x[k] : (AXIS == 1 ? c.y[k] : c.z[k]);
      int a = -pos, b = len - 1 - pos;
      if (SRC == 2) {
        a += rn, b -= rn;
        if (c.y[k] < rn || c.y[k] >= d.ny - rn || c.z[k] < rn || c.z[k] >= d.nz - rn) a = 1, b = 0;
      }
      lo[k] = a > -rn ? a : -rn, hi[k] = b < rn ? b : rn;
      if (k >= nq) lo[k] = 1, hi[k] = 0;
      lo_all = lo[k] > lo_all ? lo[k] : lo_all, hi_all = hi[k] < hi_all ? hi[k] : hi_all;
    }
    u16x2 blo = as_pk(0x00ff00ffu), bhi = as_pk(0x00ff00ffu);
    constexpr int TB = 11;  // taps whose loads are in flight together (the whole window for rn <= 5)
    for (int t0 = -rn; t0 <= rn; t0 += TB) {
      uint32_t w[TB];
#pragma unroll
      for (int u = 0; u < TB; ++u) {
        const int t = t0 + u;
        w[u] = 0xffffffffu;
        if (t > rn) continue;  // (wave-uniform: short windows issue only their own taps)
        // the four taps sit next to each other in memory; at the ends of the grid the load is moved inside and the
        // bytes are shifted back into place (what falls off is masked below: those taps are outside the grid)
        const int q = p + t * stride;
        int qc = q < 0 ? 0 : q;
        qc = (qc > d.vox - VPT) ? d.vox - VPT : qc;
        uint32_t v = load4(taps + qc);
        const int sh = (q - qc) * 8;
        v = (sh == 0) ? v : (sh > 0 ? (sh > 31 ? 0u : v >> sh) : (sh < -31 ? 0u : v << -sh));
        w[u] = v;
      }
#pragma unroll
      for (int u = 0; u < TB; ++u) {
        const int t = t0 + u;
        if (t > rn) continue;
        uint32_t wu = w[u];
        if (SRC == 1) wu = far_unless(wu, 0x64646464u);  // occupied (100) -> 0, anything else -> far
        if (SRC == 2) wu = far_unless(wu, 0xffffffffu);  // unknown (-1) -> 0
        const unsigned short tt = SQ ? (unsigned short)(t * t) : (unsigned short)0;
        const u16x2 add = {tt, tt};
        u16x2 vlo = widen_lo(wu) + add, vhi = widen_hi(wu) + add;  // far + t^2 >= 255 stays "far" after the clamp
        if (t < lo_all || t > hi_all) {  // some voxel of the quad has no such tap
          const uint32_t m0 = (t < lo[0] || t > hi[0]) ? 0x0000ffffu : 0u, m1 = (t < lo[1] || t > hi[1]) ? 0xffff0000u : 0u;
          const uint32_t m2 = (t < lo[2] || t > hi[2]) ? 0x0000ffffu : 0u, m3 = (t < lo[3] || t > hi[3]) ? 0xffff0000u : 0u;
          vlo = as_pk(as_u32(vlo) | m0 | m1), vhi = as_pk(as_u32(vhi) | m2 | m3);
        }
        blo = __builtin_elementwise_min(blo, vlo);
        bhi = __builtin_elementwise_min(bhi, vhi);
      }
    }
    const uint32_t best4 = narrow(blo, bhi);  // four squared distances (or 255)
    if (LAST == 0) {
      if (nq == VPT) store4(dst + g0 + p, best4);
      else
        for (int k = 0; k < nq; ++k) dst[g0 + p + k] = (uint8_t)byte_of(best4, k);
    } else {
      // merge into the grid read at the voxels themselves
      uint32_t g4 = 0;
      if (nq == VPT) g4 = load4(grid + g0 + p);
      else
        for (int k = 0; k < nq; ++k) g4 |= (uint32_t)(uint8_t)grid[g0 + p + k] << (8 * k);
      uint32_t r4 = 0;
#pragma unroll
      for (int k = 0; k < VPT; ++k) {
        const int8_t v = (int8_t)byte_of(g4, k);
        const int bk = byte_of(best4, k);
        int8_t r = v;
        if (bk != kFar) {
          if (LAST == 1) {
            if (tb.in1[bk]) r = 100;
          } else if (LAST == 2) {
            if (v != -1) {
              const int8_t pv = tb.val2[bk];
              if (pv > v) r = pv;
            }
          } else if (v != 100) {
            r = -1;
          }
        }
        r4 |= (uint32_t)(uint8_t)r << (8 * k);
      }
      if (nq == VPT) store4(out + g0 + p, r4);
      else
        for (int k = 0; k < nq; ++k) out[g0 + p + k] = (int8_t)byte_of(r4, k);
    }
  }
}

// ---- the region form: the raw grid changed inside a box D only ----------------------------------------------------------------
// The three stages are local with Chebyshev radii rn0, rn1, rn2, so the processed grid can change only inside W = D (+) R,
// R = rn0 + rn1 + rn2, and W is exact once the stages have run on the working box B = D (+) 2R (each stage's result is valid on
// its input region shrunk by its radius). Both boxes are clipped to the grid: where a face of B is a face of the grid, "no tap
// beyond it" is the grid's own rule; where it is not, it lies R voxels or more outside W and what the passes make of the missing
// taps never reaches a voxel that is written. So B is gathered into a dense field of its own and the SAME nine passes (k_pass, the
// packed quads included) run on it as on a small grid. The one rule that is about the world's borders and not the field's — a
// voxel seeds SetUncertainToUnknown only rn0 voxels or more inside the GRID — is decided here, in global coordinates, while
// gathering: k_region_gather writes the seeds as a byte field (0 seed, 255 none) and the first pass reads it as any distance field.
struct Region {
  int nx, ny, nz;     // the grid
  int bx, by, bz;     // B: origin in the grid
  int bnx, bny, bnz;  //    extents
  int wx, wy, wz;     // W: origin in the grid
  int wnx, wny, wnz;  //    extents
};

// thread <-> up to four voxels of one row of the box (x fastest): the rows of the grid are read and written as contiguous bytes
__global__ __launch_bounds__(256) void k_region_gather(Region r, int rn0, const int8_t* __restrict__ raw, int8_t* __restrict__ box,
                                                       uint8_t* __restrict__ seeds) {
  const int qpr = (r.bnx + VPT - 1) / VPT, rows = r.bny * r.bnz;
  for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < qpr * rows; q += gridDim.x * blockDim.x) {
    const int row = q / qpr, x0 = (q - row * qpr) * VPT, z = row / r.bny, y = row - z * r.bny;
    const int gy = y + r.by, gz = z + r.bz;
    const int n = r.bnx - x0 < VPT ? r.bnx - x0 : VPT;
    const bool inner_row = gy >= rn0 && gy < r.ny - rn0 && gz >= rn0 && gz < r.nz - rn0;
    const int8_t* in = raw + ((size_t)gz * r.ny + gy) * r.nx + (r.bx + x0);
    const size_t o = (size_t)row * r.bnx + x0;
    uint32_t v4 = 0;
    if (n == VPT) v4 = load4(in);
    else
      for (int k = 0; k < n; ++k) v4 |= (uint32_t)(uint8_t)in[k] << (8 * k);
    uint32_t s4 = inner_row ? far_unless(v4, 0xffffffffu) : 0xffffffffu;
#pragma unroll
    for (int k = 0; k < VPT; ++k) {
      const int gx = r.bx + x0 + k;
      if (gx < rn0 || gx >= r.nx - rn0) s4 |= 0xffu << (8 * k);
    }
    if (n == VPT) store4(box + o, v4), store4(seeds + o, s4);
    else
      for (int k = 0; k < n; ++k) box[o + k] = (int8_t)byte_of(v4, k), seeds[o + k] = (uint8_t)byte_of(s4, k);
  }
}

// ... and the voxels of W leave the box for the processed grid: nothing outside W is written
__global__ __launch_bounds__(256) void k_region_scatter(Region r, const int8_t* __restrict__ box, int8_t* __restrict__ out) {
  const int qpr = (r.wnx + VPT - 1) / VPT, rows = r.wny * r.wnz;
  for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < qpr * rows; q += gridDim.x * blockDim.x) {
    const int row = q / qpr, x0 = (q - row * qpr) * VPT, z = row / r.wny, y = row - z * r.wny;
    const int gy = y + r.wy, gz = z + r.wz, gx = r.wx + x0;
    const int n = r.wnx - x0 < VPT ? r.wnx - x0 : VPT;
    const int8_t* in = box + ((size_t)(gz - r.bz) * r.bny + (gy - r.by)) * r.bnx + (gx - r.bx);
    int8_t* o = out + ((size_t)gz * r.ny + gy) * r.nx + gx;
    if (n == VPT) store4(o, load4(in));
    else
      for (int k = 0; k < n; ++k) o[k] = in[k];
  }
}

thread_local std::string g_map_err;

// CreateMask (VG:192-226) folded into tables indexed by squared length; fails if two offsets of equal squared length
// disagree (they do not for any setting tried; the check keeps the equivalence honest).
int build_tables_uncached(const hdsm_map_config& c, MapTables* tb);
// (an edit in flight asks for the tables of the same configuration every call: the last ones built are kept per thread)
int build_tables(const hdsm_map_config& c, MapTables* tb) {
  thread_local bool have = false;
  thread_local hdsm_map_config last_cfg;
  thread_local MapTables last_tb;
  if (have && last_cfg.voxel_size == c.voxel_size && last_cfg.inflation_dist == c.inflation_dist && last_cfg.potential_dist == c.potential_dist &&
      last_cfg.potential_pow == c.potential_pow) {
    *tb = last_tb;
    return HDSM_OK;
  }
  const int rc = build_tables_uncached(c, tb);
  if (rc == HDSM_OK) last_cfg = c, last_tb = *tb, have = true;
  return rc;
}
int build_tables_uncached(const hdsm_map_config& c, MapTables* tb) {
  std::memset(tb, 0, sizeof *tb);
  const double res = c.voxel_size;
  tb->rn0 = (int)std::ceil(c.inflation_dist / res);
  tb->rn1 = (int)std::ceil(c.inflation_dist / res);
  tb->rn2 = (int)std::ceil(c.potential_dist / res);
  if (tb->rn1 > kRnMax || tb->rn2 > kRnMax || tb->rn1 < 0 || tb->rn2 < 0) {
    g_map_err = "mask radius above 9 voxels";
    return HDSM_ERR_BAD_ARG;
  }
  for (int pass = 0; pass < 2; ++pass) {
    const double mask_dist = pass == 0 ? c.inflation_dist : c.potential_dist;
    const double power = pass == 0 ? 1.0 : (double)c.potential_pow;
    const int rn = pass == 0 ? tb->rn1 : tb->rn2;
    int seen[256];
    for (int k = 0; k < 256; ++k) seen[k] = -1000;
    if (!(mask_dist > 0)) continue;
    for (int n0 = -rn; n0 <= rn; ++n0)
      for (int n1 = -rn; n1 <= rn; ++n1)
        for (int n2 = -rn; n2 <= rn; ++n2) {
          double dist = std::hypot(std::hypot((double)n0, (double)n1), (double)n2);
          dist = std::fabs(dist - 1);
          int val = -999;  // not in the mask
          if (!(dist * res >= mask_dist)) {
            const double h = 100.0 * std::pow(1 - std::hypot(std::hypot((double)n0, (double)n1), (double)n2) / (rn + 1), power);
            if (h > 1e-3) val = (int)(int8_t)h;
          }
          const int s = n0 * n0 + n1 * n1 + n2 * n2;
          if (seen[s] == -1000) seen[s] = val;
          else if (seen[s] != val) {
            g_map_err = "mask is not a function of the squared offset length for these parameters";
            return HDSM_ERR_BAD_ARG;
          }
        }
    int last = 1000;
    for (int s = 0; s < 256; ++s) {
      if (seen[s] == -1000 || seen[s] == -999) continue;
      if (pass == 0) tb->in1[s] = 1;
      else tb->val2[s] = (int8_t)seen[s];
      if (s > 0) {  // the nearest-voxel argument needs a value that does not increase with the length
        if (seen[s] > last) {
          g_map_err = "mask value increases with the offset length";
          return HDSM_ERR_BAD_ARG;
        }
        last = seen[s];
      }
    }
    // the origin (length 0) is in the mask only if voxel_size < mask_dist; an occupied voxel keeps its value either way
    // membership must also be "closed downwards" from the largest length held (lengths >= 1)
    bool ended = false;
    for (int s = 1; s < 256; ++s) {
      if (seen[s] == -1000) continue;
      const bool in = seen[s] != -999;
      if (!in) ended = true;
      else if (ended) {
        g_map_err = "mask membership is not monotone in the offset length";
        return HDSM_ERR_BAD_ARG;
      }
    }
    if (pass == 0 && seen[0] == -999) tb->in1[0] = 1;  // length 0 = the voxel itself is occupied: stays occupied
    if (pass == 1 && seen[0] == -999) tb->val2[0] = 0;
  }
  return HDSM_OK;
}

int run_device(const hdsm_map_config* cfg, int32_t n_grids, const int32_t dim[3], const int8_t* d_in, int8_t* d_out,
               uint8_t* scratch, hipStream_t st) {
  MapTables tb;
  if (int rc = build_tables(*cfg, &tb)) return rc;
  const int64_t vox64 = (int64_t)dim[0] * dim[1] * dim[2];
  if (vox64 < VPT) {
    g_map_err = "grids of fewer than 4 voxels are not supported";
    return HDSM_ERR_BAD_ARG;
  }
  if (vox64 >= (int64_t)1 << 30 || n_grids > 65535) {
    g_map_err = "grid too large (>= 2^30 voxels) or more than 65535 grids in one batch";
    return HDSM_ERR_CAPACITY;
  }
  Dims d{dim[0], dim[1], dim[2], (int)vox64};
  const size_t total = (size_t)vox64 * n_grids;
  uint8_t* a = scratch;
  uint8_t* b = scratch + total;
  int8_t* stage0 = reinterpret_cast<int8_t*>(b);  // output of SetUncertainToUnknown, until the inflation is applied
  const int quads = (int)((vox64 + VPT - 1) / VPT);
  const dim3 grid((unsigned)std::min<int>((quads + 255) / 256, 4096), (unsigned)n_grids), block(256);
  const uint8_t* nou = nullptr;
  const int8_t* nog = nullptr;
  uint8_t* o8 = reinterpret_cast<uint8_t*>(d_out);
  int8_t* no8 = nullptr;
  uint8_t* nod = nullptr;
  // SetUncertainToUnknown: box dilation of the inner unknown voxels, merged into scratch b (= stage0)
  hipLaunchKernelGGL((k_pass<0, 2, 0, false>), grid, block, 0, st, d, tb.rn0, tb, d_in, nou, a, no8);
  hipLaunchKernelGGL((k_pass<1, 0, 0, false>), grid, block, 0, st, d, tb.rn0, tb, nog, a, o8, no8);
  hipLaunchKernelGGL((k_pass<2, 0, 3, false>), grid, block, 0, st, d, tb.rn0, tb, d_in, o8, nod, stage0);
  // inflation: squared distances to the occupied voxels (x, y passes), merged by the z pass into scratch a
  hipLaunchKernelGGL((k_pass<0, 1, 0, true>), grid, block, 0, st, d, tb.rn1, tb, stage0, nou, a, no8);
  hipLaunchKernelGGL((k_pass<1, 0, 0, true>), grid, block, 0, st, d, tb.rn1, tb, nog, a, o8, no8);
  int8_t* inflated = reinterpret_cast<int8_t*>(a);
  hipLaunchKernelGGL((k_pass<2, 0, 1, true>), grid, block, 0, st, d, tb.rn1, tb, stage0, o8, nod, inflated);
  // potential field on the inflated grid, merged by the z pass into the output
  hipLaunchKernelGGL((k_pass<0, 1, 0, true>), grid, block, 0, st, d, tb.rn2, tb, inflated, nou, o8, no8);
  hipLaunchKernelGGL((k_pass<1, 0, 0, true>), grid, block, 0, st, d, tb.rn2, tb, nog, o8, b, no8);
  hipLaunchKernelGGL((k_pass<2, 0, 2, true>), grid, block, 0, st, d, tb.rn2, tb, inflated, b, nod, d_out);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    g_map_err = hipGetErrorString(e);
    return HDSM_ERR_DEVICE;
  }
  return HDSM_OK;
}

bool bad_args(const hdsm_map_config* cfg, int32_t n_grids, const int32_t* dim, const void* in, const void* out) {
  return !cfg || !dim || !in || !out || n_grids < 0 || dim[0] < 1 || dim[1] < 1 || dim[2] < 1 || !(cfg->voxel_size > 0) ||
         cfg->inflation_dist < 0 || cfg->potential_dist < 0 || cfg->potential_pow < 0;
}

// W and B of an edit box (lo, bdim) that lies inside the grid; an empty box gives empty W and B. A working box of fewer than four
// voxels (R = 0 and a tiny edit) is widened to four — the passes fetch quads — which costs nothing in exactness: a wider B is
// still a B.
void region_boxes(const MapTables& tb, const int32_t dim[3], const int32_t lo[3], const int32_t bdim[3], Region* r) {
  const int R = tb.rn0 + tb.rn1 + tb.rn2;
  int wl[3], wh[3], bl[3], bh[3];
  for (int ax = 0; ax < 3; ++ax) {
    if (bdim[ax] == 0) {
      *r = Region{dim[0], dim[1], dim[2], 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
      return;
    }
    wl[ax] = std::max(lo[ax] - R, 0), wh[ax] = std::min(lo[ax] + bdim[ax] + R, dim[ax]);
    bl[ax] = std::max(lo[ax] - 2 * R, 0), bh[ax] = std::min(lo[ax] + bdim[ax] + 2 * R, dim[ax]);
  }
  auto vox = [&]() { return (int64_t)(bh[0] - bl[0]) * (bh[1] - bl[1]) * (bh[2] - bl[2]); };
  for (bool grew = true; vox() < VPT && grew;) {
    grew = false;
    for (int ax = 0; ax < 3 && vox() < VPT; ++ax) {
      if (bh[ax] < dim[ax]) ++bh[ax], grew = true;
      else if (bl[ax] > 0) --bl[ax], grew = true;
    }
  }
  *r = Region{dim[0], dim[1], dim[2], bl[0], bl[1], bl[2], bh[0] - bl[0], bh[1] - bl[1], bh[2] - bl[2],
              wl[0], wl[1], wl[2], wh[0] - wl[0], wh[1] - wl[1], wh[2] - wl[2]};
}

bool bad_region_args(const hdsm_map_config* cfg, const int32_t* dim, const int32_t* lo, const int32_t* bdim) {
  if (!cfg || !dim || !lo || !bdim || dim[0] < 1 || dim[1] < 1 || dim[2] < 1 || !(cfg->voxel_size > 0) || cfg->inflation_dist < 0 ||
      cfg->potential_dist < 0 || cfg->potential_pow < 0) {
    g_map_err = "null or invalid argument";
    return true;
  }
  for (int ax = 0; ax < 3; ++ax)
    if (bdim[ax] < 0 || lo[ax] < 0 || lo[ax] > dim[ax] || bdim[ax] > dim[ax] - lo[ax]) {
      g_map_err = "the edit box does not lie inside the grid";
      return true;
    }
  return false;
}

constexpr int kRegionFields = 4;  // box-sized byte fields of the region form: the raw box and three working fields

int run_region(const hdsm_map_config* cfg, const int32_t dim[3], const int8_t* d_raw, int8_t* d_out, const int32_t lo[3], const int32_t bdim[3],
               uint8_t* scratch, hipStream_t st) {
  MapTables tb;
  if (int rc = build_tables(*cfg, &tb)) return rc;
  const int64_t gvox = (int64_t)dim[0] * dim[1] * dim[2];
  if (gvox < VPT) {
    g_map_err = "grids of fewer than 4 voxels are not supported";
    return HDSM_ERR_BAD_ARG;
  }
  if (gvox >= (int64_t)1 << 30) {
    g_map_err = "grid too large (>= 2^30 voxels)";
    return HDSM_ERR_CAPACITY;
  }
  Region r;
  region_boxes(tb, dim, lo, bdim, &r);
  if (r.wnx == 0) return HDSM_OK;
  const int vox = r.bnx * r.bny * r.bnz;
  Dims d{r.bnx, r.bny, r.bnz, vox};
  int8_t* rawbox = reinterpret_cast<int8_t*>(scratch);
  uint8_t* a = scratch + (size_t)vox;
  uint8_t* b = scratch + 2 * (size_t)vox;
  uint8_t* c = scratch + 3 * (size_t)vox;
  int8_t* stage0 = reinterpret_cast<int8_t*>(b);
  int8_t* inflated = reinterpret_cast<int8_t*>(a);
  int8_t* final_box = reinterpret_cast<int8_t*>(c);
  const dim3 block(256);
  auto blocks_for = [](int nx, int rows) { return dim3((unsigned)std::min<int>((((nx + VPT - 1) / VPT) * rows + 255) / 256, 4096)); };
  const dim3 grid((unsigned)std::min<int>(((vox + VPT - 1) / VPT + 255) / 256, 4096));
  const uint8_t* nou = nullptr;
  const int8_t* nog = nullptr;
  int8_t* no8 = nullptr;
  uint8_t* nod = nullptr;
  hipLaunchKernelGGL(k_region_gather, blocks_for(r.bnx, r.bny * r.bnz), block, 0, st, r, tb.rn0, d_raw, rawbox, c);
  // the nine passes of run_device on the box (the seeds of SetUncertainToUnknown come from the gather: pass one is a plain x pass)
  hipLaunchKernelGGL((k_pass<0, 0, 0, false>), grid, block, 0, st, d, tb.rn0, tb, nog, c, a, no8);
  hipLaunchKernelGGL((k_pass<1, 0, 0, false>), grid, block, 0, st, d, tb.rn0, tb, nog, a, c, no8);
  hipLaunchKernelGGL((k_pass<2, 0, 3, false>), grid, block, 0, st, d, tb.rn0, tb, rawbox, c, nod, stage0);
  hipLaunchKernelGGL((k_pass<0, 1, 0, true>), grid, block, 0, st, d, tb.rn1, tb, stage0, nou, a, no8);
  hipLaunchKernelGGL((k_pass<1, 0, 0, true>), grid, block, 0, st, d, tb.rn1, tb, nog, a, c, no8);
  hipLaunchKernelGGL((k_pass<2, 0, 1, true>), grid, block, 0, st, d, tb.rn1, tb, stage0, c, nod, inflated);
  hipLaunchKernelGGL((k_pass<0, 1, 0, true>), grid, block, 0, st, d, tb.rn2, tb, inflated, nou, c, no8);
  hipLaunchKernelGGL((k_pass<1, 0, 0, true>), grid, block, 0, st, d, tb.rn2, tb, nog, c, b, no8);
  hipLaunchKernelGGL((k_pass<2, 0, 2, true>), grid, block, 0, st, d, tb.rn2, tb, inflated, b, nod, final_box);
  hipLaunchKernelGGL(k_region_scatter, blocks_for(r.wnx, r.wny * r.wnz), block, 0, st, r, final_box, d_out);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    g_map_err = hipGetErrorString(e);
    return HDSM_ERR_DEVICE;
  }
  return HDSM_OK;
}

}  // namespace

extern "C" {

const char* hdsm_map_last_error(void) { return g_map_err.c_str(); }

int hdsm_map_preprocess_device(int32_t device, const hdsm_map_config* cfg, int32_t n_grids, const int32_t dim[3],
                               const int8_t* grids_in, int8_t* grids_out, void* scratch, void* hip_stream) {
  if (bad_args(cfg, n_grids, dim, grids_in, grids_out) || !scratch) return HDSM_ERR_BAD_ARG;
  if (n_grids == 0) return HDSM_OK;
  if (hipSetDevice(device) != hipSuccess) return HDSM_ERR_NO_DEVICE;
  return run_device(cfg, n_grids, dim, grids_in, grids_out, static_cast<uint8_t*>(scratch), static_cast<hipStream_t>(hip_stream));
}

int hdsm_map_preprocess(int32_t device, const hdsm_map_config* cfg, int32_t n_grids, const int32_t dim[3],
                        const int8_t* grids_in, int8_t* grids_out) {
  if (bad_args(cfg, n_grids, dim, grids_in, grids_out)) return HDSM_ERR_BAD_ARG;
  if (n_grids == 0) return HDSM_OK;
  int cnt = 0;
  if (hipGetDeviceCount(&cnt) != hipSuccess || cnt <= device || hipSetDevice(device) != hipSuccess) {
    g_map_err = "no HIP device";
    return HDSM_ERR_NO_DEVICE;
  }
  const size_t total = (size_t)dim[0] * dim[1] * dim[2] * n_grids;
  hdsm_mem::DevBuf<int8_t> d_in, d_out;
  hdsm_mem::DevBuf<uint8_t> d_scr;
  hdsm_mem::FirstError ok;
  ok(d_in.alloc(total));
  if (ok.ok()) ok(d_out.alloc(total));
  if (ok.ok()) ok(d_scr.alloc(2 * total));
  int rc = HDSM_OK;
  if (ok.ok()) ok(hipMemcpy(d_in.get(), grids_in, total, hipMemcpyHostToDevice));
  if (ok.ok()) rc = run_device(cfg, n_grids, dim, d_in.get(), d_out.get(), d_scr.get(), nullptr);
  if (ok.ok() && rc == HDSM_OK) ok(hipMemcpy(grids_out, d_out.get(), total, hipMemcpyDeviceToHost));
  if (!ok.ok()) {
    g_map_err = hipGetErrorString(ok.e);
    return HDSM_ERR_DEVICE;
  }
  return rc;
}

int hdsm_map_region_extent(const hdsm_map_config* cfg, const int32_t dim[3], const int32_t lo[3], const int32_t bdim[3], int32_t write_lo[3],
                           int32_t write_dim[3], int32_t work_lo[3], int32_t work_dim[3]) {
  if (bad_region_args(cfg, dim, lo, bdim)) return HDSM_ERR_BAD_ARG;
  MapTables tb;
  if (int rc = build_tables(*cfg, &tb)) return rc;
  Region r;
  region_boxes(tb, dim, lo, bdim, &r);
  if (write_lo) write_lo[0] = r.wx, write_lo[1] = r.wy, write_lo[2] = r.wz;
  if (write_dim) write_dim[0] = r.wnx, write_dim[1] = r.wny, write_dim[2] = r.wnz;
  if (work_lo) work_lo[0] = r.bx, work_lo[1] = r.by, work_lo[2] = r.bz;
  if (work_dim) work_dim[0] = r.bnx, work_dim[1] = r.bny, work_dim[2] = r.bnz;
  return HDSM_OK;
}

size_t hdsm_map_region_scratch_bytes(const hdsm_map_config* cfg, const int32_t dim[3], const int32_t lo[3], const int32_t bdim[3]) {
  int32_t wd[3];
  if (hdsm_map_region_extent(cfg, dim, lo, bdim, nullptr, nullptr, nullptr, wd) != HDSM_OK) return 0;
  return (size_t)kRegionFields * wd[0] * wd[1] * wd[2];
}

int hdsm_map_preprocess_region_device(int32_t device, const hdsm_map_config* cfg, const int32_t dim[3], const int8_t* raw_full, int8_t* out_full,
                                      const int32_t lo[3], const int32_t bdim[3], void* scratch, void* hip_stream) {
  if (bad_region_args(cfg, dim, lo, bdim)) return HDSM_ERR_BAD_ARG;
  if (!raw_full || !out_full) {
    g_map_err = "null grid";
    return HDSM_ERR_BAD_ARG;
  }
  if (bdim[0] == 0 || bdim[1] == 0 || bdim[2] == 0) return HDSM_OK;
  if (!scratch) {
    g_map_err = "null scratch";
    return HDSM_ERR_BAD_ARG;
  }
  if (hipSetDevice(device) != hipSuccess) return HDSM_ERR_NO_DEVICE;
  return run_region(cfg, dim, raw_full, out_full, lo, bdim, static_cast<uint8_t*>(scratch), static_cast<hipStream_t>(hip_stream));
}

int hdsm_map_preprocess_region(int32_t device, const hdsm_map_config* cfg, const int32_t dim[3], const int8_t* raw_full, int8_t* out_full,
                               const int32_t lo[3], const int32_t bdim[3]) {
  if (bad_region_args(cfg, dim, lo, bdim)) return HDSM_ERR_BAD_ARG;
  if (!raw_full || !out_full) {
    g_map_err = "null grid";
    return HDSM_ERR_BAD_ARG;
  }
  if (bdim[0] == 0 || bdim[1] == 0 || bdim[2] == 0) return HDSM_OK;
  int cnt = 0;
  if (hipGetDeviceCount(&cnt) != hipSuccess || cnt <= device || hipSetDevice(device) != hipSuccess) {
    g_map_err = "no HIP device";
    return HDSM_ERR_NO_DEVICE;
  }
  const size_t total = (size_t)dim[0] * dim[1] * dim[2], scr = hdsm_map_region_scratch_bytes(cfg, dim, lo, bdim);
  hdsm_mem::DevBuf<int8_t> d_raw, d_out;
  hdsm_mem::DevBuf<uint8_t> d_scr;
  hdsm_mem::FirstError ok;
  ok(d_raw.alloc(total));
  if (ok.ok()) ok(d_out.alloc(total));
  if (ok.ok()) ok(d_scr.alloc(scr));
  int rc = HDSM_OK;
  if (ok.ok()) ok(hipMemcpy(d_raw.get(), raw_full, total, hipMemcpyHostToDevice));
  if (ok.ok()) ok(hipMemcpy(d_out.get(), out_full, total, hipMemcpyHostToDevice));
  if (ok.ok()) rc = run_region(cfg, dim, d_raw.get(), d_out.get(), lo, bdim, d_scr.get(), nullptr);
  if (ok.ok() && rc == HDSM_OK) ok(hipMemcpy(out_full, d_out.get(), total, hipMemcpyDeviceToHost));
  if (!ok.ok()) {
    g_map_err = hipGetErrorString(ok.e);
    return HDSM_ERR_DEVICE;
  }
  return rc;
}

}  // extern "C"
