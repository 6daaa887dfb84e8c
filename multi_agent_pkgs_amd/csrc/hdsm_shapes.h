// The launch shapes of the solver kernel and the rule that picks one. hdsm_api.hip instantiates and launches every row of
// HDSM_SOLVER_SHAPES, and the CPU execution of the device source (tests/wave_emu/wave_emu.cpp) runs the same rows and exports
// pick_shape, so the two cannot drift apart. Why each capacity is what it is: the comments at the kernels in hdsm_api.hip.
// No HIP dependency: g++ compiles this header.
#pragma once

#include "hdsm_types.h"

namespace hdsm {
// staging-area capacities (staged neighbour rows, Shm::cand)
constexpr int CMAX30 = 1536;     // k_replan<32, ..>: n <= 30, one workgroup per CU
constexpr int CMAX48 = 1024;     // k_replan<48, ..>: n <= 48, one workgroup per CU
constexpr int CMAX_DUO = 768;    // k_replan_duo: n <= 30, two 256-thread workgroups per CU
constexpr int CMAX_TRI = 384;    // k_replan_tri: n <= 30, three 128-thread workgroups per CU
constexpr int CMAX_QUAD = 256;   // k_replan_quad: n <= 30, four 128-thread workgroups per CU, small LDS layout
constexpr int CMAX_DUO48 = 720;  // k_replan_duo48: n > 30, two 128-thread workgroups per CU

// X(name, kernel, NV, CMAX, SMALL, threads, per_cu): kernel<NV, CMAX, threads> runs hdsm::Solver<NV, CMAX, SMALL> with `threads`
// threads per workgroup, `per_cu` workgroups resident per CU. A row's place in the list is its hdsm::Shape.
#define HDSM_SOLVER_SHAPES(X)                                            \
  X(replan30_64, k_replan, 32, hdsm::CMAX30, false, 64, 1)               \
  X(replan30, k_replan, 32, hdsm::CMAX30, false, 256, 1)                 \
  X(replan48_64, k_replan, 48, hdsm::CMAX48, false, 64, 1)               \
  X(replan48, k_replan, 48, hdsm::CMAX48, false, 256, 1)                 \
  X(duo, k_replan_duo, 32, hdsm::CMAX_DUO, false, 256, 2)                \
  X(tri, k_replan_tri, 32, hdsm::CMAX_TRI, false, 128, 3)                \
  X(quad, k_replan_quad, 32, hdsm::CMAX_QUAD, true, 128, 4)              \
  X(duo48, k_replan_duo48, 48, hdsm::CMAX_DUO48, false, 128, 2)

#define HDSM_SHAPE_ENUM(name, kernel, nv, cmax, small, threads, per_cu) SHAPE_##name,
enum Shape : int { HDSM_SOLVER_SHAPES(HDSM_SHAPE_ENUM) NUM_SHAPES };
#undef HDSM_SHAPE_ENUM

struct ShapeRow {
  int cmax, per_cu;
};
#define HDSM_SHAPE_ROW(name, kernel, nv, cmax, small, threads, per_cu) {cmax, per_cu},
constexpr ShapeRow SHAPES[NUM_SHAPES] = {HDSM_SOLVER_SHAPES(HDSM_SHAPE_ROW)};
#undef HDSM_SHAPE_ROW

// What the choice depends on: the problem size and the execution knobs hdsm_create settles (thresholds 0 = never).
struct ShapeKnobs {
  int n, threads, P, RS;
  int duo_min, tri_min, quad_min;
};
enum ShapePass : int {
  PASS_ORDINARY,  // an ordinary launch, and pass 1 of a split launch
  PASS_ITEMS,     // pass 2 of a split launch: persistent workgroups, as many as fit the GPU at once
  PASS_RESCUE,    // the staging-overflow rescue: the largest staging area
};

// The shape for `blocks` workgroups: the most workgroups per CU the batch can keep busy (every shared-CU shape has a reduced
// staging area; the small LDS layout of quad holds 4 polyhedra of <= 20 rows). The shared-CU shapes need the 256-thread
// setting; each threshold applies on its own (with HDSM_DUO_MIN=0, quad and tri can still be set by hand).
inline Shape pick_shape(const ShapeKnobs& k, int blocks, ShapePass pass) {
  const bool n30 = k.n <= SPLIT_N_MAX, wide = k.threads == 256;
  const Shape one = n30 ? (k.threads == 64 ? SHAPE_replan30_64 : SHAPE_replan30) : (k.threads == 64 ? SHAPE_replan48_64 : SHAPE_replan48);
  const Shape two = n30 ? SHAPE_duo : SHAPE_duo48;
  if (pass == PASS_RESCUE || !wide) return one;
  if (pass == PASS_ITEMS) return k.duo_min > 0 ? two : one;
  if (n30 && k.quad_min > 0 && blocks >= k.quad_min && k.P <= 4 && k.RS <= 20) return SHAPE_quad;
  if (n30 && k.tri_min > 0 && blocks >= k.tri_min) return SHAPE_tri;
  if (k.duo_min > 0 && blocks >= k.duo_min) return two;
  return one;
}
}  // namespace hdsm
