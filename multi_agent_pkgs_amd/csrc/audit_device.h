// audit_device.h — the launch interface of the flight audit's kernels (audit_kernels.hip), used by hdsm_flight_audit_batch and
// by the device-resident loop (the launch: swarm_kernels.hip; the scratch: dswarm_audit.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "audit_core.h"
#include "device_mem.h"

namespace hdsm_audit {

struct Partial {  // the minimum of one subject over one chunk of partners
  double q;
  int32_t partner, substep;
};

// The sweep's shape: a workgroup is ONE wavefront of 64 subjects against a tile of at most 64 partners. A lane's pair evaluations
// are a serial chain (a few dozen fp64 operations and one division each, the running minimum carried along), so the time of the
// launch is the length of that chain unless there are enough wavefronts to fill the SIMDs: small tiles keep the chain short (64
// pairs per sub-step) and the grid large (4096 x 4096: 64 x 64 workgroups, 16 per CU, all resident at 6 KB of LDS each).
constexpr int SWEEP_THREADS = 64;    // subjects of a workgroup of k_audit, one per lane
constexpr int TILE_DOUBLES = 768;    // positions of a partner tile in LDS (6 KB)
constexpr int TILE_PARTNERS = 64;    // at most; fewer when step_plan + 1 points of that many partners do not fit (step_plan > 3)

// partners of a tile for step_plan = S
inline int tile_partners(int S) {
  const int fit = TILE_DOUBLES / (3 * (S + 1));
  return fit < TILE_PARTNERS ? fit : TILE_PARTNERS;
}

struct __attribute__((visibility("hidden"))) DeviceBufs {  // scratch of the audit of G records and n_local subjects with step_plan S
  int G = 0, n_local = 0, S = 0, tile = 0, chunks = 0;
  hdsm_mem::DevBuf<double> d_pos;              // [G][S + 1][3]
  hdsm_mem::DevBuf<Partial> d_part;            // [chunks][n_local]
  hdsm_mem::DevBuf<hdsm_audit_round> d_round;  // [n_local]
};
hipError_t device_alloc(DeviceBufs* b, int G, int n_local, int S);  // (on an error *b is empty again)

// One round on `st`. audit: k_audit_pack, k_audit, then k_audit_track (merge, own track, d_round, and the flight record when d_report
// is given). hist_row (may be NULL): [n_local][9] receives the 9 doubles at state0 + k * state_stride bytes of every subject.
// With audit == false only the history is written. d_range (neighbour groups; may be NULL = everybody): [G][2] = the id range (lo, hi)
// a subject takes its partners from.
hipError_t launch(const DeviceBufs& b, bool audit, const double* d_plans, const uint8_t* d_has, const int32_t* d_range, int n_hor, int first, const Weights& w,
                  const World& wd, hdsm_flight_report* d_report, double warn2, const double* state0, size_t state_stride, double* hist_row,
                  hipStream_t st);

}  // namespace hdsm_audit
