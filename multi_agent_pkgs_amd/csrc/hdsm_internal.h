// hdsm_internal.h — the entry points that cross translation units of csrc/ without being in include/, each declared ONCE. The file
// that defines one and every file that calls one include this header, so a signature that drifts does not compile (they are
// extern "C" — two are called from the tests through ctypes — and a mismatch would still link).
#pragma once
#include "../../include/hdsm_swarm.h"

extern "C" {

// (hdsm_api.hip) every device entry point of the solver handle records its "done" event; the device-resident loop defers the
// records (on = 1) and leaves one at the end of its round
int hdsm_internal_defer_done(void* handle, int on);
int hdsm_internal_record_done(void* handle, void* hip_stream);

// (exchange_kernels.hip) local ranks, for hdsm_dswarm_round_ranks. They report through hdsm_last_error.
// what hdsm_exchange_device and hdsm_dswarm_round answer to a local communicator
#define HDSM_LOCAL_COMM_REFUSED "a local communicator gathers all its ranks in one call: use hdsm_dswarm_round_ranks"
// -1 null, 0 RCCL, 1 local; device (may be NULL): the communicator's
int hdsm_internal_comm_kind(void* comm, int32_t* device);
// comms[world] are the ranks 0 .. world - 1, in that order, of ONE local group of exactly `world` ranks whose records hold rec doubles
int hdsm_internal_local_check(int32_t world, void* const* comms, int32_t rec);
// the send buffers [per][rec] of the ranks; the device tables are written (synchronously) only when one of them changed
int hdsm_internal_local_bind(int32_t world, void* const* comms, const double* const* send, int32_t per);
// before the rank's k_commit: its stream waits for every rank's "gathered" of the round before; after it: "published" is recorded
int hdsm_internal_local_commit_gate(void* comm, void* hip_stream);
int hdsm_internal_local_published(void* comm, void* hip_stream);
// the rank's stream waits for every "published", `mark` (a hipEvent_t, may be NULL) is recorded, k_gather_local, "gathered" is recorded
int hdsm_internal_local_gather(void* comm, double* plans_all, uint8_t* has_plan_all, void* hip_stream, void* mark);
// k_gather_local alone (also called from the tests): d_send [world] device pointers to shards of per * rec doubles, 8-byte aligned
int hdsm_internal_gather_local_launch(int32_t world, int32_t per, int32_t rec, const double* const* d_send, double* plans_all,
                                      uint8_t* has_plan_all, void* hip_stream);

// (swarm_flight.cpp) the hooks of the host mirror that stay C (the rest of the flight in and out of the device-resident loop is typed:
// swarm_host.h). The plain agent states (hdsm_sw::AgentS [n_local]) and the configuration of a shard; every out argument may be NULL
int hdsm_swarm_export_state(void* swarm, void* agents_out, int32_t* n_local, int32_t* n_rob, int32_t* first_id, hdsm_params* prm,
                            hdsm_swarm_config* cfg, const int8_t** world, int32_t wdim[3], double worigin[3]);
int hdsm_swarm_import_state(void* swarm, const void* agents_in, int32_t n_local);
// rounds flown on the device into the planner records: rows [n_rounds][n_local][9]
int hdsm_swarm_append_history(void* swarm, int32_t n_rounds, const double* rows);

// (audit_host.cpp) the argument checks shared by hdsm_flight_audit_host / _batch
int hdsm_internal_audit_args(int32_t n_rob, const double* plans_all, const uint8_t* has_plan, int32_t n_hor, int32_t step_plan, int32_t first,
                             int32_t n_local, double drone_radius, double drone_z_offset, const int8_t* world, const int32_t wdim[3],
                             const double worigin[3], double voxel_size, const hdsm_audit_round* out);
// hdsm_flight_audit_host with neighbour groups: range [n_rob][2] = the id range (lo, hi) a subject takes its partners from
// (NULL: everybody, which is hdsm_flight_audit_host itself)
int hdsm_internal_audit_host_grouped(int32_t n_rob, const double* plans_all, const uint8_t* has_plan, int32_t n_hor, int32_t step_plan, int32_t first,
                                     int32_t n_local, double drone_radius, double drone_z_offset, const int8_t* world, const int32_t wdim[3],
                                     const double worigin[3], double voxel_size, const int32_t* range, hdsm_audit_round* out);
// (script_host.cpp) the argument checks shared by hdsm_script_records_host / _batch
int hdsm_internal_script_args(int32_t n_script, int32_t n_knots, const double* knots, int32_t n_hor, int32_t step_plan, double dt, int32_t predict,
                              int64_t round, const double* records);
// (track_host.cpp) the argument checks shared by hdsm_track_states_host / _batch
int hdsm_internal_track_args(const hdsm_tracking* m, int32_t n, const int32_t* agent_id, const double* planned, double T, int64_t round,
                             const double* flown);
// (command_host.cpp) the argument checks shared by hdsm_command_host / _batch
int hdsm_internal_command_args(int32_t n, int32_t n_hor, int32_t step_plan, double dt, int32_t yaw_idx, double k_p_yaw, const int32_t* n_ref,
                               const double* ref_point, const double* state_before, const double* records, const int32_t* valid_in,
                               const double* state_after, const double* yaw);
// (vehicle_host.cpp) the argument checks shared by hdsm_vehicle_fly_host / _batch
int hdsm_internal_vehicle_args(const hdsm_vehicle* m, int32_t n, const int32_t* agent_id, int32_t step_plan, double dt, int64_t round,
                               const double* start, const hdsm_command* setpoint, const double* planned_end, const hdsm_vehicle_state* vstate,
                               const double* flown);
// (mission_host.cpp) the argument checks shared by hdsm_mission_step_host / _batch
int hdsm_internal_mission_args(const hdsm_mission* m, int32_t n, int64_t round, const double* states, const double* waypoints, const int32_t* count,
                               const hdsm_mission_record* records, const double* goals, const uint8_t* due);
// (assign_kernels.hip) hdsm_assign_batch with the launch of k_assign repeated reps (>= 1) times on the same inputs, each between two HIP
// events: ms [reps]. For scripts/gpu_assign_timing.py; the results are the last launch's, which are every launch's.
int hdsm_internal_assign_batch_timed(int32_t device, const hdsm_assign_setting* setting, int32_t n, int32_t n_groups, const int32_t* group_start,
                                     const double* pos, const uint8_t* active, const double* slots, int32_t* slot_of, int64_t* price,
                                     hdsm_assign_stats* stats, int32_t reps, float* ms);
// (path_host.cpp) the per-case problem (a hdsm_path::PathIn*) of hdsm_local_path_host / _dmp_host
int hdsm_internal_path_case(int32_t t, const int8_t* world, const int32_t wdim[3], const int32_t ldim[3], const int32_t* off,
                            const int32_t* ground_k, const double* origin, const double* start, const double* goal, double res, void* problem);

}  // extern "C"
