// Staging-area capacities (staged neighbour rows, Shm::cand) of the launch shapes of the solver kernel. hdsm_api.hip instantiates
// hdsm::Solver<NV, CMAX, SMALL> with these, and the CPU execution of the device source (tests/wave_emu/wave_emu.cpp) runs the same
// tuples, so the two cannot drift apart. Why each value is what it is: the comments at the kernels in hdsm_api.hip.
#pragma once

namespace hdsm {
constexpr int CMAX30 = 1536;     // k_replan<32, ..>: n <= 30, one workgroup per CU
constexpr int CMAX48 = 1024;     // k_replan<48, ..>: n <= 48, one workgroup per CU
constexpr int CMAX_DUO = 768;    // k_replan_duo: n <= 30, two 256-thread workgroups per CU
constexpr int CMAX_TRI = 384;    // k_replan_tri: n <= 30, three 128-thread workgroups per CU
constexpr int CMAX_QUAD = 256;   // k_replan_quad: n <= 30, four 128-thread workgroups per CU, small LDS layout
constexpr int CMAX_DUO48 = 720;  // k_replan_duo48: n > 30, two 128-thread workgroups per CU
}  // namespace hdsm
