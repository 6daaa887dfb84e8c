// The floor of the plan pre-pass: an EMPTY kernel with the pre-pass's launch shape on the bench line (177 workgroups of 256 threads,
// the same count of kernel arguments by size), launched back to back on one stream, each followed by a second empty kernel standing for
// the solver — so the trace shows what a launch of that shape lasts when it does nothing, and the idle queue between two launches.
// usage: rocprofv3 --kernel-trace --output-format csv -d DIR -o empty -- ./empty_launch [launches]; scripts/round_overhead.py floor DIR
// build: hipcc --offload-arch=gfx950 -O3 -o empty_launch empty_launch.hip
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
struct Pad {
  const void* p[4];
  int v[5];
};
__global__ __launch_bounds__(256) void k_empty(int, int, const double*, const unsigned char*, double*, double*, int, const int*, const int*, int*, Pad) {}
__global__ __launch_bounds__(128) void k_follow(const void*, Pad) {}
int main(int argc, char** argv) {
  const int n = argc > 1 ? std::atoi(argv[1]) : 400;
  hipStream_t st;
  if (hipStreamCreate(&st) != hipSuccess) return std::fprintf(stderr, "no device\n"), 1;
  for (int i = 0; i < n; ++i) {
    hipLaunchKernelGGL(k_empty, dim3(177), dim3(256), 0, st, 0, 0, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, Pad{});
    hipLaunchKernelGGL(k_follow, dim3(1024), dim3(128), 0, st, nullptr, Pad{});
  }
  if (hipStreamSynchronize(st) != hipSuccess) return std::fprintf(stderr, "launch failed: %s\n", hipGetErrorString(hipGetLastError())), 1;
  std::printf("%d empty launches\n", n);
  return 0;
}
