// fp64_valu_probe.hip -- what the FP64 vector ALU issues back to back on this GPU: every work item runs 8 independent chains of
// v_fma_f64 for `iters` rounds; the grid fills every CU with 8 workgroups of 256.  Prints one JSON line: FMAs / s and FLOP / s (2 per
// FMA).  The yardstick for the wave-kinematics kernel (profiles/wave_kinematics_probe.py).
//   hipcc --offload-arch=gfx950 -O3 fp64_valu_probe.hip -o fp64_valu_probe && ./fp64_valu_probe
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(x)                                                                      \
    do {                                                                              \
        hipError_t e = (x);                                                           \
        if (e != hipSuccess) {                                                        \
            std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e));               \
            std::exit(1);                                                             \
        }                                                                             \
    } while (0)

constexpr int kChains = 8;

__global__ void __launch_bounds__(256) fma_chains(double* out, int iters, double a, double b) {
    double v[kChains];
#pragma unroll
    for (int c = 0; c < kChains; ++c) v[c] = threadIdx.x * 1e-3 + c;
    for (int i = 0; i < iters; ++i) {
#pragma unroll
        for (int c = 0; c < kChains; ++c) v[c] = fma(v[c], a, b);
    }
    double s = 0.0;
#pragma unroll
    for (int c = 0; c < kChains; ++c) s += v[c];
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}

int main() {
    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, 0));
    const int blocks = prop.multiProcessorCount * 8, threads = 256, iters = 1 << 14;
    double* out = nullptr;
    CHECK(hipMalloc(&out, sizeof(double) * blocks * threads));
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    hipLaunchKernelGGL(fma_chains, dim3(blocks), dim3(threads), 0, 0, out, iters, 0.999999, 1e-7);  // warm-up
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    std::vector<float> ms(7);
    for (auto& m : ms) {
        CHECK(hipEventRecord(e0, 0));
        hipLaunchKernelGGL(fma_chains, dim3(blocks), dim3(threads), 0, 0, out, iters, 0.999999, 1e-7);
        CHECK(hipEventRecord(e1, 0));
        CHECK(hipEventSynchronize(e1));
        CHECK(hipEventElapsedTime(&m, e0, e1));
    }
    std::sort(ms.begin(), ms.end());
    const double fmas = static_cast<double>(blocks) * threads * iters * kChains, sec = 1e-3 * ms[ms.size() / 2];
    std::printf("{\"cus\": %d, \"blocks\": %d, \"threads\": %d, \"iters\": %d, \"chains\": %d, \"median_ms\": %.4f, \"fma_per_s\": %.4e, "
                "\"flop_per_s\": %.4e}\n", prop.multiProcessorCount, blocks, threads, iters, kChains, 1e3 * sec, fmas / sec, 2 * fmas / sec);
    CHECK(hipFree(out));
    return 0;
}
