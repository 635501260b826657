// CPU stand-in for the HIP runtime: enough to run skg_roialign.hip's kernels with 256 host threads per block.
#pragma once
#include <stdint.h>
#include <cmath>
#include <cstring>
#include <thread>
#include <vector>
#include <barrier>
#include <atomic>
#include <functional>
#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __shared__ static
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
struct float4 { float x, y, z, w; };
struct uint4 { uint32_t x, y, z, w; };
struct uint2 { uint32_t x, y; };
static inline uint2 make_uint2(uint32_t a, uint32_t b) { return uint2{a, b}; }
extern thread_local dim3 threadIdx, blockIdx, gridDim;
extern std::barrier<>* g_barrier;
static inline void __syncthreads() { g_barrier->arrive_and_wait(); }
static inline float __uint_as_float(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static inline uint32_t __float_as_uint(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static inline float __shfl_xor(float v, int, int) { return v; }
static inline float atomicAdd(float* p, float v) {
    std::atomic_ref<float> r(*p); float o = r.load();
    while (!r.compare_exchange_weak(o, o + v)) {}
    return o;
}
template <class T> static inline T min(T a, T b) { return a < b ? a : b; }
typedef int hipError_t; static const int hipSuccess = 0; static inline hipError_t hipGetLastError() { return 0; }
typedef void* hipStream_t; typedef void* hipEvent_t;
extern std::atomic<long long> g_oob;
template <class K, class... A>
static void emu_launch(K kernel, dim3 grid, dim3 block, A... args) {
    for (unsigned b = 0; b < grid.x; ++b) {
        std::barrier<> bar(block.x); g_barrier = &bar;
        std::vector<std::thread> th;
        for (unsigned t = 0; t < block.x; ++t)
            th.emplace_back([=, &bar]() {
                threadIdx = dim3(t); blockIdx = dim3(b); gridDim = grid;
                kernel(args...);
                bar.arrive_and_drop();
            });
        for (auto& x : th) x.join();
    }
}
#define hipLaunchKernelGGL(kernel, grid, block, shmem, stream, ...) emu_launch(kernel, grid, block, __VA_ARGS__)
