// atomic_merge.hip -- which lanes of one no-return global_atomic_add_f32 does gfx950 merge into one
// 64-byte request at the memory side?  The two 32-byte halves of every line are carried
//   ROW:   by the two 8-lane halves of one 16-lane row           (4 whole lines per instruction)
//   HALF:  by lanes l and l + 32 of one instruction              (4 whole lines per instruction)
//   SPLIT: by two consecutive instructions                       (8 half lines per instruction)
// Every instruction adds 64 floats; lines are drawn from a 32 MiB buffer (the size of the
// record of 32 poses) by a hash of (wave, iteration), so that they miss L2 lines of other waves
// like the record's do.  The tool prints the time per atomic instruction; the request count is
// TCC_ATOMIC_sum of a counter pass of its own (kernel names: merge_kernel<0 / 1 / 2>):
//   hipcc --offload-arch=gfx950 -O3 -munsafe-fp-atomics atomic_merge.hip -o atomic_merge
//   ./atomic_merge
//   rocprofv3 --pmc TCC_ATOMIC_sum -d out --output-format csv -- ./atomic_merge
// If HALF counts 4 requests per instruction like ROW, merging is per instruction; if it counts 8
// like SPLIT, merging is per 16-lane row.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>

#define CHECK(x)                                                                      \
    do {                                                                              \
        hipError_t e_ = (x);                                                          \
        if (e_ != hipSuccess) {                                                       \
            fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); \
            exit(1);                                                                  \
        }                                                                             \
    } while (0)

constexpr int kIters = 512;           // iterations per wave
constexpr int kPerIter = 4;           // atomic instructions per iteration
constexpr unsigned kLines = 1u << 19; // 64-byte lines of the buffer (32 MiB)
enum { ROW, HALF, SPLIT, N_CASES };
const char *kNames[N_CASES] = {"halves of a line in the two half rows of a row",
                               "halves of a line in lanes l and l + 32",
                               "halves of a line in two instructions"};

__device__ __forceinline__ unsigned mix(unsigned x) {
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

template <int C>
__global__ __launch_bounds__(256) void merge_kernel(float *buf, float val) {
    const unsigned lane = threadIdx.x & 63u;
    const unsigned wave = blockIdx.x * 4u + (threadIdx.x >> 6);
    // (line, float) of this lane relative to the instruction's first line
    unsigned line, fl;
    if (C == ROW) {
        line = lane >> 4;
        fl = lane & 15u;
    } else if (C == HALF) {
        line = (lane & 31u) >> 3;
        fl = (lane >> 5) * 8u + (lane & 7u);
    } else {
        line = lane >> 3;
        fl = lane & 7u;
    }
    const unsigned rel = line * 16u + fl;
    for (int it = 0; it < kIters; ++it) {
#pragma unroll
        for (int k = 0; k < kPerIter; ++k) {
            // SPLIT: instructions 2 j and 2 j + 1 share their eight lines
            const unsigned key = C == SPLIT ? (unsigned)(it * kPerIter + (k & ~1)) : (unsigned)(it * kPerIter + k);
            // (wave-uniform; the instruction's lines [base, base + 8) lie inside the buffer)
            const unsigned base = mix(wave * 0x9e3779b9u + key) % (kLines - 8u);
            const unsigned at = base * 16u + rel + (C == SPLIT && (k & 1) ? 8u : 0u);
            unsafeAtomicAdd(buf + at, val);
        }
    }
}

template <int C>
void run(int n_cu, float *buf) {
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    const int blocks = n_cu * 8;
    hipLaunchKernelGGL(merge_kernel<C>, dim3(blocks), dim3(256), 0, 0, buf, 1.0f);
    CHECK(hipDeviceSynchronize());
    CHECK(hipEventRecord(e0));
    hipLaunchKernelGGL(merge_kernel<C>, dim3(blocks), dim3(256), 0, 0, buf, 1.0f);
    CHECK(hipEventRecord(e1));
    CHECK(hipDeviceSynchronize());
    float ms = 0;
    CHECK(hipEventElapsedTime(&ms, e0, e1));
    const double instr = (double)blocks * 4 * kIters * kPerIter;
    printf("%-52s %.3f ms, %.3e atomic instructions per launch, %.3f ns each (whole GPU), %.1f GB/s of lines\n",
           kNames[C], ms, instr, ms * 1e6 / instr, instr * 256.0 / (ms * 1e6));
}

int main() {
    int dev = 0, n_cu = 0;
    CHECK(hipGetDevice(&dev));
    CHECK(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev));
    float *buf;
    CHECK(hipMalloc(&buf, (size_t)kLines * 64));
    CHECK(hipMemset(buf, 0, (size_t)kLines * 64));
    run<ROW>(n_cu, buf);
    run<HALF>(n_cu, buf);
    run<SPLIT>(n_cu, buf);
    // every launch adds 1.0f 64 times per instruction: the buffer's sum says that nothing was lost
    float *h = (float *)malloc((size_t)kLines * 64);
    CHECK(hipMemcpy(h, buf, (size_t)kLines * 64, hipMemcpyDeviceToHost));
    double sum = 0;
    for (size_t i = 0; i < (size_t)kLines * 16; ++i) sum += h[i];
    const double want = (double)n_cu * 8 * 4 * kIters * kPerIter * 64 * 2 * N_CASES;
    printf("sum of the buffer %.6e, expected %.6e\n", sum, want);
    free(h);
    CHECK(hipFree(buf));
    return sum == want ? 0 : 2;
}
