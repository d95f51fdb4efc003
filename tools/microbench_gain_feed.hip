// tools/microbench_gain_feed.hip -- how a 2-KB gain table should reach the 160 workgroups of the lag-path head.
// One "evaluation" = [the host has a fresh 2-KB table] -> one launch of 160 four-wave workgroups, each of which copies the table to
// LDS and then posts the evaluation's sequence word to its slot of a pinned mailbox -> the host, spinning, has seen all 160 words.
// Three feeds, chosen by the first argument, each a process of its own so that each runs under its own time limit:
//     copy  : the table in pinned memory, hipMemcpyAsync to device memory, then the launch reads it through a pointer (the engine so far)
//     value : the table by value in the launch's argument block, read by the lanes with a lane-dependent index
//     bar   : the host stores the table itself into fine-grained device memory it can address (only where the device reports a
//             large BAR), then the launch reads it through a pointer
// Reported: call-to-last-word latency, median / min / max / interquartile range of REPS evaluations, and the host time inside the calls.
//     hipcc -O2 --offload-arch=gfx950 -o mb_gain_feed tools/microbench_gain_feed.hip && ./mb_gain_feed value
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define CK(x) do { hipError_t e__ = (x); if (e__ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e__)); exit(1); } } while (0)

constexpr int TAB = 256;             // doubles: 2 KB
constexpr int WGS = 160, THREADS = 256;
constexpr int MBX_STRIDE = 32;       // 256-byte records, as the engine's mailbox

struct ArgsPtr { const double* tab; unsigned long long* mbx; unsigned long long seq; double* sink; };
struct ArgsVal { unsigned long long* mbx; unsigned long long seq; double* sink; double tab[TAB]; };

__device__ __forceinline__ void post(const double* lds, unsigned long long* mbx, unsigned long long seq, double* sink) {
    __syncthreads();
    if (threadIdx.x == 0) {
        // (the table is used: a word of it decides a store that never happens with the values the host writes)
        if (lds[(int)(seq & (TAB - 1))] < -1.0) sink[blockIdx.x] = lds[0];
        __hip_atomic_store(mbx + (size_t)blockIdx.x * MBX_STRIDE, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

__global__ __launch_bounds__(THREADS) void feed_ptr(const ArgsPtr A) {
    __shared__ double lds[TAB];
    lds[threadIdx.x] = A.tab[threadIdx.x];                    // THREADS == TAB
    post(lds, A.mbx, A.seq, A.sink);
}

__global__ __launch_bounds__(THREADS) void feed_val(const ArgsVal A) {
    __shared__ double lds[TAB];
    lds[threadIdx.x] = A.tab[threadIdx.x];
    post(lds, A.mbx, A.seq, A.sink);
}

static double now_us() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

int main(int argc, char** argv) {
    static_assert(THREADS == TAB, "one element per thread");
    const char* mode = argc > 1 ? argv[1] : "value";
    const int REPS = 400, WARM = 40;
    const bool m_copy = !strcmp(mode, "copy"), m_val = !strcmp(mode, "value"), m_bar = !strcmp(mode, "bar");
    if (!m_copy && !m_val && !m_bar) { printf("usage: %s copy|value|bar\n", argv[0]); return 2; }
    double *tab_pinned = nullptr, *tab_dev = nullptr, *sink = nullptr;
    unsigned long long* mbx = nullptr;
    CK(hipHostMalloc(&tab_pinned, TAB * 8));
    CK(hipHostMalloc(&mbx, (size_t)WGS * MBX_STRIDE * 8));
    CK(hipMalloc(&sink, WGS * 8));
    memset(mbx, 0, (size_t)WGS * MBX_STRIDE * 8);
    if (m_bar) {
        int large_bar = 0;
        CK(hipDeviceGetAttribute(&large_bar, hipDeviceAttributeIsLargeBar, 0));
        if (!large_bar) { printf("bar  : the device reports no large BAR -- not measured\n"); return 0; }
        CK(hipExtMallocWithFlags((void**)&tab_dev, TAB * 8, hipDeviceMallocFinegrained));
    } else {
        CK(hipMalloc(&tab_dev, TAB * 8));
    }
    hipStream_t s;
    CK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    static ArgsVal av;
    std::vector<double> total(REPS), enq(REPS);
    unsigned long long seq = 0;
    for (int it = -WARM; it < REPS; it++) {
        seq++;
        double host_tab[TAB];
        for (int i = 0; i < TAB; i++) host_tab[i] = 1e-3 * i + (double)seq;      // (a fresh table: the host's recursion)
        const double t0 = now_us();
        if (m_val) {
            av.mbx = mbx; av.seq = seq; av.sink = sink;
            memcpy(av.tab, host_tab, TAB * 8);
            hipLaunchKernelGGL(feed_val, dim3(WGS), dim3(THREADS), 0, s, av);
        } else {
            ArgsPtr ap;
            ap.tab = tab_dev; ap.mbx = mbx; ap.seq = seq; ap.sink = sink;
            if (m_copy) {
                memcpy(tab_pinned, host_tab, TAB * 8);
                CK(hipMemcpyAsync(tab_dev, tab_pinned, TAB * 8, hipMemcpyHostToDevice, s));
            } else {
                memcpy(tab_dev, host_tab, TAB * 8);            // the host's own stores through the BAR
                __atomic_thread_fence(__ATOMIC_SEQ_CST);
            }
            hipLaunchKernelGGL(feed_ptr, dim3(WGS), dim3(THREADS), 0, s, ap);
        }
        const double t1 = now_us();
        for (int g = 0; g < WGS; g++) {
            const volatile unsigned long long* w = mbx + (size_t)g * MBX_STRIDE;
            while (__atomic_load_n(w, __ATOMIC_ACQUIRE) != seq) {
                if (now_us() - t1 > 2e6) { printf("%s: no word from workgroup %d after 2 s (evaluation %d)\n", mode, g, it); return 3; }
            }
        }
        const double t2 = now_us();
        CK(hipGetLastError());
        if (it >= 0) { total[it] = t2 - t0; enq[it] = t1 - t0; }
    }
    CK(hipStreamSynchronize(s));
    std::sort(total.begin(), total.end());
    std::sort(enq.begin(), enq.end());
    printf("%-5s: call -> last word  median %6.2f us  min %6.2f  max %6.2f  iqr %5.2f | host in the calls median %5.2f us  (%d evaluations, %d workgroups)\n",
           mode, total[REPS / 2], total[0], total[REPS - 1], total[3 * REPS / 4] - total[REPS / 4], enq[REPS / 2], REPS, WGS);
    return 0;
}
