// stream_ceiling.hip -- how fast can h2o Q1's row pass stream its two 4-byte columns on this part?
// Standalone: hipcc -O3 --offload-arch=gfx950 -std=c++20 tools/stream_ceiling.hip -o tools/bin/stream_ceiling
// Two int32 columns of n rows (default 1e9: 8 GB) on the device; every variant reads all of both, best of 5 by HIP events.
//   plain : 16-byte loads in agg32_kernel's geometry (256-thread workgroups, 8 per CU, one contiguous span per workgroup,
//           8 rows per lane per step)
//   glds  : each wave streams its share of the workgroup's span through its own LDS ring of S stages by
//           global_load_lds_dwordx4 (R instructions of 1 KB per column per stage), S-1 stages ahead, retired by a counted
//           s_waitcnt vmcnt, read back with ds_read_b128 by the lanes that loaded them; "nt" sets aux = 2
//   +q1   : the same, each row also doing Q1's LDS work: a Fibonacci-hashed probe of a 256-slot key table and one ds_add_u64
// Prints one line per variant: name, waves per CU, S, ms, TB/s, and a checksum (equal across variants of one kind).
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); exit(1); } } while (0)

constexpr uint32_t EMPTY = 0x80000000u, LCAP = 256, LBITS = 8;

__global__ void fill(uint32_t* k, uint32_t* v, uint64_t n) {
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t h = (i + 1) * 0x9E3779B97F4A7C15ull;
        h ^= h >> 29; h *= 0xBF58476D1CE4E5B9ull; h ^= h >> 32;
        k[i] = 1 + (uint32_t)(h % 100);           // id1-like: 100 groups
        v[i] = 1 + (uint32_t)((h >> 40) % 5);     // v1-like
    }
}

__device__ inline void span(uint32_t total, uint32_t& lo, uint32_t& hi) {
    uint32_t per = (total + gridDim.x - 1) / gridDim.x;
    uint64_t b = (uint64_t)blockIdx.x * per, e = b + per;
    lo = b < total ? (uint32_t)b : total; hi = e < total ? (uint32_t)e : total;
}

// Q1's per-workgroup table: keys + 64-bit sums, insert on first sight
struct Tab {
    uint32_t* key; unsigned long long* acc; uint32_t* used;
    __device__ uint32_t slow(uint32_t k) const {
        uint32_t s = (k * 0x9E3779B1u) >> (32 - LBITS);
        for (uint32_t p = 0; p < LCAP; ++p) {
            uint32_t cur = key[s];
            if (cur == k) return s;
            if (cur == EMPTY) { uint32_t old = atomicCAS(&key[s], EMPTY, k); if (old == EMPTY) { atomicAdd(used, 1u); return s; } if (old == k) return s; }
            s = (s + 1) & (LCAP - 1);
        }
        return 0;
    }
    template <int M> __device__ void rows(const uint32_t (&k)[M], const uint32_t (&v)[M]) const {
        uint32_t slot[M], cur[M];
#pragma unroll
        for (int j = 0; j < M; ++j) { slot[j] = (k[j] * 0x9E3779B1u) >> (32 - LBITS); cur[j] = key[slot[j]]; }
#pragma unroll
        for (int j = 0; j < M; ++j) if (cur[j] != k[j]) slot[j] = slow(k[j]);
#pragma unroll
        for (int j = 0; j < M; ++j) atomicAdd(&acc[slot[j]], (unsigned long long)(int64_t)(int32_t)v[j]);
    }
};

template <bool WORK> __device__ Tab tab_init(unsigned char* base) {
    Tab t{reinterpret_cast<uint32_t*>(base + LCAP * 8), reinterpret_cast<unsigned long long*>(base), reinterpret_cast<uint32_t*>(base + LCAP * 12)};
    if constexpr (WORK) {
        for (uint32_t s = threadIdx.x; s < LCAP; s += blockDim.x) { t.key[s] = EMPTY; t.acc[s] = 0; }
        if (threadIdx.x == 0) *t.used = 0;
        __syncthreads();
    }
    return t;
}
template <bool WORK> __device__ void tab_flush(const Tab& t, unsigned long long local, unsigned long long* out) {
    if constexpr (WORK) {
        __syncthreads();
        for (uint32_t s = threadIdx.x; s < LCAP; s += blockDim.x) if (t.key[s] != EMPTY) local += t.acc[s] * t.key[s];
    }
    atomicAdd(out, local);
}
constexpr size_t TAB_BYTES = LCAP * 12 + 16;

// (a) plain 16-byte loads, agg32's geometry
template <bool WORK> __global__ void __launch_bounds__(256) plain_kernel(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals, uint32_t n, unsigned long long* out) {
    extern __shared__ __align__(16) unsigned char smem[];
    const Tab t = tab_init<WORK>(smem);
    unsigned long long local = 0;
    uint32_t lo, hi;
    span(n >> 3, lo, hi);
    for (uint32_t c = lo + threadIdx.x; c < hi; c += blockDim.x) {
        const size_t base = (size_t)c * 8;
        uint4 k0 = *reinterpret_cast<const uint4*>(keys + base), k1 = *reinterpret_cast<const uint4*>(keys + base + 4);
        uint4 v0 = *reinterpret_cast<const uint4*>(vals + base), v1 = *reinterpret_cast<const uint4*>(vals + base + 4);
        if constexpr (WORK) {
            const uint32_t k[8] = {k0.x, k0.y, k0.z, k0.w, k1.x, k1.y, k1.z, k1.w}, v[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
            t.rows(k, v);
        } else {
            local += (k0.x ^ v0.x) + (k0.y ^ v0.y) + (k0.z ^ v0.z) + (k0.w ^ v0.w) + (k1.x ^ v1.x) + (k1.y ^ v1.y) + (k1.z ^ v1.z) + (k1.w ^ v1.w);
        }
    }
    tab_flush<WORK>(t, local, out);
}

// (b)/(c) LDS-DMA ring per wave.  A stage = R KB of keys then R KB of values; lane l's rows of sub-block r sit at r*1024 + l*16.
// The DMA is issued by inline asm: hipcc counts a __builtin_amdgcn_global_load_lds as a pending LDS write of unknown address
// and waits vmcnt(0) before every ds_read, which drains the ring.  Hidden from it, the loads are retired by our own counted
// s_waitcnt vmcnt.  M0 (the LDS destination) is written and restored inside the statement.
template <int AUX> __device__ inline void glds16(const void* src, uint32_t lds) {
    unsigned keep;
    if constexpr (AUX == 2) asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off nt\n\ts_mov_b32 m0, %0" : "=&s"(keep) : "v"(src), "s"(lds) : "memory");
    else asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0" : "=&s"(keep) : "v"(src), "s"(lds) : "memory");
}
template <int S, int R, int AUX, bool WORK> __device__ inline void issue(const uint32_t* keys, const uint32_t* vals, uint32_t ring, uint32_t chunk, int stage) {
    const int lane = threadIdx.x & 63;
    const uint32_t st = ring + (uint32_t)stage * (2 * R * 1024);
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const size_t row = (size_t)chunk * (256 * R) + r * 256 + lane * 4;
        glds16<AUX>(keys + row, __builtin_amdgcn_readfirstlane(st + r * 1024));
        glds16<AUX>(vals + row, __builtin_amdgcn_readfirstlane(st + (R + r) * 1024));
    }
}

template <int S, int R, int AUX, bool WORK> __global__ void __launch_bounds__(1024) glds_kernel(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals, uint32_t n, unsigned long long* out) {
    extern __shared__ __align__(16) unsigned char smem[];
    const Tab t = tab_init<WORK>(smem);
    const int W = blockDim.x >> 6, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    unsigned char* ring = smem + TAB_BYTES + (size_t)w * S * 2 * R * 1024;
    const uint32_t ring_lds = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)ring);
    unsigned long long local = 0;
    uint32_t lo, hi;
    span(n / (256 * R), lo, hi);
    const uint32_t first = lo + w;
    const uint32_t m = first < hi ? (hi - first + W - 1) / W : 0;      // this wave's chunks: first, first + W, ...
#pragma unroll
    for (int s = 0; s < S - 1; ++s) if ((uint32_t)s < m) issue<S, R, AUX, WORK>(keys, vals, ring_lds, first + s * W, s);
    for (uint32_t i = 0; i < m; ++i) {
        const uint32_t ahead = i + S - 1;
        if (ahead < m) {
            issue<S, R, AUX, WORK>(keys, vals, ring_lds, first + ahead * W, ahead % S);
        }
        if (ahead < m) asm volatile("s_waitcnt vmcnt(%0)" :: "i"((S - 1) * 2 * R) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned char* st = ring + (size_t)(i % S) * (2 * R * 1024);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const uint4 kk = *reinterpret_cast<const uint4*>(st + r * 1024 + lane * 16);
            const uint4 vv = *reinterpret_cast<const uint4*>(st + (R + r) * 1024 + lane * 16);
            if constexpr (WORK) {
                const uint32_t k[4] = {kk.x, kk.y, kk.z, kk.w}, v[4] = {vv.x, vv.y, vv.z, vv.w};
                t.rows(k, v);
            } else {
                local += (kk.x ^ vv.x) + (kk.y ^ vv.y) + (kk.z ^ vv.z) + (kk.w ^ vv.w);
            }
        }
    }
    tab_flush<WORK>(t, local, out);
}

struct Run { const char* name; int wpc; int S; float ms; unsigned long long sum; };

template <class K> static Run timeit(const char* name, K kern, int grid, int block, size_t lds, int wpc, int S, const uint32_t* k, const uint32_t* v, uint32_t n, unsigned long long* out) {
    CK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipEvent_t a, b;
    CK(hipEventCreate(&a)); CK(hipEventCreate(&b));
    float best = 1e30f;
    unsigned long long sum = 0;
    for (int rep = 0; rep < 6; ++rep) {               // the first run warms up
        CK(hipMemsetAsync(out, 0, 8));
        CK(hipEventRecord(a));
        hipLaunchKernelGGL(kern, dim3(grid), dim3(block), lds, 0, k, v, n, out);
        CK(hipGetLastError());
        CK(hipEventRecord(b));
        CK(hipEventSynchronize(b));
        float ms; CK(hipEventElapsedTime(&ms, a, b));
        if (rep) best = ms < best ? ms : best;
        CK(hipMemcpy(&sum, out, 8, hipMemcpyDeviceToHost));
    }
    CK(hipEventDestroy(a)); CK(hipEventDestroy(b));
    const double tbs = 8.0 * n / (best * 1e-3) / 1e12;
    printf("%-14s waves/CU %2d  S %d   %.4f ms  %.3f TB/s  sum %llu\n", name, wpc, S, best, tbs, sum);
    fflush(stdout);
    return {name, wpc, S, best, sum};
}

int main(int argc, char** argv) {
    const uint32_t n = argc > 1 ? (uint32_t)strtoul(argv[1], nullptr, 10) : 1000000000u;
    int dev = 0, ncu = 0;
    CK(hipGetDevice(&dev));
    CK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
    uint32_t *k, *v; unsigned long long* out;
    CK(hipMalloc(&k, (size_t)n * 4)); CK(hipMalloc(&v, (size_t)n * 4)); CK(hipMalloc(&out, 8));
    hipLaunchKernelGGL(fill, dim3(4096), dim3(256), 0, 0, k, v, (uint64_t)n);
    CK(hipDeviceSynchronize());
    printf("n %u rows, %d CUs; bytes %.3f GB\n", n, ncu, 8.0 * n / 1e9);
    const int pgrid = ncu * 8;
    timeit("plain", plain_kernel<false>, pgrid, 256, TAB_BYTES, 32, 0, k, v, n, out);
    timeit("plain+q1", plain_kernel<true>, pgrid, 256, TAB_BYTES, 32, 0, k, v, n, out);
    // LDS-DMA: workgroups of W waves, B workgroups per CU, R KB per column per stage (R = 2: 8 rows per lane per stage, as agg32);
    // every shape keeps B * (W * S * 2R KB + the table) within the 160 KB of LDS per CU
#define GL(S, W, B, R, AUX, WORK, NAME) timeit(NAME, glds_kernel<S, R, AUX, WORK>, ncu * (B), 64 * (W), TAB_BYTES + (size_t)(W) * (S) * 2048 * (R), (W) * (B), S, k, v, n, out)
#define SWEEP(AUX, WORK, NAME)                                                                                     \
    GL(2, 4, 2, 2, AUX, WORK, NAME); GL(3, 4, 2, 2, AUX, WORK, NAME); GL(4, 4, 2, 2, AUX, WORK, NAME);             \
    GL(3, 8, 1, 2, AUX, WORK, NAME); GL(4, 8, 1, 2, AUX, WORK, NAME); GL(3, 4, 3, 2, AUX, WORK, NAME);             \
    GL(3, 6, 2, 2, AUX, WORK, NAME); GL(2, 4, 4, 2, AUX, WORK, NAME);                                              \
    GL(3, 4, 4, 1, AUX, WORK, NAME); GL(4, 4, 4, 1, AUX, WORK, NAME); GL(2, 8, 4, 1, AUX, WORK, NAME);             \
    GL(6, 4, 2, 1, AUX, WORK, NAME);
    SWEEP(0, false, "glds");
    SWEEP(2, false, "glds-nt");
    SWEEP(0, true, "glds+q1");
    SWEEP(2, true, "glds-nt+q1");
    timeit("plain", plain_kernel<false>, pgrid, 256, TAB_BYTES, 32, 0, k, v, n, out);
    timeit("plain+q1", plain_kernel<true>, pgrid, 256, TAB_BYTES, 32, 0, k, v, n, out);
    CK(hipFree(k)); CK(hipFree(v)); CK(hipFree(out));
    return 0;
}
