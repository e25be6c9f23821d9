// block_ops.hpp -- the wavefront and block primitives the kernels share (device code only; wavefronts of 64 lanes).
// Each exists once, so that where the barriers sit and in which order a sum is taken is decided in one place.
#pragma once
#include <hip/hip_runtime.h>

namespace sfm {

// A wavefront-uniform value moved into a scalar register: what every lane reads alike (a pose, K, a step) stays out of the
// vector registers.
__device__ __forceinline__ float uniform(float x) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x))); }

// A pointer read from memory (a field of a job struct, many pairs per launch) is a generic one, and the bodies would go through
// flat loads and stores; a kernel argument is known to be global.  Cast to the global address space and back -- with an empty asm
// in between that keeps the optimiser from folding the two casts away (and the value in scalar registers) -- a job's pointer is a
// global one for every access that follows.
template <typename T>
__device__ __forceinline__ T *global_ptr(T *p)
{
    auto g = (__attribute__((address_space(1))) T *)p;
    asm("" : "+s"(g));
    return (T *)g;
}

// Maximum over the wavefront, in every lane: folds packed arg-max keys (pack_key: count << 32 | ~id, so the first maximum wins).
__device__ __forceinline__ unsigned long long wave_max(unsigned long long k)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(k, off);
        k = o > k ? o : k;
    }
    return k;
}

// Sum of N doubles over a block of WAVES wavefronts in a fixed order -- wave butterflies, then the wave partials in wave
// order -- so the result is the same bit for bit on every run.  s_part: LDS [WAVES * N]; every thread returns with the
// totals in s_out (LDS [N]).  Both may be reused as soon as the totals have been read: the call ends with a barrier, and a
// later call writes s_out only behind its first one.
template <int WAVES, int N>
__device__ __forceinline__ void block_sum(double (&v)[N], double *s_part, double *s_out)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < N; ++q) {
        double x = v[q];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
        if (lane == 0) s_part[wave * N + q] = x;
    }
    __syncthreads();
    if ((int)threadIdx.x < N) {
        double s = s_part[threadIdx.x];
        for (int w = 1; w < WAVES; ++w) s += s_part[w * N + threadIdx.x];
        s_out[threadIdx.x] = s;
    }
    __syncthreads();
}

// Sums of COUNT (<= 64) values over the wavefront, one per lane and value, in fp64, transposed: lane L returns the sum over all 64
// lanes of v[L & (W - 1)] where W = 64 for COUNT > 32 and 32 otherwise (values past COUNT count as 0).  Log-step halving: at the
// step with lane distance d a lane keeps the half of its partial sums that its bit d selects and receives the other lane's
// partials for that half, so the steps exchange W / 2, W / 4, ..., 1 values (W - 1 shuffles) instead of six per value, and the
// shuffles of one step are independent of each other.  The first step moves the fp32 terms and adds them as doubles.  The order
// of every sum is fixed by the lane numbers alone.  (adjust.hip's system pass, chain_adjust.hip's.)
template <int D>
__device__ __forceinline__ void wave_halve(double (&a)[32], const int lane)
{
    const bool hi = (lane & D) != 0;
#pragma unroll
    for (int i = 0; i < D; ++i) {
        const double keep = hi ? a[D + i] : a[i], send = hi ? a[i] : a[D + i];
        a[i] = keep + __shfl_xor(send, D);
    }
}

template <int COUNT>
__device__ __forceinline__ double wave_transpose_sum(const float *v, const int lane)
{
    static_assert(COUNT >= 1 && COUNT <= 64, "one value per lane at the most");
    double a[32];
    if (COUNT > 32) {
        const bool hi = (lane & 32) != 0;
#pragma unroll
        for (int i = 0; i < 32; ++i) {
            const float up = 32 + i < COUNT ? v[32 + i < COUNT ? 32 + i : 0] : 0.0f;
            const float keep = hi ? up : v[i], send = hi ? v[i] : up;
            a[i] = (double)keep + (double)__shfl_xor(send, 32);
        }
    } else {
#pragma unroll
        for (int i = 0; i < 32; ++i) a[i] = i < COUNT ? (double)v[i < COUNT ? i : 0] + (double)__shfl_xor(v[i < COUNT ? i : 0], 32) : 0.0;
    }
    wave_halve<16>(a, lane);
    wave_halve<8>(a, lane);
    wave_halve<4>(a, lane);
    wave_halve<2>(a, lane);
    wave_halve<1>(a, lane);
    return a[0];
}

// Exclusive scan of one value per thread over a block of WAVES wavefronts: returns the sum of the lower threads' values and
// leaves the total in wsum[WAVES] (wsum: LDS [WAVES + 1]).  Two barriers, none in front: a caller that scans again with the
// same wsum puts a __syncthreads() between its last read of wsum and the next call.
template <int WAVES, class T>
__device__ __forceinline__ T block_scan(T v, T *wsum)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T u = __shfl_up(inc, d);
        if (lane >= d) inc += u;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    if (threadIdx.x == 0) {
        T acc = 0;
        for (int i = 0; i < WAVES; ++i) { const T t = wsum[i]; wsum[i] = acc; acc += t; }
        wsum[WAVES] = acc;
    }
    __syncthreads();
    return wsum[wave] + inc - v;
}

} // namespace sfm
