// Wave-per-row helpers shared by the loss and feature translation units
// (ngnn_loss, ngnn_consist, ngnn_contrast, ngnn_metrics, ngnn_noise): the
// cross-lane sums, the fixed-order workgroup sum, the "one wave per row, four
// rows per 256-thread workgroup" shape on both sides of the launch, and the
// cross-entropy row terms.  Moving code here must not change its arithmetic
// order: forms whose rounding differs stay apart (see the notes below).
#pragma once

#include "ngnn_internal.h"

namespace ngnn {

// ---- cross-lane reductions: every lane of the group ends with the result ----

// sum over a group of LANES consecutive lanes (a power of two, at most a wave)
template <int LANES, typename T>
__device__ __forceinline__ T group_sum(T v) {
#pragma unroll
    for (int o = LANES / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
    return group_sum<kWave>(v);
}
__device__ __forceinline__ float wave_maxf(float v) {
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

// ---- the fixed-order sum of one T-thread workgroup ----
//
// out[k] = sum over i in [0, n) of what term(i, acc) adds to acc[k], in ONE
// order whatever the hardware does: thread t adds its terms i = t, t + T, ...
// in ascending i, then a halving tree over the threads (t += t + h for h =
// T / 2 .. 1).  The N sums share the tree's barriers.  Every thread must call
// it (barriers) and every thread gets out[]; `tree` is the kernel's LDS, and
// a kernel that uses it again needs a barrier between reading out[] and the
// next call.
template <int T, int N, typename V, typename Term>
__device__ __forceinline__ void block_sum(V (&tree)[N][T], V (&out)[N], int n, Term term) {
    const int t = threadIdx.x;
    V acc[N];
#pragma unroll
    for (int k = 0; k < N; ++k) acc[k] = V(0);
    for (int i = t; i < n; i += T) term(i, acc);
#pragma unroll
    for (int k = 0; k < N; ++k) tree[k][t] = acc[k];
    __syncthreads();
    for (int h = T / 2; h > 0; h >>= 1) {
        if (t < h) {
#pragma unroll
            for (int k = 0; k < N; ++k) tree[k][t] += tree[k][t + h];
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < N; ++k) out[k] = tree[k][0];
}

// ---- one wave per row, kRowWaves rows per workgroup ----
//
//   const int lane = wave_lane(), r = wave_row();
//   if (r >= rows) return;
// launched by launch_rows(kernel, rows, stream, args...).
constexpr int kRowWaves = 4;

__device__ __forceinline__ int wave_lane() { return threadIdx.x & (kWave - 1); }
__device__ __forceinline__ int wave_row() { return blockIdx.x * kRowWaves + (threadIdx.x >> 6); }

// (the arguments are converted to the kernel's parameter types: a nullptr
// needs no cast at the call; the callers have range-checked what narrows)
template <typename... Params, typename... Args>
inline void launch_rows(void (*kernel)(Params...), int64_t rows, hipStream_t stream, Args... args) {
    hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(ceil_div(rows, kRowWaves))), dim3(kRowWaves * kWave), 0,
                       stream, static_cast<Params>(args)...);
}

// ---- cross-entropy row terms (one wave, lanes over the classes) ----

// log-sum-exp of one row (torch's log_softmax order: max, then sum of
// exp(x - max)); a NaN anywhere makes the sum NaN
__device__ __forceinline__ float row_lse(const float *__restrict__ xr, int C, int lane) {
    float m = -INFINITY;
    for (int c = lane; c < C; c += 64) m = fmaxf(m, xr[c]);
    m = wave_maxf(m);
    float s = 0.0f;
    for (int c = lane; c < C; c += 64) s += expf(xr[c] - m);
    s = wave_sum(s);
    return m + logf(s);
}

// the row's loss against label t; an out-of-range label: NaN, no OOB read
__device__ __forceinline__ float row_nll(const float *__restrict__ xr, float lse, int64_t t, int C) {
    return (t >= 0 && t < C) ? lse - xr[t] : NAN;
}

// Gradient rows are NOT shared: k_xent_fused divides each element by the
// count, k_xent_bwd and k_ct_bwd multiply by g / count -- different rounding.

}  // namespace ngnn
