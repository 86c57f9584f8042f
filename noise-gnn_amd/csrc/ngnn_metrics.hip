// Device-side epoch metrics: what the reference's training loops read back
// to the host after every batch (pipeline.py:120-125, :164-165:
// float(loss), int(out.argmax(dim=-1).eq(y).sum()), 100 * pure_ratio) and
// what its evaluation builds from the [N, C] logits (pipeline.py:182-195:
// argmax, three index gathers, three Evaluator.eval), as one launch each and
// no host read.
//
// Both kernels share one row argmax.  A group of G lanes (a power of two,
// about C / 4, so a lane holds up to four columns) takes a row; lane l reads
// columns l, l + G, ...: single-element loads, since a row starts at a
// multiple of ld elements and is only element aligned (C = 47 fp32 rows
// start at multiples of 188 B), which consecutive lanes coalesce into one
// contiguous segment per row.  Every element becomes a 64-bit key
//   (order(v) << 32) | (0xFFFFFFFF - column)
// with order() monotone over the floats, +0 == -0 and every NaN on top, so
// one unsigned max over the lane's columns and then over the group is
// torch.argmax's answer: the first index of the maximum, the first NaN if
// there is one, 0 for a row of -inf.
//
// Counters are summed per wave by shuffles and per workgroup through LDS;
// one lane per workgroup adds them to global memory with 64-bit integer
// vector atomics (the result does not depend on their order).
#include <algorithm>

#include "ngnn_rows.h"

namespace ngnn {
namespace {

constexpr int kConfusionMaxClasses = 128;
constexpr int kMaxSegments = 8;
constexpr int kStepThreads = 256;
constexpr int kSplitThreads = 1024;

typedef unsigned long long u64;

// Monotone over the floats as torch.argmax compares them: -inf < ... < -0 ==
// +0 < ... < +inf < NaN.  (ngnn_loss's loss_order_key keeps -0 below +0.)
__device__ __forceinline__ uint32_t argmax_order_key(float v) {
    if (v != v) return 0xFFFFFFFFu;
    if (v == 0.0f) return 0x80000000u;
    const uint32_t b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

template <bool BF16>
__device__ __forceinline__ float load_elem(const void *base, int64_t i) {
    if constexpr (BF16) {
        return __uint_as_float(static_cast<uint32_t>(static_cast<const uint16_t *>(base)[i]) << 16);  // (exact)
    } else {
        return static_cast<const float *>(base)[i];
    }
}

// The argmax of logits[row * ld .. + C) over the G lanes of a group (lane `gl`
// of it), known to every lane of the group afterwards.
template <bool BF16>
__device__ __forceinline__ int group_argmax(const void *logits, int64_t off, int C, int G, int gl) {
    u64 best = 0;
    for (int c = gl; c < C; c += G) {
        const u64 k = (static_cast<u64>(argmax_order_key(load_elem<BF16>(logits, off + c))) << 32) |
                      (0xFFFFFFFFu - static_cast<uint32_t>(c));
        best = k > best ? k : best;
    }
    for (int m = G >> 1; m > 0; m >>= 1) {
        const u64 o = __shfl_xor(best, m);
        best = o > best ? o : best;
    }
    return static_cast<int>(0xFFFFFFFFu - static_cast<uint32_t>(best));
}

// ------------------------------------------------------------ step metrics
template <bool BF16>
__global__ __launch_bounds__(kStepThreads) void k_step_metrics(const void *__restrict__ logits, int64_t ld, int B,
                                                               int C, int G, const int64_t *__restrict__ y,
                                                               int64_t ignore_index, const float *s0,
                                                               const float *s1, const float *s2, const float *s3,
                                                               u64 *__restrict__ acc) {
    __shared__ uint32_t s_part[kStepThreads / kWave][3];
    const int tid = threadIdx.x;
    const int gl = tid & (G - 1);
    const int per_block = kStepThreads / G;
    uint32_t n_rows = 0, n_ok = 0, n_bad = 0;
    // (the trip count is the same for every lane of a workgroup: the shuffles below run with whole groups)
    for (int64_t r0 = static_cast<int64_t>(blockIdx.x) * per_block; r0 < B;
         r0 += static_cast<int64_t>(gridDim.x) * per_block) {
        const int64_t r = r0 + tid / G;
        const bool live = r < B;
        const int64_t lab = live ? y[r] : ignore_index;
        const bool counted = live && lab >= 0 && lab < C;
        // (a row that is not counted is not read)
        const int am = group_argmax<BF16>(logits, r * ld, counted ? C : 0, G, gl);
        if (gl == 0 && live) {
            n_rows += counted;
            n_ok += counted && am == static_cast<int>(lab);
            n_bad += !counted && lab != ignore_index;
        }
    }
    n_rows = wave_sum(n_rows);
    n_ok = wave_sum(n_ok);
    n_bad = wave_sum(n_bad);
    if ((tid & (kWave - 1)) == 0) {
        s_part[tid / kWave][0] = n_rows;
        s_part[tid / kWave][1] = n_ok;
        s_part[tid / kWave][2] = n_bad;
    }
    __syncthreads();
    if (tid != 0) return;
    uint32_t t[3] = {0, 0, 0};
    for (int w = 0; w < kStepThreads / kWave; ++w)
        for (int k = 0; k < 3; ++k) t[k] += s_part[w][k];
    for (int k = 0; k < 3; ++k)
        if (t[k]) atomicAdd(acc + 1 + k, static_cast<u64>(t[k]));
    if (blockIdx.x != 0) return;
    // the launch's one thread: the step count and the scalar sums, in fp64
    atomicAdd(acc, static_cast<u64>(1));
    double *sums = reinterpret_cast<double *>(acc + 4);
    const float *s[4] = {s0, s1, s2, s3};
    for (int k = 0; k < 4; ++k)
        if (s[k]) sums[k] += static_cast<double>(*s[k]);
}

// ---------------------------------------------------------- split accuracy
struct Bounds {
    int64_t b[kMaxSegments + 1];
};

template <bool BF16>
__global__ __launch_bounds__(kSplitThreads) void k_split_accuracy(const void *__restrict__ logits, int64_t ld, int N,
                                                                  int C, int G, const int64_t *__restrict__ y,
                                                                  int64_t ignore_index,
                                                                  const int64_t *__restrict__ rows, int M, int S,
                                                                  Bounds bounds, u64 *__restrict__ counts,
                                                                  int64_t *__restrict__ pred,
                                                                  u64 *__restrict__ confusion) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_hist[];  // [C][C], with confusion only
    __shared__ uint32_t s_cnt[kMaxSegments][4];
    const int tid = threadIdx.x;
    const int CC = confusion ? C * C : 0;
    for (int k = tid; k < CC; k += kSplitThreads) s_hist[k] = 0;
    if (tid < kMaxSegments * 4) s_cnt[tid >> 2][tid & 3] = 0;
    __syncthreads();

    const int gl = tid & (G - 1);
    const int per_block = kSplitThreads / G;
    for (int64_t p0 = static_cast<int64_t>(blockIdx.x) * per_block; p0 < M;
         p0 += static_cast<int64_t>(gridDim.x) * per_block) {
        const int64_t p = p0 + tid / G;
        const bool live = p < M;
        const int64_t id = !live ? -1 : rows ? rows[p] : p;
        const bool id_ok = id >= 0 && id < N;
        const int64_t lab = id_ok ? y[id] : ignore_index;
        const bool counted = id_ok && lab >= 0 && lab < C;
        // a bad id's row is never read; an ignored or badly labelled row only for pred
        const bool read = counted || (id_ok && pred != nullptr);
        const int am = group_argmax<BF16>(logits, id * ld, read ? C : 0, G, gl);
        if (gl != 0 || !live) continue;
        int seg = 0;
        while (seg + 1 < S && p >= bounds.b[seg + 1]) ++seg;
        if (pred) pred[p] = id_ok ? am : -1;
        if (counted) {
            atomicAdd(&s_cnt[seg][0], 1u);
            if (am == static_cast<int>(lab)) atomicAdd(&s_cnt[seg][1], 1u);
            if (confusion) atomicAdd(s_hist + static_cast<int>(lab) * C + am, 1u);
        } else if (!id_ok || lab != ignore_index) {
            atomicAdd(&s_cnt[seg][2], 1u);
        } else {
            atomicAdd(&s_cnt[seg][3], 1u);
        }
    }
    __syncthreads();
    if (tid < S * 4) {
        const uint32_t v = s_cnt[tid >> 2][tid & 3];
        if (v) atomicAdd(counts + tid, static_cast<u64>(v));
    }
    for (int k = tid; k < CC; k += kSplitThreads) {
        const uint32_t v = s_hist[k];
        if (v) atomicAdd(confusion + k, static_cast<u64>(v));
    }
}

// lanes per row: the power of two at or above C / 4, at most a wave
inline int group_lanes(int64_t C) {
    int g = 1;
    while (g < kWave && 4 * g < C) g *= 2;
    return g;
}

}  // namespace
}  // namespace ngnn

using namespace ngnn;

extern "C" int ngnn_confusion_max_classes(void) { return kConfusionMaxClasses; }

extern "C" int ngnn_step_metrics(const void *logits, int64_t ld, int dtype, int64_t B, int64_t C, const int64_t *y,
                                 int64_t ignore_index, const float *s0, const float *s1, const float *s2,
                                 const float *s3, void *acc, void *stream) {
    NGNN_RETURN_IF(B < 0 || C < 1, NGNN_E_ARG);
    NGNN_RETURN_IF(!acc || (B > 0 && (!logits || !y)), NGNN_E_ARG);
    NGNN_RETURN_IF(!fits_i32(B) || !fits_i32(C), NGNN_E_RANGE);
    NGNN_RETURN_IF(ld < C, NGNN_E_SHAPE);
    NGNN_RETURN_IF(dtype != NGNN_F32 && dtype != NGNN_BF16, NGNN_E_DTYPE);
    NGNN_RETURN_IF(!aligned(acc, 8), NGNN_E_ALIGN);
    const int G = group_lanes(C);
    const int64_t grid = std::min<int64_t>(std::max<int64_t>(ceil_div(B * G, kStepThreads), 1), 8ll * num_cus());
    with_const<1, 0>(dtype == NGNN_BF16, [&](auto bf) {
        hipLaunchKernelGGL(k_step_metrics<decltype(bf)::value != 0>, dim3(static_cast<unsigned>(grid)),
                           dim3(kStepThreads), 0, as_stream(stream), logits, ld, static_cast<int>(B),
                           static_cast<int>(C), G, y, ignore_index, s0, s1, s2, s3, static_cast<u64 *>(acc));
    });
    return launch_status();
}

extern "C" int ngnn_split_accuracy(const void *logits, int64_t ld, int dtype, int64_t N, int64_t C, const int64_t *y,
                                   int64_t ignore_index, const int64_t *rows, int64_t M, int S,
                                   const int64_t *bounds, int64_t *counts, int64_t *pred, int64_t *confusion,
                                   void *stream) {
    NGNN_RETURN_IF(S < 1 || S > kMaxSegments || N < 0 || M < 0 || C < 1, NGNN_E_ARG);
    NGNN_RETURN_IF(!bounds || !counts, NGNN_E_ARG);
    NGNN_RETURN_IF(!rows && M != N && M != 0, NGNN_E_ARG);  // (an empty list needs no pointer)
    Bounds bv;
    for (int s = 0; s <= kMaxSegments; ++s) bv.b[s] = bounds[std::min(s, S)];
    NGNN_RETURN_IF(bv.b[0] != 0 || bv.b[S] != M, NGNN_E_ARG);
    for (int s = 0; s < S; ++s) NGNN_RETURN_IF(bv.b[s] > bv.b[s + 1], NGNN_E_ARG);
    NGNN_RETURN_IF(!fits_i32(N) || !fits_i32(M) || !fits_i32(C), NGNN_E_RANGE);
    NGNN_RETURN_IF(ld < C, NGNN_E_SHAPE);
    NGNN_RETURN_IF(confusion && C > kConfusionMaxClasses, NGNN_E_SHAPE);
    NGNN_RETURN_IF(dtype != NGNN_F32 && dtype != NGNN_BF16, NGNN_E_DTYPE);
    NGNN_RETURN_IF(M > 0 && N > 0 && (!logits || !y), NGNN_E_ARG);
    hipStream_t st = as_stream(stream);
    hipError_t e = hipMemsetAsync(counts, 0, sizeof(int64_t) * 4 * S, st);
    if (e == hipSuccess && confusion) e = hipMemsetAsync(confusion, 0, sizeof(int64_t) * C * C, st);
    if (e != hipSuccess) return static_cast<int>(e);
    if (M == 0) return NGNN_OK;
    if (N == 0) {  // every id is a bad one, and there is no row to read
        if (pred) e = hipMemsetAsync(pred, 0xFF, sizeof(int64_t) * M, st);
        return static_cast<int>(e);
    }
    const size_t lds = confusion ? sizeof(uint32_t) * static_cast<size_t>(C) * C : 0;
    const int G = group_lanes(C);
    const int64_t grid = std::min<int64_t>(ceil_div(M * G, kSplitThreads), 2ll * num_cus());
    with_const<1, 0>(dtype == NGNN_BF16, [&](auto bf) {
        constexpr bool kBf = decltype(bf)::value != 0;
        if (lds > 48 * 1024)
            max_dynamic_lds_once<k_split_accuracy<kBf>>(sizeof(uint32_t) * kConfusionMaxClasses * kConfusionMaxClasses);
        hipLaunchKernelGGL(k_split_accuracy<kBf>, dim3(static_cast<unsigned>(grid)), dim3(kSplitThreads), lds, st,
                           logits, ld, static_cast<int>(N), static_cast<int>(C), G, y, ignore_index, rows,
                           static_cast<int>(M), S, bv, reinterpret_cast<u64 *>(counts), pred,
                           reinterpret_cast<u64 *>(confusion));
    });
    return launch_status();
}
