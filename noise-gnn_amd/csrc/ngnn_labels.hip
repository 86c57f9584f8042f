// Label-noise injection: flip_label(labels, nbr_classes, noise_type, prob) of
// the reference's src/utils/noise.py:54-58 -- one draw per node from row
// y[i] of a row-stochastic transition matrix -- as one launch instead of a
// Python loop of .item(), np.random.multinomial and np.where per node.
//
// The draw is this library's own (include/ngnn.h): a 32-bit uniform r, a pure
// function of (seed, global node index), counted against the row's cumulative
// 32-bit thresholds.  The thresholds are non-decreasing along a row, so the
// count is an upper bound search: ceil(log2 C) LDS reads a node, the same
// number for every lane.
//
// One lane per node, a grid-stride loop over a grid of at most one 1024-thread
// workgroup per CU, four nodes a trip (four independent label loads in
// flight).  A workgroup stages the table in LDS once and gathers its share of
// counts[l][j] in an LDS histogram, flushed once with 64-bit vector atomics
// (non-zero cells only): a sym flip puts ~70 % of the nodes on the C diagonal
// cells, which one global atomic per node would serialise chip-wide.
//
// Dynamic LDS, 4 C (2 C + 1) bytes: thresholds uint32 [C][C], histogram
// uint32 [C][C], last non-zero class int32 [C].  C <= 128: 128.5 KiB of the
// CU's 160.
#include <algorithm>

#include "ngnn_sample_dev.h"

namespace ngnn {
namespace {

constexpr uint64_t kLabelSalt = 0xA0761D6478BD642Full;  // r = mix64(seed ^ mix64(i0 + i + kLabelSalt)) >> 32
constexpr int kMaxClasses = 128;
constexpr int kThreads = 1024;
constexpr int kPerTrip = 4;

inline size_t labels_lds_bytes(int64_t C) { return sizeof(uint32_t) * static_cast<size_t>(C) * (2 * C + 1); }

__global__ __launch_bounds__(kThreads) void k_flip_labels(const int64_t *__restrict__ y, int64_t n, int C,
                                                          const uint32_t *__restrict__ thr,
                                                          const int32_t *__restrict__ last, uint64_t seed,
                                                          uint64_t i0, int64_t *__restrict__ out,
                                                          uint8_t *__restrict__ clean,
                                                          unsigned long long *__restrict__ counts,
                                                          int32_t *__restrict__ bad) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const int CC = C * C;
    uint32_t *s_thr = lds;
    uint32_t *s_hist = lds + CC;
    int32_t *s_last = reinterpret_cast<int32_t *>(lds + 2 * CC);
    const int tid = threadIdx.x;
    for (int k = tid; k < CC; k += kThreads) {
        s_thr[k] = thr[k];
        s_hist[k] = 0;
    }
    // (clamped: whatever the table holds, no search leaves its row and no label leaves [0, C))
    for (int k = tid; k < C; k += kThreads) s_last[k] = min(max(last[k], 0), C - 1);
    __syncthreads();

    int step0 = 1;  // the largest power of two <= C
    while (2 * step0 <= C) step0 *= 2;
    const int64_t stride = static_cast<int64_t>(gridDim.x) * kThreads;
    int nbad = 0;
    for (int64_t base = static_cast<int64_t>(blockIdx.x) * kThreads + tid; base < n; base += kPerTrip * stride) {
        int64_t lab[kPerTrip];
#pragma unroll
        for (int u = 0; u < kPerTrip; ++u) {
            const int64_t i = base + u * stride;
            lab[u] = i < n ? y[i] : 0;
        }
#pragma unroll
        for (int u = 0; u < kPerTrip; ++u) {
            const int64_t i = base + u * stride;
            if (i >= n) continue;
            const int64_t l64 = lab[u];
            int64_t res = l64;
            if (l64 >= 0 && l64 < C) {
                const int l = static_cast<int>(l64);
                const uint32_t r =
                    static_cast<uint32_t>(mix64(seed ^ mix64(i0 + static_cast<uint64_t>(i) + kLabelSalt)) >> 32);
                // pos = #{k < jl : T[l][k] <= r}: the largest pos with T[l][pos - 1] <= r
                const uint32_t *row = s_thr + l * C;
                const int jl = s_last[l];
                int pos = 0;
                for (int s = step0; s > 0; s >>= 1) {
                    const int q = pos + s;
                    if (q <= jl && row[q - 1] <= r) pos = q;
                }
                res = pos;
                if (counts) atomicAdd(s_hist + l * C + pos, 1u);
            } else {
                ++nbad;
            }
            out[i] = res;
            if (clean) clean[i] = res == l64 ? 1 : 0;
        }
    }
    if (nbad && bad) atomicAdd(bad, nbad);
    if (!counts) return;  // (uniform over the grid)
    __syncthreads();
    for (int k = tid; k < CC; k += kThreads) {
        const uint32_t v = s_hist[k];
        if (v) atomicAdd(counts + k, static_cast<unsigned long long>(v));
    }
}

}  // namespace
}  // namespace ngnn

using namespace ngnn;

extern "C" int ngnn_flip_labels_max_classes(void) { return kMaxClasses; }

extern "C" int ngnn_flip_labels(const int64_t *y, int64_t n, int64_t C, const uint32_t *thr,
                                const int32_t *last, uint64_t seed, int64_t i0, int64_t *out,
                                uint8_t *clean, int64_t *counts, int32_t *bad, void *stream) {
    NGNN_RETURN_IF(n < 0 || C < 1 || i0 < 0, NGNN_E_ARG);
    NGNN_RETURN_IF(C > kMaxClasses, NGNN_E_SHAPE);
    NGNN_RETURN_IF(!fits_i32(n), NGNN_E_RANGE);
    if (n == 0) return NGNN_OK;
    NGNN_RETURN_IF(!y || !out || !thr || !last, NGNN_E_ARG);
    const size_t lds = labels_lds_bytes(C);
    if (lds > 48 * 1024) max_dynamic_lds_once<k_flip_labels>(labels_lds_bytes(kMaxClasses));
    const int64_t grid = std::min<int64_t>(ceil_div(n, kThreads), num_cus());
    hipLaunchKernelGGL(k_flip_labels, dim3(static_cast<unsigned>(grid)), dim3(kThreads), lds, as_stream(stream),
                       y, n, static_cast<int>(C), thr, last, seed, static_cast<uint64_t>(i0), out, clean,
                       reinterpret_cast<unsigned long long *>(counts), bad);
    return launch_status();
}
