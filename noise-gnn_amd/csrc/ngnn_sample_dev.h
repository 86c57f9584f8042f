// The sampler's draw, shared by the block sampler (ngnn_sample.hip) and the
// block-free evaluation kernels (ngnn_infer.hip): one definition, so the
// neighbours a seed row draws during layer-wise inference are bitwise the
// ones NeighborLoader's hop 0 hands it.
#pragma once

#include "ngnn_internal.h"

namespace ngnn {

constexpr int kMaxFanout = 64;

__device__ __forceinline__ uint64_t mix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// min(d, k) distinct CSR positions of a degree-d row, Floyd order; d <= k:
// all positions in CSR order.  Keyed by (seed, frontier position i).
__device__ __forceinline__ int floyd_sample(int64_t d, int fanout, uint64_t seed, int64_t i,
                                            int64_t (&sel)[kMaxFanout]) {
    const int k = d < fanout ? static_cast<int>(d) : fanout;
    if (d <= fanout) {
        for (int j = 0; j < k; ++j) sel[j] = j;
        return k;
    }
    const uint64_t base = mix64(seed ^ mix64(static_cast<uint64_t>(i) + 0x632BE59BD9B4E019ull));
    int m = 0;
    for (int64_t j = d - k; j < d; ++j) {
        const uint64_t r = mix64(base + static_cast<uint64_t>(j));
        const int64_t t = static_cast<int64_t>(
            (static_cast<unsigned __int128>(r) * static_cast<uint64_t>(j + 1)) >> 64);
        bool dup = false;
        for (int q = 0; q < m; ++q) dup |= sel[q] == t;
        sel[m++] = dup ? j : t;
    }
    return k;
}

// Lane-per-draw layout (round 6): frontier position i owns a group of KF
// lanes (KF = fanout rounded up to 8/16/32/64, a power of two dividing the
// wave), lane j its draw j.  The per-thread layout before it ran one thread
// per position -- 60 workgroups for a products hop-2 frontier, each thread a
// serial chain of draws, loads and atomics -- latency-bound at ~30 us a
// launch.  Floyd's draws are independent but for the duplicate test: draw q's
// final choice is known once draws < q are, so the group resolves them in
// fanout - 1 shuffle rounds (lane q's choice broadcast, later lanes compare).
// Same selections as floyd_sample.
template <int KF>
__device__ __forceinline__ int floyd_lane(int64_t d, int fanout, uint64_t seed, int i, int j, int &k) {
    k = d < fanout ? static_cast<int>(d) : fanout;
    if (d <= fanout) return j;
    const uint64_t base = mix64(seed ^ mix64(static_cast<uint64_t>(i) + 0x632BE59BD9B4E019ull));
    const int64_t J = d - k + j;  // (lanes j >= k compute a value nobody reads)
    const uint64_t r = mix64(base + static_cast<uint64_t>(J));
    const int32_t t = static_cast<int32_t>((static_cast<unsigned __int128>(r) * static_cast<uint64_t>(J + 1)) >> 64);
    const int32_t jw = static_cast<int32_t>(J);
    bool dup = false;
    for (int q = 0; q < k - 1; ++q) {  // (k is uniform over the group; every source lane is active)
        const int32_t fq = __shfl(dup ? jw : t, q, KF);
        dup |= j > q && fq == t;
    }
    return dup ? jw : t;
}

__host__ __device__ constexpr int sb_kf(int f) { return f <= 8 ? 8 : f <= 16 ? 16 : f <= 32 ? 32 : 64; }

// the per-hop seed of a block seeded `seed` (ngnn_sample_block, loader.sample_block)
__host__ __device__ constexpr uint64_t hop_seed(uint64_t seed, int h) {
    return seed * 1000003ull + static_cast<uint64_t>(h);
}

}  // namespace ngnn
