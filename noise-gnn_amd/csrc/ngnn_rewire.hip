// topk_rewire (the reference's src/utils/augmentation.py:36-86, directed=False):
// four global top-k selections over the N x N cosine-similarity matrix of the
// hidden state, and the two rewired edge lists that follow from them -- without
// N x N ever existing in memory.  With S = hn hn^T (hn = F.normalize(h)), A the
// edge set and D the diagonal, the selections take k2 entries each:
//   1 pos-remove  k2 smallest of  S * (A and not D ? 1 : 1000)
//   2 pos-add     k2 largest  of  S - 100 [A and not sel1] - 100 [D]
//   3 neg-remove  k2 largest  of  S * ([A] - 1000 [D])
//   4 neg-add     k2 smallest of  S * ((A ? 1000 : 1) + 1000 [D])
// pos = (A minus sel1) or sel2, neg = (A minus sel3) or sel4, each as
// torch.nonzero lists it.  Equal keys are taken in ascending flat index i*N+j.
//
// Shape.  Every entry is either EXPLICIT (an edge or a diagonal entry: at most
// E + N of them, sorted and deduplicated by flat index into the list X) or a
// plain non-edge, whose key in every selection is a monotone function of S
// alone: ascending S for selections 1 and 4, descending for 2, the constant 0
// for 3.  So
//   - the explicit entries get one dot product each and are candidates of every
//     selection, unconditionally;
//   - one dense tiled pass (exact-fp32 MFMA, 128 x 128 tile per workgroup, the
//     tile's explicit entries stamped into an LDS bitmask from X's row
//     pointers) feeds ONE histogram of S over the non-edges (kNB linear buckets
//     over [-1, 1], kept in LDS, flushed once per persistent workgroup); S is
//     symmetric, so only tiles (I, J) with I <= J are computed and an
//     off-diagonal tile stands for its transpose too (a second bitmask); a
//     one-workgroup scan finds the bucket that closes the k2 smallest and the
//     one that closes the k2 largest; a second dense pass recomputes the tiles
//     (the same instructions: bitwise the same S) and emits the entries at or
//     past those buckets as candidates, staged in LDS and appended with one
//     global atomic per tile and list;
//   - selection 3's non-edges all have key 0: its candidates are the first k2
//     flat indices of X's complement, found by a binary search each;
//   - each selection's candidates are sorted as (key, flat index) in one 64-bit
//     word (rocPRIM's device radix sort, temporary storage from the caller's
//     workspace) and cut at k2.  Selection 2's explicit keys wait for
//     selection 1; its dense candidates do not depend on it.
// The outputs are a sort + unique of (kept edges ++ additions).
// Candidate lists are bounded (k2 + kSlack non-edge entries per list).  Where
// a threshold bucket alone would overfill one (similarities concentrated in a
// narrow range), a third dense pass splits the two threshold buckets in kSub
// sub-buckets each -- about one fp32 step of S near |S| = 1 -- and the
// thresholds move to sub-buckets; without that need the pass returns at once.
// What can still overfill a list is a mass of more than 2^20 equal
// similarities at a threshold: reported in counts[2] (nothing is written out
// of bounds; the outputs are then not valid).
#include <algorithm>
#include <cstring>

#include <rocprim/device/device_radix_sort.hpp>

#include "ngnn_internal.h"

namespace ngnn {
namespace {

constexpr float kNormEps = 1e-12f;  // F.normalize's eps
constexpr int kNB = 8192;           // histogram buckets over S in [-1, 1]
constexpr int kSub = 4096;          // sub-buckets of a threshold bucket (the refinement pass)
constexpr int64_t kSlack = 1 << 20; // non-edge candidates a list may hold past k2
constexpr uint32_t kPad32 = 0xffffffffu;
constexpr uint64_t kPad64 = ~0ull;
constexpr int TM = 128;   // S tile edge per workgroup
constexpr int KC = 16;    // K chunk staged in LDS
constexpr int LDT = 20;   // LDS row stride of a staged chunk (16 + 4: conflict-free fragment reads)
constexpr int kStage = 1024;  // candidates a tile stages in LDS per list
constexpr int kNoMaxF = 1 << 20;

typedef float v4f __attribute__((ext_vector_type(4)));

struct State {
    int32_t M;         // explicit entries (|X|)
    int32_t b_lo;      // non-edges in buckets <= b_lo are candidates of selections 1 and 4
    int32_t b_hi;      // non-edges in buckets >= b_hi are candidates of selection 2
    uint32_t cnt_lo;   // emitted so far
    uint32_t cnt_hi;
    int32_t refine;    // a threshold bucket alone would overfill a list: split both in kSub
    int32_t sub_lo;    // ... and within bucket b_lo only sub-buckets <= sub_lo are candidates,
    int32_t sub_hi;    // within b_hi only those >= sub_hi
    uint32_t rem_lo;   // entries still needed from inside bucket b_lo / b_hi
    uint32_t rem_hi;
    uint32_t pad[2];
};

// order-preserving map of a float to uint32 (-0 folded into +0)
__device__ __forceinline__ uint32_t mono(float x) {
    const uint32_t b = __float_as_uint(x + 0.0f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float clamp1(float s) { return fminf(fmaxf(s, -1.0f), 1.0f); }
__device__ __forceinline__ int bucket_of(float s) {
    return min(kNB - 1, max(0, static_cast<int>((s + 1.0f) * static_cast<float>(kNB / 2))));
}
// position inside bucket b, monotone in s
__device__ __forceinline__ int sub_of(float s, int b) {
    const float t = ((s + 1.0f) * static_cast<float>(kNB / 2) - static_cast<float>(b)) * static_cast<float>(kSub);
    return min(kSub - 1, max(0, static_cast<int>(t)));
}
__device__ __forceinline__ uint64_t pack(uint32_t ukey, uint32_t idx) {
    return (static_cast<uint64_t>(ukey) << 32) | idx;
}
// the four selections' sort words (ascending = taken first)
__device__ __forceinline__ uint32_t ukey1(float s, bool a, bool d) { return mono(s * ((a && !d) ? 1.0f : 1000.0f)); }
__device__ __forceinline__ uint32_t ukey3(float s, bool a, bool d) {
    return ~mono(s * ((a ? 1.0f : 0.0f) - (d ? 1000.0f : 0.0f)));
}
__device__ __forceinline__ uint32_t ukey4(float s, bool a, bool d) {
    return mono(s * ((a ? 1000.0f : 1.0f) + (d ? 1000.0f : 0.0f)));
}
// selection 2: the penalties 100 and 200 exceed S's whole range, so the order
// is (penalty class, then S descending) exactly; S in [-1, 1] leaves room for
// the class in the word at the price of S's last bit in the penalised classes
__device__ __forceinline__ uint32_t ukey2(float s, int cls) {
    const uint32_t d = 0xBF800000u - mono(s);  // 0 at S = 1 ... 0x7F000001 at S = -1
    return cls == 0 ? d : 0x80000000u + static_cast<uint32_t>(cls - 1) * 0x40000000u + (d >> 1);
}

__device__ __forceinline__ int lower_bound_u32(const uint32_t *a, int lo, int hi, uint32_t v) {
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// ---- rows normalised once: hn[r, :Fp] = h[r, :F] / max(||h[r]||, eps), zero padded
__global__ __launch_bounds__(256) void k_normalize(const float *__restrict__ h, int64_t ldh, int n, int F,
                                                   int Fp, float *__restrict__ hn) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    const float *hr = h + static_cast<int64_t>(row) * ldh;
    float ss = 0.0f;
    for (int f = lane; f < F; f += 64) ss += hr[f] * hr[f];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o);
    const float d = fmaxf(sqrtf(ss), kNormEps);
    float *o = hn + static_cast<int64_t>(row) * Fp;
    for (int f = lane; f < Fp; f += 64) o[f] = f < F ? hr[f] / d : 0.0f;
}

// ---- sort words of the explicit entries: edges as 2*idx, the diagonal as 2*idx + 1
__global__ __launch_bounds__(256) void k_keys0(const int64_t *__restrict__ src, const int64_t *__restrict__ dst,
                                               int e, int n, uint64_t *__restrict__ keys,
                                               int32_t *__restrict__ bad) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= e + n) return;
    if (t < e) {
        const int64_t r = src[t], c = dst[t];
        if (r < 0 || r >= n || c < 0 || c >= n) {
            keys[t] = kPad64;
            if (bad) atomicAdd(bad, 1);
        } else {
            keys[t] = static_cast<uint64_t>(r * n + c) << 1;
        }
    } else {
        const uint64_t i = static_cast<uint64_t>(t - e);
        keys[t] = ((i * n + i) << 1) | 1u;
    }
}

// exclusive position of a set flag among the 1024 threads' flags, and their total
__device__ __forceinline__ int block_rank_1024(bool flag, int &total) {
    __shared__ int wsum[16];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint64_t m = __ballot(flag);
    if (lane == 0) wsum[w] = __popcll(m);
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int v = wsum[i];
        base += i < w ? v : 0;
        tot += v;
    }
    __syncthreads();
    total = tot;
    return base + __popcll(m & ((1ull << lane) - 1ull));
}

constexpr uint64_t kKey0Mask = (1ull << 34) - 1ull;  // the bits k_keys0's words are sorted on

// ---- X: the sorted words deduplicated by flat index (an edge sorts before the
// diagonal's marker of the same index, so the head's low bit tells A)
__global__ __launch_bounds__(1024) void k_compact_x(const uint64_t *__restrict__ keys, int T,
                                                    uint32_t *__restrict__ x_idx, uint8_t *__restrict__ x_a,
                                                    State *__restrict__ st) {
    int base = 0;
    for (int start = 0; start < T; start += 1024) {
        const int t = start + static_cast<int>(threadIdx.x);
        uint64_t k = kPad64;
        bool head = false;
        if (t < T) {
            k = keys[t];
            head = (k & kKey0Mask) != kKey0Mask && (t == 0 || (keys[t - 1] >> 1) != (k >> 1));
        }
        int total;
        const int p = base + block_rank_1024(head, total);
        if (head) {
            x_idx[p] = static_cast<uint32_t>(k >> 1);
            x_a[p] = static_cast<uint8_t>(!(k & 1u));
        }
        base += total;
    }
    if (threadIdx.x == 0) st->M = base;
}

__global__ __launch_bounds__(256) void k_rowptr(const uint32_t *__restrict__ x_idx, const State *__restrict__ st,
                                                int n, int32_t *__restrict__ rowptr) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i > n) return;
    rowptr[i] = lower_bound_u32(x_idx, 0, st->M, static_cast<uint32_t>(i) * static_cast<uint32_t>(n));
}

// ---- S of the explicit entries: 16 lanes per entry, float4 over the padded rows
__global__ __launch_bounds__(256) void k_xdot(const float *__restrict__ hn, int Fp, int n,
                                              const uint32_t *__restrict__ x_idx, const State *__restrict__ st,
                                              float *__restrict__ x_s) {
    const int sub = threadIdx.x & 15;
    const int t = blockIdx.x * 16 + (threadIdx.x >> 4);
    if (t >= st->M) return;  // (whole 16-lane groups)
    const uint32_t idx = x_idx[t];
    const float4 *a = reinterpret_cast<const float4 *>(hn + static_cast<int64_t>(idx / n) * Fp);
    const float4 *b = reinterpret_cast<const float4 *>(hn + static_cast<int64_t>(idx % n) * Fp);
    float s = 0.0f;
    for (int q = sub; q < Fp / 4; q += 16) {
        const float4 u = a[q], v = b[q];
        s += u.x * v.x + u.y * v.y + u.z * v.z + u.w * v.w;
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (sub == 0) x_s[t] = clamp1(s);
}

// ---- the dense pass over the non-edges.  MODE 0: histogram of S; MODE 1
// (only when a threshold bucket alone would overfill a list; returns at once
// otherwise): histograms of the positions inside the two threshold buckets;
// MODE 2: the entries at or past the thresholds become candidates.
// 256 threads = 4 waves, each a 64 x 64 quadrant of the 128 x 128 tile as 4 x 4
// v_mfma_f32_16x16x4_f32 accumulators.  A 16-wide K chunk of both operands is
// staged in LDS as [row][16 + 4]; lane group g = lane >> 4 owns k = 4g .. 4g+3
// of the chunk in both operands (one 16-B LDS read per fragment), and MFMA
// step j multiplies the groups' j-th elements: a fixed summation order, the
// same for (i, j) and (j, i), so S is bitwise symmetric.  The next chunk's
// global loads are issued before the current chunk's MFMAs.
template <int MODE>
__global__ __launch_bounds__(256) void k_dense(const float *__restrict__ hn, int Fp, int n,
                                               const uint32_t *__restrict__ x_idx,
                                               const int32_t *__restrict__ rowptr, uint32_t *__restrict__ hist,
                                               State *__restrict__ st, uint64_t *__restrict__ c1,
                                               uint64_t *__restrict__ c2, uint64_t *__restrict__ c4,
                                               uint32_t cn) {
    __shared__ __attribute__((aligned(16))) float sA[TM * LDT];
    __shared__ __attribute__((aligned(16))) float sB[TM * LDT];
    __shared__ uint32_t mask[TM * TM / 32];   // bit (li, lj): entry (row0 + li, col0 + lj) is explicit
    __shared__ uint32_t maskt[TM * TM / 32];  // bit (lj, li): its mirror (col0 + lj, row0 + li) is
    constexpr bool EMIT = MODE == 2;
    // MODE 0: the histogram; 1: [low bucket's | high bucket's] sub-histograms;
    // 2: [idx_lo | s_lo | idx_hi | s_hi] of kStage each
    __shared__ uint32_t sh[kNB];
    __shared__ uint32_t scnt[4];  // EMIT: staged counts (lo, hi), global bases (lo, hi)
    static_assert(4 * kStage <= kNB && 2 * kSub <= kNB, "the staging area and the sub-histograms alias the histogram");
    if (MODE == 1 && !st->refine) return;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int r16 = lane & 15, g = lane >> 4;
    const int wr = (w >> 1) * 64, wc = (w & 1) * 64;
    const int nt = (n + TM - 1) / TM;
    const int ntiles = nt * (nt + 1) / 2;  // tiles (I, J) with I <= J, row by row
    const int lr = tid >> 2, lq = tid & 3;  // loader: rows lr and lr + 64, floats 4 lq .. 4 lq + 3
    int b_lo = -1, b_hi = kNB, sub_lo = kSub - 1, sub_hi = 0;
    if (MODE != 0) {
        b_lo = st->b_lo;
        b_hi = st->b_hi;
        sub_lo = st->sub_lo;
        sub_hi = st->sub_hi;
    }
    if (!EMIT)
        for (int b = tid; b < kNB; b += 256) sh[b] = 0;
    uint32_t *s_idx_lo = sh, *s_idx_hi = sh + 2 * kStage;
    float *s_s_lo = reinterpret_cast<float *>(sh + kStage), *s_s_hi = reinterpret_cast<float *>(sh + 3 * kStage);

    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        // row I starts at I * nt - I (I - 1) / 2
        int ti = static_cast<int>((static_cast<float>(2 * nt + 1) -
                                   sqrtf(static_cast<float>((2 * nt + 1) * (2 * nt + 1) - 8 * tile))) * 0.5f);
        ti = min(max(ti, 0), nt - 1);
        while (ti > 0 && ti * nt - ti * (ti - 1) / 2 > tile) --ti;
        while (ti + 1 < nt && (ti + 1) * nt - (ti + 1) * ti / 2 <= tile) ++ti;
        const int tj = ti + tile - (ti * nt - ti * (ti - 1) / 2);
        const bool mirror = ti != tj;  // an off-diagonal tile also stands for its transpose
        const int row0 = ti * TM, col0 = tj * TM;
        __syncthreads();  // the previous tile's masks, staging area and operands are done with
        for (int q = tid; q < TM * TM / 32; q += 256) {
            mask[q] = 0;
            maskt[q] = 0;
        }
        if (EMIT && tid < 2) scnt[tid] = 0;
        __syncthreads();
        if (tid < TM && row0 + tid < n) {  // stamp the tile's explicit entries
            const int row = row0 + tid;
            const uint32_t first = static_cast<uint32_t>(row) * static_cast<uint32_t>(n) + col0;
            const int hi = rowptr[row + 1];
            for (int p = lower_bound_u32(x_idx, rowptr[row], hi, first); p < hi; ++p) {
                const uint32_t c = x_idx[p] - first;
                if (c >= TM) break;
                atomicOr(&mask[tid * (TM / 32) + (c >> 5)], 1u << (c & 31));
            }
        }
        if (mirror && tid >= TM && col0 + (tid - TM) < n) {  // and the transposed tile's
            const int lj = tid - TM, row = col0 + lj;
            const uint32_t first = static_cast<uint32_t>(row) * static_cast<uint32_t>(n) + row0;
            const int hi = rowptr[row + 1];
            for (int p = lower_bound_u32(x_idx, rowptr[row], hi, first); p < hi; ++p) {
                const uint32_t c = x_idx[p] - first;
                if (c >= TM) break;
                atomicOr(&maskt[lj * (TM / 32) + (c >> 5)], 1u << (c & 31));
            }
        }
        v4f acc[4][4];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) acc[a][b] = v4f{0.0f, 0.0f, 0.0f, 0.0f};
        const float4 zero4 = float4{0.0f, 0.0f, 0.0f, 0.0f};
        const bool va0 = row0 + lr < n, va1 = row0 + lr + 64 < n;
        const bool vb0 = col0 + lr < n, vb1 = col0 + lr + 64 < n;
        const float *ga0 = hn + static_cast<int64_t>(row0 + lr) * Fp + 4 * lq;
        const float *ga1 = ga0 + static_cast<int64_t>(64) * Fp;
        const float *gb0 = hn + static_cast<int64_t>(col0 + lr) * Fp + 4 * lq;
        const float *gb1 = gb0 + static_cast<int64_t>(64) * Fp;
        float4 pa0 = zero4, pa1 = zero4, pb0 = zero4, pb1 = zero4;
        if (Fp > 0) {
            pa0 = va0 ? *reinterpret_cast<const float4 *>(ga0) : zero4;
            pa1 = va1 ? *reinterpret_cast<const float4 *>(ga1) : zero4;
            pb0 = vb0 ? *reinterpret_cast<const float4 *>(gb0) : zero4;
            pb1 = vb1 ? *reinterpret_cast<const float4 *>(gb1) : zero4;
        }
        for (int k0 = 0; k0 < Fp; k0 += KC) {
            *reinterpret_cast<float4 *>(&sA[lr * LDT + 4 * lq]) = pa0;
            *reinterpret_cast<float4 *>(&sA[(lr + 64) * LDT + 4 * lq]) = pa1;
            *reinterpret_cast<float4 *>(&sB[lr * LDT + 4 * lq]) = pb0;
            *reinterpret_cast<float4 *>(&sB[(lr + 64) * LDT + 4 * lq]) = pb1;
            __syncthreads();
            if (k0 + KC < Fp) {
                const int kn = k0 + KC;
                pa0 = va0 ? *reinterpret_cast<const float4 *>(ga0 + kn) : zero4;
                pa1 = va1 ? *reinterpret_cast<const float4 *>(ga1 + kn) : zero4;
                pb0 = vb0 ? *reinterpret_cast<const float4 *>(gb0 + kn) : zero4;
                pb1 = vb1 ? *reinterpret_cast<const float4 *>(gb1 + kn) : zero4;
            }
            float4 fa[4], fb[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                fa[a] = *reinterpret_cast<const float4 *>(&sA[(wr + a * 16 + r16) * LDT + 4 * g]);
                fb[a] = *reinterpret_cast<const float4 *>(&sB[(wc + a * 16 + r16) * LDT + 4 * g]);
            }
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[a].x, fb[b].x, acc[a][b], 0, 0, 0);
                    acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[a].y, fb[b].y, acc[a][b], 0, 0, 0);
                    acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[a].z, fb[b].z, acc[a][b], 0, 0, 0);
                    acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[a].w, fb[b].w, acc[a][b], 0, 0, 0);
                }
            __syncthreads();
        }
        if (Fp == 0) __syncthreads();  // (the mask's stamps, which the K loop's barriers otherwise order)
        // C/D map: column = lane & 15, row = 4 * (lane >> 4) + register
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int li = wr + a * 16 + 4 * g + r, lj = wc + b * 16 + r16;
                    const int row = row0 + li, col = col0 + lj;
                    if (row >= n || col >= n) continue;
                    const bool e0 = !((mask[li * (TM / 32) + (lj >> 5)] >> (lj & 31)) & 1u);
                    const bool e1 = mirror && !((maskt[lj * (TM / 32) + (li >> 5)] >> (li & 31)) & 1u);
                    if (!e0 && !e1) continue;
                    const float s = clamp1(acc[a][b][r]);
                    const int bk = bucket_of(s);
                    const uint32_t both = static_cast<uint32_t>(e0) + static_cast<uint32_t>(e1);
                    if (MODE == 0) {
                        atomicAdd(&sh[bk], both);
                        continue;
                    }
                    if (bk > b_lo && bk < b_hi) continue;
                    if (MODE == 1) {
                        if (bk == b_lo) atomicAdd(&sh[sub_of(s, bk)], both);
                        if (bk == b_hi) atomicAdd(&sh[kSub + sub_of(s, bk)], both);
                        continue;
                    }
                    const bool lo = bk < b_lo || (bk == b_lo && sub_of(s, bk) <= sub_lo);
                    const bool hi = bk > b_hi || (bk == b_hi && sub_of(s, bk) >= sub_hi);
                    if (!lo && !hi) continue;
#pragma unroll
                    for (int o = 0; o < 2; ++o) {
                        if (!(o ? e1 : e0)) continue;
                        const uint32_t idx = o ? static_cast<uint32_t>(col) * static_cast<uint32_t>(n) + row
                                               : static_cast<uint32_t>(row) * static_cast<uint32_t>(n) + col;
                        if (lo) {
                            const uint32_t p = atomicAdd(&scnt[0], 1u);
                            if (p < kStage) {
                                s_idx_lo[p] = idx;
                                s_s_lo[p] = s;
                            } else {  // a tile with more candidates than the staging area
                                const uint32_t q = atomicAdd(&st->cnt_lo, 1u);
                                if (q < cn) {
                                    c1[q] = pack(ukey1(s, false, false), idx);
                                    c4[q] = pack(ukey4(s, false, false), idx);
                                }
                            }
                        }
                        if (hi) {
                            const uint32_t p = atomicAdd(&scnt[1], 1u);
                            if (p < kStage) {
                                s_idx_hi[p] = idx;
                                s_s_hi[p] = s;
                            } else {
                                const uint32_t q = atomicAdd(&st->cnt_hi, 1u);
                                if (q < cn) c2[q] = pack(ukey2(s, 0), idx);
                            }
                        }
                    }
                }
        if (EMIT) {
            __syncthreads();
            const uint32_t nlo = min(scnt[0], static_cast<uint32_t>(kStage));
            const uint32_t nhi = min(scnt[1], static_cast<uint32_t>(kStage));
            if (tid == 0 && nlo) scnt[2] = atomicAdd(&st->cnt_lo, nlo);
            if (tid == 1 && nhi) scnt[3] = atomicAdd(&st->cnt_hi, nhi);
            __syncthreads();
            for (uint32_t p = tid; p < nlo; p += 256) {
                const uint32_t q = scnt[2] + p;
                if (q < cn) {
                    c1[q] = pack(ukey1(s_s_lo[p], false, false), s_idx_lo[p]);
                    c4[q] = pack(ukey4(s_s_lo[p], false, false), s_idx_lo[p]);
                }
            }
            for (uint32_t p = tid; p < nhi; p += 256) {
                const uint32_t q = scnt[3] + p;
                if (q < cn) c2[q] = pack(ukey2(s_s_hi[p], 0), s_idx_hi[p]);
            }
        }
    }
    if (!EMIT) {  // (MODE 1: hist is the sub-histograms' global copy)
        __syncthreads();
        for (int b = tid; b < kNB; b += 256)
            if (sh[b]) atomicAdd(&hist[b], sh[b]);
    }
}

// ---- the two threshold buckets: the smallest b whose cumulative count from
// below reaches min(k2, all), and the largest whose count from above does
__global__ __launch_bounds__(1024) void k_thresholds(const uint32_t *__restrict__ hist, uint32_t k2, uint32_t cn,
                                                     State *__restrict__ st) {
    constexpr int PER = kNB / 1024;
    __shared__ uint32_t part[1024];
    uint32_t s = 0;
    for (int i = 0; i < PER; ++i) s += hist[threadIdx.x * PER + i];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x != 0) return;
    uint64_t all = 0;
    for (int i = 0; i < 1024; ++i) all += part[i];
    const uint64_t need = all < k2 ? all : k2;
    int b_lo = -1, b_hi = kNB;
    uint32_t rem_lo = 0, rem_hi = 0;
    bool refine = false;
    if (need > 0) {
        uint64_t cum = 0;
        int p = 0;
        while (cum + part[p] < need) cum += part[p++];
        int b = p * PER;
        while (cum + hist[b] < need) cum += hist[b++];
        b_lo = b;
        rem_lo = static_cast<uint32_t>(need - cum);
        refine = cum + hist[b] > cn;
        cum = 0;
        p = 1023;
        while (cum + part[p] < need) cum += part[p--];
        b = p * PER + PER - 1;
        while (cum + hist[b] < need) cum += hist[b--];
        b_hi = b;
        rem_hi = static_cast<uint32_t>(need - cum);
        refine = refine || cum + hist[b] > cn;
    }
    st->b_lo = b_lo;
    st->b_hi = b_hi;
    st->rem_lo = rem_lo;
    st->rem_hi = rem_hi;
    st->refine = refine ? 1 : 0;
    st->sub_lo = kSub - 1;  // (the whole bucket, unless k_sub_thresholds narrows it)
    st->sub_hi = 0;
}

// ---- after the refinement pass: the sub-buckets that close what is still
// needed from inside the two threshold buckets
__global__ __launch_bounds__(1024) void k_sub_thresholds(const uint32_t *__restrict__ hist2,
                                                         State *__restrict__ st) {
    if (!st->refine) return;
    constexpr int PER = kSub / 1024;
    __shared__ uint32_t part[2][1024];
    for (int e = 0; e < 2; ++e) {
        uint32_t s = 0;
        for (int i = 0; i < PER; ++i) s += hist2[e * kSub + threadIdx.x * PER + i];
        part[e][threadIdx.x] = s;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    // (rem <= the bucket's count, which the sub-histogram sums to: the scans end inside it)
    uint64_t cum = 0;
    int p = 0;
    const uint32_t rem_lo = st->rem_lo, rem_hi = st->rem_hi;
    while (p < 1023 && cum + part[0][p] < rem_lo) cum += part[0][p++];
    int b = p * PER;
    while (b < p * PER + PER - 1 && cum + hist2[b] < rem_lo) cum += hist2[b++];
    st->sub_lo = b;
    cum = 0;
    p = 1023;
    while (p > 0 && cum + part[1][p] < rem_hi) cum += part[1][p--];
    b = p * PER + PER - 1;
    while (b > p * PER && cum + hist2[kSub + b] < rem_hi) cum += hist2[kSub + b--];
    st->sub_hi = b;
}

// ---- the explicit entries' sort words.  SEL2 = false: selections 1, 3, 4;
// SEL2 = true: selection 2, once selection 1's removals are marked.
template <bool SEL2>
__global__ __launch_bounds__(256) void k_fill_explicit(const uint32_t *__restrict__ x_idx,
                                                       const uint8_t *__restrict__ x_a,
                                                       const float *__restrict__ x_s,
                                                       const uint8_t *__restrict__ rem1,
                                                       const State *__restrict__ st, int T, int n,
                                                       uint64_t *__restrict__ c1, uint64_t *__restrict__ c2,
                                                       uint64_t *__restrict__ c3, uint64_t *__restrict__ c4) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    if (t >= st->M) {
        if (SEL2) {
            c2[t] = kPad64;
        } else {
            c1[t] = kPad64;
            c3[t] = kPad64;
            c4[t] = kPad64;
        }
        return;
    }
    const uint32_t idx = x_idx[t];
    const bool a = x_a[t] != 0, d = idx / n == idx % n;
    const float s = x_s[t];
    if (SEL2) {
        c2[t] = pack(ukey2(s, ((a && !rem1[t]) ? 1 : 0) + (d ? 1 : 0)), idx);
    } else {
        c1[t] = pack(ukey1(s, a, d), idx);
        c3[t] = pack(ukey3(s, a, d), idx);
        c4[t] = pack(ukey4(s, a, d), idx);
    }
}

// ---- selection 3's non-edges (key 0 each): the r-th smallest flat index that
// is not in X is r + #{t : X[t] - t <= r}
__global__ __launch_bounds__(256) void k_zero_pool(const uint32_t *__restrict__ x_idx,
                                                   const State *__restrict__ st, int n, uint32_t zcap,
                                                   uint64_t *__restrict__ out) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= zcap) return;
    const int M = st->M;
    const uint64_t nn = static_cast<uint64_t>(n) * n;
    if (static_cast<uint64_t>(r) + M >= nn) {  // X's complement has fewer than r + 1 entries
        out[r] = kPad64;
        return;
    }
    int lo = 0, hi = M;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (x_idx[mid] - static_cast<uint32_t>(mid) <= r) lo = mid + 1;
        else hi = mid;
    }
    out[r] = pack(ukey3(0.0f, false, false), r + static_cast<uint32_t>(lo));
}

// ---- a sorted list's first k2 entries are the selection; mark the edges among them
__global__ __launch_bounds__(256) void k_take(const uint64_t *__restrict__ sorted, int k2,
                                              const uint32_t *__restrict__ x_idx, const uint8_t *__restrict__ x_a,
                                              const State *__restrict__ st, uint32_t *__restrict__ sel,
                                              int64_t *__restrict__ sel_out, uint8_t *__restrict__ rem) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= k2) return;
    const uint32_t idx = static_cast<uint32_t>(sorted[k]);
    sel[k] = idx;
    if (sel_out) sel_out[k] = idx;
    if (rem) {
        const int M = st->M;
        const int t = lower_bound_u32(x_idx, 0, M, idx);
        if (t < M && x_idx[t] == idx && x_a[t]) rem[t] = 1;
    }
}

// ---- (kept edges ++ additions), to be sorted
__global__ __launch_bounds__(256) void k_build_list(const uint32_t *__restrict__ x_idx,
                                                    const uint8_t *__restrict__ x_a,
                                                    const uint8_t *__restrict__ rem,
                                                    const State *__restrict__ st, int T,
                                                    const uint32_t *__restrict__ sel, int k2,
                                                    uint32_t *__restrict__ list) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= T + k2) return;
    if (t >= T) list[t] = sel[t - T];
    else list[t] = (t < st->M && x_a[t] && !rem[t]) ? x_idx[t] : kPad32;
}

// ---- the sorted list without duplicates, as int64 [2, cap] rows; its length
__global__ __launch_bounds__(1024) void k_compact_out(const uint32_t *__restrict__ list, int L, int n,
                                                      int64_t *__restrict__ out, int64_t cap,
                                                      int32_t *__restrict__ count,
                                                      const State *__restrict__ st, uint32_t cn,
                                                      int32_t *__restrict__ overflow) {
    int base = 0;
    for (int start = 0; start < L; start += 1024) {
        const int t = start + static_cast<int>(threadIdx.x);
        uint32_t v = kPad32;
        bool head = false;
        if (t < L) {
            v = list[t];
            head = v != kPad32 && (t == 0 || list[t - 1] != v);
        }
        int total;
        const int p = base + block_rank_1024(head, total);
        if (head && p < cap) {
            out[p] = v / static_cast<uint32_t>(n);
            out[cap + p] = v % static_cast<uint32_t>(n);
        }
        base += total;
    }
    if (threadIdx.x == 0) {
        *count = base;
        if (overflow) *overflow = (st->cnt_lo > cn || st->cnt_hi > cn) ? 1 : 0;
    }
}

// ------------------------------------------------------------------ host side
template <class K>
hipError_t sort_keys(void *tmp, size_t &bytes, const K *in, K *out, size_t count, unsigned end_bit,
                     hipStream_t st) {
    return rocprim::radix_sort_keys(tmp, bytes, in, out, count, 0u, end_bit, st);
}

template <class K>
size_t sort_temp_bytes(size_t count, unsigned end_bit) {
    size_t bytes = 0;
    if (count == 0) return 0;
    const hipError_t e = sort_keys<K>(nullptr, bytes, nullptr, nullptr, count, end_bit, nullptr);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        // no device to ask (a sizing call on a host without one): a second
        // key buffer plus the per-block histograms and look-back state
        bytes = count * sizeof(K) * 2 + (size_t{4} << 20);
    }
    return bytes;
}

size_t up256(size_t v) { return (v + 255) & ~size_t{255}; }

struct Layout {
    int64_t T, Fp, cn, cap[4], zcap, L;
    size_t hn, key0_in, key0_out, x_idx, x_a, x_s, rowptr, rem1, rem3, hist, hist2, state, cand_in[4], cand_out[4],
        sel, list_in, list_out, temp, temp_bytes, total;
};

Layout make_layout(int64_t n, int64_t F, int64_t e, int64_t k2) {
    Layout L{};
    L.T = e + n;
    L.Fp = ceil_div(F, KC) * KC;
    const int64_t nn = n * n;
    L.cn = k2 == 0 ? 0 : (nn < k2 + kSlack ? nn : k2 + kSlack);
    L.zcap = k2;
    L.cap[0] = L.cap[1] = L.cap[3] = L.T + L.cn;
    L.cap[2] = L.T + L.zcap;
    L.L = L.T + k2;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        const size_t at = off;
        off += up256(bytes);
        return at;
    };
    L.hn = take(static_cast<size_t>(n) * L.Fp * 4);
    L.key0_in = take(static_cast<size_t>(L.T) * 8);
    L.key0_out = take(static_cast<size_t>(L.T) * 8);
    L.x_idx = take(static_cast<size_t>(L.T) * 4);
    L.x_a = take(static_cast<size_t>(L.T));
    L.x_s = take(static_cast<size_t>(L.T) * 4);
    L.rowptr = take(static_cast<size_t>(n + 1) * 4);
    // (one memset clears rem1 .. state: the marks, both histograms, the state)
    L.rem1 = take(static_cast<size_t>(L.T));
    L.rem3 = take(static_cast<size_t>(L.T));
    L.hist = take(static_cast<size_t>(kNB) * 4);
    L.hist2 = take(static_cast<size_t>(2 * kSub) * 4);
    L.state = take(sizeof(State));
    for (int s = 0; s < 4; ++s) {
        L.cand_in[s] = take(static_cast<size_t>(L.cap[s]) * 8);
        L.cand_out[s] = take(static_cast<size_t>(L.cap[s]) * 8);
    }
    L.sel = take(static_cast<size_t>(4 * k2) * 4);
    L.list_in = take(static_cast<size_t>(L.L) * 4);
    L.list_out = take(static_cast<size_t>(L.L) * 4);
    size_t tb = sort_temp_bytes<uint64_t>(L.T, 34);
    for (int s = 0; s < 4; ++s) tb = std::max(tb, sort_temp_bytes<uint64_t>(L.cap[s], 64));
    tb = std::max(tb, sort_temp_bytes<uint32_t>(L.L, 32));
    L.temp_bytes = tb;
    L.temp = take(tb);
    L.total = off;
    return L;
}

int check_sizes(int64_t n, int64_t F, int64_t e, int64_t k2) {
    NGNN_RETURN_IF(n < 0 || F < 0 || e < 0 || k2 < 0, NGNN_E_ARG);
    // (n <= 65535: a flat index fits 32 bits; the list lengths below fit an int)
    NGNN_RETURN_IF(n > 65535 || F > kNoMaxF || e > (int64_t{1} << 29), NGNN_E_RANGE);
    NGNN_RETURN_IF(k2 > n * n || k2 > (int64_t{1} << 29), NGNN_E_RANGE);
    return NGNN_OK;
}

unsigned blocks(int64_t items, int per) { return static_cast<unsigned>(ceil_div(items, per)); }

}  // namespace
}  // namespace ngnn

using namespace ngnn;

extern "C" size_t ngnn_topk_rewire_workspace_bytes(int64_t n, int64_t F, int64_t e, int64_t k2) {
    if (check_sizes(n, F, e, k2) != NGNN_OK || n == 0) return 0;
    return make_layout(n, F, e, k2).total;
}

extern "C" int ngnn_topk_rewire(const float *h, int64_t ldh, int64_t n, int64_t F, const int64_t *src,
                                const int64_t *dst, int64_t e, int64_t k2, int64_t *pos, int64_t pos_cap,
                                int64_t *neg, int64_t neg_cap, int32_t *counts, int32_t *bad,
                                int64_t *sel_out, void *ws, size_t ws_bytes, void *stream) {
    const int rc = check_sizes(n, F, e, k2);
    if (rc) return rc;
    NGNN_RETURN_IF(ldh < 0 || pos_cap < 0 || neg_cap < 0, NGNN_E_ARG);
    NGNN_RETURN_IF(ldh < F, NGNN_E_SHAPE);
    NGNN_RETURN_IF(!fits_i32(pos_cap) || !fits_i32(neg_cap), NGNN_E_RANGE);
    if (n == 0) return NGNN_OK;
    NGNN_RETURN_IF((F > 0 && !h) || (e > 0 && (!src || !dst)) || (pos_cap > 0 && !pos) ||
                       (neg_cap > 0 && !neg) || !counts || !ws,
                   NGNN_E_ARG);
    NGNN_RETURN_IF(!aligned(ws, 256) || !aligned(pos, 8) || !aligned(neg, 8), NGNN_E_ALIGN);
    const Layout L = make_layout(n, F, e, k2);
    NGNN_RETURN_IF(ws_bytes < L.total, NGNN_E_WORKSPACE);

    hipStream_t st = as_stream(stream);
    char *base = static_cast<char *>(ws);
    float *hn = reinterpret_cast<float *>(base + L.hn);
    uint64_t *key0_in = reinterpret_cast<uint64_t *>(base + L.key0_in);
    uint64_t *key0_out = reinterpret_cast<uint64_t *>(base + L.key0_out);
    uint32_t *x_idx = reinterpret_cast<uint32_t *>(base + L.x_idx);
    uint8_t *x_a = reinterpret_cast<uint8_t *>(base + L.x_a);
    float *x_s = reinterpret_cast<float *>(base + L.x_s);
    int32_t *rowptr = reinterpret_cast<int32_t *>(base + L.rowptr);
    uint8_t *rem1 = reinterpret_cast<uint8_t *>(base + L.rem1);
    uint8_t *rem3 = reinterpret_cast<uint8_t *>(base + L.rem3);
    uint32_t *hist = reinterpret_cast<uint32_t *>(base + L.hist);
    uint32_t *hist2 = reinterpret_cast<uint32_t *>(base + L.hist2);
    State *state = reinterpret_cast<State *>(base + L.state);
    uint64_t *cin[4], *cout[4];
    for (int s = 0; s < 4; ++s) {
        cin[s] = reinterpret_cast<uint64_t *>(base + L.cand_in[s]);
        cout[s] = reinterpret_cast<uint64_t *>(base + L.cand_out[s]);
    }
    uint32_t *sel = reinterpret_cast<uint32_t *>(base + L.sel);
    uint32_t *list_in = reinterpret_cast<uint32_t *>(base + L.list_in);
    uint32_t *list_out = reinterpret_cast<uint32_t *>(base + L.list_out);
    void *temp = base + L.temp;
    const int ni = static_cast<int>(n), Fi = static_cast<int>(F), Fp = static_cast<int>(L.Fp);
    const int ei = static_cast<int>(e), T = static_cast<int>(L.T), k2i = static_cast<int>(k2);
    const uint32_t cn = static_cast<uint32_t>(L.cn);
    size_t tb;

#define NGNN_REWIRE_HIP(call)                                      \
    do {                                                           \
        const hipError_t e_ = (call);                              \
        if (e_ != hipSuccess) return static_cast<int>(e_);         \
    } while (0)

    // rem1, rem3, hist, state: one clear; the candidate lists' non-edge parts: pads
    NGNN_REWIRE_HIP(hipMemsetAsync(rem1, 0, L.state + sizeof(State) - L.rem1, st));
    for (int s = 0; s < 4; ++s)
        if (L.cap[s] > T)
            NGNN_REWIRE_HIP(hipMemsetAsync(cin[s] + T, 0xff, static_cast<size_t>(L.cap[s] - T) * 8, st));

    hipLaunchKernelGGL(k_normalize, dim3(blocks(n, 4)), dim3(256), 0, st, h, ldh, ni, Fi, Fp, hn);
    hipLaunchKernelGGL(k_keys0, dim3(blocks(T, 256)), dim3(256), 0, st, src, dst, ei, ni, key0_in, bad);
    tb = L.temp_bytes;
    NGNN_REWIRE_HIP(sort_keys<uint64_t>(temp, tb, key0_in, key0_out, T, 34, st));
    hipLaunchKernelGGL(k_compact_x, dim3(1), dim3(1024), 0, st, key0_out, T, x_idx, x_a, state);
    hipLaunchKernelGGL(k_rowptr, dim3(blocks(n + 1, 256)), dim3(256), 0, st, x_idx, state, ni, rowptr);
    hipLaunchKernelGGL(k_xdot, dim3(blocks(T, 16)), dim3(256), 0, st, hn, Fp, ni, x_idx, state, x_s);

    if (k2 > 0) {
        const int64_t nt = ceil_div(n, TM);
        const unsigned grid =
            static_cast<unsigned>(std::min<int64_t>(nt * (nt + 1) / 2, 2 * static_cast<int64_t>(num_cus())));
        hipLaunchKernelGGL((k_dense<0>), dim3(grid), dim3(256), 0, st, hn, Fp, ni, x_idx, rowptr, hist, state,
                           cin[0] + T, cin[1] + T, cin[3] + T, cn);
        hipLaunchKernelGGL(k_thresholds, dim3(1), dim3(1024), 0, st, hist, static_cast<uint32_t>(k2), cn, state);
        // (both return at once unless a threshold bucket alone would overfill a list)
        hipLaunchKernelGGL((k_dense<1>), dim3(grid), dim3(256), 0, st, hn, Fp, ni, x_idx, rowptr, hist2, state,
                           cin[0] + T, cin[1] + T, cin[3] + T, cn);
        hipLaunchKernelGGL(k_sub_thresholds, dim3(1), dim3(1024), 0, st, hist2, state);
        hipLaunchKernelGGL((k_dense<2>), dim3(grid), dim3(256), 0, st, hn, Fp, ni, x_idx, rowptr, hist, state,
                           cin[0] + T, cin[1] + T, cin[3] + T, cn);
        hipLaunchKernelGGL(k_zero_pool, dim3(blocks(L.zcap, 256)), dim3(256), 0, st, x_idx, state, ni,
                           static_cast<uint32_t>(L.zcap), cin[2] + T);
    }
    hipLaunchKernelGGL((k_fill_explicit<false>), dim3(blocks(T, 256)), dim3(256), 0, st, x_idx, x_a, x_s, rem1,
                       state, T, ni, cin[0], cin[1], cin[2], cin[3]);
    for (int s : {0, 2, 3}) {
        tb = L.temp_bytes;
        NGNN_REWIRE_HIP(sort_keys<uint64_t>(temp, tb, cin[s], cout[s], L.cap[s], 64, st));
        if (k2 > 0)
            hipLaunchKernelGGL(k_take, dim3(blocks(k2, 256)), dim3(256), 0, st, cout[s], k2i, x_idx, x_a, state,
                               sel + static_cast<int64_t>(s) * k2, sel_out ? sel_out + s * k2 : nullptr,
                               s == 0 ? rem1 : (s == 2 ? rem3 : nullptr));
    }
    hipLaunchKernelGGL((k_fill_explicit<true>), dim3(blocks(T, 256)), dim3(256), 0, st, x_idx, x_a, x_s, rem1,
                       state, T, ni, cin[0], cin[1], cin[2], cin[3]);
    tb = L.temp_bytes;
    NGNN_REWIRE_HIP(sort_keys<uint64_t>(temp, tb, cin[1], cout[1], L.cap[1], 64, st));
    if (k2 > 0)
        hipLaunchKernelGGL(k_take, dim3(blocks(k2, 256)), dim3(256), 0, st, cout[1], k2i, x_idx, x_a, state,
                           sel + k2, sel_out ? sel_out + k2 : nullptr, static_cast<uint8_t *>(nullptr));

    for (int o = 0; o < 2; ++o) {  // pos = (A minus sel1) or sel2;  neg = (A minus sel3) or sel4
        const uint8_t *rem = o == 0 ? rem1 : rem3;
        const uint32_t *add = sel + static_cast<int64_t>(o == 0 ? 1 : 3) * k2;
        hipLaunchKernelGGL(k_build_list, dim3(blocks(L.L, 256)), dim3(256), 0, st, x_idx, x_a, rem, state, T, add,
                           k2i, list_in);
        tb = L.temp_bytes;
        NGNN_REWIRE_HIP(sort_keys<uint32_t>(temp, tb, list_in, list_out, L.L, 32, st));
        hipLaunchKernelGGL(k_compact_out, dim3(1), dim3(1024), 0, st, list_out, static_cast<int>(L.L), ni,
                           o == 0 ? pos : neg, o == 0 ? pos_cap : neg_cap, counts + o, state, cn,
                           o == 0 ? counts + 2 : static_cast<int32_t *>(nullptr));
    }
#undef NGNN_REWIRE_HIP
    return launch_status();
}
