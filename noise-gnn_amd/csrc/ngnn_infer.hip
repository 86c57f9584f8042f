// Layer-wise inference without blocks (ABI 22).
//
// SAGE.inference / SimpleGCN.inference (sage.py:42-58, convolution.py:37-53)
// evaluate one layer at a time over every node: per loader batch the conv runs
// on a full multi-hop block and only the seed rows are kept.  Under the
// sampler's contract (ngnn_sample.hip) a seed row receives in-edges from hop 0
// only, and hop 0's draws are a pure function of (batch seed, position in the
// batch, degree).  So the rows a whole-graph pass keeps need no block: loader
// position p draws straight from the graph CSR with the batch's hop-0 seed,
// and the layer reads the previous layer's table by global node id.
//
//   ngnn_infer_draw    the draws of a run of loader positions as a
//                      target-grouped CSR of global ids (feeds the row-tile
//                      layer kernel's fused gather: wide layers)
//   ngnn_infer_narrow  the draws made in the kernel, the neighbour term
//                      gathered F_out wide from z = x W_l^T (narrowing layers)
#include <algorithm>
#include <type_traits>

#include "ngnn_internal.h"
#include "ngnn_sample_dev.h"

namespace ngnn {
namespace {

constexpr int kIdTile = 1024;  // rows per scan tile

// the loader positions [r0, r0 + n_rows) of one pass
struct InferRows {
    const int64_t *g_rowptr;
    const int32_t *g_col;
    const int64_t *seeds;  // nullable: position p is node p
    int64_t r0, n_rows, batch_size;
    int fanout;
    uint64_t seed0, seed_stride;
};

// position p's node, its CSR row start and in-degree
__device__ __forceinline__ void infer_row(const InferRows &R, int64_t row, int64_t &beg, int64_t &deg,
                                          uint64_t &hseed, int &i) {
    const int64_t p = R.r0 + row;
    const int64_t b = p / R.batch_size;
    i = static_cast<int>(p - b * R.batch_size);
    const int64_t v = R.seeds ? R.seeds[p] : p;
    beg = R.g_rowptr[v];
    deg = R.g_rowptr[v + 1] - beg;
    // block seed S_b = seed0 + b * stride (wraps as ngnn_sample_block's caller's does), hop 0
    hseed = hop_seed(R.seed0 + static_cast<uint64_t>(b) * R.seed_stride, 0);
}

// Draw j of chunk row `row` by its KF-lane group: the neighbour's global id
// for j < k, k = min(deg, fanout).  Rows past the chunk draw nothing (k = 0)
// but keep their lanes in step with the group shuffles of the wave's others.
template <int KF>
__device__ __forceinline__ int32_t infer_draw_lane(const InferRows &R, int64_t row, int j, int &k) {
    const bool valid = row < R.n_rows;
    int64_t beg, deg;
    uint64_t hseed;
    int i;
    infer_row(R, valid ? row : 0, beg, deg, hseed, i);
    if (!valid) deg = 0;
    const int s = floyd_lane<KF>(deg, R.fanout, hseed, i, j, k);
    return j < k ? R.g_col[beg + s] : -1;
}

// rowptr[r] = exclusive prefix of min(deg, fanout) INSIDE the row's tile,
// tsum[tile] = the tile's total
__global__ __launch_bounds__(kIdTile) void k_id_count(InferRows R, int32_t *__restrict__ rowptr,
                                                      int32_t *__restrict__ tsum) {
    __shared__ int s_w[kIdTile / 64];
    const int64_t row = static_cast<int64_t>(blockIdx.x) * kIdTile + threadIdx.x;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int cnt = 0;
    if (row < R.n_rows) {
        int64_t beg, deg;
        uint64_t hs;
        int i;
        infer_row(R, row, beg, deg, hs, i);
        cnt = deg < R.fanout ? static_cast<int>(deg) : R.fanout;
    }
    int inc = cnt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int a = __shfl_up(inc, o);
        if (lane >= o) inc += a;
    }
    if (lane == 63) s_w[wv] = inc;
    __syncthreads();
    int base = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kIdTile / 64; ++w) {
        base += w < wv ? s_w[w] : 0;
        total += s_w[w];
    }
    if (row < R.n_rows) rowptr[row] = base + inc - cnt;
    if (threadIdx.x == 0) tsum[blockIdx.x] = total;
}

// tsum -> its exclusive prefix, in place (one workgroup, kIdTile tiles a round)
__global__ __launch_bounds__(kIdTile) void k_id_scan(int32_t *__restrict__ tsum, int n_tiles) {
    __shared__ int s_w[kIdTile / 64];
    __shared__ int s_carry;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (threadIdx.x == 0) s_carry = 0;
    __syncthreads();
    for (int t0 = 0; t0 < n_tiles; t0 += kIdTile) {
        const int t = t0 + static_cast<int>(threadIdx.x);
        const int v = t < n_tiles ? tsum[t] : 0;
        int inc = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int a = __shfl_up(inc, o);
            if (lane >= o) inc += a;
        }
        if (lane == 63) s_w[wv] = inc;
        __syncthreads();
        int base = s_carry, total = 0;
#pragma unroll
        for (int w = 0; w < kIdTile / 64; ++w) {
            base += w < wv ? s_w[w] : 0;
            total += s_w[w];
        }
        if (t < n_tiles) tsum[t] = base + inc - v;
        __syncthreads();  // (every thread has read s_carry and s_w)
        if (threadIdx.x == 0) s_carry += total;
        __syncthreads();
    }
}

// one KF-lane group per row (k_sb_sample's layout): draw j -> col[rowptr[row] + j]
template <int KF>
__global__ __launch_bounds__(256) void k_id_draw(InferRows R, int32_t *__restrict__ rowptr,
                                                 const int32_t *__restrict__ tsum,
                                                 int32_t *__restrict__ col) {
    const int64_t gt = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    const int64_t row = gt / KF;
    const int j = static_cast<int>(gt % KF);
    if (row >= R.n_rows) return;  // (whole groups)
    int k;
    const int32_t u = infer_draw_lane<KF>(R, row, j, k);
    // (lane 0 alone reads the row's tile-local prefix, then replaces it)
    int off = j == 0 ? rowptr[row] + tsum[row / kIdTile] : 0;
    off = __shfl(off, 0, KF);
    if (j < k) col[off + j] = u;
    if (j == 0) {
        rowptr[row] = off;
        if (row == R.n_rows - 1) rowptr[R.n_rows] = off + k;
    }
}

// out[r] = act(root[r] + red_j z[nbr_j(r)] + bias): memory-bound.  A wave
// draws 64 / KF rows at once (one KF-lane group each), then takes them one
// at a time: lane (sub, cq) = (lane / 16, lane % 16) loads the 16-B column
// quad cq of neighbours sub, sub + 4, ... -- four neighbour rows per wave
// load instruction, every load of a row issued before the first sum -- and the
// pieces are then summed in draw order through shuffles (a fixed order, the
// reference's).  Slots past the row's count in a live step load the row's
// first neighbour again and are never summed.
template <int KF, bool MEAN>
__global__ __launch_bounds__(256) void k_infer_narrow(InferRows R, const float *__restrict__ z, int64_t ldz,
                                                      const float *__restrict__ root, int64_t ldr,
                                                      const float *__restrict__ bias, int Fo, int relu,
                                                      float *__restrict__ out, int64_t ldo, int vec_out) {
    constexpr int RPW = 64 / KF;  // rows per wave
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t rbase = (static_cast<int64_t>(blockIdx.x) * 4 + wv) * RPW;
    if (rbase >= R.n_rows) return;  // (whole waves)
    int k;
    const int32_t u = infer_draw_lane<KF>(R, rbase + lane / KF, lane % KF, k);
    const int cq = lane & 15, sub = lane >> 4;
    const int Fo4 = (Fo + 3) >> 2;
#pragma unroll 1
    for (int gg = 0; gg < RPW; ++gg) {
        const int64_t rr = rbase + gg;
        if (rr >= R.n_rows) break;
        const int kk = __shfl(k, gg * KF);
        const int32_t u0 = __shfl(u, gg * KF);  // (read only when kk > 0)
#pragma unroll 1
        for (int c0 = 0; c0 < Fo4; c0 += 16) {
            const bool live = c0 + cq < Fo4;
            const int c = live ? c0 + cq : Fo4 - 1;
            // (steps of four neighbours; a step past the count is skipped by
            // the whole wave; every load issues before the first sum)
            float4 v[KF / 4];
#pragma unroll
            for (int s = 0; s < KF / 4; ++s) {
                const int q = 4 * s + sub;
                const int32_t uq = __shfl(u, gg * KF + q);
                const int64_t src = q < kk ? uq : u0;
                v[s] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (4 * s < kk) v[s] = *reinterpret_cast<const float4 *>(z + src * ldz + 4 * c);
            }
            // the row's sum in draw order -- the edge order of the loader's
            // block, so the fp32 sequence of ngnn_seg_agg_fwd and of the
            // reference's scatter_add_: draw q sits in step q / 4 of lane
            // group q % 4 (every lane sums, the first group stores)
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int q = 0; q < KF; ++q) {
                if (q < kk) {  // (the whole wave together)
                    const int from = cq + 16 * (q & 3);
                    acc.x += __shfl(v[q >> 2].x, from);
                    acc.y += __shfl(v[q >> 2].y, from);
                    acc.z += __shfl(v[q >> 2].z, from);
                    acc.w += __shfl(v[q >> 2].w, from);
                }
            }
            if (sub != 0 || !live) continue;
            if (MEAN && kk > 0) {  // IEEE division, as ngnn_seg_agg_fwd's mean
                const float dk = static_cast<float>(kk);
                acc.x /= dk;
                acc.y /= dk;
                acc.z /= dk;
                acc.w /= dk;
            }
            float a[4] = {acc.x, acc.y, acc.z, acc.w};
            if (root) {  // (rows of at least ceil4(Fo) floats, 16-B aligned: checked by the caller)
                const float4 rt = *reinterpret_cast<const float4 *>(root + rr * ldr + 4 * c);
                a[0] = rt.x + a[0];
                a[1] = rt.y + a[1];
                a[2] = rt.z + a[2];
                a[3] = rt.w + a[3];
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (bias && 4 * c + e < Fo) a[e] += bias[4 * c + e];
                if (relu) a[e] = a[e] > 0.f ? a[e] : (a[e] != a[e] ? a[e] : 0.f);  // (NaN kept, as torch.relu)
            }
            float *o = out + rr * ldo + 4 * c;
            if (vec_out) {
                *reinterpret_cast<float4 *>(o) = make_float4(a[0], a[1], a[2], a[3]);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (4 * c + e < Fo) o[e] = a[e];
            }
        }
    }
}

// the checks both entries share; 0 = go on
int infer_rows_check(int64_t r0, int64_t n_rows, int64_t batch_size, int fanout) {
    NGNN_RETURN_IF(n_rows < 0 || r0 < 0 || batch_size <= 0 || fanout < 0, NGNN_E_ARG);
    NGNN_RETURN_IF(r0 % batch_size != 0, NGNN_E_ARG);
    NGNN_RETURN_IF(fanout > kMaxFanout, NGNN_E_SHAPE);
    // (32-bit edge offsets; lane indices of the draw grid are 64-bit)
    NGNN_RETURN_IF(n_rows > INT32_MAX || n_rows * std::max(fanout, 1) >= (int64_t(1) << 31), NGNN_E_RANGE);
    return NGNN_OK;
}

}  // namespace
}  // namespace ngnn

using namespace ngnn;

extern "C" size_t ngnn_infer_draw_workspace_bytes(int64_t n_rows) {
    if (n_rows < 0) return 0;
    return static_cast<size_t>(std::max<int64_t>(1, ceil_div(n_rows, kIdTile))) * sizeof(int32_t);
}

extern "C" int ngnn_infer_draw(const int64_t *g_rowptr, const int32_t *g_col, const int64_t *seeds,
                               int64_t r0, int64_t n_rows, int64_t batch_size, int fanout,
                               uint64_t seed0, uint64_t seed_stride, int32_t *rowptr, int32_t *col,
                               void *ws, size_t ws_bytes, void *stream) {
    const int rc = infer_rows_check(r0, n_rows, batch_size, fanout);
    if (rc) return rc;
    NGNN_RETURN_IF(!rowptr, NGNN_E_ARG);
    NGNN_RETURN_IF(n_rows > 0 && (!g_rowptr || !ws || (fanout > 0 && (!g_col || !col))), NGNN_E_ARG);
    NGNN_RETURN_IF(n_rows > 0 && (ws_bytes < ngnn_infer_draw_workspace_bytes(n_rows) || !aligned(ws, 4)),
                   NGNN_E_WORKSPACE);
    hipStream_t st = as_stream(stream);
    if (n_rows == 0) {  // rowptr[0] = 0
        const hipError_t e = hipMemsetAsync(rowptr, 0, sizeof(int32_t), st);
        return e == hipSuccess ? NGNN_OK : static_cast<int>(e);
    }
    const InferRows R{g_rowptr, g_col, seeds, r0, n_rows, batch_size, fanout, seed0, seed_stride};
    int32_t *tsum = static_cast<int32_t *>(ws);
    const int n_tiles = static_cast<int>(ceil_div(n_rows, kIdTile));
    hipLaunchKernelGGL(k_id_count, dim3(n_tiles), dim3(kIdTile), 0, st, R, rowptr, tsum);
    hipLaunchKernelGGL(k_id_scan, dim3(1), dim3(kIdTile), 0, st, tsum, n_tiles);
    const int kf = sb_kf(fanout);
    const unsigned grid = static_cast<unsigned>(ceil_div(n_rows * kf, 256));
    switch (kf) {
        case 8: hipLaunchKernelGGL(k_id_draw<8>, dim3(grid), dim3(256), 0, st, R, rowptr, tsum, col); break;
        case 16: hipLaunchKernelGGL(k_id_draw<16>, dim3(grid), dim3(256), 0, st, R, rowptr, tsum, col); break;
        case 32: hipLaunchKernelGGL(k_id_draw<32>, dim3(grid), dim3(256), 0, st, R, rowptr, tsum, col); break;
        default: hipLaunchKernelGGL(k_id_draw<64>, dim3(grid), dim3(256), 0, st, R, rowptr, tsum, col); break;
    }
    return launch_status();
}

extern "C" int ngnn_infer_narrow(const int64_t *g_rowptr, const int32_t *g_col, const int64_t *seeds,
                                 int64_t r0, int64_t n_rows, int64_t batch_size, int fanout,
                                 uint64_t seed0, uint64_t seed_stride, const float *z, int64_t ldz,
                                 const float *root, int64_t ld_root, const float *bias, int64_t Fo,
                                 int reduce, int relu, float *out, int64_t ldo, void *stream) {
    const int rc = infer_rows_check(r0, n_rows, batch_size, fanout);
    if (rc) return rc;
    NGNN_RETURN_IF(reduce != NGNN_REDUCE_SUM && reduce != NGNN_REDUCE_MEAN, NGNN_E_ARG);
    NGNN_RETURN_IF(Fo <= 0, NGNN_E_ARG);
    NGNN_RETURN_IF(!fits_i32(Fo), NGNN_E_RANGE);
    const int64_t Fo4 = ceil_div(Fo, 4) * 4;
    NGNN_RETURN_IF(ldz < Fo4 || ldz % 4 != 0 || ldo < Fo, NGNN_E_SHAPE);
    NGNN_RETURN_IF(root && (ld_root < Fo4 || ld_root % 4 != 0), NGNN_E_SHAPE);
    if (n_rows == 0) return NGNN_OK;
    NGNN_RETURN_IF(!g_rowptr || !z || !out || (fanout > 0 && !g_col), NGNN_E_ARG);
    NGNN_RETURN_IF(!aligned(z, 16) || (root && !aligned(root, 16)), NGNN_E_ALIGN);
    const InferRows R{g_rowptr, g_col, seeds, r0, n_rows, batch_size, fanout, seed0, seed_stride};
    const int vec_out = Fo % 4 == 0 && ldo % 4 == 0 && aligned(out, 16);
    const int kf = sb_kf(fanout);
    const unsigned grid = static_cast<unsigned>(ceil_div(n_rows, 4 * (64 / kf)));
    hipStream_t st = as_stream(stream);
    auto go = [&](auto kf_c, auto mean_c) {
        hipLaunchKernelGGL((k_infer_narrow<decltype(kf_c)::value, decltype(mean_c)::value>), dim3(grid), dim3(256), 0,
                           st, R, z, ldz, root, ld_root, bias, static_cast<int>(Fo), relu, out, ldo, vec_out);
    };
    auto by_kf = [&](auto mean_c) {
        switch (kf) {
            case 8: go(std::integral_constant<int, 8>{}, mean_c); break;
            case 16: go(std::integral_constant<int, 16>{}, mean_c); break;
            case 32: go(std::integral_constant<int, 32>{}, mean_c); break;
            default: go(std::integral_constant<int, 64>{}, mean_c); break;
        }
    };
    if (reduce == NGNN_REDUCE_MEAN) by_kf(std::true_type{});
    else by_kf(std::false_type{});
    return launch_status();
}
