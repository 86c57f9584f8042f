// Symmetric-normalised GCN (PyG 2.5.1 gcn_norm + GCNConv [ext]): the degree
// pass and the weighted neighbour aggregate, fp32 (include/ngnn.h,
// "symmetric-normalised GCN").
//
//   k_gcn_norm  one thread per target row: the self-loop rewrite, the degree
//               in CSR order (loop weight last, fp64), dinv = 1 / sqrt(deg).
//   k_gcn_wagg  out[r] = bias + dinv[r] * (sum_e (w_e dinv[c_e]) z[c_e]
//                                          + (loop_w[r] dinv[r]) z[r]).
//
// Layout / MI355X mapping of k_gcn_wagg (the k_seg_agg_fwd layout of
// ngnn_agg.hip with a coefficient per entry)
//   * one group of LPR = next_pow2(F / VEC) lanes (4..64) owns one target
//     row: F = 256 is one wave per row (16-B loads), F = 40 sixteen lanes
//     (16-B), F = 47 a wave of 4-B loads, F = 16 four lanes (16-B), F = 10
//     eight lanes (8-B) -- no wave is mostly idle at the narrow widths a
//     transformed layer has; 256 / LPR rows per workgroup.
//   * lane k of the group loads col[beg + k], w[beg + k] and dinv[col] once,
//     forms the entry's coefficient and the group broadcasts both (__shfl);
//     the gathered rows are VEC-wide coalesced loads, four in flight per lane
//     before they are accumulated in entry order.
//   * a hub row stays on its group: the order of its sum is fixed, and its
//     time is its degree's (DESIGN.md 5n prices it).
//   * no LDS, no atomics, plain vector stores; every row offset is 64-bit.
#include <initializer_list>
#include <utility>

#include "ngnn_internal.h"

namespace ngnn {
namespace {

template <int VEC>
struct Vec;
template <>
struct Vec<4> {
    using T = float4;
};
template <>
struct Vec<2> {
    using T = float2;
};
template <>
struct Vec<1> {
    using T = float;
};

template <int VEC>
__device__ __forceinline__ float &comp(typename Vec<VEC>::T &v, int i) {
    return reinterpret_cast<float *>(&v)[i];
}

template <int VEC>
__device__ __forceinline__ typename Vec<VEC>::T ld(const float *p) {
    return *reinterpret_cast<const typename Vec<VEC>::T *>(p);
}

// acc += a * v, compensated (Kahan): the product enters exactly (fma), the
// rounding error of every addition is carried in `c` and taken off the next
// term.  A hub row adds thousands of terms, and a rewired or duplicated edge
// list adds many IDENTICAL ones, whose roundings all fall the same way: the
// plain sequential fp32 sum is then off by about deg * 2^-25 (1e-5 at a
// degree of 1,000, the whole fp32 bar); the compensated one stays at an ulp.
// Same fixed order, fp32 registers, a few VALU ops per element of a
// memory-bound kernel.  (-ffp-contract=off and no fast-math: the compiler
// keeps the sequence.)
template <int VEC>
__device__ __forceinline__ void fma_into(typename Vec<VEC>::T &acc, typename Vec<VEC>::T &c, float a,
                                         typename Vec<VEC>::T v) {
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
        const float s = comp<VEC>(acc, i);
        const float y = fmaf(a, comp<VEC>(v, i), -comp<VEC>(c, i));
        const float t = s + y;
        comp<VEC>(c, i) = (t - s) - y;
        comp<VEC>(acc, i) = t;
    }
}

__global__ __launch_bounds__(256) void k_gcn_norm(const int32_t *__restrict__ rowptr,
                                                  const int32_t *__restrict__ col,
                                                  const float *__restrict__ w, int n_rows, int loops,
                                                  float *__restrict__ dinv, float *__restrict__ loop_w) {
    const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= n_rows) return;
    const int beg = rowptr[row], end = rowptr[row + 1];
    // the degree in fp64 (a hub row's thousands of fp32 weights would cost
    // ulps of dinv in fp32; one thread per row, the adds are free)
    double deg = 0.0;
    float loop = 1.0f;
    if (!w && !loops) {
        deg = static_cast<double>(end - beg);
    } else {
        for (int e = beg; e < end; ++e) {
            const float we = w ? w[e] : 1.0f;
            if (loops && col[e] == row) {
                if (w) loop = we;  // the last self-loop entry's weight wins
            } else {
                deg += static_cast<double>(we);
            }
        }
    }
    if (loops) {
        deg += static_cast<double>(loop);
        loop_w[row] = loop;
    }
    // IEEE sqrt and divide in fp64, rounded once to fp32.  deg == 0: PyG's
    // masked_fill(inf, 0); deg < 0: sqrt gives NaN, as pow(-0.5)
    dinv[row] = deg == 0.0 ? 0.0f : static_cast<float>(1.0 / sqrt(deg));
}

template <int VEC, int LPR>
__global__ __launch_bounds__(256) void k_gcn_wagg(const float *__restrict__ z, int64_t ldz, int F,
                                                  const int32_t *__restrict__ rowptr,
                                                  const int32_t *__restrict__ col,
                                                  const float *__restrict__ w,
                                                  const float *__restrict__ dinv,
                                                  const float *__restrict__ loop_w,
                                                  const float *__restrict__ bias, int n_rows,
                                                  float *__restrict__ out, int64_t ldo) {
    using V = typename Vec<VEC>::T;
    constexpr int GROUPS = 256 / LPR;
    constexpr int UNR = 4;
    const int lane = threadIdx.x % LPR;
    const int64_t row = (int64_t)blockIdx.x * GROUPS + threadIdx.x / LPR;
    if (row >= n_rows) return;  // whole group leaves together
    const int beg = rowptr[row], end = rowptr[row + 1];
    const bool loops = loop_w != nullptr;
    const float dr = dinv ? dinv[row] : 1.0f;
    const int nchunks = (F + LPR * VEC - 1) / (LPR * VEC);
    for (int ch = 0; ch < nchunks; ++ch) {
        const int f = ch * LPR * VEC + lane * VEC;
        const bool act = f < F;
        V acc, cmp;
#pragma unroll
        for (int i = 0; i < VEC; ++i) comp<VEC>(acc, i) = comp<VEC>(cmp, i) = 0.0f;
        for (int eb = beg; eb < end; eb += LPR) {
            const int n = min(LPR, end - eb);
            // a replaced self-loop entry travels as ~col: its row is not added
            int myc = 0;
            float mya = 0.0f;
            if (lane < n) {
                const int c = col[eb + lane];
                mya = w ? w[eb + lane] : 1.0f;
                if (dinv) mya *= dinv[c];
                myc = (loops && c == row) ? ~c : c;
            }
            int k = 0;
            for (; k + UNR <= n; k += UNR) {
                int c[UNR];
                float a[UNR];
                V v[UNR];
#pragma unroll
                for (int u = 0; u < UNR; ++u) {
                    c[u] = __shfl(myc, k + u, LPR);
                    a[u] = __shfl(mya, k + u, LPR);
                }
                if (act) {
#pragma unroll
                    for (int u = 0; u < UNR; ++u)
                        v[u] = ld<VEC>(z + (int64_t)(c[u] < 0 ? ~c[u] : c[u]) * ldz + f);
#pragma unroll
                    for (int u = 0; u < UNR; ++u)
                        if (c[u] >= 0) fma_into<VEC>(acc, cmp, a[u], v[u]);
                }
            }
            for (; k < n; ++k) {
                const int c0 = __shfl(myc, k, LPR);
                const float a0 = __shfl(mya, k, LPR);
                if (act && c0 >= 0) fma_into<VEC>(acc, cmp, a0, ld<VEC>(z + (int64_t)c0 * ldz + f));
            }
        }
        if (!act) continue;
        if (loops) fma_into<VEC>(acc, cmp, loop_w[row] * dr, ld<VEC>(z + row * ldz + f));
        V o;
#pragma unroll
        for (int i = 0; i < VEC; ++i)
            comp<VEC>(o, i) = fmaf(dr, comp<VEC>(acc, i), bias ? bias[f + i] : 0.0f);
        *reinterpret_cast<V *>(out + row * ldo + f) = o;
    }
}

int pick_vec(int64_t F, std::initializer_list<std::pair<const void *, int64_t>> bufs) {
    for (int v : {4, 2}) {
        bool ok = (F % v) == 0;
        for (auto &b : bufs) ok = ok && aligned(b.first, 4 * v) && (b.second % v) == 0;
        if (ok) return v;
    }
    return 1;
}

template <int VEC>
void launch_wagg(int lpr, unsigned grid_rows, hipStream_t st, const float *z, int64_t ldz, int F,
                 const int32_t *rowptr, const int32_t *col, const float *w, const float *dinv,
                 const float *loop_w, const float *bias, int n_rows, float *out, int64_t ldo) {
    with_const<4, 8, 16, 32, 64>(lpr, [&](auto L) {
        constexpr int LPR = decltype(L)::value;
        const unsigned grid = static_cast<unsigned>(ceil_div(grid_rows, 256 / LPR));
        hipLaunchKernelGGL((k_gcn_wagg<VEC, LPR>), dim3(grid), dim3(256), 0, st, z, ldz, F, rowptr, col,
                           w, dinv, loop_w, bias, n_rows, out, ldo);
    });
}

}  // namespace
}  // namespace ngnn

using namespace ngnn;

extern "C" int ngnn_gcn_norm(const int32_t *rowptr, const int32_t *col, const float *w, int64_t n_rows,
                             int add_self_loops, float *dinv, float *loop_w, void *stream) {
    NGNN_RETURN_IF(n_rows < 0 || !rowptr || !dinv, NGNN_E_ARG);
    NGNN_RETURN_IF(add_self_loops && !loop_w && n_rows > 0, NGNN_E_ARG);
    NGNN_RETURN_IF(!fits_i32(n_rows), NGNN_E_RANGE);
    if (n_rows == 0) return NGNN_OK;
    // col may be NULL when the CSR has no entries (rowptr is all zeros then)
    const unsigned grid = static_cast<unsigned>(ceil_div(n_rows, 256));
    hipLaunchKernelGGL(k_gcn_norm, dim3(grid), dim3(256), 0, as_stream(stream), rowptr, col, w,
                       (int)n_rows, add_self_loops ? 1 : 0, dinv, loop_w);
    return launch_status();
}

extern "C" int ngnn_gcn_wagg(const float *z, int64_t ldz, int64_t F, const int32_t *rowptr,
                             const int32_t *col, const float *w, const float *dinv, const float *loop_w,
                             const float *bias, int64_t n_rows, float *out, int64_t ldo, void *stream) {
    NGNN_RETURN_IF(n_rows < 0 || F < 0 || !rowptr, NGNN_E_ARG);
    NGNN_RETURN_IF(ldz < F || ldo < F, NGNN_E_SHAPE);
    NGNN_RETURN_IF(!fits_i32(n_rows) || !fits_i32(F), NGNN_E_RANGE);
    if (n_rows == 0 || F == 0) return NGNN_OK;
    NGNN_RETURN_IF(!z || !out, NGNN_E_ARG);
    const int vec = pick_vec(F, {{z, ldz}, {out, ldo}});  // (bias is read by element)
    const int64_t chunks = ceil_div(F, vec);
    int lpr = 4;
    while (lpr < 64 && lpr < chunks) lpr <<= 1;
    hipStream_t st = as_stream(stream);
    with_const<4, 2, 1>(vec, [&](auto Vc) {
        launch_wagg<decltype(Vc)::value>(lpr, (unsigned)n_rows, st, z, ldz, (int)F, rowptr, col, w, dinv,
                                         loop_w, bias, (int)n_rows, out, ldo);
    });
    return launch_status();
}
