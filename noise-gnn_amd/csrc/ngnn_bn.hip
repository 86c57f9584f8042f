// Fused ReLU - BatchNorm1d - dropout over [n_rows, F] fp32 rows (include/ngnn.h,
// "fused ReLU-BatchNorm-dropout").
//
//   training forward   k_bn_stats        per-slab (mean, M2) of every column
//                      k_bn_stats_final  Chan merge of the slabs in a fixed
//                                        order: mean, invstd, running statistics
//                      k_bn_apply        out = drop(gamma (a - mean) invstd + beta)
//   eval forward       k_bn_apply<EVAL>  the same epilogue on the running statistics
//   backward           k_bn_bwd_sums     per-slab sums of g and g xhat
//                      k_bn_bwd_final    dbeta, dgamma
//                      k_bn_bwd_dx       dx (skipped when dx == NULL)
//
// Layout / MI355X mapping
//   * a 256-thread workgroup owns one slab of kSlab = 256 rows by one column
//     tile of LPR * VEC columns: LPR = 16, 32 or 64 consecutive lanes take
//     consecutive column groups of VEC = 4 (16-B loads; F, every leading
//     dimension and base permitting) or 1, so row reads coalesce; the 256 / LPR
//     lane groups take the slab's rows round robin.
//   * the column statistics never form E[a^2] - E[a]^2: a thread loads eight
//     rows (eight independent loads in flight), takes their mean and the
//     squared deviations AROUND that mean, and merges the chunk into its
//     running (count, mean, M2) by Chan's formula.  Chunks, lane groups
//     (through LDS), slabs and the sixteen slab lanes of the finalise kernel
//     are merged in one fixed order, in fp64 registers (the kernels are
//     HBM-bound: fp64 adds are free, and mean / invstd come out rounded once).
//     Counts are never stored: they follow from the indices.
//   * no atomics, plain vector stores, every loop bounded by its arguments,
//     row offsets 64-bit; nothing branches on a value, so a NaN stays in its
//     column.
#include <initializer_list>
#include <utility>

#include "ngnn_device.h"
#include "ngnn_internal.h"

namespace ngnn {
namespace {

constexpr int kSlab = 256;     // rows per partial (ngnn_bn_slab_rows)
constexpr int kThreads = 256;  // workgroup of the slab kernels
constexpr int kChunk = 8;      // rows a thread holds at once
constexpr int kFinLanes = 16;  // slab lanes of the finalise kernels (x 64 columns)

template <int VEC>
struct Vec;
template <>
struct Vec<4> {
    using T = float4;
};
template <>
struct Vec<1> {
    using T = float;
};

template <int VEC>
__device__ __forceinline__ float &comp(typename Vec<VEC>::T &v, int i) {
    return reinterpret_cast<float *>(&v)[i];
}

// torch's relu: a NaN stays a NaN (fmaxf would drop it)
__device__ __forceinline__ float act_of(float x, int relu) { return (relu && x < 0.0f) ? 0.0f : x; }

// Where a thread of a slab kernel works: columns c .. c + VEC - 1 (c >= F: an
// idle lane) and rows r0, r0 + rstep, ... below rend.
template <int VEC>
struct Place {
    int c, rsub, rstep, slab0, rend;
    __device__ __forceinline__ Place(int lpr, int n_rows) {
        const int lane = threadIdx.x & (lpr - 1);  // lpr: a power of two
        rsub = threadIdx.x / lpr;
        rstep = kThreads / lpr;
        c = (blockIdx.y * lpr + lane) * VEC;
        slab0 = blockIdx.x * kSlab;
        rend = min(slab0 + kSlab, n_rows);
    }
    // rows of lane group j in this slab
    __device__ __forceinline__ int count(int j) const {
        const int rows = rend - slab0;
        return j < rows ? (rows - j + rstep - 1) / rstep : 0;
    }
};

// Chan's merge of (nb, mb, qb) into (na, ma, qa); counts as doubles, nb > 0
__device__ __forceinline__ void chan_merge(double na, double &ma, double &qa, double nb, double mb, double qb) {
    const double w = nb / (na + nb);
    const double d = mb - ma;
    ma += d * w;
    qa += qb + d * d * (na * w);
}

// ---------------------------------------------------------------- forward

// part[(slab * 2 + 0) * F + c] = the slab's mean of column c, [.. + 1] its M2
template <int VEC>
__global__ __launch_bounds__(kThreads) void k_bn_stats(const float *__restrict__ x, int64_t ldx, int n_rows,
                                                       int F, int lpr, int relu, double *__restrict__ part) {
    using V = typename Vec<VEC>::T;
    __shared__ double s_m[VEC][kThreads], s_q[VEC][kThreads];
    const Place<VEC> p(lpr, n_rows);
    const bool act = p.c < F;
    double m[VEC], q[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) m[i] = q[i] = 0.0;
    if (act) {
        const float *xp = x + p.c;
        int cnt = 0;
        for (int r = p.slab0 + p.rsub; r < p.rend; r += kChunk * p.rstep) {
            const int nb = min(kChunk, (p.rend - r + p.rstep - 1) / p.rstep);
            // rows past the chunk's end re-read its last row (in bounds) and are not used
            V v[kChunk];
#pragma unroll
            for (int u = 0; u < kChunk; ++u)
                v[u] = *reinterpret_cast<const V *>(xp + (int64_t)(r + min(u, nb - 1) * p.rstep) * ldx);
            const double w = (double)nb / (double)(cnt + nb);
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
                double a[kChunk], s = 0.0;
#pragma unroll
                for (int u = 0; u < kChunk; ++u) {
                    a[u] = (double)act_of(comp<VEC>(v[u], i), relu);
                    if (u < nb) s += a[u];
                }
                const double mb = nb == kChunk ? s * (1.0 / kChunk) : s / (double)nb;
                double qb = 0.0;
#pragma unroll
                for (int u = 0; u < kChunk; ++u) {
                    const double d = a[u] - mb;
                    if (u < nb) qb += d * d;
                }
                const double d = mb - m[i];
                m[i] += d * w;
                q[i] += qb + d * d * ((double)cnt * w);
            }
            cnt += nb;
        }
    }
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
        s_m[i][threadIdx.x] = m[i];
        s_q[i][threadIdx.x] = q[i];
    }
    __syncthreads();
    if (!act || p.rsub != 0) return;
    // the lane groups in ascending order (group 0 holds row slab0: never empty)
    double na = (double)p.count(0);
    for (int j = 1; j < p.rstep; ++j) {
        const int nb = p.count(j);
        if (nb == 0) break;
#pragma unroll
        for (int i = 0; i < VEC; ++i)
            chan_merge(na, m[i], q[i], (double)nb, s_m[i][j * lpr + threadIdx.x], s_q[i][j * lpr + threadIdx.x]);
        na += (double)nb;
    }
    double *pm = part + (int64_t)blockIdx.x * 2 * F + p.c;
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
        pm[i] = m[i];
        pm[F + i] = q[i];
    }
}

// one lane per column, kFinLanes slab lanes: lane j merges slabs j, j + 16, ...
// in ascending order, then lane 0 merges the sixteen in ascending order
__global__ __launch_bounds__(64 * kFinLanes) void k_bn_stats_final(
    const double *__restrict__ part, int nslabs, int n_rows, int F, double eps, double momentum,
    const int64_t *__restrict__ nbt, float *__restrict__ mean, float *__restrict__ mean_lo,
    float *__restrict__ invstd, float *__restrict__ rmean, float *__restrict__ rvar) {
    __shared__ double s_n[kFinLanes][64], s_m[kFinLanes][64], s_q[kFinLanes][64];
    const int lane = threadIdx.x & 63, j = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane;
    double n = 0.0, m = 0.0, q = 0.0;
    if (c < F) {
#pragma unroll 4
        for (int s = j; s < nslabs; s += kFinLanes) {
            const double nb = (double)min(kSlab, n_rows - s * kSlab);
            const double *ps = part + (int64_t)s * 2 * F + c;
            chan_merge(n, m, q, nb, ps[0], ps[F]);
            n += nb;
        }
    }
    s_n[j][lane] = n;
    s_m[j][lane] = m;
    s_q[j][lane] = q;
    __syncthreads();
    if (j != 0 || c >= F) return;
    for (int k = 1; k < kFinLanes; ++k) {
        const double nb = s_n[k][lane];
        if (nb == 0.0) break;  // (a count: slab lanes past nslabs are empty)
        chan_merge(n, m, q, nb, s_m[k][lane], s_q[k][lane]);
        n += nb;
    }
    // n == n_rows >= 2.  nn.BatchNorm1d: the biased variance normalises, the
    // unbiased one is tracked; momentum < 0 is the cumulative average
    const double var = q / n;
    // the mean as an fp32 pair: fp32 alone holds a mean of 4096 to 2.4e-4, which
    // would be the error of every output of that column
    const float mh = (float)m;
    mean[c] = mh;
    mean_lo[c] = (float)(m - (double)mh);
    invstd[c] = (float)(1.0 / sqrt(var + eps));
    const double mo = momentum < 0.0 ? 1.0 / (double)(*nbt + 1) : momentum;
    rmean[c] = (float)((1.0 - mo) * (double)rmean[c] + mo * m);
    rvar[c] = (float)((1.0 - mo) * (double)rvar[c] + mo * (q / (n - 1.0)));
}

// out = drop(gamma * (a - mean) * invstd + beta).  EVAL: the statistics are the
// running ones (stat1 = running_var), no dropout, nothing updated.  Training:
// thread 0 of workgroup (0, 0) counts the batch (k_bn_stats_final has read the
// old count by then).
template <int VEC, int EVAL>
__global__ __launch_bounds__(kThreads) void k_bn_apply(const float *__restrict__ x, int64_t ldx, int n_rows, int F,
                                                       int lpr, int relu, const float *__restrict__ stat0,
                                                       const float *__restrict__ stat0_lo,
                                                       const float *__restrict__ stat1,
                                                       const float *__restrict__ gamma,
                                                       const float *__restrict__ beta, double eps, Dropout drop,
                                                       const uint64_t *__restrict__ seed_dev,
                                                       float *__restrict__ out, int64_t ldo,
                                                       int64_t *__restrict__ nbt) {
    using V = typename Vec<VEC>::T;
    if (!EVAL && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *nbt += 1;
    const Place<VEC> p(lpr, n_rows);
    if (p.c >= F) return;
    if (!EVAL && seed_dev) drop.reseed(*seed_dev);
    float mu[VEC], lo[VEC], is[VEC], ga[VEC], be[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
        mu[i] = stat0[p.c + i];
        lo[i] = EVAL ? 0.0f : stat0_lo[p.c + i];
        is[i] = EVAL ? (float)(1.0 / sqrt((double)stat1[p.c + i] + eps)) : stat1[p.c + i];
        ga[i] = gamma[p.c + i];
        be[i] = beta[p.c + i];
    }
    const int cnt = p.count(p.rsub);
    const float *xp = x + (int64_t)(p.slab0 + p.rsub) * ldx + p.c;
    float *op = out + (int64_t)(p.slab0 + p.rsub) * ldo + p.c;
    const int64_t sx = (int64_t)p.rstep * ldx, so = (int64_t)p.rstep * ldo;
#pragma unroll 4
    for (int k = 0; k < cnt; ++k) {
        V v = *reinterpret_cast<const V *>(xp + k * sx);
        uint32_t keep = 0xfu;
        if (!EVAL && drop.thresh) {
            const uint32_t rk = drop.row_key((uint32_t)(p.slab0 + p.rsub + k * p.rstep));
            keep = VEC == 4 ? drop.keep4(rk, (uint32_t)p.c >> 2) : (drop.keep(rk, (uint32_t)p.c) ? 1u : 0u);
        }
        V o;
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            const float xh = ((act_of(comp<VEC>(v, i), relu) - mu[i]) - lo[i]) * is[i];
            const float y = xh * ga[i] + be[i];
            comp<VEC>(o, i) = ((keep >> i) & 1u) ? y * drop.scale : 0.0f;
        }
        *reinterpret_cast<V *>(op + k * so) = o;
    }
}

// ---------------------------------------------------------------- backward

// part[(slab * 2 + 0) * F + c] = the slab's sum of g, [.. + 1] of g * xhat,
// g = dout * keep * scale, xhat = (a - mean) * invstd as the forward formed it
template <int VEC>
__global__ __launch_bounds__(kThreads) void k_bn_bwd_sums(const float *__restrict__ dout, int64_t ldg,
                                                          const float *__restrict__ x, int64_t ldx, int n_rows,
                                                          int F, int lpr, int relu,
                                                          const float *__restrict__ mean,
                                                          const float *__restrict__ mean_lo,
                                                          const float *__restrict__ invstd, Dropout drop,
                                                          const uint64_t *__restrict__ seed_dev,
                                                          double *__restrict__ part) {
    using V = typename Vec<VEC>::T;
    __shared__ double s_b[VEC][kThreads], s_g[VEC][kThreads];
    const Place<VEC> p(lpr, n_rows);
    const bool act = p.c < F;
    double sb[VEC], sg[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) sb[i] = sg[i] = 0.0;
    if (act) {
        if (seed_dev) drop.reseed(*seed_dev);
        float mu[VEC], lo[VEC], is[VEC];
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            mu[i] = mean[p.c + i];
            lo[i] = mean_lo[p.c + i];
            is[i] = invstd[p.c + i];
        }
        const int cnt = p.count(p.rsub);
        const float *xp = x + (int64_t)(p.slab0 + p.rsub) * ldx + p.c;
        const float *gp = dout + (int64_t)(p.slab0 + p.rsub) * ldg + p.c;
        const int64_t sx = (int64_t)p.rstep * ldx, sgr = (int64_t)p.rstep * ldg;
#pragma unroll 4
        for (int k = 0; k < cnt; ++k) {
            V v = *reinterpret_cast<const V *>(xp + k * sx);
            V d = *reinterpret_cast<const V *>(gp + k * sgr);
            uint32_t keep = 0xfu;
            if (drop.thresh) {
                const uint32_t rk = drop.row_key((uint32_t)(p.slab0 + p.rsub + k * p.rstep));
                keep = VEC == 4 ? drop.keep4(rk, (uint32_t)p.c >> 2) : (drop.keep(rk, (uint32_t)p.c) ? 1u : 0u);
            }
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
                const float xh = ((act_of(comp<VEC>(v, i), relu) - mu[i]) - lo[i]) * is[i];
                const float g = ((keep >> i) & 1u) ? comp<VEC>(d, i) * drop.scale : 0.0f;
                sb[i] += (double)g;
                sg[i] += (double)g * (double)xh;
            }
        }
    }
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
        s_b[i][threadIdx.x] = sb[i];
        s_g[i][threadIdx.x] = sg[i];
    }
    __syncthreads();
    if (!act || p.rsub != 0) return;
    for (int j = 1; j < p.rstep; ++j) {  // (an empty lane group stored zeros)
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            sb[i] += s_b[i][j * lpr + threadIdx.x];
            sg[i] += s_g[i][j * lpr + threadIdx.x];
        }
    }
    double *pb = part + (int64_t)blockIdx.x * 2 * F + p.c;
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
        pb[i] = sb[i];
        pb[F + i] = sg[i];
    }
}

__global__ __launch_bounds__(64 * kFinLanes) void k_bn_bwd_final(const double *__restrict__ part, int nslabs, int F,
                                                                 float *__restrict__ dgamma,
                                                                 float *__restrict__ dbeta) {
    __shared__ double s_b[kFinLanes][64], s_g[kFinLanes][64];
    const int lane = threadIdx.x & 63, j = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane;
    double sb = 0.0, sg = 0.0;
    if (c < F) {
#pragma unroll 4
        for (int s = j; s < nslabs; s += kFinLanes) {
            const double *ps = part + (int64_t)s * 2 * F + c;
            sb += ps[0];
            sg += ps[F];
        }
    }
    s_b[j][lane] = sb;
    s_g[j][lane] = sg;
    __syncthreads();
    if (j != 0 || c >= F) return;
    for (int k = 1; k < kFinLanes; ++k) {
        sb += s_b[k][lane];
        sg += s_g[k][lane];
    }
    dbeta[c] = (float)sb;
    dgamma[c] = (float)sg;
}

// dx = [relu: x > 0] gamma invstd (g - dbeta / n - xhat dgamma / n); a NaN x
// passes the gate, as torch's threshold_backward lets it
template <int VEC>
__global__ __launch_bounds__(kThreads) void k_bn_bwd_dx(const float *__restrict__ dout, int64_t ldg,
                                                        const float *__restrict__ x, int64_t ldx, int n_rows,
                                                        int F, int lpr, int relu, const float *__restrict__ mean,
                                                        const float *__restrict__ mean_lo,
                                                        const float *__restrict__ invstd,
                                                        const float *__restrict__ gamma,
                                                        const float *__restrict__ dgamma,
                                                        const float *__restrict__ dbeta, Dropout drop,
                                                        const uint64_t *__restrict__ seed_dev,
                                                        float *__restrict__ dx, int64_t ldd) {
    using V = typename Vec<VEC>::T;
    const Place<VEC> p(lpr, n_rows);
    if (p.c >= F) return;
    if (seed_dev) drop.reseed(*seed_dev);
    const float n = (float)n_rows;
    float mu[VEC], lo[VEC], is[VEC], gi[VEC], cb[VEC], cg[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
        mu[i] = mean[p.c + i];
        lo[i] = mean_lo[p.c + i];
        is[i] = invstd[p.c + i];
        gi[i] = gamma[p.c + i] * is[i];
        cb[i] = dbeta[p.c + i] / n;
        cg[i] = dgamma[p.c + i] / n;
    }
    const int cnt = p.count(p.rsub);
    const float *xp = x + (int64_t)(p.slab0 + p.rsub) * ldx + p.c;
    const float *gp = dout + (int64_t)(p.slab0 + p.rsub) * ldg + p.c;
    float *dp = dx + (int64_t)(p.slab0 + p.rsub) * ldd + p.c;
    const int64_t sx = (int64_t)p.rstep * ldx, sgr = (int64_t)p.rstep * ldg, sd = (int64_t)p.rstep * ldd;
#pragma unroll 4
    for (int k = 0; k < cnt; ++k) {
        V v = *reinterpret_cast<const V *>(xp + k * sx);
        V d = *reinterpret_cast<const V *>(gp + k * sgr);
        uint32_t keep = 0xfu;
        if (drop.thresh) {
            const uint32_t rk = drop.row_key((uint32_t)(p.slab0 + p.rsub + k * p.rstep));
            keep = VEC == 4 ? drop.keep4(rk, (uint32_t)p.c >> 2) : (drop.keep(rk, (uint32_t)p.c) ? 1u : 0u);
        }
        V o;
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            const float xv = comp<VEC>(v, i);
            const float xh = ((act_of(xv, relu) - mu[i]) - lo[i]) * is[i];
            const float g = ((keep >> i) & 1u) ? comp<VEC>(d, i) * drop.scale : 0.0f;
            const float t = gi[i] * ((g - cb[i]) - xh * cg[i]);
            comp<VEC>(o, i) = (relu && xv <= 0.0f) ? 0.0f : t;
        }
        *reinterpret_cast<V *>(dp + k * sd) = o;
    }
}

// ---------------------------------------------------------------- host side

struct Shape {
    int vec, lpr;
    dim3 grid;
    int nslabs;
};

// 16-B accesses when F, every leading dimension and every base allow
Shape plan(int64_t n_rows, int64_t F, std::initializer_list<std::pair<const void *, int64_t>> bufs) {
    Shape s;
    bool v4 = (F % 4) == 0;
    for (auto &b : bufs)
        if (b.first) v4 = v4 && aligned(b.first, 16) && (b.second % 4) == 0;
    s.vec = v4 ? 4 : 1;
    const int64_t groups = F / s.vec;
    s.lpr = 16;
    while (s.lpr < 64 && s.lpr < groups) s.lpr <<= 1;
    s.nslabs = static_cast<int>(ceil_div(n_rows, kSlab));
    s.grid = dim3(static_cast<unsigned>(s.nslabs), static_cast<unsigned>(ceil_div(groups, s.lpr)));
    return s;
}

int check_common(int64_t n_rows, int64_t F) {
    NGNN_RETURN_IF(n_rows < 0 || F <= 0, NGNN_E_ARG);
    // (the slab index arithmetic adds kSlab to a row; at most 2^14 column tiles)
    NGNN_RETURN_IF(n_rows > INT32_MAX - kSlab || F > (1 << 20), NGNN_E_RANGE);
    return NGNN_OK;
}

}  // namespace
}  // namespace ngnn

using namespace ngnn;

extern "C" int ngnn_bn_slab_rows(void) { return kSlab; }

extern "C" size_t ngnn_bn_workspace_bytes(int64_t n_rows, int64_t F) {
    if (n_rows <= 0 || F <= 0) return 0;
    return static_cast<size_t>(ceil_div(n_rows, kSlab)) * 2 * static_cast<size_t>(F) * sizeof(double);
}

extern "C" int ngnn_bn_fwd_train(const float *x, int64_t ldx, int64_t n_rows, int64_t F, int relu,
                                 const float *gamma, const float *beta, double eps, double momentum,
                                 float *running_mean, float *running_var, int64_t *num_batches_tracked,
                                 float p_drop, uint64_t seed, const uint64_t *seed_dev, float *out, int64_t ldo,
                                 float *mean, float *mean_lo, float *invstd, void *ws, size_t ws_bytes,
                                 void *stream) {
    if (int rc = check_common(n_rows, F)) return rc;
    NGNN_RETURN_IF(n_rows < 2, NGNN_E_ARG);  // no batch statistics of one row (torch raises too)
    NGNN_RETURN_IF(!x || !gamma || !beta || !running_mean || !running_var || !num_batches_tracked || !out ||
                       !mean || !mean_lo || !invstd || bad_p(p_drop) || !(eps >= 0.0) || !(momentum <= 1.0),
                   NGNN_E_ARG);
    NGNN_RETURN_IF(ldx < F || ldo < F, NGNN_E_SHAPE);
    NGNN_RETURN_IF(!ws || ws_bytes < ngnn_bn_workspace_bytes(n_rows, F) || !aligned(ws, 8), NGNN_E_WORKSPACE);
    const Shape s = plan(n_rows, F, {{x, ldx}, {out, ldo}});
    hipStream_t st = as_stream(stream);
    double *part = static_cast<double *>(ws);
    const Dropout drop = make_dropout(p_drop, seed);
    with_const<4, 1>(s.vec, [&](auto Vc) {
        constexpr int VEC = decltype(Vc)::value;
        hipLaunchKernelGGL((k_bn_stats<VEC>), s.grid, dim3(kThreads), 0, st, x, ldx, (int)n_rows, (int)F, s.lpr,
                           relu, part);
        hipLaunchKernelGGL(k_bn_stats_final, dim3(static_cast<unsigned>(ceil_div(F, 64))), dim3(64 * kFinLanes), 0,
                           st, part, s.nslabs, (int)n_rows, (int)F, eps, momentum, num_batches_tracked, mean,
                           mean_lo, invstd, running_mean, running_var);
        hipLaunchKernelGGL((k_bn_apply<VEC, 0>), s.grid, dim3(kThreads), 0, st, x, ldx, (int)n_rows, (int)F, s.lpr,
                           relu, mean, mean_lo, invstd, gamma, beta, eps, drop, seed_dev, out, ldo,
                           num_batches_tracked);
    });
    return launch_status();
}

extern "C" int ngnn_bn_fwd_eval(const float *x, int64_t ldx, int64_t n_rows, int64_t F, int relu,
                                const float *gamma, const float *beta, double eps, const float *running_mean,
                                const float *running_var, float *out, int64_t ldo, void *stream) {
    if (int rc = check_common(n_rows, F)) return rc;
    NGNN_RETURN_IF(!gamma || !beta || !running_mean || !running_var || !(eps >= 0.0), NGNN_E_ARG);
    NGNN_RETURN_IF(ldx < F || ldo < F, NGNN_E_SHAPE);
    if (n_rows == 0) return NGNN_OK;
    NGNN_RETURN_IF(!x || !out, NGNN_E_ARG);
    const Shape s = plan(n_rows, F, {{x, ldx}, {out, ldo}});
    const Dropout drop = make_dropout(0.0f, 0);
    with_const<4, 1>(s.vec, [&](auto Vc) {
        constexpr int VEC = decltype(Vc)::value;
        hipLaunchKernelGGL((k_bn_apply<VEC, 1>), s.grid, dim3(kThreads), 0, as_stream(stream), x, ldx, (int)n_rows,
                           (int)F, s.lpr, relu, running_mean, static_cast<const float *>(nullptr), running_var, gamma, beta,
                           eps, drop,
                           static_cast<const uint64_t *>(nullptr), out, ldo, static_cast<int64_t *>(nullptr));
    });
    return launch_status();
}

extern "C" int ngnn_bn_bwd(const float *dout, int64_t ldg, const float *x, int64_t ldx, int64_t n_rows, int64_t F,
                           int relu, const float *gamma, const float *mean, const float *mean_lo,
                           const float *invstd, float p_drop,
                           uint64_t seed, const uint64_t *seed_dev, float *dgamma, float *dbeta, float *dx,
                           int64_t ldd, void *ws, size_t ws_bytes, void *stream) {
    if (int rc = check_common(n_rows, F)) return rc;
    NGNN_RETURN_IF(n_rows < 2, NGNN_E_ARG);
    NGNN_RETURN_IF(!dout || !x || !gamma || !mean || !mean_lo || !invstd || !dgamma || !dbeta || bad_p(p_drop), NGNN_E_ARG);
    NGNN_RETURN_IF(ldg < F || ldx < F || (dx && ldd < F), NGNN_E_SHAPE);
    NGNN_RETURN_IF(!ws || ws_bytes < ngnn_bn_workspace_bytes(n_rows, F) || !aligned(ws, 8), NGNN_E_WORKSPACE);
    const Shape s = plan(n_rows, F, {{dout, ldg}, {x, ldx}, {dx, ldd}});
    hipStream_t st = as_stream(stream);
    double *part = static_cast<double *>(ws);
    const Dropout drop = make_dropout(p_drop, seed);
    with_const<4, 1>(s.vec, [&](auto Vc) {
        constexpr int VEC = decltype(Vc)::value;
        hipLaunchKernelGGL((k_bn_bwd_sums<VEC>), s.grid, dim3(kThreads), 0, st, dout, ldg, x, ldx, (int)n_rows,
                           (int)F, s.lpr, relu, mean, mean_lo, invstd, drop, seed_dev, part);
        hipLaunchKernelGGL(k_bn_bwd_final, dim3(static_cast<unsigned>(ceil_div(F, 64))), dim3(64 * kFinLanes), 0,
                           st, part, s.nslabs, (int)F, dgamma, dbeta);
        if (dx)  // (batch.x needs no gradient: bn1 stops here)
            hipLaunchKernelGGL((k_bn_bwd_dx<VEC>), s.grid, dim3(kThreads), 0, st, dout, ldg, x, ldx, (int)n_rows,
                               (int)F, s.lpr, relu, mean, mean_lo, invstd, gamma, dgamma, dbeta, drop, seed_dev, dx,
                               ldd);
    });
    return launch_status();
}
