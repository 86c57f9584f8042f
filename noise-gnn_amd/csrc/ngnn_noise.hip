// SAGEPL's learnable per-node input noise (the reference's
// SAGEPL.adding_noise, src/models/layers/sagePL.py:41-49):
//   out[i, :] = x[i, :] + s * normalize(noise[id_i, :]) * rate
// with normalize = torch's F.normalize(dim=1) (divide by max(||v||, 1e-12)),
// id_i = n_id[i] (or i without n_id) and s = sign(x) on the n_id=None branch
// (NGNN_NOISE_SIGN).  Forward: one launch instead of torch's index_select,
// norm, clamp, div, mul, add and clone; backward: the normalisation's
// backward with the row's norm recomputed from the table, scattered into the
// table's gradient with float atomics (scatter = 1: duplicate ids accumulate,
// as index_add_) or stored per row (scatter = 0: the deterministic path).
//
// Shape: a group of 16, 32 or 64 lanes (by row width) owns a row; a 256-thread
// workgroup holds 16, 8 or 4 rows.  A row is read twice -- the reduction pass
// and the write pass; the second read is a row of at most a few KiB that the
// same lanes have just loaded.  The row sums go through cross-lane shuffles.
// 16-B loads and stores when the bases and leading dimensions allow (the
// elements past the last whole float4 by a scalar tail), dword accesses
// otherwise.  The atomic pass is always one dword per lane over consecutive
// addresses: a wave's instruction then covers whole 64..256-B segments, the
// shape float atomics run at their full rate in.
#include "ngnn_rows.h"

namespace ngnn {
namespace {

constexpr float kNormEps = 1e-12f;  // F.normalize's eps

__device__ __forceinline__ float sign_of(float x) {
    return x > 0.0f ? 1.0f : (x < 0.0f ? -1.0f : 0.0f);
}

// sum of v[e]^2 over the row (VEC: float4 body + scalar tail), per lane
template <int LPR, bool VEC>
__device__ __forceinline__ float row_sumsq(const float *__restrict__ v, int F, int sub) {
    float ss = 0.0f;
    const int nv = VEC ? F >> 2 : 0;
    for (int j = sub; j < nv; j += LPR) {
        const float4 a = reinterpret_cast<const float4 *>(v)[j];
        ss += a.x * a.x + a.y * a.y + a.z * a.z + a.w * a.w;
    }
    for (int e = 4 * nv + sub; e < F; e += LPR) ss += v[e] * v[e];
    return ss;
}

template <int LPR, bool VEC>
__global__ __launch_bounds__(256) void k_noise_fwd(const float *__restrict__ x, int64_t ldx,
                                                   const float *__restrict__ noise, int64_t ldn,
                                                   int64_t n_nodes, const int64_t *__restrict__ n_id,
                                                   int64_t n_rows, int F, float rate, int sgn,
                                                   float *__restrict__ out, int64_t ldo,
                                                   int32_t *__restrict__ bad) {
    constexpr int RPB = 256 / LPR;
    const int sub = threadIdx.x % LPR;
    const int64_t row = static_cast<int64_t>(blockIdx.x) * RPB + threadIdx.x / LPR;
    if (row >= n_rows) return;  // (whole lane groups: the shuffles below stay inside a group)
    const int64_t id = n_id ? n_id[row] : row;
    const float *xr = x + row * ldx;
    float *orow = out + row * ldo;
    const int nv = VEC ? F >> 2 : 0;
    if (id < 0 || id >= n_nodes) {  // the table is neither read nor written: out = x
        for (int j = sub; j < nv; j += LPR)
            reinterpret_cast<float4 *>(orow)[j] = reinterpret_cast<const float4 *>(xr)[j];
        for (int e = 4 * nv + sub; e < F; e += LPR) orow[e] = xr[e];
        if (bad && sub == 0) atomicAdd(bad, 1);
        return;
    }
    const float *vr = noise + id * ldn;
    const float ss = group_sum<LPR>(row_sumsq<LPR, VEC>(vr, F, sub));
    const float d = fmaxf(sqrtf(ss), kNormEps);
    auto one = [&](float xv, float v) {
        const float u = v / d;
        return xv + (sgn ? sign_of(xv) * u : u) * rate;
    };
    for (int j = sub; j < nv; j += LPR) {
        const float4 a = reinterpret_cast<const float4 *>(xr)[j];
        const float4 v = reinterpret_cast<const float4 *>(vr)[j];
        reinterpret_cast<float4 *>(orow)[j] = float4{one(a.x, v.x), one(a.y, v.y), one(a.z, v.z), one(a.w, v.w)};
    }
    for (int e = 4 * nv + sub; e < F; e += LPR) orow[e] = one(xr[e], vr[e]);
}

// gs = (g * rate) * s -- the gradient reaching normalize(v)
__device__ __forceinline__ float scaled_grad(float g, float rate, int sgn, const float *xr, int e) {
    const float gr = g * rate;
    return sgn ? gr * sign_of(xr[e]) : gr;
}

template <int LPR, bool VEC>
__global__ __launch_bounds__(256) void k_noise_bwd(const float *__restrict__ g, int64_t ldg,
                                                   const float *__restrict__ x, int64_t ldx,
                                                   const float *__restrict__ noise, int64_t ldn,
                                                   int64_t n_nodes, const int64_t *__restrict__ n_id,
                                                   int scatter, int64_t n_rows, int F, float rate, int sgn,
                                                   float *__restrict__ dnoise, int64_t ldd,
                                                   int32_t *__restrict__ bad) {
    constexpr int RPB = 256 / LPR;
    const int sub = threadIdx.x % LPR;
    const int64_t row = static_cast<int64_t>(blockIdx.x) * RPB + threadIdx.x / LPR;
    if (row >= n_rows) return;
    const int64_t id = n_id ? n_id[row] : row;
    const int nv = VEC ? F >> 2 : 0;
    if (id < 0 || id >= n_nodes) {  // contributes nothing; the per-row buffer gets its zeros
        if (!scatter) {
            float *dr = dnoise + row * ldd;
            for (int j = sub; j < nv; j += LPR) reinterpret_cast<float4 *>(dr)[j] = float4{0.0f, 0.0f, 0.0f, 0.0f};
            for (int e = 4 * nv + sub; e < F; e += LPR) dr[e] = 0.0f;
        }
        if (bad && sub == 0) atomicAdd(bad, 1);
        return;
    }
    const float *gr = g + row * ldg;
    const float *xr = sgn ? x + row * ldx : nullptr;
    const float *vr = noise + id * ldn;
    // one pass for both row sums: ||v||^2 and <v, gs>
    float ss = 0.0f, dt = 0.0f;
    for (int j = sub; j < nv; j += LPR) {
        const float4 v = reinterpret_cast<const float4 *>(vr)[j];
        const float4 a = reinterpret_cast<const float4 *>(gr)[j];
        ss += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
        dt += v.x * scaled_grad(a.x, rate, sgn, xr, 4 * j) + v.y * scaled_grad(a.y, rate, sgn, xr, 4 * j + 1) +
              v.z * scaled_grad(a.z, rate, sgn, xr, 4 * j + 2) + v.w * scaled_grad(a.w, rate, sgn, xr, 4 * j + 3);
    }
    for (int e = 4 * nv + sub; e < F; e += LPR) {
        const float v = vr[e];
        ss += v * v;
        dt += v * scaled_grad(gr[e], rate, sgn, xr, e);
    }
    ss = group_sum<LPR>(ss);
    dt = group_sum<LPR>(dt);
    const float nrm = sqrtf(ss);
    const bool clamped = !(nrm >= kNormEps);  // clamp_min's backward: no gradient through the norm
    const float d = clamped ? kNormEps : nrm;
    const float du = clamped ? 0.0f : dt / d;  // <u, gs>
    auto one = [&](float gv, float v, int e) {
        const float gs = scaled_grad(gv, rate, sgn, xr, e);
        return (gs - (v / d) * du) / d;
    };
    if (scatter) {
        float *dr = dnoise + id * ldd;
        for (int e = sub; e < F; e += LPR) atomicAdd(dr + e, one(gr[e], vr[e], e));
        return;
    }
    float *dr = dnoise + row * ldd;
    for (int j = sub; j < nv; j += LPR) {
        const float4 v = reinterpret_cast<const float4 *>(vr)[j];
        const float4 a = reinterpret_cast<const float4 *>(gr)[j];
        reinterpret_cast<float4 *>(dr)[j] = float4{one(a.x, v.x, 4 * j), one(a.y, v.y, 4 * j + 1),
                                                   one(a.z, v.z, 4 * j + 2), one(a.w, v.w, 4 * j + 3)};
    }
    for (int e = 4 * nv + sub; e < F; e += LPR) dr[e] = one(gr[e], vr[e], e);
}

bool vec_ok(const void *p, int64_t ld) { return aligned(p, 16) && ld % 4 == 0; }

// lanes per row: the smallest group whose first sweep covers the row
int lanes_per_row(int64_t F, bool vec) {
    const int64_t units = vec ? ceil_div(F, 4) : F;
    return units <= 16 ? 16 : (units <= 32 ? 32 : 64);
}

int check_common(int64_t ldn, int64_t n_nodes, const int64_t *n_id, int64_t n_rows,
                 int64_t F, int flags) {
    NGNN_RETURN_IF(n_rows < 0 || F < 0 || n_nodes < 0 || ldn < 0, NGNN_E_ARG);
    NGNN_RETURN_IF(flags & ~NGNN_NOISE_SIGN, NGNN_E_ARG);
    NGNN_RETURN_IF(!n_id && n_rows != n_nodes, NGNN_E_ARG);
    NGNN_RETURN_IF(ldn < F, NGNN_E_SHAPE);
    NGNN_RETURN_IF(!fits_i32(F) || !fits_i32(n_rows), NGNN_E_RANGE);
    return NGNN_OK;
}

}  // namespace
}  // namespace ngnn

using namespace ngnn;

#define NGNN_NOISE_LAUNCH(KERNEL, lpr, vec, grid_rows, ...)                                              \
    do {                                                                                                 \
        const unsigned grid_ = static_cast<unsigned>(ceil_div((grid_rows), 256 / (lpr)));                \
        if (vec) {                                                                                       \
            if ((lpr) == 16) hipLaunchKernelGGL((KERNEL<16, true>), dim3(grid_), dim3(256), 0, st, __VA_ARGS__);      \
            else if ((lpr) == 32) hipLaunchKernelGGL((KERNEL<32, true>), dim3(grid_), dim3(256), 0, st, __VA_ARGS__); \
            else hipLaunchKernelGGL((KERNEL<64, true>), dim3(grid_), dim3(256), 0, st, __VA_ARGS__);     \
        } else {                                                                                         \
            if ((lpr) == 16) hipLaunchKernelGGL((KERNEL<16, false>), dim3(grid_), dim3(256), 0, st, __VA_ARGS__);      \
            else if ((lpr) == 32) hipLaunchKernelGGL((KERNEL<32, false>), dim3(grid_), dim3(256), 0, st, __VA_ARGS__); \
            else hipLaunchKernelGGL((KERNEL<64, false>), dim3(grid_), dim3(256), 0, st, __VA_ARGS__);    \
        }                                                                                                \
    } while (0)

extern "C" int ngnn_node_noise_fwd(const float *x, int64_t ldx, const float *noise, int64_t ldn,
                                   int64_t n_nodes, const int64_t *n_id, int64_t n_rows, int64_t F,
                                   float rate, int flags, float *out, int64_t ldo, int32_t *bad,
                                   void *stream) {
    const int rc = check_common(ldn, n_nodes, n_id, n_rows, F, flags);
    if (rc) return rc;
    NGNN_RETURN_IF(ldx < F || ldo < F, NGNN_E_SHAPE);
    if (n_rows == 0 || F == 0) return NGNN_OK;
    NGNN_RETURN_IF(!x || !noise || !out, NGNN_E_ARG);
    hipStream_t st = as_stream(stream);
    const bool vec = F >= 4 && vec_ok(x, ldx) && vec_ok(noise, ldn) && vec_ok(out, ldo);
    const int lpr = lanes_per_row(F, vec);
    const int sgn = (flags & NGNN_NOISE_SIGN) != 0;
    NGNN_NOISE_LAUNCH(k_noise_fwd, lpr, vec, n_rows, x, ldx, noise, ldn, n_nodes, n_id, n_rows,
                      static_cast<int>(F), rate, sgn, out, ldo, bad);
    return launch_status();
}

extern "C" int ngnn_node_noise_bwd(const float *g, int64_t ldg, const float *x, int64_t ldx,
                                   const float *noise, int64_t ldn, int64_t n_nodes, const int64_t *n_id,
                                   int scatter, int64_t n_rows, int64_t F, float rate, int flags,
                                   float *dnoise, int64_t ldd, int32_t *bad, void *stream) {
    const int rc = check_common(ldn, n_nodes, n_id, n_rows, F, flags);
    if (rc) return rc;
    NGNN_RETURN_IF(scatter != 0 && scatter != 1, NGNN_E_ARG);
    const int sgn = (flags & NGNN_NOISE_SIGN) != 0;
    NGNN_RETURN_IF(ldg < F || ldd < F || (sgn && ldx < F), NGNN_E_SHAPE);
    if (n_rows == 0 || F == 0) return NGNN_OK;
    NGNN_RETURN_IF(!g || !noise || !dnoise || (sgn && !x), NGNN_E_ARG);
    hipStream_t st = as_stream(stream);
    // (the atomic pass is dword-wide whatever the alignment of dnoise)
    const bool vec = F >= 4 && vec_ok(g, ldg) && vec_ok(noise, ldn) && (scatter || vec_ok(dnoise, ldd));
    const int lpr = lanes_per_row(F, vec);
    NGNN_NOISE_LAUNCH(k_noise_bwd, lpr, vec, n_rows, g, ldg, x, ldx, noise, ldn, n_nodes, n_id, scatter,
                      n_rows, static_cast<int>(F), rate, sgn, dnoise, ldd, bad);
    return launch_status();
}
