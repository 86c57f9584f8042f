// The hidden-state tap of the fused SAGE stack (include/ngnn.h, "hidden-state
// tap"): a stack that returns h = relu(conv_{L-2}(...)) BEFORE dropout next to
// its logits runs layer L-2 with relu = 1, p_drop = 0 and then
//   ngnn_dropout_rows   xd = dropout(h), bit for bit what the layer's own
//                       epilogue would have stored with p_drop (same Dropout
//                       struct, same (seed, global row, global column) key,
//                       the same one product h * scale);
//   ngnn_tap_grad       dz = dy [xd > 0] yscale + dh [h > 0]: the ReLU +
//                       dropout backward of the path through xd (ngnn_sage_wgrad's
//                       dz for y != NULL) plus the ReLU backward of the tapped
//                       output, so the layer's wgrad / dgrad run once on dz
//                       with no mask.
//
// Shape (ngnn_noise.hip's): a group of 16, 32 or 64 lanes (by row width) owns
// a row, a 256-thread workgroup holds 16, 8 or 4 rows; 16-B accesses when
// every base and leading dimension allows them (the columns past the last
// whole float4 by a scalar tail), dword accesses otherwise.  The row bound is
// a device word: nothing is read back.  Hashes: a lane computes one per column
// quad it owns (byte mode: the quad's hash; bit mode: the quad's 32-column
// word), never one per element.
#include "ngnn_device.h"
#include "ngnn_rows.h"

namespace ngnn {
namespace {

// rows below min(n_rows, *bound) are live (bound null: n_rows)
__device__ __forceinline__ int64_t live_rows(int64_t n_rows, const int32_t *bound) {
    if (!bound) return n_rows;
    const int64_t b = *bound;
    return b < n_rows ? b : n_rows;
}

template <int LPR, bool VEC>
__global__ __launch_bounds__(256) void k_dropout_rows(const float *__restrict__ h, int64_t ldh, int64_t n_rows,
                                                      const int32_t *__restrict__ n_rows_dev, int F, Dropout drop,
                                                      const uint64_t *__restrict__ seed_dev,
                                                      float *__restrict__ out, int64_t ldo) {
    constexpr int RPB = 256 / LPR;
    const int sub = threadIdx.x % LPR;
    const int64_t row = static_cast<int64_t>(blockIdx.x) * RPB + threadIdx.x / LPR;
    if (row >= live_rows(n_rows, n_rows_dev)) return;
    if (seed_dev) drop.reseed(*seed_dev);
    const float *hr = h + row * ldh;
    float *orow = out + row * ldo;
    const int nv = VEC ? F >> 2 : 0;
    if (!drop.thresh) {  // p = 0: a copy (no product: every bit pattern passes)
        for (int j = sub; j < nv; j += LPR)
            reinterpret_cast<float4 *>(orow)[j] = reinterpret_cast<const float4 *>(hr)[j];
        for (int e = 4 * nv + sub; e < F; e += LPR) orow[e] = hr[e];
        return;
    }
    const uint32_t rk = drop.row_key(static_cast<uint32_t>(row));
    const float scale = drop.scale;
    for (int j = sub; j < nv; j += LPR) {
        const float4 a = reinterpret_cast<const float4 *>(hr)[j];
        const uint32_t k = drop.keep4(rk, static_cast<uint32_t>(j));  // one hash
        reinterpret_cast<float4 *>(orow)[j] = float4{(k & 1u) ? a.x * scale : 0.0f, (k & 2u) ? a.y * scale : 0.0f,
                                                     (k & 4u) ? a.z * scale : 0.0f, (k & 8u) ? a.w * scale : 0.0f};
    }
    // (dword path and tail: a lane's columns are LPR apart -- no two of them in
    // one quad, nor, past a 16-lane group's single sweep, in one 32-column word)
    for (int e = 4 * nv + sub; e < F; e += LPR)
        orow[e] = drop.keep(rk, static_cast<uint32_t>(e)) ? hr[e] * scale : 0.0f;
}

// FORM 0: dy and xd given; 1: dy given, xd null (no dropout); 2: dy null
template <int FORM>
__device__ __forceinline__ float tap_dz(float dy, float xd, float yscale, float dh, float h) {
    const float t = (h > 0.0f) ? dh : 0.0f;
    if (FORM == 2) return t;
    if (FORM == 1) return (h > 0.0f) ? dy + dh : 0.0f;
    return ((xd > 0.0f) ? dy * yscale : 0.0f) + t;
}

// (dz may alias dy: no __restrict__ on the two; a lane reads an element of dy
// before it writes the same element of dz)
template <int LPR, bool VEC, int FORM>
__global__ __launch_bounds__(256) void k_tap_grad(const float *dy, int64_t ldy, const float *__restrict__ xd,
                                                  int64_t ldx, float yscale, const float *__restrict__ dh,
                                                  int64_t ldg, const float *__restrict__ h, int64_t ldh,
                                                  int64_t n_rows, const int32_t *__restrict__ r_ptr, int F,
                                                  float *dz, int64_t ldz) {
    constexpr int RPB = 256 / LPR;
    const int sub = threadIdx.x % LPR;
    const int64_t row = static_cast<int64_t>(blockIdx.x) * RPB + threadIdx.x / LPR;
    if (row >= live_rows(n_rows, r_ptr)) return;
    const float *dyr = FORM != 2 ? dy + row * ldy : nullptr;
    const float *xr = FORM == 0 ? xd + row * ldx : nullptr;
    const float *gr = dh + row * ldg;
    const float *hr = h + row * ldh;
    float *zr = dz + row * ldz;
    const int nv = VEC ? F >> 2 : 0;
    const float4 z4{0.0f, 0.0f, 0.0f, 0.0f};
    for (int j = sub; j < nv; j += LPR) {
        const float4 a = FORM != 2 ? reinterpret_cast<const float4 *>(dyr)[j] : z4;
        const float4 x = FORM == 0 ? reinterpret_cast<const float4 *>(xr)[j] : z4;
        const float4 g = reinterpret_cast<const float4 *>(gr)[j];
        const float4 v = reinterpret_cast<const float4 *>(hr)[j];
        reinterpret_cast<float4 *>(zr)[j] =
            float4{tap_dz<FORM>(a.x, x.x, yscale, g.x, v.x), tap_dz<FORM>(a.y, x.y, yscale, g.y, v.y),
                   tap_dz<FORM>(a.z, x.z, yscale, g.z, v.z), tap_dz<FORM>(a.w, x.w, yscale, g.w, v.w)};
    }
    for (int e = 4 * nv + sub; e < F; e += LPR)
        zr[e] = tap_dz<FORM>(FORM != 2 ? dyr[e] : 0.0f, FORM == 0 ? xr[e] : 0.0f, yscale, gr[e], hr[e]);
}

bool vec_ok(const void *p, int64_t ld) { return aligned(p, 16) && ld % 4 == 0; }

// lanes per row: the smallest group whose first sweep covers the row
int lanes_per_row(int64_t F, bool vec) {
    const int64_t units = vec ? ceil_div(F, 4) : F;
    return units <= 16 ? 16 : (units <= 32 ? 32 : 64);
}

int check_rows(int64_t n_rows, int64_t F) {
    NGNN_RETURN_IF(n_rows < 0 || F < 0, NGNN_E_ARG);
    NGNN_RETURN_IF(!fits_i32(F) || !fits_i32(n_rows), NGNN_E_RANGE);
    return NGNN_OK;
}

// f(LPR, VEC) as integral constants, and the grid of 256-thread workgroups
template <class Fn>
void for_shape(int lpr, bool vec, Fn &&f) {
    with_const<16, 32, 64>(lpr, [&](auto L) { with_const<1, 0>(vec ? 1 : 0, [&](auto V) { f(L, V); }); });
}
dim3 row_grid(int64_t n_rows, int lpr) { return dim3(static_cast<unsigned>(ceil_div(n_rows, 256 / lpr))); }

}  // namespace
}  // namespace ngnn

using namespace ngnn;

extern "C" int ngnn_dropout_rows(const float *h, int64_t ldh, int64_t n_rows, const int32_t *n_rows_dev,
                                 int64_t F, float p_drop, uint64_t seed, const uint64_t *seed_dev, float *out,
                                 int64_t ldo, void *stream) {
    if (int rc = check_rows(n_rows, F)) return rc;
    NGNN_RETURN_IF(bad_p(p_drop), NGNN_E_ARG);
    NGNN_RETURN_IF(ldh < F || ldo < F, NGNN_E_SHAPE);
    if (n_rows == 0 || F == 0) return NGNN_OK;
    NGNN_RETURN_IF(!h || !out || h == out, NGNN_E_ARG);
    hipStream_t st = as_stream(stream);
    const bool vec = F >= 4 && vec_ok(h, ldh) && vec_ok(out, ldo);
    const int lpr = lanes_per_row(F, vec);
    const Dropout drop = make_dropout(p_drop, seed);
    for_shape(lpr, vec, [&](auto L, auto V) {
        hipLaunchKernelGGL((k_dropout_rows<decltype(L)::value, decltype(V)::value != 0>), row_grid(n_rows, lpr),
                           dim3(256), 0, st, h, ldh, n_rows, n_rows_dev, static_cast<int>(F), drop, seed_dev, out, ldo);
    });
    return launch_status();
}

extern "C" int ngnn_tap_grad(const float *dy, int64_t ldy, const float *xd, int64_t ldx, float yscale,
                             const float *dh, int64_t ldg, const float *h, int64_t ldh, int64_t n_rows,
                             const int32_t *r_ptr, int64_t F, float *dz, int64_t ldz, void *stream) {
    if (int rc = check_rows(n_rows, F)) return rc;
    // (a leading dimension is read only with its pointer; xd only next to dy)
    const bool masked = dy && xd;
    NGNN_RETURN_IF(ldg < F || ldh < F || ldz < F || (dy && ldy < F) || (masked && ldx < F), NGNN_E_SHAPE);
    if (n_rows == 0 || F == 0) return NGNN_OK;
    NGNN_RETURN_IF(!dh || !h || !dz, NGNN_E_ARG);
    hipStream_t st = as_stream(stream);
    const bool vec = F >= 4 && vec_ok(dh, ldg) && vec_ok(h, ldh) && vec_ok(dz, ldz) && (!dy || vec_ok(dy, ldy)) &&
                     (!masked || vec_ok(xd, ldx));
    const int lpr = lanes_per_row(F, vec);
    const int form = !dy ? 2 : (xd ? 0 : 1);
    for_shape(lpr, vec, [&](auto L, auto V) {
        with_const<0, 1, 2>(form, [&](auto Fm) {
            hipLaunchKernelGGL((k_tap_grad<decltype(L)::value, decltype(V)::value != 0, decltype(Fm)::value>),
                               row_grid(n_rows, lpr), dim3(256), 0, st, dy, ldy, xd, ldx, yscale, dh, ldg, h, ldh,
                               n_rows, r_ptr, static_cast<int>(F), dz, ldz);
        });
    });
    return launch_status();
}
