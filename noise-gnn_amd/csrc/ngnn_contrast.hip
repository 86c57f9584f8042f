// The contrastive half of the reference's train_ct step (pipeline_test.py:
// 144-166): shuffle_pos (src/utils/augmentation.py:88-102) and
// Discriminator_innerprod + BCEExeprtLoss (src/utils/data_utils.py:34-64).
//
// ngnn_shuffle_rows: per row, a uniform m-subset of the columns, the values
// at those columns permuted uniformly -- a pure function of (seed, row, F, m)
// (the draw: include/ngnn.h).  Both the subset and the permutation are taken
// by RANK COUNTING over 64-bit keys, ties by column, so the result does not
// depend on the launch geometry:
//   F <= 256: one wave per row, <= 4 columns per lane in registers, the keys'
//             upper halves in LDS (every lane reads the same key: a
//             broadcast, no bank conflict); F + m key reads and as many
//             32-bit compares per column, the full keys only where two upper
//             halves tie (k_shuffle_narrow).
//   F  > 256: one workgroup per row, the compared keys recomputed on the
//             scalar unit (no LDS table of 8 F bytes: F goes up to 65535),
//             the sorted selection p_k as uint16 in dynamic LDS.  O(F^2 / 256)
//             per thread: correct, not fast.
//
// ngnn_contrast_fwd / _bwd: one wave per selected row, both dots in one pass
// over the three rows, the row terms added in a fixed order by a second
// launch (deterministic); the backward scatters with float atomics into
// caller-prepared buffers (duplicates accumulate; distinct indices: one add
// per element onto the caller's value, bitwise reproducible).
#include "ngnn_rows.h"
#include "ngnn_sample_dev.h"

namespace ngnn {
namespace {

constexpr uint64_t kRowSalt = 0x632BE59BD9B4E019ull;   // b1 = mix64(seed ^ mix64(r + kRowSalt))
constexpr uint64_t kPermSalt = 0xD1B54A32D192ED03ull;  // b2 = mix64(b1 ^ kPermSalt)
constexpr int kNarrowF = 256;

// (key a, column / position ia) before (key b, ib)
__device__ __forceinline__ int before(uint64_t a, int ia, uint64_t b, int ib) {
    return (a < b || (a == b && ia < ib)) ? 1 : 0;
}

// One wave per row, 4 rows per workgroup, F <= 64 NK.  Lane l holds columns
// l + 64 k.  No wave leaves early (the barriers are workgroup-wide); a wave
// past the last row computes on zeros and stores nothing.
//
// The rank loops compare the keys' UPPER HALVES only (one 32-bit compare and
// one add-with-carry per pair, against two 64-bit compares): a count of
// strictly smaller upper halves never exceeds the exact rank, so
//   - the columns it puts below m include the exact m-subset, and are that
//     subset iff there are m of them;
//   - its ranks within S_r are exact iff they add up to m (m - 1) / 2.
// A wave that fails either test (two upper halves equal where it matters:
// about one row in 10^6 at F = 100) redoes that loop on the full keys,
// recomputed -- a wave-uniform branch without a barrier in it.
template <int NK>
__global__ __launch_bounds__(256) void k_shuffle_narrow(const float *__restrict__ x, int64_t ldx,
                                                        int64_t n_rows, int F, int m, uint64_t seed,
                                                        float *__restrict__ out, int64_t ldo) {
    __shared__ uint32_t sh1[4][64 * NK];
    __shared__ uint32_t sh2[4][64 * NK];
    __shared__ float sx[4][64 * NK];
    __shared__ uint16_t scol[4][64 * NK];
    // (the wave index through readfirstlane: the row's bases b1, b2 are then
    // computed once on the scalar unit, not per lane)
    const int w = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    const int64_t r = static_cast<int64_t>(blockIdx.x) * 4 + w;
    const bool live = r < n_rows;
    const float *xr = x + r * ldx;
    float *orow = out + r * ldo;
    float v[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        const int c = lane + 64 * k;
        v[k] = (live && c < F) ? xr[c] : 0.0f;
    }
    if (m <= 1) {  // (uniform) nothing moves
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const int c = lane + 64 * k;
            if (live && c < F) orow[c] = v[k];
        }
        return;
    }
    const uint64_t b1 = mix64(seed ^ mix64(static_cast<uint64_t>(r) + kRowSalt));
    const uint64_t b2 = mix64(b1 ^ kPermSalt);
    uint32_t h1[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        const int c = lane + 64 * k;
        h1[k] = static_cast<uint32_t>(mix64(b1 + static_cast<uint64_t>(c)) >> 32);
        if (c < F) {
            sh1[w][c] = h1[k];
            sx[w][c] = v[k];
        }
    }
    __syncthreads();
    int rank[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) rank[k] = 0;
    for (int c2 = 0; c2 < F; ++c2) {
        const uint32_t kk = sh1[w][c2];
#pragma unroll
        for (int k = 0; k < NK; ++k) rank[k] += kk < h1[k] ? 1 : 0;
    }
    bool sel[NK];
    int nsel = 0;
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        sel[k] = lane + 64 * k < F && rank[k] < m;
        nsel += __popcll(__ballot(sel[k]));
    }
    if (nsel != m) {  // (wave-uniform) the exact ranks
        uint64_t k1[NK];
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            k1[k] = mix64(b1 + static_cast<uint64_t>(lane + 64 * k));
            rank[k] = 0;
        }
        for (int c2 = 0; c2 < F; ++c2) {
            const uint64_t kk = mix64(b1 + static_cast<uint64_t>(c2));
#pragma unroll
            for (int k = 0; k < NK; ++k) rank[k] += before(kk, c2, k1[k], lane + 64 * k);
        }
#pragma unroll
        for (int k = 0; k < NK; ++k) sel[k] = lane + 64 * k < F && rank[k] < m;
    }
    // S_r in column order: position = selected columns before mine
    int pos[NK];
    uint32_t h2[NK];
    int base = 0;
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        const int c = lane + 64 * k;
        const uint64_t bal = __ballot(sel[k]);
        pos[k] = 0;
        h2[k] = 0;
        if (sel[k]) {
            pos[k] = base + __popcll(bal & ((1ull << lane) - 1ull));
            h2[k] = static_cast<uint32_t>(mix64(b2 + static_cast<uint64_t>(c)) >> 32);
            sh2[w][pos[k]] = h2[k];
            scol[w][pos[k]] = static_cast<uint16_t>(c);
        }
        base += __popcll(bal);
    }
    __syncthreads();
    int rho[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) rho[k] = 0;
    for (int j = 0; j < m; ++j) {
        const uint32_t kk = sh2[w][j];
#pragma unroll
        for (int k = 0; k < NK; ++k) rho[k] += kk < h2[k] ? 1 : 0;
    }
    int total = 0;
#pragma unroll
    for (int k = 0; k < NK; ++k) total += sel[k] ? rho[k] : 0;
    if (wave_sum(total) != m * (m - 1) / 2) {  // (wave-uniform) the exact ranks
        uint64_t k2[NK];
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            k2[k] = sel[k] ? mix64(b2 + static_cast<uint64_t>(lane + 64 * k)) : 0;
            rho[k] = 0;
        }
        for (int j = 0; j < m; ++j) {
            const uint64_t kk = mix64(b2 + static_cast<uint64_t>(scol[w][j]));
#pragma unroll
            for (int k = 0; k < NK; ++k) rho[k] += before(kk, j, k2[k], pos[k]);
        }
    }
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        const int c = lane + 64 * k;
        // (an unselected column's rho counts against key 0: 0, a valid slot)
        const float moved = sx[w][scol[w][rho[k] < m ? rho[k] : 0]];
        if (live && c < F) orow[c] = sel[k] ? moved : v[k];
    }
}

// One workgroup per row, any F <= 65535.  ptab: the selected columns in
// ascending order (uint16 [m], dynamic LDS).
__global__ __launch_bounds__(256) void k_shuffle_wide(const float *__restrict__ x, int64_t ldx, int F,
                                                      int m, uint64_t seed, float *__restrict__ out,
                                                      int64_t ldo) {
    extern __shared__ __attribute__((aligned(16))) uint16_t ptab[];
    __shared__ int wcnt[4];
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const int64_t r = blockIdx.x;
    const float *xr = x + r * ldx;
    float *orow = out + r * ldo;
    if (m <= 1) {
        for (int c = tid; c < F; c += 256) orow[c] = xr[c];
        return;
    }
    const uint64_t b1 = mix64(seed ^ mix64(static_cast<uint64_t>(r) + kRowSalt));
    const uint64_t b2 = mix64(b1 ^ kPermSalt);
    int base = 0;
    for (int c0 = 0; c0 < F; c0 += 256) {  // (uniform trip count)
        const int c = c0 + tid;
        const uint64_t kc = mix64(b1 + static_cast<uint64_t>(c));
        int rank = 0;
        for (int c2 = 0; c2 < F; ++c2)  // (b1, c2 uniform: the key on the scalar unit)
            rank += before(mix64(b1 + static_cast<uint64_t>(c2)), c2, kc, c);
        const bool sel = c < F && rank < m;
        const uint64_t bal = __ballot(sel);
        if (lane == 0) wcnt[w] = __popcll(bal);
        __syncthreads();
        int off = base, tot = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (q < w) off += wcnt[q];
            tot += wcnt[q];
        }
        if (sel) ptab[off + __popcll(bal & ((1ull << lane) - 1ull))] = static_cast<uint16_t>(c);
        else if (c < F) orow[c] = xr[c];
        base += tot;
        __syncthreads();
    }
    for (int j0 = 0; j0 < m; j0 += 256) {
        const int j = j0 + tid;
        const int c = ptab[j < m ? j : 0];
        const uint64_t kc = mix64(b2 + static_cast<uint64_t>(c));
        int rho = 0;
        for (int k = 0; k < m; ++k) {
            const int pk = __builtin_amdgcn_readfirstlane(static_cast<int>(ptab[k]));
            rho += before(mix64(b2 + static_cast<uint64_t>(pk)), k, kc, j);
        }
        if (j < m) orow[c] = xr[ptab[rho]];
    }
}

// ---------------------------------------------------------------------------
// contrastive discriminator loss

// max(x, 0) + log1p(exp(-|x|)); NaN stays NaN
__device__ __forceinline__ double softplus(double x) {
    return (x > 0.0 ? x : 0.0) + log1p(exp(-fabs(x)));
}

// The logits are kept in double: the positive term's gradient is
// sigma(-a) ~ e^-a, whose relative error is the ABSOLUTE error of a -- a
// float dot product of a ~ 40 (unit-scale activations, H = 256) is off by a
// few 1e-6, which would spend the whole 1e-5 gradient bar on one rounding.
// M rows of two doubles: nothing next to the three row gathers.

// one wave per selected row i: ws[i] = <h, hp>, ws[M + i] = <h, hn> at row
// idx[i]; an index outside [0, n_rows): NaN for both, nothing read, counted
__global__ __launch_bounds__(256) void k_contrast_rows(const float *__restrict__ h, int64_t ldh,
                                                       const float *__restrict__ hp, int64_t ldp,
                                                       const float *__restrict__ hn, int64_t ldn,
                                                       int64_t n_rows, int F,
                                                       const int64_t *__restrict__ idx, int M,
                                                       double *__restrict__ ws, int32_t *__restrict__ bad) {
    const int lane = wave_lane(), i = wave_row();
    if (i >= M) return;
    const int64_t r = idx[i];
    double a = NAN, b = NAN;
    if (r >= 0 && r < n_rows) {
        const float *hr = h + r * ldh, *pr = hp + r * ldp, *nr = hn + r * ldn;
        a = 0.0;
        b = 0.0;
        for (int k = lane; k < F; k += 64) {
            const double hv = hr[k];
            a += hv * static_cast<double>(pr[k]);
            b += hv * static_cast<double>(nr[k]);
        }
        a = wave_sum(a);
        b = wave_sum(b);
    } else if (bad && lane == 0) {
        atomicAdd(bad, 1);
    }
    if (lane == 0) {
        ws[i] = a;
        ws[M + i] = b;
    }
}

// one workgroup adds the row terms in a fixed order -> deterministic
__global__ __launch_bounds__(256) void k_contrast_sum(const double *__restrict__ ws, int M,
                                                      float *__restrict__ out) {
    __shared__ double tree[2][256];
    double t[2];  // positive terms, negative terms
    block_sum(tree, t, M, [&](int i, double(&a)[2]) {
        a[0] += softplus(-ws[i]);
        a[1] += softplus(ws[M + i]);
    });
    if (threadIdx.x == 0) {
        const double p = t[0] / M, n = t[1] / M;
        out[0] = static_cast<float>(p + n);
        out[1] = static_cast<float>(p);
        out[2] = static_cast<float>(n);
    }
}

// one wave per selected row: the three gradient rows, added atomically.
// sigma(-a) = 1 / (1 + e^a) directly (e^a = inf gives 0, never sigma(a) - 1).
__global__ __launch_bounds__(256) void k_contrast_bwd(const float *__restrict__ h, int64_t ldh,
                                                      const float *__restrict__ hp, int64_t ldp,
                                                      const float *__restrict__ hn, int64_t ldn,
                                                      int64_t n_rows, int F,
                                                      const int64_t *__restrict__ idx, int M,
                                                      const double *__restrict__ ws,
                                                      const float *__restrict__ g, float *__restrict__ dh,
                                                      int64_t lddh, float *__restrict__ dhp, int64_t lddp,
                                                      float *__restrict__ dhn, int64_t lddn) {
    const int lane = wave_lane(), i = wave_row();
    if (i >= M) return;
    const int64_t r = idx[i];
    if (r < 0 || r >= n_rows) return;
    const double scale = static_cast<double>(*g) / M;
    const float ca = static_cast<float>(-scale / (1.0 + exp(ws[i])));      // -(g / M) sigma(-a)
    const float cb = static_cast<float>(scale / (1.0 + exp(-ws[M + i])));  //  (g / M) sigma(b)
    const float *hr = h + r * ldh, *pr = hp + r * ldp, *nr = hn + r * ldn;
    for (int k = lane; k < F; k += 64) {
        const float hv = hr[k];
        if (dh) atomicAdd(dh + r * lddh + k, ca * pr[k] + cb * nr[k]);
        if (dhp) atomicAdd(dhp + r * lddp + k, ca * hv);
        if (dhn) atomicAdd(dhn + r * lddn + k, cb * hv);
    }
}

}  // namespace
}  // namespace ngnn

using namespace ngnn;

extern "C" int ngnn_shuffle_rows(const float *x, int64_t ldx, int64_t n_rows, int64_t F, int64_t m,
                                 uint64_t seed, float *out, int64_t ldo, void *stream) {
    NGNN_RETURN_IF(n_rows < 0 || F < 0 || m < 0 || m > F, NGNN_E_ARG);
    NGNN_RETURN_IF(ldx < F || ldo < F, NGNN_E_SHAPE);
    NGNN_RETURN_IF(!fits_i32(n_rows) || F > 65535, NGNN_E_RANGE);
    if (n_rows == 0 || F == 0) return NGNN_OK;
    NGNN_RETURN_IF(!x || !out, NGNN_E_ARG);
    hipStream_t st = as_stream(stream);
    const int Fi = static_cast<int>(F), mi = static_cast<int>(m);
    if (F <= kNarrowF) {
        const dim3 grid(static_cast<unsigned>(ceil_div(n_rows, 4)));
        if (F <= 64) hipLaunchKernelGGL(k_shuffle_narrow<1>, grid, dim3(256), 0, st, x, ldx, n_rows, Fi, mi, seed, out, ldo);
        else if (F <= 128) hipLaunchKernelGGL(k_shuffle_narrow<2>, grid, dim3(256), 0, st, x, ldx, n_rows, Fi, mi, seed, out, ldo);
        else if (F <= 192) hipLaunchKernelGGL(k_shuffle_narrow<3>, grid, dim3(256), 0, st, x, ldx, n_rows, Fi, mi, seed, out, ldo);
        else hipLaunchKernelGGL(k_shuffle_narrow<4>, grid, dim3(256), 0, st, x, ldx, n_rows, Fi, mi, seed, out, ldo);
        return launch_status();
    }
    const size_t lds = (sizeof(uint16_t) * static_cast<size_t>(m) + 15) & ~static_cast<size_t>(15);
    if (lds > 48 * 1024)
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(k_shuffle_wide),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, 144 * 1024);
    hipLaunchKernelGGL(k_shuffle_wide, dim3(static_cast<unsigned>(n_rows)), dim3(256), lds, st, x, ldx, Fi,
                       mi, seed, out, ldo);
    return launch_status();
}

extern "C" size_t ngnn_contrast_workspace_bytes(int64_t M) {
    return M > 0 ? sizeof(double) * 2 * static_cast<size_t>(M) + 256 : 0;
}

extern "C" int ngnn_contrast_fwd(const float *h, int64_t ldh, const float *hp, int64_t ldp,
                                 const float *hn, int64_t ldn, int64_t n_rows, int64_t F,
                                 const int64_t *idx, int64_t M, float *out, int32_t *bad, void *ws,
                                 size_t ws_bytes, void *stream) {
    NGNN_RETURN_IF(!h || !hp || !hn || !idx || !out || !ws, NGNN_E_ARG);
    NGNN_RETURN_IF(n_rows <= 0 || F <= 0 || M <= 0, NGNN_E_ARG);
    NGNN_RETURN_IF(ldh < F || ldp < F || ldn < F, NGNN_E_SHAPE);
    NGNN_RETURN_IF(!fits_i32(n_rows) || !fits_i32(F) || !fits_i32(M), NGNN_E_RANGE);
    NGNN_RETURN_IF(ws_bytes < ngnn_contrast_workspace_bytes(M) || !aligned(ws, 16), NGNN_E_WORKSPACE);
    double *w = static_cast<double *>(ws);
    hipStream_t st = as_stream(stream);
    launch_rows(k_contrast_rows, M, st, h, ldh, hp, ldp, hn, ldn, n_rows, (int)F, idx, (int)M, w, bad);
    int rc = launch_status();
    if (rc) return rc;
    hipLaunchKernelGGL(k_contrast_sum, dim3(1), dim3(256), 0, st, w, (int)M, out);
    return launch_status();
}

extern "C" int ngnn_contrast_bwd(const float *h, int64_t ldh, const float *hp, int64_t ldp,
                                 const float *hn, int64_t ldn, int64_t n_rows, int64_t F,
                                 const int64_t *idx, int64_t M, const void *ws, const float *grad_scale,
                                 float *dh, int64_t lddh, float *dhp, int64_t lddp, float *dhn,
                                 int64_t lddn, void *stream) {
    NGNN_RETURN_IF(!h || !hp || !hn || !idx || !ws || !grad_scale, NGNN_E_ARG);
    NGNN_RETURN_IF(n_rows <= 0 || F <= 0 || M <= 0, NGNN_E_ARG);
    NGNN_RETURN_IF(ldh < F || ldp < F || ldn < F, NGNN_E_SHAPE);
    NGNN_RETURN_IF((dh && lddh < F) || (dhp && lddp < F) || (dhn && lddn < F), NGNN_E_SHAPE);
    NGNN_RETURN_IF(!fits_i32(n_rows) || !fits_i32(F) || !fits_i32(M), NGNN_E_RANGE);
    if (!dh && !dhp && !dhn) return NGNN_OK;
    launch_rows(k_contrast_bwd, M, as_stream(stream), h, ldh, hp, ldp, hn, ldn, n_rows, (int)F, idx, (int)M,
                static_cast<const double *>(ws), grad_scale, dh, lddh, dhp, lddp, dhn, lddn);
    return launch_status();
}
