// The uncertainty-weighted consistency term of the reference's train_ct step
// (pipeline_ctp.py:127-135): get_uncertainty_batch (losses.py:185-204) and
// fix_cr (losses.py:206-246) on log-probabilities, fp32.
//
// ngnn_nbr_uncertainty: one wave per output row i < R, lanes over the
//   classes (a chunk loop for C > 64).  With p = exp(logp):
//     s_i = sum_{e in list(i)} p[col[e]]   (list order, compensated fp32, no atomics)
//     ptc = s_i / (deg_i + epsilon);  h_i = -sum_k ptc_k log2(ptc_k + 1e-5)
//     w_i = exp(-h_i / log2(nbr_classes))
//   list(i) is row i of the by-source CSR (Block.transposed()).
// ngnn_fix_cr_fwd / _bwd: one wave per row r < B; the row terms go to the
//   workspace and one workgroup adds them in a fixed order (second launch),
//   as ngnn_bc_loss_fwd.  The backward recomputes from the inputs.
#include "ngnn_rows.h"

namespace ngnn {
namespace {

// (the reference adds the Python double 1e-5 to a float tensor: rounded once)
constexpr float kEntEps = static_cast<float>(1e-5);

__global__ __launch_bounds__(256) void k_nbr_unc(const float *__restrict__ logp, int64_t ld, int n_rows,
                                                 int C, const int32_t *__restrict__ rowptr,
                                                 const int32_t *__restrict__ col, int R, float lg,
                                                 float epsilon, float *__restrict__ w) {
    const int lane = wave_lane(), i = wave_row();
    if (i >= R) return;
    const int beg = rowptr[i], end = rowptr[i + 1];
    const float den = static_cast<float>(end - beg) + epsilon;
    float h = 0.0f;
    for (int c0 = 0; c0 < C; c0 += 64) {
        const int k = c0 + lane;
        const bool on = k < C;
        float s = 0.0f, comp = 0.0f;
        // 64 list entries per coalesced load, handed round by lane
        for (int base = beg; base < end; base += 64) {
            const int n = min(64, end - base);
            const int jv = lane < n ? col[base + lane] : 0;
            // an id outside the rows reads nothing and poisons the row (a lane
            // past C reads nothing either; its NaN is never looked at)
            auto term = [&](int t) -> float {
                const int j = __shfl(jv, t);
                const bool ok = on && static_cast<unsigned>(j) < static_cast<unsigned>(n_rows);
                return ok ? expf(logp[static_cast<int64_t>(j) * ld + k]) : NAN;
            };
            // compensated (Kahan): a plain fp32 running sum drifts by n/2 ulp
            // over a hub's list of near-equal terms (3e-5 of w at 3,000 entries)
            auto add = [&](float v) {
                const float y = v - comp;
                const float u = s + y;
                comp = (u - s) - y;
                s = u;
            };
            int t = 0;
            for (; t + 4 <= n; t += 4) {  // four loads in flight, a fixed order within the list
                const float a = term(t), b = term(t + 1), c = term(t + 2), d = term(t + 3);
                add((a + b) + (c + d));
            }
            for (; t < n; ++t) add(term(t));
        }
        if (on) {
            const float ptc = s / den;
            h -= ptc * log2f(ptc + kEntEps);
        }
    }
    h = wave_sum(h);
    if (lane == 0) w[i] = expf(-h / lg);
}

// torch.max's order over (value, index): a NaN beats every number, the first
// index wins among equals
__device__ __forceinline__ bool beats(float v, int i, float bv, int bi) {
    const bool vn = v != v, bn = bv != bv;
    if (vn != bn) return vn;
    if (vn) return i < bi;
    return v > bv || (v == bv && i < bi);
}

constexpr int kHard = 0, kL2 = 2;  // (1: soft labels)

// part (forward only): the row's term of the sum; d_pure / d_noisy (when
// given): the gradient rows for *g (g NULL: unit scale)
__global__ __launch_bounds__(256) void k_fixcr_rows(const float *__restrict__ yp, int64_t ldp,
                                                    const float *__restrict__ yn, int64_t ldn, int B,
                                                    int C, int mode, float p_cutoff,
                                                    const float *__restrict__ w,
                                                    float *__restrict__ part, const float *__restrict__ g,
                                                    float *__restrict__ dp, int64_t lddp,
                                                    float *__restrict__ dn, int64_t lddn) {
    const int lane = wave_lane(), r = wave_row();
    if (r >= B) return;
    const float *ypr = yp + static_cast<int64_t>(r) * ldp;
    const float *ynr = yn + static_cast<int64_t>(r) * ldn;
    float *dpr = dp ? dp + static_cast<int64_t>(r) * lddp : nullptr;
    float *dnr = dn ? dn + static_cast<int64_t>(r) * lddn : nullptr;
    const float gs = g ? *g : 1.0f;
    if (mode == kL2) {
        float s = 0.0f;
        for (int k = lane; k < C; k += 64) {
            const float d = ynr[k] - ypr[k];
            s += d * d;
        }
        s = wave_sum(s);
        if (part && lane == 0) part[r] = s;
        if (!dpr && !dnr) return;
        const float scale = 2.0f * gs / (static_cast<float>(B) * static_cast<float>(C));
        for (int k = lane; k < C; k += 64) {
            const float d = scale * (ynr[k] - ypr[k]);
            if (dnr) dnr[k] = d;
            if (dpr) dpr[k] = -d;
        }
        return;
    }
    // the pseudo label: max and first argmax of pp = exp(y_pure), and sum pp
    float bv = -INFINITY, spp = 0.0f;
    int bi = INT32_MAX;
    for (int k = lane; k < C; k += 64) {
        const float pp = expf(ypr[k]);
        spp += pp;
        if (beats(pp, k, bv, bi)) bv = pp, bi = k;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o);
        const int oi = __shfl_xor(bi, o);
        if (beats(ov, oi, bv, bi)) bv = ov, bi = oi;
    }
    spp = wave_sum(spp);
    const float m = bv >= p_cutoff ? 1.0f : 0.0f;  // (a NaN maximum: masked, as torch's ge)
    // the reference feeds the probabilities pn = exp(y_noisy) to
    // cross_entropy as logits: log-sum-exp over pn
    float mx = -INFINITY;
    for (int k = lane; k < C; k += 64) mx = fmaxf(mx, expf(ynr[k]));
    mx = wave_maxf(mx);
    float se = 0.0f;
    for (int k = lane; k < C; k += 64) se += expf(expf(ynr[k]) - mx);  // a NaN anywhere: NaN
    se = wave_sum(se);
    const float lse = mx + logf(se);
    const float wr = w ? w[r] : 1.0f;
    if (part) {
        float l;
        if (mode == kHard) {
            l = lse - expf(ynr[bi]);
        } else {
            float a = 0.0f;
            for (int k = lane; k < C; k += 64) a += expf(ypr[k]) * (expf(ynr[k]) - lse);
            l = -wave_sum(a);
        }
        // the mask multiplies: a NaN row term stays NaN when masked out
        if (lane == 0) part[r] = wr * (l * m);
    }
    if (!dpr && !dnr) return;
    const float c = gs * m * wr / static_cast<float>(B);
    for (int k = lane; k < C; k += 64) {
        const float pn = expf(ynr[k]);
        const float sk = expf(pn - lse);
        if (mode == kHard) {
            if (dnr) dnr[k] = c * (sk - (k == bi ? 1.0f : 0.0f)) * pn;
            if (dpr) dpr[k] = 0.0f;
        } else {
            const float pp = expf(ypr[k]);
            if (dnr) dnr[k] = c * (sk * spp - pp) * pn;
            if (dpr) dpr[k] = -c * pp * (pn - lse);
        }
    }
}

// one workgroup adds the row terms in a fixed order -> deterministic
__global__ __launch_bounds__(256) void k_fixcr_sum(const float *__restrict__ part, int B, float denom,
                                                   float *__restrict__ loss) {
    __shared__ float tree[1][256];
    float s[1];
    block_sum(tree, s, B, [&](int i, float(&a)[1]) { a[0] += part[i]; });
    if (threadIdx.x == 0) *loss = s[0] / denom;
}

constexpr int64_t kMaxC = 65535;

int fixcr_check(const float *lp_pure, int64_t ldp, const float *lp_noisy, int64_t ldn, int64_t B,
                int64_t C, int mode, const float *d_pure, int64_t lddp, const float *d_noisy,
                int64_t lddn) {
    NGNN_RETURN_IF(!lp_pure || !lp_noisy || B <= 0 || C <= 0 || mode < kHard || mode > kL2, NGNN_E_ARG);
    NGNN_RETURN_IF(ldp < C || ldn < C || (d_pure && lddp < C) || (d_noisy && lddn < C), NGNN_E_SHAPE);
    NGNN_RETURN_IF(!fits_i32(B) || C > kMaxC, NGNN_E_RANGE);
    return NGNN_OK;
}

}  // namespace
}  // namespace ngnn

using namespace ngnn;

extern "C" int ngnn_nbr_uncertainty(const float *logp, int64_t ld, int64_t n_rows, int64_t C,
                                    const int32_t *rowptr, const int32_t *col, int64_t R,
                                    int64_t nbr_classes, float epsilon, float *w, void *stream) {
    NGNN_RETURN_IF(n_rows < 0 || C < 0 || R < 0 || R > n_rows || nbr_classes < 2, NGNN_E_ARG);
    NGNN_RETURN_IF(ld < C, NGNN_E_SHAPE);
    NGNN_RETURN_IF(!fits_i32(n_rows) || !fits_i32(R) || C > kMaxC, NGNN_E_RANGE);
    if (R == 0) return NGNN_OK;
    // (col is read only where a list is not empty: a CSR without edges may pass NULL)
    NGNN_RETURN_IF(!logp || !rowptr || !w, NGNN_E_ARG);
    const float lg = log2f(static_cast<float>(nbr_classes));
    launch_rows(k_nbr_unc, R, as_stream(stream), logp, ld, (int)n_rows, (int)C, rowptr, col, (int)R, lg, epsilon, w);
    return launch_status();
}

extern "C" size_t ngnn_fix_cr_workspace_bytes(int64_t B) {
    return B > 0 ? sizeof(float) * static_cast<size_t>(B) + 256 : 0;
}

extern "C" int ngnn_fix_cr_fwd(const float *lp_pure, int64_t ldp, const float *lp_noisy, int64_t ldn,
                               int64_t B, int64_t C, int mode, float p_cutoff, const float *w, float *loss,
                               float *d_pure, int64_t lddp, float *d_noisy, int64_t lddn, void *ws,
                               size_t ws_bytes, void *stream) {
    NGNN_RETURN_IF(!loss || !ws, NGNN_E_ARG);
    int rc = fixcr_check(lp_pure, ldp, lp_noisy, ldn, B, C, mode, d_pure, lddp, d_noisy, lddn);
    if (rc) return rc;
    NGNN_RETURN_IF(ws_bytes < ngnn_fix_cr_workspace_bytes(B) || !aligned(ws, 16), NGNN_E_WORKSPACE);
    float *part = static_cast<float *>(ws);
    hipStream_t st = as_stream(stream);
    launch_rows(k_fixcr_rows, B, st, lp_pure, ldp, lp_noisy, ldn, (int)B, (int)C, mode, p_cutoff, w, part, nullptr,
                d_pure, lddp, d_noisy, lddn);
    rc = launch_status();
    if (rc) return rc;
    const float denom = mode == kL2 ? static_cast<float>(B) * static_cast<float>(C) : static_cast<float>(B);
    hipLaunchKernelGGL(k_fixcr_sum, dim3(1), dim3(256), 0, st, part, (int)B, denom, loss);
    return launch_status();
}

extern "C" int ngnn_fix_cr_bwd(const float *lp_pure, int64_t ldp, const float *lp_noisy, int64_t ldn,
                               int64_t B, int64_t C, int mode, float p_cutoff, const float *w,
                               const float *grad_scale, float *d_pure, int64_t lddp, float *d_noisy,
                               int64_t lddn, void *stream) {
    NGNN_RETURN_IF(!grad_scale, NGNN_E_ARG);
    int rc = fixcr_check(lp_pure, ldp, lp_noisy, ldn, B, C, mode, d_pure, lddp, d_noisy, lddn);
    if (rc) return rc;
    if (!d_pure && !d_noisy) return NGNN_OK;  // no gradient wanted: nothing to launch
    launch_rows(k_fixcr_rows, B, as_stream(stream), lp_pure, ldp, lp_noisy, ldn, (int)B, (int)C, mode, p_cutoff, w,
                nullptr, grad_scale, d_pure, lddp, d_noisy, lddn);
    return launch_status();
}
