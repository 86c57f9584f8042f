// Seed-row cross entropy for the training step: the loss the reference's
// loop takes on the first batch_size rows of the SAGE output
// (pipeline.py:158, F.cross_entropy(out[:batch_size], y[:batch_size])
// [ext: torch]), as two launches instead of the ~9 of softmax / nll /
// slice-backward / fills.
//
// forward : loss = sum_{r<B, y_r != ignore} (lse(x_r) - x_r[y_r]) / #valid
//           one wave per row, then one workgroup adds the row losses in a
//           fixed order (second launch) -> deterministic.
// backward: d x_r[c] = g (softmax(x_r)[c] - [c == y_r]) / #valid for r < B,
//           0 for ignored rows; rows >= B are not written (the caller keeps
//           them zero).  One wave per row.
#include "ngnn_rows.h"

namespace ngnn {
namespace {

// the one-launch forward + gradient recounts the labels per workgroup
// (B^2 / 4 reads): above this many seed rows the O(B) three-launch path
constexpr int64_t kXentFusedMaxB = 4096;

// one wave per row: ws[r] = row loss (0 if ignored), ws[B + r] = 1/0 valid
__global__ __launch_bounds__(256) void k_xent_rows(const float *__restrict__ x, int64_t ld, int B,
                                                   int C, const int64_t *__restrict__ y,
                                                   int64_t ignore, float *__restrict__ ws) {
    const int lane = wave_lane(), r = wave_row();
    if (r >= B) return;
    const int64_t t = y[r];
    float l = 0.0f, v = 0.0f;
    if (t != ignore) {
        const float *xr = x + static_cast<int64_t>(r) * ld;
        const float lse = row_lse(xr, C, lane);
        l = row_nll(xr, lse, t, C);
        v = 1.0f;
    }
    if (lane == 0) {
        ws[r] = l;
        ws[B + r] = v;
    }
}

// one workgroup adds the row losses in a fixed order (strided per thread,
// then a fixed tree) -> deterministic; a separate launch, so no cross-XCD
// fences or tickets are needed
__global__ __launch_bounds__(256) void k_xent_sum(const float *__restrict__ ws, int B,
                                                  float *__restrict__ loss,
                                                  float *__restrict__ count) {
    __shared__ float tree[2][256];
    float t[2];  // loss sum, valid rows
    block_sum(tree, t, B, [&](int i, float(&a)[2]) {
        a[0] += ws[i];
        a[1] += ws[B + i];
    });
    if (threadIdx.x == 0) {
        *loss = t[0] / t[1];  // 0/0 = NaN when every row is ignored, as torch
        *count = t[1];
    }
}

__global__ __launch_bounds__(256) void k_xent_bwd(const float *__restrict__ x, int64_t ld, int B,
                                                  int C, const int64_t *__restrict__ y,
                                                  int64_t ignore, const float *__restrict__ ws,
                                                  const float *__restrict__ g,
                                                  const float *__restrict__ count,
                                                  float *__restrict__ dx, int64_t ldd) {
    const int lane = wave_lane(), r = wave_row();
    if (r >= B) return;
    const float *xr = x + static_cast<int64_t>(r) * ld;
    float *dr = dx + static_cast<int64_t>(r) * ldd;
    const int64_t t = y[r];
    if (t == ignore) {
        for (int c = lane; c < C; c += 64) dr[c] = 0.0f;
        return;
    }
    // recomputed rather than read back from ws: another forward on the same
    // workspace (two losses per step, co-teaching) may have overwritten it
    (void)ws;
    const float lse = row_lse(xr, C, lane);
    const float scale = (g ? *g : 1.0f) / *count;  // (g NULL: the unit scale of loss.backward())
    for (int c = lane; c < C; c += 64) {
        const float p = expf(xr[c] - lse);
        dr[c] = scale * (p - (c == t ? 1.0f : 0.0f));
    }
}

// forward AND the unit-scale gradient in ONE launch (the training step's
// loss.backward(1) needs nothing else): every workgroup counts the valid
// labels of y[0..B) itself (B int64 reads from L2: no count pass), each wave
// takes one row -- its loss and its gradient row (softmax - onehot) / count
// (zeros for an ignored row) -- the workgroup adds its rows' losses in wave
// order, and the LAST workgroup to finish (a device ticket) adds the
// workgroup sums in a fixed order: loss = sum / count, deterministic.
// ws: partial sums [gridDim.x] floats; ticket (uint32, zero between calls).
// Every workgroup reads all B labels, so the count costs B^2 / 4 label reads
// in all: the host takes this kernel only for B <= kXentFusedMaxB (the
// training step's seed rows) and the three-launch O(B) path above it.
// The hand-off is the measured gfx950 form of MI355X_MICROARCH.md ("Valid
// forms", first table row): every partial an agent-scope (sc1) store drained
// by s_waitcnt vmcnt(0) before ONE agent-scope atomic add per workgroup, the
// last adder reads every partial with agent-scope (sc1) loads.  It leans on
// gfx9's vmcnt counting stores and on sc1 codegen, hence the target check.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "k_xent_fused's fence-free hand-off is verified for gfx950 only"
#endif
__global__ __launch_bounds__(256) void k_xent_fused(const float *__restrict__ x, int64_t ld, int B,
                                                    int C, const int64_t *__restrict__ y,
                                                    int64_t ignore, float *__restrict__ part,
                                                    uint32_t *__restrict__ ticket,
                                                    float *__restrict__ loss,
                                                    float *__restrict__ count,
                                                    float *__restrict__ dx, int64_t ldd) {
    __shared__ float s_red[1][256];
    __shared__ float s_row[4];
    __shared__ int s_last;
    const int lane = wave_lane(), wv = threadIdx.x >> 6;
    float red[1];
    block_sum(s_red, red, B, [&](int i, float(&a)[1]) { a[0] += (y[i] != ignore) ? 1.0f : 0.0f; });
    const float cnt = red[0];
    const int r = wave_row();
    float l = 0.0f;
    if (r < B) {
        const float *xr = x + static_cast<int64_t>(r) * ld;
        float *dr = dx + static_cast<int64_t>(r) * ldd;
        const int64_t t = y[r];
        if (t == ignore) {
            for (int c = lane; c < C; c += 64) dr[c] = 0.0f;
        } else {
            const float lse = row_lse(xr, C, lane);
            l = row_nll(xr, lse, t, C);
            for (int c = lane; c < C; c += 64)
                dr[c] = (expf(xr[c] - lse) - (c == t ? 1.0f : 0.0f)) / cnt;
        }
    }
    if (lane == 0) s_row[wv] = l;
    __syncthreads();
    if (threadIdx.x == 0) {
        // hand-off without fences (MI355X_MICROARCH.md, inter-workgroup
        // visibility): the partial goes out as an agent-scope (sc1,
        // write-through) store, drained before the ticket; the last workgroup
        // reads every partial with agent-scope (sc1) loads.  (An agent fence
        // pair -- L2 write-back + invalidate -- cost ~10 us here.)
        __hip_atomic_store(part + blockIdx.x, ((s_row[0] + s_row[1]) + s_row[2]) + s_row[3],
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        s_last = atomicAdd(ticket, 1u) == gridDim.x - 1;
    }
    __syncthreads();
    if (!s_last) return;
    // (s_red again: the two barriers above separate it from cnt's read)
    block_sum(s_red, red, static_cast<int>(gridDim.x), [&](int i, float(&a)[1]) {
        a[0] += __hip_atomic_load(part + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    });
    if (threadIdx.x == 0) {
        *loss = red[0] / cnt;  // 0/0 = NaN when every row is ignored, as torch
        *count = cnt;
        *ticket = 0u;
    }
}

// ---------------------------------------------------------------------------
// Co-teaching loss (CTLoss.forward, losses.py:19-49) on the device.  The
// reference takes each model's per-row cross entropy, np.argsort's it on the
// host (two device->host syncs per batch), keeps the num_remember smallest
// rows of each model and trains each model on the rows the OTHER model kept.
//
// ws (floats): l[2][B] row losses, v[2][B] valid flags, sel[2][B] "row gets
// gradient" flags, cnt[2] selected valid rows per model.
// Sort order: ascending loss, ties by row index (np.argsort's default
// quicksort leaves tie order unspecified; NaN sorts last, as numpy).

constexpr int kCtMaxB = 8192;  // bitonic sort of 64-bit keys in 64 KiB of LDS

__global__ __launch_bounds__(256) void k_ct_rows(const float *__restrict__ y1, int64_t ld1,
                                                 const float *__restrict__ y2, int64_t ld2, int B,
                                                 int C, const int64_t *__restrict__ t,
                                                 int64_t ignore, float *__restrict__ ws) {
    const int lane = wave_lane(), g = wave_row();
    if (g >= 2 * B) return;
    const int m = g >= B, r = g - m * B;
    const float *xr = (m ? y2 : y1) + static_cast<int64_t>(r) * (m ? ld2 : ld1);
    const int64_t c = t[r];
    float l = 0.0f, v = 0.0f;
    if (c != ignore) {
        const float lse = row_lse(xr, C, lane);
        l = row_nll(xr, lse, c, C);
        v = 1.0f;
    }
    if (lane == 0) {
        ws[m * B + r] = l;
        ws[2 * B + m * B + r] = v;
    }
}

// ascending losses by their bits (-0 before +0), NaN last.  (ngnn_metrics'
// argmax_order_key makes -0 == +0, as torch.argmax compares: not this one)
__device__ __forceinline__ uint32_t loss_order_key(float f) {
    if (f != f) return 0xffffffffu;
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// workgroup m sorts model m's selection keys skey[m][B] (CTLoss: its row
// losses, ws itself; CoDiLoss: CE - co_lambda * JS); selects, for the OTHER
// model o, the rows model m keeps: loss_o = mean CE of model o over them;
// pure_m = mean noise_or_not[ind[kept_m]]
__global__ __launch_bounds__(1024) void k_ct_select(float *__restrict__ ws,
                                                    const float *__restrict__ skey, int B, int R,
                                                    const int64_t *__restrict__ ind,
                                                    const uint8_t *__restrict__ clean,
                                                    int64_t n_clean, int64_t *__restrict__ ind1,
                                                    int64_t *__restrict__ ind2,
                                                    float *__restrict__ out,
                                                    int *__restrict__ err) {
    __shared__ uint64_t key[kCtMaxB];
    __shared__ float tree[3][1024];
    const int m = blockIdx.x, o = 1 - m, tid = threadIdx.x;
    int P = 1;
    while (P < B) P <<= 1;
    const float *l = skey + m * B;
    for (int i = tid; i < P; i += 1024)
        key[i] = i < B ? (static_cast<uint64_t>(loss_order_key(l[i])) << 32) | static_cast<uint32_t>(i)
                       : ~0ull;
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P; i += 1024) {
                const int p = i ^ j;
                if (p > i) {
                    const uint64_t a = key[i], b = key[p];
                    const bool up = (i & k) == 0;
                    if ((a > b) == up) {
                        key[i] = b;
                        key[p] = a;
                    }
                }
            }
            __syncthreads();
        }
    }
    int64_t *im = m ? ind2 : ind1;
    for (int i = tid; i < B; i += 1024) im[i] = static_cast<int64_t>(key[i] & 0xffffffffu);
    float *sel = ws + 4 * B + o * B;  // rows of model o that receive gradient
    for (int i = tid; i < B; i += 1024) sel[i] = 0.0f;
    __syncthreads();
    const float *lo = ws + o * B, *vo = ws + 2 * B + o * B;
    float t[3];  // model o's loss sum and valid rows over the kept rows, model m's clean rows
    int bad = 0;
    block_sum(tree, t, R, [&](int j, float(&a)[3]) {
        const int r = static_cast<int>(key[j] & 0xffffffffu);
        sel[r] = 1.0f;
        a[0] += lo[r];  // ignored rows hold 0
        a[1] += vo[r];
        if (clean) {
            const int64_t g = ind ? ind[r] : r;
            if (g < 0 || g >= n_clean) bad = 1;
            else a[2] += clean[g] ? 1.0f : 0.0f;
        }
    });
    if (bad) atomicOr(err, 1);
    if (tid == 0) {
        out[o] = t[0] / t[1];                       // 0/0 = NaN, as torch's empty mean
        out[2 + m] = clean ? t[2] / static_cast<float>(R) : NAN;
        ws[6 * B + o] = t[1];
    }
}

// d y_m[r] = g / cnt_m (softmax(y_m[r]) - onehot) for the rows the other
// model selected, 0 elsewhere (rows [0, B) all written)
__global__ __launch_bounds__(256) void k_ct_bwd(const float *__restrict__ y, int64_t ld, int B, int C,
                                                const int64_t *__restrict__ t, int64_t ignore,
                                                const float *__restrict__ ws, int m,
                                                const float *__restrict__ g, float *__restrict__ dy,
                                                int64_t ldd) {
    const int lane = wave_lane(), r = wave_row();
    if (r >= B) return;
    const float *xr = y + static_cast<int64_t>(r) * ld;
    float *dr = dy + static_cast<int64_t>(r) * ldd;
    const int64_t c = t[r];
    if (ws[4 * B + m * B + r] == 0.0f || c == ignore) {
        for (int k = lane; k < C; k += 64) dr[k] = 0.0f;
        return;
    }
    const float lse = row_lse(xr, C, lane);
    const float scale = *g / ws[6 * B + m];
    for (int k = lane; k < C; k += 64) {
        const float p = expf(xr[k] - lse);
        dr[k] = scale * (p - (k == c ? 1.0f : 0.0f));
    }
}

// ---------------------------------------------------------------------------
// CoDi loss (CoDiLoss.forward, losses.py:106-137): CTLoss's exchange with the
// selection key CE - co_lambda * JS(y_1, y_2), JS detached.  One wave takes
// row r of BOTH models (the JS term needs both softmaxes):
//   js[r] = sum_k mean_k (log mean_k - (lp_k + lq_k) / 2),
//   mean = (softmax y_1 + softmax y_2) / 2  (js_loss_compute: kl_div with
//   target mean on both sides; a term with mean_k == 0 is 0, xlogy's rule).
// ws: CTLoss's layout (l, v, sel, cnt -- k_ct_bwd reads it as is), then the
// keys key[2][B] from float 6 B + 4 on.
__global__ __launch_bounds__(256) void k_codi_rows(const float *__restrict__ y1, int64_t ld1,
                                                   const float *__restrict__ y2, int64_t ld2, int B,
                                                   int C, const int64_t *__restrict__ t,
                                                   int64_t ignore, float co_lambda,
                                                   float *__restrict__ ws, float *__restrict__ skey,
                                                   float *__restrict__ js_out) {
    const int lane = wave_lane(), r = wave_row();
    if (r >= B) return;
    const float *a = y1 + static_cast<int64_t>(r) * ld1;
    const float *b = y2 + static_cast<int64_t>(r) * ld2;
    const float lse1 = row_lse(a, C, lane), lse2 = row_lse(b, C, lane);
    float js = 0.0f;
    for (int k = lane; k < C; k += 64) {
        const float lp = a[k] - lse1, lq = b[k] - lse2;
        const float mean = 0.5f * (expf(lp) + expf(lq));
        // (mean == 0: 0, not 0 * -inf; a NaN mean stays NaN)
        if (mean != 0.0f) js += mean * (logf(mean) - 0.5f * (lp + lq));
    }
    js = wave_sum(js);
    const int64_t c = t[r];
    float l1 = 0.0f, l2 = 0.0f, v = 0.0f;
    if (c != ignore) {
        l1 = row_nll(a, lse1, c, C);
        l2 = row_nll(b, lse2, c, C);
        v = 1.0f;
    }
    if (lane == 0) {
        ws[r] = l1;
        ws[B + r] = l2;
        ws[2 * B + r] = v;
        ws[3 * B + r] = v;
        skey[r] = l1 - co_lambda * js;
        skey[B + r] = l2 - co_lambda * js;
        if (js_out) js_out[r] = js;
    }
}

// ---------------------------------------------------------------------------
// Backward loss correction (backward_correction, losses.py:51-70):
//   loss = -(1 / (B C)) sum_r sum_k w_r[k] log q_rk,  w_r = Cinv[y_r],
//   q = clamp(softmax(x_r), 1e-5, 1 - 1e-5)
//   d x_rj = -(g / (B C)) (w_rj m_rj - p_rj sum_k w_rk m_rk),
//   m_rk = [1e-5 <= p_rk <= 1 - 1e-5]  (clamp's gradient: closed interval)
// One wave per row; part[r] = sum_k w_r[k] log q_rk (forward only), dx row r
// (when dx is given; g NULL: unit scale).  A label outside [0, C) reads no
// Cinv row: its partial and its gradient row are NaN.
// (torch rounds clamp's double bounds to the tensor's float once)
constexpr float kBcLo = static_cast<float>(1e-5), kBcHi = static_cast<float>(1.0 - 1e-5);

__global__ __launch_bounds__(256) void k_bc_rows(const float *__restrict__ x, int64_t ld, int B, int C,
                                                 const int64_t *__restrict__ y,
                                                 const float *__restrict__ cinv, int64_t ldc,
                                                 float *__restrict__ part, const float *__restrict__ g,
                                                 float *__restrict__ dx, int64_t ldd) {
    const int lane = wave_lane(), r = wave_row();
    if (r >= B) return;
    const float *xr = x + static_cast<int64_t>(r) * ld;
    const int64_t t = y[r];
    const bool ok = t >= 0 && t < C;
    const float *w = cinv + (ok ? t : 0) * ldc;
    const float lse = row_lse(xr, C, lane);
    float s = 0.0f, wm = 0.0f;
    for (int k = lane; k < C; k += 64) {
        const float p = expf(xr[k] - lse);
        const float wk = ok ? w[k] : NAN;
        s += wk * logf(p < kBcLo ? kBcLo : (p > kBcHi ? kBcHi : p));  // (a NaN passes, as clamp)
        if (p >= kBcLo && p <= kBcHi) wm += wk;
    }
    s = wave_sum(s);
    wm = wave_sum(wm);
    if (part && lane == 0) part[r] = s;
    if (!dx) return;
    float *dr = dx + static_cast<int64_t>(r) * ldd;
    const float scale = -(g ? *g : 1.0f) / (static_cast<float>(B) * static_cast<float>(C));
    for (int k = lane; k < C; k += 64) {
        const float p = expf(xr[k] - lse);
        const float wk = ok ? w[k] : NAN;
        dr[k] = scale * ((p >= kBcLo && p <= kBcHi ? wk : 0.0f) - p * wm);
    }
}

// one workgroup adds the row partials in a fixed order -> deterministic
__global__ __launch_bounds__(256) void k_bc_sum(const float *__restrict__ part, int B, int C,
                                                float *__restrict__ loss) {
    __shared__ float tree[1][256];
    float s[1];
    block_sum(tree, s, B, [&](int i, float(&a)[1]) { a[0] += part[i]; });
    if (threadIdx.x == 0) *loss = -s[0] / (static_cast<float>(B) * static_cast<float>(C));
}

}  // namespace
}  // namespace ngnn

using namespace ngnn;

extern "C" size_t ngnn_seed_xent_workspace_bytes(int64_t B) {
    return B > 0 ? sizeof(float) * 3 * static_cast<size_t>(B) + 256 : 0;
}

extern "C" int ngnn_seed_xent_fwd(const float *logits, int64_t ld, int64_t B, int64_t C,
                                  const int64_t *y, int64_t ignore_index, float *loss, float *count,
                                  void *ws, size_t ws_bytes, void *stream) {
    NGNN_RETURN_IF(!logits || !y || !loss || !count || !ws || B <= 0 || C <= 0, NGNN_E_ARG);
    NGNN_RETURN_IF(ld < C, NGNN_E_SHAPE);
    NGNN_RETURN_IF(!fits_i32(B) || !fits_i32(C), NGNN_E_RANGE);
    NGNN_RETURN_IF(ws_bytes < ngnn_seed_xent_workspace_bytes(B) || !aligned(ws, 16), NGNN_E_WORKSPACE);
    float *w = static_cast<float *>(ws);
    launch_rows(k_xent_rows, B, as_stream(stream), logits, ld, (int)B, (int)C, y, ignore_index, w);
    int rc = launch_status();
    if (rc) return rc;
    hipLaunchKernelGGL(k_xent_sum, dim3(1), dim3(256), 0, as_stream(stream), w, (int)B, loss, count);
    return launch_status();
}

extern "C" int ngnn_seed_xent_fwd_grad(const float *logits, int64_t ld, int64_t B, int64_t C,
                                       const int64_t *y, int64_t ignore_index, float *loss,
                                       float *count, float *dlogits, int64_t ldd, void *ws,
                                       size_t ws_bytes, void *stream) {
    NGNN_RETURN_IF(!logits || !y || !loss || !count || !dlogits || !ws || B <= 0 || C <= 0,
                   NGNN_E_ARG);
    NGNN_RETURN_IF(ld < C || ldd < C, NGNN_E_SHAPE);
    NGNN_RETURN_IF(!fits_i32(B) || !fits_i32(C), NGNN_E_RANGE);
    NGNN_RETURN_IF(ws_bytes < ngnn_seed_xent_workspace_bytes(B) || !aligned(ws, 16), NGNN_E_WORKSPACE);
    float *w = static_cast<float *>(ws);
    hipStream_t st = as_stream(stream);
    if (B > kXentFusedMaxB) {
        // large seed sets (a full-batch loader): rows, fixed-order sum, then the
        // gradient rows at unit scale -- O(B) label reads
        launch_rows(k_xent_rows, B, st, logits, ld, (int)B, (int)C, y, ignore_index, w);
        hipLaunchKernelGGL(k_xent_sum, dim3(1), dim3(256), 0, st, w, (int)B, loss, count);
        launch_rows(k_xent_bwd, B, st, logits, ld, (int)B, (int)C, y, ignore_index, w, nullptr, count, dlogits, ldd);
        return launch_status();
    }
    // the ticket sits past the row-loss area of ngnn_seed_xent_fwd (3 B floats)
    uint32_t *ticket = reinterpret_cast<uint32_t *>(w + 3 * B);
    launch_rows(k_xent_fused, B, st, logits, ld, (int)B, (int)C, y, ignore_index, w, ticket, loss, count,
                dlogits, ldd);
    return launch_status();
}

extern "C" int ngnn_seed_xent_bwd(const float *logits, int64_t ld, int64_t B, int64_t C,
                                  const int64_t *y, int64_t ignore_index, const void *ws,
                                  const float *grad_scale, const float *count, float *dlogits,
                                  int64_t ldd, void *stream) {
    NGNN_RETURN_IF(!logits || !y || !ws || !grad_scale || !count || !dlogits || B <= 0 || C <= 0,
                   NGNN_E_ARG);
    NGNN_RETURN_IF(ld < C || ldd < C, NGNN_E_SHAPE);
    NGNN_RETURN_IF(!fits_i32(B) || !fits_i32(C), NGNN_E_RANGE);
    launch_rows(k_xent_bwd, B, as_stream(stream), logits, ld, (int)B, (int)C, y, ignore_index,
                static_cast<const float *>(ws), grad_scale, count, dlogits, ldd);
    return launch_status();
}

extern "C" size_t ngnn_ct_loss_workspace_bytes(int64_t B) {
    return B > 0 ? sizeof(float) * (6 * static_cast<size_t>(B) + 2) + sizeof(int) + 256 : 0;
}

extern "C" int ngnn_ct_loss_fwd(const float *y1, int64_t ld1, const float *y2, int64_t ld2, int64_t B,
                                int64_t C, const int64_t *y_noise, int64_t ignore_index,
                                int64_t num_remember, const int64_t *ind, const uint8_t *noise_or_not,
                                int64_t n_noise, float *out, int64_t *ind1_sorted,
                                int64_t *ind2_sorted, void *ws, size_t ws_bytes, int *err,
                                void *stream) {
    NGNN_RETURN_IF(!y1 || !y2 || !y_noise || !out || !ind1_sorted || !ind2_sorted || !ws || !err,
                   NGNN_E_ARG);
    NGNN_RETURN_IF(B <= 0 || C <= 0 || num_remember < 0 || num_remember > B, NGNN_E_ARG);
    NGNN_RETURN_IF(noise_or_not && n_noise <= 0, NGNN_E_ARG);
    NGNN_RETURN_IF(ld1 < C || ld2 < C || B > kCtMaxB, NGNN_E_SHAPE);
    NGNN_RETURN_IF(!fits_i32(C), NGNN_E_RANGE);
    NGNN_RETURN_IF(ws_bytes < ngnn_ct_loss_workspace_bytes(B) || !aligned(ws, 16), NGNN_E_WORKSPACE);
    float *w = static_cast<float *>(ws);
    hipStream_t st = as_stream(stream);
    launch_rows(k_ct_rows, 2 * B, st, y1, ld1, y2, ld2, (int)B, (int)C, y_noise, ignore_index, w);
    int rc = launch_status();
    if (rc) return rc;
    hipLaunchKernelGGL(k_ct_select, dim3(2), dim3(1024), 0, st, w, w, (int)B, (int)num_remember, ind,
                       noise_or_not, n_noise, ind1_sorted, ind2_sorted, out, err);
    return launch_status();
}

extern "C" int ngnn_ct_loss_bwd(int model, const float *y, int64_t ld, int64_t B, int64_t C,
                                const int64_t *y_noise, int64_t ignore_index, const void *ws,
                                const float *grad, float *dy, int64_t ldd, void *stream) {
    NGNN_RETURN_IF(model < 0 || model > 1 || !y || !y_noise || !ws || !grad || !dy, NGNN_E_ARG);
    NGNN_RETURN_IF(B <= 0 || C <= 0, NGNN_E_ARG);
    NGNN_RETURN_IF(ld < C || ldd < C || B > kCtMaxB, NGNN_E_SHAPE);
    NGNN_RETURN_IF(!fits_i32(C), NGNN_E_RANGE);
    launch_rows(k_ct_bwd, B, as_stream(stream), y, ld, (int)B, (int)C, y_noise, ignore_index,
                static_cast<const float *>(ws), model, grad, dy, ldd);
    return launch_status();
}

extern "C" size_t ngnn_codi_loss_workspace_bytes(int64_t B) {
    return B > 0 ? sizeof(float) * (8 * static_cast<size_t>(B) + 4) + 256 : 0;
}

extern "C" int ngnn_codi_loss_fwd(const float *y1, int64_t ld1, const float *y2, int64_t ld2, int64_t B,
                                  int64_t C, const int64_t *y_noise, int64_t ignore_index,
                                  int64_t num_remember, float co_lambda, const int64_t *ind,
                                  const uint8_t *noise_or_not, int64_t n_noise, float *out,
                                  int64_t *ind1_sorted, int64_t *ind2_sorted, float *js_out, void *ws,
                                  size_t ws_bytes, int *err, void *stream) {
    NGNN_RETURN_IF(!y1 || !y2 || !y_noise || !out || !ind1_sorted || !ind2_sorted || !ws || !err,
                   NGNN_E_ARG);
    NGNN_RETURN_IF(B <= 0 || C <= 0 || num_remember < 0 || num_remember > B, NGNN_E_ARG);
    NGNN_RETURN_IF(noise_or_not && n_noise <= 0, NGNN_E_ARG);
    NGNN_RETURN_IF(ld1 < C || ld2 < C || B > kCtMaxB, NGNN_E_SHAPE);
    NGNN_RETURN_IF(!fits_i32(C), NGNN_E_RANGE);
    NGNN_RETURN_IF(ws_bytes < ngnn_codi_loss_workspace_bytes(B) || !aligned(ws, 16), NGNN_E_WORKSPACE);
    float *w = static_cast<float *>(ws);
    float *skey = w + 6 * B + 4;
    // an empty selection keeps every row (losses.py:125-128)
    const int R = static_cast<int>(num_remember == 0 ? B : num_remember);
    hipStream_t st = as_stream(stream);
    launch_rows(k_codi_rows, B, st, y1, ld1, y2, ld2, (int)B, (int)C, y_noise, ignore_index, co_lambda, w, skey,
                js_out);
    int rc = launch_status();
    if (rc) return rc;
    hipLaunchKernelGGL(k_ct_select, dim3(2), dim3(1024), 0, st, w, skey, (int)B, R, ind, noise_or_not,
                       n_noise, ind1_sorted, ind2_sorted, out, err);
    return launch_status();
}

extern "C" int ngnn_codi_loss_bwd(int model, const float *y, int64_t ld, int64_t B, int64_t C,
                                  const int64_t *y_noise, int64_t ignore_index, const void *ws,
                                  const float *grad, float *dy, int64_t ldd, void *stream) {
    // JS is detached: CTLoss's backward on the rows the other model kept
    return ngnn_ct_loss_bwd(model, y, ld, B, C, y_noise, ignore_index, ws, grad, dy, ldd, stream);
}

extern "C" size_t ngnn_bc_loss_workspace_bytes(int64_t B) {
    return B > 0 ? sizeof(float) * static_cast<size_t>(B) + 256 : 0;
}

extern "C" int ngnn_bc_loss_fwd(const float *logits, int64_t ld, int64_t B, int64_t C,
                                const int64_t *labels, const float *Cinv, int64_t ldc, float *loss,
                                float *dlogits, int64_t ldd, void *ws, size_t ws_bytes, void *stream) {
    NGNN_RETURN_IF(!logits || !labels || !Cinv || !loss || !ws || B <= 0 || C <= 0, NGNN_E_ARG);
    NGNN_RETURN_IF(ld < C || ldc < C || (dlogits && ldd < C), NGNN_E_SHAPE);
    NGNN_RETURN_IF(!fits_i32(B) || !fits_i32(C), NGNN_E_RANGE);
    NGNN_RETURN_IF(ws_bytes < ngnn_bc_loss_workspace_bytes(B) || !aligned(ws, 16), NGNN_E_WORKSPACE);
    float *w = static_cast<float *>(ws);
    hipStream_t st = as_stream(stream);
    launch_rows(k_bc_rows, B, st, logits, ld, (int)B, (int)C, labels, Cinv, ldc, w, nullptr, dlogits, ldd);
    int rc = launch_status();
    if (rc) return rc;
    hipLaunchKernelGGL(k_bc_sum, dim3(1), dim3(256), 0, st, w, (int)B, (int)C, loss);
    return launch_status();
}

extern "C" int ngnn_bc_loss_bwd(const float *logits, int64_t ld, int64_t B, int64_t C,
                                const int64_t *labels, const float *Cinv, int64_t ldc,
                                const float *grad_scale, float *dlogits, int64_t ldd, void *stream) {
    NGNN_RETURN_IF(!logits || !labels || !Cinv || !grad_scale || !dlogits || B <= 0 || C <= 0,
                   NGNN_E_ARG);
    NGNN_RETURN_IF(ld < C || ldc < C || ldd < C, NGNN_E_SHAPE);
    NGNN_RETURN_IF(!fits_i32(B) || !fits_i32(C), NGNN_E_RANGE);
    launch_rows(k_bc_rows, B, as_stream(stream), logits, ld, (int)B, (int)C, labels, Cinv, ldc, nullptr,
                grad_scale, dlogits, ldd);
    return launch_status();
}
