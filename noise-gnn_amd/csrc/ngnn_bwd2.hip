// Backward of the two-layer forward (ngnn_sage2_fwd):
// every weight gradient of SAGE(K0 -> 256 -> F1) from the top-layer output
// gradient dy (rows < R, the seed rows the loss reads) in three launches.
//
// The reference's autograd (sage.py:33-39 under loss.backward(),
// pipeline.py:155-160) computes, per layer, dW_l = dz^T agg, dW_r = dz^T h_in,
// db = sum dz and the input gradient through the transposed aggregation.  For
// the top layer the aggregation is linear, so with g = the mean/sum
// aggregation of dy scattered onto its SOURCE rows (g[s] = sum_{d <- s} dy[d]
// / deg(d), rows < R'):
//
//     dW_l1 = g^T h         dW_r1 = dy^T h         db1 = sum dy
//     dh    = dy W_r1 + g W_l1              (rows < R'; the narrow form)
//     dz0   = dh * [h > 0] * 1/(1-p)        (ReLU + dropout backward)
//     dW_l0 = dz0^T agg0    dW_r0 = dz0^T x        db0 = sum dz0
//
// -- dW_l1 needs no rebuilt neighbour aggregate of h, and dh never leaves the
// chip.  Launches:
//   k_lowdim_scatter (ngnn_sage_bwd.hip)  g, float atomics (no image blocks);
//   k_bwd2  per 32-row chunk of rows < R' and 64 hidden columns: X = [dy | g]
//           and h / x / agg0 rows staged in LDS as two fp16 parts each;
//           dh = X [W_r1; W_l1] on MFMA, masked, split, exchanged between
//           the two row-tile waves; then dW_r0 / dW_l0 (A = dz0^T) and
//           [dW_r1; dW_l1] (A = X^T, B = h) on MFMA with transposed LDS reads
//           (ds_read_b64_tr_b16).  Partials per row slice -> slabs;
//   k_bwd2_reduce  fixed-order slab sums into the six gradients; clears g.
//
// Arithmetic (H2, as the forward; round 5): every operand is scaled by a power
// of two that puts its block's max |v| in [2^14, 2^15) and split into two fp16
// parts, v 2^e = v1 + v2 (+ r, |r| <= 2^-22 |v 2^e|); products a1 b1 + a1 b2 +
// a2 b1 on fp16 MFMAs (each exact in fp32, fp32 accumulation): ~3 2^-22
// relative per product, fp32-class (tests/gradbar.py: max|g - g_ref| <= 1e-5
// max|g_ref|; the round-4 two-part bf16 split, 2^-17, measured up to 1.1e-5).
// The weight-gradient products sum over ROWS, so a scale must be uniform over
// the rows of an MFMA: one scale per operand per 32-row chunk (its max over
// the chunk, found while the chunk's loads land: each wave's maxima go
// through LDS at the barrier that ends the previous chunk -- no barrier of
// its own); each chunk's products start from zero and are unscaled (v_ldexp,
// exact) into the fp32 accumulators.  dh = X W1 sums over F1, so its scales
// are X's chunk scale and the wave's W1 slice scale; dz0 is scaled by the
// bound 96 2^30 yscale of |dh| in those units (a constant shift, e_dz).
//
// Chunks and dy: dy is zero past the seed rows, so only the first ceil(R / 32)
// chunks (the seed chunks) hold any.  A row slice owns every S-th chunk (s,
// s + S, ...), which deals the seed chunks over the slices, and a chunk
// without dy skips the dy loads, their share of X's maximum, their split and
// LDS stores, db1's sum, stage B's dy-only k-chunk and the dW_r1 products.
//  * For finite inputs the skipping leaves every accumulator as it was: the
//    skipped products are exact zeros added to a +0 or non-zero sum, and X's
//    maximum is unchanged because dy was 0 there.
//  * The cyclic ownership changes which rows each slab sums, so the fp32
//    summation order differs from a contiguous split: rounding only, inside
//    the 1e-5 bars.  Two launches still agree bit for bit.
//  * Non-finite h or W_r1 against the zero dy of rows >= R no longer gives
//    NaN in dW_r1 or dh: those products are not formed.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <type_traits>

#include "ngnn_device.h"

namespace ngnn {

// the narrow scatter (ngnn_sage_bwd.hip): g[col[e]] += dy[d] (/ deg(d)) over
// target rows d < *r_ptr, C4 floats per g row, no weight-image blocks
int lowdim_scatter_launch(const float *dy, int64_t ldy, const int32_t *rowptr, const int32_t *col, int n_rows,
                          const int32_t *r_ptr, int Fo, int C4, float *g, int mean, hipStream_t st);

namespace {

typedef _Float16 bf8 __attribute__((ext_vector_type(8)));  // (fp16 parts; the names kept from the bf16 split)
typedef _Float16 bf4 __attribute__((ext_vector_type(4)));
typedef short s4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) _Float16 L16;  // an LDS fp16 (32-bit addresses)
constexpr int kOOB = static_cast<int>(0xF0000000u);  // past every buffer range (< 3.75 GiB)

constexpr int B2_ROWS = 32;            // rows per chunk: one 16x16x32 MFMA k-step
constexpr int B2_NC = 64;              // hidden columns per workgroup
constexpr int B2_NCH = 256 / B2_NC;    // workgroups per row slice
constexpr int B2_THREADS = 512;
// LDS row strides (bf16 elements): 56 / 40 / 72 dwords -- odd multiples of 8
// dwords, so a transposed read's 8 rows x 32 B land on disjoint banks
constexpr int XS = 112, HS = 80, KS = 144;
constexpr int IMG_X = 2 * B2_ROWS * XS;  // bf16 per image buffer (2 parts)
constexpr int IMG_H = 2 * B2_ROWS * HS;
constexpr int IMG_K = 2 * B2_ROWS * KS;
constexpr int SA = 4 * 2 * 64 * 8;       // dz0 A fragments: [n-tile 4][part 2][lane 64][8]
constexpr int BUF = IMG_X + IMG_H + 2 * IMG_K + SA;  // bf16 per pipeline buffer

struct B2Args {
    const float *dy;  // [*, ldy] rows < R
    int64_t ldy;
    int F1;
    const float *g;  // [n_rows][C4] rows < R' (zero past F1)
    int C4;
    const float *wr1, *wl1;  // [F1, 256]
    int64_t ldw1;
    const float *h;  // [*, ldh] rows < R'
    int64_t ldh;
    float yscale;
    int e_dz;  // dz0's fp16 scale: |dh| 2^(eX + eW) <= 96 2^30, times yscale, shifted by 2^-e_dz
    const float *x;
    const float *const *x_dev;
    const int64_t *xrow;
    const int64_t *const *xrow_dev;
    int64_t x_rows;
    int64_t ldx;
    int K0;
    const float *agg;  // [*, ld_agg] rows < R'
    int64_t ld_agg;
    const int32_t *rowptr;
    int n_rows;
    const int32_t *r_ptr, *rn_ptr;
    float *slab;  // [S][slab floats]
    int S;
    float *step_inc;  // nullable: the folded Adam step's count, advanced once here
    const uint64_t *gate;  // the graph slot's contract gate (ABI 20): no advance when gated
    const int64_t *gate_gen;
};

__host__ __device__ inline int64_t b2_slab_floats(int K0, int F1) {
    return 512LL * K0 + 256 + 512LL * F1 + F1;
}

// two fp16 parts (round to nearest even) of a scaled value
__device__ __forceinline__ void split2(float v, _Float16 &p1, _Float16 &p2) {
    p1 = static_cast<_Float16>(v);
    p2 = static_cast<_Float16>(v - static_cast<float>(p1));
}

__device__ __forceinline__ v4f mfma3(bf8 a1, bf8 a2, bf8 b1, bf8 b2, v4f acc) {  // smallest terms first
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a2, b1, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1, b2, acc, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a1, b1, acc, 0, 0, 0);
}

// transposed read: the 16-lane group q takes the 4 x 16 block at rows
// r0 + 4q .. + 3, columns c0 .. + 15 of a [rows][stride] bf16 image; lane i of
// the group receives column c0 + i of those rows (cdna_hip_programming.md T10)
__device__ __forceinline__ s4 tr_read(const L16 *img, int stride, int r0, int c0, int ln) {
    const int q = ln >> 4, i = ln & 15;
    const L16 *p = img + (r0 + 4 * q + (i >> 2)) * stride + c0 + 4 * (i & 3);
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4 *)(p));
}

// the MFMA operand over rows {4q .. 4q+3, 16+4q .. 16+4q+3} (the dz0
// fragments' k order) of columns c0 + (lane & 15)
__device__ __forceinline__ bf8 tr_frag(const L16 *img, int stride, int c0, int ln) {
    const s4 a = tr_read(img, stride, 0, c0, ln), b = tr_read(img, stride, 16, c0, ln);
    typedef short s8 __attribute__((ext_vector_type(8)));
    const s8 v{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
    return __builtin_bit_cast(bf8, v);
}

// an LDS-only workgroup barrier (ngnn_fwd2.hip): vector-memory loads in
// flight stay in flight -- __syncthreads() would drain vmcnt
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

__device__ __forceinline__ float sum_xor16(float v) {
    const int x = __float_as_int(v);
    const auto r = __builtin_amdgcn_permlane16_swap(x, x, false, false);
    return __int_as_float(static_cast<int>(r[0])) + __int_as_float(static_cast<int>(r[1]));
}
__device__ __forceinline__ float sum_xor32(float v) {
    const int x = __float_as_int(v);
    const auto r = __builtin_amdgcn_permlane32_swap(x, x, false, false);
    return __int_as_float(static_cast<int>(r[0])) + __int_as_float(static_cast<int>(r[1]));
}

// Workgroup = (row slice s, hidden chunk nc): 8 waves.  Stage B (dh): wave
// (rt = w >> 2, nt = w & 3) -> dh rows 16 rt .. + 15, columns 16 nt .. + 15 of
// the chunk.  Stage C0: wave (mat = w >> 2, nt) -> dW_r0 (mat 0, B = x) or
// dW_l0 (mat 1, B = agg0) rows n of tile nt, all K0 columns.  Stage C1: wave
// w -> tiles w, w + 8, w + 16 of the 24 [dW_r1; dW_l1] tiles (6 f-tiles x 4
// n-tiles): both kinds on every wave.
// KT: 16-column tiles of K0 computed (past K0 the images hold zeros)
// LAG: a chunk's maxima published at the barrier that ends the previous chunk
// (its loads waited for right after stage B) -- else after stage C, at a
// barrier of their own (the loads keep stage C to land)
// ROOT false (ABI 18, dW_r0 = dW_r1 = NULL: a SimpleGCN stack, whose root
// weights are zero): no x rows staged, no dW_r0 / dW_r1 products -- stage
// C0's dW_l0 tiles split over all eight waves, stage C1's W_l1 tiles over
// the eight, stage B skips the dy-only K chunk (its W_r1 rows are zero)
// DBG (profiling builds only, NGNN_B2_DBG_BUILD): bit 0 -- constant chunk
// scales, no maxima (wrong results: the time the chunk maxima cost)
template <bool XR, int KT, bool LAG, bool ROOT = true, int DBG = 0>
__global__ __launch_bounds__(B2_THREADS, 1) void k_bwd2(B2Args a) {
    extern __shared__ __attribute__((aligned(16))) __bf16 lb_[];
    L16 *lb = (L16 *)(lb_);  // (an address-space cast: the shared array IS in LDS)
    float *sred = reinterpret_cast<float *>(lb_ + 2 * BUF);  // [2][256] reductions at the end

    const int t = threadIdx.x;
    // (the folded Adam step: k_bwd2_reduce, the next launch, reads the
    // advanced count -- stream order, no ticket)
    if (a.step_inc && blockIdx.x == 0 && t == 0 && !slot_gated(a.gate, a.gate_gen))
        *a.step_inc = *a.step_inc + 1.0f;
    const int wv = __builtin_amdgcn_readfirstlane(t >> 6);
    const int ln = t & 63, q = ln >> 4, l16 = ln & 15;
    // block -> (slice, chunk): the 4 chunks of a slice on one XCD (blocks b,
    // b + 8 share one), so they share the slice's X / x / agg0 rows in L2
    const int bx = blockIdx.x;
    const int nc = (bx >> 3) & (B2_NCH - 1);
    const int s = (bx >> 5) * 8 + (bx & 7);
    const int n0 = nc * B2_NC;
    const int R = min(a.n_rows, *a.r_ptr);
    const int Rn = max(R, min(a.n_rows, *a.rn_ptr));
    const int S = a.S;
    const int C = (Rn + B2_ROWS - 1) / B2_ROWS;  // chunks below Rn
    // slice s owns chunks s, s + S, s + 2 S, ... < C; the seed chunks (those
    // with a dy row: c < Cs) are the first ones, so they spread over the
    // slices -- a chunk past them has no dy and skips everything dy feeds
    const int Cs = (R + B2_ROWS - 1) / B2_ROWS;
    const int K0 = a.K0, F1 = a.F1;

    // ---- stage-B operand: [W_r1; W_l1] rows k = 32 kc + 8 q + j (W_r1 rows
    // 0..47, W_l1 rows 48..95, zero past F1), column n0 + 16 nt + l16
    const int rt = wv >> 2, nt = wv & 3;
    bf8 wb[3][2];
    int eW;  // the slice's scale
    {
        // (buffer loads over the F1 weight rows: all 24 in flight, no branches)
        const i32x4 wrr = make_rsrc(a.wr1, static_cast<uint32_t>(F1 * a.ldw1 * 4));
        const i32x4 wlr = make_rsrc(a.wl1, static_cast<uint32_t>(F1 * a.ldw1 * 4));
        const int n = n0 + 16 * nt + l16;
        float v[3][8];
#pragma unroll
        for (int kc = 0; kc < 3; ++kc)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int k = 32 * kc + 8 * q + j;
                const int f = k < 48 ? k : k - 48;
                const int o = f < F1 ? (f * static_cast<int>(a.ldw1) + n) * 4 : kOOB;
                v[kc][j] = k < 48 ? buf_load1(wrr, o, 0, 0) : buf_load1(wlr, o, 0, 0);
            }
        // the wave's scale: its slice is n-tile nt of [W_r1; W_l1] (the same
        // for both row-tile waves of nt and for stage C0's wave of nt)
        float mx = 0.0f;
#pragma unroll
        for (int kc = 0; kc < 3; ++kc)
#pragma unroll
            for (int j = 0; j < 8; ++j) mx = fmaxf(mx, fabsf(v[kc][j]));
        eW = __builtin_amdgcn_readfirstlane(h2_exp(wave_max(mx)));
#pragma unroll
        for (int kc = 0; kc < 3; ++kc)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                _Float16 p1, p2;
                split2(__builtin_amdgcn_ldexpf(v[kc][j], eW), p1, p2);
                wb[kc][0][j] = p1;
                wb[kc][1][j] = p2;
            }
    }
    const float *xb = a.x_dev ? gload(a.x_dev, 0) : a.x;
    const int64_t *xrow = !XR ? nullptr : a.xrow_dev ? gload(a.xrow_dev, 0) : a.xrow;

    // ---- per-thread staging map (512 threads, one 32-row chunk)
    //   dy: column fd = t % 48, rows t / 48 + 10 u (t < 480, u < 4)
    //   g:  row t / 12, float4 t % 12 (t < 384);  h: row t / 16, float4 t % 16
    //   x / agg0: row t / 16, columns 8 (t % 16) .. + 7 (two float4)
    const int fd = t % 48, rd = t / 48;
    const int rg = t / 12, cg = t % 12;
    const int rh = t >> 4, ch = t & 15;
    const int rx = t >> 4, cx = t & 15;
    struct Pre {
        float dyv[4];
        v4f gv, hv, xv[2], av[2];
        int d0, d1;  // rowptr of the agg row (edgeless rows masked at staging)
        int xi;      // XR: n_id of the x row of the NEXT chunk (one chunk ahead)
    };
    // every operand through a buffer resource over its live rows: 32-bit
    // offsets = a per-thread base + the chunk's row offset, no 64-bit
    // address arithmetic per load; rows past the range read 0
    const i32x4 dyr = make_rsrc(a.dy, static_cast<uint32_t>(static_cast<int64_t>(R) * a.ldy * 4));
    const i32x4 gr = make_rsrc(a.g, static_cast<uint32_t>(static_cast<int64_t>(Rn) * a.C4 * 4));
    const i32x4 hr = make_rsrc(a.h, static_cast<uint32_t>(static_cast<int64_t>(Rn) * a.ldh * 4));
    const i32x4 ar = make_rsrc(a.agg, static_cast<uint32_t>(static_cast<int64_t>(Rn) * a.ld_agg * 4));
    const i32x4 rpr = make_rsrc(a.rowptr, static_cast<uint32_t>(static_cast<int64_t>(Rn + 1) * 4));
    const int64_t xrows = xrow ? a.x_rows : static_cast<int64_t>(Rn);
    const i32x4 xrr = make_rsrc_u(xb, static_cast<uint32_t>(xrows * a.ldx * 4));
    const i32x4 ir = make_rsrc_u(xrow, static_cast<uint32_t>(xrow ? static_cast<int64_t>(Rn) * 8 : 0));
    const uint32_t ldy4 = static_cast<uint32_t>(a.ldy) * 4u, ldh4 = static_cast<uint32_t>(a.ldh) * 4u;
    const uint32_t lda4 = static_cast<uint32_t>(a.ld_agg) * 4u, ldx4 = static_cast<uint32_t>(a.ldx) * 4u;
    const uint32_t C44 = static_cast<uint32_t>(a.C4) * 4u;
    auto iload = [&](int c) __attribute__((always_inline)) -> int {  // low word of n_id
        const int r = c * B2_ROWS + rx;
        return buf_load1i(ir, (c < C && r < Rn) ? 8 * r : kOOB, 0, 0);
    };
    // (the slice's next chunk is c + S; dyv is loaded, and read, on seed
    // chunks only)
    auto load = [&](int c, Pre &p) __attribute__((always_inline)) {
        const int r0 = c * B2_ROWS;
        const bool live = c < C;
        if (c < Cs) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int lr = rd + 10 * u, r = r0 + lr;
                const bool ok = t < 480 && lr < B2_ROWS && r < R && fd < F1;
                p.dyv[u] =
                    buf_load1(dyr, ok ? static_cast<int>(static_cast<uint32_t>(r) * ldy4) + 4 * fd : kOOB, 0, 0);
            }
        }
        {
            const int r = r0 + rg;
            const bool ok = live && t < 384 && r < Rn && 4 * cg < a.C4;
            p.gv = buf_load4(gr, ok ? static_cast<int>(static_cast<uint32_t>(r) * C44) + 16 * cg : kOOB, 0, 0);
        }
        {
            const int r = r0 + rh;
            p.hv = buf_load4(hr, (live && r < Rn) ? static_cast<int>(static_cast<uint32_t>(r) * ldh4) + 4 * (n0 + 4 * ch) : kOOB,
                             0, 0);
        }
        {
            const int r = r0 + rx;
            const bool okr = live && r < Rn;
            // (XR: this chunk's n_id word arrived a chunk ago)
            const uint32_t xr = (XR && xrow) ? static_cast<uint32_t>(p.xi) : static_cast<uint32_t>(r);
            if (XR) p.xi = iload(c + S);
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int k = 8 * cx + 4 * u;
                const bool ok = okr && k < K0;
                if constexpr (ROOT) p.xv[u] = buf_load4(xrr, ok ? static_cast<int>(xr * ldx4) + 4 * k : kOOB, 0, 0);
                else p.xv[u] = v4f{0.f, 0.f, 0.f, 0.f};
                p.av[u] = buf_load4(ar, ok ? static_cast<int>(static_cast<uint32_t>(r) * lda4) + 4 * k : kOOB, 0, 0);
            }
            // (an edgeless row's aggregate counts as 0: its row may never be
            // written -- tested at staging, so no load waits on these)
            p.d0 = buf_load1i(rpr, okr ? 4 * r : kOOB, 0, 0);
            p.d1 = buf_load1i(rpr, okr ? 4 * r + 4 : kOOB, 0, 0);
        }
    };
    // per-chunk scales: X = [dy | g], h, x, agg0 (powers of two, uniform)
    struct Exps {
        int X, H, x, a;
    };
    // the chunk's maxima over the values staging writes (loads past a range
    // read 0; edgeless rows' aggregate counts as 0), wave-reduced, into LDS
    // slot sl (8 waves x 4); every thread reads them back after a barrier
    float4 *smax = reinterpret_cast<float4 *>(sred + 2 * 256 + 480);  // [2][8]
    // (hd: the chunk has dy rows -- past them dy is 0 and X's maximum is g's)
    auto publish_max = [&](const auto &p, int sl, bool hd) __attribute__((always_inline)) {
        if (DBG & 1) return;
        float mX = amax4(p.gv);
        if (hd)
            mX = fmaxf(mX, fmaxf(fmaxf(fabsf(p.dyv[0]), fabsf(p.dyv[1])), fmaxf(fabsf(p.dyv[2]), fabsf(p.dyv[3]))));
        float mH = amax4(p.hv);
        float mx = fmaxf(amax4(p.xv[0]), amax4(p.xv[1]));
        float ma = p.d1 > p.d0 ? fmaxf(amax4(p.av[0]), amax4(p.av[1])) : 0.0f;
        mX = wave_max(mX);
        mH = wave_max(mH);
        mx = wave_max(mx);
        ma = wave_max(ma);
        if (ln == 0) smax[sl * 8 + wv] = float4{mX, mH, mx, ma};
    };
    // (a scale may grow by at most 2^20 from one chunk to the next, so the
    // accumulators, rescaled in place by the change, never overflow; a chunk
    // held below its own scale has values 2^20 under the previous one's)
    auto read_exps = [&](int sl, const Exps &pe, bool first) __attribute__((always_inline)) -> Exps {
        if (DBG & 1) return Exps{10, 10, 10, 10};
        float4 m = smax[sl * 8];
#pragma unroll
        for (int w = 1; w < 8; ++w) {
            const float4 o = smax[sl * 8 + w];
            m.x = fmaxf(m.x, o.x);
            m.y = fmaxf(m.y, o.y);
            m.z = fmaxf(m.z, o.z);
            m.w = fmaxf(m.w, o.w);
        }
        Exps e{__builtin_amdgcn_readfirstlane(h2_exp(m.x)), __builtin_amdgcn_readfirstlane(h2_exp(m.y)),
               __builtin_amdgcn_readfirstlane(h2_exp(m.z)), __builtin_amdgcn_readfirstlane(h2_exp(m.w))};
        if (!first) {
            e.X = min(e.X, pe.X + 20);
            e.H = min(e.H, pe.H + 20);
            e.x = min(e.x, pe.x + 20);
            e.a = min(e.a, pe.a + 20);
        }
        return e;
    };
    // two fp16 parts of 8 floats (scaled by 2^e) -> part images at (row, col), 16 B each
    auto put8 = [&](L16 *img, int part_stride, int off, v4f v0, v4f v1, int e) __attribute__((always_inline)) {
        bf8 p1, p2;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            _Float16 a1, a2;
            split2(__builtin_amdgcn_ldexpf(i < 4 ? v0[i] : v1[i - 4], e), a1, a2);
            p1[i] = a1;
            p2[i] = a2;
        }
        *reinterpret_cast<__attribute__((address_space(3))) bf8 *>(img + off) = p1;
        *reinterpret_cast<__attribute__((address_space(3))) bf8 *>(img + part_stride + off) = p2;
    };
    // two fp16 parts of 4 floats (scaled by 2^e) -> part images at (row, col), 8 B each
    auto put4 = [&](L16 *img, int part_stride, int off, v4f v, int e) __attribute__((always_inline)) {
        bf4 p1, p2;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            _Float16 a1, a2;
            split2(__builtin_amdgcn_ldexpf(v[i], e), a1, a2);
            p1[i] = a1;
            p2[i] = a2;
        }
        *reinterpret_cast<__attribute__((address_space(3))) bf4 *>(img + off) = p1;
        *reinterpret_cast<__attribute__((address_space(3))) bf4 *>(img + part_stride + off) = p2;
    };
    float d1acc = 0.0f;  // db1 partial: column fd, rows of this thread
    // hd: the chunk has dy rows.  Without them X's dy columns are not
    // written: nothing reads columns 0..31 of such a chunk, and columns
    // 32..47 (stage B's k-chunk 1 holds them next to g) are zeroed when the
    // buffer last held a seed chunk or nothing yet (zx)
    auto stage_images = [&](const Pre &p, L16 *buf, const Exps &e, bool hd, bool zx) __attribute__((always_inline)) {
        L16 *ix = buf, *ih = ix + IMG_X, *ik = ih + IMG_H, *ia = ik + IMG_K;
        if (zx) {  // 32 rows x 2 parts x 8 column pairs, 4 B per thread
            L16 *z = ix + ((t >> 3) & 1) * B2_ROWS * XS + (t >> 4) * XS + 32 + 2 * (t & 7);
            *reinterpret_cast<__attribute__((address_space(3))) int *>(z) = 0;
        }
        if (hd && t < 480) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int lr = rd + 10 * u;
                if (lr < B2_ROWS) {
                    _Float16 a1, a2;
                    split2(__builtin_amdgcn_ldexpf(p.dyv[u], e.X), a1, a2);
                    ix[lr * XS + fd] = a1;
                    ix[B2_ROWS * XS + lr * XS + fd] = a2;
                    d1acc += p.dyv[u];
                }
            }
        }
        if (t < 384) put4(ix, B2_ROWS * XS, rg * XS + 48 + 4 * cg, p.gv, e.X);
        put4(ih, B2_ROWS * HS, rh * HS + 4 * ch, p.hv, e.H);
        if constexpr (ROOT) put8(ik, B2_ROWS * KS, rx * KS + 8 * cx, p.xv[0], p.xv[1], e.x);
        const bool deg = p.d1 > p.d0;
        const v4f z4{0.f, 0.f, 0.f, 0.f};
        put8(ia, B2_ROWS * KS, rx * KS + 8 * cx, deg ? p.av[0] : z4, deg ? p.av[1] : z4, e.a);
    };

    // ---- stage B: dh tile (rt, nt) -> masked dz0 parts into sA
    float d0acc = 0.0f;  // db0 partial: column 16 nt + l16, rows 16 rt + 4 q + i
    // (k-chunk 0 is dy columns 0..31 only: skipped on a chunk without dy, as
    // the root-free form skips it everywhere -- exact zeros either way)
    auto stage_b = [&](L16 *buf, const Exps &e, bool hd) __attribute__((always_inline)) {
        const L16 *ix = buf, *ih = ix + IMG_X;
        L16 *sa = buf + IMG_X + IMG_H + 2 * IMG_K;
        v4f acc{0.f, 0.f, 0.f, 0.f};
        auto kstep = [&](int kc) __attribute__((always_inline)) {
            const int off = (16 * rt + l16) * XS + 32 * kc + 8 * q;
            const bf8 a1 = *reinterpret_cast<const __attribute__((address_space(3))) bf8 *>(ix + off);
            const bf8 a2 = *reinterpret_cast<const __attribute__((address_space(3))) bf8 *>(ix + B2_ROWS * XS + off);
            acc = mfma3(a1, a2, wb[kc][0], wb[kc][1], acc);
        };
        if (ROOT && hd) kstep(0);
        kstep(1);
        kstep(2);
        // mask: the sign of h's first part (a positive h below 2^-39 of its
        // chunk's max rounds to +0 -- a pre-activation that far inside fp32's
        // noise of the ReLU kink)
        const s4 hm = tr_read(ih, HS, 16 * rt, 16 * nt, ln);
        v4f dz;
        const int eu = -(e.X + eW);  // acc -> dh
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            dz[i] = hm[i] > 0 ? acc[i] * a.yscale : 0.0f;
            d0acc += __builtin_amdgcn_ldexpf(dz[i], eu);
        }
        bf4 p1, p2;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            _Float16 a1, a2;
            split2(__builtin_amdgcn_ldexpf(dz[i], -a.e_dz), a1, a2);
            p1[i] = a1;
            p2[i] = a2;
        }
        L16 *d = sa + ((nt * 2) * 64 + ln) * 8 + 4 * rt;
        *reinterpret_cast<__attribute__((address_space(3))) bf4 *>(d) = p1;
        *reinterpret_cast<__attribute__((address_space(3))) bf4 *>(d + 64 * 8) = p2;
    };

    // ---- stage C: the weight-gradient products of one staged chunk
    // ROOT: wave (mat, nt) takes dW_r0 (mat 0) or dW_l0 (mat 1) rows of
    // n-tile nt over all KT column tiles, and tiles wv + 8 u of the 24 of
    // [dW_r1; dW_l1] (tile tt = 4 mf + nn: f-tile mf = mat + 2 u, n-tile nn =
    // nt for all three, so one h fragment serves them).  Tiles 0..11 are
    // dW_r1, 12..23 dW_l1: waves 0-3 hold 2 + 1 of them, waves 4-7 1 + 2, and
    // a chunk without dy costs a wave its dW_l1 tiles only.  Root-free: dW_l0
    // column tiles kt = (wv >> 2) + 2 i, and tiles wv + 8 u of the 12 of
    // dW_l1 (f-tiles 3..5)
    constexpr int NK0 = ROOT ? KT : (KT + 1) / 2;
    constexpr int NC1 = ROOT ? 3 : 2;
    constexpr int C1_TILES = 24;
    const int mat = wv >> 2;
    auto c0_kt = [&](int i) { return ROOT ? i : mat + 2 * i; };
    auto c1_tile = [&](int u) { return ROOT ? wv + 8 * u : (wv + 8 * u < 12 ? 12 + wv + 8 * u : C1_TILES); };
    v4f acc0[NK0], acc1[NC1];
#pragma unroll
    for (int i = 0; i < NK0; ++i) acc0[i] = v4f{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < NC1; ++i) acc1[i] = v4f{0.f, 0.f, 0.f, 0.f};
    // the accumulators hold sums in the units of the last chunk added:
    // 2^E0 (dz0 2^(eX + eW - e_dz) times x / agg0 2^(ex | ea)), 2^E1[u] (X
    // 2^eX times h 2^eH); each chunk rescales them by the change (v_ldexp,
    // exact unless a sum falls below fp32's range) and its MFMAs accumulate
    // on top.  A dW_r1 tile is rescaled, and its exponent moved, on seed
    // chunks only.  Those are the first chunks of the slice's sequence, one
    // after the other, so its exponent too moves by one chunk-to-chunk step
    // at a time -- at most 2^20 per operand, read_exps' clamp -- and after
    // the last seed chunk the tile rests until the final unscaling.
    int E0 = 0, E1[NC1] = {};
    bool acc_empty = true;
    // HD: the chunk has dy rows (compile time: one straight-line body each)
    auto stage_c = [&](const L16 *buf, const Exps &e, auto hd_c) __attribute__((always_inline)) {
        constexpr bool HD = decltype(hd_c)::value;
        // (a rooted wave's tile 0 is dW_r1, tile 2 dW_l1, tile 1 by its half)
        auto c1_on = [&](int u) {
            if (!ROOT) return c1_tile(u) < C1_TILES;
            return HD || u == 2 || (u == 1 && mat);
        };
        const L16 *ix = buf, *ih = ix + IMG_X, *ik = ih + IMG_H, *ia = ik + IMG_K;
        const L16 *sa = ia + IMG_K;
        // C0: A = dz0^T of n-tile nt (both row tiles), B = x / agg0 tiles
        const bf8 a1 = *reinterpret_cast<const __attribute__((address_space(3))) bf8 *>(sa + ((nt * 2) * 64 + ln) * 8);
        const bf8 a2 = *reinterpret_cast<const __attribute__((address_space(3))) bf8 *>(sa + ((nt * 2 + 1) * 64 + ln) * 8);
        const L16 *img = (mat || !ROOT) ? ia : ik;
        // every fragment read of the stage issued before its first MFMA (the
        // reads' latency once per chunk, not once per tile)
        bf8 b1[KT], b2[KT], x1[3], x2[3];
#pragma unroll
        for (int i = 0; i < NK0; ++i) {
            const int kt = c0_kt(i);
            b1[i] = tr_frag(img, KS, 16 * kt, ln);
            b2[i] = tr_frag(img + B2_ROWS * KS, KS, 16 * kt, ln);
        }
        // C1: tiles of [dW_r1; dW_l1] (f-tile mf, n-tile nt): A = X^T, B = h
        // (X's dy columns, f-tiles 0..2, are read on seed chunks only)
        const bf8 h1 = tr_frag(ih, HS, 16 * nt, ln), h2 = tr_frag(ih + B2_ROWS * HS, HS, 16 * nt, ln);
#pragma unroll
        for (int u = 0; u < NC1; ++u)
            if (c1_on(u)) {
                const int mf = c1_tile(u) >> 2;
                x1[u] = tr_frag(ix, XS, 16 * mf, ln);
                x2[u] = tr_frag(ix + B2_ROWS * XS, XS, 16 * mf, ln);
            }
        const int e0 = e.X + eW - a.e_dz + ((mat || !ROOT) ? e.a : e.x);
        const int e1 = e.X + e.H;
        if (!acc_empty) {
#pragma unroll
            for (int i = 0; i < NK0; ++i) acc0[i] = ldexp4(acc0[i], e0 - E0);
#pragma unroll
            for (int u = 0; u < NC1; ++u)
                if (c1_on(u)) acc1[u] = ldexp4(acc1[u], e1 - E1[u]);
        }
        E0 = e0;
#pragma unroll
        for (int u = 0; u < NC1; ++u)
            if (c1_on(u)) E1[u] = e1;
        acc_empty = false;
#pragma unroll
        for (int i = 0; i < NK0; ++i)
            if (c0_kt(i) < KT) acc0[i] = mfma3(a1, a2, b1[i], b2[i], acc0[i]);
#pragma unroll
        for (int u = 0; u < NC1; ++u)
            if (c1_on(u)) acc1[u] = mfma3(x1[u], x2[u], h1, h2, acc1[u]);
    };
    auto stage_c_of = [&](const L16 *buf, const Exps &e, bool hd) __attribute__((always_inline)) {
        if (hd) stage_c(buf, e, std::true_type{});
        else stage_c(buf, e, std::false_type{});
    };

    // ---- pipeline over the slice's chunks (two LDS buffers):
    //   phase 1: stage C(c - 1) on buffer (c-1)&1; images of chunk c into
    //            buffer c&1 (from registers); loads of chunk c + 1 issued
    //   barrier
    //   phase 2: stage B(c) on buffer c&1 -> its dz0 fragments
    //   barrier
    //   (and, before the second barrier, chunk c + 1's maxima: its loads have
    //   landed by then -- published to the next iteration's staging)
    // The slice's j-th chunk is c = s + j S and uses buffer (and maxima
    // slot) j & 1.  hd / hdn / hdp: chunk c / its successor / its
    // predecessor has dy rows (uniform; once false it stays false).
    Pre pre;
    pre.xi = XR ? iload(s) : 0;
    if (XR) asm volatile("" : "+v"(pre.xi));  // (the first chunk's n_id: waited here once)
    Exps ep{0, 0, 0, 0};
    if (s < C) {
        load(s, pre);
        if (LAG) publish_max(pre, 0, s < Cs);
    }
    if (LAG) lds_barrier();
#ifdef NGNN_B2_SETPRIO
    // (A/B: static priority for the second-dispatched half, waves 4-7 --
    // MI355X_MICROARCH.md, scheduling item 4)
    if (wv >= 4) __builtin_amdgcn_s_setprio(1);
#endif
    int j = 0;
    bool hdp = false;
    for (int c = s; c < C; c += S, ++j) {
        L16 *cur = lb + (j & 1) * BUF, *prv = lb + ((j & 1) ^ 1) * BUF;
        const bool hd = c < Cs, hdn = c + S < Cs;
        // (the buffer's dy columns 32..47 hold the values of the chunk two
        // back, or nothing yet)
        const bool zx = !hd && (j < 2 || c - 2 * S < Cs);
        if (LAG) {
            // chunk c's images first (buffer j & 1: the chunk two back's,
            // whose stage C ran before the last two barriers), then the next
            // chunk's loads, which land during stage C of the previous chunk
            // and stage B(c) -- its maxima are published after stage B
            const Exps ec = read_exps(j & 1, ep, j == 0);
            stage_images(pre, cur, ec, hd, zx);
            load(c + S, pre);
            if (j > 0) stage_c_of(prv, ep, hdp);
            lds_barrier();  // (LDS only: the next chunk's loads stay in flight)
            stage_b(cur, ec, hd);
            publish_max(pre, (j + 1) & 1, hdn);
            lds_barrier();
            ep = ec;
            hdp = hd;
            continue;
        }
        if (j > 0) stage_c_of(prv, ep, hdp);
        publish_max(pre, j & 1, hd);
        lds_barrier();
        const Exps ec = read_exps(j & 1, ep, j == 0);
        stage_images(pre, cur, ec, hd, zx);
        load(c + S, pre);
        lds_barrier();  // (LDS only: the next chunk's loads stay in flight)
        stage_b(cur, ec, hd);
        lds_barrier();
        ep = ec;
        hdp = hd;
    }
    if (j > 0) stage_c_of(lb + ((j - 1) & 1) * BUF, ep, hdp);
    // back to true units
#pragma unroll
    for (int i = 0; i < NK0; ++i) acc0[i] = ldexp4(acc0[i], -E0);
#pragma unroll
    for (int u = 0; u < NC1; ++u) acc1[u] = ldexp4(acc1[u], -E1[u]);

    // ---- this workgroup's part of slab s (zeros for an empty slice)
    float *slab = a.slab + static_cast<int64_t>(s) * b2_slab_floats(K0, F1);
    {
        const i32x4 sr = make_rsrc(slab, static_cast<uint32_t>(b2_slab_floats(K0, F1) * 4));
        // dW_r0 / dW_l0 rows n = n0 + 16 nt + 4 q + i, columns 16 kt + l16
        // (root-free: dW_l0 only; dW_r0's slab region is left unwritten --
        // the reduce skips the absent gradients)
        const int base0 = (mat || !ROOT) ? 256 * K0 : 0;
#pragma unroll
        for (int j = 0; j < NK0; ++j) {
            const int k = 16 * c0_kt(j) + l16;
#pragma unroll
            for (int i = 0; i < 4; ++i)
                buf_store1(acc0[j][i], sr, k < K0 ? 4 * (base0 + (n0 + 16 * nt + 4 * q + i) * K0 + k) : kOOB, 0, 0);
        }
        // dW_r1 / dW_l1 rows f = 16 mf + 4 q + i (< 48: W_r1, else W_l1),
        // columns n0 + 16 nn + l16
#pragma unroll
        for (int u = 0; u < NC1; ++u) {
            const int tt = c1_tile(u), mf = tt >> 2, nn = tt & 3;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int f = 16 * mf + 4 * q + i;
                const int fr = f < 48 ? f : f - 48;
                const int o = 512 * K0 + 256 + (f < 48 ? 0 : 256 * F1) + fr * 256 + n0 + 16 * nn + l16;
                buf_store1(acc1[u][i], sr, (tt < C1_TILES && fr < F1) ? 4 * o : kOOB, 0, 0);
            }
        }
    }
    // db0: lanes (q) then the two row-tile waves; db1: the 10 threads of a column
    float v0 = sum_xor32(sum_xor16(d0acc));
    __syncthreads();
    if (q == 0) sred[rt * 64 + nt * 16 + l16] = v0;
    if (t < 480) sred[128 + t] = d1acc;
    __syncthreads();
    if (t < 64) slab[512LL * K0 + n0 + t] = sred[t] + sred[64 + t];
    if (nc == 0 && t < F1) {
        float v = 0.0f;
        for (int r = 0; r < 10; ++r) v += sred[128 + r * 48 + t];
        slab[512LL * K0 + 256 + 512LL * F1 + t] = v;
    }
}

// Adam over the six gradients as they are summed (ngnn_adam_fold): the
// update of ngnn_adam_step's k_adam, element by element, same arithmetic
struct AdamFold {
    float *p[6], *m[6], *v[6];  // in the reduce's order: W_r0, W_l0, b0, W_r1, W_l1, b1
    float *step;
    float lr, b1, b2, eps, wd;
    const uint64_t *gate;  // (ABI 20) the slot's contract gate: no update when gated
    const int64_t *gate_gen;
};

// out = sum over slabs in slab order; with ADAM the parameters are updated
// from them too (k_bwd2 has advanced the step count already: t = *step);
// then g rows < R' back to zero (blocks >= n_red)
template <bool ADAM>
__global__ __launch_bounds__(256) void k_bwd2_reduce(const float *__restrict__ slab, int S, int K0, int F1,
                                                      float *dwr0, float *dwl0, float *db0, float *dwr1,
                                                      float *dwl1, float *db1, float *g, int C4, int n_rows,
                                                      const int32_t *r_ptr, const int32_t *rn_ptr, int n_red,
                                                      AdamFold af) {
    const int64_t total = b2_slab_floats(K0, F1);
    if (static_cast<int>(blockIdx.x) >= n_red) {  // g clearing blocks
        const int R = min(n_rows, *r_ptr);
        const int Rn = max(R, min(n_rows, *rn_ptr));
        const int64_t n4 = static_cast<int64_t>(Rn) * C4 / 4;
        for (int64_t i = (static_cast<int64_t>(blockIdx.x) - n_red) * 256 + threadIdx.x; i < n4;
             i += static_cast<int64_t>(gridDim.x - n_red) * 256)
            reinterpret_cast<v4f *>(g)[i] = v4f{0.f, 0.f, 0.f, 0.f};
        return;
    }
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= total) return;
    const int64_t A = 256LL * K0, Bf = 256LL * F1;
    int k;
    int64_t e;
    if (i < A) k = 0, e = i;
    else if (i < 2 * A) k = 1, e = i - A;
    else if (i < 2 * A + 256) k = 2, e = i - 2 * A;
    else if (i < 2 * A + 256 + Bf) k = 3, e = i - 2 * A - 256;
    else if (i < 2 * A + 256 + 2 * Bf) k = 4, e = i - 2 * A - 256 - Bf;
    else k = 5, e = i - 2 * A - 256 - 2 * Bf;
    float *const outs[6] = {dwr0, dwl0, db0, dwr1, dwl1, db1};
    if (!outs[k]) return;  // (a root-free stack's dW_r0 / dW_r1: not computed, not stepped)
    float t = 0.0f;
    if (ADAM) t = *af.step;  // (issued before the slab loads)
    float v = 0.0f;
    int sl = 0;
    // (32 slab loads in flight per thread: the launch is a few waves per
    // SIMD, so each batch costs one HBM round trip -- the sum stays in slab
    // order, one element at a time)
    for (; sl + 32 <= S; sl += 32) {
        float w[32];
#pragma unroll
        for (int u = 0; u < 32; ++u) w[u] = slab[static_cast<int64_t>(sl + u) * total + i];
#pragma unroll
        for (int u = 0; u < 32; ++u) v += w[u];
    }
    for (; sl + 8 <= S; sl += 8) {
        float w[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) w[u] = slab[static_cast<int64_t>(sl + u) * total + i];
#pragma unroll
        for (int u = 0; u < 8; ++u) v += w[u];
    }
    for (; sl < S; ++sl) v += slab[static_cast<int64_t>(sl) * total + i];
    outs[k][e] = v;
    if (ADAM && !slot_gated(af.gate, af.gate_gen)) {  // k_adam's update (ngnn_optim.hip) of element e of tensor k
        const float bc1 = 1.0f - powf(af.b1, t);
        const float bc2s = sqrtf(1.0f - powf(af.b2, t));
        const float step_size = af.lr / bc1;
        float gr = v, p = af.p[k][e], m = af.m[k][e], vv = af.v[k][e];
        if (af.wd != 0.0f) gr = gr + af.wd * p;
        m = m + (1.0f - af.b1) * (gr - m);
        vv = af.b2 * vv + (1.0f - af.b2) * gr * gr;
        const float denom = sqrtf(vv) / bc2s + af.eps;
        p = p - step_size * (m / denom);
        af.m[k][e] = m;
        af.v[k][e] = vv;
        af.p[k][e] = p;
    }
}

constexpr int B2_S = 64;  // row slices (x 4 hidden chunks = 256 workgroups)

struct Ws3 {
    size_t g, slab, total;
};
// slabs first, then g: g's offset does not depend on n_rows, so a zeroed
// workspace grown for more rows keeps every g row it ever held at zero
Ws3 ws3_layout(int64_t n_rows, int64_t K0, int64_t F1) {
    Ws3 w;
    const int64_t C4 = (F1 + 3) & ~int64_t{3};
    w.slab = 0;
    const size_t sb = static_cast<size_t>(B2_S) * b2_slab_floats(static_cast<int>(K0), static_cast<int>(F1)) * 4;
    w.g = (sb + 255) & ~size_t{255};
    w.total = w.g + static_cast<size_t>(std::max<int64_t>(n_rows, 1)) * C4 * 4;
    return w;
}

// ---------------------------------------------------------------- host half
// ngnn_sage2_bwd's arguments, in the ABI's order: the entry fills it once, by
// position, and the steps below take it.
struct Sage2Bwd {
    const float *dy;
    int64_t ldy, F1;
    const float *wl1, *wr1;
    int64_t ldw1;
    const float *h;
    int64_t ldh;
    float yscale;
    const float *x;
    const float *const *x_dev;
    const int64_t *xrow;
    const int64_t *const *xrow_dev;
    int64_t x_rows, ldx, K0;
    const float *agg0;
    int64_t ld_agg;
    const int32_t *rowptr, *col;
    int64_t n_rows;
    const int32_t *r_ptr, *rnext_ptr;
    int reduce;
    float *dwl1, *dbl1, *dwr1, *dwl0, *dbl0, *dwr0;
    const float *g_pre;
    const ngnn_adam_fold *adam;
    void *ws;
    size_t ws_bytes;
    // (ABI 18: dW_r0 and dW_r1 both NULL -- a root-free stack, SimpleGCN's
    // W_r = 0: x is not read and may be NULL; wr1 is still read -- zeros)
    bool root() const { return dwr0 || dwr1; }
    bool indexed() const { return xrow || xrow_dev; }
    int C4() const { return static_cast<int>((F1 + 3) & ~int64_t{3}); }
};

// Every argument error of the entry, before any launch.  The order of the
// checks decides which code a call with several faults gets: part of the
// contract (tests/test_sage2_args_cpu.py restates it).
int sage2_bwd_check(const Sage2Bwd &B) {
    NGNN_RETURN_IF(B.reduce != NGNN_REDUCE_MEAN && B.reduce != NGNN_REDUCE_SUM, NGNN_E_ARG);
    NGNN_RETURN_IF(B.F1 <= 0 || B.F1 > 48 || B.K0 <= 0 || B.K0 > 128 || B.K0 % 4 != 0, NGNN_E_SHAPE);
    NGNN_RETURN_IF(B.n_rows < 0 || !fits_i32(B.n_rows), NGNN_E_RANGE);
    const bool root = B.root(), indexed = B.indexed();
    NGNN_RETURN_IF(!B.dy || !B.wl1 || !B.wr1 || !B.h || (root && !B.x && !B.x_dev) || !B.agg0 || !B.rowptr ||
                       !B.col || !B.r_ptr || !B.rnext_ptr || !B.dwl1 || !B.dbl1 || (root && (!B.dwr1 || !B.dwr0)) ||
                       !B.dwl0 || !B.dbl0 || !B.ws,
                   NGNN_E_ARG);
    NGNN_RETURN_IF(!root && indexed, NGNN_E_ARG);
    NGNN_RETURN_IF(B.ldy < B.F1 || B.ldw1 < 256 || B.ldh < 256 || B.ldh % 4 != 0 || B.ldx < B.K0 || B.ldx % 4 != 0 ||
                       B.ld_agg < B.K0 || B.ld_agg % 4 != 0,
                   NGNN_E_SHAPE);
    NGNN_RETURN_IF((B.x && !aligned(B.x, 16)) || !aligned(B.h, 16) || !aligned(B.agg0, 16) || !aligned(B.ws, 256) ||
                       (B.g_pre && !aligned(B.g_pre, 16)),
                   NGNN_E_ALIGN);
    NGNN_RETURN_IF(indexed && B.x_rows <= 0, NGNN_E_ARG);
    // 32-bit buffer offsets: every operand's live rows within kRangeMax (as
    // ngnn_sage2_fwd checks; past it the resources would truncate)
    const int64_t n = B.n_rows;
    NGNN_RETURN_IF(n * B.ldh * 4 > kRangeMax || n * B.ld_agg * 4 > kRangeMax || n * B.ldy * 4 > kRangeMax ||
                       std::max(n, indexed ? B.x_rows : 0) * B.ldx * 4 > kRangeMax || n * B.C4() * 4 > kRangeMax,
                   NGNN_E_RANGE);
    if (B.adam) {
        NGNN_RETURN_IF(!B.adam->step, NGNN_E_ARG);
        for (int k = 0; k < 6; ++k)
            NGNN_RETURN_IF(!B.adam->param[k] || !B.adam->exp_avg[k] || !B.adam->exp_avg_sq[k], NGNN_E_ARG);
    }
    NGNN_RETURN_IF(B.ws_bytes < ws3_layout(B.n_rows, B.K0, B.F1).total, NGNN_E_WORKSPACE);
    return NGNN_OK;
}

// k_bwd2's arguments; g and slab are the workspace's pieces
B2Args bwd2_args(const Sage2Bwd &B, float *g, float *slab) {
    B2Args b;
    b.dy = B.dy, b.ldy = B.ldy, b.F1 = static_cast<int>(B.F1);
    // (g_pre: the forward's loss head scattered it already -- the workspace's
    // g stays zero, and the reduce's clearing blocks have nothing to do)
    b.g = B.g_pre ? B.g_pre : g, b.C4 = B.C4();
    b.wr1 = B.wr1, b.wl1 = B.wl1, b.ldw1 = B.ldw1, b.h = B.h, b.ldh = B.ldh, b.yscale = B.yscale;
    // |dh| in the scaled units <= 96 2^30 (two operands of max < 2^15, 96
    // terms); dz0 = dh yscale must stay below fp16's 2^16 after 2^-e_dz
    int e = 0;
    (void)std::frexp(std::max(B.yscale, 1.0f), &e);  // yscale <= 2^e
    b.e_dz = 21 + e;
    b.x = B.x, b.x_dev = B.x_dev, b.xrow = B.xrow, b.xrow_dev = B.xrow_dev, b.x_rows = B.x_rows, b.ldx = B.ldx;
    b.K0 = static_cast<int>(B.K0), b.agg = B.agg0, b.ld_agg = B.ld_agg, b.rowptr = B.rowptr;
    b.n_rows = static_cast<int>(B.n_rows), b.r_ptr = B.r_ptr, b.rn_ptr = B.rnext_ptr;
    b.slab = slab, b.S = B2_S;
    b.step_inc = B.adam ? B.adam->step : nullptr;
    b.gate = B.adam ? B.adam->gate : nullptr;
    b.gate_gen = B.adam ? B.adam->gate_gen : nullptr;
    return b;
}

#ifdef NGNN_B2_DBG_BUILD
constexpr bool kB2DbgBuild = true;
#else
constexpr bool kB2DbgBuild = false;
#endif

// The one k_bwd2 launch.  Instantiated: XR x KT {4, 7, 8} x LAG with a root
// term; root-free with XR false only (x is not read, and sage2_bwd_check
// refuses an index there); DBG 1 (profiling builds, NGNN_B2_DBG=1) on the
// rooted lagged kernels only -- the `if constexpr` keeps the others out.
// (This nesting emits the kernels in the order they have always had in the
// object file.)
int launch_bwd2(const Sage2Bwd &B, const B2Args &b, hipStream_t st) {
    // (A/B switch, read once; default lagged: measured 43.8 vs 44.6 us per
    // call, tools/bwd2_micro.py)
    static const bool lag = env_not_zero("NGNN_B2_LAG");
    static const int dbg_env = kB2DbgBuild ? env_int("NGNN_B2_DBG", 0) : 0;
    const bool root = B.root();
    const int dbg = (root && lag && dbg_env == 1) ? 1 : 0;
    // (+ the chunk maxima: [2][8] float4)
    const size_t lds = static_cast<size_t>(2) * BUF * 2 + 2 * 256 * 4 + 480 * 4 + 2 * 8 * 16;
    with_const<1, 0>(B.indexed(), [&](auto xr_c) {
    with_const<4, 7, 8>(B.K0 <= 64 ? 4 : B.K0 <= 112 ? 7 : 8, [&](auto kt_c) {
    with_const<0, 1>(root, [&](auto root_c) {
    with_const<1, 0>(lag, [&](auto lag_c) {
    with_const<1, 0>(dbg, [&](auto dbg_c) {
        constexpr bool ROOT = decltype(root_c)::value != 0, LAG = decltype(lag_c)::value != 0;
        constexpr bool XR = decltype(xr_c)::value != 0 && ROOT;  // (root-free: x is not read)
        constexpr int DBG = decltype(dbg_c)::value;
        if constexpr (DBG == 0 || (kB2DbgBuild && ROOT && LAG)) {
            constexpr auto fn = k_bwd2<XR, decltype(kt_c)::value, LAG, ROOT, DBG>;
            max_dynamic_lds_once<fn>(lds);
            hipLaunchKernelGGL(fn, dim3(B2_S * B2_NCH), dim3(B2_THREADS), lds, st, b);
        }
    }); }); }); }); });
    return launch_status();
}

// ngnn_adam_fold in the reduce's tensor order (zeros without one)
AdamFold adam_fold(const ngnn_adam_fold *adam) {
    AdamFold af{};
    if (!adam) return af;
    // (the header's order dW_l1, db1, dW_r1, dW_l0, db0, dW_r0 -> the reduce's)
    static const int ord[6] = {5, 3, 4, 2, 0, 1};
    for (int k = 0; k < 6; ++k) {
        af.p[k] = adam->param[ord[k]];
        af.m[k] = adam->exp_avg[ord[k]];
        af.v[k] = adam->exp_avg_sq[ord[k]];
    }
    af.step = adam->step;
    af.lr = adam->lr, af.b1 = adam->beta1, af.b2 = adam->beta2, af.eps = adam->eps, af.wd = adam->weight_decay;
    af.gate = adam->gate, af.gate_gen = adam->gate_gen;
    return af;
}

}  // namespace
}  // namespace ngnn

using namespace ngnn;

extern "C" size_t ngnn_sage2_bwd_workspace_bytes(int64_t n_rows, int64_t K0, int64_t F1) {
    if (n_rows < 0 || K0 <= 0 || F1 <= 0) return 0;
    return ws3_layout(n_rows, K0, F1).total;
}

extern "C" int ngnn_sage2_bwd(const float *dy, int64_t ldy, int64_t F1, const float *wl1, const float *wr1,
                              int64_t ldw1, const float *h, int64_t ldh, float yscale, const float *x,
                              const float *const *x_dev, const int64_t *xrow, const int64_t *const *xrow_dev,
                              int64_t x_rows, int64_t ldx, int64_t K0, const float *agg0, int64_t ld_agg,
                              const int32_t *rowptr, const int32_t *col, int64_t n_rows, const int32_t *r_ptr,
                              const int32_t *rnext_ptr, int reduce, float *dwl1, float *dbl1, float *dwr1,
                              float *dwl0, float *dbl0, float *dwr0, const float *g_pre,
                              const ngnn_adam_fold *adam, void *ws, size_t ws_bytes, void *stream) {
    const Sage2Bwd B{dy, ldy, F1, wl1, wr1, ldw1, h, ldh, yscale, x, x_dev, xrow, xrow_dev, x_rows, ldx, K0, agg0,
                     ld_agg, rowptr, col, n_rows, r_ptr, rnext_ptr, reduce, dwl1, dbl1, dwr1, dwl0, dbl0, dwr0,
                     g_pre, adam, ws, ws_bytes};
    if (const int rc = sage2_bwd_check(B)) return rc;
    hipStream_t st = as_stream(stream);
    const Ws3 L = ws3_layout(n_rows, K0, F1);
    float *g = reinterpret_cast<float *>(static_cast<char *>(ws) + L.g);
    float *slab = reinterpret_cast<float *>(static_cast<char *>(ws) + L.slab);
    if (n_rows > 0 && !g_pre) {
        const int rc = lowdim_scatter_launch(dy, ldy, rowptr, col, static_cast<int>(n_rows), r_ptr,
                                             static_cast<int>(F1), B.C4(), g, reduce == NGNN_REDUCE_MEAN, st);
        if (rc) return rc;
    }
    if (const int rc = launch_bwd2(B, bwd2_args(B, g, slab), st)) return rc;
    const int n_red = static_cast<int>(ceil_div(b2_slab_floats(static_cast<int>(K0), static_cast<int>(F1)), 256));
    const int n_clr = g_pre ? 0 : 64;
    with_const<1, 0>(adam != nullptr, [&](auto adam_c) {
        hipLaunchKernelGGL(k_bwd2_reduce<decltype(adam_c)::value != 0>, dim3(n_red + n_clr), dim3(256), 0, st, slab,
                           B2_S, static_cast<int>(K0), static_cast<int>(F1), dwr0, dwl0, dbl0, dwr1, dwl1, dbl1, g,
                           B.C4(), static_cast<int>(n_rows), r_ptr, rnext_ptr, n_red, adam_fold(adam));
    });
    return launch_status();
}
