// Row-tile fused SAGEConv layer forward for gfx950 (the default forward path
// of ngnn_sage_fwd whenever the packed W_r fits in LDS).
//
// Same contract as the 64-row kernel in ngnn_sage.hip (one SAGEConv layer of
// sage.py:33-39: out = act(b + x W_r^T + [deg>0] agg(x) W_l^T), relu, hash
// dropout), re-decomposed for the MFMA / store-issue balance that kernel's
// ablation showed (profiles/ablation_r01: its dword-store epilogue alone ran
// at 1.85 TB/s, and the MFMA loop at ~55 % of the f32 MFMA rate):
//
//   * one 512-thread workgroup per CU, persistent; W_r (and W_l when both
//     fit) is copied ONCE per workgroup into LDS in fragment order (the
//     ngnn_pack_weight layout), bias too;
//   * each wave owns 16-row tiles: tile t -> workgroup t % G, wave
//     (t / G) % 8, so consecutive tiles (NeighborLoader puts every row with
//     in-edges first) spread over all CUs and both waves of a SIMD;
//   * MFMA operands are swapped w.r.t. the 64-row kernel: A = W (16 output
//     features from LDS, one ds_read_b128 = 4 k-steps), B = x (16 graph rows
//     straight from HBM into registers, no LDS staging, no barrier), so each
//     lane ends with 4 CONSECUTIVE output features of one row -> 16-B stores;
//   * the next tile's x fragments are prefetched before the current tile's
//     MFMAs; W fragments for the next k-step are read before the current
//     k-step's MFMAs (two register sets);
//   * tiles whose rows have in-edges gather the aggregate into registers in
//     the same lane layout (per column, edge order, then / max(deg,1): the
//     fp32 sequence of ngnn_seg_agg_fwd, so the aggregate is bit-identical),
//     neighbour indices preloaded 16 per row and broadcast by ds_bpermute.
//
// Root-term arithmetic (X3, the default): fp32-accurate 3 x bf16 split MFMA.
// x and W_r are each split v = v1 + v2 + v3 (bf16, round to nearest: |v -
// v1 - v2 - v3| <= 2^-27 |v|) and x.W_r^T is accumulated in fp32 from the six
// products whose magnitude reaches 2^-18 of the leading term (v1w1, v1w2,
// v2w1, v2w2, v1w3, v3w1; each bf16 x bf16 product is exact in fp32; the
// three dropped terms are <= 2^-26 relative) on v_mfma_f32_16x16x32_bf16:
// 6 bf16 MFMAs at 16 cycles = 96 cycles per 32-deep k-chunk vs 8 fp32
// 16x16x4 MFMAs at 32 = 256.  The error is below the fp32 rounding of the
// reference's own GEMM.  A tail of K % 32 <= 12 columns
// runs on exact fp32 MFMA steps (cheaper than a padded bf16 chunk).  With
// NGNN_MATH_EXACT_F32 OR-ed into `reduce`, every product is exact-fp32
// v_mfma_f32_16x16x4_f32 (a fmaf chain).  The neighbour term (edge tiles)
// stays on exact fp32 MFMA with W_l fp32.
//
// Bytes per launch: 4*(N*K + E*K + E + N + 1 + N*F_out) (x, gathered rows,
// col, rowptr, out) + the optional saved aggregate; flops 2*N*K*F_out +
// 2*N_edge_rows*K*F_out.
#include <cstdlib>

#include "ngnn_sage_rt_kern.h"

namespace ngnn {
int g_num_cus[64];

int num_cus() {
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (dev < 0 || dev >= 64) return 256;
    if (!g_num_cus[dev]) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
            n = 256;
        g_num_cus[dev] = n;
    }
    return g_num_cus[dev];
}

namespace {

// (NTW, reduce) -> the instantiation unit's entry (ngnn_rt_tu.hip)
int dispatch_rt(int ntw, const RtArgs &a, int reduce, bool wl_lds, bool x3, int n_tiles,
                size_t lds, hipStream_t st) {
#define NGNN_RT_CALL(N, R) \
    if (ntw == N && reduce == R) return NGNN_RT_FN(N, R)(a, wl_lds, x3, n_tiles, lds, st);
    NGNN_RT_FOR_EACH(NGNN_RT_CALL)
#undef NGNN_RT_CALL
    return NGNN_E_ARG;
}

// ---- narrow-mode neighbour term: out[d, :Fo] += reduce_{e into d} z[col[e], :Fo]
// for rows d with in-edges below min(n_rows, *n_rows_dev, *n_edge_rows_dev):
// mean/sum of z = x W_l^T (linear, so equal to W_l . mean(x) up to fp32
// rounding).  16 lanes per row (float4 columns), 4 rows per wave, 8
// neighbour rows in flight per lane; per column edge order from 0, then
// / deg for mean.
constexpr int NA_UNR = 16;

// max / sum over the 16 lanes of a row group (a DPP row: lanes 16 k ..
// 16 k + 15, all active together) on VALU only: quad_perm [1,0,3,2] and
// [2,3,0,1] combine a quad, row_half_mirror the two quads of a half,
// row_mirror the two halves -- every lane ends with the row's value
__device__ __forceinline__ float max16(float v) {
    v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, false)));
    v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xF, 0xF, false)));
    v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x141, 0xF, 0xF, false)));
    return fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x140, 0xF, 0xF, false)));
}
__device__ __forceinline__ float sum16(float v) {
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, false));
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xF, 0xF, false));
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x141, 0xF, 0xF, false));
    return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x140, 0xF, 0xF, false));
}

// HEAD (the loss head, ngnn_xent_head): the rows d < B are visited with or
// without in-edges; once a row's logits are final the group takes its cross
// entropy -- max, sum of exp and the label's logit over the group, the
// gradient row (softmax - onehot) / count as ngnn_seed_xent_fwd_grad writes
// it -- and scatters the gradient row onto its sources (g[col[e]] += dy[d] /
// deg(d), as the backward's narrow scatter).  count: every workgroup that
// holds seed rows counts the valid labels itself (B label reads from L2, no
// count pass).  The loss: per-group sums in row order, per workgroup in
// group order, and the last workgroup to finish (a device ticket) adds the
// workgroup partials in a fixed order -- deterministic; the hand-off is
// k_xent_fused's (ngnn_loss.hip: agent-scope partial stores drained before
// one ticket atomic, agent-scope loads by the last adder).
// WIDE: z row offsets by a full 32-bit multiply (n_rows or the row bytes past
// 24 bits); else v_mul_u32_u24.  Edge offsets are unsigned 32-bit: col reads
// are exact below 2^30 edges (the resource's 3.75 GiB range).
template <bool MEAN, bool HEAD, bool WIDE = false>
__global__ __launch_bounds__(256) void k_narrow_agg(const float *__restrict__ z, int64_t ldz, int Fo,
                                                    const int32_t *__restrict__ rowptr,
                                                    const int32_t *__restrict__ col, int n_rows,
                                                    const int32_t *__restrict__ n_rows_dev,
                                                    const int32_t *__restrict__ n_edge_dev,
                                                    float *__restrict__ out, int64_t ldo, NarrowHead hd) {
    int nr = n_rows;
    if (n_rows_dev) nr = min(nr, *n_rows_dev);
    if (n_edge_dev) nr = min(nr, *n_edge_dev);
    const int sub = threadIdx.x & 15;
    const int F4 = (Fo + 3) >> 2;
    // index words through buffer resources (masked slots read 0, no
    // branches): a row's first 16 neighbour ids in ONE round trip, then its
    // 16 z rows in one more (a fanout of <= 16 needs exactly two)
    const i32x4 cr = make_rsrc(col, 0xF0000000u);
    const uint32_t ldz4 = static_cast<uint32_t>(ldz) * 4u;
    constexpr int OOB = static_cast<int>(0xF0000000u);
    // the neighbour mean / sum of z of row d, columns 4 c4 .. 4 c4 + 3
    auto gather = [&](int beg, int end, int c4) __attribute__((always_inline)) {
        v4f acc{0.f, 0.f, 0.f, 0.f};
        for (int e = beg; e < end; e += NA_UNR) {
            int id[NA_UNR];
#pragma unroll
            for (int u = 0; u < NA_UNR; ++u)
                id[u] = buf_load1i(cr, e + u < end ? static_cast<int>(4u * static_cast<uint32_t>(e + u)) : OOB, 0, 0);
            const i32x4 zr = make_rsrc(z, 0xF0000000u);
            v4f v[NA_UNR];
#pragma unroll
            for (int u = 0; u < NA_UNR; ++u)
                v[u] = buf_load4(zr, e + u < end ? static_cast<int>((WIDE ? static_cast<uint32_t>(id[u]) * ldz4
                                                               : __umul24(static_cast<uint32_t>(id[u]), ldz4))) + 16 * c4
                                                  : OOB,
                                 0, 0);
#pragma unroll
            for (int u = 0; u < NA_UNR; ++u)
                if (e + u < end) acc += v[u];
        }
        if (MEAN && end > beg) acc = acc / static_cast<float>(end - beg);
        return acc;
    };
    const int stride = (gridDim.x * blockDim.x) >> 4;
    if constexpr (!HEAD) {
        for (int d = (blockIdx.x * blockDim.x + threadIdx.x) >> 4; d < nr; d += stride) {
            const int beg = rowptr[d], end = rowptr[d + 1];
            if (beg == end) continue;
            for (int c4 = sub; c4 < F4; c4 += 16) {
                const v4f acc = gather(beg, end, c4);
                float *o = out + static_cast<int64_t>(d) * ldo + 4 * c4;
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (4 * c4 + j < Fo) o[j] += acc[j];
            }
        }
    } else {
        // (host: F4 <= 16, one column quad per lane; B <= n_rows)
        __shared__ float s_red[256];
        __shared__ float s_grp[16];
        // rows to workgroups as the plain kernel's (16 consecutive row slots
        // per workgroup and pass), except that the first 2 B8 slots (B8 =
        // ceil8(B)) interleave: a workgroup's groups 0-7 take 8 consecutive
        // seed rows, groups 8-15 the 8 rows B8 + the same offset -- the seed
        // rows, and their scatter atomics, spread over twice the workgroups
        // with the row locality kept.  (Measured alternatives,
        // tools/fwd2_micro.py --head: seed rows one per workgroup over all
        // of them spread the atomics but cost the rest of the launch its row
        // locality, 36 us against 18; 4 per workgroup on wave 0 of ceil(B /
        // 4) workgroups, 25.)
        const int B = hd.B, G = static_cast<int>(gridDim.x), bx = static_cast<int>(blockIdx.x);
        const int B8 = (B + 7) & ~7;
        const int nh = min(G, B8 >> 3);  // workgroups holding seed rows
        const bool hwg = bx < nh;              // (uniform)
        float cnt = 0.0f;
        if (hd.cnt_in) {
            cnt = *hd.cnt_in;
        } else if (hwg) {
            float c = 0.0f;
            for (int i = threadIdx.x; i < B; i += 256) c += (hd.y[i] != hd.ignore) ? 1.0f : 0.0f;
            s_red[threadIdx.x] = c;
            __syncthreads();
            for (int h = 128; h > 0; h >>= 1) {
                if (threadIdx.x < h) s_red[threadIdx.x] += s_red[threadIdx.x + h];
                __syncthreads();
            }
            cnt = s_red[0];
        }
        float lsum = 0.0f;
        const int c4 = sub;
        const i32x4 zr = make_rsrc(z, 0xF0000000u);
        // the seed-edge counts of this call (the selector read once; the
        // loss's last adder flips it below, after every head workgroup read it)
        int ssel = 0;
        i32x4 scr = make_rsrc(nullptr, 0u);
        if (hd.scnt_base && hwg) {
            ssel = hd.scnt_base[2 * hd.scnt_stride] & 1;
            scr = make_rsrc(hd.scnt_base + ssel * hd.scnt_stride, static_cast<uint32_t>(hd.scnt_stride) * 4u);
        }
        const int dl = max(nr, B);
        const int vl = max(dl, 2 * B8);
        for (int v = (bx * 256 + static_cast<int>(threadIdx.x)) >> 4; v < vl; v += 16 * G) {
            const int vg = v & 15;
            const int d = v < 2 * B8 ? ((v >> 4) << 3) + (vg & 7) + (vg >= 8 ? B8 : 0) : v;
            if (d >= dl) continue;
            const bool hrow = d < B;
            const int beg = rowptr[d], end = (d < nr) ? rowptr[d + 1] : beg;
            if (beg == end && !hrow) continue;
            // the label, the root logits and the first 16 neighbour ids in
            // one round trip; the ids stay in registers for the scatter
            const int64_t t = hrow ? hd.y[d] : 0;
            float *o = out + static_cast<int64_t>(d) * ldo + 4 * c4;
            v4f ov{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (4 * c4 + j < Fo) ov[j] = o[j];
            int id[NA_UNR];
#pragma unroll
            for (int u = 0; u < NA_UNR; ++u) id[u] = buf_load1i(cr, beg + u < end ? 4 * (beg + u) : OOB, 0, 0);
            v4f acc{0.f, 0.f, 0.f, 0.f};
            // a seed row's sources' edge counts (1: the source's g row takes
            // one plain store); read with the gathers, used at the scatter
            int scn[NA_UNR];
#pragma unroll
            for (int u = 0; u < NA_UNR; ++u)
                scn[u] = buf_load1i(scr, (hrow && beg + u < end) ? static_cast<int>(4u * static_cast<uint32_t>(id[u])) : OOB, 0, 0);
            if (c4 < F4 && end > beg) {
                v4f v[NA_UNR];
#pragma unroll
                for (int u = 0; u < NA_UNR; ++u)
                    v[u] = buf_load4(zr, beg + u < end ? static_cast<int>(__umul24(static_cast<uint32_t>(id[u]), ldz4)) + 16 * c4 : OOB,
                                     0, 0);
#pragma unroll
                for (int u = 0; u < NA_UNR; ++u)
                    if (beg + u < end) acc += v[u];
                // (rare: more than 16 neighbours -- the rest in further round trips,
                // edge order kept: the sum continues from the first 16)
                for (int e = beg + NA_UNR; e < end; e += NA_UNR) {
                    int ie[NA_UNR];
#pragma unroll
                    for (int u = 0; u < NA_UNR; ++u) ie[u] = buf_load1i(cr, e + u < end ? 4 * (e + u) : OOB, 0, 0);
#pragma unroll
                    for (int u = 0; u < NA_UNR; ++u)
                        v[u] = buf_load4(zr, e + u < end ? static_cast<int>(__umul24(static_cast<uint32_t>(ie[u]), ldz4)) + 16 * c4 : OOB,
                                         0, 0);
#pragma unroll
                    for (int u = 0; u < NA_UNR; ++u)
                        if (e + u < end) acc += v[u];
                }
                if (MEAN) acc = acc / static_cast<float>(end - beg);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (4 * c4 + j < Fo && end > beg) {
                    ov[j] = ov[j] + acc[j];
                    o[j] = ov[j];  // (edgeless rows keep their bits, -0.0 included)
                }
            if (!hrow) continue;
            if (hd.dbg & 4) continue;  // (profiling: no cross entropy)
            // the row's cross entropy (torch's log_softmax order: max, then
            // the sum of exp(x - max))
            float m = -INFINITY;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (4 * c4 + j < Fo) m = fmaxf(m, ov[j]);
            m = max16(m);
            float s = 0.0f, ot = 0.0f;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (4 * c4 + j < Fo) {
                    s += expf(ov[j] - m);
                    if (4 * c4 + j == t) ot = ov[j];
                }
            s = sum16(s);
            ot = sum16(ot);  // (the label's logit: one lane holds it, the others add 0)
            const float lse = m + logf(s);
            const bool ign = t == hd.ignore;
            const float l = ign ? 0.0f : ((t >= 0 && t < Fo) ? lse - ot : NAN);  // out-of-range label: NaN
            v4f dv{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (4 * c4 + j < Fo && !ign) dv[j] = (expf(ov[j] - lse) - (4 * c4 + j == t ? 1.0f : 0.0f)) / cnt;
            float *dr = hd.dy + static_cast<int64_t>(d) * hd.ldd + 4 * c4;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (4 * c4 + j < Fo) dr[j] = dv[j];
            if (hd.g && !ign && end > beg && !(hd.dbg & 1)) {
                if (MEAN) dv = dv * (1.0f / static_cast<float>(end - beg));
                // the row's sources from the registers (no load between the
                // atomics); past 16 neighbours, reloaded 16 at a time
#pragma unroll
                for (int u = 0; u < NA_UNR; ++u)
                    if (beg + u < end) {
                        float *gr = hd.g + static_cast<int64_t>(id[u]) * hd.ldg + 4 * c4;
                        if (scn[u] == 1) {
                            // the source's only seed edge: its g row (zeroed by
                            // the edge launch) is this row's contribution
                            if (c4 < F4) *reinterpret_cast<v4f *>(gr) = dv;
                        } else {
#pragma unroll
                            for (int j = 0; j < 4; ++j)
                                if (4 * c4 + j < Fo && dv[j] != 0.0f) atomicAdd(gr + j, dv[j]);  // exact 0 adds nothing
                        }
                    }
                for (int e = beg + NA_UNR; e < end; e += NA_UNR) {
                    int ie[NA_UNR];
#pragma unroll
                    for (int u = 0; u < NA_UNR; ++u) ie[u] = buf_load1i(cr, e + u < end ? 4 * (e + u) : OOB, 0, 0);
#pragma unroll
                    for (int u = 0; u < NA_UNR; ++u)
                        if (e + u < end) {
                            float *gr = hd.g + static_cast<int64_t>(ie[u]) * hd.ldg + 4 * c4;
#pragma unroll
                            for (int j = 0; j < 4; ++j)
                                if (4 * c4 + j < Fo && dv[j] != 0.0f) atomicAdd(gr + j, dv[j]);
                        }
                }
            }
            lsum += l;
        }
        if (hwg && !(hd.dbg & 2)) {
            // the loss: the workgroup's rows in group order, then a two-level
            // hand-off by one lane behind an LDS-only barrier (the waves'
            // scatter atomics and stores stay in flight) -- groups of 32
            // workgroups count on their own ticket, the last of a group adds
            // the group's partials in order and counts on the top ticket,
            // whose last adds the group sums in order (same-address atomics
            // serialise at the memory side: 32 per address instead of one per
            // workgroup)
            if (sub == 0) s_grp[threadIdx.x >> 4] = lsum;
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            float p = 0.0f;
            for (int i = 0; i < 16; ++i) p += s_grp[i];
            if (threadIdx.x == 0) {
                float *gpart = hd.part;            // [32] group sums
                float *wpart = hd.part + 32;       // [nh] workgroup partials
                uint32_t *tick1 = hd.ticket + 16;  // [32] group tickets
                __hip_atomic_store(wpart + bx, p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                const int gi = bx >> 5, g0 = gi << 5, gs = min(32, nh - g0), ngr = (nh + 31) >> 5;
                if (atomicAdd(tick1 + gi, 1u) == static_cast<uint32_t>(gs - 1)) {
                    float v[32];
#pragma unroll
                    for (int i = 0; i < 32; ++i)
                        v[i] = i < gs ? __hip_atomic_load(wpart + g0 + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0f;
                    float a = 0.0f;
#pragma unroll
                    for (int i = 0; i < 32; ++i) a += v[i];
                    tick1[gi] = 0u;  // (every member has counted: ready for the next call)
                    __hip_atomic_store(gpart + gi, a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    if (atomicAdd(hd.ticket, 1u) == static_cast<uint32_t>(ngr - 1)) {
#pragma unroll
                        for (int i = 0; i < 32; ++i)
                            v[i] = i < ngr ? __hip_atomic_load(gpart + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0f;
                        float t = 0.0f;
#pragma unroll
                        for (int i = 0; i < 32; ++i) t += v[i];
                        *hd.loss = t / cnt;  // 0/0 = NaN when every row is ignored, as torch
                        *hd.count = cnt;
                        *hd.ticket = 0u;
                        // the next call's edge launch counts into the other array
                        if (hd.scnt_base) hd.scnt_base[2 * hd.scnt_stride] = ssel ^ 1;
                    }
                }
            }
        }
    }
}

// ---- GCNConv(normalize=False) aggregation of transformed rows, with the
// layer epilogue: out[d] = act(sum_{e into d} z[col[e]] + b) for EVERY row
// d < min(n_rows, *n_rows_dev) (rows without in-edges: act(b)) -- PyG's
// propagate(lin(x)) (aggr='add', edge order from 0) then + bias
// (convolution.py:29-35).  ReLU and the quad-hash dropout exactly as the
// row-tile epilogue (global column keys, col_base 0).  16 lanes per row,
// float4 columns, 8 neighbour rows in flight per lane.
template <bool VEC>
__global__ __launch_bounds__(256) void k_gcn_agg(const float *__restrict__ z, int64_t ldz, int Fo,
                                                 const int32_t *__restrict__ rowptr,
                                                 const int32_t *__restrict__ col, int n_rows,
                                                 const int32_t *__restrict__ n_rows_dev,
                                                 const float *__restrict__ bias, Epi epi,
                                                 const uint64_t *__restrict__ seed_dev,
                                                 float *__restrict__ out, int64_t ldo) {
    int nr = n_rows;
    if (n_rows_dev) nr = min(nr, *n_rows_dev);
    if (seed_dev) epi.drop.reseed(*seed_dev);
    const int sub = threadIdx.x & 15;
    const int F4 = (Fo + 3) >> 2;
    for (int d = (blockIdx.x * blockDim.x + threadIdx.x) >> 4; d < nr; d += (gridDim.x * blockDim.x) >> 4) {
        const int beg = rowptr[d], end = rowptr[d + 1];
        const uint32_t rk = epi.drop.thresh ? epi.drop.row_key(static_cast<uint32_t>(d)) : 0u;
        for (int c4 = sub; c4 < F4; c4 += 16) {
            v4f acc{0.f, 0.f, 0.f, 0.f};
            for (int e = beg; e < end; e += NA_UNR) {
                v4f v[NA_UNR];
#pragma unroll
                for (int u = 0; u < NA_UNR; ++u) {
                    const int ee = min(e + u, end - 1);
                    v[u] = *reinterpret_cast<const v4f *>(z + static_cast<int64_t>(col[ee]) * ldz + 4 * c4);
                }
#pragma unroll
                for (int u = 0; u < NA_UNR; ++u)
                    if (e + u < end) acc += v[u];
            }
            const uint32_t k4 = epi.drop.thresh ? epi.drop.keep4(rk, static_cast<uint32_t>(c4)) : 0xfu;
            v4f o;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = 4 * c4 + j;
                float y = acc[j] + ((bias && c < Fo) ? bias[c] : 0.0f);
                bool zero = epi.relu && y < 0.0f;  // NaN passes, like torch.relu
                if (epi.drop.thresh) zero = zero || !((k4 >> j) & 1u);
                o[j] = zero ? 0.0f : (epi.drop.thresh ? y * epi.drop.scale : y);
            }
            float *op = out + static_cast<int64_t>(d) * ldo + 4 * c4;
            if (VEC) {
                *reinterpret_cast<v4f *>(op) = o;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (4 * c4 + j < Fo) op[j] = o[j];
            }
        }
    }
}

// W_l [Fo, K] (bf16-exact fp32 values, row stride ldw) -> the bf16 image
// [NT][CL][64] x 8 of the row-tile kernel's bf16 neighbour term (RtArgs::wlb):
// element j of lane (q, m) in chunk c is W_l[16 t + m][32 c + 4 q + j] (j < 4)
// or [32 c + 16 + 4 q + j - 4] (j >= 4); zero outside Fo x K.  One thread per
// element (RNE conversion -- exact on bf16-exact weights).
__global__ __launch_bounds__(256) void k_pack_wl_b16(const float *__restrict__ w, int64_t ldw, int Fo, int K,
                                                     int CL, int NT, uint16_t *__restrict__ dst) {
    const int64_t idx = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
    if (idx >= static_cast<int64_t>(NT) * CL * 512) return;
    const int j = idx & 7, lane = (idx >> 3) & 63;
    const int64_t tc = idx >> 9;
    const int c = static_cast<int>(tc % CL), t = static_cast<int>(tc / CL);
    const int q = lane >> 4, n = 16 * t + (lane & 15);
    const int k = 32 * c + (j < 4 ? 4 * q + j : 16 + 4 * q + j - 4);
    const float v = (n < Fo && k < K) ? w[static_cast<int64_t>(n) * ldw + k] : 0.0f;
    dst[idx] = __builtin_bit_cast(uint16_t, static_cast<__bf16>(v));
}

}  // namespace

// bytes of the bf16 W_l image (k_pack_wl_b16)
size_t wl_b16_bytes(int64_t Fo, int64_t K) {
    return static_cast<size_t>(ceil_div(Fo, 16)) * static_cast<size_t>(ceil_div(K, 32)) * 64 * 16;
}

// out[d, :Fo] += mean / sum_{e into d} z[col[e], :Fo] for the rows with
// in-edges (the narrow output layer's neighbour term; also ngnn_fwd2.hip);
// head (nullable): the loss head over rows < head->B (ngnn_fwd2.hip)
int narrow_agg_launch(const float *z, int64_t ldz, int64_t Fo, const int32_t *rowptr, const int32_t *col,
                      int64_t n_rows, const int32_t *n_rows_dev, int64_t n_edge_rows,
                      const int32_t *n_edge_rows_dev, int reduce, float *out, int64_t ldo, hipStream_t st,
                      const NarrowHead *head) {
    const int64_t rows = std::max<int64_t>(1, std::min(n_edge_rows, n_rows));
    // (32-bit buffer offsets into z; past 24-bit rows or row bytes the z
    // offsets take the full multiply: k_narrow_agg<..., WIDE>)
    NGNN_RETURN_IF(n_rows * ldz * 4 >= 0xF0000000ll, NGNN_E_RANGE);
    const bool wide = n_rows >= (1 << 24) || ldz * 4 >= (1 << 24);
    NGNN_RETURN_IF(head && (Fo > 64 || head->B <= 0 || head->B > n_rows), NGNN_E_ARG);
    NGNN_RETURN_IF(head && n_rows >= (1 << 24), NGNN_E_RANGE);
    const unsigned grid = static_cast<unsigned>(
        std::max<int64_t>(1, std::min<int64_t>(head ? std::min(4 * num_cus(), 1024) : 4 * num_cus(),
                                               ceil_div(std::max<int64_t>(rows, head ? 2 * ((head->B + 7) & ~int64_t{7}) : 0), 16))));
    // (the head's hand-off: at most 32 groups of 32 workgroups)
    const NarrowHead hd = head ? *head : NarrowHead{};
    auto go = [&](auto mean_c, auto head_c) {
        if (wide && !decltype(head_c)::value)  // (the loss head's blocks are NeighborLoader-sized)
            hipLaunchKernelGGL((k_narrow_agg<decltype(mean_c)::value, false, true>), dim3(grid), dim3(256), 0,
                               st, z, ldz, static_cast<int>(Fo), rowptr, col, static_cast<int>(n_rows), n_rows_dev,
                               n_edge_rows_dev, out, ldo, hd);
        else
            hipLaunchKernelGGL((k_narrow_agg<decltype(mean_c)::value, decltype(head_c)::value>), dim3(grid), dim3(256),
                               0, st, z, ldz, static_cast<int>(Fo), rowptr, col, static_cast<int>(n_rows), n_rows_dev,
                               n_edge_rows_dev, out, ldo, hd);
    };
    const bool mean = reduce == NGNN_REDUCE_MEAN;
    if (head) {
        if (mean) go(std::true_type{}, std::true_type{});
        else go(std::false_type{}, std::true_type{});
    } else {
        if (mean) go(std::true_type{}, std::false_type{});
        else go(std::false_type{}, std::false_type{});
    }
    return launch_status();
}

// The row-tile kernel's LDS envelope (declared in ngnn_device.h)
RtImage rt_root_image(int64_t K, bool x3, bool w1, bool no_root, int max_ntw) {
    RtImage im{};
    im.C = static_cast<int>(K / 32);
    im.T4 = static_cast<int>(ceil_div(K % 32, 4));
    if (im.T4 > X3_TAIL_MAX) {
        im.C += 1;
        im.T4 = 0;
        im.kpad = 1;
    }
    // (no root term: the X3 layout with an empty image -- no MFMAs, no LDS)
    if (no_root) im.C = im.T4 = im.kpad = 0;
    im.frag_kb = static_cast<size_t>(ceil_div(K, 16)) * 64 * sizeof(v4f);
    im.root_kb = x3 ? (static_cast<size_t>((w1 ? 1 : 3) * im.C) * 64 * 16 + static_cast<size_t>(im.T4) * 64 * 4)
                    : im.frag_kb;
    // (no root term: the slice width is set by the W_l image alone)
    const size_t img_kb = no_root ? im.frag_kb : im.root_kb;
    for (int c : {16, 8, 6, 4, 3, 2})
        if (c <= max_ntw && static_cast<size_t>(c) * img_kb <= kRtLdsCap) {
            im.ntw_max = c;
            break;
        }
    return im;
}

namespace {

// ---- sage_fwd_rowtile's steps: plan, per-slice W_l staging, launch.  The
// plan: a layer's form and its column slicing -- outputs wider than one slice
// (<= 256 columns, fewer when K is large) run as one launch per slice.
struct RtPlan {
    bool x3;  // root term in the X3 layout (3 x bf16 split; also "no root term")
    bool w1;  // bf16-exact weights (NGNN_W_BF16): a one-part image (MEAN / SUM kernels)
    bool narrow, no_root;
    int KG;
    RtImage im;
    int64_t slice;  // output columns per launch
};

// false: outside the envelope.  raw: PyG Linear rows (ldw > 0), else packed
// fragments.  narrow: one launch computes [x W_r^T | x W_l^T] (2 NT1 tiles),
// no column slicing -- both halves in one image.
bool rt_plan(int64_t K, int64_t Fo, bool raw, bool exact, bool w_bf16, int reduce, bool narrow, bool no_root,
             RtPlan &p) {
    p.x3 = (!exact && raw) || no_root;
    p.w1 = w_bf16 && p.x3 && !no_root && reduce != NGNN_REDUCE_MAX;
    p.narrow = narrow;
    p.no_root = no_root;
    p.KG = static_cast<int>(ceil_div(K, 16));
    p.im = rt_root_image(K, p.x3, p.w1, no_root, NGNN_RT_MAXNTW);
    if (p.im.ntw_max == 0 || (narrow && 2 * ceil_div(Fo, 16) > p.im.ntw_max)) return false;
    p.slice = narrow ? Fo : 16 * static_cast<int64_t>(p.im.ntw_max);
    return true;
}

// One column slice of Fo_c outputs: its tiles, the kernel instantiation and
// the dynamic LDS.  W_l (fp32) shares the LDS when both fit (wl_lds);
// otherwise its fragments stream from L2 (stage_wl).
struct RtSlice {
    int NT1, NT, NTW;
    bool wl_lds;
    size_t lds;
};

RtSlice rt_slice(const RtPlan &p, int64_t Fo_c, bool has_l) {
    RtSlice s;
    s.NT1 = static_cast<int>(ceil_div(Fo_c, 16));
    s.NT = p.narrow ? 2 * s.NT1 : s.NT1;
    s.NTW = s.NT <= 2 ? 2 : s.NT <= 3 ? 3 : s.NT <= 4 ? 4 : s.NT <= 6 ? 6 : s.NT <= 8 ? 8 : 16;
    const size_t rbytes = static_cast<size_t>(s.NTW) * p.im.root_kb;
    const size_t wbytes = static_cast<size_t>(s.NTW) * p.im.frag_kb;
    const size_t bbytes = static_cast<size_t>(s.NTW) * 16 * sizeof(float);
    s.wl_lds = has_l && rbytes + wbytes + bbytes <= kRtLdsCap + 1024;
    s.lds = rbytes + (s.wl_lds ? wbytes : 0) + bbytes;
    return s;
}

// The launch arguments of column slice [c0, c0 + Fo_c), but for a streamed
// W_l (stage_wl) and the prebuilt root image (build_image).
// (RtArgs::tile_end_dev is dead -- null, never read; removing it moves the
// later kernel arguments: for a change that re-measures)
RtArgs slice_args(const LayerFwd &L, const RtPlan &p, const RtSlice &s, int64_t c0, int64_t Fo_c, bool has_l,
                  const Dropout &drop) {
    RtArgs a{};
    a.x = L.x;
    a.ldx = L.ldx;
    a.K = static_cast<int>(L.K);
    a.KG = p.KG;
    a.n_rows = static_cast<int>(L.n_rows);
    a.n_rows_dev = L.n_rows_dev;
    a.rowptr = L.rowptr;
    a.col = L.col;
    // a slice's weights: packed fragments are n-tile major (contiguous
    // sub-array); raw weights are rows [c0, c0 + Fo_c)
    const int64_t woff = L.ldw ? c0 * L.ldw / 4 : (c0 / 16) * p.KG * 64;
    a.wl = has_l ? static_cast<const v4f *>(L.wl) + woff : nullptr;
    a.wr = p.no_root ? nullptr : static_cast<const v4f *>(L.wr) + woff;
    a.wr_raw = (L.ldw && !p.no_root) ? static_cast<const float *>(L.wr) + c0 * L.ldw : nullptr;
    a.ldw = L.ldw;
    a.C = p.im.C;
    a.T4 = p.im.T4;
    a.kpad = p.im.kpad;
    a.wlb_fo = static_cast<int>(L.Fo);
    a.CL = static_cast<int>(ceil_div(L.K, 32));
    a.NT = s.NT;
    a.NT1 = s.NT1;
    // (unknown: every row may have in-edges -- no root-only phase)
    a.n_edge = static_cast<int>(L.n_edge_rows < 0 ? L.n_rows : std::min(L.n_edge_rows, L.n_rows));
    a.n_edge_dev = L.n_edge_rows_dev;
    a.wz_raw = p.narrow ? static_cast<const float *>(L.wl) : nullptr;
    a.z = L.z;
    a.ldz = L.ldz;
    a.Fo = static_cast<int>(Fo_c);
    a.out = L.out_bf16 ? reinterpret_cast<float *>(reinterpret_cast<uint16_t *>(L.out) + c0) : L.out + c0;
    a.ldo = L.ldo;
    a.vec_out = (Fo_c % 4 == 0) && (L.ldo % 4 == 0) && aligned(a.out, L.out_bf16 ? 8 : 16);
    a.out_bf16 = L.out_bf16;
    a.agg_out = (c0 == 0 && !p.narrow && !L.agg_pre) ? L.agg_out : nullptr;
    a.ld_agg = L.ld_agg;
    // later column slices read the aggregate the first one saved (the
    // launches are stream-ordered) instead of gathering it again; agg_pre:
    // every slice reads it (written by a separate aggregate launch)
    a.agg_in = ((c0 > 0 || L.agg_pre) && !p.narrow && has_l) ? L.agg_out : nullptr;
    a.epi = Epi{L.bias ? L.bias + c0 : nullptr, L.relu, drop, static_cast<int>(c0)};
    a.seed_dev = L.seed_dev;
    a.x_dev = L.x_dev;
    a.xrow = L.xrow;
    a.xrow_dev = L.xrow_dev;
    a.x_rows = L.x_rows;
    a.col_x = (L.xrow || L.xrow_dev) ? L.col_x : nullptr;
    a.x_bf16 = L.x_bf16;
    a.w1 = p.w1;
    return a;
}

// W_l of slice c0 streamed from L2 (it does not fit the LDS beside the root
// image) out of the caller's workspace, packed there once, with the first
// slice: as fp32 fragments (ngnn_pack_weight's layout; NGNN_WL_PREPACKED: the
// producer keeps them current), or for one-part (bf16-exact) layers as the
// bf16 image behind them -- the neighbour term on bf16 MFMA, no fp32 pack.
// img_pre: the root image's own launch (build_image) packs W_l too, handed
// a.wlp_* / a.wlb_src, instead of a pack launch here.  Returns a workspace or
// launch error.
int stage_wl(const LayerFwd &L, const RtPlan &p, int64_t c0, bool img_pre, RtArgs &a, hipStream_t st) {
    const int64_t K = L.K, Fo = L.Fo;
    const float *wl = static_cast<const float *>(L.wl);
    if (L.ldw) {  // (packed weights stream as they are)
        if (c0 == 0 && !p.w1) {
            if (!L.ws || L.ws_bytes < ngnn_pack_weight_bytes(Fo, K)) return NGNN_E_WORKSPACE;
            if (img_pre && !L.wl_prepacked) {
                a.wlp_src = wl;
                a.wlp_dst = static_cast<v4f *>(L.ws);
                a.wlp_fo = static_cast<int>(Fo);
            } else if (!L.wl_prepacked) {
                const int rc = ngnn_pack_weight(wl, L.ldw, Fo, K, L.ws, st);
                if (rc) return rc;
            }
        }
        a.wl = static_cast<const v4f *>(L.ws) + (c0 / 16) * p.KG * 64;
    }
    if (p.w1) {
        if (!L.ldw || !L.ws || L.ws_bytes < ngnn_pack_weight_bytes(Fo, K) + wl_b16_bytes(Fo, K))
            return NGNN_E_WORKSPACE;
        uint16_t *img16 = reinterpret_cast<uint16_t *>(static_cast<char *>(L.ws) + ngnn_pack_weight_bytes(Fo, K));
        if (c0 == 0 && img_pre) {
            a.wlb_src = wl;
        } else if (c0 == 0) {
            const int NTa = static_cast<int>(ceil_div(Fo, 16));
            const int64_t total = static_cast<int64_t>(NTa) * a.CL * 512;
            hipLaunchKernelGGL(k_pack_wl_b16, dim3(static_cast<unsigned>(ceil_div(total, 256))), dim3(256), 0, st,
                               wl, L.ldw, static_cast<int>(Fo), static_cast<int>(K), a.CL, NTa, img16);
            const int rc = launch_status();
            if (rc) return rc;
        }
        a.wlb = img16 + (c0 / 16) * a.CL * 64 * 8;
    }
    return NGNN_OK;
}

// One slice's launches: k_sage_rt over all its tiles, or -- when a k_root
// instantiation (ngnn_root.hip) covers this layer -- k_sage_rt on the tiles
// with in-edges (none in narrow mode), then k_root on the tiles past the
// edge-row bound.
int launch_slice(RtArgs &a, const RtPlan &p, const RtSlice &s, int reduce, int n_tiles, hipStream_t st) {
    const bool vec = a.vec_out && (a.Fo == a.NT * 16);
    const int form = (p.x3 && !NGNN_RT_STATIC && !p.no_root) ? rt_form(a, s.NTW, vec) : 0;
    // policy (NGNN_ROOT, read once): 1 (default) k_root for layers with no
    // in-kernel neighbour term (narrow mode: every tile); 2 also split the
    // layers with edge tiles (k_sage_rt edge tiles, then k_root -- measured
    // slower on products layer 0: the edge tiles alone then hold the GPU
    // ~48 us, in one launch they overlap the root tiles); 0 never
    static const int policy = env_int("NGNN_ROOT", 1);
    const bool want_root = policy == 2 || (policy == 1 && !a.wl);
    if (form && want_root && launch_root(a, s.NTW, form, vec, st, true) == NGNN_OK) {
        if (a.wl) {
            a.root_split = 1;
            const int rc = dispatch_rt(s.NTW, a, reduce, s.wl_lds, p.x3, n_tiles, s.lds, st);
            if (rc) return rc;
            a.root_split = 0;
        }
        return launch_root(a, s.NTW, form, vec, st);
    }
    return dispatch_rt(s.NTW, a, reduce, s.wl_lds, p.x3, n_tiles, s.lds, st);
}

}  // namespace

// Returns 1 and stores the launch status in *rc when the row-tile kernel
// takes this call, 0 when the shape is outside its envelope (the caller then
// runs the 64-row kernel).  Envelope: no input mask, K % 4 == 0 with 16-B
// aligned rows, the W_r image of one column slice fitting in LDS (rt_plan /
// rt_root_image).  L.exact: fp32 MFMA for the root term (else the 3 x bf16
// split, raw weights only).
int sage_fwd_rowtile(const LayerFwd &L, hipStream_t st, int *rc) {
    // (with x_dev the run-time address must be 16-B aligned, as torch's are)
    if (L.K % 4 != 0 || L.ldx % 4 != 0 || (!L.x_dev && !aligned(L.x, 16))) return 0;
    if (L.ldw && (L.ldw % 4 != 0 || !aligned(L.wr, 16) || (L.wl && !aligned(L.wl, 16)))) return 0;
    const bool no_root = L.wr == nullptr;  // raw weights only (checked by the caller)
    if (L.agg_out && (L.ld_agg % 4 != 0 || !aligned(L.agg_out, 16))) return 0;
    // the gather reads neighbour rows through one resource over all of x
    // (unsigned 32-bit offsets below kOOB); every other operand is addressed
    // per 16-row tile (no size limit)
    const bool indexed = L.xrow != nullptr || L.xrow_dev != nullptr;
    // (a graph slot may load materialized batches too: the word then holds 0)
    const int64_t ebytes = L.x_bf16 ? 2 : 4;
    if ((indexed ? std::max(L.x_rows, L.n_rows) : L.n_rows) * L.ldx * ebytes > kRangeMax ||
        (indexed && L.x_rows <= 0))
        return 0;
    const bool narrow = L.z != nullptr;
    RtPlan p;
    if (!rt_plan(L.K, L.Fo, L.ldw > 0, L.exact, L.w_bf16, L.reduce, narrow, no_root, p)) return 0;
    // bf16 rows: X3 layout only, 8-B aligned rows (ldx a multiple of 4 elements)
    if (L.x_bf16 && !p.x3) return 0;
    // narrow mode: X3 only, no neighbour term, no saved aggregate
    if (narrow && (!p.x3 || !L.wl || L.ldz < ceil_div(L.Fo, 16) * 16 || L.ldz % 4 != 0 || !aligned(L.z, 16)))
        return 0;
    // (development builds hold the fp32 split-bf16 MEAN kernels only)
    if (NGNN_RT_FAST_BUILD && (!p.x3 || L.x_bf16 || p.w1 || L.reduce != NGNN_REDUCE_MEAN)) return 0;
    const Dropout drop = make_dropout(L.p_drop, L.seed);
    const bool has_l = L.wl != nullptr && !narrow;
    const int n_tiles = static_cast<int>(ceil_div(L.n_rows, RT_ROWS));
    for (int64_t c0 = 0; c0 < L.Fo; c0 += p.slice) {
        const int64_t Fo_c = std::min<int64_t>(p.slice, L.Fo - c0);
        const RtSlice s = rt_slice(p, Fo_c, has_l);
        RtArgs a = slice_args(L, p, s, c0, Fo_c, has_l, drop);
        // the split-bf16 root image built once (k_x3_image) into img_ws and
        // DMA-copied by every workgroup (else each workgroup builds it)
        const bool img_pre = p.x3 && !no_root && L.img_ws &&
                             x3_image_bytes(s.NTW, p.im.C, p.im.T4, p.w1) <= kImgWsBytes;
        if (has_l && !s.wl_lds && (*rc = stage_wl(L, p, c0, img_pre, a, st))) return 1;
        if (L.out_bf16 && !(a.vec_out && Fo_c % 16 == 0 && p.w1)) {  // bf16 rows: whole 16-column tiles of a one-part-image layer
            *rc = NGNN_E_SHAPE;
            return 1;
        }
        if (img_pre && (*rc = build_image(a, s.NTW, L.img_ws, st))) return 1;
        a.wlb_src = nullptr;
        a.wlp_src = nullptr;
        if ((*rc = launch_slice(a, p, s, L.reduce, n_tiles, st))) return 1;
    }
    return 1;
}

}  // namespace ngnn

using namespace ngnn;

extern "C" size_t ngnn_sage_fwd_raw_workspace_bytes(int64_t K, int64_t Fo, int64_t n_rows) {
    // a packed W_l (when it cannot sit in LDS), or narrow mode's z rows, or
    // the wide path's aggregate rows (inference: no saved-aggregate buffer)
    const size_t z = static_cast<size_t>(std::max<int64_t>(n_rows, 0)) * ceil_div(Fo, 16) * 16 *
                     sizeof(float);
    // (the wide tail: X3's 6-part weight image, or H2's 2-part image + its
    // row / column exponent arrays -- whichever is larger for these rows, so
    // the H2 form never drops back to X3 for want of room)
    const size_t nr = static_cast<size_t>(std::max<int64_t>(n_rows, 0));
    const size_t h2_tail = static_cast<size_t>(8) * Fo * ceil_div(K, 32) * 32 + (2 * Fo + 2 * nr) * 4 + 1024 + 512;
    const size_t wide = (sage_wide_preferred(K, Fo, false) || sage_wide_preferred(K, Fo, true))
                            ? sage_wide_workspace_bytes(K, n_rows) + std::max(wide_wimg_bytes(K, Fo), h2_tail) + 256
                            : 0;
    // + the prebuilt root image at the workspace's tail (kImgWsBytes); the
    // packed W_l is followed by its bf16 image (one-part layers)
    return std::max({ngnn_pack_weight_bytes(Fo, K) + wl_b16_bytes(Fo, K), z, wide}) + kImgWsBytes;
}

// The routing of ngnn_sage_fwd_raw below, without a call: its order (narrow
// mode, the wide path, the row-tile kernel) over the same rt_plan /
// sage_wide_preferred, for raw weights with a root term.
extern "C" int64_t ngnn_sage_fwd_slice_cols(int64_t K, int64_t Fo, int flags) {
    const bool exact = (flags & NGNN_MATH_EXACT_F32) != 0, narrow = (flags & NGNN_FWD_NARROW) != 0;
    const bool x_bf16 = (flags & NGNN_X_BF16) != 0, w_bf16 = (flags & NGNN_W_BF16) != 0;
    const bool out_bf16 = (flags & NGNN_OUT_BF16) != 0;
    const int reduce = flags & ~(NGNN_MATH_EXACT_F32 | NGNN_FWD_NARROW | NGNN_X_BF16 | NGNN_W_BF16 |
                                 NGNN_WL_PREPACKED | NGNN_OUT_BF16);
    NGNN_RETURN_IF(reduce < NGNN_REDUCE_SUM || reduce > NGNN_REDUCE_MAX || K <= 0 || Fo <= 0, NGNN_E_ARG);
    NGNN_RETURN_IF(!fits_i32(K) || !fits_i32(Fo), NGNN_E_RANGE);
    if ((x_bf16 && exact) || (out_bf16 && narrow) || K % 4 != 0) return 0;
    RtPlan p;
    if (narrow && reduce != NGNN_REDUCE_MAX && rt_plan(K, Fo, true, exact, w_bf16, reduce, true, false, p) && p.x3)
        return p.slice;
    if (!x_bf16 && !out_bf16 && sage_wide_preferred(K, Fo, exact)) return 0;
    if (!rt_plan(K, Fo, true, exact, w_bf16, reduce, false, false, p) || (x_bf16 && !p.x3)) return 0;
    return p.slice;
}

extern "C" int ngnn_sage_fwd_raw(const float *x, const float *const *x_dev, const int64_t *xrow,
                                 const int64_t *const *xrow_dev, int64_t x_rows, int64_t ldx,
                                 int64_t K, int64_t n_rows, const int32_t *n_rows_dev,
                                 int64_t n_edge_rows, const int32_t *n_edge_rows_dev,
                                 const int32_t *rowptr, const int32_t *col, const int32_t *col_x,
                                 int reduce, const float *wl, const float *wr,
                                 int64_t ldw, const float *bias, int64_t Fo, float *out,
                                 int64_t ldo, int relu, float p_drop, uint64_t seed,
                                 const uint64_t *seed_dev, float *agg_out, int64_t ld_agg, void *ws,
                                 size_t ws_bytes, void *stream) {
    // the flag bits of `reduce`, decoded once into the call descriptor
    LayerFwd L;
    L.exact = (reduce & NGNN_MATH_EXACT_F32) != 0;
    const bool want_narrow = (reduce & NGNN_FWD_NARROW) != 0;
    L.x_bf16 = (reduce & NGNN_X_BF16) != 0;
    L.w_bf16 = (reduce & NGNN_W_BF16) != 0;
    L.wl_prepacked = (reduce & NGNN_WL_PREPACKED) != 0;
    L.out_bf16 = (reduce & NGNN_OUT_BF16) != 0;
    reduce &= ~(NGNN_MATH_EXACT_F32 | NGNN_FWD_NARROW | NGNN_X_BF16 | NGNN_W_BF16 |
                NGNN_WL_PREPACKED | NGNN_OUT_BF16);
    // bf16 rows: the split-bf16 root term only
    if (L.x_bf16 && L.exact) return NGNN_E_SHAPE;
    if (L.out_bf16 && want_narrow) return NGNN_E_SHAPE;
    NGNN_RETURN_IF(reduce < NGNN_REDUCE_SUM || reduce > NGNN_REDUCE_MAX, NGNN_E_ARG);
    // wr == NULL: no root term (GCNConv = SAGEConv with W_r = 0: the layer
    // aggregates first, out = act(b + agg(x) W_l^T))
    NGNN_RETURN_IF(K <= 0 || Fo <= 0 || n_rows < 0 || (!wr && !wl), NGNN_E_ARG);
    NGNN_RETURN_IF(!wr && (want_narrow || ldw <= 0), NGNN_E_ARG);
    NGNN_RETURN_IF(wl && !rowptr, NGNN_E_ARG);
    NGNN_RETURN_IF(ldx < K || ldo < Fo || ldw < K, NGNN_E_SHAPE);
    NGNN_RETURN_IF(agg_out && ld_agg < K, NGNN_E_SHAPE);
    NGNN_RETURN_IF(!fits_i32(K) || !fits_i32(n_rows) || !fits_i32(Fo), NGNN_E_RANGE);
    NGNN_RETURN_IF(p_drop < 0.0f || !(p_drop <= 1.0f), NGNN_E_ARG);
    if (n_rows == 0) return NGNN_OK;
    NGNN_RETURN_IF((!x && !x_dev) || !out, NGNN_E_ARG);
    hipStream_t st = as_stream(stream);
    L.x = x, L.x_dev = x_dev, L.xrow = xrow, L.xrow_dev = xrow_dev, L.x_rows = x_rows, L.col_x = col_x, L.ldx = ldx;
    L.K = K, L.Fo = Fo, L.n_rows = n_rows, L.n_rows_dev = n_rows_dev;
    L.n_edge_rows = n_edge_rows, L.n_edge_rows_dev = n_edge_rows_dev;
    L.rowptr = rowptr, L.col = col, L.reduce = reduce;
    L.wl = wl, L.wr = wr, L.ldw = ldw, L.bias = bias;
    L.out = out, L.ldo = ldo, L.relu = relu, L.p_drop = p_drop, L.seed = seed, L.seed_dev = seed_dev;
    L.agg_out = agg_out, L.ld_agg = ld_agg, L.ws = ws, L.ws_bytes = ws_bytes;
    int rc = NGNN_OK;
    // narrow mode (MEAN / SUM): the neighbour term aggregated in the F_out-wide
    // space (z = x W_l^T, then a gather of z), no saved aggregate
    const int64_t ldz = ceil_div(Fo, 16) * 16;
    // the root image's region: the workspace's last kImgWsBytes (16-B aligned)
    // when the rest still holds z (narrow) / a packed W_l
    const size_t head = want_narrow ? static_cast<size_t>(n_rows) * ldz * sizeof(float)
                                    : ngnn_pack_weight_bytes(Fo, K) + wl_b16_bytes(Fo, K);
    // (NGNN_IMG=0, read once: every workgroup builds its image -- A/B only)
    static const bool img_on = env_int("NGNN_IMG", 1) != 0;
    if (img_on && ws && aligned(ws, 16) && ws_bytes >= head + kImgWsBytes + 16) {
        const uintptr_t e = (reinterpret_cast<uintptr_t>(ws) + ws_bytes - kImgWsBytes) & ~uintptr_t(15);
        L.img_ws = reinterpret_cast<void *>(e);
    }
    if (want_narrow && wl && reduce != NGNN_REDUCE_MAX && !agg_out && !relu && !(p_drop > 0.0f) &&
        ws && aligned(ws, 16) &&
        ws_bytes >= static_cast<size_t>(n_rows) * ldz * sizeof(float)) {
        LayerFwd n = L;  // (the workspace holds z; no saved aggregate)
        n.z = static_cast<float *>(ws);
        n.ldz = ldz;
        n.agg_out = nullptr;
        if (sage_fwd_rowtile(n, st, &rc)) {
            if (rc) return rc;
            return narrow_agg_launch(n.z, ldz, Fo, rowptr, col, n_rows, n_rows_dev, n_edge_rows,
                                     n_edge_rows_dev, reduce, out, ldo, st, nullptr);
        }
    }
    // wide layers (the row-tile kernel's weight image too large for its LDS,
    // or K % 4 != 0): aggregate launch + 2-D tiled dual GEMM
    // (x_dev: a graph slot's batch rows in place -- K % 4 != 0 rows too, the
    // wide kernels load them at 4-B alignment)
    if ((x || x_dev) && !xrow && !xrow_dev && !L.x_bf16 && !L.out_bf16 && sage_wide_preferred(K, Fo, L.exact) &&
        (agg_out || !wl || ws_bytes >= sage_wide_workspace_bytes(K, n_edge_rows)))
        return sage_fwd_wide(L, st);
    // max layers with a wide input: the aggregate by its own launch (a wave per
    // row, every column in flight) into the saved-aggregate buffer, which the
    // row-tile kernel's edge tiles then read densely -- its in-kernel gather
    // walks 16-row tiles one 128-column chunk at a time (Amazon-Computers'
    // 512 -> 10 layer: 67 us for ~3k rows with in-edges)
    // NGNN_AGGPRE (read once; A/B): 1 -- mean / sum layers too (layer 0 of
    // products: its 16.2 k rows with in-edges gathered at full occupancy
    // instead of inside the row-tile kernel, one wave per 16-row tile)
    static const int aggpre_all = env_int("NGNN_AGGPRE", 0);
    L.agg_pre = (reduce == NGNN_REDUCE_MAX ? K >= 256 : aggpre_all == 1) && wl && agg_out &&
                (x || x_dev) && !xrow && !xrow_dev && !L.x_bf16 && ld_agg % 4 == 0 &&
                aligned(agg_out, 16);
    if (L.agg_pre) {
        rc = sage_wide_aggregate(L, st);
        if (rc) return rc;
    }
    if (!sage_fwd_rowtile(L, st, &rc)) return NGNN_E_SHAPE;  // outside the row-tile envelope: pack + ngnn_sage_fwd
    return rc;
}

extern "C" int ngnn_gcn_agg_fwd(const float *z, int64_t ldz, int64_t Fo, const int32_t *rowptr,
                                const int32_t *col, int64_t n_rows, const int32_t *n_rows_dev,
                                const float *bias, int relu, float p_drop, uint64_t seed,
                                const uint64_t *seed_dev, float *out, int64_t ldo, void *stream) {
    NGNN_RETURN_IF(Fo <= 0 || n_rows < 0 || p_drop < 0.0f || !(p_drop <= 1.0f), NGNN_E_ARG);
    NGNN_RETURN_IF(ldz < ceil_div(Fo, 4) * 4 || ldz % 4 != 0 || ldo < Fo, NGNN_E_SHAPE);
    NGNN_RETURN_IF(!fits_i32(n_rows) || !fits_i32(Fo), NGNN_E_RANGE);
    if (n_rows == 0) return NGNN_OK;
    NGNN_RETURN_IF(!z || !rowptr || !col || !out, NGNN_E_ARG);
    NGNN_RETURN_IF(!aligned(z, 16), NGNN_E_ALIGN);
    const Epi epi{bias, relu, make_dropout(p_drop, seed), 0};
    const unsigned grid = static_cast<unsigned>(
        std::max<int64_t>(1, std::min<int64_t>(8 * num_cus(), ceil_div(n_rows, 16))));
    const bool vec = Fo % 4 == 0 && ldo % 4 == 0 && aligned(out, 16);
    if (vec)
        hipLaunchKernelGGL(k_gcn_agg<true>, dim3(grid), dim3(256), 0, as_stream(stream), z, ldz,
                           static_cast<int>(Fo), rowptr, col, static_cast<int>(n_rows), n_rows_dev,
                           bias, epi, seed_dev, out, ldo);
    else
        hipLaunchKernelGGL(k_gcn_agg<false>, dim3(grid), dim3(256), 0, as_stream(stream), z, ldz,
                           static_cast<int>(Fo), rowptr, col, static_cast<int>(n_rows), n_rows_dev,
                           bias, epi, seed_dev, out, ldo);
    return launch_status();
}
