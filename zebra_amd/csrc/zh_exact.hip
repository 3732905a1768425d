// zh_exact.hip -- exact k-nearest-neighbour search over every live stored row (zh_search_exact_batch): no forest, no pair lists.
//
// The scan scores every (live row, query) pair with the canonical sums of zh_device.h (row_pair_sums / lane_sums_generic +
// wave_combine<KIND>, the same association order as the sweeps and zh_distance_batch), so every key is bit-equal to the one
// zh_distance_batch returns for that pair.  The table is taken in row chunks (positions of the live-row list): per chunk the
// keys of all queries land in a scratch [query][position], the leaf-visit select of zh_search.hip keeps every sub-chunk's
// top_k by (key, id), final_kernel merges a query's sub-chunks, and the chunk's answer is merged into the running one.
// The scan is a wave per pair: a wave holds EXR stored rows in registers, the block's queries come through LDS (ExactTile::QT at a time),
// and the finished sums wait in lane registers (pair p in lane p) so that key_of and the stores run for all pairs at once.

#include "zh_internal.h"
#include "zh_device.h"

#define EXR 4  // stored rows per wave (registers): a query read from LDS serves EXR pairs

template <int D>
struct ExactTile {
    static constexpr int NV = RowVec<D>::NV;
    static constexpr int QT = D <= 512 ? 16 : 8;  // queries per LDS tile: EXR * QT <= 64 pairs per wave and tile
};

// keys[b * ld + (p - p0)] = key of (live row at position p, query b) for p in [p0, p0 + nr); live[p] = stored row id
template <int D, int KIND>
__global__ __launch_bounds__(256) void exact_score_kernel(const float *__restrict__ X, const uint32_t *__restrict__ live, uint64_t p0,
                                                          uint32_t nr, const float *__restrict__ Q, const float *__restrict__ QQ, uint32_t B,
                                                          int metric, int param, uint64_t *__restrict__ keys, uint64_t ld) {
    constexpr int NV = ExactTile<D>::NV, QT = ExactTile<D>::QT;
    __shared__ float4 qs[QT][NV * 64];
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t rl0 = (blockIdx.x * 4 + wv) * EXR;  // the wave's first row (relative to p0)
    float4 v[EXR][NV];
    float rn[EXR];
#pragma unroll
    for (int r = 0; r < EXR; r++) {
        const uint32_t rl = rl0 + r < nr ? rl0 + r : nr - 1;
        load_row<D, true>(X + (size_t)live[p0 + rl] * D, lane, v[r]);
        rn[r] = 0.f;
        if (KIND == K_COS) {  // the stored row's squared norm, as exact_key computes it
            float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int j = 0; j < NV; j++) {
                const bool act = (j < RowVec<D>::NJ) || (lane < (uint32_t)RowVec<D>::REM4);
                if (act) sq4(v[r][j], c);
            }
            rn[r] = wave_sum_canonical((c.x + c.y) + (c.z + c.w));
        }
    }
    for (uint32_t q0 = 0; q0 < B; q0 += QT) {
        const uint32_t nq = B - q0 < (uint32_t)QT ? B - q0 : (uint32_t)QT;
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < (uint32_t)QT * NV * 64; i += 256) {
            const uint32_t m = i / (NV * 64), e4 = i % (NV * 64);
            float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
            if (m < nq && e4 < (uint32_t)(D / 4)) t = reinterpret_cast<const float4 *>(Q + (size_t)(q0 + m) * D)[e4];
            qs[m][e4] = t;
        }
        __syncthreads();
        float m0 = 0.f, m1 = 0.f;  // the sums of pair (m, r) wait in lane m * EXR + r
        for (uint32_t m = 0; m < nq; m++) {
            float4 q[NV];
#pragma unroll
            for (int j = 0; j < NV; j++) q[j] = qs[m][lane + 64 * j];
#pragma unroll
            for (int r = 0; r < EXR; r++) {
                float s0 = 0.f, s1 = 0.f;
                row_pair_sums<D, KIND>(v[r], q, lane, param, s0, s1);
                if (lane == m * EXR + r) { m0 = s0; m1 = KIND == K_COS ? rn[r] : s1; }
            }
        }
        const uint32_t m = lane / EXR, r = lane % EXR;
        if (m < nq && rl0 + r < nr)
            keys[(size_t)(q0 + m) * ld + rl0 + r] = key_of(metric, param, m0, m1, KIND == K_COS ? QQ[q0 + m] : 0.f);
    }
}

// any d: a wave per row, the query straight from memory (lane_sums_generic)
template <int KIND>
__global__ __launch_bounds__(256) void exact_score_generic_kernel(const float *__restrict__ X, uint32_t d, const uint32_t *__restrict__ live,
                                                                  uint64_t p0, uint32_t nr, const float *__restrict__ Q,
                                                                  const float *__restrict__ QQ, uint32_t B, int metric, int param,
                                                                  uint64_t *__restrict__ keys, uint64_t ld) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t rl = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (rl >= nr) return;
    const float *x = X + (size_t)live[p0 + rl] * d;
    for (uint32_t b = 0; b < B; b++) {
        float s0, s1;
        lane_sums_generic<KIND>(x, Q + (size_t)b * d, d, lane, param, s0, s1);
        if (lane == 0) keys[(size_t)b * ld + rl] = key_of(metric, param, s0, s1, KIND == K_COS ? QQ[b] : 0.f);
    }
}

hipError_t zh_launch_exact_score(const float *dX, uint32_t d, const uint32_t *dLive, uint64_t p0, uint32_t nr, const float *dQ,
                                 const float *dQQ, uint32_t B, int metric, int param, uint64_t *dKeys, uint64_t ld, hipStream_t s) {
    if (!nr || !B) return hipSuccess;
    return zh_dispatch_kind_dim(metric, d, [&](auto kind, auto dim) {
        constexpr int KIND = decltype(kind)::value, D = decltype(dim)::value;
        if constexpr (D > 0)
            hipLaunchKernelGGL((exact_score_kernel<D, KIND>), dim3((nr + 4 * EXR - 1) / (4 * EXR)), dim3(256), 0, s, dX, dLive, p0, nr, dQ, dQQ, B, metric, param,
                               dKeys, ld);
        else
            hipLaunchKernelGGL(exact_score_generic_kernel<KIND>, dim3((nr + 3) / 4), dim3(256), 0, s, dX, d, dLive, p0, nr, dQ, dQQ, B, metric, param, dKeys, ld);
        return hipGetLastError();
    });
}

// One "visit" per (query, sub-chunk of L positions): select_kernel keeps its take = min(k, len) smallest (key, id), final_kernel
// reads a query's nsub visits as one contiguous candidate run.  candBase[b * nsub] = first candidate of query b (B * nsub + 1 entries).
__global__ __launch_bounds__(256) void exact_visits_kernel(uint32_t B, uint32_t nsub, uint32_t nr, uint32_t L, uint32_t k, uint64_t p0, uint64_t ld,
                                                           ZhVisit *__restrict__ visits, uint64_t *__restrict__ candBase) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, n = (uint64_t)B * nsub;
    const uint32_t kk = k < L ? k : L;
    const uint32_t last_len = nr - (nsub - 1) * L, last_take = k < last_len ? k : last_len;
    const uint64_t per_q = (uint64_t)(nsub - 1) * kk + last_take;
    if (i < n) {
        const uint32_t b = (uint32_t)(i / nsub), sub = (uint32_t)(i % nsub);
        ZhVisit v;
        v.b = b;
        v.leaf_off = (uint32_t)(p0 + (uint64_t)sub * L);
        v.len = sub + 1 < nsub ? L : last_len;
        v.take = k < v.len ? k : v.len;
        v.row_off = (uint64_t)b * ld + (uint64_t)sub * L;
        v.cand_off = (uint64_t)b * per_q + (uint64_t)sub * kk;
        v.node = 0;
        v.pad = 0;
        visits[i] = v;
        candBase[i] = v.cand_off;
    }
    if (i == 0) candBase[n] = (uint64_t)B * per_q;
}

hipError_t zh_launch_exact_visits(uint32_t B, uint32_t nsub, uint32_t nr, uint32_t L, uint32_t k, uint64_t p0, uint64_t ld, ZhVisit *dVisits,
                                  uint64_t *dCandBase, hipStream_t s) {
    const uint64_t n = (uint64_t)B * nsub;
    hipLaunchKernelGGL(exact_visits_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, B, nsub, nr, L, k, p0, ld, dVisits, dCandBase);
    return hipGetLastError();
}

// no neighbours: counts 0, every id / key slot UINT64_MAX
__global__ __launch_bounds__(256) void exact_empty_kernel(uint32_t B, uint32_t k, uint64_t *__restrict__ ids, uint64_t *__restrict__ keys,
                                                          uint32_t *__restrict__ counts) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < (uint64_t)B * k) { ids[i] = ~0ull; keys[i] = ~0ull; }
    if (i < B) counts[i] = 0;
}

hipError_t zh_launch_exact_empty(uint32_t B, uint32_t k, uint64_t *dIds, uint64_t *dKeys, uint32_t *dCounts, hipStream_t s) {
    const uint64_t n = std::max<uint64_t>((uint64_t)B * k, B);
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(exact_empty_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, B, k, dIds, dKeys, dCounts);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// Path 2 (L2SQ, L2, cosine at d = 256 .. 1024): a dense matrix-core scan of the index's fp16 row copy (row_half_kernel's tiles, position p holds
// row perm[p] for p < perm_rows, else row p) against qhalf_kernel's fp16 copy of the queries (layout 1).  Every (live row, query) pair gets
// approx_interval's [lo, hi] around its key (zh_approx_bound(metric, d, 1): the same four-accumulator sum scan_mfma_kernel forms, the copy's
// measured rho).  A query keeps the (row, lo, hi) of every pair with lo <= tau_q; after each row chunk exact_prune_kernel sets tau_q to the k-th
// smallest hi of its list and drops the entries with lo > tau_q.  tau_q is always the hi of k distinct live rows, so no row of the true top-k and
// no row tied with the k-th key is ever dropped; the survivors get the canonical key and final_kernel ranks them by (key, id).  A list that runs
// over raises *over: the host answers that internal batch by path 1.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool exact_live(const uint32_t *__restrict__ bits, uint32_t id) { return (bits[id >> 5] >> (id & 31)) & 1u; }

// FILT (the filtered search): liveBits is the allowed-and-live bitmap by POSITION (a tile's 16 positions are half a word of it), and a wave whose
// tile is masked whole returns before it loads anything and counts itself in over[1]
// The tile's load and product are tile_load's and tile_dot's (zh_device.h) written out: through those helpers the compiler waits for every load of a
// query's halves before its product at d = 1024 (the filtered scan: 27 % slower, measured) -- any change to the sum's order there is one here too.
template <int D, int KINDA, bool FILT>
__global__ __launch_bounds__(256) void exact_mfma_kernel(const u32x4 *__restrict__ Xh, const float2 *__restrict__ rowMeta,
                                                         const uint32_t *__restrict__ perm, uint64_t perm_rows, const uint32_t *__restrict__ liveBits,
                                                         uint64_t p_begin, uint64_t p_end, const u32x4 *__restrict__ Qh,
                                                         const float4 *__restrict__ qmeta, uint32_t B, float Kc, float rho,
                                                         const uint32_t *__restrict__ tau, uint32_t *__restrict__ cnt, uint32_t *__restrict__ lid,
                                                         uint32_t *__restrict__ llo, uint32_t *__restrict__ lhi, uint32_t cap, uint32_t *__restrict__ over) {
    constexpr int NS = D / 32;  // MFMA steps of a tile (K = 32 each)
    const uint32_t lane = threadIdx.x & 63, c16 = lane & 15, h = lane >> 4;
    const uint32_t wid = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t tile = p_begin / 16 + (uint64_t)blockIdx.x * 4 + wid;
    const uint64_t p0 = tile * 16;
    if (p0 >= p_end) return;
    if (FILT) {
        if (((liveBits[p0 >> 5] >> (p0 & 31)) & 0xFFFFu) == 0u) {
            if (lane == 0) atomicAdd(over + 1, 1u);
            return;
        }
    }
    f16x8 A[NS];
    const u32x4 *tp = Xh + (size_t)tile * (NS * 64) + lane;
#pragma unroll
    for (int st = 0; st < NS; st++) A[st] = __builtin_bit_cast(f16x8, __builtin_nontemporal_load(tp + 64 * st));
    // this lane's outputs: rows 4 h + i of the tile (register i), column c16
    bool valid[4];
    uint32_t id[4];
    float2 meta[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const uint64_t p = p0 + 4 * h + i;
        valid[i] = p < p_end;
        id[i] = valid[i] ? (perm && p < perm_rows ? perm[p] : (uint32_t)p) : 0u;
        valid[i] = valid[i] && (FILT ? ((liveBits[p >> 5] >> (p & 31)) & 1u) != 0u : exact_live(liveBits, id[i]));
        meta[i] = valid[i] ? rowMeta[p] : make_float2(0.f, 0.f);
    }
    for (uint32_t q0 = 0; q0 < B; q0 += 16) {
        const uint32_t b = q0 + c16, bq = b < B ? b : B - 1;
        const u32x4 *qp = Qh + (size_t)bq * (D / 8) + h;  // step st: piece 4 st + h of the query (qhalf layout 1 = the A operand's k order)
        f32x4 acc[4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
        for (int st = 0; st < NS; st++)
            acc[st & 3] = __builtin_amdgcn_mfma_f32_16x16x32_f16(A[st], __builtin_bit_cast(f16x8, qp[4 * st]), acc[st & 3], 0, 0, 0);
        const f32x4 t = (acc[0] + acc[1]) + (acc[2] + acc[3]);
        if (b < B) {
            const float4 qm = qmeta[b];
            const uint32_t tq = tau[b];
#pragma unroll
            for (int i = 0; i < 4; i++) {
                if (!valid[i]) continue;
                const uint64_t iv = approx_interval<KINDA>(t[i] * meta[i].y, meta[i].x, qm, Kc, rho, 0.f);
                const uint32_t lo = (uint32_t)iv, hi = (uint32_t)(iv >> 32);
                if (lo <= tq) {
                    const uint32_t slot = atomicAdd(&cnt[b], 1u);
                    if (slot < cap) {
                        const size_t o = (size_t)b * cap + slot;
                        lid[o] = id[i]; llo[o] = lo; lhi[o] = hi;
                    } else
                        atomicOr(over, 1u);
                }
            }
        }
    }
}

// per query (a block): tau = min(tau, the k-th smallest hi of the list), entries with lo > tau dropped (compacted through `scratch`)
__global__ __launch_bounds__(256) void exact_prune_kernel(uint32_t k, uint32_t *__restrict__ tau, uint32_t *__restrict__ cnt, uint32_t *__restrict__ lid,
                                                          uint32_t *__restrict__ llo, uint32_t *__restrict__ lhi, uint32_t cap,
                                                          uint32_t *__restrict__ scratch, const uint32_t *__restrict__ over) {
    __shared__ uint32_t hist[256], s_sel[2], s_n;
    const uint32_t b = blockIdx.x, tid = threadIdx.x;
    if (*over) return;  // (the batch is answered by path 1)
    const uint32_t n = cnt[b];
    if (n <= k) return;
    const size_t ob = (size_t)b * cap;
    // the k-th smallest hi: radix select, 8 bits a round from the top
    uint32_t prefix = 0, need = k;
    for (int sh = 24; sh >= 0; sh -= 8) {
        hist[tid] = 0;
        __syncthreads();
        const uint32_t mask = sh == 24 ? 0u : (0xFFFFFFFFu << (sh + 8));
        for (uint32_t i = tid; i < n; i += 256) {
            const uint32_t v = lhi[ob + i];
            if ((v & mask) == prefix) atomicAdd(&hist[(v >> sh) & 255u], 1u);
        }
        __syncthreads();
        if (tid == 0) {
            uint32_t c = 0, j = 0;
            for (; j < 256; j++) {
                if (c + hist[j] >= need) break;
                c += hist[j];
            }
            s_sel[0] = j; s_sel[1] = need - c;
        }
        __syncthreads();
        prefix |= s_sel[0] << sh;
        need = s_sel[1];
        __syncthreads();
    }
    const uint32_t t = prefix < tau[b] ? prefix : tau[b];
    if (tid == 0) s_n = 0;
    __syncthreads();
    uint32_t *sid = scratch + ob * 3, *slo = sid + cap, *shi = slo + cap;
    for (uint32_t i = tid; i < n; i += 256) {
        const uint32_t lo = llo[ob + i];
        if (lo <= t) {
            const uint32_t o = atomicAdd(&s_n, 1u);
            sid[o] = lid[ob + i]; slo[o] = lo; shi[o] = lhi[ob + i];
        }
    }
    __syncthreads();
    const uint32_t n2 = s_n;
    for (uint32_t i = tid; i < n2; i += 256) { lid[ob + i] = sid[i]; llo[ob + i] = slo[i]; lhi[ob + i] = shi[i]; }
    if (tid == 0) { cnt[b] = n2; tau[b] = t; }
}

// the survivors' canonical keys (grid (SX, B), waves striding over query b's list, the query in registers); slots past the list get (~0, ~0) so
// that final_kernel can read every query's cap slots as its candidates
template <int D, int KIND>
__global__ __launch_bounds__(256) void exact_survivor_keys_kernel(const float *__restrict__ X, const float *__restrict__ Q, const float *__restrict__ QQ,
                                                                  int metric, int param, const uint32_t *__restrict__ cnt, const uint32_t *__restrict__ lid,
                                                                  uint32_t cap, uint64_t *__restrict__ ckeys, uint32_t *__restrict__ cids,
                                                                  const uint32_t *__restrict__ over) {
    if (*over) return;
    constexpr int NV = RowVec<D>::NV;
    const uint32_t b = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t ns = cnt[b], stride = gridDim.x * 4u;
    const size_t ob = (size_t)b * cap;
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x + ns; i < cap; i += gridDim.x * 256) { ckeys[ob + i] = ~0ull; cids[ob + i] = ~0u; }
    float4 q[NV];
    load_row<D>(Q + (size_t)b * D, lane, q);
    const float qq = KIND == K_COS ? QQ[b] : 0.f;
    for (uint32_t i = blockIdx.x * 4u + wv; i < ns; i += stride) {
        const uint32_t rid = lid[ob + i];
        float4 v[NV];
        load_row<D>(X + (size_t)rid * D, lane, v);
        float s0 = 0.f, s1 = 0.f;
        row_pair_sums<D, KIND>(v, q, lane, param, s0, s1);
        if (KIND == K_COS) {
            float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int j = 0; j < NV; j++) {
                const bool act = (j < RowVec<D>::NJ) || (lane < (uint32_t)RowVec<D>::REM4);
                if (act) sq4(v[j], c);
            }
            s1 = wave_sum_canonical((c.x + c.y) + (c.z + c.w));
        }
        if (lane == 0) { ckeys[ob + i] = key_of(metric, param, s0, s1, qq); cids[ob + i] = rid; }
    }
}

bool zh_exact_mfma_supported(uint32_t d, int metric) {
    return zh_mfma_dim(d) && (metric == ZH_L2SQ || metric == ZH_L2 || metric == ZH_COSINE);
}

hipError_t zh_launch_exact_mfma(uint32_t d, int metric, int mode, const ZhExact2 &e, uint64_t p_begin, uint64_t p_end, hipStream_t s, bool filtered) {
    if (p_begin >= p_end || !e.B) return hipSuccess;
    if (p_begin % 16) return hipErrorInvalidValue;
    const uint64_t tiles = (p_end - p_begin + 15) / 16, blocks = (tiles + 3) / 4;
    return zh_mfma_dispatch(d, metric, mode, [&](auto D, auto K) {
        const auto kernel = filtered ? exact_mfma_kernel<D, K, true> : exact_mfma_kernel<D, K, false>;
        hipLaunchKernelGGL(kernel, dim3((uint32_t)blocks), dim3(256), 0, s, (const u32x4 *)e.Xh, e.rowMeta, e.perm, e.perm_rows, e.liveBits, p_begin, p_end,
                           (const u32x4 *)e.Qh, e.qmeta, e.B, e.Kc, e.rho, e.tau, e.cnt, e.lid, e.llo, e.lhi, e.cap, e.over);
    });
}

hipError_t zh_launch_exact_prune(const ZhExact2 &e, uint32_t k, uint32_t *dScratch, hipStream_t s) {
    hipLaunchKernelGGL(exact_prune_kernel, dim3(e.B), dim3(256), 0, s, k, e.tau, e.cnt, e.lid, e.llo, e.lhi, e.cap, dScratch, (const uint32_t *)e.over);
    return hipGetLastError();
}

template <int D>
static void launch_surv_d(const float *dX, const float *dQ, const float *dQQ, int metric, int mode, const ZhExact2 &e, uint64_t *dCKeys, uint32_t *dCIds,
                          hipStream_t s) {
    const dim3 grid(16, e.B);
    if (metric == ZH_COSINE)
        hipLaunchKernelGGL((exact_survivor_keys_kernel<D, K_COS>), grid, dim3(256), 0, s, dX, dQ, dQQ, metric, mode, e.cnt, e.lid, e.cap, dCKeys, dCIds,
                           (const uint32_t *)e.over);
    else
        hipLaunchKernelGGL((exact_survivor_keys_kernel<D, K_L2>), grid, dim3(256), 0, s, dX, dQ, dQQ, metric, mode, e.cnt, e.lid, e.cap, dCKeys, dCIds,
                           (const uint32_t *)e.over);
}

hipError_t zh_launch_exact_survivor_keys(const float *dX, uint32_t d, const float *dQ, const float *dQQ, int metric, int mode, const ZhExact2 &e,
                                         uint64_t *dCKeys, uint32_t *dCIds, hipStream_t s) {
    switch (d) {
    case 256: launch_surv_d<256>(dX, dQ, dQQ, metric, mode, e, dCKeys, dCIds, s); break;
    case 384: launch_surv_d<384>(dX, dQ, dQQ, metric, mode, e, dCKeys, dCIds, s); break;
    case 512: launch_surv_d<512>(dX, dQ, dQQ, metric, mode, e, dCKeys, dCIds, s); break;
    case 768: launch_surv_d<768>(dX, dQ, dQQ, metric, mode, e, dCKeys, dCIds, s); break;
    case 1024: launch_surv_d<1024>(dX, dQ, dQQ, metric, mode, e, dCKeys, dCIds, s); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
