// zh_range.hip -- exact range search (zh_search_range_batch, driver in zh_api.hip): every live stored row whose canonical key is <= a per-query
// threshold key, as a CSR over the queries, each segment ascending by (key, id).  DESIGN.md s14.
//
// A hit is (query, stored row, key).  Both paths append hits to ONE pool per internal batch -- v = query << 32 | row and the key, two u64 arrays --
// and count them per query in cnt[] whether or not the pool still has room: the totals and offsets stay exact when the caller's capacity is too
// small (or 0: count only).  A pool slot is taken with one atomic per WAVE (ballot, popcount, the lane's rank among the set bits), not one per hit.
//   path 1  exact_score_kernel (zh_exact.hip) keys a row chunk into the key scratch [query][position]; range_collect_kernel reads it.
//   path 2  range_mfma_kernel scans the fp16 row copy exactly as exact_mfma_kernel does (same tiles, same four-accumulator sum, same
//           approx_interval, live bitmap and perm) against a FIXED per-query bound tau_q (range_tau_kernel) and appends the pairs with lo <= tau_q
//           to a candidate pool; range_survivors_kernel gives every candidate the canonical key, judges key <= max_key, counts and compacts.
// Then a per-query exclusive scan of cnt gives the offsets (range_offsets_kernel, 64-bit: totals may pass 2^32) and the pool is ordered by
// (query, key, id) with three stable LSD radix sorts (row bits, then the key, then the query bits; rocPRIM through hipCUB).
#include <hipcub/hipcub.hpp>

#include "zh_internal.h"
#include "zh_device.h"

// ---- path 1: the hits of a keyed row chunk.  grid (ceil(nr / 256), B): a wave reads 64 consecutive positions of ONE query ----
__global__ __launch_bounds__(256) void range_collect_kernel(const uint64_t *__restrict__ keys, uint64_t ld, const uint32_t *__restrict__ live, uint64_t p0,
                                                            uint32_t nr, const uint64_t *__restrict__ maxk, uint32_t *__restrict__ cnt,
                                                            unsigned long long *__restrict__ ctr, uint64_t *__restrict__ pv, uint64_t *__restrict__ pk,
                                                            uint64_t cap) {
    const uint32_t b = blockIdx.y, lane = threadIdx.x & 63;
    const uint32_t rl = blockIdx.x * 256 + threadIdx.x;
    uint64_t key = 0;
    bool hit = false;
    if (rl < nr) {
        key = keys[(size_t)b * ld + rl];
        hit = key <= maxk[b];
    }
    const uint64_t m = __ballot(hit);
    if (!m) return;  // (wave-uniform)
    if (lane == 0) atomicAdd(&cnt[b], (uint32_t)__popcll(m));  // always: the count stays exact when the pool is full
    const unsigned long long slot = wave_slots(ctr, m, lane);
    if (hit && slot < cap) {
        pv[slot] = ((uint64_t)b << 32) | live[p0 + rl];
        pk[slot] = key;
    }
}

hipError_t zh_launch_range_collect(const uint64_t *dKeys, uint64_t ld, const uint32_t *dLive, uint64_t p0, uint32_t nr, uint32_t B,
                                   const uint64_t *dMaxKeys, uint32_t *dCnt, unsigned long long *dHitCtr, uint64_t *dPoolV, uint64_t *dPoolK,
                                   uint64_t pool_cap, hipStream_t s) {
    if (!nr || !B) return hipSuccess;
    hipLaunchKernelGGL(range_collect_kernel, dim3((nr + 255) / 256, B), dim3(256), 0, s, dKeys, ld, dLive, p0, nr, dMaxKeys, dCnt, dHitCtr, dPoolV, dPoolK,
                       pool_cap);
    return hipGetLastError();
}

// ---- path 2: the fixed bound.  tau_q = the threshold key mapped into approx_interval's sortable-f32 domain, rounded towards admitting more, so that
// key <= max_key implies lo <= tau_q for every pair (DESIGN.md s14 has the derivation):
//   L2SQ            the interval holds d* (the canonical f32 sum), key = bits of (double)d*: d* <= D = the threshold as a double;
//   L2              key = bits of sqrt((double)d*), a correctly rounded sqrt: d* <= D^2 (1 + 2^-51), formed in f64 with 2^-49 to cover its own roundings;
//   cosine literal  the interval holds the clipped distance c, key = bits of c: c <= D;
//   cosine parity   key = bits of K = 1 - c, compared unsigned: K > 0 ascending, then K < 0 by |K|; the interval holds w = K > 0 ? K : 2 - K, which
//                   is monotone in that order: w <= D for a non-negative threshold, w <= 2 + |D| for a negative one.
// The f64 bound becomes the next f32 above its rounding.  A threshold that is no finite number (or, outside the parity key, has its sign bit set:
// at or above every key those metrics produce) admits everything, and so does every pair approx_interval is not certain of: its lo is 0.
__global__ __launch_bounds__(256) void range_tau_kernel(const uint64_t *__restrict__ maxk, uint32_t B, int kinda, int is_l2, uint32_t *__restrict__ tau) {
    const uint32_t b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    const uint64_t mk = maxk[b], mag = mk & 0x7FFFFFFFFFFFFFFFull;
    const bool neg = (mk >> 63) != 0;
    uint32_t t = 0xFFFFFFFFu;
    if (mag < 0x7FF0000000000000ull && (kinda == 2 || !neg)) {
        const double D = __longlong_as_double((long long)mag);
        double w = D;
        if (kinda == 2) w = neg ? 2.0 + D : D;
        else if (is_l2) w = (D * D) * (1.0 + 1.7763568394002505e-15);  // 2^-49
        uint32_t u = __float_as_uint((float)w);  // w >= 0: round to nearest, then one f32 up (+inf stays)
        if (u < 0x7F800000u) u++;
        t = u | 0x80000000u;  // f32_sortable of a non-negative float
    }
    tau[b] = t;
}

hipError_t zh_launch_range_tau(const uint64_t *dMaxKeys, uint32_t B, int metric, int mode, uint32_t *dTau, hipStream_t s) {
    if (!B) return hipSuccess;
    const int kinda = metric != ZH_COSINE ? 0 : (mode == ZH_COSINE_PARITY ? 2 : 1);
    hipLaunchKernelGGL(range_tau_kernel, dim3((B + 255) / 256), dim3(256), 0, s, dMaxKeys, B, kinda, metric == ZH_L2 ? 1 : 0, dTau);
    return hipGetLastError();
}

// exact_mfma_kernel's scan (zh_exact.hip; FILT = false) with the list replaced: a pair with lo <= tau_q goes to the candidate pool as query << 32 | row.
// No per-query cap and no prune pass: tau never moves, so one launch covers the table.  *ctr counts every candidate; past cap they are not stored and
// the host answers the batch by path 1.
template <int D, int KINDA>
__global__ __launch_bounds__(256) void range_mfma_kernel(const u32x4 *__restrict__ Xh, const float2 *__restrict__ rowMeta, const uint32_t *__restrict__ perm,
                                                         uint64_t perm_rows, const uint32_t *__restrict__ liveBits, uint64_t p_begin, uint64_t p_end,
                                                         const u32x4 *__restrict__ Qh, const float4 *__restrict__ qmeta, uint32_t B, float Kc, float rho,
                                                         const uint32_t *__restrict__ tau, uint64_t *__restrict__ cand, uint64_t cap,
                                                         unsigned long long *__restrict__ ctr) {
    const uint32_t lane = threadIdx.x & 63, c16 = lane & 15, h = lane >> 4;
    const uint32_t wid = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t tile = p_begin / 16 + (uint64_t)blockIdx.x * 4 + wid;
    const uint64_t p0 = tile * 16;
    if (p0 >= p_end) return;
    f16x8 A[D / 32];
    tile_load<D, true>(A, Xh, (size_t)tile, lane);
    // this lane's outputs: rows 4 h + i of the tile (register i), column c16
    bool valid[4];
    uint32_t id[4];
    float2 meta[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const uint64_t p = p0 + 4 * h + i;
        valid[i] = p < p_end;
        id[i] = valid[i] ? (perm && p < perm_rows ? perm[p] : (uint32_t)p) : 0u;
        valid[i] = valid[i] && ((liveBits[id[i] >> 5] >> (id[i] & 31)) & 1u);
        meta[i] = valid[i] ? rowMeta[p] : make_float2(0.f, 0.f);
    }
    for (uint32_t q0 = 0; q0 < B; q0 += 16) {
        const uint32_t b = q0 + c16, bq = b < B ? b : B - 1;
        const u32x4 *qp = Qh + (size_t)bq * (D / 8) + h;  // step st: piece 4 st + h of the query (qhalf layout 1 = the A operand's k order)
        const TileSums t = tile_dot<D / 32, 4>(A, qp);
        const float4 qm = qmeta[bq];
        const uint32_t tq = tau[bq];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            bool pass = false;
            if (b < B && valid[i]) pass = (uint32_t)approx_interval<KINDA>(t[i] * meta[i].y, meta[i].x, qm, Kc, rho, 0.f) <= tq;
            pool_push(ctr, cand, cap, pass, ((uint64_t)b << 32) | id[i], lane);
        }
    }
}

hipError_t zh_launch_range_mfma(uint32_t d, int metric, int mode, const ZhExact2 &e, uint64_t p_begin, uint64_t p_end, uint64_t *dCand, uint64_t cand_cap,
                                unsigned long long *dCandCtr, hipStream_t s) {
    if (p_begin >= p_end || !e.B) return hipSuccess;
    if (p_begin % 16) return hipErrorInvalidValue;
    const uint64_t tiles = (p_end - p_begin + 15) / 16, blocks = (tiles + 3) / 4;
    return zh_mfma_dispatch(d, metric, mode, [&](auto D, auto K) {
        hipLaunchKernelGGL((range_mfma_kernel<D, K>), dim3((uint32_t)blocks), dim3(256), 0, s, (const u32x4 *)e.Xh, e.rowMeta, e.perm, e.perm_rows, e.liveBits,
                           p_begin, p_end, (const u32x4 *)e.Qh, e.qmeta, e.B, e.Kc, e.rho, (const uint32_t *)e.tau, dCand, cand_cap, dCandCtr);
    });
}

// The candidates' canonical keys, in the manner of exact_survivor_keys_kernel -- and their judgement.  A wave takes 64 candidates at a time: pair j's
// sums wait in lane j, so that key_of, the comparison with the query's threshold and the pool's atomic run once for all 64.
template <int D, int KIND>
__global__ __launch_bounds__(256) void range_survivors_kernel(const float *__restrict__ X, const float *__restrict__ Q, const float *__restrict__ QQ, int metric,
                                                              int param, const uint64_t *__restrict__ cand, const unsigned long long *__restrict__ candCtr,
                                                              uint64_t cand_cap, const uint64_t *__restrict__ maxk, uint32_t *__restrict__ cnt,
                                                              unsigned long long *__restrict__ ctr, uint64_t *__restrict__ pv, uint64_t *__restrict__ pk,
                                                              uint64_t cap) {
    const uint64_t n = *candCtr;
    if (n > cand_cap) return;  // (the pool ran over: the batch is answered by path 1)
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t wave = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = (uint64_t)gridDim.x * 4;
    for (uint64_t g = wave * 64; g < n; g += n_waves * 64) {
        const uint32_t m = n - g < 64 ? (uint32_t)(n - g) : 64u;
        const uint64_t mine = lane < m ? cand[g + lane] : 0ull;
        const uint32_t my_row = (uint32_t)mine, my_b = (uint32_t)(mine >> 32);
        float m0 = 0.f, m1 = 0.f;
        for (uint32_t j = 0; j < m; j++) {
            const uint32_t row = (uint32_t)__builtin_amdgcn_readlane((int)my_row, (int)j), b = (uint32_t)__builtin_amdgcn_readlane((int)my_b, (int)j);
            float s0 = 0.f, s1 = 0.f, qq = 0.f;
            table_pair_sums<D, KIND, false>(X, row, Q, b, lane, param, s0, s1, qq);  // (the query's norm is QQ's, below)
            if (lane == j) { m0 = s0; m1 = s1; }
        }
        uint64_t key = 0;
        bool hit = false;
        if (lane < m) {
            key = key_of(metric, param, m0, m1, KIND == K_COS ? QQ[my_b] : 0.f);
            hit = key <= maxk[my_b];
        }
        const uint64_t hm = __ballot(hit);
        if (hm) {  // (wave-uniform)
            const unsigned long long slot = wave_slots(ctr, hm, lane);
            if (hit) {
                atomicAdd(&cnt[my_b], 1u);
                if (slot < cap) { pv[slot] = mine; pk[slot] = key; }
            }
        }
    }
}

template <int D>
static void launch_range_surv_d(const float *dX, const float *dQ, const float *dQQ, int metric, int mode, const uint64_t *dCand,
                                const unsigned long long *dCandCtr, uint64_t cand_cap, const uint64_t *dMaxKeys, uint32_t *dCnt,
                                unsigned long long *dHitCtr, uint64_t *dPoolV, uint64_t *dPoolK, uint64_t pool_cap, uint32_t blocks, hipStream_t s) {
    if (metric == ZH_COSINE)
        hipLaunchKernelGGL((range_survivors_kernel<D, K_COS>), dim3(blocks), dim3(256), 0, s, dX, dQ, dQQ, metric, mode, dCand, dCandCtr, cand_cap, dMaxKeys, dCnt,
                           dHitCtr, dPoolV, dPoolK, pool_cap);
    else
        hipLaunchKernelGGL((range_survivors_kernel<D, K_L2>), dim3(blocks), dim3(256), 0, s, dX, dQ, dQQ, metric, mode, dCand, dCandCtr, cand_cap, dMaxKeys, dCnt,
                           dHitCtr, dPoolV, dPoolK, pool_cap);
}

hipError_t zh_launch_range_survivors(const float *dX, uint32_t d, const float *dQ, const float *dQQ, int metric, int mode, const uint64_t *dCand,
                                     const unsigned long long *dCandCtr, uint64_t cand_cap, const uint64_t *dMaxKeys, uint32_t *dCnt,
                                     unsigned long long *dHitCtr, uint64_t *dPoolV, uint64_t *dPoolK, uint64_t pool_cap, hipStream_t s) {
    // the candidate count is known on the device only: enough waves for 64 candidates each up to the pool's size, at most 4096 of them
    const uint32_t blocks = (uint32_t)std::min<uint64_t>(1024, std::max<uint64_t>(1, (cand_cap + 255) / 256));
#define ZH_RG_SURV(DD) case DD: launch_range_surv_d<DD>(dX, dQ, dQQ, metric, mode, dCand, dCandCtr, cand_cap, dMaxKeys, dCnt, dHitCtr, dPoolV, dPoolK, pool_cap, blocks, s); break
    switch (d) {
        ZH_RG_SURV(256);
        ZH_RG_SURV(384);
        ZH_RG_SURV(512);
        ZH_RG_SURV(768);
        ZH_RG_SURV(1024);
    default: return hipErrorInvalidValue;
    }
#undef ZH_RG_SURV
    return hipGetLastError();
}

// ---- both paths: the offsets.  off[i] = base + the hits of queries before i of this internal batch (B <= 1024), off[B] = base + all of them ----
__global__ __launch_bounds__(1024) void range_offsets_kernel(const uint32_t *__restrict__ cnt, uint32_t B, uint64_t base, uint64_t *__restrict__ off) {
    __shared__ uint64_t sm[1024];
    const uint32_t i = threadIdx.x;
    const uint64_t c = i < B ? cnt[i] : 0u;
    sm[i] = c;
    __syncthreads();
    for (uint32_t o = 1; o < 1024; o <<= 1) {  // inclusive scan
        const uint64_t x = i >= o ? sm[i - o] : 0ull;
        __syncthreads();
        sm[i] += x;
        __syncthreads();
    }
    if (i < B) off[i] = base + sm[i] - c;
    if (i == B - 1) off[B] = base + sm[i];
}

hipError_t zh_launch_range_offsets(const uint32_t *dCnt, uint32_t B, uint64_t base, uint64_t *dOff, hipStream_t s) {
    if (!B || B > 1024) return hipErrorInvalidValue;
    hipLaunchKernelGGL(range_offsets_kernel, dim3(1), dim3(1024), 0, s, dCnt, B, base, dOff);
    return hipGetLastError();
}

// ---- both paths: the order, for every pool of this library (the joins' too: zh_join.hip).  Three stable LSD sorts of (v, k): by the low field of
// v (lo_values of them), by the key, by the high field of v (hi_values of them; skip_high: there is one value only and the pass is left out)
// -> (high, key, low).  *v_out / *k_out = the ordered arrays.  dTmp == nullptr: *tmp_bytes = what the three sorts of n entries need at most ----
hipError_t zh_launch_pool_sort(uint64_t *dV[2], uint64_t *dK[2], uint64_t n, uint64_t lo_values, uint64_t hi_values, bool skip_high, void *dTmp,
                               size_t *tmp_bytes, const uint64_t **v_out, const uint64_t **k_out, hipStream_t s) {
    hipcub::DoubleBuffer<uint64_t> v(dV[0], dV[1]), k(dK[0], dK[1]);
    const int lb = field_bits(lo_values), hb = field_bits(hi_values);
    hipError_t e;
    if (!dTmp) {
        size_t a = 0, b = 0, c = 0;
        if ((e = hipcub::DeviceRadixSort::SortPairs(nullptr, a, v, k, n, 0, lb, s)) != hipSuccess) return e;
        if ((e = hipcub::DeviceRadixSort::SortPairs(nullptr, b, k, v, n, 0, 64, s)) != hipSuccess) return e;
        if ((e = hipcub::DeviceRadixSort::SortPairs(nullptr, c, v, k, n, 32, 32 + hb, s)) != hipSuccess) return e;
        *tmp_bytes = std::max<size_t>(std::max(a, b), std::max<size_t>(c, 1));
        return hipSuccess;
    }
    size_t bytes = *tmp_bytes;
    if ((e = hipcub::DeviceRadixSort::SortPairs(dTmp, bytes, v, k, n, 0, lb, s)) != hipSuccess) return e;
    bytes = *tmp_bytes;
    if ((e = hipcub::DeviceRadixSort::SortPairs(dTmp, bytes, k, v, n, 0, 64, s)) != hipSuccess) return e;
    bytes = *tmp_bytes;
    if (!skip_high && (e = hipcub::DeviceRadixSort::SortPairs(dTmp, bytes, v, k, n, 32, 32 + hb, s)) != hipSuccess) return e;
    *v_out = v.Current();
    *k_out = k.Current();
    return hipSuccess;
}

__global__ __launch_bounds__(256) void range_emit_kernel(const uint64_t *__restrict__ v, const uint64_t *__restrict__ k, uint64_t n, uint64_t id_base,
                                                         uint64_t *__restrict__ ids, uint64_t *__restrict__ keys) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) { ids[i] = id_base + (v[i] & 0xFFFFFFFFull); keys[i] = k[i]; }
}

// the pool of an internal batch ordered by (query, key, row) and written out; B == 1 has one query value and no third pass
hipError_t zh_launch_range_sort(uint64_t *dV[2], uint64_t *dK[2], uint64_t n, uint64_t n_rows, uint32_t B, void *dTmp, size_t *tmp_bytes, uint64_t id_base,
                                uint64_t *dOutIds, uint64_t *dOutKeys, hipStream_t s) {
    if (dTmp && !n) return hipSuccess;
    const uint64_t *v = nullptr, *k = nullptr;
    const hipError_t e = zh_launch_pool_sort(dV, dK, n, n_rows, B, B <= 1, dTmp, tmp_bytes, &v, &k, s);
    if (e != hipSuccess || !dTmp) return e;
    hipLaunchKernelGGL(range_emit_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, v, k, n, id_base, dOutIds, dOutKeys);
    return hipGetLastError();
}
