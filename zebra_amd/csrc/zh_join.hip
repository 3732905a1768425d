// zh_join.hip -- exact self-join (zh_self_join, driver in zh_api.hip): every unordered pair of distinct live stored rows (a, b), a < b by row number,
// whose key is <= ONE threshold key.  The key of a pair is the key zh_distance_batch gives for stored row b against a query equal to the f32 values
// of row a; that orientation is the definition, and every key below is computed in it.  The answer is three parallel arrays ascending by
// (a, key, b), ids = id_base + row.  DESIGN.md s15.
//
// A hit is (a, b, key).  Both paths append hits to ONE pool per call -- v = a << 32 | b and the key, two u64 arrays -- and count them in *ctr whether
// or not the pool still has room: the total stays exact when the caller's capacity is too small (or 0: count only).  A pool slot is taken with one
// atomic per WAVE (wave_slots, zh_device.h).  The pool's kernels -- collect, survivors, the order -- are written once here and serve the join
// between two indexes (zh_xjoin.hip) and the forest join (zh_fjoin.hip) too: the self-join passes its one table, row count and id base twice.
//   path 1  a panel of up to 1024 live rows is gathered device-to-device into a query buffer (join_gather_kernel), exact_score_kernel (zh_exact.hip)
//           keys the row chunks from the panel's first row on into the key scratch [query][position], pair_collect_kernel takes the keys <= max_key
//           whose row number is greater than the query row's.
//   path 2  join_mfma_kernel: BOTH operands of v_mfma_f32_16x16x32_f16 are tiles of the index's fp16 row copy (the A and the B operand have the same
//           per-lane layout: lane l holds line l % 16, k-chunk l / 16), so a 16 x 16 block of the table's Gram matrix needs no conversion, and only
//           the blocks on or above the diagonal are computed: the held-tile walk of zh_device.h with the pool sink's
//           upper-triangle rule, so a tile crosses L2 -> CU once per 64 held rows.  approx_interval (unchanged) gives the pair's interval: the
//           held row is its "stored row", the LDS row its "query", whose qm = {scale, |x|^2, an upper bound of |x|, dq = rho times that bound
//           rounded up} comes from the row's rowMeta entry (join_prep_kernel).  Pairs with lo <= tau go to a candidate pool as
//           min(id) << 32 | max(id); pair_survivors_kernel gives every candidate the canonical key of (row b, query = f32 row a), both rows
//           read from the f32 table, judges key <= max_key, counts and compacts.
// Then, while the capacity holds, the pool is ordered by (a, key, b) with three stable LSD radix sorts (b bits, then the key, then the a bits;
// rocPRIM through hipCUB) and pair_emit_kernel writes the three arrays.
// Scratch (all per call, released before return): path 2 holds 20 bytes per position (qm and the id-or-masked word), 8 bytes per candidate slot of
// one panel (at most max(1.25 x the capacity left, 256 per held row) and never more than the panel's pairs) and a block table of 4 bytes per 64 held
// rows; path 1 the exact search's query buffer and key scratch (<= 1 GiB); both 16 bytes per hit-pool slot (<= the capacity), and for the order as
// much again plus hipCUB's temporary storage, and 24 bytes per hit of staging for the host call.
#include <algorithm>

#include "zh_internal.h"
#include "zh_device.h"

// ---- path 1: the panel's rows as queries.  One wave per row ----
__global__ __launch_bounds__(256) void join_gather_kernel(const float *__restrict__ X, uint32_t d, const uint32_t *__restrict__ rows, uint32_t B,
                                                          float *__restrict__ Q) {
    const uint32_t b = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (b >= B) return;
    const float *x = X + (size_t)rows[b] * d;
    float *q = Q + (size_t)b * d;
    for (uint32_t e = lane; e < d; e += 64) q[e] = x[e];
}

hipError_t zh_launch_join_gather(const float *dX, uint32_t d, const uint32_t *dRows, uint32_t B, float *dQ, hipStream_t s) {
    if (!B) return hipSuccess;
    hipLaunchKernelGGL(join_gather_kernel, dim3((B + 3) / 4), dim3(256), 0, s, dX, d, dRows, B, dQ);
    return hipGetLastError();
}

// the hits of a keyed row chunk: key <= max_key and, UPPER (the self-join's triangle), the stored row's number above the query row's; the join
// between two indexes takes the full rectangle.  grid (ceil(nr / 256), B)
template <bool UPPER>
__global__ __launch_bounds__(256) void pair_collect_kernel(const uint64_t *__restrict__ keys, uint64_t ld, const uint32_t *__restrict__ live, uint64_t p0,
                                                           uint32_t nr, const uint32_t *__restrict__ qrows, uint64_t max_key,
                                                           unsigned long long *__restrict__ ctr, uint64_t *__restrict__ pv, uint64_t *__restrict__ pk,
                                                           uint64_t cap) {
    const uint32_t b = blockIdx.y, lane = threadIdx.x & 63;
    const uint32_t rl = blockIdx.x * 256 + threadIdx.x;
    const uint32_t a = qrows[b];
    uint64_t key = 0;
    uint32_t row = 0;
    bool hit = false;
    if (rl < nr) {
        row = live[p0 + rl];
        key = keys[(size_t)b * ld + rl];
        hit = (!UPPER || row > a) && key <= max_key;
    }
    const uint64_t m = __ballot(hit);
    if (!m) return;  // (wave-uniform)
    const unsigned long long slot = wave_slots(ctr, m, lane);  // always: the count stays exact when the pool is full
    if (hit && slot < cap) {
        pv[slot] = ((uint64_t)a << 32) | row;
        pk[slot] = key;
    }
}

hipError_t zh_launch_pair_collect(const uint64_t *dKeys, uint64_t ld, const uint32_t *dLive, uint64_t p0, uint32_t nr, const uint32_t *dQRows, uint32_t B,
                                  bool upper, uint64_t max_key, unsigned long long *dHitCtr, uint64_t *dPoolV, uint64_t *dPoolK, uint64_t pool_cap,
                                  hipStream_t s) {
    if (!nr || !B) return hipSuccess;
    const auto kernel = upper ? pair_collect_kernel<true> : pair_collect_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3((nr + 255) / 256, B), dim3(256), 0, s, dKeys, ld, dLive, p0, nr, dQRows, max_key, dHitCtr, dPoolV, dPoolK, pool_cap);
    return hipGetLastError();
}

// ---- path 2: what the scan reads per POSITION of the copy (ceil(n / 16) * 16 of them).  cid = the row's number, or UINT32_MAX for a removed row
// and for the tail of the last tile.  qm = approx_interval's view of the row as a query (row_as_query, zh_device.h): {1 / sigma, f32 |x|^2,
// nq >= |x|, dq >= |x - x'|}, x' the copy's row; all four NaN -- nothing certain, every pair of the row a candidate -- for a row that is not usable,
// a scale outside 2^-104 .. 2^76 or a norm that is no finite number. ----
__global__ __launch_bounds__(256) void join_prep_kernel(const float2 *__restrict__ rowMeta, const uint32_t *__restrict__ perm, uint64_t perm_rows,
                                                        const uint32_t *__restrict__ liveBits, uint64_t n_rows, uint64_t n_pos, float rho,
                                                        float4 *__restrict__ qm, uint32_t *__restrict__ cid) {
    const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n_pos) return;
    uint32_t id = 0xFFFFFFFFu;
    float4 o = make_float4(NAN, NAN, NAN, NAN);
    if (p < n_rows) {
        const uint32_t r = perm && p < perm_rows ? perm[p] : (uint32_t)p;
        if ((liveBits[r >> 5] >> (r & 31)) & 1u) id = r;
        o = row_as_query(rowMeta[p], rho);
    }
    qm[p] = o;
    cid[p] = id;
}

hipError_t zh_launch_join_prep(const float2 *dRowMeta, const uint32_t *dPerm, uint64_t perm_rows, const uint32_t *dLiveBits, uint64_t n_rows, float rho,
                               float4 *dQm, uint32_t *dCid, hipStream_t s) {
    const uint64_t n_pos = (n_rows + 15) / 16 * 16;
    if (!n_pos) return hipSuccess;
    hipLaunchKernelGGL(join_prep_kernel, dim3((uint32_t)((n_pos + 255) / 256)), dim3(256), 0, s, dRowMeta, dPerm, perm_rows, dLiveBits, n_rows, n_pos, rho, dQm,
                       dCid);
    return hipGetLastError();
}

// The launch geometry of a panel of held tiles [tileA0, tileA1) of T (tileA0 a multiple of 4; tileA1 one too, or T).  A block holds four consecutive
// tiles from I0 = tileA0 + 4 ab and walks ONE chunk of ZH_JOIN_CHUNK tiles J, chunk c = [I0 + c CH, min(T, I0 + (c + 1) CH)): chunks are counted from
// the block's own diagonal, so none lies wholly below it and none is launched that would.  first[ab] = the panel's blocks before held block ab
// (first[n_ab] = all of them).  A wave skips the tiles J < I of the first chunk, and a block's chunks cover [I0, T) once: wave I issues T - I tile
// products.  Returns their sum over the panel -- the `tiles` of zh_join_info, from the geometry alone.
uint64_t zh_join_geometry(uint64_t T, uint64_t tileA0, uint64_t tileA1, uint32_t *first) {
    const uint64_t n_ab = (tileA1 - tileA0 + 3) / 4;
    uint64_t blocks = 0, products = 0;
    for (uint64_t ab = 0; ab < n_ab; ab++) {
        const uint64_t I0 = tileA0 + 4 * ab;
        first[ab] = (uint32_t)blocks;
        blocks += (T - I0 + ZH_JOIN_CHUNK - 1) / ZH_JOIN_CHUNK;
        for (uint64_t I = I0; I < I0 + 4 && I < T; I++) products += T - I;
    }
    first[n_ab] = (uint32_t)blocks;
    return products;
}

template <int D, int KINDA>
__global__ __launch_bounds__(256) void join_mfma_kernel(const u32x4 *__restrict__ Xh, const float2 *__restrict__ rowMeta, const float4 *__restrict__ qm,
                                                        const uint32_t *__restrict__ cid, uint64_t T, uint64_t tileA0, const uint32_t *__restrict__ first,
                                                        uint32_t n_ab, float Kc, float rho, const uint32_t *__restrict__ tau, uint64_t *__restrict__ cand,
                                                        uint64_t cap, unsigned long long *__restrict__ ctr) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wid = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t ab = last_le(n_ab, blockIdx.x, [&](uint32_t i) { return first[i]; });  // the held block (block-uniform)
    const uint64_t I0 = tileA0 + 4ull * ab, I = I0 + wid;
    const uint64_t Jb = I0 + (uint64_t)(blockIdx.x - first[ab]) * ZH_JOIN_CHUNK, Je = Jb + ZH_JOIN_CHUNK < T ? Jb + ZH_JOIN_CHUNK : T;
    const bool active = I < T;  // (wave-uniform: the table's last block may hold fewer than four tiles)
    f16x8 A[D / 32];
    held_tile<D>(A, Xh, (size_t)I, active, lane);
    PoolSink<KINDA, true, uint64_t> sink{lane, I, tau[0], Kc, rho, cand, cap, ctr};
    sink.hold(active, cid, rowMeta);
    held_walk<D>(A, active, Xh, cid, qm, Jb, Je, sink);  // (a wave skips the tiles J < I of the first chunk)
}

hipError_t zh_launch_join_mfma(uint32_t d, int metric, int mode, const void *dXh, const float2 *dRowMeta, const float4 *dQm, const uint32_t *dCid,
                               uint64_t n_rows, uint64_t tileA0, const uint32_t *dFirst, uint32_t n_ab, uint32_t blocks, float Kc, float rho,
                               const uint32_t *dTau, uint64_t *dCand, uint64_t cand_cap, unsigned long long *dCandCtr, hipStream_t s) {
    const uint64_t T = (n_rows + 15) / 16;
    if (!blocks || !n_ab) return hipSuccess;
    if (tileA0 % 4 || tileA0 >= T) return hipErrorInvalidValue;
    return zh_mfma_dispatch(d, metric, mode, [&](auto D, auto K) {
        hipLaunchKernelGGL((join_mfma_kernel<D, K>), dim3(blocks), dim3(256), 0, s, (const u32x4 *)dXh, dRowMeta, dQm, dCid, T, tileA0, dFirst, n_ab, Kc, rho,
                           dTau, dCand, cand_cap, dCandCtr);
    });
}

// The candidates' canonical keys, in the manner of range_survivors_kernel -- and their judgement, for the three joins.  A candidate is a << 32 | b:
// the key is that of STORED row b of table XB against the QUERY row a of table XA, both f32 tables; the cosine's query norm is qnorm_kernel's sum
// (the canonical one) of row a.  The self-join and the forest join pass their one table twice: XA and XB are only read, so that two __restrict__
// pointers alias there breaks no promise.  A wave takes 64 candidates at a time: pair j's sums wait in lane j, so that key_of, the comparison and
// the pool's atomic run once for all 64.  OWNED (the forest join, candidates met in tree t): the first-tree rule comes first, only the pairs it
// leaves get a key and *keyed += their number; the plain kernel reads none of leaf_of, T, t and keyed.  TWO = false (XA == XB, the launcher sees
// to it): both rows' addresses come from ONE per-lane base -- the second base is a register pair, which at d = 768 (cosine) and in the OWNED
// kernel at d >= 512 is the step from 6 waves per SIMD to 5.
template <int D, int KIND, bool OWNED, bool TWO>
__global__ __launch_bounds__(256) void pair_survivors_kernel(const float *__restrict__ XA, const float *__restrict__ XB, int metric, int param,
                                                             const uint64_t *__restrict__ cand, const unsigned long long *__restrict__ candCtr,
                                                             uint64_t cand_cap, const uint32_t *__restrict__ leaf_of, uint32_t T, uint32_t t, uint64_t max_key,
                                                             unsigned long long *__restrict__ ctr, unsigned long long *__restrict__ keyed,
                                                             uint64_t *__restrict__ pv, uint64_t *__restrict__ pk, uint64_t cap) {
    const uint64_t n = *candCtr;
    if (n > cand_cap) return;  // (the pool ran over: the panel or batch is answered by path 1)
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t wave = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = (uint64_t)gridDim.x * 4;
    for (uint64_t g = wave * 64; g < n; g += n_waves * 64) {
        const uint32_t m = n - g < 64 ? (uint32_t)(n - g) : 64u;
        const uint64_t mine = lane < m ? cand[g + lane] : 0ull;
        const uint32_t my_b = (uint32_t)mine, my_a = (uint32_t)(mine >> 32);
        uint64_t own = 0;
        if constexpr (OWNED) {
            own = __ballot(lane < m && fjoin_owned(leaf_of, T, t, my_a, my_b));
            if (!own) continue;  // (wave-uniform)
            if (lane == 0) atomicAdd(keyed, (unsigned long long)__popcll(own));
        }
        float m0 = 0.f, m1 = 0.f, mq = 0.f;
        for (uint32_t j = 0; j < m; j++) {
            if constexpr (OWNED) {
                if (!((own >> j) & 1ull)) continue;  // (wave-uniform)
            }
            const uint32_t row = (uint32_t)__builtin_amdgcn_readlane((int)my_b, (int)j), qrow = (uint32_t)__builtin_amdgcn_readlane((int)my_a, (int)j);
            float s0 = 0.f, s1 = 0.f, qq = 0.f;
            table_pair_sums<D, KIND, true>(TWO ? XB : XA, row, XA, qrow, lane, param, s0, s1, qq);
            if (lane == j) { m0 = s0; m1 = s1; mq = qq; }
        }
        uint64_t key = 0;
        bool hit = false;
        if (OWNED ? (bool)((own >> lane) & 1ull) : lane < m) {
            key = key_of(metric, param, m0, m1, mq);
            hit = key <= max_key;
        }
        const uint64_t hm = __ballot(hit);
        if (hm) {  // (wave-uniform)
            const unsigned long long slot = wave_slots(ctr, hm, lane);
            if (hit && slot < cap) { pv[slot] = mine; pk[slot] = key; }
        }
    }
}

// dLeafOf == nullptr: the plain kernel (T, t and dKeyed are not read); the forest join has one table
template <int D, int KIND>
static void launch_pair_surv(const float *dXA, const float *dXB, int metric, int mode, const uint64_t *dCand, const unsigned long long *dCandCtr,
                             uint64_t cand_cap, const uint32_t *dLeafOf, uint32_t T, uint32_t t, uint64_t max_key, unsigned long long *dHitCtr,
                             unsigned long long *dKeyed, uint64_t *dPoolV, uint64_t *dPoolK, uint64_t pool_cap, hipStream_t s) {
    // the candidate count is known on the device only: enough waves for 64 candidates each up to the pool's size, at most 4096 of them
    const uint32_t blocks = (uint32_t)std::min<uint64_t>(1024, std::max<uint64_t>(1, (cand_cap + 255) / 256));
    const auto kernel = dLeafOf      ? pair_survivors_kernel<D, KIND, true, false>
                        : dXA == dXB ? pair_survivors_kernel<D, KIND, false, false>
                                     : pair_survivors_kernel<D, KIND, false, true>;
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, s, dXA, dXB, metric, mode, dCand, dCandCtr, cand_cap, dLeafOf, T, t, max_key, dHitCtr, dKeyed, dPoolV,
                       dPoolK, pool_cap);
}

hipError_t zh_launch_pair_survivors(const float *dXA, const float *dXB, uint32_t d, int metric, int mode, const uint64_t *dCand,
                                    const unsigned long long *dCandCtr, uint64_t cand_cap, const uint32_t *dLeafOf, uint32_t T, uint32_t t, uint64_t max_key,
                                    unsigned long long *dHitCtr, unsigned long long *dKeyed, uint64_t *dPoolV, uint64_t *dPoolK, uint64_t pool_cap,
                                    hipStream_t s) {
    if (dLeafOf && dXA != dXB) return hipErrorInvalidValue;
#define ZH_PAIR_SURV(DD)                                                                                                                                   \
    case DD:                                                                                                                                                \
        if (metric == ZH_COSINE)                                                                                                                            \
            launch_pair_surv<DD, K_COS>(dXA, dXB, metric, mode, dCand, dCandCtr, cand_cap, dLeafOf, T, t, max_key, dHitCtr, dKeyed, dPoolV, dPoolK, pool_cap, s); \
        else                                                                                                                                                \
            launch_pair_surv<DD, K_L2>(dXA, dXB, metric, mode, dCand, dCandCtr, cand_cap, dLeafOf, T, t, max_key, dHitCtr, dKeyed, dPoolV, dPoolK, pool_cap, s);  \
        break
    switch (d) {
        ZH_PAIR_SURV(256);
        ZH_PAIR_SURV(384);
        ZH_PAIR_SURV(512);
        ZH_PAIR_SURV(768);
        ZH_PAIR_SURV(1024);
    default: return hipErrorInvalidValue;
    }
#undef ZH_PAIR_SURV
    return hipGetLastError();
}

// a panel whose candidates ran over: its live rows (positions [p_begin, p_end) of the copy, any order) as path 1's query rows; *dCount += their number
__global__ __launch_bounds__(256) void join_panel_rows_kernel(const uint32_t *__restrict__ cid, uint64_t p_begin, uint64_t p_end, uint32_t *__restrict__ list,
                                                              unsigned long long *__restrict__ count) {
    const uint64_t p = p_begin + (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t id = p < p_end ? cid[p] : 0xFFFFFFFFu;
    const bool on = id != 0xFFFFFFFFu;
    const uint64_t m = __ballot(on);
    if (!m) return;  // (wave-uniform)
    const unsigned long long slot = wave_slots(count, m, lane);
    if (on) list[slot] = id;
}

hipError_t zh_launch_join_panel_rows(const uint32_t *dCid, uint64_t p_begin, uint64_t p_end, uint32_t *dList, unsigned long long *dCount, hipStream_t s) {
    if (p_begin >= p_end) return hipSuccess;
    hipLaunchKernelGGL(join_panel_rows_kernel, dim3((uint32_t)((p_end - p_begin + 255) / 256)), dim3(256), 0, s, dCid, p_begin, p_end, dList, dCount);
    return hipGetLastError();
}

// ---- both paths: the order (a, key, b): zh_launch_pool_sort (zh_range.hip) over the b bits, the key and the a bits of the pool, then the emit ----
__global__ __launch_bounds__(256) void pair_emit_kernel(const uint64_t *__restrict__ v, const uint64_t *__restrict__ k, uint64_t n, uint64_t id_base_a,
                                                        uint64_t id_base_b, uint64_t *__restrict__ out_a, uint64_t *__restrict__ out_b,
                                                        uint64_t *__restrict__ keys) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) { out_a[i] = id_base_a + (v[i] >> 32); out_b[i] = id_base_b + (v[i] & 0xFFFFFFFFull); keys[i] = k[i]; }
}

// the pool of a join ordered by (a, key, b) and written out: the b bits of v hold n_rows_b values, the a bits n_rows_a; each side has its id base
hipError_t zh_launch_pair_sort(uint64_t *dV[2], uint64_t *dK[2], uint64_t n, uint64_t n_rows_a, uint64_t n_rows_b, void *dTmp, size_t *tmp_bytes,
                               uint64_t id_base_a, uint64_t id_base_b, uint64_t *dOutA, uint64_t *dOutB, uint64_t *dOutKeys, hipStream_t s) {
    if (dTmp && !n) return hipSuccess;
    const uint64_t *v = nullptr, *k = nullptr;
    const hipError_t e = zh_launch_pool_sort(dV, dK, n, n_rows_b, n_rows_a, false, dTmp, tmp_bytes, &v, &k, s);
    if (e != hipSuccess || !dTmp) return e;
    hipLaunchKernelGGL(pair_emit_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, v, k, n, id_base_a, id_base_b, dOutA, dOutB, dOutKeys);
    return hipGetLastError();
}
