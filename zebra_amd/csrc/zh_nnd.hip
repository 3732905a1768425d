// zh_nnd.hip -- NN-descent's incremental rounds (zh_knn_graph_descent, driver in zh_api.hip).  Round 1 is zh_refine.hip's and zh_reverse.hip's; from
// round 2 on the graph stays on the device as u32 row numbers [stored rows][k] with its keys beside it, and a line keys only what a NEW entry brings
// up.  With U_r(x) = the line round r + 1 ranks over (N'(G_r)(x), then the kept reverse neighbours R'(x) of G_r; w = k + rev_k wide) an entry of
// U_r(x) is new when U_{r-1}(x) does not hold it, and round r + 1 gathers for row a
//   every new e of U_r(a);  all of U_r(e) for a new e;  the new entries of U_r(e) for an old e,
// drops a itself and the members of its own forward line N'(G_r)(a), keys the rest and ranks them together with the forward line, whose keys are
// carried.  That is bit for bit the full round's line: what only old hops reach was a candidate the round before and lost to k rows that are
// candidates again.
//
//   nnd_rows_kernel   round 1's ids -> row numbers (the only u64 -> u32 pass of the call; a round's output is already N': live, distinct, no self)
//   nnd_flag_kernel   a wave per stored line, lane j its entry j of U_r: new if no entry of U_{r-1}(x) equals it (shuffles) -> one u64 mask a line;
//                     the population count is a popcount away and is not stored
//   nnd_plan_kernel   a wave per live line: the exact raw gather count (per own entry: 1 + w if new, popcount(mask(e)) if old); 0 -> the line is
//                     copied across; otherwise its row goes on the list -- from the front if the count fits ZH_REFINE_CAP_SMALL, from the back if not
//   nnd_line_kernel   256-thread blocks striding over one half of the list (the counts are read on the device: no readback before the launch),
//                     refine_line_kernel's stages: gather into LDS, sort, compact the distinct rows that the forward line does not hold
//                     (refine_compact, the drop bitmap its predicate), key them (refine_key_list: the SAME routine, so the same arithmetic), sort
//                     by (key, id), merge the best 64 with the forward line in a 128-slot sort, write the first k row numbers and keys to the
//                     OTHER table (never in place: other blocks read this round's lines meanwhile)
//   nnd_emit_kernel   at the end: row numbers -> ids with id_base, tails 2^64 - 1, counts
// The wave-per-line kernels are launched ZH_LINES_PER_LAUNCH lines at a time (zh_for_line_pieces); nnd_line_kernel's instantiation is
// zh_dispatch_kind_dim's (zh_device.h).  DESIGN.md s25.
#include "zh_refine_dev.h"

// a wave per line, lane j its entry j (k <= 64)
__global__ __launch_bounds__(256) void nnd_rows_kernel(const uint64_t *__restrict__ ids, uint64_t id_base, uint64_t nl, uint32_t k, uint32_t *__restrict__ tab) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t i = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= nl || lane >= k) return;
    const uint64_t id = ids[i * k + lane];
    tab[i * k + lane] = id == ~0ull ? RF_NONE : (uint32_t)(id - id_base);
}

__global__ __launch_bounds__(256) void nnd_emit_kernel(const uint32_t *__restrict__ tab, const uint64_t *__restrict__ keys, uint32_t k, uint64_t id_base,
                                                       uint64_t nl, uint64_t *__restrict__ out_ids, uint64_t *__restrict__ out_keys,
                                                       uint32_t *__restrict__ out_counts) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t i = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= nl) return;  // (wave-uniform)
    const uint32_t r = lane < k ? tab[i * k + lane] : RF_NONE;
    const uint32_t have = (uint32_t)__popcll(__ballot(r != RF_NONE));
    if (lane < k) {
        out_ids[i * k + lane] = r == RF_NONE ? ~0ull : id_base + r;
        out_keys[i * k + lane] = r == RF_NONE ? ~0ull : keys[i * k + lane];
    }
    if (lane == 0) out_counts[i] = have;
}

__global__ __launch_bounds__(256) void nnd_flag_kernel(const uint32_t *__restrict__ prev, uint32_t wp, const uint32_t *__restrict__ cur, uint32_t wc,
                                                       uint64_t x0, uint64_t nl, uint64_t *__restrict__ mask) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t i = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= nl) return;  // (wave-uniform)
    const uint64_t x = x0 + i;
    const uint32_t c = lane < wc ? cur[x * wc + lane] : RF_NONE;
    const uint32_t p = lane < wp ? prev[x * wp + lane] : RF_NONE;
    bool isnew = c != RF_NONE;
    for (uint32_t j = 0; j < wp; j++) {  // (wave-uniform bound; by every lane)
        const uint32_t o = (uint32_t)__shfl((int)p, (int)j, 64);
        isnew = isnew && o != c;
    }
    const uint64_t m = __ballot(isnew);
    if (lane == 0) mask[x] = m;
}

__global__ __launch_bounds__(256) void nnd_plan_kernel(const uint32_t *__restrict__ U, uint32_t w, uint32_t k, const uint64_t *__restrict__ mask,
                                                       const uint32_t *__restrict__ rows, uint64_t i0, uint64_t nl, uint64_t n_live,
                                                       const uint64_t *__restrict__ keys, uint32_t *__restrict__ tab_next, uint64_t *__restrict__ keys_next,
                                                       uint32_t *__restrict__ list, unsigned long long *__restrict__ ctr) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t i = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= nl) return;  // (wave-uniform)
    const uint32_t a = rows[i0 + i];
    const uint32_t e = lane < w ? U[(size_t)a * w + lane] : RF_NONE;
    const uint64_t ma = mask[a];
    uint32_t raw = 0;
    if (e != RF_NONE) raw = ((ma >> lane) & 1ull) ? 1u + w : (uint32_t)__popcll(mask[e]);
    for (int o = 32; o > 0; o >>= 1) raw += (uint32_t)__shfl_xor((int)raw, o, 64);
    if (raw == 0) {  // nothing new within two hops: the line stands
        if (lane < k) {
            tab_next[(size_t)a * k + lane] = e;
            keys_next[(size_t)a * k + lane] = keys[(size_t)a * k + lane];
        }
    } else if (lane == 0) {
        if (raw <= ZH_REFINE_CAP_SMALL) list[atomicAdd(&ctr[4], 1ull)] = a;
        else list[n_live - 1 - atomicAdd(&ctr[5], 1ull)] = a;  // (the two ends never meet: n_live lines in all)
    }
}

template <int D, int KIND, int CAP>
__global__ __launch_bounds__(256) void nnd_line_kernel(const float *__restrict__ X, uint32_t d, const uint32_t *__restrict__ U, uint32_t w, uint32_t k,
                                                       const uint64_t *__restrict__ mask, const uint64_t *__restrict__ keys, const float *__restrict__ QQ,
                                                       const uint32_t *__restrict__ list, uint64_t n_live, int metric, int param,
                                                       uint32_t *__restrict__ tab_next, uint64_t *__restrict__ keys_next, unsigned long long *__restrict__ ctr) {
    constexpr bool LARGE = CAP > ZH_REFINE_CAP_SMALL;
    __shared__ uint64_t s_key[CAP];
    __shared__ uint32_t s_id[CAP];
    __shared__ uint64_t s_mkey[128];  // the merge: the best 64 of the keyed candidates, then the forward line with its carried keys
    __shared__ uint32_t s_mid[128];
    __shared__ uint32_t s_own[64], s_off[65], s_scan[256], s_drop[CAP / 32], s_red[4];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const unsigned long long cnt = ctr[LARGE ? 5 : 4];  // (final: the plan pass is done)
    for (unsigned long long b = blockIdx.x; b < cnt; b += gridDim.x) {  // (block-uniform)
        const uint32_t a = LARGE ? list[n_live - 1 - b] : list[b];
        const uint64_t ma = mask[a];
        const uint32_t pn = (uint32_t)__popcll(ma);
        // ---- (a) the line of a, the forward part with its keys into the merge's upper half, and where every entry's stretch of the gather begins
        if (wv == 0) {
            const uint32_t e = lane < w ? U[(size_t)a * w + lane] : RF_NONE;
            const bool isnew = (ma >> lane) & 1ull;
            uint32_t c = 0;
            if (e != RF_NONE) c = isnew ? w : (uint32_t)__popcll(mask[e]);
            uint32_t inc = c;
            for (uint32_t o = 1; o < 64; o <<= 1) {
                const uint32_t t = (uint32_t)__shfl_up((int)inc, o, 64);
                if (lane >= o) inc += t;
            }
            s_own[lane] = e;
            s_off[lane] = pn + inc - c;
            if (lane == 63) s_off[64] = pn + inc;
            s_mid[64 + lane] = lane < k ? e : RF_NONE;
            s_mkey[64 + lane] = (lane < k && e != RF_NONE) ? keys[(size_t)a * k + lane] : ~0ull;
            if (isnew) s_id[__popcll(ma & ((1ull << lane) - 1ull))] = e;  // (a new entry is a row: never a, never RF_NONE)
        }
        __syncthreads();
        const uint32_t raw = s_off[64], np2 = next_pow2(raw);  // (raw <= CAP: the plan pass's count, list by list)
        uint32_t mine = 0;
        for (uint32_t j = wv; j < w; j += 4) {  // (wave-uniform)
            const uint32_t e = s_own[j];
            if (e == RF_NONE) continue;
            const uint32_t off = s_off[j];
            const uint32_t v = lane < w ? U[(size_t)e * w + lane] : RF_NONE;
            if ((ma >> j) & 1ull) {
                if (lane < w) s_id[off + lane] = v == a ? RF_NONE : v;
                mine += v != RF_NONE ? 1u : 0u;
            } else {
                const uint64_t me = mask[e];
                if ((me >> lane) & 1ull) {
                    s_id[off + (uint32_t)__popcll(me & ((1ull << lane) - 1ull))] = v == a ? RF_NONE : v;
                    mine++;
                }
            }
        }
        for (uint32_t e = raw + tid; e < np2; e += 256) s_id[e] = RF_NONE;
        for (uint32_t e = tid; e < (np2 + 31) / 32; e += 256) s_drop[e] = 0;
        const uint32_t listed = pn + block_sum_u32(mine, s_red);
        block_bitonic_sort_u32(s_id, np2);
        // the members of the forward line are candidates already: the first slot of each, where the list holds it, is marked
        if (tid < k) {
            const uint32_t f = s_own[tid];
            if (f != RF_NONE) {
                uint32_t lo = 0, hi = np2;
                while (lo < hi) {
                    const uint32_t mid = (lo + hi) >> 1;
                    if (s_id[mid] < f) lo = mid + 1; else hi = mid;
                }
                if (lo < np2 && s_id[lo] == f) atomicOr(&s_drop[lo >> 5], 1u << (lo & 31));
            }
        }
        __syncthreads();
        // the first entry of every row number that is not marked, compacted to the front
        const uint32_t S = refine_compact<CAP>(s_id, s_key, s_scan, np2, [&](uint32_t i) { return !((s_drop[i >> 5] >> (i & 31)) & 1u); }), up2 = next_pow2(S);
        // ---- (b) the keys of S(a): wave wv takes candidates 4 R t + 4 c + wv, c < R at a time
        if (S) {  // (block-uniform)
            const float *q = X + (size_t)a * d;
            RowRegs<D> qreg;
            if constexpr (D > 0) load_row<D>(q, lane, qreg);
            refine_key_list<D, KIND>(X, d, s_id, S, q, qreg, KIND == K_COS ? QQ[a] : 0.f, lane, wv, metric, param, s_key);
            // ---- (c) rank by (key, id); the slots from S to up2 hold (all ones, UINT32_MAX) and stay last
            block_bitonic_sort<uint32_t>(s_key, s_id, up2);
        }
        if (tid < 64) {
            const bool have = S && tid < up2;
            s_mkey[tid] = have ? s_key[tid] : ~0ull;
            s_mid[tid] = have ? s_id[tid] : RF_NONE;
        }
        block_bitonic_sort<uint32_t>(s_mkey, s_mid, 128);
        mine = 0;
        if (tid < k) {
            const uint32_t r = s_mid[tid];
            if (r != RF_NONE) {
                bool old = false;
                for (uint32_t j = 0; j < k; j++) old = old || s_own[j] == r;
                mine = old ? 0u : 1u;
            }
            tab_next[(size_t)a * k + tid] = r;
            keys_next[(size_t)a * k + tid] = r != RF_NONE ? s_mkey[tid] : ~0ull;
        }
        const uint32_t updates = block_sum_u32(mine, s_red);
        if (tid == 0) {
            if (listed) atomicAdd(&ctr[0], (unsigned long long)listed);
            if (S) {
                atomicAdd(&ctr[1], (unsigned long long)S);
                atomicAdd(&ctr[3], 1ull);
            }
            if (updates) atomicAdd(&ctr[2], (unsigned long long)updates);
        }
        __syncthreads();  // (the line's LDS is read)
    }
}

// ---------------------------------------------------------------------------------------------------------------- launchers
hipError_t zh_launch_nnd_rows(const uint64_t *dIds, uint64_t id_base, uint64_t nl, uint32_t k, uint32_t *dTab, hipStream_t s) {
    if (!k || k > ZH_REFINE_MAX_IN_K) return hipErrorInvalidValue;
    zh_for_line_pieces(nl, [&](uint64_t b0, uint64_t m, uint32_t blocks) {
        hipLaunchKernelGGL(nnd_rows_kernel, dim3(blocks), dim3(256), 0, s, dIds + b0 * k, id_base, m, k, dTab + b0 * k);
    });
    return hipGetLastError();
}

hipError_t zh_launch_nnd_emit(const uint32_t *dTab, const uint64_t *dKeys, uint32_t k, uint64_t id_base, uint64_t nl, uint64_t *dOutIds, uint64_t *dOutKeys,
                              uint32_t *dOutCounts, hipStream_t s) {
    if (!k || k > ZH_REFINE_MAX_IN_K) return hipErrorInvalidValue;
    zh_for_line_pieces(nl, [&](uint64_t b0, uint64_t m, uint32_t blocks) {
        hipLaunchKernelGGL(nnd_emit_kernel, dim3(blocks), dim3(256), 0, s, dTab + b0 * k, dKeys + b0 * k, k, id_base, m, dOutIds + b0 * k, dOutKeys + b0 * k,
                           dOutCounts + b0);
    });
    return hipGetLastError();
}

hipError_t zh_launch_nnd_flag(const uint32_t *dPrev, uint32_t wp, const uint32_t *dCur, uint32_t wc, uint64_t n_rows, uint64_t *dMask, hipStream_t s) {
    if (!wp || wp > ZH_REFINE_MAX_IN_K || !wc || wc > ZH_REFINE_MAX_IN_K) return hipErrorInvalidValue;
    zh_for_line_pieces(n_rows, [&](uint64_t b0, uint64_t m, uint32_t blocks) {
        hipLaunchKernelGGL(nnd_flag_kernel, dim3(blocks), dim3(256), 0, s, dPrev, wp, dCur, wc, b0, m, dMask);
    });
    return hipGetLastError();
}

hipError_t zh_launch_nnd_plan(const uint32_t *dU, uint32_t w, uint32_t k, const uint64_t *dMask, const uint32_t *dRows, uint64_t n_live, const uint64_t *dKeys,
                              uint32_t *dTabNext, uint64_t *dKeysNext, uint32_t *dList, unsigned long long *dCtr, hipStream_t s) {
    if (!k || k > w || w > ZH_REFINE_MAX_IN_K) return hipErrorInvalidValue;
    zh_for_line_pieces(n_live, [&](uint64_t b0, uint64_t m, uint32_t blocks) {
        hipLaunchKernelGGL(nnd_plan_kernel, dim3(blocks), dim3(256), 0, s, dU, w, k, dMask, dRows, b0, m, n_live, dKeys, dTabNext, dKeysNext, dList, dCtr);
    });
    return hipGetLastError();
}

// both halves of the list, each by its instantiation; a half that is empty costs blocks that read one counter and leave
hipError_t zh_launch_nnd_lines(const float *dX, uint32_t d, const uint32_t *dU, uint32_t w, uint32_t k, const uint64_t *dMask, const uint64_t *dKeys, const float *dQQ,
                               const uint32_t *dList, uint64_t n_live, int metric, int param, uint32_t *dTabNext, uint64_t *dKeysNext, unsigned long long *dCtr,
                               hipStream_t s) {
    if (!n_live) return hipSuccess;
    if (!k || k > w || w > ZH_REFINE_MAX_IN_K || w + w * w > ZH_REFINE_CAP_LARGE) return hipErrorInvalidValue;
    const uint32_t small = (uint32_t)std::min<uint64_t>(n_live, 4096), large = (uint32_t)std::min<uint64_t>(n_live, 1024);
    return zh_dispatch_kind_dim(metric, d, [&](auto kind, auto dim) {
        constexpr int KIND = decltype(kind)::value, D = decltype(dim)::value;
        hipLaunchKernelGGL((nnd_line_kernel<D, KIND, ZH_REFINE_CAP_SMALL>), dim3(small), dim3(256), 0, s, dX, d, dU, w, k, dMask, dKeys, dQQ, dList, n_live, metric, param,
                           dTabNext, dKeysNext, dCtr);
        if (w + w * w > ZH_REFINE_CAP_SMALL)  // (otherwise no line's count passes the small one's slots, and the back of the list is empty)
            hipLaunchKernelGGL((nnd_line_kernel<D, KIND, ZH_REFINE_CAP_LARGE>), dim3(large), dim3(256), 0, s, dX, d, dU, w, k, dMask, dKeys, dQQ, dList, n_live, metric,
                               param, dTabNext, dKeysNext, dCtr);
        return hipGetLastError();
    });
}
