// zh_gsearch.hip -- graph search (zh_search_graph_batch, driver in zh_api.hip): a best-first walk over the k-NN graph an index keeps
// (zh_index_set_graph: zh_launch_refine_rows' table of u32 row numbers, [g_rows][g_k], UINT32_MAX for a masked entry).  Per query:
//   the beam B = the first `beam` of the query's valid seeds by (key, id), every entry unexpanded; then, while B has an unexpanded entry (and the
//   iteration cap is not reached): P = its first `width` unexpanded entries, marked expanded; cand = the live rows their lines name, each once,
//   minus the rows in B now; B = the first `beam` of B union cand by (key, id).  The answer is the first top_k of B.
// Keys, ids, tails and counts as zh_exact.hip: what is approximate is the set of rows that get a key, never the arithmetic.  DESIGN.md s24.
//
//   gsearch_kernel   a 256-thread block per query, nothing per candidate leaves the block.  The query sits in registers (load_row's lane layout; the
//                    generic kernel reads it from memory), the beam in LDS: slots [0, 256) hold B sorted by (key, row), the id word is row << 1 |
//                    expanded; slots [256, 512) hold an iteration's candidates.  An iteration: (1) a ballot / prefix pass over the beam's flags picks
//                    P; (2) thread e reads entry e % g_k of parent e / g_k's line and tests it against the live bitmap; (3) it is dropped if an
//                    EARLIER parent's line holds it (a line holds no row twice: zh_launch_refine_rows) or the beam does -- a broadcast scan of the
//                    beam's id words, every lane reading the same LDS address; (4) the survivors are compacted; (5) the four waves key them,
//                    ZH_REFINE_INFLIGHT rows in flight per wave (refine_line_kernel's step (b), refine_key's arithmetic); (6) every beam entry
//                    and every candidate finds its place in the union by counting: the candidates below it (one broadcast pass over the at most
//                    256 of them) plus, for a candidate, the beam entries below it (a binary search of the sorted beam) -- all (key, row) pairs are
//                    distinct, so the counts are a permutation; what lands below `beam` is written there.  No sort: eight barriers an iteration.
// Step (5) is refine_key_list's loop (zh_refine_dev.h) written out here, with >> 1 on the id word: shared, gsearch_kernel<1024, K_COS> lost an
// occupancy step or the width-4 searches 1 to 2 % of their speed, depending on the row a slot past the list reloads.  The key itself
// is the shared refine_key.
//
//   gsearch_filtered_kernel   zh_search_graph_filtered_batch: the same block body (gsearch_block<D, KIND, FILT>) with a second list R in
//                    LDS, the first top_k by (key, row) of the rows keyed so far that the call's allowed-AND-live bitmap allows.  The walk does not see
//                    the filter.  Inside absorb, once the keys are in ckey: (F1) a candidate whose bit is set passes unless R holds it now -- a
//                    broadcast scan of R's at most top_k id words -- and says so in bit 0 of its candidate word; (F2) step (6)'s pass over the
//                    candidates also counts the passing ones below each entry of R and below each candidate, and a passing candidate adds the
//                    entries of R below it by a binary search; (F3) what lands below top_k is written.  One barrier more an iteration.  A row keyed
//                    again is in R (dropped) or lost to a full R whose last entry never rises (loses again): R is exact.  The answer is R.
//
//   gsearch_steered_kernel    zh_search_graph_steered_batch: the unfiltered body (gsearch_block<D, KIND, false, STEER>) walking the rows of
//                    the allowed-AND-live bitmap only.  The seed test and step (2) read `allow`; with hops == 2 a disallowed live entry of a parent's
//                    line is a bridge, and between step (3) and absorb: (S1) the direct rows and the bridges are compacted, each in (parent, entry)
//                    order; (S2) in passes of up to GS_HOP_SUB x 256 table entries, thread e holding entry e % g_k of bridge e / g_k of each
//                    sub-pass, the entries whose `allow` bit is set are compacted in emission order, dropped if an earlier one of the pass, the
//                    candidate list so far or the beam holds the row, and appended to the list up to slot 255 -- first emission wins, the list is
//                    cut at 256.  Four barriers a pass.  Thread t then takes entry t of the list into absorb, which is unchanged; the answer is B.
#include "zh_refine_dev.h"  // refine_key, RowRegs, RF_NONE, ZH_REFINE_INFLIGHT: the key of a gathered row against a row held in registers

#define GS_SLOTS ZH_GRAPH_MAX_BEAM  // beam slots, and candidate slots behind them (width * g_k <= 256, seeds <= 64)
static_assert(GS_SLOTS == 256, "one thread per beam slot and per candidate slot");
static_assert(GS_SLOTS == ZH_GRAPH_MAX_CAND, "the steered walk's cut is the candidate slots of the block");
#define GS_HOP_SUB 4  // sub-passes of 256 table entries a thread holds per second-hop pass (gsearch_steered_kernel)

// (key, row) below (key, row)
__device__ __forceinline__ bool gs_less(uint64_t ka, uint32_t ra, uint64_t kb, uint32_t rb) { return ka < kb || (ka == kb && ra < rb); }

// the block of all three kernels.  FILT: the second list (allow: the allowed-AND-live bitmap of the call's filter pass; null without).  STEER: the
// walk over the rows of `allow` alone, `hops` 1 or 2; s_br [GS_SLOTS] and s_wx [4 GS_HOP_SUB] are the steered kernel's own LDS (null without)
template <int D, int KIND, bool FILT, bool STEER = false>
__device__ __forceinline__ void gsearch_block(const float *__restrict__ X, uint32_t d, uint64_t n_rows, const uint32_t *__restrict__ tab, uint64_t g_rows, uint32_t g_k,
                                              const uint32_t *__restrict__ bits, const uint32_t *__restrict__ allow, const float *__restrict__ Q,
                                              const float *__restrict__ QQ, const uint64_t *__restrict__ seeds, uint32_t n_seed, uint64_t id_base, uint32_t top_k,
                                              uint32_t beam, uint32_t width, uint32_t max_iters, int metric, int param, uint64_t *__restrict__ out_ids,
                                              uint64_t *__restrict__ out_keys, uint32_t *__restrict__ out_counts, unsigned long long *__restrict__ ctr,
                                              uint32_t hops = 0, uint32_t *s_br = nullptr, uint32_t *s_wx = nullptr) {
    constexpr int R = ZH_REFINE_INFLIGHT;
    __shared__ uint64_t s_key[2 * GS_SLOTS];
    __shared__ uint32_t s_id[2 * GS_SLOTS];
    __shared__ uint32_t s_raw[GS_SLOTS], s_par[GS_SLOTS], s_wc[4];
    __shared__ uint64_t r_key[FILT ? GS_SLOTS : 1];  // the second list: the first top_k allowed rows met so far, sorted by (key, row)
    __shared__ uint32_t r_id[FILT ? GS_SLOTS : 1];   // (plain row numbers)
    uint32_t nr = 0, n_off = 0;  // |R| (block-uniform); the allowed rows this WAVE's lanes saw offered (wave-uniform)
    const uint32_t tid = threadIdx.x, lane = tid & 63, wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const size_t b = blockIdx.x;
    const float *q = Q + b * d;
    const float qq = KIND == K_COS ? QQ[b] : 0.f;
    RowRegs<D> qreg;
    if constexpr (D > 0) load_row<D>(q, lane, qreg);
    uint64_t *ckey = s_key + GS_SLOTS;
    uint32_t *cid = s_id + GS_SLOTS;
    uint32_t nb = 0;  // |B| (block-uniform)
    uint32_t n_seeds = 0, n_iter = 0, n_exp = 0, n_keyed = 0, capped = 0;
    uint32_t n_direct = 0, n_via = 0, n_bridge = 0, n_full = 0;  // (STEER)

    // thread tid's candidate row v (RF_NONE: none) joins the beam: steps (4) to (6).  -> the candidates keyed.  (Every thread calls it.)
    auto absorb = [&](uint32_t v) -> uint32_t {
        // (4) compaction: a wave's survivors by ballot, the waves' counts through LDS
        const unsigned long long m = __ballot(v != RF_NONE);
        if (lane == 0) s_wc[wv] = (uint32_t)__popcll(m);
        __syncthreads();
        const uint32_t c0 = s_wc[0], c1 = s_wc[1], c2 = s_wc[2], c3 = s_wc[3];
        const uint32_t U = (c0 + c1) + (c2 + c3);
        if (v != RF_NONE) cid[(wv > 0 ? c0 : 0u) + (wv > 1 ? c1 : 0u) + (wv > 2 ? c2 : 0u) + (uint32_t)__popcll(m & ((1ull << lane) - 1))] = v << 1;
        __syncthreads();
        if (!U) return 0;  // (block-uniform)
        // (5) the keys: wave wv takes candidates 4 R t + 4 c + wv, c < R at a time
        if constexpr (D > 0) {
            constexpr int NV = RowVec<D>::NV;
            for (uint32_t i0 = wv; i0 < U; i0 += 4 * R) {
                float4 x[R][NV];
#pragma unroll
                for (int c = 0; c < R; c++) {
                    const uint32_t i = i0 + 4 * c < U ? i0 + 4 * c : U - 1;  // (a slot past the list loads the last row again: straight-line loads)
                    load_row<D>(X + (size_t)((uint32_t)__builtin_amdgcn_readfirstlane((int)cid[i]) >> 1) * D, lane, x[c]);
                }
#pragma unroll
                for (int c = 0; c < R; c++) {
                    const uint64_t key = refine_key<D, KIND>(x[c], nullptr, q, qreg, qq, d, lane, metric, param);
                    if (lane == 0 && i0 + 4 * c < U) ckey[i0 + 4 * c] = key;
                }
            }
        } else {
            for (uint32_t i = wv; i < U; i += 4) {
                const uint64_t key = refine_key<0, KIND>(nullptr, X + (size_t)(cid[i] >> 1) * d, q, nullptr, qq, d, lane, metric, param);
                if (lane == 0) ckey[i] = key;
            }
        }
        __syncthreads();
        // (6) places in the union: beam entry tid and candidate tid each count what lies below them
        const bool hb = tid < nb, hc = tid < U;
        const uint64_t kb = hb ? s_key[tid] : 0, kc = hc ? ckey[tid] : 0;
        const uint32_t ib = hb ? s_id[tid] : 0, ic = hc ? cid[tid] : 0;
        uint32_t pb = tid, pc = 0;
        // (F1) candidate tid is offered to R if its bit in the allowed-AND-live bitmap is set, and passes unless R holds it now
        const bool hr = FILT && tid < nr;
        uint64_t kr = 0;
        uint32_t ir = 0, pr = tid, pcr = 0, n_pass = 0;
        bool pass = false;
        if constexpr (FILT) {
            if (hr) { kr = r_key[tid]; ir = r_id[tid]; }
            const uint32_t rc = ic >> 1;
            const bool offered = hc && ((allow[rc >> 5] >> (rc & 31)) & 1u);
            n_off += (uint32_t)__popcll(__ballot(offered));
            bool in_r = false;
            for (uint32_t j = 0; j < nr; j++) in_r = in_r || r_id[j] == rc;  // (broadcast reads)
            pass = offered && !in_r;
            if (pass) cid[tid] = ic | 1u;  // (a candidate's flag bit is free until it joins the beam, which it does as ic)
            __syncthreads();
        }
        for (uint32_t j = 0; j < U; j++) {  // (every lane reads the same words: LDS broadcasts)
            const uint64_t kj = ckey[j];
            const uint32_t wj = cid[j], rj = wj >> 1;
            pb += gs_less(kj, rj, kb, ib >> 1) ? 1u : 0u;
            const uint32_t below_c = gs_less(kj, rj, kc, ic >> 1) ? 1u : 0u;
            pc += below_c;
            if constexpr (FILT) {  // (F2) the same count among the passing candidates, for R's entries and for the candidate
                const uint32_t fj = wj & 1u;
                n_pass += fj;
                pr += gs_less(kj, rj, kr, ir) ? fj : 0u;
                pcr += below_c & fj;
            }
        }
        if constexpr (FILT) {
            if (pass) {  // the entries of R below the candidate
                uint32_t lo = 0, hi = nr;
                while (lo < hi) {
                    const uint32_t mid = (lo + hi) >> 1;
                    if (gs_less(r_key[mid], r_id[mid], kc, ic >> 1)) lo = mid + 1;
                    else hi = mid;
                }
                pcr += lo;
            }
        }
        if (hc) {  // the beam entries below the candidate: the first of the sorted beam that is not
            uint32_t lo = 0, hi = nb;
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if (gs_less(s_key[mid], s_id[mid] >> 1, kc, ic >> 1)) lo = mid + 1;
                else hi = mid;
            }
            pc += lo;
        }
        __syncthreads();  // (the beam is read: its slots are written next)
        if (hb && pb < beam) { s_key[pb] = kb; s_id[pb] = ib; }
        if (hc && pc < beam) { s_key[pc] = kc; s_id[pc] = ic; }
        nb = nb + U < beam ? nb + U : beam;
        if constexpr (FILT) {  // (F3) what lands below top_k is written (the barrier above closed the reads of R too)
            if (hr && pr < top_k) { r_key[pr] = kr; r_id[pr] = ir; }
            if (pass && pcr < top_k) { r_key[pcr] = kc; r_id[pcr] = ic >> 1; }
            nr = nr + n_pass < top_k ? nr + n_pass : top_k;
        }
        __syncthreads();
        return U;
    };

    // ---- the seeds: S(q) = the live stored rows they name, each once (STEER: the allowed live rows)
    {
        uint32_t v = RF_NONE;
        if (tid < n_seed) {
            const uint64_t r = seeds[b * n_seed + tid] - id_base;  // (an id below id_base wraps past every row number)
            if constexpr (STEER) {
                if (r < n_rows && ((allow[r >> 5] >> (r & 31)) & 1u)) v = (uint32_t)r;
            } else {
                if (r < n_rows && ((bits[r >> 5] >> (r & 31)) & 1u)) v = (uint32_t)r;
            }
        }
        s_raw[tid] = v;
        __syncthreads();
        if (v != RF_NONE)
            for (uint32_t j = 0; j < tid; j++)
                if (s_raw[j] == v) { v = RF_NONE; break; }
        n_seeds = absorb(v);
        n_keyed = n_seeds;
    }
    // ---- the iterations
    for (; n_iter <= n_rows; n_iter++) {  // (a row is expanded at most once, DESIGN.md s24: the bound is never the reason the loop ends)
        // (1) P: the first `width` unexpanded entries of the sorted beam
        const bool un = tid < nb && !(s_id[tid] & 1u);
        const unsigned long long m = __ballot(un);
        if (lane == 0) s_wc[wv] = (uint32_t)__popcll(m);
        __syncthreads();
        const uint32_t c0 = s_wc[0], c1 = s_wc[1], c2 = s_wc[2], c3 = s_wc[3];
        const uint32_t left = (c0 + c1) + (c2 + c3);
        if (!left) break;  // (block-uniform)
        if (max_iters && n_iter == max_iters) { capped = 1; break; }
        const uint32_t rank = (wv > 0 ? c0 : 0u) + (wv > 1 ? c1 : 0u) + (wv > 2 ? c2 : 0u) + (uint32_t)__popcll(m & ((1ull << lane) - 1));
        if (un && rank < width) {
            s_par[rank] = s_id[tid] >> 1;
            s_id[tid] |= 1u;
        }
        const uint32_t np = left < width ? left : width;
        __syncthreads();
        n_exp += np;
        // (2) the parents' lines: thread e holds entry e % g_k of parent e / g_k (np * g_k <= 256: the host's check)
        uint32_t v = RF_NONE, br = RF_NONE;  // (STEER: v a direct row, br a bridge -- live, not allowed, hops == 2)
        const uint32_t pe = tid / g_k;
        if (pe < np) {
            const uint32_t p = s_par[pe];
            if (p < g_rows) v = tab[(size_t)p * g_k + (tid - pe * g_k)];  // (a row appended since the attach has an empty line)
            if constexpr (STEER) {
                if (v != RF_NONE && !((allow[v >> 5] >> (v & 31)) & 1u)) {
                    if (hops == 2 && ((bits[v >> 5] >> (v & 31)) & 1u)) br = v;  // (a removed row is skipped, not hopped through)
                    v = RF_NONE;
                }
            } else {
                if (v != RF_NONE && !((bits[v >> 5] >> (v & 31)) & 1u)) v = RF_NONE;  // (removed since the attach)
            }
        }
        s_raw[tid] = v;
        if constexpr (STEER) s_br[tid] = br;
        __syncthreads();
        // (3) once each, and not in the beam
        if (v != RF_NONE) {
            const uint32_t before = pe * g_k;  // (the entries of earlier parents' lines)
            for (uint32_t j = 0; j < before; j++)
                if (s_raw[j] == v) { v = RF_NONE; break; }
        }
        if constexpr (STEER) {
            if (br != RF_NONE) {  // H holds a bridge once: at its first (parent, entry)
                const uint32_t before = pe * g_k;
                for (uint32_t j = 0; j < before; j++)
                    if (s_br[j] == br) { br = RF_NONE; break; }
            }
        }
        {
            bool in_beam = false;
            for (uint32_t j = 0; j < nb; j++) in_beam = in_beam || (s_id[j] >> 1) == v;  // (broadcast reads; v = RF_NONE matches no row below 2^31)
            if (in_beam) v = RF_NONE;
        }
        if constexpr (STEER) {
            uint32_t nd = 0;  // the direct rows of cand (block-uniform)
            if (hops == 2) {
                // (S1) the direct rows to the front of s_raw, the bridges H to the front of s_br, both in (parent, entry) order
                const unsigned long long mv = __ballot(v != RF_NONE), mh = __ballot(br != RF_NONE);
                if (lane == 0) { s_wx[wv] = (uint32_t)__popcll(mv); s_wx[4 + wv] = (uint32_t)__popcll(mh); }
                __syncthreads();  // (closes step (3)'s reads of s_raw, s_br and the beam's id words)
                const uint32_t d0 = s_wx[0], d1 = s_wx[1], d2 = s_wx[2], d3 = s_wx[3], h0 = s_wx[4], h1 = s_wx[5], h2 = s_wx[6], h3 = s_wx[7];
                const unsigned long long below = (1ull << lane) - 1;
                nd = (d0 + d1) + (d2 + d3);
                const uint32_t nh = (h0 + h1) + (h2 + h3);
                if (v != RF_NONE) s_raw[((wv > 0 ? d0 : 0u) + (wv > 1 ? d1 : 0u) + (wv > 2 ? d2 : 0u) + (uint32_t)__popcll(mv & below)) & (GS_SLOTS - 1)] = v;
                if (br != RF_NONE) s_br[((wv > 0 ? h0 : 0u) + (wv > 1 ? h1 : 0u) + (wv > 2 ? h2 : 0u) + (uint32_t)__popcll(mh & below)) & (GS_SLOTS - 1)] = br;
                __syncthreads();
                n_bridge += nh;
                // (S2) the second hop, in passes of up to GS_HOP_SUB sub-passes of bpp bridges each: thread tid holds entry tid % g_k of bridge
                // tid / g_k of every sub-pass.  The entries whose `allow` bit is set go, in emission order, to cid (free between two absorbs);
                // a pass takes as many leading sub-passes as fit its 256 slots (the first always does).  Then entry t of cid is dropped if an
                // earlier entry of cid, the list so far (s_raw[0, nc)) or the beam holds its row, and the survivors go behind the list, up to
                // slot 255.  Four barriers a pass.
                uint32_t nc = nd;
                const uint32_t bpp = GS_SLOTS / g_k, e = tid - pe * g_k;
                for (uint32_t hb = 0; hb < nh && nc < GS_SLOTS;) {  // (block-uniform)
                    uint32_t mrow[GS_HOP_SUB];
                    unsigned long long mm[GS_HOP_SUB];
#pragma unroll
                    for (int sp = 0; sp < GS_HOP_SUB; sp++) {
                        uint32_t x = RF_NONE;
                        const uint32_t h = hb + sp * bpp + pe;
                        if (pe < bpp && h < nh) {
                            const uint32_t u = s_br[h];
                            if (u < g_rows) x = tab[(size_t)u * g_k + e];  // (a bridge appended since the attach has an empty line)
                            if (x != RF_NONE && !((allow[x >> 5] >> (x & 31)) & 1u)) x = RF_NONE;
                        }
                        mrow[sp] = x;
                        mm[sp] = __ballot(x != RF_NONE);
                        if (lane == 0) s_wx[4 * sp + wv] = (uint32_t)__popcll(mm[sp]);
                    }
                    __syncthreads();
                    uint32_t tot = 0, take = 0, mine[GS_HOP_SUB];
#pragma unroll
                    for (int sp = 0; sp < GS_HOP_SUB; sp++) {
                        const uint32_t c0 = s_wx[4 * sp], c1 = s_wx[4 * sp + 1], c2 = s_wx[4 * sp + 2], c3 = s_wx[4 * sp + 3];
                        const uint32_t c = (c0 + c1) + (c2 + c3);
                        const bool in = take == (uint32_t)sp && (sp == 0 || tot + c <= GS_SLOTS);
                        mine[sp] = in ? tot + (wv > 0 ? c0 : 0u) + (wv > 1 ? c1 : 0u) + (wv > 2 ? c2 : 0u) + (uint32_t)__popcll(mm[sp] & below) : GS_SLOTS;
                        if (in) { tot += c; take++; }
                    }
#pragma unroll
                    for (int sp = 0; sp < GS_HOP_SUB; sp++)
                        if (mrow[sp] != RF_NONE && mine[sp] < GS_SLOTS) cid[mine[sp]] = mrow[sp];
                    __syncthreads();
                    uint32_t x = RF_NONE;
                    if (wv * 64 < tot) {  // (wave-uniform)
                        if (tid < tot) x = cid[tid];
                        uint32_t dup = 0;  // (no short cut: the broadcast reads of a scan are independent and stay in flight together)
                        const uint32_t lim = tot < wv * 64 + 63 ? tot : wv * 64 + 63;  // (the entries before the wave's last lane)
#pragma unroll 8
                        for (uint32_t j = 0; j < lim; j++) dup |= (uint32_t)(j < tid) & (uint32_t)(cid[j] == x);
#pragma unroll 8
                        for (uint32_t j = 0; j < nc; j++) dup |= (uint32_t)(s_raw[j] == x);
#pragma unroll 8
                        for (uint32_t j = 0; j < nb; j++) dup |= (uint32_t)((s_id[j] >> 1) == x);
                        if (dup) x = RF_NONE;
                    }
                    const unsigned long long ms = __ballot(x != RF_NONE);
                    if (lane == 0) s_wx[wv] = (uint32_t)__popcll(ms);
                    __syncthreads();  // (closes the reads of cid and of the list)
                    const uint32_t s0 = s_wx[0], s1 = s_wx[1], s2 = s_wx[2], s3 = s_wx[3];
                    const uint32_t at = nc + (wv > 0 ? s0 : 0u) + (wv > 1 ? s1 : 0u) + (wv > 2 ? s2 : 0u) + (uint32_t)__popcll(ms & below);
                    if (x != RF_NONE && at < GS_SLOTS) s_raw[at] = x;  // (first emission wins; what would land at slot 256 or later is dropped)
                    const uint32_t grown = nc + ((s0 + s1) + (s2 + s3));
                    nc = grown < GS_SLOTS ? grown : GS_SLOTS;
                    hb += take * bpp;
                    __syncthreads();
                }
                v = tid < nc ? s_raw[tid] : RF_NONE;  // (absorb's compaction keeps the order)
            }
            const uint32_t U = absorb(v);
            n_keyed += U;
            if (hops != 2) nd = U;
            n_direct += nd;
            n_via += U - nd;
            n_full += U == GS_SLOTS ? 1u : 0u;
        } else {
            n_keyed += absorb(v);  // (its first barrier closes the reads of the beam's id words)
        }
    }
    // ---- the answer: the first top_k of B; under a filter, R
    const uint32_t have = FILT ? nr : nb < top_k ? nb : top_k;
    for (uint32_t i = tid; i < top_k; i += 256) {
        if constexpr (FILT) {
            out_ids[b * top_k + i] = i < have ? id_base + r_id[i] : ~0ull;
            out_keys[b * top_k + i] = i < have ? r_key[i] : ~0ull;
        } else {
            out_ids[b * top_k + i] = i < have ? id_base + (s_id[i] >> 1) : ~0ull;
            out_keys[b * top_k + i] = i < have ? s_key[i] : ~0ull;
        }
    }
    if constexpr (FILT) {
        if (lane == 0 && n_off) atomicAdd(&ctr[5], (unsigned long long)n_off);
        if (tid == 0 && have) atomicAdd(&ctr[6], (unsigned long long)have);
    }
    if constexpr (STEER) {
        if (tid == 0) {
            if (n_direct) atomicAdd(&ctr[5], (unsigned long long)n_direct);
            if (n_via) atomicAdd(&ctr[6], (unsigned long long)n_via);
            if (n_bridge) atomicAdd(&ctr[7], (unsigned long long)n_bridge);
            if (n_full) atomicAdd(&ctr[8], (unsigned long long)n_full);
            if (have) atomicAdd(&ctr[9], (unsigned long long)have);
        }
    }
    if (tid == 0) {
        out_counts[b] = have;
        if (n_seeds) atomicAdd(&ctr[0], (unsigned long long)n_seeds);
        if (n_iter) atomicAdd(&ctr[1], (unsigned long long)n_iter);
        if (n_exp) atomicAdd(&ctr[2], (unsigned long long)n_exp);
        if (n_keyed) atomicAdd(&ctr[3], (unsigned long long)n_keyed);
        if (capped) atomicAdd(&ctr[4], 1ull);
    }
}

template <int D, int KIND>
__global__ __launch_bounds__(256) void gsearch_kernel(const float *__restrict__ X, uint32_t d, uint64_t n_rows, const uint32_t *__restrict__ tab, uint64_t g_rows,
                                                      uint32_t g_k, const uint32_t *__restrict__ bits, const float *__restrict__ Q, const float *__restrict__ QQ,
                                                      const uint64_t *__restrict__ seeds, uint32_t n_seed, uint64_t id_base, uint32_t top_k, uint32_t beam,
                                                      uint32_t width, uint32_t max_iters, int metric, int param, uint64_t *__restrict__ out_ids,
                                                      uint64_t *__restrict__ out_keys, uint32_t *__restrict__ out_counts, unsigned long long *__restrict__ ctr) {
    gsearch_block<D, KIND, false>(X, d, n_rows, tab, g_rows, g_k, bits, nullptr, Q, QQ, seeds, n_seed, id_base, top_k, beam, width, max_iters, metric, param, out_ids,
                                  out_keys, out_counts, ctr);
}

// the same walk, answering from R: allow = allowed AND live (zh_launch_filter_and's bitmap), ctr[5] = offered, ctr[6] = returned
template <int D, int KIND>
__global__ __launch_bounds__(256) void gsearch_filtered_kernel(const float *__restrict__ X, uint32_t d, uint64_t n_rows, const uint32_t *__restrict__ tab,
                                                               uint64_t g_rows, uint32_t g_k, const uint32_t *__restrict__ bits, const uint32_t *__restrict__ allow,
                                                               const float *__restrict__ Q, const float *__restrict__ QQ, const uint64_t *__restrict__ seeds,
                                                               uint32_t n_seed, uint64_t id_base, uint32_t top_k, uint32_t beam, uint32_t width, uint32_t max_iters,
                                                               int metric, int param, uint64_t *__restrict__ out_ids, uint64_t *__restrict__ out_keys,
                                                               uint32_t *__restrict__ out_counts, unsigned long long *__restrict__ ctr) {
    gsearch_block<D, KIND, true>(X, d, n_rows, tab, g_rows, g_k, bits, allow, Q, QQ, seeds, n_seed, id_base, top_k, beam, width, max_iters, metric, param, out_ids,
                                 out_keys, out_counts, ctr);
}

// the steered walk (zh_search_graph_steered_batch): B holds rows of `allow` only; a disallowed live entry of a parent's line is hopped
// over (hops == 2).  ctr[5..9] = direct, via_bridge, bridges, cand_full, returned
template <int D, int KIND>
__global__ __launch_bounds__(256) void gsearch_steered_kernel(const float *__restrict__ X, uint32_t d, uint64_t n_rows, const uint32_t *__restrict__ tab,
                                                              uint64_t g_rows, uint32_t g_k, const uint32_t *__restrict__ bits, const uint32_t *__restrict__ allow,
                                                              const float *__restrict__ Q, const float *__restrict__ QQ, const uint64_t *__restrict__ seeds,
                                                              uint32_t n_seed, uint64_t id_base, uint32_t top_k, uint32_t beam, uint32_t width, uint32_t max_iters,
                                                              uint32_t hops, int metric, int param, uint64_t *__restrict__ out_ids, uint64_t *__restrict__ out_keys,
                                                              uint32_t *__restrict__ out_counts, unsigned long long *__restrict__ ctr) {
    __shared__ uint32_t s_br[GS_SLOTS], s_wx[4 * GS_HOP_SUB];  // an iteration's bridges; the waves' counts of the second-hop stage
    gsearch_block<D, KIND, false, true>(X, d, n_rows, tab, g_rows, g_k, bits, allow, Q, QQ, seeds, n_seed, id_base, top_k, beam, width, max_iters, metric, param,
                                        out_ids, out_keys, out_counts, ctr, hops, s_br, s_wx);
}

hipError_t zh_launch_gsearch(const float *dX, uint32_t d, uint64_t n_rows, const uint32_t *dTab, uint64_t g_rows, uint32_t g_k, const uint32_t *dBits,
                             const uint32_t *dAllow, const float *dQ, const float *dQQ, const uint64_t *dSeeds, uint32_t n_seed, uint32_t B, uint64_t id_base, uint32_t top_k,
                             uint32_t beam, uint32_t width, uint32_t max_iters, int metric, int param, uint64_t *dOutIds, uint64_t *dOutKeys,
                             uint32_t *dOutCounts, unsigned long long *dCtr, hipStream_t s) {
    if (!B) return hipSuccess;
    if (!g_k || g_k > ZH_REFINE_MAX_IN_K || !width || (uint64_t)width * g_k > GS_SLOTS || !n_seed || n_seed > ZH_GRAPH_MAX_SEEDS || !top_k || top_k > beam ||
        beam > ZH_GRAPH_MAX_BEAM || n_rows >= (1ull << 31))
        return hipErrorInvalidValue;
    return zh_dispatch_kind_dim(metric, d, [&](auto kind, auto dim) {
        if (dAllow)
            hipLaunchKernelGGL((gsearch_filtered_kernel<decltype(dim)::value, decltype(kind)::value>), dim3(B), dim3(256), 0, s, dX, d, n_rows, dTab, g_rows, g_k,
                               dBits, dAllow, dQ, dQQ, dSeeds, n_seed, id_base, top_k, beam, width, max_iters, metric, param, dOutIds, dOutKeys, dOutCounts, dCtr);
        else
            hipLaunchKernelGGL((gsearch_kernel<decltype(dim)::value, decltype(kind)::value>), dim3(B), dim3(256), 0, s, dX, d, n_rows, dTab, g_rows, g_k, dBits, dQ,
                               dQQ, dSeeds, n_seed, id_base, top_k, beam, width, max_iters, metric, param, dOutIds, dOutKeys, dOutCounts, dCtr);
        return hipGetLastError();
    });
}

hipError_t zh_launch_gsearch_steered(const float *dX, uint32_t d, uint64_t n_rows, const uint32_t *dTab, uint64_t g_rows, uint32_t g_k, const uint32_t *dBits,
                                     const uint32_t *dAllow, const float *dQ, const float *dQQ, const uint64_t *dSeeds, uint32_t n_seed, uint32_t B, uint64_t id_base,
                                     uint32_t top_k, uint32_t beam, uint32_t width, uint32_t max_iters, uint32_t hops, int metric, int param, uint64_t *dOutIds,
                                     uint64_t *dOutKeys, uint32_t *dOutCounts, unsigned long long *dCtr, hipStream_t s) {
    if (!B) return hipSuccess;
    if (!g_k || g_k > ZH_REFINE_MAX_IN_K || !width || (uint64_t)width * g_k > GS_SLOTS || !n_seed || n_seed > ZH_GRAPH_MAX_SEEDS || !top_k || top_k > beam ||
        beam > ZH_GRAPH_MAX_BEAM || n_rows >= (1ull << 31) || !dAllow || hops < 1 || hops > 2)
        return hipErrorInvalidValue;
    return zh_dispatch_kind_dim(metric, d, [&](auto kind, auto dim) {
        hipLaunchKernelGGL((gsearch_steered_kernel<decltype(dim)::value, decltype(kind)::value>), dim3(B), dim3(256), 0, s, dX, d, n_rows, dTab, g_rows, g_k, dBits,
                           dAllow, dQ, dQQ, dSeeds, n_seed, id_base, top_k, beam, width, max_iters, hops, metric, param, dOutIds, dOutKeys, dOutCounts, dCtr);
        return hipGetLastError();
    });
}
