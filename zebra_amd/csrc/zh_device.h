// zh_device.h -- device helpers shared by the kernel translation units (zh_search.hip, zh_approx.hip): the canonical
// butterflies and sums, key finalisers, row loads, the LDS bitonic sort and the select partition.  Moved verbatim out of
// zh_search.hip in round 4 so that the half-width scan compiles on its own.  Since then also the matrix-core vector types of
// every scan and, at the end, the pair pool's helpers (range search, forest range search, the three joins).
//
// Last, what the matrix-core scans of the exact and forest families (path 2) share.  tile_dot is their tile product -- the
// summation order zh_approx_bound(metric, d, 1) is valid for (exact_mfma_kernel alone writes it out: zh_exact.hip says why).  held_tile / held_walk are the three joins' and the two graphs' scheme, written once:
// a wave holds a 16-row tile in registers and the block walks a chunk of column tiles through two LDS buffers, one tile ahead; what becomes of a
// 16 x 16 block of sums is a sink's business -- PoolSink appends the pairs with lo <= tau to a candidate pool (the joins; with or without the
// upper-triangle rule), ListSink to the held line's own (row, lo, hi) list (the graphs).  A kernel is its geometry, a sink and one call of the walk.
// zh_mfma_dispatch is the host's one switch over the dimensions and interval kinds these scans are built for.
#pragma once
#include <type_traits>

#include "zh_internal.h"

#define WAVE 64

typedef float f32x16 __attribute__((ext_vector_type(16)));
// v_mfma_f32_16x16x32_f16's operands and result, and the 16-byte piece every fp16 tile is moved in
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------------------------------------
// small helpers
// ------------------------------------------------------------------------------------------------
// The canonical 64-lane xor-butterfly (steps 1,2,4,8,16,32; lane l adds its partner group's value).  After a step
// every lane of a 2^k group holds the same value, so the partner may be ANY lane of the partner group: steps 1,2 are
// DPP quad_perm, 4 and 8 DPP row_half_mirror / row_mirror, 16 and 32 gfx950's v_permlane16_swap / v_permlane32_swap (a
// register-to-register exchange of 16- / 32-lane rows: both operands = s gives {my row pair's first value, its second} in
// the two results, and a + b == b + a bit for bit, as is max) -- no LDS round trip (round 2 used ds_swizzle for 16 and two
// v_readlane for 32: an lgkmcnt wait per scored (row, query) pair), no ds_bpermute; bit-identical to s + __shfl_xor(s, m).
template <int CTRL>
__device__ __forceinline__ float dpp_mov(float x) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xF, 0xF, false));
}
struct OpAdd { __device__ __forceinline__ static float f(float a, float b) { return a + b; } };
struct OpMax { __device__ __forceinline__ static float f(float a, float b) { return fmaxf(a, b); } };
template <class OP>
__device__ __forceinline__ float xor16(float s) {  // every lane: OP(value of the even 16-lane row of its pair, value of the odd one)
    const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(s), __float_as_uint(s), false, false);
    return OP::f(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
template <class OP>
__device__ __forceinline__ float wave_butterfly(float s) {
    s = OP::f(s, dpp_mov<0xB1>(s));   // quad_perm [1,0,3,2]  : xor 1
    s = OP::f(s, dpp_mov<0x4E>(s));   // quad_perm [2,3,0,1]  : xor 2
    s = OP::f(s, dpp_mov<0x141>(s));  // row_half_mirror      : other quad of the 8
    s = OP::f(s, dpp_mov<0x140>(s));  // row_mirror           : other 8 of the 16
    s = xor16<OP>(s);
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(s), __float_as_uint(s), false, false);  // {lanes 0..31's value, lanes 32..63's}
    return OP::f(__uint_as_float(r[0]), __uint_as_float(r[1]));  // xor 32
}
__device__ __forceinline__ float wave_sum_canonical(float s) { return wave_butterfly<OpAdd>(s); }
__device__ __forceinline__ uint64_t f64_bits(double x) { return (uint64_t)__double_as_longlong(x); }

// simsimd cos(): cosine DISTANCE clipped at 0 with the two zero-norm cases; then distance.rs:23-25
__device__ __forceinline__ uint64_t key_cosine(float ab, float a2, float b2, int mode) {
    double c;
    if (a2 == 0.0f && b2 == 0.0f) c = 0.0;
    else if (ab == 0.0f) c = 1.0;
    else {
        double r = 1.0 - (double)ab / sqrt((double)a2 * (double)b2);
        c = r > 0.0 ? r : 0.0;
    }
    return f64_bits(mode == ZH_COSINE_PARITY ? 1.0 - c : c);
}
__device__ __forceinline__ uint64_t key_l2(float l2sq, int metric) {
    return f64_bits(metric == ZH_L2SQ ? (double)l2sq : sqrt((double)l2sq));
}

// ---- the `distances`-crate metrics (distance.rs:51-98,116-190): f32 result, key = f32 bits widened ----
enum { K_L2 = 0, K_COS = 1, K_MAX = 2, K_CANB = 3, K_BRAY = 4, K_ABS = 5, K_P3 = 6, K_P4 = 7, K_HAMM = 8, K_PP = 9 };

__host__ __device__ inline int zh_kind_of(int metric) {
    switch (metric) {
    case ZH_COSINE: return K_COS;
    case ZH_CHEBYSHEV: return K_MAX;
    case ZH_CANBERRA: return K_CANB;
    case ZH_BRAY_CURTIS: return K_BRAY;
    case ZH_MANHATTAN: return K_ABS;
    case ZH_L3: return K_P3;
    case ZH_L4: return K_P4;
    case ZH_HAMMING: return K_HAMM;
    case ZH_MINKOWSKI: case ZH_PNORM: return K_PP;
    default: return K_L2;
    }
}

// The host's one table of the canonical-row kernels' instantiations (exact_score_kernel, refine_line_kernel, nnd_line_kernel, prune_line_kernel,
// gsearch_kernel, gsearch_filtered_kernel, gsearch_steered_kernel, gext_rerank_kernel): ten kinds; d = 128 / 384 / 768 specialised for every kind,
// 256 / 512 / 1024 as well for the two simsimd kinds; any other d is the generic 0.  tests/test_gpu_dispatch_table.py walks all of it.
// -> f(kind, dim), both std::integral_constant<int, ..>, so that a generic lambda names its kernel with them.
template <int KIND, class F>
inline hipError_t zh_dispatch_dim(uint32_t d, F &f) {
    using K = std::integral_constant<int, KIND>;
    if constexpr (KIND == K_L2 || KIND == K_COS) {
        switch (d) {
        case 256: return f(K{}, std::integral_constant<int, 256>{});
        case 512: return f(K{}, std::integral_constant<int, 512>{});
        case 1024: return f(K{}, std::integral_constant<int, 1024>{});
        default: break;
        }
    }
    switch (d) {
    case 128: return f(K{}, std::integral_constant<int, 128>{});
    case 384: return f(K{}, std::integral_constant<int, 384>{});
    case 768: return f(K{}, std::integral_constant<int, 768>{});
    default: return f(K{}, std::integral_constant<int, 0>{});
    }
}
template <class F>
inline hipError_t zh_dispatch_kind_dim(int metric, uint32_t d, F f) {
    switch (zh_kind_of(metric)) {
    case K_COS: return zh_dispatch_dim<K_COS>(d, f);
    case K_MAX: return zh_dispatch_dim<K_MAX>(d, f);
    case K_CANB: return zh_dispatch_dim<K_CANB>(d, f);
    case K_BRAY: return zh_dispatch_dim<K_BRAY>(d, f);
    case K_ABS: return zh_dispatch_dim<K_ABS>(d, f);
    case K_P3: return zh_dispatch_dim<K_P3>(d, f);
    case K_P4: return zh_dispatch_dim<K_P4>(d, f);
    case K_HAMM: return zh_dispatch_dim<K_HAMM>(d, f);
    case K_PP: return zh_dispatch_dim<K_PP>(d, f);
    default: return zh_dispatch_dim<K_L2>(d, f);
    }
}

__device__ __forceinline__ float powi_f32(float a, int b) {  // compiler-rt __powisf2 (Rust f32::powi)
    const bool recip = b < 0;
    float r = 1.0f;
    for (;;) {
        if (b & 1) r *= a;
        b /= 2;
        if (b == 0) break;
        a *= a;
    }
    return recip ? 1.0f / r : r;
}

// s^(1/p), 1 <= p <= 64: fixed Newton iteration in f64 (only + * /), bit-identical to the oracle's root_p
__device__ __forceinline__ double root_p(double s, int p) {
    if (!(s > 0.0) || s == (double)INFINITY || p == 1) return s;
    if (p == 2) return sqrt(s);
    uint64_t u = (uint64_t)__double_as_longlong(s);
    int e = (int)((u >> 52) & 0x7FF) - 1023;
    int fl = e >= 0 ? e / p : -((-e + p - 1) / p);
    int rem = e - fl * p;
    double y = ldexp((1.0 + (double)rem / (double)p) * (1.0 + 1.0 / (double)p), fl);
    for (int it = 0; it < 16; it++) {
        double yp = 1.0;
        for (int i = 0; i < p - 1; i++) yp *= y;
        y = ((double)(p - 1) * y + s / yp) / (double)p;
    }
    return y;
}

// s^(1/p), p > 64: exp(ln(s) / p) from fixed f64 series (the oracle's root_big, operation for operation)
__device__ __forceinline__ double root_big(double s, double p) {
    uint64_t u = (uint64_t)__double_as_longlong(s);
    int e = (int)((u >> 52) & 0x7FF) - 1023;
    u = (u & 0x000FFFFFFFFFFFFFull) | 0x3FF0000000000000ull;
    double m = __longlong_as_double((long long)u);
    if (m > 1.4142135623730951) { m = m * 0.5; e += 1; }
    const double z = (m - 1.0) / (m + 1.0), z2 = z * z;
    double t = 0.0;
    for (int k = 25; k >= 1; k -= 2) t = t * z2 + 1.0 / (double)k;
    const double LN2 = 0.6931471805599453;
    const double x = ((double)e * LN2 + 2.0 * z * t) / p;
    const double xs = x / LN2;
    const int n = (int)(xs < 0.0 ? xs - 0.5 : xs + 0.5);
    const double r = x - (double)n * LN2;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k <= 20; k++) { term = term * r / (double)k; sum = sum + term; }
    return ldexp(sum, n);
}

// distances::vectors::minkowski's `sum.powf(1 / p)` for ANY i32 p (distance.rs:160-174; Default is power 0): the oracle's root_any
__device__ __forceinline__ double root_any(double s, int p) {
    if (s != s) return s;
    if (p == 0) return s > 1.0 ? (double)INFINITY : (s == 1.0 ? 1.0 : 0.0);
    const long long ap = p < 0 ? -(long long)p : (long long)p;
    double r;
    if (!(s > 0.0) || s == (double)INFINITY || ap == 1) r = s;
    else r = ap <= 64 ? root_p(s, (int)ap) : root_big(s, (double)ap);
    if (p > 0) return r;
    if (r == 0.0) return (double)INFINITY;
    if (r == (double)INFINITY) return 0.0;
    return 1.0 / r;
}

// sums -> DistanceUnit for every metric; s0/s1 are the canonical sums, qq the query norm (cosine)
__device__ __forceinline__ uint64_t key_of(int metric, int param, float s0, float s1, float qq) {
    float f;
    switch (metric) {
    case ZH_COSINE: return key_cosine(s0, s1, qq, param);
    case ZH_L2SQ: case ZH_L2: return key_l2(s0, metric);
    case ZH_BRAY_CURTIS: f = s0 / s1; break;
    case ZH_L3: f = (float)root_p((double)s0, 3); break;
    case ZH_L4: f = sqrtf(sqrtf(s0)); break;
    case ZH_HAMMING: return (uint64_t)s0;
    case ZH_MINKOWSKI: f = (float)root_any((double)s0, param); break;
    default: f = s0; break;  // CHEBYSHEV, CANBERRA, MANHATTAN, PNORM
    }
    return (uint64_t)__float_as_uint(f);
}

// one element of the per-lane accumulation, by kind (a = stored, q = query)
template <int KIND>
__device__ __forceinline__ void acc_elem(float a, float q, float &x0, float &x1, int power) {
    if (KIND == K_L2) { float df = a - q; x0 = __builtin_fmaf(df, df, x0); }
    else if (KIND == K_COS) { x0 = __builtin_fmaf(a, q, x0); }
    else {
        float ad = fabsf(a - q);
        if (KIND == K_MAX) x0 = fmaxf(x0, ad);
        else if (KIND == K_CANB) x0 = x0 + ad / (fabsf(a) + fabsf(q));
        else if (KIND == K_BRAY) { x0 = x0 + ad; x1 = x1 + fabsf(a + q); }
        else if (KIND == K_ABS) x0 = x0 + ad;
        else if (KIND == K_P3) x0 = x0 + ad * (ad * ad);
        else if (KIND == K_P4) { float t = ad * ad; x0 = x0 + t * t; }
        else if (KIND == K_HAMM) x0 = x0 + (float)__popc((__float_as_uint(a) ^ __float_as_uint(q)) & 0xFFu);
        else x0 = x0 + powi_f32(ad, power);
    }
}
// Four consecutive elements of a lane (one float4 of the row against one of the query) into the lane's four accumulators.
// The two simsimd kinds use gfx950's PACKED f32 instructions (v_pk_add_f32 / v_pk_fma_f32: two IEEE operations per lane and
// instruction, the only way to the f32 VALU peak): (x, y) and (z, w) are aligned register pairs of the loaded float4, every
// component is the same fused / unfused operation as the scalar form, so the sums are bit-identical -- at half the vector
// instructions (the table scan spends 13-20 % of its time on them: a build without the arithmetic, profiles/r03_ab_scan_*).
typedef float f32x2 __attribute__((ext_vector_type(2)));
template <int KIND>
__device__ __forceinline__ void acc4(const float4 &v, const float4 &q, float4 &a, float4 &e, int power) {
    if constexpr (KIND == K_L2 || KIND == K_COS) {
        const f32x2 v0 = {v.x, v.y}, v1 = {v.z, v.w}, q0 = {q.x, q.y}, q1 = {q.z, q.w};
        f32x2 a0 = {a.x, a.y}, a1 = {a.z, a.w};
        if constexpr (KIND == K_L2) {
            const f32x2 d0 = v0 - q0, d1 = v1 - q1;
            a0 = __builtin_elementwise_fma(d0, d0, a0);
            a1 = __builtin_elementwise_fma(d1, d1, a1);
        } else {
            a0 = __builtin_elementwise_fma(v0, q0, a0);
            a1 = __builtin_elementwise_fma(v1, q1, a1);
        }
        a.x = a0.x; a.y = a0.y; a.z = a1.x; a.w = a1.y;
    } else {
        acc_elem<KIND>(v.x, q.x, a.x, e.x, power);
        acc_elem<KIND>(v.y, q.y, a.y, e.y, power);
        acc_elem<KIND>(v.z, q.z, a.z, e.z, power);
        acc_elem<KIND>(v.w, q.w, a.w, e.w, power);
    }
}
// c += v * v, component-wise (the stored row's squared norm for cosine), packed
__device__ __forceinline__ void sq4(const float4 &v, float4 &c) {
    const f32x2 v0 = {v.x, v.y}, v1 = {v.z, v.w};
    f32x2 c0 = {c.x, c.y}, c1 = {c.z, c.w};
    c0 = __builtin_elementwise_fma(v0, v0, c0);
    c1 = __builtin_elementwise_fma(v1, v1, c1);
    c.x = c0.x; c.y = c0.y; c.z = c1.x; c.w = c1.y;
}
template <int KIND>
__device__ __forceinline__ float wave_combine(float x, float y, float z, float w) {
    if (KIND == K_MAX) return wave_butterfly<OpMax>(fmaxf(fmaxf(x, y), fmaxf(z, w)));
    return wave_sum_canonical((x + y) + (z + w));
}


// ------------------------------------------------------------------------------------------------
// canonical row sums: one wave per row, lane-strided float4
// ------------------------------------------------------------------------------------------------
// generic (runtime d, any d): element e handled by lane (e mod 256)/4, component e mod 4
template <int KIND>
__device__ __forceinline__ void lane_sums_generic(const float *__restrict__ a, const float *__restrict__ q,
                                                  uint32_t d, uint32_t lane, int power, float &o_s0, float &o_s1) {
    float x0[4] = {0, 0, 0, 0}, x1[4] = {0, 0, 0, 0};
    for (uint32_t base = 0; base < d; base += 256) {
#pragma unroll
        for (int t = 0; t < 4; t++) {
            uint32_t e = base + 4 * lane + t;
            if (e < d) {
                float av = a[e];
                acc_elem<KIND>(av, q[e], x0[t], x1[t], power);
                if (KIND == K_COS) x1[t] = __builtin_fmaf(av, av, x1[t]);
            }
        }
    }
    o_s0 = wave_combine<KIND>(x0[0], x0[1], x0[2], x0[3]);
    o_s1 = (KIND == K_COS || KIND == K_BRAY) ? wave_combine<K_L2>(x1[0], x1[1], x1[2], x1[3]) : 0.0f;
}


template <int D>
struct RowVec {
    static constexpr int NJ = D / 256;            // full 1-KiB pieces
    static constexpr int REM4 = (D % 256) / 4;    // lanes holding the last, partial piece
    static constexpr int NV = NJ + (REM4 ? 1 : 0);
};

template <bool NT>
__device__ __forceinline__ float4 ld16(const float4 *p) {
    if (NT) {  // streamed once: non-temporal hint (global_load_dwordx4 ... nt)
        f32x4 t = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(p));
        return make_float4(t.x, t.y, t.z, t.w);
    }
    return *p;
}
template <int D, bool NT = false>
__device__ __forceinline__ void load_row(const float *__restrict__ row, uint32_t lane, float4 *v) {
    const float4 *r4 = reinterpret_cast<const float4 *>(row);
#pragma unroll
    for (int j = 0; j < RowVec<D>::NJ; j++) v[j] = ld16<NT>(r4 + lane + 64 * j);
    if (RowVec<D>::REM4) {
        v[RowVec<D>::NJ] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (lane < (uint32_t)RowVec<D>::REM4) v[RowVec<D>::NJ] = ld16<NT>(r4 + lane + 64 * RowVec<D>::NJ);
    }
}


// one stored row (in the canonical lane layout) against one query: the canonical sums of the pair
template <int D, int KIND>
__device__ __forceinline__ void row_pair_sums(const float4 *v, const float4 *q, uint32_t lane, int power, float &s0, float &s1) {
    constexpr int NV = RowVec<D>::NV;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f), e = a;
#pragma unroll
    for (int j = 0; j < NV; j++) {
        const bool act = (j < RowVec<D>::NJ) || (lane < (uint32_t)RowVec<D>::REM4);
        if (act) acc4<KIND>(v[j], q[j], a, e, power);
    }
    s0 = wave_combine<KIND>(a.x, a.y, a.z, a.w);
    if (KIND == K_BRAY) s1 = wave_combine<K_L2>(e.x, e.y, e.z, e.w);
}

// ------------------------------------------------------------------------------------------------
// LDS bitonic sort of (key, id) ascending; n is a power of two
// ------------------------------------------------------------------------------------------------
template <typename IdT>
__device__ __forceinline__ void block_bitonic_sort(uint64_t *sk, IdT *si, uint32_t n) {
    const uint32_t tid = threadIdx.x, nt = blockDim.x;
    for (uint32_t size = 2; size <= n; size <<= 1) {
        for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (uint32_t i = tid; i < (n >> 1); i += nt) {
                uint32_t lo = ((i & ~(stride - 1)) << 1) | (i & (stride - 1));
                uint32_t hi = lo + stride;
                bool asc = (lo & size) == 0;
                uint64_t ka = sk[lo], kb = sk[hi];
                IdT ia = si[lo], ib = si[hi];
                bool gt = ka > kb || (ka == kb && ia > ib);
                if (gt == asc) { sk[lo] = kb; sk[hi] = ka; si[lo] = ib; si[hi] = ia; }
            }
        }
    }
    __syncthreads();
}

__device__ __forceinline__ uint32_t next_pow2(uint32_t x) {
    uint32_t p = 2;
    while (p < x) p <<= 1;
    return p;
}

// per visit: the `take` smallest (key, id) of the leaf (lsh.rs:317-323); take == len copies all.
// The candidates of a query are sorted again by the final kernel, so a visit's slice of the pool
// need not be ordered: select = partition.  Fast path (leaf fits the LDS buffer): histogram
// refinement of the unsigned key range, 8 bits per round, until the bucket that holds the take-th
// key is small; everything below it is emitted as is, the bucket itself is sorted by (key, id).
// Slow path (leaf longer than the buffer, or a large group of equal keys): streaming bitonic sort.
#define SEL_SMALL 512

__device__ __forceinline__ void select_slow(const ZhVisit &v, const uint32_t *__restrict__ leaf_ids,
                                            const uint64_t *__restrict__ keys, uint64_t *__restrict__ cand_keys,
                                            uint32_t *__restrict__ cand_ids, uint64_t *sk, uint32_t *si, uint32_t cap) {
    const uint32_t tid = threadIdx.x;
    uint32_t have = 0, pos = 0;
    while (pos < v.len) {
        uint32_t m = cap - have;
        if (m > v.len - pos) m = v.len - pos;
        for (uint32_t i = tid; i < m; i += 256) {
            sk[have + i] = keys[v.row_off + pos + i];
            si[have + i] = leaf_ids[(size_t)v.leaf_off + pos + i];
        }
        uint32_t total = have + m, np2 = next_pow2(total);
        for (uint32_t i = total + tid; i < np2; i += 256) { sk[i] = ~0ull; si[i] = ~0u; }
        block_bitonic_sort<uint32_t>(sk, si, np2);
        have = total < v.take ? total : v.take;
        pos += m;
    }
    for (uint32_t i = tid; i < have; i += 256) {
        cand_keys[v.cand_off + i] = sk[i];
        cand_ids[v.cand_off + i] = si[i];
    }
}

// KEY(i): the visit's i-th key, from the LDS copy when the leaf fits it, else straight from the
// (L2 / Infinity-Cache resident) key scratch -- a few 8-B passes against the 4*d bytes the sweep read
template <bool IN_LDS>
__device__ __forceinline__ void select_fast(const ZhVisit &v, const uint32_t *__restrict__ leaf_ids,
                                            const uint64_t *__restrict__ gkeys, uint64_t *__restrict__ cand_keys,
                                            uint32_t *__restrict__ cand_ids, uint64_t *sk, uint32_t *si,
                                            uint32_t *s_u32, bool &need_slow) {
    const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    // carve-up of si[]: tk (SEL_SMALL u64) | ti (SEL_SMALL u32) | hist (256 u32) | wmin/wmax (8 u64)
    uint64_t *tk = reinterpret_cast<uint64_t *>(si);
    uint32_t *ti = si + 2 * SEL_SMALL;
    uint32_t *hist = si + 3 * SEL_SMALL;
    uint64_t *wred = reinterpret_cast<uint64_t *>(si + 3 * SEL_SMALL + 256);
    const uint64_t *kp = gkeys + v.row_off;
#define SEL_KEY(i) (IN_LDS ? sk[i] : kp[i])
    uint64_t kmin = ~0ull, kmax = 0;
    for (uint32_t i = tid; i < v.len; i += 256) {
        uint64_t k = kp[i];
        if (IN_LDS) sk[i] = k;
        kmin = k < kmin ? k : kmin;
        kmax = k > kmax ? k : kmax;
    }
    for (int m = 1; m < 64; m <<= 1) {
        uint64_t a = __shfl_xor(kmin, m), b = __shfl_xor(kmax, m);
        kmin = a < kmin ? a : kmin;
        kmax = b > kmax ? b : kmax;
    }
    if (lane == 0) { wred[wv] = kmin; wred[4 + wv] = kmax; }
    __syncthreads();
    uint64_t lo = wred[0], hi = wred[4];
    for (int w = 1; w < 4; w++) { lo = wred[w] < lo ? wred[w] : lo; hi = wred[4 + w] > hi ? wred[4 + w] : hi; }
    uint32_t need = v.take;   // how many to take from [lo, hi]; every key < lo is already taken
    uint32_t inb = v.len;     // keys inside [lo, hi]
    while (inb > SEL_SMALL && inb != need) {
        uint64_t range = hi - lo;
        if (range == 0) break;  // > SEL_SMALL equal keys: slow path
        int sh = 64 - __clzll((long long)range) - 8;
        if (sh < 0) sh = 0;
        __syncthreads();
        hist[tid] = 0;
        __syncthreads();
        for (uint32_t i = tid; i < v.len; i += 256) {
            uint64_t k = SEL_KEY(i);
            if (k >= lo && k <= hi) atomicAdd(&hist[(uint32_t)((k - lo) >> sh)], 1u);
        }
        __syncthreads();
        if (wv == 0) {  // find the bucket holding the need-th key
            uint32_t h0 = hist[4 * lane], h1 = hist[4 * lane + 1], h2 = hist[4 * lane + 2], h3 = hist[4 * lane + 3];
            uint32_t ssum = h0 + h1 + h2 + h3, inc = ssum;
            for (int m = 1; m < 64; m <<= 1) {
                uint32_t t = __shfl_up(inc, m);
                if ((int)lane >= m) inc += t;
            }
            uint32_t exc = inc - ssum;
            bool mine = exc < need && need <= inc;
            if (mine) {
                uint32_t c = exc, j = 4 * lane, hb = h0;
                if (need > c + h0) { c += h0; j++; hb = h1;
                    if (need > c + h1) { c += h1; j++; hb = h2;
                        if (need > c + h2) { c += h2; j++; hb = h3; } } }
                s_u32[0] = j; s_u32[1] = c; s_u32[2] = hb;
            }
        }
        __syncthreads();
        uint32_t j = s_u32[0], before = s_u32[1];
        inb = s_u32[2];
        need -= before;
        uint64_t nlo = lo + ((uint64_t)j << sh);
        uint64_t nhi = nlo + ((1ull << sh) - 1);
        if (nhi < nlo) nhi = hi;
        lo = nlo;
        hi = nhi < hi ? nhi : hi;
    }
    if (inb > SEL_SMALL && inb != need) { need_slow = true; return; }
    const bool take_all_bucket = (inb == need);
    // emit: keys < lo (and the whole bucket when it is taken whole) straight to the pool; otherwise the
    // bucket's members go to the small sort buffer
    __syncthreads();
    if (tid == 0) { s_u32[3] = 0; s_u32[4] = 0; }
    __syncthreads();
    for (uint32_t i = tid; i < v.len; i += 256) {
        uint64_t k = SEL_KEY(i);
        bool below = k < lo || (take_all_bucket && k <= hi);
        bool inside = !take_all_bucket && k >= lo && k <= hi;
        if (below) {
            uint32_t o = atomicAdd(&s_u32[3], 1u);
            cand_keys[v.cand_off + o] = k;
            cand_ids[v.cand_off + o] = leaf_ids[(size_t)v.leaf_off + i];
        } else if (inside) {
            uint32_t o = atomicAdd(&s_u32[4], 1u);
            if (o < SEL_SMALL) { tk[o] = k; ti[o] = leaf_ids[(size_t)v.leaf_off + i]; }
        }
    }
    __syncthreads();
    if (!take_all_bucket && need > 0) {
        uint32_t nb = s_u32[4] < SEL_SMALL ? s_u32[4] : SEL_SMALL, base = s_u32[3];
        uint32_t np2 = next_pow2(nb);
        for (uint32_t i = nb + tid; i < np2; i += 256) { tk[i] = ~0ull; ti[i] = ~0u; }
        block_bitonic_sort<uint32_t>(tk, ti, np2);
        for (uint32_t i = tid; i < need && i < nb; i += 256) {
            cand_keys[v.cand_off + base + i] = tk[i];
            cand_ids[v.cand_off + base + i] = ti[i];
        }
    }
#undef SEL_KEY
}


__device__ __forceinline__ uint32_t f32_sortable(float x) {
    const uint32_t u = __float_as_uint(x);
    return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}

// ---- the half-width scans' interval around a key (moved verbatim out of zh_approx.hip; zh_exact.hip uses it too) ----
// The L2 family's interval is V -+ E: V from the pair's sums, E from the norms.  Both as functions of their own, because the fused sweep's pre-test
// (fused_pretest) evaluates V the same way and E at an upper bound of nx: every operation of l2_E is non-decreasing in nx >= 0 (all factors are
// non-negative) and so is its rounded result -- E(nx_max) >= E(nx) in f32, whatever the roundings.
__device__ __forceinline__ float l2_V(float s, float a2, const float4 qm) {
    const float sh = s * qm.x, sum = a2 + qm.y;
    return sum - 2.0f * sh;
}
__device__ __forceinline__ float l2_E(float nx, const float4 qm, float Kc, float rho, float rho_n) {
    const float nn = nx + qm.z;
    // |s / sigma - x.q| <= |x| dq + |x - x'| (|q| + dq), |x - x'| <= rho |x| (rho = 0: the scan multiplied the f32 row)
    return Kc * nn * nn + 2.02f * nx * (qm.w + rho * (qm.z + qm.w)) + 2.2f * rho_n * nx * nx;
}
// the interval of one (row, query) pair from its sums: sortable lo | sortable hi << 32; (0, all ones) = nothing certain
template <int KINDA>
__device__ __forceinline__ uint64_t approx_interval(float s, float a2, const float4 qm, float Kc, float rho, float rho_n) {
    uint32_t lo_s = 0u, hi_s = 0xFFFFFFFFu;
    const float sh = s * qm.x;
    if (KINDA == 0) {
        // rho_n != 0: a2 is the ROUNDED row's |x'|^2 (sweep128h_kernel): |x| <= |x'| (1 + 2 rho_n), ||x'|^2 - |x|^2| <= 2.2 rho_n |x'|^2
        const float nx = sqrtf(a2) * (1.0f + 1e-5f) * (1.0f + 2.0f * rho_n), nn = nx + qm.z, sum = a2 + qm.y;
        const float V = l2_V(s, a2, qm);
        const float E = l2_E(nx, qm, Kc, rho, rho_n);
        if ((V - V == 0.f) && (E - E == 0.f) && nn > 1e-12f && sum < 1e37f) { lo_s = f32_sortable(V - E); hi_s = f32_sortable(V + E); }
    } else {
        const float nx = sqrtf(a2), nq = sqrtf(qm.y);
        if (nx > 1e-12f && nq > 1e-12f && (sh - sh == 0.f) && (nx - nx == 0.f) && (nq - nq == 0.f)) {
            float r = 1.0f - sh / (nx * nq);
            r = r > 0.f ? r : 0.f;
            const float dqr = qm.w / nq;
            const float e = Kc + 1.01f * (dqr + rho * (1.0f + dqr) + rho_n);
            float v = r;
            bool ok = true;
            if (KINDA == 2) {  // ZH_COSINE_PARITY keys compare as the bits of 1 - distance: as pf_value<2>
                const float key = 1.0f - r;
                ok = fabsf(key) > e;
                v = key > 0.f ? key : 2.0f - key;
            }
            if (ok && (v - v == 0.f) && (e - e == 0.f)) { lo_s = f32_sortable(v - e); hi_s = f32_sortable(v + e); }
        }
    }
    return ((uint64_t)hi_s << 32) | lo_s;
}

// A STORED row of the fp16 copy as approx_interval's query (the joins and the graphs: join_prep_kernel, fknn_gather_kernel): rm = the row's rowMeta
// {f32 |x|^2, 1 / sigma}, rho the copy's -> {1 / sigma, |x|^2, nq >= |x|, dq >= |x - x'|}, x' the copy's row: l2_E's comment gives |x - x'| <= rho |x|
// for every usable row of the copy, so dq = rho * nq rounded up (two roundings of 2^-24 each, under the factor's 2^-21).  The tests are
// qhalf_kernel's: a scale outside 2^-104 .. 2^76 (an exponent outside -90 .. 90), a row that is not usable or a norm that is no finite number
// leaves all four NaN -- nothing certain, every pair of the row a candidate.
__device__ __forceinline__ float4 row_as_query(const float2 rm, float rho) {
    float4 o = make_float4(NAN, NAN, NAN, NAN);
    if (rm.y >= 4.930380657631324e-32f && rm.y <= 7.555786372591432e+22f && (rm.x - rm.x == 0.f)) {  // 2^-104, 2^76
        const float nq = sqrtf(rm.x) * (1.0f + 1e-5f);
        o = make_float4(rm.y, rm.x, nq, (rho * nq) * 1.0000005f);
    }
    return o;
}

// ---- the leaf-major sweeps' view of a batch: flat rows = the rows of group 0, then group 1, ... (moved out of zh_search.hip) ----
// lane i of a sweep wave -> (group, stored row, position in the group) of flat row r0 + i.  With the wave-start table the
// search is confined to the <= 64 groups the wave's 64 rows can span (every group has at least one row), and skipped when
// the whole wave lies in one group (the common case with leaves of thousands of rows).
__device__ __forceinline__ void resolve_flat_rows(uint64_t r0, uint32_t cnt, uint32_t lane, const ZhGroup *__restrict__ groups,
                                                  const uint64_t *__restrict__ groupRowOff, uint64_t n_groups,
                                                  const uint32_t *__restrict__ waveGroup, const uint32_t *__restrict__ leaf_ids,
                                                  uint32_t &my_g, uint32_t &my_id, uint32_t &my_within,
                                                  uint32_t *my_leaf_off = nullptr, uint32_t *my_len = nullptr) {
    const uint64_t r = r0 + (lane < cnt ? lane : cnt - 1);
    uint64_t lo = 0, hi = n_groups;  // last group with row offset <= r
    if (waveGroup) {
        lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)waveGroup[r0 >> 6]);
        hi = lo + 64 < n_groups ? lo + 64 : n_groups;
        if (lo + 1 >= n_groups || groupRowOff[lo + 1] > r0 + cnt - 1) hi = lo + 1;  // wave-uniform: one group
    }
    while (hi - lo > 1) {
        uint64_t mid = (lo + hi) >> 1;
        if (groupRowOff[mid] <= r) lo = mid; else hi = mid;
    }
    my_g = (uint32_t)lo;
    my_within = (uint32_t)(r - groupRowOff[lo]);
    const uint32_t lo_off = groups[lo].leaf_off;
    if (my_leaf_off) *my_leaf_off = lo_off;
    if (my_len) *my_len = groups[lo].len;
    my_id = leaf_ids ? leaf_ids[(size_t)lo_off + my_within] : lo_off + my_within;
}

// ------------------------------------------------------------------------------------------------
// the pair pool: what range search, forest range search and the three joins share.  A hit is (left << 32 | right, key), appended to ONE pool per
// call or internal batch and counted whether or not the pool still has room, so the total stays exact when the caller's capacity is too small.
// ------------------------------------------------------------------------------------------------
// The lanes of `m` (a ballot) get consecutive pool slots: one atomic for the WAVE, taken by lane 0 (every lane of the wave is active at the call), not
// one per hit.  The counter runs on past the pool: the caller stores only where slot < cap, and *ctr is the exact count afterwards.
__device__ __forceinline__ unsigned long long wave_slots(unsigned long long *__restrict__ ctr, uint64_t m, uint32_t lane) {
    unsigned long long base = 0;
    if (lane == 0) base = atomicAdd(ctr, (unsigned long long)__popcll(m));
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)base);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(base >> 32));
    return (((unsigned long long)hi << 32) | lo) + (unsigned long long)__popcll(m & ((1ull << lane) - 1ull));
}

// the radix sorts' width of a field (host side): bits that hold 0 .. values - 1
static inline int field_bits(uint64_t values) {
    int b = 1;
    while (b < 32 && (1ull << b) < values) b++;
    return b;
}

// The canonical sums of STORED row `row` of table XB against QUERY row `qrow` of table XA, both f32 (the survivors kernels: one wave, every lane
// active).  s0 / s1 are key_of's sums: for the cosine s1 is the stored row's squared norm and, where QQ asks for it, qq the query row's -- both
// qnorm_kernel's canonical sum.  XA and XB may be one table: both are only read.
template <int D, int KIND, bool QQ>
__device__ __forceinline__ void table_pair_sums(const float *__restrict__ XB, uint32_t row, const float *__restrict__ XA, uint32_t qrow, uint32_t lane,
                                                int param, float &s0, float &s1, float &qq) {
    constexpr int NV = RowVec<D>::NV;
    float4 v[NV], q[NV];
    load_row<D>(XB + (size_t)row * D, lane, v);
    load_row<D>(XA + (size_t)qrow * D, lane, q);
    row_pair_sums<D, KIND>(v, q, lane, param, s0, s1);
    if (KIND == K_COS) {
        float4 c = make_float4(0.f, 0.f, 0.f, 0.f), cq = c;
#pragma unroll
        for (int jj = 0; jj < NV; jj++) {
            const bool act = (jj < RowVec<D>::NJ) || (lane < (uint32_t)RowVec<D>::REM4);
            if (act) {
                sq4(v[jj], c);
                if (QQ) sq4(q[jj], cq);
            }
        }
        s1 = wave_sum_canonical((c.x + c.y) + (c.z + c.w));
        if (QQ) qq = wave_sum_canonical((cq.x + cq.y) + (cq.z + cq.w));
    }
}

// the forest join's first-tree rule: tree t owns the pair (a, b) when no earlier tree holds both rows in one leaf (leaf_of: zh_fjoin.hip)
__device__ __forceinline__ bool fjoin_owned(const uint32_t *__restrict__ leaf_of, uint32_t T, uint32_t t, uint32_t a, uint32_t b) {
    const uint32_t *la = leaf_of + (size_t)a * T, *lb = leaf_of + (size_t)b * T;
    for (uint32_t u = 0; u < t; u++) {
        const uint32_t x = la[u];
        if (x != 0xFFFFFFFFu && x == lb[u]) return false;
    }
    return true;
}

// one candidate per lane of `pass` into a pool: slots by wave_slots (every lane of the wave is active at the call), stored while the pool has room
__device__ __forceinline__ void pool_push(unsigned long long *__restrict__ ctr, uint64_t *__restrict__ cand, uint64_t cap, bool pass, uint64_t v,
                                          uint32_t lane) {
    const uint64_t m = __ballot(pass);
    if (m) {  // (wave-uniform)
        const unsigned long long slot = wave_slots(ctr, m, lane);  // the counter runs on past the pool
        if (pass && slot < cap) cand[slot] = v;
    }
}

// the last i < n with at(i) <= x (at ascending, at(0) <= x): a block's entry in a table of first blocks
template <class AT>
__device__ __forceinline__ uint32_t last_le(uint32_t n, uint32_t x, AT at) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (at(mid) <= x) lo = mid; else hi = mid;
    }
    return lo;
}

// ------------------------------------------------------------------------------------------------
// the matrix-core family scans (path 2 of the exact and forest families)
// ------------------------------------------------------------------------------------------------
// A tile is 16 rows of an fp16 copy in the MFMA operand's own order: D / 32 steps of 64 pieces of 16 bytes, lane l's piece of step st at 64 st + l.
// NT: the tile is streamed once (exact and range search)
template <int D, bool NT = false>
__device__ __forceinline__ void tile_load(f16x8 (&A)[D / 32], const u32x4 *__restrict__ X, size_t tile, uint32_t lane) {
    const u32x4 *tp = X + tile * (D * 2) + lane;
#pragma unroll
    for (int st = 0; st < D / 32; st++) {
        if constexpr (NT) A[st] = __builtin_bit_cast(f16x8, __builtin_nontemporal_load(tp + 64 * st));
        else A[st] = __builtin_bit_cast(f16x8, tp[64 * st]);
    }
}

// The 16 x 16 block of dot products of tile A (registers) and a tile whose piece of step st lies at bp[STRIDE * st]: 64 for a tile in operand order
// (LDS), 4 for a query's halves (qhalf layout 1).  Four accumulators, step st into acc[st & 3], then (acc0 + acc1) + (acc2 + acc3): the summation
// order of scan_mfma_kernel and the ONLY one zh_approx_bound(metric, d, 1) bounds -- every interval of the family scans rests on this order.
// [i] sums one of the lane's four elements where it is used, all() the four at once: the same additions in the same order.  Which of the two a
// scan takes decides only how the compiler schedules it: with all() the scans that read the other operand from global memory (range, forest range)
// need fewer registers, reach a higher occupancy and wait for every load before its product -- range search at d = 768 lost 20 % that way,
// measured.  exact_mfma_kernel (zh_exact.hip) keeps its own copy of these lines: at d = 1024 either form cost its filtered scan 27 %.
struct TileSums {
    f32x4 acc[4];
    __device__ __forceinline__ float operator[](int i) const { return (acc[0][i] + acc[1][i]) + (acc[2][i] + acc[3][i]); }
    __device__ __forceinline__ f32x4 all() const { return (acc[0] + acc[1]) + (acc[2] + acc[3]); }
};
template <int NS, int STRIDE>
__device__ __forceinline__ TileSums tile_dot(const f16x8 (&A)[NS], const u32x4 *bp) {
    TileSums t = {{{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}}};
#pragma unroll
    for (int st = 0; st < NS; st++)
        t.acc[st & 3] = __builtin_amdgcn_mfma_f32_16x16x32_f16(A[st], __builtin_bit_cast(f16x8, bp[STRIDE * st]), t.acc[st & 3], 0, 0, 0);
    return t;
}

// The held-tile walk (the three joins and the two graphs).  A block's four waves hold one tile each in registers -- a wave without one (`active`
// false, wave-uniform) holds zeros, still moves tiles and meets every barrier -- and walk the column tiles [Jb, Je) of a table (CA: the tiles, crow:
// a row-or-masked word per position, cqm: approx_interval's view of the row as a query) through two LDS buffers of 32 d bytes: tile J + 1, its crow
// and its cqm are fetched while tile J is multiplied, one barrier per tile.  LDS holds a tile as global memory does, so each of ds_read_b128's four
// 16-lane groups reads 16 distinct 16-byte slots: no conflict, no padding.  TI: the type tile numbers and positions are computed in.
template <int D>
__device__ __forceinline__ void held_tile(f16x8 (&A)[D / 32], const u32x4 *__restrict__ X, size_t tile, bool active, uint32_t lane) {
    if (active) tile_load<D>(A, X, tile, lane);
    else {
#pragma unroll
        for (int st = 0; st < D / 32; st++) A[st] = f16x8{0, 0, 0, 0, 0, 0, 0, 0};
    }
}
// sink.wants(J): does this wave multiply tile J (wave-uniform); sink(J, t, cb, qb): lane l's four sums t[i] = held row 4 (l / 16) + i against column
// row l % 16 of tile J, whose crow and cqm are cb and qb
template <int D, typename TI, class SINK>
__device__ __forceinline__ void held_walk(const f16x8 (&A)[D / 32], bool active, const u32x4 *__restrict__ CA, const uint32_t *__restrict__ crow,
                                          const float4 *__restrict__ cqm, TI Jb, TI Je, const SINK &sink) {
    constexpr int NS = D / 32;        // MFMA steps of a tile (K = 32 each) = its KiB
    constexpr int PIECES = NS * 64;   // 16-byte pieces of a tile
    constexpr int PT = PIECES / 256;  // ... per thread of the block
    __shared__ u32x4 sB[2][PIECES];
    const uint32_t tid = threadIdx.x, lane = tid & 63, c16 = lane & 15;
    {
        const u32x4 *src = CA + (size_t)Jb * PIECES + tid;
#pragma unroll
        for (int k = 0; k < PT; k++) sB[0][k * 256 + tid] = src[k * 256];
    }
    // the column rows' row-or-masked word and qm travel one tile ahead, like the tile itself: nothing of tile J is fetched in its compute phase
    uint32_t cb_next = crow[Jb * 16 + c16];
    float4 qb_next = cqm[Jb * 16 + c16];
    __syncthreads();
    for (TI J = Jb; J < Je; J++) {
        const uint32_t cur = (uint32_t)(J - Jb) & 1u;
        const bool more = J + 1 < Je;  // (block-uniform)
        const uint32_t cb = cb_next;
        const float4 qb = qb_next;
        u32x4 pf[PT];
        if (more) {
            const u32x4 *src = CA + (size_t)(J + 1) * PIECES + tid;
#pragma unroll
            for (int k = 0; k < PT; k++) pf[k] = src[k * 256];
            cb_next = crow[(J + 1) * 16 + c16];
            qb_next = cqm[(J + 1) * 16 + c16];
        }
        if (active && sink.wants(J)) sink(J, tile_dot<NS, 64>(A, &sB[cur][lane]).all(), cb, qb);  // (wave-uniform)
        if (more) {
#pragma unroll
            for (int k = 0; k < PT; k++) sB[cur ^ 1][k * 256 + tid] = pf[k];
        }
        __syncthreads();  // buffer cur ^ 1 was last read in the step before, which every wave left through this barrier
    }
}

// The pool sink (the joins): a pair with lo <= tau goes to the candidate pool, left << 32 | right; a masked row on either side is no pair.  UPPER
// (one table against itself): only tiles on or above the wave's diagonal, in the diagonal tile only held row 4 h + i before column row c16, and the
// pair as min << 32 | max (positions are not ids under a row order); else the full rectangle, held << 32 | column.
template <int KINDA, bool UPPER, typename TI>
struct PoolSink {
    uint32_t lane;
    TI I;  // the wave's held tile
    uint32_t tq;
    float Kc, rho;
    uint64_t *__restrict__ cand;
    uint64_t cap;
    unsigned long long *__restrict__ ctr;
    uint32_t id[4];  // this lane's held rows 4 h + i: the row-or-masked word and rowMeta
    float2 meta[4];
    __device__ __forceinline__ void hold(bool active, const uint32_t *__restrict__ rows, const float2 *__restrict__ rmeta) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            id[i] = 0xFFFFFFFFu;
            meta[i] = make_float2(0.f, 0.f);
            if (active) {
                const TI p = I * 16 + 4 * (lane >> 4) + i;
                id[i] = rows[p];
                if (id[i] != 0xFFFFFFFFu) meta[i] = rmeta[p];
            }
        }
    }
    __device__ __forceinline__ bool wants(TI J) const { return !UPPER || J >= I; }
    __device__ __forceinline__ void operator()(TI J, const f32x4 t, uint32_t cb, const float4 qb) const {
        const uint32_t c16 = lane & 15, h = lane >> 4;
        const bool diag = UPPER && J == I;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            bool pass = false;
            if (id[i] != 0xFFFFFFFFu && cb != 0xFFFFFFFFu && (!diag || 4 * h + i < c16))
                pass = (uint32_t)approx_interval<KINDA>(t[i] * meta[i].y, meta[i].x, qb, Kc, rho, 0.f) <= tq;
            const bool swap = UPPER && cb < id[i];
            pool_push(ctr, cand, cap, pass, ((uint64_t)(swap ? cb : id[i]) << 32) | (swap ? id[i] : cb), lane);
        }
    }
};

// The list sink (the graphs): every held line has its own tau, count and (row, lo, hi) list -- ZhExact2's layout, `cap` slots a line of which `lim`
// may be filled.  Self is the column with the line's own row number; a masked row on either side is no pair.  The 16 lanes of a k-group h share
// the line: one atomic for the group, taken by its first passing lane.  A list that runs over raises *over.  SELF = false (the k-NN join between two
// indexes: the two sides' row numbers are unrelated) skips no column for its number.
template <int KINDA, bool SELF = true>
struct ListSink {
    uint32_t lane;
    float Kc, rho;
    uint32_t *__restrict__ cnt, *__restrict__ lid, *__restrict__ llo, *__restrict__ lhi;
    uint32_t cap, lim;
    uint32_t *__restrict__ over;
    uint32_t id[4], line[4], tq[4];  // this lane's held lines line0 + 4 h + i
    float2 meta[4];
    __device__ __forceinline__ void hold(bool active, uint32_t line0, const uint32_t *__restrict__ rows, const float2 *__restrict__ rmeta,
                                         const uint32_t *__restrict__ tau) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            id[i] = 0xFFFFFFFFu; line[i] = 0; tq[i] = 0; meta[i] = make_float2(0.f, 0.f);
            if (active) {
                line[i] = line0 + 4 * (lane >> 4) + i;
                id[i] = rows[line[i]];
                if (id[i] != 0xFFFFFFFFu) { meta[i] = rmeta[line[i]]; tq[i] = tau[line[i]]; }
            }
        }
    }
    template <typename TI>
    __device__ __forceinline__ bool wants(TI) const { return true; }
    template <typename TI>
    __device__ __forceinline__ void operator()(TI, const f32x4 t, uint32_t cb, const float4 qb) const {
        const uint32_t c16 = lane & 15, h = lane >> 4;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            bool pass = false;
            uint32_t lo = 0, hi = 0;
            if (id[i] != 0xFFFFFFFFu && cb != 0xFFFFFFFFu && (!SELF || cb != id[i])) {
                const uint64_t iv = approx_interval<KINDA>(t[i] * meta[i].y, meta[i].x, qb, Kc, rho, 0.f);
                lo = (uint32_t)iv; hi = (uint32_t)(iv >> 32);
                pass = lo <= tq[i];
            }
            const uint64_t m = __ballot(pass);
            if (m) {  // (wave-uniform)
                const uint32_t gm = (uint32_t)(m >> (16 * h)) & 0xFFFFu;
                const uint32_t leader = gm ? (uint32_t)__builtin_ctz(gm) : 0u;
                uint32_t base = 0;
                if (pass && c16 == leader) base = atomicAdd(&cnt[line[i]], (uint32_t)__popc(gm));
                base = (uint32_t)__shfl((int)base, (int)(16 * h + leader), 64);
                if (pass) {
                    const uint32_t slot = base + (uint32_t)__popc(gm & ((1u << c16) - 1u));
                    if (slot < lim) {
                        const size_t o = (size_t)line[i] * cap + slot;
                        lid[o] = cb; llo[o] = lo; lhi[o] = hi;
                    } else
                        atomicOr(over, 1u);
                }
            }
        }
    }
};

// The record sink (test / debug: zh_debug_walk_pairs, zh_walkdbg.hip; no product path): EVERY pair of the rectangle held positions [p0, p1) x the
// walked column positions leaves one record at (held position - p0) * ncol + column position -- the positions, either side's row-or-masked word,
// the interval as the two product sinks would form it (the same call of approx_interval on the same operands; they form it for unmasked pairs
// only) and the sum it was formed from.  Nothing is stored at or past `cap`.
template <int KINDA, typename TI>
struct RecordSink : PoolSink<KINDA, false, TI> {  // the held rows' words and rowMeta by the pool sink's own hold(); its pool stays null
    using PoolSink<KINDA, false, TI>::lane;
    using PoolSink<KINDA, false, TI>::I;
    using PoolSink<KINDA, false, TI>::Kc;
    using PoolSink<KINDA, false, TI>::rho;
    using PoolSink<KINDA, false, TI>::id;
    using PoolSink<KINDA, false, TI>::meta;
    zh_debug_walk_pair *__restrict__ out;
    uint64_t cap, p0, p1, ncol;
    __device__ __forceinline__ RecordSink(uint32_t lane_, TI I_, float Kc_, float rho_, zh_debug_walk_pair *out_, uint64_t cap_, uint64_t p0_, uint64_t p1_,
                                          uint64_t ncol_)
        : PoolSink<KINDA, false, TI>{lane_, I_, 0u, Kc_, rho_, nullptr, 0, nullptr}, out(out_), cap(cap_), p0(p0_), p1(p1_), ncol(ncol_) {}
    __device__ __forceinline__ bool wants(TI) const { return true; }
    __device__ __forceinline__ void operator()(TI J, const f32x4 t, uint32_t cb, const float4 qb) const {
        const uint32_t c16 = lane & 15, h = lane >> 4;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint64_t hp = (uint64_t)I * 16 + 4 * h + i, cp = (uint64_t)J * 16 + c16;
            if (hp < p0 || hp >= p1 || cp >= ncol) continue;
            const uint64_t slot = (hp - p0) * ncol + cp;
            if (slot >= cap) continue;
            const float s = t[i] * meta[i].y;
            const uint64_t iv = approx_interval<KINDA>(s, meta[i].x, qb, Kc, rho, 0.f);
            zh_debug_walk_pair r;
            r.held_pos = (uint32_t)hp; r.col_pos = (uint32_t)cp; r.held_row = id[i]; r.col_row = cb;
            r.lo = (uint32_t)iv; r.hi = (uint32_t)(iv >> 32); r.raw_s = s;
            out[slot] = r;
        }
    }
};

// ---- host side: the ONE list of dimensions the family scans are built for, and their launch dispatch ----
template <int... DS>
struct ZhDims {};
typedef ZhDims<256, 384, 512, 768, 1024> ZhMfmaDims;
// f(D, KINDA) (integral constants) for the d of the list; false: d is not in it
template <int KINDA, class F, int... DS>
static inline bool zh_mfma_dispatch_d(uint32_t d, F &f, ZhDims<DS...>) {
    return ((d == (uint32_t)DS && (f(std::integral_constant<int, DS>{}, std::integral_constant<int, KINDA>{}), true)) || ...);
}
static inline bool zh_mfma_dim(uint32_t d) {
    auto none = [](auto, auto) {};
    return zh_mfma_dispatch_d<0>(d, none, ZhMfmaDims{});
}
// f launches the <D, KINDA> instantiation of a family's scan; KINDA = approx_interval's: 0 the L2 metrics, 1 the cosine, 2 its parity key
template <class F>
static inline hipError_t zh_mfma_dispatch(uint32_t d, int metric, int mode, F f) {
    const bool known = metric != ZH_COSINE          ? zh_mfma_dispatch_d<0>(d, f, ZhMfmaDims{})
                       : mode == ZH_COSINE_PARITY ? zh_mfma_dispatch_d<2>(d, f, ZhMfmaDims{})
                                                  : zh_mfma_dispatch_d<1>(d, f, ZhMfmaDims{});
    return known ? hipGetLastError() : hipErrorInvalidValue;
}
