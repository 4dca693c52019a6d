// nm_match_select.hpp -- device helpers that more than one of the matcher's units use: the running top-3 keys and the end of a
// segment, the fp32 MFMA k-groups, the reference's exact distance chain and the last step of its scan.
#pragma once
#include "nm_match_fp.hpp"
#include "nm_match_types.hpp"

namespace nm_match {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// Running best / second best / third best of one lane's query, as integer KEYS. The MFMA pipe and the VALU do not overlap
// on a SIMD here (measured: every epilogue instruction adds to the kernel time), so the selection is written for the
// fewest instructions: a key is the distance's bit pattern with its low 5 bits replaced by the slot (0..31) of the
// candidate inside the current 64-candidate group (v_and_or_b32), keys order like the distances under signed integer
// comparison (positive floats; the slightly negative values that rounding can produce for near-duplicates all lie
// within the finalize margin of zero), and inserting a key into a sorted triple is min + med3 + med3 -- the slot
// travels inside the key. Per group the triple of the 32 accumulator values is built this way (4 instructions per
// element) and its three keys are merged into the running triple, whose two best also carry the group number.
// Truncating 5 mantissa bits lowers a value by < 2^-18 relative: the finalize margin accounts for it.
constexpr int KEY_SLOT_BITS = 5;
constexpr int KEY_INF = 0x7fffffff;

__device__ __forceinline__ int imed3(int a, int b, int c)        // the compiler only recognises some of the min/max forms
{
    int r;
    asm("v_med3_i32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
__device__ __forceinline__ void key_insert3(int &k1, int &k2, int &k3, int k)
{
    const int n3 = imed3(k2, k3, k), n2 = imed3(k1, k2, k);
    k1 = min(k1, k); k2 = n2; k3 = n3;
}
struct Top3 { int k1, k2, k3, t1, t2; };                          // keys + group tags of the two best
__device__ __forceinline__ void top3_merge(Top3 &t, int k, int tag)
{
    t.k3 = imed3(t.k2, t.k3, k);
    const bool lt1 = k < t.k1, lt2 = k < t.k2;
    t.k2 = lt1 ? t.k1 : (lt2 ? k : t.k2);
    t.t2 = lt1 ? t.t1 : (lt2 ? tag : t.t2);
    t.k1 = lt1 ? k : t.k1;
    t.t1 = lt1 ? tag : t.t1;
}
template <int BITS = KEY_SLOT_BITS>
__device__ __forceinline__ float key_value(int k) { return __int_as_float(k & ~((1 << BITS) - 1)); }

// used by the lane-half merge at the end of the kernel (values + full indices)
struct Top2 { float m1, m2, m3; int i1, i2; };

__device__ __forceinline__ void top2_insert(Top2 &t, float d, int j)
{
    t.m3 = __builtin_amdgcn_fmed3f(t.m2, t.m3, d);      // third smallest of {m1, m2, m3, d} (m2 <= m3)
    const bool lt1 = d < t.m1, lt2 = d < t.m2;
    t.m2 = lt1 ? t.m1 : (lt2 ? d : t.m2);
    t.i2 = lt1 ? t.i1 : (lt2 ? j : t.i2);
    t.m1 = lt1 ? d : t.m1;
    t.i1 = lt1 ? j : t.i1;
}

// fold the 2 x 16 accumulator values of one 64-candidate group into the running triple (see Top3 above)
template <int BITS = KEY_SLOT_BITS>
__device__ __forceinline__ void select_half(const f32x16 &acc0, const f32x16 &acc1, Top3 &best, int tag)
{
    int g1 = KEY_INF, g2 = KEY_INF, g3 = KEY_INF;
#pragma unroll
    for (int e = 0; e < 16; ++e) key_insert3(g1, g2, g3, (__float_as_int(acc0[e]) & ~((1 << BITS) - 1)) | e);
#pragma unroll
    for (int e = 0; e < 16; ++e) key_insert3(g1, g2, g3, (__float_as_int(acc1[e]) & ~((1 << BITS) - 1)) | (16 + e));
    if (__any(g1 < best.k3)) {
        top3_merge(best, g1, tag);
        top3_merge(best, g2, tag);
        top3_merge(best, g3, tag);
    }
}

// 2 x (32 candidates x 32 queries x 128 + 1 k-pairs): acc[g] = |b_j|^2 + |a_i|^2 - 2 a_i.b_j for candidates
// 64 half + 32 g + (row of the accumulator layout). rowp = this lane's candidate row of group 0 at its k offset 4 h.
// The MFMAs are hand-placed (inline asm): the two accumulator chains alternate, and the "memory" clobbers keep the
// fragment reads of k-group t+1 (ordinary loads, counted and waited for by the compiler at their first use) above the
// MFMAs of k-group t. hipcc's own schedule of the equivalent builtins waits for every read right after issuing it and
// runs the chains one after the other.
#define NM_MFMA "v_mfma_f32_32x32x2_f32 "
// k-groups T0 .. T1 - 1 (8 values of k each) of both accumulators; NORMS: the chain starts with the augmented k-pair, otherwise
// from the inline constant 0. mfma_half = all 16 groups (the matcher's screen). The distance pass splits k into two chains.
template <int T0, int T1, bool NORMS>
__device__ __forceinline__ void mfma_kgroups(f32x16 &acc0, f32x16 &acc1, const float *rowp, const float *normp,
                                             const float4 (&qf)[16], float nq)
{
    const float *r0 = rowp, *r1 = rowp + 32 * KP;
    float4 c0 = *reinterpret_cast<const float4 *>(r0 + 8 * T0), c1 = *reinterpret_cast<const float4 *>(r1 + 8 * T0);
    if (NORMS) {
        const float cn0 = normp[0], cn1 = normp[32 * KP];  // column 128 + h: (nb_j, 1) for h = (0, 1)
        // augmented k-pair: (nb_j * 1) + (1 * na_i), accumulators start from the inline constant 0
        asm volatile(NM_MFMA "%0, %2, %4, 0\n\t" NM_MFMA "%1, %3, %4, 0"
                     : "=&v"(acc0), "=&v"(acc1) : "v"(cn0), "v"(cn1), "v"(nq) : "memory");
    }
#pragma unroll
    for (int t = T0; t < T1; ++t) {
        float4 n0 = c0, n1 = c1;
        if (t + 1 < T1) {                               // next k-group's fragments fly during this group's 8 MFMAs
            n0 = *reinterpret_cast<const float4 *>(r0 + 8 * (t + 1));
            n1 = *reinterpret_cast<const float4 *>(r1 + 8 * (t + 1));
        }
        if (!NORMS && t == T0)                          // first instruction of a chain without the norm pair: C = 0
            asm volatile(NM_MFMA "%0, %2, %10, 0\n\t" NM_MFMA "%1, %6, %10, 0\n\t"
                         NM_MFMA "%0, %3, %11, %0\n\t" NM_MFMA "%1, %7, %11, %1\n\t"
                         NM_MFMA "%0, %4, %12, %0\n\t" NM_MFMA "%1, %8, %12, %1\n\t"
                         NM_MFMA "%0, %5, %13, %0\n\t" NM_MFMA "%1, %9, %13, %1"
                         : "=&v"(acc0), "=&v"(acc1)
                         : "v"(c0.x), "v"(c0.y), "v"(c0.z), "v"(c0.w), "v"(c1.x), "v"(c1.y), "v"(c1.z), "v"(c1.w),
                           "v"(qf[t].x), "v"(qf[t].y), "v"(qf[t].z), "v"(qf[t].w)
                         : "memory");
        else
            asm volatile(NM_MFMA "%0, %2, %10, %0\n\t" NM_MFMA "%1, %6, %10, %1\n\t"
                         NM_MFMA "%0, %3, %11, %0\n\t" NM_MFMA "%1, %7, %11, %1\n\t"
                         NM_MFMA "%0, %4, %12, %0\n\t" NM_MFMA "%1, %8, %12, %1\n\t"
                         NM_MFMA "%0, %5, %13, %0\n\t" NM_MFMA "%1, %9, %13, %1"
                         : "+v"(acc0), "+v"(acc1)
                         : "v"(c0.x), "v"(c0.y), "v"(c0.z), "v"(c0.w), "v"(c1.x), "v"(c1.y), "v"(c1.z), "v"(c1.w),
                           "v"(qf[t].x), "v"(qf[t].y), "v"(qf[t].z), "v"(qf[t].w)
                         : "memory");
        c0 = n0; c1 = n1;
    }
    // an MFMA's result may be read by a non-MFMA instruction only 18 wait states after its issue (16-pass XDL op):
    // the compiler does not see inside the asm statements, so the padding is explicit
    asm volatile("s_nop 15\n\ts_nop 3" : "+v"(acc0), "+v"(acc1));
}
#undef NM_MFMA

// End of a segment: decode (value, candidate index) of the two best, merge the two lane halves (same query, disjoint
// candidates), publish into this segment's slot of the query block. c0 = first candidate of the segment.
// BITS 5: tag = 64-candidate group of the segment. BITS 6 (coarse pass): tag = tile iteration n, the sixth slot bit tells
// group 2 n - 1 (0) from group 2 n (1).
template <int BITS = KEY_SLOT_BITS>
__device__ __forceinline__ void segment_publish(const Top3 &best, const MatchPlan &plan, const PlanGroup &grp, int pc, int qbl,
                                                int vg, bool ends_piece, int c0, int h, int qi, int nA, int S,
                                                float4 *__restrict__ partial, float *__restrict__ partial3)
{
    auto index_of = [&](int k, int tag) {
        const int slot = k & 31, g = slot >> 4, e = slot & 15;
        const int group = (BITS == 6) ? 2 * tag - 1 + ((k >> 5) & 1) : tag;
        return c0 + group * 64 + 32 * g + (e & 3) + 8 * (e >> 2) + 4 * h;
    };
    Top2 m;
    m.m1 = key_value<BITS>(best.k1); m.m2 = key_value<BITS>(best.k2); m.m3 = key_value<BITS>(best.k3);
    m.i1 = (best.k1 != KEY_INF) ? index_of(best.k1, best.t1) : -1;
    m.i2 = (best.k2 != KEY_INF) ? index_of(best.k2, best.t2) : -1;
    if (best.k1 == KEY_INF) m.m1 = __builtin_inff();
    if (best.k2 == KEY_INF) m.m2 = __builtin_inff();
    if (best.k3 == KEY_INF) m.m3 = __builtin_inff();
    Top2 o;
    o.m1 = __shfl_xor(m.m1, 32); o.m2 = __shfl_xor(m.m2, 32); o.m3 = __shfl_xor(m.m3, 32);
    o.i1 = __shfl_xor(m.i1, 32); o.i2 = __shfl_xor(m.i2, 32);
    if (o.i1 >= 0) top2_insert(m, o.m1, o.i1);
    if (o.i2 >= 0) top2_insert(m, o.m2, o.i2);
    m.m3 = __builtin_fminf(m.m3, o.m3);         // o.m3 >= o.m2 >= the merged m2: only the third value can change
    // slot = how many segments of this query block come before this one in the plan's order
    const int slot = plan_slot(plan, grp, pc, qbl, vg);
    if (h == 0 && qi < nA) {
        partial[(size_t)qi * S + slot] = make_float4(m.m1, __int_as_float(m.i1), m.m2, __int_as_float(m.i2));
        partial3[(size_t)qi * S + slot] = m.m3;
        if (pc == plan.C - 1 && ends_piece) {     // this segment ends the block: blank the slots nobody writes
            for (int k = slot + 1; k < S; ++k) {
                partial[(size_t)qi * S + k] = make_float4(__builtin_inff(), __int_as_float(-1), __builtin_inff(), __int_as_float(-1));
                partial3[(size_t)qi * S + k] = __builtin_inff();
            }
        }
    }
}

__device__ __forceinline__ float exact_dist(const float4 *__restrict__ a, const float4 *__restrict__ b)
{
    float4 x[DIM / 4], y[DIM / 4];
#pragma unroll
    for (int k = 0; k < DIM / 4; ++k) { x[k] = a[k]; y[k] = b[k]; }     // all 64 loads in flight together
    float acc = 0.0f;
#pragma unroll
    for (int k = 0; k < DIM / 4; ++k) {
        float t;
        t = x[k].x - y[k].x; acc = __builtin_fmaf(t, t, acc);
        t = x[k].y - y[k].y; acc = __builtin_fmaf(t, t, acc);
        t = x[k].z - y[k].z; acc = __builtin_fmaf(t, t, acc);
        t = x[k].w - y[k].w; acc = __builtin_fmaf(t, t, acc);
    }
    return acc;
}

// Last step of the reference's scan (match.cu:91-116), given what the scan's comparisons make of a row: m1 = its smallest
// non-NaN distance at the LOWEST index idx (or NaN with idx 0 when the distance to candidate 0 is NaN: `current < NaN` is
// false for good), m2 = the smallest of the OTHER non-NaN distances, +inf when there is none. The scan starts min_2 at
// 2139095040.0f (the int 0x7f800000 converted, not +inf) and OVERWRITES it with the old minimum at every replacement
// (:97), so that initial value survives only while the minimum sits at candidate 0: clamp iff idx == 0 (idx < 0: the row
// has no distance below +inf at all; its ratio test fails either way).
// mode 0: ratio test -> result[i] (untouched when min2 <= 0); mode 1: emit the shard triple, min2 UNCLAMPED -- the merge
// over the shards applies the clamp, on the global index (idx here is already global).
__device__ __forceinline__ void emit_match(int i, float m1, int idx, float m2, int mode, float ambiguity,
                                           int *__restrict__ result, float *__restrict__ min1_out,
                                           int *__restrict__ idx_out, float *__restrict__ min2_out)
{
    if (mode == 1) { min1_out[i] = m1; idx_out[i] = idx; min2_out[i] = m2; return; }
    if (idx <= 0 && MIN2_INIT < m2) m2 = MIN2_INIT;
    if (m2 > 0) {
        const float q = m1 / m2;
        result[i] = (q < ambiguity) ? idx : -1;
    }
}

__device__ __forceinline__ void top2_merge(float &m1, int &i1, float &m2, float o1, int oi, float o2)
{
    const bool take = (o1 < m1) || (o1 == m1 && oi < i1);
    const float lo = take ? o1 : m1, hi = take ? m1 : o1;
    const float s2 = take ? o2 : m2;
    i1 = take ? oi : i1;
    m1 = lo;
    m2 = (hi < s2) ? hi : s2;
}

}  // namespace nm_match
