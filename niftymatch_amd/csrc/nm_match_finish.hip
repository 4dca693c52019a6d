// nm_match_finish.hip -- what follows a screen: the exact finalize pass and the rows of the second pass of the two-stage screen.
#include "nm_match_select.hpp"

namespace nm_match {
namespace {

// Four lanes per query. Each lane scans a quarter of the query's 2*S partial candidates, the quad merges them into the
// 4 best by (approximate distance, index), every lane recomputes ONE of them EXACTLY (sum_k fma(t,t,acc), k ascending:
// all loads in flight together), and lane 0 of the quad forms the exact (min1, idx, min2).
// Proof obligation: every candidate NOT recomputed has an approximate distance >= rest (the minimum over the chunks'
// third-best values and everything that dropped out of a top-4 list). If rest is not safely above the exact min2
// (margin = bound on the MFMA formulation's error), the query is appended to the fallback list instead of being emitted.
//
// STAGE 0: the single-pass screens (fp32, bf16x3). Two-stage screen: STAGE 1 after the fp16 coarse pass -- the same proof
// with the coarse pass's error bound (below); an unproven row goes to the list of the bf16x3 pass instead of the exact
// fallback -- and STAGE 2 after the bf16x3 pass over the listed rows: partial lists, norms and the row count are in list
// order (r), everything else belongs to row i = f1_list[r].
template <int STAGE>
__device__ __forceinline__ void finalize_block(const MatchBatch &bt, const MatchPair &c, int block, int nA, int S)
{
    const float *__restrict__ A = c.A, *__restrict__ B = c.B;
    const int mode = c.mode, index_offset = c.index_offset;
    const float4 *__restrict__ partial = c.partial;
    const float *__restrict__ partial3 = c.partial3;
    const float *__restrict__ na = c.na;
    const float ambiguity = bt.ambiguity;
    int *__restrict__ result = c.result;
    float *__restrict__ min1_out = c.min1, *__restrict__ min2_out = c.min2;
    int *__restrict__ idx_out = c.idx1;
    int *__restrict__ fb_count = c.fb_count, *__restrict__ fb_list = c.fb_list;
    const int t = block * 256 + threadIdx.x;
    const int sub = t & 3;
    const bool live = (t >> 2) < nA;
    const int iq = live ? (t >> 2) : nA - 1;             // row of the partial lists
    const int i = (STAGE == 2) ? c.f1_list[iq] : iq;     // row of A / of the outputs
    float cd[4]; int ci[4];
    float rest = __builtin_inff();
#pragma unroll
    for (int k = 0; k < 4; ++k) { cd[k] = __builtin_inff(); ci[k] = -1; }
    const int nB = pair_nB(c);
    auto insert = [&](float d, int j) {
        if (j < 0 || j >= nB) return;                // absent, or a row of the last tile's padding (bf16x3: finite "norm")
#pragma unroll
        for (int k = 0; k < 4; ++k) {                // sorted insertion by (approx distance, index)
            const bool lt = (d < cd[k]) || (d == cd[k] && j < ci[k]);
            if (lt) { const float td = cd[k]; const int tj = ci[k]; cd[k] = d; ci[k] = j; d = td; j = tj; }
        }
        if (j >= 0) rest = __builtin_fminf(rest, d);  // fell off the end of the list: not going to be recomputed
    };
    for (int s = sub; s < S; s += 4) {
        const float4 p = partial[(size_t)iq * S + s];
        rest = __builtin_fminf(rest, partial3[(size_t)iq * S + s]);
        insert(p.x, __float_as_int(p.y));
        insert(p.z, __float_as_int(p.w));
    }
#pragma unroll
    for (int m = 1; m <= 2; m <<= 1) {               // quad butterfly: afterwards all 4 lanes hold the same sorted top-4
        float od[4]; int oi[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) { od[k] = __shfl_xor(cd[k], m); oi[k] = __shfl_xor(ci[k], m); }
        rest = __builtin_fminf(rest, __shfl_xor(rest, m));
#pragma unroll
        for (int k = 0; k < 4; ++k) insert(od[k], oi[k]);
    }
    rest = __builtin_fminf(rest, __builtin_fminf(__shfl_xor(rest, 1), __shfl_xor(rest, 2)));
    rest = __builtin_fminf(rest, __builtin_fminf(__shfl_xor(rest, 1), __shfl_xor(rest, 2)));
    // (Round 3: staging the four candidate rows of every query through LDS -- half a wave per 512-byte row, whole cache lines,
    // then each lane walks its row at the conflict-free pitch -- was built and measured: 155 us per 16-pair call instead of
    // 146. The kernel moves ~500 MB of scattered 512-byte rows per call, ~3.3 TB/s out of L2 / Infinity Cache: it is bound by
    // that gather, not by the shape of its load instructions.)
    // Ratio test decided by the screen alone (mode 0: only result[i] is wanted). Let E(bn) bound |value(j) - d_ref(j)| for a
    // candidate of norm |b_j| <= bn (as in the proof below; + 2^-18 for the key truncation and gamma_130 for d_ref against d,
    // both relative to at most (sqrt na + bn)^2), and Et(X) := E(min(sqrt na + sqrt X, sqrt nb_max)): a candidate with
    // d_ref(j) <= X has |b_j| <= sqrt na + sqrt X (triangle inequality), so its value is <= X + Et(X). The two smallest
    // values v1 <= v2 sit at j1, j2, every other candidate has a value >= v2. Hence
    //   * every d_ref exceeds lo1 := v1 - Et(v1) (a candidate at or below it would have a value below v1), every d_ref
    //     but j1's exceeds lo2 := v2 - Et(v2), and min2 <= hi2 := max(v1 + E(|b_j1|), v2 + E(|b_j2|)) with the two
    //     candidates' own norms;
    //   * lo1 >= ambiguity hi2 (1 + 1e-5) with lo2 > 0 gives min1 / min2 >= ambiguity after its rounding -> -1 (the scan's
    //     clamp of min2 only lowers min2);
    //   * with hi1 := v1 + E(|b_j1|):  v2 > hi1 + Et(hi1) makes j1 the unique minimum (any other candidate at or below hi1
    //     would have a value below v2), min2 > lo2, and hi1 < ambiguity lo2 (1 - 1e-5) gives min1 / min2 < ambiguity -> j1
    //     (not taken for global index 0, where the scan's clamp of min2 could matter).
    // Most rows of a SIFT pair are decided here and never gather their candidates' 512-byte rows, which is what this kernel's
    // time was (3 KB per row; round 3). Any comparison with a NaN fails: the row takes the exact route.
    const float nai = na[i], nbm = c.nbmax[0];
    const bool in_domain = (STAGE == 1) ? (nai < F16_NORM_LIMIT && nbm < F16_NORM_LIMIT) : (nai < NORM_LIMIT && nbm < NORM_LIMIT);
    if (mode == 0 && in_domain && ci[1] >= 0) {
        const float sna = __builtin_sqrtf(nai), snb = __builtin_sqrtf(nbm);
        // (+ 2^-18 key truncation + gamma_130; the coarse pass's keys drop a sixth bit: 2^-17)
        const float coeff = (STAGE == 2 ? bt.err_coeff2 : bt.err_coeff) + (STAGE == 1 ? 1.6e-5f : 1.2e-5f);
        const float rai = (STAGE == 1) ? c.ra[i] : 0.f, rbm = (STAGE == 1) ? c.nbmax[1] : 0.f;
        auto E_of = [&](float bn, float rbj) {            // bn: upper bound of |b_j|, rbj: of its fp16 residual norm
            float e = coeff * ((sna + bn) * (sna + bn)) * 1.0001f + 1e-30f;
            if (STAGE == 1) e += 2.0f * (rai * (bn + rbj) + (sna * 1.000001f + rai) * rbj + rai * rbj) * 1.0001f;
            return e;
        };
        auto Et = [&](float X) {
            const float bn = __builtin_fminf(sna + __builtin_sqrtf(__builtin_fmaxf(X, 0.f)) * 1.00001f, snb);
            return E_of(bn, __builtin_fminf(rbm, 4.8829e-4f * bn + 7e-4f));
        };
        const float v1 = cd[0], v2 = cd[1];
        const float e1 = E_of(__builtin_sqrtf(c.nb[ci[0]]) * 1.000001f, (STAGE == 1) ? c.rb[ci[0]] : 0.f);
        const float e2 = E_of(__builtin_sqrtf(c.nb[ci[1]]) * 1.000001f, (STAGE == 1) ? c.rb[ci[1]] : 0.f);
        const float lo1 = v1 - Et(v1), lo2 = v2 - Et(v2), hi1 = v1 + e1, hi2 = __builtin_fmaxf(hi1, v2 + e2);
        int quick = 0;
        if (lo2 > 0.f && lo1 >= ambiguity * hi2 * 1.00001f) quick = 1;
        else if (lo2 > 0.f && v2 > hi1 + Et(hi1) && ambiguity > 0.f && hi1 < ambiguity * lo2 * 0.99999f && ci[0] + index_offset > 0) quick = 2;
        if (quick) {                                      // the same for the four lanes of the quad
            if (live && sub == 0) result[i] = (quick == 1) ? -1 : ci[0] + index_offset;
            return;
        }
    }
    const int mine = (sub == 0) ? ci[0] : (sub == 1) ? ci[1] : (sub == 2) ? ci[2] : ci[3];
    float d = 0.f;
    if (mine >= 0)
        d = exact_dist(reinterpret_cast<const float4 *>(A + (size_t)i * DIM),
                       reinterpret_cast<const float4 *>(B + (size_t)mine * DIM));
    float ed[4]; int ei[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) { ed[k] = __shfl(d, ((threadIdx.x & 63) & ~3) + k); ei[k] = ci[k]; }
    if (!live || sub != 0) return;
    if (STAGE == 1) {
        // outside the coarse pass's domain (|2 x| must stay inside the fp16 range: squared norms below F16_NORM_LIMIT; NaN and
        // inf fail the comparison too): the bf16x3 pass decides, or passes the row on to the exact scan
        if (!(nai < F16_NORM_LIMIT) || !(*c.nbmax < F16_NORM_LIMIT)) {
            const int pos = atomicAdd(pair_f1_count(c), 1);
            c.f1_list[pos] = i;
            return;
        }
    } else if (!(nai < NORM_LIMIT) || !(*c.nbmax < NORM_LIMIT)) {    // outside the screens' domain (NaN, inf, huge): exact scan
        const int pos = atomicAdd(fb_count, 1);
        fb_list[pos] = i;
        return;
    }
    // exact minimum at the lowest index and second smallest of the recomputed candidates (+inf: there is no second)
    float m1 = __builtin_inff(), m2 = __builtin_inff(); int idx = 0x7fffffff;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (ei[k] < 0) continue;
        if (ed[k] < m1 || (ed[k] == m1 && ei[k] < idx)) { m2 = m1; m1 = ed[k]; idx = ei[k]; }
        else if (ed[k] < m2) m2 = ed[k];
    }
    if (idx == 0x7fffffff) return;
    // Proof obligation ("matcher theorem"): every candidate j that was NOT recomputed must have a
    // reference distance d_ref(j) > m2. With u = 2^-24, gamma_n = n u / (1 - n u):
    //   * the MFMA value is a 130-step fma chain nb^ + na^ - 2 sum a_k b_k with 129 roundings, products exact:
    //     |d~ - (na^ + nb^ - 2 a.b)| <= gamma_129 (na^ + nb^ + 2 sum |a_k b_k|) <= gamma_129 (sqrt na + sqrt nb)^2 (1 + gamma_128)
    //   * the norms are 128-step fma chains of squares: |na^ - na| <= gamma_128 na, the same for nb
    //     => |d~(j) - d(j)| <= 2 gamma_129 (sqrt na + sqrt nb_j)^2 =: E_j
    //   * the reference chain sum fma(t,t,acc), t = fl(a_k - b_k), gives d_ref >= d (1 - gamma_130)
    //   * a key reports d~ with its low 5 mantissa bits replaced: |value - d~| < 2^-18 |d~|
    // Suppose d_ref(j) <= m2. Then d(j) <= M := m2 (1 + gamma_131), and sqrt nb_j <= min(sqrt na + sqrt M, sqrt nb_max)
    // (triangle inequality; nb_max = the largest candidate norm, nbmax_kernel), so with s := min(2 sqrt na + sqrt M,
    // sqrt na + sqrt nb_max):  value(j) <= (M + 2 gamma_129 s^2) (1 + 2^-18) =: bound, and rest <= value(j) <= bound.
    // Hence rest > bound proves the row; otherwise the row is re-scanned exactly. Deterministic for every input
    // (2 gamma_129 = 1.5378e-5; the constants below carry the slop of evaluating the bound itself in fp32).
    const float sna = __builtin_sqrtf(nai);
    const float sq = __builtin_fminf(2.0f * sna + __builtin_sqrtf(m2), sna + __builtin_sqrtf(*c.nbmax));
    float bound = (m2 * 1.00001f + (STAGE == 2 ? bt.err_coeff2 : bt.err_coeff) * (sq * sq)) * 1.00001f + 1e-30f;      // 1 + 2^-17 = 1.0000076
    if (STAGE == 1) {
        // Coarse pass: the MFMA chain sums the norms and the EXACT products of the fp16 images a_h (= -image / 2) and b_h,
        // so err_coeff sq^2 above bounds its distance from  na + nb - 2 a_h.b_h  (134 terms instead of 130: the coefficient
        // carries a factor 2 of slack), and   a.b - a_h.b_h = e_a.b_h + a_h.e_b + e_a.e_b   with e = x - x_h gives
        //   |d~(j) - d(j)| <= err_coeff sq^2 + 2 (ra |b_h| + |a_h| rb_j + ra rb_j),   ra = |e_a|, rb_j = |e_b_j|  (Cauchy-Schwarz),
        // ra and rb_j being the upper bounds prep_kernel<2> computed from the images themselves. For a candidate with
        // d_ref(j) <= m2:  |b_j| <= bn := sq - sqrt na  (the triangle inequality / nb_max, as above),  |b_h| <= bn + rb_j,
        // |a_h| <= sqrt na + ra,  and  rb_j <= min(rb_max, 2^-11 bn + 7e-4): round-to-nearest fp16 loses at most 2^-11
        // relative per element, 2^-14 absolute per element of the 128 below the normal range (subnormal or flushed alike).
        const float bn = (sq - sna) * 1.000001f;
        const float rbj = __builtin_fminf(c.nbmax[1], 4.8829e-4f * bn + 7e-4f);
        const float rai = c.ra[i];
        const float e16 = 2.0f * (rai * (bn + rbj) + (sna * 1.000001f + rai) * rbj + rai * rbj);
        bound = (bound + e16 * 1.00001f) * 1.00001f;
    }
    if (!(rest > bound) && rest < __builtin_inff()) {    // a NaN bound (norms at the edge of the domain) proves nothing
        if (STAGE == 1) {
            const int pos = atomicAdd(pair_f1_count(c), 1);
            c.f1_list[pos] = i;
        } else {
            const int pos = atomicAdd(fb_count, 1);
            fb_list[pos] = i;
        }
        return;
    }
    emit_match(i, m1, idx + index_offset, m2, mode, ambiguity, result, min1_out, idx_out, min2_out);
}

// 64 rows per 256-thread block; the blocks of a pair stride over its rows (STAGE 0 / 1: the grid covers the batch's largest
// set or the capacity, one block per workgroup; STAGE 2: a few workgroups per pair walk the short list)
template <int STAGE>
__global__ __launch_bounds__(256) void match_finalize_kernel(MatchBatch bt)
{
    const MatchPair &c = bt.p[blockIdx.y];
    if (pair_nA(c) <= 0 || pair_nB(c) <= 0) return;      // device-sized call with an empty set: nothing was screened
    const int nA = (STAGE == 2) ? min(max(*pair_f1_count(c), 0), pair_nA(c)) : pair_nA(c);
    const int S = (STAGE == 2) ? pair_plan2(c)->S : pair_S(c);
    for (int block = blockIdx.x; block * 64 < nA; block += gridDim.x) finalize_block<STAGE>(bt, c, block, nA, S);
}

// Two-stage screen, between its passes: the rows the coarse pass listed get what the bf16x3 kernel reads -- split images
// (scaled by -2) and norms in LIST order -- and the first wave of every pair makes the work plan for their number (the
// same make_plan_on as everywhere). Half a wave per listed row, as in prep_kernel.
__global__ __launch_bounds__(256) void fine_rows_kernel(MatchBatch bt)
{
    const MatchPair &c = bt.p[blockIdx.y];
    const int nA = pair_nA(c), nB = pair_nB(c), lane = threadIdx.x & 63, k4 = lane & 31;
    const int count = (nA > 0 && nB > 0) ? min(max(*pair_f1_count(c), 0), nA) : 0;
    if (blockIdx.x == 0 && threadIdx.x < 64) {
        const MatchPlan p = make_plan_on(count, nB, bt.n_cu2, bt.n_xcd, lane, 64, [](int v) { return nmw::wave_max(v); });
        MatchPlan q = p;
        if (count == 0) q.G = 0;                          // nothing listed: every workgroup of the second pass leaves at once
        if (lane == 0) *pair_plan2(c) = q;
    }
    for (int blk = blockIdx.x; blk * PREP_ROWS < count; blk += gridDim.x)
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int r = blk * PREP_ROWS + (threadIdx.x >> 6) * 4 + (lane >> 5) + 2 * q;
        if (r >= count) continue;
        const int i = c.f1_list[r];
        const float4 x = reinterpret_cast<const float4 *>(c.A + (size_t)i * DIM)[k4];
        unsigned h0, l0, h1, l1, h2, l2, h3, l3;
        bf16_split(-2.0f * x.x, h0, l0); bf16_split(-2.0f * x.y, h1, l1);
        bf16_split(-2.0f * x.z, h2, l2); bf16_split(-2.0f * x.w, h3, l3);
        unsigned *dst = c.As + (size_t)r * DIM;
        reinterpret_cast<uint2 *>(dst)[k4] = make_uint2(h0 | (h1 << 16), h2 | (h3 << 16));
        reinterpret_cast<uint2 *>(dst + 64)[k4] = make_uint2(l0 | (l1 << 16), l2 | (l3 << 16));
        if (k4 == 0) c.na2[r] = c.na[i];
    }
}

}  // namespace

void launch_finalize(int stage, const MatchBatch &bt, dim3 grid, hipStream_t st)
{
    if (stage == 2) hipLaunchKernelGGL(match_finalize_kernel<2>, grid, dim3(256), 0, st, bt);
    else if (stage) hipLaunchKernelGGL(match_finalize_kernel<1>, grid, dim3(256), 0, st, bt);
    else hipLaunchKernelGGL(match_finalize_kernel<0>, grid, dim3(256), 0, st, bt);
}

void launch_fine_rows(const MatchBatch &bt, dim3 grid, hipStream_t st)
{
    hipLaunchKernelGGL(fine_rows_kernel, grid, dim3(256), 0, st, bt);
}

}  // namespace nm_match
