// nm_match_screen.hip -- the matcher's screening passes: row preparation, the three MFMA screens and the kernels that run them.
// (The overview of the fused path is in nm_match.hip.)
#include "nm_match_select.hpp"

namespace nm_match {
namespace {

// Half a wave per row of A (nA rows) and B (nB rows, then the padding of the last 128-candidate tile) of every pair, four
// rows per wave in flight (a lane holds one float4 of two rows):
//   * ||x||^2 as RN32 of a binary64 sum of exact squares (error <= 2^-24 relative: the screens' bounds count on it);
//     rows past nB get +inf (fp32 screen) -- the MFMA kernels stage whole tiles;
//   * MODE 1 (bf16x3 screen): the row's split image [128 x bf16 hi | 128 x bf16 lo] (A is scaled by -2 first: exact), and
//     for candidates the 16-byte k-slot (nb_h, nb_m, nb_l, 1, 1, 1, 0, 0) that adds the norms inside the MFMA chain;
//   * MODE 2 (two-stage screen): the same for the candidates only (the rows of A that need the bf16x3 pass are split
//     later, fine_rows_kernel), plus the fp16 images [128 x fp16] of -2 A and of B (round to nearest even) and an upper
//     bound of the 2-norm of each row's rounding residual x - x_h (x_h = what the image holds, unscaled).
template <int MODE>
__global__ __launch_bounds__(256) void prep_kernel(MatchBatch bt)
{
    const MatchPair &c = bt.p[blockIdx.y];
    const int nA = pair_nA(c), nB = pair_nB(c), lane = threadIdx.x & 63, k4 = lane & 31;
    const int padded = nm_divup_dev(nB, TILE_C) * TILE_C;
    if (blockIdx.x == 0 && threadIdx.x == 0 && c.fb_count) {     // first launch of a match call: resets the row lists
        *c.fb_count = 0;
        if (MODE == 2) *pair_f1_count(c) = 0;
    }
    const int r0 = blockIdx.x * PREP_ROWS + (threadIdx.x >> 6) * 4 + (lane >> 5);    // this lane's rows: r0 and r0 + 2
    float4 v[2];
    int row[2]; bool isA[2], live[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        int i = r0 + 2 * q;
        isA[q] = i < nA;
        if (!isA[q]) i -= nA;
        row[q] = i;
        live[q] = isA[q] || i < nB;
        v[q] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (live[q]) v[q] = reinterpret_cast<const float4 *>((isA[q] ? c.A : c.B) + (size_t)i * DIM)[k4];
    }
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int i = row[q];
        if (!live[q]) {                                   // uniform per half wave
            if (i < padded && k4 == 0) {
                c.nb[i] = __builtin_inff();
                if (MODE) c.nbslot[i] = make_uint4(BF16_BIG, BF16_ONE << 16, BF16_ONE | (BF16_ONE << 16), 0u);
            }
            continue;
        }
        const float4 x = v[q];
        double acc = ((double)x.x * (double)x.x + (double)x.y * (double)x.y) + ((double)x.z * (double)x.z + (double)x.w * (double)x.w);
#pragma unroll
        for (int d = 16; d >= 1; d >>= 1) acc += __shfl_xor(acc, d);   // hand-written: nmw::wave_sum<16> changes prep_kernel<0>'s code
        const float nrm = (float)acc;
        const float sc = isA[q] ? -2.0f : 1.0f;
        if (MODE == 1 || (MODE == 2 && !isA[q])) {
            unsigned h0, l0, h1, l1, h2, l2, h3, l3;
            bf16_split(sc * x.x, h0, l0); bf16_split(sc * x.y, h1, l1);
            bf16_split(sc * x.z, h2, l2); bf16_split(sc * x.w, h3, l3);
            unsigned *dst = (isA[q] ? c.As : c.Bs) + (size_t)i * DIM;
            reinterpret_cast<uint2 *>(dst)[k4] = make_uint2(h0 | (h1 << 16), h2 | (h3 << 16));
            reinterpret_cast<uint2 *>(dst + 64)[k4] = make_uint2(l0 | (l1 << 16), l2 | (l3 << 16));
        }
        float res = 0.f;
        if (MODE == 2) {
            const unsigned b0 = f16_bits(sc * x.x), b1 = f16_bits(sc * x.y), b2 = f16_bits(sc * x.z), b3 = f16_bits(sc * x.w);
            unsigned *dst = (isA[q] ? c.Ah : c.Bh) + (size_t)i * (DIM / 2);
            reinterpret_cast<uint2 *>(dst)[k4] = make_uint2(b0 | (b1 << 16), b2 | (b3 << 16));
            // residual of what the image holds: x - x_h is exact in binary32 (x_h is x rounded to fewer bits; the scaling
            // by -2 and back is exact). An infinite x_h (|2 x| beyond the fp16 range) gives an infinite residual: such
            // rows lie outside the coarse pass's domain anyway (F16_NORM_LIMIT) and go to the bf16x3 pass.
            const float inv = isA[q] ? -0.5f : 1.0f;
            const float e0 = x.x - inv * f16_value(b0), e1 = x.y - inv * f16_value(b1);
            const float e2 = x.z - inv * f16_value(b2), e3 = x.w - inv * f16_value(b3);
            res = (e0 * e0 + e1 * e1) + (e2 * e2 + e3 * e3);
            res = nmw::wave_sum<16>(res);
            // upper bound of the residual's 2-norm: the 131 binary32 roundings above cost < 1e-5 relative, squares that
            // underflow < 1e-18 absolute
            res = __builtin_sqrtf(res) * 1.00002f + 1e-18f;
        }
        if (k4 == 0) {
            (isA[q] ? c.na : c.nb)[i] = nrm;
            if (MODE == 2) (isA[q] ? c.ra : c.rb)[i] = res;
            if (MODE && !isA[q]) {
                unsigned h, m, l;
                bf16_three(nrm, h, m, l);
                c.nbslot[i] = (nrm < 3.0e38f) ? make_uint4(h | (m << 16), l | (BF16_ONE << 16), BF16_ONE | (BF16_ONE << 16), 0u)
                                              : make_uint4(BF16_BIG, BF16_ONE << 16, BF16_ONE | (BF16_ONE << 16), 0u);
            }
        }
    }
}

// max_j ||b_j||^2 of every pair (one workgroup per pair): tightens the error bound of match_finalize_kernel. Two-stage
// screen (c.rb set): also the largest candidate residual norm, into the next float.
__global__ __launch_bounds__(1024) void nbmax_kernel(MatchBatch bt)
{
    __shared__ float s[32];
    const MatchPair &c = bt.p[blockIdx.x];
    const int nB = pair_nB(c);
    if (c.d_plan && threadIdx.x >= 960) {
        // device-sized call: the last wave makes the work plan for the real sizes (make_plan_on: the same function the host
        // runs for the host-sized entries), its lanes sharing the slot count, while the others reduce the norms
        const int lane = threadIdx.x & 63;
        const MatchPlan p = make_plan_on(pair_nA(c), nB, bt.n_cu, bt.n_xcd, lane, 64, [](int v) { return nmw::wave_max(v); });
        if (lane == 0) *c.d_plan = p;
    }
    // +inf as soon as one candidate norm is not a finite number below NORM_LIMIT (fmax would drop a NaN): the finalize
    // pass then sends EVERY row of the pair to the exact fallback, which is the reference's own scan
    // (eight loads of either array in flight per thread: the kernel is ONE workgroup per pair, i.e. a chain of memory round trips;
    // with one element per trip it took 9 us of a 127 us single-pair match)
    float m = 0.f, mr = 0.f;
    for (int i0 = threadIdx.x; i0 < nB; i0 += 8 * 1024) {
        float v[8], e[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int i = i0 + k * 1024;
            v[k] = (i < nB) ? c.nb[i] : 0.f;
            e[k] = (c.rb && i < nB) ? c.rb[i] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            m = (v[k] < NORM_LIMIT) ? __builtin_fmaxf(m, v[k]) : __builtin_inff();
            mr = (e[k] < NORM_LIMIT) ? __builtin_fmaxf(mr, e[k]) : __builtin_inff();
        }
    }
#pragma unroll                                              // hand-written: two nmw::wave_max change nbmax_kernel's code
    for (int d = 32; d >= 1; d >>= 1) { m = __builtin_fmaxf(m, __shfl_xor(m, d)); mr = __builtin_fmaxf(mr, __shfl_xor(mr, d)); }
    if ((threadIdx.x & 63) == 0) { s[threadIdx.x >> 6] = m; s[16 + (threadIdx.x >> 6)] = mr; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 16; ++w) { m = __builtin_fmaxf(m, s[w]); mr = __builtin_fmaxf(mr, s[16 + w]); }
        c.nbmax[0] = m;
        c.nbmax[1] = mr;
    }
}

// grid = G persistent workgroups (see MatchPlan), 512 threads = 8 waves (2 per SIMD). Wave w owns queries i0 + 32 w .. +31
// of the current query block with their MFMA fragments resident in VGPRs; candidate tiles of 128 rows stream through a
// double-buffered LDS image (row pitch KP). Dynamic LDS: 2 * TILE_C * KP floats.
// MFMA orientation: rows (accumulator registers) = candidates, columns (lanes) = queries, so every lane scans its own
// query's candidates in increasing index order and the running best/second-best never crosses lanes in the loop.
//
// What the instruction stream is built around (measured on MI355X, profiles/r02_mfma_*_microbench.txt): the fp32 MFMA
// shares the SIMD's vector datapath with the VALU -- every VALU instruction of either wave of a SIMD takes ~4-5 cycles
// away from the MFMAs (a bare 32x32x2 loop runs 154 TFLOP/s at 2.39 GHz; 2 VALU per MFMA cut it to 121) -- and an LDS
// operand read that is waited for right after its issue stalls the wave for the LDS latency every 4 MFMAs. So:
//   * staging uses raw buffer loads (the SRD's range check zero-fills rows >= nB: no compares, no address arithmetic
//     beyond one per-lane offset; the tile advances through the scalar offset) and the norms array is padded with +inf;
//   * the candidate fragments of k-group t+1 are requested before the MFMAs of k-group t;
//   * selection stays branch-free at 4 VALU instructions per value (Top3). A threshold test per value (one v_cmp +
//     wave vote + scalar branch, inserting only values below the running third best) was measured SLOWER (315 vs 298 us):
//     a segment restarts its triple every ~2 300 candidates, so ~30 % of the values still take the insertion and the 32
//     branches per group cost more than they save; staggering the two waves of a SIMD by half a tile changed nothing.
__device__ __forceinline__ void mfma_half(f32x16 &acc0, f32x16 &acc1, const float *rowp, const float *normp,
                                          const float4 (&qf)[16], float nq)
{
    mfma_kgroups<0, 16, true>(acc0, acc1, rowp, normp, qf, nq);
}

// The bf16x3 screen: the same two 32 x 32 accumulators from v_mfma_f32_32x32x16_bf16 on the SPLIT operands
//   a = a_h + a_l + r_a,  b = b_h + b_l + r_b   (bf16 pieces, |r| <= 2^-16 |x|):   a.b ~ a_h.b_h + a_h.b_l + a_l.b_h
// -- 3 x 8 instructions of 32 cycles per accumulator instead of 64 fp32 instructions of 64 cycles (5.3x fewer MFMA
// cycles), plus one instruction whose k-slots carry the norms as exact sums of three bf16 each. rowp = this lane's
// candidate row of group 0 at its k offset (8 h bf16 = 4 h dwords); a row is [hi: 64 dwords | lo: 64 dwords | slot: 4].
// qf[s] / qf[8 + s] = the query's hi / lo pieces of k-step s (k = 16 s + 8 h ..+7), already scaled by -2.
// The value differs from the exact distance by at most MatchBatch::err_coeff (sqrt na + sqrt nb)^2.
#define NM_MFMA "v_mfma_f32_32x32x16_bf16 "
// One k-step (k = 16 T .. 16 T + 15) of both accumulators: 6 MFMAs, and -- SELECT -- between them the insertion of four
// values of the PREVIOUS 64-candidate group (p0..p3 = its accumulator registers 4 T .. 4 T + 3, slots E0 .. E0 + 3) into
// that group's running key triple (g1 <= g2 <= g3): v_and_or (key), v_med3, v_med3, v_min per value, two or three
// between consecutive MFMAs. Unlike the fp32 MFMA, the bf16 MFMA leaves the SIMD's VALU port free while it runs
// (MI355X_MICROARCH.md, "instructions hidden per MFMA gap"), so the selection of one group costs nothing while the next
// group's products are formed; with the selection AFTER the MFMAs (as in the fp32 kernel) the two waves of a SIMD ran in
// lockstep, their selections coincided, and the MFMA pipe idled 49 % of the time (profiles/r02_j_*).
template <bool SELECT, int E0>
__device__ __forceinline__ void bf16_kstep(f32x16 &acc0, f32x16 &acc1, const u32x4 h0, const u32x4 l0, const u32x4 h1,
                                           const u32x4 l1, const u32x4 qh, const u32x4 ql, float p0, float p1, float p2,
                                           float p3, int &g1, int &g2, int &g3)
{
    if (SELECT) {
        int k;
        const int mask = ~((1 << KEY_SLOT_BITS) - 1);
        asm volatile(NM_MFMA "%0, %6, %10, %0\n\t"
                     "v_and_or_b32 %5, %12, %16, %17\n\t"
                     "v_med3_i32 %4, %3, %4, %5\n\t"
                     "v_med3_i32 %3, %2, %3, %5\n\t"
                     NM_MFMA "%1, %8, %10, %1\n\t"
                     "v_min_i32 %2, %2, %5\n\t"
                     "v_and_or_b32 %5, %13, %16, %18\n\t"
                     "v_med3_i32 %4, %3, %4, %5\n\t"
                     NM_MFMA "%0, %6, %11, %0\n\t"
                     "v_med3_i32 %3, %2, %3, %5\n\t"
                     "v_min_i32 %2, %2, %5\n\t"
                     "v_and_or_b32 %5, %14, %16, %19\n\t"
                     NM_MFMA "%1, %8, %11, %1\n\t"
                     "v_med3_i32 %4, %3, %4, %5\n\t"
                     "v_med3_i32 %3, %2, %3, %5\n\t"
                     "v_min_i32 %2, %2, %5\n\t"
                     NM_MFMA "%0, %7, %10, %0\n\t"
                     "v_and_or_b32 %5, %15, %16, %20\n\t"
                     "v_med3_i32 %4, %3, %4, %5\n\t"
                     "v_med3_i32 %3, %2, %3, %5\n\t"
                     NM_MFMA "%1, %9, %10, %1\n\t"
                     "v_min_i32 %2, %2, %5"
                     : "+v"(acc0), "+v"(acc1), "+v"(g1), "+v"(g2), "+v"(g3), "=&v"(k)
                     : "v"(h0), "v"(l0), "v"(h1), "v"(l1), "v"(qh), "v"(ql), "v"(p0), "v"(p1), "v"(p2), "v"(p3), "s"(mask),
                       "n"(E0), "n"(E0 + 1), "n"(E0 + 2), "n"(E0 + 3)
                     : "memory");
    } else {
        asm volatile(NM_MFMA "%0, %2, %6, %0\n\t" NM_MFMA "%1, %4, %6, %1\n\t"
                     NM_MFMA "%0, %2, %7, %0\n\t" NM_MFMA "%1, %4, %7, %1\n\t"
                     NM_MFMA "%0, %3, %6, %0\n\t" NM_MFMA "%1, %5, %6, %1"
                     : "+v"(acc0), "+v"(acc1)
                     : "v"(h0), "v"(l0), "v"(h1), "v"(l1), "v"(qh), "v"(ql)
                     : "memory");
    }
}

// (acc0, acc1) <- the 64-candidate group at rowp; SELECT: the previous group's accumulators (prev0, prev1) are folded into
// the key triple (g1, g2, g3) meanwhile. The group's values may be read by the VALU 10 wait states after the last MFMA
// (8-pass XDL op): the next call's first VALU instruction comes after two more MFMAs and the explicit s_nop below.
template <bool SELECT>
__device__ __forceinline__ void mfma_half_bf16(f32x16 &acc0, f32x16 &acc1, const f32x16 &prev0, const f32x16 &prev1,
                                               const char *tb, const unsigned (&foff)[8], const char *slotp,
                                               const u32x4 (&qf)[16], const u32x4 qslot, int &g1, int &g2, int &g3)
{
    // tb = this lane's candidate row of group 0 in the tile image (512-byte rows, 16-byte chunks XOR-swizzled by row & 15,
    // see bf16 staging in match_top2_kernel); foff[t] = byte offset of the lane's hi chunk of k-step t; lo = + 256;
    // group 1 = + 32 rows
    constexpr int G1 = 32 * 512;
    u32x4 h0 = *reinterpret_cast<const u32x4 *>(tb + foff[0]), l0 = *reinterpret_cast<const u32x4 *>(tb + 256 + foff[0]);
    u32x4 h1 = *reinterpret_cast<const u32x4 *>(tb + G1 + foff[0]), l1 = *reinterpret_cast<const u32x4 *>(tb + G1 + 256 + foff[0]);
    const u32x4 s0 = *reinterpret_cast<const u32x4 *>(slotp), s1 = *reinterpret_cast<const u32x4 *>(slotp + 32 * 16);
    asm volatile(NM_MFMA "%0, %2, %4, 0\n\t" NM_MFMA "%1, %3, %4, 0\n\ts_nop 15\n\ts_nop 3"
                 : "=&v"(acc0), "=&v"(acc1) : "v"(s0), "v"(s1), "v"(qslot) : "memory");
#define NM_KSTEP(T)                                                                                                      \
    {                                                                                                                    \
        u32x4 nh0 = h0, nl0 = l0, nh1 = h1, nl1 = l1;                                                                    \
        if (T + 1 < 8) { /* next k-step's fragments fly during this step's 6 MFMAs */                                    \
            nh0 = *reinterpret_cast<const u32x4 *>(tb + foff[(T + 1) & 7]);                                              \
            nl0 = *reinterpret_cast<const u32x4 *>(tb + 256 + foff[(T + 1) & 7]);                                        \
            nh1 = *reinterpret_cast<const u32x4 *>(tb + G1 + foff[(T + 1) & 7]);                                         \
            nl1 = *reinterpret_cast<const u32x4 *>(tb + G1 + 256 + foff[(T + 1) & 7]);                                   \
        }                                                                                                                \
        const f32x16 &pv = (T < 4) ? prev0 : prev1;                                                                      \
        bf16_kstep<SELECT, 4 * T>(acc0, acc1, h0, l0, h1, l1, qf[T], qf[8 + T], pv[(4 * T) & 15], pv[(4 * T + 1) & 15],    \
                                  pv[(4 * T + 2) & 15], pv[(4 * T + 3) & 15], g1, g2, g3);                                \
        h0 = nh0; l0 = nl0; h1 = nh1; l1 = nl1;                                                                          \
    }
    NM_KSTEP(0) NM_KSTEP(1) NM_KSTEP(2) NM_KSTEP(3) NM_KSTEP(4) NM_KSTEP(5) NM_KSTEP(6) NM_KSTEP(7)
#undef NM_KSTEP
}
#undef NM_MFMA

// The coarse pass of the two-stage screen: ONE product per k (v_mfma_f32_32x32x16_f16 on the fp16 images of -2 A and B:
// 8 + 1 MFMAs per accumulator and 64-candidate group instead of 24 + 1), norms through the same bf16 k-slot instruction.
// Its value differs from the exact distance by the fp16 rounding of the operands, which match_finalize_kernel<1> bounds
// per row from the residual norms (prep_kernel<2>); the rows it cannot prove are screened again by the bf16x3 kernel.
// tb = this lane's candidate row of group 0 in the tile image (256-byte rows, 16-byte chunks XOR-swizzled by row & 15);
// foff[t] = byte offset of the lane's chunk of k-step t; group 1 = + 32 rows. qf[s] = the query's k-step s (k = 16 s + 8 h ..+7).
#ifdef NM_STUB_NOMFMA                           // diagnostic builds only (see f16_kstep): the instruction becomes an assembler comment
#define NM_MFMA_H "; v_mfma_f32_32x32x16_f16 "
#else
#define NM_MFMA_H "v_mfma_f32_32x32x16_f16 "
#endif
// The coarse pass folds once per TILE ITERATION: the keys of the two groups selected in it (2 n - 1, selected beside the first
// group of tile n, and 2 n) share one pair of running keys, told apart by a sixth slot bit; 2^-17 instead of 2^-18 of a
// value is dropped, which the finalize constants cover.
constexpr int COARSE_SLOT_BITS = 6;
// Selection in the coarse pass keeps the TWO smallest keys of a 64-candidate group (v_and_or, v_med3, v_min: three
// instructions per value instead of four -- the selection is this kernel's largest single cost) and hands the second
// one to the running triple a second time as the group's third: every value of the group it did not keep is >= it, which
// is all the third key is for (the lower bound `rest` of the finalize pass). The price: a segment whose two best
// candidates share a group reports third == second and its row goes to the second pass (~0.5 % of the rows more).
// Diagnostic builds only (tools/build_variant.py stub_X nm_match_screen.hip -DNM_STUB_X=1; tools/gpu_coarse_ab.sh): NM_STUB_NOSELECT drops
// the selection instructions, NM_STUB_NOMFMA the matrix instructions, NM_STUB_NODMA the tile requests of the ring. Round 6, 16-pair
// launch, one box, three alternations, us per pair: whole 36.8 | no selection 31.7 | no MFMA 22.3 | no requests 33.6 | neither
// selection nor MFMA 16.2 | none of the three 12.6 (fragment reads, norm slots, barriers, fold, publication). The MFMAs' share is
// their own pipe time (37.8 GFLOP at the 2.5 PFLOP/s peak = 15.1 us per pair): NOTHING else of an iteration runs under them -- the
// per-tile barrier keeps the eight waves in the same phase, so a SIMD's two waves want the matrix pipe together and stall together.
// profiles/r06_y_coarse_stubs.txt. No stub executes in the product.
template <bool SELECT_, int E0>
__device__ __forceinline__ void f16_kstep(f32x16 &acc0, f32x16 &acc1, const u32x4 h0, const u32x4 h1, const u32x4 qh,
                                          float p0, float p1, float p2, float p3, int &g1, int &g2)
{
#ifdef NM_STUB_NOSELECT
    constexpr bool SELECT = false;
#else
    constexpr bool SELECT = SELECT_;
#endif
    if (SELECT) {
        int k;
        const int mask = ~((1 << COARSE_SLOT_BITS) - 1);
        asm volatile(NM_MFMA_H "%0, %5, %7, %0\n\t"
                     "v_and_or_b32 %4, %8, %12, %13\n\t"
                     "v_med3_i32 %3, %2, %3, %4\n\t"
                     "v_min_i32 %2, %2, %4\n\t"
                     "v_and_or_b32 %4, %9, %12, %14\n\t"
                     "v_med3_i32 %3, %2, %3, %4\n\t"
                     "v_min_i32 %2, %2, %4\n\t"
                     NM_MFMA_H "%1, %6, %7, %1\n\t"
                     "v_and_or_b32 %4, %10, %12, %15\n\t"
                     "v_med3_i32 %3, %2, %3, %4\n\t"
                     "v_min_i32 %2, %2, %4\n\t"
                     "v_and_or_b32 %4, %11, %12, %16\n\t"
                     "v_med3_i32 %3, %2, %3, %4\n\t"
                     "v_min_i32 %2, %2, %4"
                     : "+v"(acc0), "+v"(acc1), "+v"(g1), "+v"(g2), "=&v"(k)
                     : "v"(h0), "v"(h1), "v"(qh), "v"(p0), "v"(p1), "v"(p2), "v"(p3), "s"(mask),
                       "n"(E0), "n"(E0 + 1), "n"(E0 + 2), "n"(E0 + 3)
                     : "memory");
    } else {
        asm volatile(NM_MFMA_H "%0, %2, %4, %0\n\t" NM_MFMA_H "%1, %3, %4, %1"
                     : "+v"(acc0), "+v"(acc1) : "v"(h0), "v"(h1), "v"(qh) : "memory");
    }
}

// The coarse pass is software-pipelined over HALF groups (4 k-steps of both accumulators): with two MFMAs per k-step a
// k-step lasts ~64-128 cycles, less than an LDS read under load, so the fragments of a whole half group (8 x 16 bytes per
// lane) are requested while the previous half group is multiplied.
// fr[2 t], fr[2 t + 1] = the lane's chunks of k-step KS0 + t for the two accumulators.
// (Round 6, measured: the fragment reads are NOT what the kernel waits for -- a diagnostic build that issues HALF of them (the
// second accumulator reusing the first one's chunk; what 64 queries per wave would save) runs the 16-pair launch in 593.4-595.4
// against 600.2-601.0 us, three alternations on one box: -1.2 %. profiles/r06_y_coarse_half_fragment_reads.txt)
template <int KS0>
__device__ __forceinline__ void f16_fetch(u32x4 (&fr)[8], const char *tb, const unsigned (&foff)[8])
{
    constexpr int G1 = 32 * 256;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        fr[2 * t] = *reinterpret_cast<const u32x4 *>(tb + foff[KS0 + t]);
        fr[2 * t + 1] = *reinterpret_cast<const u32x4 *>(tb + G1 + foff[KS0 + t]);
    }
}
// the norms of a 64-candidate group start its two accumulators (bf16 k-slots, as in the bf16x3 kernel)
__device__ __forceinline__ void f16_slots(f32x16 &acc0, f32x16 &acc1, const char *slotp, const u32x4 qslot)
{
    const u32x4 s0 = *reinterpret_cast<const u32x4 *>(slotp), s1 = *reinterpret_cast<const u32x4 *>(slotp + 32 * 16);
    // No wait states behind them: the next instruction on acc0 is an MFMA that accumulates into exactly the registers this
    // one writes (the XDL pipe interlocks that case, whatever the operand type), and the first VALU instruction that reads
    // an accumulator reads one of the PREVIOUS group, whose last MFMA is more than 16 instructions back.
    asm volatile("v_mfma_f32_32x32x16_bf16 %0, %2, %4, 0\n\tv_mfma_f32_32x32x16_bf16 %1, %3, %4, 0"
                 : "=&v"(acc0), "=&v"(acc1) : "v"(s0), "v"(s1), "v"(qslot) : "memory");
}
// k-steps KS0 .. KS0 + 3 of (acc0, acc1); SELECT: the 16 values of pv (one accumulator of the PREVIOUS group; slots
// 4 KS0 .. 4 KS0 + 15 of that group) are folded into the key triple meanwhile
template <bool SELECT, int KS0, int EB = 0>        // EB: slot base of the selected group (0: group 2 n - 1, 32: group 2 n)
__device__ __forceinline__ void f16_half(f32x16 &acc0, f32x16 &acc1, const f32x16 &pv, const u32x4 (&fr)[8],
                                         const u32x4 (&qf)[16], int &g1, int &g2)
{
    f16_kstep<SELECT, EB + 4 * KS0>(acc0, acc1, fr[0], fr[1], qf[KS0], pv[0], pv[1], pv[2], pv[3], g1, g2);
    f16_kstep<SELECT, EB + 4 * KS0 + 4>(acc0, acc1, fr[2], fr[3], qf[KS0 + 1], pv[4], pv[5], pv[6], pv[7], g1, g2);
    f16_kstep<SELECT, EB + 4 * KS0 + 8>(acc0, acc1, fr[4], fr[5], qf[KS0 + 2], pv[8], pv[9], pv[10], pv[11], g1, g2);
    f16_kstep<SELECT, EB + 4 * KS0 + 12>(acc0, acc1, fr[6], fr[7], qf[KS0 + 3], pv[12], pv[13], pv[14], pv[15], g1, g2);
}
#undef NM_MFMA_H

// SCR 0 (fp32 screen): A, B are the fp32 descriptor rows. SCR 1 (bf16x3): A, B are the split images written by prep_kernel
// (same 512-byte rows) and nbslot replaces nb.
// Device-sized launches (d_plan != NULL): nA_arg / nB_arg are the capacities, the real sizes and the plan made for them
// (nbmax_kernel) are read from device memory, and the grid is one workgroup per CU of which the first plan.G work.
template <int SCR>
__device__ __forceinline__ void match_top2_body(const float *__restrict__ A, int nA_arg,
                                                const float *__restrict__ B, int nB_arg,
                                                const float *__restrict__ na, const float *__restrict__ nb,
                                                const uint4 *__restrict__ nbslot,
                                                MatchPlan plan_arg, float4 *__restrict__ partial,
                                                float *__restrict__ partial3,
                                                const int *__restrict__ d_nA, const int *__restrict__ d_nB,
                                                const MatchPlan *__restrict__ d_plan, const int wg)
{
    static_assert(SCR == 0 || SCR == 1, "the coarse pass of the two-stage screen has its own kernel (match_coarse_kernel)");
    constexpr bool BF16 = SCR == 1, DMA = SCR != 0;
    constexpr int ROWB = DIM * 4;                         // bytes per row of the A / B images these screens read
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int srow = tid >> 5, scol = (tid & 31) * 4;     // staging coordinates: 16 rows x 32 float4 per pass
    int nA = nA_arg, nB = nB_arg;
    MatchPlan plan = plan_arg;
    if (d_plan) {                                         // uniform: scalar loads
        if (d_nA) nA = min(max(*d_nA, 0), nA_arg);
        if (d_nB) nB = min(max(*d_nB, 0), nB_arg);
        plan = *d_plan;
        if (nA <= 0 || nB <= 0 || wg >= plan.G) return;   // an empty set is a no-op for the pair, as in the reference
    }
    if (wg >= plan.G) return;                             // (group launches are sized for the chip, not for the plan)
    const int S = plan.S;
    const int xg = wg % plan.X, vg = wg / plan.X;         // XCD group (blocks b, b + X share an XCD) and position in it
    const PlanGroup grp = plan_group(plan, xg);
    const unit_t u_begin = group_begin(grp, vg), u_end = group_begin(grp, vg + 1);
    SegIter it;
    it.init(u_begin, u_end);

    // range-checked views: rows >= nB / nA read as zeros (the host refuses sets of 2^22 rows or more)
    const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(B), 0, nB * ROWB, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(A), 0, nA * ROWB, 0x00020000);
    const int voff = (srow * DIM + scol) * 4;

    u32x4 st[8];
    float stn = 0.f;
    uint4 sts = make_uint4(0u, 0u, 0u, 0u);
    auto stage_load = [&](int tile) {                     // candidates tile*128 .. +127 -> registers
        const int jb = tile * TILE_C;
#pragma unroll
        for (int it = 0; it < 8; ++it) st[it] = __builtin_amdgcn_raw_buffer_load_b128(rsB, voff, (jb + 16 * it) * (DIM * 4), 0);
        if (tid < TILE_C) {                               // padded up to T * 128 by prep_kernel
            if (DMA) sts = nbslot[jb + tid];
            else stn = nb[jb + tid];
        }
    };
    auto stage_write = [&](float *buf) {
#pragma unroll
        for (int it = 0; it < 8; ++it) *reinterpret_cast<u32x4 *>(&buf[(srow + 16 * it) * KP + scol]) = st[it];
        if (tid < TILE_C) {                               // augmented k-pair / k-slot
            if (DMA) *reinterpret_cast<uint4 *>(&buf[tid * KP + DIM]) = sts;
            else *reinterpret_cast<float2 *>(&buf[tid * KP + DIM]) = make_float2(stn, 1.0f);
        }
    };

    // bf16x3 screen: the candidate tiles go global -> LDS directly (buffer_load ... lds: no staging registers, no
    // ds_write pass). One wave-instruction lands 1 KiB = two 512-byte rows, lane-linear, so the tile image has NO row
    // padding; bank conflicts are avoided by XOR-swizzling the 16-byte chunks of a row with (row & 15) -- applied to the
    // per-lane SOURCE address here and to the fragment reads' offsets (foff), the same involution on both sides. The
    // 16-byte norm slots live in their own 2 KiB per buffer behind the two 64 KiB images (same total as the padded layout).
    constexpr int IMG = TILE_C * ROWB, SLOT0 = 2 * IMG, SLOTB = TILE_C * 16;
    constexpr int DMA_N = IMG / (8 * 1024);               // wave-instructions per wave and tile
    char *const ldsb = reinterpret_cast<char *>(lds);
    unsigned foff[8], dvoff[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        foff[t] = (unsigned)(((2 * t + h) ^ (r & 15)) << 4);
        const int p = lane & 31, key = (2 * t + (lane >> 5)) & 15;        // wave-instruction t of a wave covers rows 2 (8 wave + t) + (lane >> 5)
        dvoff[t] = (unsigned)((lane >> 5) * (DIM * 4) + (((p & 16) | ((p & 15) ^ key)) << 4));
    }
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);      // scalar for the compiler: M0 and the scalar offset depend on it
    auto dma_tile = [&](int tile, int b) {
#pragma unroll
        for (int t = 0; t < DMA_N; ++t) {
            typedef __attribute__((address_space(3))) void lds_void;
            lds_void *dst = (lds_void *)(ldsb + b * IMG + (wave_u * DMA_N + t) * 1024);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, dst, 16, (int)dvoff[t],
                                                     (tile * TILE_C + (1024 / ROWB) * (wave_u * DMA_N + t)) * ROWB, 0, 0);
        }
    };

    unit_t u;
    while (it.next(plan, grp, u)) {
        int pc, qbl, tt, Lc;
        plan_locate(plan, grp, u, pc, qbl, tt, Lc);
        const int qb = grp.q0 + qbl, t0 = pc * plan.Tc + tt;
        const int ntiles = min(Lc - tt, (int)(u_end - u));
        const int i0 = qb * QB;
        const int c0 = t0 * TILE_C;

        // ---- segment prologue: the first candidate tile is requested first (its latency hides behind the query staging),
        //      queries -> LDS (coalesced) -> per-lane MFMA fragments in VGPRs ----
        if (DMA) { if (tid < TILE_C) sts = nbslot[t0 * TILE_C + tid]; }
        else stage_load(t0);
#pragma unroll 4
        for (int it = 0; it < QB / 16; ++it) {
            const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rsA, voff, (i0 + 16 * it) * (DIM * 4), 0);
            *reinterpret_cast<u32x4 *>(&lds[(srow + 16 * it) * KP + scol]) = v;
        }
        __syncthreads();
        float4 qf[16];
        u32x4 qw[16];
        const int qi = i0 + wave * 32 + r;
#pragma unroll
        for (int t = 0; t < 16; ++t) {      // the -2 of  |a|^2 + |b|^2 - 2 a.b  rides on the query fragments (once per segment)
            if (BF16) {              // hi pieces of k-steps 0..7, then the lo pieces (prep_kernel applied the -2)
                qw[t] = *reinterpret_cast<const u32x4 *>(&lds[(wave * 32 + r) * KP + 8 * t + 4 * h]);
            } else {
                const float4 v = *reinterpret_cast<const float4 *>(&lds[(wave * 32 + r) * KP + 8 * t + 4 * h]);
                qf[t] = make_float4(-2.f * v.x, -2.f * v.y, -2.f * v.z, -2.f * v.w);
            }
        }
        const float nav = (qi < nA) ? na[qi] : 0.f;
        const float nq = (h == 0) ? 1.0f : nav;
        u32x4 qslot = {0u, 0u, 0u, 0u};     // k-slots (1, 1, 1, na_h, na_m, na_l, 0, 0) on the lanes that hold k = 0..7
        if (DMA && h == 0) {
            unsigned nh, nm, nl;
            bf16_three(nav, nh, nm, nl);
            qslot = (u32x4){BF16_ONE | (BF16_ONE << 16), BF16_ONE | (nh << 16), nm | (nl << 16), 0u};
        }
        __syncthreads();
        if (DMA) {
            dma_tile(t0, 0);
            if (tid < TILE_C) *reinterpret_cast<uint4 *>(ldsb + SLOT0 + tid * 16) = sts;
            // A wave's LDS-DMA rows are read by all 8 waves after the barrier: every wave must have drained ITS transfers
            // before it arrives. hipcc emits this wait today, but the workgroup-scope fence model does not oblige it to
            // (LDS-DMA is tracked per wave): a half-landed tile would make the screen miss a true neighbour and the finalize
            // pass would then "prove" a wrong row. Explicit, so that no toolchain change can move it.
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        } else {
            stage_write(lds);
        }
        __syncthreads();

        Top3 best;
        best.k1 = best.k2 = best.k3 = KEY_INF; best.t1 = best.t2 = 0;

        // A wave multiplies its 32 queries with 64 candidates at a time (two 32 x 32 accumulators), then folds the 32
        // values each lane holds into its running triple. Within a lane the candidate index increases with (tile, half, g, e).
        f32x16 a0, a1;
        if (DMA) {
            // software pipeline over the 64-candidate groups: the MFMAs of group i run while group i - 1 is selected
            f32x16 b0, b1;
            const bool wave_live = __builtin_amdgcn_readfirstlane(i0 + wave * 32) < nA;
            auto fold = [&](int g1, int g2, int g3, int tag) {
                if (__any(g1 < best.k3)) {
                    top3_merge(best, g1, tag);
                    top3_merge(best, g2, tag);
                    top3_merge(best, g3, tag);
                }
            };
            // tile n + 1 starts landing in the other buffer at the START of tile n (every wave left that buffer before the
            // last barrier); the barrier at the end of tile n waits for it (vmcnt(0), emitted by the compiler)
            for (int n = 0; n < ntiles; ++n) {
                const int b = n & 1;
                const char *tb = ldsb + b * IMG + r * ROWB;
                const char *sp = ldsb + SLOT0 + b * SLOTB + r * 16;
                if (n + 1 < ntiles) {
                    if (tid < TILE_C) sts = nbslot[(t0 + n + 1) * TILE_C + tid];
                    dma_tile(t0 + n + 1, b ^ 1);
                }
                int g1 = KEY_INF, g2 = KEY_INF, g3 = KEY_INF;
                if (!wave_live) {
                    // none of this wave's 32 queries exists (the second pass of the two-stage screen lists a few dozen rows
                    // per 256-row block): it only moves its share of the tiles
                } else if (n == 0) {
                    mfma_half_bf16<false>(a0, a1, b0, b1, tb, foff, sp, qw, qslot, g1, g2, g3);
                } else {
                    mfma_half_bf16<true>(a0, a1, b0, b1, tb, foff, sp, qw, qslot, g1, g2, g3);
                    fold(g1, g2, g3, 2 * n - 1);
                }
                g1 = g2 = g3 = KEY_INF;
                if (wave_live) {
                    mfma_half_bf16<true>(b0, b1, a0, a1, tb + 64 * ROWB, foff, sp + 64 * 16, qw, qslot, g1, g2, g3);
                    fold(g1, g2, g3, 2 * n);
                }
                if (n + 1 < ntiles && tid < TILE_C) *reinterpret_cast<uint4 *>(ldsb + SLOT0 + (b ^ 1) * SLOTB + tid * 16) = sts;
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // tile n + 1 has landed (this wave's share): see the prologue
                __syncthreads();
            }
            if (wave_live) {
                asm volatile("s_nop 15\n\ts_nop 3" : "+v"(b0), "+v"(b1));
                select_half(b0, b1, best, 2 * ntiles - 1);
            }
        } else
        for (int n = 0; n < ntiles; ++n) {
            const float *buf = lds + (n & 1) * (TILE_C * KP);
            const float *rowp = buf + r * KP + 4 * h, *normp = buf + r * KP + DIM + h;
            if (n + 1 < ntiles) stage_load(t0 + n + 1);
            mfma_half(a0, a1, rowp, normp, qf, nq);
            select_half(a0, a1, best, 2 * n);
            mfma_half(a0, a1, rowp + 64 * KP, normp + 64 * KP, qf, nq);
            select_half(a0, a1, best, 2 * n + 1);
            if (n + 1 < ntiles) stage_write(lds + ((n + 1) & 1) * (TILE_C * KP));
            __syncthreads();
        }

        segment_publish(best, plan, grp, pc, qbl, vg, tt + ntiles == Lc, c0, h, qi, nA, S, partial, partial3);
        __syncthreads();                                  // the next segment's prologue reuses the LDS
    }
}

// The coarse pass of the two-stage screen as ONE stream of candidate tiles per workgroup. A workgroup's range is 2-3
// segments of ~8 tiles, and with one product per k a tile lasts ~2 us: the segment prologue of the kernels above (query
// rows, their norms and the first candidate tile requested one after the other, each global-memory latency exposed to all
// eight waves) cost as much as four tiles. Here
//   * the query block has its own 64 KiB LDS region, filled by LDS-DMA in the same swizzled row layout as the tiles;
//   * the NEXT segment's queries are requested as soon as every wave holds the current fragments (after the first barrier
//     of the segment), its first two candidate tiles as stream tiles g + 1, g + 2 of the ring below, its norms into
//     registers: a segment change is a barrier that is taken anyway, eight LDS reads and the publication of the previous
//     segment's result;
//   * the tile ring runs across segments: after the barrier of stream tile g (taken once every wave holds its last
//     fragments of g, after the third of the four half groups) tile g + 2 is requested into the buffer g just left.
// A segment that follows a one-tile segment (or starts the range) cannot have been requested ahead and takes the slow
// path: request, wait, barrier. LDS: 2 x 32 KiB tiles | 2 x 2 KiB norm slots | 64 KiB queries = 135 168 B.
// ONE launch per call: the workgroups are persistent over the PAIRS of the call too (every pair's plan is in device memory,
// nbmax_kernel), so the launch, the kernel-argument and plan loads and the drain of the slowest workgroup are paid once
// per call instead of once per pair (~9 us of fixed cost per pair beside ~40 us of tiles when each pair was a launch).
#ifndef NM_COARSE_CROSS
#define NM_COARSE_CROSS 1
#endif
#ifndef NM_COARSE_PRIO_LO
#define NM_COARSE_PRIO_LO 0
#endif
#ifndef NM_COARSE_PRIO_HI
#define NM_COARSE_PRIO_HI 2
#endif
#ifndef NM_COARSE_PRIO
#define NM_COARSE_PRIO 1
#endif
// Diagnostic builds only (tools/build_variant.py ... -DNM_COARSE_STAMPS=1, read by tools/kcoarse_stamps.py): s_memtime at eight
// points of a tile iteration, every wave of workgroup 0, the first 64 iterations. No stamp executes in the product.
#ifdef NM_COARSE_STAMPS
__device__ unsigned long long nm_coarse_stamps[8 * 64 * 8];
#define NM_STAMP(K)                                                                                                      \
    do {                                                                                                                 \
        __builtin_amdgcn_sched_barrier(0);                                                                               \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(stamp_t[K]) :: "memory");                              \
        __builtin_amdgcn_sched_barrier(0);                                                                               \
    } while (0)
#else
#define NM_STAMP(K) do { } while (0)
#endif
__global__ __launch_bounds__(512, 1) void match_coarse_kernel(MatchBatch bt)
{
    constexpr int ROWB = DIM * 2, IMG = TILE_C * ROWB, SLOT0 = 2 * IMG, SLOTB = TILE_C * 16, QREG = SLOT0 + 2 * SLOTB;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    char *const ldsb = reinterpret_cast<char *>(lds);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int wg = blockIdx.x;

    // LDS-DMA: one wave-instruction lands 1 KiB = four 256-byte rows, lane-linear; the 16-byte chunks of a row are XOR-swizzled
    // with (row & 15) on the SOURCE side here and in the fragment reads' offsets (foff). Wave-instruction t of a wave covers
    // rows 4 (N wave + t) + (lane >> 4), N = 4 (tile) or 8 (query block): row & 15 = (4 t + (lane >> 4)) & 15 either way.
    unsigned foff[8], dvoff[4];
#pragma unroll
    for (int t = 0; t < 8; ++t) foff[t] = (unsigned)(((2 * t + h) ^ (r & 15)) << 4);
#pragma unroll
    for (int t = 0; t < 4; ++t) dvoff[t] = (unsigned)((lane >> 4) * ROWB + (((lane & 15) ^ ((4 * t + (lane >> 4)) & 15)) << 4));
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    typedef __attribute__((address_space(3))) void lds_void;
    // Pair directory: sizes and plan of every pair of the call, read once by sixteen lanes (the device-memory latency of
    // the plan used to be exposed to all eight waves at every pair change) and kept in 1 KiB of LDS behind the query region.
    constexpr int DIR = QREG + QB * ROWB, DIR_STRIDE = 16, NAV = DIR + 1024;     // + 8 x 256 B of query norms
    static_assert(sizeof(MatchPlan) == 10 * sizeof(int) && DIR_STRIDE >= 12, "directory entry: nA, nB, the plan");
    int *const dir = reinterpret_cast<int *>(ldsb + DIR);
    if (tid < bt.n) {
        const MatchPair &c = bt.p[tid];
        const int *pl = reinterpret_cast<const int *>(c.d_plan);
        int *d = dir + tid * DIR_STRIDE;
        d[0] = pair_nA(c); d[1] = pair_nB(c);
#pragma unroll
        for (int k = 0; k < 10; ++k) d[2 + k] = pl[k];
    }
    __syncthreads();

    // What a workgroup needs of the pair a segment belongs to. The segments of ALL pairs of the call form one stream: the
    // segment after a pair's last one is the first of the next pair in which this workgroup has work, requested ahead like any
    // other (until round 5 every pair began with the slow path below: plan load, request, wait, barrier -- ~2 us of 41).
    struct PairCtx {
        int pq, nA, vg;
        MatchPlan plan;
        PlanGroup grp;
        unit_t u_end;
        SegIter it;
        __amdgpu_buffer_rsrc_t rsA, rsB, rsS, rsN;        // fp16 images of the queries / candidates, the candidates' norm k-slots,
        float4 *partial;                                  // the queries' norms
        float *partial3;
    };
    struct Seg { int pc, qbl, tt, Lc, qb, t0, ntiles; };
    // the first pair >= from in which this workgroup has a segment; u: the local unit where that segment starts
    auto open_pair = [&](int from, PairCtx &cx, unit_t &u) -> bool {
        for (int pq = from; pq < bt.n; ++pq) {
            const int *d = dir + pq * DIR_STRIDE;
            const int nA = __builtin_amdgcn_readfirstlane(d[0]), nB = __builtin_amdgcn_readfirstlane(d[1]);
            if (nA <= 0 || nB <= 0) continue;             // an empty set is a no-op for the pair, as in the reference
            MatchPlan plan;
            plan.qblocks = __builtin_amdgcn_readfirstlane(d[2]); plan.T = __builtin_amdgcn_readfirstlane(d[3]);
            plan.G = __builtin_amdgcn_readfirstlane(d[4]); plan.S = __builtin_amdgcn_readfirstlane(d[5]);
            plan.X = __builtin_amdgcn_readfirstlane(d[6]); plan.Gx = __builtin_amdgcn_readfirstlane(d[7]);
            plan.Tc = __builtin_amdgcn_readfirstlane(d[8]); plan.C = __builtin_amdgcn_readfirstlane(d[9]);
            plan.q_base = __builtin_amdgcn_readfirstlane(d[10]); plan.q_rem = __builtin_amdgcn_readfirstlane(d[11]);
            int xg, vg;
            if (bt.pair_xcd > 0) {                        // the pair lives on one XCD: its A and B images cross the fabric once
                if (pq % bt.pair_xcd != wg % bt.pair_xcd) continue;
                xg = 0; vg = wg / bt.pair_xcd;            // (the plan is a one-group plan: X = 1)
                if (vg >= plan.G) continue;
            } else {
                if (wg >= plan.G) continue;
                xg = wg % plan.X; vg = wg / plan.X;
            }
            const MatchPair &c = bt.p[pq];
            cx.pq = pq; cx.nA = nA; cx.plan = plan;
            cx.vg = vg;
            cx.grp = plan_group(plan, xg);
            cx.u_end = group_begin(cx.grp, cx.vg + 1);
            cx.it.init(group_begin(cx.grp, cx.vg), cx.u_end);
            cx.rsB = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned *>(c.Bh), 0, nB * ROWB, 0x00020000);
            cx.rsA = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned *>(c.Ah), 0, nA * ROWB, 0x00020000);
            // (prep_kernel pads the slots to whole tiles)
            cx.rsS = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint4 *>(c.nbslot), 0, plan.T * SLOTB, 0x00020000);
            cx.rsN = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(c.na), 0, nA * 4, 0x00020000);
            cx.partial = c.partial; cx.partial3 = c.partial3;
            if (cx.it.next(cx.plan, cx.grp, u)) return true;
        }
        return false;
    };
    // A tile = its 32 KiB image (four 1 KiB pieces per wave) and its 2 KiB of norm k-slots (one piece each from waves 0 and 1),
    // all by LDS-DMA. (Until round 5 the slots went through registers -- loaded when the tile was requested, written to LDS an
    // iteration later: the compiler carried them around the loop in a phi, and its copy on the back edge waited with vmcnt(0),
    // i.e. for the tile image requested a few hundred cycles earlier. Every iteration exposed a whole request latency:
    // ~900 of ~5 500 cycles, `tools/kcoarse_stamps.py`.)
    typedef __amdgpu_buffer_rsrc_t rsrc_t;
    auto dma_piece = [&](rsrc_t rsB, int tile, int b, int t) {
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, (lds_void *)(ldsb + b * IMG + (wave_u * 4 + t) * 1024), 16, (int)dvoff[t],
                                                 (tile * TILE_C + 4 * (wave_u * 4 + t)) * ROWB, 0, 0);
    };
    auto dma_slots = [&](rsrc_t rsS, int tile, int b) {
        if (wave_u < 2)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsS, (lds_void *)(ldsb + SLOT0 + b * SLOTB + wave_u * 1024), 16, lane * 16,
                                                     tile * SLOTB + wave_u * 1024, 0, 0);
    };
    // (Round 6, measured: a tile requested by FOUR of the eight waves, eight pieces each -- waves 0-3, or waves 4-7, the ones the
    // stamps show on the critical path -- is 0.8 % slower either way: 603-608 against 599 us per 16-pair launch, three alternations.
    // profiles/r06_zz_coarse_dma_waves.txt)
    auto dma_tile = [&](rsrc_t rsB, rsrc_t rsS, int tile, int b) {
#pragma unroll
        for (int t = 0; t < 4; ++t) dma_piece(rsB, tile, b, t);
        dma_slots(rsS, tile, b);
    };
    auto dma_queries = [&](rsrc_t rsA, int i0) {
#pragma unroll
        for (int t = 0; t < 8; ++t)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (lds_void *)(ldsb + QREG + (wave_u * 8 + t) * 1024), 16, (int)dvoff[t & 3],
                                                     (i0 + 4 * (wave_u * 8 + t)) * ROWB, 0, 0);
    };
    auto locate = [&](const PairCtx &cx, unit_t u) {
        Seg sg;
        plan_locate(cx.plan, cx.grp, u, sg.pc, sg.qbl, sg.tt, sg.Lc);
        sg.qb = cx.grp.q0 + sg.qbl; sg.t0 = sg.pc * cx.plan.Tc + sg.tt;
        sg.ntiles = min(sg.Lc - sg.tt, (int)(cx.u_end - u));
        return sg;
    };
    // the norms of a wave's 32 queries: 128 B of the wave's own 256-byte LDS slot, by LDS-DMA as well (rows >= nA read as 0) -- no
    // load of the tile loop returns into registers, so no wait of the compiler's can stand in it
    auto dma_norms = [&](rsrc_t rsN, int qb) {
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsN, (lds_void *)(ldsb + NAV + wave_u * 256), 4, r * 4, (qb * QB + wave_u * 32) * 4, 0, 0);
    };
    auto norm_read = [&]() { return *reinterpret_cast<const float *>(ldsb + NAV + wave * 256 + r * 4); };

    PairCtx pc_cur, pc_nxt;
    unit_t u;
#ifdef NM_COARSE_STAMPS
    int stamp_it = 0;
    unsigned long long stamp_t[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#endif
    if (!open_pair(0, pc_cur, u)) return;
    pc_nxt = pc_cur;
    Seg cur = locate(pc_cur, u);
    bool ahead = false;                                   // the current segment's queries and first tile(s) were requested ahead
    int g = 0;                                            // stream tile index of the current segment's first tile (its parity picks the buffer)
    u32x4 frA[8], frB[8];
    for (;;) {
        unit_t u_next = 0;
        bool have_next = pc_cur.it.next(pc_cur.plan, pc_cur.grp, u_next);
        bool cross = false, restart = false;              // the next segment is the first of another pair (restart: A/B builds only)
        if (!have_next && open_pair(pc_cur.pq + 1, pc_nxt, u_next)) {
            if (NM_COARSE_CROSS) have_next = cross = true;
            else restart = true;
        }
        // the descriptors the NEXT segment's requests go through, by value (a reference picked at run time sent the
        // contexts to scratch memory and every request through a waterfall loop)
        const rsrc_t nA_rs = cross ? pc_nxt.rsA : pc_cur.rsA, nB_rs = cross ? pc_nxt.rsB : pc_cur.rsB;
        const rsrc_t nS_rs = cross ? pc_nxt.rsS : pc_cur.rsS, nN_rs = cross ? pc_nxt.rsN : pc_cur.rsN;
        Seg nxt = cur;
        if (have_next) nxt = cross ? locate(pc_nxt, u_next) : locate(pc_cur, u_next);
        const int ntiles = cur.ntiles, t0 = cur.t0;
        if (!ahead) {
            // slow path. Every wave is past the barrier of the previous stream tile (or this is the start): both tile buffers,
            // the slots and the query region are free
            dma_queries(pc_cur.rsA, cur.qb * QB);
            dma_norms(pc_cur.rsN, cur.qb);
            dma_tile(pc_cur.rsB, pc_cur.rsS, t0, g & 1);
            if (ntiles > 1) dma_tile(pc_cur.rsB, pc_cur.rsS, t0 + 1, (g + 1) & 1);    // stream tile g + 1
            // (LDS-DMA is tracked per wave: every wave drains ITS transfers before the barrier -- see match_top2_body)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            f16_fetch<0>(frA, ldsb + (g & 1) * IMG + r * ROWB, foff);
        }
        const float nav = norm_read();                    // (requested ahead: landed before the previous segment's second barrier)
        // per-lane MFMA fragments of the wave's 32 queries (k-steps 0..7; prep_kernel applied the -2) and the norm k-slot
        u32x4 qw[16];
#pragma unroll
        for (int t = 0; t < 8; ++t) qw[t] = *reinterpret_cast<const u32x4 *>(ldsb + QREG + (wave * 32 + r) * ROWB + foff[t]);
        u32x4 qslot = {0u, 0u, 0u, 0u};
        if (h == 0) {
            unsigned nh, nm, nl;
            bf16_three(nav, nh, nm, nl);
            qslot = (u32x4){BF16_ONE | (BF16_ONE << 16), BF16_ONE | (nh << 16), nm | (nl << 16), 0u};
        }
        Top3 best;
        best.k1 = best.k2 = best.k3 = KEY_INF; best.t1 = best.t2 = 0;
        auto fold = [&](int g1, int g2, int g3, int tag) {
            if (__any(g1 < best.k3)) {
                top3_merge(best, g1, tag);
                top3_merge(best, g2, tag);
                top3_merge(best, g3, tag);
            }
        };
        bool next_ahead = false;
        f32x16 a0, a1, b0, b1;
        for (int n = 0; n < ntiles; ++n) {
            const int b = (g + n) & 1;
            const char *tb = ldsb + b * IMG + r * ROWB;
            const char *sp = ldsb + SLOT0 + b * SLOTB + r * 16;
            int g1 = KEY_INF, g2 = KEY_INF;               // of groups 2 n - 1 (slots 0..31) and 2 n (slots 32..63) together
            // Issue priority: the two waves of a SIMD do not share it evenly -- one of them runs almost at its solo speed and
            // then idles ~1 200 cycles at the tile's barrier, the other (the critical path) takes ~30 % longer through the same
            // instructions (tools/kcoarse_stamps.py). A wave is raised from the barrier to the end of the iteration (the
            // request of the next tile and the last half group) and lowered for the first three half groups: -1.0 to -1.4 % per
            // launch, same box (static priorities for half the waves: no change; alternating by tile parity: -0.7 %).
            if (NM_COARSE_PRIO) __builtin_amdgcn_s_setprio(NM_COARSE_PRIO_LO);
            NM_STAMP(0);
            f16_fetch<4>(frB, tb, foff);
            f16_slots(a0, a1, sp, qslot);
            if (n == 0) {
                f16_half<false, 0>(a0, a1, b0, frA, qw, g1, g2);
                NM_STAMP(1);
                f16_fetch<0>(frA, tb + 64 * ROWB, foff);
                f16_half<false, 4>(a0, a1, b1, frB, qw, g1, g2);
            } else {
                f16_half<true, 0>(a0, a1, b0, frA, qw, g1, g2);
                NM_STAMP(1);
                f16_fetch<0>(frA, tb + 64 * ROWB, foff);
                f16_half<true, 4>(a0, a1, b1, frB, qw, g1, g2);
            }
            NM_STAMP(2);
            f16_fetch<4>(frB, tb + 64 * ROWB, foff);
            f16_slots(b0, b1, sp + 64 * 16, qslot);
            f16_half<true, 0, 32>(b0, b1, a0, frA, qw, g1, g2);
            NM_STAMP(3);
            // stream tiles g + n + 1 (requested an iteration ago: landed by now) and g + n + 2 (to be requested)
            const bool in1 = n + 1 < ntiles, in2 = n + 2 < ntiles;
            const bool ex1 = in1 || have_next;
            bool ex2 = false;                                         // stream tile g + n + 2 exists and is requested in this iteration
            int tile2 = 0;
            if (ex1) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                NM_STAMP(4);
                __syncthreads();
                if (NM_COARSE_PRIO) __builtin_amdgcn_s_setprio(NM_COARSE_PRIO_HI);
                NM_STAMP(5);
                const int k2 = n + 2 - ntiles;                        // index in the next segment when tile g + n + 2 lies there
                ex2 = in2 || (have_next && ntiles >= 2 && k2 < nxt.ntiles);
                tile2 = in2 ? t0 + n + 2 : nxt.t0 + k2;
                if (n == 0 && have_next && ntiles >= 2) {             // every wave holds its fragments: the query region is free
                    dma_queries(nA_rs, nxt.qb * QB);
                    dma_norms(nN_rs, nxt.qb);
                    next_ahead = true;
                }
                if (in1 || next_ahead) f16_fetch<0>(frA, ldsb + (b ^ 1) * IMG + r * ROWB, foff);
            }
            NM_STAMP(6);
            // (The request spread over the last half group, one piece behind each k-step, measured 1.5 % SLOWER than five
            // instructions back to back here: 651 against 642 us per 16-pair launch, same box.)
#ifndef NM_STUB_NODMA
            if (ex2) dma_tile(in2 ? pc_cur.rsB : nB_rs, in2 ? pc_cur.rsS : nS_rs, tile2, b);
#endif
            f16_half<true, 4, 32>(b0, b1, a1, frB, qw, g1, g2);
            fold(g1, g2, g2, n);
            NM_STAMP(7);
#ifdef NM_COARSE_STAMPS
            if (wg == 0 && stamp_it < 64 && lane == 0) {              // (the stores' cost falls into segment 7 -> 0')
#pragma unroll
                for (int k = 0; k < 8; ++k) nm_coarse_stamps[(wave * 64 + stamp_it) * 8 + k] = stamp_t[k];
            }
            ++stamp_it;
#endif
        }
        asm volatile("s_nop 15\n\ts_nop 3" : "+v"(b0), "+v"(b1));
        select_half<COARSE_SLOT_BITS>(b0, b1, best, ntiles);       // group 2 ntiles - 1: slots 0..31 of "iteration" ntiles
        segment_publish<COARSE_SLOT_BITS>(best, pc_cur.plan, pc_cur.grp, cur.pc, cur.qbl, pc_cur.vg, cur.tt + ntiles == cur.Lc, t0 * TILE_C, h,
                        cur.qb * QB + wave * 32 + r, pc_cur.nA, pc_cur.plan.S, pc_cur.partial, pc_cur.partial3);
        if (!have_next) {
            if (!restart) break;
            __syncthreads();                              // NM_COARSE_CROSS=0: every pair starts with the slow path, as until round 5
            pc_cur = pc_nxt; cur = locate(pc_cur, u_next); ahead = false; g = 0;
            continue;
        }
        g += ntiles;
        ahead = next_ahead;
        cur = nxt;
        if (cross) pc_cur = pc_nxt;
    }
}

template <int SCR>
__global__ __launch_bounds__(512, 2) void match_top2_kernel(const float *__restrict__ A, int nA_arg,
                                                           const float *__restrict__ B, int nB_arg,
                                                           const float *__restrict__ na, const float *__restrict__ nb,
                                                           const uint4 *__restrict__ nbslot,
                                                           MatchPlan plan_arg, float4 *__restrict__ partial,
                                                           float *__restrict__ partial3,
                                                           const int *__restrict__ d_nA, const int *__restrict__ d_nB,
                                                           const MatchPlan *__restrict__ d_plan)
{
    match_top2_body<SCR>(A, nA_arg, B, nB_arg, na, nb, nbslot, plan_arg, partial, partial3, d_nA, d_nB, d_plan, (int)blockIdx.x);
}

// Round 6: the single-pass screens with ONE XCD PER PAIR, like the coarse pass: a launch covers `xcd` pairs of the call (first,
// first + 1, ...), pair first + (b mod xcd) on the workgroups b of that XCD with local index b / xcd, each under a one-group plan
// for n_cu / xcd workgroups (host-sized calls: plans.p; device-sized: the pair's d_plan, made for that geometry by nbmax_kernel).
struct MatchPlanPack { MatchPlan p[8]; };
template <int SCR>
__global__ __launch_bounds__(512, 2) void match_top2_group_kernel(MatchBatch bt, int first, int xcd, MatchPlanPack plans)
{
    const int k = (int)blockIdx.x % xcd;
    const MatchPair &c = bt.p[first + k];
    match_top2_body<SCR>(SCR ? reinterpret_cast<const float *>(c.As) : c.A, c.nA, SCR ? reinterpret_cast<const float *>(c.Bs) : c.B, c.nB,
                         c.na, c.nb, c.nbslot, plans.p[k], c.partial, c.partial3, c.d_nA, c.d_nB, c.d_plan, (int)blockIdx.x / xcd);
}

// Second pass of the two-stage screen, all pairs of a call in ONE launch (blockIdx.y = pair): the bf16x3 screen on the
// rows the coarse pass listed (fine_rows_kernel wrote their split images, norms and the work plan for their number).
// Usually a percent of the rows: most workgroups find plan.G below their index and leave.
__global__ __launch_bounds__(512, 2) void match_top2_rows_kernel(MatchBatch bt)
{
    const MatchPair &c = bt.p[blockIdx.y];
    match_top2_body<1>(reinterpret_cast<const float *>(c.As), c.nA, reinterpret_cast<const float *>(c.Bs), c.nB, c.na2, c.nb,
                       c.nbslot, MatchPlan{}, c.partial, c.partial3, pair_f1_count(c), c.d_nB, pair_plan2(c), (int)blockIdx.x);
}

}  // namespace

int launch_prep(const MatchBatch &bt, int screen, int max_rows, hipStream_t st)
{
    const dim3 pg(nm_divup(max_rows, PREP_ROWS), bt.n);
    if (screen == 2) hipLaunchKernelGGL(prep_kernel<2>, pg, dim3(256), 0, st, bt);
    else if (screen) hipLaunchKernelGGL(prep_kernel<1>, pg, dim3(256), 0, st, bt);
    else hipLaunchKernelGGL(prep_kernel<0>, pg, dim3(256), 0, st, bt);
    NM_LAUNCH_CHECK();
    hipLaunchKernelGGL(nbmax_kernel, dim3(bt.n), dim3(1024), 0, st, bt);
    NM_LAUNCH_CHECK();
    return 0;
}

int screen_set_lds(int screen, bool grouped, size_t lds_bytes, size_t lds_full)
{
    // per call: the attribute is per device, and a process may drive several (cheap host-side call, not a stream op)
    NM_RETURN_IF(hipFuncSetAttribute(screen == 2 ? reinterpret_cast<const void *>(match_coarse_kernel)
                                     : screen ? reinterpret_cast<const void *>(match_top2_kernel<1>)
                                              : reinterpret_cast<const void *>(match_top2_kernel<0>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
    if (screen == 2)
        NM_RETURN_IF(hipFuncSetAttribute(reinterpret_cast<const void *>(match_top2_rows_kernel),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_full));
    else if (grouped)
        NM_RETURN_IF(hipFuncSetAttribute(screen ? reinterpret_cast<const void *>(match_top2_group_kernel<1>)
                                                : reinterpret_cast<const void *>(match_top2_group_kernel<0>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
    return 0;
}

void launch_screen(const MatchBatch &bt, const MatchPlan *plans, int q, int screen, bool dev_sized, int grid, int n_cu,
                   size_t lds_bytes, hipStream_t st)
{
    const MatchPair &c = bt.p[q];
    const MatchPlan plan_arg = dev_sized ? MatchPlan{} : plans[q];
    if (screen == 2) {
        if (q == 0) hipLaunchKernelGGL(match_coarse_kernel, dim3(n_cu), dim3(512), lds_bytes, st, bt);
    } else if (bt.pair_xcd > 0) {
        // one launch per `xcd` pairs (the first pair's events bracket it, the others' are recorded back to back)
        if (q % bt.pair_xcd == 0) {
            MatchPlanPack pk{};
            for (int k = 0; k < bt.pair_xcd; ++k) pk.p[k] = dev_sized ? MatchPlan{} : plans[q + k];
            if (screen) hipLaunchKernelGGL(match_top2_group_kernel<1>, dim3(n_cu), dim3(512), lds_bytes, st, bt, q, bt.pair_xcd, pk);
            else hipLaunchKernelGGL(match_top2_group_kernel<0>, dim3(n_cu), dim3(512), lds_bytes, st, bt, q, bt.pair_xcd, pk);
        }
    } else if (screen)
        hipLaunchKernelGGL(match_top2_kernel<1>, dim3(grid), dim3(512), lds_bytes, st,
                           reinterpret_cast<const float *>(c.As), c.nA, reinterpret_cast<const float *>(c.Bs), c.nB,
                           c.na, c.nb, c.nbslot, plan_arg, c.partial, c.partial3, c.d_nA, c.d_nB, c.d_plan);
    else
        hipLaunchKernelGGL(match_top2_kernel<0>, dim3(grid), dim3(512), lds_bytes, st, c.A, c.nA, c.B, c.nB,
                           c.na, c.nb, c.nbslot, plan_arg, c.partial, c.partial3, c.d_nA, c.d_nB, c.d_plan);
}

void launch_rows(const MatchBatch &bt, int n_wg2, size_t lds_full, hipStream_t st)
{
    hipLaunchKernelGGL(match_top2_rows_kernel, dim3(n_wg2, bt.n), dim3(512), lds_full, st, bt);
}

}  // namespace nm_match

#ifdef NM_COARSE_STAMPS
extern "C" __attribute__((visibility("default"))) int nm_debug_coarse_stamps(unsigned long long *host_dst)
{
    return (int)hipMemcpyFromSymbol(host_dst, HIP_SYMBOL(nm_match::nm_coarse_stamps), sizeof(nm_match::nm_coarse_stamps));
}
#endif
