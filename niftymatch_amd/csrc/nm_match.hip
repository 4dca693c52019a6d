// nm_match.hip -- brute-force 128-D squared-L2 matcher for gfx950.
// Replaces kernels/transpose.cu:9-40, kernels/match.cu:14-150 and sift/siftfunctions.cu:15-40.
//
// Fused path (nm_sift_match_f32 / nm_sift_match_shard_f32), never materialising the nA x nB matrix:
//   1. norms_kernel        ||a||^2, ||b||^2
//   2. match_top2_kernel   fp32 MFMA (v_mfma_f32_32x32x2_f32): d~[j][i] = nb_j + na_i - 2 a_i.b_j as ONE accumulation
//                          chain (K = 128 products + 1 augmented k-pair carrying the norms); every lane keeps a running
//                          best/second-best/third-best per query over the candidates it sees (integer keys, see Top3);
//                          256 persistent workgroups over balanced unit ranges, a partial list per segment (MatchPlan).
//   3. match_finalize_kernel  per query: pick the 4 best partial candidates, recompute their distances EXACTLY in the
//                          reference's order (sum_k fma(t,t,acc), t = a_k - b_k, k ascending: match.cu:36-42), then apply
//                          the scan semantics of match.cu:91-116 (lowest index wins ties, min2 initial 2139095040.0f,
//                          result untouched when min2 <= 0). Each segment also reports the VALUE of its third best; when
//                          anything not recomputed comes within the error margin of the exact min2, the query goes to
//   4. match_fallback_kernel (+ match_fallback_merge_kernel), which scan all candidates exactly (a fraction of a
//                          percent of the queries), 64 candidate slices per listed query.
// This file is the driver: the screen choice, the work plans and run_fused_batch, which launches the kernels of
// nm_match_screen.hip (1-2), nm_match_finish.hip (3-4), nm_match_shard.hip (multi-GPU merge) through the launchers declared in
// nm_match_types.hpp. nm_match_distance.hip holds the API building blocks (transpose / bf_distance / get_sift_matches), which
// keep the reference's layouts and are exact, and the materialised distance matrix.
#include <atomic>
#include <cstdlib>
#include <cstring>

#include "nm_match_types.hpp"
#include "../../include/nm_abi.h"

namespace nm_match {
namespace {

static MatchPlan make_plan(int nA, int nB, int wg_per_cu = 1)
{
    // one persistent workgroup per CU of the current device (256 on MI355X SPX); two for the coarse pass of the two-stage
    // screen, whose 68 KiB of LDS let two workgroups share a CU (four waves per SIMD instead of two)
    return make_plan_on(nA, nB, nm_cu_count() * wg_per_cu, nm_xcd_count(), 0, 1, [](int s) { return s; });
}

// Which MFMA screen match_top2 runs: 0 = fp32 (v_mfma_f32_32x32x2_f32, K = 128 exact products), 1 = bf16x3 (split
// operands on v_mfma_f32_32x32x16_bf16), 2 = two-stage (a coarse pass with ONE fp16 product per k on
// v_mfma_f32_32x32x16_f16, then the bf16x3 screen on the rows -- about a percent on SIFT data -- whose coarse result
// cannot be proven). All feed the same exact finalize / fallback, so the results are identical; only the time differs.
// NM_MATCH_SCREEN=f32|bf16x3|f16 or nm_sift_match_set_screen() select it (process-wide).
static std::atomic<int> g_screen{-1};
static int match_screen()
{
    int v = g_screen.load(std::memory_order_relaxed);
    if (v < 0) {
        const char *e = getenv("NM_MATCH_SCREEN");
        v = (e && (!strcmp(e, "f32") || !strcmp(e, "0"))) ? 0 : (e && (!strcmp(e, "bf16x3") || !strcmp(e, "1"))) ? 1 : 2;
        g_screen.store(v, std::memory_order_relaxed);
    }
    return v;
}
// |screen value - exact squared distance| <= coeff (sqrt na + sqrt nb)^2  
// (two-stage screen: the coarse pass's fp32 accumulation only -- 134 terms, with a factor 2 of slack -- see match_finalize_kernel<1>)
// Round 4: the bf16x3 coefficient rose from 2.75e-5 to 3.15e-5. Its accumulation share was 65 u (u = 2^-24): twice the
// 25 u + 7 u of the model H-bf16 as probed by hand in round 2. nm_selftest_mfma_model (4.2e9 random results per instruction
// on MI355X, profiles/r04_b_mfma_model.txt) measures single instructions up to 1.91 x (bf16) / 1.73 x (f16) that model --
// the combination of the two halves and C loses up to one ulp, not half of one -- so 65 u was the bound itself, without
// slack. The share is now 140 u = 8.3e-6: 2.2 x the 64 u that the measured law |D - exact| <= 2 (u |D| + 7 u (pmax_lo +
// pmax_hi)) gives for a chain of 25 instructions (2 (25 u + 7 u)), and 3.2 x the largest chain error the self-test's
// adversarial families reach (2.6e-6). The coarse pass's 3.2e-5 = 537 u stands: its 9 instructions need 2 (9 u + 7 u) = 32 u.
static float screen_err_coeff(int screen) { return screen == 2 ? 3.2e-5f : screen ? 3.15e-5f : 1.56e-5f; }
// The share of those coefficients that covers the accumulation inside the matrix instructions (a hardware premise, measured
// by nm_selftest_mfma_model and asserted by tests/test_gpu_match.py): the whole of the coarse pass's coefficient (its
// representation error is bounded separately from measured residual norms), 140 x 2^-24 of the bf16x3 coefficient (the rest
// is the split's representation error, 2.31e-5, and the norms), and the fp32 screen's 2 gamma_129 fma-chain bound.
extern "C" __attribute__((visibility("default"))) float nm_sift_match_accum_budget(int screen)
{
    return screen == 2 ? screen_err_coeff(2) : screen == 1 ? 140.0f * 5.9604645e-8f : screen_err_coeff(0);
}

// One XCD per pair (round 6): with a multiple of the XCD count of pairs in the call, pair q is screened by the 32 workgroups of
// XCD q mod 8 alone (the XCDs work on 8 pairs side by side) instead of by all 256 on pair after pair: every XCD's L2 then
// fetches ITS pairs' fp16 images once (2 x 3.1 MB, which it holds) where each of the 8 L2s fetched every pair's candidate
// tiles (643 MB per 16-pair launch against 146 MB algorithmic). NM_COARSE_PAIR_XCD=0 keeps the old division of the
// coarse pass, NM_TOP2_PAIR_XCD=0 that of the single-pass screens (one launch per `xcd` pairs); each is read once per process.
static bool pairs_share_xcds(int screen, int n_pairs)
{
    const int xcd = nm_xcd_count(), n_cu = nm_cu_count();
    if (!(xcd > 1 && xcd <= 8 && n_cu % xcd == 0 && n_pairs >= xcd && n_pairs % xcd == 0)) return false;
    static const int env = [] { const char *e = getenv("NM_COARSE_PAIR_XCD"); return e ? atoi(e) : 1; }();
    static const int env1 = [] { const char *e = getenv("NM_TOP2_PAIR_XCD"); return e ? atoi(e) : 1; }();
    return (screen == 2 ? env : env1) != 0;
}

struct MatchJob {                 // host-side description of one pair of a (possibly batched) call
    const float *A, *B;
    int nA, nB, mode, index_offset;
    int *result;
    float *min1, *min2;
    int *idx1;
    void *workspace;
    const int *d_nA, *d_nB;       // device-sized call: nA / nB above are the capacities, the real sizes live here
};

// norms (1 launch for all pairs) -> MFMA top-2 (1 launch per pair) -> finalize, fallback, merge (1 launch each)
static int run_fused_batch(const MatchJob *jobs, int n, float ambiguity, hipStream_t st, int phases = 7)
{
    if (n <= 0) return 0;
    if (n > MATCH_MAX_BATCH) return (int)hipErrorInvalidValue;
    MatchBatch bt{};
    MatchPlan plans[MATCH_MAX_BATCH];
    const int screen = match_screen();
    bt.ambiguity = ambiguity;
    bt.err_coeff = screen_err_coeff(screen);
    bt.err_coeff2 = screen_err_coeff(1);
    int max_rows = 0, max_a = 0;
    bool dev_sized = false;
    // persistent workgroups per CU of the (first) screening pass. (Two for the coarse pass -- its 68 KiB of LDS would allow
    // it -- measured 70 us instead of 58: half as many tiles per segment, twice the segment prologues.)
    const int wg_per_cu = 1;
    for (int k = 0; k < n; ++k) {
        const MatchJob &j = jobs[k];
        if (j.nA <= 0 || j.nB <= 0) continue;                 // empty sets: a no-op for this pair, as in the reference
        // 32-bit byte ranges of the SRDs, and the plan's 32-bit unit arithmetic (qblocks x T must stay far below 2^31):
        // checked BEFORE any plan is made
        if (j.nA >= MATCH_MAX_ROWS || j.nB >= MATCH_MAX_ROWS) return (int)hipErrorInvalidValue;
        const int q = bt.n++;
        const bool dev = j.d_nA != nullptr;
        if (q > 0 && dev != dev_sized) return (int)hipErrorInvalidValue;
        dev_sized = dev;
        if (!dev) plans[q] = make_plan(j.nA, j.nB, wg_per_cu);
        const MatchWs w = carve(j.workspace, j.nA, j.nB);
        MatchPair &c = bt.p[q];
        c.A = j.A; c.B = j.B; c.nA = j.nA; c.nB = j.nB; c.na = w.na; c.nb = w.nb; c.partial = w.partial;
        c.partial3 = w.partial3; c.fb_count = w.fb_count; c.fb_list = w.fb_list; c.nbmax = reinterpret_cast<float *>(w.fb_count + CB_NBMAX);
        c.S = dev ? MAX_CHUNKS : plans[q].S; c.mode = j.mode;
        c.index_offset = j.index_offset; c.result = j.result; c.min1 = j.min1; c.min2 = j.min2; c.idx1 = j.idx1;
        c.As = w.As; c.Bs = w.Bs; c.nbslot = w.nbslot;
        if (screen == 2) { c.Ah = w.Ah; c.Bh = w.Bh; c.ra = w.ra; c.rb = w.rb; c.na2 = w.na2; c.f1_list = w.f1_list; }
        c.d_nA = j.d_nA; c.d_nB = j.d_nB;
        // inside the 256-byte counter block. The two-stage screen's coarse kernel takes every pair's plan from there (one
        // launch for all pairs of the call), so nbmax_kernel makes it for the host-sized entries too
        c.d_plan = (dev || screen == 2) ? reinterpret_cast<MatchPlan *>(w.fb_count + CB_PLAN) : nullptr;
        max_rows = max(max_rows, j.nA + nm_divup(j.nB, TILE_C) * TILE_C);
        max_a = max(max_a, j.nA);
    }
    if (bt.n == 0) return 0;
    const int n_cu = nm_cu_count();
    // second pass of the two-stage screen: about a percent of the rows, so a quarter of the CUs per pair is plenty and the
    // launch (one grid row per pair) does not spend its time dispatching workgroups that find nothing to do
    // (calls of a few pairs -- the 100k x 100k all-pairs case lists thousands of rows -- keep the whole chip). A pair of a
    // 16-pair call lists 10-25 rows of one 256-row block: 16 workgroups of ~6 tiles each instead of 47 of 2, and the 16
    // pairs' second passes run side by side in one round of workgroups.
    const int xcd = nm_xcd_count();
    int n_wg2 = n_cu;
    if (bt.n >= 4) n_wg2 = max(2 * xcd, (n_cu / bt.n) / xcd * xcd);
    if (n_wg2 > n_cu || n_wg2 % xcd != 0) n_wg2 = n_cu;
    bt.n_cu = n_cu * wg_per_cu; bt.n_cu2 = n_wg2; bt.n_xcd = nm_xcd_count();
    bt.pair_xcd = 0;
    if (pairs_share_xcds(screen, bt.n)) {
        bt.pair_xcd = xcd; bt.n_cu = n_cu / xcd; bt.n_xcd = 1;
        if (screen != 2 && !dev_sized)                           // host-sized plans are made here: for the XCD's share of the chip
            for (int q = 0; q < bt.n; ++q) {
                plans[q] = make_plan_on(bt.p[q].nA, bt.p[q].nB, bt.n_cu, 1, 0, 1, [](int v) { return v; });
                bt.p[q].S = plans[q].S;
            }
    }
    if (phases & NM_MATCH_PHASE_PREP) {
        if (const int rc = launch_prep(bt, screen, max_rows, st)) return rc;
    }
    const size_t lds_full = (size_t)2 * TILE_C * KP * sizeof(float);
    // coarse pass: two 32 KiB images + the norm slots; the staged query block (256 rows at a 272-byte pitch) is as large
    const size_t lds_bytes = screen == 2 ? lds_full + 1024 + 2048 : lds_full;      // + the coarse pass's pair directory and query norms
    static_assert(2 * TILE_C * (DIM * 2) + 2 * TILE_C * 16 + QB * (DIM * 2) == 2 * TILE_C * KP * sizeof(float),
                  "coarse pass: two tile images, the norm slots and the query region take what the other screens' tiles take");
    if (const int rc = screen_set_lds(screen, bt.pair_xcd > 0, lds_bytes, lds_full)) return rc;
    for (int q = 0; (phases & NM_MATCH_PHASE_SCREEN) && q < bt.n; ++q) {
        // device-sized: one workgroup per CU, of which the first plan.G (decided on the device) work
        const int grid = dev_sized ? n_cu * wg_per_cu : plans[q].G;
        // (profiling hook: one event pair per PAIR of the call. The two-stage screen's coarse pass is one launch for all
        // pairs: the first pair's events bracket it, the others are recorded back to back.)
        nm_prof_begin(NM_PROF_MATCH_TOP2, st);
        launch_screen(bt, plans, q, screen, dev_sized, grid, n_cu, lds_bytes, st);
        nm_prof_end(NM_PROF_MATCH_TOP2, st);
        NM_LAUNCH_CHECK();
    }
    if (!(phases & NM_MATCH_PHASE_FINISH)) return 0;
    const dim3 fg(nm_divup(4 * max_a, 256), bt.n);
    if (screen == 2) {
        // coarse result proven -> emitted; the others are listed, split, screened by the bf16x3 kernel (all pairs in one
        // launch, its plan made on the device for the number listed) and finalized as the single-pass screens are
        launch_finalize(1, bt, fg, st);
        NM_LAUNCH_CHECK();
        // (the lists are short: a few workgroups per pair stride over them, see the kernels)
        launch_fine_rows(bt, dim3(min(bt.n >= 4 ? 64 : 1024, nm_divup(max_a, PREP_ROWS)), bt.n), st);
        NM_LAUNCH_CHECK();
        launch_rows(bt, n_wg2, lds_full, st);
        NM_LAUNCH_CHECK();
        launch_finalize(2, bt, dim3(min((int)fg.x, bt.n >= 4 ? 32 : 512), bt.n), st);
    } else {
        launch_finalize(0, bt, fg, st);
    }
    NM_LAUNCH_CHECK();
    return launch_fallback(bt, st);
}

static int run_fused(const float *A, int nA, const float *B, int nB, int mode, int index_offset, float ambiguity,
                     int *result, float *min1, int *idx1, float *min2, void *workspace, hipStream_t st)
{
    const MatchJob j{A, B, nA, nB, mode, index_offset, result, min1, min2, idx1, workspace, nullptr, nullptr};
    return run_fused_batch(&j, 1, ambiguity, st);
}

}  // namespace
}  // namespace nm_match
using namespace nm_match;

extern "C" {

// Upper bound for every call with nA' <= nA and nB' <= nB on the same workspace (the grid plan, hence the number of
// candidate chunks S <= MAX_CHUNKS, depends on the actual sizes).
size_t nm_sift_match_workspace_bytes(int nA, int nB) { return pair_workspace_bytes(nA, nB); }

int nm_sift_match_set_screen(int screen)
{
    if (screen < 0 || screen > 2) return (int)hipErrorInvalidValue;
    g_screen.store(screen, std::memory_order_relaxed);
    return 0;
}
int nm_sift_match_get_screen(void) { return match_screen(); }

int nm_sift_match_pairs_per_launch(int n_pairs)
{
    if (n_pairs <= 0) return 0;
    const int screen = match_screen(), xcd = nm_xcd_count();
    if (screen == 2) return n_pairs;
    return pairs_share_xcds(screen, n_pairs) ? xcd : 1;
}

size_t nm_sift_match_batch_workspace_bytes(int n, const int *nA, const int *nB)
{
    size_t total = 0;
    for (int k = 0; k < n; ++k) total += pair_workspace_bytes(nA ? nA[k] : 0, nB ? nB[k] : 0);
    return total;
}

int nm_sift_match_batch_f32(int n, const float *const *A, const int *nA, const float *const *B, const int *nB,
                            int *const *result, float ambiguity, void *workspace, void *stream)
{
    if (n <= 0) return 0;
    if (n > MATCH_MAX_BATCH || !A || !nA || !B || !nB || !result || !workspace) return (int)hipErrorInvalidValue;
    MatchJob jobs[MATCH_MAX_BATCH];
    char *ws = static_cast<char *>(workspace);
    for (int k = 0; k < n; ++k) {
        jobs[k] = MatchJob{A[k], B[k], nA[k], nB[k], 0, 0, result[k], nullptr, nullptr, nullptr, ws, nullptr, nullptr};
        ws += pair_workspace_bytes(nA[k], nB[k]);
    }
    return run_fused_batch(jobs, n, ambiguity, nm_stream(stream));
}

// Device-sized batch: what a live client needs -- the frame driver leaves its descriptor count on the DEVICE
// (d_num_items, siftfunctions.cu:165-178 keeps it on the host after a synchronisation per level), and this entry reads it
// there. Every grid and the workspace are laid out for (capA, capB); the work plan is made on the device for the real
// sizes. No host synchronisation, no allocation: detect -> match chains on a stream and can be captured in a HIP graph
// that is replayed on different frames.
size_t nm_sift_match_batch_dev_workspace_bytes(int n, int capA, int capB)
{
    return (size_t)(n > 0 ? n : 0) * pair_workspace_bytes(capA, capB);
}

int nm_sift_match_batch_dev_f32(int n, const float *const *A, const int *const *d_nA, const float *const *B,
                                const int *const *d_nB, int capA, int capB, int *const *result, float ambiguity,
                                void *workspace, void *stream)
{
    return nm_sift_match_batch_dev_phases_f32(NM_MATCH_PHASE_PREP | NM_MATCH_PHASE_SCREEN | NM_MATCH_PHASE_FINISH, n, A, d_nA, B,
                                              d_nB, capA, capB, result, ambiguity, workspace, stream);
}

int nm_sift_match_batch_dev_phases_f32(int phases, int n, const float *const *A, const int *const *d_nA, const float *const *B,
                                       const int *const *d_nB, int capA, int capB, int *const *result, float ambiguity,
                                       void *workspace, void *stream)
{
    if (n <= 0) return 0;
    if (phases <= 0 || phases > 7) return (int)hipErrorInvalidValue;
    if (n > MATCH_MAX_BATCH || !A || !d_nA || !B || !d_nB || !result || !workspace || capA <= 0 || capB <= 0)
        return (int)hipErrorInvalidValue;
    MatchJob jobs[MATCH_MAX_BATCH];
    char *ws = static_cast<char *>(workspace);
    for (int k = 0; k < n; ++k) {
        if (!A[k] || !B[k] || !d_nA[k] || !d_nB[k] || !result[k]) return (int)hipErrorInvalidValue;
        jobs[k] = MatchJob{A[k], B[k], capA, capB, 0, 0, result[k], nullptr, nullptr, nullptr, ws, d_nA[k], d_nB[k]};
        ws += pair_workspace_bytes(capA, capB);
    }
    return run_fused_batch(jobs, n, ambiguity, nm_stream(stream), phases);
}

// HOST functions for tests: the plan for (nA, nB) on n_wg persistent workgroups in n_xcd XCDs, made as run_fused_batch makes it
// (one caller, no reduction). (n_wg, n_xcd) = (nm_cu_count() / nm_xcd_count(), 1) is the one-group plan of a pair that has an XCD
// to itself (pairs_share_xcds).
int nm_sift_match_plan_on(int nA, int nB, int n_wg, int n_xcd, int plan[10])
{
    if (!plan || nA < 0 || nB < 0 || nA >= MATCH_MAX_ROWS || nB >= MATCH_MAX_ROWS || n_wg < 1 || n_xcd < 1) return (int)hipErrorInvalidValue;
    const MatchPlan p = make_plan_on(nA, nB, n_wg, n_xcd, 0, 1, [](int v) { return v; });
    plan[0] = p.qblocks; plan[1] = p.T; plan[2] = p.G; plan[3] = p.S; plan[4] = p.X; plan[5] = p.Gx;
    plan[6] = p.Tc; plan[7] = p.C; plan[8] = p.q_base; plan[9] = p.q_rem;
    return 0;
}

int nm_sift_match_plan(int nA, int nB, int plan[10]) { return nm_sift_match_plan_on(nA, nB, nm_cu_count(), nm_xcd_count(), plan); }

// The segments workgroup `wg` of that plan processes, in order, as rows (query block, first tile, tiles, slot, ends_block);
// returns their number (at most max_segments are written).
int nm_sift_match_plan_segments_on(int nA, int nB, int n_wg, int n_xcd, int wg, int *segments, int max_segments)
{
    if (nA < 0 || nB < 0 || wg < 0 || nA >= MATCH_MAX_ROWS || nB >= MATCH_MAX_ROWS || n_wg < 1 || n_xcd < 1) return -1;
    const MatchPlan p = make_plan_on(nA, nB, n_wg, n_xcd, 0, 1, [](int v) { return v; });
    if (wg >= p.G) return 0;
    const int xg = wg % p.X, vg = wg / p.X;
    const PlanGroup grp = plan_group(p, xg);
    const unit_t u_end = group_begin(grp, vg + 1);
    SegIter it;
    it.init(group_begin(grp, vg), u_end);
    int n = 0;
    unit_t u;
    while (it.next(p, grp, u)) {
        int pc, qbl, tt, Lc;
        plan_locate(p, grp, u, pc, qbl, tt, Lc);
        const int ntiles = (int)((Lc - tt) < (u_end - u) ? (Lc - tt) : (u_end - u));
        if (segments && n < max_segments) {
            int *r = segments + 5 * n;
            r[0] = grp.q0 + qbl; r[1] = pc * p.Tc + tt; r[2] = ntiles; r[3] = plan_slot(p, grp, pc, qbl, vg);
            r[4] = (pc == p.C - 1 && tt + ntiles == Lc) ? 1 : 0;
        }
        ++n;
    }
    return n;
}

int nm_sift_match_plan_segments(int nA, int nB, int wg, int *segments, int max_segments)
{
    return nm_sift_match_plan_segments_on(nA, nB, nm_cu_count(), nm_xcd_count(), wg, segments, max_segments);
}

int nm_sift_match_fallback_count(const void *workspace, int nA, int nB, int *host_count, void *stream)
{
    if (!workspace || !host_count || nA <= 0 || nB <= 0) return (int)hipErrorInvalidValue;
    MatchWs w = carve(const_cast<void *>(workspace), nA, nB);
    NM_RETURN_IF(hipMemcpyAsync(host_count, w.fb_count, sizeof(int), hipMemcpyDeviceToHost, nm_stream(stream)));
    return (int)hipStreamSynchronize(nm_stream(stream));
}

int nm_sift_match_second_pass_count(const void *workspace, int nA, int nB, int *host_count, void *stream)
{
    if (!workspace || !host_count || nA <= 0 || nB <= 0) return (int)hipErrorInvalidValue;
    MatchWs w = carve(const_cast<void *>(workspace), nA, nB);
    NM_RETURN_IF(hipMemcpyAsync(host_count, w.fb_count + CB_F1_COUNT, sizeof(int), hipMemcpyDeviceToHost, nm_stream(stream)));
    return (int)hipStreamSynchronize(nm_stream(stream));
}

int nm_sift_match_f32(const float *A, int nA, const float *B, int nB, float *distance, int *result, float ambiguity,
                      void *workspace, void *stream)
{
    if (nA <= 0 || nB <= 0) return 0;
    hipStream_t st = nm_stream(stream);
    if (distance) {                     // distance[i * nB + j]: rows = queries, columns = candidates
        if (!workspace) return (int)hipErrorInvalidValue;
        const int rc = run_distance(A, nA, B, nB, distance, carve(workspace, nA, nB), st);
        if (rc) return rc;
    }
    return run_fused(A, nA, B, nB, 0, 0, ambiguity, result, nullptr, nullptr, nullptr, workspace, st);
}

int nm_sift_match_shard_f32(const float *A, int nA, const float *B_shard, int nB_shard, int index_offset, float *min1,
                            int *idx1, float *min2, void *workspace, void *stream)
{
    if (nA > 0 && nB_shard <= 0) {      // nothing to scan: (inf, -1, min2 initial) loses against every real candidate
        launch_shard_neutral(min1, idx1, min2, nA, nm_stream(stream));
        NM_LAUNCH_CHECK();
        return 0;
    }
    return run_fused(A, nA, B_shard, nB_shard, 1, index_offset, 0.f, nullptr, min1, idx1, min2, workspace,
                     nm_stream(stream));
}

}  // extern "C"
