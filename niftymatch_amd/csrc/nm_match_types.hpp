// nm_match_types.hpp -- what the matcher's translation units share: the pair / batch records the kernels take, the counter
// block, the workspace layout and the launchers each kernel unit exposes to the driver (nm_match.hip).
#pragma once
#include <type_traits>

#include "nm_common.hpp"
#include "nm_match_plan.hpp"

namespace nm_match {

constexpr int KP = 132;            // LDS row pitch (floats): 128 data + norm slot + pad; 132 mod 64 = 4 -> b128 reads conflict-free
constexpr int PREP_ROWS = 16;       // rows per 256-thread workgroup

// Everything the small launches around the MFMA kernel need for one (A, B) pair. A batched call (nm_sift_match_batch_f32)
// runs norms / finalize / fallback / merge ONCE for all its pairs (the pair is a grid dimension) and only the MFMA
// kernel once per pair: the ~45 us of dependent-launch gaps and tiny launches per match shrink to a few per call.
struct MatchPair {
    const float *A, *B;
    float *na, *nb;
    float *nbmax;              // max of the candidate norms (one float), for the finalize bound
    float4 *partial;
    float *partial3;
    int *fb_count, *fb_list;
    int *result;
    float *min1, *min2;
    int *idx1;
    unsigned *As, *Bs;         // bf16x3 screen: split images of A (scaled by -2) and B, 512 B per row (hi | lo)
    uint4 *nbslot;             // bf16x3 screen: the candidates' norm k-slots, padded to whole tiles
    // two-stage screen (f16 coarse pass, then bf16x3 on the rows it could not prove): fp16 images of A (scaled by -2) and B,
    // 256 B per row; the 2-norms of their rounding residuals a - a_h, b - b_h (rounded up); the list of unproven rows
    // (its counter, the max of rb and the second work plan live in the pair's 256-byte counter block, see CounterWord)
    // and the norms of the listed rows in list order. As above holds the split images of the LISTED rows in this mode.
    unsigned *Ah, *Bh;
    float *ra, *rb, *na2;
    int *f1_list;
    int nA, nB, S, mode, index_offset;
    // Device-sized call (nm_sift_match_batch_dev_f32): the real sizes are read from device memory (what the frame driver
    // left in d_num_items), nA / nB above are the CAPACITIES every grid and the workspace are laid out for, and the work
    // plan is made on the device (nbmax_kernel) into d_plan. NULL for the host-sized entries.
    const int *d_nA, *d_nB;
    MatchPlan *d_plan;
};
// sizes / partial-list stride of a pair as the kernels see them
__device__ __forceinline__ int pair_nA(const MatchPair &c) { return c.d_nA ? min(max(*c.d_nA, 0), c.nA) : c.nA; }
__device__ __forceinline__ int pair_nB(const MatchPair &c) { return c.d_nB ? min(max(*c.d_nB, 0), c.nB) : c.nB; }
__device__ __forceinline__ int pair_S(const MatchPair &c) { return c.d_plan ? c.d_plan->S : c.S; }
// The pair's 256-byte counter block (MatchPair::fb_count points at its first word), as word offsets.
enum CounterWord {
    CB_FALLBACK_COUNT = 0,     // rows listed for the exact fallback
    CB_F1_COUNT = 4,           // rows the coarse pass left to the bf16x3 pass
    CB_NBMAX = 16,             // max candidate norm (MatchPair::nbmax) ...
    CB_RB_MAX = 17,            // ... and max candidate residual norm behind it (nbmax[1])
    CB_PLAN = 32,              // device-side plan (10 words)
    CB_PLAN2 = 44,             // plan of the bf16x3 pass (10 words)
    CB_DIST_REPORT = 60        // distance pass: number of blocks its fix-up found listed
};
static_assert(CB_RB_MAX == CB_NBMAX + 1 && CB_PLAN + 10 <= CB_PLAN2 && CB_PLAN2 + 10 <= CB_DIST_REPORT && CB_DIST_REPORT < 64, "counter block");
__device__ __forceinline__ int *pair_f1_count(const MatchPair &c) { return c.fb_count + CB_F1_COUNT; }
__device__ __forceinline__ MatchPlan *pair_plan2(const MatchPair &c) { return reinterpret_cast<MatchPlan *>(c.fb_count + CB_PLAN2); }
constexpr int MATCH_MAX_BATCH = 16;
struct MatchBatch {
    MatchPair p[MATCH_MAX_BATCH];
    int n;
    float ambiguity;
    float err_coeff;           // |screen value - exact d| <= err_coeff (sqrt na + sqrt nb)^2 for the screen in use
    float err_coeff2;          // two-stage screen: the same for its second (bf16x3) pass; err_coeff then covers the fp32
                               // accumulation of the coarse pass only, the fp16 rounding enters through ra / rb
    int n_cu, n_xcd;           // device-sized calls: the geometry the device-side plan is made for (n_cu = persistent workgroups)
    int n_cu2;                 // two-stage screen: workgroups of the second pass (one per CU), for the plan fine_rows_kernel makes
    int pair_xcd;              // coarse pass (round 6): > 0 = the number of XCDs when every pair of the call belongs to ONE of them
                               // (pair q to XCD q mod pair_xcd: the workgroups wg with wg mod pair_xcd == q mod pair_xcd, local
                               // index wg / pair_xcd, under a one-group plan for n_cu workgroups); 0 = every workgroup on every pair
};
static_assert(sizeof(MatchBatch) <= 4096, "kernel arguments are limited to 4 KB");

__device__ __forceinline__ int nm_divup_dev(int a, int b) { return (a + b - 1) / b; }

struct MatchWs { float *na, *nb; float4 *partial; float *partial3; int *fb_count, *fb_list; unsigned *As, *Bs; uint4 *nbslot;
                 unsigned *Ah, *Bh; float *ra, *rb, *na2; int *f1_list; };

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// The one layout of a pair's workspace: every region in order, 256-byte aligned. Fills w when there is a base; returns the end offset.
inline size_t workspace_layout(char *base, int nA, int nB, MatchWs &w)
{
    size_t off = 0;
    auto take = [&](auto *&p, size_t bytes) {
        if (base) p = reinterpret_cast<std::remove_reference_t<decltype(p)>>(base + off);
        off += align256(bytes);
    };
    take(w.na, (size_t)nA * 4);
    take(w.nb, ((size_t)nB + TILE_C) * 4);                        // + the +inf padding of a tile
    take(w.fb_count, 256);                                        // the counter block (CounterWord)
    take(w.fb_list, (size_t)nA * 4);
    // partial / partial3 are dead once match_finalize_kernel has run: the fallback reuses the space from `partial` on
    // for its FB_SPLIT slice results per listed query (<= nA * MAX_CHUNKS float4, covered by the workspace bound)
    take(w.partial, (size_t)nA * MAX_CHUNKS * sizeof(float4));
    take(w.partial3, (size_t)nA * MAX_CHUNKS * sizeof(float));
    take(w.As, (size_t)nA * DIM * 4);
    take(w.Bs, (size_t)nB * DIM * 4);
    take(w.nbslot, ((size_t)nB + TILE_C) * sizeof(uint4));
    take(w.Ah, (size_t)nA * DIM * 2);
    take(w.Bh, (size_t)nB * DIM * 2);
    take(w.ra, (size_t)nA * 4);
    take(w.rb, (size_t)nB * 4);
    take(w.na2, (size_t)nA * 4);
    take(w.f1_list, (size_t)nA * 4);
    return off;
}
inline MatchWs carve(void *workspace, int nA, int nB)
{
    MatchWs w;
    workspace_layout(static_cast<char *>(workspace), nA, nB, w);
    return w;
}
constexpr size_t WORKSPACE_SLACK = 256;     // unused bytes the byte count has always carried behind the last region
inline size_t pair_workspace_bytes(int nA, int nB)
{
    MatchWs w;
    return workspace_layout(nullptr, nA < 0 ? 0 : nA, nB < 0 ? 0 : nB, w) + WORKSPACE_SLACK;
}

// ---- launchers of the kernel units (hidden visibility; run_fused_batch in nm_match.hip decides, these only launch) ----
// nm_match_screen.hip: prep_kernel<screen> + nbmax_kernel; the LDS attribute of the screen kernels a call may launch; the screen
// launch of pair q (nothing when an earlier pair's launch covers q); the second pass of the two-stage screen
int launch_prep(const MatchBatch &bt, int screen, int max_rows, hipStream_t st);
int screen_set_lds(int screen, bool grouped, size_t lds_bytes, size_t lds_full);
void launch_screen(const MatchBatch &bt, const MatchPlan *plans, int q, int screen, bool dev_sized, int grid, int n_cu,
                   size_t lds_bytes, hipStream_t st);
void launch_rows(const MatchBatch &bt, int n_wg2, size_t lds_full, hipStream_t st);
// nm_match_finish.hip: match_finalize_kernel<stage>, fine_rows_kernel
void launch_finalize(int stage, const MatchBatch &bt, dim3 grid, hipStream_t st);
void launch_fine_rows(const MatchBatch &bt, dim3 grid, hipStream_t st);
// nm_match_shard.hip
void launch_shard_neutral(float *min1, int *idx1, float *min2, int nA, hipStream_t st);
// nm_match_distance.hip: match_fallback_kernel + match_fallback_merge_kernel; the distance matrix of nm_sift_match_f32
int launch_fallback(const MatchBatch &bt, hipStream_t st);
int run_distance(const float *A, int nA, const float *B, int nB, float *distance, const MatchWs &w, hipStream_t st);

}  // namespace nm_match
