// nm_match_plan.hpp -- the matcher's work plan: units, segments and partial-list slots (host and device code, no runtime calls).
#pragma once
#include <hip/hip_runtime.h>

namespace nm_match {

constexpr int DIM = 128;
constexpr int TILE_C = 128;        // candidates per LDS tile
constexpr int QB = 256;            // queries per workgroup (32 per wave, fragments resident in VGPRs)
constexpr int MAX_CHUNKS = 64;     // upper bound of the number S of segments (partial lists) per query block of any plan

// Work = qblocks x T units, a unit being (256 queries) x (one 128-candidate tile). The grid is G persistent workgroups
// (one per CU: the kernel owns the LDS), each taking a contiguous range of `base` or `base+1` units of a linear order:
// every CU carries the same MFMA load to within one tile and the chip drains at once. A range is processed as SEGMENTS:
// maximal runs of consecutive tiles of one query block (the query fragments are reloaded per segment). Segment k of a
// query block writes partial slot k; the segment that finishes the block also blanks the slots up to S.
//
// The linear order is XCD-aware (round 2). Workgroups b and b + X share an XCD and its 4 MB L2 (X = 8 on MI355X: blocks
// are dealt round-robin over the XCDs; speed only, never correctness). Group x = the workgroups {x, x + X, ...} gets a
// contiguous share of the query blocks, and orders its units PIECE-major: the candidate tiles are cut into C chunks of
// Tc tiles (Tc ~ the units per workgroup), and the order runs chunk by chunk, inside a chunk query block by query block.
// The ~nq workgroups that work on one chunk at the same time then stream the SAME candidate tiles, so the XCD's L2
// serves them once instead of every query block re-streaming the candidate set from the Infinity Cache. With X = 1 and
// C = 1 this is the plain query-block-major order (used for small problems and single-XCD partitions).
struct MatchPlan { int qblocks, T, G, S, X, Gx, Tc, C, q_base, q_rem; };
// Unit indices: qblocks x T <= 2^14 x 2^15 (the entries refuse sets of 2^22 rows or more), so 32 bits hold them. (They were
// 64-bit until round 3: the ~20 integer divisions a workgroup makes per segment to find its way through the plan were
// expanded to 64-bit software division on the vector unit -- ~7 us per segment of the coarse pass.)
typedef int unit_t;
struct PlanGroup { int nq, q0, base, rem; };

#define NM_HD __host__ __device__ __forceinline__
// x / d for 0 <= x, 0 < d. On the device an integer division is ~40 vector instructions, and a workgroup makes a few dozen of
// them per segment on values that are the same for all its lanes: below 2^20 (305 k units at 100k x 100k) the quotient comes
// from one v_rcp_f32 and a remainder check instead (the estimate is off by at most one there: 2^20 x 2^-22 relative error
// + the truncation).
NM_HD int pdiv(int x, int d)
{
#if defined(__HIP_DEVICE_COMPILE__)
    if (x < (1 << 20)) {
        int q = (int)((float)x * __builtin_amdgcn_rcpf((float)d));
        int r = x - q * d;
        if (r < 0) { q -= 1; r += d; }
        if (r >= d) q += 1;
        return q;
    }
#endif
    return x / d;
}
NM_HD PlanGroup plan_group(const MatchPlan &p, int x)
{
    PlanGroup g;
    g.nq = p.q_base + (x < p.q_rem ? 1 : 0);
    g.q0 = x * p.q_base + (x < p.q_rem ? x : p.q_rem);
    const unit_t U = (unit_t)g.nq * p.T;
    g.base = pdiv(U, p.Gx);
    g.rem = U - g.base * p.Gx;
    return g;
}
NM_HD unit_t group_begin(const PlanGroup &g, int v) { return (unit_t)v * g.base + (v < g.rem ? v : g.rem); }
NM_HD int group_owner(const PlanGroup &g, unit_t ul)            // local workgroup whose range holds local unit ul
{
    const unit_t cut = (unit_t)g.rem * (g.base + 1);
    if (ul < cut) return pdiv(ul, g.base + 1);            // (one division, not both: the values are uniform)
    return g.rem + pdiv(ul - cut, g.base);
}
// local unit ul -> chunk c, local query block qbl, tile offset tt inside the piece, piece length Lc
NM_HD void plan_locate(const MatchPlan &p, const PlanGroup &g, unit_t ul, int &c, int &qbl, int &tt, int &Lc)
{
    const unit_t per_chunk = (unit_t)g.nq * p.Tc;
    c = pdiv(ul, per_chunk);
    const int r = (int)(ul - (unit_t)c * per_chunk);
    Lc = p.T - c * p.Tc < p.Tc ? p.T - c * p.Tc : p.Tc;
    qbl = pdiv(r, Lc);
    tt = r - qbl * Lc;
}
// workgroups (of the group) that work on piece (c, qbl)
NM_HD void piece_owners(const MatchPlan &p, const PlanGroup &g, int c, int qbl, int &first, int &last)
{
    const int Lc = p.T - c * p.Tc < p.Tc ? p.T - c * p.Tc : p.Tc;
    const unit_t P = (unit_t)g.nq * c * p.Tc + (unit_t)qbl * Lc;
    first = group_owner(g, P);
    last = group_owner(g, P + Lc - 1);
}
// partial-list slot of the segment that local workgroup v owns in piece (c, qbl)
NM_HD int plan_slot(const MatchPlan &p, const PlanGroup &g, int c, int qbl, int v)
{
    int slot = 0, f, l;
    for (int cc = 0; cc < c; ++cc) { piece_owners(p, g, cc, qbl, f, l); slot += l - f + 1; }
    piece_owners(p, g, c, qbl, f, l);
    return slot + (v - f);
}

// A workgroup's segments in PROCESSING order. Its range is contiguous in the piece-major order, so only its first segment
// can start in the middle of a piece (the tail another workgroup left). If more pieces of the same chunk follow, that
// tail is processed AFTER them: every workgroup then walks a chunk's tiles in ascending tile index from the chunk's first
// tile, in step with the other workgroups of its XCD on the same chunk -- the first reader of a candidate tile misses in
// L2, the others hit. (Slots and results do not depend on the processing order.)
struct SegIter {
    unit_t u, u_end, u0;
    bool have_def;
    unit_t def_u;
    NM_HD void init(unit_t b, unit_t e) { u = b; u0 = b; u_end = e; have_def = false; def_u = 0; }
    // next segment: local unit where it starts (its length follows from plan_locate); false when done
    NM_HD bool next(const MatchPlan &p, const PlanGroup &g, unit_t &seg_u)
    {
        for (;;) {
            if (u >= u_end) {
                if (have_def) { have_def = false; seg_u = def_u; return true; }
                return false;
            }
            int c, qbl, tt, Lc;
            plan_locate(p, g, u, c, qbl, tt, Lc);
            const unit_t n = (Lc - tt) < (u_end - u) ? (Lc - tt) : (u_end - u);
            if (have_def) {
                int dc, dq, dt, dl;
                plan_locate(p, g, def_u, dc, dq, dt, dl);
                if (dc != c) { have_def = false; seg_u = def_u; return true; }     // chunk changes: flush the tail first
            } else if (u == u0 && tt > 0 && u + n < u_end) {
                int c2, q2, t2, l2;
                plan_locate(p, g, u + n, c2, q2, t2, l2);
                if (c2 == c) { have_def = true; def_u = u; u += n; continue; }      // defer the leading tail
            }
            seg_u = u;
            u += n;
            return true;
        }
    }
};

// Largest number of partial-list slots any query block needs under plan p. The (group, local query block) pairs are dealt
// over `nlanes` callers (host: 1; device: the lanes of one wave, which then take the maximum over the wave).
NM_HD int plan_max_slots_part(const MatchPlan &p, int lane, int nlanes)
{
    int S = 1;
    // query block k belongs to group x = the one whose [q0, q0 + nq) holds it (plan_group), found without a loop so that
    // the lanes of a wave run the same instructions on their own k (a `continue` per foreign k would serialise them)
    const int cut = p.q_rem * (p.q_base + 1);
    for (int k = lane; k < p.qblocks; k += nlanes) {
        const int x = (k < cut) ? k / (p.q_base + 1) : p.q_rem + (k - cut) / p.q_base;
        const PlanGroup g = plan_group(p, x);
        const int qbl = k - g.q0;
        int f, l;
        piece_owners(p, g, p.C - 1, qbl, f, l);
        const int n = plan_slot(p, g, p.C - 1, qbl, l) + 1;
        if (n > S) S = n;
    }
    return S;
}

NM_HD int hd_divup(int a, int b) { return (a + b - 1) / b; }
// Largest descriptor-set size (exclusive) the matcher accepts: the SRDs address rows with 32-bit byte offsets, and the work
// plan's unit indices are 32-bit (unit_t): qblocks x T = (2^22 / 256) x (2^22 / 128) = 2^29 units at the limit. Every entry
// that makes a plan rejects larger sets first (hipErrorInvalidValue).
constexpr int MATCH_MAX_ROWS = 1 << 22;

// The plan for (nA, nB) on a device of n_cu compute units in n_xcd XCDs. REDUCE(S) turns a caller's partial maximum into
// the maximum over all callers (identity on the host). Every caller computes the same plan.
template <typename Reduce>
NM_HD MatchPlan make_plan_on(int nA, int nB, int n_cu, int n_xcd, int lane, int nlanes, Reduce reduce)
{
    MatchPlan p;
    p.qblocks = hd_divup(nA > 0 ? nA : 1, QB);
    p.T = hd_divup(nB > 0 ? nB : 1, TILE_C);
    const unit_t U = (unit_t)p.qblocks * p.T;
    // XCD-grouped order: the whole chip is used, the query blocks split over the XCDs to within 3 %, and every XCD has a
    // few query blocks to share tiles between
    if (n_xcd > 1 && n_cu % n_xcd == 0 && U >= 4L * n_cu && p.qblocks >= 2 * n_xcd &&
        (unit_t)hd_divup(p.qblocks, n_xcd) * n_xcd * 100 <= (unit_t)p.qblocks * 103) {
        p.G = n_cu; p.X = n_xcd; p.Gx = n_cu / n_xcd;
        p.q_base = p.qblocks / n_xcd; p.q_rem = p.qblocks % n_xcd;
        const unit_t upw = U / n_cu;                                   // units per workgroup
        int C = (int)((p.T + upw / 2) / (upw > 0 ? upw : 1));       // chunks ~ T / units-per-workgroup
        if (C < 1) C = 1;
        if (C > p.T) C = p.T;
        p.Tc = hd_divup(p.T, C);
        p.C = hd_divup(p.T, p.Tc);
        p.S = reduce(plan_max_slots_part(p, lane, nlanes));
        if (p.S <= MAX_CHUNKS) return p;
    }
    // plain query-block-major order over one group
    const int min_len = hd_divup(p.T, MAX_CHUNKS - 2);            // a block spans <= MAX_CHUNKS - 2 whole ranges + 2 ends
    unit_t G = U / min_len;
    if (G > n_cu) G = n_cu;
    if (G < 1) G = 1;
    p.G = (int)G; p.X = 1; p.Gx = p.G;
    p.q_base = p.qblocks; p.q_rem = 0;
    p.Tc = p.T; p.C = 1;
    p.S = reduce(plan_max_slots_part(p, lane, nlanes));
    return p;
}

}  // namespace nm_match
