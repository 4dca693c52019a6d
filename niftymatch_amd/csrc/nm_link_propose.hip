// nm_link_propose.hip -- which frame pairs of a sequence to link at all (no reference counterpart: the reference matches one
// pair at a time and leaves the choice of pairs to its client). Two entries:
//   nm_link_votes_dev_u8: for all n (n - 1) ordered pairs (a, b) of n <= 64 frames of unsigned-char descriptors, how many rows
//      of frame a pass the u8 matcher's ratio test against frame b. TWO launches whatever n is:
//      1. link_norms_kernel (grid ceil(rows / 256) x n): |row - 128|^2 as an int, ONE table per frame (not per pair): rows from
//         n_k up to the next multiple of 32 get PAD_NORM. The query side never reads those (a lane past n_a repeats the last
//         real row), so the table serves a frame both as query and as candidate. Its first workgroup of a frame also zeroes
//         that frame's row of `votes`, which launch 2 adds into.
//      2. link_votes_kernel (grid ceil(cap / 256) x n x Z), on the tile stream of nm_match_u8_dev.hpp: a wave owns 64 query
//         rows of frame a and loads their fragments and norms ONCE; it then streams the candidate tiles of the other frames one
//         frame after the other. Per frame b: the two-entry list starts empty, fold_top2 per tile, the lane halves are merged
//         (the two smallest of their four distances; the vote needs no index), emit_u8's test, a ballot per query group, and
//         one popcount per (wave, b) goes into votes[a][b] with an integer atomic add (exact in any order; a zero is not
//         added). blockIdx.z takes the z-th part of the candidate frames, so that a call of few rows still fills the chip.
//         No LDS.
//   nm_link_rank_dev: the vote matrix -> a ranked link list for nm_mosaic_adjust_dev_f32. ONE launch of one workgroup: the
//      candidates (a < b, b - a >= min_gap, score = min(votes[a][b], votes[b][a]) >= min_votes) are compacted in (a, b) order
//      with nmw::block_rank, ranked by counting on the key (score, then (a, b) ascending; unique keys, so a total order), and
//      walked in that order by one lane out of LDS under the per-frame and total limits.
// The host twins: the votes are a loop over ordered pairs through the matcher's own host pair function and a count; the
// ranking is a sort and the same walk.
#include "nm_common.hpp"
#include "nm_match_u8_dev.hpp"
#include "nm_pair_batch.hpp"
#include "nm_wave_dev.hpp"
#include "../../include/nm_abi.h"

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <vector>

namespace {

using namespace nmu8;

constexpr int QB = QW * TB / 64;            // queries per workgroup
constexpr int MAX_FRAMES = NM_LINK_PROPOSE_MAX_FRAMES;
constexpr int MAX_PAIRS = MAX_FRAMES * (MAX_FRAMES - 1) / 2;
constexpr int RANK_TB = 1024, RANK_WAVES = RANK_TB / 64;
constexpr int FILL_BLOCKS = 512;            // the scan's grid is split over the candidate frames while it has fewer workgroups
static_assert(MAX_FRAMES == nmp::MAX_BATCH, "the frame tables are pair-batch slot tables");
static_assert(NM_LINK_PROPOSE_MAX_LINKS == NM_MOSAIC_ADJUST_MAX_LINKS, "a full link list is one adjustment call");
static_assert(MAX_FRAMES * MAX_FRAMES <= 4 * RANK_TB, "four matrix entries per thread of the ranking workgroup");

std::atomic<int> g_split{0};                // 0: by the grid's size (FILL_BLOCKS); z >= 1: that many parts

struct FrameRows {                          // 2 x 64 pointers, 1 KB of kernel arguments
    const unsigned char *desc[MAX_FRAMES];
    const int *d_count[MAX_FRAMES];
};

__host__ __device__ inline size_t norm_rows(int cap) { return ((size_t)cap + TILE - 1) / TILE * TILE; }
// frame k's norms: norm_rows(cap) ints, a multiple of 128 bytes
__host__ __device__ inline int *norms_of(void *ws, int k, int cap) { return static_cast<int *>(ws) + (size_t)k * norm_rows(cap); }

__global__ __launch_bounds__(TB) void link_norms_kernel(const FrameRows f, int n, int cap, int *__restrict__ votes,
                                                        void *__restrict__ ws)
{
    const int k = blockIdx.y;
    const size_t row = (size_t)blockIdx.x * TB + threadIdx.x;
    const int nk = nmp::clip(*f.d_count[k], cap);
    if (row < norm_rows(cap)) norms_of(ws, k, cap)[row] = row < (size_t)nk ? row_norm(f.desc[k] + row * DIM) : PAD_NORM;
    if (blockIdx.x == 0 && (int)threadIdx.x < n) votes[k * n + threadIdx.x] = 0;
}

__global__ __launch_bounds__(TB) void link_votes_kernel(const FrameRows f, int n, int cap, float ambiguity, int per_z,
                                                        int *__restrict__ votes, void *__restrict__ ws)
{
    const int a = blockIdx.y, lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const int nA = nmp::clip(*f.d_count[a], cap);
    const int q0 = blockIdx.x * QB + (threadIdx.x >> 6) * QW;
    if (q0 >= nA) return;                                            // uniform over the wave; no barrier follows
    const unsigned char *__restrict__ Ad = f.desc[a];
    const int *__restrict__ na = norms_of(ws, a, cap);

    Frag qf[QG];
    int nq[QG];
    bool real[QG];                                                   // half 0 speaks for the query, and only for a real one
#pragma unroll
    for (int g = 0; g < QG; ++g) {
        const int qi = q0 + 32 * g + r, qrow = last_real(qi, nA);    // a lane past nA repeats the last row and votes nothing
        qf[g] = load_frag(Ad + (size_t)qrow * DIM, h);
        nq[g] = na[qrow];
        real[g] = h == 0 && qi < nA;
    }

    const int b0 = blockIdx.z * per_z, b1 = min(b0 + per_z, n);
    for (int b = b0; b < b1; ++b) {
        const int nB = nmp::clip(*f.d_count[b], cap);
        if (b == a || nB <= 0) continue;                             // uniform over the wave
        int ld[QG][2], lj[QG][2];
#pragma unroll
        for (int g = 0; g < QG; ++g) { ld[g][0] = ld[g][1] = LIST_INF; lj[g][0] = lj[g][1] = NO_ROW; }

        for_tiles(f.desc[b], norms_of(ws, b, cap), nB, 0, (nB + TILE - 1) / TILE, r, h, [&](int t, const Frag cf, const Norm16 cn) {
#pragma unroll
            for (int g = 0; g < QG; ++g) {
                const i32x16 acc = tile_product(cf, qf[g]);
                int key[16];
#pragma unroll
                for (int e = 0; e < 16; ++e) key[e] = ((nq[g] + cn.g[e >> 2][e & 3] - 2 * acc[e]) << 4) | e;
                fold_top2(ld[g], lj[g], key, t, h);
            }
        });

        int count = 0;
#pragma unroll
        for (int g = 0; g < QG; ++g) {
            // the halves hold disjoint candidates of the same query: the two smallest of their four distances
            const int o1 = __shfl_xor(ld[g][0], 32), o2 = __shfl_xor(ld[g][1], 32);
            const int m1 = min(ld[g][0], o1), m2 = min(max(ld[g][0], o1), min(ld[g][1], o2));
            int res = -1;
            emit_u8(m1, 0, m2, ambiguity, &res);
            count += __popcll(__ballot(real[g] && res >= 0));
        }
        if (lane == 0 && count > 0) atomicAdd(votes + a * n + b, count);
    }
}

// ---- ranking ----
// A candidate's key: higher sorts first. The score on top, below it the matrix position a n + b counted down, so that equal
// scores go by (a, b) ascending. Keys of different pairs differ.
__host__ __device__ inline long long rank_key(int score, int a, int b, int n)
{
    return ((long long)score << 12) | (long long)(MAX_FRAMES * MAX_FRAMES - 1 - (a * n + b));
}
__host__ __device__ inline int key_score(long long key) { return (int)(key >> 12); }
__host__ __device__ inline int key_pos(long long key) { return MAX_FRAMES * MAX_FRAMES - 1 - (int)(key & 4095); }

__host__ __device__ inline bool is_candidate(const int *votes, int n, int a, int b, int min_votes, int min_gap, int *score)
{
    if (a >= b || b - a < min_gap) return false;
    const int va = votes[a * n + b], vb = votes[b * n + a];
    *score = va < vb ? va : vb;
    return *score >= min_votes;
}

// The serial part, shared by the device's one lane and the host twin: walk the C keys in descending order, accept under the
// limits, write the accepted links in acceptance order. deg: n ints, zeroed. Returns the number accepted.
__host__ __device__ inline int rank_walk(const long long *sorted, int C, int n, int per_frame, int max_links, int *deg, int *link_a,
                                         int *link_b, int *link_score)
{
    int taken = 0;
    for (int c = 0; c < C && taken < max_links; ++c) {
        const long long key = sorted[c];
        const int pos = key_pos(key), a = pos / n, b = pos % n;
        if (per_frame > 0 && (deg[a] >= per_frame || deg[b] >= per_frame)) continue;
        ++deg[a]; ++deg[b];
        link_a[taken] = a; link_b[taken] = b; link_score[taken] = key_score(key);
        ++taken;
    }
    return taken;
}

__global__ __launch_bounds__(RANK_TB) void link_rank_kernel(int n, const int *__restrict__ votes, int min_votes, int min_gap,
                                                            int per_frame, int max_links, int *__restrict__ link_a,
                                                            int *__restrict__ link_b, int *__restrict__ link_score,
                                                            int *__restrict__ d_links)
{
    __shared__ long long s_key[MAX_PAIRS], s_sorted[MAX_PAIRS];
    __shared__ int s_cnt[RANK_WAVES], s_deg[MAX_FRAMES], s_taken;
    const int tid = threadIdx.x;
    if (tid < MAX_FRAMES) s_deg[tid] = 0;

    int C = 0;                                                       // candidates, compacted in (a, b) order
    for (int base = 0; base < n * n; base += RANK_TB) {              // uniform trip count
        const int pos = base + tid, a = pos / n, b = pos % n;
        int score = 0, total;
        const bool cand = pos < n * n && is_candidate(votes, n, a, b, min_votes, min_gap, &score);
        const int at = C + nmw::block_rank<RANK_WAVES>(cand, s_cnt, total);
        if (cand) s_key[at] = rank_key(score, a, b, n);
        C += total;
        __syncthreads();                                             // s_cnt is free again; after the last pass: s_key is complete
    }
    for (int c = tid; c < C; c += RANK_TB) {                         // rank by counting: the keys above the own one
        const long long key = s_key[c];
        int above = 0;
        for (int q = 0; q < C; ++q) above += s_key[q] > key ? 1 : 0;
        s_sorted[above] = key;
    }
    __syncthreads();
    if (tid == 0) s_taken = rank_walk(s_sorted, C, n, per_frame, max_links, s_deg, link_a, link_b, link_score);
    __syncthreads();
    const int taken = s_taken;
    for (int s = taken + tid; s < max_links; s += RANK_TB) { link_a[s] = -1; link_b[s] = -1; link_score[s] = 0; }
    if (tid == 0) *d_links = taken;
}

bool votes_args_ok(int n, const unsigned char *const *desc, const int *const *count, int cap, const int *votes)
{
    return nmp::range_ok(n, cap) && nmp::tables_ok(n, {desc, count}, {}, {votes});
}

bool rank_args_ok(int n, const int *votes, int min_votes, int min_gap, int per_frame, int max_links, const int *link_a,
                  const int *link_b, const int *link_score, const int *d_links)
{
    return n >= 1 && n <= MAX_FRAMES && min_votes >= 1 && min_gap >= 1 && per_frame >= 0 && max_links >= 1 &&
           max_links <= NM_LINK_PROPOSE_MAX_LINKS && votes && link_a && link_b && link_score && d_links;
}

// Parts of the candidate-frame range (blockIdx.z): one while the grid fills the chip on its own, else as many as bring it to
// FILL_BLOCKS workgroups, at most n
int split_of(int n, int cap)
{
    const int forced = g_split.load(std::memory_order_relaxed);
    const long long blocks = (long long)nm_divup(cap, QB) * n;
    int z = forced > 0 ? forced : (int)((FILL_BLOCKS + blocks - 1) / blocks);
    return z < 1 ? 1 : (z > n ? n : z);
}

}  // namespace

extern "C" int nm_link_votes_set_split(int z)
{
    return g_split.exchange(z < 1 || z > MAX_FRAMES ? 0 : z);
}

extern "C" size_t nm_link_votes_workspace_bytes(int n, int cap)
{
    if (!nmp::range_ok(n, cap)) return 0;
    return (size_t)n * norm_rows(cap) * sizeof(int);
}

extern "C" int nm_link_votes_dev_u8(int n, const unsigned char *const *desc, const int *const *d_count, int cap,
                                    float ambiguity, int *votes, void *workspace, void *stream)
{
    if (!votes_args_ok(n, desc, d_count, cap, votes) || !workspace || !operands_aligned(n, desc, desc, workspace))
        return (int)hipErrorInvalidValue;
    FrameRows rows;
    nmp::fill_slots(rows.desc, desc, 0, n); nmp::fill_slots(rows.d_count, d_count, 0, n);
    hipLaunchKernelGGL(link_norms_kernel, dim3((unsigned)((norm_rows(cap) + TB - 1) / TB), n), dim3(TB), 0, nm_stream(stream),
                       rows, n, cap, votes, workspace);
    NM_LAUNCH_CHECK();
    const int z = split_of(n, cap), per_z = nm_divup(n, z);
    hipLaunchKernelGGL(link_votes_kernel, dim3(nm_divup(cap, QB), n, nm_divup(n, per_z)), dim3(TB), 0, nm_stream(stream), rows, n,
                       cap, ambiguity, per_z, votes, workspace);
    NM_LAUNCH_CHECK();
    return 0;
}

extern "C" int nm_link_votes_host_u8(int n, const unsigned char *const *desc, const int *const *count, int cap,
                                     float ambiguity, int *votes)
{
    if (!votes_args_ok(n, desc, count, cap, votes)) return (int)hipErrorInvalidValue;
    std::vector<int> result;
    for (int a = 0; a < n; ++a)
        for (int b = 0; b < n; ++b) {
            const int nA = nmp::clip(*count[a], cap), nB = nmp::clip(*count[b], cap);
            int v = 0;
            if (a != b) {
                result.assign((size_t)nA, -1);
                match_pair_host(desc[a], nA, desc[b], nB, ambiguity, result.data());
                for (int i = 0; i < nA; ++i) v += result[i] >= 0 ? 1 : 0;
            }
            votes[a * n + b] = v;
        }
    return 0;
}

extern "C" int nm_link_rank_dev(int n, const int *votes, int min_votes, int min_gap, int per_frame, int max_links,
                                int *link_a, int *link_b, int *link_score, int *d_links, void *stream)
{
    if (!rank_args_ok(n, votes, min_votes, min_gap, per_frame, max_links, link_a, link_b, link_score, d_links))
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(link_rank_kernel, dim3(1), dim3(RANK_TB), 0, nm_stream(stream), n, votes, min_votes, min_gap, per_frame,
                       max_links, link_a, link_b, link_score, d_links);
    NM_LAUNCH_CHECK();
    return 0;
}

extern "C" int nm_link_rank_host(int n, const int *votes, int min_votes, int min_gap, int per_frame, int max_links,
                                 int *link_a, int *link_b, int *link_score, int *d_links)
{
    if (!rank_args_ok(n, votes, min_votes, min_gap, per_frame, max_links, link_a, link_b, link_score, d_links))
        return (int)hipErrorInvalidValue;
    std::vector<long long> keys;
    for (int a = 0; a < n; ++a)
        for (int b = a + 1; b < n; ++b) {
            int score;
            if (is_candidate(votes, n, a, b, min_votes, min_gap, &score)) keys.push_back(rank_key(score, a, b, n));
        }
    std::sort(keys.begin(), keys.end(), [](long long x, long long y) { return x > y; });
    int deg[MAX_FRAMES] = {0};
    const int taken = rank_walk(keys.data(), (int)keys.size(), n, per_frame, max_links, deg, link_a, link_b, link_score);
    for (int s = taken; s < max_links; ++s) { link_a[s] = -1; link_b[s] = -1; link_score[s] = 0; }
    *d_links = taken;
    return 0;
}
