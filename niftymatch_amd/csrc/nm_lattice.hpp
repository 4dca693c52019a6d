// nm_lattice.hpp -- the lattice of the link stages (nm_link_verify.hip, nm_link_refine.hip) and of the exposure sums
// (nm_mosaic_exposure.hip): shape, limits and argument checks, stated once. Frame A is sampled at (stride u + stride / 2,
// stride v + stride / 2), u < fw / stride, v < fh / stride. Tiles of TILE_W x TILE_H points, row-major; a workgroup of WAVES
// waves takes the tiles g, g + step, .., a wave the rows wave, wave + WAVES, .. of a tile, a lane the column `lane`. That
// loop is NOT here: link_verify_accumulate_kernel, mosaic_exposure_sums_kernel and nmlr::walk_lane each write it out.
#pragma once
#include "nm_common.hpp"
#include "nm_pair_batch.hpp"

namespace nmlat {
constexpr int THREADS = 256, WAVES = THREADS / 64;
constexpr int TILE_W = 64, TILE_H = 32, MAX_STRIDE = 64;
constexpr long long MAX_LATTICE = 1ll << 28;      // lattice points per frame at most

struct Lattice { int lw, lh, tiles_x, tiles; };
inline Lattice lattice_of(int fw, int fh, int stride)
{
    const int lw = fw / stride, lh = fh / stride, tiles_x = nm_divup(lw, TILE_W);
    return Lattice{lw, lh, tiles_x, tiles_x * nm_divup(lh, TILE_H)};
}
inline bool lattice_ok(int fw, int fh, int stride)
{
    if (!nm_size_ok(fw) || !nm_size_ok(fh) || stride < 1 || stride > MAX_STRIDE) return false;
    return (long long)(fw / stride) * (long long)(fh / stride) <= MAX_LATTICE;
}
struct FrameTables {                        // a link stage's gray planes: 2 x 64 pointers, 1 KB of kernel arguments
    const float *a[nmp::MAX_BATCH];
    const float *b[nmp::MAX_BATCH];
};
inline bool frames_ok(int n, const float *const *grayA, const float *const *grayB, int fw, int fh, const float *H, int stride)
{
    return n >= 1 && n <= nmp::MAX_BATCH && lattice_ok(fw, fh, stride) && nmp::tables_ok(n, {grayA, grayB}, {}, {H});
}
}  // namespace nmlat
