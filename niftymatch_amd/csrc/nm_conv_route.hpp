// nm_conv_route.hpp -- which kernel a Gaussian launch gets, decided ONCE, and the grid it runs on. HOST ONLY (no HIP types: any
// C++17 compiler takes it). nm_pyramid.hip asks nm_conv_route for every frame and launches what it answers; nm_conv_route_of
// (include/nm_abi.h) hands the same answer out, and tests/test_conv_route.py pins it without a GPU.
#pragma once

// The radii with unrolled kernels (the SIFT defaults: base blur 7, levels 5 7 8 10 13, and 12 / 16 of the API's sigmas 3 / 4).
// The one list: the route and the radius-to-template dispatch both expand it.
#define NM_CONV_RADII(X) X(5) X(7) X(8) X(10) X(12) X(13) X(16)

enum NmConvRoute {                 // = NM_CONV_ROUTE_* of include/nm_abi.h
    NM_CONV_NONE = 0,              // empty image: the launch is a no-op
    NM_CONV_PACKED = 1,            // conv_pk_kernel
    NM_CONV_PACKED_BUF = 2,        // conv_pk_kernel<..., WRITE_BUF>: the API path, `buffer` receives the row pass
    NM_CONV_TILE = 3,              // conv_sep_kernel: odd widths, misaligned planes, planes of 4 GiB and more
    NM_CONV_GENERIC = 4,           // any other radius: two passes through `buffer`
    NM_CONV_INVALID = 5            // the call is rejected
};

// One frame's route. img_low4: the low four address bits of the image; out_low4: those of result | buffer.
inline NmConvRoute nm_conv_route(int width, int height, int radius, bool result, bool buffer, bool dog, bool grad,
                                 unsigned img_low4, unsigned out_low4)
{
    if (width <= 0 || height <= 0) return NM_CONV_NONE;
    if (radius < 0) return NM_CONV_INVALID;
    bool unrolled = false;
#define NM_CONV_IS(R) unrolled = unrolled || radius == R;
    NM_CONV_RADII(NM_CONV_IS)
#undef NM_CONV_IS
    if (!unrolled) return buffer ? NM_CONV_GENERIC : NM_CONV_INVALID;      // the row pass needs a real intermediate
    if (buffer && (dog || grad)) return NM_CONV_INVALID;                   // the API path never asks for the fused outputs
    // the packed kernel: float4 staging and 32-bit byte offsets into a plane
    const bool packable = width % 4 == 0 && (img_low4 & 15) == 0 && (unsigned long long)width * height * 4 < (1ull << 32);
    if (packable && !buffer) return NM_CONV_PACKED;
    if (packable && result && (out_low4 & 15) == 0) return NM_CONV_PACKED_BUF;      // float4 stores of the row pass
    return NM_CONV_TILE;
}

// The XCD-banded grid of both fixed-radius kernels: 64 x 32 tiles, dealt so that the workgroups of one XCD (blockIdx % nxcd)
// walk one contiguous band of the image; one tile per workgroup, the blocks of a frame a multiple of nxcd.
struct NmConvGrid { int tiles_x, ntiles, nxcd, blocks_per_frame; };
inline NmConvGrid nm_conv_grid(int width, int height, int nxcd)
{
    NmConvGrid g;
    g.tiles_x = (width + 63) / 64;
    g.ntiles = g.tiles_x * ((height + 31) / 32);
    g.nxcd = nxcd;
    g.blocks_per_frame = (g.ntiles + nxcd - 1) / nxcd * nxcd;
    return g;
}
