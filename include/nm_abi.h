/*
 * include/nm_abi.h -- C ABI of libnm_hip.so: the MI355X (gfx950) drop-in for NiftyMatch's SIFT detect/describe +
 * brute-force L2 match path.
 *
 * Every entry point replaces one host launcher of the reference (file:line under /root/reference/src/gpu/) and
 * keeps its argument order and meaning. Differences common to all of them:
 *   - plain C: raw DEVICE pointers, ints, floats; `stream` is a hipStream_t passed as void* (NULL = default stream);
 *   - float2/float4 arrays are passed as float* with the same memory layout (x,y[,z,w] interleaved);
 *   - the return value is 0 on success or the hipError_t of the failing launch / API call (the reference prints
 *     and exit()s inside the launcher, helper_cuda.h getLastCudaError; the C++ wrappers in niftymatch_amd/nm/ restore
 *     that convention on top of this status);
 *   - textures are replaced by plain row-major planes (the reference's fetches are exact texel loads,
 *     utils/cudatex2D.cu:15-19);
 *   - all launches are asynchronous on `stream`; none allocates, frees or synchronises unless stated.
 * All functions are re-entrant; all state lives in the arguments.
 */
#ifndef NM_ABI_H
#define NM_ABI_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define NM_API __attribute__((visibility("default")))
#else
#define NM_API
#endif

/* ---- integer helpers: the reference's only extern "C" symbols (kernels/cudamath.h:18-45, cudamath.cu:5-23) ---- */
NM_API int DivUp(int a, int b);
NM_API int DivDown(int a, int b);
NM_API int AlignUp(int a, int b);
NM_API int AlignDown(int a, int b);

/* ---- library / device ---- */
NM_API const char *nm_version(void);                 /* "niftymatch_amd <ver> gfx950" */
NM_API int nm_device_count(int *count);              /* hipGetDeviceCount */
NM_API int nm_set_device(int device);                /* replaces CudaUtils::setup_CUDA (utils/cudautils.cpp:19-28) */
NM_API const char *nm_error_string(int status);      /* hipGetErrorString */

/* Fill `count` 32-bit words at device pointer dst with `pattern` (replaces thrust::fill / device_vector value
 * initialisation, sift/siftfunctions.cu:84-85,120-121, sift/pyramidata.cu:42-46).                                */
NM_API int nm_fill_u32(void *dst, size_t count, unsigned int pattern, void *stream);

/* Profiling hook (no reference counterpart; the reference's CudaTimer brackets whole calls, utils/cudatimer.cu:3-22).
 * While a (start, stop) hipEvent_t pair is registered for `site`, the launcher records start immediately before and
 * stop immediately after that kernel (sequence) on the stream it launches on. Pass NULLs to clear. Per host thread.
 *   NM_PROF_MATCH_TOP2 : the MFMA screening kernel inside nm_sift_match_f32 / _shard_f32 / _batch[_dev]_f32: one launch per
 *                        pair under the fp32 and bf16x3 screens; under the two-stage screen ONE launch (its coarse pass)
 *                        for all pairs of the call
 *   NM_PROF_PYRAMID_O0 : the octave-0 pyramid sequence (5 fused Gaussian + DoG + gradient launches) inside
 *                        nm_sift_detect_describe[_batch] / nm_sift_octave_pyramid (all frames of a batch)       */
#define NM_PROF_MATCH_TOP2 0
#define NM_PROF_PYRAMID_O0 1
#define NM_PROF_DESCRIBE 2      /* frame_desc_kernel inside nm_sift_detect_describe[_batch] (all frames of the call) */
#define NM_PROF_ORIENT 3        /* frame_orient_kernel of the same calls */
#define NM_PROF_DETECT_O0 4     /* detect_stage_kernel of octave 0 of the same calls (per-octave launches, not the tail launch) */
#define NM_PROF_DISTANCE 5      /* distance_mfma_kernel inside nm_sift_match_f32 when `distance` is materialised on the MFMA */
#define NM_PROF_SITES 6
NM_API int nm_profile_events(int site, void *start_event, void *stop_event);
/* The same with a caller-owned list of npairs (start, stop) hipEvent_t pairs, events[2k], events[2k+1], consumed by the
 * k-th launch of the site (a batched call launches the MFMA kernel once per pair; under the two-stage screen, whose coarse
 * pass is one launch per call, the call's FIRST pair brackets that launch and the pairs of its other pairs are recorded
 * back to back, so that a list of one pair per matched pair stays valid and sums to the launch). npairs = 0 clears. */
NM_API int nm_profile_event_pairs(int site, void *const *events, int npairs);

/* Self-test (no reference counterpart): the gradient's fast correctly-rounded square root is compared with the IEEE
 * expansion for EVERY float of its domain [2^-96, 2^96) and 0; *d_mismatches (device) receives the number of differing
 * inputs. Must be 0. */
NM_API int nm_selftest_sqrt(unsigned long long *d_mismatches, void *stream);
/* Self-test (no reference counterpart): the descriptor's window weight (float)exp((nx^2 + ny^2) / 8) (kernels/descriptor.cu:108)
 * is evaluated on voting samples by a division-free form whose result is proven equal to the spec's binary64 sequence unless
 * it reports a nearby binary32 rounding boundary (then the spec sequence runs). Every float of the form's domain [0, 12.875] is
 * compared. d_out (device, 3 x unsigned long long): [0] unreported differences (must be 0), [1] inputs that report a nearby
 * boundary, [2] inputs tested. */
NM_API int nm_selftest_expw(unsigned long long *d_out, void *stream);
/* Self-test (no reference counterpart): the orientation kernel (kernels/orientation.cu:39-75, 181-192) hoists a keypoint's part of
 * each vote's arithmetic -- the window test in binary32, r2 / (2 sigma^2) with the divisor's reciprocal refined once, the 3-tap
 * mean's division by 3 as a binary32 residual correction. Each form is compared with the expression it replaces: the two
 * one-operand forms over ALL 2^32 binary32 inputs, the division on 2^32 pseudo-random pairs of its domain. d_out (device,
 * 5 x unsigned long long): [0] differing thirds (must be 0), [1] inputs the third's guard rejects (2^24 + 1), [2] differing window
 * tests (must be 0), [3] differing quotients (must be 0), [4] quotients tested. */
NM_API int nm_selftest_orient(unsigned long long *d_out, void *stream);
/* Self-test of the matrix-pipe rounding premise under the matcher's proofs (no reference counterpart; what it protects is
 * the exact scan of kernels/match.cu:83-117, which match_finalize_kernel must reproduce from MFMA-screened candidates).
 * instruction: 0 = v_mfma_f32_32x32x16_bf16 (bf16x3 screen, every norm k-slot), 1 = v_mfma_f32_32x32x16_f16 (coarse pass of
 * the default two-stage screen). Runs, on the current device: the operand / accumulator layout probe, the directed rounding
 * cases, about n_random random single instructions, and about n_chains x 1024 accumulator chains issued exactly as the
 * screens issue them (one bf16 norm k-slot instruction, then 8 f16 or 24 bf16 instructions) on adversarial row families
 * incl. fp16-subnormal operands, each against binary64. d_out: NM_SELFTEST_MFMA_OUTPUTS floats on the device:
 *   [0] layout mismatches (must be 0)
 *   [1] C = 1 + 16 x 2^-25: (D - 1) in ulp (4 = dot product formed first)      [2] C = 1 + 2^-24 (1 + 2^-6): 1 = round to nearest
 *   [3] 1 + 15 x 2^-25, C = 0: ulp above 1                                      [4] C = 2^24 + 16 x 1: D - 2^24 (16 = summed first)
 *   [5] random instructions: max |D - exact| / (2^-24 (|C| + sum |a_k b_k|))
 *   [6] the same against the model: max |D - exact| / (2^-24 |exact| + 7 x 2^-24 (pmax_lo + pmax_hi)); <= 1 = inside the
 *       model whose DOUBLE the kernels' constants assume              [7] random instructions run
 *   [8] chains: max |value - exact of the same operand images| / (sqrt na + sqrt nb)^2 -- to be held against
 *       nm_sift_match_accum_budget(screen)                             [9] the same over the fp16-subnormal families only
 *   [10] chain launches of 1024 chains each                            [11] same-half truncation probe, ulp above 1 */
#define NM_SELFTEST_MFMA_OUTPUTS 16
NM_API int nm_selftest_mfma_model(int instruction, int n_random, int n_chains, float *d_out, void *stream);
/* The same for the fp32 instruction v_mfma_f32_32x32x2_f32 (the matcher's fp32 screen; the materialised distance pass of
 * nm_sift_match_f32): about n_random single results and n_chains x 1024 accumulator chains against binary64. d_out: 8 floats:
 *   [0] max |D - exact| / (2^-24 (|C| + |a0 b0| + |a1 b1|)) (<= 2 = two roundings: the premise of both bounds)
 *   [1] results equal to fma(a1, b1, fma(a0, b0, C))    [2] results equal to the correctly rounded exact sum    [5] results tested
 *   [3] the distance pass's form (two chains of 64 k-steps + one add): max |v - exact| / (sqrt na + sqrt nb)^2, to be held
 *       against nm_sift_match_distance_budget()    [4] the fp32 screen's form (one 130-step chain), against
 *       nm_sift_match_accum_budget(0) */
NM_API int nm_selftest_mfma_f32(int n_random, int n_chains, float *d_out, void *stream);
/* DIST_C of the MFMA distance pass (HOST function): |value - exact distance of the centred rows| <= DIST_C (sqrt nx + sqrt ny)^2
 * is what its acceptance test assumes; 67 + 8 roundings' worth with 15 % of slack. */
NM_API float nm_sift_match_distance_budget(void);
/* What the finalize pass budgets for the accumulation error of a screen's MFMA chain, as a multiple of
 * (sqrt na + sqrt nb)^2 (HOST function; screen: 0 = fp32, 1 = bf16x3, 2 = two-stage coarse pass): the share of
 * screen_err_coeff that is a hardware premise rather than arithmetic. The self-test's [8] must stay below half of it. */
NM_API float nm_sift_match_accum_budget(int screen);

/* ---- host-side scale-space constants ---- */
/* PyramidData::create_kernel_for_sigma (sift/pyramidata.cu:105-123). HOST function: writes 2*radius+1 normalised
 * taps to host memory `taps` (may be NULL to query) and returns radius = ceil(4*sigma).                          */
NM_API int nm_create_kernel_for_sigma(float sigma, float *taps);

/* ---- pyramid stages ---- */
/* convolve<float> (kernels/convolution.h:19-23, convolution.cu:141-159): zero-padded separable correlation,
 * `buffer` receives the row pass, `result` the column pass of `buffer`. `kernel` = 2r+1 taps in DEVICE memory.   */
NM_API int nm_convolve_f32(float *result, const float *image, float *buffer, int width, int height,
                           const float *kernel, int kernel_radius, void *stream);
/* HOST function (no device access): which kernel a Gaussian launch of ONE frame gets -- the decision nm_convolve_f32 and the frame
 * driver's batched launches act on (niftymatch_amd/csrc/nm_conv_route.hpp). has_*: whether the pointer is given (the frame driver
 * passes no buffer; nm_convolve_f32 passes result and buffer, no dog, no grad); image_low4 / out_low4: the low four address bits
 * of the image / of result | buffer. In this precedence: an empty image is NONE whatever the radius; radius < 0 is INVALID; a
 * radius outside {5, 7, 8, 10, 12, 13, 16} is GENERIC with a buffer and INVALID without; a buffer with dog or grad is INVALID;
 * width % 4 == 0, a 16-byte aligned image and a plane below 4 GiB give PACKED without a buffer and PACKED_BUF with a result and
 * 16-byte aligned result and buffer; everything else is TILE (scalar staging, size_t indices). A batch is ONE launch when every
 * frame is PACKED with the same set of outputs, else frame by frame. Pinned by tests/test_conv_route.py. */
#define NM_CONV_ROUTE_NONE 0       /* empty image: no launch */
#define NM_CONV_ROUTE_PACKED 1     /* conv_pk_kernel */
#define NM_CONV_ROUTE_PACKED_BUF 2 /* conv_pk_kernel<..., WRITE_BUF> */
#define NM_CONV_ROUTE_TILE 3       /* conv_sep_kernel, the LDS tile fallback */
#define NM_CONV_ROUTE_GENERIC 4    /* the two-pass any-radius kernels */
#define NM_CONV_ROUTE_INVALID 5    /* the call is rejected */
NM_API int nm_conv_route_of(int width, int height, int radius, int has_result, int has_buffer, int has_dog, int has_grad,
                            unsigned image_low4, unsigned out_low4);
/* downsample_by_2<float> (kernels/downsample.h:21-24, downsample.cu:20-29): the one-plane case of the frame driver's batched
 * decimation launch. */
NM_API int nm_downsample2_f32(float *result, int result_width, int result_height, const float *source,
                              int source_width, int source_height, void *stream);
/* subtract<float> (kernels/cudamath.h:56-60, cudamath.cu:57-67): C = A - B. The one-plane case of nm_subtract_batch_f32's
 * launch (at most 4096 workgroups; the batch: 2048 per plane). */
NM_API int nm_subtract_f32(const float *A, const float *B, float *C, int width, int height, void *stream);
/* gradient<float> (kernels/cudamath.h:71-75, cudamath.cu:72-80): result is float2 (magnitude, angle in (0,2pi]).
 * Deviation: the 1-pixel border, which the reference never writes, is written as (0,0).            */
NM_API int nm_gradient_f32(const float *source, float *result, int width, int height, void *stream);

/* The loops of compute_dog (sift/siftfunctions.cu:42-51) and compute_gradients (:53-63) as ONE launch each: arrays of n
 * device plane pointers (host arrays), n <= 8 / n <= 3. Same arithmetic as nm_subtract_f32 / nm_gradient_f32. */
NM_API int nm_subtract_batch_f32(int n, const float *const *A, const float *const *B, float *const *C, int width,
                                 int height, void *stream);
NM_API int nm_gradient_batch_f32(int n, const float *const *source, float *const *result, int width, int height,
                                 void *stream);

/* ---- keypoints ---- */
/* find_keypoints, unmasked overload (kernels/keypoint.h:25-32, keypoint.cu:240-251). current/down/up are DoG
 * planes (were cudaTextureObject_t). `result` is the dense width*height float4 map, pre-filled with -1 by the
 * caller as in the reference (sift/siftfunctions.cu:120-121).                                                   */
NM_API int nm_find_keypoints_f32(const float *current, const float *down, const float *up, int width, int height,
                                 float peak_threshold, float edge_threshold, float xper, float sigma_0,
                                 int num_dogs, int dog, float *result, void *stream);
/* find_keypoints, masked overload (kernels/keypoint.h:52-59, keypoint.cu:226-237). `mask` is the full-resolution
 * mask plane mask_width x mask_height; it is sampled exactly as the reference's bilinear border texture fetch at
 * ((x+0.5)*xper, (y+0.5)*xper) (keypoint.cu:214).                                                                */
NM_API int nm_find_keypoints_masked_f32(const float *current, const float *mask, int mask_width, int mask_height,
                                        const float *down, const float *up, int width, int height,
                                        float peak_threshold, float edge_threshold, float xper, float sigma_0,
                                        int num_dogs, int dog, float *result, void *stream);
/* PyramidData::gpu_collate_keypoints_for_level's thrust::copy_if (sift/pyramidata.cu:84-88): stable compaction
 * of the entries with w >= 0 among the first num_pixels of `dense` into `out`; the count is written to the
 * DEVICE int *d_count. workspace: nm_compact_workspace_bytes(num_pixels) bytes of device scratch. NULL dense, out,
 * d_count or workspace: hipErrorInvalidValue (num_pixels <= 0 only needs d_count), as nm_compact_keypoints3.        */
NM_API size_t nm_compact_workspace_bytes(int num_pixels);
NM_API int nm_compact_keypoints(const float *dense, int num_pixels, float *out, int *d_count, void *workspace,
                                void *stream);

/* The three find_keypoints calls of compute_keypoints[_with_mask] (sift/siftfunctions.cu:65-134) in ONE launch: dog[0..4]
 * are the octave's DoG planes, level l searches dog[l+1] between dog[l] and dog[l+2]; mask may be NULL. EVERY pixel of
 * the first width*height float4 of result[0..2] is written (the accepted keypoint or (-1,-1,-1,-1)), so only the part
 * of a map beyond width*height needs the reference's reset (siftfunctions.cu:120-121).                            */
NM_API int nm_find_keypoints3_f32(const float *const dog[5], const float *mask, int mask_width, int mask_height,
                                  int width, int height, float peak_threshold, float edge_threshold, float xper,
                                  float sigma_0, int num_dogs, float *const result[3], void *stream);
/* The same launch, which also resets entries [width * height, reset_end[l]) of result[l] to -1 (reset_end NULL: nothing):
 * compute_keypoints' per-octave reset of the dense maps (thrust::fill, sift/siftfunctions.cu:120-121) without launches of its
 * own -- the detection writes every entry of the octave's region, only what a larger octave left behind it needs the reset. */
NM_API int nm_find_keypoints3_reset_f32(const float *const dog[5], const float *mask, int mask_width, int mask_height,
                                        int width, int height, float peak_threshold, float edge_threshold, float xper,
                                        float sigma_0, int num_dogs, float *const result[3], const size_t reset_end[3],
                                        void *stream);
/* The frame driver's detection of one octave on caller-provided DoG planes: fused 3-level detection straight into ordered
 * lists, no dense maps (what nm_sift_detect_describe does per octave). The orchestration rules of compute_orientations /
 * compute_descriptors are applied: an empty level ends the octave (siftfunctions.cu:145,160), at most `capacity`
 * keypoints in total (:165-169). out: capacity float4, the levels' raster-ordered lists back to back; d_counts: 3 device
 * ints = keypoints kept per level. workspace: nm_find_keypoints3_compact_workspace_bytes(width, height) bytes.        */
NM_API size_t nm_find_keypoints3_compact_workspace_bytes(int width, int height);
NM_API int nm_find_keypoints3_compact_f32(const float *const dog[5], int width, int height, float peak_threshold,
                                          float edge_threshold, float xper, float sigma_0, int num_dogs, int capacity,
                                          float *out, int *d_counts, void *workspace, void *stream);
/* Tuning (extension, no counterpart in the reference): the batched detection launches of the frame driver take unit groups of 20
 * image rows instead of 5 when the launch still has at least `min_groups` of them (default 2048; results are identical
 * either way, tests/test_gpu_frame.py). min_groups < 0 restores the default; INT_MAX disables the tall form. Returns the
 * previous value. */
NM_API int nm_sift_set_detect_tall_min(int min_groups);
/* Process-wide: issue order of detect/describe calls that take the per-octave launches (more frames than the octave tail
 * serves). 0: levels 1-5 of every octave on the caller's stream; 1: levels 4-5 go to the detection stream in front of the
 * octave's detection, so that the small octaves' launches run beside the large octaves'; 2 (cross): levels 4-5 go to a third
 * stream (the call's description stream) instead, detection stays beside the next octave's levels 1-3 -- the call then uses
 * three streams, and a captured call is a graph with three parallel branches. Same launches and identical results in every
 * order (tests/test_gpu_frame_skew.py, tests/test_gpu_frame_cross.py). Any other value restores the default: NM_FRAME_SKEW in
 * the environment (read once); when that is unset, order 2 for calls of at least NM_FRAME_CROSS_MIN_FRAMES frames (a build
 * constant that the environment variable of the same name overrides, read once; 0 = never, the built-in value) and order 0 for
 * all others. Orders 1 and 2 apply to calls with one description pass that take the per-octave launches; every other call is
 * issued in order 0. Returns the previous value (for the default: NM_FRAME_SKEW's, 0 when unset). */
NM_API int nm_sift_set_frame_skew(int mode);
/* nm_compact_keypoints for three dense maps at once (three launches instead of nine); d_counts: 3 device ints. */
NM_API size_t nm_compact3_workspace_bytes(int num_pixels);
NM_API int nm_compact_keypoints3(const float *const dense[3], int num_pixels, float *const out[3], int *d_counts,
                                 void *workspace, void *stream);

/* ---- orientation + descriptor ---- */
/* detect_orientations (kernels/orientation.h:19-24, orientation.cu:219-230). `result` float2 per keypoint,
 * pre-filled with (-1,-1) by the caller (pyramidata.cu:90): only the peaks found are written (a kernel of its own; the
 * *_levels launches below write -1 themselves).                                                                    */
NM_API int nm_detect_orientations(const float *key_pts, const float *grad, int num_pts, int octave_width,
                                  int octave_height, float gauss_factor, float xper, float *result, void *stream);
/* compute_sift_descriptors (kernels/descriptor.h:25-30, descriptor.cu:243-255): the one-list case of the *_levels launch. */
NM_API int nm_compute_sift_descriptors(const float *key_pts, const float *orients, const float *grad, int num_pts,
                                       int octave_width, int octave_height, int num_dogs, float xper, float *desc,
                                       float *x, float *y, void *stream);

/* detect_orientations / compute_sift_descriptors for the (up to three) level lists of one octave in ONE launch each: the
 * loops of compute_orientations / compute_descriptors (sift/siftfunctions.cu:136-181). Host arrays of n_levels device
 * pointers and counts. nm_detect_orientations_levels writes both components of every result (unset = -1): no pre-fill. */
NM_API int nm_detect_orientations_levels(int n_levels, const float *const *key_pts, const int *num_pts, const float *grad,
                                         int octave_width, int octave_height, float gauss_factor, float xper,
                                         float *const *result, void *stream);
NM_API int nm_compute_sift_descriptors_levels(int n_levels, const float *const *key_pts, const float *const *orients,
                                              const int *num_pts, const float *grad, int octave_width, int octave_height,
                                              int num_dogs, float xper, float *const *desc, float *const *x,
                                              float *const *y, void *stream);
/* Device-sized forms of the two (round 5): the three level counts of the octave are read ON THE DEVICE (d_counts: what
 * nm_compact_keypoints3 left there), so the host needs no count to issue them -- the reference's client synchronises once
 * per level for it (thrust::copy_if, sift/pyramidata.cu:84-91). An empty level ends the octave (siftfunctions.cu:145,160);
 * max_pts is the room of every level list (key_pts, result / orients) and is ENFORCED: a level count above it is clipped to
 * max_pts, both kernels touch entries [0, max_pts) only, and those entries are what the unclipped lists would give.
 * Descriptors go to the CONTAINER's arrays: slot = running count + kept keypoints of the earlier levels + index, the running
 * count read from *d_base_in (NULL: host_base) and clipped at `capacity` (siftfunctions.cu:165-169); the new running count
 * is written to *d_items_out. h_counts (3 ints) / h_items (1 int): device-accessible pointers of pinned host memory that
 * receive the clipped counts / the new running count, valid once `stream` has reached the launch (or NULL). nm/lazy_count.h
 * is the C++ layer's use of them.                                                                                        */
NM_API int nm_detect_orientations_levels_dev(const float *const *key_pts, const int *d_counts, int max_pts, const float *grad,
                                             int octave_width, int octave_height, float gauss_factor, float xper,
                                             float *const *result, int *h_counts, void *stream);
NM_API int nm_compute_sift_descriptors_levels_dev(const float *const *key_pts, const float *const *orients, const int *d_counts,
                                                  int max_pts, const int *d_base_in, int host_base, int capacity,
                                                  int *d_items_out, int *h_items, const float *grad, int octave_width,
                                                  int octave_height, int num_dogs, float xper, float *desc, float *x, float *y,
                                                  void *stream);

/* ---- matcher ---- */
/* transpose<float> (kernels/transpose.h:16-21, transpose.cu:33-40): odata[x*height+y] = idata[y*width+x]. */
NM_API int nm_transpose_f32(float *odata, const float *idata, int width, int height, void *stream);
/* compute_brute_force_distance<float> (kernels/match.h:18-23, match.cu:120-135): A is the TRANSPOSED query set
 * (dim x size_A), B is size_B x dim, result[j*size_A + i] = squared L2 distance. dim must be 128.               */
NM_API int nm_bf_distance_f32(const float *A, int size_A, const float *B, int size_B, int sift_vector_size,
                              float *result, void *stream);
/* get_sift_matches<float> (kernels/match.h:40-46, match.cu:141-150): per-row best / second best + ratio test. */
NM_API int nm_get_sift_matches_f32(const float *distance, int rows, int cols, int buffer_width, int *result,
                                   float ambiguity, void *stream);

/* compute_sift_matches (sift/siftfunctions.h:19-21, siftfunctions.cu:15-40) on raw descriptor arrays:
 * A: nA x 128, B: nB x 128 row-major. Fused MFMA path; `distance` (nA x nB) is optional (NULL = do not
 * materialise; extension). result[i] in {-1, 0..nB-1}, left untouched when the second-best distance is <= 0
 * (match.cu:107-116). Match decisions are made on distances recomputed exactly in the reference's summation
 * order; rows whose best two cannot be proven from the MFMA pass are re-scanned exactly. workspace:
 * nm_sift_match_workspace_bytes(nA, nB) bytes of device scratch.
 * Domain: ANY float input gives the reference scan's answer. The MFMA screens themselves work on descriptors whose
 * squared norms are finite and below 1e37; a query row outside that, and every row of a call in which ANY candidate is
 * outside it (NaN, +-inf, huge), is matched by the exact fallback alone, i.e. by the scan of match.cu:88-116 with its
 * behaviour on such values: a NaN distance to candidate 0 stays the row's minimum for good (the row becomes -1), a NaN
 * distance to any other candidate is skipped (`current < x` is false), and min2 is exact also above 2139095040 -- the scan
 * overwrites it with the old minimum at every replacement (:97), so its initial value 2139095040.0f only bounds a row whose
 * minimum sits at candidate 0. Such calls are correct, not fast (one exact 128-D distance per pair of rows).        */
NM_API size_t nm_sift_match_workspace_bytes(int nA, int nB);
/* How nm_sift_match_f32 fills a requested `distance` (process-wide; NM_MATCH_DISTANCE=exact|mfma sets the initial value):
 *   1 (default) = on the fp32 matrix cores, as the squared-norm expansion of the rows centred on the mean row of B
 *       (compute_brute_force_distance, kernels/match.cu:14-80, is the reference this replaces: 3 flop per (i, j, k) on scalar
 *       ALUs). EVERY entry is within 1e-4 relative of the reference's chain acc = fma(t, t, acc), t = a_k - b_k: an entry is
 *       kept only if a rigorous bound on the contraction's rounding error stays below that; all others
 *       -- near-duplicates, exact copies, cancellation, non-finite values -- are recomputed by the reference's own chain and
 *       are bit-equal to it (should the list of 32 x 32 blocks holding such entries overflow, the whole matrix is). The pass
 *       uses the same `workspace`.
 *   0 = the exact VALU kernel: every entry bit-equal to the reference's chain (what nm_bf_distance_f32, the building block,
 *       always computes).
 * result[] does not depend on the mode: match decisions are made on exactly recomputed distances either way.
 * nm_sift_match_distance_listed: diagnostics of the LAST such pass on `workspace` (same nA, nB): 32 x 32 blocks of the matrix
 * that held an entry outside the bound and were re-examined (-1 if the pass took the exact kernel for lack of scratch: fewer
 * than ~80 query rows), and the capacity of the block list (more listed than that = the whole matrix came from the exact
 * kernel). Synchronises `stream`. */
NM_API int nm_sift_match_set_distance_mode(int mode);
NM_API int nm_sift_match_get_distance_mode(void);
NM_API int nm_sift_match_distance_listed(const void *workspace, int nA, int nB, int *listed, int *capacity, void *stream);
/* Which MFMA screen the fused matcher runs before its exact finalize (process-wide; results are identical):
 * 0 = fp32 (v_mfma_f32_32x32x2_f32 on the descriptors themselves), 1 = bf16x3 (v_mfma_f32_32x32x16_bf16 on operands
 * split into two bf16 pieces: ~3x faster, a few more rows take the exact fallback), 2 = two-stage (a coarse pass with one
 * fp16 product per k on v_mfma_f32_32x32x16_f16 whose error is bounded per row from the norms of the fp16 rounding
 * residuals; rows it cannot prove -- about a percent on SIFT descriptors, every row when a squared norm reaches 1e9 -- are
 * screened again by the bf16x3 kernel; ~2x faster again). Default 2; the environment variable
 * NM_MATCH_SCREEN=f32|bf16x3|f16 sets the initial value. Extension: the reference has one (exact VALU) path. */
NM_API int nm_sift_match_set_screen(int screen);
NM_API int nm_sift_match_get_screen(void);
/* How many pairs ONE launch of the screening kernel covers in a batched call of n_pairs non-empty pairs under the current screen
 * (diagnostic: what a timing harness divides a launch's duration by). Round 6: when n_pairs is a multiple of the device's XCD count
 * every pair of a launch belongs to one XCD (its workgroups alone screen it, the XCDs work on 8 pairs side by side): the two-stage
 * screen's coarse pass is one launch for all n_pairs, the single-pass screens launch once per 8 pairs; otherwise the coarse pass
 * still covers all pairs and the single-pass screens launch once per pair. NM_COARSE_PAIR_XCD=0 / NM_TOP2_PAIR_XCD=0 keep the
 * divisions of rounds 3-5. Results never depend on the division. */
NM_API int nm_sift_match_pairs_per_launch(int n_pairs);
/* n <= 16 independent matches in one call (arrays of n): the norms, finalize and fallback launches cover all pairs at
 * once (the pair is a grid dimension), only the MFMA kernel runs once per pair -- 4 + n stream operations instead of
 * 5 n. result[k] as in nm_sift_match_f32 (no distance matrices). workspace: nm_sift_match_batch_workspace_bytes bytes
 * (the per-pair bounds laid end to end, in order). */
#define NM_SIFT_MATCH_MAX_BATCH 16
NM_API size_t nm_sift_match_batch_workspace_bytes(int n, const int *nA, const int *nB);
NM_API int nm_sift_match_batch_f32(int n, const float *const *A, const int *nA, const float *const *B, const int *nB,
                                   int *const *result, float ambiguity, void *workspace, void *stream);
/* The same with the set sizes read from DEVICE memory: d_nA[k] / d_nB[k] point at the int the frame driver wrote
 * (d_num_items of nm_sift_detect_describe[_batch]; the reference keeps SiftData::_num_items on the host after one
 * synchronisation per level, sift/siftfunctions.cu:165-178, and compute_sift_matches reads it there, :15-40). A live
 * client therefore chains detect -> match on a stream with no host read-back, and a HIP graph captured over both replays
 * correctly on frames with different keypoint counts. capA / capB bound the sizes (values above them are clipped, as the
 * frame driver clips at its capacity; a size <= 0 makes the pair a no-op): every grid and the workspace are laid out for
 * them, and the work plan for the real sizes is made on the device. Results are identical to the host-sized entry called
 * with the same sizes. workspace: nm_sift_match_batch_dev_workspace_bytes(n, capA, capB) bytes.
 * nm_sift_match_fallback_count(workspace + k * (that / n), capA, capB, ...) reads pair k's fallback count. */
NM_API size_t nm_sift_match_batch_dev_workspace_bytes(int n, int capA, int capB);
NM_API int nm_sift_match_batch_dev_f32(int n, const float *const *A, const int *const *d_nA, const float *const *B,
                                       const int *const *d_nB, int capA, int capB, int *const *result, float ambiguity,
                                       void *workspace, void *stream);
/* The same call cut into its three dependent phases, for clients that pipeline several calls over streams of their own:
 * PREP (norms, split operand images, the device-side work plan: streaming, ~5 us per pair), SCREEN (the MFMA kernel, one
 * launch per pair: it fills the chip by itself) and FINISH (exact finalize, fallback, merge: latency-bound gathers that
 * leave most of the chip idle). The phases of one call must run in this order on the same workspace -- the CLIENT orders
 * them with its events -- but PREP of call k + 1 and FINISH of call k - 1 may run on a second stream beside SCREEN of call k
 * (bench.py does that: the MFMA launches stay back to back on one stream). phases = 7 is nm_sift_match_batch_dev_f32. */
#define NM_MATCH_PHASE_PREP 1
#define NM_MATCH_PHASE_SCREEN 2
#define NM_MATCH_PHASE_FINISH 4
NM_API int nm_sift_match_batch_dev_phases_f32(int phases, int n, const float *const *A, const int *const *d_nA,
                                              const float *const *B, const int *const *d_nB, int capA, int capB,
                                              int *const *result, float ambiguity, void *workspace, void *stream);
/* HOST functions (no device access; on a box without a GPU the MI355X geometry of 256 CUs / 8 XCDs is assumed): the work
 * distribution the matcher uses for (nA, nB). plan[0..9] = query blocks of 256 rows, candidate tiles of 128 rows, persistent
 * workgroups G, partial lists per query S (<= 64, what the workspace bound assumes), XCD groups X, workgroups per group,
 * tiles per chunk Tc, chunks C, query blocks per group (base, and how many groups hold one more). Units = blocks x tiles;
 * group x = workgroups {x, x + X, ...} holds a contiguous share of the query blocks and walks its units chunk by chunk,
 * query block by query block inside a chunk, so that the workgroups of one XCD stream the same candidate tiles together.
 * nm_sift_match_plan_segments lists what workgroup `wg` does, in order: rows of 5 ints (query block, first tile, number of
 * tiles, partial-list slot, 1 if the segment completes its query block); returns the number of segments. For tests and
 * capacity planning. Sets of 2^22 (4 194 304) rows or more are outside the matcher's domain (32-bit byte offsets and unit
 * indices): nm_sift_match_plan returns an error status, nm_sift_match_plan_segments -1, and every matching entry point
 * returns an error status before any plan is made.
 * The _on forms take the geometry instead of the device's: n_wg persistent workgroups in n_xcd XCDs (both >= 1, else the same
 * errors). (n_wg, n_xcd) = (CUs / XCDs, 1) is the one-group plan a pair runs under when it has an XCD to itself
 * (nm_sift_match_pairs_per_launch): X = 1 and G <= n_wg. The plain forms are the _on forms on the device's CUs and XCDs. */
NM_API int nm_sift_match_plan(int nA, int nB, int plan[10]);
NM_API int nm_sift_match_plan_segments(int nA, int nB, int wg, int *segments, int max_segments);
NM_API int nm_sift_match_plan_on(int nA, int nB, int n_wg, int n_xcd, int plan[10]);
NM_API int nm_sift_match_plan_segments_on(int nA, int nB, int n_wg, int n_xcd, int wg, int *segments, int max_segments);
NM_API int nm_sift_match_f32(const float *A, int nA, const float *B, int nB, float *distance, int *result,
                             float ambiguity, void *workspace, void *stream);
/* Diagnostics: number of query rows of the LAST nm_sift_match_f32 / _shard_f32 call on `workspace` (same nA, nB) that took
 * the exact full-scan fallback because the MFMA candidate pass could not prove its top-2. Synchronises the stream. */
NM_API int nm_sift_match_fallback_count(const void *workspace, int nA, int nB, int *host_count, void *stream);
/* The same for the two-stage screen: rows whose coarse (fp16) result could not be proven and that the bf16x3 pass screened
 * again. Meaningful after a call under screen 2 only (the counter is reset by such calls). Synchronises the stream. */
NM_API int nm_sift_match_second_pass_count(const void *workspace, int nA, int nB, int *host_count, void *stream);
/* Multi-GPU building blocks (no reference counterpart: the reference is single-GPU). A shard call scans the local
 * rows [0,nB_shard) of B and emits, per query row: min1 = the smallest non-NaN distance of the shard, index1 +
 * index_offset = its lowest index (-1 if the shard has no distance below +inf), min2 = the smallest of the shard's OTHER
 * non-NaN distances, +inf if there is none -- NOT clamped to the scan's initial 2139095040.0f, which only bounds a row
 * whose minimum sits at global candidate 0 (match.cu:91,97) and is applied by the merge. The shard that holds global
 * candidate 0 (index_offset == 0) reports (NaN, 0, smallest other) for a row whose distance to that candidate is NaN, as
 * the scan keeps it. The merge combines n_shards such triples per row, given shard-major (n_shards x nA), in ascending
 * shard order so that the lowest global index wins ties, and applies the clamp and the ratio test: the result equals
 * the single-GPU scan for every input. */
NM_API int nm_sift_match_shard_f32(const float *A, int nA, const float *B_shard, int nB_shard, int index_offset,
                                   float *min1, int *idx1, float *min2, void *workspace, void *stream);
NM_API int nm_sift_match_merge_f32(const float *min1, const int *idx1, const float *min2, int n_shards, int nA,
                                   int *result, float ambiguity, void *stream);

/* The whole sharded match as ONE call per rank (native counterpart of niftymatch_amd/parallel.py::match_sharded): every
 * rank holds all of A and rows [index_offset, index_offset + nB_shard) of B; the call computes the shard triples, issues
 * ONE ncclAllGather of 3 * nA int32 per rank (12 B per row: latency-bound, far below the per-link xGMI bandwidth) on
 * `stream`, and merges the n_ranks triples in ascending rank order so that the lowest global index wins ties
 * (match.cu:94-105). nccl_comm is the caller's ncclComm_t (RCCL), passed as void* to keep this header free of rccl.h;
 * ncclAllGather is resolved from the running process, libnm_hip.so does not link librccl. n_ranks = 1 needs no
 * communicator. Shards must be passed in rank order: rank g's index_offset = rows of B held by ranks < g.
 * workspace: nm_sift_match_allgather_workspace_bytes(nA, nB_shard, n_ranks) bytes. No reference counterpart (single-GPU). */
/* The merge step alone, on the buffer the all-gather produces: rank g's block is (min1[nA], idx1[nA], min2[nA]) as int32
 * bit patterns at packed + g * 3 * nA. Ranks in ascending order = ascending global candidate index (Q14). */
NM_API int nm_sift_match_merge_packed_f32(const int *packed, int n_shards, int nA, int *result, float ambiguity,
                                          void *stream);
NM_API size_t nm_sift_match_allgather_workspace_bytes(int nA, int nB_shard, int n_ranks);
NM_API int nm_sift_match_allgather_f32(const float *A, int nA, const float *B_shard, int nB_shard, int index_offset,
                                       int n_ranks, int *result, float ambiguity, void *workspace, void *nccl_comm,
                                       void *stream);

/* ---- "next" rows of SURVEY.md 8(f): the element-wise stages either side of the path ---- */
/* cuda_grayscale<float> (kernels/bgra_2_gray.h:14-18, bgra_2_gray.cu:9-31): 0.07 B + 0.72 G + 0.21 R. bgra = uchar4. */
NM_API int nm_grayscale_f32(const unsigned char *bgra, float *output, int width, int height, void *stream);
/* cuda_extract_channel<float> (bgra_2_gray.cu:36-62): channel 0..3 = B, G, R, A. */
NM_API int nm_extract_channel_f32(const unsigned char *bgra, float *output, int width, int height, int channel,
                                  void *stream);
/* cuda_put_channel<float> (bgra_2_gray.cu:65-92): channel 3 writes 255, as the reference does. */
NM_API int nm_put_channel_f32(unsigned char *bgra, const float *input, int width, int height, int channel, void *stream);
/* cuda_set_alpha_to_const (bgra_2_gray.cu:95-112). */
NM_API int nm_set_alpha_to_const(unsigned char *bgra, int width, int height, unsigned char val, void *stream);
/* cuda_cast<float, unsigned char> (kernels/cast.h:17-22, cast.cu:8-39): saturates at max_val when max_val != 0. */
NM_API int nm_cast_f32_u8(const float *src, size_t cols, size_t rows, unsigned char *dst, unsigned char max_val,
                          void *stream);
/* downsample_by_2<uchar4> (kernels/downsample.cu:32). */
NM_API int nm_downsample2_u8x4(unsigned char *result, int result_width, int result_height, const unsigned char *source,
                               int source_width, int source_height, void *stream);
/* align_points (kernels/ransac.h:8-10, ransac.cu:29-59): gathers the matched coordinates; unmatched rows get -1. */
NM_API int nm_align_points(const float *src_x, const float *src_y, const float *dst_x, const float *dst_y,
                           float *c_src_x, float *c_src_y, float *c_dst_x, float *c_dst_y, const int *matches,
                           int num_pts, void *stream);

/* ---- N3/N4 warps. The reference samples cudaTextureObject_t's made by CudaTex2D (utils/cudatex2D.cu:13-19: border
 * addressing, linear filter, unnormalised coordinates, normalised-float reads). Here a texture is a device plane
 * (pointer, width, height, texel format); the filter is done in software with the texture unit's 1/256 weights.   */
#define NM_TEX_U8N 0      /* unsigned char, read as c/255          (cudaReadModeNormalizedFloat) */
#define NM_TEX_U8X4N 1    /* uchar4, each channel read as c/255 */
#define NM_TEX_F32 2      /* float, read as is                      (cudaReadModeElementType) */
/* cuda_undistort (kernels/undistort.h:30-35, undistort.cu:7-64): camera_matrix = fx, fy, cx, cy; distortion_coeffs =
 * k1, k2, k3 (device pointers, as in the reference). */
NM_API int nm_undistort_map_f32(const float *x, const float *y, size_t cols, size_t rows, const float *camera_matrix,
                                const float *distortion_coeffs, float *u, float *v, void *stream);
/* resample_undistort (kernels/resample.h:34-38, resample.cu:100-113,234-248): tex(x+.5, y+.5) * 255.9999f */
NM_API int nm_resample_undistort_f32(const void *tex, int tex_width, int tex_height, int tex_format, const float *x,
                                     const float *y, size_t cols, size_t rows, float *undistorted, void *stream);
/* resample_mask (resample.h:12-14, resample.cu:69-82,207-216) */
NM_API int nm_resample_mask_u8(unsigned char *result, const void *tex, int tex_width, int tex_height, int tex_format,
                               int cols, int rows, const float *x_pos, const float *y_pos, float threshold, void *stream);
/* resample_perspective_transform (resample.h:7-10, resample.cu:84-98,116-204): fills x_pos / y_pos with the (inverse)
 * projective map of the pixel grid and samples the uchar4 texture there; one launch instead of two. */
NM_API int nm_resample_perspective_u8x4(unsigned char *result, const unsigned char *tex, int tex_width, int tex_height,
                                        int cols, int rows, float *x_pos, float *y_pos, const float *mat3x3, int inverse,
                                        void *stream);
/* resample_2D<uchar4> (resample.cu:116-204, the sampling half of resample_perspective_transform) on a map the caller
 * supplies: result[p], channel c, = (unsigned char)(s[c] * 255.9999f) with s = the uchar4 sample of tex at
 * (x[p] + 0.5f, y[p] + 0.5f), exactly as nm_resample_perspective_u8x4 writes it after projecting (a coordinate outside
 * the sampler's support, NaN and +-inf included, samples 0). tex is tex_width x tex_height uchar4, x / y / result are
 * cols x rows. Returns 0 without launching when cols or rows <= 0, hipErrorInvalidValue when tex_width or tex_height
 * <= 0. */
NM_API int nm_resample_map_u8x4(unsigned char *result, const unsigned char *tex, int tex_width, int tex_height,
                                const float *x, const float *y, int cols, int rows, void *stream);
/* transform_blend (resample.h:16-20, resample.cu:7-66,218-232): frame (uchar4), frame_mask and frame_wts are fw x fh. */
NM_API int nm_transform_blend(unsigned char *canvas, int cw, int ch, const unsigned char *frame, int fw, int fh, int nw,
                              int nh, const float *mat3x3, int tx, int ty, const void *frame_mask, int mask_format,
                              float *canvas_wts, const void *frame_wts, int wts_format, void *stream);

/* RANSAC hypothesis evaluation (kernels/ransac.cu:430-521 kernels + the max_element/copy of :523-694).
 * model: 0 translation (1 sample per hypothesis), 1 similarity (2), 2 homography (4). rand_list: DEVICE array of
 * iterations * samples point indices (the reference draws them on the host, ransac.cu:543-551; see the C++ wrappers).
 * Outputs (device): homographies iterations x 9 (zeros for a hypothesis with a repeated index), inliers iterations,
 * H_best 9 floats = the hypothesis at the FIRST maximum of inliers, *d_position its index (may be NULL).
 * Points with src_x < 0 (unmatched rows of align_points) are ignored. The null vector of the design matrix is found by
 * an independent one-sided Jacobi, not the reference's GSL port: see csrc/nm_ransac_math.hpp.                     */
NM_API int nm_ransac_f32(int model, const float *src_x, const float *src_y, const float *dst_x, const float *dst_y,
                         int num_pts, const int *rand_list, int iterations, float inlier_threshold,
                         float *homographies, int *inliers, float *H_best, int *d_position, void *stream);

/* Seed of the host-side sampler used by the C++ ransac_* wrappers (0 = std::random_device, the reference's behaviour). */
NM_API void nm_ransac_seed(unsigned int seed);

/* Batched RANSAC with DEVICE-side sampling (no reference counterpart): n <= NM_RANSAC_MAX_BATCH frame pairs in three
 * launches on `stream`, no allocation, no synchronisation, no host read -- capturable into a HIP graph together with
 * nm_sift_match_batch_dev_f32. Pair k (arrays of n):
 *   src_x/src_y[k]  frame A's keypoint coordinates (e.g. an arena's x / y), dst_x/dst_y[k] frame B's;
 *   matches[k]      the pair's result of nm_sift_match_batch[_dev]_f32 (row i of A -> a row of B, or -1);
 *   d_nA[k]         DEVICE int, A's row count (e.g. the arena's num_items), clipped to [0, capA]; rows beyond it are never read.
 * The valid rows V_k are the rows i < min(nA, capA), ascending, with matches[k][i] >= 0 and src_x[k][i] >= 0 (exactly the rows
 * where align_points leaves c_src_x >= 0); m_k = |V_k|. Hypothesis t, sample s of S = 1, 2, 4 samples (model 0, 1, 2) uses row
 * V_k[j], j = nm_ransac_batch_sample(seeds[k], t, s, S, m_k): SplitMix64 of c = (seed << 32) | (t S + s), i.e.
 *   z = c + 0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^= z >> 31;
 *   j = ((z >> 32) * m) >> 32                                                         (64-bit unsigned arithmetic)
 * seeds is a HOST array of n. A pair's result depends only on its own inputs and seed, never on its slot in the call. Fit,
 * repeated-index rule and inlier test are those of nm_ransac_f32, so the results equal nm_ransac_f32 on the aligned rows with
 * rand_list[t][s] = V_k[j], bit for bit. Outputs (device): H_best n x 9 (the hypothesis at the FIRST maximum of the counts),
 * best_inliers n, position n, status n (1; 0 when m_k is below the model's minimum of 2, 2, 4 points -- then H_best is 0,
 * best_inliers 0, position -1). Optional (may be NULL): homographies n x iterations x 9, inliers n x iterations, every
 * hypothesis (rows of a status-0 pair are zero). workspace: nm_ransac_batch_dev_workspace_bytes(n, capA, iterations) bytes
 * (0 for arguments out of range). The call returns hipErrorInvalidValue, touching no device memory, for model not in
 * {0, 1, 2}, n not in [1, 64], iterations not in [1, 2^20], capA not in [1, 2^22), a non-finite threshold or a NULL required
 * pointer. The C++ ransac_* wrappers keep the reference's host mt19937 sampler: this entry draws different samples.    */
#define NM_RANSAC_MAX_BATCH 64
#define NM_RANSAC_MAX_ITERATIONS (1 << 20)
NM_API size_t nm_ransac_batch_dev_workspace_bytes(int n, int capA, int iterations);
NM_API int nm_ransac_batch_dev_f32(int model, int n,
                                   const float *const *src_x, const float *const *src_y, const int *const *d_nA, int capA,
                                   const float *const *dst_x, const float *const *dst_y, const int *const *matches,
                                   int iterations, float inlier_threshold, const unsigned int *seeds,
                                   float *H_best, int *best_inliers, int *position, int *status,
                                   float *homographies, int *inliers, void *workspace, void *stream);
/* Host-only: the batched entry's sampler, for tests and for clients that reproduce a draw. Returns j in [0, m), or -1 for
 * samples not in {1, 2, 4}, sample not in [0, samples), hypothesis not in [0, 2^20) or m < 1.                          */
NM_API int nm_ransac_batch_sample(unsigned int seed, int hypothesis, int sample, int samples, int m);

/* Batched least-squares refit of RANSAC models over their inliers, with inlier masks (no reference counterpart: the
 * reference hands out the hypothesis fitted to its minimal sample). n <= NM_RANSAC_MAX_BATCH pairs in ONE launch on
 * `stream` whatever n and rounds are; no allocation, no synchronisation, no host read, no workspace -- capturable into a
 * HIP graph behind nm_ransac_batch_dev_f32. src_x .. matches, d_nA, capA and the valid rows V_k are those of
 * nm_ransac_batch_dev_f32. H_in: device, n x 9 (e.g. H_best); status_in: device, n ints, NULL = all 1.
 *   Classification: row i of V_k is an inlier of a map H when nmr_is_inlier(H, .., inlier_threshold) holds
 *   (csrc/nm_ransac_math.hpp, the test of nm_ransac_f32), so with rounds = 0 the count equals best_inliers bit for bit.
 *   One round: S = inliers of H_cur, c_cur = |S|; stop if c_cur < 1, 2, 4 (model 0, 1, 2); H_new = the least-squares fit to
 *   all of S, its nine values rounded to fp32; stop unless all nine are finite; c_new = inliers of H_new; stop unless
 *   c_new >= c_cur; else H_cur = H_new (its inliers are the next round's S). At most `rounds` in [0, 4] rounds; the count
 *   never falls, and with no accepted round H_out is H_in bit for bit.
 *   Fits (fp64 from the fp32 coordinates, fma explicit, IEEE divide and sqrt; the sums below in the order given last):
 *     translation  t = (sum d - sum s) / c, per axis.
 *     similarity   c1 = sum s / c, c2 = sum d / c, s_c = s - c1, d_c = d - c2; a = (sum fma(s_cx, d_cx, s_cy d_cy)
 *                  + i sum fma(s_cx, d_cy, -(s_cy d_cx))) / sum fma(s_cx, s_cx, s_cy s_cy); t = c2 - a c1;
 *                  H = (Re a, -Im a, t_x; Im a, Re a, t_y; 0, 0, 1).
 *     homography   normalised DLT. s1 = sqrt(2) / (sum |s_c| / c), s2 alike; a = s_c s1, b = d_c s2, p = (a_x, a_y, 1).
 *                  Each inlier gives the equations (0, -p, b_y p) and (p, 0, -b_x p); their 9 x 9 moment matrix is built
 *                  from the 24 sums of P = (a_x^2, a_x a_y, a_x, a_y^2, a_y, 1), b_x P, b_y P and fma(b_x, b_x, b_y b_y) P.
 *                  Its eigenvector of the smallest eigenvalue comes from a cyclic two-sided Jacobi in round-robin order:
 *                  in step t = 0 .. 8 of a sweep index t rests and (t + k) % 9 meets (t - k) % 9, k = 1 .. 4; the four
 *                  rotations (Golub & Van Loan 8.5; skipped when |a_pq| <= 2^-52 sqrt(|a_pp a_qq|)) are computed from
 *                  the matrix as the step finds it, then all columns are rotated (A J, V J), then all rows (J^T A), and
 *                  a_pq = a_qp = 0 is stored; sweeps end when one rotates nothing (30 at most). The column of V at the
 *                  first smallest diagonal entry is denormalised (inv(T2) Hn T1) and divided by its last entry.
 *     Sums: 512 virtual lanes; lane l adds rows l, l + 512, .. of the pair's arrays in ascending order (only inliers
 *     contribute); each group of 64 lanes is reduced as v[l] += v[l + d] for d = 32, 16, .. 1; the 8 group totals are
 *     added in ascending order. No atomics: a pair's outputs depend on that pair's inputs alone, never on n, on the pair's
 *     slot or on scheduling.
 * Outputs (device): H_out n x 9, count n (inliers of H_out), status n, rounds_done n (accepted rounds); optional (may be
 * NULL): mask n x capA bytes (mask[k capA + i] = 1 for an inlier row of H_out, else 0; all capA bytes of a pair are written)
 * and rms n (sqrt of the mean squared reprojection distance over the final inliers, the distances and the sum in fp64 from
 * the fp32 map; 0 without inliers). A pair with status_in != 1 or a non-finite value in H_in gets status 0 and zeros in
 * every output; every other pair gets status 1, so H_out and status can go to nm_mosaic_plan_f32 as they are.
 * Returns hipErrorInvalidValue, touching no device memory, for model not in {0, 1, 2}, n not in [1, 64], rounds not in
 * [0, 4], capA not in [1, 2^22), a non-finite threshold, a NULL required pointer or a NULL among the first n table entries.
 * nm_ransac_refit_host_f32: the same with every pointer in host memory (nA[k] points to a host int), compiled from the
 * same functions (csrc/nm_ransac_refit_math.hpp): host and device results are identical bit for bit.                    */
#define NM_RANSAC_REFIT_MAX_ROUNDS 4
NM_API int nm_ransac_refit_batch_dev_f32(int model, int n,
                                         const float *const *src_x, const float *const *src_y, const int *const *d_nA,
                                         int capA, const float *const *dst_x, const float *const *dst_y,
                                         const int *const *matches, const float *H_in, const int *status_in,
                                         float inlier_threshold, int rounds, float *H_out, int *count, int *status,
                                         int *rounds_done, unsigned char *mask, float *rms, void *stream);
NM_API int nm_ransac_refit_host_f32(int model, int n,
                                    const float *const *src_x, const float *const *src_y, const int *const *nA, int capA,
                                    const float *const *dst_x, const float *const *dst_y, const int *const *matches,
                                    const float *H_in, const int *status_in, float inlier_threshold, int rounds,
                                    float *H_out, int *count, int *status, int *rounds_done, unsigned char *mask,
                                    float *rms);

/* Batched homography-guided matching (no reference counterpart: the reference's matcher is blind and nothing returns to the
 * descriptors once a model is known). Given pair k's map H_k (frame A pixels -> frame B pixels, e.g. H_out of
 * nm_ransac_refit_batch_dev_f32), every row of A is matched again, by the reference's scan, against those rows of B alone
 * that lie within sqrt(radius2) pixels of where H_k sends it: more correspondences than the blind ratio test keeps, all of
 * them inliers of H_k, ready for a second refit. n <= NM_MATCH_GUIDED_MAX_BATCH pairs in THREE launches on `stream`
 * whatever n is (pair slots 0-31, slots 32-63, the counts); no allocation, no synchronisation, no host read, no workspace
 * -- capturable into a HIP graph behind the refit. Brute-force gating (every row of A against every row of B); a spatial
 * grid over B is out of scope. Pair k (tables of n pointers, the tables themselves in HOST memory):
 *   A[k] / B[k]        descriptors, nA x 128 / nB x 128 row-major (an arena's desc);
 *   ax, ay / bx, by    the rows' keypoint coordinates (an arena's x / y);
 *   d_nA[k], d_nB[k]   DEVICE ints, the row counts: nA = clip(*d_nA[k], 0, capA), nB = clip(*d_nB[k], 0, capB). Rows beyond
 *                      them are never read;
 *   H + 9 k            device, nine floats row-major; status_in: device, n ints, NULL = all 1.
 * Per pair, all fp32 (fma explicit, IEEE division):
 *   Unusable pair: status_in[k] != 1 or a non-finite value in H_k: result[k][0 .. capA) = -1, count[k] = 0
 *     (best_distance[k][0 .. capA) = +inf).
 *   Valid rows: i < nA with ax[i] >= 0 (the rule of nm_ransac_batch_dev_f32 and of the refit; a NaN is not >= 0). Any
 *     other row has no candidates.
 *   Gate: candidate j < nB passes for row i exactly when nmr_is_inlier(H_k, ax[i], ay[i], bx[j], by[j], radius2) holds
 *     (csrc/nm_ransac_math.hpp), i.e. with h = H_k
 *       x = fmaf(h0, ax, h1 * ay) + h2;  y = fmaf(h3, ax, h4 * ay) + h5;  z = fmaf(h6, ax, h7 * ay) + h8;
 *       px = x / z;  py = y / z;  ex = bx[j] - px;  ey = by[j] - py;  fmaf(ex, ex, ey * ey) < radius2
 *     (px, py are computed once per row: the same operations, the same bits). A NaN anywhere fails the gate, so a row
 *     projected with z = 0 has no candidates; so has every row when radius2 <= 0.
 *   Distance of a gated candidate: the chain of nm_bf_distance_f32, acc = 0; acc = fmaf(t, t, acc) with t = A[i][q] - B[j][q],
 *     q = 0 .. 127 in this order -- bit-equal to it.
 *   Decision: get_sift_matches' scan (kernels/match.cu:88-116) over the gated candidates in ascending j: the first one sets
 *     min1 (whatever its value) and the index, min2 starts at 2139095040.0f; a later d with d < min1 moves min1 to min2 and
 *     takes its place, else d < min2 replaces min2 (strict <). The row's result is the index when min2 > 0 and
 *     min1 / min2 < ambiguity and min1 < max_distance (+inf disables the last test), else -1; -1 also without any gated
 *     candidate. With a gate that passes every candidate and max_distance = +inf the result therefore equals
 *     nm_sift_match_f32 on a prior of -1, bit for bit (nB >= 1).
 * Outputs: result[k] (device, capA ints; ALL capA entries are written, -1 beyond nA), count (device, n ints: entries >= 0 of
 * result[k]), best_distance (optional table, may be NULL: best_distance[k] device, capA floats = the row's min1, +inf for
 * a row without a gated candidate). result[k] can go to nm_ransac_refit_batch_dev_f32 as matches[k] as it is. A pair's
 * outputs depend on that pair's inputs alone, never on n, on the pair's slot or on scheduling (no atomics).
 * Returns hipErrorInvalidValue, touching no device memory, for n not in [1, 64], capA or capB not in [1, 2^22), a non-finite
 * radius2 or ambiguity, a NaN max_distance, a NULL required pointer (every argument but status_in, best_distance and
 * stream) or a NULL among the first n entries of a table.
 * nm_sift_match_guided_host_f32: the same with every pointer in host memory (nA[k] / nB[k] point to host ints), compiled
 * from the same functions (csrc/nm_match_guided_math.hpp): host and device results are identical bit for bit.          */
#define NM_MATCH_GUIDED_MAX_BATCH 64
NM_API int nm_sift_match_guided_batch_dev_f32(int n,
                                              const float *const *A, const float *const *ax, const float *const *ay,
                                              const int *const *d_nA, int capA,
                                              const float *const *B, const float *const *bx, const float *const *by,
                                              const int *const *d_nB, int capB,
                                              const float *H, const int *status_in, float radius2, float ambiguity,
                                              float max_distance, int *const *result, int *count,
                                              float *const *best_distance, void *stream);
NM_API int nm_sift_match_guided_host_f32(int n,
                                         const float *const *A, const float *const *ax, const float *const *ay,
                                         const int *const *nA, int capA,
                                         const float *const *B, const float *const *bx, const float *const *by,
                                         const int *const *nB, int capB,
                                         const float *H, const int *status_in, float radius2, float ambiguity,
                                         float max_distance, int *const *result, int *count,
                                         float *const *best_distance);

/* Batched mutual-nearest-neighbour filtering of a match list (the cross-check of a brute-force matcher; no reference
 * counterpart: the reference's matcher tests one direction only, so several rows of A may claim the same row of B, and a
 * client cross-checks with a second, swapped call and a comparison on the host). Given pair k's match list (e.g. the result
 * of nm_sift_match_batch_dev_f32), a match i -> j is kept only when i is also the best row of A for column j. n <=
 * NM_MATCH_MUTUAL_MAX_BATCH pairs in THREE launches on `stream` whatever n is (claims, scan, counts); no allocation, no
 * synchronisation, no host read -- capturable into a HIP graph behind the matcher. It reads only the public inputs below,
 * nothing of the blind matcher's plans, screens or workspace. Pair k (tables of n pointers, the tables in HOST memory):
 *   A[k] / B[k]        descriptors, nA x 128 / nB x 128 row-major (an arena's desc);
 *   d_nA[k], d_nB[k]   DEVICE ints, the row counts: nA = clip(*d_nA[k], 0, capA), nB = clip(*d_nB[k], 0, capB). Rows beyond
 *                      them are never read;
 *   matches[k]         device, capA ints: the list to filter (entries at and beyond nA are never read).
 * Per pair, all fp32 (fma explicit, IEEE):
 *   Distance: d(i, j) is the chain of nm_bf_distance_f32, acc = 0; acc = fmaf(t, t, acc) with t = A[i][q] - B[j][q],
 *     q = 0 .. 127 in this order -- bit-equal to it.
 *   Claim: row i < nA claims column j = matches[k][i] when 0 <= j < nB. Any other value (-1, below -1, >= nB) is no claim.
 *   Keep: with tau = d(i, j), the claim is kept exactly when tau == tau (tau is not NaN), no i' < nA has d(i', j) < tau, and
 *     no i' < i has d(i', j) == tau: i is the first minimum of column j in an ascending scan with strict <, the index
 *     get_sift_matches' scan (kernels/match.cu:88-116) returns for the swapped call. A rival row with a NaN distance beats
 *     nothing.
 *   The chain never decreases (t * t >= 0, rounding is monotone, a NaN stays a NaN), so a rival row is abandoned as soon as
 *     its partial sum, looked at every 16 dimensions, is no longer <= tau: this changes no result.
 * Outputs: result[k] (device, capA ints; ALL capA entries are written: j for a kept claim, else -1, -1 beyond nA; it may
 * alias no input), count (device, n ints: entries >= 0 of result[k]), forward_distance (optional table, may be NULL:
 * forward_distance[k] device, capA floats = tau for a claiming row, +inf otherwise). The kept matches of a pair are
 * injective (no two rows keep the same j). result[k] can go to nm_ransac_batch_dev_f32, nm_ransac_refit_batch_dev_f32 and
 * nm_align_points as matches[k] as it is. A pair's outputs depend on that pair's inputs alone, never on n, on the pair's
 * slot or on scheduling (no atomics; a beaten claim's -1 may be stored by several workgroups, always the same value).
 * workspace: device, nm_sift_match_mutual_workspace_bytes(n, capA) bytes (0 for arguments out of range), no contents
 * expected or preserved.
 * Returns hipErrorInvalidValue, touching no device memory, for n not in [1, 64], capA or capB not in [1, 2^22), a NULL
 * required pointer (every argument but forward_distance and stream) or a NULL among the first n entries of a table.
 * nm_sift_match_mutual_host_f32: the same with every pointer in host memory (nA[k] / nB[k] point to host ints), no workspace
 * and no stream, compiled from the same functions (csrc/nm_match_mutual_math.hpp): host and device results are identical
 * bit for bit.                                                                                                            */
#define NM_MATCH_MUTUAL_MAX_BATCH 64
NM_API size_t nm_sift_match_mutual_workspace_bytes(int n, int capA);
NM_API int nm_sift_match_mutual_batch_dev_f32(int n, const float *const *A, const int *const *d_nA, int capA,
                                              const float *const *B, const int *const *d_nB, int capB,
                                              const int *const *matches, int *const *result, int *count,
                                              float *const *forward_distance, void *workspace, void *stream);
NM_API int nm_sift_match_mutual_host_f32(int n, const float *const *A, const int *const *nA, int capA,
                                         const float *const *B, const int *const *nB, int capB,
                                         const int *const *matches, int *const *result, int *count,
                                         float *const *forward_distance);

/* ---- Descriptor finish (no reference counterpart: the reference's descriptors stay raw fp32 histograms, its
 * normalize_histogram in kernels/descriptor.cu is never called). nm_sift_desc_finish_batch_dev turns the raw rows of
 * n in [1, NM_DESC_FINISH_MAX_BATCH] frames into the standard SIFT form in ONE launch on `stream` (the frame is a grid
 * dimension): no allocation, no synchronisation, no host read, so it can be captured into a HIP graph behind the frame
 * driver. desc, d_num_items, out_f32, out_u8: HOST tables of n device pointers.
 *   desc[k]         capacity x 128 floats, row-major (an arena's desc);
 *   d_num_items[k]  DEVICE int, the row count: rows = clip(*d_num_items[k], 0, capacity). Rows at and beyond it are neither
 *                   read nor written;
 *   out_f32[k]      capacity x 128 floats, out_u8[k] capacity x 128 unsigned chars. Either table may be NULL, not both;
 *                   out_f32[k] may be desc[k] (in place). Outputs overlap nothing else.
 * Per row, all IEEE binary32, fused only where fmaf is written (csrc/nm_desc_finish_math.hpp), v = the 128 elements:
 *   sum(p): the row is held as 64 pairs, pair l = elements (2 l, 2 l + 1), each with one partial p[l]; then for
 *     d = 32, 16, 8, 4, 2, 1 in this order every p[l] becomes p[l] + p[l ^ d] (the xor butterfly of a wave with one pair
 *     per lane); the sum is p[0].
 *   NM_DESC_L2:
 *     1. s = sum(fmaf(v[2l+1], v[2l+1], v[2l] * v[2l])).
 *     2. If s is zero or not finite (it is zero also when every square underflows: elements below about 1e-23), every
 *        output element of the row is 0 (fp32 +0, code 0).
 *     3. v = v / sqrtf(s) element by element; v = fminf(v, 0.2f); then steps 1 and 3's division once more on the clipped row.
 *     4. code = min(255, (int)rintf(512 * v)), round half to even; anything not above zero is code 0.
 *   NM_DESC_ROOT (RootSIFT): steps 1-3, then t = sum(v[2l] + v[2l+1]), v = sqrtf(v / t) (the row has unit L2 norm), then 4.
 * The domain is the non-negative histogram the describe stage writes. A negative element keeps its sign through L2 and gets
 * code 0; RootSIFT makes a NaN of it (code 0).
 * Returns hipErrorInvalidValue, before anything is launched or dereferenced, for n not in [1, 64], capacity not in
 * [1, 2^22), a mode other than the two, desc or d_num_items NULL, both output tables NULL, or a NULL among the first n
 * entries of a given table.
 * nm_sift_desc_finish_host: the same with every pointer in host memory and no stream, compiled from the same functions:
 * host and device results are identical bit for bit.                                                                    */
#define NM_DESC_FINISH_MAX_BATCH 64
#define NM_DESC_L2 0
#define NM_DESC_ROOT 1
NM_API int nm_sift_desc_finish_batch_dev(int n, const float *const *desc, const int *const *d_num_items, int capacity,
                                         float *const *out_f32, unsigned char *const *out_u8, int mode, void *stream);
NM_API int nm_sift_desc_finish_host(int n, const float *const *desc, const int *const *num_items, int capacity,
                                    float *const *out_f32, unsigned char *const *out_u8, int mode);

/* ---- Keypoint selection: the strongest `keep` rows of a frame, spread over a gx x gy grid (no reference counterpart: the
 * reference keeps the first `capacity` rows in octave / level / raster order, sift/siftdata.h:12-15, which at 1080p and 2048
 * rows is a stripe along the top of the finest level). nm_sift_select_batch_dev selects in n in [1, NM_SELECT_MAX_BATCH]
 * frames in FOUR launches on `stream` whatever n is (score, group, round, gather): no allocation, no synchronisation, no
 * host read, so it can be captured into a HIP graph behind nm_sift_detect_describe_batch and in front of
 * nm_sift_desc_finish_batch_dev. Every table is a HOST table of n device pointers; capacity is the room of every input and
 * output of a frame, in rows:
 *   d_num_items[k]  DEVICE int, the row count: m = clip(*d_num_items[k], 0, capacity); a negative count is 0;
 *   x[k], y[k]      capacity floats, full-resolution coordinates in a width x height frame (an arena's x, y);
 *   scores[k]       optional table: capacity floats. Without it desc is required and gives the default score;
 *   desc[k], desc_u8[k], kpts[k], orients[k]   optional payload tables: capacity x 128 floats (8-byte aligned) / capacity x 128
 *                   unsigned chars (2-byte aligned) / capacity float4 / capacity float2;
 *   out_x[k] .. out_orients[k]   the same shapes; an out_* table is required exactly when its input table is given;
 *   out_index[k]    optional: capacity ints, the source row of each output row;
 *   d_out_items[k]  DEVICE int.
 * Per frame, from that frame's inputs alone (never n, the slot or scheduling):
 *   1. Score: s_i = scores[k][i], or without scores step 1 of the finish on desc[k]'s row i, v = its 128 elements:
 *      s_i = sum(fmaf(v[2l+1], v[2l+1], v[2l] * v[2l])) with the finish's sum(p) (64 pairs, xor butterfly d = 32 .. 1): the
 *      squared norm of the raw histogram, bit-identical on host and device (csrc/nm_select_math.hpp).
 *      u_i = s_i when s_i > 0 and finite, else +0: NaN, negative, zero and infinite scores rank last.
 *   2. Cell: cw = DivUp(width, gx), ch = DivUp(height, gy). xi = 0 unless x_i >= 0 (a NaN lands in pixel 0), width - 1 when
 *      x_i >= width, else (int)x_i; yi the same in height. cell = (yi / ch) * gx + xi / cw.
 *   3. Beats: row i beats row j when u_i > u_j, or u_i == u_j and i < j.
 *   4. Round: r_i = the number of rows of i's cell that beat i.
 *   5. Precedence: i precedes j when r_i < r_j, or r_i == r_j and i beats j: every cell's best, strongest first, then every
 *      cell's second best, ...
 *   6. Selected: the first min(keep, m) rows of that total order.
 *   7. Output: the selected rows in ASCENDING SOURCE INDEX (the octave / level / raster order the matcher's first-minimum
 *      rule and every later stage see), copied byte for byte to every given out_* table; out_index[k][t] = the source row
 *      of output row t; *d_out_items[k] = min(keep, m). Rows at and beyond that count are not written. No output may
 *      overlap an input or another output.
 * It follows: gx = gy = 1 is the top keep rows by score; keep >= m copies the frame; a cell's selected rows are its best
 * ones; the selected counts of two cells differ by more than one only when the smaller cell is exhausted; with keep no
 * smaller than the number of non-empty cells every non-empty cell has a selected row.
 * Cost: the round launch compares every row with the rows of its own cell, sum over cells of size^2 key compares -- all
 * rows in one cell is capacity^2, which is why capacity stops at 65536.
 * workspace: device, 8-byte aligned, nm_sift_select_workspace_bytes(n, capacity, gx, gy) bytes (0 for arguments out of
 * range), no contents expected or preserved.
 * Returns hipErrorInvalidValue, before anything is launched or dereferenced, for n not in [1, 64], capacity not in
 * [1, 65536], gx or gy not in [1, 64], keep not in [1, capacity], width or height < 1, a NULL d_num_items, x, y, out_x,
 * out_y, d_out_items or workspace (or a workspace that is not 8-byte aligned), neither scores nor desc, an out_* table without
 * its input table or the reverse, a NULL among the first n entries of a given table, or an output pointer equal to its
 * input pointer.
 * nm_sift_select_host: the same with every pointer in host memory, no workspace and no stream, from the same score, cell
 * and key functions and the same argument checks: host and device results are identical bit for bit.                   */
#define NM_SELECT_MAX_BATCH 64
#define NM_SELECT_MAX_CAPACITY 65536
#define NM_SELECT_MAX_GRID 64
NM_API size_t nm_sift_select_workspace_bytes(int n, int capacity, int gx, int gy);
NM_API int nm_sift_select_batch_dev(int n, int capacity, int width, int height, int gx, int gy, int keep,
                                    const int *const *d_num_items, const float *const *x, const float *const *y,
                                    const float *const *scores, const float *const *desc,
                                    const unsigned char *const *desc_u8, const float *const *kpts,
                                    const float *const *orients, float *const *out_x, float *const *out_y,
                                    float *const *out_desc, unsigned char *const *out_desc_u8, float *const *out_kpts,
                                    float *const *out_orients, int *const *out_index, int *const *d_out_items,
                                    void *workspace, void *stream);
NM_API int nm_sift_select_host(int n, int capacity, int width, int height, int gx, int gy, int keep,
                               const int *const *num_items, const float *const *x, const float *const *y,
                               const float *const *scores, const float *const *desc, const unsigned char *const *desc_u8,
                               const float *const *kpts, const float *const *orients, float *const *out_x,
                               float *const *out_y, float *const *out_desc, unsigned char *const *out_desc_u8,
                               float *const *out_kpts, float *const *out_orients, int *const *out_index,
                               int *const *out_items);

/* ---- Brute-force matching of unsigned-char descriptors on the i8 matrix cores (no reference counterpart: the reference
 * matches fp32 rows). n in [1, NM_MATCH_U8_MAX_BATCH] pairs in TWO launches on `stream` whatever n is (row norms, match);
 * no allocation, no synchronisation, no host read. Pair k (HOST tables of n device pointers):
 *   A[k] / B[k]        capA x 128 / capB x 128 unsigned chars, row-major, 16-byte aligned (out_u8 of the finish);
 *   d_nA[k], d_nB[k]   DEVICE ints: nA = clip(*d_nA[k], 0, capA), nB = clip(*d_nB[k], 0, capB). Rows beyond them are never
 *                      read. A pair with nA <= 0 or nB <= 0 is a no-op;
 *   result[k]          device, capA ints; entries at and beyond nA are not written.
 * Semantics: result[k] is what nm_sift_match_f32 writes for the same pair when its inputs are the float copies of the u8
 * rows and result is pre-filled the same way. In full: d(i, j) = sum over q of (A[i][q] - B[j][q])^2 as an exact integer
 * (<= 128 * 255^2 < 2^23, so also an exact float); the scan of kernels/match.cu:88-116 runs on those values as floats:
 * min1 = d(i, 0), index 0, min2 = 2139095040.0f; for j = 1 .. nB - 1 a d < min1 moves min1 to min2 and takes (d, j), else
 * a d < min2 replaces min2 -- the first minimum wins ties; a row whose min2 is 0 is left unwritten; otherwise
 * result[i] = (min1 / min2 < ambiguity) ? index : -1 with an fp32 divide. A pair's result depends on that pair's inputs
 * alone, never on n, the slot or scheduling (no atomics).
 * workspace: device, 16-byte aligned, nm_sift_match_u8_workspace_bytes(n, capA, capB) bytes (0 for arguments out of
 * range), no contents expected or preserved.
 * Returns hipErrorInvalidValue, touching no device memory, for n not in [1, 64], capA or capB not in [1, 2^22), a NULL
 * table, workspace or entry among the first n of a table, or a descriptor pointer or workspace that is not 16-byte aligned.
 * nm_sift_match_u8_host: the same with every pointer in host memory (no alignment rule), no workspace and no stream; the
 * same argument checks and the same last step, results identical to the device entry's.                               */
#define NM_MATCH_U8_MAX_BATCH 64
NM_API size_t nm_sift_match_u8_workspace_bytes(int n, int capA, int capB);
NM_API int nm_sift_match_u8_batch_dev(int n, const unsigned char *const *A, const int *const *d_nA, int capA,
                                      const unsigned char *const *B, const int *const *d_nB, int capB,
                                      int *const *result, float ambiguity, void *workspace, void *stream);
NM_API int nm_sift_match_u8_host(int n, const unsigned char *const *A, const int *const *nA, int capA,
                                 const unsigned char *const *B, const int *const *nB, int capB, int *const *result,
                                 float ambiguity);

/* ---- k-nearest-neighbour matching of unsigned-char descriptors on the i8 matrix cores (no reference counterpart): for
 * every row of A the k nearest rows of B with their distances, where nm_sift_match_u8_batch_dev gives one index already cut
 * by one ratio. n in [1, NM_MATCH_KNN_U8_MAX_BATCH] pairs in TWO launches on `stream` whatever n and k are (row norms, k-NN);
 * no allocation, no synchronisation, no host read -- capturable into a HIP graph. Pair p (HOST tables of n device pointers):
 *   A[p] / B[p]        capA x 128 / capB x 128 unsigned chars, row-major, 16-byte aligned (out_u8 of the finish);
 *   d_nA[p], d_nB[p]   DEVICE ints: nA = clip(*d_nA[p], 0, capA), nB = clip(*d_nB[p], 0, capB). Rows beyond them are never
 *                      read. A pair with nA <= 0 or nB <= 0 is a no-op;
 *   index[p]           device, capA x k ints, row-major; rows at and beyond nA are not written;
 *   distance[p]        device, capA x k ints, the same layout. The `distance` table may be NULL: indices only.
 * k in [1, NM_MATCH_KNN_U8_MAX_K]. Per pair, all integers:
 *   Distance: d(i, j) = sum over q of (A[i][q] - B[j][q])^2, exact (<= 128 * 255^2 = 8 323 200).
 *   Order: for a row i < nA the candidates j < nB are ordered by (d(i, j), j) ascending -- a total order; the lowest index
 *     wins every tie.
 *   Filled slots: with m = min(k, nB), index[p][i * k + s] and distance[p][i * k + s] hold the s-th candidate of that order
 *     and its distance, for s < m.
 *   Empty slots: for m <= s < k the index is -1 and the distance 0x7fffffff.
 * A pair's outputs depend on that pair's inputs alone, never on n, the slot or scheduling (no atomics). Column 0 of index
 * and distance is the matcher's first minimum and min1; columns 0 and 1 of a k >= 2 call put through the matcher's last step
 * (min2 = 2139095040.0f when nB == 1) give nm_sift_match_u8_batch_dev's result for any ambiguity.
 * workspace: device, 16-byte aligned, nm_sift_match_knn_u8_workspace_bytes(n, capA, capB) bytes (0 for arguments out of
 * range; the matcher's figure), no contents expected or preserved.
 * Returns hipErrorInvalidValue, before anything is launched or dereferenced, for k not in [1, 8], n not in [1, 64], capA or
 * capB not in [1, 2^22), a NULL A, d_nA, B, d_nB, index or workspace, a NULL among the first n entries of one of those
 * tables or of a `distance` table that was given, or a descriptor pointer or workspace that is not 16-byte aligned.
 * nm_sift_match_knn_u8_host: the same with every pointer in host memory (no alignment rule), no workspace and no stream: a
 * plain loop with sorted insertion on (d, j), the same argument checks, results identical to the device entry's.        */
#define NM_MATCH_KNN_U8_MAX_BATCH 64
#define NM_MATCH_KNN_U8_MAX_K 8
NM_API size_t nm_sift_match_knn_u8_workspace_bytes(int n, int capA, int capB);
NM_API int nm_sift_match_knn_u8_batch_dev(int n, const unsigned char *const *A, const int *const *d_nA, int capA,
                                          const unsigned char *const *B, const int *const *d_nB, int capB, int k,
                                          int *const *index, int *const *distance, void *workspace, void *stream);
NM_API int nm_sift_match_knn_u8_host(int n, const unsigned char *const *A, const int *const *nA, int capA,
                                     const unsigned char *const *B, const int *const *nB, int capB, int k,
                                     int *const *index, int *const *distance);

/* ---- Mutual-nearest-neighbour filtering of a match list over unsigned-char descriptors on the i8 matrix cores: the
 * cross-check of the byte pipeline (finish -> nm_sift_match_u8_batch_dev -> this -> RANSAC), no reference counterpart. It is
 * nm_sift_match_mutual_batch_dev_f32 on bytes: given pair k's match list, a match i -> j is kept only when i is also the
 * best row of A for column j. n in [1, NM_MATCH_MUTUAL_U8_MAX_BATCH] pairs in THREE launches on `stream` whatever n is
 * (claims with the row norms, scan, counts); no allocation, no synchronisation, no host read -- capturable into a HIP graph
 * behind the matcher. Pair k (tables of n pointers, the tables in HOST memory):
 *   A[k] / B[k]        capA x 128 / capB x 128 unsigned chars, row-major, 16-byte aligned (out_u8 of the finish);
 *   d_nA[k], d_nB[k]   DEVICE ints, the row counts: nA = clip(*d_nA[k], 0, capA), nB = clip(*d_nB[k], 0, capB). Rows beyond
 *                      them are never read;
 *   matches[k]         device, capA ints: the list to filter (entries at and beyond nA are never read).
 * Per pair, all integers:
 *   Distance: d(i, j) = sum over q of (A[i][q] - B[j][q])^2, exact (<= 128 * 255^2 = 8 323 200 < 2^23).
 *   Claim: row i < nA claims column j = matches[k][i] when 0 <= j < nB. Any other value (-1, below -1, >= nB) is no claim.
 *   Keep: with tau = d(i, j), the claim is kept exactly when no i' < nA has d(i', j) < tau and no i' < i has
 *     d(i', j) == tau: i is the first minimum of column j in an ascending scan with strict <.
 *   There is no NaN case: bytes have none, every distance is a number and every claim has a tau.
 * Outputs: result[k] (device, capA ints; ALL capA entries are written: j for a kept claim, else -1, -1 beyond nA; it may
 * alias no input), count (device, n ints: entries >= 0 of result[k]), forward_distance (optional table, may be NULL:
 * forward_distance[k] device, capA floats = (float)tau, which is exact, for a claiming row and +inf otherwise). A pair with
 * nA <= 0 or nB <= 0 still gets its result filled with -1, its forward distances with +inf and count 0. The kept matches
 * of a pair are injective. result[k] can go to nm_ransac_batch_dev_f32, nm_ransac_refit_batch_dev_f32 and nm_align_points
 * as matches[k] as it is. A pair's outputs depend on that pair's inputs alone, never on n, on the pair's slot or on
 * scheduling (no atomics; a beaten claim's -1 may be stored by several workgroups, always the same value).
 * Equivalence: result, count and forward_distance equal those of nm_sift_match_mutual_batch_dev_f32 on float copies of the
 * same bytes, bit for bit: differences are <= 255, squares <= 65 025 and partial sums < 2^24, so every step of that
 * entry's fmaf chain is exact and its NaN rules never apply.
 * workspace: device, 16-byte aligned, nm_sift_match_mutual_u8_workspace_bytes(n, capA, capB) bytes (0 for arguments out of
 * range), no contents expected or preserved.
 * Returns hipErrorInvalidValue, before anything is launched or dereferenced, for n not in [1, 64], capA or capB not in
 * [1, 2^22), a NULL required pointer (every argument but forward_distance and stream), a NULL among the first n entries of
 * a table, or a descriptor pointer or workspace that is not 16-byte aligned.
 * nm_sift_match_mutual_u8_host: the same with every pointer in host memory (nA[k] / nB[k] point to host ints, no alignment
 * rule), no workspace and no stream: a plain loop over int distances with the same claim and keep predicates and the same
 * argument checks; results identical to the device entry's.                                                            */
#define NM_MATCH_MUTUAL_U8_MAX_BATCH 64
NM_API size_t nm_sift_match_mutual_u8_workspace_bytes(int n, int capA, int capB);
NM_API int nm_sift_match_mutual_u8_batch_dev(int n, const unsigned char *const *A, const int *const *d_nA, int capA,
                                             const unsigned char *const *B, const int *const *d_nB, int capB,
                                             const int *const *matches, int *const *result, int *count,
                                             float *const *forward_distance, void *workspace, void *stream);
NM_API int nm_sift_match_mutual_u8_host(int n, const unsigned char *const *A, const int *const *nA, int capA,
                                        const unsigned char *const *B, const int *const *nB, int capB,
                                        const int *const *matches, int *const *result, int *count,
                                        float *const *forward_distance);

/* ---- Homography-guided matching of unsigned-char descriptors: the guided stage of the byte pipeline (finish ->
 * nm_sift_match_u8_batch_dev -> nm_sift_match_mutual_u8_batch_dev -> RANSAC -> refit -> this -> refit), no reference
 * counterpart. It is nm_sift_match_guided_batch_dev_f32 on bytes: the argument list is that entry's, except that A[k] / B[k]
 * are capA x 128 / capB x 128 unsigned chars, row-major, 16-byte aligned (out_u8 of the finish). n in
 * [1, NM_MATCH_GUIDED_U8_MAX_BATCH] pairs in THREE launches on `stream` whatever n is (pair slots 0-31, slots 32-63, the
 * counts); no workspace, no allocation, no synchronisation, no host read, no atomics -- capturable into a HIP graph behind
 * the refit. Rows of A beyond nA and rows of B beyond nB are never read.
 * Semantics: result[k], count[k] and best_distance[k] are what nm_sift_match_guided_batch_dev_f32 writes for the same pair
 * when A and B are float copies of the bytes, bit for bit. In full:
 *   Unusable pair, valid rows and gate: those of the fp32 entry, unchanged, on the fp32 coordinates and H (status_in[k] != 1
 *     or a non-finite H_k: result -1, count 0, best_distance +inf; valid rows i < nA with ax[i] >= 0; the gate is
 *     nmr_is_inlier's fp32 sequence with the projection computed once per row; a NaN passes no gate).
 *   Distance: d(i, j) = sum over q of (A[i][q] - B[j][q])^2, an exact integer <= 128 * 255^2 = 8 323 200 < 2^23, hence an
 *     exact float too. (The kernel forms it as |a|^2 + |b|^2 - 2 a.b in unsigned 32-bit arithmetic, every term < 2^23; the
 *     order of summation is free. The fp32 entry's fmaf chain is exact on such values: differences <= 255, partial sums
 *     < 2^24.)
 *   Decision: get_sift_matches' scan as the fp32 entry states it, on (float)d over the gated candidates in ascending j: the
 *     first one sets min1 and the index, min2 starts at 2139095040.0f, a later d < min1 moves min1 to min2 and takes its
 *     place, else d < min2 replaces min2 (strict <). result = index when min2 > 0 and min1 / min2 < ambiguity (fp32
 *     divide) and min1 < max_distance, else -1; -1 also without a gated candidate. With a gate that passes everything and
 *     max_distance = +inf the result equals nm_sift_match_u8_batch_dev's on a result pre-filled with -1 (nB >= 1).
 * Outputs: result[k] (device, capA ints; ALL capA entries are written, -1 beyond nA), count (device, n ints: entries >= 0 of
 * result[k]), best_distance (optional table, may be NULL: best_distance[k] device, capA floats = (float)min1, +inf for a row
 * without a gated candidate). A pair's outputs depend on that pair's inputs alone, never on n, the slot or scheduling.
 * Returns hipErrorInvalidValue, before anything is launched or dereferenced, for what the fp32 entry refuses (n not in
 * [1, 64], capA or capB not in [1, 2^22), a non-finite radius2 or ambiguity, a NaN max_distance, a NULL required pointer --
 * every argument but status_in, best_distance and stream -- or a NULL among the first n entries of a table) and for a
 * descriptor pointer that is not 16-byte aligned.
 * nm_sift_match_guided_u8_host: the same with every pointer in host memory (nA[k] / nB[k] point to host ints, no alignment
 * rule), compiled from the same functions (csrc/nm_match_guided_math.hpp, csrc/nm_match_guided_u8_math.hpp): host and
 * device results are identical bit for bit.                                                                            */
#define NM_MATCH_GUIDED_U8_MAX_BATCH 64
NM_API int nm_sift_match_guided_u8_batch_dev(int n,
                                             const unsigned char *const *A, const float *const *ax, const float *const *ay,
                                             const int *const *d_nA, int capA,
                                             const unsigned char *const *B, const float *const *bx, const float *const *by,
                                             const int *const *d_nB, int capB,
                                             const float *H, const int *status_in, float radius2, float ambiguity,
                                             float max_distance, int *const *result, int *count,
                                             float *const *best_distance, void *stream);
NM_API int nm_sift_match_guided_u8_host(int n,
                                        const unsigned char *const *A, const float *const *ax, const float *const *ay,
                                        const int *const *nA, int capA,
                                        const unsigned char *const *B, const float *const *bx, const float *const *by,
                                        const int *const *nB, int capB,
                                        const float *H, const int *status_in, float radius2, float ambiguity,
                                        float max_distance, int *const *result, int *count,
                                        float *const *best_distance);

/* ---- Mosaic plan and batched blend (no reference counterpart: the reference's client places frames on the host and
 * calls transform_blend once per frame). Together with nm_ransac_batch_dev_f32 the chain detect -> match -> RANSAC ->
 * plan -> blend runs on one stream with no host read and can be captured into one HIP graph.
 *
 * nm_mosaic_record: one frame's placement (64 bytes). m comes first, so &records[k] is a valid mat3x3 for
 * nm_transform_blend; nm_transform_blend(canvas, .., frame_k, fw, fh, nw, nh, records[k].m, tx, ty, ..) blends frame k.
 * placed = 1 for a placed frame; an unplaced frame's record is all zero. reserved is written as 0.
 *
 * nm_mosaic_plan_f32: n in [1, NM_MOSAIC_MAX_BATCH] frames. H (device, (n-1) x 9 row-major; may be NULL for n = 1): pair k
 * maps frame-k pixels to frame-(k+1) pixels (H_best of nm_ransac_batch_dev_f32 for A = frame k, B = frame k+1). status
 * (device, n-1 ints) may be NULL: every link valid. Frames are fw x fh, the canvas cw x ch; frame-0 coordinate (0, 0)
 * lands on canvas pixel (ox, oy). M_first (device, 9 floats) maps the mosaic's reference coordinates to frame-0 pixels,
 * NULL = identity; a previous call's last chain row continues a longer sequence. All arithmetic is fp32, fmaf explicit:
 *   M_0 = M_first as given (or I). Link k is valid when (status == NULL || status[k] == 1) and all nine H_k are finite;
 *   then p[r][c] = fmaf(h[r][2], m[2][c], fmaf(h[r][1], m[1][c], h[r][0] * m[0][c])) with m = M_k, and
 *   M_{k+1} = p / p[8] element by element (IEEE division). An invalid link, or p[8] zero or not finite, BREAKS the chain:
 *   frames k+1 .. n-1 get zero records and zero chain rows.
 *   Footprint of a chained frame k: W = invert3x3(M_k) (csrc/nm_warp_math.hpp), the corners (-1, -1), (fw, -1), (-1, fh),
 *   (fw, fh) (the sampler's support) through project(W, x, y). A corner with denominator s <= 0, or a non-finite
 *   projection, leaves frame k ALONE unplaced (zero record; its chain row is still written, later frames keep the chain).
 *   Else box = (floor(min x) - 1, floor(min y) - 1, ceil(max x) + 1, ceil(max y) + 1), exclusive upper edge, in frame-0
 *   coordinates; X0 = clamp(box.x0 + ox, 0, cw), X1 = clamp(box.x1 + ox, 0, cw) in float, then to int (Y alike with oy,
 *   ch); tx = X0, nw = max(X1 - X0, 0), ty, nh alike. A frame wholly off the canvas has nw or nh = 0 and placed = 1.
 *   Local map: m = M_k T(tx - ox, ty - oy): columns 0 and 1 of M_k, column 2 = fmaf(M[r][0], dx, fmaf(M[r][1], dy, M[r][2]))
 *   with dx = tx - ox, dy = ty - oy; project(m, x, y) of local grid pixel (x, y) is the frame-k pixel that
 *   nm_transform_blend samples for canvas pixel (x + tx, y + ty).
 * Outputs (device): records n; chain n x 9 (optional): M_k (frame-0 coordinates -> frame-k pixels); extent 4 floats
 * (optional): (min x0, min y0, max x1, max y1) of the boxes of all placed frames before clipping, in frame-0 coordinates
 * (all 0 when no frame is placed). One launch of one workgroup (one lane chains, one lane per frame places), no
 * allocation, no synchronisation. Returns hipErrorInvalidValue, touching no device memory, for n not in [1, 64], fw, fh,
 * cw or ch not in [1, 32767], |ox| or |oy| >= 2^20, records NULL, or H NULL with n > 1.
 * nm_mosaic_plan_host_f32: the same with every pointer in host memory, compiled from the same functions: host and
 * device results are identical bit for bit.
 *
 * nm_transform_blend_batch: n in [1, NM_MOSAIC_MAX_BATCH] frames into one canvas (uchar4 cw x ch, cw and ch in
 * [1, 32767]) in ONE launch. frames, masks, wts: HOST arrays of n device pointers (fw x fh uchar4 frames; scalar
 * masks / weights of mask_format / wts_format, NM_TEX_U8N or NM_TEX_F32); pointers may repeat. records: device, n. The
 * result equals, bit for bit and on canvas and canvas_wts alike, for k = 0 .. n-1 in order:
 *   nm_transform_blend(canvas, cw, ch, frames[k], fw, fh, records[k].nw, records[k].nh, records[k].m, records[k].tx,
 *                      records[k].ty, masks[k], mask_format, canvas_wts, wts[k], wts_format)
 * for records with |tx|, |ty| < 2^24 and nw, nh in [0, 2^15). Pixels no frame writes keep their bytes. Any record values
 * are safe (rectangles are clipped in 64-bit arithmetic). Each canvas pixel is read once and written at most once: one
 * lane runs the blend step of every covering frame in index order in registers. Returns hipErrorInvalidValue, touching
 * no device memory, for n, cw, ch out of range, fw or fh < 1, a non-scalar format or a NULL pointer.               */
#define NM_MOSAIC_MAX_BATCH 64
typedef struct nm_mosaic_record {
    float m[9];
    int tx, ty, nw, nh;
    int placed;
    int reserved[2];
} nm_mosaic_record;
NM_API int nm_mosaic_plan_f32(int n, const float *H, const int *status, int fw, int fh, int cw, int ch, int ox, int oy,
                              const float *M_first, nm_mosaic_record *records, float *chain, float *extent,
                              void *stream);
NM_API int nm_mosaic_plan_host_f32(int n, const float *H, const int *status, int fw, int fh, int cw, int ch, int ox,
                                   int oy, const float *M_first, nm_mosaic_record *records, float *chain, float *extent);
NM_API int nm_transform_blend_batch(unsigned char *canvas, int cw, int ch, float *canvas_wts, int n,
                                    const unsigned char *const *frames, int fw, int fh, const void *const *masks,
                                    int mask_format, const void *const *wts, int wts_format,
                                    const nm_mosaic_record *records, void *stream);

/* nm_mosaic_place_f32: the placement half of the plan on a GIVEN chain, e.g. chain_out of nm_mosaic_adjust_dev_f32. chain
 * (device, n x 9): M_k, mosaic coordinates -> frame-k pixels; frame_status (device, n ints) may be NULL: every frame given.
 * Frame k is placed exactly as the plan places a chained frame (footprint, box, record, above) when frame_status[k] == 1
 * and all nine M_k are finite and no corner fails; otherwise its record is zero. extent (optional) as for the plan. On
 * the plan's own chain output (frame_status NULL) records and extent equal the plan's bit for bit: the zero rows of a
 * broken chain have no inverse and stay unplaced. One launch of one workgroup; the plan's refusals, and chain NULL.
 * nm_mosaic_place_host_f32: the same with every pointer in host memory, the same functions, identical bit for bit.     */
NM_API int nm_mosaic_place_f32(int n, const float *chain, const int *frame_status, int fw, int fh, int cw, int ch, int ox,
                               int oy, nm_mosaic_record *records, float *extent, void *stream);
NM_API int nm_mosaic_place_host_f32(int n, const float *chain, const int *frame_status, int fw, int fh, int cw, int ch,
                                    int ox, int oy, nm_mosaic_record *records, float *extent);

/* ---- Batched link verification (no reference counterpart): may the map of a frame pair be chained? RANSAC and the refit
 * report "enough rows and H finite"; a map fitted to coincidental matches, a reflected or collapsing map, or a map between
 * frames that do not overlap carries status 1 all the same, and nm_mosaic_plan_f32 would chain through it. This stage
 * looks at H and at the two gray planes. n in [1, NM_LINK_VERIFY_MAX_BATCH] pairs in TWO launches on `stream` whatever n
 * is (accumulate, finalize); no allocation, no synchronisation, no host read -- capturable into a HIP graph behind the
 * refit and in front of the plan.
 * grayA, grayB: HOST tables of n device pointers to fw x fh fp32 gray planes (those nm_frame_ingest_batch_f32 writes and
 * nm_sift_detect_describe_batch reads; values in [0, 255]); pointers may repeat. mask: optional device plane fw x fh shared
 * by all frames; a pixel is seen where mask > 0.5. H: device, n x 9, H_k maps frame-A pixels to frame-B pixels. status_in,
 * inliers: device, n ints each, optional (inliers is e.g. the refit's count).
 * Per pair k four gates; each failed gate sets a bit of reason[k], status_out[k] = (reason[k] == 0):
 *   1 NM_LINK_UNUSABLE      unless (status_in == NULL || status_in[k] == 1) and all nine H_k are finite. Such a pair gets
 *                           reason exactly 1 and zeros in stats; no other gate is looked at.
 *   2 NM_LINK_FEW_INLIERS   when inliers != NULL and inliers[k] < min_inliers.
 *   4 NM_LINK_BAD_GEOMETRY  the corners c0 .. c3 = (0,0), (fw,0), (fw,fh), (0,fh) go through project_den / project
 *                           (csrc/nm_warp_math.hpp; fp32, fmaf explicit, IEEE division). All four denominators must be
 *                           finite and > 0. From the fp32 projections p_c, in fp64: e_c = p_{c+1} - p_c (indices mod 4),
 *                           turn_c = fma(e_c.x, e_{c+1}.y, -(e_c.y e_{c+1}.x)) must be > 0 for all four (convex,
 *                           orientation kept; a NaN fails), S = 0.5 (((t_0 + t_1) + t_2) + t_3) with
 *                           t_c = fma(p_c.x, p_{c+1}.y, -(p_{c+1}.x p_c.y)), r = S / ((double)fw (double)fh), and
 *                           1 / (double)max_area_ratio <= r <= max_area_ratio must hold.
 *   8 NM_LINK_LOW_OVERLAP, 16 NM_LINK_LOW_NCC   photometric, from seven exact integer sums over a lattice of A:
 *     Lattice: pixels (x, y) = (s u + s/2, s v + s/2), u < fw / s, v < fh / s (integer divisions), s = stride.
 *     A value v has the level q = (int)rintf(v * 16.0f) when 0 <= v <= 255 (a NaN has none).
 *     A lattice pixel counts into L when the mask sees it and A's value there has a level qa.
 *     It also counts into N when: den = project_den(H_k, x, y) is finite and > 0; with (xp, yp) = project(H_k, x, y) the
 *     sampler's tex_setup accepts (xp + 0.5f, yp + 0.5f) on B -- the convention of nm_resample_perspective_u8x4: pixel
 *     centres lie at integer coordinates of H's frame, the sampler takes them at + 0.5, so inside it
 *     xb = (xp + 0.5f) - 0.5f, accepted when -1 <= xb < fw and -1 <= yb < fh, i = floor(xb), j = floor(yb),
 *     a = floor((xb - i) 256 + 0.5) / 256, b alike; the four taps (i, j), (i+1, j), (i, j+1), (i+1, j+1) all lie inside B
 *     (0 <= i, i + 1 < fw, 0 <= j, j + 1 < fh; a tap of weight 0 included); the mask sees all four; all four hold a level
 *     q_t. The integer weights are w_t = 65536 {(1-a)(1-b), a(1-b), (1-a)b, ab} (they sum to 65536) and
 *     qb = (w_0 q_0 + w_1 q_1 + w_2 q_2 + w_3 q_3 + 32768) >> 16.
 *     Sums (unsigned 64-bit): L, N, and over the pixels of N: sum qa, sum qb, sum qa^2, sum qb^2, sum qa qb. Integers: they
 *     depend on the pair's inputs alone, never on summation order, n, the pair's slot or scheduling.
 *     Finalize (fp64, fma explicit, IEEE divide and sqrt): overlap = N / L (0 when L = 0); cov = fma(N, Sab, -(Sa Sb)),
 *     va = fma(N, Saa, -(Sa Sa)), vb alike; ncc = cov / sqrt(va vb) when N >= 2, va > 0 and vb > 0, else 0;
 *     gain = cov / va when N >= 1 and va > 0, else 0; bias = fma(-gain, Sa, Sb) / (16 N), mean_a = Sa / (16 N),
 *     mean_b = Sb / (16 N) (all 0 when N = 0): B ~ gain A + bias in gray values.
 *     Bit 8 when overlap < min_overlap, bit 16 when ncc < min_ncc.
 * Outputs (device): status_out n (can go to nm_mosaic_plan_f32, the refit and the guided entries as it is), reason n,
 * stats n x 8 doubles = (N, L, overlap, ncc, gain, bias, mean_a, mean_b); every pair that passes gate 1 gets all eight
 * whatever the other gates say. workspace: device, nm_link_verify_workspace_bytes(n) bytes (0 for n out of range), any
 * contents.
 * Returns hipErrorInvalidValue, touching no device memory, for n not in [1, 64], fw or fh not in [1, 32767], stride not
 * in [1, 64], (fw / stride)(fh / stride) > 2^28 (every sum then stays below 2^53, which fp64 holds exactly), a non-finite
 * max_area_ratio, min_overlap or min_ncc, max_area_ratio < 1, min_inliers < 0, a NULL required pointer or a NULL among the
 * first n table entries.
 * nm_link_verify_host_f32: the same with every pointer in host memory, compiled from the same functions
 * (csrc/nm_link_verify_math.hpp): host and device results are identical bit for bit.
 * nm_link_verify_sums_host_f32: the seven sums themselves (host memory, n x 7, in the order above; zeros for a pair whose
 * H is not finite), for tests and for clients that want their own statistics.                                        */
#define NM_LINK_VERIFY_MAX_BATCH 64
#define NM_LINK_UNUSABLE 1
#define NM_LINK_FEW_INLIERS 2
#define NM_LINK_BAD_GEOMETRY 4
#define NM_LINK_LOW_OVERLAP 8
#define NM_LINK_LOW_NCC 16
NM_API size_t nm_link_verify_workspace_bytes(int n);
NM_API int nm_link_verify_batch_dev_f32(int n, const float *const *grayA, const float *const *grayB, int fw, int fh,
                                        const float *mask, const float *H, const int *status_in, const int *inliers,
                                        int stride, int min_inliers, float max_area_ratio, float min_overlap,
                                        float min_ncc, int *status_out, int *reason, double *stats, void *workspace,
                                        void *stream);
NM_API int nm_link_verify_host_f32(int n, const float *const *grayA, const float *const *grayB, int fw, int fh,
                                   const float *mask, const float *H, const int *status_in, const int *inliers,
                                   int stride, int min_inliers, float max_area_ratio, float min_overlap, float min_ncc,
                                   int *status_out, int *reason, double *stats);
NM_API int nm_link_verify_sums_host_f32(int n, const float *const *grayA, const float *const *grayB, int fw, int fh,
                                        const float *mask, const float *H, int stride, unsigned long long *sums);

/* ---- Batched direct (photometric) refinement of link maps (no reference counterpart). The refit fits a map to keypoint
 * coordinates; this stage moves it by a few inverse compositional Gauss-Newton steps on the level difference of the two
 * gray planes over the verification's lattice, with a gain and a bias between the frames. It belongs between the refit and
 * nm_link_verify_batch_dev_f32, whose conventions it keeps: n in [1, NM_LINK_REFINE_MAX_BATCH] pairs, TWO launches per
 * iteration on `stream` whatever n is (accumulate, solve; 2 x iterations per call), no allocation, no synchronisation, no
 * host read, no kernel that waits for another workgroup -- capturable into a HIP graph.
 * grayA, grayB, mask, status_in: as for the verification. H_in: device, n x 9, H_k maps frame-A pixels to frame-B pixels.
 * model: NM_LINK_REFINE_TRANSLATION (2 parameters), _AFFINE (6) or _HOMOGRAPHY (8). iterations in
 * [1, NM_LINK_REFINE_MAX_ITERATIONS].
 * A pair is usable when (status_in == NULL || status_in[k] == 1) and all nine H_in are finite. The iterate H is kept in
 * fp64 (start: H_in as it is); each iteration walks the lattice under Hf = H rounded to fp32 (the first under H_in):
 *   Lattice, mask rule, levels q and the sample qb of B under Hf: exactly those of the verification (above). A lattice pixel
 *   counts into L as there. It counts into N when it counts into the verification's N and, in addition, its four neighbours
 *   (x-1, y), (x+1, y), (x, y-1), (x, y+1) lie inside A, are seen by the mask and hold a level.
 *   Per pixel of N, all fp64, every product and every sum rounded on its own (no fused multiply-add in the accumulation):
 *     gx = 0.5 (q(x+1, y) - q(x-1, y)), gy = 0.5 (q(x, y+1) - q(x, y-1));  h = 0.5 max(fw, fh), cx = 0.5 (fw - 1),
 *     cy = 0.5 (fh - 1);  X = (x - cx) / h, Y = (y - cy) / h;  gX = h gx, gY = h gy;  d = gX X + gY Y;
 *     J = (gX X, gX Y, gX, gY X, gY Y, gY, -(X d), -(Y d), NM_LINK_REFINE_GAIN_SCALE qa, NM_LINK_REFINE_BIAS_SCALE);
 *     r = qb - qa. The two scales (4 and 8192, powers of two) bring the photometric columns to the magnitude of the
 *     geometric ones on textured frames (gX is about h x 16 x the gray gradient, qa at most 4080).
 *   67 sums, s <- s + term: s[e(i, j)] of J_i J_j for i <= j, e = 10 i - i (i - 1) / 2 + (j - i) (the upper triangle of
 *   J^T J by rows, 55 entries); s[55 + i] of J_i r; s[65] of r r; s[66] = L, one added per pixel of L. N is no sum of its
 *   own: s[54] = BIAS_SCALE^2 N exactly.
 *   SUMMATION ORDER (part of the result; it depends on fw, fh and stride alone, never on n, the pair's slot, the grid or
 *   scheduling). Lattice column u, row v: tile (u / 64, v / 32), tiles numbered by rows, tiles_x = ceil(lw / 64) to a row.
 *   Virtual workgroup g of 256 owns the tiles g, g + 256, .. in ascending order; in a tile, virtual wave w of 4 owns the
 *   rows w, w + 4, .. in ascending order and lane l of 64 the column l. A lane adds its pixels in that order, each sum from
 *   +0. The 64 lanes of a wave are combined by the butterfly of nmw::wave_reduce: for d = 32, 16, .., 1: v_l <- v_l +
 *   v_(l + d) for l < d; v_0 is the wave's sum. A workgroup's row is ((((+0 + w_0) + w_1) + w_2) + w_3), the total
 *   (((+0 + row_0) + row_1) + ..) over the rows g < min(tiles, 256).
 *   Solve (fp64, fma explicit, IEEE divide and sqrt): rms = sqrt(s[65] / N) / 16 (0 when N = 0). N < min_pixels ends the
 *   pair (FEW_PIXELS). Columns c_0 < c_1 < ..: the model's (translation 2, 5; affine 0 .. 5; homography 0 .. 7), then 8
 *   and 9; A_ij = s[e(c_i, c_j)], b_i = s[55 + c_i]. Cholesky by columns j = 0, 1, ..: d = A_jj, then d <- fma(-L_jk,
 *   L_jk, d) for k = 0 .. j-1; a d that is not positive and finite ends the pair (SINGULAR); L_jj = sqrt(d); for i > j:
 *   t = A_ji, t <- fma(-L_ik, L_jk, t) for k = 0 .. j-1, L_ij = t / L_jj. Forward: t = b_i, t <- fma(-L_ik, y_k, t) for
 *   k = 0 .. i-1, y_i = t / L_ii. Backward, i descending: t = y_i, t <- fma(-L_ki, x_k, t) for k = i+1 .., x_i = t / L_ii.
 *   A non-finite x ends the pair (SINGULAR). p_c = x of column c (0 outside the model), alpha, beta = x of columns 8, 9;
 *   gain = fma(GAIN_SCALE, alpha, 1), bias = BIAS_SCALE beta / 16: B ~ gain A + bias in gray values.
 *   Step: W = [[1 + p0, p1, p2], [p3, 1 + p4, p5], [p6, p7, 1]], T = [[1/h, 0, -(cx/h)], [0, 1/h, -(cy/h)], [0, 0, 1]],
 *   Ti = [[h, 0, cx], [0, h, cy], [0, 0, 1]], M = Ti (W T) with (P Q)[r][c] = fma(P[r][2], Q[2][c], fma(P[r][1], Q[1][c],
 *   P[r][0] Q[0][c])). Its size is the largest displacement of the corners (0,0), (fw,0), (fw,fh), (0,fh) under M:
 *   den = fma(M6, x, fma(M7, y, M8)), dx = fma(M0, x, fma(M1, y, M2)) / den - x, dy alike, sqrt(fma(dx, dx, dy dy));
 *   +inf unless every den > 0 and every displacement is finite. Update: H' = H adj(M) (the same product; adj(M) =
 *   det(M) M^-1, elements fma(t4, t8, -(t7 t5)) .. as csrc/nm_warp_math.hpp's invert3x3 without the division), then every
 *   element divided by H'[8], the way the plan divides. A size > max_step (or NaN), or an H' that is not finite in fp32,
 *   is NOT applied and ends the pair (STEP). Else H <- H', and a size < NM_LINK_REFINE_CONVERGED_STEP (2^-7 pixel, half
 *   the sampler's weight step in each direction) ends the pair (CONVERGED). A pair still running after the last
 *   iteration ends there (ITERATIONS). The launches of later iterations skip a pair that has ended: its workgroups leave
 *   on a flag read from the workspace.
 * Outputs (device), written when the pair ends: H_out n x 9 = H rounded to fp32 after the last applied step; a pair with
 * no applied step keeps H_out = H_in bit for bit. status_out[k] = 1 exactly when at least one step was applied (an
 * unusable pair: 0). H_out and status_out go to the verification, the plan, the refit and the guided entries as they are.
 * stats n x NM_LINK_REFINE_STATS doubles = (N, L of the last walk; rms at H_in; rms at the last walk; gain, bias and the
 * step's size in pixels from the last walk's solve, 0 where it solved nothing, the size of a refused step included;
 * steps applied; the end reason NM_LINK_REFINE_END_*). An unusable pair has zeros and END_UNUSABLE.
 * workspace: device, nm_link_refine_workspace_bytes(n) bytes (0 for n out of range; n times the bytes of one pair), 8-byte
 * aligned, any contents.
 * Returns hipErrorInvalidValue, touching no device memory, for n, fw, fh, stride or a lattice outside the verification's
 * bounds, a model outside [0, 2], iterations outside [1, 8], min_pixels < 1, max_step not finite or <= 0, a NULL required
 * pointer or a NULL among the first n table entries.
 * nm_link_refine_host_f32: the same with every pointer in host memory, compiled from the same functions
 * (csrc/nm_link_refine_math.hpp), walking the same summation order: host and device results are identical bit for bit.
 * nm_link_refine_sums_host_f32: the 67 sums of one walk under H (host memory, n x 67 doubles in the order above; zeros
 * for a pair whose H is not finite), for tests.                                                                        */
#define NM_LINK_REFINE_MAX_BATCH 64
#define NM_LINK_REFINE_MAX_ITERATIONS 8
#define NM_LINK_REFINE_TRANSLATION 0
#define NM_LINK_REFINE_AFFINE 1
#define NM_LINK_REFINE_HOMOGRAPHY 2
#define NM_LINK_REFINE_GAIN_SCALE 4.0
#define NM_LINK_REFINE_BIAS_SCALE 8192.0
#define NM_LINK_REFINE_CONVERGED_STEP 0.0078125
#define NM_LINK_REFINE_STATS 9
#define NM_LINK_REFINE_END_ITERATIONS 0
#define NM_LINK_REFINE_END_CONVERGED 1
#define NM_LINK_REFINE_END_UNUSABLE 2
#define NM_LINK_REFINE_END_FEW_PIXELS 3
#define NM_LINK_REFINE_END_SINGULAR 4
#define NM_LINK_REFINE_END_STEP 5
NM_API size_t nm_link_refine_workspace_bytes(int n);
NM_API int nm_link_refine_batch_dev_f32(int n, const float *const *grayA, const float *const *grayB, int fw, int fh,
                                        const float *mask, const float *H_in, const int *status_in, int model, int stride,
                                        int iterations, int min_pixels, float max_step, float *H_out, int *status_out,
                                        double *stats, void *workspace, void *stream);
NM_API int nm_link_refine_host_f32(int n, const float *const *grayA, const float *const *grayB, int fw, int fh,
                                   const float *mask, const float *H_in, const int *status_in, int model, int stride,
                                   int iterations, int min_pixels, float max_step, float *H_out, int *status_out,
                                   double *stats);
NM_API int nm_link_refine_sums_host_f32(int n, const float *const *grayA, const float *const *grayB, int fw, int fh,
                                        const float *mask, const float *H, int stride, double *sums);

/* ---- Global adjustment of a mosaic's frame maps over all links, loop closures included (no reference counterpart). The
 * plan multiplies the sequential maps, so the links' errors add up along the chain and a link between non-consecutive
 * frames cannot be used. This stage is a joint least-squares adjustment (Gauss-Newton with Levenberg damping) of the maps
 * G_k (frame-k pixels -> mosaic coordinates, the inverse of the plan's chain row M_k) over the matched points of all
 * usable links, one anchor frame held fixed. It minimises
 *     sum over usable links l = (a, b), sum over contributing rows i:  || pi(G_a p_i) - pi(G_b q_i) ||^2.
 * (iterations + 1) x (ceil(L / 64) + 1) launches on `stream` (per round one accumulate launch per group of up to 64 links
 * and one assemble-and-solve launch of one workgroup), no allocation, no synchronisation, no host read, no kernel that
 * waits for another workgroup -- capturable into a HIP graph. A round boundary is a launch boundary.
 * n frames in [2, 64], L links in [1, NM_MOSAIC_ADJUST_MAX_LINKS]. link_a, link_b: HOST int arrays of L, indices in
 * [0, n), a != b, any order, repeats allowed, either direction. Per link the six point tables of
 * nm_ransac_refit_batch_dev_f32 (HOST arrays of L device pointers; src is frame a, dst frame b) with its valid rows:
 * nA = clip(*d_nA[l], 0, capA), row i < nA is valid when j = matches[l][i] >= 0 and src_x[l][i] >= 0. mask (device,
 * L x capA bytes, the refit's mask; optional): a valid row contributes when mask[l capA + i] != 0; NULL: every valid row.
 * link_status (device, L ints; optional), e.g. the verification's status_out. chain_in (device, n x 9 fp32): the plan's
 * chain. anchor: host int in [0, n). fw, fh in [1, 32767]; iterations in [1, NM_MOSAIC_ADJUST_MAX_ITERATIONS];
 * min_rows >= 4; damping >= 0 and max_step > 0 (pixels), both finite.
 * Normalisation: h = max(fw, fh) / 2, T = [[1/h, 0, -(cx/h)], [0, 1/h, -(cy/h)], [0, 0, 1]] with cx = fw / 2, cy = fh / 2,
 * Ti = [[h, 0, cx], [0, h, cy], [0, 0, 1]], applied to pixels and mosaic coordinates alike. 3 x 3 products are
 * (P Q)[r][c] = fma(P[r][2], Q[2][c], fma(P[r][1], Q[1][c], P[r][0] Q[0][c])); inv(m) = adj(m) / det(m) element by
 * element, then every element over element [8], with adj as in the link refinement and det = fma(m0, adj0, fma(m1,
 * adj3, m2 adj6)). All fp64 from the fp32 inputs.
 * Participation: G_k = inv(M_k), Gh_k = T (G_k Ti) with every element over its [8]. Frame k participates when its nine
 * chain values, G_k and Gh_k are all finite (the plan's zero rows after a broken link do not). Link l is usable when
 * (link_status == NULL || link_status[l] == 1), both frames participate, and at least min_rows rows contribute at the
 * first iterate; the set of usable links is fixed there. Unknowns: elements 0 .. 7 of Gh_k of every participating frame
 * but the anchor, in ascending frame order. A non-participating anchor ends the call at once (UNUSABLE).
 * Per contributing row, all fp64, every product and every sum rounded on its own (no fused multiply-add), IEEE division:
 *   px = (src_x - cx) / h, py = (src_y - cy) / h, q alike from dst; da = (Ga6 px + Ga7 py) + Ga8, db alike with Gb, q; a
 *   row whose da or db is not finite and > 0 does not contribute. ux = ((Ga0 px + Ga1 py) + Ga2) / da, uy alike from
 *   Ga3..5, v alike from Gb and q; r = u - v. Columns 0 .. 7 are frame a's, 8 .. 15 frame b's:
 *     Jx = (px/da, py/da, 1/da, 0, 0, 0, (-(ux px))/da, (-(ux py))/da,  then the negatives of the same with q, v, db)
 *     Jy = (0, 0, 0, px/da, py/da, 1/da, (-(uy px))/da, (-(uy py))/da,  then the negatives of the same with q, v, db)
 *   NM_MOSAIC_ADJUST_SUMS = 153 sums, s <- s + t: s[e(i, j)], e = 16 i - i (i - 1) / 2 + (j - i) for i <= j (136): t =
 *   Jx_i Jx_j + Jy_i Jy_j, where a product with a structurally zero factor (Jx of columns 3..5 and 11..13, Jy of 0..2 and
 *   8..10) is left out together with its addition, and an entry with no product left is not touched (+0); s[136 + i]:
 *   t = Jx_i rx + Jy_i ry under the same rule; s[152]: t = rx rx + ry ry. The row count is an integer.
 *   SUMMATION ORDER (part of the result; a link's sums depend on the link's inputs and the current maps of its two frames
 *   alone, never on L, n, the link's slot in its launch, or scheduling; no atomics): the refit's. Virtual lane t of 512
 *   adds the rows t, t + 512, .. ascending, each sum from +0. Each group of 64 lanes is combined by the butterfly of
 *   nmw::wave_reduce (for d = 32, 16, .., 1: v_l <- v_l + v_(l + d) for l < d); the eight group totals are added
 *   ascending, ((g0 + g1) + g2) + .. .
 * A round at iterate t = 0 .. iterations accumulates every usable link and then:
 *   cost_t = sum of s[152] over the usable links ascending from +0; rows_t the sum of their counts. Link rms = h
 *   sqrt(s[152] / count). For t > 0, a cost_t that is not <= cost_(t-1), or rows_t != rows_(t-1), restores the iterate
 *   t - 1 and ends the call (COST_ROSE; the step count is taken back by one). Else, if the last applied step was below
 *   NM_MOSAIC_ADJUST_CONVERGED_STEP the call ends (CONVERGED), and at t = iterations it ends (ITERATIONS): the last
 *   accumulation only measures the cost. Hence the final cost never exceeds the initial one.
 *   Assembly: A (dimension N = 8 x unknown frames <= 504) and g; every entry is the sum of the usable links' contributions
 *   (J^T J entries by symmetry, s[136 + i] into g) added in ascending link order from +0; rows and columns of the anchor
 *   are left out. Then A_ii <- A_ii (1 + damping), and a diagonal entry that is exactly 0 becomes 1 (a frame without a
 *   usable link stays where it is).
 *   Cholesky with explicit fma: column j = 0, 1, ..: d = A_jj, d <- fma(-L_jk, L_jk, d) for k = 0 .. j-1 ascending; a d that
 *   is not finite and > 0 ends the call (SINGULAR, no step); L_jj = sqrt(d); for i > j: v = A_ij, v <- fma(-L_ik, L_jk, v)
 *   for k ascending, L_ij = v / L_jj. Forward: v = g_i, v <- fma(-L_ik, y_k, v) for k = 0 .. i-1, y_i = v / L_ii.
 *   Backward, i descending: v = y_i, v <- fma(-L_ki, x_k, v) for k = i+1 .. N-1 ascending, x_i = v / L_ii. A non-finite x
 *   ends the call (SINGULAR). A rank-deficient system (e.g. with damping = 0 a component of frames that no usable link
 *   ties to the anchor) has a pivot that is zero in exact arithmetic; rounded, it comes out non-positive (SINGULAR) or
 *   tiny and positive, which gives a huge finite step and, with it above max_step, STEP. Which of the two is decided by
 *   rounding; in either case no step is applied and no output is NaN.
 *   Step: Gh'_k[q] = Gh_k[q] - x[8 slot_k + q], q < 8. Its size is the largest over the unknown frames and the corners (0,0),
 *   (fw,0), (fw,fh), (0,fh), normalised to (X, Y), of h sqrt(fma(dx, dx, dy dy)) with dx = fma(G'0, X, fma(G'1, Y, G'2)) /
 *   d' - (the same with G) / d, d = fma(G6, X, fma(G7, Y, G8)); +inf unless every d and d' is > 0, every distance finite
 *   and the frame's new chain row (below) finite in fp32. A size > max_step (or NaN) is NOT applied and ends the call
 *   (STEP). Else the iterate t is kept as the previous one and Gh <- Gh'.
 * Outputs (device), written when the call ends: chain_out n x 9 fp32: inv(Ti (Gh_k T)) rounded, for every participating
 * frame but the anchor when at least one step stays applied; the anchor's row, the rows of non-participating frames, and
 * all rows when no step stays applied, are chain_in bit for bit. frame_status n ints: 1 = the frame participates.
 * link_rms L x 2 doubles: the link's rms in pixels at the first and at the final iterate, 0 for a link that is not usable.
 * stats NM_MOSAIC_ADJUST_STATS doubles: first cost, final cost (normalised units squared), contributing rows, usable
 * links, unknown frames, steps applied, the last step's size in pixels (a refused one included), the end reason
 * NM_MOSAIC_ADJUST_END_* (numbered as NM_LINK_REFINE_END_* where they coincide).
 * workspace: device, nm_mosaic_adjust_workspace_bytes(n, L) bytes (0 out of range), 8-byte aligned, any contents: the
 * links' sum rows, A, the current and the previous iterate, the state.
 * Returns hipErrorInvalidValue, touching no device memory, for any range above, a NULL required pointer or a NULL among
 * the first L table entries.
 * nm_mosaic_adjust_host_f32: the same with every pointer in host memory, compiled from the same functions
 * (csrc/nm_mosaic_adjust_math.hpp) over the same virtual lanes and chains: identical bit for bit.
 * nm_mosaic_adjust_sums_host_f32: one link's 153 sums and row count under the normalised maps Ga, Gb (9 doubles each,
 * host memory; mask: the link's capA bytes or NULL), for tests.                                                        */
#define NM_MOSAIC_ADJUST_MAX_LINKS 256
#define NM_MOSAIC_ADJUST_MAX_ITERATIONS 16
#define NM_MOSAIC_ADJUST_SUMS 153
#define NM_MOSAIC_ADJUST_STATS 8
#define NM_MOSAIC_ADJUST_CONVERGED_STEP 0.0078125
#define NM_MOSAIC_ADJUST_END_ITERATIONS 0
#define NM_MOSAIC_ADJUST_END_CONVERGED 1
#define NM_MOSAIC_ADJUST_END_UNUSABLE 2
#define NM_MOSAIC_ADJUST_END_NO_LINK 3
#define NM_MOSAIC_ADJUST_END_SINGULAR 4
#define NM_MOSAIC_ADJUST_END_STEP 5
#define NM_MOSAIC_ADJUST_END_COST_ROSE 6
NM_API size_t nm_mosaic_adjust_workspace_bytes(int n, int L);
NM_API int nm_mosaic_adjust_dev_f32(int n, int L, const int *link_a, const int *link_b, const float *const *src_x,
                                    const float *const *src_y, const int *const *d_nA, int capA,
                                    const float *const *dst_x, const float *const *dst_y, const int *const *matches,
                                    const unsigned char *mask, const int *link_status, const float *chain_in, int anchor,
                                    int fw, int fh, int iterations, int min_rows, double damping, double max_step,
                                    float *chain_out, int *frame_status, double *link_rms, double *stats, void *workspace,
                                    void *stream);
NM_API int nm_mosaic_adjust_host_f32(int n, int L, const int *link_a, const int *link_b, const float *const *src_x,
                                     const float *const *src_y, const int *const *nA, int capA, const float *const *dst_x,
                                     const float *const *dst_y, const int *const *matches, const unsigned char *mask,
                                     const int *link_status, const float *chain_in, int anchor, int fw, int fh,
                                     int iterations, int min_rows, double damping, double max_step, float *chain_out,
                                     int *frame_status, double *link_rms, double *stats);
NM_API int nm_mosaic_adjust_sums_host_f32(const float *src_x, const float *src_y, int nA, int capA, const float *dst_x,
                                          const float *dst_y, const int *matches, const unsigned char *mask, int fw, int fh,
                                          const double *Ga, const double *Gb, double *sums, int *count);

/* ---- Mosaic exposure compensation (no reference counterpart): per-frame, per-channel gains that level the brightness and
 * colour steps between frames of different exposure, between nm_mosaic_adjust_dev_f32 / nm_mosaic_place_f32 and the blend.
 * Three stages: measure (per-link overlap sums from the BGRA frames), solve (gains from the sums), apply (the gained
 * blend). All on `stream` with no allocation, no synchronisation, no host read and no workspace; no kernel waits for
 * another workgroup: measure -> solve -> place -> gained blend can be captured into one HIP graph.
 *
 * nm_mosaic_exposure_sums_dev (measure): n in [2, 64] frames, L in [1, NM_EXPOSURE_MAX_LINKS] links (a link joins two
 * different frames and at least one link is required, so n = 1 is always refused: two frames and one link are the
 * smallest input; the same holds for nm_mosaic_gains_dev). frames: HOST table of n
 * device pointers to fw x fh uchar4 (B, G, R, A) frames as the blend takes them; pointers may repeat. link_a, link_b: HOST
 * int arrays of L (the adjustment's convention), indices in [0, n), a != b. H: device, L x 9 fp32, H_l maps frame-a pixels
 * to frame-b pixels. mask: optional device fp32 plane fw x fh shared by all frames; a pixel is seen where mask > 0.5.
 * link_status: optional device ints, L. stride in [1, 64]; lo, hi bytes, 0 <= lo <= hi <= 255.
 *   Lattice, projection and sampler are those of nm_link_verify_batch_dev_f32 above: lattice pixels (x, y) =
 *   (s u + s/2, s v + s/2), u < fw / s, v < fh / s; a lattice pixel passes when the mask sees it, den = project_den(H_l, x, y)
 *   is finite and > 0, tex_setup accepts (xp + 0.5f, yp + 0.5f) on frame b, the four taps (i, j), (i+1, j), (i, j+1),
 *   (i+1, j+1) all lie inside frame b and the mask sees all four; the integer weights are w_t = 65536 {(1-a)(1-b), a(1-b),
 *   (1-a)b, ab}. For such a pixel and channel c in {B, G, R} (bytes 0, 1, 2 of a uchar4): a_c is frame a's byte at the
 *   pixel, b_c = (w_0 p_0c + w_1 p_1c + w_2 p_2c + w_3 p_3c + 32768) >> 16 from frame b's four tap bytes p_tc. The pixel
 *   COUNTS only when all three a_c and all twelve p_tc lie in [lo, hi] (a tap of weight 0 included; the alpha bytes are not
 *   looked at): a clipped pixel carries no exposure information.
 *   sums: device, L x NM_EXPOSURE_SUMS unsigned 64-bit = (N, Sa_B, Sa_G, Sa_R, Sb_B, Sb_G, Sb_R): the number of counting
 *   pixels and the sums of their a_c and b_c. Integers: they depend on the link's inputs alone, never on L, n, the link's
 *   slot, the launch grouping or scheduling. A link with link_status[l] != 1 or a non-finite H_l gets seven zeros.
 *   TWO launches whatever L is, the first a single workgroup that zeroes the sums (a kernel, not a memset node: see DESIGN.md
 *   section 7, "Median composite"): the frame pointers (512 B) and the link indices (512 B) travel
 *   as kernel arguments; a link's lattice tiles are dealt to up to 256 workgroups, each ending in one vector atomic add per
 *   sum. Returns hipErrorInvalidValue, touching no device memory, for n not in [2, 64], L not in [1, 256], fw or fh not in
 *   [1, 32767], stride not in [1, 64], (fw / stride)(fh / stride) > 2^28, lo < 0, lo > hi, hi > 255, a NULL frames, link_a,
 *   link_b, H or sums, a NULL among the first n frame pointers, a link index outside [0, n) or a link with a == b.
 * nm_mosaic_exposure_sums_host: the same with every pointer in host memory, compiled from the same functions
 * (csrc/nm_mosaic_exposure_math.hpp): identical bit for bit.
 *
 * nm_mosaic_gains_dev (solve): one launch of one workgroup. n, L, link_a, link_b as above; sums: device, L x 7 as measured;
 * link_status optional device ints. Link l is USABLE when (link_status == NULL || link_status[l] == 1) and
 * N_l >= min_pixels. mode NM_EXPOSURE_PER_CHANNEL solves one system per channel c with abar_l = Sa_c / N, bbar_l = Sb_c / N;
 * NM_EXPOSURE_COMMON solves one system with abar_l = ((Sa_B + Sa_G) + Sa_R) / (3 N), bbar alike, and writes its gain to all
 * three channels. All in fp64, fma explicit, IEEE division and sqrt. Per system the gains g minimise
 *     sum over usable links  N_l [ (g_a abar_l - g_b bbar_l)^2 / sigma_n^2 + ((1 - g_a)^2 + (1 - g_b)^2) / sigma_g^2 ]
 *   which is linear and, by the prior, strictly positive definite: no anchor. With N = (double)N_l,
 *   wn = N / (sigma_n sigma_n), wg = N / (sigma_g sigma_g), the n x n matrix M and right-hand side r start at +0 and take
 *   the usable links in ascending order, every entry its own chain s <- s + t or s <- s - t:
 *     M[a][a] += fma(wn abar, abar, wg);  M[b][b] += fma(wn bbar, bbar, wg);  M[a][b] -= (wn abar) bbar;
 *     M[b][a] -= (wn abar) bbar;  r[a] += wg;  r[b] += wg.
 *   A frame with no usable link gets M[k][k] = 1, r[k] = 1: its gain is exactly 1. The Cholesky and the two substitutions
 *   are the written-order ones of the adjustment (csrc/nm_chol_math.hpp): left-looking by columns, element i of column j
 *   v = M[j][i], v = fma(-M[k][i], M[j][k], v) for k < j in order, pivot sqrt(v) (not > 0 or not finite: SINGULAR),
 *   M[j][i] = M[i][j] = v / pivot, r as column n; backward x_i = (r_i - chain) / M[i][i], chain v = fma(-M[i][k], x_k, v)
 *   for k = i+1 .. n-1. The cost of a system at gains g, links ascending from +0:
 *     e = fma(g_a, abar, -(g_b bbar)), da = 1 - g_a, db = 1 - g_b, cost <- cost + fma(wn e, e, wg fma(da, da, db db)).
 *   gains: device, n x 3 fp32 in B, G, R order, clamp((float)g, g_min, g_max). stats: device, NM_EXPOSURE_STATS doubles:
 *   the cost at g = 1 (B, G, R), the cost at the unclamped solution (B, G, R) (COMMON: the one system's figure three
 *   times), the usable links, the frames with at least one usable link, and the end reason NM_EXPOSURE_END_OK, _NO_LINK
 *   (no usable link) or _SINGULAR (a failed pivot or a non-finite solution). On NO_LINK and SINGULAR all gains are 1 and
 *   the second three costs repeat the first three. No output is ever NaN.
 *   Returns hipErrorInvalidValue, touching no device memory, for n not in [2, 64], L not in [1, 256], a NULL link_a, link_b,
 *   sums, gains or stats, a link index outside [0, n) or a link with a == b, min_pixels < 1, sigma_n or sigma_g outside
 *   [NM_EXPOSURE_SIGMA_MIN, NM_EXPOSURE_SIGMA_MAX] (a NaN included; inside it no term can overflow), g_min or g_max not
 *   finite, g_min <= 0, g_min > 1, g_max < 1, or an unknown mode.
 * nm_mosaic_gains_host: the same with every pointer in host memory, compiled from the same functions: identical bit for bit.
 *
 * nm_transform_blend_batch_gain (apply): nm_transform_blend_batch above with gains (device, n x 3 fp32, or NULL). The blend
 * step of frame k becomes blend_sample, then r[c] = r[c] * gains[3 k + c] for c = 0, 1, 2 (one fp32 multiply each), then
 * blend_combine (csrc/nm_warp_math.hpp). Weights, mask, alpha and canvas_wts are untouched: canvas_wts equals the ungained
 * call's for any gains. nm_u8_sat does the clipping: on a canvas pixel of weight 0 the stored byte is
 * nm_u8_sat(r[c] g 255.9999f), so a gain of 0 stores 0 (what a black frame would, on every pixel) and a byte is 255 as soon as
 * r[c] g 255.9999f >= 255; gains are not range-checked (a negative or NaN product stores 0 there). One launch; each
 * canvas pixel is read once and written at most once. With gains == NULL, or every gain exactly 1.0f, canvas and canvas_wts
 * equal nm_transform_blend_batch's bit for bit (x * 1.0f == x). The refusals are nm_transform_blend_batch's.            */
#define NM_EXPOSURE_MAX_LINKS 256
#define NM_EXPOSURE_SUMS 7
#define NM_EXPOSURE_STATS 9
#define NM_EXPOSURE_PER_CHANNEL 0
#define NM_EXPOSURE_COMMON 1
#define NM_EXPOSURE_END_OK 0
#define NM_EXPOSURE_END_NO_LINK 1
#define NM_EXPOSURE_END_SINGULAR 2
#define NM_EXPOSURE_SIGMA_MIN 1e-6
#define NM_EXPOSURE_SIGMA_MAX 1e6
NM_API int nm_mosaic_exposure_sums_dev(int n, int L, const unsigned char *const *frames, const int *link_a,
                                       const int *link_b, int fw, int fh, const float *mask, const float *H,
                                       const int *link_status, int stride, int lo, int hi, unsigned long long *sums,
                                       void *stream);
NM_API int nm_mosaic_exposure_sums_host(int n, int L, const unsigned char *const *frames, const int *link_a,
                                        const int *link_b, int fw, int fh, const float *mask, const float *H,
                                        const int *link_status, int stride, int lo, int hi, unsigned long long *sums);
NM_API int nm_mosaic_gains_dev(int n, int L, const int *link_a, const int *link_b, const unsigned long long *sums,
                               const int *link_status, int min_pixels, double sigma_n, double sigma_g, float g_min,
                               float g_max, int mode, float *gains, double *stats, void *stream);
NM_API int nm_mosaic_gains_host(int n, int L, const int *link_a, const int *link_b, const unsigned long long *sums,
                                const int *link_status, int min_pixels, double sigma_n, double sigma_g, float g_min,
                                float g_max, int mode, float *gains, double *stats);
NM_API int nm_transform_blend_batch_gain(unsigned char *canvas, int cw, int ch, float *canvas_wts, int n,
                                         const unsigned char *const *frames, int fw, int fh, const void *const *masks,
                                         int mask_format, const void *const *wts, int wts_format,
                                         const nm_mosaic_record *records, const float *gains, void *stream);

/* ---- Two-band mosaic blend (no reference counterpart): the step after gain compensation in Brown & Lowe's pipeline. Low
 * frequencies are mixed smoothly across a seam, high frequencies come from ONE frame, the one of largest weight.
 * Everything runs on `stream` with no allocation, no synchronisation and no host read, no kernel waits
 * for another workgroup, the launch count does not depend on n: capturable into a HIP graph behind nm_mosaic_place_f32 and
 * nm_mosaic_gains_dev.
 *
 * DEFINITION. For frame k with a placed record (m, tx, ty, nw, nh) and local pixel (x, y), 0 <= x < nw, 0 <= y < nh:
 *   ok, r, w = blend_sample(m, frame k, mask k, weights k, x, y), exactly as the batched blend calls it
 *   (csrc/nm_warp_math.hpp); C_k[c] = r[c] * gains[3 k + c] for c = 0, 1, 2 (one fp32 multiply, as in the gained blend; no
 *   multiply when gains == NULL); the validity is v_k = ok && w > 0; where v_k is false, C_k = 0 and w_k = 0. A frame is
 *   USED when it is placed, nw > 0, nh > 0 and nw * nh (in 64-bit) <= tile_cap; every other frame is skipped, everywhere.
 *   The tile of a used frame holds (C_B, C_G, C_R, w) for EVERY local pixel, on the canvas or not.
 *   Label. For each canvas pixel inside at least one used rectangle, k* is the used frame with the largest w_k there,
 *   ties to the lowest index; "none" when no frame is valid there. I_k = (k* == k); I_k = 0 off the canvas.
 *   Low band. g[0..R], R in [0, NM_BANDS_MAX_RADIUS]: t_i = exp(-i^2 / (2 sigma^2)), S = t_0 + 2 (t_1 + .. + t_R) summed in
 *   ascending i, g[i] = (float)(t_i / S), all in double on the HOST (nm_mosaic_bands_taps returns them); the taps travel
 *   as kernel arguments and exp is never evaluated on the device. Per frame, five planes are blurred over its own
 *   nw x nh rectangle with zeros outside it, rows first, then columns:  L_k = g * (v_k C_k) (three channels),
 *   V_k = g * v_k,  M_k = g * I_k. One pass of one plane s at one pixel is (csrc/nm_mosaic_bands_math.hpp, tap_sum)
 *       acc = g[0] s(0);  for i = 1 .. R:  acc = fma(g[i], s(-i) + s(i), acc)
 *   in fp32, nothing left to contraction. l_k = L_k / V_k where v_k holds (V_k >= g[0]^2 > 0 there).
 *   Compose. For a labelled canvas pixel, over the used frames valid at that pixel (v_k) in index order, k* included:
 *       num_c = fma(M_k, l_k,c - l_k*,c, num_c),  den = den + M_k      (both from 0)
 *       out_c = C_k*,c + num_c / den;   the stored byte is nm_u8_sat(out_c * 255.9999f), alpha 255
 *   canvas_wts, if given, receives w_k*. Unlabelled pixels (and every pixel outside all used rectangles) keep their bytes
 *   and their weight; a labelled pixel is overwritten, not accumulated into. den > 0 wherever a label exists (the centre
 *   taps). Where only one frame has M_k > 0 (single coverage, or more than R pixels, in both axes' maximum norm, from any
 *   label change inside the frame) num is exactly 0 and the pixel is that frame's own sample bit for bit; R = 0 is exact
 *   winner-take-all.
 *
 * nm_mosaic_warp_tiles (device only, ONE launch): frames, masks, wts (HOST tables of n device pointers), fw, fh, the
 *   formats, records and gains (device; gains may be NULL) as nm_transform_blend_batch_gain takes them. tiles: device,
 *   16-byte aligned, n x tile_cap x 4 floats; frame k owns the slot at k * tile_cap pixels, pixel (x, y) at y * nw + x;
 *   nothing is written outside a used frame's first nw * nh pixels, nothing at all for a skipped frame. stats: device,
 *   NM_BANDS_STATS ints: used frames, skipped frames.
 *   Refused with hipErrorInvalidValue before any device memory is touched: n outside [1, NM_MOSAIC_MAX_BATCH], fw or fh
 *   outside [1, 32767], a format other than NM_TEX_U8N / NM_TEX_F32, tile_cap outside [1, 2^30], a NULL table, table
 *   entry, records, tiles or stats, tiles not 16-byte aligned.
 * nm_mosaic_bands_dev (label, row blur, column blur, compose: FOUR launches whatever n is, no memset node): tiles and
 *   records as above; canvas uchar4 cw x ch, cw and ch in [1, 32767]; canvas_wts fp32 cw x ch or NULL; R, sigma (sigma
 *   is not read when R == 0). workspace: device, 16-byte aligned, nm_mosaic_bands_workspace_bytes(n, tile_cap, cw, ch)
 *   bytes (0 out of range), any contents: the label plane (one byte per canvas pixel, rounded up to 256 bytes), then
 *   2 x n x tile_cap x 20 bytes of blurred planes.
 *   Refused the same way: n, tile_cap, cw or ch out of range, R outside [0, NM_BANDS_MAX_RADIUS], R > 0 with a sigma that
 *   is not finite and positive, a NULL tiles, records, canvas or workspace, tiles or workspace not 16-byte aligned.
 * nm_mosaic_bands_host: the same with every pointer in host memory, compiled from the same functions: canvas and
 *   canvas_wts identical to the device's bit for bit. The warp launch has no host twin (the sampler is device code).   */
#define NM_BANDS_MAX_RADIUS 32
#define NM_BANDS_STATS 2
NM_API size_t nm_mosaic_bands_workspace_bytes(int n, long long tile_cap, int cw, int ch);
NM_API int nm_mosaic_bands_taps(int R, double sigma, float *g);
NM_API int nm_mosaic_warp_tiles(int n, const unsigned char *const *frames, int fw, int fh, const void *const *masks,
                                int mask_format, const void *const *wts, int wts_format, const nm_mosaic_record *records,
                                const float *gains, float *tiles, long long tile_cap, int *stats, void *stream);
NM_API int nm_mosaic_bands_dev(int n, const float *tiles, long long tile_cap, const nm_mosaic_record *records,
                               unsigned char *canvas, int cw, int ch, float *canvas_wts, int R, double sigma,
                               void *workspace, void *stream);
NM_API int nm_mosaic_bands_host(int n, const float *tiles, long long tile_cap, const nm_mosaic_record *records,
                                unsigned char *canvas, int cw, int ch, float *canvas_wts, int R, double sigma,
                                void *workspace);

/* ---- Median mosaic composite (no reference counterpart): a per-pixel order statistic over the stack of tiles that
 * nm_mosaic_warp_tiles wrote. Whatever shows in fewer than half of the frames valid at a canvas pixel (an instrument, a
 * bubble, a highlight moving over a still background) is rejected there; the feather blend shows it as a ghost and the
 * two-band blend as a patch cut along a seam. ONE launch, plus one single-workgroup launch that zeroes counts only when
 * counts is given (a kernel, not a memset node: see DESIGN.md section 7); on `stream` with no
 * allocation, no synchronisation and no host read, no workspace, no workgroup waits for another: capturable into a HIP
 * graph behind nm_mosaic_place_f32, nm_mosaic_gains_dev and nm_mosaic_warp_tiles.
 *
 * DEFINITION. tiles, tile_cap and records as nm_mosaic_bands_dev takes them.
 *   Frames and samples. Frame k is USED exactly as in the two-band blend: placed, nw > 0, nh > 0 and nw * nh (in 64-bit) <=
 *   tile_cap. For canvas pixel (X, Y) and a used frame whose rectangle [tx, tx + nw) x [ty, ty + nh) (clipped to the canvas
 *   in 64-bit) contains it, the sample is t_k = tiles[k * tile_cap + (Y - ty) * nw + (X - tx)] = (C_B, C_G, C_R, w).
 *   Key. y_k = (0.07f * C_B + 0.72f * C_G) + 0.21f * C_R: three fp32 products and two fp32 sums, each rounded, no fma
 *   (numpy float32 reproduces it bit for bit).
 *   Validity. v_k = w > w_min && w <= FLT_MAX && y_k is finite. m is the number of valid frames at the pixel. Where
 *   m == 0, every output at that pixel keeps its contents.
 *   Median frame. rank(k) = #{ valid j : y_j < y_k, or y_j == y_k and j < k }: a total order (+0 and -0 are equal keys
 *   and fall to the index), so any selection algorithm gives the same answer. k~ is the valid frame of rank
 *   floor((m - 1) / 2), the LOWER median.
 *   Inliers. A valid k is an inlier when fabsf(y_k - y_k~) <= tau, with one fp32 subtraction. s is the number of inliers;
 *   k~ is one, so s >= 1.
 *   Modes. NM_MEDIAN_SELECT: out = C_k~ and the weight written is w_k~. NM_MEDIAN_MEAN: over the inliers in index order,
 *   from 0, num_c = fmaf(w_k, C_k,c, num_c), den = den + w_k; out_c = num_c / den and the weight written is den.
 *   Stores. The byte stored is nm_u8_sat(out_c * 255.9999f), alpha 255. canvas_wts (optional, fp32 cw x ch) receives the
 *   weight; support (optional, unsigned char cw x ch) receives s; label (optional, unsigned char cw x ch) receives k~. A
 *   pixel with m > 0 is overwritten, not accumulated into.
 *   Counts. counts (optional, device, n x 2 unsigned 64-bit; zeroed by the call): counts[2 k] is the number of
 *   canvas pixels at which frame k is valid, counts[2 k + 1] the number at which it is valid but not an inlier. Exact
 *   integers, whatever the scheduling: a client reads from them which frames hold a moving object.
 *   Refused with hipErrorInvalidValue before any device memory is touched: n outside [1, NM_MOSAIC_MAX_BATCH], tile_cap
 *   outside [1, 2^30], cw or ch outside [1, 32767], an unknown mode, w_min negative or not finite, tau negative or NaN
 *   (+inf is allowed: every valid frame is an inlier), a NULL tiles, records or canvas, tiles not 16-byte aligned.
 * nm_mosaic_median_host: the same with every pointer in host memory, compiled from the same functions
 *   (csrc/nm_mosaic_median_math.hpp): every output identical to the device's bit for bit.                             */
#define NM_MEDIAN_SELECT 0
#define NM_MEDIAN_MEAN 1
NM_API int nm_mosaic_median_dev(int n, const float *tiles, long long tile_cap, const nm_mosaic_record *records,
                                unsigned char *canvas, int cw, int ch, float *canvas_wts, int mode, float w_min, float tau,
                                unsigned char *support, unsigned char *label, unsigned long long *counts, void *stream);
NM_API int nm_mosaic_median_host(int n, const float *tiles, long long tile_cap, const nm_mosaic_record *records,
                                 unsigned char *canvas, int cw, int ch, float *canvas_wts, int mode, float w_min, float tau,
                                 unsigned char *support, unsigned char *label, unsigned long long *counts);

/* ---- Frame masks and feather weights (no reference counterpart): per frame and per pixel, what is not scene at all (the
 * black surround of an endoscope's disc, a saturated highlight, whatever a shared base plane rules out) and how much to
 * trust the rest (a feather that falls to 0 towards the nearest such pixel). The planes are the mask / weight inputs of
 * every later stage: nm_sift_arena_set_mask, the `mask > 0.5` planes of link verification, refinement and the exposure
 * sums, masks[k] / wts[k] of nm_transform_blend_batch(_gain) and nm_mosaic_warp_tiles. TWO launches whatever n is, plus one
 * single-workgroup launch that zeroes counts only when counts is given (a kernel, not a memset node: see the median
 * composite above and DESIGN.md section 7); on `stream` with no allocation, no synchronisation and no host read, no
 * workgroup waits for another: capturable into a HIP graph behind nm_frame_ingest_batch_f32.
 *
 * DEFINITION. frames: HOST table of n device pointers to fw x fh uchar4 (BGRA) frames, as nm_frame_ingest_batch_f32 takes
 * them; pointers may repeat. For frame k and pixel p = (x, y):
 *   Photometric test. mx = max(B, G, R) of the byte pixel; alpha is ignored. p is RAW-BAD when mx < lo (dark: outside the
 *   optics) or mx > hi (saturated). lo = 0 turns the dark test off, hi = 255 the bright one.
 *   Seeds. p is a SEED when base != NULL and base[y fw + x] == 0 (base: optional device plane, fw x fh unsigned chars,
 *   shared by all frames, e.g. what nm_resample_mask_u8 made from the undistortion map; unconditional), or when p is
 *   raw-bad and at least min_count pixels of the 3 x 3 window centred on p are raw-bad. The window includes p; window pixels
 *   outside the frame do not count. min_count in [1, 9]; with 1 every raw-bad pixel is a seed. (The despeckle step: one dark
 *   noise pixel does not punch a hole of radius margin.)
 *   Clipped squared distance. S is the set of seeds of frame k and, when border != 0, every integer lattice point outside
 *   [0, fw) x [0, fh). D(p) = min(R R, min over q in S of |p - q|^2): an exact integer in [0, R R], R in [1, 64]. A seed
 *   farther than R in either axis cannot change it.
 *   Outputs. VALID = D(p) > margin margin, margin in [0, R).
 *     masks[k][p] = valid ? 255 : 0 (mask_format NM_TEX_U8N, unsigned char) or valid ? 1.0f : 0.0f (NM_TEX_F32): both
 *       satisfy every consumer's rule.
 *     wts[k][p]   = valid ? (sqrtf((float)D) - (float)margin) / (float)(R - margin) : 0.0f: the square root, the
 *       subtraction and the division are fp32, each correctly rounded, no fma; the value lies in (0, 1].
 *     dist2[k][p] = D (unsigned short).
 *     counts[2 k] = the number of seeds inside frame k, counts[2 k + 1] its number of valid pixels (device, n x 2 unsigned
 *       64-bit, zeroed by the call). Exact integers, whatever the scheduling.
 *   masks, wts, dist2 are HOST tables of n device pointers to fw x fh planes; each of the three tables and counts is
 *   optional (NULL), at least one must be given. Outputs must not overlap each other, the inputs or the workspace.
 *   Input-only dependence. A frame's outputs depend on its pixels, base and the parameters alone: not on n, on its slot, on
 *   the previous contents of any output or of the workspace, or on scheduling.
 *   workspace: device, nm_frame_weights_workspace_bytes(n, fw, fh) bytes (0 for arguments out of range; one byte per pixel
 *   with rows padded to 64, no alignment rule), no contents expected or preserved.
 *   Refused with hipErrorInvalidValue before any device access: n outside [1, NM_FRAME_WEIGHTS_MAX_BATCH], fw or fh outside
 *   [1, 32767], lo or hi outside [0, 255], min_count outside [1, 9], R outside [1, NM_FRAME_WEIGHTS_MAX_RADIUS], margin
 *   outside [0, R), an unknown mask_format, no output requested, a NULL frames, a NULL among the first n entries of any
 *   given table, a NULL workspace.
 * nm_frame_weights_host: the same with every pointer in host memory, no workspace and no stream, compiled from the same
 *   functions (csrc/nm_frame_weights_math.hpp): every output identical to the device's bit for bit.
 * nm_frame_weights_set_grid_cap (tuning and tests, process-wide): both passes launch min(units, cap) workgroups that stride
 *   over their units; cap >= 1 fixes the cap, any other value restores the default (8 per compute unit). Results are
 *   identical for every cap. Returns the previous setting (0: the default).                                           */
#define NM_FRAME_WEIGHTS_MAX_BATCH 64
#define NM_FRAME_WEIGHTS_MAX_RADIUS 64
NM_API size_t nm_frame_weights_workspace_bytes(int n, int fw, int fh);
NM_API int nm_frame_weights_batch_dev(int n, const unsigned char *const *frames, int fw, int fh,
                                      const unsigned char *base, int lo, int hi, int min_count, int border, int R,
                                      int margin, void *const *masks, int mask_format, float *const *wts,
                                      unsigned short *const *dist2, unsigned long long *counts, void *workspace,
                                      void *stream);
NM_API int nm_frame_weights_host(int n, const unsigned char *const *frames, int fw, int fh, const unsigned char *base,
                                 int lo, int hi, int min_count, int border, int R, int margin, void *const *masks,
                                 int mask_format, float *const *wts, unsigned short *const *dist2,
                                 unsigned long long *counts);
NM_API int nm_frame_weights_set_grid_cap(int cap);

/* ---- Frame quality and keyframe choice (no reference counterpart): which frames of a video go into a mosaic at all. Three
 * entries and their host twins, each on `stream` with no allocation, no synchronisation and no host read, no workgroup
 * waits for another: capturable into a HIP graph behind nm_frame_ingest_batch_f32, nm_frame_weights_batch_dev and
 * nm_mosaic_plan_f32. Every table is a HOST table of device pointers, as in the stages above.
 *
 * nm_frame_quality_batch_dev: exact integer statistics per frame and per cell of a gx x gy grid. TWO launches whatever n is
 * (a kernel that zeroes stats, then one walk over the pixels).
 *   frames: n in [1, NM_FRAME_QUALITY_MAX_BATCH] device pointers to fw x fh uchar4 (BGRA) frames; pointers may repeat.
 *   masks: optional table of n fw x fh planes in mask_format NM_TEX_U8N or NM_TEX_F32. lo, hi in [0, 255]. gx in
 *   [1, min(NM_FRAME_QUALITY_MAX_GRID, fw)], gy in [1, min(NM_FRAME_QUALITY_MAX_GRID, fh)].
 *   DEFINITION. For frame k and pixel p = (x, y):
 *     mx = max(B, G, R); alpha is ignored. Y = (7 B + 72 G + 21 R + 50) / 100 in integer arithmetic, in [0, 255]: the
 *     gray plane's weights as a rounded rational, this stage's own luminance.
 *     ELIGIBLE: no masks, or the mask is valid at p under the `mask > 0.5` rule of the link stages: byte >= 128
 *     (NM_TEX_U8N), value > 0.5f (NM_TEX_F32). DARK: eligible and mx < lo. BRIGHT: eligible and mx > hi. GOOD: eligible and
 *     neither. MEASURED: p and its four edge neighbours lie inside the frame and all five are good.
 *     On measured pixels L = Y(x-1,y) + Y(x+1,y) + Y(x,y-1) + Y(x,y+1) - 4 Y(x,y) and
 *     G2 = (Y(x+1,y) - Y(x-1,y))^2 + (Y(x,y+1) - Y(x,y-1))^2.
 *     Cell of p: ((x gx) / fw, (y gy) / fh), integer division.
 *   stats: device, n x gy x gx x 8 unsigned 64-bit words, zeroed by the call. Per (frame, cell): [0] measured pixels,
 *     [1] sum of Y, [2] of Y^2, [3] of L^2, [4] of G2 over the measured pixels, [5] dark, [6] bright, [7] eligible pixels.
 *   BOUNDS. Per pixel L^2 <= 1020^2 = 1 040 400 and G2 <= 2 x 255^2 = 130 050 fit 32 bits; per frame every sum stays below
 *     32767^2 x 1 040 400 < 2^51 < 2^53, so a double holds each word exactly. All words are exact integers: they do not
 *     depend on scheduling, on n, on the slot a frame sits in or on the previous contents of stats.
 *   Refused with hipErrorInvalidValue before any launch or device access: n outside [1, 64], fw or fh outside [1, 32767],
 *     lo or hi outside [0, 255], gx or gy out of range, an unknown mask_format with masks given, a NULL frames or stats, a
 *     NULL among the first n entries of a given table.
 * nm_frame_quality_host: the same with every pointer in host memory (csrc/nm_frame_quality_math.hpp): identical words.
 * nm_frame_quality_set_grid_cap (tuning and tests, process-wide): the walk launches min(units, cap) workgroups; cap >= 1
 *   fixes the cap, any other value restores the default (8 per compute unit). Results are identical for every cap. Returns
 *   the previous setting (0: the default).
 *
 * nm_keyframe_pick_dev: which frames to keep, ONE launch of one workgroup. Inputs on the device: stats with its gx, gy;
 * chain (n x 9 fp32, row k = M_k mapping mosaic coordinates to frame-k pixels: the chain of nm_mosaic_plan_f32 or
 * nm_mosaic_adjust_dev_f32); frame_status (optional, n ints). Host values: n, fw, fh, keep in [1, 64]; cell_min >= 1
 * (suggested 64), min_pixels >= 0 (1024), max_bad in [0, 1] (0.25), rel in [0, 1] (0.6), w in [0, 8] (2),
 * 0 <= d_min <= d_max finite, in pixels (32, 128), carry.
 *   DEFINITION, every fp operation a single IEEE operation in the written order, no contraction:
 *     Totals: the integer sums over a frame's cells of words [0], [1], [5], [6], [7].
 *     Score: a cell QUALIFIES when its word [0] >= cell_min; its sharpness is (double)[3] / (double)[0]. The frame's score
 *       is the LOWER median of the qualifying cells' sharpness ordered by (value, cell index), 0 without one. With
 *       gx = gy = 1 it is the mean squared Laplacian.
 *     Usable: frame_status is NULL or 1 and the nine chain values are finite and not all zero (else NM_KEYFRAME_STATUS); a
 *       cell qualifies and the total measured count is >= min_pixels (else NM_KEYFRAME_FEW);
 *       (double)(dark + bright) <= max_bad * (double)eligible (else NM_KEYFRAME_BAD).
 *     Blurred: ref_k = the largest score of a usable frame j with |j - k| <= w (0 without one); a usable frame with
 *       score_k < rel * ref_k is NM_KEYFRAME_BLURRED and not usable for the walk. rel = 0 turns the test off.
 *     Motion: d(a, b) with W_a = invert3x3(M_a): for the corners c = (0,0), (fw-1,0), (0,fh-1), (fw-1,fh-1) of frame a,
 *       q = project(M_b, project(W_a, c)) with the functions of the mosaic plan (csrc/nm_warp_math.hpp); d is the largest
 *       |q.x - c.x| or |q.y - c.y| in fp32, +inf when a denominator is <= 0 or a value is not finite.
 *     Walk: the first keyframe is frame 0 when carry != 0, whatever its flags (the previous chunk's last keyframe: a long
 *       video is walked 63 new frames at a time), else the first usable frame. From keyframe `last`, the window closes at the
 *       first usable j > last with d(last, j) > d_max; the candidates are the usable j > last before the closing frame with
 *       d(last, j) >= d_min; the next keyframe is the candidate of the largest score, the lowest index on a tie; with no
 *       candidate and a closing frame it is the closing frame, flagged NM_KEYFRAME_JUMP; with neither the walk ends. It
 *       also ends after keep keyframes; key_count[1] = 1 when another keyframe would have followed.
 *   Outputs (device, every entry written; all but keys and key_count optional): keys[keep] the chosen indices ascending,
 *     -1 beyond the count; key_count[2] = count, truncated; key_status[keep] 1 for a filled slot else 0 (frame_status of
 *     nm_mosaic_place_f32); flags[n] of NM_KEYFRAME_* bits; scores[n x 4] doubles: score, sum Y / measured, (dark + bright)
 *     / eligible (0 for a zero divisor), ref; H_keys[(keep-1) x 9], H_status[keep-1]: H_keys[i] maps keyframe i pixels to
 *     keyframe i+1 pixels: p = M_b W_a with p[3r+c] = fmaf(M_b[3r+2], W_a[6+c], fmaf(M_b[3r+1], W_a[3+c], M_b[3r] W_a[c])),
 *     divided by p[8]; status 1 when both slots are filled, every value is finite and p[8] != 0, else a zero row and 0:
 *     the H and status of nm_mosaic_plan_f32 and the start maps of the link stages on the gathered frames.
 *   Refused with hipErrorInvalidValue before the launch: a host value out of range, d_min > d_max or either not finite,
 *     max_bad or rel outside [0, 1], a NULL stats, chain, keys or key_count.
 * nm_keyframe_pick_host: the same with every pointer in host memory, from the same functions: identical outputs.
 *
 * nm_slots_gather_dev: dst[i], i in [0, keep), receives the `bytes` bytes of src[keys[i]] when keys[i] lies in [0, n), else
 * `bytes` copies of the byte `fill`. src: n device pointers (may repeat), dst: keep device pointers (must not overlap
 * anything), keys on the device. ONE launch; 16-byte words when every pointer and bytes are multiples of 16, bytes
 * otherwise (a matter of speed, not of results). Serves frames, planes, masks, weights, descriptor and coordinate tables and
 * single count words. Refused: n or keep outside [1, 64], bytes outside [1, 2^31), a NULL table or entry, a NULL keys.
 * nm_slots_gather_host: the same with every pointer in host memory.                                                  */
#define NM_FRAME_QUALITY_MAX_BATCH 64
#define NM_FRAME_QUALITY_MAX_GRID 8
#define NM_KEYFRAME_STATUS 1
#define NM_KEYFRAME_FEW 2
#define NM_KEYFRAME_BAD 4
#define NM_KEYFRAME_BLURRED 8
#define NM_KEYFRAME_KEY 16
#define NM_KEYFRAME_JUMP 32
NM_API int nm_frame_quality_batch_dev(int n, const unsigned char *const *frames, int fw, int fh, const void *const *masks,
                                      int mask_format, int lo, int hi, int gx, int gy, unsigned long long *stats,
                                      void *stream);
NM_API int nm_frame_quality_host(int n, const unsigned char *const *frames, int fw, int fh, const void *const *masks,
                                 int mask_format, int lo, int hi, int gx, int gy, unsigned long long *stats);
NM_API int nm_frame_quality_set_grid_cap(int cap);
NM_API int nm_keyframe_pick_dev(int n, const unsigned long long *stats, int gx, int gy, const float *chain,
                                const int *frame_status, int fw, int fh, int keep, long long cell_min, long long min_pixels,
                                double max_bad, double rel, int w, float d_min, float d_max, int carry, int *keys,
                                int *key_count, int *key_status, int *flags, double *scores, float *H_keys, int *H_status,
                                void *stream);
NM_API int nm_keyframe_pick_host(int n, const unsigned long long *stats, int gx, int gy, const float *chain,
                                 const int *frame_status, int fw, int fh, int keep, long long cell_min, long long min_pixels,
                                 double max_bad, double rel, int w, float d_min, float d_max, int carry, int *keys,
                                 int *key_count, int *key_status, int *flags, double *scores, float *H_keys, int *H_status);
NM_API int nm_slots_gather_dev(int n, const void *const *src, int keep, void *const *dst, const int *keys, long long bytes,
                               int fill, void *stream);
NM_API int nm_slots_gather_host(int n, const void *const *src, int keep, void *const *dst, const int *keys, long long bytes,
                                int fill);

/* ---- Gray pyramid and point tracking (no reference counterpart): a pyramidal Lucas-Kanade (KLT) tracker between the gray
 * planes of frame pairs. Its output is the point tables of the stages behind the matcher (src_x / src_y / dst_x / dst_y,
 * matches, a device count), made without descriptors: nm_ransac_batch_dev_f32, nm_ransac_refit_batch_dev_f32, the guided
 * entries and nm_mosaic_adjust_dev_f32 take them as they stand. Two stages and their host twins, each on `stream` with no
 * allocation, no synchronisation and no host read, no workgroup waits for another: capturable into one HIP graph from
 * nm_frame_ingest_batch_f32 to the refit. Every table is a HOST table of device pointers; n in [1, NM_KLT_MAX_BATCH]; a
 * pair's (a frame's) results depend on its own inputs alone, not on n, its slot, scheduling or what the outputs held.
 *
 * nm_gray_pyramid_batch_f32: gray[k] (fw x fh fp32, the ingest's planes) -> pyr[k], ONE block of `levels` planes per
 * frame, so that a pair costs two pointers of the tracker's kernel arguments.
 *   Sizes: w_0 = fw, w_(l+1) = (w_l + 1) >> 1, h alike. Level l starts nm_gray_pyramid_offset(fw, fh, l) floats into the
 *     block: the running sum of w_j h_j over j < l, each term rounded up to a multiple of 4; the block holds
 *     nm_gray_pyramid_floats(fw, fh, levels) floats (the offset of level `levels`; 0 for a refused shape). levels in
 *     [1, NM_KLT_MAX_LEVELS]; refused when the coarsest level would be narrower or lower than 2.
 *   Filter: level 0 is gray[k] bit for bit. With s(t) = the pixel at clamp(2X + t, 0, w_l - 1) of row y of level l,
 *     h(X, y) = (((s(-2) + s(2)) + 4 (s(-1) + s(1))) + 6 s(0)) * 0.0625f, every operation one IEEE binary32 operation, no
 *     contraction; pixel (X, Y) of level l + 1 is the same form over h(X, clamp(2Y + t, 0, h_l - 1)), t = -2 .. 2. Pixel
 *     centres lie at integer coordinates at every level: a level-0 coordinate x is x / 2^l at level l.
 *   Mask pyramid (mask and mask_pyr both given or both NULL; one for all frames): mask is the link stages' fw x fh fp32
 *     plane, a pixel is seen where mask > 0.5. mask_pyr receives nm_gray_pyramid_floats BYTES, level l at the same offset
 *     counted in bytes: level 0 is 1 (seen) or 0, a pixel of level l + 1 is 1 exactly when all 25 clamped taps of level l
 *     are 1; the bytes between levels are 0.
 *   Launches: max(levels - 1, 1) for all n frames (the first also stores level 0) plus one for the mask block.
 *   Refused with hipErrorInvalidValue before any launch or device access: n outside [1, 64], fw or fh outside [1, 32767],
 *     levels out of range or too many for the frame, a NULL gray or pyr or a NULL among their first n entries, exactly one
 *     of mask / mask_pyr NULL. A block must not overlap any input or other block.
 * nm_gray_pyramid_host_f32: the same with every pointer in host memory (csrc/nm_klt_math.hpp): identical bits.
 *
 * nm_klt_track_batch_dev_f32. Per pair k: pyrA[k], pyrB[k] pyramid blocks (pointers may repeat); src_x[k], src_y[k],
 * d_nA[k], capA exactly as nm_ransac_batch_dev_f32 takes them (nA = clip(*d_nA[k], 0, capA), read on the device); mask_pyr
 * (optional) the mask block; H_in (optional, n x 9 fp32 on the device) with status_in (optional, n ints, needs H_in)
 * predicted maps A -> B. Host values: fw, fh, levels as for the pyramid; radius r in [1, NM_KLT_MAX_RADIUS]; iterations in
 * [1, NM_KLT_MAX_ITERATIONS]; eps > 0, max_step > 0, min_eig >= 0, max_residual >= 0, fb_max >= 0, all finite.
 *   DEFINITION. Whatever is summed is an integer, so host, device and any order of summation agree bit for bit; the fp64
 *   steps are single IEEE operations in the written order, no contraction.
 *     Level of a value: q = (int)rintf(v * 16.0f) when 0 <= v <= 255, else the pixel holds no level (a NaN holds none).
 *     Window: a window has a centre c given in fp64; (cx, cy) = ((float)c.x, (float)c.y) is formed ONCE. The window is
 *       outside when not (0 <= cx < w_l and 0 <= cy < h_l). i = floorf(cx), ax = (int)floorf((cx - i) * 256.0f + 0.5f) in
 *       [0, 256], j and ay alike; the four integer weights (256 - ax)(256 - ay), ax (256 - ay), (256 - ax) ay, ax ay sum
 *       to 65536 and are shared by every tap of the window (the verification's sampler, formed once per window).
 *     Sample at tap (u, v), u and v whole numbers: from the pixels (i + u, j + v), (i + u + 1, j + v), (i + u, j + v + 1),
 *       (i + u + 1, j + v + 1): (sum of weight x level + 32768) >> 16. A sample is valid when its four pixels lie inside
 *       the plane, hold a level and, with a mask block, have byte 1 at that level.
 *     Row i of pair k is tried when i < nA, src_x >= 0 and both coordinates are finite, else it is NM_KLT_ABSENT. State in
 *       fp64: p = (src_x, src_y), displacement d.
 *     Start: with H_in given, status_in NULL or status_in[k] == 1 and the nine values of H_k finite:
 *       d = (double)project(H_k, p) - p with project and project_den of csrc/nm_warp_math.hpp on the fp32 coordinates; a
 *       denominator that is not finite and > 0, or a projection that is not finite, loses the row (NM_KLT_START).
 *       Otherwise d = 0.
 *     Descent: d is multiplied by 2^-(levels-1), then for l = levels - 1 .. 0, with p_l = p 2^-l:
 *       Template on plane l of A, window centre p_l: T(u, v) for |u|, |v| <= r, gx = T(u+1, v) - T(u-1, v),
 *         gy = T(u, v+1) - T(u, v-1) (integers, no factor 1/2; the window has radius r + 1 and every sample of it
 *         but the four corners, which enter no difference, must be valid); Gxx = sum gx^2, Gxy = sum gx gy,
 *         Gyy = sum gy^2 over the (2r+1)^2 taps (< 2^34, held in 64 bits).
 *       Texture gate, fp64: det = Gxx Gyy - Gxy Gxy; lam = ((Gxx + Gyy) - sqrt((Gxx - Gyy)^2 + 4 (Gxy Gxy))) / 2. The
 *         window is flat when det is not finite and > 0, or lam / (1024 (2r+1)^2) < min_eig (gray^2 per tap; 1024 = 32^2).
 *       Iteration: on plane l of B, window centre p_l + d: e = sample - T per tap, bx = sum e gx, by = sum e gy (64 bits);
 *         sx = 2 (Gyy bx - Gxy by) / det, sy = 2 (Gxx by - Gxy bx) / det; a step with a non-finite component or
 *         max(|sx|, |sy|) > max_step is refused; else d = d - s, and the level ends when max(|sx|, |sy|) < eps or after
 *         `iterations` steps.
 *       Failures: an invalid template sample or an outside template window, an invalid sample or outside window on B
 *         (NM_KLT_BORDER), a flat window (NM_KLT_FLAT), a refused step (NM_KLT_STEP). At l > 0 the level is skipped: d
 *         returns to its value on entry to the level. At l = 0 the row is lost with that code.
 *       Between levels d is doubled.
 *     Residual: one more evaluation on plane 0 of B at the final d against level 0's template: an invalid sample is
 *       NM_KLT_BORDER; residual = (double)(sum |e|) / (16 (2r+1)^2) in gray values; with max_residual > 0 a residual above
 *       it loses the row (NM_KLT_RESIDUAL).
 *     Result: dst = ((float)(p.x + d.x), (float)(p.y + d.y)).
 *     Forward-backward check (fb_max > 0): the same procedure, residual test included, from B to A with
 *       p' = (double)dst and start displacement -d, ending at d'. The row is lost (NM_KLT_FB) when that track is lost or when
 *       max(|(double)(float)(p'.x + d'.x) - src_x|, the same in y) > fb_max; that maximum, as fp32, is the fb_error.
 *   Outputs (device): dst_x[k], dst_y[k]: capA floats each, ALL written, -1 for a lost or absent row; matches[k]: capA
 *     ints, i for a tracked row i, else -1; count: n unsigned 64-bit words, the tracked rows per pair; optional tables
 *     reason[k] (capA bytes, the NM_KLT_* code, 0 for a tracked row), residual[k] (capA floats, -1 where no residual was
 *     formed) and fb_error[k] (capA floats, -1 where the backward track gave none).
 *   Launches: the shared zeroing kernel on count (not a memset node: CHANGELOG.md, median composite), then one launch per
 *     32 pair slots: ONE for n <= 32, two above (eleven tables of 64 pointers do not fit the 4 KB of kernel arguments).
 *   Refused with hipErrorInvalidValue before any launch or device access: n outside [1, 64], capA outside [1, 2^22), the
 *     pyramid's refusals for fw, fh, levels, radius or iterations out of range, a value that is not finite, eps <= 0,
 *     max_step <= 0, a negative min_eig, max_residual or fb_max, status_in without H_in, a NULL count, a NULL required
 *     table or a NULL among the first n entries of a table that is given.
 * nm_klt_track_host_f32: the same with every pointer in host memory, from the same functions: identical outputs.
 * nm_klt_sums_host (tests): the integer sums of one evaluation at `level`: template window centre (px, py) 2^-level on
 *   pyrA, other window centre that + (dx, dy) on pyrB; sums[6] = Gxx, Gxy, Gyy, bx, by, sum |e|; *flags bit 0: the
 *   template is outside or holds an invalid sample, bit 1: the same of the other window (sums of a flagged window are
 *   not defined).
 * nm_klt_set_grid_cap (tuning and tests, process-wide): the pyramid, mask and tracker launches use min(units, cap)
 *   workgroups; cap >= 1 fixes the cap, any other value restores the default (8 per compute unit). Results are identical
 *   for every cap. Returns the previous setting (0: the default).
 * nm_klt_set_lanes (tuning and tests, process-wide): the lanes of a wave that share a point in the tracker's kernel: 8, 16
 *   or 32 fixes them, any other value restores the default (16). Results are identical for every setting (the sums are
 *   integers). Returns the previous setting (0: the default).                                                           */
#define NM_KLT_MAX_BATCH 64
#define NM_KLT_MAX_LEVELS 6
#define NM_KLT_MAX_RADIUS 7
#define NM_KLT_MAX_ITERATIONS 16
#define NM_KLT_OK 0
#define NM_KLT_ABSENT 1
#define NM_KLT_START 2
#define NM_KLT_BORDER 3
#define NM_KLT_FLAT 4
#define NM_KLT_STEP 5
#define NM_KLT_RESIDUAL 6
#define NM_KLT_FB 7
NM_API size_t nm_gray_pyramid_floats(int fw, int fh, int levels);
NM_API size_t nm_gray_pyramid_offset(int fw, int fh, int level);
NM_API int nm_gray_pyramid_batch_f32(int n, const float *const *gray, int fw, int fh, int levels, float *const *pyr,
                                     const float *mask, unsigned char *mask_pyr, void *stream);
NM_API int nm_gray_pyramid_host_f32(int n, const float *const *gray, int fw, int fh, int levels, float *const *pyr,
                                    const float *mask, unsigned char *mask_pyr);
NM_API int nm_klt_track_batch_dev_f32(int n, const float *const *pyrA, const float *const *pyrB, int fw, int fh, int levels,
                                      const unsigned char *mask_pyr, const float *const *src_x, const float *const *src_y,
                                      const int *const *d_nA, int capA, const float *H_in, const int *status_in, int radius,
                                      int iterations, float eps, float max_step, float min_eig, float max_residual,
                                      float fb_max, float *const *dst_x, float *const *dst_y, int *const *matches,
                                      unsigned long long *count, unsigned char *const *reason, float *const *residual,
                                      float *const *fb_error, void *stream);
NM_API int nm_klt_track_host_f32(int n, const float *const *pyrA, const float *const *pyrB, int fw, int fh, int levels,
                                 const unsigned char *mask_pyr, const float *const *src_x, const float *const *src_y,
                                 const int *const *nA, int capA, const float *H_in, const int *status_in, int radius,
                                 int iterations, float eps, float max_step, float min_eig, float max_residual, float fb_max,
                                 float *const *dst_x, float *const *dst_y, int *const *matches, unsigned long long *count,
                                 unsigned char *const *reason, float *const *residual, float *const *fb_error);
NM_API int nm_klt_sums_host(const float *pyrA, const float *pyrB, const unsigned char *mask_pyr, int fw, int fh, int levels,
                            int level, int radius, double px, double py, double dx, double dy, long long *sums, int *flags);
NM_API int nm_klt_set_grid_cap(int cap);
NM_API int nm_klt_set_lanes(int lanes);

/* ---- Corner detection (no reference counterpart): Shi-Tomasi "good features to track" corners of gray planes, the points
 * to hand to nm_klt_track_batch_dev_f32. The score is the tracker's own level-0 texture gate at integer pixel centres,
 * where the sampler's weights are (65536, 0, 0, 0) and a sample is the pixel's level itself: a corner is a point the tracker
 * will not call NM_KLT_FLAT or NM_KLT_BORDER at level 0. Everything summed is an integer and the fp64 steps are the gate's,
 * so host and device agree bit for bit. The output (x, y, score, a device count) is what nm_sift_select_batch_dev takes
 * (xs, ys, scores, d_counts) to spread the strongest `keep` over a grid, in source order:
 *   ingest -> pyramid -> corners -> select -> track -> RANSAC -> refit
 * on one stream, capturable into one HIP graph, with no host read and no host-made point table.
 *
 * nm_klt_corners_batch_dev_f32. Every table is a HOST table of device pointers, n in [1, NM_KLT_MAX_BATCH].
 *   gray[k]      an fw x fh fp32 plane; a pyramid block is valid (level 0 lies at offset 0 and is the plane bit for bit);
 *   mask         optional, fw x fh bytes, 1 = seen, one for all frames; a mask_pyr block is valid for the same reason;
 *   held_x[k], held_y[k], d_held[k], cap_held   optional, all three tables or none: points the caller already tracks in
 *                frame k, nH = clip(*d_held[k], 0, cap_held) read on the device; cap_held in [1, 2^22);
 *   radius r in [1, NM_KLT_MAX_RADIUS]; nms in [1, NM_KLT_CORNERS_MAX_NMS]; min_eig >= 0 and finite; cap in [1, 2^22).
 *   DEFINITION.
 *     Level: q(x, y) = (int)rintf(v * 16.0f) when 0 <= v <= 255, else the pixel holds no level (a NaN holds none); with
 *       mask, a pixel whose byte is 0 holds no level.
 *     Window: a pixel (x, y) has a window when every pixel (x + u, y + v) with -(r+1) <= u, v <= r+2 lies in the plane and
 *       holds a level: the tracker's template window of radius r + 1 at an integer centre plus its four corner pixels, so
 *       "has a window" implies a valid level-0 template (the converse fails only at those four pixels).
 *     Sums: gx(p) = q(p.x+1, p.y) - q(p.x-1, p.y), gy alike; Gxx = sum gx^2, Gxy = sum gx gy, Gyy = sum gy^2 over the
 *       (2r+1)^2 pixels |u|, |v| <= r: the first three words of nm_klt_sums_host(level 0, px = x, py = y) exactly.
 *       Gxx, Gyy <= 225 x 4080^2 = 3 745 440 000 fit an unsigned 32-bit word and no signed one; |Gxy| has the same bound
 *       (33 bits signed).
 *     Score: a pixel is scored when it has a window and the tracker's texture gate does not call it flat: det = Gxx Gyy -
 *       Gxy Gxy is finite and > 0 and e = lam / (1024 (2r+1)^2) >= min_eig with
 *       lam = ((Gxx + Gyy) - sqrt((Gxx - Gyy)^2 + 4 (Gxy Gxy))) / 2, the gate's fp64 operations in the gate's order; its
 *       score is (float)e, one rounding. Every other pixel has score -1.
 *     Corner: a scored pixel p is a corner when (1) for every other scored pixel p' at Chebyshev distance <= nms,
 *       score(p) > score(p'), or the scores are equal and p comes first in raster order (y, then x); pixels that are not
 *       scored do not compete; and (2) no tried held row lies within Chebyshev distance nms of p, measured from
 *       (rintf(hx), rintf(hy)); a held row i is tried when i < nH, hx >= 0 and both coordinates are finite. Held pixels still
 *       compete as neighbours: only their own corner status is removed.
 *   Outputs (device): a frame's corners in raster order, x[k][j], y[k][j] whole-number floats, score[k][j]; with more than
 *     cap corners the first cap in raster order; d_count[k] = min(total, cap); d_total[k] (optional) = total; both are
 *     always written, 0 is a valid value; rows at and beyond the count are not written. score_plane[k] (optional table):
 *     fw x fh floats, every pixel written. A frame's results depend on its own inputs alone: not on n, its slot,
 *     scheduling, the grid cap or what the outputs or the workspace held before.
 *   workspace: device, nm_klt_corners_workspace_bytes(n, fw, fh) bytes (0 for arguments out of range): a score plane per
 *     frame, a 64-bit word of corner flags per 64 pixels of a row, a byte plane of held marks with a border of 16. No
 *     contents expected or preserved.
 *   Launches: THREE whatever n is (response, non-maximum suppression into the flag words, scan and write), FOUR with held
 *     points (the marks, behind the response pass, which zeroes the mark planes). Nothing else is zeroed: every word the
 *     call reads it has written. The order of the output comes from a scan of per-tile-row counts, never from an atomic.
 *     No allocation, no synchronisation, no host read; no workgroup waits for another.
 *   Refused with hipErrorInvalidValue before any launch or device access: n outside [1, 64], fw or fh outside [1, 32767],
 *     radius, nms, cap or (with held points) cap_held out of range, a min_eig that is negative or not finite, a held triple
 *     given in part, a NULL gray, x, y, score or d_count, a NULL among the first n entries of a given table, a NULL
 *     workspace.
 * nm_klt_corners_host_f32: the same with every pointer in host memory, no workspace and no stream: identical outputs.
 * nm_klt_corners_set_grid_cap (tuning and tests, process-wide): every launch uses min(units, cap) workgroups; cap >= 1 fixes
 *   the cap, any other value restores the default (8 per compute unit). Results are identical for every cap. Returns the
 *   previous setting (0: the default).                                                                                  */
#define NM_KLT_CORNERS_MAX_NMS 16
NM_API size_t nm_klt_corners_workspace_bytes(int n, int fw, int fh);
NM_API int nm_klt_corners_batch_dev_f32(int n, const float *const *gray, int fw, int fh, const unsigned char *mask,
                                        const float *const *held_x, const float *const *held_y, const int *const *d_held,
                                        int cap_held, int radius, int nms, float min_eig, int cap, float *const *x,
                                        float *const *y, float *const *score, int *d_count, int *d_total,
                                        float *const *score_plane, void *workspace, void *stream);
NM_API int nm_klt_corners_host_f32(int n, const float *const *gray, int fw, int fh, const unsigned char *mask,
                                   const float *const *held_x, const float *const *held_y, const int *const *held, int cap_held,
                                   int radius, int nms, float min_eig, int cap, float *const *x, float *const *y,
                                   float *const *score, int *count, int *total, float *const *score_plane);
NM_API int nm_klt_corners_set_grid_cap(int cap);

/* ---- Link proposal: which frame pairs of a sequence to link at all (no reference counterpart). Two steps, both on
 * `stream` with no allocation, no synchronisation and no host read -- capturable into a HIP graph.
 * nm_link_votes_dev_u8: the u8 matcher's ratio test for ALL ordered pairs of n in [1, NM_LINK_PROPOSE_MAX_FRAMES] frames,
 * each pair reduced to a count, in TWO launches whatever n is (row norms once per frame, vote scan on the i8 matrix cores).
 *   desc[k]      HOST table of n device pointers: cap x 128 unsigned chars, row-major, 16-byte aligned (out_u8 of the
 *                finish, out_desc_u8 of the selection). Two slots may name the same table;
 *   d_count[k]   HOST table of n device pointers to DEVICE ints: n_k = clip(*d_count[k], 0, cap). Rows beyond n_k are never
 *                read;
 *   cap          in [1, 2^22);
 *   votes        device, n x n ints, row-major; EVERY entry is written.
 * Semantics: for a != b, votes[a n + b] is the number of rows i < n_a for which nm_sift_match_u8_host on (A = desc[a],
 * nA = n_a, B = desc[b], nB = n_b, ambiguity), with result pre-filled with -1, leaves result[i] >= 0. As one rule: a row
 * counts when it passes the matcher's last step (min1 / min2 < ambiguity with an fp32 divide of the exact integer
 * distances), so a row whose second distance is 0 does not count, and a row against n_b == 1 is tested against
 * min2 = 2139095040.0f and counts. votes[a n + a] = 0; a frame with no rows has zeros in its row and its column. The count
 * does not depend on which of several equal minima comes first. The output depends on the inputs alone: not on the previous
 * contents of votes or the workspace, on n, on the slot a frame sits in (permuting the frames permutes votes) or on
 * scheduling (the only sums are integer sums).
 * workspace: device, 16-byte aligned, nm_link_votes_workspace_bytes(n, cap) bytes (0 for arguments out of range), no
 * contents expected or preserved.
 * Returns hipErrorInvalidValue, before anything is launched or dereferenced, for n not in [1, 64], cap not in [1, 2^22), a
 * NULL desc, d_count, votes or workspace, a NULL among the first n entries of a table, or a descriptor pointer or
 * workspace that is not 16-byte aligned.
 * nm_link_votes_host_u8: the same with every pointer in host memory (no alignment rule), no workspace and no stream: a
 * loop over the ordered pairs through the matcher's host pair function and a count; identical results.
 * nm_link_votes_set_split (tuning, process-wide): the vote scan's grid is (ceil(cap / 256), n, z), the candidate frames of
 * a query wave divided into z parts. z in [1, 64] fixes the number of parts (clipped to n); any other value restores the
 * default, which takes one part when ceil(cap / 256) n reaches 512 workgroups and else as many as reach it. Results are
 * identical for every z. Returns the previous setting (0: the default).
 *
 * nm_link_rank_dev: the vote matrix -> a ranked link list sized for nm_mosaic_adjust_dev_f32, in ONE launch of one
 * workgroup. All integers:
 *   Score: for a < b, score(a, b) = min(votes[a n + b], votes[b n + a]): both directions must agree.
 *   Candidates: the pairs a < b with b - a >= min_gap and score >= min_votes. min_gap >= 1 (2 leaves out the sequential
 *     links), min_votes >= 1.
 *   Order: by (score descending, a ascending, b ascending) -- a total order.
 *   Walk: the candidates are taken in that order. One is accepted when fewer than max_links are accepted so far and, if
 *     per_frame > 0, each of its two frames has fewer than per_frame accepted links; otherwise it is passed over and the
 *     walk goes on. per_frame = 0: no limit per frame; per_frame >= 0.
 *   Outputs (device): link_a, link_b, link_score, max_links ints each, max_links in [1, NM_LINK_PROPOSE_MAX_LINKS]: the
 *     accepted links in acceptance order with their scores; every entry at and beyond the accepted count is -1 / -1 / 0.
 *     *d_links: the accepted count. No output keeps a previous value.
 * Returns hipErrorInvalidValue, before anything is launched or dereferenced, for n not in [1, 64], min_votes < 1,
 * min_gap < 1, per_frame < 0, max_links not in [1, 256] or a NULL pointer.
 * nm_link_rank_host: the same with every pointer in host memory and no stream: a sort and the same walk.
 * The pair tables of the stages that follow are HOST tables of device pointers, so the client reads d_links and the three
 * lists once to build them.                                                                                            */
#define NM_LINK_PROPOSE_MAX_FRAMES 64
#define NM_LINK_PROPOSE_MAX_LINKS 256
NM_API size_t nm_link_votes_workspace_bytes(int n, int cap);
NM_API int nm_link_votes_dev_u8(int n, const unsigned char *const *desc, const int *const *d_count, int cap,
                                float ambiguity, int *votes, void *workspace, void *stream);
NM_API int nm_link_votes_host_u8(int n, const unsigned char *const *desc, const int *const *count, int cap,
                                 float ambiguity, int *votes);
NM_API int nm_link_votes_set_split(int z);
NM_API int nm_link_rank_dev(int n, const int *votes, int min_votes, int min_gap, int per_frame, int max_links,
                            int *link_a, int *link_b, int *link_score, int *d_links, void *stream);
NM_API int nm_link_rank_host(int n, const int *votes, int min_votes, int min_gap, int per_frame, int max_links,
                             int *link_a, int *link_b, int *link_score, int *d_links);

/* ---- Batched frame ingest (no reference counterpart: the reference's client undistorts and converts each frame with
 * its own launches). nm_frame_ingest_batch_f32 turns n camera frames into the fp32 gray planes SIFT reads and,
 * optionally, their undistorted BGRA frames, in ONE launch.
 * frames, gray, undistorted: HOST arrays of n device pointers (gray can be handed straight to
 * nm_sift_detect_describe_batch). Each frame is fw x fh uchar4 (BGRA). One map is shared by all frames (one camera):
 * map_x / map_y are cols x rows floats, e.g. from nm_undistort_map_f32, or any map. Each output is cols x rows.
 *   With a map: undistorted[k] equals nm_resample_map_u8x4(frames[k], map_x, map_y) bit for bit, and gray[k] equals
 *   nm_grayscale_f32 of that uchar4 result bit for bit. gray is always computed from the rounded uchar4 pixel, also
 *   when undistorted is NULL (gray only). For B, G, R and gray this is also what the per-frame channel chain
 *   nm_extract_channel_f32 -> nm_cast_f32_u8 -> nm_resample_undistort_f32 (NM_TEX_U8N) -> nm_put_channel_f32 per
 *   channel, then nm_grayscale_f32, produces; alpha is the sampled alpha, as in resample_2D<uchar4> (the chain's
 *   put_channel(3) writes 255 instead).
 *   Identity mode (map_x == map_y == NULL): a batched nm_grayscale_f32, gray[k] = nm_grayscale_f32(frames[k]). It
 *   requires cols == fw, rows == fh and undistorted == NULL.
 * One launch; no allocation, no synchronisation, no host read, so the call can be captured into a HIP graph. A frame's
 * result does not depend on its slot in the call or on n. Frame pointers may repeat; outputs must not overlap the
 * inputs or each other. Nothing outside each cols x rows output plane is written.
 * Returns hipErrorInvalidValue, before any device access, for n not in [1, NM_INGEST_MAX_BATCH]; fw, fh, cols or rows
 * not in [1, 32767]; frames or gray NULL or holding a NULL among its first n; exactly one of map_x / map_y NULL;
 * identity mode with undistorted != NULL or cols != fw or rows != fh; undistorted non-NULL but holding a NULL.      */
#define NM_INGEST_MAX_BATCH 64
NM_API int nm_frame_ingest_batch_f32(int n, const unsigned char *const *frames, int fw, int fh, const float *map_x,
                                     const float *map_y, int cols, int rows, float *const *gray,
                                     unsigned char *const *undistorted, void *stream);

/* ---- per-frame driver ---- */
/* The per-octave client loop the reference leaves to its caller, run entirely on `stream` with no
 * host synchronisation and no allocation: Gaussian pyramid + DoG + gradients + extrema + ordered compaction +
 * orientations + descriptors of one grayscale fp32 frame. An arena owns every intermediate buffer
 * (replaces PyramidData, sift/pyramidata.cu:24-50) and is bound to one stream at a time. The two helper streams and the
 * events of a call belong to the caller's stream, not to an arena: the library keeps one set per caller stream and device
 * (up to 16; calls on further streams use a set of their first arena's), made when a stream issues its first call -- or,
 * for a call that is being captured, beforehand -- and kept until the process ends.                                */
typedef struct nm_sift_arena nm_sift_arena;
NM_API int nm_sift_arena_create(int width, int height, int capacity, nm_sift_arena **arena);
NM_API void nm_sift_arena_destroy(nm_sift_arena *arena);
NM_API size_t nm_sift_arena_bytes(const nm_sift_arena *arena);
/* The reference's run-time knobs for the calls that follow on this arena. SiftParams::_peak_threshold and
 * _edge_threshold are public fields a client sets between frames (sift/siftparams.h:97-98; read per call by
 * compute_keypoints, sift/siftfunctions.cu:123-125): defaults 0 and 10. edge_threshold must be > 0. All arenas of one
 * batched call must hold the same pair. Host-side setters (no stream operation): they take effect for the calls ENQUEUED
 * afterwards; a HIP graph captured earlier keeps the values it was captured with.                                 */
NM_API int nm_sift_arena_set_params(nm_sift_arena *arena, float peak_threshold, float edge_threshold);
NM_API int nm_sift_arena_get_params(const nm_sift_arena *arena, float *peak_threshold, float *edge_threshold);
/* compute_keypoints_with_mask (sift/siftfunctions.cu:65-98, kernels/keypoint.cu:204-224): detection only where the
 * full-resolution mask, fetched with the reference's bilinear border texture at ((x+0.5) xper, (y+0.5) xper), is >= 1.
 * mask: caller-owned DEVICE plane of exactly the arena's width x height floats, read by every later call until it is
 * replaced; NULL removes it. Per arena: the frames of a batched call may have different masks or none.               */
NM_API int nm_sift_arena_set_mask(nm_sift_arena *arena, const float *mask, int mask_width, int mask_height);
/* Diagnostics of the octave-tail launch (csrc/nm_tail.hip; the octaves >= 2 of a call run as ONE persistent launch whose
 * work items draw tickets): the plan's segments (5 ints each: kind 0 = levels 1..3 / whole plane, 1 = levels 4..5, 2 = detect,
 * 3 = scan + gather, 4 = gradient planes of a whole octave; slot; items per frame; first item per frame; octave) and, when the
 * arena was created under NM_TAIL_TRACE=1 and was the first arena of the last call, 4 words per item of that launch (meta,
 * clock at ticket, at inputs ready, at done; 100 MHz). Returns the items per frame (0: this geometry takes the per-octave
 * launches; < 0: error). Synchronises the device when `out` is given. */
NM_API int nm_sift_arena_tail_trace(const nm_sift_arena *arena, unsigned long long *out, int max_items, int *segments,
                                    int max_segments);
NM_API int nm_sift_arena_tail_segments(const nm_sift_arena *arena);
/* Failure reporting of the octave-tail launch. Every wait inside it is bounded (~2 s); a wait that times out sets a sticky
 * error word, the remaining work items of THAT launch are drained without working, and the launch leaves its state clean for
 * the next call. What the caller sees: d_num_items of every frame of that call reads -1 (outputs of that call are invalid;
 * the device-sized matcher entries treat a negative size as 0), and nm_sift_arena_tail_status -- on the first arena of the
 * call, whose state words the launch used -- writes *status = 1 (0 after a complete launch; synchronises `stream`). The
 * call after a failed one is unaffected. nm_sift_arena_tail_inject_error is a TEST HOOK that sets the sticky word as a
 * timed-out wait would (synchronises the device).                                                                       */
NM_API int nm_sift_arena_tail_status(const nm_sift_arena *arena, int *status, void *stream);
NM_API int nm_sift_arena_tail_inject_error(nm_sift_arena *arena);
/* HOST function: the number of kernel launches one nm_sift_detect_describe[_batch] call of n frames on this arena issues
 * (1080p: 23 for n <= 2, where the octave tail is used; 51 above). */
NM_API int nm_sift_arena_launches_per_call(const nm_sift_arena *arena, int n);
/* HOST function (no device access): the octave-tail plan for a width x height frame whose tail starts at octave T (the frame
 * driver uses T = 2; NM_FRAME_TAIL=1..3 in the environment when an arena is created). segments: 8 ints each (kind, slot, items
 * per frame, first item per frame, octave, 1 if the whole plane is one item, octave width, octave height), in the order in
 * which the launch's tickets run through them -- an item only ever waits for items of EARLIER segments; info: items per
 * frame, LDS bytes of the tail launch, of the scan launch, number of tail octaves. Returns the number of segments; 0 when the
 * geometry is not covered (too few octaves, radii other than the SIFT defaults, LDS) and takes the per-octave launches. */
NM_API int nm_sift_tail_plan(int width, int height, int T, int *segments, int max_segments, int info[4]);
/* HOST function (no device access): the schedule of one nm_sift_detect_describe[_batch] call as the frame driver walks it, for a
 * RESOLVED configuration: num_octaves (1..20); first_tail = first octave of the octave tail, num_octaves without it; split =
 * octaves described early (0: one description pass; with the tail split = first_tail); write_dog (NM_FRAME_DOG; never with the
 * tail); order 0..2 (nm_sift_set_frame_skew; 0 with the tail or a split). ops: six ints per op in issue order -- kind (0 base
 * blur, 1 levels lo..hi, 2 detect + scan + gather, 3 tail, 4 tail scan, 5 describe octaves [lo, hi), 6 record, 7 wait, 8 join:
 * record on the helper stream, the caller's stream waits), stream (0 caller's, 1 side, 2 description), octave, lo, hi, event
 * (-1 none, 0 ev_pyr[octave], 1 ev_top[octave], 2 ev_det, 3 ev_desc, 4 ev_join). At most max_ops ops are written. Returns the
 * number of ops (<= 149), 0 for a configuration the driver never resolves to. Properties: tests/test_frame_plan.py. */
NM_API int nm_sift_frame_plan(int num_octaves, int first_tail, int split, int write_dog, int order, int *ops, int max_ops);
/* HOST function (no device access): the configuration the frame driver resolves a call of n frames to, on arenas of num_octaves
 * octaves whose octave-tail plan starts at octave tail_first (0: no tail plan). selected_order: what nm_sift_set_frame_skew set,
 * -1 for the default. split / cross_min_frames: NM_FRAME_SPLIT_DESCRIBE / NM_FRAME_CROSS_MIN_FRAMES as the call shall see them,
 * < 0 for the process's own. cfg: num_octaves, first_tail, split, write_dog, order -- the arguments of nm_sift_frame_plan.
 * Returns 0, hipErrorInvalidValue for arguments out of range. nm_sift_frame_cross_min_frames: the process's threshold (0: the
 * cross order is never the default). Tests: tests/test_frame_plan_order_default.py. */
NM_API int nm_sift_frame_resolve(int num_octaves, int tail_first, int n, int selected_order, int split, int cross_min_frames,
                                 int cfg[5]);
NM_API int nm_sift_frame_cross_min_frames(void);
/* gray: width*height fp32 on the device. Outputs on the device: desc capacity x 128, x,y capacity (full-resolution
 * coordinates, descriptor.cu:75-77), d_num_items = number of descriptors written (<= capacity,
 * siftfunctions.cu:165-169). kpts (capacity float4) and orients (capacity float2) are optional (NULL).        */
NM_API int nm_sift_detect_describe(nm_sift_arena *arena, const float *gray, float *desc, float *x, float *y,
                                   float *kpts, float *orients, int *d_num_items, void *stream);
/* The same for n <= NM_SIFT_MAX_BATCH frames in ONE launch sequence (arrays of n pointers; the arenas must be distinct
 * and of equal width, height and capacity; kpts, orients, d_num_items may be NULL or hold NULLs). EVERY launch covers
 * all frames of the call (the frame is a grid dimension): a single 1080p frame is only ~4 workgroups per CU at octave
 * 0 and its higher octaves are pure launch latency, a batch fills the chip and shares the ~60 launches. Results are
 * identical to n separate nm_sift_detect_describe calls. No reference counterpart (the reference processes one frame
 * per call sequence, sift/siftfunctions.cu:42-181).
 * STREAM CAPTURE: the call uses events only (no synchronisation, no allocation) and can be captured into a HIP graph on
 * `stream`. Internally it forks the first arena's side stream(s) off `stream` and joins EVERY forked stream back into
 * `stream` directly before it returns (also on an error path). A client that captures around these calls must follow the
 * same rule for its own streams: on ROCm 7.2 a forked stream that is joined into ANOTHER forked stream (s1 -> s2 -> s3,
 * then s3 -> s2 -> s1) crashes the capturing process inside hipStreamEndCapture / instantiate; s1 -> s2, s1 -> s3 or
 * s1 -> s2 -> s3 with s2 -> s1 and s3 -> s1 are safe (tools/capture_shapes.py reproduces both). The same holds for
 * nm_sift_match_batch[_dev]_f32, which run on `stream` alone.                                                           */
#define NM_SIFT_MAX_BATCH 64
NM_API int nm_sift_detect_describe_batch(nm_sift_arena *const *arenas, int n, const float *const *gray,
                                         float *const *desc, float *const *x, float *const *y, float *const *kpts,
                                         float *const *orients, int *const *d_num_items, void *stream);
/* Measurement aid: only the scale-space launches of nm_sift_detect_describe_batch (base blur + every octave's Gaussian
 * levels, DoG planes, gradient planes and decimation), on `stream`, no detection. The planes it leaves in the arenas
 * are those of the last octave. bench.py times this sequence for the whole-pyramid roofline (SURVEY.md 8(d):
 * 108 B per octave-pixel + 36 B for the gradients).                                                              */
NM_API int nm_sift_scale_space_batch(nm_sift_arena *const *arenas, int n, const float *const *gray, void *stream);
/* The same chain with (write_dog = 1, what nm_sift_scale_space_batch does: levels + DoG + gradient planes, the 108 B per
 * octave-pixel yardstick) or without (0) materialised DoG planes. nm_sift_detect_describe[_batch] runs the latter: its
 * detection kernel subtracts consecutive levels itself, so 16 of the chain's 64 written bytes per pixel are never moved.
 * write_dog | 2: the same without the fused gradient planes, i.e. with write_dog = 3 exactly the work of the reference's
 * convolve + compute_dog loops (6 level writes + 5 DoG planes per octave: the 108 B per octave-pixel yardstick alone). */
NM_API int nm_sift_scale_space_batch_ex(nm_sift_arena *const *arenas, int n, const float *const *gray, int write_dog,
                                        void *stream);
/* Pointers into the arena for stage-level inspection (tests, profiling): Gaussian level l (0..5) and DoG d (0..4)
 * planes of the LAST processed octave geometry are overwritten per octave, so these are meaningful only after
 * nm_sift_octave_pyramid().                                                                                      */
NM_API float *nm_sift_arena_level(nm_sift_arena *arena, int level);
NM_API float *nm_sift_arena_dog(nm_sift_arena *arena, int dog);
NM_API float *nm_sift_arena_grad(nm_sift_arena *arena);
/* Gaussian levels 1..5 + DoG 0..4 + gradients 0..2 of one octave whose level 0 already sits in
 * nm_sift_arena_level(arena,0) with geometry ow x oh (the fused pyramid stage, timed by bench.py).            */
NM_API int nm_sift_octave_pyramid(nm_sift_arena *arena, int ow, int oh, void *stream);

#ifdef __cplusplus
}
#endif
#endif
