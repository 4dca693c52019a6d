// mfma_i8_model.hip -- how v_mfma_i32_32x32x32_i8 lays out its operands, probed with exact asymmetric integer data on the
// device the u8 matcher (csrc/nm_match_u8.hip) runs on. The assumed map:
//   A / B: lane l supplies row / column l % 32, k = 16 (l / 32) .. + 15 as the 16 signed bytes of its four registers, byte j
//          of the fragment (register j / 4, bits 8 (j % 4) ..) = k offset j;
//   C / D: register e of lane l = row (e & 3) + 8 (e >> 2) + 4 (l / 32), column l % 32 (the dtype-independent map).
// Probes: (L) random signed bytes over the whole range, A and B unrelated (a transposed operand or accumulator map, or a
// permuted k order on one side only, changes almost every output); (K) one-hot rows that put a single product at each k in
// turn, with a different value per k, so a k order that differs BETWEEN the operands shows even where (L) would sum over it;
// (S) the extremes -128 x -128 x 32 + C and 127 x -128. Every sum is exact in i32.
// Diagnostic only; nothing in the product links it.
//   hipcc --offload-arch=gfx950 -O3 tools/micro/mfma_i8_model.hip -o niftymatch_amd/lib/mfma_i8_model
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e_), __LINE__); exit(1); } } while (0)

// one instruction per wave: A (32 rows x 32 k, signed bytes), B given as Bt (32 columns x 32 k), C and D 32 x 32 ints
__global__ __launch_bounds__(64) void one_mfma(const int8_t *A, const int8_t *Bt, const int *C, int *D, int n)
{
    const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
    for (int t = blockIdx.x; t < n; t += gridDim.x) {
        const i32x4 fa = *reinterpret_cast<const i32x4 *>(A + (size_t)t * 1024 + r * 32 + 16 * h);
        const i32x4 fb = *reinterpret_cast<const i32x4 *>(Bt + (size_t)t * 1024 + r * 32 + 16 * h);
        i32x16 acc;
        for (int e = 0; e < 16; ++e) acc[e] = C[(size_t)t * 1024 + ((e & 3) + 8 * (e >> 2) + 4 * h) * 32 + r];
        acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa, fb, acc, 0, 0, 0);
        for (int e = 0; e < 16; ++e) D[(size_t)t * 1024 + ((e & 3) + 8 * (e >> 2) + 4 * h) * 32 + r] = acc[e];
    }
}

int main()
{
    const int NL = 64;                              // random instructions
    const int N = NL + 2;
    std::vector<int8_t> A((size_t)N * 1024, 0), Bt((size_t)N * 1024, 0);
    std::vector<int> C((size_t)N * 1024, 0), D((size_t)N * 1024, 0);
    uint64_t s = 0x9E3779B97F4A7C15ull;
    auto rnd = [&]() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); };
    for (int t = 0; t < NL; ++t) {
        for (int i = 0; i < 1024; ++i) { A[(size_t)t * 1024 + i] = (int8_t)(rnd() & 255); Bt[(size_t)t * 1024 + i] = (int8_t)(rnd() & 255); }
        for (int i = 0; i < 1024; ++i) C[(size_t)t * 1024 + i] = (int)(rnd() % 2001) - 1000;
    }
    // (K) row m of A is one-hot at k = m with value m + 1; every column of B holds k + 2 at k (+ the column number at k = 0):
    // D[m][n] = (m + 1) (m + 2 + (m == 0 ? n : 0)) only if both operands agree on where k = m sits.
    const int tk = NL;
    for (int m = 0; m < 32; ++m) A[(size_t)tk * 1024 + m * 32 + m] = (int8_t)(m + 1);
    for (int n = 0; n < 32; ++n) for (int k = 0; k < 32; ++k) Bt[(size_t)tk * 1024 + n * 32 + k] = (int8_t)(k + 2 + (k == 0 ? n : 0));
    // (S) extremes
    const int ts = NL + 1;
    for (int m = 0; m < 32; ++m) for (int k = 0; k < 32; ++k) {
        A[(size_t)ts * 1024 + m * 32 + k] = (int8_t)((m & 1) ? 127 : -128);
        Bt[(size_t)ts * 1024 + m * 32 + k] = (int8_t)-128;
    }
    for (int i = 0; i < 1024; ++i) C[(size_t)ts * 1024 + i] = i;

    int8_t *dA, *dB; int *dC, *dD;
    CK(hipMalloc(&dA, A.size())); CK(hipMalloc(&dB, Bt.size())); CK(hipMalloc(&dC, C.size() * 4)); CK(hipMalloc(&dD, D.size() * 4));
    CK(hipMemcpy(dA, A.data(), A.size(), hipMemcpyHostToDevice)); CK(hipMemcpy(dB, Bt.data(), Bt.size(), hipMemcpyHostToDevice));
    CK(hipMemcpy(dC, C.data(), C.size() * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(one_mfma, dim3(N), dim3(64), 0, 0, dA, dB, dC, dD, N);
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(D.data(), dD, D.size() * 4, hipMemcpyDeviceToHost));

    auto wrong = [&](int t0, int t1) {
        int bad = 0;
        for (int t = t0; t < t1; ++t)
            for (int m = 0; m < 32; ++m) for (int n = 0; n < 32; ++n) {
                long long e = C[(size_t)t * 1024 + m * 32 + n];
                for (int k = 0; k < 32; ++k) e += (long long)A[(size_t)t * 1024 + m * 32 + k] * (long long)Bt[(size_t)t * 1024 + n * 32 + k];
                if ((long long)D[(size_t)t * 1024 + m * 32 + n] != e) ++bad;
            }
        return bad;
    };
    const int bl = wrong(0, NL), bk = wrong(tk, tk + 1), bs = wrong(ts, ts + 1);
    printf("(L) random signed bytes, %d outputs : %d differ from the assumed layout\n", NL * 1024, bl);
    printf("(K) one product per k, 1024 outputs : %d differ\n", bk);
    printf("(S) extremes, 1024 outputs          : %d differ (D[0][0] = %d, expected %d)\n", bs, D[(size_t)ts * 1024], 32 * 128 * 128);
    return (bl || bk || bs) ? 1 : 0;
}
