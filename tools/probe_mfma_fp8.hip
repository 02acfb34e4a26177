// probe_mfma_fp8.hip — error of ONE v_mfma_scale_f32_16x16x128_f8f6f4 (e4m3 x e4m3, unit e8m0 scales: the instruction of the fp8
// GEMM, csrc/gemm256.hip) against fp64, in units of 2^-24 * (|c| + sum |a| |b|): the instruction alone, one MFMA per wave, not the
// GEMM.  Operands as the GEMM's: a = e4m3(normal), b = e4m3 bytes of a row quantised to +-448 (normal * 448 / 3.2, saturating).
// Pass 1 starts from c = 0 (the first 128-deep step of a tile), pass 2 from the fp32 result of another wave's pass 1 (every later
// step).  The products of two e4m3 values are exact in fp32, so everything printed is what the instruction's own summation loses.
// The bound in tests/gemm_fp8_ref.py takes twice the larger figure printed here per 128-deep step.
//   hipcc --offload-arch=gfx950 -O2 tools/probe_mfma_fp8.hip -o probe_mfma_fp8 && ./probe_mfma_fp8
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

typedef int v8i __attribute__((ext_vector_type(8)));
typedef float v4f __attribute__((ext_vector_type(4)));

// lane l: A row l & 15 and B column l & 15, k = 32 (l >> 4) .. + 31 (both operands in the same k order); D rows 4 (l >> 4) + i, column l & 15
__global__ __launch_bounds__(64) void probe(const unsigned char* A, const unsigned char* B, const float* Cin, float* D) {
    const int w = blockIdx.x, l = threadIdx.x;
    const v8i a = *reinterpret_cast<const v8i*>(A + ((size_t)w * 16 + (l & 15)) * 128 + (l >> 4) * 32);
    const v8i b = *reinterpret_cast<const v8i*>(B + ((size_t)w * 16 + (l & 15)) * 128 + (l >> 4) * 32);
    v4f c = {0.f, 0.f, 0.f, 0.f};
    if (Cin)
        for (int i = 0; i < 4; ++i) c[i] = Cin[((size_t)w * 16 + 4 * (l >> 4) + i) * 16 + (l & 15)];
#if defined(__gfx950__)
    c = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, 0, 0, 0, 0x7F7F7F7F, 0, 0x7F7F7F7F);
#endif
    for (int i = 0; i < 4; ++i) D[((size_t)w * 16 + 4 * (l >> 4) + i) * 16 + (l & 15)] = c[i];
}

static double dec[256];
static void init_dec() {
    for (int v = 0; v < 256; ++v) {
        const int e = (v >> 3) & 15, m = v & 7;
        double x = e == 0 ? m / 8.0 * std::ldexp(1.0, -6) : (1.0 + m / 8.0) * std::ldexp(1.0, e - 7);
        if (e == 15 && m == 7) x = NAN;
        dec[v] = (v & 128) ? -x : x;
    }
}
static unsigned char enc(double x) {   // saturating, round to nearest, ties to the even code
    const double a = std::fmin(std::fabs(x), 448.0);
    int lo = 0;
    while (lo < 0x7E && dec[lo + 1] <= a) ++lo;
    if (lo < 0x7E) {
        const double dl = a - dec[lo], dh = dec[lo + 1] - a;
        if (dh < dl || (dh == dl && (lo & 1))) ++lo;
    }
    return (unsigned char)(lo | (x < 0 ? 128 : 0));
}
static uint64_t rng = 0x9E3779B97F4A7C15ull;
static double uni() {
    rng = rng * 6364136223846793005ull + 1442695040888963407ull;
    return ((rng >> 11) + 0.5) / 9007199254740992.0;
}
static double normal() { return std::sqrt(-2.0 * std::log(uni())) * std::cos(2.0 * M_PI * uni()); }

int main() {
    init_dec();
    const int W = 8192;   // waves = MFMAs per pass: 2 M dot products of depth 128
    std::vector<unsigned char> A((size_t)W * 16 * 128), B(A.size());
    for (auto& v : A) v = enc(normal());
    for (auto& v : B) v = enc(normal() * 448.0 / 3.2);
    const size_t nd = (size_t)W * 256;
    unsigned char *dA, *dB;
    float *dC, *dD;
    if (hipMalloc(&dA, A.size()) || hipMalloc(&dB, B.size()) || hipMalloc(&dC, nd * 4) || hipMalloc(&dD, nd * 4)) return 1;
    if (hipMemcpy(dA, A.data(), A.size(), hipMemcpyHostToDevice) || hipMemcpy(dB, B.data(), B.size(), hipMemcpyHostToDevice)) return 1;
    std::vector<float> D0(nd), D1(nd), Cin(nd);
    probe<<<W, 64>>>(dA, dB, nullptr, dD);
    if (hipMemcpy(D0.data(), dD, nd * 4, hipMemcpyDeviceToHost)) return 1;
    for (int w = 0; w < W; ++w)   // pass 2 starts from the other wave's result: as large as what a GEMM carries, unrelated to this step
        for (int e = 0; e < 256; ++e) Cin[(size_t)w * 256 + e] = D0[(size_t)(w ^ 1) * 256 + e];
    if (hipMemcpy(dC, Cin.data(), nd * 4, hipMemcpyHostToDevice)) return 1;
    probe<<<W, 64>>>(dA, dB, dC, dD);
    if (hipMemcpy(D1.data(), dD, nd * 4, hipMemcpyDeviceToHost)) return 1;
    const double G = std::ldexp(1.0, -24);
    double worst[2] = {0, 0}, worst_t[2] = {0, 0}, sum[2] = {0, 0};
    for (int w = 0; w < W; ++w)
        for (int i = 0; i < 16; ++i)
            for (int j = 0; j < 16; ++j) {
                double s = 0, sa = 0;
                for (int k = 0; k < 128; ++k) {
                    const double p = dec[A[((size_t)w * 16 + i) * 128 + k]] * dec[B[((size_t)w * 16 + j) * 128 + k]];
                    s += p;
                    sa += std::fabs(p);
                }
                for (int pass = 0; pass < 2; ++pass) {
                    const double c = pass ? (double)Cin[(size_t)w * 256 + i * 16 + j] : 0.0;
                    const std::vector<float>& D = pass ? D1 : D0;
                    const double want = c + s, unit = G * (std::fabs(c) + sa);
                    const double e = std::fabs((double)D[(size_t)w * 256 + i * 16 + j] - want) / unit;
                    worst[pass] = std::fmax(worst[pass], e);
                    sum[pass] += e;
                    worst_t[pass] = std::fmax(worst_t[pass], std::fabs((double)D[(size_t)w * 256 + j * 16 + i] - want) / unit);   // the transposed map: must be huge
                }
            }
    for (int pass = 0; pass < 2; ++pass)
        printf("%s: max |d - fp64| = %.3f, mean %.4f, in units of 2^-24 (|c| + sum |a||b|) over %zu outputs "
               "(index map check: %.3g with D transposed)\n",
               pass ? "c = a previous result" : "c = 0", worst[pass], sum[pass] / (double)nd, nd, worst_t[pass]);
    return 0;
}
