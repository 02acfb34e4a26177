// probe_sincos.hip — absolute error of v_sin_f32 / v_cos_f32 (argument in revolutions) on the arguments the QKV + RoPE epilogue
// gives them (gemm_common.h: rev = v_fract(pos * inv_freq[j] / (2 pi)), pos < 4096, j < 32) and on a dense sweep of [0, 1),
// against fp64 sin / cos of 2 pi times the SAME fp32 argument: the instructions alone, not the argument's rounding.
// The bound in tests/gemm_epi_ref.py takes twice the larger figure printed here.
//   hipcc --offload-arch=gfx950 -O2 tools/probe_sincos.hip -o probe_sincos && ./probe_sincos
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <vector>

__global__ void probe(const float* x, float* s, float* c, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        s[i] = __builtin_amdgcn_sinf(x[i]);
        c[i] = __builtin_amdgcn_cosf(x[i]);
    }
}

int main() {
    std::vector<float> x;
    for (int pos = 0; pos < 4096; ++pos)
        for (int j = 0; j < 32; ++j) {
            const float f = (float)((1.0 / std::pow(10000.0, j / 32.0)) / (2.0 * M_PI));
            const float t = (float)pos * f;
            x.push_back(t - std::floor(t));
        }
    const size_t n_rope = x.size();
    for (int i = 0; i < (1 << 20); ++i) x.push_back((float)i / (float)(1 << 20));
    const int n = (int)x.size();
    float *dx, *ds, *dc;
    if (hipMalloc(&dx, n * 4) || hipMalloc(&ds, n * 4) || hipMalloc(&dc, n * 4)) return 1;
    if (hipMemcpy(dx, x.data(), n * 4, hipMemcpyHostToDevice)) return 1;
    probe<<<(n + 255) / 256, 256>>>(dx, ds, dc, n);
    std::vector<float> s(n), c(n);
    if (hipMemcpy(s.data(), ds, n * 4, hipMemcpyDeviceToHost) || hipMemcpy(c.data(), dc, n * 4, hipMemcpyDeviceToHost)) return 1;
    double es[2] = {0, 0}, ec[2] = {0, 0};
    for (int i = 0; i < n; ++i) {
        const double a = 2.0 * M_PI * (double)x[i];
        const int k = (size_t)i >= n_rope;
        es[k] = std::fmax(es[k], std::fabs((double)s[i] - std::sin(a)));
        ec[k] = std::fmax(ec[k], std::fabs((double)c[i] - std::cos(a)));
    }
    printf("rope arguments (4096 x 32): max |v_sin - sin| %.3e  max |v_cos - cos| %.3e\n", es[0], ec[0]);
    printf("dense [0, 1) in steps of 2^-20: max |v_sin - sin| %.3e  max |v_cos - cos| %.3e\n", es[1], ec[1]);
    return 0;
}
