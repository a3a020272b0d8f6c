// sincos_ulp -- the error of the device's sincosf against float64 over 2^20 phases in [-8, 8) (the pilot phase the modulation meter takes lies in
// [0, 2 pi + 0.7)): the largest error in ulp of the true value, and the largest absolute error in units of 2^-24.  DESIGN.md 4.11 quotes the result;
// tests/meter_model.py's SINCOS_ULP is it, rounded up.
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -o sincos_ulp sincos_ulp.hip && ./sincos_ulp
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <vector>

__global__ void k(const float *x, float *s, float *c, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) sincosf(x[i], &s[i], &c[i]);
}

int main() {
    const int n = 1 << 20;
    std::vector<float> x(n), s(n), c(n);
    for (int i = 0; i < n; i++) x[i] = (float)(-8.0 + 16.0 * ((double)i + 0.37) / n);
    float *dx, *ds, *dc;
    if (hipMalloc(&dx, 4 * n) != hipSuccess || hipMalloc(&ds, 4 * n) != hipSuccess || hipMalloc(&dc, 4 * n) != hipSuccess) { printf("no device\n"); return 1; }
    hipMemcpy(dx, x.data(), 4 * n, hipMemcpyHostToDevice);
    hipLaunchKernelGGL(k, dim3(n / 256), dim3(256), 0, 0, dx, ds, dc, n);
    if (hipMemcpy(s.data(), ds, 4 * n, hipMemcpyDeviceToHost) != hipSuccess) { printf("kernel failed\n"); return 1; }
    hipMemcpy(c.data(), dc, 4 * n, hipMemcpyDeviceToHost);
    double worst_ulp = 0, worst_abs = 0;
    for (int i = 0; i < n; i++) {
        const double t[2] = {std::sin((double)x[i]), std::cos((double)x[i])}, g[2] = {(double)s[i], (double)c[i]};
        for (int q = 0; q < 2; q++) {
            int e; std::frexp(t[q], &e);
            const double ulp = std::ldexp(1.0, e - 24), err = std::fabs(g[q] - t[q]);
            if (err / ulp > worst_ulp) worst_ulp = err / ulp;
            if (err / std::ldexp(1.0, -24) > worst_abs) worst_abs = err / std::ldexp(1.0, -24);
        }
    }
    printf("sincosf over %d phases in [-8, 8): worst error %.3f ulp of the true value, %.3f x 2^-24 absolute\n", n, worst_ulp, worst_abs);
    hipFree(dx); hipFree(ds); hipFree(dc);
    return 0;
}
