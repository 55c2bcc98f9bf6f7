// Probe: the device math library's erf and exp as the library's kernels get them (gfx950, -O3, no fast-math), for the constants
// ERF_U / EXP_U of tests/_fantasy_bounds.py.  Evaluates erf at N arguments over [-6.5, 6.5] (7/8 of them on a jittered uniform grid,
// 1/8 log-spaced in magnitude from 1e-300 to 1, alternating sign) and exp at N arguments over [-745, 0] (the same split, the
// log-spaced ones negative), and writes four arrays of N raw doubles -- erf arguments, erf results, exp arguments, exp results -- to
// the file named on the command line.  tools/libm_ulp_read.py compares them with a long-double reference.
// With a third argument "logei": erfc at N arguments over [-29, 1.4143] (the arguments -u / sqrt 2 of LogEI's direct branch, u in [-2, 40];
// the same split, the log-spaced ones of alternating sign) and log at N arguments log-spaced over [1e-20, 100] (LogEI's log arguments),
// for ERFC_U / LOG_U of tests/_logei_bounds.py, in the same file layout (python tools/libm_ulp_read.py FILE logei).
// Build: hipcc --offload-arch=gfx950 -O3 tools/libm_ulp_probe.hip -o tools/libm_ulp_probe
// Run:   tools/libm_ulp_probe /tmp/libm_ulp.bin && python tools/libm_ulp_read.py /tmp/libm_ulp.bin
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#define CK(x) do{hipError_t e=(x); if(e!=hipSuccess){printf("HIP error %s line %d\n", hipGetErrorString(e), __LINE__); exit(1);} }while(0)

__global__ __launch_bounds__(256) void probe(const double* __restrict__ xe, double* __restrict__ ye, const double* __restrict__ xx,
                                             double* __restrict__ yx, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  ye[i] = erf(xe[i]);
  yx[i] = exp(xx[i]);
}

__global__ __launch_bounds__(256) void probe_logei(const double* __restrict__ xe, double* __restrict__ ye, const double* __restrict__ xx,
                                                   double* __restrict__ yx, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  ye[i] = erfc(xe[i]);
  yx[i] = log(xx[i]);
}

int main(int argc, char** argv) {
  if (argc < 2) { printf("usage: %s OUTPUT [N] [logei]\n", argv[0]); return 2; }
  const bool logei = argc > 3 && argv[3][0] == 'l';
  const int n = argc > 2 ? atoi(argv[2]) : 1 << 20;
  if (n < 8) { printf("N must be at least 8\n"); return 2; }
  std::vector<double> xe(n), xx(n), ye(n), yx(n);
  const int nu = n - n / 8;
  for (int i = 0; i < n; ++i) {
    if (i < nu) {
      const double t = (i + fmod(i * 0.6180339887498949, 1.0)) / nu;   // (jitter: no argument on a round binary fraction)
      xe[i] = -6.5 + 13.0 * t;
      xx[i] = -745.0 * t;
    } else {
      const double mag = pow(10.0, -300.0 * (double)(i - nu) / (n - nu));
      xe[i] = (i & 1) ? -mag : mag;
      xx[i] = -mag;
    }
    if (logei) {
      xe[i] = i < nu ? -29.0 + 30.4143 * (xe[i] + 6.5) / 13.0 : xe[i];
      xx[i] = pow(10.0, -20.0 + 22.0 * (i + 0.5) / n);
    }
  }
  double *dxe, *dye, *dxx, *dyx;
  const size_t bytes = (size_t)n * sizeof(double);
  CK(hipMalloc(&dxe, bytes)); CK(hipMalloc(&dye, bytes)); CK(hipMalloc(&dxx, bytes)); CK(hipMalloc(&dyx, bytes));
  CK(hipMemcpy(dxe, xe.data(), bytes, hipMemcpyHostToDevice));
  CK(hipMemcpy(dxx, xx.data(), bytes, hipMemcpyHostToDevice));
  if (logei) hipLaunchKernelGGL(probe_logei, dim3((n + 255) / 256), dim3(256), 0, 0, dxe, dye, dxx, dyx, n);
  else hipLaunchKernelGGL(probe, dim3((n + 255) / 256), dim3(256), 0, 0, dxe, dye, dxx, dyx, n);
  CK(hipGetLastError());
  CK(hipDeviceSynchronize());
  CK(hipMemcpy(ye.data(), dye, bytes, hipMemcpyDeviceToHost));
  CK(hipMemcpy(yx.data(), dyx, bytes, hipMemcpyDeviceToHost));
  CK(hipFree(dxe)); CK(hipFree(dye)); CK(hipFree(dxx)); CK(hipFree(dyx));
  FILE* f = fopen(argv[1], "wb");
  if (!f) { printf("cannot open %s\n", argv[1]); return 1; }
  const std::vector<double>* parts[4] = {&xe, &ye, &xx, &yx};
  for (const auto* p : parts)
    if (fwrite(p->data(), sizeof(double), n, f) != (size_t)n) { printf("short write\n"); return 1; }
  fclose(f);
  if (logei) printf("%d arguments each: erfc over [-29, 1.4143], log over [1e-20, 100] -> %s\n", n, argv[1]);
  else printf("%d arguments each: erf over [-6.5, 6.5], exp over [-745, 0] -> %s\n", n, argv[1]);
  return 0;
}
