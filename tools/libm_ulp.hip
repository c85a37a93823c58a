// expf / logf of the device math library, element for element, as csrc/lovasz.hip calls them (the library's compile flags):
// tools/libm_ulp.py measures their largest error in units in the last place against float64.
#include <hip/hip_runtime.h>
#include <stdint.h>

__global__ void libm_apply_kernel(const float *__restrict__ x, int64_t n, int which, float *__restrict__ y) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    y[i] = which == 0 ? expf(x[i]) : logf(x[i]);
}

// which: 0 = expf, 1 = logf; returns the hipError_t of the launch
extern "C" int libm_apply(const float *x, int64_t n, int which, float *y, void *stream) {
    if (n <= 0) return 0;
    if (!x || !y || (which != 0 && which != 1)) return -1;
    hipLaunchKernelGGL(libm_apply_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, n, which, y);
    return (int)hipGetLastError();
}
