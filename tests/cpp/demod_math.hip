// demod_math.hip — the two operations csrc/demod.hip takes from the compiler as correctly rounded: `/` and sqrtf, built
// with demod.o's flags.
//
//   demod_math IN OUT    IN: n pairs as float x[n] then float y[n];  OUT: float q[n] = x / y, then
//                        float r[n] = sqrtf(fabsf(x)), as the device computed them.
// The test compares OUT with NumPy's float32 division and root, bit for bit (tests/test_gpu_demod.py).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>

#include <vector>

#pragma clang fp contract(off)

__global__ void div_sqrt(const float *x, const float *y, int n, float *q, float *r) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    q[i] = x[i] / y[i];
    r[i] = sqrtf(fabsf(x[i]));
}

#define CK(x)                                                              \
    do {                                                                   \
        if ((x) != hipSuccess) {                                           \
            printf("hip error at %s:%d\n", __FILE__, __LINE__);           \
            return 2;                                                      \
        }                                                                  \
    } while (0)

int main(int argc, char **argv) {
    if (argc != 3) return 3;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 3;
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    if (bytes <= 0 || bytes % 8 != 0 || bytes > (1L << 28)) return 3;
    const int n = (int)(bytes / 8);
    std::vector<float> h(2 * (size_t)n);
    if (fread(h.data(), 4, h.size(), f) != h.size()) return 3;
    fclose(f);
    float *in, *out;
    CK(hipMalloc(&in, (size_t)bytes));
    CK(hipMalloc(&out, (size_t)bytes));
    CK(hipMemcpy(in, h.data(), (size_t)bytes, hipMemcpyHostToDevice));
    div_sqrt<<<(n + 255) / 256, 256>>>(in, in + n, n, out, out + n);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(h.data(), out, (size_t)bytes, hipMemcpyDeviceToHost));
    f = fopen(argv[2], "wb");
    if (!f || fwrite(h.data(), 4, h.size(), f) != h.size()) return 3;
    fclose(f);
    printf("pairs %d\n", n);
    return 0;
}
