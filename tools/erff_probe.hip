// erff of the device over a list of float32 arguments: the measured constant of the GEGLU bound (tests/transformer_check.py, Y_ERF).
//   hipcc -O3 --offload-arch=gfx950 tools/erff_probe.hip -o erff_probe ; ./erff_probe in.f32 out.f32
// in.f32: raw little-endian floats; out.f32: erff of each, as the library's kernels compute it (same compiler, same flags, no
// fast-math).  tools/spatial_transformer_rate.py --erff-probe compares them with float64 erf.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <vector>

__global__ void erff_kernel(const float* in, float* out, long n) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = erff(in[i]);
}

#define CHECK(e)                                                                  \
    do {                                                                          \
        hipError_t err_ = (e);                                                    \
        if (err_ != hipSuccess) {                                                 \
            std::fprintf(stderr, "%s: %s\n", #e, hipGetErrorString(err_));       \
            return 2;                                                             \
        }                                                                         \
    } while (0)

int main(int argc, char** argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: %s in.f32 out.f32\n", argv[0]);
        return 1;
    }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 1;
    std::fseek(f, 0, SEEK_END);
    const long n = std::ftell(f) / (long)sizeof(float);
    std::fseek(f, 0, SEEK_SET);
    std::vector<float> h((size_t)n);
    if (n <= 0 || std::fread(h.data(), sizeof(float), (size_t)n, f) != (size_t)n) return 1;
    std::fclose(f);
    float *din = nullptr, *dout = nullptr;
    CHECK(hipMalloc(&din, n * sizeof(float)));
    CHECK(hipMalloc(&dout, n * sizeof(float)));
    CHECK(hipMemcpy(din, h.data(), n * sizeof(float), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(erff_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, din, dout, n);
    CHECK(hipGetLastError());
    CHECK(hipMemcpy(h.data(), dout, n * sizeof(float), hipMemcpyDeviceToHost));
    f = std::fopen(argv[2], "wb");
    if (!f || std::fwrite(h.data(), sizeof(float), (size_t)n, f) != (size_t)n) return 1;
    std::fclose(f);
    std::printf("erff of %ld values\n", n);
    return 0;
}
