// cosf and sinf of the device over a list of float32 arguments: the measured constant of the timestep-embedding bound
// (tests/unet_check.py, Y_SINCOS).
//   hipcc -O3 --offload-arch=gfx950 tools/sincos_probe.hip -o sincos_probe ; ./sincos_probe in.f32 out.f32
// in.f32: n raw little-endian floats; out.f32: 2 n floats, cosf of each and then sinf of each, as the library's kernels compute
// them (same compiler, same flags, no fast-math).  tools/unet_rate.py --sincos-probe compares them with float64 cos / sin.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <vector>

__global__ void sincos_kernel(const float* in, float* out, long n) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        out[i] = cosf(in[i]);
        out[n + i] = sinf(in[i]);
    }
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
    CHECK(hipMalloc(&dout, 2 * n * sizeof(float)));
    CHECK(hipMemcpy(din, h.data(), n * sizeof(float), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(sincos_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, din, dout, n);
    CHECK(hipGetLastError());
    h.resize((size_t)(2 * n));
    CHECK(hipMemcpy(h.data(), dout, 2 * n * sizeof(float), hipMemcpyDeviceToHost));
    f = std::fopen(argv[2], "wb");
    if (!f || std::fwrite(h.data(), sizeof(float), (size_t)(2 * n), f) != (size_t)(2 * n)) return 1;
    std::fclose(f);
    std::printf("cosf and sinf of %ld values\n", n);
    return 0;
}
