// The head of LPIPS-VGG (lib/utils.py:137-149 of the reference scores frames with lpips.LPIPS(net='vgg', version='0.1'); the formulas as lib/lpips.py restates
// them from the published lpips 0.1 source).  The backbone is the VGG stack of k4_vgg.hip on a batch of two; this file holds what follows a tapped level:
//
//   k4_lpips_head      one tap.  f [2][n_pix][C] are the two images' post-ReLU features, w [C] the tap's 1x1 weights.  Per pixel
//                          n_i = f_i / (sqrt(sum_c f_i[c]^2) + 1e-10)                  (normalize_tensor)
//                          v   = sum_c w[c] (n_0[c] - n_1[c])^2                        (the difference squared, then NetLinLayer's 1x1 convolution)
//                      and the tap's value is the mean of v over the pixels (spatial_average).  Elementwise arithmetic in fp32 as the package has it; the three
//                      sums (squares over channels, weighted differences over channels, pixels) are fp64 partials in one fixed order: a wave owns a pixel and
//                      adds its lanes' terms on a fixed butterfly, a workgroup adds its 64 pixels in (wave, turn) order into `workspace`, and a finishing
//                      launch adds the workgroups' partials in index order and writes taps[slot] = sum / n_pix in fp64.
//   k4_lpips_total     out[0] = fp32(sum_k taps[k]) added in fp64 in tap order, out[1 + k] = fp32(taps[k]): each value is rounded once.
//   k4_lpips_check_frame  the shape guard of the whole metric.
// No atomics, no host synchronisation: two calls give identical bits, and swapping the two images does too ((a - b)^2 == (b - a)^2 in fp32).
#include "k4_common.h"

#define K4_LPIPS_SPAN 64                 // pixels per workgroup: 4 waves x 16 turns
#define K4_LPIPS_EPS 1e-10f

__device__ __forceinline__ double lp_wave_sum(double s) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
    return s;
}

// NC = C / 64 channels per lane: lane l holds channels l + 64 * j (a wave's load of one j is one 256-byte line)
template <int NC>
__global__ __launch_bounds__(256) void k4_lpips_head_kernel(const float* __restrict__ f, int64_t n_pix, const float* __restrict__ w, double* __restrict__ part) {
    constexpr int C = NC * 64;
    __shared__ double sh[4];
    const int lane = k4_lane(), wv = (int)(threadIdx.x >> 6);
    const float* const f0 = f;
    const float* const f1 = f + (size_t)n_pix * C;
    float wl[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) wl[j] = w[lane + 64 * j];
    const int64_t base = (int64_t)blockIdx.x * K4_LPIPS_SPAN;
    double acc = 0.0;
    for (int turn = 0; turn < K4_LPIPS_SPAN / 4; ++turn) {
        const int64_t p = base + turn * 4 + wv;                      // wave-uniform
        if (p >= n_pix) break;
        float a[NC], b[NC];
        double sa = 0.0, sb = 0.0;
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            a[j] = f0[(size_t)p * C + lane + 64 * j];
            b[j] = f1[(size_t)p * C + lane + 64 * j];
            sa += (double)(a[j] * a[j]);
            sb += (double)(b[j] * b[j]);
        }
        sa = lp_wave_sum(sa); sb = lp_wave_sum(sb);
        const float da = sqrtf((float)sa) + K4_LPIPS_EPS, db = sqrtf((float)sb) + K4_LPIPS_EPS;
        double v = 0.0;
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            const float d = a[j] / da - b[j] / db;
            v += (double)(wl[j] * (d * d));
        }
        acc += lp_wave_sum(v);
    }
    if (lane == 0) sh[wv] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

__global__ __launch_bounds__(256) void k4_lpips_finish_kernel(const double* __restrict__ part, int nparts, int64_t n_pix, double* __restrict__ out) {
    __shared__ double sh[4];
    double s = 0.0;
    for (int i = (int)threadIdx.x; i < nparts; i += 256) s += part[i];
    s = lp_wave_sum(s);
    if ((threadIdx.x & 63u) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) out[0] = ((sh[0] + sh[1]) + (sh[2] + sh[3])) / (double)n_pix;
}

__global__ void k4_lpips_total_kernel(const double* __restrict__ taps, int n, float* __restrict__ out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double s = 0.0;
    for (int k = 0; k < n; ++k) { s += taps[k]; out[1 + k] = (float)taps[k]; }
    out[0] = (float)s;
}

extern "C" int64_t k4_lpips_workspace_bytes(int64_t n_pix) {
    if (n_pix <= 0 || n_pix > (1LL << 26)) return -1;
    return (n_pix + K4_LPIPS_SPAN - 1) / K4_LPIPS_SPAN * 8;
}

extern "C" int k4_lpips_head(const float* f, int64_t n_pix, int32_t channels, const float* w, void* workspace, double* taps, int32_t slot, void* stream) {
    if (!f || !w || !workspace || !taps || n_pix <= 0 || channels <= 0 || slot < 0) return K4_ERR_BAD_ARG;
    if (channels != 64 && channels != 128 && channels != 256 && channels != 512) return K4_ERR_UNSUPPORTED;
    if (n_pix > (1LL << 26) || (((uintptr_t)workspace | (uintptr_t)taps) & 7) != 0) return K4_ERR_UNSUPPORTED;
    const int nparts = (int)((n_pix + K4_LPIPS_SPAN - 1) / K4_LPIPS_SPAN);
    double* const part = reinterpret_cast<double*>(workspace);
    return k4_taped(stream, [=](void* stream) -> int {
        const hipStream_t st = (hipStream_t)stream;
        const dim3 grid((unsigned)nparts), block(256);
        switch (channels) {
            case 64: hipLaunchKernelGGL(k4_lpips_head_kernel<1>, grid, block, 0, st, f, n_pix, w, part); break;
            case 128: hipLaunchKernelGGL(k4_lpips_head_kernel<2>, grid, block, 0, st, f, n_pix, w, part); break;
            case 256: hipLaunchKernelGGL(k4_lpips_head_kernel<4>, grid, block, 0, st, f, n_pix, w, part); break;
            default: hipLaunchKernelGGL(k4_lpips_head_kernel<8>, grid, block, 0, st, f, n_pix, w, part); break;
        }
        hipLaunchKernelGGL(k4_lpips_finish_kernel, dim3(1), dim3(256), 0, st, (const double*)part, nparts, n_pix, taps + slot);
        return k4_check_launch();
    });
}

extern "C" int k4_lpips_total(const double* taps, int32_t n_taps, float* out, void* stream) {
    if (!taps || !out || n_taps <= 0) return K4_ERR_BAD_ARG;
    if (n_taps > 16 || ((uintptr_t)taps & 7) != 0) return K4_ERR_UNSUPPORTED;
    return k4_taped(stream, [=](void* stream) -> int {
        hipLaunchKernelGGL(k4_lpips_total_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, taps, (int)n_taps, out);
        return k4_check_launch();
    });
}

// Four floor-mode 2x2 pools lie between the frame and the last tap: below 16 a pooled level would be empty; above 2^26 pixels over the batch of two the
// 3x3 layers refuse.
extern "C" int k4_lpips_check_frame(int32_t H, int32_t W) {
    if (H <= 0 || W <= 0) return K4_ERR_BAD_ARG;
    if (H < 16 || W < 16 || (int64_t)H * W * 2 > (1 << 26)) return K4_ERR_UNSUPPORTED;
    return 0;
}
