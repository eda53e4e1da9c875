// Frame evaluation on gfx950: the SSIM map / mean and the squared-difference sum (PSNR) of two device-resident frames in ONE pass
// (lib/utils.py:88-134 and run_sr.py:143,1132-1133 of the reference).
//
// Arithmetic.  The reference filters float32 images with a float64 tap table, so every filtered moment is a float64 sum of float32 values, and
// img0**2, img1**2, img0*img1 are float32 products rounded BEFORE they are filtered.  The kernel does the same: (double)(x * x) is a plain fp32
// multiply, every sum is fp64 in tap order n-1..0 (vertical pass first, as the reference's filt_fn; the order of a direct convolution's inner loop), mu*mu is a statement of its own (under
// -ffp-contract=on nothing fuses across statements, so E[x^2] - mu^2 is the reference's two roundings).  An fp32 accumulation is 5e-7 .. 2e-4 away
// from the reference's map and fp64 products 2e-8 .. 2e-7; this form is within 5e-13.
//
// Layout.  Both images are addressed as rows of a vector of 3W elements j = 3 * x + c whose horizontal taps sit 3 apart; an image's own pixel and
// channel strides turn j into an address (channel-last: the row itself; planar: three planes), so the two images may differ in layout.
// A workgroup of 256 threads owns a strip of MT_COLS(n) = 256 - 3 (n - 1) output elements of that vector and a band of MT_ROWS output rows and
// walks down the rows.  Thread t loads element j0 + t of the next input row of both images (clamped in the load where asked), puts it in an LDS ring of the last n
// rows, forms the five vertical sums of its column from the ring (x, y, x*x, y*y, x*y), leaves them in one LDS row, and the first MT_COLS(n) threads
// take the horizontal sums from that row and evaluate the quotient.  No moment image goes to memory; apart from the strip / band halos every input
// element is fetched once; without a map nothing per pixel is written.
//
// Reductions.  A thread adds its map entries (row order) and the squared differences of the input elements its workgroup owns (each element has one
// owner) in fp64; the workgroup adds its threads in a fixed tree and writes two partials; a one-workgroup launch adds the partials in index order.
// No atomics: two calls give the same bits.  Both totals stay on the device.
#include "k4_common.h"

#define MT_THREADS 256
#define MT_ROWS 64
#define MT_MAX_TAPS 31
#define MT_COLS(n) (MT_THREADS - 3 * ((n) - 1))
#define MT_LDS_BYTES(n) ((size_t)5 * MT_THREADS * sizeof(double) + (size_t)2 * (n) * MT_THREADS * sizeof(float))

struct MetricImage { const float* p; int64_t pstride, cstride; int clamp01; };
struct MetricArgs {
    MetricImage a, b;
    int H, W, n, strips;
    double c1, c2;
    double taps[MT_MAX_TAPS];
    double* map;
    double* part;
};

__device__ __forceinline__ float mt_load(const float* p, int clamp01) {
    const float v = *p;
    return clamp01 ? (v < 0.f ? 0.f : (v > 1.f ? 1.f : v)) : v;          // torch.clamp: NaN fails both comparisons and stays
}

__device__ __forceinline__ double mt_block_sum(double s, double* sh) {     // 256 threads, fixed tree
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
    __syncthreads();
    if ((threadIdx.x & 63u) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

__global__ __launch_bounds__(MT_THREADS) void k4_metric_kernel(const MetricArgs A) {
    extern __shared__ double mt_lds[];
    double* const vs = mt_lds;                                              // [5][256] vertical sums of the current output row
    float* const ringx = reinterpret_cast<float*>(mt_lds + 5 * MT_THREADS); // [n][256] the last n rows of image a
    float* const ringy = ringx + A.n * MT_THREADS;                          // [n][256] ... of image b
    __shared__ double sh[4];
    const int t = (int)threadIdx.x, n = A.n;
    const int strip = (int)blockIdx.x % A.strips, band = (int)blockIdx.x / A.strips;
    const int cols = MT_COLS(n);
    const int Ho = A.H - n + 1, Wo3 = 3 * (A.W - n + 1), W3 = 3 * A.W;
    const int j0 = strip * cols, yo0 = band * MT_ROWS, yo1 = min(yo0 + MT_ROWS, Ho);
    const int r0 = yo0, r1 = yo1 + n - 1;                                   // input rows of this band (r1 <= H)
    const int jin = j0 + t;
    const bool in_image = jin < W3;
    // one owner per input element for the squared differences: the strip's own columns (the last strip: to the end of the row), the band's own rows (the last band: to H)
    const bool own_col = in_image && (t < cols || strip == A.strips - 1);
    const int own_r1 = yo1 == Ho ? A.H : yo1;
    const int px = jin / 3, ch = jin - 3 * px;
    const float* pa = A.a.p, * pb = A.b.p;
    int64_t rsa = 0, rsb = 0;
    if (in_image) {
        rsa = (int64_t)A.W * A.a.pstride; rsb = (int64_t)A.W * A.b.pstride;
        pa += (int64_t)ch * A.a.cstride + (int64_t)px * A.a.pstride + (int64_t)r0 * rsa;
        pb += (int64_t)ch * A.b.cstride + (int64_t)px * A.b.pstride + (int64_t)r0 * rsb;
    }
    const int jout = j0 + t;
    const bool out_col = t < cols && jout < Wo3;
    double ssim_acc = 0.0, ssd_acc = 0.0;
    float nx = 0.f, ny = 0.f;
    if (in_image) { nx = mt_load(pa, A.a.clamp01); ny = mt_load(pb, A.b.clamp01); }
    int slot = 0;
    for (int r = r0; r < r1; ++r) {
        const float cx = nx, cy = ny;
        if (in_image && r + 1 < r1) { pa += rsa; pb += rsb; nx = mt_load(pa, A.a.clamp01); ny = mt_load(pb, A.b.clamp01); }
        if (own_col && r < own_r1) {
            const float d = cx - cy;
            const float dd = d * d;                                          // np.square(rgb - gt): an fp32 square
            ssd_acc += (double)dd;
        }
        ringx[slot * MT_THREADS + t] = cx;
        ringy[slot * MT_THREADS + t] = cy;
        __syncthreads();
        if (r - r0 >= n - 1) {                                               // (uniform) the ring holds rows r-n+1 .. r: output row r-n+1
            int s = slot;                                                    // slot of the newest row: taps n-1 .. 0, a direct convolution's order
            double v0 = 0.0, v1 = 0.0, v00 = 0.0, v11 = 0.0, v01 = 0.0;
            for (int k = n - 1; k >= 0; --k) {
                const double f = A.taps[k];
                const float x = ringx[s * MT_THREADS + t], y = ringy[s * MT_THREADS + t];
                const float xx = x * x, yy = y * y, xy = x * y;
                v0 = fma(f, (double)x, v0);
                v1 = fma(f, (double)y, v1);
                v00 = fma(f, (double)xx, v00);
                v11 = fma(f, (double)yy, v11);
                v01 = fma(f, (double)xy, v01);
                s = s == 0 ? n - 1 : s - 1;
            }
            vs[0 * MT_THREADS + t] = v0;
            vs[1 * MT_THREADS + t] = v1;
            vs[2 * MT_THREADS + t] = v00;
            vs[3 * MT_THREADS + t] = v11;
            vs[4 * MT_THREADS + t] = v01;
            __syncthreads();
            if (out_col) {
                double mu0 = 0.0, mu1 = 0.0, e00 = 0.0, e11 = 0.0, e01 = 0.0;
                for (int k = n - 1; k >= 0; --k) {
                    const double f = A.taps[k];
                    const int i = t + 3 * k;                                 // <= cols - 1 + 3 (n - 1) = 255
                    mu0 = fma(f, vs[0 * MT_THREADS + i], mu0);
                    mu1 = fma(f, vs[1 * MT_THREADS + i], mu1);
                    e00 = fma(f, vs[2 * MT_THREADS + i], e00);
                    e11 = fma(f, vs[3 * MT_THREADS + i], e11);
                    e01 = fma(f, vs[4 * MT_THREADS + i], e01);
                }
                const double mu00 = mu0 * mu0;
                const double mu11 = mu1 * mu1;
                const double mu01 = mu0 * mu1;
                double s00 = e00 - mu00;
                double s11 = e11 - mu11;
                double s01 = e01 - mu01;
                // np.maximum(0., s): a NaN stays (fmax(0., NaN) would return 0 and hide it)
                s00 = s00 < 0.0 ? 0.0 : s00;
                s11 = s11 < 0.0 ? 0.0 : s11;
                // np.sign(s01) * np.minimum(np.sqrt(s00 * s11), np.abs(s01)), NaN from either side kept
                const double g = sqrt(s00 * s11), a01 = fabs(s01);
                const double m = g != g ? g : (a01 != a01 ? a01 : (g < a01 ? g : a01));
                const double sg = s01 > 0.0 ? 1.0 : (s01 < 0.0 ? -1.0 : s01);        // sign(+-0) = 0, sign(NaN) = NaN
                s01 = sg * m;
                const double numer = (2.0 * mu01 + A.c1) * (2.0 * s01 + A.c2);
                const double denom = (mu00 + mu11 + A.c1) * (s00 + s11 + A.c2);
                const double q = numer / denom;
                ssim_acc += q;
                if (A.map) A.map[(int64_t)(r - n + 1) * Wo3 + jout] = q;
            }
        }
        slot = slot + 1 == n ? 0 : slot + 1;
    }
    const double s_ssim = mt_block_sum(ssim_acc, sh);
    const double s_ssd = mt_block_sum(ssd_acc, sh);
    if (t == 0) { A.part[2 * (int64_t)blockIdx.x] = s_ssim; A.part[2 * (int64_t)blockIdx.x + 1] = s_ssd; }
}

// sums[0] = the sum of the SSIM map, sums[1] = the sum of squared differences: the partials in index order (a thread takes every 256th, then the fixed tree)
__global__ __launch_bounds__(MT_THREADS) void k4_metric_finish_kernel(const double* __restrict__ part, int nparts, double* __restrict__ sums) {
    __shared__ double sh[4];
    double s0 = 0.0, s1 = 0.0;
    for (int i = (int)threadIdx.x; i < nparts; i += MT_THREADS) { s0 += part[2 * i]; s1 += part[2 * i + 1]; }
    s0 = mt_block_sum(s0, sh);
    s1 = mt_block_sum(s1, sh);
    if (threadIdx.x == 0) { sums[0] = s0; sums[1] = s1; }
}

static int64_t mt_blocks(int64_t H, int64_t W, int64_t n) {
    if (n < 1 || n > MT_MAX_TAPS || H < n || W < n || H * W * 3 >= (1LL << 31) || 3 * W + MT_THREADS >= (1LL << 31)) return -1;
    const int64_t strips = (3 * (W - n + 1) + MT_COLS(n) - 1) / MT_COLS(n), bands = (H - n + 1 + MT_ROWS - 1) / MT_ROWS;
    return strips * bands;
}

extern "C" int64_t k4_frame_metrics_workspace_bytes(int32_t H, int32_t W, int32_t n_taps) {
    const int64_t nb = mt_blocks(H, W, n_taps);
    return nb < 0 ? -1 : nb * 16;
}

extern "C" int k4_frame_metrics(const float* img0, int64_t pixel_stride0, int64_t channel_stride0, int32_t clamp0,
                                const float* img1, int64_t pixel_stride1, int64_t channel_stride1, int32_t clamp1,
                                int32_t H, int32_t W, const double* taps, int32_t n_taps, double c1, double c2,
                                double* ssim_map, void* workspace, double* sums, void* stream) {
    if (!img0 || !img1 || !taps || !workspace || !sums || H <= 0 || W <= 0 || n_taps < 1 || pixel_stride0 < 1 || pixel_stride1 < 1 ||
        channel_stride0 < 1 || channel_stride1 < 1) return K4_ERR_BAD_ARG;
    if (n_taps > MT_MAX_TAPS || H < n_taps || W < n_taps) return K4_ERR_UNSUPPORTED;
    // element and column indices are 32-bit in the kernel: refused, never wrapped (the last strip's threads count up to 255 columns past the row's end)
    if ((int64_t)H * W * 3 >= (1LL << 31) || (int64_t)3 * W + MT_THREADS >= (1LL << 31)) return K4_ERR_UNSUPPORTED;
    if ((((uintptr_t)workspace | (uintptr_t)sums | (uintptr_t)ssim_map) & 7) != 0 || (((uintptr_t)img0 | (uintptr_t)img1) & 3) != 0) return K4_ERR_UNSUPPORTED;
    const int64_t nb = mt_blocks(H, W, n_taps);
    if (nb < 1 || nb > (1 << 24)) return K4_ERR_UNSUPPORTED;
    MetricArgs A;
    A.a = MetricImage{img0, pixel_stride0, channel_stride0, clamp0 != 0};
    A.b = MetricImage{img1, pixel_stride1, channel_stride1, clamp1 != 0};
    A.H = H; A.W = W; A.n = n_taps;
    A.strips = (3 * (W - n_taps + 1) + MT_COLS(n_taps) - 1) / MT_COLS(n_taps);
    A.c1 = c1; A.c2 = c2;
    for (int k = 0; k < MT_MAX_TAPS; ++k) A.taps[k] = k < n_taps ? taps[k] : 0.0;          // by value: the caller's table need not outlive the call
    A.map = ssim_map;
    A.part = reinterpret_cast<double*>(workspace);
    const size_t lds = MT_LDS_BYTES(n_taps);
    return k4_taped(stream, [=](void* stream) -> int {
        // the limit is raised once per device, so to the LARGEST size any later call can ask for (n_taps 28..31 pass 64 KiB), not to this call's
        K4_ENSURE_DYN_LDS(k4_metric_kernel, MT_LDS_BYTES(MT_MAX_TAPS));
        hipLaunchKernelGGL(k4_metric_kernel, dim3((unsigned)nb), dim3(MT_THREADS), lds, (hipStream_t)stream, A);
        const int rc = k4_check_launch();
        if (rc != 0) return rc;                                                            // no finishing launch over partials that were never written
        hipLaunchKernelGGL(k4_metric_finish_kernel, dim3(1), dim3(MT_THREADS), 0, (hipStream_t)stream, A.part, (int)nb, sums);
        return k4_check_launch();
    });
}
