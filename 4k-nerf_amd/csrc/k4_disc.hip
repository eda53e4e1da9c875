// The U-Net discriminator of the "+gan" joint recipes on gfx950 (lib/sr_unetdisc.py:7-62 upstream; run_sr.py:916-957, 1016-1049).
//
//   k4_disc_conv_s2        4x4 stride-2 pad-1 convolution, NHWC, and its input gradient (a stride-2 transposed convolution = four
//                          phases of 2x2 taps); the same kernel also runs a 3x3 stride-1 input gradient of any width (conv4 at
//                          num_feat=64 has 512 outputs, beyond k4_conv_weight_bf16x6_bytes).  Implicit GEMM on
//                          v_mfma_f32_32x32x16_bf16 with the exact 3-term bf16 split of both operands (6 partial products, fp32
//                          accumulation: the arithmetic of k4_conv2d_nhwc_bf16x6).  A workgroup owns a tile of 32*MT output pixels x
//                          32*NT output channels; its four (or eight) WAVES SPLIT THE REDUCTION (tap, 16-channel chunk) round-robin and are summed
//                          through LDS in wave order -- the deep layers are small images with long reductions (32x32 pixels, K = 4096):
//                          a pixel-only decomposition would leave most of the chip idle.  The activation fragment (8 channels of one
//                          pixel per lane) is fetched as two 16-byte loads and split in registers; the weight fragments come pre-split
//                          in the layout of k4_conv2d_nhwc_bf16x6's operand ([chunk][term][tap][2][NOUT][8] bf16, taps = 16 or 9).
//   k4_disc_wgrad_s2       dW[co][ci][dy][dx] = sum_p dY[p][co] X[2p - 1 + (dy, dx)][ci]: the pixel GEMM of k4_sr_bwd.hip for the strided
//                          taps, 64 x 64 tiles per wave where the layer has them, split-K over bands of output rows into a partial
//                          buffer that a second launch sums IN BAND ORDER (no float atomics: the result does not depend on the run).
//   k4_bilinear2x_*        F.interpolate(scale_factor=2, mode='bilinear', align_corners=False) forward (of a + b when a skip tensor is
//                          given) and backward.
//   k4_sn_prepare          torch.nn.utils.spectral_norm's weight: one power iteration (training), sigma, and weight_orig / sigma written
//                          directly as the two packed operands (forward form, input-gradient form) the convolutions read.
//   k4_sn_project_grad     the backward of that division with u, v constant.
//   k4_gan_loss_fwd / bwd  mean(softplus(-+x)) on logits (BCEWithLogitsLoss against all-ones / all-zeros).
// Every reduction here runs in a fixed order.
#include "k4_common.h"

typedef float dc_f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 dc_bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 dc_bf16x2 __attribute__((ext_vector_type(2)));
typedef float dc_f32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ unsigned dc_pk_bf16(float lo, float hi) {               // v_cvt_pk_bf16_f32 (RNE)
    const dc_f32x2 v = {lo, hi};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, dc_bf16x2));
}
// x == t0 + t1 + t2 exactly (bf16 terms, RNE of the successive remainders)
__device__ __forceinline__ void dc_split3(const float (&v)[8], uint4& t0, uint4& t1, uint4& t2) {
    unsigned p0[4], p1[4], p2[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float a = v[2 * i], b = v[2 * i + 1];
        p0[i] = dc_pk_bf16(a, b);
        const float ra = a - __uint_as_float(p0[i] << 16), rb = b - __uint_as_float(p0[i] & 0xffff0000u);
        p1[i] = dc_pk_bf16(ra, rb);
        const float sa = ra - __uint_as_float(p1[i] << 16), sb = rb - __uint_as_float(p1[i] & 0xffff0000u);
        p2[i] = dc_pk_bf16(sa, sb);
    }
    t0 = make_uint4(p0[0], p0[1], p0[2], p0[3]); t1 = make_uint4(p1[0], p1[1], p1[2], p1[3]); t2 = make_uint4(p2[0], p2[1], p2[2], p2[3]);
}
#define DC_MFMA(ACC, A, B) ACC = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(dc_bf16x8, A), __builtin_bit_cast(dc_bf16x8, B), ACC, 0, 0, 0)
// the six products of the 3-term splits that are not below 2^-23 of the full product, smallest first
#define DC_MFMA6(ACC, A0, A1, A2, B0, B1, B2) do { DC_MFMA(ACC, A2, B0); DC_MFMA(ACC, A0, B2); DC_MFMA(ACC, A1, B1); \
                                                   DC_MFMA(ACC, A1, B0); DC_MFMA(ACC, A0, B1); DC_MFMA(ACC, A0, B0); } while (0)

// ---------------------------------------------------------------------------------------------------------------------------------
// convolution / input gradient
// ---------------------------------------------------------------------------------------------------------------------------------
struct DiscConv {
    const float* x; int cin, x_stride, Hin, Win;         // the tensor that is gathered from
    const uint4* w; int NOUT, taps;                      // packed operand: [ceil(cin/16)][3][taps][2][NOUT][8] bf16
    float* y; int cout, y_stride, Hy, Wy;                // the tensor that is written (all of it, each element once)
    int Ho, Wo;                                          // output positions per phase
    int mode;                                            // K4_DISC_CONV_*
    int lrelu; float slope;
};

template <int MT, int NT, int KS>
__global__ __launch_bounds__(64 * KS) void k4_disc_conv_kernel(const DiscConv P) {
    __shared__ float red[KS - 1][MT * NT * 16 * 64];
    const int lane = k4_lane(), wv = (int)(threadIdx.x >> 6), half = lane >> 5, l31 = lane & 31;
    // in = o * S + O + j * DJ, weight tap = T0 + j * TS (per axis), j < nj; out = o * OM + OO
    int S, Oy, Ox, DJ, T0y, T0x, TS, nj, KW, OM, OOy, OOx;
    if (P.mode == K4_DISC_CONV_FWD) { S = 2; Oy = Ox = -1; DJ = 1; T0y = T0x = 0; TS = 1; nj = 4; KW = 4; OM = 1; OOy = OOx = 0; }
    else if (P.mode == K4_DISC_CONV_DGRAD) {
        const int py = (int)blockIdx.z >> 1, px = (int)blockIdx.z & 1;            // input row 2a + py gets dY rows a + py - j through taps dy = 1 - py + 2j
        S = 1; Oy = py; Ox = px; DJ = -1; T0y = 1 - py; T0x = 1 - px; TS = 2; nj = 2; KW = 4; OM = 2; OOy = py; OOx = px;
    } else { S = 1; Oy = Ox = 1; DJ = -1; T0y = T0x = 0; TS = 1; nj = 3; KW = 3; OM = 1; OOy = OOx = 0; }      // K4_DISC_CONV_DGRAD3: dX[p] = sum dY[p + 1 - d] W[.][.][d]
    const int npix = P.Ho * P.Wo;
    const int pix0 = (int)blockIdx.x * 32 * MT;
    const int nb0 = (int)blockIdx.y * NT;
    int oy[MT], ox[MT];
    bool pok[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        const int p = pix0 + m * 32 + l31;
        pok[m] = p < npix;
        oy[m] = p / P.Wo; ox[m] = p - oy[m] * P.Wo;
    }
    dc_f32x16 acc[MT][NT];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int n = 0; n < NT; ++n) acc[m][n] = (dc_f32x16)(0.f);
    const int nch = (P.cin + 15) >> 4;
    const int steps = nj * nj * nch;
    const size_t plane = (size_t)P.taps * 2 * P.NOUT;                             // 16-byte units per (chunk, term)
    // one step = (tap, 16-channel chunk); the fetches of step s + KS are issued in front of the matrix instructions of step s
    float4 xa[MT][2];
    uint4 wb[NT][3];
    auto fetch = [&](int s) {
        const int ch = s % nch, t = s / nch;
        const int j = t / nj, i = t - j * nj;
        const int tap = (T0y + j * TS) * KW + (T0x + i * TS);
        const int c0 = ch * 16 + half * 8;
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            const int iy = oy[m] * S + Oy + j * DJ, ix = ox[m] * S + Ox + i * DJ;
            if (pok[m] && iy >= 0 && iy < P.Hin && ix >= 0 && ix < P.Win && c0 < P.cin) {                 // (cin % 8 == 0: checked by the entry point)
                const float4* q = reinterpret_cast<const float4*>(P.x + ((size_t)iy * P.Win + ix) * P.x_stride + c0);
                xa[m][0] = q[0]; xa[m][1] = q[1];
            } else {
                xa[m][0] = make_float4(0.f, 0.f, 0.f, 0.f); xa[m][1] = make_float4(0.f, 0.f, 0.f, 0.f);     // (two statements: the chained form crashed this ROCm's Machine Copy Propagation pass)
            }
        }
        const uint4* wp = P.w + ((size_t)ch * 3) * plane + ((size_t)tap * 2 + half) * P.NOUT + (size_t)nb0 * 32 + l31;
#pragma unroll
        for (int n = 0; n < NT; ++n) { wb[n][0] = wp[n * 32]; wb[n][1] = wp[plane + n * 32]; wb[n][2] = wp[2 * plane + n * 32]; }
    };
    if (wv < steps) fetch(wv);
    for (int s = wv; s < steps; s += KS) {
        uint4 a[MT][3], b[NT][3];
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            const float v[8] = {xa[m][0].x, xa[m][0].y, xa[m][0].z, xa[m][0].w, xa[m][1].x, xa[m][1].y, xa[m][1].z, xa[m][1].w};
            dc_split3(v, a[m][0], a[m][1], a[m][2]);
        }
#pragma unroll
        for (int n = 0; n < NT; ++n) { b[n][0] = wb[n][0]; b[n][1] = wb[n][1]; b[n][2] = wb[n][2]; }
        if (s + KS < steps) fetch(s + KS);
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int m = 0; m < MT; ++m) DC_MFMA6(acc[m][n], a[m][0], a[m][1], a[m][2], b[n][0], b[n][1], b[n][2]);
    }
    // the waves' partial tiles, summed in wave order
    if (wv > 0) {
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int n = 0; n < NT; ++n)
#pragma unroll
                for (int r = 0; r < 16; ++r) red[wv - 1][((m * NT + n) * 16 + r) * 64 + lane] = acc[m][n][r];
    }
    __syncthreads();
    if (wv != 0) return;
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int n = 0; n < NT; ++n) {
            const int co = (nb0 + n) * 32 + l31;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int q = ((m * NT + n) * 16 + r) * 64 + lane;
                float v = acc[m][n][r];
#pragma unroll
                for (int k = 0; k < KS - 1; ++k) v += red[k][q];
                if (P.lrelu) v = v > 0.f ? v : v * P.slope;
                const int p = pix0 + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;           // accumulator register r of lane l = D[pixel][channel l31]
                if (p < npix && co < P.cout) {
                    const int py = p / P.Wo, px = p - py * P.Wo;
                    P.y[((size_t)(py * OM + OOy) * P.Wy + (px * OM + OOx)) * P.y_stride + co] = v;
                }
            }
        }
}

extern "C" int64_t k4_disc_weight_bytes(int32_t cout, int32_t cin, int32_t ksize) {
    if (cout <= 0 || cin <= 0 || (ksize != 3 && ksize != 4)) return -1;
    return (int64_t)((cin + 15) / 16) * 3 * ksize * ksize * 2 * ((cout + 31) / 32 * 32) * 16;
}

extern "C" int k4_disc_conv_s2(const float* x, int32_t cin, int32_t x_stride, int32_t Hin, int32_t Win, const void* w_split,
                               float* y, int32_t cout, int32_t y_stride, int32_t mode, int32_t lrelu, float slope, void* stream) {
    if (!x || !w_split || !y || cin <= 0 || cout <= 0 || Hin <= 0 || Win <= 0 || x_stride < cin || y_stride < cout) return K4_ERR_BAD_ARG;
    if (mode != K4_DISC_CONV_FWD && mode != K4_DISC_CONV_DGRAD && mode != K4_DISC_CONV_DGRAD3) return K4_ERR_BAD_ARG;
    if (cin % 8 != 0 || x_stride % 4 != 0 || ((uintptr_t)x & 15) != 0) return K4_ERR_UNSUPPORTED;               // 16-byte activation loads
    if (mode == K4_DISC_CONV_FWD && ((Hin & 1) || (Win & 1))) return K4_ERR_UNSUPPORTED;
    if ((int64_t)Hin * Win > (1 << 28)) return K4_ERR_UNSUPPORTED;
    DiscConv P{};
    P.x = x; P.cin = cin; P.x_stride = x_stride; P.Hin = Hin; P.Win = Win;
    P.w = reinterpret_cast<const uint4*>(w_split); P.NOUT = (cout + 31) / 32 * 32; P.taps = mode == K4_DISC_CONV_DGRAD3 ? 9 : 16;
    P.y = y; P.cout = cout; P.y_stride = y_stride;
    if (mode == K4_DISC_CONV_FWD) { P.Ho = P.Hy = Hin / 2; P.Wo = P.Wy = Win / 2; }
    else if (mode == K4_DISC_CONV_DGRAD) { P.Ho = Hin; P.Wo = Win; P.Hy = 2 * Hin; P.Wy = 2 * Win; }             // x is dY [Hin][Win]; per phase one output per dY position
    else { P.Ho = P.Hy = Hin; P.Wo = P.Wy = Win; }
    P.mode = mode; P.lrelu = lrelu; P.slope = slope;
    const int nblk = P.NOUT / 32, npix = P.Ho * P.Wo, phases = mode == K4_DISC_CONV_DGRAD ? 4 : 1;
    return k4_taped(stream, [=](void* stream) -> int {
        // tile: the largest of (64 x 64), (32 x 64), (32 x 32) [pixels x channels] that still gives the chip a workgroup per CU; the smaller tiles split the
        // reduction over eight waves instead of four while the grid leaves SIMDs with fewer than two waves
        const int ncu = k4_num_cus();
        const bool n2 = nblk % 2 == 0;
        const int64_t wg22 = (int64_t)((npix + 63) / 64) * (nblk / 2) * phases;
        const int64_t wg12 = (int64_t)((npix + 31) / 32) * (nblk / 2) * phases, wg11 = (int64_t)((npix + 31) / 32) * nblk * phases;
        const hipStream_t st = (hipStream_t)stream;
        if (n2 && wg22 >= ncu) hipLaunchKernelGGL((k4_disc_conv_kernel<2, 2, 4>), dim3((unsigned)((npix + 63) / 64), (unsigned)(nblk / 2), (unsigned)phases), dim3(256), 0, st, P);
        else if (n2 && wg12 >= 2 * ncu) hipLaunchKernelGGL((k4_disc_conv_kernel<1, 2, 4>), dim3((unsigned)((npix + 31) / 32), (unsigned)(nblk / 2), (unsigned)phases), dim3(256), 0, st, P);
        else if (n2) hipLaunchKernelGGL((k4_disc_conv_kernel<1, 2, 8>), dim3((unsigned)((npix + 31) / 32), (unsigned)(nblk / 2), (unsigned)phases), dim3(512), 0, st, P);
        else if (wg11 >= 2 * ncu) hipLaunchKernelGGL((k4_disc_conv_kernel<1, 1, 4>), dim3((unsigned)((npix + 31) / 32), (unsigned)nblk, (unsigned)phases), dim3(256), 0, st, P);
        else hipLaunchKernelGGL((k4_disc_conv_kernel<1, 1, 8>), dim3((unsigned)((npix + 31) / 32), (unsigned)nblk, (unsigned)phases), dim3(512), 0, st, P);
        return k4_check_launch();
    });
}

// ---------------------------------------------------------------------------------------------------------------------------------
// weight gradient of the 4x4 stride-2 layer
// ---------------------------------------------------------------------------------------------------------------------------------
struct DiscWgrad {
    const float* x; int cin, x_stride, H, W;             // the layer's input [H][W][x_stride]
    const float* gy; int cout, gy_stride;                // dY [H/2][W/2][gy_stride]
    float* part;                                         // [bands][cout][cin][16]
    int ci_tiles, co_tiles, bands, rows;                 // rows of dY per band
};

template <int MI, int MJ>
__global__ __launch_bounds__(256) void k4_disc_wgrad_kernel(const DiscWgrad P) {
    __shared__ float red[3][MI * MJ * 16 * 64];
    const int lane = k4_lane(), wv = (int)(threadIdx.x >> 6), half = lane >> 5, l31 = lane & 31;
    int b = (int)blockIdx.x;
    const int band = b % P.bands; b /= P.bands;
    const int cot = b % P.co_tiles; b /= P.co_tiles;
    const int cit = b % P.ci_tiles; b /= P.ci_tiles;
    const int tap = b, dy = tap >> 2, dx = tap & 3;
    const int Ho = P.H >> 1, Wo = P.W >> 1;
    dc_f32x16 acc[MI][MJ];
#pragma unroll
    for (int m = 0; m < MI; ++m)
#pragma unroll
        for (int n = 0; n < MJ; ++n) acc[m][n] = (dc_f32x16)(0.f);
    const int chunks = (Wo + 15) >> 4;
    const int y0 = band * P.rows, y1 = min(y0 + P.rows, Ho);
    const int units = (y1 - y0) * chunks;
    for (int u = wv; u < units; u += 4) {
        const int Y = y0 + u / chunks, X0 = (u % chunks) * 16 + half * 8;
        const int sy = 2 * Y - 1 + dy;
        const bool row_ok = sy >= 0 && sy < P.H;
        uint4 a[MI][3], bb[MJ][3];
#pragma unroll
        for (int m = 0; m < MI; ++m) {
            const int ci = (cit * MI + m) * 32 + l31;
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int X = X0 + e, sx = 2 * X - 1 + dx;
                v[e] = (ci < P.cin && row_ok && X < Wo && sx >= 0 && sx < P.W) ? P.x[((size_t)sy * P.W + sx) * P.x_stride + ci] : 0.f;
            }
            dc_split3(v, a[m][0], a[m][1], a[m][2]);
        }
#pragma unroll
        for (int n = 0; n < MJ; ++n) {
            const int co = (cot * MJ + n) * 32 + l31;
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int X = X0 + e;
                v[e] = (co < P.cout && X < Wo) ? P.gy[((size_t)Y * Wo + X) * P.gy_stride + co] : 0.f;
            }
            dc_split3(v, bb[n][0], bb[n][1], bb[n][2]);
        }
#pragma unroll
        for (int m = 0; m < MI; ++m)
#pragma unroll
            for (int n = 0; n < MJ; ++n) DC_MFMA6(acc[m][n], a[m][0], a[m][1], a[m][2], bb[n][0], bb[n][1], bb[n][2]);
    }
    if (wv > 0) {
#pragma unroll
        for (int m = 0; m < MI; ++m)
#pragma unroll
            for (int n = 0; n < MJ; ++n)
#pragma unroll
                for (int r = 0; r < 16; ++r) red[wv - 1][((m * MJ + n) * 16 + r) * 64 + lane] = acc[m][n][r];
    }
    __syncthreads();
    if (wv != 0) return;
    float* const out = P.part + (size_t)band * P.cout * P.cin * 16;
#pragma unroll
    for (int m = 0; m < MI; ++m)
#pragma unroll
        for (int n = 0; n < MJ; ++n) {
            const int co = (cot * MJ + n) * 32 + l31;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int q = ((m * MJ + n) * 16 + r) * 64 + lane;
                const float v = ((acc[m][n][r] + red[0][q]) + red[1][q]) + red[2][q];
                const int ci = (cit * MI + m) * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                if (ci < P.cin && co < P.cout) out[((size_t)co * P.cin + ci) * 16 + tap] = v;
            }
        }
}

__global__ __launch_bounds__(256) void k4_disc_band_sum_kernel(const float* __restrict__ part, int bands, int64_t n, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float s = part[i];
    for (int b = 1; b < bands; ++b) s += part[(size_t)b * n + i];
    out[i] = s;
}

static void disc_wgrad_plan(int cin, int cout, int H, int ncu, int& mi, int& mj, int& bands, int& rows) {
    mi = cin % 64 == 0 ? 2 : 1; mj = cout % 64 == 0 ? 2 : 1;
    const int tiles = 16 * ((cin + 32 * mi - 1) / (32 * mi)) * ((cout + 32 * mj - 1) / (32 * mj));
    const int Ho = H / 2;
    int want = (4 * ncu + tiles - 1) / tiles;
    if (want < 1) want = 1;
    if (want > Ho) want = Ho;
    rows = (Ho + want - 1) / want;
    bands = (Ho + rows - 1) / rows;
}

extern "C" int64_t k4_disc_wgrad_workspace_bytes(int32_t cin, int32_t cout, int32_t H, int32_t W) {
    if (cin <= 0 || cout <= 0 || H < 2 || W < 2 || (H & 1) || (W & 1)) return -1;
    int mi, mj, bands, rows;
    disc_wgrad_plan(cin, cout, H, k4_num_cus(), mi, mj, bands, rows);
    return (int64_t)bands * cout * cin * 16 * 4;
}

extern "C" int k4_disc_wgrad_s2(const float* x, int32_t cin, int32_t x_stride, int32_t H, int32_t W, const float* gy, int32_t cout, int32_t gy_stride,
                                float* dw, float* workspace, int64_t workspace_bytes, void* stream) {
    if (!x || !gy || !dw || !workspace || cin <= 0 || cout <= 0 || x_stride < cin || gy_stride < cout || H < 2 || W < 2) return K4_ERR_BAD_ARG;
    if ((H & 1) || (W & 1)) return K4_ERR_UNSUPPORTED;
    if (workspace_bytes < k4_disc_wgrad_workspace_bytes(cin, cout, H, W)) return K4_ERR_BAD_ARG;
    return k4_taped(stream, [=](void* stream) -> int {
        DiscWgrad P{};
        P.x = x; P.cin = cin; P.x_stride = x_stride; P.H = H; P.W = W; P.gy = gy; P.cout = cout; P.gy_stride = gy_stride; P.part = workspace;
        int mi, mj;
        disc_wgrad_plan(cin, cout, H, k4_num_cus(), mi, mj, P.bands, P.rows);
        P.ci_tiles = (cin + 32 * mi - 1) / (32 * mi); P.co_tiles = (cout + 32 * mj - 1) / (32 * mj);
        const unsigned grid = (unsigned)(16 * P.ci_tiles * P.co_tiles * P.bands);
        if (mi == 2 && mj == 2) hipLaunchKernelGGL((k4_disc_wgrad_kernel<2, 2>), dim3(grid), dim3(256), 0, (hipStream_t)stream, P);
        else if (mj == 2) hipLaunchKernelGGL((k4_disc_wgrad_kernel<1, 2>), dim3(grid), dim3(256), 0, (hipStream_t)stream, P);
        else if (mi == 2) hipLaunchKernelGGL((k4_disc_wgrad_kernel<2, 1>), dim3(grid), dim3(256), 0, (hipStream_t)stream, P);
        else hipLaunchKernelGGL((k4_disc_wgrad_kernel<1, 1>), dim3(grid), dim3(256), 0, (hipStream_t)stream, P);
        const int64_t n = (int64_t)cout * cin * 16;
        hipLaunchKernelGGL(k4_disc_band_sum_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, workspace, P.bands, n, dw);
        return k4_check_launch();
    });
}

// ---------------------------------------------------------------------------------------------------------------------------------
// x2 bilinear resampling, align_corners=False (aten upsample_bilinear2d: source = (o + 0.5) / 2 - 0.5 clamped at 0, the upper neighbour
// clamped at the last row; the same index / weight arithmetic here)
// ---------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void bl_src(int o, int n, int& i0, int& i1, float& l0, float& l1) {
    float s = ((float)o + 0.5f) * 0.5f - 0.5f;
    s = s < 0.f ? 0.f : s;
    i0 = (int)s;
    i1 = i0 + (i0 < n - 1 ? 1 : 0);
    l1 = s - (float)i0; l0 = 1.f - l1;
}
__device__ __forceinline__ float4 bl_ld(const float* a, const float* b, size_t o) {
    float4 v = *reinterpret_cast<const float4*>(a + o);
    if (b) { const float4 w = *reinterpret_cast<const float4*>(b + o); v.x += w.x; v.y += w.y; v.z += w.z; v.w += w.w; }
    return v;
}
__global__ __launch_bounds__(256) void k4_bilinear2x_kernel(const float* __restrict__ a, const float* __restrict__ b, int H, int W, int C4, float* __restrict__ y) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t total = (int64_t)4 * H * W * C4;
    if (idx >= total) return;
    const int c = (int)(idx % C4);
    int64_t r = idx / C4;
    const int ox = (int)(r % (2 * W)), oy = (int)(r / (2 * W));
    int y0, y1, x0, x1; float hy0, hy1, hx0, hx1;
    bl_src(oy, H, y0, y1, hy0, hy1); bl_src(ox, W, x0, x1, hx0, hx1);
    const size_t C = (size_t)C4 * 4;
    const float4 p00 = bl_ld(a, b, ((size_t)y0 * W + x0) * C + 4 * c), p01 = bl_ld(a, b, ((size_t)y0 * W + x1) * C + 4 * c);
    const float4 p10 = bl_ld(a, b, ((size_t)y1 * W + x0) * C + 4 * c), p11 = bl_ld(a, b, ((size_t)y1 * W + x1) * C + 4 * c);
    float4 o;
    o.x = hy0 * (hx0 * p00.x + hx1 * p01.x) + hy1 * (hx0 * p10.x + hx1 * p11.x);
    o.y = hy0 * (hx0 * p00.y + hx1 * p01.y) + hy1 * (hx0 * p10.y + hx1 * p11.y);
    o.z = hy0 * (hx0 * p00.z + hx1 * p01.z) + hy1 * (hx0 * p10.z + hx1 * p11.z);
    o.w = hy0 * (hx0 * p00.w + hx1 * p01.w) + hy1 * (hx0 * p10.w + hx1 * p11.w);
    *reinterpret_cast<float4*>(y + ((size_t)oy * 2 * W + ox) * C + 4 * c) = o;
}
// the (at most four) output rows that read input row i, with their weights: the transpose of the table above
__device__ __forceinline__ int bl_adj(int i, int n, int (&o)[4], float (&w)[4]) {
    int k = 0;
    if (i >= 1) { o[k] = 2 * i - 1; w[k] = 0.25f; ++k; }
    o[k] = 2 * i; w[k] = i == 0 ? 1.f : 0.75f; ++k;
    o[k] = 2 * i + 1; w[k] = i == n - 1 ? 1.f : 0.75f; ++k;
    if (i <= n - 2) { o[k] = 2 * i + 2; w[k] = 0.25f; ++k; }
    return k;
}
__global__ __launch_bounds__(256) void k4_bilinear2x_bwd_kernel(const float* __restrict__ gy, int H, int W, int C4, float* __restrict__ gx) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t total = (int64_t)H * W * C4;
    if (idx >= total) return;
    const int c = (int)(idx % C4);
    int64_t r = idx / C4;
    const int X = (int)(r % W), Y = (int)(r / W);
    int oys[4], oxs[4]; float wy[4], wx[4];
    const int ny = bl_adj(Y, H, oys, wy), nx = bl_adj(X, W, oxs, wx);
    const size_t C = (size_t)C4 * 4;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int j = 0; j < ny; ++j) {
        float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int i = 0; i < nx; ++i) {
            const float4 g = *reinterpret_cast<const float4*>(gy + ((size_t)oys[j] * 2 * W + oxs[i]) * C + 4 * c);
            t.x += wx[i] * g.x; t.y += wx[i] * g.y; t.z += wx[i] * g.z; t.w += wx[i] * g.w;
        }
        s.x += wy[j] * t.x; s.y += wy[j] * t.y; s.z += wy[j] * t.z; s.w += wy[j] * t.w;
    }
    *reinterpret_cast<float4*>(gx + ((size_t)Y * W + X) * C + 4 * c) = s;
}

extern "C" int k4_bilinear2x_nhwc(const float* x, const float* add, int32_t H, int32_t W, int32_t channels, float* y, void* stream) {
    if (!x || !y || H <= 0 || W <= 0 || channels <= 0) return K4_ERR_BAD_ARG;
    if (channels % 4 != 0 || (((uintptr_t)x | (uintptr_t)y | (uintptr_t)add) & 15) != 0) return K4_ERR_UNSUPPORTED;
    const int64_t total = (int64_t)4 * H * W * (channels / 4);
    if ((total + 255) / 256 > 0x7fffffffLL) return K4_ERR_UNSUPPORTED;
    return k4_taped(stream, [=](void* stream) -> int {
        hipLaunchKernelGGL(k4_bilinear2x_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, add, H, W, channels / 4, y);
        return k4_check_launch();
    });
}
extern "C" int k4_bilinear2x_bwd_nhwc(const float* grad_y, int32_t H, int32_t W, int32_t channels, float* grad_x, void* stream) {
    if (!grad_y || !grad_x || H <= 0 || W <= 0 || channels <= 0) return K4_ERR_BAD_ARG;
    if (channels % 4 != 0 || (((uintptr_t)grad_y | (uintptr_t)grad_x) & 15) != 0) return K4_ERR_UNSUPPORTED;
    const int64_t total = (int64_t)H * W * (channels / 4);
    if ((total + 255) / 256 > 0x7fffffffLL) return K4_ERR_UNSUPPORTED;
    return k4_taped(stream, [=](void* stream) -> int {
        hipLaunchKernelGGL(k4_bilinear2x_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, grad_y, H, W, channels / 4, grad_x);
        return k4_check_launch();
    });
}

// ---------------------------------------------------------------------------------------------------------------------------------
// spectral norm (torch.nn.utils.spectral_norm, one power iteration): Wm = weight_orig as [cout][K]
//   training:  v = normalize(Wm^T u), u = normalize(Wm v)   (x / max(|x|, eps)),   sigma = u . (Wm v),   W = weight_orig / sigma
//   eval    :  sigma = u . (Wm v) with the stored u, v
// ---------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float sn_wave_sum(float v) {                     // butterfly: every lane ends with the same bits
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
// t[k] = sum_co Wm[co][k] u[co], co ascending
__global__ __launch_bounds__(256) void k4_sn_wtu_kernel(const float* __restrict__ w, const float* __restrict__ u, int cout, int K, float* __restrict__ t) {
    const int k = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (k >= K) return;
    float s = 0.f;
    for (int co = 0; co < cout; ++co) s = fmaf(w[(size_t)co * K + k], u[co], s);
    t[k] = s;
}
// s[co] = Wm[co] . v', v' = train ? t / max(|t|, eps) : v; one wave per row; the wave of row 0 stores v'
__global__ __launch_bounds__(256) void k4_sn_wv_kernel(const float* __restrict__ w, const float* __restrict__ t, float* __restrict__ v, int cout, int K, int train,
                                                        float eps, float* __restrict__ s) {
    const int lane = k4_lane();
    const int co = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (co >= cout) return;
    float nrm = 1.f;
    if (train) {
        float ss = 0.f;
        for (int k = lane; k < K; k += 64) ss = fmaf(t[k], t[k], ss);
        nrm = fmaxf(sqrtf(sn_wave_sum(ss)), eps);
    }
    float acc = 0.f;
    for (int k = lane; k < K; k += 64) {
        const float vk = train ? t[k] / nrm : v[k];
        acc = fmaf(w[(size_t)co * K + k], vk, acc);
        if (train && co == 0) v[k] = vk;
    }
    acc = sn_wave_sum(acc);
    if (lane == 0) s[co] = acc;
}
__device__ __forceinline__ float sn_block_sum(float v, float* sh) {          // 256 threads, fixed tree
    v = sn_wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63u) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}
// one workgroup: training: u = s / max(|s|, eps); sigma = u . s
__global__ __launch_bounds__(256) void k4_sn_finish_kernel(const float* __restrict__ s, float* __restrict__ u, int cout, int train, float eps, float* __restrict__ sigma) {
    __shared__ float sh[4];
    float nrm = 1.f;
    if (train) {
        float ss = 0.f;
        for (int i = (int)threadIdx.x; i < cout; i += 256) ss = fmaf(s[i], s[i], ss);
        nrm = fmaxf(sqrtf(sn_block_sum(ss, sh)), eps);
    }
    float d = 0.f;
    for (int i = (int)threadIdx.x; i < cout; i += 256) {
        const float ui = train ? s[i] / nrm : u[i];
        if (train) u[i] = ui;
        d = fmaf(ui, s[i], d);
    }
    d = sn_block_sum(d, sh);
    if (threadIdx.x == 0) sigma[0] = d;
}
// weight_orig / sigma as packed operands; blockIdx.y = 0: `out_fwd` (v = W[n][c][tap]); 1: `out_bwd` in `bwd_form`
//   K4_DISC_PACK_FLIP (the 3x3 input-gradient operand of k4_conv2d_nhwc_bf16x6): v = W[c][n][taps - 1 - tap];  K4_DISC_PACK_T (k4_disc_conv_s2): v = W[c][n][tap]
__global__ __launch_bounds__(256) void k4_sn_pack_kernel(const float* __restrict__ w, const float* __restrict__ sigma, int cout, int cin, int taps, int bwd_form,
                                                          uint4* __restrict__ out_fwd, uint4* __restrict__ out_bwd) {
    const bool bwd = blockIdx.y == 1;
    const int n_l = bwd ? cin : cout, c_l = bwd ? cout : cin;
    const int NOUT = (n_l + 31) / 32 * 32, nch = (c_l + 15) / 16;
    const int idx = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (idx >= nch * taps * 2 * NOUT) return;
    const float sg = sigma ? sigma[0] : 1.f;
    const int n = idx % NOUT;
    int r = idx / NOUT;
    const int g2 = r & 1; r >>= 1;
    const int tap = r % taps, ch = r / taps;
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int c = ch * 16 + g2 * 8 + e;
        float q = 0.f;
        if (n < n_l && c < c_l)
            q = !bwd ? w[((size_t)n * cin + c) * taps + tap] : w[((size_t)c * cin + n) * taps + (bwd_form == K4_DISC_PACK_FLIP ? taps - 1 - tap : tap)];
        v[e] = q / sg;
    }
    uint4 t0, t1, t2;
    dc_split3(v, t0, t1, t2);
    const size_t plane = (size_t)taps * 2 * NOUT;
    uint4* const o = (bwd ? out_bwd : out_fwd) + ((size_t)ch * 3) * plane + ((size_t)tap * 2 + g2) * NOUT + n;
    o[0] = t0; o[plane] = t1; o[2 * plane] = t2;
}

extern "C" int k4_sn_prepare(const float* weight_orig, float* u, float* v, int32_t cout, int32_t cin, int32_t ksize, int32_t train, float eps,
                             float* sigma, float* workspace, void* w_fwd, void* w_bwd, int32_t bwd_form, void* stream) {
    if (!weight_orig || !u || !v || !sigma || !workspace || cout <= 0 || cin <= 0 || (ksize != 3 && ksize != 4)) return K4_ERR_BAD_ARG;
    if (w_bwd && bwd_form != K4_DISC_PACK_FLIP && bwd_form != K4_DISC_PACK_T) return K4_ERR_BAD_ARG;
    const int taps = ksize * ksize;
    const int64_t K64 = (int64_t)cin * taps;
    if (K64 > (1 << 24) || (int64_t)cout * K64 > (1LL << 30)) return K4_ERR_UNSUPPORTED;
    const int K = (int)K64;
    return k4_taped(stream, [=](void* stream) -> int {
        hipStream_t st = (hipStream_t)stream;
        float* const t = workspace;                      // [K]
        float* const s = workspace + K;                  // [cout]
        if (train) hipLaunchKernelGGL(k4_sn_wtu_kernel, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, st, weight_orig, (const float*)u, cout, K, t);
        hipLaunchKernelGGL(k4_sn_wv_kernel, dim3((unsigned)((cout + 3) / 4)), dim3(256), 0, st, weight_orig, (const float*)t, v, cout, K, train, eps, s);
        hipLaunchKernelGGL(k4_sn_finish_kernel, dim3(1), dim3(256), 0, st, (const float*)s, u, cout, train, eps, sigma);
        if (w_fwd || w_bwd) {
            const int tot_f = ((cin + 15) / 16) * taps * 2 * ((cout + 31) / 32 * 32), tot_b = ((cout + 15) / 16) * taps * 2 * ((cin + 31) / 32 * 32);
            const int tot = tot_f > tot_b ? tot_f : tot_b;
            if (w_fwd && w_bwd)
                hipLaunchKernelGGL(k4_sn_pack_kernel, dim3((unsigned)((tot + 255) / 256), 2), dim3(256), 0, st, weight_orig, (const float*)sigma, cout, cin, taps, bwd_form,
                                   reinterpret_cast<uint4*>(w_fwd), reinterpret_cast<uint4*>(w_bwd));
            else if (w_fwd)
                hipLaunchKernelGGL(k4_sn_pack_kernel, dim3((unsigned)((tot_f + 255) / 256), 1), dim3(256), 0, st, weight_orig, (const float*)sigma, cout, cin, taps, bwd_form,
                                   reinterpret_cast<uint4*>(w_fwd), (uint4*)nullptr);
            else
                return K4_ERR_BAD_ARG;
        }
        return k4_check_launch();
    });
}

// dL/dweight_orig = G / sigma - (<G, weight_orig> / sigma^2) outer(u, v)
#define K4_SN_DOT_SPAN 16384
__global__ __launch_bounds__(256) void k4_sn_dot_kernel(const float* __restrict__ g, const float* __restrict__ w, int64_t n, float* __restrict__ part) {
    __shared__ float sh[4];
    const int64_t base = (int64_t)blockIdx.x * K4_SN_DOT_SPAN;
    float d = 0.f;
    for (int i = (int)threadIdx.x; i < K4_SN_DOT_SPAN; i += 256) {
        const int64_t q = base + i;
        if (q < n) d = fmaf(g[q], w[q], d);
    }
    d = sn_block_sum(d, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = d;
}
__global__ __launch_bounds__(256) void k4_sn_project_kernel(const float* __restrict__ g, const float* __restrict__ part, int nparts, const float* __restrict__ u,
                                                             const float* __restrict__ v, const float* __restrict__ sigma, int K, int64_t n, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float dot = 0.f;
    for (int b = 0; b < nparts; ++b) dot += part[b];
    const float sg = sigma[0];
    const int co = (int)(i / K), k = (int)(i - (int64_t)co * K);
    out[i] = g[i] / sg - (dot / (sg * sg)) * (u[co] * v[k]);
}
extern "C" int k4_sn_project_grad(const float* g, const float* weight_orig, const float* u, const float* v, const float* sigma, int32_t cout, int32_t K,
                                  float* workspace, float* out, void* stream) {
    if (!g || !weight_orig || !u || !v || !sigma || !workspace || !out || cout <= 0 || K <= 0) return K4_ERR_BAD_ARG;
    const int64_t n = (int64_t)cout * K;
    if (n > (1LL << 30)) return K4_ERR_UNSUPPORTED;
    const int nparts = (int)((n + K4_SN_DOT_SPAN - 1) / K4_SN_DOT_SPAN);
    return k4_taped(stream, [=](void* stream) -> int {
        hipLaunchKernelGGL(k4_sn_dot_kernel, dim3((unsigned)nparts), dim3(256), 0, (hipStream_t)stream, g, weight_orig, n, workspace);
        hipLaunchKernelGGL(k4_sn_project_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, g, (const float*)workspace, nparts, u, v, sigma, K, n, out);
        return k4_check_launch();
    });
}
extern "C" int64_t k4_sn_workspace_floats(int32_t cout, int32_t cin, int32_t ksize) {
    if (cout <= 0 || cin <= 0 || ksize <= 0) return -1;
    const int64_t K = (int64_t)cin * ksize * ksize, n = K * cout;
    const int64_t a = K + cout, b = (n + K4_SN_DOT_SPAN - 1) / K4_SN_DOT_SPAN;
    return a > b ? a : b;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// vanilla GAN loss on logits: target real: mean(softplus(-x)); fake: mean(softplus(x))     (BCEWithLogitsLoss against ones / zeros)
// ---------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float gan_softplus(float z) { return fmaxf(z, 0.f) + log1pf(expf(-fabsf(z))); }
__global__ __launch_bounds__(1024) void k4_gan_loss_kernel(const float* __restrict__ x, int64_t n, int real, float scale, float* __restrict__ loss) {
    __shared__ double sh[16];
    double s = 0.0;                                                          // one workgroup, fixed order; fp64 partial sums, one fp32 rounding
    for (int64_t i = threadIdx.x; i < n; i += 1024) s += (double)gan_softplus(real ? -x[i] : x[i]);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
    if ((threadIdx.x & 63u) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int q = 0; q < 16; ++q) t += sh[q];
        loss[0] = (float)(t / (double)n) * scale;
    }
}
__global__ __launch_bounds__(256) void k4_gan_loss_bwd_kernel(const float* __restrict__ x, int64_t n, int real, float scale, const float* __restrict__ go, float* __restrict__ gx) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float z = real ? -x[i] : x[i];
    const float e = expf(-fabsf(z));
    const float sig = z >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);           // sigmoid(z), stable on both sides
    const float g = (go ? go[0] : 1.f) * scale / (float)n;
    gx[i] = (real ? -sig : sig) * g;
}
extern "C" int k4_gan_loss_fwd(const float* logits, int64_t n, int32_t target_is_real, float scale, float* loss, void* stream) {
    if (!logits || !loss || n <= 0) return K4_ERR_BAD_ARG;
    return k4_taped(stream, [=](void* stream) -> int {
        hipLaunchKernelGGL(k4_gan_loss_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, logits, n, target_is_real, scale, loss);
        return k4_check_launch();
    });
}
extern "C" int k4_gan_loss_bwd(const float* logits, int64_t n, int32_t target_is_real, float scale, const float* grad_loss, float* grad_logits, void* stream) {
    if (!logits || !grad_logits || n <= 0 || (n + 255) / 256 > 0x7fffffffLL) return K4_ERR_BAD_ARG;
    return k4_taped(stream, [=](void* stream) -> int {
        hipLaunchKernelGGL(k4_gan_loss_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, logits, n, target_is_real, scale, grad_loss, grad_logits);
        return k4_check_launch();
    });
}
