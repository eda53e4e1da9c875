// The perceptual and style terms of the "+gan" joint recipes on gfx950: a frozen VGG19 up to conv5_4 on the decoder output and the ground-truth patch
// (run_sr.py:670-678, 934-945; the formulas as lib/sr_loss.py:123-188 restates them), its input gradient, and the loss heads.
//
//   k4_vgg_conv3x3       3x3 stride-1 pad-1 convolution (or its input gradient, or a 1x1 product) on a batch of NHWC images: implicit GEMM on
//                        v_mfma_f32_32x32x16_bf16 with the exact 3-term bf16 split of both operands (6 partial products, fp32 accumulation: the arithmetic
//                        of k4_disc_conv_s2, with the correction products in an accumulator of their own: VG_MFMA6).  A workgroup owns MT tiles of 4 x 8 output pixels x 32*NT output channels; its four (or eight) waves split
//                        the reduction (tap, 16-channel chunk) round-robin and are summed through LDS in wave order -- conv5_x is 16 x 16 pixels with
//                        K = 4608.  A lane's 16 accumulator registers hold, for one channel, a 4-row x 4-column patch of the tile, so the 2x2 max pool
//                        that follows a layer is taken in registers in the epilogue.  Any H, W >= 1: a partial tile's pixels outside the image gather zeros and
//                        store nothing, and the pool is floor-mode (odd H or W: the last row or column is in no window).  Epilogue, forward: bias, the pre-ReLU copy of a tapped layer, ReLU,
//                        the pooled image.  Epilogue, input gradient: the ReLU mask of the producing layer (saved activation > 0) and an added seed.
//   k4_vgg_conv1_1       the first layer (3 planar input channels, normalisation (x - mean) / std in the load) and its input gradient (1 / std in the
//                        store, planar): 27-term sums in plain fp32, one fixed order.
//   k4_vgg_pool_bwd      gradient of the 2x2 max pool, routed to the first maximum of a window in (dy, dx) order, with the ReLU mask and an added seed.
//   k4_vgg_l1_* / gram   the loss heads: mean |a - b| (fixed-order fp64 partial sums, one fp32 rounding), its sign gradient, the Gram matrices of both
//                        images (a C x C product over the pixels, split over pixel bands that are summed in band order) and the operand of the Gram
//                        term's gradient, which is a 1x1 product of k4_vgg_conv3x3.
// No float atomics: every reduction runs in a fixed order, two runs give identical bits.
#include "k4_common.h"

typedef float vg_f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 vg_bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 vg_bf16x2 __attribute__((ext_vector_type(2)));
typedef float vg_f32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ unsigned vg_pk_bf16(float lo, float hi) {               // v_cvt_pk_bf16_f32 (RNE)
    const vg_f32x2 v = {lo, hi};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, vg_bf16x2));
}
// x == t0 + t1 + t2 exactly (bf16 terms, RNE of the successive remainders)
__device__ __forceinline__ void vg_split3(const float (&v)[8], uint4& t0, uint4& t1, uint4& t2) {
    unsigned p0[4], p1[4], p2[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float a = v[2 * i], b = v[2 * i + 1];
        p0[i] = vg_pk_bf16(a, b);
        const float ra = a - __uint_as_float(p0[i] << 16), rb = b - __uint_as_float(p0[i] & 0xffff0000u);
        p1[i] = vg_pk_bf16(ra, rb);
        const float sa = ra - __uint_as_float(p1[i] << 16), sb = rb - __uint_as_float(p1[i] & 0xffff0000u);
        p2[i] = vg_pk_bf16(sa, sb);
    }
    t0 = make_uint4(p0[0], p0[1], p0[2], p0[3]); t1 = make_uint4(p1[0], p1[1], p1[2], p1[3]); t2 = make_uint4(p2[0], p2[1], p2[2], p2[3]);
}
#define VG_MFMA(ACC, A, B) ACC = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(vg_bf16x8, A), __builtin_bit_cast(vg_bf16x8, B), ACC, 0, 0, 0)
// the six largest of the nine products of the 3-term splits; each of the three that are dropped (A1 B2, A2 B1, A2 B2) is at most 2^-24 of the full product
// (|a1| <= 2^-8 |a|, |a2| <= 2^-16 |a|).  The leading product A0 B0 has its own accumulator (HI); the five
// correction products, each below 2^-8 of it, are summed in a second one (LO, smallest first) and the two are added once, in fp32, after the reduction.
// Measured on gfx950: with all six in ONE accumulator the matrix instruction drops most of a correction product's bits when it adds it to the much larger
// running sum, and not symmetrically -- every output shrinks by about 1.5e-8 per layer, which after 16 layers put the perceptual term 2e-7 and the style term
// (quadratic in the features) 8e-7 below fp64, four to forty times torch fp32's deviation.  With two accumulators: 5e-8 and 1e-7 at most, and the largest error of
// a K = 4608 layer falls from 7.6e-7 to 3.6e-7 of the largest output (torch fp32 on the CPU: 3.3e-7).
#define VG_MFMA6(HI, LO, A0, A1, A2, B0, B1, B2) do { VG_MFMA(LO, A2, B0); VG_MFMA(LO, A0, B2); VG_MFMA(LO, A1, B1); \
                                                       VG_MFMA(LO, A1, B0); VG_MFMA(LO, A0, B1); VG_MFMA(HI, A0, B0); } while (0)

// ---------------------------------------------------------------------------------------------------------------------------------
// convolution / input gradient / 1x1 product
// ---------------------------------------------------------------------------------------------------------------------------------
struct VggConv {
    const float* x; int cin, H, W, B;                    // the tensor that is gathered from: [B][H][W][cin]
    const uint4* w; int NOUT, taps;                      // packed operand: [cin/16][3][taps][2][NOUT][8] bf16
    const float* bias;                                   // forward: [cout] or NULL
    float* y; float* y_pre; float* y_pool; int cout;     // [B][H][W][cout] (y, y_pre), [B][H/2][W/2][cout] (y_pool); each may be NULL
    const float* mask; const float* add;                 // input gradient: [B][H][W][cout] or NULL
    int mode, relu;
    int tiles_x, tiles_y, ntiles;
};

template <int MT, int NT, int KS>
__global__ __launch_bounds__(64 * KS, KS == 4 ? 2 : 1) void k4_vgg_conv_kernel(const VggConv P) {
    __shared__ float red[KS - 1][MT * NT * 16 * 64];
    const int lane = k4_lane(), wv = (int)(threadIdx.x >> 6), half = lane >> 5, l31 = lane & 31;
    // in = o + O + j * DJ, weight tap = j * 3 + i; one tap: in = o
    const int nj = P.taps == 9 ? 3 : 1;
    const int O = P.taps == 9 ? (P.mode == K4_VGG_CONV_DGRAD ? 1 : -1) : 0, DJ = P.mode == K4_VGG_CONV_DGRAD ? -1 : 1;
    const int nb0 = (int)blockIdx.y * NT;
    const int per_img = P.tiles_x * P.tiles_y;
    int oy[MT], ox[MT], img[MT];
    bool pok[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        const int t = (int)blockIdx.x * MT + m;
        img[m] = t / per_img;
        const int r = t - img[m] * per_img;
        const int ty = r / P.tiles_x, tx = r - ty * P.tiles_x;
        oy[m] = ty * 4 + (l31 >> 3); ox[m] = tx * 8 + (l31 & 7);
        pok[m] = t < P.ntiles && oy[m] < P.H && ox[m] < P.W;
    }
    vg_f32x16 acc[MT][NT];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int n = 0; n < NT; ++n) acc[m][n] = (vg_f32x16)(0.f);
    vg_f32x16 lo[MT][NT];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int n = 0; n < NT; ++n) lo[m][n] = (vg_f32x16)(0.f);
    const int nch = P.cin >> 4;
    const int steps = nj * nj * nch;
    const size_t plane = (size_t)P.taps * 2 * P.NOUT;                             // 16-byte units per (chunk, term)
    // one step = (tap, 16-channel chunk); the fetches of step s + KS are issued in front of the matrix instructions of step s
    float4 xa[MT][2];
    uint4 wb[NT][3];
    auto fetch = [&](int s) {
        const int ch = s % nch, t = s / nch;
        const int j = t / nj, i = t - j * nj;
        const int c0 = ch * 16 + half * 8;
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            const int iy = oy[m] + O + j * DJ, ix = ox[m] + O + i * DJ;
            if (pok[m] && iy >= 0 && iy < P.H && ix >= 0 && ix < P.W) {
                const float4* q = reinterpret_cast<const float4*>(P.x + (((size_t)img[m] * P.H + iy) * P.W + ix) * P.cin + c0);
                xa[m][0] = q[0]; xa[m][1] = q[1];
            } else {
                xa[m][0] = make_float4(0.f, 0.f, 0.f, 0.f); xa[m][1] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
        const uint4* wp = P.w + ((size_t)ch * 3) * plane + ((size_t)t * 2 + half) * P.NOUT + (size_t)nb0 * 32 + l31;
#pragma unroll
        for (int n = 0; n < NT; ++n) { wb[n][0] = wp[n * 32]; wb[n][1] = wp[plane + n * 32]; wb[n][2] = wp[2 * plane + n * 32]; }
    };
    if (wv < steps) fetch(wv);
    for (int s = wv; s < steps; s += KS) {
        uint4 a[MT][3], b[NT][3];
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            const float v[8] = {xa[m][0].x, xa[m][0].y, xa[m][0].z, xa[m][0].w, xa[m][1].x, xa[m][1].y, xa[m][1].z, xa[m][1].w};
            vg_split3(v, a[m][0], a[m][1], a[m][2]);
        }
#pragma unroll
        for (int n = 0; n < NT; ++n) { b[n][0] = wb[n][0]; b[n][1] = wb[n][1]; b[n][2] = wb[n][2]; }
        if (s + KS < steps) fetch(s + KS);
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                VG_MFMA6(acc[m][n], lo[m][n], a[m][0], a[m][1], a[m][2], b[n][0], b[n][1], b[n][2]);
            }
    }
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int n = 0; n < NT; ++n) acc[m][n] += lo[m][n];
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
    const int Hp = P.H >> 1, Wp = P.W >> 1;
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        const int t = (int)blockIdx.x * MT + m;
        if (t >= P.ntiles) continue;
        const int rr = t - img[m] * per_img;
        const int ty = rr / P.tiles_x, tx = rr - ty * P.tiles_x;
#pragma unroll
        for (int n = 0; n < NT; ++n) {
            const int co = (nb0 + n) * 32 + l31;
            const bool cok = co < P.cout;
            const float bias = (P.bias && cok) ? P.bias[co] : 0.f;
            float o[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int q = ((m * NT + n) * 16 + r) * 64 + lane;
                float v = acc[m][n][r];
#pragma unroll
                for (int k = 0; k < KS - 1; ++k) v += red[k][q];
                // accumulator register r of lane l = D[tile pixel (r & 3) + 8 (r >> 2) + 4 half][channel l31]: row r >> 2, column 4 half + (r & 3) of the 4 x 8 tile
                const int py = ty * 4 + (r >> 2), px = tx * 8 + 4 * half + (r & 3);
                const bool ok = cok && py < P.H && px < P.W;
                const size_t idx = (((size_t)img[m] * P.H + py) * P.W + px) * P.cout + co;
                if (P.mode == K4_VGG_CONV_FWD) {
                    v += bias;
                    if (ok && P.y_pre) P.y_pre[idx] = v;
                    if (P.relu) v = v > 0.f ? v : 0.f;
                } else {
                    if (ok && P.mask) v = P.mask[idx] > 0.f ? v : 0.f;
                    if (ok && P.add) v += P.add[idx];
                }
                if (ok && P.y) P.y[idx] = v;
                o[r] = v;
            }
            if (P.y_pool) {
#pragma unroll
                for (int wy = 0; wy < 2; ++wy)
#pragma unroll
                    for (int wx = 0; wx < 2; ++wx) {
                        const float v = fmaxf(fmaxf(o[(2 * wy) * 4 + 2 * wx], o[(2 * wy) * 4 + 2 * wx + 1]), fmaxf(o[(2 * wy + 1) * 4 + 2 * wx], o[(2 * wy + 1) * 4 + 2 * wx + 1]));
                        const int qy = ty * 2 + wy, qx = tx * 4 + 2 * half + wx;
                        if (cok && qy < Hp && qx < Wp) P.y_pool[(((size_t)img[m] * Hp + qy) * Wp + qx) * P.cout + co] = v;
                    }
            }
        }
    }
}

extern "C" int64_t k4_vgg_weight_bytes(int32_t outputs, int32_t inputs, int32_t ksize) {
    if (outputs <= 0 || inputs <= 0 || inputs % 16 != 0 || (ksize != 3 && ksize != 1)) return -1;
    return (int64_t)(inputs / 16) * 3 * ksize * ksize * 2 * ((outputs + 31) / 32 * 32) * 16;
}

extern "C" int k4_vgg_conv3x3(const float* x, int32_t cin, int32_t H, int32_t W, int32_t batch, const void* w_split, int32_t ksize, const float* bias,
                              float* y, float* y_pre, float* y_pool, int32_t cout, int32_t mode, int32_t relu, const float* mask, const float* add, void* stream) {
    if (!x || !w_split || (!y && !y_pre) || cin <= 0 || cout <= 0 || H <= 0 || W <= 0 || batch <= 0) return K4_ERR_BAD_ARG;
    if (mode != K4_VGG_CONV_FWD && mode != K4_VGG_CONV_DGRAD) return K4_ERR_BAD_ARG;
    if (ksize != 3 && ksize != 1) return K4_ERR_BAD_ARG;
    if (mode == K4_VGG_CONV_FWD && (mask || add)) return K4_ERR_BAD_ARG;
    if (mode == K4_VGG_CONV_DGRAD && (bias || y_pre || y_pool || relu)) return K4_ERR_BAD_ARG;
    if (cin % 16 != 0 || ((uintptr_t)x & 15) != 0) return K4_ERR_UNSUPPORTED;                                   // 16-byte activation loads
    // floor mode (torchvision's MaxPool2d(2, 2)): an odd last row or column belongs to no window.  The epilogue bounds a window by qy < H / 2 and qx < W / 2,
    // so every window it stores lies inside the image; an image with H or W below 2 has no window at all and is refused
    if (y_pool && (H < 2 || W < 2 || !relu)) return K4_ERR_UNSUPPORTED;
    if ((int64_t)H * W * batch > (1 << 26)) return K4_ERR_UNSUPPORTED;
    VggConv P{};
    P.x = x; P.cin = cin; P.H = H; P.W = W; P.B = batch;
    P.w = reinterpret_cast<const uint4*>(w_split); P.NOUT = (cout + 31) / 32 * 32; P.taps = ksize * ksize;
    P.bias = bias; P.y = y; P.y_pre = y_pre; P.y_pool = y_pool; P.cout = cout; P.mask = mask; P.add = add; P.mode = mode; P.relu = relu;
    P.tiles_x = (W + 7) / 8; P.tiles_y = (H + 3) / 4; P.ntiles = P.tiles_x * P.tiles_y * batch;
    const int nblk = P.NOUT / 32, nt = P.ntiles;
    return k4_taped(stream, [=](void* stream) -> int {
        // tile: the largest of (64 x 64), (32 x 64), (32 x 32) [pixels x channels] that still gives the chip a workgroup per CU; the smaller tiles split the
        // reduction over eight waves instead of four while the grid leaves SIMDs with fewer than two waves (the rule of k4_disc_conv_s2)
        const int ncu = k4_num_cus();
        const bool n2 = nblk % 2 == 0;
        const int64_t wg22 = (int64_t)((nt + 1) / 2) * (nblk / 2), wg12 = (int64_t)nt * (nblk / 2), wg11 = (int64_t)nt * nblk;
        const hipStream_t st = (hipStream_t)stream;
        if (n2 && wg22 >= ncu) hipLaunchKernelGGL((k4_vgg_conv_kernel<2, 2, 4>), dim3((unsigned)((nt + 1) / 2), (unsigned)(nblk / 2)), dim3(256), 0, st, P);
        else if (n2 && wg12 >= 2 * ncu) hipLaunchKernelGGL((k4_vgg_conv_kernel<1, 2, 4>), dim3((unsigned)nt, (unsigned)(nblk / 2)), dim3(256), 0, st, P);
        else if (n2) hipLaunchKernelGGL((k4_vgg_conv_kernel<1, 2, 8>), dim3((unsigned)nt, (unsigned)(nblk / 2)), dim3(512), 0, st, P);
        else if (wg11 >= 2 * ncu) hipLaunchKernelGGL((k4_vgg_conv_kernel<1, 1, 4>), dim3((unsigned)nt, (unsigned)nblk), dim3(256), 0, st, P);
        else hipLaunchKernelGGL((k4_vgg_conv_kernel<1, 1, 8>), dim3((unsigned)nt, (unsigned)nblk), dim3(512), 0, st, P);
        return k4_check_launch();
    });
}

// w [cout][cin][taps] fp32 -> the packed operand; K4_VGG_CONV_FWD: v(n, c) = W[n][c][tap] (n over cout); K4_VGG_CONV_DGRAD: v(n, c) = W[c][n][tap] (n over cin)
__global__ __launch_bounds__(256) void k4_vgg_pack_kernel(const float* __restrict__ w, int cout, int cin, int taps, int form, uint4* __restrict__ out) {
    const bool bwd = form == K4_VGG_CONV_DGRAD;
    const int n_l = bwd ? cin : cout, c_l = bwd ? cout : cin;
    const int NOUT = (n_l + 31) / 32 * 32, nch = c_l / 16;
    const int idx = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (idx >= nch * taps * 2 * NOUT) return;
    const int n = idx % NOUT;
    int r = idx / NOUT;
    const int g2 = r & 1; r >>= 1;
    const int tap = r % taps, ch = r / taps;
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int c = ch * 16 + g2 * 8 + e;
        v[e] = n < n_l ? (!bwd ? w[((size_t)n * cin + c) * taps + tap] : w[((size_t)c * cin + n) * taps + tap]) : 0.f;
    }
    uint4 t0, t1, t2;
    vg_split3(v, t0, t1, t2);
    const size_t plane = (size_t)taps * 2 * NOUT;
    uint4* const o = out + ((size_t)ch * 3) * plane + ((size_t)tap * 2 + g2) * NOUT + n;
    o[0] = t0; o[plane] = t1; o[2 * plane] = t2;
}

extern "C" int k4_vgg_pack_weight(const float* w, int32_t cout, int32_t cin, int32_t ksize, int32_t form, void* w_split, void* stream) {
    if (!w || !w_split || cout <= 0 || cin <= 0 || (ksize != 3 && ksize != 1)) return K4_ERR_BAD_ARG;
    if (form != K4_VGG_CONV_FWD && form != K4_VGG_CONV_DGRAD) return K4_ERR_BAD_ARG;
    const int c_l = form == K4_VGG_CONV_DGRAD ? cout : cin, n_l = form == K4_VGG_CONV_DGRAD ? cin : cout;
    if (c_l % 16 != 0) return K4_ERR_UNSUPPORTED;
    const int64_t tot = (int64_t)(c_l / 16) * ksize * ksize * 2 * ((n_l + 31) / 32 * 32);
    if (tot > (1 << 30)) return K4_ERR_UNSUPPORTED;
    return k4_taped(stream, [=](void* stream) -> int {
        hipLaunchKernelGGL(k4_vgg_pack_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, cout, cin, ksize * ksize, form,
                           reinterpret_cast<uint4*>(w_split));
        return k4_check_launch();
    });
}

// ---------------------------------------------------------------------------------------------------------------------------------
// conv1_1: 3 planar channels in, 64 out
// ---------------------------------------------------------------------------------------------------------------------------------
struct Vgg11 { const float* img[2]; };
__global__ __launch_bounds__(256) void k4_vgg_conv1_1_kernel(const Vgg11 I, int H, int W, const float* __restrict__ mean, const float* __restrict__ stdv,
                                                              const float* __restrict__ w, const float* __restrict__ bias, int cout,
                                                              float* __restrict__ y, float* __restrict__ y_pre) {
    const int p = (int)blockIdx.x * 256 + (int)threadIdx.x;
    const int b = (int)blockIdx.z, cg = (int)blockIdx.y;                    // 16 output channels per thread
    if (p >= H * W) return;
    const int py = p / W, px = p - py * W;
    const float* const x = I.img[b];
    float in[27];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int d = 0; d < 9; ++d) {
            const int iy = py - 1 + d / 3, ix = px - 1 + d % 3;
            in[c * 9 + d] = (iy >= 0 && iy < H && ix >= 0 && ix < W) ? (x[((size_t)c * H + iy) * W + ix] - mean[c]) / stdv[c] : 0.f;       // zero padding of the NORMALISED image
        }
    const k4_cptr wc = k4_const(w), bc = k4_const(bias);
    float o[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int co = cg * 16 + k;
        float s = 0.f;
#pragma unroll
        for (int q = 0; q < 27; ++q) s = fmaf(in[q], wc[co * 27 + q], s);
        o[k] = s + bc[co];
    }
    const size_t base = ((size_t)b * H * W + p) * cout + cg * 16;
#pragma unroll
    for (int k = 0; k < 16; k += 4) {
        if (y_pre) *reinterpret_cast<float4*>(y_pre + base + k) = make_float4(o[k], o[k + 1], o[k + 2], o[k + 3]);
        if (y) *reinterpret_cast<float4*>(y + base + k) = make_float4(fmaxf(o[k], 0.f), fmaxf(o[k + 1], 0.f), fmaxf(o[k + 2], 0.f), fmaxf(o[k + 3], 0.f));
    }
}
extern "C" int k4_vgg_conv1_1(const float* x0, const float* x1, int32_t H, int32_t W, const float* mean, const float* stdv, const float* w, const float* bias,
                              int32_t cout, float* y, float* y_pre, void* stream) {
    if (!x0 || !mean || !stdv || !w || !bias || (!y && !y_pre) || H <= 0 || W <= 0 || cout <= 0) return K4_ERR_BAD_ARG;
    if (cout % 16 != 0 || (((uintptr_t)y | (uintptr_t)y_pre) & 15) != 0 || (int64_t)H * W > (1 << 26)) return K4_ERR_UNSUPPORTED;
    Vgg11 I{}; I.img[0] = x0; I.img[1] = x1;
    return k4_taped(stream, [=](void* stream) -> int {
        hipLaunchKernelGGL(k4_vgg_conv1_1_kernel, dim3((unsigned)((H * W + 255) / 256), (unsigned)(cout / 16), x1 ? 2u : 1u), dim3(256), 0, (hipStream_t)stream,
                           I, H, W, mean, stdv, w, bias, cout, y, y_pre);
        return k4_check_launch();
    });
}

// d image [3][H][W] = (1 / std) sum_{co, d} g[p + 1 - d][co] W[co][ci][d]; four interleaved chains over co inside a tap, taps in order
__global__ __launch_bounds__(256) void k4_vgg_conv1_1_bwd_kernel(const float* __restrict__ g, int H, int W, int cout, const float* __restrict__ w,
                                                                  const float* __restrict__ stdv, float* __restrict__ gx) {
    const int p = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (p >= H * W) return;
    const int py = p / W, px = p - py * W;
    const k4_cptr wc = k4_const(w);
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    for (int d = 0; d < 9; ++d) {
        const int qy = py + 1 - d / 3, qx = px + 1 - d % 3;
        if (qy < 0 || qy >= H || qx < 0 || qx >= W) continue;
        const float4* gp = reinterpret_cast<const float4*>(g + ((size_t)qy * W + qx) * cout);
        float s0[4] = {0.f, 0.f, 0.f, 0.f}, s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};       // four chains per tap: shorter sums, one fixed order
        for (int c4 = 0; c4 < cout / 4; ++c4) {
            const float4 v = gp[c4];
            const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int co = c4 * 4 + k;
                s0[k] = fmaf(e[k], wc[co * 27 + d], s0[k]);
                s1[k] = fmaf(e[k], wc[co * 27 + 9 + d], s1[k]);
                s2[k] = fmaf(e[k], wc[co * 27 + 18 + d], s2[k]);
            }
        }
        a0 += (s0[0] + s0[1]) + (s0[2] + s0[3]);
        a1 += (s1[0] + s1[1]) + (s1[2] + s1[3]);
        a2 += (s2[0] + s2[1]) + (s2[2] + s2[3]);
    }
    const size_t n = (size_t)H * W;
    gx[p] = a0 / stdv[0]; gx[n + p] = a1 / stdv[1]; gx[2 * n + p] = a2 / stdv[2];
}
extern "C" int k4_vgg_conv1_1_bwd(const float* grad_y, int32_t H, int32_t W, int32_t cout, const float* w, const float* stdv, float* grad_x, void* stream) {
    if (!grad_y || !w || !stdv || !grad_x || H <= 0 || W <= 0 || cout <= 0) return K4_ERR_BAD_ARG;
    if (cout % 4 != 0 || ((uintptr_t)grad_y & 15) != 0 || (int64_t)H * W > (1 << 26)) return K4_ERR_UNSUPPORTED;
    return k4_taped(stream, [=](void* stream) -> int {
        hipLaunchKernelGGL(k4_vgg_conv1_1_bwd_kernel, dim3((unsigned)((H * W + 255) / 256)), dim3(256), 0, (hipStream_t)stream, grad_y, H, W, cout, w, stdv, grad_x);
        return k4_check_launch();
    });
}

// ---------------------------------------------------------------------------------------------------------------------------------
// 2x2 max pool, backward: out [H][W][C] = (first maximum of its window in (dy, dx) order && act > 0 ? gp : 0) + add
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k4_vgg_pool_bwd_kernel(const float* __restrict__ act, const float* __restrict__ gp, const float* __restrict__ add,
                                                               int H, int W, int C4, int relu_mask, float* __restrict__ out) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int Hp = H >> 1, Wp = W >> 1;
    if (idx >= (int64_t)Hp * Wp * C4) return;
    const int c = (int)(idx % C4);
    const int64_t r = idx / C4;
    const int qx = (int)(r % Wp), qy = (int)(r / Wp);
    const size_t C = (size_t)C4 * 4;
    const float4 g4 = *reinterpret_cast<const float4*>(gp + ((size_t)qy * Wp + qx) * C + 4 * c);
    const float g[4] = {g4.x, g4.y, g4.z, g4.w};
    float a[4][4];
    size_t off[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        off[k] = ((size_t)(2 * qy + (k >> 1)) * W + (2 * qx + (k & 1))) * C + 4 * c;
        const float4 v = *reinterpret_cast<const float4*>(act + off[k]);
        a[k][0] = v.x; a[k][1] = v.y; a[k][2] = v.z; a[k][3] = v.w;
    }
    float o[4][4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        int best = 0;
#pragma unroll
        for (int k = 1; k < 4; ++k) if (a[k][e] > a[best][e]) best = k;                   // aten max_pool2d: replaced on `>` only -- the first maximum stays
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k][e] = (k == best && (!relu_mask || a[k][e] > 0.f)) ? g[e] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float4 v = make_float4(o[k][0], o[k][1], o[k][2], o[k][3]);
        if (add) { const float4 w = *reinterpret_cast<const float4*>(add + off[k]); v.x += w.x; v.y += w.y; v.z += w.z; v.w += w.w; }
        *reinterpret_cast<float4*>(out + off[k]) = v;
    }
}
extern "C" int k4_vgg_pool_bwd(const float* act, const float* grad_pooled, const float* add, int32_t H, int32_t W, int32_t channels, int32_t relu_mask,
                               float* grad_full, void* stream) {
    if (!act || !grad_pooled || !grad_full || H <= 0 || W <= 0 || channels <= 0) return K4_ERR_BAD_ARG;
    if ((H & 1) || (W & 1) || channels % 4 != 0 || (((uintptr_t)act | (uintptr_t)grad_pooled | (uintptr_t)add | (uintptr_t)grad_full) & 15) != 0) return K4_ERR_UNSUPPORTED;
    const int64_t total = (int64_t)(H / 2) * (W / 2) * (channels / 4);
    if ((total + 255) / 256 > 0x7fffffffLL) return K4_ERR_UNSUPPORTED;
    return k4_taped(stream, [=](void* stream) -> int {
        hipLaunchKernelGGL(k4_vgg_pool_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, act, grad_pooled, add, H, W, channels / 4,
                           relu_mask, grad_full);
        return k4_check_launch();
    });
}

// ---------------------------------------------------------------------------------------------------------------------------------
// loss heads
// ---------------------------------------------------------------------------------------------------------------------------------
#define K4_VGG_L1_SPAN 8192
__device__ __forceinline__ double vg_block_sum(double s, double* sh) {              // 256 threads, fixed tree
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
    __syncthreads();
    if ((threadIdx.x & 63u) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}
__global__ __launch_bounds__(256) void k4_vgg_l1_part_kernel(const float* __restrict__ a, const float* __restrict__ b, int64_t n, double* __restrict__ part) {
    __shared__ double sh[4];
    const int64_t base = (int64_t)blockIdx.x * K4_VGG_L1_SPAN;
    double s = 0.0;
    for (int i = (int)threadIdx.x; i < K4_VGG_L1_SPAN; i += 256) {
        const int64_t q = base + i;
        if (q < n) s += (double)fabsf(a[q] - b[q]);
    }
    s = vg_block_sum(s, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}
__global__ __launch_bounds__(256) void k4_vgg_l1_finish_kernel(const double* __restrict__ part, int nparts, int64_t n, float scale, double* __restrict__ loss) {
    __shared__ double sh[4];
    double s = 0.0;
    for (int i = (int)threadIdx.x; i < nparts; i += 256) s += part[i];
    s = vg_block_sum(s, sh);
    if (threadIdx.x == 0) loss[0] = s / (double)n * (double)scale;
}
extern "C" int64_t k4_vgg_l1_workspace_bytes(int64_t n) { return n <= 0 ? -1 : (n + K4_VGG_L1_SPAN - 1) / K4_VGG_L1_SPAN * 8; }
extern "C" int k4_vgg_l1_fwd(const float* a, const float* b, int64_t n, float scale, void* workspace, double* loss, void* stream) {
    if (!a || !b || !workspace || !loss || n <= 0) return K4_ERR_BAD_ARG;
    const int64_t nparts = (n + K4_VGG_L1_SPAN - 1) / K4_VGG_L1_SPAN;
    if (nparts > (1 << 24) || (((uintptr_t)workspace | (uintptr_t)loss) & 7) != 0) return K4_ERR_UNSUPPORTED;
    return k4_taped(stream, [=](void* stream) -> int {
        hipLaunchKernelGGL(k4_vgg_l1_part_kernel, dim3((unsigned)nparts), dim3(256), 0, (hipStream_t)stream, a, b, n, reinterpret_cast<double*>(workspace));
        hipLaunchKernelGGL(k4_vgg_l1_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const double*>(workspace), (int)nparts, n, scale, loss);
        return k4_check_launch();
    });
}
// grad_a = grad_loss[0] (NULL: 1) * scale / n * sign(a - b) (+ add)
__global__ __launch_bounds__(256) void k4_vgg_l1_bwd_kernel(const float* __restrict__ a, const float* __restrict__ b, int64_t n, float scale, const float* __restrict__ go,
                                                             const float* __restrict__ add, float* __restrict__ ga) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float g = (float)((double)(go ? go[0] : 1.f) * (double)scale / (double)n);           // one rounding
    const float d = a[i] - b[i];
    float v = d > 0.f ? g : (d < 0.f ? -g : 0.f);
    if (add) v += add[i];
    ga[i] = v;
}
extern "C" int k4_vgg_l1_bwd(const float* a, const float* b, int64_t n, float scale, const float* grad_loss, const float* add, float* grad_a, void* stream) {
    if (!a || !b || !grad_a || n <= 0) return K4_ERR_BAD_ARG;
    if ((n + 255) / 256 > 0x7fffffffLL) return K4_ERR_UNSUPPORTED;
    return k4_taped(stream, [=](void* stream) -> int {
        hipLaunchKernelGGL(k4_vgg_l1_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a, b, n, scale, grad_loss, add, grad_a);
        return k4_check_launch();
    });
}

// Gram matrices: G[img][i][j] = sum_p f[img][p][i] f[img][p][j] / (C P); 64 x 64 tiles, the pixels cut in bands, a band's 16-pixel chunks dealt to the four waves
struct VggGram { const float* f; int P, C, bands, rows, tiles; float* part; };
__global__ __launch_bounds__(256, 2) void k4_vgg_gram_kernel(const VggGram G) {
    __shared__ float red[3][4 * 16 * 64];
    const int lane = k4_lane(), wv = (int)(threadIdx.x >> 6), half = lane >> 5, l31 = lane & 31;
    int b = (int)blockIdx.x;
    const int band = b % G.bands; b /= G.bands;
    const int jt = b % G.tiles; b /= G.tiles;
    const int it = b % G.tiles; b /= G.tiles;
    const int img = b;
    const float* const f = G.f + (size_t)img * G.P * G.C;
    vg_f32x16 acc[2][2], lo[2][2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) { acc[m][n] = (vg_f32x16)(0.f); lo[m][n] = (vg_f32x16)(0.f); }
    const int p0 = band * G.rows, p1 = min(p0 + G.rows, G.P);
    const int units = (p1 - p0 + 15) >> 4;
    for (int u = wv; u < units; u += 4) {
        const int X0 = p0 + u * 16 + half * 8;
        uint4 a[2][3], bb[2][3];
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            const int ci = (it * 2 + m) * 32 + l31, cj = (jt * 2 + m) * 32 + l31;
            float v[8], q[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const bool ok = X0 + e < p1;
                v[e] = ok ? f[(size_t)(X0 + e) * G.C + ci] : 0.f;
                q[e] = ok ? f[(size_t)(X0 + e) * G.C + cj] : 0.f;
            }
            vg_split3(v, a[m][0], a[m][1], a[m][2]);
            vg_split3(q, bb[m][0], bb[m][1], bb[m][2]);
        }
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int n = 0; n < 2; ++n) VG_MFMA6(acc[m][n], lo[m][n], a[m][0], a[m][1], a[m][2], bb[n][0], bb[n][1], bb[n][2]);
    }
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) acc[m][n] += lo[m][n];
    if (wv > 0) {
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int n = 0; n < 2; ++n)
#pragma unroll
                for (int r = 0; r < 16; ++r) red[wv - 1][((m * 2 + n) * 16 + r) * 64 + lane] = acc[m][n][r];
    }
    __syncthreads();
    if (wv != 0) return;
    float* const out = G.part + ((size_t)band * 2 + img) * G.C * G.C;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            const int cj = (jt * 2 + n) * 32 + l31;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int q = ((m * 2 + n) * 16 + r) * 64 + lane;
                const float v = ((acc[m][n][r] + red[0][q]) + red[1][q]) + red[2][q];
                const int ci = (it * 2 + m) * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                out[(size_t)ci * G.C + cj] = v;
            }
        }
}
__global__ __launch_bounds__(256) void k4_vgg_gram_finish_kernel(const float* __restrict__ part, int bands, int64_t n, float denom, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float s = part[i];
    for (int b = 1; b < bands; ++b) s += part[(size_t)b * n + i];
    out[i] = s / denom;
}
static void vgg_gram_plan(int P, int C, int ncu, int& bands, int& rows) {
    const int tiles = 2 * (C / 64) * (C / 64);
    int want = (2 * ncu + tiles - 1) / tiles;
    const int most = (P + 63) / 64;
    if (want > most) want = most;
    if (want < 1) want = 1;
    rows = ((P + want - 1) / want + 15) / 16 * 16;
    bands = (P + rows - 1) / rows;
}
extern "C" int64_t k4_vgg_gram_workspace_bytes(int32_t n_pix, int32_t channels) {
    if (n_pix <= 0 || channels <= 0 || channels % 64 != 0) return -1;
    int bands, rows;
    vgg_gram_plan(n_pix, channels, k4_num_cus(), bands, rows);
    return (int64_t)bands * 2 * channels * channels * 4;
}
extern "C" int k4_vgg_gram(const float* f, int32_t n_pix, int32_t channels, float* workspace, int64_t workspace_bytes, float* gram, void* stream) {
    if (!f || !workspace || !gram || n_pix <= 0 || channels <= 0) return K4_ERR_BAD_ARG;
    if (channels % 64 != 0 || channels > 4096 || n_pix > (1 << 26)) return K4_ERR_UNSUPPORTED;
    if (workspace_bytes < k4_vgg_gram_workspace_bytes(n_pix, channels)) return K4_ERR_BAD_ARG;
    return k4_taped(stream, [=](void* stream) -> int {
        VggGram G{};
        G.f = f; G.P = n_pix; G.C = channels; G.part = workspace; G.tiles = channels / 64;
        vgg_gram_plan(n_pix, channels, k4_num_cus(), G.bands, G.rows);
        hipLaunchKernelGGL(k4_vgg_gram_kernel, dim3((unsigned)(2 * G.tiles * G.tiles * G.bands)), dim3(256), 0, (hipStream_t)stream, G);
        const int64_t n = (int64_t)2 * channels * channels;
        hipLaunchKernelGGL(k4_vgg_gram_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const float*)workspace, G.bands, n,
                           (float)channels * (float)n_pix, gram);
        return k4_check_launch();
    });
}
// the operand of the Gram term's gradient: d/df of scale * mean|Gx - Gg| is f M with M[j][i] = grad_loss * scale / (C^2) * (s_ij + s_ji) / (C P), s = sign(Gx - Gg)
// (= (2 / (C P)) S_sym f); packed as a one-tap operand of k4_vgg_conv3x3: v(n = i, c = j)
__global__ __launch_bounds__(256) void k4_vgg_gram_bwd_pack_kernel(const float* __restrict__ gram, int C, double coef, const float* __restrict__ go, uint4* __restrict__ out) {
    const int idx = (int)blockIdx.x * 256 + (int)threadIdx.x;
    const int nch = C / 16;
    if (idx >= nch * 2 * C) return;
    const int n = idx % C;
    int r = idx / C;
    const int g2 = r & 1, ch = r >> 1;
    const float k = (float)((double)(go ? go[0] : 1.f) * coef);
    const float* const gx = gram; const float* const gg = gram + (size_t)C * C;
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int c = ch * 16 + g2 * 8 + e;
        const float d0 = gx[(size_t)n * C + c] - gg[(size_t)n * C + c], d1 = gx[(size_t)c * C + n] - gg[(size_t)c * C + n];
        const float s = (d0 > 0.f ? 1.f : (d0 < 0.f ? -1.f : 0.f)) + (d1 > 0.f ? 1.f : (d1 < 0.f ? -1.f : 0.f));
        v[e] = k * s;
    }
    uint4 t0, t1, t2;
    vg_split3(v, t0, t1, t2);
    const size_t plane = (size_t)2 * C;
    uint4* const o = out + ((size_t)ch * 3) * plane + (size_t)g2 * C + n;
    o[0] = t0; o[plane] = t1; o[2 * plane] = t2;
}
extern "C" int k4_vgg_gram_bwd_pack(const float* gram, int32_t n_pix, int32_t channels, float scale, const float* grad_loss, void* w_split, void* stream) {
    if (!gram || !w_split || n_pix <= 0 || channels <= 0) return K4_ERR_BAD_ARG;
    if (channels % 32 != 0 || channels > 4096) return K4_ERR_UNSUPPORTED;
    const double coef = (double)scale / ((double)channels * (double)channels) / ((double)channels * (double)n_pix);
    const int tot = (channels / 16) * 2 * channels;
    return k4_taped(stream, [=](void* stream) -> int {
        hipLaunchKernelGGL(k4_vgg_gram_bwd_pack_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, (hipStream_t)stream, gram, channels, coef, grad_loss,
                           reinterpret_cast<uint4*>(w_split));
        return k4_check_launch();
    });
}
