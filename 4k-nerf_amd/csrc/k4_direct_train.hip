// One training step of the direct-colour DirectVoxGO (rgbnet_dim = 0: rgb = sigmoid(k0), no MLP) in three launches: render + per-ray loss partials,
// an ordered fp64 reduction of the loss terms (run_sr.py:523-546), and the gradients of density.grid and k0.grid.  No per-sample value reaches memory
// and the host is never waited for: the backward REPLAYS a ray, 64 steps at a time from its far end, from the transmittance the forward
// checkpointed at the start of every chunk.
//
// A sample's point, mask decision, density, alpha, transmittance and weight are the staged op sequence's bits (k4_staged_ops.h: aabb_t, n_steps_of,
// k_pts_fill's point, k4s_maskcache, k4s_grid_corners / k4s_grid_blend, k4s_raw2alpha; k_alpha2weight's sequential product), so the set of shaded
// samples is the staged path's.  What differs is the order of sums: a ray's colour is summed per lane and then across lanes, and the gradients are
// float atomics straight into the dense gradient tensors (not reproducible bit for bit from run to run, like the staged scatter).
#include "k4_common.h"
#include "k4_staged_ops.h"

#define K4D_THREADS 256                          // four waves = four rays per workgroup; no LDS, no barrier
#define K4D_MAX_CHUNKS 64                        // one bit per chunk in a ray's 64-bit chunk mask: max_steps <= 4096

extern "C" int32_t k4_direct_train_chunks(int32_t max_steps) {
    if (max_steps < 1 || max_steps > K4D_MAX_CHUNKS * K4_WAVE) return -1;
    return (max_steps + K4_WAVE - 1) / K4_WAVE;
}

// what the walk of one ray starts from: k_pts_count's t_min / N_steps and k_pts_fill's start and direction
struct K4dRay { float start[3], dir[3]; int n_steps; bool cut; };
__device__ __forceinline__ K4dRay k4d_ray(const k4_direct_train_desc& A, int64_t r, int n_chunks) {
    K4dRay R;
    float t_min, t_max;
    aabb_t(A.rays_o, A.rays_d, A.xyz_min, A.xyz_max, A.near, 1e9f, r, t_min, t_max);
    const float rn = ray_norm(A.rays_d, r);
    const int64_t n = n_steps_of(t_min, t_max, rn, A.stepdist);
    R.cut = n > (int64_t)n_chunks * K4_WAVE;                                                    // max_steps was no bound: the forward says so (NaN), never silently
    R.n_steps = (int)(R.cut ? (int64_t)n_chunks * K4_WAVE : n);                                 // never past the checkpoint table
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        R.start[c] = fmaf(A.rays_d[r * 3 + c], t_min, A.rays_o[r * 3 + c]);
        R.dir[c] = A.rays_d[r * 3 + c] / rn;
    }
    return R;
}
// step k of the ray: inside the box and on an occupied cell of the mask cache?
__device__ __forceinline__ bool k4d_sample(const k4_direct_train_desc& A, const K4dRay& R, int k, bool valid, float (&p)[3]) {
    const float dist = A.stepdist * (float)k;
#pragma unroll
    for (int c = 0; c < 3; ++c) p[c] = fmaf(R.dir[c], dist, R.start[c]);
    if (!valid || k4s_outbbox(p, A.xyz_min, A.xyz_max)) return false;
    return k4s_maskcache(A.mask, p[0], p[1], p[2], A.xyz2ijk_scale, A.xyz2ijk_shift, A.mask_dims[0], A.mask_dims[1], A.mask_dims[2]) != 0;
}
__device__ __forceinline__ void k4d_shade(const float* __restrict__ k0, size_t plane, const size_t (&idx)[8], const float (&w)[8], float (&rgb)[3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) rgb[c] = 1.f / (1.f + expf(-k4s_grid_blend(k0 + plane * c, idx, w)));
}
__device__ __forceinline__ float k4d_wave_sum(float v) {                 // fixed lane order; the sum is valid in lane 0
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    return v;
}

// ---------------------------------------------------------------- forward: one wave walks one ray in depth order, lanes = 64 consecutive steps
__global__ __launch_bounds__(K4D_THREADS) void k_direct_train_fwd(const k4_direct_train_desc A, int n_chunks) {
    const int lane = k4_lane();
    const int64_t r = (int64_t)blockIdx.x * (K4D_THREADS / K4_WAVE) + (threadIdx.x >> 6);
    if (r >= A.n_rays) return;
    const K4dRay R = k4d_ray(A, r, n_chunks);
    const int X = A.dims[0], Y = A.dims[1], Z = A.dims[2];
    const size_t plane = (size_t)X * Y * Z;
    const float thres = A.fast_color_thres;
    const bool filt = thres > 0.f;
    const float tgt[3] = {A.target[r * 3 + 0], A.target[r * 3 + 1], A.target[r * 3 + 2]};
    float T = 1.f;
    bool stopped = false;
    int end = R.n_steps, shaded = 0;
    unsigned long long cmask = 0;
    float acc[3] = {0.f, 0.f, 0.f}, per = 0.f;
    for (int base = 0; base < R.n_steps; base += K4_WAVE) {
        const int k = base + lane;
        float p[3];
        const bool keep = k4d_sample(A, R, k, k < R.n_steps, p);
        if (stopped) {                                                   // (thres == 0 only) behind the stop the staged list still holds every in-mask sample
            shaded += __popcll(__ballot(keep));
            continue;
        }
        if (lane == 0) A.ckpt[r * n_chunks + (base >> 6)] = T;
        size_t idx[8];
        float w[8], e, alpha = 0.f;
        if (keep) {
            k4s_grid_corners(p[0], p[1], p[2], A.xyz_min, A.xyz_max, X, Y, Z, idx, w);
            k4s_raw2alpha(k4s_grid_blend(A.density, idx, w), A.act_shift, A.interval, e, alpha);
        }
        const bool apass = keep && (filt ? alpha > thres : true);
        // the exact sequential product of k_alpha2weight over the alpha-passing samples, incl. the sample that crosses T < 1e-3
        float myw = 0.f;
        bool hit = false;
        uint64_t bm = __ballot(apass);
        while (bm && !stopped) {
            const int l = __builtin_ctzll(bm);
            const float al = k4_readlane(alpha, l);
            if (lane == l) { myw = T * al; hit = true; }
            T = fmaf(-T, al, T);
            bm &= bm - 1;
            if (T < 1e-3f) { stopped = true; end = base + l + 1; }
        }
        if (__ballot(hit)) cmask |= 1ull << (base >> 6);
        const bool wpass = hit && (filt ? myw > thres : true);
        shaded += __popcll(__ballot(filt ? wpass : keep));
        if (wpass) {
            float rgb[3];
            k4d_shade(A.k0, plane, idx, w, rgb);
            float d2 = 0.f;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                acc[c] = fmaf(myw, rgb[c], acc[c]);
                const float d = rgb[c] - tgt[c];
                d2 = fmaf(d, d, d2);
            }
            per = fmaf(myw, d2, per);
        }
        if (stopped && filt) break;                                      // nothing behind the stop is needed
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[c] = k4d_wave_sum(acc[c]);
    per = k4d_wave_sum(per);
    if (R.cut) T = acc[0] = per = __int_as_float(0x7fc00000);            // a ray cut at the table: NaN in every output of the ray and in the terms
    if (lane == 0) {
        float photo = 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float m = __fadd_rn(acc[c], __fmul_rn(T, A.bg));       // rgb_marched = sum + alphainv_last * bg (lib/dvgo.py:425-427)
            A.rgb_marched[r * 3 + c] = m;
            const float d = m - tgt[c];
            photo = fmaf(d, d, photo);
        }
        const float pc = fminf(fmaxf(T, 1e-6f), 1.f - 1e-6f);            // clamp(1e-6, 1 - 1e-6) on an fp32 tensor
        A.alphainv_last[r] = T;
        A.n_shaded[r] = shaded;
        A.end_step[r] = end;
        A.chunk_mask[r] = cmask;
        A.partials[r * 3 + 0] = photo;
        A.partials[r * 3 + 1] = pc * logf(pc) + (1.f - pc) * logf(1.f - pc);
        A.partials[r * 3 + 2] = per;
    }
}

// ---------------------------------------------------------------- the loss terms from the per-ray partials: fp64, fixed order, no atomics
__global__ __launch_bounds__(K4D_THREADS) void k_direct_train_terms(const float* __restrict__ partials, int64_t n_rays, float w_main, float w_ent, float w_per,
                                                                    float* __restrict__ terms, float* __restrict__ total) {
    __shared__ double sh[3][K4D_THREADS];
    double s[3] = {0.0, 0.0, 0.0};
    for (int64_t i = threadIdx.x; i < n_rays; i += K4D_THREADS)
#pragma unroll
        for (int c = 0; c < 3; ++c) s[c] += (double)partials[i * 3 + c];
#pragma unroll
    for (int c = 0; c < 3; ++c) sh[c][threadIdx.x] = s[c];
    __syncthreads();
    for (int off = K4D_THREADS / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off)
#pragma unroll
            for (int c = 0; c < 3; ++c) sh[c][threadIdx.x] += sh[c][threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double n = (double)n_rays;                                 // n == 0: 0 / 0, the mean of an empty tensor
        const double photo = (double)w_main * (sh[0][0] / (3.0 * n));
        const double entropy = w_ent != 0.f ? -(double)w_ent * (sh[1][0] / n) : 0.0;
        const double rgbper = w_per != 0.f ? (double)w_per * (sh[2][0] / n) : 0.0;
        terms[0] = (float)photo;
        terms[1] = (float)(-10.0 * log10(photo));
        terms[2] = (float)entropy;
        terms[3] = (float)rgbper;
        *total = (float)(photo + entropy + rgbper);
    }
}

// ---------------------------------------------------------------- backward: one wave per ray, its chunks from the far end
// Per chunk the samples are recomputed and the product replayed from the chunk's checkpoint: T_i and w_i carry the forward's bits.  With
//   g    = grad_total * weight_main * 2 (rgb_marched - target) / (3 n_rays)
//   gw_m = g . rgb_m for a shaded sample, 0 for one the weight filter dropped
//   gl   = bg (g_0 + g_1 + g_2) + d entropy / d alphainv_last   (0 outside the clamp interval, as torch's clamp)
// the alpha gradient is k_alpha2weight_bwd's  gw_i T_i - back_i / (1 - alpha_i + 1e-10),  back_i = gl ainv + sum_{j > i} gw_j w_j  (a suffix scan over the
// lanes plus the carry of the chunks behind), the density gradient k_raw2alpha_bwd's expression of it, and the colour gradient
//   (w_m g + weight_rgbper 2 (rgb_m - target) w_m / n_rays) rgb_m (1 - rgb_m).
// Both are scattered onto the 8 corners with float atomics: 32 adds = 128 B per shaded sample.
__global__ __launch_bounds__(K4D_THREADS) void k_direct_train_bwd(const k4_direct_train_desc A, int n_chunks, const float* __restrict__ grad_total,
                                                                  float* __restrict__ g_density, float* __restrict__ g_k0) {
    const int lane = k4_lane();
    const int64_t r = (int64_t)blockIdx.x * (K4D_THREADS / K4_WAVE) + (threadIdx.x >> 6);
    if (r >= A.n_rays) return;
    const unsigned long long cmask = A.chunk_mask[r];
    if (!cmask) return;                                                  // no sample entered the product: nothing depends on the grids
    const K4dRay R = k4d_ray(A, r, n_chunks);
    const int X = A.dims[0], Y = A.dims[1], Z = A.dims[2];
    const size_t plane = (size_t)X * Y * Z;
    const float thres = A.fast_color_thres;
    const bool filt = thres > 0.f;
    const float G = *grad_total, inv_n = 1.f / (float)A.n_rays;
    const float ainv = A.alphainv_last[r];
    const int end = A.end_step[r];
    float tgt[3], g[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        tgt[c] = A.target[r * 3 + c];
        g[c] = G * A.weight_main * 2.f * (A.rgb_marched[r * 3 + c] - tgt[c]) / (3.f * (float)A.n_rays);
    }
    float gl = A.bg * (g[0] + g[1] + g[2]);
    if (A.weight_entropy_last != 0.f && ainv >= 1e-6f && ainv <= 1.f - 1e-6f)
        gl += G * (-A.weight_entropy_last * inv_n) * (logf(ainv) - logf(1.f - ainv));
    const float cper = G * A.weight_rgbper * 2.f * inv_n;
    float carry = gl * ainv;                                             // back behind the chunk being processed (wave-uniform)
    for (int chunk = (end - 1) >> 6; chunk >= 0; --chunk) {
        if (!((cmask >> chunk) & 1)) continue;
        const int k = chunk * K4_WAVE + lane;
        float p[3];
        const bool keep = k4d_sample(A, R, k, k < end, p);
        size_t idx[8];
        float w[8], e = 0.f, alpha = 0.f;
        if (keep) {
            k4s_grid_corners(p[0], p[1], p[2], A.xyz_min, A.xyz_max, X, Y, Z, idx, w);
            k4s_raw2alpha(k4s_grid_blend(A.density, idx, w), A.act_shift, A.interval, e, alpha);
        }
        const bool apass = keep && (filt ? alpha > thres : true);
        float T = A.ckpt[r * n_chunks + chunk], myT = 1.f, myw = 0.f;
        for (uint64_t bm = __ballot(apass); bm; bm &= bm - 1) {          // k < end: every one of these entered the forward's product
            const int l = __builtin_ctzll(bm);
            const float al = k4_readlane(alpha, l);
            if (lane == l) { myT = T; myw = T * al; }
            T = fmaf(-T, al, T);
        }
        const bool shade = apass && (filt ? myw > thres : true);
        float rgb[3] = {0.f, 0.f, 0.f}, gw = 0.f;
        if (shade) {
            k4d_shade(A.k0, plane, idx, w, rgb);
            gw = g[0] * rgb[0] + g[1] * rgb[1] + g[2] * rgb[2];
        }
        const float term = gw * myw;
        float incl = term;                                               // inclusive sum over lanes lane..63 = this sample and the ones behind it
#pragma unroll
        for (int off = 1; off < K4_WAVE; off <<= 1) {
            const float v = __shfl_down(incl, off);
            if (lane + off < K4_WAVE) incl += v;
        }
        if (apass) {
            const float ga = gw * myT - (carry + (incl - term)) / (1.f - alpha + 1e-10f);
            const float gd = K4S_RAW2ALPHA_BWD(e, A.interval, ga);
            if (gd != 0.f)
#pragma unroll
                for (int c = 0; c < 8; ++c)
                    if (w[c] != 0.f) unsafeAtomicAdd(g_density + idx[c], w[c] * gd);
        }
        if (shade) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const float gk = (myw * g[ch] + cper * (rgb[ch] - tgt[ch]) * myw) * (rgb[ch] * (1.f - rgb[ch]));
                if (gk != 0.f)
#pragma unroll
                    for (int c = 0; c < 8; ++c)
                        if (w[c] != 0.f) unsafeAtomicAdd(g_k0 + plane * ch + idx[c], w[c] * gk);
            }
        }
        carry += __shfl(incl, 0);
    }
}

// ---------------------------------------------------------------- C ABI
static int k4d_check(const k4_direct_train_desc* d, int& n_chunks) {
    if (!d || d->n_rays < 0) return K4_ERR_BAD_ARG;
    if (d->density_ch != 1 || d->k0_ch != 3 || d->k0_layout != 0) return K4_ERR_UNSUPPORTED;           // channel-major fp32 DenseGrid pair, direct colour
    n_chunks = k4_direct_train_chunks(d->max_steps);
    if (n_chunks < 0) return K4_ERR_UNSUPPORTED;                                                         // max_steps outside the checkpoint table
    if (!d->density || !d->k0 || !d->mask || !d->xyz_min || !d->xyz_max || !d->xyz2ijk_scale || !d->xyz2ijk_shift) return K4_ERR_BAD_ARG;
    for (int a = 0; a < 3; ++a)
        if (d->dims[a] <= 0 || d->mask_dims[a] <= 0) return K4_ERR_BAD_ARG;
    if (!(d->stepdist > 0.f) || !(d->interval > 0.f) || !(d->fast_color_thres >= 0.f)) return K4_ERR_BAD_ARG;
    if (d->n_rays > 0 && (!d->rays_o || !d->rays_d || !d->target || !d->rgb_marched || !d->alphainv_last || !d->n_shaded || !d->end_step ||
                          !d->partials || !d->ckpt || !d->chunk_mask)) return K4_ERR_BAD_ARG;
    if (d->n_rays > (int64_t)0x7fffffff * (K4D_THREADS / K4_WAVE)) return K4_ERR_UNSUPPORTED;
    return K4_OK;
}

extern "C" int k4_direct_train_fwd(const k4_direct_train_desc* desc, float* terms, float* total, void* stream) {
    int n_chunks = 0;
    const int rc = k4d_check(desc, n_chunks);
    if (rc) return rc;
    if (!terms || !total) return K4_ERR_BAD_ARG;
    if (desc->n_rays > 0) {
        const unsigned blocks = (unsigned)((desc->n_rays + K4D_THREADS / K4_WAVE - 1) / (K4D_THREADS / K4_WAVE));
        hipLaunchKernelGGL(k_direct_train_fwd, dim3(blocks), dim3(K4D_THREADS), 0, (hipStream_t)stream, *desc, n_chunks);
        const int e = k4_check_launch();
        if (e) return e;
    }
    hipLaunchKernelGGL(k_direct_train_terms, dim3(1), dim3(K4D_THREADS), 0, (hipStream_t)stream, desc->partials, desc->n_rays, desc->weight_main,
                       desc->weight_entropy_last, desc->weight_rgbper, terms, total);
    return k4_check_launch();
}

extern "C" int k4_direct_train_bwd(const k4_direct_train_desc* desc, const float* grad_total, float* grad_density, float* grad_k0, void* stream) {
    int n_chunks = 0;
    const int rc = k4d_check(desc, n_chunks);
    if (rc) return rc;
    if (!grad_total || !grad_density || !grad_k0) return K4_ERR_BAD_ARG;
    if (desc->n_rays == 0) return K4_OK;
    const unsigned blocks = (unsigned)((desc->n_rays + K4D_THREADS / K4_WAVE - 1) / (K4D_THREADS / K4_WAVE));
    hipLaunchKernelGGL(k_direct_train_bwd, dim3(blocks), dim3(K4D_THREADS), 0, (hipStream_t)stream, *desc, n_chunks, grad_total, grad_density, grad_k0);
    return k4_check_launch();
}
