// The one-launch marchers of k4_staged.hip (k_march_contracted, k_march_vq, k_march_bivox): what a grid and an rgbnet are to them, and the walk of
// one wave along one ray that all three run.  Included by k4_staged.hip only.
#pragma once
#include "k4_common.h"

// a density grid with its colour-feature grid (channel-major [C][X][Y][Z]; k_march_vq has none: its feature is the codebook's) and its mask cache
struct K4Grid {
    const float* density; const float* k0; int C, X, Y, Z; const float *mn, *mx;
    const uint8_t* mask; int MX, MY, MZ; const float *sc, *sh;
};
// a Linear-ReLU rgbnet (the nn.Linear tensors) and the frequencies of the embedding among its inputs (view directions; k_march_vq: positions)
struct K4Net {
    const float *w1, *b1, *w2, *b2, *w3, *b3; int dim0, n_hidden; const float* freq; int n_pe;
};

// o' = (o - c) / r, d' = d / |d|: every op rounded once, as the tensor expressions of sample_ray (lib/dcvgo.py, lib/dbvgo.py)
__device__ __forceinline__ void k4w_unit_ray(const float* __restrict__ ro, const float* __restrict__ rd, int64_t ray, const float (&c)[3], const float (&r)[3],
                                             float (&o)[3], float (&d)[3]) {
    const float dv[3] = {rd[ray * 3 + 0], rd[ray * 3 + 1], rd[ray * 3 + 2]};
    const float dn = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(dv[0], dv[0]), __fmul_rn(dv[1], dv[1])), __fmul_rn(dv[2], dv[2])));
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        o[a] = __fdiv_rn(__fsub_rn(ro[ray * 3 + a], c[a]), r[a]);
        d[a] = __fdiv_rn(dv[a], dn);
    }
}

// What a model supplies to the walk (lambdas, inlined):
//   n_steps                      steps of this pass
//   sample(k, valid, p) -> pre   the point of step k and whether it passes the model's pre-filter.  Runs for all 64 lanes of a chunk (valid = k < n_steps),
//                                never under a divergent branch: it may be wave-collective and carry state from chunk to chunk
//   mask(p) -> bool              the mask cache at p
//   alpha(p) -> float            the activated density at p
//   shade(k, rgb)                the colour of survivor k
//   depth(k) -> float            the survivor's term of the depth sum
template <class SAMPLE, class MASK, class ALPHA, class SHADE, class DEPTH>
struct K4WalkParts { int n_steps; SAMPLE sample; MASK mask; ALPHA alpha; SHADE shade; DEPTH depth; };
template <class SAMPLE, class MASK, class ALPHA, class SHADE, class DEPTH>
__device__ __forceinline__ K4WalkParts<SAMPLE, MASK, ALPHA, SHADE, DEPTH> k4w_parts(int n_steps, SAMPLE sample, MASK mask, ALPHA alpha, SHADE shade, DEPTH depth) {
    return {n_steps, sample, mask, alpha, shade, depth};
}

// T, sum[0..2] = sum w rgb and sum[3] = sum w depth(k) (valid in lane 0), cnt = {pre, mask-pass, alpha-pass, shaded} (wave-uniform; zero unless
// counting), last = the last kept step or -1 (all lanes; TRACK_LAST only)
struct K4WalkOut { float T; float sum[4]; unsigned long long cnt[4]; int last; };

// the survivor queue (step, weight) of the block's one wave; a kernel that walks twice (k_march_bivox) puts a barrier between its walks
__shared__ int k4w_qk[128];
__shared__ float k4w_qw[128];

// One pass of one ray by one wave, lanes = 64 consecutive steps, in depth order:
//   filters   pre (sample) -> mask -> alpha > thres -> the exact sequential transmittance product of k_alpha2weight over the alpha-passing samples
//             incl. the T < 1e-3 stop -> weight > thres.  thres == 0 skips both `>` filters: every in-mask sample in front of the stop is shaded
//   shading   survivors are queued in LDS (k4w_qk / k4w_qw) and shaded 64 at a time, lane = survivor, in queue order: the order in which a
//             lane's fmaf(w, rgb, acc) terms arrive is the order of the result's bits
//   sums      wave reduction in a fixed lane order
// COUNT: the kernel can count samples (`count` asks for it); counting walks the whole ray.  TRACK_LAST: also return the last kept step -- without a
// threshold the in-mask samples behind the stop are kept too (lib/dbvgo.py:273,283), so then the walk goes on to the ray's end as well.
template <bool COUNT, bool TRACK_LAST, class PARTS>
__device__ __forceinline__ K4WalkOut k4w_walk(const PARTS& M, int lane, float thres, bool count) {
    int* const qk = k4w_qk;
    float* const qw = k4w_qw;
    const uint64_t below = lane ? (~0ull >> (64 - lane)) : 0ull;
    const bool filt = thres > 0.f;
    if (!COUNT) count = false;
    float T = 1.f;
    bool stopped = false;
    int nq = 0, my_last = -1;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    unsigned long long c_pre = 0, c_mask = 0, c_alpha = 0, c_shade = 0;
    // (where the compiler does not inline this at both of its calls, what it captures lives in scratch: values, and one reference)
    auto shade_queue = [&acc, lane, shade = M.shade, depth = M.depth](int n) {
        if (lane < n) {
            const int k = k4w_qk[lane];
            const float wk = k4w_qw[lane];
            float rgb[3];
            shade(k, rgb);
            acc[0] = fmaf(wk, rgb[0], acc[0]);
            acc[1] = fmaf(wk, rgb[1], acc[1]);
            acc[2] = fmaf(wk, rgb[2], acc[2]);
            acc[3] = fmaf(wk, depth(k), acc[3]);
        }
    };
    for (int base = 0; base < M.n_steps; base += 64) {
        if (stopped && !count && !(TRACK_LAST && !filt)) break;          // nothing behind the stop is needed
        const int k = base + lane;
        float p[3];
        const bool pre = M.sample(k, k < M.n_steps, p);
        bool keep = pre;
        if (keep) keep = M.mask(p);
        float alpha = 0.f;
        if (keep && (!stopped || count)) alpha = M.alpha(p);
        const bool apass = keep && (filt ? alpha > thres : true);
        // transmittance: the exact sequential product of k_alpha2weight over the alpha-passing samples in step order
        float myw = 0.f;
        bool hit = false;                                                // this lane's sample entered the product
        uint64_t bm = __ballot(apass);
        while (bm && !stopped) {
            const int l = __builtin_ctzll(bm);
            const float al = k4_readlane(alpha, l);
            if (lane == l) { myw = T * al; hit = true; }
            T = fmaf(-T, al, T);
            bm &= bm - 1;
            if (T < 1e-3f) stopped = true;
        }
        // the weight rule: the sample entered the product and, with a threshold, its weight passes (behind the stop w = 0 adds nothing: not queued)
        const bool wpass = hit && (filt ? myw > thres : true);
        const uint64_t sm = __ballot(wpass);
        const int ns = __popcll(sm);
        if (count) {
            c_pre += __popcll(__ballot(pre));
            c_mask += __popcll(__ballot(keep));
            c_alpha += __popcll(__ballot(apass));
            c_shade += ns;
        }
        if (TRACK_LAST && (filt ? wpass : keep)) my_last = k;
        if (wpass) {
            const int slot = nq + __popcll(sm & below);
            qk[slot] = k;
            qw[slot] = myw;
        }
        nq += ns;
        __syncthreads();
        if (nq >= 64) {
            shade_queue(64);
            __syncthreads();
            int rest = nq - 64, mk = 0; float mw = 0.f;
            if (lane < rest) { mk = qk[64 + lane]; mw = qw[64 + lane]; }
            __syncthreads();
            if (lane < rest) { qk[lane] = mk; qw[lane] = mw; }
            __syncthreads();
            nq = rest;
        }
    }
    shade_queue(nq);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[c] += __shfl_down(acc[c], off);
        if (TRACK_LAST) my_last = max(my_last, __shfl_xor(my_last, off));
    }
    if (!filt) c_shade = c_alpha;                                        // no weight filter: every alpha sample is shaded (w = 0 behind the stop)
    return K4WalkOut{T, {acc[0], acc[1], acc[2], acc[3]}, {c_pre, c_mask, c_alpha, c_shade}, my_last};
}
