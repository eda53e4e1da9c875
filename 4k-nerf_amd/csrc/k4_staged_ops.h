// Per-sample / per-pixel arithmetic of the staged kernels (k4_staged.hip) that other translation units must repeat BIT FOR BIT: the trilinear
// corner set of the grid lookup, the density activation and the ray of a pixel.  One expression tree each, inlined wherever it is used
// (k4_staged.hip, k4_prep.hip, k4_direct_train.hip): a decision taken on these values in one file is the decision the staged op sequence takes.
#pragma once
#include "k4_common.h"

// the cell and the eight weights of F.grid_sample(bilinear, align_corners=True) at a world position on an [X][Y][Z] grid spanning [mn, mx]
__device__ __forceinline__ K4Tri k4s_grid_tri(float x, float y, float z, const float* __restrict__ mn, const float* __restrict__ mx, int X, int Y, int Z) {
    const float nx = k4_norm_coord(x, mn[0], mx[0]);
    const float ny = k4_norm_coord(y, mn[1], mx[1]);
    const float nz = k4_norm_coord(z, mn[2], mx[2]);
    return k4_tri_setup(k4_unnorm(nx, X), k4_unnorm(ny, Y), k4_unnorm(nz, Z));
}
// corner indices / weights of F.grid_sample(bilinear, align_corners=True, zero padding) on an [X][Y][Z] grid
__device__ __forceinline__ void k4s_tri_corners(const K4Tri& t, int X, int Y, int Z, size_t (&idx)[8], float (&w)[8]) {
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const int xx = t.x0 + K4_CX(c), yy = t.y0 + K4_CY(c), zz = t.z0 + K4_CZ(c);
        const bool ok = (unsigned)xx < (unsigned)X && (unsigned)yy < (unsigned)Y && (unsigned)zz < (unsigned)Z;
        idx[c] = ok ? ((size_t)xx * Y + yy) * Z + zz : 0;
        w[c] = ok ? t.w[c] : 0.f;
    }
}
__device__ __forceinline__ void k4s_grid_corners(float x, float y, float z, const float* __restrict__ mn, const float* __restrict__ mx,
                                                 int X, int Y, int Z, size_t (&idx)[8], float (&w)[8]) {
    k4s_tri_corners(k4s_grid_tri(x, y, z, mn, mx, X, Y, Z), X, Y, Z, idx, w);
}
__device__ __forceinline__ void k4s_raw2alpha(float den, float shift, float iv, float& e, float& al) {
    e = expf(den + shift);
    al = (iv == 1.f) ? 1.f - 1.f / (1.f + e) : 1.f - powf(1.f + e, -iv);
}
// its backward (.cu:507-530): d alpha / d density times the incoming gradient, from the saved e = exp(density + shift).  A macro, so that
// k_raw2alpha_bwd (k4_staged.hip) keeps the expression it always had, token for token, and with it its code object.
#define K4S_RAW2ALPHA_BWD(e, iv, g) (fminf((e), 1e10f) * powf(1.f + (e), -(iv) - 1.f) * (iv) * (g))

// the out-of-box test, the mask cache and the blend of a lookup (moved here verbatim from k4_staged.hip)
__device__ __forceinline__ bool k4s_outbbox(const float (&p)[3], const float* __restrict__ mn, const float* __restrict__ mx) {
    return (mn[0] > p[0]) | (mn[1] > p[1]) | (mn[2] > p[2]) | (mx[0] < p[0]) | (mx[1] < p[1]) | (mx[2] < p[2]);
}
__device__ __forceinline__ uint8_t k4s_maskcache(const uint8_t* __restrict__ world, float x, float y, float z, const float* __restrict__ sc,
                                                 const float* __restrict__ sh, int si, int sj, int sk) {
    const int a = k4_round_half_away(fmaf(x, sc[0], sh[0]));
    const int b = k4_round_half_away(fmaf(y, sc[1], sh[1]));
    const int c = k4_round_half_away(fmaf(z, sc[2], sh[2]));
    uint8_t v = 0;
    if ((unsigned)a < (unsigned)si && (unsigned)b < (unsigned)sj && (unsigned)c < (unsigned)sk)
        v = world[((size_t)a * sj + b) * sk + c] != 0;
    return v;
}
__device__ __forceinline__ float k4s_grid_blend(const float* __restrict__ g, const size_t (&idx)[8], const float (&w)[8]) {
    float v = 0.f;
#pragma unroll
    for (int c = 0; c < 8; ++c) v += g[idx[c]] * w[c];
    return v;
}
// ray-AABB helpers (.cu:12-79; moved here verbatim from k4_staged.hip)
__device__ __forceinline__ void aabb_t(const float* o, const float* d, const float* mn, const float* mx,
                                        float near, float far, int64_t r, float& t_min, float& t_max) {
    const float vx = d[r * 3 + 0] == 0.f ? 1e-6f : d[r * 3 + 0];
    const float vy = d[r * 3 + 1] == 0.f ? 1e-6f : d[r * 3 + 1];
    const float vz = d[r * 3 + 2] == 0.f ? 1e-6f : d[r * 3 + 2];
    const float ax = (mx[0] - o[r * 3 + 0]) / vx, ay = (mx[1] - o[r * 3 + 1]) / vy, az = (mx[2] - o[r * 3 + 2]) / vz;
    const float bx = (mn[0] - o[r * 3 + 0]) / vx, by = (mn[1] - o[r * 3 + 1]) / vy, bz = (mn[2] - o[r * 3 + 2]) / vz;
    t_min = fmaxf(fminf(fmaxf(fmaxf(fminf(ax, bx), fminf(ay, by)), fminf(az, bz)), far), near);
    t_max = fmaxf(fminf(fminf(fminf(fmaxf(ax, bx), fmaxf(ay, by)), fmaxf(az, bz)), far), near);
}
__device__ __forceinline__ float ray_norm(const float* d, int64_t r) {
    return sqrtf(fmaf(d[r * 3 + 2], d[r * 3 + 2], fmaf(d[r * 3 + 1], d[r * 3 + 1], d[r * 3 + 0] * d[r * 3 + 0])));
}
__device__ __forceinline__ int64_t n_steps_of(float t_min, float t_max, float rnorm, float stepdist) {
    return (int64_t)fmaxf(ceilf((t_max - t_min) * rnorm / stepdist), 1.f);      // at least 1 point (.cu:53)
}

// get_rays_of_a_view (lib/dvgo.py:516-582) for ONE pixel: pixel -> camera direction -> world ray -> unit view direction (BEFORE the NDC
// warp) -> optional NDC warp (near = 1, focal = K[0][0]).  The arithmetic restates the reference's torch op sequence one rounding at a time
// (__fmul_rn/__fadd_rn/__fdiv_rn: no contraction).  K = [3][3] intrinsics, M = [3][4] camera-to-world (row stride 4), both wave-uniform.
__device__ __forceinline__ void k4s_ray_of_pixel(int row, int col, int H, int W, k4_cptr K, k4_cptr M, int ndc, int inverse_y, int flip_x, int flip_y,
                                                 float pix_off, float c_w, float c_h, float (&o)[3], float (&v)[3], float (&vd)[3]) {
    const float i = (float)(flip_x ? W - 1 - col : col) + pix_off;
    const float j = (float)(flip_y ? H - 1 - row : row) + pix_off;
    float d[3];
    d[0] = __fdiv_rn(__fsub_rn(i, K[2]), K[0]);
    d[1] = __fdiv_rn(__fsub_rn(j, K[5]), K[4]);
    d[2] = 1.f;
    if (!inverse_y) { d[1] = -d[1]; d[2] = -1.f; }
#pragma unroll
    for (int a = 0; a < 3; ++a) {                                // torch.sum(dirs[..., None, :] * c2w[:3,:3], -1)
        v[a] = __fadd_rn(__fadd_rn(__fmul_rn(d[0], M[a * 4 + 0]), __fmul_rn(d[1], M[a * 4 + 1])), __fmul_rn(d[2], M[a * 4 + 2]));
        o[a] = M[a * 4 + 3];
    }
    const float nrm = __fsqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(v[0], v[0]), __fmul_rn(v[1], v[1])), __fmul_rn(v[2], v[2])));
#pragma unroll
    for (int a = 0; a < 3; ++a) vd[a] = __fdiv_rn(v[a], nrm);
    if (ndc) {                                                   // ndc_rays, near = 1 (lib/dvgo.py:557-574)
        const float t = __fdiv_rn(-__fadd_rn(1.f, o[2]), v[2]);
#pragma unroll
        for (int a = 0; a < 3; ++a) o[a] = __fadd_rn(o[a], __fmul_rn(t, v[a]));
        const float o0 = __fdiv_rn(__fmul_rn(c_w, o[0]), o[2]);
        const float o1 = __fdiv_rn(__fmul_rn(c_h, o[1]), o[2]);
        const float o2 = __fadd_rn(1.f, __fdiv_rn(2.f, o[2]));
        const float d0 = __fmul_rn(c_w, __fsub_rn(__fdiv_rn(v[0], v[2]), __fdiv_rn(o[0], o[2])));
        const float d1 = __fmul_rn(c_h, __fsub_rn(__fdiv_rn(v[1], v[2]), __fdiv_rn(o[1], o[2])));
        const float d2 = __fdiv_rn(-2.f, o[2]);
        o[0] = o0; o[1] = o1; o[2] = o2; v[0] = d0; v[1] = d1; v[2] = d2;
    }
}
// -1./(W/(2.*focal)) as the reference evaluates it: Python double arithmetic, cast to fp32 by the tensor multiply
static inline float k4s_ndc_scale(int extent, float focal) { return (float)(-1.0 / ((double)extent / (2.0 * (double)focal))); }
