// Vector-matrix factored grids (TensoRFGrid, lib/grid.py:157-268 of the reference) on gfx950: lookup, its backward, dense expansion, total variation.
//
// The reference evaluates a lookup as six F.grid_sample calls, three elementwise products, a cat and a mm, with [n][3R] intermediates in memory.
// Here a point's six interpolated values live in registers, forward and backward (the backward recomputes them from the point).  The factors are
// read in CHECKPOINT layout ([R][A][B]): under training they change every iteration, so a component-last repack would be paid per call, and
// the factors of a 160^3 scene at rank 48 are a few MB -- they stay in L2.
#include "k4_common.h"

#define K4T_THREADS 256
#define K4T_BWD_THREADS 512
#define K4T_MAX_FVEC 8192                    // floats of the fvec gradient's workgroup sums (LDS)
#define K4T_MAX_LDS (144 * 1024)

struct K4TFactors {
    const float *xy, *xz, *yz, *xv, *yv, *zv, *fvec;
    int C, R, Rxy, X, Y, Z;
};

// One axis of F.grid_sample(bilinear, align_corners=True, zero padding), coordinate arithmetic of k4s_grid_corners (k4_staged.hip): the two
// node indices (0 where the node is outside: its weight is 0 then) and weights.
struct K4TAxis { int i0, i1; float w0, w1; };
__device__ __forceinline__ K4TAxis k4t_axis(float p, float lo, float hi, int size, bool valid) {
    const float u = k4_unnorm(k4_norm_coord(p, lo, hi), size);
    const float f = floorf(u);
    const int a = (int)f;
    const bool ok0 = valid && (unsigned)a < (unsigned)size, ok1 = valid && (unsigned)(a + 1) < (unsigned)size;
    K4TAxis r;
    r.i0 = ok0 ? a : 0; r.i1 = ok1 ? a + 1 : 0;
    r.w0 = ok0 ? (f + 1.f) - u : 0.f; r.w1 = ok1 ? u - f : 0.f;
    return r;
}
__device__ __forceinline__ float k4t_plane(const float* __restrict__ p, int B, const K4TAxis& a, const K4TAxis& b) {
    return (a.w0 * b.w0) * p[(size_t)a.i0 * B + b.i0] + (a.w0 * b.w1) * p[(size_t)a.i0 * B + b.i1] +
           (a.w1 * b.w0) * p[(size_t)a.i1 * B + b.i0] + (a.w1 * b.w1) * p[(size_t)a.i1 * B + b.i1];
}
__device__ __forceinline__ float k4t_vec(const float* __restrict__ v, const K4TAxis& a) { return a.w0 * v[a.i0] + a.w1 * v[a.i1]; }

// ---------------------------------------------------------------- forward: one thread per point
template <int MAXC>
__global__ __launch_bounds__(K4T_THREADS) void k_tensorf_sample(K4TFactors F, const float* __restrict__ xyz, const float* __restrict__ mn,
                                                                const float* __restrict__ mx, int64_t n, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const K4TAxis ax = k4t_axis(xyz[i * 3 + 0], mn[0], mx[0], F.X, true);
    const K4TAxis ay = k4t_axis(xyz[i * 3 + 1], mn[1], mx[1], F.Y, true);
    const K4TAxis az = k4t_axis(xyz[i * 3 + 2], mn[2], mx[2], F.Z, true);
    float acc[MAXC];
#pragma unroll
    for (int c = 0; c < MAXC; ++c) acc[c] = 0.f;
    const size_t sxy = (size_t)F.X * F.Y, sxz = (size_t)F.X * F.Z, syz = (size_t)F.Y * F.Z;
    const int C = F.C;
    // group g: 0 = xy plane * z vector (Rxy components), 1 = xz * y, 2 = yz * x; fvec rows in that order
    for (int g = 0; g < 3; ++g) {
        const int nr = g == 0 ? F.Rxy : F.R;
        const int row0 = g == 0 ? 0 : g == 1 ? F.Rxy : F.Rxy + F.R;
        float part = 0.f;
        for (int r = 0; r < nr; ++r) {
            float feat;
            if (g == 0) feat = k4t_plane(F.xy + sxy * r, F.Y, ax, ay) * k4t_vec(F.zv + (size_t)F.Z * r, az);
            else if (g == 1) feat = k4t_plane(F.xz + sxz * r, F.Z, ax, az) * k4t_vec(F.yv + (size_t)F.Y * r, ay);
            else feat = k4t_plane(F.yz + syz * r, F.Z, ay, az) * k4t_vec(F.xv + (size_t)F.X * r, ax);
            if (MAXC == 1) part += feat;
            else {
                const float* __restrict__ f = F.fvec + (size_t)(row0 + r) * C;
#pragma unroll
                for (int c = 0; c < MAXC; ++c)
                    if (c < C) acc[c] = fmaf(feat, f[c], acc[c]);
            }
        }
        if (MAXC == 1) acc[0] += part;
    }
#pragma unroll
    for (int c = 0; c < MAXC; ++c)
        if (c < C) out[i * C + c] = acc[c];
}

// ---------------------------------------------------------------- backward
// A persistent grid of workgroups; each takes tiles of K4T_BWD_THREADS consecutive points, one thread per point.  Per component the thread
// recomputes the plane and vector values, derives g = sum_c grad_out[c] * fvec[row][c] (C == 1: grad_out) and adds
//   plane corners  += weight * g * vector value        (fp32 atomics straight into the gradient, checkpoint layout)
//   vector entries += weight * g * plane value         (VLDS: workgroup sums in LDS, flushed once when the workgroup is done; else atomics)
//   fvec[row][c]   += sum over the tile's points of feat * grad_out[c]: the products feat go through LDS, C x G threads each add a strided
//                     share of the tile's points and add their partial sum to the workgroup's [rows][C] sums in LDS (flushed at the end).
// LDS (dynamic): [nf * C] fvec sums | [T][C] grad_out of the tile | [T] feat | VLDS: zv, yv, xv sums.
template <int MAXC, bool VLDS>
__global__ __launch_bounds__(K4T_BWD_THREADS) void k_tensorf_sample_bwd(K4TFactors F, const float* __restrict__ gout, const float* __restrict__ xyz,
                                                                        const float* __restrict__ mn, const float* __restrict__ mx, int64_t n, int64_t n_tiles,
                                                                        float* __restrict__ g_xy, float* __restrict__ g_xz, float* __restrict__ g_yz,
                                                                        float* __restrict__ g_xv, float* __restrict__ g_yv, float* __restrict__ g_zv,
                                                                        float* __restrict__ g_fvec) {
    extern __shared__ float k4t_lds[];
    constexpr int T = K4T_BWD_THREADS;
    const int tid = (int)threadIdx.x;
    const int C = F.C;
    const int nf = F.Rxy + 2 * F.R;
    const int n_fv = MAXC > 1 ? nf * C : 0;
    float* const s_fv = k4t_lds;
    float* const s_go = s_fv + n_fv;
    float* const s_feat = s_go + (MAXC > 1 ? T * C : 0);
    float* const s_zv = s_feat + (MAXC > 1 ? T : 0);
    float* const s_yv = s_zv + (size_t)F.Rxy * F.Z;
    float* const s_xv = s_yv + (size_t)F.R * F.Y;
    const int n_vec = VLDS ? F.Rxy * F.Z + F.R * F.Y + F.R * F.X : 0;
    for (int j = tid; j < n_fv; j += T) s_fv[j] = 0.f;
    for (int j = tid; j < n_vec; j += T) s_zv[j] = 0.f;
    __syncthreads();
    const size_t sxy = (size_t)F.X * F.Y, sxz = (size_t)F.X * F.Z, syz = (size_t)F.Y * F.Z;
    // fvec reduction: thread -> (channel fc, group fg); fg strides over the tile's points
    const int G = MAXC > 1 ? T / C : 1;
    const int fc = tid % (MAXC > 1 ? C : 1), fg = tid / (MAXC > 1 ? C : 1);

    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t i = tile * T + tid;
        const bool valid = i < n;
        const int64_t ic = valid ? i : 0;
        const K4TAxis ax = k4t_axis(xyz[ic * 3 + 0], mn[0], mx[0], F.X, valid);
        const K4TAxis ay = k4t_axis(xyz[ic * 3 + 1], mn[1], mx[1], F.Y, valid);
        const K4TAxis az = k4t_axis(xyz[ic * 3 + 2], mn[2], mx[2], F.Z, valid);
        float go[MAXC];
#pragma unroll
        for (int c = 0; c < MAXC; ++c) go[c] = (valid && c < C) ? gout[ic * C + c] : 0.f;
        if (MAXC > 1) {
#pragma unroll
            for (int c = 0; c < MAXC; ++c)
                if (c < C) s_go[tid * C + c] = go[c];
        }
        for (int g = 0; g < 3; ++g) {
            const int nr = g == 0 ? F.Rxy : F.R;
            const int row0 = g == 0 ? 0 : g == 1 ? F.Rxy : F.Rxy + F.R;
            // plane axes (a, b) and the vector's axis v of this group
            const K4TAxis& pa = g == 2 ? ay : ax;
            const K4TAxis& pb = g == 0 ? ay : az;
            const K4TAxis& va = g == 0 ? az : g == 1 ? ay : ax;
            const int B = g == 0 ? F.Y : F.Z;
            const int V = g == 0 ? F.Z : g == 1 ? F.Y : F.X;
            const size_t sp = g == 0 ? sxy : g == 1 ? sxz : syz;
            const float* const plane = g == 0 ? F.xy : g == 1 ? F.xz : F.yz;
            const float* const vec = g == 0 ? F.zv : g == 1 ? F.yv : F.xv;
            float* const gplane = g == 0 ? g_xy : g == 1 ? g_xz : g_yz;
            float* const gvec = VLDS ? (g == 0 ? s_zv : g == 1 ? s_yv : s_xv) : (g == 0 ? g_zv : g == 1 ? g_yv : g_xv);
            const float w00 = pa.w0 * pb.w0, w01 = pa.w0 * pb.w1, w10 = pa.w1 * pb.w0, w11 = pa.w1 * pb.w1;
            const size_t o00 = (size_t)pa.i0 * B + pb.i0, o01 = (size_t)pa.i0 * B + pb.i1, o10 = (size_t)pa.i1 * B + pb.i0, o11 = (size_t)pa.i1 * B + pb.i1;
            for (int r = 0; r < nr; ++r) {
                const float pv = k4t_plane(plane + sp * r, B, pa, pb);
                const float vv = k4t_vec(vec + (size_t)V * r, va);
                float gr;
                if (MAXC == 1) gr = go[0];
                else {
                    const float* __restrict__ f = F.fvec + (size_t)(row0 + r) * C;
                    gr = 0.f;
#pragma unroll
                    for (int c = 0; c < MAXC; ++c)
                        if (c < C) gr = fmaf(go[c], f[c], gr);
                }
                const float gp = gr * vv, gv = gr * pv;
                float* const gpl = gplane + sp * r;
                if (w00 != 0.f) unsafeAtomicAdd(gpl + o00, w00 * gp);
                if (w01 != 0.f) unsafeAtomicAdd(gpl + o01, w01 * gp);
                if (w10 != 0.f) unsafeAtomicAdd(gpl + o10, w10 * gp);
                if (w11 != 0.f) unsafeAtomicAdd(gpl + o11, w11 * gp);
                float* const gvr = gvec + (size_t)V * r;
                if (VLDS) {
                    if (va.w0 != 0.f) k4_lds_add(gvr + va.i0, va.w0 * gv);
                    if (va.w1 != 0.f) k4_lds_add(gvr + va.i1, va.w1 * gv);
                } else {
                    if (va.w0 != 0.f) unsafeAtomicAdd(gvr + va.i0, va.w0 * gv);
                    if (va.w1 != 0.f) unsafeAtomicAdd(gvr + va.i1, va.w1 * gv);
                }
                if (MAXC > 1) {
                    s_feat[tid] = pv * vv;                     // (an invalid point: all weights 0 -> 0)
                    __syncthreads();
                    if (fg < G) {
                        float s = 0.f;
                        for (int p = fg; p < T; p += G) s = fmaf(s_feat[p], s_go[p * C + fc], s);
                        k4_lds_add(s_fv + (row0 + r) * C + fc, s);
                    }
                    __syncthreads();
                }
            }
        }
        if (MAXC > 1) __syncthreads();                         // s_go is rewritten by the next tile
    }
    __syncthreads();
    for (int j = tid; j < n_fv; j += T) {
        const float v = s_fv[j];
        if (v != 0.f) unsafeAtomicAdd(g_fvec + j, v);
    }
    if (VLDS) {
        const int nz = F.Rxy * F.Z, ny = F.R * F.Y, nx = F.R * F.X;
        for (int j = tid; j < nz; j += T) { const float v = s_zv[j]; if (v != 0.f) unsafeAtomicAdd(g_zv + j, v); }
        for (int j = tid; j < ny; j += T) { const float v = s_yv[j]; if (v != 0.f) unsafeAtomicAdd(g_yv + j, v); }
        for (int j = tid; j < nx; j += T) { const float v = s_xv[j]; if (v != 0.f) unsafeAtomicAdd(g_xv + j, v); }
    }
}

// ---------------------------------------------------------------- dense expansion: one thread per voxel, all channels
template <int MAXC>
__global__ __launch_bounds__(K4T_THREADS) void k_tensorf_dense(K4TFactors F, float* __restrict__ out) {
    const int64_t nvox = (int64_t)F.X * F.Y * F.Z;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nvox) return;
    const int z = (int)(t % F.Z), y = (int)((t / F.Z) % F.Y), x = (int)(t / ((int64_t)F.Z * F.Y));
    const size_t sxy = (size_t)F.X * F.Y, sxz = (size_t)F.X * F.Z, syz = (size_t)F.Y * F.Z;
    const int C = F.C;
    float acc[MAXC];
#pragma unroll
    for (int c = 0; c < MAXC; ++c) acc[c] = 0.f;
    for (int g = 0; g < 3; ++g) {
        const int nr = g == 0 ? F.Rxy : F.R;
        const int row0 = g == 0 ? 0 : g == 1 ? F.Rxy : F.Rxy + F.R;
        float part = 0.f;
        for (int r = 0; r < nr; ++r) {
            float feat;
            if (g == 0) feat = F.xy[sxy * r + (size_t)x * F.Y + y] * F.zv[(size_t)F.Z * r + z];
            else if (g == 1) feat = F.xz[sxz * r + (size_t)x * F.Z + z] * F.yv[(size_t)F.Y * r + y];
            else feat = F.yz[syz * r + (size_t)y * F.Z + z] * F.xv[(size_t)F.X * r + x];
            if (MAXC == 1) part += feat;
            else {
                const float* __restrict__ f = F.fvec + (size_t)(row0 + r) * C;
#pragma unroll
                for (int c = 0; c < MAXC; ++c)
                    if (c < C) acc[c] = fmaf(feat, f[c], acc[c]);
            }
        }
        if (MAXC == 1) acc[0] += part;
    }
#pragma unroll
    for (int c = 0; c < MAXC; ++c)
        if (c < C) out[(size_t)c * nvox + t] = acc[c];
}

// ---------------------------------------------------------------- total variation of one factor [R][A][B]
// d/dp of smooth_l1(d, beta = 1) summed: the derivative w.r.t. d is d for |d| < 1, else sign(d) -- a clamp to [-1, 1].
__device__ __forceinline__ float k4t_sl1(float d) { return fminf(fmaxf(d, -1.f), 1.f); }
__global__ __launch_bounds__(K4T_THREADS) void k_tensorf_tv(const float* __restrict__ p, float* __restrict__ grad, int64_t total, int A, int B, float wa, float wb) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const int b = (int)(t % B), a = (int)((t / B) % A);
    const float v = p[t];
    float s = 0.f;
    if (a > 0) s += wa * k4t_sl1(v - p[t - B]);
    if (a + 1 < A) s -= wa * k4t_sl1(p[t + B] - v);
    if (b > 0) s += wb * k4t_sl1(v - p[t - 1]);
    if (b + 1 < B) s -= wb * k4t_sl1(p[t + 1] - v);
    grad[t] += s / 6.f;
}

// ---------------------------------------------------------------- entry points
#define ST ((hipStream_t)stream)
#define REQ(c) do { if (!(c)) return K4_ERR_BAD_ARG; } while (0)
static inline unsigned k4t_blocks(int64_t n, int threads) { return (unsigned)((n + threads - 1) / threads); }

static int k4t_factors(K4TFactors& F, const float* xy, const float* xz, const float* yz, const float* xv, const float* yv, const float* zv, const float* fvec,
                       int32_t C, int32_t R, int32_t Rxy, int32_t X, int32_t Y, int32_t Z) {
    REQ(xy && xz && yz && xv && yv && zv && C > 0 && R > 0 && Rxy > 0 && X > 0 && Y > 0 && Z > 0 && (C == 1 || fvec));
    if (C > 32) return K4_ERR_UNSUPPORTED;
    F.xy = xy; F.xz = xz; F.yz = yz; F.xv = xv; F.yv = yv; F.zv = zv; F.fvec = fvec;
    F.C = C; F.R = R; F.Rxy = Rxy; F.X = X; F.Y = Y; F.Z = Z;
    return K4_OK;
}
// the instantiation for C channels: 1, 4, 12 or 32 accumulators
#define K4T_BY_C(C, CALL) do { if ((C) == 1) { CALL(1); } else if ((C) <= 4) { CALL(4); } else if ((C) <= 12) { CALL(12); } else { CALL(32); } } while (0)

extern "C" int k4_tensorf_sample(const float* xy, const float* xz, const float* yz, const float* xv, const float* yv, const float* zv, const float* fvec,
                                 int32_t C, int32_t R, int32_t Rxy, int32_t X, int32_t Y, int32_t Z,
                                 const float* xyz, const float* mn, const float* mx, int64_t n, float* out, void* stream) {
    K4TFactors F;
    const int rc = k4t_factors(F, xy, xz, yz, xv, yv, zv, fvec, C, R, Rxy, X, Y, Z);
    if (rc != K4_OK) return rc;
    REQ(mn && mx && n >= 0);
    if (n == 0) return K4_OK;
    REQ(xyz && out);
#define K4T_CALL(M) hipLaunchKernelGGL(k_tensorf_sample<M>, dim3(k4t_blocks(n, K4T_THREADS)), dim3(K4T_THREADS), 0, ST, F, xyz, mn, mx, n, out)
    K4T_BY_C(C, K4T_CALL);
#undef K4T_CALL
    return k4_check_launch();
}

template <int MAXC, bool VLDS>
static int k4t_launch_bwd(const K4TFactors& F, size_t lds, unsigned blocks, const float* go, const float* xyz, const float* mn, const float* mx, int64_t n, int64_t n_tiles,
                          float* g_xy, float* g_xz, float* g_yz, float* g_xv, float* g_yv, float* g_zv, float* g_fvec, void* stream) {
    // (raised once per kernel and device: to the largest size any later call can ask for)
    K4_ENSURE_DYN_LDS((k_tensorf_sample_bwd<MAXC, VLDS>), K4T_MAX_LDS);
    hipLaunchKernelGGL((k_tensorf_sample_bwd<MAXC, VLDS>), dim3(blocks), dim3(K4T_BWD_THREADS), lds, ST, F, go, xyz, mn, mx, n, n_tiles,
                       g_xy, g_xz, g_yz, g_xv, g_yv, g_zv, g_fvec);
    return k4_check_launch();
}

extern "C" int k4_tensorf_sample_backward(const float* grad_out, const float* xy, const float* xz, const float* yz, const float* xv, const float* yv,
                                          const float* zv, const float* fvec, int32_t C, int32_t R, int32_t Rxy, int32_t X, int32_t Y, int32_t Z,
                                          const float* xyz, const float* mn, const float* mx, int64_t n,
                                          float* g_xy, float* g_xz, float* g_yz, float* g_xv, float* g_yv, float* g_zv, float* g_fvec, void* stream) {
    K4TFactors F;
    const int rc = k4t_factors(F, xy, xz, yz, xv, yv, zv, fvec, C, R, Rxy, X, Y, Z);
    if (rc != K4_OK) return rc;
    REQ(mn && mx && n >= 0 && g_xy && g_xz && g_yz && g_xv && g_yv && g_zv && (C == 1 || g_fvec));
    if (n == 0) return K4_OK;
    REQ(xyz && grad_out);
    const int64_t n_fv = C > 1 ? (int64_t)(Rxy + 2 * R) * C : 0;
    if (n_fv > K4T_MAX_FVEC) return K4_ERR_UNSUPPORTED;
    const int64_t base = n_fv + (C > 1 ? (int64_t)K4T_BWD_THREADS * (C + 1) : 0);
    const int64_t n_vec = (int64_t)Rxy * Z + (int64_t)R * Y + (int64_t)R * X;
    const bool vlds = (base + n_vec) * 4 <= K4T_MAX_LDS;
    const size_t lds = (size_t)(base + (vlds ? n_vec : 0)) * 4;
    const int64_t n_tiles = (n + K4T_BWD_THREADS - 1) / K4T_BWD_THREADS;
    // persistent: the LDS sums are flushed once per workgroup.  The vector sums in LDS allow one workgroup per CU (two when they are small).
    const int64_t cap = (int64_t)k4_num_cus() * (lds > 64 * 1024 ? 1 : 2);
    const unsigned blocks = (unsigned)(n_tiles < cap ? n_tiles : cap);
#define K4T_CALL(M) return vlds ? k4t_launch_bwd<M, true>(F, lds, blocks, grad_out, xyz, mn, mx, n, n_tiles, g_xy, g_xz, g_yz, g_xv, g_yv, g_zv, g_fvec, stream) \
                                : k4t_launch_bwd<M, false>(F, lds, blocks, grad_out, xyz, mn, mx, n, n_tiles, g_xy, g_xz, g_yz, g_xv, g_yv, g_zv, g_fvec, stream)
    K4T_BY_C(C, K4T_CALL);
#undef K4T_CALL
    return K4_ERR_BAD_ARG;
}

extern "C" int k4_tensorf_dense(const float* xy, const float* xz, const float* yz, const float* xv, const float* yv, const float* zv, const float* fvec,
                                int32_t C, int32_t R, int32_t Rxy, int32_t X, int32_t Y, int32_t Z, float* out, void* stream) {
    K4TFactors F;
    const int rc = k4t_factors(F, xy, xz, yz, xv, yv, zv, fvec, C, R, Rxy, X, Y, Z);
    if (rc != K4_OK) return rc;
    REQ(out);
    const int64_t nvox = (int64_t)X * Y * Z;
#define K4T_CALL(M) hipLaunchKernelGGL(k_tensorf_dense<M>, dim3(k4t_blocks(nvox, K4T_THREADS)), dim3(K4T_THREADS), 0, ST, F, out)
    K4T_BY_C(C, K4T_CALL);
#undef K4T_CALL
    return k4_check_launch();
}

extern "C" int k4_tensorf_tv_add_grad(const float* param, float* grad, int32_t R, int32_t A, int32_t B, float wa, float wb, void* stream) {
    REQ(param && grad && R > 0 && A > 0 && B > 0);
    const int64_t total = (int64_t)R * A * B;
    hipLaunchKernelGGL(k_tensorf_tv, dim3(k4t_blocks(total, K4T_THREADS)), dim3(K4T_THREADS), 0, ST, param, grad, total, A, B, wa, wb);
    return k4_check_launch();
}
