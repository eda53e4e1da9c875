// Vector-quantised colour features (VQGrid, lib/grid.py:38-103 of the reference) on gfx950: the two-layer projection with its backward, the prepared
// codebook, the nearest-codeword search, and the exponential-moving-average codebook update.
//
// The reference evaluates a lookup as two Linear layers, an [n][n_embed] distance matrix, a max over it, a one-hot matrix of the same size and two
// matrix products with that one-hot.  Here a point's projected vector stays in registers while the codebook streams past it from LDS, and nothing of
// size n x n_embed exists.  Every result is a function of the inputs alone: fp32 FMA chains in a fixed order, fixed-size slabs of points summed
// in slab order, no floating-point atomics (no atomics at all).
//
//   dist(i, e) = (|v_i|^2 - (2 v_i) . E_e) + |E_e|^2          lib/grid.py:68-72, in that association; the smallest wins, the lowest index on a tie
#include "k4_vq.h"
#include <algorithm>

#define VQ_T 256                   // threads of the per-point kernels: thread = point
#define VQ_CHUNK_BYTES (48 * 1024) // LDS a chunk of the prepared codebook may take
#define VQ_SLAB 2048               // points of one partial sum (weight gradients, per-code sums): fixed, so the summation order is too

static inline int vq_stride(int dim) { return (dim + 1 + 3) / 4 * 4; }           // floats of a prepared row: the codeword, |e|^2, padding to 16 bytes
static inline int vq_chunk(int dim) { return VQ_CHUNK_BYTES / (vq_stride(dim) * 4); }

// ---------------------------------------------------------------- projection forward: h = relu(W1 x + b1), v = W2 h + b2
// thread = point; the tile's inputs transposed in LDS (lane = point: conflict-free), weights read with wave-uniform indices (scalar loads).
__global__ __launch_bounds__(VQ_T) void k_vq_project_fwd(const float* __restrict__ x, int64_t n, int in_dim, int dim, const float* __restrict__ w1g,
                                                         const float* __restrict__ b1g, const float* __restrict__ w2g, const float* __restrict__ b2g,
                                                         float* __restrict__ h_out, float* __restrict__ v_out) {
    __shared__ float xs[VQ_MAXIN * VQ_T];
    const int64_t base = (int64_t)blockIdx.x * VQ_T;
    const int cnt = (int)min((int64_t)VQ_T, n - base);
    for (int t = threadIdx.x; t < cnt * in_dim; t += VQ_T) {
        const int p = t / in_dim, k = t - p * in_dim;
        xs[k * VQ_T + p] = x[base * in_dim + t];
    }
    __syncthreads();
    if ((int)threadIdx.x >= cnt) return;
    const k4_cptr w1 = k4_const(w1g), b1 = k4_const(b1g), w2 = k4_const(w2g), b2 = k4_const(b2g);
    float h[VQ_MAXD], v[VQ_MAXD];
    vq_project_point<VQ_MAXD>([&](int k) { return xs[k * VQ_T + threadIdx.x]; }, in_dim, dim, w1, b1, w2, b2, h, v);
    const int64_t i = base + threadIdx.x;
#pragma unroll
    for (int j = 0; j < VQ_MAXD; ++j)
        if (j < dim) {
            if (h_out) h_out[i * dim + j] = h[j];
            v_out[i * dim + j] = v[j];
        }
}

// ---------------------------------------------------------------- projection backward
// gh = (W2^T gv) gated by h > 0, and gx = W1^T gh when wanted; the weight gradients are outer-product sums over the points (below).
__global__ __launch_bounds__(VQ_T) void k_vq_project_bwd(const float* __restrict__ gv, const float* __restrict__ h, int64_t n, int in_dim, int dim,
                                                         const float* __restrict__ w1g, const float* __restrict__ w2g, float* __restrict__ gh_out,
                                                         float* __restrict__ gx) {
    const int64_t i = (int64_t)blockIdx.x * VQ_T + threadIdx.x;
    if (i >= n) return;
    const k4_cptr w1 = k4_const(w1g), w2 = k4_const(w2g);
    float g[VQ_MAXD], gh[VQ_MAXD];
#pragma unroll
    for (int j = 0; j < VQ_MAXD; ++j) { g[j] = j < dim ? gv[i * dim + j] : 0.f; gh[j] = 0.f; }
#pragma unroll
    for (int j = 0; j < VQ_MAXD; ++j) {
        if (j < dim) {
#pragma unroll
            for (int k = 0; k < VQ_MAXD; ++k)
                if (k < dim) gh[k] = fmaf(g[j], w2[j * dim + k], gh[k]);
        }
    }
#pragma unroll
    for (int k = 0; k < VQ_MAXD; ++k)
        if (k < dim) {
            gh[k] = h[i * dim + k] > 0.f ? gh[k] : 0.f;
            gh_out[i * dim + k] = gh[k];
        }
    if (gx) {
        for (int m = 0; m < in_dim; ++m) {
            float a = 0.f;
#pragma unroll
            for (int k = 0; k < VQ_MAXD; ++k)
                if (k < dim) a = fmaf(gh[k], w1[k * in_dim + m], a);
            gx[i * in_dim + m] = a;
        }
    }
}

// part[slab][a][b] = sum over the slab's points, in point order, of A[i][a] * (b < db ? B[i][b] : 1): a layer's weight gradient (b < db) and bias
// gradient (b == db) of one slab.  thread = one (a, b); a wave reads consecutive b.
__global__ __launch_bounds__(256) void k_vq_outer_partial(const float* __restrict__ A, int da, const float* __restrict__ B, int db, int64_t n,
                                                          float* __restrict__ part) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= da * (db + 1)) return;
    const int a = t / (db + 1), b = t - a * (db + 1);
    const int64_t i0 = (int64_t)blockIdx.y * VQ_SLAB, i1 = min(n, i0 + VQ_SLAB);
    float acc = 0.f;
    if (b < db) for (int64_t i = i0; i < i1; ++i) acc = fmaf(A[i * da + a], B[i * db + b], acc);
    else for (int64_t i = i0; i < i1; ++i) acc += A[i * da + a];
    part[((int64_t)blockIdx.y * da + a) * (db + 1) + b] = acc;
}
// gw[a][b], gb[a] = the slabs' partial sums added in slab order
__global__ __launch_bounds__(256) void k_vq_outer_reduce(const float* __restrict__ part, int n_slab, int da, int db, float* __restrict__ gw, float* __restrict__ gb) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= da * (db + 1)) return;
    const int a = t / (db + 1), b = t - a * (db + 1);
    float acc = 0.f;
    for (int s = 0; s < n_slab; ++s) acc += part[(int64_t)s * da * (db + 1) + t];
    if (b < db) gw[a * db + b] = acc; else gb[a] = acc;
}

// ---------------------------------------------------------------- prepared codebook: row e = [E[0..dim)[e], |E_e|^2, 0...]
__global__ __launch_bounds__(256) void k_vq_pack(const float* __restrict__ embed, int dim, int n_embed, int S, float* __restrict__ pack) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n_embed) return;
    float e2 = 0.f;
    for (int k = 0; k < dim; ++k) {
        const float c = embed[(int64_t)k * n_embed + e];
        pack[(int64_t)e * S + k] = c;
        e2 = __fadd_rn(e2, __fmul_rn(c, c));                 // embed.pow(2).sum(0): the squares rounded, added over the channels in order
    }
    pack[(int64_t)e * S + dim] = e2;
    for (int k = dim + 1; k < S; ++k) pack[(int64_t)e * S + k] = 0.f;
}

// ---------------------------------------------------------------- assignment: thread = point, the codebook walked in LDS chunks
// A workgroup stages `chunk` prepared rows at a time; every lane reads the same row (LDS broadcast).  The running best is replaced only by a
// strictly smaller distance and codes are visited in index order, so the lowest index wins a tie, within a chunk and across chunks.
__global__ __launch_bounds__(VQ_T) void k_vq_assign(const float* __restrict__ v_in, int64_t n, int dim, const float* __restrict__ pack, int n_embed, int S,
                                                    int chunk, int64_t* __restrict__ ind, float* __restrict__ quant, double* __restrict__ diff_part) {
    extern __shared__ __attribute__((aligned(16))) float cb[];
    __shared__ double red[VQ_T / 64];
    const int64_t i = (int64_t)blockIdx.x * VQ_T + threadIdx.x;
    const bool live = i < n;
    float v[VQ_MAXD];
#pragma unroll
    for (int j = 0; j < VQ_MAXD; ++j) v[j] = (live && j < dim) ? v_in[i * dim + j] : 0.f;
    const float v2 = vq_norm2(v, dim);
    float best = 0.f;
    int best_e = -1;
    for (int e0 = 0; e0 < n_embed; e0 += chunk) {
        const int ne = min(chunk, n_embed - e0);
        __syncthreads();                                      // the previous chunk has been read by every wave
        for (int t = threadIdx.x; t < ne * S; t += VQ_T) cb[t] = pack[(int64_t)e0 * S + t];
        __syncthreads();
        vq_scan_rows<VQ_MAXD>((const float*)cb, ne, e0, S, dim, v, v2, best, best_e);
    }
    double sq = 0.0;
    if (live) {
        ind[i] = best_e;
        const float* const row = pack + (int64_t)best_e * S;
#pragma unroll
        for (int j = 0; j < VQ_MAXD; ++j)
            if (j < dim) {
                const float r = __fsub_rn(row[j], v[j]);      // quantize - vq_input
                quant[i * dim + j] = __fadd_rn(v[j], r);      // vq_input + (quantize - vq_input), lib/grid.py:96: not the codeword itself
                sq += (double)__fmul_rn(r, r);
            }
    }
    // diff: the workgroup's sum of squares in fp64, lanes then waves in a fixed order
    for (int o = 32; o > 0; o >>= 1) sq += __shfl_down(sq, o);
    if (k4_lane() == 0) red[threadIdx.x >> 6] = sq;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int w = 0; w < VQ_T / 64; ++w) s += red[w];
        diff_part[blockIdx.x] = s;
    }
}
// diff = mean((e - v)^2): the workgroups' sums added in workgroup order, fp64, rounded once
__global__ void k_vq_diff(const double* __restrict__ part, int n_part, double count, float* __restrict__ diff) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double s = 0.0;
    for (int p = 0; p < n_part; ++p) s += part[p];
    *diff = (float)(s / count);                               // 0 / 0 = NaN for an empty input, as torch's mean of nothing
}

// ---------------------------------------------------------------- per-code counts and sums of v (training mode)
// wave = (code, slab of points): lanes stride through the slab in point order and keep fp64 sums of the points assigned to the code; the 64 lanes'
// sums are then added in a fixed butterfly.  stat[slab][code][0] = count, [1 + j] = sum of v[.][j].
__global__ __launch_bounds__(64) void k_vq_code_sums(const int64_t* __restrict__ ind, const float* __restrict__ v, int64_t n, int dim, int n_embed,
                                                     double* __restrict__ stat) {
    const int e = blockIdx.x, lane = threadIdx.x;
    const int64_t i0 = (int64_t)blockIdx.y * VQ_SLAB, i1 = min(n, i0 + VQ_SLAB);
    double acc[VQ_MAXD], cnt = 0.0;
#pragma unroll
    for (int j = 0; j < VQ_MAXD; ++j) acc[j] = 0.0;
    for (int64_t i = i0 + lane; i < i1; i += 64) {
        if (ind[i] != e) continue;
        cnt += 1.0;
#pragma unroll
        for (int j = 0; j < VQ_MAXD; ++j)
            if (j < dim) acc[j] += (double)v[i * dim + j];
    }
    double* const out = stat + ((int64_t)blockIdx.y * n_embed + e) * (dim + 1);
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_down(cnt, o);
    if (lane == 0) out[0] = cnt;
#pragma unroll
    for (int j = 0; j < VQ_MAXD; ++j)
        if (j < dim) {
            double a = acc[j];
            for (int o = 32; o > 0; o >>= 1) a += __shfl_down(a, o);
            if (lane == 0) out[1 + j] = a;
        }
}

// ---------------------------------------------------------------- codebook update (lib/grid.py:80-93)
// cluster_size = cluster_size * decay + (1 - decay) * count;  embed_avg = embed_avg * decay + (1 - decay) * sum    (mul_, then add_ with alpha)
__global__ __launch_bounds__(256) void k_vq_ema(const double* __restrict__ stat, int n_slab, int dim, int n_embed, float decay, float one_minus,
                                                float* __restrict__ cluster_size, float* __restrict__ embed_avg) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n_embed * (dim + 1)) return;
    const int e = t / (dim + 1), c = t - e * (dim + 1);
    double s = 0.0;
    for (int k = 0; k < n_slab; ++k) s += stat[((int64_t)k * n_embed + e) * (dim + 1) + c];
    float* const dst = c == 0 ? cluster_size + e : embed_avg + (int64_t)(c - 1) * n_embed + e;
    *dst = fmaf((float)s, one_minus, __fmul_rn(*dst, decay));
}
// n = cluster_size.sum();  embed = embed_avg / ((cluster_size + eps) / (n + n_embed * eps) * n)
__global__ __launch_bounds__(256) void k_vq_normalize(const float* __restrict__ cluster_size, const float* __restrict__ embed_avg, int dim, int n_embed,
                                                      float eps, float n_eps, float* __restrict__ embed) {
    __shared__ double red[256];
    double s = 0.0;
    for (int e = threadIdx.x; e < n_embed; e += 256) s += (double)cluster_size[e];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    const float nsum = (float)red[0];
    const float den = __fadd_rn(nsum, n_eps);
    const int64_t total = (int64_t)dim * n_embed;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
        const int e = (int)(t % n_embed);
        const float cs = __fmul_rn(__fdiv_rn(__fadd_rn(cluster_size[e], eps), den), nsum);
        embed[t] = __fdiv_rn(embed_avg[t], cs);
    }
}

// ---------------------------------------------------------------- entry points
static bool vq_shape_ok(int in_dim, int dim) { return in_dim >= 1 && in_dim <= VQ_MAXIN && dim >= 1 && dim <= VQ_MAXD; }
static inline int64_t vq_slabs(int64_t n) { return n > 0 ? (n + VQ_SLAB - 1) / VQ_SLAB : 1; }

extern "C" int k4_vq_project_fwd(const float* x, int64_t n_pts, int32_t in_dim, int32_t dim, const float* w1, const float* b1, const float* w2, const float* b2,
                                 float* h, float* v, void* stream) {
    if (n_pts < 0 || !vq_shape_ok(in_dim, dim)) return K4_ERR_BAD_ARG;
    if (n_pts == 0) return K4_OK;
    if (!x || !w1 || !b1 || !w2 || !b2 || !v) return K4_ERR_BAD_ARG;
    const int64_t nb = (n_pts + VQ_T - 1) / VQ_T;
    if (nb > 0x7fffffffLL) return K4_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(k_vq_project_fwd, dim3((unsigned)nb), dim3(VQ_T), 0, (hipStream_t)stream, x, n_pts, in_dim, dim, w1, b1, w2, b2, h, v);
    return k4_check_launch();
}

extern "C" int64_t k4_vq_project_bwd_workspace_bytes(int64_t n_pts, int32_t in_dim, int32_t dim) {
    if (n_pts < 0 || !vq_shape_ok(in_dim, dim)) return -1;
    return 4 * (n_pts * dim + vq_slabs(n_pts) * ((int64_t)dim * (in_dim + 1) + (int64_t)dim * (dim + 1)));
}

extern "C" int k4_vq_project_bwd(const float* x, const float* h, const float* grad_v, int64_t n_pts, int32_t in_dim, int32_t dim, const float* w1, const float* w2,
                                 float* grad_x, float* gw1, float* gb1, float* gw2, float* gb2, float* workspace, int64_t workspace_bytes, void* stream) {
    if (n_pts < 0 || !vq_shape_ok(in_dim, dim) || !gw1 || !gb1 || !gw2 || !gb2) return K4_ERR_BAD_ARG;
    if (workspace_bytes < k4_vq_project_bwd_workspace_bytes(n_pts, in_dim, dim) || !workspace) return K4_ERR_BAD_ARG;
    if (n_pts > 0 && (!x || !h || !grad_v || !w1 || !w2)) return K4_ERR_BAD_ARG;
    const int64_t nb = (n_pts + VQ_T - 1) / VQ_T;
    if (nb > 0x7fffffffLL || vq_slabs(n_pts) > 65535) return K4_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    float* const gh = workspace;
    float* const p1 = gh + n_pts * dim;                                   // [slab][dim][in_dim + 1]
    float* const p2 = p1 + vq_slabs(n_pts) * dim * (in_dim + 1);          // [slab][dim][dim + 1]
    const int ns = (int)vq_slabs(n_pts);
    if (n_pts > 0) {
        hipLaunchKernelGGL(k_vq_project_bwd, dim3((unsigned)nb), dim3(VQ_T), 0, st, grad_v, h, n_pts, in_dim, dim, w1, w2, gh, grad_x);
    }
    const int t1 = dim * (in_dim + 1), t2 = dim * (dim + 1);
    // (n_pts == 0: one slab without points, its sums are zeros)
    hipLaunchKernelGGL(k_vq_outer_partial, dim3((t1 + 255) / 256, ns), dim3(256), 0, st, gh, dim, x, in_dim, n_pts, p1);
    hipLaunchKernelGGL(k_vq_outer_partial, dim3((t2 + 255) / 256, ns), dim3(256), 0, st, grad_v, dim, h, dim, n_pts, p2);
    hipLaunchKernelGGL(k_vq_outer_reduce, dim3((t1 + 255) / 256), dim3(256), 0, st, p1, ns, dim, in_dim, gw1, gb1);
    hipLaunchKernelGGL(k_vq_outer_reduce, dim3((t2 + 255) / 256), dim3(256), 0, st, p2, ns, dim, dim, gw2, gb2);
    return k4_check_launch();
}

extern "C" int64_t k4_vq_codebook_floats(int32_t dim, int32_t n_embed) {
    if (dim < 1 || dim > VQ_MAXD || n_embed < 1) return -1;
    return (int64_t)n_embed * vq_stride(dim);
}
extern "C" int32_t k4_vq_chunk_codes(int32_t dim) { return (dim < 1 || dim > VQ_MAXD) ? -1 : vq_chunk(dim); }

extern "C" int k4_vq_prepare_codebook(const float* embed, int32_t dim, int32_t n_embed, float* prepared, void* stream) {
    if (!embed || !prepared || dim < 1 || dim > VQ_MAXD || n_embed < 1) return K4_ERR_BAD_ARG;
    hipLaunchKernelGGL(k_vq_pack, dim3((n_embed + 255) / 256), dim3(256), 0, (hipStream_t)stream, embed, dim, n_embed, vq_stride(dim), prepared);
    return k4_check_launch();
}

extern "C" int64_t k4_vq_assign_workspace_bytes(int64_t n_pts, int32_t dim, int32_t n_embed, int32_t with_stats) {
    if (n_pts < 0 || dim < 1 || dim > VQ_MAXD || n_embed < 1) return -1;
    const int64_t nb = (n_pts + VQ_T - 1) / VQ_T;
    return 8 * (nb + 1) + (with_stats ? 8 * vq_slabs(n_pts) * n_embed * (dim + 1) : 0);
}

extern "C" int k4_vq_assign(const float* v, int64_t n_pts, int32_t dim, const float* prepared, int32_t n_embed, int64_t* ind, float* quantize, float* diff,
                            int32_t with_stats, void* workspace, int64_t workspace_bytes, void* stream) {
    if (n_pts < 0 || dim < 1 || dim > VQ_MAXD || n_embed < 1 || !prepared || !diff || !workspace) return K4_ERR_BAD_ARG;
    if (workspace_bytes < k4_vq_assign_workspace_bytes(n_pts, dim, n_embed, with_stats)) return K4_ERR_BAD_ARG;
    if (n_pts > 0 && (!v || !ind || !quantize)) return K4_ERR_BAD_ARG;
    const int64_t nb = (n_pts + VQ_T - 1) / VQ_T;
    if (nb > 0x7fffffffLL || vq_slabs(n_pts) > 65535) return K4_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    double* const part = (double*)workspace;
    const int S = vq_stride(dim), chunk = std::min(vq_chunk(dim), (int)n_embed);
    if (n_pts > 0)
        hipLaunchKernelGGL(k_vq_assign, dim3((unsigned)nb), dim3(VQ_T), (size_t)chunk * S * 4, st, v, n_pts, dim, prepared, n_embed, S, chunk, ind, quantize, part);
    hipLaunchKernelGGL(k_vq_diff, dim3(1), dim3(64), 0, st, part, (int)nb, (double)n_pts * (double)dim, diff);
    if (with_stats)
        hipLaunchKernelGGL(k_vq_code_sums, dim3((unsigned)n_embed, (unsigned)vq_slabs(n_pts)), dim3(64), 0, st, ind, v, n_pts, dim, n_embed, part + nb + 1);
    return k4_check_launch();
}

extern "C" int k4_vq_update_codebook(const void* workspace, int64_t n_pts, int32_t dim, int32_t n_embed, float decay, float one_minus_decay, float eps,
                                     float n_embed_eps, float* cluster_size, float* embed_avg, float* embed, void* stream) {
    if (n_pts < 0 || dim < 1 || dim > VQ_MAXD || n_embed < 1 || !workspace || !cluster_size || !embed_avg || !embed) return K4_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    const int64_t nb = (n_pts + VQ_T - 1) / VQ_T;
    const double* const stat = (const double*)workspace + nb + 1;
    const int64_t t = (int64_t)n_embed * (dim + 1);
    if ((t + 255) / 256 > 0x7fffffffLL) return K4_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(k_vq_ema, dim3((unsigned)((t + 255) / 256)), dim3(256), 0, st, stat, (int)vq_slabs(n_pts), dim, n_embed, decay, one_minus_decay, cluster_size, embed_avg);
    const int64_t blocks = std::min<int64_t>(((int64_t)dim * n_embed + 255) / 256, 1024);
    hipLaunchKernelGGL(k_vq_normalize, dim3((unsigned)blocks), dim3(256), 0, st, cluster_size, embed_avg, dim, n_embed, eps, n_embed_eps, embed);
    return k4_check_launch();
}
