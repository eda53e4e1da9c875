// Per-point arithmetic of the vector-quantised features, shared by the kernels of k4_vq.hip and the one-launch marcher k_march_vq (k4_staged.hip): one
// expression tree each, so a codeword chosen by the marcher is the codeword the staged lookup chooses.
#pragma once
#include "k4_common.h"

#define VQ_MAXD 32                 // channels of a codeword
#define VQ_MAXIN 63                // 3 + 6 * 10 embedded coordinates

// h = relu(W1 x + b1), v = W2 h + b2 for one point: bias first, then an fp32 FMA chain over the inputs in order.  x_of(k): the k-th input.
// MAXD: the compile-time bound of `dim` a caller's register arrays are sized for (8 | 16 | 32): the guarded chains are the same whatever it is.
template <int MAXD, class XOF>
__device__ __forceinline__ void vq_project_point(XOF&& x_of, int in_dim, int dim, k4_cptr w1, k4_cptr b1, k4_cptr w2, k4_cptr b2,
                                                 float (&h)[MAXD], float (&v)[MAXD]) {
#pragma unroll
    for (int j = 0; j < MAXD; ++j) h[j] = j < dim ? b1[j] : 0.f;
    for (int k = 0; k < in_dim; ++k) {
        const float xv = x_of(k);
#pragma unroll
        for (int j = 0; j < MAXD; ++j)
            if (j < dim) h[j] = fmaf(xv, w1[j * in_dim + k], h[j]);
    }
#pragma unroll
    for (int j = 0; j < MAXD; ++j) { h[j] = fmaxf(h[j], 0.f); v[j] = j < dim ? b2[j] : 0.f; }
#pragma unroll
    for (int k = 0; k < MAXD; ++k) {
        if (k < dim) {
#pragma unroll
            for (int j = 0; j < MAXD; ++j)
                if (j < dim) v[j] = fmaf(h[k], w2[j * dim + k], v[j]);
        }
    }
}

// |v|^2 as flatten.pow(2).sum(1): the squares rounded, added over the channels in order
template <int MAXD>
__device__ __forceinline__ float vq_norm2(const float (&v)[MAXD], int dim) {
    float v2 = 0.f;
#pragma unroll
    for (int j = 0; j < MAXD; ++j)
        if (j < dim) v2 = __fadd_rn(v2, __fmul_rn(v[j], v[j]));
    return v2;
}

// `ne` prepared rows (stride S: the codeword, then |e|^2) holding the codes e0, e0 + 1, ...: dist = (|v|^2 - (2 v) . E_e) + |E_e|^2 (lib/grid.py:68-72);
// the running best is replaced only by a strictly smaller distance, so the lowest index wins a tie.
template <int MAXD, class ROWS>
__device__ __forceinline__ void vq_scan_rows(ROWS rows, int ne, int e0, int S, int dim, const float (&v)[MAXD], float v2, float& best, int& best_e) {
    for (int e = 0; e < ne; ++e) {
        float dot = 0.f;
#pragma unroll
        for (int j = 0; j < MAXD; ++j)
            if (j < dim) dot = fmaf(2.f * v[j], rows[e * S + j], dot);
        const float d = __fadd_rn(__fsub_rn(v2, dot), rows[e * S + dim]);
        if (best_e < 0 || d < best) { best = d; best_e = e0 + e; }
    }
}
