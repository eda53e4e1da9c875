// Scene preparation: what a scene-reconstruction run computes ONCE before its first iteration (run_sr.py:222-291, 366, 440-448 of the reference) --
// per-voxel view counts, the camera-frustum box, the near-camera density mask, the box of the coarse geometry.  Each is one streaming launch (the
// view count: two per view) on values that carry the bits of the staged op sequence (k4_staged_ops.h), so the decisions are the staged path's.
#include <limits.h>
#include "k4_common.h"
#include "k4_staged_ops.h"

#define K4_THREADS 256
static inline unsigned k4_blocks(int64_t n) { return (unsigned)((n + K4_THREADS - 1) / K4_THREADS); }

// ---------------------------------------------------------------- voxel_count_views (lib/dvgo.py:235-268)
// The reference looks an all-ones grid up at every sample of every ray of a view and counts the voxels whose gradient exceeds 1: per voxel the SUM of
// the trilinear weights the view's samples put on it.  Here the weights are summed as 32.32 fixed point (round(w * 2^32), w in [0, 1]) with integer
// atomics: order-independent, so the predicate sum > 1 is the same on every run and for every order of the rays.
//
// Why an accumulator cannot wrap.  (a) One atomic adds at most 2^32 + 1 (k4p_add clamps: a lane's merged run s > 2^32 already decides the predicate, and
// min(s, 2^32 + 1) decides it the same way).  (b) A lane issues at most one atomic per (sample, corner), so one LAUNCH adds at most
// n_rays * n_samples * (2^32 + 1) to a voxel; the entry point cuts a view into launches of n_rays * n_samples <= 2^30, i.e. < 2^63 per launch.
// (c) A lane adds only after it READ a value <= 2^32.  Values only grow between two finalise passes and a launch starts with clean caches, so once a
// voxel exceeds 2^32 at the end of a launch no later launch adds to it.  Hence value <= 2^32 + 2^30 * (2^32 + 1) < 2^63 always, for any number of rays.
#define K4P_ONE (1ull << 32)

__device__ __forceinline__ void k4p_add(unsigned long long* __restrict__ acc, size_t i, unsigned long long s) {
    if (s == 0) return;
    // plain (cacheable) read first: only sum > 1 is needed and the terms are non-negative, so a voxel that is already past 1 needs no more adds.  A stale
    // read costs one redundant add and cannot change the predicate.  This is what keeps a view's ~10^9 corner terms off the atomic units.
    if (acc[i] > K4P_ONE) return;
    atomicAdd(acc + i, s > K4P_ONE ? K4P_ONE + 1 : s);
}

// One lane walks one ray; consecutive lanes take consecutive rays.  Sample i sits where the staged method's tensor expressions put it, one rounding
// per torch op:  vec = d == 0 ? 1e-6 : d;  t_min = clamp(max_c min((max_c - o_c) / vec_c, (min_c - o_c) / vec_c), near, 1e9)  (far is ignored, as
// upstream);  t_i = t_min + (step * i) / |d|;  p = o + d * t_i.  Zero padding: there is no box test -- a sample outside the box still feeds those of
// its corners that are grid nodes.  A sample is skipped only when its cell has no corner on the grid (cell index outside [-1, size - 1] on some axis).
// Each coordinate of p is monotone in i, so the samples whose cell touches the grid are consecutive: the walk ends at the first miss after a hit.
// Per corner slot a lane keeps the last voxel and its running sum in registers and issues the add when the voxel changes (stepsize 0.5: every other sample).
__global__ void __launch_bounds__(K4_THREADS)
k_count_views_walk(const float* __restrict__ ro, const float* __restrict__ rd, int64_t n_rays, const float* __restrict__ mn, const float* __restrict__ mx,
                   int X, int Y, int Z, float near, float step, int n_samples, unsigned long long* __restrict__ acc) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rays) return;
    float o[3], d[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) { o[a] = ro[r * 3 + a]; d[a] = rd[r * 3 + a]; }
    float tmin = 0.f;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float vec = d[a] == 0.f ? 1e-6f : d[a];
        const float t = fminf(__fdiv_rn(__fsub_rn(mx[a], o[a]), vec), __fdiv_rn(__fsub_rn(mn[a], o[a]), vec));
        tmin = a == 0 ? t : fmaxf(tmin, t);
    }
    tmin = fminf(fmaxf(tmin, near), 1e9f);
    const float nrm = __fsqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(d[0], d[0]), __fmul_rn(d[1], d[1])), __fmul_rn(d[2], d[2])));

    size_t pidx[8];
    unsigned long long psum[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) { pidx[c] = 0; psum[c] = 0; }
    bool seen = false;
    for (int i = 0; i < n_samples; ++i) {
        const float t = __fadd_rn(tmin, __fdiv_rn(__fmul_rn(step, (float)i), nrm));
        const K4Tri tri = k4s_grid_tri(__fadd_rn(o[0], __fmul_rn(d[0], t)), __fadd_rn(o[1], __fmul_rn(d[1], t)), __fadd_rn(o[2], __fmul_rn(d[2], t)),
                                       mn, mx, X, Y, Z);
        const bool touches = tri.x0 >= -1 && tri.x0 < X && tri.y0 >= -1 && tri.y0 < Y && tri.z0 >= -1 && tri.z0 < Z;
        if (!touches) {
            if (seen) break;
            continue;
        }
        seen = true;
        size_t idx[8];
        float w[8];
        k4s_tri_corners(tri, X, Y, Z, idx, w);              // idx < X*Y*Z wherever w != 0 (corners off the grid: w = 0)
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            if (!(w[c] > 0.f)) continue;
            const unsigned long long q = __float2ull_rn(w[c] * 4294967296.f);
            if (idx[c] == pidx[c]) {
                psum[c] += q;                                // <= n_samples * 2^32 < 2^63
            } else {
                k4p_add(acc, pidx[c], psum[c]);
                pidx[c] = idx[c];
                psum[c] = q;
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 8; ++c) k4p_add(acc, pidx[c], psum[c]);
}

// count += (sum > 1), sum = 0: one streaming pass; nothing model-specific (any sampler's accumulate pass can sit in front of it)
__global__ void k_count_views_finalise(unsigned long long* __restrict__ acc, float* __restrict__ count, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (acc[i] > K4P_ONE) count[i] += 1.f;
    acc[i] = 0;
}

// ---------------------------------------------------------------- maskout_near_cam_vox (lib/dvgo.py:186-198)
// A thread per grid node, a loop over the cameras: density = -100 where min_cam sqrt((dx*dx + dy*dy) + dz*dz) <= near_clip, every operation rounded on
// its own as the tensor expression (nodes - cam).pow(2).sum(-1).sqrt() does.  ax / ay / az: the node coordinates per axis (the linspaces the staged
// method's node table is a meshgrid of).
__global__ void k_near_cam_mask(const float* __restrict__ ax, const float* __restrict__ ay, const float* __restrict__ az, int X, int Y, int Z,
                                const float* __restrict__ cam, int n_cam, float near_clip, float* __restrict__ density) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)X * Y * Z) return;
    const int z = (int)(i % Z), y = (int)((i / Z) % Y), x = (int)(i / ((int64_t)Y * Z));
    const float px = ax[x], py = ay[y], pz = az[z];
    const k4_cptr C = k4_const(cam);                         // uniform index: scalar loads
    float nearest = INFINITY;
    for (int c = 0; c < n_cam; ++c) {
        const float dx = __fsub_rn(px, C[c * 3 + 0]), dy = __fsub_rn(py, C[c * 3 + 1]), dz = __fsub_rn(pz, C[c * 3 + 2]);
        nearest = fminf(nearest, __fsqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz))));
    }
    if (nearest <= near_clip) density[i] = -100.f;
}

// ---------------------------------------------------------------- order-independent min / max reductions
// fp32 -> int32 with the same order (an involution: the decoder is the same expression); min / max of the keys are integer atomics
__device__ __forceinline__ int k4p_key(float f) {
    const int k = __float_as_int(f);
    return k ^ ((k >> 31) & 0x7fffffff);
}
// lo[3] -> min, hi[3] -> max over the workgroup (4 waves), then one atomic pair per value into out[0..2] (min) / out[3..5] (max)
__device__ __forceinline__ void k4p_block_minmax(int (&lo)[3], int (&hi)[3], int* __restrict__ out) {
    __shared__ int part[K4_THREADS / K4_WAVE][6];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) {
            lo[a] = min(lo[a], __shfl_xor(lo[a], s));
            hi[a] = max(hi[a], __shfl_xor(hi[a], s));
        }
    const int wave = (int)(threadIdx.x / K4_WAVE);
    if (k4_lane() == 0)
#pragma unroll
        for (int a = 0; a < 3; ++a) { part[wave][a] = lo[a]; part[wave][3 + a] = hi[a]; }
    __syncthreads();
    if (threadIdx.x < 6) {
        int v = part[0][threadIdx.x];
        for (int wv = 1; wv < K4_THREADS / K4_WAVE; ++wv) v = threadIdx.x < 3 ? min(v, part[wv][threadIdx.x]) : max(v, part[wv][threadIdx.x]);
        if (threadIdx.x < 3) atomicMin(out + threadIdx.x, v);
        else atomicMax(out + threadIdx.x, v);
    }
}

// ---------------------------------------------------------------- compute_bbox_by_cam_frustrm (run_sr.py:222-268)
// All training views in one launch: blockIdx.y = view (its own H, W, K, c2w), a workgroup strides over the view's pixels.  Per pixel the ray of
// get_rays_of_a_view (k4s_ray_of_pixel) and the points o + dir * t_k, k < n_t (dir = the unit view direction when use_viewdirs, else rays_d), mul and
// add rounded separately.  keys [n_views][6]: per view min xyz / max xyz as k4p_key integers (the caller fills them with the keys of +inf / -inf).
__global__ void __launch_bounds__(K4_THREADS)
k_frustum_bounds(const int32_t* __restrict__ hw, const float* __restrict__ Ks, const float* __restrict__ c2ws, const float* __restrict__ ndc_scale,
                 int ndc, int inverse_y, int flip_x, int flip_y, int use_viewdirs, int n_t, float t0, float t1, int* __restrict__ keys) {
    const int view = (int)blockIdx.y;
    const int H = hw[view * 2 + 0], W = hw[view * 2 + 1];
    const k4_cptr K = k4_const(Ks + (size_t)view * 9), M = k4_const(c2ws + (size_t)view * 12);
    const float c_w = ndc_scale[view * 2 + 0], c_h = ndc_scale[view * 2 + 1];
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    const int64_t n_pix = (int64_t)H * W;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n_pix; p += (int64_t)gridDim.x * blockDim.x) {
        const int row = (int)(p / W), col = (int)(p - (int64_t)row * W);
        float o[3], v[3], u[3];
        k4s_ray_of_pixel(row, col, H, W, K, M, ndc, inverse_y, flip_x, flip_y, 0.5f, c_w, c_h, o, v, u);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float dir = use_viewdirs ? u[a] : v[a];
            const float p0 = __fadd_rn(o[a], __fmul_rn(dir, t0));
            const float p1 = n_t > 1 ? __fadd_rn(o[a], __fmul_rn(dir, t1)) : p0;
            lo[a] = fminf(lo[a], fminf(p0, p1));
            hi[a] = fmaxf(hi[a], fmaxf(p0, p1));
        }
    }
    int klo[3], khi[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) { klo[a] = k4p_key(lo[a]); khi[a] = k4p_key(hi[a]); }
    k4p_block_minmax(klo, khi, keys + (size_t)view * 6);
}

// ---------------------------------------------------------------- compute_bbox_by_coarse_geo (run_sr.py:271-291)
// One pass over the dense density grid: alpha = raw2alpha(density + act_shift, interval) (k4s_raw2alpha) at the NODE itself, and per axis the integer
// min / max of the node indices with alpha > thres.  out[6] = {min x, y, z, max x, y, z}; the caller fills {INT_MAX x 3, -1 x 3}.
__global__ void __launch_bounds__(K4_THREADS)
k_coarse_geo_bounds(const float* __restrict__ density, int X, int Y, int Z, float shift, float interval, float thres, int* __restrict__ out) {
    int lo[3] = {INT_MAX, INT_MAX, INT_MAX}, hi[3] = {-1, -1, -1};
    const int64_t n = (int64_t)X * Y * Z;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        float e, alpha;
        k4s_raw2alpha(density[i], shift, interval, e, alpha);
        if (alpha > thres) {
            const int c[3] = {(int)(i / ((int64_t)Y * Z)), (int)((i / Z) % Y), (int)(i % Z)};
#pragma unroll
            for (int a = 0; a < 3; ++a) { lo[a] = min(lo[a], c[a]); hi[a] = max(hi[a], c[a]); }
        }
    }
    k4p_block_minmax(lo, hi, out);
}

// ---------------------------------------------------------------- C ABI
#define ST ((hipStream_t)stream)
#define REQ(c) do { if (!(c)) return K4_ERR_BAD_ARG; } while (0)
#define K4P_MAX_GRID 65535

extern "C" int k4_count_views_walk(const float* rays_o, const float* rays_d, int64_t n_rays, const float* xyz_min, const float* xyz_max,
                                   int32_t X, int32_t Y, int32_t Z, float near, float step, int32_t n_samples, uint64_t* acc, void* stream) {
    REQ(xyz_min && xyz_max && acc && X > 0 && Y > 0 && Z > 0 && n_rays >= 0 && n_samples >= 0 && n_samples <= (1 << 20));
    if (n_rays == 0 || n_samples == 0) return K4_OK;
    REQ(rays_o && rays_d);
    const int64_t per_launch = ((int64_t)1 << 30) / n_samples;             // n_rays * n_samples <= 2^30 per launch: the no-wrap bound above
    for (int64_t r0 = 0; r0 < n_rays; r0 += per_launch) {
        const int64_t n = n_rays - r0 < per_launch ? n_rays - r0 : per_launch;
        hipLaunchKernelGGL(k_count_views_walk, dim3(k4_blocks(n)), dim3(K4_THREADS), 0, ST, rays_o + r0 * 3, rays_d + r0 * 3, n, xyz_min, xyz_max,
                           X, Y, Z, near, step, n_samples, (unsigned long long*)acc);
        const int rc = k4_check_launch();
        if (rc) return rc;
    }
    return K4_OK;
}
extern "C" int k4_count_views_finalise(uint64_t* acc, float* count, int64_t n_voxels, void* stream) {
    REQ(n_voxels >= 0 && n_voxels <= (int64_t)K4_THREADS * 0x7fffffff);
    if (n_voxels == 0) return K4_OK;
    REQ(acc && count);
    hipLaunchKernelGGL(k_count_views_finalise, dim3(k4_blocks(n_voxels)), dim3(K4_THREADS), 0, ST, (unsigned long long*)acc, count, n_voxels);
    return k4_check_launch();
}
extern "C" int k4_near_cam_mask(const float* axis_x, const float* axis_y, const float* axis_z, int32_t X, int32_t Y, int32_t Z, const float* cam_o,
                                int32_t n_cam, float near_clip, float* density, void* stream) {
    REQ(axis_x && axis_y && axis_z && cam_o && density && X > 0 && Y > 0 && Z > 0 && n_cam > 0 && (int64_t)X * Y <= 0x7fffffff / Z * (int64_t)K4_THREADS);
    hipLaunchKernelGGL(k_near_cam_mask, dim3(k4_blocks((int64_t)X * Y * Z)), dim3(K4_THREADS), 0, ST, axis_x, axis_y, axis_z, X, Y, Z, cam_o, n_cam,
                       near_clip, density);
    return k4_check_launch();
}
extern "C" int k4_frustum_bounds(const int32_t* hw, const float* Ks, const float* c2ws, const float* ndc_scale, int32_t n_views, int64_t max_pixels,
                                 int32_t ndc, int32_t inverse_y, int32_t flip_x, int32_t flip_y, int32_t use_viewdirs, int32_t n_t, float t0, float t1,
                                 int32_t* keys, void* stream) {
    REQ(hw && Ks && c2ws && ndc_scale && keys && n_views > 0 && n_views <= 65535 && max_pixels > 0 && (n_t == 1 || n_t == 2));
    const int64_t bx = k4_blocks(max_pixels);
    hipLaunchKernelGGL(k_frustum_bounds, dim3((unsigned)(bx < K4P_MAX_GRID ? bx : K4P_MAX_GRID), (unsigned)n_views), dim3(K4_THREADS), 0, ST, hw, Ks, c2ws,
                       ndc_scale, ndc, inverse_y, flip_x, flip_y, use_viewdirs, n_t, t0, t1, keys);
    return k4_check_launch();
}
extern "C" int k4_coarse_geo_bounds(const float* density, int32_t X, int32_t Y, int32_t Z, float act_shift, float interval, float thres, int32_t* out6,
                                    void* stream) {
    REQ(density && out6 && X > 0 && Y > 0 && Z > 0);
    const int64_t bx = k4_blocks((int64_t)X * Y * Z);
    hipLaunchKernelGGL(k_coarse_geo_bounds, dim3((unsigned)(bx < K4P_MAX_GRID ? bx : K4P_MAX_GRID)), dim3(K4_THREADS), 0, ST, density, X, Y, Z, act_shift,
                       interval, thres, out6);
    return k4_check_launch();
}
