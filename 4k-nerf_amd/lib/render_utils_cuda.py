"""Drop-in for the reference's JIT-built ``render_utils_cuda`` extension module.

Same 13 function names, argument order and returned tensors as the pybind11 module defined in
/root/reference/lib/cuda/render_utils.cpp:170-184, implemented on the gfx950 staged kernels of
``csrc/k4_staged.hip`` through the C ABI (``include/k4nerf.h``).  Differences, all deliberate:
  * kernels run on torch's CURRENT stream (the reference uses the legacy default stream);
  * launch errors are checked; inputs must be GPU + contiguous (same guard as render_utils.cpp:46-48);
  * ``sample_pts_on_rays`` still needs one host sync for the data-dependent total length (as the
    reference does at render_utils_kernel.cu:212) -- the fused marcher has none.
"""
import torch

from .. import _native as N

__all__ = ['infer_t_minmax', 'infer_n_samples', 'infer_ray_start_dir', 'sample_pts_on_rays',
           'sample_ndc_pts_on_rays', 'sample_bg_pts_on_rays', 'maskcache_lookup', 'raw2alpha',
           'raw2alpha_backward', 'raw2alpha_nonuni', 'raw2alpha_nonuni_backward', 'alpha2weight',
           'alpha2weight_backward']


def _f(x):
    return float(x)


def infer_t_minmax(rays_o, rays_d, xyz_min, xyz_max, near, far):
    n = rays_o.shape[0]
    t_min = torch.empty([n], dtype=torch.float32, device=rays_o.device)
    t_max = torch.empty_like(t_min)
    N.check(N.lib().k4_infer_t_minmax(N.f32(rays_o), N.f32(rays_d), N.f32(xyz_min), N.f32(xyz_max),
                                      _f(near), _f(far), n, N.f32(t_min), N.f32(t_max), N.stream()), 'infer_t_minmax')
    return [t_min, t_max]


def infer_n_samples(rays_d, t_min, t_max, stepdist):
    n = t_min.shape[0]
    out = torch.empty([n], dtype=torch.int64, device=rays_d.device)
    N.check(N.lib().k4_infer_n_samples(N.f32(rays_d), N.f32(t_min), N.f32(t_max), _f(stepdist), n,
                                       N.ptr(out), N.stream()), 'infer_n_samples')
    return out


def infer_ray_start_dir(rays_o, rays_d, t_min):
    start = torch.empty_like(rays_o)
    rdir = torch.empty_like(rays_o)
    N.check(N.lib().k4_infer_ray_start_dir(N.f32(rays_o), N.f32(rays_d), N.f32(t_min), rays_o.shape[0],
                                           N.f32(start), N.f32(rdir), N.stream()), 'infer_ray_start_dir')
    return [start, rdir]


def sample_pts_on_rays(rays_o, rays_d, xyz_min, xyz_max, near, far, stepdist):
    """-> [rays_pts, mask_outbbox, ray_id, step_id, N_steps, t_min, t_max]  (render_utils_kernel.cu:241)"""
    dev = rays_o.device
    n = rays_o.shape[0]
    N_steps = torch.empty([n], dtype=torch.int64, device=dev)
    t_min = torch.empty([n], dtype=torch.float32, device=dev)
    t_max = torch.empty_like(t_min)
    L = N.lib()
    N.check(L.k4_sample_pts_on_rays_count(N.f32(rays_o), N.f32(rays_d), N.f32(xyz_min), N.f32(xyz_max),
                                          _f(near), _f(far), _f(stepdist), n, N.ptr(N_steps), N.f32(t_min),
                                          N.f32(t_max), N.stream()), 'sample_pts_on_rays(count)')
    cum = N_steps.cumsum(0)
    total = int(cum[-1].item()) if n > 0 else 0
    pts = torch.empty([total, 3], dtype=torch.float32, device=dev)
    mask = torch.empty([total], dtype=torch.bool, device=dev)
    ray_id = torch.empty([total], dtype=torch.int64, device=dev)
    step_id = torch.empty([total], dtype=torch.int64, device=dev)
    N.check(L.k4_sample_pts_on_rays_fill(N.f32(rays_o), N.f32(rays_d), N.f32(xyz_min), N.f32(xyz_max),
                                         N.f32(t_min), N.ptr(cum), _f(stepdist), n, total, N.f32(pts),
                                         N.ptr(mask), N.ptr(ray_id), N.ptr(step_id), N.stream()),
            'sample_pts_on_rays(fill)')
    return [pts, mask, ray_id, step_id, N_steps, t_min, t_max]


def sample_ndc_pts_on_rays(rays_o, rays_d, xyz_min, xyz_max, N_samples):
    n = rays_o.shape[0]
    pts = torch.empty([n, N_samples, 3], dtype=torch.float32, device=rays_o.device)
    mask = torch.empty([n, N_samples], dtype=torch.bool, device=rays_o.device)
    N.check(N.lib().k4_sample_ndc_pts_on_rays(N.f32(rays_o), N.f32(rays_d), N.f32(xyz_min), N.f32(xyz_max),
                                              n, int(N_samples), N.f32(pts), N.ptr(mask), N.stream()),
            'sample_ndc_pts_on_rays')
    return [pts, mask]


def sample_bg_pts_on_rays(rays_o, rays_d, t_max, bg_preserve, N_samples):
    """-> rays_pts [n_rays, N_samples, 3]: the inverse-sphere background samples of lib/dbvgo.py (render_utils_kernel.cu:301-340)"""
    n = rays_o.shape[0]
    pts = torch.empty([n, int(N_samples), 3], dtype=torch.float32, device=rays_o.device)
    if n == 0:
        return pts
    N.check(N.lib().k4_sample_bg_pts_on_rays(N.f32(rays_o), N.f32(rays_d), N.f32(t_max), _f(bg_preserve), int(N_samples), n,
                                             N.f32(pts), N.stream()), 'sample_bg_pts_on_rays')
    return pts


def maskcache_lookup(world, xyz, xyz2ijk_scale, xyz2ijk_shift):
    n = xyz.shape[0]
    out = torch.zeros([n], dtype=torch.bool, device=xyz.device)
    if n == 0:
        return out
    N.check(N.lib().k4_maskcache_lookup(N.ptr(world), N.f32(xyz), N.f32(xyz2ijk_scale), N.f32(xyz2ijk_shift),
                                        world.shape[0], world.shape[1], world.shape[2], n, N.ptr(out), N.stream()),
            'maskcache_lookup')
    return out


def hit_coarse_geo(rays_o, rays_d, xyz_min, xyz_max, near, far, stepdist, world, xyz2ijk_scale, xyz2ijk_shift):
    """Not one of the reference's 13: ``sample_pts_on_rays`` + ``maskcache_lookup`` + "any sample of the ray inside the box and occupied?" in one
    launch (k4_hit_coarse_geo), without the sample list.  rays [n, 3] -> bool [n]."""
    n = rays_o.shape[0]
    hit = torch.empty([n], dtype=torch.bool, device=rays_o.device)
    if n == 0:
        return hit
    N.check(N.lib().k4_hit_coarse_geo(N.f32(rays_o), N.f32(rays_d), N.f32(xyz_min), N.f32(xyz_max), _f(near), _f(far), _f(stepdist), n,
                                      N.ptr(world), N.f32(xyz2ijk_scale), N.f32(xyz2ijk_shift), world.shape[0], world.shape[1], world.shape[2],
                                      N.ptr(hit), N.stream()), 'hit_coarse_geo')
    return hit


def patch_hit_counts(hit, bs):
    """hit [n_img, H, W] bool / uint8 -> int32 [n_img, P]: the hit rays of every ``patch_gen`` entry for tiles of side ``bs`` (k4_patch_hit_counts)."""
    n_img, H, W = (int(v) for v in hit.shape)
    P = int(N.lib().k4_patch_hit_entries(H, W, int(bs)))
    if P < 0:
        raise N.K4Error(f'patch_hit_counts: bad arguments (H, W, bs) = {(H, W, bs)}')
    counts = torch.empty([n_img, P], dtype=torch.int32, device=hit.device)
    if n_img == 0:
        return counts
    N.check(N.lib().k4_patch_hit_counts(N.ptr(hit), n_img, H, W, int(bs), N.ptr(counts), N.stream()), 'patch_hit_counts')
    return counts


# ---- scene preparation (csrc/k4_prep.hip): not among the reference's 13 either -----------------------------------------------------------------
def count_views_walk(rays_o, rays_d, xyz_min, xyz_max, near, step, n_samples, acc):
    """One view of ``voxel_count_views``: the trilinear weights of every sample of rays [n, 3] added to acc [X, Y, Z] (int64 storage of the unsigned
    32.32 fixed-point sums), no sample list in memory (k4_count_views_walk)."""
    X, Y, Z = (int(v) for v in acc.shape)
    if acc.dtype != torch.int64:
        raise N.K4Error(f'count_views_walk: int64 accumulator expected, got {acc.dtype}')
    N.check(N.lib().k4_count_views_walk(N.f32(rays_o), N.f32(rays_d), rays_o.shape[0], N.f32(xyz_min), N.f32(xyz_max), X, Y, Z, _f(near), _f(step),
                                        int(n_samples), N.ptr(acc), N.stream()), 'count_views_walk')


def count_views_finalise(acc, count):
    """count += (acc > 1.0); acc = 0 (k4_count_views_finalise).  count: fp32 with acc's number of elements."""
    if acc.dtype != torch.int64 or count.numel() != acc.numel():
        raise N.K4Error('count_views_finalise: an int64 accumulator and a count of the same size expected')
    N.check(N.lib().k4_count_views_finalise(N.ptr(acc), N.f32(count), acc.numel(), N.stream()), 'count_views_finalise')


def near_cam_mask(axes, cam_o, near_clip, density):
    """density [.., X, Y, Z] (in place) = -100 at the nodes (axes[0][i], axes[1][j], axes[2][k]) within near_clip of a camera centre (k4_near_cam_mask)."""
    X, Y, Z = (int(a.shape[0]) for a in axes)
    if density.numel() != X * Y * Z:
        raise N.K4Error('near_cam_mask: the density grid does not have the axes\' shape')
    N.check(N.lib().k4_near_cam_mask(N.f32(axes[0]), N.f32(axes[1]), N.f32(axes[2]), X, Y, Z, N.f32(cam_o), cam_o.shape[0], _f(near_clip),
                                     N.f32(density), N.stream()), 'near_cam_mask')


def _order_key(x):
    """fp32 <-> int32 with the same order (its own inverse; k4p_key of csrc/k4_prep.hip)."""
    k = x.view(torch.int32)
    return k ^ ((k >> 31) & 0x7fffffff)


def frustum_bounds(hw, Ks, c2ws, ndc_scale, max_pixels, ndc, inverse_y, flip_x, flip_y, use_viewdirs, ts):
    """Per view min / max of the points o + dir * t, t in ts (one or two values), over the rays of get_rays_of_a_view: hw int32 [n, 2], Ks [n, 3, 3],
    c2ws [n, 3, 4], ndc_scale [n, 2] on the device -> fp32 [n, 6] = min xyz, max xyz (k4_frustum_bounds)."""
    n = int(hw.shape[0])
    if hw.dtype != torch.int32 or tuple(Ks.shape) != (n, 3, 3) or tuple(c2ws.shape) != (n, 3, 4) or tuple(ndc_scale.shape) != (n, 2):
        raise N.K4Error('frustum_bounds: hw int32 [n, 2], Ks [n, 3, 3], c2ws [n, 3, 4], ndc_scale [n, 2] expected')
    inf = torch.full([n, 3], float('inf'), dtype=torch.float32, device=hw.device)
    keys = _order_key(torch.cat([inf, -inf], 1).contiguous()).contiguous()
    N.check(N.lib().k4_frustum_bounds(N.ptr(hw), N.f32(Ks), N.f32(c2ws), N.f32(ndc_scale), n, int(max_pixels), int(bool(ndc)), int(bool(inverse_y)),
                                      int(bool(flip_x)), int(bool(flip_y)), int(bool(use_viewdirs)), len(ts), _f(ts[0]), _f(ts[-1]),
                                      N.ptr(keys), N.stream()), 'frustum_bounds')
    return _order_key(keys).view(torch.float32)


def coarse_geo_bounds(density, act_shift, interval, thres):
    """density [X, Y, Z] -> int32 [6] on the device: min / max node index per axis where raw2alpha(density + act_shift, interval) > thres;
    {INT32_MAX x 3, -1 x 3} when no node passes (k4_coarse_geo_bounds)."""
    X, Y, Z = (int(v) for v in density.shape)
    out = torch.tensor([2 ** 31 - 1] * 3 + [-1] * 3, dtype=torch.int32).to(density.device)
    N.check(N.lib().k4_coarse_geo_bounds(N.f32(density), X, Y, Z, _f(act_shift), _f(interval), _f(thres), N.ptr(out), N.stream()), 'coarse_geo_bounds')
    return out


def _raw2alpha(density, shift, interval, ipp):
    exp_d = torch.empty_like(density)
    alpha = torch.empty_like(density)
    N.check(N.lib().k4_raw2alpha(N.f32(density), _f(shift), _f(interval), None if ipp is None else N.f32(ipp),
                                 density.shape[0], N.f32(exp_d), N.f32(alpha), N.stream()), 'raw2alpha')
    return [exp_d, alpha]


def raw2alpha(density, shift, interval):
    return _raw2alpha(density, shift, interval, None)


def raw2alpha_nonuni(density, shift, interval):
    return _raw2alpha(density, shift, 0.0, interval)


def _raw2alpha_bwd(exp_d, grad_back, interval, ipp):
    grad = torch.empty_like(exp_d)
    N.check(N.lib().k4_raw2alpha_backward(N.f32(exp_d), N.f32(grad_back), _f(interval),
                                          None if ipp is None else N.f32(ipp), exp_d.shape[0], N.f32(grad),
                                          N.stream()), 'raw2alpha_backward')
    return grad


def raw2alpha_backward(exp_d, grad_back, interval):
    return _raw2alpha_bwd(exp_d, grad_back, interval, None)


def raw2alpha_nonuni_backward(exp_d, grad_back, interval):
    return _raw2alpha_bwd(exp_d, grad_back, 0.0, interval)


def alpha2weight(alpha, ray_id, n_rays):
    """-> [weight, T, alphainv_last, i_start, i_end]"""
    dev = alpha.device
    n_rays = int(n_rays)
    weight = torch.empty_like(alpha)
    T = torch.empty_like(alpha)
    ainv = torch.empty([n_rays], dtype=alpha.dtype, device=dev)
    i_start = torch.empty([n_rays], dtype=torch.int64, device=dev)
    i_end = torch.empty([n_rays], dtype=torch.int64, device=dev)
    N.check(N.lib().k4_alpha2weight(N.f32(alpha), N.ptr(ray_id), alpha.shape[0], n_rays, N.f32(weight), N.f32(T),
                                    N.f32(ainv), N.ptr(i_start), N.ptr(i_end), N.stream()), 'alpha2weight')
    return [weight, T, ainv, i_start, i_end]


def alpha2weight_backward(alpha, weight, T, alphainv_last, i_start, i_end, n_rays, grad_weights, grad_last):
    grad = torch.empty_like(alpha)
    gw, gl = grad_weights.contiguous(), grad_last.contiguous()       # named: the copies must outlive the launch
    N.check(N.lib().k4_alpha2weight_backward(N.f32(alpha), N.f32(weight), N.f32(T), N.f32(alphainv_last),
                                             N.ptr(i_start), N.ptr(i_end), int(n_rays), alpha.shape[0],
                                             N.f32(gw), N.f32(gl), N.f32(grad), N.stream()), 'alpha2weight_backward')
    return grad
