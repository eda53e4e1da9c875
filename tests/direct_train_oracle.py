"""Oracle of the direct-colour DirectVoxGO training step (rgbnet_dim = 0; run_sr.py:523-546 on lib/dvgo.py:327-437).  TEST INFRASTRUCTURE ONLY.

``evaluate``     the graph in fp64 torch autograd ON A GIVEN SAMPLE LIST: the samples that passed the alpha filter (points and ray ids, in depth
                 order per ray) and, per sample, whether the weight filter kept it.  Lookups (align_corners=True, zero padding), the activation,
                 the sequential transmittance product with its T < 1e-3 stop, sigmoid, and the three loss lines.  The list is an input, so the
                 oracle never decides a filter: it measures arithmetic error only.
``sample_list``  a restatement of the sampler and the three filters in fp32 or fp64, for the golden generator's condition that no sample of a
                 golden scene sits within rounding of a decision.
``chunks``       the checkpoint-table arithmetic of the fused kernels.
"""
import numpy as np
import torch
import torch.nn.functional as F

FAR = 1e9


def chunks(n_steps):
    """64-step chunks of a ray of n_steps steps = floats per ray of the transmittance checkpoint table."""
    return (int(n_steps) + 63) // 64


def lookup(grid, pts, xyz_min, xyz_max):
    """DenseGrid.forward (lib/grid.py:117-128) in the grid's dtype -> [n, C]."""
    ind = ((pts - xyz_min) / (xyz_max - xyz_min)).flip((-1,)) * 2 - 1
    out = F.grid_sample(grid, ind.reshape(1, 1, 1, -1, 3), mode='bilinear', align_corners=True)
    return out.reshape(grid.shape[1], -1).T


def raw2alpha(density, shift, interval):
    return 1 - (1 + torch.exp(density + shift)) ** (-interval)


def points_of(rays_o, rays_d, xyz_min, xyz_max, near, stepdist, ray_id, step_id):
    """k_pts_fill's expression in fp32 (fma emulated through fp64: the product of two fp32 values is exact there)."""
    o, d, mn, mx = (t.float() for t in (rays_o, rays_d, xyz_min, xyz_max))
    vec = torch.where(d == 0, torch.full_like(d, 1e-6), d)
    t_min = torch.minimum((mx - o) / vec, (mn - o) / vec).amax(-1).clamp(min=near, max=FAR)
    fma = lambda a, b, c: (a.double() * b.double() + c.double()).float()
    rn = fma(d[:, 2], d[:, 2], fma(d[:, 1], d[:, 1], d[:, 0] * d[:, 0])).sqrt()
    start = fma(d, t_min[:, None], o)
    direction = d / rn[:, None]
    dist = (torch.tensor(stepdist, dtype=torch.float32) * step_id.float())
    return fma(direction[ray_id], dist[:, None], start[ray_id])


def sample_list(sd, fast_color_thres, rays_o, rays_d, near, stepdist, interval, dtype):
    """The sampler and the filters of lib/dvgo.py:295-369 restated in `dtype` -> dict(ray_id, step_id: the shaded list; a_ray_id, a_step_id: the
    alpha-passing list in front of and including each ray's stop; shaded: which of those the weight filter keeps)."""
    o, d = rays_o.to(dtype), rays_d.to(dtype)
    mn, mx = sd['xyz_min'].to(dtype), sd['xyz_max'].to(dtype)
    vec = torch.where(d == 0, torch.full_like(d, 1e-6), d)
    ra, rb = (mx - o) / vec, (mn - o) / vec
    t_min = torch.minimum(ra, rb).amax(-1).clamp(min=near, max=FAR)
    t_max = torch.maximum(ra, rb).amin(-1).clamp(min=near, max=FAR)
    rn = d.norm(dim=-1)
    n_steps = torch.ceil((t_max - t_min) * rn / stepdist).clamp(min=1).long()
    ray_id = torch.repeat_interleave(torch.arange(len(o)), n_steps)
    first = torch.cumsum(n_steps, 0) - n_steps
    step_id = torch.arange(int(n_steps.sum())) - first[ray_id]
    start, direction = o + d * t_min[:, None], d / rn[:, None]
    pts = start[ray_id] + direction[ray_id] * (torch.tensor(stepdist, dtype=dtype) * step_id.to(dtype))[:, None]
    keep = ((mn <= pts) & (pts <= mx)).all(-1)
    mask = sd['mask_cache.mask']
    u = pts * sd['mask_cache.xyz2ijk_scale'].to(dtype) + sd['mask_cache.xyz2ijk_shift'].to(dtype)
    ijk = torch.where(u >= 0, torch.floor(u + 0.5), torch.ceil(u - 0.5)).long()             # C round(): halves away from zero
    inside = ((ijk >= 0) & (ijk < torch.tensor(mask.shape))).all(-1)
    ijk = ijk.clamp(min=0).minimum(torch.tensor(mask.shape) - 1)
    keep &= inside & mask[ijk[:, 0], ijk[:, 1], ijk[:, 2]]
    pts, ray_id, step_id = pts[keep], ray_id[keep], step_id[keep]
    alpha = raw2alpha(lookup(sd['density.grid'].to(dtype), pts, mn, mx)[:, 0], sd['act_shift'].to(dtype), interval)
    if fast_color_thres > 0:
        m = alpha > fast_color_thres
        ray_id, step_id, alpha = ray_id[m], step_id[m], alpha[m]
    a = alpha.numpy()
    rid = ray_id.numpy()
    w = np.zeros_like(a)
    live = np.zeros(len(a), dtype=bool)
    T, cur, stopped = a.dtype.type(1), -1, False
    for i in range(len(a)):
        if rid[i] != cur:
            T, cur, stopped = a.dtype.type(1), rid[i], False
        if stopped:
            continue
        live[i] = True
        w[i] = T * a[i]
        T = a.dtype.type(np.float64(T) - np.float64(T) * np.float64(a[i]))                    # fmaf(-T, a, T)
        stopped = T < 1e-3
    live = torch.from_numpy(live)
    shaded = torch.from_numpy(w > fast_color_thres) if fast_color_thres > 0 else torch.ones(len(a), dtype=torch.bool)
    if fast_color_thres > 0:
        out_ray, out_step = ray_id[live & shaded], step_id[live & shaded]
    else:
        out_ray, out_step = ray_id, step_id                                                   # no filter: the list keeps the samples behind the stop
    return {'ray_id': out_ray, 'step_id': out_step, 'a_ray_id': ray_id[live], 'a_step_id': step_id[live], 'shaded': shaded[live]}


def evaluate(density, k0, xyz_min, xyz_max, act_shift, interval, pts, ray_id, shaded, target, n_rays, bg, weight_main, weight_entropy_last,
             weight_rgbper, grad_total=1.0):
    """fp64 autograd of the training step on the alpha-passing samples `pts` [M, 3] of rays `ray_id` [M] (sorted, depth order inside a ray);
    `shaded` [M]: the weight filter's decisions.  Samples behind a ray's stop may be present: they get weight 0.
    -> dict(total, photo, psnr, entropy, rgbper, rgb_marched [n, 3], alphainv_last [n], grad_density, grad_k0), all fp64."""
    dd = density.detach().double().clone().requires_grad_(True)
    kk = k0.detach().double().clone().requires_grad_(True)
    mn, mx, pts, tgt = xyz_min.double(), xyz_max.double(), pts.double(), target.double()
    M = len(ray_id)
    alpha = raw2alpha(lookup(dd, pts, mn, mx)[:, 0], act_shift.double(), float(interval))
    counts = torch.bincount(ray_id, minlength=n_rays)
    L = max(int(counts.max()) if M else 0, 1)
    col = torch.arange(M) - (torch.cumsum(counts, 0) - counts)[ray_id]
    A = torch.zeros([n_rays, L], dtype=torch.float64).index_put((ray_id, col), alpha)
    incl = torch.cumprod(1 - A, 1)
    excl = torch.cat([torch.ones([n_rays, 1], dtype=torch.float64), incl[:, :-1]], 1)
    crossed = incl.detach() < 1e-3
    stop = torch.where(crossed.any(1), crossed.float().argmax(1), torch.full([n_rays], L - 1))
    live = torch.arange(L)[None] <= stop[:, None]                                             # the crossing sample included
    ainv = incl.gather(1, stop[:, None])[:, 0]
    w = (excl * A * live)[ray_id, col] * shaded.double()
    rgb = torch.sigmoid(lookup(kk, pts, mn, mx))
    marched = torch.zeros([n_rays, 3], dtype=torch.float64).index_add(0, ray_id, w[:, None] * rgb) + ainv[:, None] * bg
    photo = weight_main * F.mse_loss(marched, tgt)
    total = photo
    entropy = rgbper = torch.zeros([], dtype=torch.float64)
    if weight_entropy_last > 0:
        lo, hi = float(np.float32(1e-6)), float(np.float32(1 - 1e-6))                         # the fp32 tensor's clamp bounds
        p = ainv.clamp(lo, hi)
        entropy = weight_entropy_last * -(p * torch.log(p) + (1 - p) * torch.log(1 - p)).mean()
        total = total + entropy
    if weight_rgbper > 0:
        rgbper = weight_rgbper * ((rgb - tgt[ray_id]).pow(2).sum(-1) * w.detach()).sum() / n_rays
        total = total + rgbper
    (total * grad_total).backward()
    zero = lambda g, t: torch.zeros_like(t) if g is None else g
    return {'total': total.detach(), 'photo': photo.detach(), 'psnr': -10 * torch.log10(photo.detach()), 'entropy': entropy.detach(),
            'rgbper': rgbper.detach(), 'rgb_marched': marched.detach(), 'alphainv_last': ainv.detach(),
            'grad_density': zero(dd.grad, dd), 'grad_k0': zero(kk.grad, kk)}
