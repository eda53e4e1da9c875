"""CPU oracle of DirectContractedVoxGO.forward (/root/reference/lib/dcvgo.py:255-383).  TEST INFRASTRUCTURE ONLY.

Restates the contracted-space marcher in fp32 torch on the CPU, in the style of ``oracle/marcher.py`` and on its pieces
(DenseGrid / MaskGrid lookups, the colour MLP, the view-direction PE, ``segment_coo``) and on ``oracle/native_cpu.py``
(``raw2alpha``, ``alpha2weight``).  ``cumdist_thres`` (lib/cuda/ub360_utils_kernel.cu:12-32) is the sequential scan with reset,
vectorised over rays only: every add is the one the per-ray loop makes, in the same order.

The model is described by the checkpoint contents (``model_kwargs``, ``model_state_dict``) alone.  Pinned by
``tests/golden/march_dcvgo_*.npz`` (the reference's own class run on the CPU, tests/gen_contracted_golden.py).
"""
import numpy as np
import torch

from oracle import native_cpu as nat
from oracle.marcher import dense_grid, mask_grid, _rgbnet_layers, _mlp, _pe, _segment_sum


def cumdist_thres(dist, thres):
    """mask[r, i] = (c > thres) for c += dist[r, i], reset to 0 after every hit (fp32, in step order)."""
    dist = dist.float()
    thres = torch.tensor(float(np.float32(thres)), dtype=torch.float32)
    c = torch.zeros(dist.shape[0], dtype=torch.float32)
    out = torch.zeros(dist.shape, dtype=torch.bool)
    for i in range(dist.shape[1]):
        c = c + dist[:, i]
        over = c > thres
        c = c * (~over).float()
        out[:, i] = over
    return out


def geometry(model_kwargs, sd):
    """world_size / voxel_size_ratio of DirectContractedVoxGO._set_grid_resolution (lib/dcvgo.py:60-62,125-131), torch fp32."""
    xyz_min, xyz_max = sd['xyz_min'].float(), sd['xyz_max'].float()
    vsb = ((xyz_max - xyz_min).prod() / model_kwargs['num_voxels_base']).pow(1 / 3)
    vs = ((xyz_max - xyz_min).prod() / model_kwargs['num_voxels']).pow(1 / 3)
    ws = ((xyz_max - xyz_min) / vs).long()
    return {'world_size': ws, 'world_len': int(ws[0]), 'voxel_size_ratio': vs / vsb}


def step_table(world_len, stepsize, bg_len=0.2):
    """t of every step (lib/dcvgo.py:239-247)."""
    N_inner = int(2 / (2 + 2 * bg_len) * world_len / stepsize) + 1
    b_inner = torch.linspace(0, 2, N_inner + 1)
    b_outer = 2 / torch.linspace(1, 1 / 128, N_inner + 1)
    return torch.cat([(b_inner[1:] + b_inner[:-1]) * 0.5, (b_outer[1:] + b_outer[:-1]) * 0.5])


def sample_ray(sd, contracted_norm, world_len, rays_o, rays_d, stepsize, bg_len=0.2):
    """lib/dcvgo.py:213-253 -> (ray_pts [N, n, 3], inner_mask [N, n], t [n])."""
    o = (rays_o.float() - sd['scene_center'].float()) / sd['scene_radius'].float()
    d = rays_d.float() / rays_d.float().norm(dim=-1, keepdim=True)
    t = step_table(world_len, stepsize, bg_len)
    pts = o[:, None, :] + d[:, None, :] * t[None, :, None]
    norm = pts.abs().amax(dim=-1, keepdim=True) if contracted_norm == 'inf' else pts.norm(dim=-1, keepdim=True)
    inner = norm <= 1
    pts = torch.where(inner, pts, pts / norm * ((1 + bg_len) - norm.reciprocal() * bg_len))
    return pts, inner.squeeze(-1), t


def forward(model_kwargs, sd, rays_o, rays_d, viewdirs, stepsize, bg=0, render_depth=False, counters=None, **_ignored):
    """Every key of lib/dcvgo.py:358-380 (+ depth); counters: pre-mask (inner | cumdist), after mask_cache, after alpha, after w."""
    bg_len = float(model_kwargs.get('bg_len', 0.2))
    geo = geometry(model_kwargs, sd)
    thres = float(model_kwargs.get('fast_color_thres', 0))
    xyz_min, xyz_max = sd['xyz_min'].float(), sd['xyz_max'].float()
    N = rays_o.shape[0]
    pts, inner, t = sample_ray(sd, model_kwargs.get('contracted_norm', 'inf'), geo['world_len'], rays_o, rays_d, stepsize, bg_len)
    n_max = len(t)
    interval = stepsize * geo['voxel_size_ratio']
    ray_id = torch.arange(N).view(-1, 1).expand(N, n_max).flatten()
    step_id = torch.arange(n_max).view(1, -1).expand(N, n_max).flatten()

    mask = inner.clone()
    dist_thres = (2 + 2 * bg_len) / geo['world_len'] * stepsize * 0.95
    dist = (pts[:, 1:] - pts[:, :-1]).norm(dim=-1)
    mask[:, 1:] |= cumdist_thres(dist, dist_thres)
    m = mask.flatten()
    pts, inner, tt, ray_id, step_id = pts.reshape(-1, 3)[m], inner.flatten()[m], t[None].expand(N, n_max).flatten()[m], ray_id[m], step_id[m]
    n_pre = pts.shape[0]

    m = mask_grid(sd['mask_cache.mask'], pts, sd['mask_cache.xyz2ijk_scale'].float(), sd['mask_cache.xyz2ijk_shift'].float())
    pts, inner, tt, ray_id, step_id = pts[m], inner[m], tt[m], ray_id[m], step_id[m]
    n_mask = pts.shape[0]

    density = dense_grid(sd['density.grid'].float(), pts, xyz_min, xyz_max)
    _, alpha = nat.raw2alpha(density.flatten(), float(sd['act_shift']), float(interval))
    if thres > 0:
        m = alpha > thres
        pts, inner, tt, ray_id, step_id, density, alpha = pts[m], inner[m], tt[m], ray_id[m], step_id[m], density[m], alpha[m]
    n_alpha = pts.shape[0]
    weights, _, alphainv_last, _, _ = nat.alpha2weight(alpha, ray_id, N)
    if thres > 0:
        m = weights > thres
        pts, inner, tt, ray_id, step_id, density, alpha, weights = (pts[m], inner[m], tt[m], ray_id[m], step_id[m], density[m], alpha[m],
                                                                    weights[m])
    n_shade = pts.shape[0]

    k0 = dense_grid(sd['k0.grid'].float(), pts, xyz_min, xyz_max)
    if k0.dim() == 1:
        k0 = k0.unsqueeze(-1)
    layers = _rgbnet_layers(sd)
    if layers is None:
        rgb = torch.sigmoid(k0)
    else:
        emb = _pe(viewdirs.float(), sd['viewfreq'].float()).flatten(0, -2)[ray_id]
        rgb = torch.sigmoid(_mlp(layers, torch.cat([k0, emb], -1)))
    rgb_marched = _segment_sum(weights.unsqueeze(-1) * rgb, ray_id, N)
    rgb_marched += alphainv_last.unsqueeze(-1) * bg
    wsum_mid = _segment_sum(weights[inner], ray_id[inner], N)
    s = 1 - (1 + tt).reciprocal()
    ret = {'alphainv_last': alphainv_last, 'weights': weights, 'wsum_mid': wsum_mid, 'rgb_marched': rgb_marched, 'raw_density': density,
           'raw_alpha': alpha, 'raw_rgb': rgb, 'ray_id': ray_id, 'step_id': step_id, 'n_max': n_max, 't': tt, 's': s}
    if render_depth:
        ret['depth'] = _segment_sum(weights * s, ray_id, N)
    if counters is not None:
        counters.update(n_rays=N, n_total=N * n_max, n_pre=n_pre, n_mask=n_mask, n_alpha=n_alpha, n_shade=n_shade)
    return ret
