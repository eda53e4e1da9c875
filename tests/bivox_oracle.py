"""CPU oracle of DirectBiVoxGO (/root/reference/lib/dbvgo.py).  TEST INFRASTRUCTURE ONLY.

``sample_bg_pts_on_rays`` (lib/cuda/render_utils_kernel.cu:301-340) in two forms:
  * ``sample_bg_pts_fp32``   -- the fp32 tensor form of ``oracle/native_cpu.py`` (what the reference's Python runs on through the stubs of
                                ``oracle/ref_import.py`` when the goldens are made);
  * ``sample_bg_pts_source`` -- numpy, rounding as the CUDA source does: its ``1.`` literals make ``t_inner - 1. + 1. / (1. - (float)i_step /
                                N_samples)`` and ``R*R/(t*t) * (1.-bg_preserve) + R/t * bg_preserve`` evaluate in fp64 (the fp32 sub-expressions
                                first, in fp32) before the assignment to ``float`` rounds them; ``o + d*t`` and the sum of squares are FMAs.
``forward`` restates the two-pass ``DirectBiVoxGO.forward`` (lib/dbvgo.py:310-397) in fp32 torch on the pieces of ``oracle/marcher.py`` and
``oracle/native_cpu.py``, with the sample counters of both passes.  The model is described by the checkpoint contents alone.  Pinned by
``tests/golden/march_dbvgo_*.npz`` (the reference's own class run on the CPU, tests/gen_bivox_golden.py).
"""
import numpy as np
import torch

from oracle import native_cpu as nat
from oracle.marcher import dense_grid, mask_grid, _rgbnet_layers, _mlp, _pe, _segment_sum

sample_bg_pts_fp32 = nat.sample_bg_pts_on_rays


def _fma32(a, b, c):
    """fp32 fma through fp64: the 24x24-bit product is exact, the sum rounds once in fp64 and once to fp32."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def sample_bg_pts_source(rays_o, rays_d, t_max, bg_preserve, N_samples):
    """[n_rays, N_samples, 3] fp32 (numpy), every operation in the precision the CUDA source gives it."""
    f32, f64 = np.float32, np.float64
    o = np.asarray(rays_o, dtype=f32)[:, None, :]
    d = np.asarray(rays_d, dtype=f32)[:, None, :]
    t_inner = np.asarray(t_max, dtype=f32)[:, None]
    N_samples = int(N_samples)
    bgp = f32(bg_preserve)                                            # `const float bg_preserve`
    frac = np.arange(N_samples, dtype=f32)[None, :] / f32(N_samples)  # (float)i_step / N_samples: fp32
    t = ((t_inner.astype(f64) - 1.) + 1. / (1. - frac.astype(f64))).astype(f32)
    q = _fma32(d, t[..., None], o)
    x, y, z = q[..., 0], q[..., 1], q[..., 2]
    tn = np.sqrt(_fma32(z, z, _fma32(y, y, x * x)))                   # norm3: sqrt(x*x + y*y + z*z), contracted
    m = np.maximum(np.abs(x), np.maximum(np.abs(y), np.abs(z)))
    R = tn / m
    a = (R * R) / (tn * tn)
    b = (R / tn) * bgp
    s = (a.astype(f64) * (1. - f64(bgp)) + b.astype(f64)).astype(f32)
    return q * s[..., None]


def geometry(model_kwargs):
    """world_size / voxel_size / voxel_size_ratio of DirectBiVoxGO._set_grid_resolution on the -/+1 box (lib/dbvgo.py:41-43,130-135), torch fp32."""
    ext = torch.Tensor([2, 2, 2])
    vsb = (ext.prod() / model_kwargs['num_voxels_base']).pow(1 / 3)
    vs = (ext.prod() / model_kwargs['num_voxels']).pow(1 / 3)
    return {'world_size': (ext / vs).long(), 'voxel_size': vs, 'voxel_size_ratio': vs / vsb}


def n_outer(model_kwargs, stepsize):
    """lib/dbvgo.py:234,242 with the host float32 ``stepdist.item()``."""
    stepdist = stepsize * geometry(model_kwargs)['voxel_size']
    return stepdist, int(np.sqrt(3) / stepdist.item() * (1 - float(model_kwargs.get('bg_preserve', 0.5)))) + 1


def _sub(sd, prefix, i):
    """The keys ``<prefix>.<i>.*`` of a DirectBiVoxGO state_dict under the single-module names ``<prefix>.*``."""
    p = f'{prefix}.{i}.'
    return {prefix + '.' + k[len(p):]: v for k, v in sd.items() if k.startswith(p)}


def _pass(sd, i, pts, ray_id, step_id, viewdirs, interval, N, thres, prev=None):
    """DirectBiVoxGO._forward (lib/dbvgo.py:247-308) for grid pair i -> (dict, [after prev, after mask, after alpha, after w])."""
    xyz_min, xyz_max = sd['xyz_min'].float(), sd['xyz_max'].float()
    if prev is not None:
        m = prev > thres
        ray_id, step_id, pts = ray_id.view(N, -1)[m].reshape(-1), step_id.view(N, -1)[m].reshape(-1), pts.view(N, -1, 3)[m].reshape(-1, 3)
    cnt = [pts.shape[0]]
    m = mask_grid(sd[f'mask_cache.{i}.mask'], pts, sd[f'mask_cache.{i}.xyz2ijk_scale'].float(), sd[f'mask_cache.{i}.xyz2ijk_shift'].float())
    pts, ray_id, step_id = pts[m], ray_id[m], step_id[m]
    cnt.append(pts.shape[0])
    density = dense_grid(sd[f'density.{i}.grid'].float(), pts, xyz_min, xyz_max)
    _, alpha = nat.raw2alpha(density.flatten(), float(sd['act_shift']), float(interval))
    if thres > 0:
        m = alpha > thres
        pts, ray_id, step_id, alpha = pts[m], ray_id[m], step_id[m], alpha[m]
    cnt.append(pts.shape[0])
    weights, _, alphainv_last, _, _ = nat.alpha2weight(alpha, ray_id, N)
    if thres > 0:
        m = weights > thres
        pts, ray_id, step_id, alpha, weights = pts[m], ray_id[m], step_id[m], alpha[m], weights[m]
    cnt.append(pts.shape[0])
    k0 = dense_grid(sd[f'k0.{i}.grid'].float(), pts, xyz_min, xyz_max)
    if k0.dim() == 1:
        k0 = k0.unsqueeze(-1)
    layers = _rgbnet_layers(_sub(sd, 'rgbnet', i))
    if layers is None:
        rgb = torch.sigmoid(k0)
    else:
        emb = _pe(viewdirs.float(), sd['viewfreq'].float()).flatten(0, -2)[ray_id]
        rgb = torch.sigmoid(_mlp(layers, torch.cat([k0, emb], -1)))
    return dict(rgb=rgb, alpha=alpha, weights=weights, alphainv_last=alphainv_last, ray_id=ray_id, step_id=step_id), cnt


def _segment_max(src, index, out):
    if src.numel():
        out.scatter_reduce_(0, index, src, reduce='amax', include_self=True)
    return out


def forward(model_kwargs, sd, rays_o, rays_d, viewdirs, stepsize, bg=0, render_depth=False, counters=None, bg_sampler='fp32', passes=None,
            **_ignored):
    """Every key of lib/dbvgo.py:360-395.  counters: ``fg`` / ``bg`` = [pre-filter, after mask_cache, after alpha, shaded] of each pass.
    bg_sampler: 'fp32' (oracle/native_cpu.py) or 'source' (sample_bg_pts_source).  passes: a dict that receives the two per-pass dicts."""
    thres = float(model_kwargs.get('fast_color_thres', 0))
    bgp = float(model_kwargs.get('bg_preserve', 0.5))
    geo = geometry(model_kwargs)
    N = rays_o.shape[0]
    o = (rays_o.float() - sd['scene_center'].float()) / sd['scene_radius'].float()
    d = rays_d.float() / rays_d.float().norm(dim=-1, keepdim=True)
    stepdist, N_outer = n_outer(model_kwargs, stepsize)
    pts, outbbox, ray_id, step_id, _, _, t_max = nat.sample_pts_on_rays(o, d, sd['xyz_min'].float(), sd['xyz_max'].float(), 0, 2 * np.sqrt(3),
                                                                        stepdist)
    inb = ~outbbox
    pts, ray_id, step_id = pts[inb], ray_id[inb], step_id[inb]
    if bg_sampler == 'fp32':
        outer = sample_bg_pts_fp32(o, d, t_max, bgp, N_outer)
    else:
        outer = torch.from_numpy(sample_bg_pts_source(o.numpy(), d.numpy(), t_max.numpy(), bgp, N_outer))
    interval = stepsize * geo['voxel_size_ratio']
    fg, cnt_fg = _pass(sd, 0, pts, ray_id, step_id, viewdirs, interval, N, thres)
    rid = torch.arange(N).view(-1, 1).expand(N, N_outer).flatten()
    sid = torch.arange(N_outer).view(1, -1).expand(N, N_outer).flatten()
    bq, cnt_bg = _pass(sd, 1, outer.reshape(-1, 3), rid, sid, viewdirs, interval, N, thres, prev=fg['alphainv_last'])
    Tf, Tb = fg['alphainv_last'], bq['alphainv_last']
    rgb_marched = _segment_sum(fg['weights'].unsqueeze(-1) * fg['rgb'], fg['ray_id'], N) + \
        Tf.unsqueeze(-1) * _segment_sum(bq['weights'].unsqueeze(-1) * bq['rgb'], bq['ray_id'], N) + (Tf * Tb).unsqueeze(-1) * bg
    ret = {'rgb_marched': rgb_marched, 'alphainv_last': torch.cat([Tf, Tb]), 'weights': torch.cat([fg['weights'], bq['weights']]),
           'raw_alpha': torch.cat([fg['alpha'], bq['alpha']]), 'raw_rgb': torch.cat([fg['rgb'], bq['rgb']]),
           'ray_id': torch.cat([fg['ray_id'], bq['ray_id']])}
    if render_depth:
        depth_fg = _segment_sum(fg['weights'] * fg['step_id'], fg['ray_id'], N)
        depth_bg = _segment_sum(bq['weights'] * bq['step_id'], bq['ray_id'], N)
        last_fg = _segment_max(fg['step_id'].float(), fg['ray_id'], torch.zeros([N]))
        last_bg = _segment_max(bq['step_id'].float(), bq['ray_id'], last_fg.clone())
        ret['depth'] = depth_fg + Tf * (1 + last_fg + depth_bg) + Tf * Tb * (2 + last_fg + last_bg)
    if counters is not None:
        counters.update(n_rays=N, n_outer=N_outer, fg=cnt_fg, bg=cnt_bg)
    if passes is not None:
        passes.update(fg=fg, bg=bq)
    return ret


def depth_scale(model_kwargs, fg_step_max, stepsize):
    """The largest value the depth formula can take: 2 + max foreground step + N_outer - 1 (a weighted sum of step indices, not of [0, 1] values)."""
    return 2 + int(fg_step_max) + n_outer(model_kwargs, stepsize)[1] - 1
