"""Generate ``tests/golden/{march_dbvgo_*,grad_dbvgo,occ_dbvgo}.npz`` from the REFERENCE's own ``lib/dbvgo.py``.  TEST INFRASTRUCTURE ONLY.
Usage (build container, where the reference tree exists):  PYTHONDONTWRITEBYTECODE=1 python tests/gen_bivox_golden.py

The reference module is imported unmodified on the CPU through the stubs of ``oracle/ref_import.py`` (the JIT ``load`` of render_utils_cuda
-> oracle/native_cpu.py).  After the import the module's ``segment_coo`` name is replaced by a function that also serves ``reduce='max'``
(lib/dbvgo.py:382-391; the stub asserts 'sum').  With ``rgbnet_dim <= 0`` upstream builds ``rgbnet = None`` and indexes it in forward: the coarse
case sets ``model.rgbnet = [None, None]``.  Upstream's constructor registers ONE mask tensor in both MaskGrids, so a strict load on the CPU would
leave both with the background's mask: each reference model gets its own copies before the state is loaded (the package's class does the same).

Condition on the inputs (asserted here): on every golden the reference, the fp32 restatement and the source-rounded restatement
(tests/bivox_oracle.py) produce identical ray_id / step_id lists of both passes, so no sample sits within an ulp of a filter or mask decision and
a mismatch on the GPU is a defect, not a tie.  A case whose seed fails the condition moves to the next seed.
"""
import contextlib
import importlib
import io
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, HERE]

from oracle import ref_import                  # noqa: E402
import nerf4k_amd                              # noqa: E402,F401
from nerf4k_amd import scene                   # noqa: E402
import bivox_oracle as bo                      # noqa: E402

GOLDEN = os.path.join(HERE, 'golden')


def _segment_coo(src, index, out=None, dim_size=None, reduce='sum'):
    if reduce == 'sum':
        return ref_import._segment_coo(src, index, out=out, dim_size=dim_size)
    assert reduce == 'max' and out is not None
    if src.numel():
        out.scatter_reduce_(0, index, src, reduce='amax', include_self=True)
    return out


def load_reference_dbvgo():
    cpp_ext, real_load = ref_import._install_stubs()
    saved_path = list(sys.path)
    saved_lib = {k: v for k, v in sys.modules.items() if k == 'lib' or k.startswith('lib.')}
    for k in saved_lib:
        del sys.modules[k]
    sys.path.insert(0, ref_import.REFERENCE_ROOT)
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            dbvgo = importlib.import_module('lib.dbvgo')
    finally:
        cpp_ext.load = real_load
        sys.path[:] = saved_path
        for k in [k for k in sys.modules if k == 'lib' or k.startswith('lib.')]:
            del sys.modules[k]
        sys.modules.update(saved_lib)
    dbvgo.segment_coo = _segment_coo
    return dbvgo


def _np(v):
    if torch.is_tensor(v):
        v = v.detach().cpu()
        if v.dtype == torch.int64:
            v = v.int()                 # index tensors stored as int32 (size)
        return v.numpy()
    return np.asarray(v)


def _kwargs_json(kw):
    return json.dumps({k: (v.tolist() if isinstance(v, np.ndarray) or torch.is_tensor(v) else v) for k, v in kw.items()})


def _ref_model(ref, ck):
    with contextlib.redirect_stdout(io.StringIO()):
        model = ref.DirectBiVoxGO(**ck['model_kwargs'])
        if model.rgbnet is None:
            model.rgbnet = [None, None]
    for mc in model.mask_cache:          # upstream hands ONE tensor to both MaskGrids (`mask.bool()` of a bool tensor is the tensor itself): un-aliased,
        mc.mask = mc.mask.clone()        # or loading mask_cache.1.mask would overwrite mask_cache.0.mask
    model.load_state_dict(ck['model_state_dict'])
    return model


def _rays(H, W, pose_i, n_keep):
    """n_keep rays of a view from inside the cube (t_min clamps to 0) plus 16 made by hand: from outside the cube into it, from outside past it
    (misses), along an axis (two zero direction components) from inside and from outside.  201 rays for n_keep = 185: no multiple of 64."""
    from oracle import marcher
    ro, rd, vd = marcher.get_rays_of_a_view(H, W, scene.unbounded_K(H, W), scene.unbounded_poses()[pose_i], ndc=False)
    sel = torch.randperm(H * W, generator=torch.Generator().manual_seed(pose_i))[:n_keep].sort().values
    ro, rd = ro.reshape(-1, 3)[sel], rd.reshape(-1, 3)[sel]
    c = torch.tensor(scene.UNBOUNDED_CENTER, dtype=torch.float32)
    R = scene.UNBOUNDED_RADIUS
    g = torch.Generator().manual_seed(100 + pose_i)
    extra_o, extra_d = [], []
    for i in range(6):                                   # outside, aimed at a point inside the cube
        p = torch.randn(3, generator=g)
        p = p / p.abs().max() * (1.3 + 0.1 * i)
        tgt = (torch.rand(3, generator=g) * 2 - 1) * 0.5
        extra_o.append(c + R * p)
        extra_d.append((tgt - p) * 0.7)
    for i in range(5):                                   # outside, aimed past the cube
        p = torch.randn(3, generator=g)
        p = p / p.abs().max() * 1.5
        q = torch.randn(3, generator=g)
        q = q / q.abs().max() * 1.6
        q[int(p.abs().argmax())] = p[int(p.abs().argmax())] * 1.1
        extra_o.append(c + R * p)
        extra_d.append(q - p)
    axis = [(0.131, -0.207, -0.413), (-0.317, 0.223, 0.109), (0.271, 0.153, -1.37), (0.419, -1.29, 0.057), (1.43, 0.211, -0.171)]
    dirs = [(0., 0., 1.), (0., -1., 0.), (0., 0., 1.), (0., 1., 0.), (-1., 0., 0.)]
    for p, dd in zip(axis, dirs):                        # two zero direction components: from inside (2) and from outside (3)
        extra_o.append(c + R * torch.tensor(p))
        extra_d.append(torch.tensor(dd) * 1.7)
    ro = torch.cat([ro, torch.stack(extra_o)]).contiguous()
    rd = torch.cat([rd, torch.stack(extra_d)]).contiguous()
    return [ro, rd, (rd / rd.norm(dim=-1, keepdim=True)).contiguous()]


def _common(ck, rk):
    arrs = {'model_class': np.array(ck['model_class']), 'model_kwargs_json': np.array(_kwargs_json(ck['model_kwargs'])),
            'render_kwargs_json': np.array(json.dumps(rk))}
    for k, v in ck['model_state_dict'].items():
        arrs['sd/' + k] = _np(v)
    return arrs


def _save(name, arrs):
    path = os.path.join(GOLDEN, name + '.npz')
    np.savez_compressed(path, **arrs)
    print(f'{name}: {os.path.getsize(path) / 1024:.1f} KiB')
    assert os.path.getsize(path) < 1000 * 1024


CASES = {
    # N_outer = 26 (< 64, no multiple of anything convenient), up to ~100 foreground steps
    'march_dbvgo_w128': dict(cfg=dict(seed=81, num_voxels=30 ** 3, rgbnet_dim=2, rgbnet_width=128, rgbnet_depth=3, fast_color_thres=1e-4,
                                      bg_preserve=0.5, stepsize=0.5), bg=1),
    # N_outer = 78 and up to ~190 foreground steps: both passes cross a 64-lane chunk; threshold 0: the last-step rule
    'march_dbvgo_w64': dict(cfg=dict(seed=82, num_voxels=28 ** 3, rgbnet_dim=3, rgbnet_width=64, rgbnet_depth=2, viewbase_pe=2,
                                     fast_color_thres=0, bg_preserve=0.2, stepsize=0.25), bg=0),
    'march_dbvgo_w32_nomlp': dict(cfg=dict(seed=83, num_voxels=24 ** 3, rgbnet_dim=6, rgbnet_width=32, bg_use_mlp=False, fast_color_thres=1e-3,
                                           bg_preserve=0.5, stepsize=0.5), bg=1),
    'march_dbvgo_coarse': dict(cfg=dict(seed=84, num_voxels=28 ** 3, rgbnet_dim=0, fast_color_thres=0, bg_preserve=0.35, stepsize=0.5), bg=0),
}


def _reference_passes(model, rays, rk):
    """The reference's own per-pass sample lists: sample_ray + _forward as forward strings them (lib/dbvgo.py:322-344)."""
    N = len(rays[0])
    ray_pts, ray_id, step_id, outer = model.sample_ray(ori_rays_o=rays[0], ori_rays_d=rays[1], **rk)
    interval = rk['stepsize'] * model.voxel_size_ratio
    fg = model._forward(ray_pts=ray_pts, viewdirs=rays[2], interval=interval, N=N, mask_grid=model.mask_cache[0], density_grid=model.density[0],
                        k0_grid=model.k0[0], rgbnet=model.rgbnet[0], ray_id=ray_id, step_id=step_id)
    bg = model._forward(ray_pts=outer, viewdirs=rays[2], interval=interval, N=N, mask_grid=model.mask_cache[1], density_grid=model.density[1],
                        k0_grid=model.k0[1], rgbnet=model.rgbnet[1], prev_alphainv_last=fg['alphainv_last'])
    return fg, bg, outer.shape[1]


def _march_case(ref, name, c, pose_i, seed):
    ck = scene.make_bivox_checkpoint(**dict(c['cfg'], seed=seed))
    rk = dict(ck['render_kwargs'], bg=c['bg'])
    rays = _rays(24, 32, pose_i, 185)
    model = _ref_model(ref, ck)
    with torch.no_grad():
        out = model(*rays, **rk)
        fg, bg, N_outer = _reference_passes(model, rays, rk)
    # the condition on the inputs: three sample lists, identical in both passes
    cnts = []
    for sampler in ('fp32', 'source'):
        cnt, ps = {}, {}
        bo.forward(ck['model_kwargs'], ck['model_state_dict'], *rays, counters=cnt, passes=ps, bg_sampler=sampler, **rk)
        for tag, want in (('fg', fg), ('bg', bg)):
            if not (torch.equal(ps[tag]['ray_id'], want['ray_id']) and torch.equal(ps[tag]['step_id'], want['step_id'])):
                return None
        assert cnt['n_outer'] == N_outer
        cnts.append(cnt['fg'] + cnt['bg'])
    if cnts[0] != cnts[1]:
        return None
    fg_steps = int(fg['step_id'].max()) if fg['step_id'].numel() else 0
    n_fg_max = int(ref.render_utils_cuda.sample_pts_on_rays(
        (rays[0] - model.scene_center) / model.scene_radius, rays[1] / rays[1].norm(dim=-1, keepdim=True), model.xyz_min, model.xyz_max, 0,
        2 * np.sqrt(3), rk['stepsize'] * model.voxel_size)[4].max())
    arrs = _common(ck, rk)
    for k, v in zip(('rays_o', 'rays_d', 'viewdirs'), rays):
        arrs['in/' + k] = _np(v)
    for k, v in out.items():
        arrs['out/' + k] = _np(v)
    arrs['aux/counters'] = np.asarray(cnts[0], dtype=np.int64)
    arrs['aux/n_outer'] = np.array(N_outer)
    arrs['aux/fg_step_max'] = np.array(fg_steps)
    arrs['aux/fg_steps_sampled_max'] = np.array(n_fg_max)
    for tag, p in (('fg', fg), ('bg', bg)):
        arrs[f'aux/{tag}_ray_id'], arrs[f'aux/{tag}_step_id'] = _np(p['ray_id']), _np(p['step_id'])
    print(f'{name}: seed {seed}, N_outer {N_outer}, longest foreground ray {n_fg_max} steps, counters {cnts[0]}, '
          f'mean T_fg*T_bg {float((out["alphainv_last"][:len(rays[0])] * out["alphainv_last"][len(rays[0]):]).mean()):.3f}')
    return arrs


def gen_march(ref):
    for i, (name, c) in enumerate(CASES.items()):
        for seed in range(c['cfg']['seed'], c['cfg']['seed'] + 1000, 100):
            arrs = _march_case(ref, name, c, i, seed)
            if arrs is not None:
                break
            print(f'{name}: seed {seed} holds a tie between the restatements, next seed')
        else:
            raise SystemExit(f'{name}: no seed without ties')
        _save(name, arrs)


def gen_grad(ref):
    ck = scene.make_bivox_checkpoint(seed=85, num_voxels=24 ** 3, rgbnet_dim=3, rgbnet_width=32, viewbase_pe=2, fast_color_thres=1e-4, stepsize=0.5)
    rk = dict(ck['render_kwargs'], bg=1)
    rays = _rays(24, 32, 5, 160)
    model = _ref_model(ref, ck)
    target = torch.rand([rays[0].shape[0], 3], generator=torch.Generator().manual_seed(3))
    out = model(*rays, global_step=0, **rk)
    loss = F.mse_loss(out['rgb_marched'], target)
    loss.backward()
    arrs = _common(ck, rk)
    for k, v in zip(('rays_o', 'rays_d', 'viewdirs'), rays):
        arrs['in/' + k] = _np(v)
    arrs['target'] = _np(target)
    arrs['loss'] = np.array(float(loss))
    for k, p in model.named_parameters():
        if p.grad is not None:
            arrs['grad/' + k] = _np(p.grad)
    _save('grad_dbvgo', arrs)


def gen_occ(ref):
    ck = scene.make_bivox_checkpoint(seed=86, num_voxels=18 ** 3, rgbnet_dim=0, fast_color_thres=1e-3)
    model = _ref_model(ref, ck)
    arrs = _common(ck, ck['render_kwargs'])
    plus = 1.5
    with torch.no_grad():
        model.density[0].grid += plus
        model.density[1].grid += plus
    arrs['density_plus'] = np.array(plus)
    with contextlib.redirect_stdout(io.StringIO()):
        model.update_occupancy_cache()
    for i in range(2):
        arrs[f'upd/mask{i}'] = _np(model.mask_cache[i].mask)
    new = 22 ** 3
    with contextlib.redirect_stdout(io.StringIO()):
        model.scale_volume_grid(new)
    arrs['new_num_voxels'] = np.array(new)
    arrs['scale/world_size'] = _np(model.world_size)
    for i in range(2):
        arrs[f'scale/density{i}'] = _np(model.density[i].grid)
        arrs[f'scale/k0{i}'] = _np(model.k0[i].grid)
        arrs[f'scale/mask{i}'] = _np(model.mask_cache[i].mask)
    _save('occ_dbvgo', arrs)


if __name__ == '__main__':
    if not ref_import.available():
        raise SystemExit('the reference tree is not present: nothing to generate')
    torch.manual_seed(0)
    ref = load_reference_dbvgo()
    gen_march(ref)
    gen_grad(ref)
    gen_occ(ref)
