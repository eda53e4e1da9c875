"""DirectBiVoxGO (nerf4k_amd.lib.dbvgo) on the MI355X: the background sampler against its source-rounded restatement, the staged and the fused
(k4_march_bivox_fwd) paths against the reference-made goldens (tests/gen_bivox_golden.py) and the CPU oracle (tests/bivox_oracle.py), training
gradients, occupancy maintenance and the render loop."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import nerf4k_amd  # noqa: F401
from nerf4k_amd import _native as N, scene, render
from nerf4k_amd.lib import dbvgo, dvgo, render_utils_cuda, utils
from nerf4k_amd.lib.masked_adam import MaskedAdam
from helpers import GOLDEN, NATIVE_TOL, load_march_golden, psnr
import bivox_oracle as bo

pytestmark = pytest.mark.gpu
GOLD = ['march_dbvgo_w128', 'march_dbvgo_w64', 'march_dbvgo_w32_nomlp', 'march_dbvgo_coarse']
FLOAT_KEYS = ('rgb_marched', 'alphainv_last', 'weights', 'raw_alpha', 'raw_rgb', 'depth')


def _model(ck):
    return utils.model_from_checkpoint_dict(ck).cuda()


def _aux(name):
    z = np.load(os.path.join(GOLDEN, name + '.npz'))
    return {k[4:]: z[k] for k in z.files if k.startswith('aux/')}


def _dscale(g, aux):
    return bo.depth_scale(g['model_kwargs'], aux['fg_step_max'], g['render_kwargs']['stepsize'])


def _frame_rays(H, W, pose_i):
    pose = torch.from_numpy(scene.unbounded_poses()[pose_i]).cuda()
    ro, rd, vd = dvgo.get_rays_of_a_view(H, W, scene.unbounded_K(H, W), pose, False, inverse_y=False, flip_x=False, flip_y=False)
    return ro.reshape(-1, 3), rd.reshape(-1, 3), vd.reshape(-1, 3)


@pytest.mark.parametrize('bg_preserve', [0.2, 0.5])
@pytest.mark.parametrize('n_samples', [1, 63, 64, 65, 130])
def test_bg_sampler_vs_the_source_rounded_restatement(n_samples, bg_preserve):
    """k4_sample_bg_pts_on_rays against tests/bivox_oracle.sample_bg_pts_source on 257 rays; bound helpers.NATIVE_TOL['aabb/pts'] (6e-7 absolute,
    points in about [-1.2, 1.2]).  Largest difference measured on an MI355X over the ten cases: 0 (every coordinate bit for bit)."""
    g = torch.Generator().manual_seed(7)
    n = 257
    o = (torch.rand([n, 3], generator=g) * 2 - 1) * 0.9
    d = torch.randn([n, 3], generator=g)
    d[:6] = torch.tensor([[0, 0, 1.], [0, -1, 0], [1, 0, 0], [0, 0.6, 0.8], [-0.6, 0, 0.8], [0.8, -0.6, 0]])
    d = d / d.norm(dim=-1, keepdim=True)
    lo, hi = torch.Tensor([-1, -1, -1]).cuda(), torch.Tensor([1, 1, 1]).cuda()
    t_max = render_utils_cuda.infer_t_minmax(o.cuda(), d.cuda(), lo, hi, 0, 2 * np.sqrt(3))[1]
    got = render_utils_cuda.sample_bg_pts_on_rays(o.cuda(), d.cuda(), t_max, bg_preserve, n_samples)
    want = bo.sample_bg_pts_source(o.numpy(), d.numpy(), t_max.cpu().numpy(), bg_preserve, n_samples)
    assert got.shape == (n, n_samples, 3) and got.dtype == torch.float32
    err = float(np.abs(got.cpu().numpy().astype(np.float64) - want.astype(np.float64)).max())
    print(f'sample_bg_pts_on_rays N={n_samples} bg_preserve={bg_preserve}: max |diff| = {err:.3e}')
    assert err <= NATIVE_TOL['aabb/pts'][0], err
    m = got.abs().amax(-1)
    assert float(m.min()) >= bg_preserve - 1e-6 and float(m.max()) <= 1 + 1e-6                  # the inf-norm shell [bg_preserve, 1]
    empty = render_utils_cuda.sample_bg_pts_on_rays(torch.zeros([0, 3], device='cuda'), torch.zeros([0, 3], device='cuda'),
                                                    torch.zeros([0], device='cuda'), bg_preserve, n_samples)
    assert empty.shape == (0, n_samples, 3)


def _check_vs_reference(out, g, aux, keys, what):
    ds = _dscale(g, aux)
    for k in keys:
        s = ds if k == 'depth' else 1.0
        a, b = out[k].cpu(), g['out'][k]
        assert a.shape == b.shape, (what, k, a.shape, b.shape)
        err = float((a - b).abs().max()) if a.numel() else 0.0
        print(f'{what} {k}: max |diff| = {err:.3e} (scale {s})')
        assert psnr(a / s, b / s) >= 80, (what, k, psnr(a / s, b / s))
        assert err <= 1e-5 * s, (what, k, err)


@pytest.mark.parametrize('name', GOLD)
def test_golden_staged_every_key(name):
    g, aux = load_march_golden(name), _aux(name)
    model = _model(g).eval()
    r = {k: v.cuda() for k, v in g['rays'].items()}
    with torch.no_grad():
        out = model(r['rays_o'], r['rays_d'], r['viewdirs'], k4_staged=True, **g['render_kwargs'])
    ref = g['out']
    assert set(out) == set(ref) | {'rgb_feature'}, set(out) ^ set(ref)
    assert out['rgb_feature'] is out['rgb_marched']
    assert torch.equal(out['ray_id'].cpu(), ref['ray_id'].long())
    assert out['alphainv_last'].shape[0] == 2 * r['rays_o'].shape[0]
    _check_vs_reference(out, g, aux, FLOAT_KEYS, name + ' staged')
    # sample_ray: the reference's tuple, the foreground list before any filter, the background table
    pts, ray_id, step_id, outer = model.sample_ray(ori_rays_o=r['rays_o'], ori_rays_d=r['rays_d'], stepsize=g['render_kwargs']['stepsize'])
    assert pts.shape[0] == ray_id.shape[0] == step_id.shape[0] == int(aux['counters'][0])
    assert outer.shape == (r['rays_o'].shape[0], int(aux['n_outer']), 3)


@pytest.mark.parametrize('name', GOLD)
def test_golden_fused(name):
    """The one-launch inference path (k4_march_bivox_fwd) on every golden scene: the reference's rgb_marched / depth / alphainv_last, the staged
    path's to 1e-5 (depth on its scale), the sample counters of both passes exactly (the goldens hold no ties), the same bits with and without
    counters.  Measured on an MI355X: against the reference at most 1.8e-6 (rgb, alphainv_last) and 2.0e-6 of its scale (depth); fused - staged at
    most 8.3e-7 and 3.8e-7 of the scale; all 32 counters equal."""
    g, aux = load_march_golden(name), _aux(name)
    model = _model(g).eval()
    assert model._k4_fusable()
    r = {k: v.cuda() for k, v in g['rays'].items()}
    cnt = torch.zeros(8, dtype=torch.int64, device='cuda')
    with torch.no_grad():
        fused = model(r['rays_o'], r['rays_d'], r['viewdirs'], **g['render_kwargs'])
        counted = model(r['rays_o'], r['rays_d'], r['viewdirs'], k4_counters=cnt, **g['render_kwargs'])
        staged = model(r['rays_o'], r['rays_d'], r['viewdirs'], k4_staged=True, **g['render_kwargs'])
    assert set(fused) == {'alphainv_last', 'rgb_marched', 'rgb_feature', 'depth'} and fused['rgb_feature'] is fused['rgb_marched']
    keys = ('rgb_marched', 'depth', 'alphainv_last')
    _check_vs_reference(fused, g, aux, keys, name + ' fused')
    ds = _dscale(g, aux)
    for k in keys:
        s = ds if k == 'depth' else 1.0
        err = float((fused[k] - staged[k]).abs().max())
        print(f'{name} fused - staged {k}: {err:.3e}')
        assert err <= 1e-5 * s, (name, k, err)
        assert torch.equal(fused[k], counted[k]), (name, k)
    print(f'{name} counters {cnt.cpu().tolist()} golden {aux["counters"].tolist()}')
    assert cnt.cpu().tolist() == aux['counters'].tolist()


FRAMES = [dict(seed=91, num_voxels=64 ** 3, rgbnet_dim=12, rgbnet_width=128),
          dict(seed=92, num_voxels=48 ** 3, rgbnet_dim=6, rgbnet_width=64, bg_use_mlp=False, fast_color_thres=1e-3)]


@pytest.mark.parametrize('cfg', FRAMES)
def test_frame_vs_oracle(cfg):
    """A 48x48 frame of a larger seeded scene, fused and staged, against the CPU oracle (the source-rounded background sampler: the device's
    arithmetic): >= 80 dB, >= 99.8 % of rays within 2e-5 and every ray within 1e-4 (depth on the scale of its formula), the criterion of
    test_dcvgo_gpu.py::test_frame_vs_oracle.  The counters of both passes equal the oracle's within that test's tie tolerance; fused == staged to
    2e-5; neither pass is empty.  On the CPU the two restatements of the sampler agree with each other on these seeds: 100 % of rays within
    2e-5 for rgb / depth / alphainv_last on both (largest 6.9e-7 on seed 91, 6.6e-7 on seed 92), identical counters.  Measured on an MI355X, fused
    and staged alike: seed 91 (64^3, 12 channels, width 128) 99.957 % of rays within 2e-5 for rgb (largest 5.2e-5, 120.1 dB) and depth (largest
    2.2e-5 of its scale, 126.6 dB), 100 % for alphainv_last (largest 2.0e-6); seed 92 (48^3, no background MLP) 100 % everywhere (largest
    1.8e-6).  Counters: seed 91 differs from the oracle by one foreground bbox sample and one shaded background sample of ~280,000 / ~39,000,
    seed 92 equals it."""
    ck = scene.make_bivox_checkpoint(**cfg)
    model = _model(ck).eval()
    ro, rd, vd = _frame_rays(48, 48, 1)
    n = ro.shape[0]
    cnt_dev = torch.zeros(8, dtype=torch.int64, device='cuda')
    with torch.no_grad():
        fused = model(ro, rd, vd, k4_counters=cnt_dev, **ck['render_kwargs'])
        fused_plain = model(ro, rd, vd, **ck['render_kwargs'])
        staged = model(ro, rd, vd, k4_staged=True, **ck['render_kwargs'])
    cnt, ps = {}, {}
    want = bo.forward(ck['model_kwargs'], ck['model_state_dict'], ro.cpu(), rd.cpu(), vd.cpu(), counters=cnt, passes=ps, bg_sampler='source',
                      **ck['render_kwargs'])
    fg_max = int(ps['fg']['step_id'].max()) if ps['fg']['step_id'].numel() else 0
    ds = bo.depth_scale(ck['model_kwargs'], fg_max, ck['render_kwargs']['stepsize'])
    keys = ('rgb_marched', 'depth', 'alphainv_last')
    for tag, out in (('fused', fused), ('staged', staged)):
        for k in keys:
            s = ds if k == 'depth' else 1.0
            a, b = out[k].cpu() / s, want[k] / s
            rows = 2 * n if k == 'alphainv_last' else n
            err = (a - b).abs().reshape(rows, -1).amax(-1)
            share = float((err <= 2e-5).float().mean())
            print(f'{tag} {k}: {100 * share:.3f} % of rays within 2e-5, largest {float(err.max()):.2e}, {psnr(a, b):.1f} dB')
            assert psnr(a, b) >= 80, (tag, k, psnr(a, b))
            assert share >= 0.998 and float(err.max()) <= 1e-4, (tag, k, float(err.max()), share)
    for k in keys:
        s = ds if k == 'depth' else 1.0
        assert torch.equal(fused[k], fused_plain[k]), k                     # counting does not change the result
        assert float((fused[k] - staged[k]).abs().max()) <= 2e-5 * s, (k, float((fused[k] - staged[k]).abs().max()))
    cd = cnt_dev.cpu().tolist()
    tol = lambda m: max(2, m // 10000)
    print('counters', cd, 'oracle', cnt['fg'] + cnt['bg'])
    for got, exp in zip(cd, cnt['fg'] + cnt['bg']):
        assert abs(got - exp) <= tol(exp), (cd, cnt)
    assert abs(staged['ray_id'].shape[0] - (cnt['fg'][3] + cnt['bg'][3])) <= tol(cnt['fg'][3] + cnt['bg'][3])
    T = fused['alphainv_last']
    assert float((T[:n] * T[n:]).mean()) < 0.98 and cd[3] > 0 and cd[7] > 0          # neither pass is empty


def _close(got, want, name, rel=2e-5):
    got, want = got.detach().cpu().double(), want.double()
    assert got.shape == want.shape, (name, got.shape, want.shape)
    err = float((got - want).abs().max()) if got.numel() else 0.0
    assert err <= rel * float(want.abs().max() if want.numel() else 0) + 1e-9, (name, err)


def _npz_checkpoint(name):
    z = np.load(os.path.join(GOLDEN, name + '.npz'))
    kw = json.loads(str(z['model_kwargs_json']))
    ck = {'model_class': str(z['model_class']), 'model_kwargs': kw,
          'model_state_dict': {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith('sd/')}}
    return z, ck


def test_training_gradients_match_the_reference():
    """grad_dbvgo.npz: the reference's loss and its gradients of both density grids, both k0 grids and both rgbnets (bounds of
    test_dcvgo_gpu.py::test_training_gradients_match_the_reference); then one MaskedAdam step moves both density grids and leaves everything finite."""
    z, ck = _npz_checkpoint('grad_dbvgo')
    rk = json.loads(str(z['render_kwargs_json']))
    model = _model(ck)
    r = [torch.from_numpy(z['in/' + k]).cuda() for k in ('rays_o', 'rays_d', 'viewdirs')]
    with torch.enable_grad():
        out = model(*r, global_step=0, **rk)
        loss = F.mse_loss(out['rgb_marched'], torch.from_numpy(z['target']).cuda())
        loss.backward()
    assert abs(float(loss) - float(z['loss'])) <= 2e-6 * max(1.0, abs(float(z['loss'])))
    named = dict(model.named_parameters())
    grads = [k for k in z.files if k.startswith('grad/')]
    assert {'grad/density.0.grid', 'grad/density.1.grid', 'grad/k0.0.grid', 'grad/k0.1.grid'} <= set(grads)
    assert any(k.startswith('grad/rgbnet.0.') for k in grads) and any(k.startswith('grad/rgbnet.1.') for k in grads)
    for k in grads:
        assert named[k[5:]].grad is not None, k
        _close(named[k[5:]].grad, torch.from_numpy(z[k]), k)

    class Cfg(dict):
        __getattr__ = dict.__getitem__
    cfg = Cfg(lrate_decay=20, lrate_density=1e-1, lrate_k0=1e-1, lrate_rgbnet=1e-3, skip_zero_grad_fields=['density', 'k0'])
    before = [g.grid.detach().clone() for g in model.density]
    opt = utils.create_optimizer_or_freeze_model(model, cfg, global_step=0)
    assert isinstance(opt, MaskedAdam)
    opt.step()
    torch.cuda.synchronize()
    for i in range(2):
        assert not torch.equal(model.density[i].grid.detach(), before[i]), i
    assert all(torch.isfinite(p).all() for p in model.parameters())


def test_occupancy_maintenance_matches_the_reference():
    """occ_dbvgo.npz: update_occupancy_cache and scale_volume_grid (which REPLACES each mask, lib/dbvgo.py:170-185) against the reference: mask
    mismatch share <= 2e-3, grids within 2e-5, as for dcvgo; the grown model renders finite values on both paths."""
    z, ck = _npz_checkpoint('occ_dbvgo')
    model = _model(ck)
    with torch.no_grad():
        for i in range(2):
            model.density[i].grid += float(z['density_plus'])

    def same_mask(got, want, what):
        got = got.cpu().numpy()
        assert got.shape == want.shape, (what, got.shape, want.shape)
        assert float((got != want).mean()) <= 2e-3, (what, float((got != want).mean()))
    model.update_occupancy_cache()
    for i in range(2):
        same_mask(model.mask_cache[i].mask, z[f'upd/mask{i}'], f'update_occupancy_cache {i}')
    assert not np.array_equal(z['upd/mask0'], z['upd/mask1'])
    model.scale_volume_grid(int(z['new_num_voxels']))
    assert model.world_size.tolist() == z['scale/world_size'].tolist()
    for i in range(2):
        np.testing.assert_allclose(model.density[i].grid.detach().cpu().numpy(), z[f'scale/density{i}'], rtol=0, atol=2e-5)
        np.testing.assert_allclose(model.k0[i].grid.detach().cpu().numpy(), z[f'scale/k0{i}'], rtol=0, atol=2e-5)
        same_mask(model.mask_cache[i].mask, z[f'scale/mask{i}'], f'scale_volume_grid {i}')
    ro, rd, vd = _frame_rays(16, 16, 0)
    with torch.no_grad():
        for staged in (False, True):
            out = model(ro, rd, vd, stepsize=0.5, bg=1, render_depth=True, k4_staged=staged)
            assert torch.isfinite(out['rgb_marched']).all() and torch.isfinite(out['depth']).all()


def test_tensorf_grids_fused_equals_staged():
    """density_type / k0_type 'TensoRFGrid': the module's lookup when staged, the cached dense expansion when fused."""
    torch.manual_seed(5)
    nv = 24 ** 3
    model = dbvgo.DirectBiVoxGO(xyz_min=[-1.4, -1.55, -1.3], xyz_max=[1.6, 1.45, 1.7], num_voxels=nv, num_voxels_base=nv, alpha_init=1e-2,
                                fast_color_thres=1e-4, density_type='TensoRFGrid', k0_type='TensoRFGrid', density_config={'n_comp': 4},
                                k0_config={'n_comp': 6}, rgbnet_dim=6, rgbnet_width=32, viewbase_pe=2).cuda().eval()
    with torch.no_grad():
        for dg in model.density:
            for name in ('xy_plane', 'xz_plane', 'yz_plane'):
                getattr(dg, name).mul_(40.0)
    assert model._k4_fusable()
    ro, rd, vd = _frame_rays(24, 24, 2)
    with torch.no_grad():
        fused = model(ro, rd, vd, stepsize=0.5, bg=1, render_depth=True)
        staged = model(ro, rd, vd, stepsize=0.5, bg=1, render_depth=True, k4_staged=True)
    n = ro.shape[0]
    fg_ids = staged['ray_id']
    ds = 2 + int(np.sqrt(3) * 2 / (0.5 * float(model.voxel_size))) + 1 + model._n_outer(0.5)[1] - 1     # an upper bound of the largest depth value
    assert float((fused['alphainv_last'][:n] * fused['alphainv_last'][n:]).mean()) < 0.98 and fg_ids.numel() > 0
    for k in ('rgb_marched', 'depth', 'alphainv_last'):
        s = ds if k == 'depth' else 1.0
        assert float((fused[k] - staged[k]).abs().max()) <= 1e-5 * s, (k, float((fused[k] - staged[k]).abs().max()))


def test_unsupported_rgbnet_width_takes_the_staged_path():
    ck = scene.make_bivox_checkpoint(seed=3, num_voxels=20 ** 3, rgbnet_dim=3, rgbnet_width=48, viewbase_pe=2)
    model = _model(ck).eval()
    assert not model._k4_fusable()
    ro, rd, vd = _frame_rays(12, 12, 0)
    with torch.no_grad():
        out = model(ro, rd, vd, **ck['render_kwargs'])
    assert 'weights' in out and 'ray_id' in out and torch.isfinite(out['rgb_marched']).all()          # the staged path's keys
    want = bo.forward(ck['model_kwargs'], ck['model_state_dict'], ro.cpu(), rd.cpu(), vd.cpu(), bg_sampler='source', **ck['render_kwargs'])
    assert float((out['rgb_marched'].cpu() - want['rgb_marched']).abs().max()) < 1e-4
    # the library itself refuses the shape: K4_ERR_UNSUPPORTED, not a launch
    d = N.BivoxDesc()
    d.n_rays, d.n_outer, d.stepdist = 1, 4, 0.1
    d.rays_o = d.rays_d = d.viewdirs = d.xyz_min = d.xyz_max = d.rgb = d.depth = d.alphainv_fg = d.alphainv_bg = ro.data_ptr()
    d.width[0] = 48
    assert N.lib().k4_march_bivox_fwd(N.C.byref(d), N.stream()) == N.K4_ERR_UNSUPPORTED


def test_render_viewpoints_and_parameter_changes():
    ck = scene.make_bivox_checkpoint(seed=4, num_voxels=40 ** 3, rgbnet_dim=6, rgbnet_width=64)
    model = _model(ck).eval()
    H = W = 32
    K = scene.unbounded_K(H, W)
    poses = torch.from_numpy(scene.unbounded_poses()[:2])
    rk = dict(ck['render_kwargs'])
    rgbs, depths, bgmaps, psnrs, viewdirs_all, feats = render.render_viewpoints(model, poses, np.array([[H, W]] * 2), np.stack([K, K]),
                                                                               ndc=False, render_kwargs=rk)
    assert np.asarray(rgbs).shape == (2, H, W, 3) and np.asarray(depths).shape[:3] == (2, H, W) and np.asarray(bgmaps).shape == (2, H, W, 1)
    assert np.isfinite(np.asarray(rgbs)).all()
    ro, rd, vd = _frame_rays(H, W, 0)
    with torch.no_grad():
        out = model(ro, rd, vd, **rk)
    n = H * W
    T = (out['alphainv_last'][:n] * out['alphainv_last'][n:]).reshape(H, W, 1).cpu().numpy()
    assert np.array_equal(np.asarray(bgmaps)[0], T)                                     # the factor of `bg` in rgb_marched
    assert np.array_equal(np.asarray(rgbs)[0].reshape(-1, 3), out['rgb_marched'].cpu().numpy())
    # a second forward after in-place parameter changes sees the new values (the plan is keyed on versions)
    with torch.no_grad():
        model.density[1].grid += 2.0
        model.rgbnet[0][0].weight.mul_(0.5)
        again = model(ro, rd, vd, **rk)
        staged = model(ro, rd, vd, k4_staged=True, **rk)
    assert not torch.equal(again['rgb_marched'], out['rgb_marched'])
    assert float((again['rgb_marched'] - staged['rgb_marched']).abs().max()) <= 1e-5
    model.bg_preserve = 0.3
    with torch.no_grad():
        third = model(ro, rd, vd, **rk)
        staged3 = model(ro, rd, vd, k4_staged=True, **rk)
    assert not torch.equal(third['rgb_marched'], again['rgb_marched'])
    assert float((third['rgb_marched'] - staged3['rgb_marched']).abs().max()) <= 1e-5


def test_one_launch_with_more_than_64_survivors_on_a_ray_and_without_thresholds():
    """The twin of test_vq_gpu.py's test of this name on k_march_bivox.  fast_color_thres = 0 on two all-occupied masks: every in-box sample in
    front of the T < 1e-3 stop is shaded, so a ray queues more than 64 survivors -- the queue is flushed mid-ray and its rest moved -- and shades
    in its third 64-lane chunk (36^3 voxels, stepsize 0.25; 24x32 frame, width 32 in both passes).  Without a threshold every in-mask sample is
    kept, also behind the stop, and the background is walked whatever T_fg is: the last kept step of both passes enters depth.  The frame contract
    of tests/test_march_gpu.py between the one launch and the staged path (>= 99.9 % of the rays within 2e-5, every ray within 2e-3) on rgb,
    alphainv_last and depth -- depth, a weighted sum of step indices, on the scale of its formula (bivox_oracle.depth_scale) as everywhere in this
    file: fp32 does not resolve 2e-5 on values of several hundred; the same bits with and without counters; no weight filter: n_shade == n_alpha
    in both passes.
    Measured on an MI355X with the library of the commit before the shared walk: 175 weighted foreground samples on the fullest ray (last weighted
    step 174) and 63 background ones, 39 of 768 rays stop in the foreground, every ray has background survivors; 100 % of the rays within 2e-5
    for all three outputs, largest 1.5e-6 (rgb), 1.2e-6 of its scale 238 (depth), 8.3e-7 (alphainv_last); counters 103924 four times for the
    foreground, 48384 for the background."""
    ck = scene.make_bivox_checkpoint(seed=58, num_voxels=36 ** 3, rgbnet_dim=6, rgbnet_width=32, fast_color_thres=0, stepsize=0.25, n_blobs=5)
    for i in range(2):
        ck['model_state_dict'][f'mask_cache.{i}.mask'] = torch.ones_like(ck['model_state_dict'][f'mask_cache.{i}.mask'])
    model = _model(ck).eval()
    assert model._k4_fusable() and float(model.fast_color_thres) == 0
    ro, rd, vd = _frame_rays(24, 32, 1)
    n, rk = ro.shape[0], ck['render_kwargs']
    cnt = torch.zeros(8, dtype=torch.int64, device='cuda')
    with torch.no_grad():
        staged = model(ro, rd, vd, k4_staged=True, **rk)
        fused = model(ro, rd, vd, **rk)
        counted = model(ro, rd, vd, k4_counters=cnt, **rk)
        # the staged path's two passes one by one (_forward_staged's calls): steps and weights per pass
        pts, ray_id, step_id, outer = model.sample_ray(ori_rays_o=ro, ori_rays_d=rd, stepsize=rk['stepsize'])
        both = dict(viewdirs=vd, interval=rk['stepsize'] * model.voxel_size_ratio, N_=n)
        fg = model._forward(ray_pts=pts, mask_grid=model.mask_cache[0], density_grid=model.density[0], k0_grid=model.k0[0], rgbnet=model._rgbnet_of(0),
                            ray_id=ray_id, step_id=step_id, **both)
        bgp = model._forward(ray_pts=outer, mask_grid=model.mask_cache[1], density_grid=model.density[1], k0_grid=model.k0[1], rgbnet=model._rgbnet_of(1),
                             prev_alphainv_last=fg['alphainv_last'], **both)
    assert torch.equal(torch.cat([fg['weights'], bgp['weights']]), staged['weights'])
    T_fg = fg['alphainv_last']
    per_ray = [torch.bincount(p['ray_id'][p['weights'] > 0], minlength=n) for p in (fg, bgp)]
    last = [int(p['step_id'][p['weights'] > 0].max()) for p in (fg, bgp)]
    walked_bg = torch.bincount(bgp['ray_id'], minlength=n) > 0
    stops_fg = T_fg < 1e-3
    print(f'most weighted samples on a ray fg {int(per_ray[0].max())} bg {int(per_ray[1].max())}, last weighted step fg {last[0]} bg {last[1]}, '
          f'rays stopping in the foreground {int(stops_fg.sum())}, rays with background survivors {int((per_ray[1] > 0).sum())} of {n}')
    assert 'weights' not in fused and int(per_ray[0].max()) > 64 and max(last) >= 128
    assert int(stops_fg.sum()) > 0 and bool(walked_bg[stops_fg].all())          # T_fg <= 0 never holds: the background is walked behind a stop too
    assert int(((per_ray[1] > 0) & ~stops_fg).sum()) > 0
    ds = bo.depth_scale(ck['model_kwargs'], int(fg['step_id'].max()), rk['stepsize'])
    for k in ('rgb_marched', 'depth', 'alphainv_last'):
        s = ds if k == 'depth' else 1.0
        d = (fused[k] - staged[k]).abs() / s
        d = d.amax(-1) if d.dim() > 1 else d
        print(f'{k}: max|err| {float(d.max()):.3e} (scale {s}), within 2e-5: {float((d <= 2e-5).float().mean()):.5f}')
        assert float((d <= 2e-5).float().mean()) >= 0.999 and float(d.max()) <= 2e-3, (k, float(d.max()))
        assert torch.equal(fused[k], counted[k]), k
    c = cnt.cpu().tolist()
    print('counters', c)
    assert c[3] == c[2] > 0 and c[7] == c[6] > 0
