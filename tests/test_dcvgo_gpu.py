"""DirectContractedVoxGO (nerf4k_amd.lib.dcvgo) on the MI355X: the staged HIP path against the reference-made goldens
(tests/gen_contracted_golden.py) and the CPU oracle (tests/contracted_oracle.py), k4_cumdist_thres against the sequential scan, training
gradients, occupancy maintenance, the render loop and the joint step's weight_nearclip term."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import nerf4k_amd  # noqa: F401
from nerf4k_amd import scene, render, joint_train
from nerf4k_amd.lib import dcvgo, utils, sr_esrnet
from helpers import GOLDEN, load_march_golden, psnr
import contracted_oracle as co

pytestmark = pytest.mark.gpu
GOLD = ['march_dcvgo_inf', 'march_dcvgo_l2', 'march_dcvgo_coarse', 'march_dcvgo_coarse_l2']
KEYS = ('rgb_marched', 'depth', 'alphainv_last', 'wsum_mid', 'weights', 'raw_density', 'raw_alpha', 'raw_rgb', 't', 's')


def _model(ck):
    return utils.model_from_checkpoint_dict(ck).cuda()


def _close(got, want, name, rel=2e-5):
    got, want = got.detach().cpu().double(), want.double()
    assert got.shape == want.shape, (name, got.shape, want.shape)
    err = float((got - want).abs().max()) if got.numel() else 0.0
    assert err <= rel * float(want.abs().max() if want.numel() else 0) + 1e-9, (name, err)


@pytest.mark.parametrize('name', GOLD)
def test_golden_staged_every_key(name):
    g = load_march_golden(name)
    model = _model(g).eval()
    r = {k: v.cuda() for k, v in g['rays'].items()}
    with torch.no_grad():
        out = model(r['rays_o'], r['rays_d'], r['viewdirs'], k4_staged=True, **g['render_kwargs'])
    ref = g['out']
    assert set(out) == set(ref) | {'rgb_feature'}, set(out) ^ set(ref)
    assert out['rgb_feature'] is out['rgb_marched'] and out['n_max'] == int(ref['n_max'])
    assert torch.equal(out['ray_id'].cpu(), ref['ray_id'].long()) and torch.equal(out['step_id'].cpu(), ref['step_id'].long())
    for k in KEYS:
        # raw_density is a trilinear blend of grid values up to ~30: the HIP lookup and PyTorch's CPU grid_sample round the eight products in
        # another order, ~2 ulp of the CORNER values (3e-6 relative to the densest voxel); weights / depth carry that on
        atol = 3e-6 * float(g['model_state_dict']['density.grid'].abs().max()) if k == 'raw_density' else 1e-5
        assert psnr(out[k].cpu(), ref[k]) >= 80, (name, k)
        assert torch.allclose(out[k].cpu(), ref[k], rtol=0, atol=atol), (name, k, float((out[k].cpu() - ref[k]).abs().max()))


@pytest.mark.parametrize('name', GOLD)
def test_golden_fused(name):
    """The one-launch inference path (k4_march_contracted_fwd) on every golden scene: the reference's rgb_marched / depth / alphainv_last,
    and the staged path's to the order of the final sums."""
    g = load_march_golden(name)
    model = _model(g).eval()
    assert model._k4_fusable()
    r = {k: v.cuda() for k, v in g['rays'].items()}
    with torch.no_grad():
        fused = model(r['rays_o'], r['rays_d'], r['viewdirs'], **g['render_kwargs'])
        staged = model(r['rays_o'], r['rays_d'], r['viewdirs'], k4_staged=True, **g['render_kwargs'])
    assert set(fused) == {'alphainv_last', 'rgb_marched', 'rgb_feature', 'depth'} and fused['rgb_feature'] is fused['rgb_marched']
    for k in ('rgb_marched', 'depth', 'alphainv_last'):
        assert psnr(fused[k].cpu(), g['out'][k]) >= 80, (name, k)
        assert torch.allclose(fused[k].cpu(), g['out'][k], rtol=0, atol=1e-5), (name, k, float((fused[k].cpu() - g['out'][k]).abs().max()))
        # (the two paths agree to the golden's tolerance: d / |d| and the l2 norm are one rounded sum of squares here, torch's reduction there)
        assert torch.allclose(fused[k], staged[k], rtol=0, atol=1e-5), (name, k, float((fused[k] - staged[k]).abs().max()))


def _seq_cumdist(d, thres):
    t32 = np.float32(thres)
    out = np.zeros(d.shape, dtype=bool)
    for r in range(d.shape[0]):
        c = np.float32(0)
        for i in range(d.shape[1]):
            c = np.float32(c + d[r, i])
            out[r, i] = c > t32
            c = np.float32(c * np.float32(not out[r, i]))
    return out


def test_cumdist_thres_is_the_sequential_scan_exactly():
    g = torch.Generator().manual_seed(11)
    d = (torch.rand([301, 257], generator=g) * 0.03).float()
    d[0, :] = 0.25                       # 0.25 + 0.25 = 0.5 == thres exactly: not over; the third add crosses
    d[1, :] = 0.125                      # partial sums hit the threshold exactly on every 4th step
    d[2, ::2] = 0.0
    d[3, :] = float('inf')
    d[4, :] = 0.0
    thres = 0.5
    d[5:] *= 20                          # mixed: resets every one to a few steps
    got = dcvgo.ub360_utils_cuda.cumdist_thres(d.cuda(), thres).cpu().numpy()
    want = _seq_cumdist(d.numpy(), thres)
    assert np.array_equal(got, want), int((got != want).sum())
    assert np.array_equal(got, co.cumdist_thres(d, thres).numpy())
    assert not got[0, 1] and got[0, 2] and not got[1, 3] and got[1, 4]
    # the thresholds the model uses, on a model's own distance table
    ck = scene.make_unbounded_checkpoint(seed=3, num_voxels=48 ** 3, rgbnet_dim=0)
    model = _model(ck)
    ro, rd, _ = _frame_rays(24, 24, 2)
    pts, _, _ = model.sample_ray(ori_rays_o=ro, ori_rays_d=rd, stepsize=0.5)
    dist = (pts[:, 1:] - pts[:, :-1]).norm(dim=-1)
    th = (2 + 2 * model.bg_len) / model.world_len * 0.5 * 0.95
    assert np.array_equal(dcvgo.ub360_utils_cuda.cumdist_thres(dist, th).cpu().numpy(), _seq_cumdist(dist.cpu().numpy(), th))
    assert dcvgo.ub360_utils_cuda.cumdist_thres(torch.zeros([0, 5], device='cuda'), 0.1).shape == (0, 5)


def _frame_rays(H, W, pose_i):
    from nerf4k_amd.lib import dvgo
    pose = torch.from_numpy(scene.unbounded_poses()[pose_i]).cuda()
    ro, rd, vd = dvgo.get_rays_of_a_view(H, W, scene.unbounded_K(H, W), pose, False, inverse_y=False, flip_x=False, flip_y=False)
    return ro.reshape(-1, 3), rd.reshape(-1, 3), vd.reshape(-1, 3)


FRAMES = [dict(seed=51, num_voxels=96 ** 3, contracted_norm='inf', rgbnet_dim=12, rgbnet_width=128),
          dict(seed=52, num_voxels=80 ** 3, contracted_norm='l2', rgbnet_dim=6, rgbnet_width=64, fast_color_thres=1e-3),
          dict(seed=53, num_voxels=64 ** 3, contracted_norm='inf', rgbnet_dim=0)]


def frame_errors(cfg):
    """64x64 frame of a seeded scene: fused, staged and the CPU oracle -> (outputs, oracle, oracle counters, fused counters)."""
    ck = scene.make_unbounded_checkpoint(**cfg)
    model = _model(ck).eval()
    ro, rd, vd = _frame_rays(64, 64, 1)
    cnt_dev = torch.zeros(8, dtype=torch.int64, device='cuda')
    with torch.no_grad():
        fused = model(ro, rd, vd, k4_counters=cnt_dev, **ck['render_kwargs'])
        fused_plain = model(ro, rd, vd, **ck['render_kwargs'])
        staged = model(ro, rd, vd, k4_staged=True, **ck['render_kwargs'])
    cnt = {}
    want = co.forward(ck['model_kwargs'], ck['model_state_dict'], ro.cpu(), rd.cpu(), vd.cpu(), counters=cnt, **ck['render_kwargs'])
    return fused, fused_plain, staged, want, cnt, cnt_dev.cpu().tolist()


@pytest.mark.parametrize('cfg', FRAMES)
def test_frame_vs_oracle(cfg):
    """A 64x64 frame of a larger seeded scene, fused and staged, against the CPU oracle: >= 80 dB, and 99.8 % of rays within 2e-5 with
    every ray within 1e-4.  test_dvgo_frame_vs_oracle asks 99.9 %; measured here (both paths alike, so the arithmetic they share and not
    the fused kernel): seed 51 (96^3, 12 channels, width 128) 99.854 % of rays within 2e-5, largest 6.0e-5, 113.7 dB; seeds 52 / 53
    100 % / 99.95 %.  The density lookups round trilinear blends of values up to ~30 in another order than PyTorch's CPU grid_sample and
    ~200 samples per ray carry that through alpha and T.  The fused sample counters equal the oracle's within the tie tolerance; fused ==
    staged to the order of the final sums."""
    fused, fused_plain, staged, want, cnt, cd = frame_errors(cfg)
    for tag, out in (('fused', fused), ('staged', staged)):
        for k in ('rgb_marched', 'depth', 'alphainv_last'):
            a, b = out[k].cpu(), want[k]
            assert psnr(a, b) >= 80, (tag, k, psnr(a, b))
            err = (a - b).abs().reshape(a.shape[0], -1).amax(-1)
            assert float((err <= 2e-5).float().mean()) >= 0.998 and float(err.max()) <= 1e-4, \
                (tag, k, float(err.max()), float((err <= 2e-5).float().mean()))
    for k in ('rgb_marched', 'depth', 'alphainv_last'):
        assert torch.equal(fused[k], fused_plain[k]), k                     # counting does not change the result
        assert torch.allclose(fused[k], staged[k], rtol=0, atol=2e-5), (k, float((fused[k] - staged[k]).abs().max()))
    tol = lambda n: max(2, n // 10000)
    for i, key in enumerate(('n_pre', 'n_mask', 'n_alpha', 'n_shade')):
        assert abs(cd[i] - cnt[key]) <= tol(cnt[key]), (key, cd[:4], cnt)
    assert abs(staged['ray_id'].shape[0] - cnt['n_shade']) <= tol(cnt['n_shade'])
    assert float(fused['alphainv_last'].mean()) < 0.98          # the scene is not empty


def test_training_gradients_match_the_reference():
    z = np.load(os.path.join(GOLDEN, 'grad_dcvgo.npz'))
    kw = json.loads(str(z['model_kwargs_json']))
    ck = {'model_class': str(z['model_class']), 'model_kwargs': kw,
          'model_state_dict': {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith('sd/')}}
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
    assert {'grad/density.grid', 'grad/k0.grid'} <= set(grads) and any(k.startswith('grad/rgbnet') for k in grads)
    for k in grads:
        assert named[k[5:]].grad is not None, k
        _close(named[k[5:]].grad, torch.from_numpy(z[k]), k)


def test_occupancy_maintenance_matches_the_reference():
    z = np.load(os.path.join(GOLDEN, 'occ_dcvgo.npz'))
    kw = json.loads(str(z['model_kwargs_json']))
    ck = {'model_class': str(z['model_class']), 'model_kwargs': kw,
          'model_state_dict': {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith('sd/')}}
    model = _model(ck)
    with torch.no_grad():
        model.density.grid += float(z['density_plus'])

    def same_mask(got, want, what):
        got = got.cpu().numpy()
        assert got.shape == want.shape, (what, got.shape, want.shape)
        assert float((got != want).mean()) <= 2e-3, (what, float((got != want).mean()))
    model.update_occupancy_cache()
    same_mask(model.mask_cache.mask, z['upd/mask'], 'update_occupancy_cache')
    model.scale_volume_grid(int(z['new_num_voxels']))
    assert model.world_size.tolist() == z['scale/world_size'].tolist()
    np.testing.assert_allclose(model.density.grid.detach().cpu().numpy(), z['scale/density'], rtol=0, atol=2e-5)
    np.testing.assert_allclose(model.k0.grid.detach().cpu().numpy(), z['scale/k0'], rtol=0, atol=2e-5)
    same_mask(model.mask_cache.mask, z['scale/mask'], 'scale_volume_grid')
    # lt_nviews: every voxel no view samples is cleared; the grown model still renders
    ro, rd, _ = _frame_rays(16, 16, 0)
    before = int(model.mask_cache.mask.sum())
    model.update_occupancy_cache_lt_nviews(ro, rd, [ro.shape[0]], dict(stepsize=0.5), 1)
    assert 0 < int(model.mask_cache.mask.sum()) <= before
    with torch.no_grad():
        out = model(ro, rd, rd / rd.norm(dim=-1, keepdim=True), stepsize=0.5, bg=1, render_depth=True)
    assert torch.isfinite(out['rgb_marched']).all()


def test_render_viewpoints_and_fast_color_thres_schedule():
    ck = scene.make_unbounded_checkpoint(seed=61, num_voxels=48 ** 3, rgbnet_dim=6, rgbnet_width=64)
    model = _model(ck).eval()
    H, W = 24, 32
    K = scene.unbounded_K(H, W)
    poses = torch.from_numpy(scene.unbounded_poses()[:2])
    rk = dict(ck['render_kwargs'])
    rgbs, depths, bgmaps, psnrs, viewdirs_all, feats = render.render_viewpoints(model, poses, np.array([[H, W]] * 2), np.stack([K, K]),
                                                                               ndc=False, render_kwargs=rk)
    assert np.asarray(rgbs).shape == (2, H, W, 3) and np.isfinite(np.asarray(rgbs)).all()
    ro, rd, vd = _frame_rays(H, W, 0)
    want = co.forward(ck['model_kwargs'], ck['model_state_dict'], ro.cpu(), rd.cpu(), vd.cpu(), **rk)
    assert float(np.abs(np.asarray(rgbs)[0].reshape(-1, 3) - want['rgb_marched'].numpy()).max()) < 1e-4
    # fast_color_thres as a {global_step: value} schedule (lib/dcvgo.py:47-53,269-271)
    m2 = dcvgo.DirectContractedVoxGO(**dict(ck['model_kwargs'], fast_color_thres={0: 0, 5: 1e-2}))
    m2.load_state_dict(ck['model_state_dict'])
    m2 = m2.cuda()
    with torch.no_grad():
        a = m2(ro, rd, vd, global_step=1, k4_staged=True, **rk)
        assert m2.fast_color_thres == 0
        b = m2(ro, rd, vd, global_step=5, k4_staged=True, **rk)
    assert m2.fast_color_thres == 1e-2 and b['ray_id'].shape[0] < a['ray_id'].shape[0]


def _joint_setup(weight_nearclip, weight_distortion, near_clip):
    ck = scene.make_unbounded_checkpoint(seed=71, num_voxels=40 ** 3, rgbnet_dim=6, rgbnet_width=32, viewbase_pe=2, fast_color_thres=1e-4)
    model = _model(ck)
    from oracle import sr as osr
    net = sr_esrnet.SFTNet(3, scale=4, num_feat=64, num_block=1, num_grow_ch=32, num_cond=1)
    net.load_state_dict(osr.make_state_dict(seed=3, num_block=1))
    net = net.cuda().train()
    pr = pc = 8
    ro, rd, vd = _frame_rays(pr, pc, 3)
    g = torch.Generator().manual_seed(9)
    target = torch.rand([pr * pc, 3], generator=g).cuda()
    target_4x = torch.rand([16 * pr * pc, 3], generator=g).cuda()
    cfg = joint_train.JointCfg.fern_lg_joint_l1(weight_nearclip=weight_nearclip, weight_distortion=weight_distortion, N_rand=pr * pc, N_patch=1)
    rk = dict(ck['render_kwargs'], rand_bkgd=True)
    tr = joint_train.JointTrainer(model, net, cfg, rk, n_train_images=4, near_clip=near_clip)
    return model, tr, (ro, rd, vd, target, target_4x, pr, pc)


def test_weight_nearclip_gradient_is_the_reference_expression():
    near_clip = 0.9
    model, tr, batch = _joint_setup(1.0, 0.0, near_clip)
    with torch.enable_grad():
        rr = model(*batch[:3], global_step=0, is_train=True, **tr.render_kwargs)
        rgb_sr = torch.zeros([1, 3, 4 * batch[5], 4 * batch[6]], device='cuda', requires_grad=True)
        ls = tr.losses(rr, rgb_sr, batch[3], batch[4], batch[5], batch[6], batch[0].shape[0])
        assert 'nearclip' in ls and float(ls['nearclip']) == 0.0
        g, = torch.autograd.grad(ls['nearclip'], rr['raw_density'])
    near = (rr['t'] < near_clip / float(model.scene_radius[0])).float()
    assert near.sum() > 0
    assert torch.equal(g, near * 1.0)
    # without near_clip, or on a model without 't', the term raises
    model2, tr2, _ = _joint_setup(1.0, 0.0, None)
    with pytest.raises(ValueError):
        tr2.losses(rr, rgb_sr, batch[3], batch[4], batch[5], batch[6], batch[0].shape[0])
    rr_no_t = {k: v for k, v in rr.items() if k != 't'}
    with pytest.raises(ValueError):
        tr.losses(rr_no_t, rgb_sr, batch[3], batch[4], batch[5], batch[6], batch[0].shape[0])


def test_joint_step_with_nearclip_and_distortion():
    model, tr, batch = _joint_setup(0.5, 0.01, 0.9)
    before = {k: v.detach().clone() for k, v in model.named_parameters()}
    hist = [tr.step(*batch, global_step=1 + i) for i in range(2)]
    for ls in hist:
        for k in ('total', 'distortion', 'nearclip'):
            assert k in ls and np.isfinite(float(ls[k])), (k, ls.get(k))
    changed = [k for k, v in model.named_parameters() if not torch.equal(v.detach(), before[k])]
    assert 'density.grid' in changed and 'k0.grid' in changed and any(k.startswith('rgbnet') for k in changed), changed
    # distortion_loss of the module is the joint loop's term
    with torch.enable_grad():
        rr = model(*batch[:3], global_step=0, is_train=True, **tr.render_kwargs)
        a = dcvgo.distortion_loss(rr['weights'], rr['s'], rr['n_max'], rr['ray_id'])
        a.backward()
    assert torch.isfinite(a) and model.density.grid.grad is not None


def test_one_launch_with_more_than_64_survivors_on_a_ray_and_without_thresholds():
    """The twin of test_vq_gpu.py's test of this name on k_march_contracted.  fast_color_thres = 0 on an all-occupied mask: every sample that passes
    inner | cumdist in front of the T < 1e-3 stop is shaded, so a ray queues more than 64 survivors -- the queue is flushed mid-ray and its rest
    moved -- and shades in its third 64-lane chunk (36^3 voxels, stepsize 0.25: 242 steps per ray; 24x32 frame, width 32).  The frame contract of
    tests/test_march_gpu.py between the one launch and the staged path (>= 99.9 % of the rays within 2e-5, every ray within 2e-3), depth included;
    the same bits with and without counters; no weight filter: n_shade == n_alpha.
    Measured on an MI355X with the library of the commit before the shared walk: 167 weighted samples on the fullest ray, last weighted step 241 of
    242; 100 % of the 768 rays within 2e-5 for all three outputs, largest 9.5e-7 (rgb), 1.1e-6 (depth), 1.6e-6 (alphainv_last); counters
    106968 four times."""
    ck = scene.make_unbounded_checkpoint(seed=57, num_voxels=36 ** 3, rgbnet_dim=6, rgbnet_width=32, fast_color_thres=0, stepsize=0.25, n_blobs=4)
    ck['model_state_dict']['mask_cache.mask'] = torch.ones_like(ck['model_state_dict']['mask_cache.mask'])
    model = _model(ck).eval()
    assert model._k4_fusable() and float(model.fast_color_thres) == 0
    ro, rd, vd = _frame_rays(24, 32, 1)
    cnt = torch.zeros(4, dtype=torch.int64, device='cuda')
    with torch.no_grad():
        staged = model(ro, rd, vd, k4_staged=True, **ck['render_kwargs'])
        fused = model(ro, rd, vd, **ck['render_kwargs'])
        counted = model(ro, rd, vd, k4_counters=cnt, **ck['render_kwargs'])
    live = staged['weights'] > 0                                  # (the staged path keeps the zero-weight samples behind the stop)
    per_ray = torch.bincount(staged['ray_id'][live], minlength=ro.shape[0])
    last = int(staged['step_id'][live].max())
    print(f'most weighted samples on a ray {int(per_ray.max())}, last weighted step {last} of {staged["n_max"]}')
    assert 'weights' not in fused and int(per_ray.max()) > 64 and last >= 128
    for k in ('rgb_marched', 'depth', 'alphainv_last'):
        d = (fused[k] - staged[k]).abs()
        d = d.amax(-1) if d.dim() > 1 else d
        print(f'{k}: max|err| {float(d.max()):.3e}, within 2e-5: {float((d <= 2e-5).float().mean()):.5f}')
        assert float((d <= 2e-5).float().mean()) >= 0.999 and float(d.max()) <= 2e-3, (k, float(d.max()))
        assert torch.equal(fused[k], counted[k]), k
    c = cnt.cpu().tolist()
    print('counters', c)
    assert c[3] == c[2] > 0 and c[0] >= c[1] >= c[2]
