"""Scene preparation on the GPU (csrc/k4_prep.hip): the fused view count, the near-camera mask, the frustum box and the coarse-geometry box against
the reference's golden, the float64 oracle (tests/scene_prep_oracle.py) and the staged methods.

Tolerances.  The view count is compared EXACTLY on every voxel none of whose per-view float64 sums lies within 1e-3 of 1 (the fp32 sums deviate from
float64 by ~1e-5 at these shapes; tests/test_scene_prep_cpu.py holds the left-out share to <= 1 % per scene, and to zero on the golden).  Everything
else is ``torch.equal``: masks, boxes and indices are decisions on values that carry the staged path's bits."""
import numpy as np
import pytest
import torch

import nerf4k_amd  # noqa: F401
from nerf4k_amd import _native as N, scene, scene_prep
from nerf4k_amd.lib import dvgo as D, utils
from nerf4k_amd.lib.masked_adam import MaskedAdam
import scene_prep_oracle as O

pytestmark = pytest.mark.gpu


def _case_model(case):
    return D.DirectVoxGO(**O.dvgo_kwargs(case['extent_cells'])).cuda()


def _count_args(case, device='cpu'):
    return dict(rays_o_tr=torch.from_numpy(case['rays_o']).to(device), rays_d_tr=torch.from_numpy(case['rays_d']).to(device), imsz=case['imsz'],
                near=case['near'], far=6.0, stepsize=case['stepsize'], downrate=case['downrate'], irregular_shape=case['irregular_shape'])


@pytest.fixture(scope='module')
def golden():
    ck, rk, z = O.golden_occ()
    return dict(ck=ck, rk=rk, z=z, ro=torch.from_numpy(z['cnt/rays_o']), rd=torch.from_numpy(z['cnt/rays_d']))


def test_count_equals_the_reference_golden(golden):
    model = utils.model_from_checkpoint_dict(golden['ck']).cuda()
    rk, z = golden['rk'], golden['z']
    cnt = model.k4_voxel_count_views(golden['ro'], golden['rd'], [1, 1], near=rk['near'], far=rk['far'], stepsize=rk['stepsize'], downrate=1)
    assert cnt.shape == (1, 1, 12, 12, 12) and cnt.dtype == torch.float32 and cnt.is_cuda
    differ = int((cnt.cpu().numpy() != z['cnt/count']).sum())
    print(f'voxels that differ from the golden: {differ} of {cnt.numel()}')
    assert differ == 0


@pytest.mark.parametrize('name', O.COUNT_CASES)
def test_count_equals_the_oracle_and_the_staged_method(name):
    case = O.count_case(name)
    kw, world, sums = O.oracle_of_case(case)
    want, compared = O.count_and_band(sums)
    model = _case_model(case)
    assert model.world_size.tolist() == world
    fused = model.k4_voxel_count_views(**_count_args(case)).cpu().numpy()
    staged = model.voxel_count_views(**_count_args(case)).cpu().numpy()
    sel = compared[None, None]
    print(f'{name}: compared {int(compared.sum())} of {compared.size}; fused != oracle: {int((fused != want)[sel].sum())}; '
          f'staged != oracle: {int((staged != want)[sel].sum())}; fused != staged anywhere: {int((fused != staged).sum())}')
    assert np.array_equal(fused[sel], want[sel])
    assert np.array_equal(staged[sel], want[sel])
    if name == 'no_wrap_64x64_identical':                    # 4096 equal rays per view: one count per view wherever the ray passes
        assert set(np.unique(fused).tolist()) == {0.0, float(len(case['imsz']))} and compared.all()


def test_count_repeats_and_ignores_ray_order_and_ray_device():
    case = O.count_case('irregular_unequal_views_inside_camera')
    model = _case_model(case)
    a = model.k4_voxel_count_views(**_count_args(case))
    assert torch.equal(a, model.k4_voxel_count_views(**_count_args(case)))
    assert torch.equal(a, model.k4_voxel_count_views(**_count_args(case, 'cuda')))
    g = torch.Generator().manual_seed(3)
    starts = np.concatenate([[0], np.cumsum(case['imsz'])])
    perm = torch.cat([int(s) + torch.randperm(int(n), generator=g) for s, n in zip(starts[:-1], case['imsz'])])
    shuffled = dict(case, rays_o=case['rays_o'][perm.numpy()], rays_d=case['rays_d'][perm.numpy()])
    assert torch.equal(a, model.k4_voxel_count_views(**_count_args(shuffled)))
    regular = O.count_case('cubic_24x17_downrate2')          # [n, H, W, 3] tables on the device: the strided slice is taken there
    m2 = _case_model(regular)
    assert torch.equal(m2.k4_voxel_count_views(**_count_args(regular)), m2.k4_voxel_count_views(**_count_args(regular, 'cuda')))


def test_per_voxel_init_equals_the_staged_sequence(golden):
    rk = golden['rk']
    # the golden's two views, each given twice: counts reach 4, so `cnt <= 2` clears part of the mask and keeps the rest
    kw = dict(rays_o_tr=torch.cat([golden['ro']] * 2), rays_d_tr=torch.cat([golden['rd']] * 2), imsz=[1] * 4, near=rk['near'], far=rk['far'],
              stepsize=rk['stepsize'], downrate=1, irregular_shape=False)
    a = utils.model_from_checkpoint_dict(golden['ck']).cuda()
    opt_a = MaskedAdam([{'params': [a.density.grid], 'lr': 0.1, 'skip_zero_grad': True}])
    cnt = a.voxel_count_views(**kw)                          # run_sr.py:441-448 on the staged count
    opt_a.set_pervoxel_lr(cnt)
    a.mask_cache.mask[cnt.squeeze() <= 2] = False
    b = utils.model_from_checkpoint_dict(golden['ck']).cuda()
    opt_b = MaskedAdam([{'params': [b.density.grid], 'lr': 0.1, 'skip_zero_grad': True}])
    got = scene_prep.per_voxel_init(b, opt_b, **kw)
    assert torch.equal(got, cnt)
    assert torch.equal(opt_b.per_lr, opt_a.per_lr) and opt_b.per_lr.shape == cnt.shape
    assert torch.equal(b.mask_cache.mask, a.mask_cache.mask)
    assert 0 < int(b.mask_cache.mask.sum()) < b.mask_cache.mask.numel()


def test_near_mask_equals_the_golden_and_the_staged_method(golden):
    model = utils.model_from_checkpoint_dict(golden['ck']).cuda()
    version = model.density.grid._version
    model.k4_maskout_near_cam_vox(torch.tensor([[0.4, 0.3, 0.2], [-0.5, 0.1, 0.0]]), 0.35)
    assert model.density.grid._version > version
    want = golden['z']['near/density'] == -100
    assert 0 < want.sum() < want.size
    assert np.array_equal(model.density.grid.detach().cpu().numpy() == -100, want)
    # 150 cameras (more than one of the staged method's chunks of 100) on a non-cubic grid
    g = torch.Generator().manual_seed(5)
    cams = (torch.rand([150, 3], generator=g) * 2 - 1) * torch.tensor([1.4, 2.0, 1.6])
    kw = O.dvgo_kwargs((9.5, 14.5, 11.5))
    a, b = D.DirectVoxGO(**kw).cuda(), D.DirectVoxGO(**kw).cuda()
    with torch.no_grad():
        a.density.grid.copy_(torch.randn(a.density.grid.shape, generator=g))
        b.density.grid.copy_(a.density.grid)
    a.maskout_near_cam_vox(cams, 0.3)
    b.k4_maskout_near_cam_vox(cams, 0.3)
    hit = float((a.density.grid == -100).float().mean())
    print(f'nodes within 0.3 of a camera: {hit:.3f}')
    assert 0.05 < hit < 0.95
    assert torch.equal(a.density.grid, b.density.grid)


def test_near_mask_raises_for_a_factored_density():
    model = D.DirectVoxGO(density_type='TensoRFGrid', density_config={'n_comp': 2}, **O.dvgo_kwargs((6.5, 6.5, 6.5))).cuda()
    with pytest.raises(NotImplementedError):
        model.k4_maskout_near_cam_vox(torch.zeros(1, 3), 0.1)


def _staged_frustum(HW, Ks, poses, idx, ts, ndc, inverse_y, flip_x, flip_y, use_viewdirs):
    """The package's get_rays_of_a_view (device pose) and the min / max over every point o + dir * t of every view."""
    lo, hi = torch.full([3], float('inf')), torch.full([3], -float('inf'))
    for i in idx:
        ro, rd, vd = D.get_rays_of_a_view(int(HW[i][0]), int(HW[i][1]), Ks[i], poses[i].cuda(), ndc, inverse_y=inverse_y, flip_x=flip_x, flip_y=flip_y)
        pts = torch.stack([ro + (vd if use_viewdirs else rd) * t for t in ts])
        lo, hi = torch.minimum(lo, pts.amin((0, 1, 2)).cpu()), torch.maximum(hi, pts.amax((0, 1, 2)).cpu())
    return lo, hi


def test_frustum_bounds_ndc_llff():
    H, W = 24, 32
    K = scene.LLFF_K.copy()
    K[:2] *= W / scene.LLFF_HW[1]
    poses = torch.from_numpy(scene.llff_spiral_poses())
    idx = [2, 7, 11]
    HW, Ks = np.array([[H, W]] * len(poses)), np.stack([K] * len(poses))
    flags = dict(ndc=True, inverse_y=False, flip_x=False, flip_y=False)
    lo, hi = scene_prep.compute_bbox_by_cam_frustrm(HW, Ks, poses, idx, 0.0, 1.0, **flags)
    assert not lo.is_cuda and lo.dtype == torch.float32 and lo.shape == (3,)
    want = _staged_frustum(HW, Ks, poses, idx, [0.0, 1.0], use_viewdirs=False, **flags)
    print('ndc box', lo.tolist(), hi.tolist())
    assert torch.equal(lo, want[0]) and torch.equal(hi, want[1])


def test_frustum_bounds_views_of_two_sizes_with_flips():
    sizes = [(20, 20), (24, 17), (20, 20), (13, 31)]
    poses = torch.stack([torch.from_numpy(scene.lego_pose(theta_deg=t, phi_deg=p)) for t, p in ((30, -30), (140, -10), (250, -50), (-60, -20))])
    HW, Ks = np.array(sizes), np.stack([scene.lego_K(h, w) for h, w in sizes])
    idx = [0, 1, 3]
    flags = dict(ndc=False, inverse_y=True, flip_x=True, flip_y=False)
    lo, hi = scene_prep.compute_bbox_by_cam_frustrm(HW, Ks, poses, idx, 2.0, 6.0, **flags)
    want = _staged_frustum(HW, Ks, poses, idx, [2.0, 6.0], use_viewdirs=True, **flags)
    print('bounded box', lo.tolist(), hi.tolist())
    assert torch.equal(lo, want[0]) and torch.equal(hi, want[1])
    assert (hi - lo).min() > 1


def test_frustum_bounds_unbounded():
    H, W = 18, 26
    poses = torch.from_numpy(scene.unbounded_poses(n_frames=5))
    HW, Ks = np.array([[H, W]] * 5), np.stack([scene.unbounded_K(H, W)] * 5)
    idx = [0, 1, 2, 4]
    flags = dict(ndc=False, inverse_y=False, flip_x=False, flip_y=False)
    lo, hi = scene_prep.compute_bbox_by_cam_frustrm(HW, Ks, poses, idx, 0.0, 1.0, unbounded_inward=True, unbounded_inner_r=0.8, near_clip=0.2, **flags)
    pmin, pmax = _staged_frustum(HW, Ks, poses, idx, [0.2], use_viewdirs=False, **flags)
    center = (pmin + pmax) * 0.5                                              # run_sr.py:250-253 on the six numbers
    radius = (center - pmin).max() * 0.8
    print('unbounded cube', lo.tolist(), hi.tolist())
    assert torch.equal(lo, center - radius) and torch.equal(hi, center + radius)


def _geo_model(name):
    extent, seed, thres = O.GEO_CASES[name]
    model = D.DirectVoxGO(**O.dvgo_kwargs(extent)).cuda()
    with torch.no_grad():
        model.density.grid.copy_(torch.from_numpy(O.geo_density(model.world_size.tolist(), seed))[None, None])
    return model, thres


def _staged_geo(model, thres):
    """run_sr.py:275-286 on the staged ops: density looked up at the node positions, activate_density, the mask, amin / amax."""
    dev = model.xyz_min.device
    interp = torch.stack(torch.meshgrid(*[torch.linspace(0, 1, int(n), device=dev) for n in model.world_size], indexing='ij'), -1)
    dense_xyz = model.xyz_min * (1 - interp) + model.xyz_max * interp
    with torch.no_grad():
        alpha = model.activate_density(model.density(dense_xyz))
    active = dense_xyz[alpha > thres]
    return active.amin(0), active.amax(0)


@pytest.mark.parametrize('name', sorted(O.GEO_CASES))
def test_coarse_geo_bounds_equal_the_staged_composition(name):
    model, thres = _geo_model(name)
    lo, hi = scene_prep.coarse_geo_bounds(model, thres)
    want = _staged_geo(model, thres)
    idx, _ = O.geo_oracle(model.density.grid.detach().cpu().numpy()[0, 0], float(model.act_shift), float(model.voxel_size_ratio), thres)
    print(f'{name}: box {lo.tolist()} .. {hi.tolist()}, node indices {idx}')
    assert torch.equal(lo, want[0]) and torch.equal(hi, want[1])
    assert (lo > model.xyz_min).all() and (hi < model.xyz_max).all()
    with pytest.raises(ValueError):
        scene_prep.coarse_geo_bounds(model, 2.0)


def test_compute_bbox_by_coarse_geo_round_trips_through_a_checkpoint(tmp_path):
    model, thres = _geo_model('noncubic_9x14x11')
    path = str(tmp_path / 'coarse_last.tar')
    torch.save({'global_step': 0, 'model_kwargs': model.get_kwargs(), 'model_state_dict': model.state_dict()}, path)
    lo, hi = scene_prep.compute_bbox_by_coarse_geo(D.DirectVoxGO, path, thres)
    want = scene_prep.coarse_geo_bounds(model, thres)
    assert torch.equal(lo, want[0]) and torch.equal(hi, want[1])


def test_cpu_model_raises_on_a_gpu_machine(golden):
    model = utils.model_from_checkpoint_dict(golden['ck'])
    with pytest.raises(N.K4Error):
        model.k4_voxel_count_views(golden['ro'], golden['rd'], [1, 1], near=2.0, far=6.0, stepsize=0.5)
