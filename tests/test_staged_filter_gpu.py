"""The staged sample filter and shading step the voxel-grid models share (lib/dvgo._VoxGOCommon._k4_filter_samples / _k4_shade) on the MI355X:
every tensor they return, bit for bit, against the reference's statements written out here with boolean-mask indexing on the same inputs --
DirectVoxGO (the filter called directly), DirectBiVoxGO (a background pass through ``_forward``), DirectContractedVoxGO (the filter with its
three extra columns) and DirectMPIGO (``k4_presel=False``).  Tiny shapes: 7 rays, 8^3 voxels.  Each case first makes sure that every filter it
runs both drops and keeps samples (the random density is scaled up until it does), so that a filter that passes everything cannot pass."""
import pytest
import torch

import nerf4k_amd  # noqa: F401
from nerf4k_amd.lib import dbvgo, dcvgo, dmpigo, dvgo

pytestmark = pytest.mark.gpu
N_RAYS = 7
SCALES = (2.0, 4.0, 8.0, 16.0, 32.0, 64.0, 128.0, 256.0)


@pytest.fixture(autouse=True)
def _no_grad():
    with torch.no_grad():
        yield


def _randomise(model, seed, scale):
    """Random densities (times ``scale``), colour features and occupancy masks, the same for the same seed."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in dvgo._each(model.density):
            m.grid.copy_(torch.randn(m.grid.shape, generator=g) * scale)
        for m in dvgo._each(model.k0):
            m.grid.copy_(torch.randn(m.grid.shape, generator=g))
        for m in dvgo._each(model.mask_cache):
            m.mask.copy_(torch.rand(m.mask.shape, generator=g) > 0.3)
    return model


def _rays(seed, z0=-3.0):
    """7 rays from around (0, 0, z0) through the unit cube around the origin."""
    g = torch.Generator().manual_seed(seed)
    o = torch.tensor([0., 0., z0]) + (torch.rand([N_RAYS, 3], generator=g) - 0.5) * 0.6
    d = (torch.rand([N_RAYS, 3], generator=g) - 0.5) * 1.2 - o
    return o.cuda(), d.cuda(), (d / d.norm(dim=-1, keepdim=True)).cuda()


def _reference_filter(ray_pts, ray_id, cols, interval, n_rays, mask_grid, density_of, shift, thres):
    """The reference's statements (lib/dvgo.py:352-378, lib/dbvgo.py:264-292, lib/dcvgo.py:306-328, lib/dmpigo.py:311-333): one boolean-mask
    indexing per tensor and filter.  ``cols``: name -> per-sample tensor.  -> (the filtered tensors by name, the masks of the filters that ran)."""
    cols = dict(cols)
    mask1 = mask_grid(ray_pts)
    ray_pts = ray_pts[mask1]
    ray_id = ray_id[mask1]
    cols = {k: v[mask1] for k, v in cols.items()}
    density = density_of(ray_pts)
    alpha = dvgo.Raw2Alpha.apply(density.flatten(), shift, interval).reshape(density.shape)
    masks = [mask1]
    if thres > 0:
        mask2 = (alpha > thres)
        ray_pts = ray_pts[mask2]
        ray_id = ray_id[mask2]
        density = density[mask2]
        alpha = alpha[mask2]
        cols = {k: v[mask2] for k, v in cols.items()}
        masks.append(mask2)
    weights, alphainv_last = dvgo.Alphas2Weights.apply(alpha, ray_id, n_rays)
    if thres > 0:
        mask3 = (weights > thres)
        ray_pts = ray_pts[mask3]
        ray_id = ray_id[mask3]
        density = density[mask3]
        alpha = alpha[mask3]
        weights = weights[mask3]
        cols = {k: v[mask3] for k, v in cols.items()}
        masks.append(mask3)
    return dict(cols, ray_pts=ray_pts, ray_id=ray_id, density=density, alpha=alpha, weights=weights, alphainv_last=alphainv_last), masks


def _drops_and_keeps(masks):
    return all(bool(m.any()) and not bool(m.all()) for m in masks)


def _scaled_until_every_filter_bites(make_model, seed, reference):
    """The model at the first density scale at which every filter of ``reference(model) -> (tensors, masks)`` both drops and keeps samples."""
    for scale in SCALES:
        model = _randomise(make_model(), seed, scale).cuda()
        want, masks = reference(model)
        if _drops_and_keeps(masks):
            break
    assert _drops_and_keeps(masks), [(int(m.sum()), m.numel()) for m in masks]
    print('density scale', scale, 'kept / of per filter', [(int(m.sum()), m.numel()) for m in masks])
    return model, want, masks


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    assert torch.equal(got, want), what


def _view_emb(viewdirs, viewfreq, ray_id):
    emb = (viewdirs.unsqueeze(-1) * viewfreq).flatten(-2)
    emb = torch.cat([viewdirs, emb.sin(), emb.cos()], -1)
    return emb.flatten(0, -2)[ray_id]


VOX = dict(xyz_min=[-1., -1., -1.], xyz_max=[1., 1., 1.], num_voxels=8 ** 3, num_voxels_base=8 ** 3, alpha_init=1e-2)


@pytest.mark.parametrize('thres', [0, 1e-2])
def test_dvgo_filter_called_directly(thres):
    ro, rd, vd = _rays(11)
    stepsize = 0.5

    def inputs(model):
        ray_pts, ray_id, step_id, _, _ = model.sample_ray(rays_o=ro, rays_d=rd, near=0.2, far=1e9, stepsize=stepsize)
        return ray_pts, ray_id, step_id, stepsize * model.voxel_size_ratio

    def reference(model):
        ray_pts, ray_id, step_id, interval = inputs(model)
        return _reference_filter(ray_pts, ray_id, {'step_id': step_id}, interval, N_RAYS, model.mask_cache, model.density, model.act_shift, thres)

    model, want, masks = _scaled_until_every_filter_bites(lambda: dvgo.DirectVoxGO(fast_color_thres=thres, **VOX), 21, reference)
    assert len(masks) == (3 if thres > 0 else 1)
    ray_pts, ray_id, step_id, interval = inputs(model)
    for keep_density in (False, True):
        g_pts, g_id, (g_step,), g_alpha, g_w, g_last, g_dens = model._k4_filter_samples(
            ray_pts, ray_id, (step_id,), interval, N_RAYS, model.mask_cache, model.density, keep_density=keep_density)
        for name, got in (('ray_pts', g_pts), ('ray_id', g_id), ('step_id', g_step), ('alpha', g_alpha), ('weights', g_w), ('alphainv_last', g_last)):
            _same(got, want[name], name)
        if keep_density:
            _same(g_dens, want['density'], 'density')
        else:
            assert g_dens is None
    # the coarse colour grid: sigmoid(k0)
    _same(model._k4_shade(model.k0(g_pts), vd, g_id, model.rgbnet), torch.sigmoid(model.k0(want['ray_pts'])), 'rgb')


@pytest.mark.parametrize('direct', [True, False])
def test_dvgo_shading_step(direct):
    """k0 features + view embedding -> rgb, with and without the diffuse add (lib/dvgo.py:380-412), against the statements on the same rgbnet op."""
    torch.manual_seed(5)
    model = _randomise(dvgo.DirectVoxGO(fast_color_thres=0, rgbnet_dim=6, rgbnet_direct=direct, rgbnet_width=32, rgbnet_depth=3, viewbase_pe=2, **VOX),
                       22, 1.0).cuda()
    ro, rd, vd = _rays(12)
    ray_pts, ray_id = model.sample_ray(rays_o=ro, rays_d=rd, near=0.2, far=1e9, stepsize=0.5)[:2]
    assert ray_pts.shape[0] > N_RAYS
    k0 = model.k0(ray_pts)
    emb = _view_emb(vd, model.viewfreq, ray_id)
    if direct:
        want = model._k4_rgbnet_sigmoid(torch.cat([k0, emb], -1))
    else:
        want = model._k4_rgbnet_sigmoid(torch.cat([k0[:, 3:], emb], -1), k0[:, :3])
    _same(model._k4_shade(model.k0(ray_pts), vd, ray_id, model.rgbnet, direct=direct), want, 'rgb')


def test_dbvgo_background_pass():
    """DirectBiVoxGO._forward on 7 rays x 5 outer samples; the foreground's alphainv_last drops rays 1, 3 and 5 (lib/dbvgo.py:257-262)."""
    thres, n_outer = 1e-2, 5
    torch.manual_seed(6)
    g = torch.Generator().manual_seed(13)
    pts_outer = ((torch.rand([N_RAYS, n_outer, 3], generator=g) * 2 - 1) * 0.98).cuda()
    vd = _rays(13)[2]
    prev = torch.tensor([0.9, 0.001, 0.5, 0.0, 0.3, 0.005, 1.0]).cuda()
    interval = 0.5

    def reference(model):
        ray_id, step_id = dvgo.create_full_step_id(pts_outer.shape[:2], device=pts_outer.device)
        rows = (prev > thres)
        assert bool(rows.any()) and not bool(rows.all())
        ray_id = ray_id.view(N_RAYS, -1)[rows].view(-1)
        step_id = step_id.view(N_RAYS, -1)[rows].view(-1)
        ray_pts = pts_outer.reshape(-1, 3).view(N_RAYS, -1, 3)[rows].view(-1, 3)
        return _reference_filter(ray_pts, ray_id, {'step_id': step_id}, interval, N_RAYS, model.mask_cache[1], model.density[1], model.act_shift, thres)

    make = lambda: dbvgo.DirectBiVoxGO(fast_color_thres=thres, rgbnet_dim=6, rgbnet_width=32, rgbnet_depth=3, viewbase_pe=2, **VOX)      # noqa: E731
    model, want, masks = _scaled_until_every_filter_bites(make, 23, reference)
    assert len(masks) == 3
    got = model._forward(ray_pts=pts_outer, viewdirs=vd, interval=interval, N_=N_RAYS, mask_grid=model.mask_cache[1], density_grid=model.density[1],
                         k0_grid=model.k0[1], rgbnet=model._rgbnet_of(1), prev_alphainv_last=prev)
    assert set(got) == {'rgb', 'alpha', 'weights', 'alphainv_last', 'ray_id', 'step_id'}
    for name in ('alpha', 'weights', 'alphainv_last', 'ray_id', 'step_id'):
        _same(got[name], want[name], name)
    assert not set(want['ray_id'].tolist()) & {1, 3, 5}
    feat = torch.cat([model.k0[1](want['ray_pts']), _view_emb(vd, model.viewfreq, want['ray_id'])], -1)
    _same(got['rgb'], model._k4_rgbnet_sigmoid(feat, net=model.rgbnet[1]), 'rgb')


def test_dcvgo_filter_with_its_three_columns():
    thres, stepsize = 1e-2, 0.5
    ro, rd, vd = _rays(14)

    def inputs(model):
        ray_pts, inner_mask, t = model.sample_ray(ori_rays_o=ro, ori_rays_d=rd, stepsize=stepsize)
        ray_id, step_id = dvgo.create_full_step_id(ray_pts.shape[:2], device=ray_pts.device)
        cols = {'inner_mask': inner_mask.flatten(), 't': t[None].expand(N_RAYS, len(t)).flatten(), 'step_id': step_id}
        return ray_pts.reshape(-1, 3), ray_id, cols, stepsize * model.voxel_size_ratio

    def reference(model):
        ray_pts, ray_id, cols, interval = inputs(model)
        return _reference_filter(ray_pts, ray_id, cols, interval, N_RAYS, model.mask_cache, model.density, model.act_shift, thres)

    make = lambda: dcvgo.DirectContractedVoxGO(fast_color_thres=thres, **VOX)      # noqa: E731
    model, want, masks = _scaled_until_every_filter_bites(make, 24, reference)
    assert len(masks) == 3
    ray_pts, ray_id, cols, interval = inputs(model)
    g_pts, g_id, (g_inner, g_t, g_step), g_alpha, g_w, g_last, g_dens = model._k4_filter_samples(
        ray_pts, ray_id, (cols['inner_mask'], cols['t'], cols['step_id']), interval, N_RAYS, model.mask_cache, model.density, keep_density=True)
    for name, got in (('ray_pts', g_pts), ('ray_id', g_id), ('inner_mask', g_inner), ('t', g_t), ('step_id', g_step), ('density', g_dens),
                      ('alpha', g_alpha), ('weights', g_w), ('alphainv_last', g_last)):
        _same(got, want[name], name)
    assert bool(want['inner_mask'].any()) and not bool(want['inner_mask'].all())          # samples inside and outside the unit cube survive


@pytest.mark.parametrize('fused_input', [True, False])
def test_dmpigo_filter_by_filter_form(fused_input, monkeypatch):
    """DirectMPIGO's staged forward with ``k4_presel=False`` at mpi_depth 8; the colour MLP's input in one launch and op by op (lib/dmpigo.py:336-379)."""
    monkeypatch.setattr(dmpigo, '_FUSED_MLP_INPUT', fused_input)
    thres, stepsize = 1e-2, 0.5
    torch.manual_seed(7)
    g = torch.Generator().manual_seed(15)
    ro = torch.cat([(torch.rand([N_RAYS, 2], generator=g) * 2 - 1) * 0.9, -torch.ones([N_RAYS, 1])], -1).cuda()
    rd = torch.cat([(torch.rand([N_RAYS, 2], generator=g) * 2 - 1) * 0.8, 2 * torch.ones([N_RAYS, 1])], -1).cuda()
    vd = rd / rd.norm(dim=-1, keepdim=True)
    rk = dict(near=0, far=1, stepsize=stepsize, bg=0.5, render_depth=True)
    n_samples = int((8 - 1) / stepsize) + 1

    def reference(model):
        ray_pts, ray_id, step_id, n, _ = model.sample_ray(rays_o=ro, rays_d=rd, near=0, far=1, stepsize=stepsize)
        assert n == n_samples
        return _reference_filter(ray_pts, ray_id, {'step_id': step_id}, stepsize * model.voxel_size_ratio, N_RAYS, model.mask_cache,
                                 lambda p: model.density(p) + model.act_shift(p), 0, thres)

    make = lambda: dmpigo.DirectMPIGO(xyz_min=[-1., -1., -1.], xyz_max=[1., 1., 1.], num_voxels=8 ** 3, mpi_depth=8, fast_color_thres=thres,      # noqa: E731
                                      rgbnet_dim=6, rgbnet_width=32, rgbnet_depth=3, viewbase_pe=2, spatial_pe=2, act_type='relu', mode_type='mlp')
    model, want, masks = _scaled_until_every_filter_bites(make, 25, reference)
    assert len(masks) == 3
    out = model(ro, rd, vd, k4_staged=True, k4_presel=False, **rk)
    for key, name in (('raw_alpha', 'alpha'), ('weights', 'weights'), ('alphainv_last', 'alphainv_last'), ('ray_id', 'ray_id')):
        _same(out[key], want[name], key)
    _same(out['s'], (want['step_id'] + 0.5) / n_samples, 's')
    assert out['n_max'] == n_samples
    if not fused_input:
        pts = want['ray_pts']
        pe_spa = ((pts - model.xyz_min) / (model.xyz_max - model.xyz_min)).flip((-1,)) * 2 - 1
        pe_emb = (pe_spa.unsqueeze(-1) * model.posfreq).flatten(-2)
        pe_emb = torch.cat([pe_spa, pe_emb.sin(), pe_emb.cos()], -1)
        feat = torch.cat([model.k0(pts), pe_emb, _view_emb(vd, model.viewfreq, want['ray_id'])], -1)
        _same(out['raw_rgb'], model._k4_rgbnet_sigmoid(feat), 'raw_rgb')
