"""DirectBiVoxGO (nerf4k_amd.lib.dbvgo) without a GPU: the CPU oracle (tests/bivox_oracle.py) against the reference-made goldens
(tests/gen_bivox_golden.py), the checkpoint contract, and the drop-in boundary (no CPU path)."""
import os

import numpy as np
import pytest
import torch

import nerf4k_amd  # noqa: F401
from nerf4k_amd import _native as N, scene
from nerf4k_amd.lib import dbvgo, dcvgo, dvgo, dmpigo, grid, render_utils_cuda, utils
from helpers import GOLDEN, load_march_golden, psnr
import bivox_oracle as bo

GOLD = ['march_dbvgo_w128', 'march_dbvgo_w64', 'march_dbvgo_w32_nomlp', 'march_dbvgo_coarse']


def _aux(name):
    z = np.load(os.path.join(GOLDEN, name + '.npz'))
    return {k[4:]: z[k] for k in z.files if k.startswith('aux/')}


@pytest.mark.parametrize('sampler', ['fp32', 'source'])
@pytest.mark.parametrize('name', GOLD)
def test_oracle_matches_reference_golden(name, sampler):
    """Both restatements of the background sampler give the reference's sample lists of both passes exactly (the goldens hold no ties) and
    its outputs within 1e-5 and 80 dB (``depth`` on the scale of the largest value its formula can take), the bound the device tests hold the
    kernels to against the same goldens.  Oracle and reference are two fp32 evaluations: the host's exp / pow differ by an ulp or two between
    CPU types (alpha carries ~2.4e-7 of that, helpers.NATIVE_TOL['r2a_*/alpha']), a transmittance is a product of up to ~150 such factors, and
    the source-rounded sampler moves the background points by up to 6e-7 (test_bg_sampler_restatements_agree), which the density lookup
    multiplies by the grid's slope.  Measured: 2.4e-6 at most (raw_alpha, weights)."""
    g, aux = load_march_golden(name), _aux(name)
    r = g['rays']
    cnt, ps = {}, {}
    with torch.no_grad():
        out = bo.forward(g['model_kwargs'], g['model_state_dict'], r['rays_o'], r['rays_d'], r['viewdirs'], counters=cnt, passes=ps,
                         bg_sampler=sampler, **g['render_kwargs'])
    ref = g['out']
    assert set(out) == set(ref)
    assert torch.equal(out['ray_id'], ref['ray_id'].long())
    for tag in ('fg', 'bg'):
        assert np.array_equal(ps[tag]['ray_id'].numpy(), aux[tag + '_ray_id']) and np.array_equal(ps[tag]['step_id'].numpy(), aux[tag + '_step_id'])
    assert cnt['fg'] + cnt['bg'] == aux['counters'].tolist() and cnt['n_outer'] == int(aux['n_outer'])
    assert ref['alphainv_last'].shape[0] == 2 * r['rays_o'].shape[0]
    dscale = bo.depth_scale(g['model_kwargs'], aux['fg_step_max'], g['render_kwargs']['stepsize'])
    for k in ('rgb_marched', 'alphainv_last', 'weights', 'raw_alpha', 'raw_rgb', 'depth'):
        s = dscale if k == 'depth' else 1.0
        assert out[k].shape == ref[k].shape, k
        assert psnr(out[k] / s, ref[k] / s) >= 80, (name, k)
        assert torch.allclose(out[k], ref[k], rtol=0, atol=1e-5 * s), (name, k, float((out[k] - ref[k]).abs().max()))


def test_goldens_cover_the_cases_they_were_made_for():
    n_outer = {n: int(_aux(n)['n_outer']) for n in GOLD}
    assert n_outer['march_dbvgo_w64'] > 64 and 0 < n_outer['march_dbvgo_w128'] < 64 and n_outer['march_dbvgo_w128'] % 8
    assert int(_aux('march_dbvgo_w64')['fg_steps_sampled_max']) > 64 and int(_aux('march_dbvgo_w128')['fg_steps_sampled_max']) > 64
    thres = {n: load_march_golden(n)['model_kwargs']['fast_color_thres'] for n in GOLD}
    assert thres['march_dbvgo_w64'] == 0 and thres['march_dbvgo_coarse'] == 0 and thres['march_dbvgo_w128'] > 0
    g = load_march_golden('march_dbvgo_w128')
    r = g['rays']
    assert r['rays_o'].shape[0] % 64 != 0
    assert int(((r['rays_d'] == 0).sum(-1) == 2).sum()) >= 2                                   # two zero direction components
    o = (r['rays_o'] - g['model_state_dict']['scene_center']) / g['model_state_dict']['scene_radius']
    inside = (o.abs().amax(-1) < 1)
    assert inside.any() and (~inside).any()
    # rays from outside that miss the cube: no foreground sample inside the bbox, yet the background pass runs
    aux = _aux('march_dbvgo_w128')
    from oracle import native_cpu as nat
    d = r['rays_d'] / r['rays_d'].norm(dim=-1, keepdim=True)
    stepdist, _ = bo.n_outer(g['model_kwargs'], g['render_kwargs']['stepsize'])
    pts, outb, rid, _, _, _, _ = nat.sample_pts_on_rays(o, d, torch.Tensor([-1, -1, -1]), torch.Tensor([1, 1, 1]), 0, 2 * np.sqrt(3), stepdist)
    hit = torch.zeros(o.shape[0], dtype=torch.bool)
    hit[rid[~outb]] = True
    assert (~hit & ~inside).any() and (hit & ~inside).any()
    assert aux['counters'][4] > 0


def test_bg_sampler_restatements_agree():
    """fp32 tensor form vs the source-rounded form: a few ulp of values in about [-1.2, 1.2]."""
    g = torch.Generator().manual_seed(3)
    o = (torch.rand([64, 3], generator=g) * 2 - 1) * 0.8
    d = torch.randn([64, 3], generator=g)
    d = d / d.norm(dim=-1, keepdim=True)
    from oracle import native_cpu as nat
    t_max = nat.infer_t_minmax(o, d, torch.Tensor([-1, -1, -1]), torch.Tensor([1, 1, 1]), 0, 2 * np.sqrt(3))[1]      # where the ray leaves the cube
    for n, bgp in ((1, 0.5), (65, 0.2), (130, 0.5)):
        a = bo.sample_bg_pts_fp32(o, d, t_max, bgp, n).numpy()
        b = bo.sample_bg_pts_source(o.numpy(), d.numpy(), t_max.numpy(), bgp, n)
        assert a.shape == b.shape == (64, n, 3) and b.dtype == np.float32
        assert np.abs(a - b).max() <= 6e-7
        m = np.abs(b).max(-1)
        assert m.min() >= bgp - 1e-6 and m.max() <= 1 + 1e-6                                    # the inf-norm shell [bg_preserve, 1]


def _keys(rgbnet_dim, bg_use_mlp, depth=3):
    keys = {'scene_center', 'scene_radius', 'xyz_min', 'xyz_max', 'act_shift'}
    for i in range(2):
        keys |= {f'density.{i}.grid', f'density.{i}.xyz_min', f'density.{i}.xyz_max', f'k0.{i}.grid', f'k0.{i}.xyz_min', f'k0.{i}.xyz_max',
                 f'mask_cache.{i}.mask', f'mask_cache.{i}.xyz2ijk_scale', f'mask_cache.{i}.xyz2ijk_shift'}
    if rgbnet_dim > 0:
        keys.add('viewfreq')
        for i in range(2 if bg_use_mlp else 1):
            for layer in ['0'] + [f'{2 + j}.0' for j in range(depth - 2)] + [str(depth)]:
                keys |= {f'rgbnet.{i}.{layer}.weight', f'rgbnet.{i}.{layer}.bias'}
    return keys


@pytest.mark.parametrize('rgbnet_dim,bg_use_mlp', [(6, True), (6, False), (0, True)])
def test_state_dict_keys_of_the_three_constructor_variants(rgbnet_dim, bg_use_mlp):
    m = dbvgo.DirectBiVoxGO(xyz_min=[-2, -2, -2], xyz_max=[2, 2, 2], num_voxels=12 ** 3, num_voxels_base=12 ** 3, alpha_init=1e-2,
                            rgbnet_dim=rgbnet_dim, bg_use_mlp=bg_use_mlp, rgbnet_width=32)
    assert set(m.state_dict().keys()) == _keys(rgbnet_dim, bg_use_mlp)
    assert m.k0[0].grid.shape[1] == (rgbnet_dim or 3) and m.k0[1].grid.shape[1] == (rgbnet_dim if rgbnet_dim and bg_use_mlp else 3)
    assert torch.equal(m.xyz_min, torch.Tensor([-1, -1, -1])) and torch.equal(m.scene_radius, torch.Tensor([2, 2, 2]))
    assert m.mask_cache[0].mask.data_ptr() != m.mask_cache[1].mask.data_ptr()
    ck = scene.make_bivox_checkpoint(seed=1, num_voxels=12 ** 3, rgbnet_dim=rgbnet_dim, bg_use_mlp=bg_use_mlp, rgbnet_width=32)
    assert set(ck['model_state_dict']) == _keys(rgbnet_dim, bg_use_mlp)
    for i in range(2):                                                                          # neither mask is trivial
        mk = ck['model_state_dict'][f'mask_cache.{i}.mask']
        assert 0 < int(mk.sum()) < mk.numel()


@pytest.mark.parametrize('name', GOLD)
def test_checkpoint_contract(name):
    """model_class(**model_kwargs) + strict load_state_dict with the reference's key names, in both directions; get_kwargs() holds the
    reference's keys plus bg_preserve / bg_use_mlp and round-trips; a checkpoint written upstream (without the two) loads with the defaults."""
    g = load_march_golden(name)
    model = utils.model_from_checkpoint_dict(g)
    assert isinstance(model, dbvgo.DirectBiVoxGO)
    assert set(model.state_dict().keys()) == set(g['model_state_dict'].keys())
    for k, v in model.state_dict().items():
        assert torch.equal(v, g['model_state_dict'][k]), k                                      # (both masks keep their own content)
    kw = model.get_kwargs()
    upstream = {'xyz_min', 'xyz_max', 'num_voxels', 'num_voxels_base', 'alpha_init', 'voxel_size_ratio', 'mask_cache_world_size',
                'fast_color_thres', 'density_type', 'k0_type', 'density_config', 'k0_config', 'rgbnet_dim', 'rgbnet_depth', 'rgbnet_width',
                'viewbase_pe'}
    assert set(kw) == upstream | {'bg_preserve', 'bg_use_mlp'}
    assert np.array_equal(kw['xyz_min'], [-1, -1, -1]) and np.array_equal(kw['xyz_max'], [1, 1, 1])
    for k in ('num_voxels', 'num_voxels_base', 'mask_cache_world_size', 'fast_color_thres', 'rgbnet_dim', 'bg_preserve', 'bg_use_mlp'):
        assert kw[k] == g['model_kwargs'][k], k
    model2 = dbvgo.DirectBiVoxGO(**kw)
    model2.load_state_dict(model.state_dict())
    assert torch.equal(model2.scene_center, g['model_state_dict']['scene_center']) and model2.bg_preserve == model.bg_preserve
    assert list(model2.world_size) == list(model.world_size) == list(g['model_state_dict']['density.0.grid'].shape[2:])
    if g['model_kwargs']['bg_use_mlp']:
        old = dbvgo.DirectBiVoxGO(**{k: v for k, v in kw.items() if k in upstream})
        old.load_state_dict(model.state_dict())
        assert old.bg_preserve == 0.5 and old.bg_use_mlp is True


def test_n_outer_uses_the_host_float32_stepdist():
    for nv, stepsize, bgp in ((30 ** 3, 0.5, 0.5), (28 ** 3, 0.25, 0.2), (160 ** 3, 0.5, 0.5), (1000003, 0.3, 0.35)):
        m = dbvgo.DirectBiVoxGO(xyz_min=[-1, -1, -1], xyz_max=[1, 1, 1], num_voxels=nv, num_voxels_base=nv, alpha_init=1e-2, bg_preserve=bgp)
        stepdist = stepsize * ((torch.Tensor([2, 2, 2]).prod() / nv).pow(1 / 3))
        want = int(np.sqrt(3) / stepdist.item() * (1 - bgp)) + 1
        assert m._n_outer(stepsize)[1] == want == bo.n_outer(dict(num_voxels=nv, num_voxels_base=nv, bg_preserve=bgp), stepsize)[1]


def test_the_other_models_and_create_grid_are_untouched():
    assert isinstance(grid.create_grid('DenseGrid', channels=1, world_size=[4, 4, 4], xyz_min=[-1] * 3, xyz_max=[1] * 3), grid.DenseGrid)
    with pytest.raises(NotImplementedError):
        grid.create_grid('VQGrid', channels=1, world_size=[4, 4, 4], xyz_min=[-1] * 3, xyz_max=[1] * 3)
    for name, cls in (('march_mpi_base', dmpigo.DirectMPIGO), ('march_dvgo_base', dvgo.DirectVoxGO), ('march_dcvgo_inf', dcvgo.DirectContractedVoxGO)):
        g = load_march_golden(name)
        model = utils.model_from_checkpoint_dict(g)
        assert type(model) is cls and set(model.state_dict().keys()) == set(g['model_state_dict'].keys())
        assert model._k4_fusable() and dvgo._each(model.density) == [model.density] and dvgo._each(model.rgbnet) == [model.rgbnet]


def test_cpu_inputs_raise():
    ck = scene.make_bivox_checkpoint(seed=1, num_voxels=12 ** 3, rgbnet_dim=3, rgbnet_width=32, viewbase_pe=2)
    model = utils.model_from_checkpoint_dict(ck)
    ro, rd = torch.zeros(4, 3), torch.ones(4, 3)
    with pytest.raises(N.K4Error):
        model(ro, rd, rd, **ck['render_kwargs'])
    with pytest.raises(N.K4Error):
        model.sample_ray(ori_rays_o=ro, ori_rays_d=rd, stepsize=0.5)
    with pytest.raises(N.K4Error):
        render_utils_cuda.sample_bg_pts_on_rays(ro, rd, torch.ones(4), 0.5, 8)
    with pytest.raises(N.K4Error):
        model._k4_rgbnet_sigmoid(torch.zeros(4, 18), net=model.rgbnet[1])
    assert hasattr(N.lib(), 'k4_march_bivox_fwd') and hasattr(N.lib(), 'k4_sample_bg_pts_on_rays')
    assert N.C.sizeof(N.BivoxDesc) % 8 == 0 and N.K4_ABI_VERSION >= 21
