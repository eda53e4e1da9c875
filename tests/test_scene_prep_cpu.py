"""Host-side facts of scene preparation (no GPU): the entry points are declared, bound and exported; there is no CPU path; the float64 oracle
(tests/scene_prep_oracle.py) reproduces the reference's count on the golden; and the seeded scenes of the GPU tests meet the conditions those tests
rely on -- few voxels in the undecidable band around 1, no alpha near the coarse-geometry threshold."""
import os
import re

import numpy as np
import pytest
import torch

import nerf4k_amd  # noqa: F401
from nerf4k_amd import _native as N, scene, scene_prep
from nerf4k_amd.lib import dvgo as D, utils
import scene_prep_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('k4_count_views_walk', 'k4_count_views_finalise', 'k4_near_cam_mask', 'k4_frustum_bounds', 'k4_coarse_geo_bounds')


def test_entry_points_are_declared_bound_and_exported():
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'k4nerf.h')).read(), flags=re.S)
    for s in SYMBOLS:
        assert re.search(r'\bint\s+%s\s*\(' % s, header), f'{s} is not declared in include/k4nerf.h'
        assert s in N._EXTRA_SIGS, f'{s} is not bound in _native.py'
        assert hasattr(N.lib(), s), f'{s} is not exported by the library'
    assert len(N._EXTRA_SIGS['k4_count_views_walk'][0]) == 13 and len(N._EXTRA_SIGS['k4_frustum_bounds'][0]) == 16
    for name in ('k4_voxel_count_views', 'k4_maskout_near_cam_vox'):
        assert callable(getattr(D.DirectVoxGO, name))
    for name in ('compute_bbox_by_cam_frustrm', 'compute_bbox_by_coarse_geo', 'coarse_geo_bounds', 'per_voxel_init'):
        assert callable(getattr(scene_prep, name))


def test_cpu_only_calls_raise(tmp_path, monkeypatch):
    ck, rk, z = O.golden_occ()
    model = utils.model_from_checkpoint_dict(ck)                  # a CPU model: raises with or without a GPU in the machine
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)   # (the two module-level functions pick the device themselves)
    with pytest.raises(N.K4Error):
        model.k4_voxel_count_views(torch.from_numpy(z['cnt/rays_o']), torch.from_numpy(z['cnt/rays_d']), [1, 1], near=rk['near'], far=rk['far'],
                                   stepsize=rk['stepsize'], downrate=1)
    with pytest.raises(N.K4Error):
        model.k4_maskout_near_cam_vox(torch.tensor([[0.4, 0.3, 0.2]]), 0.35)
    with pytest.raises(N.K4Error):
        scene_prep.coarse_geo_bounds(model, 1e-3)
    path = str(tmp_path / 'coarse_last.tar')
    torch.save(ck, path)
    with pytest.raises(N.K4Error):
        scene_prep.compute_bbox_by_coarse_geo(D.DirectVoxGO, path, 1e-3)
    K = scene.lego_K(20, 20)
    with pytest.raises(N.K4Error):
        scene_prep.compute_bbox_by_cam_frustrm(np.array([[20, 20]]), np.stack([K]), torch.eye(4)[None], [0], 2.0, 6.0, ndc=False, inverse_y=False,
                                               flip_x=False, flip_y=False)


def test_a_factored_density_raises_before_any_launch():
    model = D.DirectVoxGO(density_type='TensoRFGrid', density_config={'n_comp': 2}, **O.dvgo_kwargs((6.5, 6.5, 6.5)))
    with pytest.raises(NotImplementedError):
        model.k4_maskout_near_cam_vox(torch.zeros(1, 3), 0.1)


def test_oracle_reproduces_the_reference_count_on_the_golden():
    ck, rk, z = O.golden_occ()
    kw = ck['model_kwargs']
    world, voxel_size = O.world_of(kw)
    assert world == [12, 12, 12] and O.n_samples_of(world, rk['stepsize']) == 46
    sums = O.count_sums(z['cnt/rays_o'], z['cnt/rays_d'], [1, 1], kw['xyz_min'], kw['xyz_max'], world, rk['near'], rk['stepsize'], voxel_size)
    count, compared = O.count_and_band(sums)
    assert np.array_equal(count, z['cnt/count'])
    assert compared.all() and float(np.abs(sums - 1).min()) > 2e-3


@pytest.mark.parametrize('name', O.COUNT_CASES)
def test_count_scenes_keep_the_band_small(name):
    case = O.count_case(name)
    kw, world, sums = O.oracle_of_case(case)
    count, compared = O.count_and_band(sums)
    assert sums.shape[0] == len(case['imsz'])
    excluded = 1 - float(compared.mean())
    print(f'{name}: world {world}, excluded share {excluded:.4f}, counts up to {count.max():.0f}, seen voxels {(count > 0).mean():.2f}, max sum {sums.max():.1f}')
    assert excluded <= O.MAX_EXCLUDED
    assert 0 < (count > 0).mean() and (count == 0).any()                    # a real mix of seen and unseen voxels
    if name == 'noncubic_3views_20x20':
        assert world == [9, 14, 11]
    if name == 'no_wrap_64x64_identical':                                    # thousands of contributions per voxel, every seen voxel once per view
        assert sums.max() > 2000 and set(np.unique(count).tolist()) == {0.0, 2.0}
    if name == 'irregular_unequal_views_inside_camera':
        assert (case['rays_d'] == 0).any(1).sum() >= 100 and len(set(case['imsz'])) == 3
    if name == 'cubic_24x17_downrate2':                                      # some rays of the sliced views never touch the padded grid
        lo, hi = np.asarray(kw['xyz_min'], np.float64), np.asarray(kw['xyz_max'], np.float64)
        o = O.split_views(case['rays_o'], case['imsz'], 2, False)[0].astype(np.float64)
        d = O.split_views(case['rays_d'], case['imsz'], 2, False)[0].astype(np.float64)
        assert o.shape == (1 * 12 * 17, 3)                                   # the literal slice strides dimension 0 and the rows, not the columns
        a, b = (hi - o) / d, (lo - o) / d
        misses = np.minimum(a, b).max(-1) > np.maximum(a, b).min(-1)
        assert 0 < misses.sum() < len(misses)


@pytest.mark.parametrize('name', sorted(O.GEO_CASES))
def test_geo_scenes_keep_alpha_away_from_the_threshold(name):
    extent, seed, thres = O.GEO_CASES[name]
    kw = O.dvgo_kwargs(extent)
    world, _ = O.world_of(kw)
    den = O.geo_density(world, seed)
    shift = np.log(1 / (1 - kw['alpha_init']) - 1)
    idx, margin = O.geo_oracle(den, shift, 1.0, thres)
    print(f'{name}: world {world}, bounds {idx}, margin {margin:.2e}')
    assert margin > 1e-4
    assert idx is not None and all(0 < idx[a] and idx[3 + a] < world[a] - 1 for a in range(3)), 'the box must lie strictly inside the grid'
    assert O.geo_oracle(den, shift, 1.0, 2.0)[0] is None                     # a threshold above every alpha
