"""TensoRFGrid (nerf4k_amd.lib.grid) without a GPU: the fp64 oracle against the reference-made goldens (tests/gen_tensorf_golden.py), the checkpoint
contract of the class and of the models that take it, and the drop-in boundary (no CPU path)."""
import numpy as np
import pytest
import torch

import nerf4k_amd  # noqa: F401
from nerf4k_amd import _native as N
from nerf4k_amd.lib import grid as kgrid, utils, dvgo, dmpigo
from helpers import load_march_golden
import tensorf_oracle as to

CASES = ['c1', 'c9', 'r48']


def _arr(c, k):
    return torch.from_numpy(c['arr'][k])


@pytest.mark.parametrize('name', CASES)
def test_oracle_lookup_and_gradients_match_the_reference(name):
    c = to.load_grid_case(name)
    for tag in ('', 'cell_') if name != 'r48' else ('',):
        pts, go = _arr(c, tag + 'pts'), _arr(c, tag + 'go')
        to.check(c, tag + 'out', to.lookup(c['sd'], pts), name + '/')
        for k, g in to.gradients(c['sd'], pts, go).items():
            to.check(c, f'{tag}grad/{k}', g, name + '/')


@pytest.mark.parametrize('name', ['c1', 'c9'])
def test_oracle_dense_tv_resize_match_the_reference(name):
    c = to.load_grid_case(name)
    to.check(c, 'dense', to.dense(c['sd']), name + '/')
    tv = to.tv_grad(c['tvsd'], 0.3, 0.2, 0.1)
    d = c['tvsd']['xy_plane'][:, :, 1:] - c['tvsd']['xy_plane'][:, :, :-1]
    assert bool((d.abs() > 1).any()) and bool((d.abs() < 1).any())          # both smooth-L1 branches occur
    for k in to.FACTORS:
        to.check(c, 'tv/' + k, tv[k], name + '/')
    for k, v in to.resize(c['sd'], [9, 8, 11]).items():
        to.check(c, 'scaled/' + k, v, name + '/')


@pytest.mark.parametrize('name', ['c1', 'c9'])
def test_create_grid_returns_the_class_with_the_reference_state_dict(name):
    c = to.load_grid_case(name)
    g = kgrid.create_grid('TensoRFGrid', channels=c['channels'], world_size=torch.tensor(c['world']), xyz_min=[-1.0, -0.5, 0.25], xyz_max=[1.5, 0.75, 2.0],
                          config=c['config'])
    assert isinstance(g, kgrid.TensoRFGrid)
    sd = g.state_dict()
    assert list(sd.keys()) == c['keys']
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(v.shape) for k, v in c['sd'].items()}
    assert ('f_vec' in sd) == (c['channels'] > 1)
    g.load_state_dict(c['sd'])                                     # strict
    # the reference's initial distributions: N(0, 0.1^2) factors, kaiming-uniform f_vec (bound 1 / sqrt(fan_in = C))
    big = kgrid.TensoRFGrid(12, [40, 40, 40], [0, 0, 0], [1, 1, 1], {'n_comp': 16})
    assert abs(float(big.xy_plane.detach().std()) - 0.1) < 5e-3 and abs(float(big.xy_plane.detach().mean())) < 5e-3
    assert float(big.f_vec.detach().abs().max()) <= 1 / np.sqrt(12) + 1e-6 and float(big.f_vec.detach().abs().max()) > 0.9 / np.sqrt(12)
    assert 'n_comp=' in g.extra_repr()


def test_vqgrid_still_raises():
    with pytest.raises(NotImplementedError):
        kgrid.create_grid('VQGrid', channels=1, world_size=[4, 4, 4], xyz_min=[0, 0, 0], xyz_max=[1, 1, 1], config={})


def test_cpu_lookup_raises():
    g = kgrid.TensoRFGrid(3, [4, 5, 6], [0, 0, 0], [1, 1, 1], {'n_comp': 2})
    with pytest.raises(N.K4Error):
        g(torch.rand([7, 3]))
    with pytest.raises(N.K4Error):
        g.get_dense_grid()
    with pytest.raises(N.K4Error):
        g.total_variation_add_grad(1, 1, 1, True)
    with pytest.raises(N.K4Error):
        g.scale_volume_grid([5, 6, 7])


@pytest.mark.parametrize('name,cls', [('tensorf_march_dvgo', dvgo.DirectVoxGO), ('tensorf_march_mpi', dmpigo.DirectMPIGO)])
def test_model_kwargs_round_trip_through_load_model(name, cls, tmp_path):
    g = load_march_golden(name)
    model = utils.model_from_checkpoint_dict(g)                     # strict load of the reference's state dict
    assert isinstance(model.density, kgrid.TensoRFGrid) and isinstance(model.k0, kgrid.TensoRFGrid)
    kw = model.get_kwargs()
    assert kw['density_type'] == kw['k0_type'] == 'TensoRFGrid' and kw['k0_config'] == {'n_comp': 4} and kw['density_config'] == {'n_comp': 4}
    path = str(tmp_path / 'ck.tar')
    torch.save({'model_kwargs': kw, 'model_state_dict': model.state_dict()}, path)
    again = utils.load_model(cls, path)
    assert set(again.state_dict().keys()) == set(g['model_state_dict'].keys())
    for k, v in again.state_dict().items():
        assert torch.equal(v, g['model_state_dict'][k].to(v.dtype)), k


def test_methods_that_write_density_grid_raise_for_a_factored_density():
    model = utils.model_from_checkpoint_dict(load_march_golden('tensorf_march_dvgo'))
    with pytest.raises(NotImplementedError):
        model.maskout_near_cam_vox(torch.zeros([1, 3]), 0.1)
