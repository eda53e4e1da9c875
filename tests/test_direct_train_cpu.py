"""CPU-side checks of the fused direct-colour training step (lib/train_ops.dvgo_direct_render_loss, csrc/k4_direct_train.hip): the fp64 oracle of
tests/direct_train_oracle.py against the reference's own terms and gradients (tests/golden/grad_dvgo_direct.npz), the support predicate, and the
checkpoint-table arithmetic."""
import json
import os

import numpy as np
import pytest
import torch

import nerf4k_amd  # noqa: F401
from nerf4k_amd import _native as N, scene
from nerf4k_amd.lib import train_ops, utils
from helpers import GOLDEN
import direct_train_oracle as dto


def load_golden():
    z = np.load(os.path.join(GOLDEN, 'grad_dvgo_direct.npz'), allow_pickle=False)
    kw = json.loads(str(z['model_kwargs_json']))
    for k in ('xyz_min', 'xyz_max'):
        kw[k] = np.asarray(kw[k], dtype=np.float32)
    g = {'ck': {'model_class': str(z['model_class']), 'model_kwargs': kw,
                'model_state_dict': {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith('sd/')}},
         'rk': json.loads(str(z['render_kwargs_json'])), 'weights': json.loads(str(z['weights_json'])), 'target': torch.from_numpy(z['target']),
         'stepdist': float(z['stepdist']), 'interval': float(z['interval'])}
    for group in ('in', 'term', 'out', 'list', 'grad'):
        g[group] = {k[len(group) + 1:]: torch.from_numpy(np.asarray(z[k])) for k in z.files if k.startswith(group + '/')}
    for k in ('ray_id', 'step_id', 'a_ray_id', 'a_step_id'):
        g['list'][k] = g['list'][k].long()
    return g


def oracle_on(sd, rays_o, rays_d, near, stepdist, interval, a_ray_id, a_step_id, shaded, target, bg, weights, grad_total=1.0):
    pts = dto.points_of(rays_o, rays_d, sd['xyz_min'], sd['xyz_max'], near, stepdist, a_ray_id, a_step_id)
    return dto.evaluate(sd['density.grid'], sd['k0.grid'], sd['xyz_min'], sd['xyz_max'], sd['act_shift'], interval, pts, a_ray_id, shaded, target,
                        len(rays_o), bg, grad_total=grad_total, **weights)


def test_oracle_reproduces_the_reference_terms_and_gradients():
    """The reference ran in fp32: its terms within 2e-6 and its gradients within 2e-5 of the tensor's largest entry, the bounds
    tests/test_train_gpu.py holds the staged path to."""
    g = load_golden()
    L = g['list']
    got = oracle_on(g['ck']['model_state_dict'], g['in']['rays_o'], g['in']['rays_d'], g['rk']['near'], g['stepdist'], g['interval'],
                    L['a_ray_id'], L['a_step_id'], L['shaded'].bool(), g['target'], g['rk']['bg'], g['weights'])
    for k in ('total', 'photo', 'entropy', 'rgbper'):
        want = float(g['term'][k])
        assert abs(float(got[k]) - want) <= 2e-6 * max(1.0, abs(want)), (k, float(got[k]), want)
    for k, name in (('rgb_marched', 'rgb_marched'), ('alphainv_last', 'alphainv_last')):
        assert float((got[k] - g['out'][name].double()).abs().max()) <= 2e-6, k
    for k, name in (('grad_density', 'density.grid'), ('grad_k0', 'k0.grid')):
        want = g['grad'][name].double()
        assert float(want.abs().max()) > 0
        assert float((got[k] - want).abs().max()) <= 2e-5 * float(want.abs().max()) + 1e-9, name
    # the lists are consistent: the shaded list is the alpha-passing list under the weight filter
    assert torch.equal(L['a_ray_id'][L['shaded'].bool()], L['ray_id']) and torch.equal(L['a_step_id'][L['shaded'].bool()], L['step_id'])


def test_support_predicate_decisions_and_reasons():
    ck = scene.make_lego_checkpoint(num_voxels=10 ** 3, rgbnet_dim=0)
    model = utils.model_from_checkpoint_dict(ck)
    ok, why = model.k4_direct_train_supported()
    assert not ok and 'GPU' in why                                        # everything else holds: only the device is wrong here
    ok, why = model.k4_direct_train_supported(rand_bkgd=True)
    assert not ok and 'rand_bkgd' in why
    model.mask_cache = None
    ok, why = model.k4_direct_train_supported()
    assert not ok and 'mask cache' in why
    net = utils.model_from_checkpoint_dict(scene.make_lego_checkpoint(num_voxels=10 ** 3, rgbnet_dim=6, rgbnet_width=32))
    ok, why = net.k4_direct_train_supported()
    assert not ok and 'rgbnet' in why
    kw = dict(ck['model_kwargs'], density_type='TensoRFGrid', density_config={'n_comp': 2})
    from nerf4k_amd.lib import dvgo
    ok, why = dvgo.DirectVoxGO(**kw).k4_direct_train_supported()
    assert not ok and 'TensoRFGrid' in why
    # the entry point raises the predicate's reason; the terms outside the coarse recipe raise too
    r = torch.zeros([4, 3])
    with pytest.raises(N.K4Error, match='rgbnet'):
        train_ops.dvgo_direct_render_loss(net, r, r, r, near=2., stepsize=0.5, bg=1, weight_main=1.0)
    with pytest.raises(N.K4Error, match='GPU'):
        train_ops.dvgo_direct_render_loss(utils.model_from_checkpoint_dict(ck), r, r, r, near=2., stepsize=0.5, bg=1, weight_main=1.0)


def test_chunk_and_checkpoint_table_arithmetic():
    """ceil(steps / 64) chunks per ray, one float per chunk and ray, for every step count 1..512; outside 1..4096 the table refuses."""
    import __graft_entry__ as g
    g.build()
    lib = N.lib()
    for steps in range(1, 513):
        want = -(-steps // 64)
        assert dto.chunks(steps) == want
        assert lib.k4_direct_train_chunks(steps) == want
        assert train_ops.direct_train_table(7, steps) == (want, 7 * want)
        # the last step of the ray lies in the last chunk, and the chunk before it does not hold it
        assert (steps - 1) >> 6 == want - 1
    assert train_ops.direct_train_table(0, 1) == (1, 0)
    # a 100^3 grid at stepsize 0.5: the box diagonal bounds a ray at ceil(sqrt(3) * 100 / 0.5) + 2 steps = 6 floats per ray
    assert dto.chunks(int(np.ceil(np.sqrt(3) * 100 / 0.5)) + 2) == 6
    assert lib.k4_direct_train_chunks(4096) == 64
    for bad in (0, -1, 4097):
        assert lib.k4_direct_train_chunks(bad) == -1
        with pytest.raises(N.K4Error):
            train_ops.direct_train_table(1, bad)
