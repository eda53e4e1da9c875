"""Pins the CPU oracle against vectors produced by the reference's own Python
(tests/golden/*.npz, generator oracle/gen_golden.py).  CPU only."""
import os

import numpy as np
import pytest
import torch

from oracle import marcher, sr as osr, ref_import
from helpers import GOLDEN, load_march_golden

MARCH = ['march_mpi_base', 'march_mpi_pe', 'march_mpi_half',
         'march_dvgo_base', 'march_dvgo_nodirect', 'march_dvgo_coarse']


@pytest.mark.parametrize('name', MARCH)
def test_marcher_oracle_matches_reference_python(name):
    g = load_march_golden(name)
    fn = {'DirectMPIGO': marcher.mpi_forward, 'DirectVoxGO': marcher.dvgo_forward}[g['model_class']]
    r = g['rays']
    out = fn(g['model_kwargs'], g['model_state_dict'], r['rays_o'], r['rays_d'], r['viewdirs'],
             **g['render_kwargs'])
    ref = g['out']
    assert set(ref.keys()) == set(out.keys())
    # index tensors bit-exact: every mask decision of the reference is reproduced
    assert torch.equal(out['ray_id'], ref['ray_id'])
    for k, v in ref.items():
        o = out[k] if torch.is_tensor(out[k]) else torch.tensor(out[k])
        assert o.shape == v.shape, k
        assert torch.allclose(o.float(), v.float(), rtol=0, atol=1e-6), (k, float((o.float() - v.float()).abs().max()))
    # in-place aliasing of the reference (lib/dmpigo.py:392-397, lib/dvgo.py:425-427)
    assert out['rgb_marched'] is out['rgb_feature']
    assert len(ref['weights']) > 100


def test_rays_match_reference():
    z = np.load(os.path.join(GOLDEN, 'rays_views.npz'))
    H, W = int(z['H']), int(z['W'])
    for tag, ndc in (('ndc', True), ('persp', False)):
        ro, rd, vd = marcher.get_rays_of_a_view(H, W, z[f'{tag}/K'], z[f'{tag}/c2w'], ndc)
        for a, k in ((ro, 'rays_o'), (rd, 'rays_d'), (vd, 'viewdirs')):
            assert torch.allclose(a, torch.from_numpy(z[f'{tag}/{k}']), rtol=0, atol=1e-6), (tag, k)


@pytest.mark.parametrize('name', ['sr_full5', 'sr_tiles', 'sr_tiles510geom'])
def test_sr_oracle_matches_reference_module(name):
    z = np.load(os.path.join(GOLDEN, name + '.npz'))
    sd = osr.make_state_dict(seed=int(z['seed']), num_block=int(z['num_block']))
    x, cond, y = (torch.from_numpy(z[k]) for k in ('x', 'cond', 'y'))
    if int(z['tile']) < 0:
        o = osr.sftnet_forward(sd, x, cond.unsqueeze(0))
    else:
        o = osr.tile_process(sd, x, cond, int(z['tile']))
    assert o.shape == y.shape
    assert float((o - y).abs().max()) < 2e-5, float((o - y).abs().max())


def test_sr_spec_counts():
    """458 state-dict tensors, 3,955,811 parameters at the default configuration."""
    spec = osr.state_dict_spec()
    assert len(spec) == 458
    assert sum(int(np.prod(s)) for _, s in spec) == 3955811


def test_tile_geometry_llff_510():
    """1008x756 @ tile 510 pad 10 -> padded windows 520x520, 508x520, 520x256, 508x256 (w x h)."""
    t = osr.tile_geometry(756, 1008, 510, 10)
    wh = [(xp1 - xp0, yp1 - yp0) for (_, _, _, _, yp0, yp1, xp0, xp1) in t]
    assert wh == [(520, 520), (508, 520), (520, 256), (508, 256)]
    assert sum(w * h for w, h in wh) == 797728


def test_reference_still_importable_and_live_equal():
    """Reference classes vs oracle on a fresh seeded case (oracle/gen_golden.py::live_case): against the reference's output stored in
    tests/golden/live_mpi_seed3.npz, and -- where the reference tree exists (build container) -- against the live reference module too."""
    import contextlib, io
    from oracle import gen_golden
    ck, rays = gen_golden.live_case()
    z = np.load(os.path.join(GOLDEN, 'live_mpi_seed3.npz'))
    for k, v in zip(('rays_o', 'rays_d', 'viewdirs'), rays):            # the case is the one the vectors were made for
        assert np.array_equal(v.numpy(), z['in/' + k]), k
    for k, v in ck['model_state_dict'].items():
        assert np.array_equal(v.numpy(), z['sd/' + k]), k
    wants = [{k: torch.from_numpy(z['out/' + k]) for k in ('ray_id', 'rgb_marched')}]
    if ref_import.available():
        ref = ref_import.load_reference()
        with contextlib.redirect_stdout(io.StringIO()):
            m = ref.dmpigo.DirectMPIGO(**ck['model_kwargs'])
        m.load_state_dict(ck['model_state_dict'])
        with torch.no_grad():
            wants.append(m(*rays, **ck['render_kwargs']))
    got = marcher.mpi_forward(ck['model_kwargs'], ck['model_state_dict'], *rays, **ck['render_kwargs'])
    for want in wants:
        assert torch.equal(got['ray_id'], want['ray_id'])
        assert torch.allclose(got['rgb_marched'], want['rgb_marched'], atol=1e-6)


@pytest.mark.parametrize('name', ['grad_mpi', 'grad_dvgo'])
def test_training_goldens_are_consistent_with_the_forward_oracle(name):
    """tests/golden/grad_*.npz (reference modules under autograd) record the training loss of their forward pass: the forward
    oracle on the same checkpoint / rays / target must reproduce it, and every recorded gradient must belong to a parameter of
    the checkpoint with the parameter's shape."""
    import json
    z = np.load(os.path.join(GOLDEN, name + '.npz'), allow_pickle=False)
    kw = json.loads(str(z['model_kwargs_json']))
    for k in ('xyz_min', 'xyz_max'):
        kw[k] = np.asarray(kw[k], dtype=np.float32)
    sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith('sd/')}
    rays = [torch.from_numpy(z['in/' + k]) for k in ('rays_o', 'rays_d', 'viewdirs')]
    rk = json.loads(str(z['render_kwargs_json']))
    out = marcher.forward(str(z['model_class']), kw, sd, *rays, **rk)
    loss = torch.nn.functional.mse_loss(out['rgb_marched'].float(), torch.from_numpy(z['target']))
    assert abs(float(loss) - float(z['loss'])) <= 1e-6, (float(loss), float(z['loss']))
    grads = {k[5:]: z[k] for k in z.files if k.startswith('grad/')}
    assert len(grads) >= 6 and 'density.grid' in grads and 'k0.grid' in grads
    for k, g in grads.items():
        assert k in sd and tuple(sd[k].shape) == g.shape, k
        assert np.isfinite(g).all()
    assert float(np.abs(grads['k0.grid']).max()) > 0 and float(np.abs(grads['density.grid']).max()) > 0


# ---------------------------------------------------------------------------------------------------------------------
# Reference-COMPILED pins: vectors produced by the reference's own lib/cuda/*.cu built for gfx950 (oracle/build_ref.py) and run on
# an MI355X (oracle/gen_native_golden.py).  They pin the native layer of the oracle, which the reference-Python goldens above
# cannot (there native_cpu.py stood in for the extension on both sides).
# ---------------------------------------------------------------------------------------------------------------------
def test_native_cpu_matches_reference_compiled_kernels():
    from oracle import native_cpu
    from helpers import load_native_golden, replay_native, check_native
    G = load_native_golden()
    check_native(replay_native(native_cpu, G, 'cpu'), G, 'oracle/native_cpu.py')
    # the fixtures do exercise the edge cases they are meant to
    S, M, A = G['native_sampler'], G['native_mask'], G['native_alpha']
    assert (S['in/rays_d'] == 0).any() and int(S['n_samples'].min()) == 1 and int(S['n_samples'].max()) > 100
    assert S['aabb/mask_outbbox'].any() and S['ndc256/mask_outbbox'].any() and not S['ndc256/mask_outbbox'].all()
    idx = M['in/xyz'] * M['in/scale'] + M['in/shift']
    assert (np.abs(idx - np.floor(idx) - 0.5) == 0).sum() > 100            # exact .5 ties are present
    assert np.isinf(A['r2a_a/exp']).any() and (A['r2a_a/alpha'] == 1).any() and (A['r2a_a/alpha'] == 0).any()
    seg = A['a2w/i_end'] - A['a2w/i_start']
    cnt = np.bincount(A['in/ray_id'], minlength=int(A['in/n_rays']))
    assert (seg < cnt).any() and (cnt == 0).any()                            # rays cut by the T < 1e-3 stop; rays without points


def test_optim_oracle_matches_reference_compiled_kernels():
    """oracle/optim.py against adam_upd_cuda / total_variation_cuda compiled from the reference.  atol 5e-7: the moments are sums
    of two products whose FMA contraction order is the compiler's choice (values ~1e-1: <= 1 ulp of the larger product)."""
    import json
    from oracle import optim as O
    z = np.load(os.path.join(GOLDEN, 'optim_ref.npz'))
    hyp = json.loads(str(z['hyper_json']))
    for name in ('adam_upd', 'masked_adam_upd', 'adam_upd_with_perlr'):
        for step in (1, 7):
            p, m, v = O.adam_upd(z['in/param'], z['in/grad'], z['in/exp_avg'], z['in/exp_avg_sq'], step, hyp['beta1'], hyp['beta2'],
                                 hyp['lr'], hyp['eps'], perlr=z['in/perlr'] if name.endswith('perlr') else None,
                                 masked=name == 'masked_adam_upd')
            for got, key in ((p, 'param'), (m, 'exp_avg'), (v, 'exp_avg_sq')):
                np.testing.assert_allclose(got, z[f'{name}/{step}/{key}'], rtol=0, atol=5e-7, err_msg=f'{name}/{step}/{key}')
            if name == 'masked_adam_upd':
                untouched = z['in/grad'] == 0
                assert np.array_equal(z[f'{name}/{step}/param'][untouched], z['in/param'][untouched])      # the reference skips them
    for dense in (True, False):
        g = O.total_variation_add_grad(z['in/param'], z['in/grad'], 0.3, 0.2, 0.7, dense)
        np.testing.assert_allclose(g, z[f'tv/{"dense" if dense else "sparse"}/grad'], rtol=0, atol=5e-7)


@pytest.mark.parametrize('name', MARCH)
def test_marcher_oracle_matches_reference_native_end_to_end(name):
    """native_march_*: the march_* inputs evaluated with the reference's COMPILED kernels serving every native step (on the GPU
    box) -- per-ray outputs of the all-CPU oracle must agree to 2e-6 (device expf/powf vs libm differ by an ulp per sample)."""
    g = load_march_golden(name)
    z = np.load(os.path.join(GOLDEN, 'native_' + name + '.npz'))
    r = g['rays']
    out = marcher.forward(g['model_class'], g['model_kwargs'], g['model_state_dict'], r['rays_o'], r['rays_d'], r['viewdirs'],
                          **g['render_kwargs'])
    for k in ('rgb_marched', 'alphainv_last', 'depth'):
        if k in z.files:
            d = float(np.abs(out[k].numpy() - z[k]).max())
            assert d <= 2e-6, (k, d)
