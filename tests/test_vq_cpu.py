"""CPU-side checks of the vector-quantised feature field: the restatement (tests/vq_oracle.py) against the goldens made by the reference's own classes
(tests/gen_vq_golden.py), the drop-in boundary of ``VQGrid`` / ``DirectQVGO`` (constructor, key sets, get_kwargs round trip, what raises) and the
declared entry points.  Nothing here needs a GPU."""
import os
import re

import numpy as np
import pytest
import torch

import nerf4k_amd  # noqa: F401
from nerf4k_amd import _native as N, scene
from nerf4k_amd.lib import dmpigo, dvqgo, grid, utils
from helpers import GOLDEN, load_march_golden
import vq_oracle as vo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARCH = ['march_dvqgo_base', 'march_dvqgo_half', 'march_dvqgo_deep_opaque', 'march_dvqgo_w64_d2']
GRID_CASES = ['base', 'one', 'odd', 'chunked']
# the reference's keys (lib/grid.py:46-58, lib/dvqgo.py:32-142 on a CPU build of its modules)
VQ_KEYS = {'xyz_min', 'xyz_max', 'embed', 'cluster_size', 'embed_avg', 'project_layer.0.weight', 'project_layer.0.bias', 'project_layer.2.weight',
           'project_layer.2.bias'}
REF_KWARGS = {'xyz_min', 'xyz_max', 'num_voxels', 'mpi_depth', 'voxel_size_ratio', 'mask_cache_path', 'mask_cache_thres', 'mask_cache_world_size',
              'fast_color_thres', 'density_type', 'k0_type', 'density_config', 'k0_config', 'mode_type', 'act_type', 'rgbnet_dim', 'rgbnet_depth',
              'rgbnet_width', 'viewbase_pe', 'spatial_pe'}


def load_grid_case(name):
    """-> (state dict of a VQGrid, x, expectations) of one bare-grid fixture; fp16-stored arrays widen exactly."""
    z = np.load(os.path.join(GOLDEN, 'vq_grid.npz'), allow_pickle=False)
    p = name + '/'
    sd = {k[len(p) + 3:]: torch.from_numpy(z[k].astype(np.float32)) for k in z.files if k.startswith(p + 'sd/')}
    sd.setdefault('embed_avg', sd['embed'].clone())
    want = {k[len(p):]: torch.from_numpy(z[k].astype(np.int64) if z[k].dtype == np.int16 else z[k]) for k in z.files
            if k.startswith(p) and not k.startswith(p + 'sd/') and k != p + 'x'}
    return sd, torch.from_numpy(z[p + 'x'].astype(np.float32)), want


@pytest.mark.parametrize('name', GRID_CASES)
def test_restatement_equals_the_grid_golden(name):
    sd, x, want = load_grid_case(name)
    in_dim, dim, n_embed, n = want['shape'].tolist()
    assert x.shape == (n, in_dim) and sd['embed'].shape == (dim, n_embed)
    st, aux = vo.vq_state(sd), {}
    q, diff, ind = vo.vq_forward(st, x, aux=aux)
    assert torch.equal(ind, want['ind']) and torch.equal(aux['v'], want['v']) and torch.equal(diff, want['diff'])
    assert torch.equal(q, want['v'] + (sd['embed'].t()[want['ind']] - want['v']))
    if 'train1/ind' in want:
        for i, xi in enumerate((x, x, x[:0])):
            _, d, ind = vo.vq_forward(st, xi, training=True)
            t = f'train{i + 1}/'
            assert torch.equal(ind, want[t + 'ind'])
            assert torch.equal(d, want[t + 'diff']) or (xi.numel() == 0 and bool(torch.isnan(d)) and bool(torch.isnan(want[t + 'diff'])))
            for k in ('cluster_size', 'embed_avg', 'embed'):
                assert torch.equal(st[k], want[t + k]), (t, k)
                assert float(want[t + 'spread/' + k]) > 0


@pytest.mark.parametrize('name', MARCH)
def test_restatement_equals_the_model_golden(name):
    g = load_march_golden(name)
    r = g['rays']
    assert r['rays_o'].shape == (67, 3)
    aux = {}
    out = vo.forward(g['model_kwargs'], g['model_state_dict'], r['rays_o'], r['rays_d'], r['viewdirs'], aux=aux, **g['render_kwargs'])
    ref = g['out']
    assert set(ref) | {'rgb_feature'} == set(out)
    assert torch.equal(out['ray_id'], ref['ray_id'].long()) and torch.equal(out['s'], ref['s']) and int(ref['n_max']) == out['n_max']
    z = np.load(os.path.join(GOLDEN, name + '.npz'))
    assert np.array_equal(aux['embed_ind'].numpy(), z['aux/embed_ind']) and np.array_equal(aux['step_id'].numpy(), z['aux/step_id'])
    for k in ('weights', 'raw_alpha', 'raw_rgb', 'rgb_marched', 'depth', 'alphainv_last'):
        assert torch.allclose(out[k], ref[k], rtol=0, atol=1e-6), (k, float((out[k] - ref[k]).abs().max()))


def test_create_grid_returns_a_vqgrid_with_the_reference_keys():
    vq = grid.create_grid('VQGrid', input_dim=15, channels=6, world_size=64, xyz_min=[-1, -1, -1], xyz_max=[1, 1, 1], config={})
    assert isinstance(vq, grid.VQGrid) and (vq.dim, vq.n_embed, vq.decay, vq.eps) == (6, 64, 0.99, 1e-5)
    sd = vq.state_dict()
    assert set(sd) == VQ_KEYS
    assert sd['embed'].shape == (6, 64) and sd['cluster_size'].shape == (64,) and sd['embed_avg'].shape == (6, 64)
    assert sd['project_layer.0.weight'].shape == (6, 15) and sd['project_layer.2.weight'].shape == (6, 6)
    assert torch.equal(sd['embed'], sd['embed_avg']) and not bool(sd['cluster_size'].any())         # lib/grid.py:49-52
    assert not [k for k, _ in vq.named_parameters() if not k.startswith('project_layer.')]
    with pytest.raises(NotImplementedError, match='VQGrid'):
        grid.create_grid('HashGrid')


@pytest.mark.parametrize('name', MARCH)
def test_checkpoint_contract(name):
    """load_model semantics (lib/utils.py:62-66): the reference's key set loads strictly, and -- unlike upstream, whose get_kwargs() omits n_cluster --
    the model rebuilds from its own get_kwargs()."""
    g = load_march_golden(name)
    model = utils.model_from_checkpoint_dict(g)
    assert isinstance(model, dvqgo.DirectQVGO) and isinstance(model, dmpigo.DirectMPIGO) and isinstance(model.k0, grid.VQGrid)
    assert set(model.state_dict()) == set(g['model_state_dict'])
    assert {k[3:] for k in model.state_dict() if k.startswith('k0.')} == VQ_KEYS
    kw = model.get_kwargs()
    assert set(kw) == REF_KWARGS | {'n_cluster'}
    model2 = dvqgo.DirectQVGO(**kw)
    model2.load_state_dict(model.state_dict())
    for k, v in model.state_dict().items():
        assert torch.equal(model2.state_dict()[k], v), k
    assert model2.k0.project_layer[0].in_features == 3 + 6 * kw['spatial_pe']


def test_load_model_round_trips_through_a_checkpoint_file(tmp_path):
    ck = scene.make_vq_checkpoint(seed=3, num_voxels=12 * 12 * 8, mpi_depth=8)
    assert ck['model_class'] == 'DirectQVGO' and ck['model_kwargs']['k0_type'] == 'VQGrid'
    model = utils.model_from_checkpoint_dict(ck)
    path = str(tmp_path / 'fine_last.tar')
    torch.save({'global_step': 1, 'model_kwargs': model.get_kwargs(), 'model_state_dict': model.state_dict()}, path)
    again = utils.load_model(dvqgo.DirectQVGO, path)
    assert again.n_cluster == 64 and all(torch.equal(v, again.state_dict()[k]) for k, v in model.state_dict().items())


def test_cpu_tensors_raise():
    g = load_march_golden('march_dvqgo_base')
    model = utils.model_from_checkpoint_dict(g)
    r = g['rays']
    with pytest.raises(N.K4Error):
        model(r['rays_o'], r['rays_d'], r['viewdirs'], **g['render_kwargs'])
    with pytest.raises(N.K4Error):
        model.k0(torch.zeros(4, 15))
    with pytest.raises(N.K4Error):
        model.k0.project(torch.zeros(4, 15))
    with pytest.raises(N.K4Error):
        model.k0.embed_code(torch.zeros(4, dtype=torch.long))


def test_what_upstream_cannot_run_raises_with_the_reason():
    kw = utils.model_from_checkpoint_dict(load_march_golden('march_dvqgo_base')).get_kwargs()
    for mode in ('TRANS', 'adain', 'adain_vq'):
        with pytest.raises(NotImplementedError, match='never defines'):
            dvqgo.DirectQVGO(**dict(kw, mode_type=mode))
    with pytest.raises(NotImplementedError, match='relu'):
        dvqgo.DirectQVGO(**dict(kw, act_type='gauss'))
    with pytest.raises(NotImplementedError, match='viewbase_pe'):
        dvqgo.DirectQVGO(**dict(kw, viewbase_pe=2))
    with pytest.raises(NotImplementedError, match='rgbnet_dim'):
        dvqgo.DirectQVGO(**dict(kw, rgbnet_dim=0))
    with pytest.raises(NotImplementedError, match='VQGrid'):
        dvqgo.DirectQVGO(**dict(kw, k0_type='DenseGrid'))
    model = dvqgo.DirectQVGO(**kw)
    with pytest.raises(NotImplementedError, match='total_variation'):
        model.k0_total_variation_add_grad(1e-3, True)


def test_entry_points_are_declared():
    hdr = open(os.path.join(ROOT, 'include', 'k4nerf.h')).read()
    assert int(re.search(r'#define\s+K4_ABI_VERSION\s+(\d+)', hdr).group(1)) == N.K4_ABI_VERSION >= 22
    for name in ('k4_vq_project_fwd', 'k4_vq_project_bwd_workspace_bytes', 'k4_vq_project_bwd', 'k4_vq_codebook_floats', 'k4_vq_chunk_codes',
                 'k4_vq_prepare_codebook', 'k4_vq_assign_workspace_bytes', 'k4_vq_assign', 'k4_vq_update_codebook'):
        assert re.search(r'\b' + name + r'\s*\(', hdr), name
        assert name in N._EXTRA_SIGS, name
        assert hasattr(N.lib(), name), name
    # the one-launch entry point and its descriptor: the loader's mirror has the header's fields in the header's order
    for name in ('k4_march_vq_fwd', 'k4_grid_sample_3d_backward_terms', 'k4_sorted_segment_add'):
        assert re.search(r'\b' + name + r'\s*\(', hdr) and name in N._EXTRA_SIGS and hasattr(N.lib(), name), name
    body = re.search(r'typedef struct k4_vq_desc \{(.*?)\} k4_vq_desc;', hdr, re.S).group(1)
    fields = [re.sub(r'\[\d+\]', '', d.split()[-1].lstrip('*')) for d in body.replace('\n', ' ').split(';') if d.strip()]
    assert fields == [f[0] for f in N.VqDesc._fields_], (fields, [f[0] for f in N.VqDesc._fields_])
    assert N.C.sizeof(N.VqDesc) % 8 == 0 and N.VqDesc.n_samples.offset == N.VqDesc.n_rays.offset + 8
    # sizes the host derives without a device: a prepared row is the codeword, |e|^2, padded to 16 bytes; a chunk fits 48 KB of LDS
    L = N.lib()
    assert L.k4_vq_codebook_floats(6, 64) == 64 * 8 and L.k4_vq_codebook_floats(32, 2500) == 2500 * 36
    assert L.k4_vq_chunk_codes(32) * 36 * 4 <= 48 * 1024 < (L.k4_vq_chunk_codes(32) + 1) * 36 * 4
    assert L.k4_vq_chunk_codes(32) < 2500                     # the 2500-code fixture is walked in chunks
    assert L.k4_vq_codebook_floats(33, 64) < 0 and L.k4_vq_project_bwd_workspace_bytes(10, 64, 6) < 0
