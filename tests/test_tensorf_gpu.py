"""TensoRFGrid on the GPU (csrc/k4_tensorf.hip through nerf4k_amd.lib.grid.TensoRFGrid) against the reference-made goldens of
tests/gen_tensorf_golden.py and the fp64 oracle tests/tensorf_oracle.py.

Tolerances are measured, not chosen: per key 4 x err32, the fp32 reference's own distance from the fp64 reference (stored in the goldens; the
margin of 4 covers another summation order over components and points and FMA contraction).  Where a case has no golden key (one point, the
large-world path) the bound is the rounding-error bound of the sum written next to it, evaluated with the oracle on absolute values.
Float-atomic sums: gradients are not bitwise reproducible from run to run."""
import numpy as np
import pytest
import torch

import nerf4k_amd  # noqa: F401
from nerf4k_amd.lib import grid as kgrid, utils
from helpers import load_march_golden
import tensorf_oracle as to

pytestmark = pytest.mark.gpu
U = 2.0 ** -24                         # unit roundoff of fp32


def _grid(c, sd=None):
    g = kgrid.create_grid('TensoRFGrid', channels=c['channels'], world_size=torch.tensor(c['world']), xyz_min=[0, 0, 0], xyz_max=[1, 1, 1], config=c['config'])
    g.load_state_dict(c['sd'])
    if sd is not None:
        g.load_state_dict(sd, strict=False)
    return g.cuda()


def _arr(c, k):
    return torch.from_numpy(c['arr'][k])


def _run(g, pts, go):
    for p in g.parameters():
        p.grad = None
    out = g(pts.cuda())
    out.backward(go.cuda().reshape(out.shape))
    torch.cuda.synchronize()
    return out.detach(), {k: p.grad for k, p in g.named_parameters()}


@pytest.mark.parametrize('name,tag', [('c1', ''), ('c1', 'cell_'), ('c9', ''), ('c9', 'cell_'), ('r48', '')])
def test_lookup_and_gradients_match_the_reference(name, tag):
    c = to.load_grid_case(name)
    g = _grid(c)
    pts, go = _arr(c, tag + 'pts'), _arr(c, tag + 'go')
    out, grads = _run(g, pts, go)
    assert out.shape == ((pts.shape[0], c['channels']) if c['channels'] > 1 else (pts.shape[0],))
    with torch.no_grad():
        assert torch.equal(g(pts.cuda()), out)                       # the no-grad forward is the same kernel
    to.check(c, tag + 'out', out, f'{name}/')
    for k in grads:
        to.check(c, f'{tag}grad/{k}', grads[k], f'{name}/')
    # the exact corners of the box are inside (weight 1 on the corner node), a point beyond one voxel outside gets nothing
    if tag == '':
        want = _arr(c, 'out')
        assert float(want[0].abs().max()) > 0 and float(want[1].abs().max()) > 0


@pytest.mark.parametrize('name', ['c1', 'c9'])
@pytest.mark.parametrize('n', [0, 1])
def test_lookup_of_no_point_and_of_one_point(name, n):
    """n == 0 returns empty outputs and zero gradients without a launch.  n == 1 against the fp64 oracle: every output and gradient entry is one
    sum of at most K = 4 * 2 * (Rxy + 2R) * C products of <= 5 factors, so |error| <= (K + 5) u * (the same sum over absolute values) (u = 2^-24)."""
    c = to.load_grid_case(name)
    g = _grid(c)
    pts, go = _arr(c, 'pts')[3:3 + n], _arr(c, 'go')[3:3 + n]
    out, grads = _run(g, pts, go)
    assert out.shape == ((n, c['channels']) if c['channels'] > 1 else (n,))
    if n == 0:
        assert all(float(v.abs().max()) == 0 for v in grads.values())
        return
    sd_abs = {k: (v.abs() if k not in ('xyz_min', 'xyz_max') else v) for k, v in c['sd'].items()}
    K = 8 * (c['config']['n_comp_xy'] + 2 * c['config']['n_comp']) * c['channels'] + 5
    err = float((out.cpu().double().reshape(n, -1) - to.lookup(c['sd'], pts)).abs().max())
    bound = K * U * float(to.lookup(sd_abs, pts).max())
    print(f'{name} n=1 out: {err:.3e} <= {bound:.3e}')
    assert err <= bound
    want, wabs = to.gradients(c['sd'], pts, go), to.gradients(sd_abs, pts, go.abs())
    for k in want:
        err, bound = float((grads[k].cpu().double() - want[k]).abs().max()), K * U * float(wabs[k].max())
        print(f'{name} n=1 grad/{k}: {err:.3e} <= {bound:.3e}')
        assert err <= bound, k


def test_vectors_too_large_for_lds_take_the_atomic_path():
    """Rank 48 on a 300^3 world: the vector sums (48 * 900 floats) exceed the workgroup's LDS budget, the backward adds them with global atomics.  Against
    the fp64 oracle; bound as above with the number of points that can meet in one entry (all 700) as the number of terms."""
    gen = torch.Generator().manual_seed(3)
    g = kgrid.TensoRFGrid(3, [300, 300, 300], [0, 0, 0], [1, 1, 1], {'n_comp': 48})
    n = 700
    pts, go = torch.rand([n, 3], generator=gen) * 1.1 - 0.05, torch.randn([n, 3], generator=gen)
    sd = {k: v.detach().clone() for k, v in g.state_dict().items()}
    out, grads = _run(g.cuda(), pts, go)
    sd_abs = {k: (v.abs() if k not in ('xyz_min', 'xyz_max') else v) for k, v in sd.items()}
    K = 8 * 144 * 3 + 5
    err, bound = float((out.cpu().double() - to.lookup(sd, pts)).abs().max()), K * U * float(to.lookup(sd_abs, pts).max())
    print(f'large world out: {err:.3e} <= {bound:.3e}')
    assert err <= bound
    want, wabs = to.gradients(sd, pts, go), to.gradients(sd_abs, pts, go.abs())
    for k in want:
        err, bound = float((grads[k].cpu().double() - want[k]).abs().max()), (K + n) * U * float(wabs[k].max())
        print(f'large world grad/{k}: {err:.3e} <= {bound:.3e}')
        assert err <= bound, k


@pytest.mark.parametrize('name', ['c1', 'c9'])
def test_dense_expansion_total_variation_and_resize(name):
    c = to.load_grid_case(name)
    g = _grid(c)
    dense = g.get_dense_grid()
    assert tuple(dense.shape) == (1, c['channels'], *c['world'])
    to.check(c, 'dense', dense, f'{name}/')
    # total variation: into a missing .grad, then into a pre-existing non-zero one
    gt = _grid(c, c['tvsd'])
    assert all(p.grad is None for p in gt.parameters())
    gt.total_variation_add_grad(0.3, 0.2, 0.1, True)
    for k in to.FACTORS:
        to.check(c, 'tv/' + k, getattr(gt, k).grad, f'{name}/missing grad: ')
    if c['channels'] > 1:
        assert gt.f_vec.grad is None
    for k in to.FACTORS:
        getattr(gt, k).grad = torch.full_like(getattr(gt, k), 0.5)
    gt.total_variation_add_grad(0.3, 0.2, 0.1, False)                # dense_mode is ignored
    for k in to.FACTORS:                                             # (the one addition to the existing value rounds once more: u * |sum|)
        want = 0.5 + _arr(c, 'tv/' + k).double()
        err, bound = float((getattr(gt, k).grad.cpu().double() - want).abs().max()), to.tol(c, 'tv/' + k) + U * float(want.abs().max())
        print(f'{name}/existing grad tv/{k}: {err:.3e} <= {bound:.3e}')
        assert err <= bound, k
    old = {k: getattr(g, k) for k in to.FACTORS}
    g.scale_volume_grid([9, 8, 11])
    for k in to.FACTORS:
        assert getattr(g, k) is not old[k] and isinstance(getattr(g, k), torch.nn.Parameter)
        to.check(c, 'scaled/' + k, getattr(g, k), f'{name}/')
    assert g(torch.rand([5, 3]).cuda()).shape[0] == 5


@pytest.mark.parametrize('name', ['c1', 'c9'])
def test_factored_lookup_equals_dense_lookup_of_the_expansion(name):
    """Trilinear interpolation of sum_r plane_r (x) vec_r is the factored lookup in real arithmetic, zero padding included (the valid corners form a product
    set).  Both sides are fp32: the factored side is within 4 err32(out) of the truth, the expansion's nodes within 4 err32(dense) (a convex blend keeps
    that), and the dense blend adds 8 products + 7 sums: 12 u max|dense|."""
    c = to.load_grid_case(name)
    g = _grid(c)
    d = kgrid.DenseGrid(c['channels'], c['world'], c['sd']['xyz_min'], c['sd']['xyz_max']).cuda()
    with torch.no_grad():
        d.grid.copy_(g.get_dense_grid())
        pts = _arr(c, 'pts').cuda()
        a, b = g(pts), d(pts)
    err = float((a.double() - b.double()).abs().max())
    bound = to.tol(c, 'out') + to.tol(c, 'dense') + 12 * U * float(d.grid.detach().abs().max())
    print(f'{name}: factored vs dense lookup {err:.3e} <= {bound:.3e}')
    assert err <= bound


# ---------------------------------------------------------------------------------------------------------------- models
def _march_golden(name):
    g = load_march_golden(name)
    z = np.load(f'{__import__("helpers").GOLDEN}/{name}.npz', allow_pickle=False)
    extra = {k: z[k] for k in z.files if k.split('/')[0] in ('train', 'grad', 'out')}
    return g, extra


def _hold(extra, sec, key, got, what):
    want = torch.from_numpy(extra[f'{sec}/{key}']).double()
    t = 4 * float(extra[f'{sec}/err32/{key}'])
    err = float((got.detach().cpu().double().reshape(want.shape) - want).abs().max())
    print(f'{what} {sec}/{key}: {err:.3e} <= 4 x err32 = {t:.3e}')
    return err <= t, (what, sec, key, err, t)


FLOAT_KEYS = ('alphainv_last', 'weights', 'rgb_marched', 'rgb_feature', 'raw_alpha', 'raw_rgb', 'depth')


@pytest.mark.parametrize('name', ['tensorf_march_dvgo', 'tensorf_march_mpi'])
def test_march_goldens_staged_fused_and_training(name):
    """The reference's models with factored density and k0.  Staged path: every key, ``ray_id`` exact (the goldens' selections sit clear of the threshold: the
    generator asserts it), floats within 4 x err32.  Fused path (dense expansions through the accessor): rgb_marched / depth / alphainv_last at the
    tolerance of the fused-vs-golden test of DenseGrid models, atol 5e-6.  Training: outputs and the gradients of rgb_marched.sum() for all factor parameters."""
    g, extra = _march_golden(name)
    model = utils.model_from_checkpoint_dict(g).cuda().eval()
    assert isinstance(model.density, kgrid.TensoRFGrid) and isinstance(model.k0, kgrid.TensoRFGrid) and model._k4_fusable()
    r = {k: v.cuda() for k, v in g['rays'].items()}
    failed = []
    with torch.no_grad():
        staged = model(r['rays_o'], r['rays_d'], r['viewdirs'], k4_staged=True, **g['render_kwargs'])
        fused = model(r['rays_o'], r['rays_d'], r['viewdirs'], **g['render_kwargs'])
    ref = g['out']
    ref_keys = {k for k in ref if not k.startswith('err32/')}
    assert ref_keys <= set(staged.keys()) and set(staged.keys()) - ref_keys <= {'n_max'}      # (the generator stores the tensors of the reference's dict)
    assert torch.equal(staged['ray_id'].cpu(), ref['ray_id'].long())
    for k in FLOAT_KEYS + (('s',) if 's' in ref else ()):
        ok, info = _hold(extra, 'out', k, staged[k], name + ' staged')
        if not ok:
            failed.append(info)
    assert staged['rgb_marched'] is staged['rgb_feature']
    assert 'weights' not in fused                                       # the fused kernels ran, not the staged sequence
    for k in ('rgb_marched', 'depth', 'alphainv_last'):
        err = float((fused[k].cpu().double() - ref[k].double()).abs().max())
        print(f'{name} fused {k}: {err:.3e} <= 5e-6')
        assert err <= 5e-6, (name, k, err)
    # a second fused call reuses the cached expansions; a changed factor re-keys them
    key = ('dense', id(model.k0))
    cached = model._k4_cache()[key][1]
    with torch.no_grad():
        model(r['rays_o'], r['rays_d'], r['viewdirs'], **g['render_kwargs'])
        assert model._k4_cache()[key][1] is cached
        model.k0.x_vec.mul_(1.0)
        model(r['rays_o'], r['rays_d'], r['viewdirs'], **g['render_kwargs'])
        assert model._k4_cache()[key][1] is not cached
    # training
    model.train()
    out = model(r['rays_o'], r['rays_d'], r['viewdirs'], global_step=0, **g['render_kwargs'])
    assert torch.equal(out['ray_id'].cpu(), torch.from_numpy(extra['train/ray_id']).long())
    out['rgb_marched'].sum().backward()
    torch.cuda.synchronize()
    for k in FLOAT_KEYS:
        ok, info = _hold(extra, 'train', k, out[k], name + ' training')
        if not ok:
            failed.append(info)
    names = [k[len('grad/'):] for k in extra if k.startswith('grad/') and not k.startswith('grad/err32/')]
    assert len(names) == 13
    params = dict(model.named_parameters())
    for k in names:
        ok, info = _hold(extra, 'grad', k, params[k].grad, name)
        if not ok:
            failed.append(info)
    assert not failed, failed
