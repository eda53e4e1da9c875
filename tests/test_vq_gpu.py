"""GPU parity of the vector-quantised feature field (csrc/k4_vq.hip, lib/grid.VQGrid, lib/dvqgo.DirectQVGO) against goldens made by the reference's own
classes on the CPU (tests/gen_vq_golden.py).

The generator asserts that every vector reaching a codebook has a best / second-best distance gap above 1e-5 * max|dist| -- about 40 fp32 dot-product
rounding bounds -- so the chosen indices are compared EXACTLY and no sample is excluded.  Tolerances, none of them new:
  * projected vectors, diff, returned features: |err| <= 2e-6 * max|want| + 2e-7, what tests/test_train_ops_gpu.py allows k4_rgbnet_fwd against its
    oracle (the same arithmetic class: fp32 FMA chains against CPU Linear layers);
  * cluster_size: 2 ulp (2.4e-7 relative), the native kernels' tolerance of tests/helpers.py; embed_avg / embed: 4 x the spread the fixture stores per
    training call between the reference's fp32 buffers and an fp64 update (the sums depend on the summation order);
  * the model: index lists exact, values within 3e-6 (the staged path of tests/test_march_gpu.py); the one launch within 5e-6 of the golden and of
    the staged path (that file's bound for the fused call);
  * gradients: |err| <= 2e-5 * max|grad| + 1e-9, as tests/test_train_gpu.py for grad_mpi.npz.
"""
import copy
import json
import os

import numpy as np
import pytest
import torch

import nerf4k_amd  # noqa: F401
from nerf4k_amd import _native as N, render, scene
from nerf4k_amd.lib import dvqgo, grid, utils
from helpers import GOLDEN, load_march_golden
from test_vq_cpu import GRID_CASES, MARCH, load_grid_case
import vq_oracle as vo

pytestmark = pytest.mark.gpu


def _close(got, want, name, rel=2e-6, abs_=2e-7):
    got, want = got.detach().cpu().double(), want.detach().double()
    assert got.shape == want.shape, (name, got.shape, want.shape)
    scale = float(want.abs().max()) if want.numel() else 0.0
    err = float((got - want).abs().max()) if want.numel() else 0.0
    print(f'{name}: max|err| {err:.3e}, bound {rel * scale + abs_:.3e}')
    assert err <= rel * scale + abs_, (name, err, scale)


def _vq(sd):
    dim, n_embed = sd['embed'].shape
    vq = grid.create_grid('VQGrid', input_dim=sd['project_layer.0.weight'].shape[1], channels=dim, world_size=n_embed, xyz_min=[-1, -1, -1],
                          xyz_max=[1, 1, 1], config={})
    vq.load_state_dict(dict(sd, xyz_min=vq.xyz_min, xyz_max=vq.xyz_max))
    return vq.cuda().eval()


@pytest.mark.parametrize('name', GRID_CASES)
def test_lookup_matches_the_reference(name):
    sd, x, want = load_grid_case(name)
    vq = _vq(sd)
    before = {k: v.clone() for k, v in vq.state_dict().items()}
    versions = [b._version for b in (vq.embed, vq.cluster_size, vq.embed_avg)]
    with torch.no_grad():
        q, diff, ind = vq(x.cuda())
        v = vq.project(x.cuda())
    assert ind.dtype == torch.int64 and q.shape == (x.shape[0], vq.dim) and diff.shape == () and diff.dtype == torch.float32
    assert torch.equal(ind.cpu(), want['ind'])
    assert torch.equal(q, v + (vq.embed.t()[ind] - v))                      # lib/grid.py:96 on the kernel's own v: not the codeword itself
    assert torch.equal(vq.embed_code(ind), vq.embed.t()[ind])
    _close(v, want['v'], 'v')
    _close(diff, want['diff'], 'diff')
    _close(q, want['v'] + (sd['embed'].t()[want['ind']] - want['v']), 'quantize')
    # eval mode leaves the buffers bit-identical and their versions alone
    assert all(torch.equal(before[k], t) for k, t in vq.state_dict().items())
    assert versions == [b._version for b in (vq.embed, vq.cluster_size, vq.embed_avg)]
    with torch.no_grad():                                                   # the same inputs give the same bits
        q2, diff2, ind2 = vq(x.cuda())
    assert torch.equal(q, q2) and torch.equal(diff, diff2) and torch.equal(ind, ind2)


def test_lookup_of_an_empty_input_and_of_leading_axes():
    sd, x, want = load_grid_case('base')
    vq = _vq(sd)
    with torch.no_grad():
        q, diff, ind = vq(x[:0].cuda())
        assert q.shape == (0, 6) and ind.shape == (0,) and bool(torch.isnan(diff))        # torch's mean of nothing
        q, diff, ind = vq(x[:0].reshape(0, 4, 15).cuda())
        assert q.shape == (0, 4, 6) and ind.shape == (0, 4)
        q, diff, ind = vq(x.reshape(8, 125, 15).cuda())
    assert q.shape == (8, 125, 6) and torch.equal(ind.cpu().reshape(-1), want['ind'])


def test_the_lowest_index_wins_an_exact_tie_within_a_chunk_and_across_chunks():
    dim = 8
    chunk = int(N.lib().k4_vq_chunk_codes(dim))
    n_embed = chunk + 76
    g = torch.Generator().manual_seed(11)
    embed = torch.randn([dim, n_embed], generator=g)
    # (first, copy): inside the first chunk, across the boundary (twice, one of them with a third copy), inside the second chunk
    pairs = [(5, 17), (100, chunk + 3), (chunk - 1, chunk), (chunk + 10, chunk + 70)]
    for a, b in pairs:
        embed[:, b] = embed[:, a]
    embed[:, chunk + 40] = embed[:, 100]
    vq = grid.VQGrid(input_dim=dim, channels=dim, world_size=n_embed, xyz_min=[-1, -1, -1], xyz_max=[1, 1, 1])
    with torch.no_grad():
        # v = (x + 16) - 16: the projection hands the point through to within rounding, so a point placed on a codeword is nearest to it
        vq.project_layer[0].weight.copy_(torch.eye(dim)); vq.project_layer[0].bias.fill_(16.)
        vq.project_layer[2].weight.copy_(torch.eye(dim)); vq.project_layer[2].bias.fill_(-16.)
        vq.embed.copy_(embed)
    cols = [a for a, _ in pairs] + [b for _, b in pairs] + [chunk + 40] + list(range(0, n_embed, 97))
    x = embed[:, cols].t().contiguous()
    st = vo.vq_state(vq.state_dict())
    _, _, want = vo.vq_forward(st, x)                                        # (-dist).max(1) on the CPU returns the first maximum
    first = {b: a for a, b in pairs}
    first[chunk + 40] = 100
    assert want.tolist() == [first.get(c, c) for c in cols]
    vq = vq.cuda().eval()
    with torch.no_grad():
        _, _, ind = vq(x.cuda())
    assert ind.cpu().tolist() == want.tolist()


@pytest.mark.parametrize('name', ['base', 'one'])
def test_training_mode_moves_the_codebook_as_the_reference_does(name):
    sd, x, want = load_grid_case(name)
    vq = _vq(sd)
    with torch.no_grad():
        q_eval, _, _ = vq(x.cuda())
    vq.train()
    bufs = ('cluster_size', 'embed_avg', 'embed')
    for i, xi in enumerate((x, x, x[:0])):
        t = f'train{i + 1}/'
        old = vq.embed.clone()
        versions = [getattr(vq, k)._version for k in bufs]
        ptrs = [getattr(vq, k).data_ptr() for k in bufs]
        with torch.no_grad():                                               # whatever the autograd mode
            q, diff, ind = vq(xi.cuda())
            v = vq.project(xi.cuda())
        assert torch.equal(ind.cpu(), want[t + 'ind'])
        assert torch.equal(q, v + (old.t()[ind] - v))                       # the features come from the OLD codebook
        if i == 0:
            assert torch.equal(q, q_eval)
        if xi.numel():
            _close(diff, want[t + 'diff'], t + 'diff')
        else:
            assert bool(torch.isnan(diff))
        assert all(getattr(vq, k)._version > ver for k, ver in zip(bufs, versions))          # in place, versions bumped
        assert ptrs == [getattr(vq, k).data_ptr() for k in bufs]
        cs, cs_want = vq.cluster_size.cpu().double(), want[t + 'cluster_size'].double()
        err = float(((cs - cs_want).abs() / cs_want.abs()).max())
        print(f'{t}cluster_size: max relative error {err:.3e}')
        assert err <= 2.4e-7, (t, err)
        for k in ('embed_avg', 'embed'):
            err = float((getattr(vq, k).cpu().double() - want[t + k].double()).abs().max())
            bound = 4 * float(want[t + 'spread/' + k])
            print(f'{t}{k}: max|err| {err:.3e}, 4 x spread {bound:.3e}')
            assert err <= bound, (t, k, err, bound)
    # ... and the next lookup uses the moved codebook
    vq.eval()
    with torch.no_grad():
        q, _, ind = vq(x.cuda())
        v = vq.project(x.cuda())
    assert torch.equal(q, v + (vq.embed.t()[ind] - v))


def test_straight_through_gradient_of_the_grid():
    sd, x, _ = load_grid_case('base')
    vq = _vq(sd)
    x = x[:300]
    g = torch.Generator().manual_seed(5)
    gq = torch.randn([300, 6], generator=g)
    # the restatement under fp32 autograd on the CPU
    st = {k: (v.requires_grad_(True) if k.startswith('project_layer') else v) for k, v in vo.vq_state(sd).items()}
    xr = x.clone().requires_grad_(True)
    q, diff, _ = vo.vq_forward(st, xr)
    ((q * gq).sum() + 3.0 * diff).backward()
    xd = x.cuda().requires_grad_(True)
    qd, dd, _ = vq(xd)
    ((qd * gq.cuda()).sum() + 3.0 * dd).backward()
    names = {'project_layer.0.weight': vq.project_layer[0].weight, 'project_layer.0.bias': vq.project_layer[0].bias,
             'project_layer.2.weight': vq.project_layer[2].weight, 'project_layer.2.bias': vq.project_layer[2].bias}
    for k, p in names.items():
        _close(p.grad, st[k].grad, k, rel=2e-5, abs_=1e-9)
    _close(xd.grad, xr.grad, 'grad_x', rel=2e-5, abs_=1e-9)
    assert all(b.grad is None and not b.requires_grad for b in (vq.embed, vq.cluster_size, vq.embed_avg))
    # an input that does not require a gradient gets none computed
    vq.zero_grad(set_to_none=True)
    x2 = x.cuda()
    vq(x2)[0].sum().backward()
    assert x2.grad is None and vq.project_layer[0].weight.grad is not None


def _model(g):
    return utils.model_from_checkpoint_dict(g).cuda().eval()


@pytest.mark.parametrize('name', MARCH)
def test_model_golden(name):
    g = load_march_golden(name)
    model = _model(g)
    r = {k: v.cuda() for k, v in g['rays'].items()}
    ref = g['out']
    z = np.load(os.path.join(GOLDEN, name + '.npz'))
    with torch.no_grad():
        staged = model(r['rays_o'], r['rays_d'], r['viewdirs'], k4_staged=True, **g['render_kwargs'])
        out = model(r['rays_o'], r['rays_d'], r['viewdirs'], k4_fused=True, **g['render_kwargs'])
        auto = model(r['rays_o'], r['rays_d'], r['viewdirs'], **g['render_kwargs'])
    # by itself the model takes the one launch only where it was measured to pay (profiles/dvqgo_call_time.md): width 32, <= 8 channels, a small codebook
    assert ('weights' in auto) == (name == 'march_dvqgo_w64_d2')
    assert set(ref.keys()) | {'rgb_feature'} == set(staged.keys())
    assert torch.equal(staged['ray_id'].cpu(), ref['ray_id'].long()) and staged['n_max'] == int(ref['n_max'])
    # step_id through s = (step_id + 0.5) / N_samples: exact once rounded back (the device's division by a scalar may differ from the CPU's in the last bit)
    assert float((staged['s'].cpu() - ref['s']).abs().max()) <= 1.2e-7
    assert np.array_equal(np.round(staged['s'].cpu().numpy() * staged['n_max'] - 0.5).astype(np.int64), z['aux/step_id'])
    for k in ('weights', 'raw_alpha', 'raw_rgb', 'rgb_marched', 'depth', 'alphainv_last'):
        err = float((staged[k].cpu() - ref[k]).abs().max())
        print(f'{name} staged {k}: max|err| {err:.3e}')
        assert err <= 3e-6, (k, err)
    assert staged['rgb_marched'] is staged['rgb_feature']
    # the one launch: no per-sample tensors, the values of the golden and of the staged path
    assert set(out) == {'rgb_marched', 'rgb_feature', 'alphainv_last', 'depth', 'n_max'} and out['n_max'] == staged['n_max']
    for k in ('rgb_marched', 'depth', 'alphainv_last'):
        err, err_s = float((out[k].cpu() - ref[k]).abs().max()), float((out[k] - staged[k]).abs().max())
        print(f'{name} fused {k}: max|err| {err:.3e} against the golden, {err_s:.3e} against the staged path')
        assert err <= 5e-6 and err_s <= 5e-6, (name, k, err, err_s)
    assert out['rgb_marched'] is out['rgb_feature']
    with torch.no_grad():                                                               # the same inputs give the same bits
        again = model(r['rays_o'], r['rays_d'], r['viewdirs'], k4_fused=True, **g['render_kwargs'])
    assert all(torch.equal(out[k], again[k]) for k in ('rgb_marched', 'depth', 'alphainv_last'))
    with torch.no_grad():                                                               # ... and without render_depth there is no depth
        kw = dict(g['render_kwargs'], render_depth=False, k4_fused=True)
        assert 'depth' not in model(r['rays_o'], r['rays_d'], r['viewdirs'], **kw)


def test_one_launch_with_more_than_64_survivors_on_a_ray_and_without_thresholds():
    """fast_color_thres = 0 on an all-occupied mask: every in-box sample up to the T < 1e-3 stop is shaded (lib/dvqgo.py:305,314 skip both filters), so a
    ray of 159 samples queues more than 64 survivors -- the queue is flushed mid-ray and its rest moved -- and shades in its second and third 64-lane chunk.
    The frame contract of tests/test_march_gpu.py between the one launch and the staged path."""
    ck = scene.make_vq_checkpoint(seed=44, num_voxels=32 * 32 * 80, mpi_depth=80, stepsize=0.5, n_blobs=6)
    ck['model_kwargs']['fast_color_thres'] = 0
    ck['model_state_dict']['mask_cache.mask'] = torch.ones_like(ck['model_state_dict']['mask_cache.mask'])
    model = _model(ck)
    H, W = 24, 32
    K = scene.LLFF_K.copy()
    K[:2] *= W / scene.LLFF_HW[1]
    from nerf4k_amd.lib import dvgo
    ro, rd, vd = [t.reshape(-1, 3) for t in dvgo.get_rays_of_a_view(H, W, K, torch.from_numpy(scene.llff_spiral_poses()[2]).cuda(), True, inverse_y=False,
                                                                    flip_x=False, flip_y=False)]
    with torch.no_grad():
        staged = model(ro, rd, vd, k4_staged=True, **ck['render_kwargs'])
        out = model(ro, rd, vd, k4_fused=True, **ck['render_kwargs'])
    live = staged['weights'] > 0                                  # (the staged path keeps the zero-weight samples behind the stop)
    per_ray = torch.bincount(staged['ray_id'][live], minlength=ro.shape[0])
    last = (staged['s'][live] * staged['n_max'] - 0.5).round().max()
    print(f'most weighted samples on a ray {int(per_ray.max())}, last weighted step {int(last)} of {staged["n_max"]}')
    assert 'weights' not in out and int(per_ray.max()) > 64 and int(last) >= 128
    for k in ('rgb_marched', 'depth', 'alphainv_last'):
        d = (out[k] - staged[k]).abs()
        d = d.amax(-1) if d.dim() > 1 else d
        print(f'{k}: max|err| {float(d.max()):.3e}')
        assert float((d <= 2e-5).float().mean()) >= 0.999 and float(d.max()) <= 2e-3, (k, float(d.max()))


@pytest.mark.parametrize('cfg', [
    dict(seed=41, num_voxels=40 * 40 * 80, mpi_depth=80, rgbnet_width=128, rgbnet_depth=3, n_cluster=300, rgbnet_dim=12, spatial_pe=4, opaque=True),
    dict(seed=42, num_voxels=48 * 48 * 40, mpi_depth=40, rgbnet_width=128, rgbnet_depth=2, n_cluster=1, rgbnet_dim=1, spatial_pe=0, stepsize=0.5),
    dict(seed=43, num_voxels=48 * 48 * 40, mpi_depth=40, rgbnet_width=32, rgbnet_depth=3, n_cluster=2500, rgbnet_dim=32, spatial_pe=10),
])
def test_one_launch_frame_equals_the_staged_path(cfg):
    """A 48x64 frame, shapes at the limits (63 embedded inputs, 32 channels, one codeword, width 128, two 64-lane chunks per ray): the frame contract
    of tests/test_march_gpu.py (>= 99.9 % of the rays within 2e-5, every ray within 2e-3) between the one launch and the staged path."""
    ck = scene.make_vq_checkpoint(**cfg)
    model = _model(ck)
    H, W = 48, 64
    K = scene.LLFF_K.copy()
    K[:2] *= W / scene.LLFF_HW[1]
    from nerf4k_amd.lib import dvgo
    ro, rd, vd = [t.reshape(-1, 3) for t in dvgo.get_rays_of_a_view(H, W, K, torch.from_numpy(scene.llff_spiral_poses()[7]).cuda(), True, inverse_y=False,
                                                                    flip_x=False, flip_y=False)]
    with torch.no_grad():
        staged = model(ro, rd, vd, k4_staged=True, **ck['render_kwargs'])
        out = model(ro, rd, vd, k4_fused=True, **ck['render_kwargs'])
    assert 'weights' in staged and 'weights' not in out and staged['ray_id'].numel() > 1000
    for k in ('rgb_marched', 'depth', 'alphainv_last'):
        d = (out[k] - staged[k]).abs()
        d = d.amax(-1) if d.dim() > 1 else d
        print(f'{k}: max|err| {float(d.max()):.3e}, within 2e-5: {float((d <= 2e-5).float().mean()):.5f}')
        assert float((d <= 2e-5).float().mean()) >= 0.999 and float(d.max()) <= 2e-3, (k, float(d.max()))


@pytest.mark.parametrize('name', MARCH)
def test_model_chooses_the_reference_codewords(name):
    """The codebook indices of the shaded samples on the staged path, exact: the model's own embedding and projection feed the search (the one launch
    uses the same expressions and is held to the golden's colours above)."""
    g = load_march_golden(name)
    model = _model(g)
    z = np.load(os.path.join(GOLDEN, name + '.npz'))
    r = {k: v.cuda() for k, v in g['rays'].items()}
    seen = {}
    hook = model.k0.register_forward_hook(lambda m, a, o: seen.update(ind=o[2]))
    with torch.no_grad():
        model(r['rays_o'], r['rays_d'], r['viewdirs'], k4_staged=True, **g['render_kwargs'])
    hook.remove()
    assert np.array_equal(seen['ind'].cpu().numpy(), z['aux/embed_ind'])


def _load_grad_golden():
    z = np.load(os.path.join(GOLDEN, 'grad_dvqgo.npz'), allow_pickle=False)
    kw = json.loads(str(z['model_kwargs_json']))
    for k in ('xyz_min', 'xyz_max'):
        kw[k] = np.asarray(kw[k], dtype=np.float32)
    part = lambda p: {k[len(p):]: torch.from_numpy(z[k]) for k in z.files if k.startswith(p)}
    ck = {'model_class': str(z['model_class']), 'model_kwargs': kw, 'model_state_dict': part('sd/')}
    return ck, json.loads(str(z['render_kwargs_json'])), part('in/'), part('cot/'), float(z['loss']), part('grad/'), torch.from_numpy(z['out/ray_id'])


def _loss_and_backward(model, rk, rays, cot):
    with torch.enable_grad():
        out = model(rays['rays_o'].cuda(), rays['rays_d'].cuda(), rays['viewdirs'].cuda(), global_step=0, **rk)
        loss = sum((out[k] * c.cuda()).sum() for k, c in cot.items())
        loss.backward()
    return out, loss.detach()


def test_gradients_match_the_reference():
    ck, rk, rays, cot, loss_ref, grads, ray_id = _load_grad_golden()
    model = utils.model_from_checkpoint_dict(ck).cuda().eval()
    out, loss = _loss_and_backward(model, rk, rays, cot)
    assert torch.equal(out['ray_id'].cpu(), ray_id.long())
    # the loss is sum(out * cot): every output value may be off by the staged path's 3e-6, weighted by its cotangent
    bound = 3e-6 * sum(float(c.abs().sum()) for c in cot.values())
    assert abs(float(loss) - loss_ref) <= bound, (float(loss), loss_ref, bound)
    named = dict(model.named_parameters())
    assert {'density.grid'} | {k for k in grads if k.startswith(('k0.project_layer.', 'rgbnet.'))} == set(grads) and set(grads) <= set(named)
    for k, want in grads.items():
        assert named[k].grad is not None, k
        _close(named[k].grad, want, k, rel=2e-5, abs_=1e-9)
    assert all(b.grad is None for b in (model.k0.embed, model.k0.cluster_size, model.k0.embed_avg))


def test_same_state_gives_the_same_bits():
    """The training-mode forward + backward twice from copies of one state: outputs, every gradient (density.grid's too: DirectQVGO switches its density
    grid to the fixed-order gradient, DenseGrid.ordered_grad) and the moved buffers are bit-equal."""
    ck, rk, rays, cot, _, _, _ = _load_grad_golden()
    base = utils.model_from_checkpoint_dict(ck).cuda().train()
    assert base.density.ordered_grad
    runs = []
    for _ in range(2):
        m = copy.deepcopy(base)
        out, loss = _loss_and_backward(m, rk, rays, cot)
        runs.append((m, out, loss))
    (m0, o0, l0), (m1, o1, l1) = runs
    assert torch.equal(l0, l1)
    for k in ('rgb_marched', 'alphainv_last', 'weights', 'raw_rgb', 'raw_alpha', 'ray_id', 's'):
        assert torch.equal(o0[k], o1[k]), k
    g0, g1 = dict(m0.named_parameters()), dict(m1.named_parameters())
    assert 'density.grid' in g0 and float(g0['density.grid'].grad.abs().max()) > 0
    for k in g0:
        if g0[k].requires_grad:
            assert g0[k].grad is not None and torch.equal(g0[k].grad, g1[k].grad), k
    for k in ('embed', 'cluster_size', 'embed_avg'):
        assert torch.equal(getattr(m0.k0, k), getattr(m1.k0, k)), k
        assert not torch.equal(getattr(m0.k0, k), getattr(base.k0, k)), k               # training mode moved them
    # training mode without autograd moves them as well, and takes the same path
    m2 = copy.deepcopy(base)
    with torch.no_grad():
        o2 = m2(rays['rays_o'].cuda(), rays['rays_d'].cuda(), rays['viewdirs'].cuda(), **rk)
    assert 'weights' in o2 and torch.equal(m2.k0.embed, m0.k0.embed)


def test_render_viewpoints_from_a_checkpoint_file(tmp_path):
    ck = scene.make_vq_checkpoint(seed=6, num_voxels=40 * 40 * 32, mpi_depth=32)
    path = str(tmp_path / 'fine_last.tar')
    torch.save({'global_step': 0, 'model_kwargs': ck['model_kwargs'], 'model_state_dict': ck['model_state_dict']}, path)
    model = utils.load_model(dvqgo.DirectQVGO, path).cuda().eval()
    H, W = 24, 32
    K = scene.LLFF_K.copy()
    K[:2] *= W / scene.LLFF_HW[1]
    poses = torch.from_numpy(scene.llff_spiral_poses()[:2])
    rgbs, depths, bgmaps, psnrs, viewdirs_all, feats = render.render_viewpoints(model, poses, np.array([[H, W]] * 2), np.stack([K, K]), ndc=True,
                                                                               render_kwargs=ck['render_kwargs'])
    assert np.asarray(rgbs).shape == (2, H, W, 3) and np.asarray(depths).shape == (2, H, W, 1) and np.asarray(bgmaps).shape == (2, H, W, 1)
    assert np.isfinite(np.asarray(rgbs)).all() and float(np.asarray(rgbs).std()) > 1e-3
    from oracle import marcher
    ro, rd, vd = marcher.get_rays_of_a_view(H, W, K, poses[0].numpy(), ndc=True)
    want = vo.forward(ck['model_kwargs'], ck['model_state_dict'], ro.reshape(-1, 3), rd.reshape(-1, 3), vd.reshape(-1, 3), **ck['render_kwargs'])
    d = np.abs(np.asarray(feats)[0].reshape(-1, 3) - want['rgb_marched'].numpy()).max(-1)
    # the frame contract of tests/test_march_gpu.py: >= 99.9 % of the rays within 2e-5, every ray within 2e-3
    assert float((d <= 2e-5).mean()) >= 0.999 and float(d.max()) <= 2e-3, (float((d <= 2e-5).mean()), float(d.max()))
