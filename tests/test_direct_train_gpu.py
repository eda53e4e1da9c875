"""The fused direct-colour training step (lib/train_ops.dvgo_direct_render_loss: k4_direct_train_fwd / _bwd) against the staged path -- ``model(...,
k4_staged=True)`` under autograd plus the eager loss lines of run_sr.py:523-546 -- on the same inputs, and both against the fp64 oracle of
tests/direct_train_oracle.py evaluated on the staged path's own sample list.

Exact: ``alphainv_last``, the per-ray shaded count (bincount of the staged ray_id), a second fused forward against the first.
Toleranced: ``rgb_marched``, every loss term and both gradients.  With x64 the oracle's value and E(x) = max|x - x64| / max|x64|, a tensor passes when
E(fused) <= max(4 E(staged), n 2^-24); n = the largest number of terms one of its sums takes (samples of the longest ray for the per-ray values and
the loss terms, contributions to the busiest voxel for a gradient), read from the staged list.  Both errors are printed per tensor.
"""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import nerf4k_amd  # noqa: F401
from nerf4k_amd import _native as N, scene
from nerf4k_amd.lib import dvgo, grid as G, render_utils_cuda, train_ops, utils
import direct_train_oracle as dto
from test_direct_train_cpu import load_golden

pytestmark = pytest.mark.gpu

WEIGHTS = dict(weight_main=1.0, weight_entropy_last=0.01, weight_rgbper=0.1)                 # configs/default.py, coarse stage
ULP = 2.0 ** -24


def lego_rays(hw, theta=30., phi=-30., radius=4.0, every=1):
    ro, rd, _ = dvgo.get_rays_of_a_view(hw, hw, scene.lego_K(hw, hw), torch.Tensor(scene.lego_pose(theta, phi, radius)), False,
                                        inverse_y=False, flip_x=False, flip_y=False)
    return ro.reshape(-1, 3)[::every].contiguous().cuda(), rd.reshape(-1, 3)[::every].contiguous().cuda()


def target_for(n, seed=5):
    return torch.rand([n, 3], generator=torch.Generator().manual_seed(seed)).cuda()


def make_model(**kw):
    ck = scene.make_lego_checkpoint(rgbnet_dim=0, **kw)
    rk = {k: ck['render_kwargs'][k] for k in ('near', 'far', 'bg', 'stepsize')}
    return ck, utils.model_from_checkpoint_dict(ck).cuda(), rk


def eager_loss(out, target, n_rays, weight_main, weight_entropy_last, weight_rgbper):
    """run_sr.py:523-546 -> (loss, {term: detached value})."""
    loss = weight_main * F.mse_loss(out['rgb_marched'], target)
    terms = {'photo': loss.detach().clone(), 'entropy': torch.zeros([]), 'rgbper': torch.zeros([])}
    terms['psnr'] = -10. * torch.log10(terms['photo'])
    if weight_entropy_last > 0:
        pout = out['alphainv_last'].clamp(1e-6, 1 - 1e-6)
        ent = weight_entropy_last * -(pout * torch.log(pout) + (1 - pout) * torch.log(1 - pout)).mean()
        terms['entropy'] = ent.detach()
        loss = loss + ent
    if weight_rgbper > 0:
        rgbper = (out['raw_rgb'] - target[out['ray_id']]).pow(2).sum(-1)
        per = weight_rgbper * (rgbper * out['weights'].detach()).sum() / n_rays
        terms['rgbper'] = per.detach()
        loss = loss + per
    terms['total'] = loss.detach()
    return loss, terms


def staged_step(model, ro, rd, target, rk, weights):
    model.zero_grad(set_to_none=True)
    with torch.enable_grad():
        out = model(ro, rd, rd, k4_staged=True, **rk)
        loss, terms = eager_loss(out, target, len(ro), **weights)
        loss.backward()
    return {'terms': terms, 'rgb_marched': out['rgb_marched'].detach(), 'alphainv_last': out['alphainv_last'].detach(), 'ray_id': out['ray_id'],
            'grad_density': model.density.grid.grad.clone(), 'grad_k0': model.k0.grid.grad.clone()}


def fused_step(model, ro, rd, target, rk, weights):
    model.zero_grad(set_to_none=True)
    with torch.enable_grad():
        out = train_ops.dvgo_direct_render_loss(model, ro, rd, target, **rk, **weights)
        assert out['total'].dim() == 0 and out['total'].grad_fn is not None
        out['total'].backward()
    terms = dict(out['terms'], psnr=out['psnr'], total=out['total'].detach())
    return {'terms': terms, 'rgb_marched': out['rgb_marched'], 'alphainv_last': out['alphainv_last'], 'n_shaded': out['n_shaded'],
            'grad_density': model.density.grid.grad.clone(), 'grad_k0': model.k0.grid.grad.clone()}


@torch.no_grad()
def staged_lists(model, ro, rd, rk):
    """The staged op sequence up to the weight filter (DirectVoxGO._forward_staged), keeping what it drops on the way: the alpha-passing samples
    (points, ray ids), the weight filter's decision on each, and the longest ray's step count."""
    ray_pts, ray_id, step_id, _, _ = model.sample_ray(rays_o=ro, rays_d=rd, **rk)
    m = model.mask_cache(ray_pts)
    ray_pts, ray_id, step_id = ray_pts[m], ray_id[m], step_id[m]
    alpha = model.activate_density(model.density(ray_pts), rk['stepsize'] * model.voxel_size_ratio)
    thres = model.fast_color_thres
    if thres > 0:
        m = alpha > thres
        ray_pts, ray_id, step_id, alpha = ray_pts[m], ray_id[m], step_id[m], alpha[m]
    weights, ainv = dvgo.Alphas2Weights.apply(alpha, ray_id, len(ro))
    shaded = weights > thres if thres > 0 else torch.ones_like(ray_id, dtype=torch.bool)
    return {'pts': ray_pts.cpu(), 'ray_id': ray_id.cpu(), 'step_id': step_id.cpu(), 'shaded': shaded.cpu(), 'weights': weights.cpu(), 'ainv': ainv.cpu()}


def busiest_voxel(model, pts):
    """The largest number of trilinear corner terms any voxel of the grid receives from `pts`."""
    if len(pts) == 0:
        return 1
    dims = torch.tensor(model.density.grid.shape[2:])
    mn, mx = model.xyz_min.cpu().double(), model.xyz_max.cpu().double()
    base = torch.floor((pts.double() - mn) / (mx - mn) * (dims - 1)).long()
    count = torch.zeros(int(dims.prod()), dtype=torch.long)
    for c in range(8):
        ijk = base + torch.tensor([(c >> 2) & 1, (c >> 1) & 1, c & 1])
        ok = ((ijk >= 0) & (ijk < dims)).all(-1)
        count += torch.bincount(((ijk[:, 0] * dims[1] + ijk[:, 1]) * dims[2] + ijk[:, 2])[ok], minlength=len(count))
    return max(int(count.max()), 1)


def rel_err(x, x64):
    x, x64 = torch.as_tensor(x).detach().double().cpu(), torch.as_tensor(x64).double()
    scale = float(x64.abs().max()) if x64.numel() else 0.0
    err = float((x - x64).abs().max()) if x64.numel() else 0.0
    return err, scale


def hold(name, fused, staged, x64, n):
    """E(fused) <= max(4 E(staged), n 2^-24); a tensor the oracle holds at exactly zero must be exactly zero."""
    ef, scale = rel_err(fused, x64)
    es, _ = rel_err(staged, x64)
    if scale == 0.0:
        print(f'  {name}: oracle all zero, fused max {ef:.3g}, staged max {es:.3g}')
        assert ef == 0.0, name
        return
    print(f'  {name}: E(fused) {ef / scale:.3g}  E(staged) {es / scale:.3g}  n {n}  bound {max(4 * es / scale, n * ULP):.3g}')
    assert ef / scale <= max(4 * es / scale, n * ULP), (name, ef / scale, es / scale, n)


def check_case(model, ro, rd, target, rk, weights=WEIGHTS):
    n = len(ro)
    st = staged_step(model, ro, rd, target, rk, weights)
    fu = fused_step(model, ro, rd, target, rk, weights)
    # exact
    assert torch.equal(fu['alphainv_last'], st['alphainv_last'])
    assert torch.equal(fu['n_shaded'].long(), torch.bincount(st['ray_id'], minlength=n))
    again = train_ops.dvgo_direct_render_loss(model, ro, rd, target, **rk, **weights)
    for k in ('rgb_marched', 'alphainv_last', 'n_shaded'):
        assert torch.equal(again[k], fu[k]), k
    for k in ('photo', 'entropy', 'rgbper'):
        assert torch.equal(again['terms'][k], fu['terms'][k]), k
    assert torch.equal(again['total'].detach(), fu['terms']['total']) and torch.equal(again['psnr'], fu['terms']['psnr'])
    # toleranced, against the fp64 oracle on the staged list
    L = staged_lists(model, ro, rd, rk)
    assert torch.equal(L['ray_id'][L['shaded']] if model.fast_color_thres > 0 else L['ray_id'], st['ray_id'].cpu())
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    x64 = dto.evaluate(sd['density.grid'], sd['k0.grid'], sd['xyz_min'], sd['xyz_max'], sd['act_shift'], float(rk['stepsize'] * model.voxel_size_ratio),
                       L['pts'], L['ray_id'], L['shaded'], target.cpu(), n, rk['bg'], **weights)
    n_ray = max(int(torch.bincount(L['ray_id']).max()) if len(L['ray_id']) else 1, 1)
    hold('rgb_marched', fu['rgb_marched'], st['rgb_marched'], x64['rgb_marched'], n_ray)
    for k in ('photo', 'entropy', 'rgbper', 'total'):
        hold(k, fu['terms'][k], st['terms'][k], x64[k], n_ray)
    hold('psnr', fu['terms']['psnr'], st['terms']['psnr'], x64['psnr'], n_ray)
    hold('grad density.grid', fu['grad_density'], st['grad_density'], x64['grad_density'], busiest_voxel(model, L['pts']))
    hold('grad k0.grid', fu['grad_k0'], st['grad_k0'], x64['grad_k0'], busiest_voxel(model, L['pts'][L['shaded']]))
    return fu, st, L, x64


def test_golden_scene_matches_the_staged_path_the_oracle_and_the_reference():
    g = load_golden()
    model = utils.model_from_checkpoint_dict(g['ck']).cuda()
    ro, rd, target = g['in']['rays_o'].cuda(), g['in']['rays_d'].cuda(), g['target'].cuda()
    fu, st, L, _ = check_case(model, ro, rd, target, g['rk'], g['weights'])
    assert torch.equal(L['ray_id'][L['shaded']], g['list']['ray_id']) and torch.equal(L['step_id'][L['shaded']], g['list']['step_id'])
    # the reference's own numbers, with the bounds test_training_step_gradients_match_the_reference holds grad_dvgo to
    for k in ('total', 'photo', 'entropy', 'rgbper'):
        want = float(g['term'][k])
        assert abs(float(fu['terms'][k]) - want) <= 2e-6 * max(1.0, abs(want)), (k, float(fu['terms'][k]), want)
    for k, name in (('grad_density', 'density.grid'), ('grad_k0', 'k0.grid')):
        want = g['grad'][name].double()
        err = float((fu[k].cpu().double() - want).abs().max())
        assert err <= 2e-5 * float(want.abs().max()) + 1e-9, (name, err)


def test_three_chunk_rays_on_a_48_cubed_grid():
    _, model, rk = make_model(seed=41, num_voxels=48 ** 3)
    ro, rd = lego_rays(24)
    n_steps = render_utils_cuda.sample_pts_on_rays(ro, rd, model.xyz_min, model.xyz_max, rk['near'], 1e9, rk['stepsize'] * model.voxel_size)[4]
    assert int(n_steps.max()) > 128                                                        # rays of three 64-step chunks
    check_case(model, ro[:573], rd[:573], target_for(573), rk)                             # 573 rays: no multiple of the 4 rays of a workgroup


def _uniform(model, density):
    with torch.no_grad():
        model.density.grid.fill_(density)
        model.mask_cache.mask.fill_(True)
    torch.autograd.graph.increment_version(model.mask_cache.mask)


def test_opaque_wall_stops_in_the_first_chunk():
    _, model, rk = make_model(seed=42, num_voxels=24 ** 3)
    _uniform(model, 5.0)                                                                    # alpha ~ 0.37 per sample: T < 1e-3 after 16 samples
    ro, rd = lego_rays(12)
    fu, st, L, _ = check_case(model, ro, rd, target_for(len(ro)), rk)
    hit = fu['n_shaded'] > 0
    assert bool(hit.any()) and bool((fu['alphainv_last'][hit] < 1e-3).all()) and int(fu['n_shaded'].max()) < 64
    assert int(L['step_id'][L['weights'] > 0].max()) < 64


def test_crossing_sample_on_lane_63():
    """A uniform density chosen so that the transmittance of a ray through the box falls below 1e-3 at its 64th sample: on the rays whose step 0 lies
    in the box that is lane 63 of the first chunk (asserted), on the others lane 0 of the second."""
    _, model, rk = make_model(seed=43, num_voxels=48 ** 3)
    interval = float(rk['stepsize'] * model.voxel_size_ratio)
    one_minus_a = np.exp(np.log(1e-3) / 63.5)                                               # (1 - a)^64 < 1e-3 <= (1 - a)^63
    x = np.log(one_minus_a ** (-1.0 / interval) - 1.0)                                      # 1 - a = (1 + e^x)^-interval
    _uniform(model, float(x) - float(model.act_shift))
    ro, rd = lego_rays(16)
    ro = torch.cat([ro, ro + 0.62 * rd])                                                    # the second half starts nearer to the box
    rd = torch.cat([rd, rd])
    fu, st, L, _ = check_case(model, ro, rd, target_for(len(ro)), rk)
    live = L['weights'] > 0
    last = torch.zeros(len(ro), dtype=torch.long).scatter_reduce(0, L['ray_id'][live], L['step_id'][live], 'amax', include_self=True)
    crossed = L['ainv'] < 1e-3
    assert bool((crossed & (last % 64 == 63)).any()), sorted(set((last[crossed] % 64).tolist()))


ODD = {
    # rays that miss the box take the one out-of-box step of k_pts_count (N_steps >= 1)
    'miss': (lambda o, d: (torch.cat([o[:37], o[:5] * 0 + torch.tensor([5., 5., 5.], device='cuda')]),
                           torch.cat([d[:37], d[:5] * 0 + torch.tensor([1., 0.2, 0.1], device='cuda')])), {}),
    # rays that start inside the box: near = 0.2 from origins around the centre
    'inside': (lambda o, d: (o[:41] * 0.0 + torch.tensor([0.11, -0.23, 0.31], device='cuda') + 0.3 * d[:41].flip(0) / 4, d[:41]), {'near': 0.2}),
    # a zero direction component (two, for the axis-parallel ones): the 1e-6 substitute of aabb_t
    'zero_dir': (lambda o, d: (torch.cat([o[:29], torch.tensor([[0.2, 0.1, 4.0], [0.3, -0.2, 3.5], [-4., 0.1, 0.2]], device='cuda')]),
                               torch.cat([d[:29], torch.tensor([[0., 0., -1.], [0., 0.05, -1.], [1.1, 0., 0.]], device='cuda')])), {}),
}


@pytest.mark.parametrize('kind', sorted(ODD))
def test_odd_rays(kind):
    _, model, rk = make_model(seed=44, num_voxels=24 ** 3)
    make, extra = ODD[kind]
    ro, rd = lego_rays(12)
    ro, rd = (t.contiguous() for t in make(ro[40:], rd[40:]))
    rk = dict(rk, **extra)
    fu, st, L, _ = check_case(model, ro, rd, target_for(len(ro)), rk)
    n_steps = render_utils_cuda.sample_pts_on_rays(ro, rd, model.xyz_min, model.xyz_max, rk['near'], 1e9, rk['stepsize'] * model.voxel_size)[4]
    if kind == 'miss':
        assert bool((n_steps[-5:] == 1).all()) and bool((fu['n_shaded'][-5:] == 0).all()) and bool((fu['alphainv_last'][-5:] == 1).all())
    if kind == 'inside':
        inbox = ((ro > model.xyz_min) & (ro < model.xyz_max)).all(-1)
        assert bool(inbox.all()) and int(fu['n_shaded'].max()) > 0
    if kind == 'zero_dir':
        assert int((rd == 0).sum()) == 5


def test_empty_scene_has_zero_gradients():
    _, model, rk = make_model(seed=45, num_voxels=24 ** 3)
    _uniform(model, -100.0)
    ro, rd = lego_rays(10)
    fu, st, L, _ = check_case(model, ro, rd, target_for(len(ro)), rk)
    assert len(L['ray_id']) == 0 and int(fu['n_shaded'].sum()) == 0
    assert bool((fu['alphainv_last'] == 1).all())
    assert int(fu['grad_density'].count_nonzero()) == 0 and int(fu['grad_k0'].count_nonzero()) == 0      # incl. the entropy term: clamped at 1 - 1e-6


def test_zero_rays():
    _, model, rk = make_model(seed=45, num_voxels=16 ** 3)
    e = torch.zeros([0, 3], device='cuda')
    fu = fused_step(model, e, e, e, rk, WEIGHTS)
    assert fu['rgb_marched'].shape == (0, 3) and fu['alphainv_last'].shape == (0,)
    assert bool(torch.isnan(fu['terms']['photo']))                                         # the mean of an empty tensor, as F.mse_loss
    assert int(fu['grad_density'].count_nonzero()) == 0 and int(fu['grad_k0'].count_nonzero()) == 0
    assert fu['grad_density'].shape == model.density.grid.shape and fu['grad_k0'].shape == model.k0.grid.shape


def test_threshold_zero_switches_both_filters_off():
    _, model, rk = make_model(seed=46, num_voxels=24 ** 3, fast_color_thres=0)
    assert model.fast_color_thres == 0
    with torch.no_grad():
        model.density.grid += 6.0                                                          # some rays reach their stop: samples behind it stay listed
    ro, rd = lego_rays(14)
    fu, st, L, _ = check_case(model, ro, rd, target_for(len(ro)), rk)
    assert bool((L['weights'] == 0).any()) and bool((fu['alphainv_last'] < 1e-3).any())


@pytest.mark.parametrize('bg', [0, 1])
def test_background(bg):
    _, model, rk = make_model(seed=47, num_voxels=24 ** 3)
    ro, rd = lego_rays(14)
    check_case(model, ro, rd, target_for(len(ro)), dict(rk, bg=bg))


def test_mask_cache_of_another_resolution():
    _, model, rk = make_model(seed=48, num_voxels=24 ** 3)
    coarse = F.interpolate(model.mask_cache.mask[None, None].float(), size=(17, 19, 13), mode='nearest')[0, 0] > 0
    model.mask_cache = G.MaskGrid(path=None, mask=coarse, xyz_min=model.xyz_min, xyz_max=model.xyz_max).cuda()
    assert tuple(model.mask_cache.mask.shape) != tuple(model.density.grid.shape[2:])
    ro, rd = lego_rays(14)
    fu, *_ = check_case(model, ro, rd, target_for(len(ro)), rk)
    assert int(fu['n_shaded'].sum()) > 0


def test_64_identical_rays_contend_on_the_same_voxels():
    """64 copies of one ray: every atomic of the backward meets 63 others on its address.  A ray's gradient in a batch of n is 1/n of its gradient
    alone, so the 64 sum to the single ray's: compared within the rule above, n = the busiest voxel's contributions."""
    _, model, rk = make_model(seed=49, num_voxels=24 ** 3)
    ro, rd = lego_rays(12)
    pick = int(torch.bincount(staged_lists(model, ro, rd, rk)['ray_id'], minlength=len(ro)).argmax())
    ro64, rd64 = ro[pick:pick + 1].repeat(64, 1), rd[pick:pick + 1].repeat(64, 1)
    tgt = target_for(1).repeat(64, 1)
    fu, st, L, x64 = check_case(model, ro64, rd64, tgt, rk)
    assert int(fu['n_shaded'][0]) > 4
    one = fused_step(model, ro64[:1].contiguous(), rd64[:1].contiguous(), tgt[:1].contiguous(), rk, WEIGHTS)
    n = busiest_voxel(model, L['pts'])
    for k in ('grad_density', 'grad_k0'):
        hold(k + ' (64 x one ray / 64)', fu[k], one[k], x64[k], n)


@pytest.mark.parametrize('off', ['weight_entropy_last', 'weight_rgbper', 'both'])
def test_term_weights_switch_their_term_off(off):
    _, model, rk = make_model(seed=50, num_voxels=24 ** 3)
    ro, rd = lego_rays(14)
    w = dict(WEIGHTS)
    for k in (['weight_entropy_last', 'weight_rgbper'] if off == 'both' else [off]):
        w[k] = 0.0
    fu, *_ = check_case(model, ro, rd, target_for(len(ro)), rk, w)
    for k, term in (('weight_entropy_last', 'entropy'), ('weight_rgbper', 'rgbper')):
        assert (float(fu['terms'][term]) == 0.0) == (w[k] == 0.0)


class _Cfg(dict):
    __getattr__ = dict.__getitem__


def _loop(model, step_fn, ro, rd, target, rk, count, steps=6, lr=1e-1):
    """-> (the total of every step, the gradients (density.grid, k0.grid) of every step)."""
    opt = utils.create_optimizer_or_freeze_model(model, _Cfg(lrate_decay=20, lrate_density=lr, lrate_k0=lr, skip_zero_grad_fields=['density', 'k0']), global_step=0)
    opt.set_pervoxel_lr(count)
    totals, grads = [], []
    for _ in range(steps):
        opt.zero_grad(set_to_none=True)
        out = step_fn(model, ro, rd, target, rk, WEIGHTS)
        totals.append(float(out['terms']['total']))
        grads.append((out['grad_density'], out['grad_k0']))
        opt.step()
    return totals, grads


THETA = 1.0 / 16


def test_six_optimizer_steps_reduce_the_loss_and_track_the_staged_loop():
    """zero_grad, loss, backward, MaskedAdam.step with a per-voxel learning rate, six times, fused and staged from the same start; then the parameters
    of the two loops are compared directly, E = max|fused - staged| / max|staged| (printed).

    The bound.  Both paths sum a voxel's gradient in fp32 from at most n terms (n = the busiest voxel's contributions, read from the staged list), so the
    two gradients differ by at most a = 2 n 2^-24 max|g| in a voxel.  Adam's step lr s m^ / (sqrt(v^) + eps), s <= 1, does not change when every
    gradient of a voxel is scaled by one factor, so what matters is the RELATIVE difference of a voxel's gradients: rho = a / |g|.  That is unbounded
    where |g| is rounding noise, so the comparison is over the voxels S whose staged gradient keeps one sign over the six steps, stays at or above
    THETA max|g| of its step, and varies by at most 4x over the steps; S must hold at least 64 voxels of each grid.  On S, rho <= 2 n 2^-24 / THETA, m^
    moves by at most a factor 1 +- rho and sqrt(v^) likewise, |m^| / sqrt(v^) <= max|g| / min|g| <= 4, so one step differs by at most
    lr * 4 * 2 rho / (1 - rho) and six steps by  steps * lr * 8.4 * rho  (the feedback of that difference into the later gradients is of second order).
    A wrong sign or a missing term in the backward moves the voxels of S by about lr per step and fails this by orders of magnitude."""
    ck, model, rk = make_model(seed=51, num_voxels=24 ** 3)
    other = utils.model_from_checkpoint_dict(ck).cuda()
    ro, rd = lego_rays(16)
    target = target_for(len(ro))
    L = staged_lists(other, ro, rd, rk)
    n = {'density': busiest_voxel(other, L['pts']), 'k0': busiest_voxel(other, L['pts'][L['shaded']])}
    count = (torch.rand(model.density.grid.shape, generator=torch.Generator().manual_seed(2)) * 30 + 1).cuda()
    steps, lr = 6, 1e-1
    fused, _ = _loop(model, fused_step, ro, rd, target, rk, count, steps, lr)
    staged, grads = _loop(other, staged_step, ro, rd, target, rk, count, steps, lr)
    print('  totals fused', fused, 'staged', staged)
    assert fused[-1] < fused[0], fused
    assert model.density.grid.grad is not None and model.density.grid.grad.shape == model.density.grid.shape
    for i, name in enumerate(('density', 'k0')):
        g = torch.stack([gr[i] for gr in grads])                                           # [steps, ...] of the staged loop
        top = g.abs().flatten(1).max(1).values.reshape(-1, *[1] * (g.dim() - 1))
        S = ((g > 0).all(0) | (g < 0).all(0)) & (g.abs() >= THETA * top).all(0) & (g.abs().max(0).values <= 4 * g.abs().min(0).values)
        assert int(S.sum()) >= 64, (name, int(S.sum()))
        a, b = getattr(model, name).grid.detach(), getattr(other, name).grid.detach()
        rho = 2 * n[name] * ULP / THETA
        bound = steps * lr * 8.4 * rho
        diff, scale = float((a - b)[S].abs().max()), float(b.abs().max())
        full = float((a - b).abs().max())
        print(f'  {name}.grid after {steps} steps: |S| {int(S.sum())}, n {n[name]}, max|fused - staged| on S {diff:.3g} (E {diff / scale:.3g}), '
              f'bound {bound:.3g} (E {bound / scale:.3g}); over all voxels {full:.3g} (E {full / scale:.3g})')
        assert diff <= bound, (name, diff, bound)


def test_writing_a_returned_tensor_before_backward_raises():
    """The backward launch re-reads the forward's outputs and the grids: an in-place write in between is refused, not silently used."""
    _, model, rk = make_model(seed=54, num_voxels=16 ** 3)
    ro, rd = lego_rays(8)
    out = train_ops.dvgo_direct_render_loss(model, ro, rd, target_for(len(ro)), **rk, **WEIGHTS)
    out['rgb_marched'].add_(1.0)
    with pytest.raises(N.K4Error, match='modified in place'):
        out['total'].backward()
    out = train_ops.dvgo_direct_render_loss(model, ro, rd, target_for(len(ro)), **rk, **WEIGHTS)
    with torch.no_grad():
        model.k0.grid.add_(0.5)
    with pytest.raises(RuntimeError, match='modified by an inplace operation'):
        out['total'].backward()


def test_a_model_with_an_rgbnet_raises_the_reason():
    ck = scene.make_lego_checkpoint(num_voxels=16 ** 3, rgbnet_dim=6, rgbnet_width=32)
    model = utils.model_from_checkpoint_dict(ck).cuda()
    ro, rd = lego_rays(6)
    with pytest.raises(N.K4Error, match='rgbnet'):
        train_ops.dvgo_direct_render_loss(model, ro, rd, target_for(len(ro)), near=2., stepsize=0.5, bg=1, **WEIGHTS)
    _, direct, rk = make_model(seed=52, num_voxels=16 ** 3)
    for term in ('weight_nearclip', 'weight_distortion'):
        with pytest.raises(N.K4Error, match='nearclip and distortion'):
            train_ops.dvgo_direct_render_loss(direct, ro, rd, target_for(len(ro)), **rk, **WEIGHTS, **{term: 0.01})
    assert direct.k4_direct_train_supported() == (True, '')


def test_a_fused_step_leaves_no_stale_cache_behind():
    """After a fused step and the optimizer's in-place update, a plain render equals one from a freshly loaded copy of the same parameters."""
    ck, model, rk = make_model(seed=53, num_voxels=24 ** 3)
    ro, rd = lego_rays(16)
    with torch.no_grad():
        model(ro, rd, rd, **rk)                                                            # the render path's caches exist before the step
    _loop(model, fused_step, ro, rd, target_for(len(ro)), rk, torch.ones_like(model.density.grid).detach(), steps=1)
    fresh = utils.model_from_checkpoint_dict(ck)
    fresh.load_state_dict(copy.deepcopy(model.state_dict()))
    fresh = fresh.cuda()
    with torch.no_grad():
        a, b = model(ro, rd, rd, **rk), fresh(ro, rd, rd, **rk)
    for k in ('rgb_marched', 'alphainv_last'):
        assert torch.equal(a[k], b[k]), k
    assert model.density.grad_route.idle and model.k0.grad_route.idle
