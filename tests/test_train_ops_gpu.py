"""GPU parity of the marcher's training-graph kernels (csrc/k4_train.hip, lib/train_ops.py) and of the joint training step
(4k-nerf_amd/joint_train.py; SURVEY.md 3.4, 8f rank 1 "MLP bwd"):
  * k4_rgbnet_fwd / k4_rgbnet_bwd against the oracle's fp64 autograd of the same nn.Sequential + sigmoid
    (tolerance: fp32 FMA chains of <= 129 terms forward, sums over n samples in the weight gradients:
     |err| <= 1e-5 * max|want| + 1e-7 per tensor), deterministic (two runs bit-equal), shapes incl. ragged tiles, n = 0 and 1;
  * k4_distortion_loss against the oracle's literal O(n^2) definition incl. empty rays, single-sample rays and rays longer
    than one 64-sample scan step (1e-5 relative);
  * one joint iteration (DirectMPIGO train forward -> SFTNet -> 5 loss terms -> backward) against tests/golden/grad_joint.npz
    = the same iteration on the REFERENCE's own modules (oracle/gen_golden.py::gen_grad_joint), then JointTrainer.step
    (TV add-grad + MaskedAdam x 2 + lr decay) lowering the loss over a few iterations.
"""
import json
import os

import numpy as np
import pytest
import torch

import nerf4k_amd  # noqa: F401
from nerf4k_amd import _native as N, joint_train
from nerf4k_amd.lib import dmpigo, sr_esrnet, train_ops, utils
from oracle import sr as osr, train_ops as oto
from helpers import GOLDEN

pytestmark = pytest.mark.gpu


def _close(got, want, name, rel=1e-5, abs_=1e-7):
    got, want = got.detach().cpu().double(), want.detach().double()
    assert got.shape == want.shape, (name, got.shape, want.shape)
    scale = float(want.abs().max()) if want.numel() else 0.0
    err = float((got - want).abs().max()) if want.numel() else 0.0
    assert err <= rel * scale + abs_, (name, err, scale)


@pytest.mark.parametrize('dim0,width,depth,n,with_add', [(15, 64, 3, 1000, False), (39, 128, 3, 333, False), (39, 128, 2, 200, True),
                                                         (7, 32, 3, 64, True), (64, 32, 2, 1, False), (27, 64, 2, 129, False),
                                                         (15, 64, 3, 0, False), (33, 128, 3, 70000, True)])
def test_rgbnet_kernels_match_fp64_autograd(dim0, width, depth, n, with_add):
    g = torch.Generator().manual_seed(dim0 * 1000 + width + depth)
    net = dmpigo._mlp(dim0, width, depth, 3)
    with torch.no_grad():
        for p in net.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * (0.5 / max(p.shape[-1], 1) ** 0.5 if p.dim() == 2 else 0.1))
    assert train_ops.rgbnet_supported(net)
    x = torch.randn([n, dim0], generator=g)
    add = torch.randn([n, 3], generator=g) * 0.3 if with_add else None
    gy = torch.randn([n, 3], generator=g)
    # oracle, fp64
    lins = [m for m in net.modules() if isinstance(m, torch.nn.Linear)]
    # A hidden unit whose pre-activation is within rounding of 0 gets its ReLU gate from the ROUNDING (fp32 chain vs fp64): such samples
    # (a few per 10^5 x 256 units) are given a zero output gradient on both sides -- the comparison is about arithmetic, not about ties.
    with torch.no_grad():
        h, amb = x.double(), torch.zeros([n], dtype=torch.bool)
        for l in lins[:-1]:
            z = torch.nn.functional.linear(h, l.weight.double(), l.bias.double())
            amb |= (z.abs() < 1e-5).any(1)
            h = torch.relu(z)
        gy[amb] = 0
        # expected share: P(|z| < 1e-5) ~ 1.6e-5 per unit (z ~ N(0, 0.5)) x up to 256 hidden units = 0.2-0.7 % of the samples (467 of 70000 in
        # the largest case; the band is ~20x the fp32 chain's own error in z, the smallest that keeps the comparison free of rounding ties)
        assert int(amb.sum()) <= max(2, n // 100)
    wr = [(l.weight.detach().double().requires_grad_(True), l.bias.detach().double().requires_grad_(True)) for l in lins]
    xr = x.double().requires_grad_(True)
    ar = None if add is None else add.double().requires_grad_(True)
    yr = oto.rgbnet_sigmoid(xr, wr, ar)
    yr.backward(gy.double())
    # HIP
    net = net.cuda()
    xd = x.cuda().requires_grad_(True)
    ad = None if add is None else add.cuda().requires_grad_(True)
    y = train_ops.rgbnet_sigmoid(net, xd, ad)
    _close(y, yr, 'rgb', rel=2e-6, abs_=2e-7)
    y.backward(gy.cuda())
    _close(xd.grad, xr.grad, 'grad_x')
    if ad is not None:
        _close(ad.grad, ar.grad, 'grad_add')
    lins_d = [m for m in net.modules() if isinstance(m, torch.nn.Linear)]
    for i, (l, (w, b)) in enumerate(zip(lins_d, wr)):
        _close(l.weight.grad, w.grad, f'grad_w{i}')
        _close(l.bias.grad, b.grad, f'grad_b{i}')
    if n > 0:                                                        # no atomics: a second evaluation is bit-identical
        first = [p.grad.clone() for p in net.parameters()] + [xd.grad.clone()]
        net.zero_grad(set_to_none=True)
        xd.grad = None
        train_ops.rgbnet_sigmoid(net, xd, ad).backward(gy.cuda())
        for a, b in zip(first, [p.grad for p in net.parameters()] + [xd.grad]):
            assert torch.equal(a, b)
    # inference form (no activations saved) gives the same values
    with torch.no_grad():
        assert torch.equal(train_ops.rgbnet_sigmoid(net, xd.detach(), None if ad is None else ad.detach()), y.detach())


def test_rgbnet_unsupported_shapes_are_reported():
    assert not train_ops.rgbnet_supported(dmpigo._mlp(15, 64, 4, 3))          # two hidden->hidden layers
    assert not train_ops.rgbnet_supported(dmpigo._mlp(70, 64, 3, 3))          # dim0 > 64
    assert not train_ops.rgbnet_supported(dmpigo._mlp(15, 48, 3, 3))          # width
    L = N.lib()
    assert L.k4_rgbnet_bwd_workspace_bytes(100, 15, 48, 1) < 0
    x = torch.zeros([4, 15], device='cuda')
    assert L.k4_rgbnet_fwd(N.f32(x), 4, 15, 48, 1, N.f32(x), N.f32(x), N.f32(x), N.f32(x), N.f32(x), N.f32(x), None, None, None, N.f32(x),
                           N.stream()) == N.K4_ERR_UNSUPPORTED
    with pytest.raises(N.K4Error):
        train_ops.rgbnet_sigmoid(dmpigo._mlp(15, 64, 3, 3), torch.zeros([4, 15]))


def test_distortion_loss_matches_the_definition():
    g = torch.Generator().manual_seed(4)
    per = [0, 1, 5, 70, 3, 0, 130, 64, 65, 0]                         # empty rays, one sample, > one scan step, exact multiples
    ray_id = torch.cat([torch.full([c], r, dtype=torch.long) for r, c in enumerate(per)])
    w = torch.rand([ray_id.numel()], generator=g) * 0.2
    s = torch.cat([torch.sort(torch.rand([c], generator=g)).values for c in per])
    interval = 1 / 256
    wr = w.double().requires_grad_(True)
    want = oto.distortion_loss(wr, s.double(), interval, ray_id)
    want.backward()
    wd = w.cuda().requires_grad_(True)
    got = train_ops.flatten_eff_distloss(wd, s.cuda(), interval, ray_id.cuda())
    assert abs(float(got) - float(want)) <= 1e-5 * abs(float(want)), (float(got), float(want))
    (got * 3.0).backward()
    _close(wd.grad, wr.grad * 3.0, 'grad_w', rel=1e-5, abs_=1e-7)
    # the last ray being empty does not change the normaliser (ray_id.max() + 1 = 9 here, as the package computes it)
    assert int(ray_id.max()) + 1 == 9
    # with the batch's ray count as launch bound (no read-back of ray_id.max()): same value, same gradient
    wb = w.cuda().requires_grad_(True)
    gotb = train_ops.flatten_eff_distloss(wb, s.cuda(), interval, ray_id.cuda(), n_rays=len(per) + 7)
    (gotb * 3.0).backward()
    assert float(gotb) == float(got) and torch.equal(wb.grad, wd.grad)
    with pytest.raises(ValueError):
        train_ops.flatten_eff_distloss(wd, s.cuda(), interval, ray_id.cuda().int())
    # no samples at all
    e = train_ops.flatten_eff_distloss(torch.zeros([0], device='cuda', requires_grad=True), torch.zeros([0], device='cuda'), interval,
                                       torch.zeros([0], dtype=torch.long, device='cuda'))
    assert float(e) == 0.0


@pytest.mark.parametrize('C,V,frac', [(12, 100003, 0.01), (1, 4097, 0.5), (9, 70000, 0.0), (3, 513, 1.0)])
def test_touched_voxels_matches_the_dense_scan(C, V, frac):
    """k4_touched_voxels (one pass, wave-aggregated append, retry when the list overflows) == (g != 0).any(0).nonzero()."""
    g = torch.Generator().manual_seed(C + V)
    grad = torch.zeros([C, V])
    hit = torch.rand([V], generator=g) < frac
    grad[torch.randint(0, C, [int(hit.sum())], generator=g), hit.nonzero().flatten()] = 1.5
    grad = grad.cuda()
    want = (grad != 0).any(0).nonzero().flatten().to(torch.int32)
    for cap in (None, 7):                                             # 7: forces the overflow / retry path
        got = joint_train.touched_voxels(grad, cap=cap)
        assert got.dtype == torch.int32 and torch.equal(got, want)


def _load_joint():
    z = np.load(os.path.join(GOLDEN, 'grad_joint.npz'), allow_pickle=False)
    kw = json.loads(str(z['model_kwargs_json']))
    for k in ('xyz_min', 'xyz_max'):
        kw[k] = np.asarray(kw[k], dtype=np.float32)
    ck = {'model_class': str(z['model_class']), 'model_kwargs': kw,
          'model_state_dict': {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith('sd/')}}
    model = utils.model_from_checkpoint_dict(ck).cuda().train()
    nb = int(z['num_block'])
    net = sr_esrnet.SFTNet(3, scale=4, num_feat=64, num_block=nb, num_grow_ch=32, num_cond=1)
    net.load_state_dict(osr.make_state_dict(seed=int(z['sr_seed']), num_block=nb))
    net = net.cuda().train()
    rk = json.loads(str(z['render_kwargs_json']))
    cfg = joint_train.JointCfg.fern_lg_joint_l1(**json.loads(str(z['cfg_json'])))
    batch = [torch.from_numpy(z['in/' + k]).cuda() for k in ('rays_o', 'rays_d', 'viewdirs')] + \
            [torch.from_numpy(z['target']).cuda(), torch.from_numpy(z['target_4x']).cuda(), int(z['patch'][0]), int(z['patch'][1])]
    return z, model, net, rk, cfg, batch


def test_joint_iteration_matches_the_reference_modules():
    z, model, net, rk, cfg, batch = _load_joint()
    tr = joint_train.JointTrainer(model, net, cfg, rk, n_train_images=17)
    with torch.enable_grad():
        rr, rgb_sr, ls = tr.forward(*batch, global_step=int(z['global_step']))
        ls['total'].backward()
    _close(rr['rgb_feature'], torch.from_numpy(z['out/rgb_feature']), 'rgb_feature', rel=2e-6, abs_=2e-7)
    _close(rr['depth'], torch.from_numpy(z['out/depth']), 'depth', rel=2e-6, abs_=2e-7)
    _close(rgb_sr, torch.from_numpy(z['out/rgb_sr']), 'rgb_sr', rel=2e-5)
    for k in ('photo', 'l1', 'entropy_last', 'distortion', 'rgbper', 'total'):
        want = float(z['loss/' + k])
        assert abs(float(ls[k]) - want) <= 1e-5 * max(abs(want), 1e-4), (k, float(ls[k]), want)
    named = dict(model.named_parameters())
    n_checked = 0
    for k in z.files:
        if k.startswith('grad/'):
            assert named[k[5:]].grad is not None, k
            _close(named[k[5:]].grad, torch.from_numpy(z[k]), k, rel=5e-5, abs_=1e-9)
            n_checked += 1
    assert n_checked >= 6
    sr_named = dict(net.named_parameters())
    for k in z.files:
        if k.startswith('sr_grad/'):
            _close(sr_named[k[8:]].grad, torch.from_numpy(z[k]), k, rel=5e-5, abs_=1e-9)
    stats = z['sr_stats']
    gsum = np.array([float(sr_named[str(nm)].grad.double().sum()) for nm in z['sr_names']])
    gnorm = np.array([float(sr_named[str(nm)].grad.double().norm()) for nm in z['sr_names']])
    assert np.abs(gnorm - stats[:, 1]).max() <= 1e-4 * stats[:, 1].max()
    assert np.abs(gsum - stats[:, 0]).max() <= 1e-4 * np.abs(stats[:, 0]).max() + 1e-7


def test_joint_trainer_steps_lower_the_loss():
    z, model, net, rk, cfg, batch = _load_joint()
    cfg = joint_train.JointCfg(dict(cfg, tv_before=100, tv_dense_before=2))
    tr = joint_train.JointTrainer(model, net, cfg, rk, n_train_images=17)
    lr0 = [pg['lr'] for pg in tr.optimizer.param_groups]
    before = {k: v.detach().clone() for k, v in model.named_parameters()}
    hist = [float(tr.step(*batch, global_step=1 + i)['total']) for i in range(8)]
    assert hist[-1] < hist[0], hist
    assert all(np.isfinite(hist))
    changed = [k for k, v in model.named_parameters() if not torch.equal(v.detach(), before[k])]
    assert 'density.grid' in changed and 'k0.grid' in changed and any(k.startswith('rgbnet') for k in changed)
    factor = 0.1 ** (1 / (cfg.lrate_decay * 1000))
    for a, pg in zip(lr0, tr.optimizer.param_groups):
        assert abs(pg['lr'] - a * factor ** 8) <= 1e-12 * a
    assert tr.last_exchange == {'world': 1}
    # the render path after training steps sees the updated parameters (repack caches re-key on the bumped versions)
    with torch.no_grad():
        a = model(*batch[:3], **{k: v for k, v in rk.items() if k != 'rand_bkgd'})
        b = model(*batch[:3], k4_staged=True, **{k: v for k, v in rk.items() if k != 'rand_bkgd'})
    assert torch.allclose(a['rgb_marched'], b['rgb_marched'], atol=2e-5)


def test_dense_tv_written_ahead_of_backward_and_side_stream_adam_equal_the_reference_order(monkeypatch):
    """JointTrainer.step writes the DENSE total-variation term into the grid gradients' buffers before the backward pass (side stream;
    the lookups' backward accumulates into them) instead of adding it after (run_sr.py:1005-1011): grad = term + scatter either way.
    Three steps each way from the same state: same losses, same parameters (scatter atomics reorder sums: 1e-5 relative), and the
    sparse-TV steps (global_step >= tv_dense_before) take the reference's order in both.  Likewise the k0 grid's optimizer step on a
    second stream (MaskedAdam.update_on_side_stream): readers of the grid wait for it, results unchanged."""
    from nerf4k_amd.lib import masked_adam
    monkeypatch.setattr(masked_adam, '_MULTI_BELOW', 1000)      # the test scene's grids (19 440 / 2 160 floats) take the large-tensor path of the LLFF grids
    res = []
    for seed_on, adam_side in ((False, False), (True, False), (False, True), (True, True)):
        z, model, net, rk, cfg, batch = _load_joint()
        cfg = joint_train.JointCfg(dict(cfg, tv_before=100, tv_dense_before=3))          # steps 1, 2 dense; step 3 sparse
        monkeypatch.setattr(joint_train, '_TV_SEED', seed_on)
        monkeypatch.setattr(joint_train, '_ADAM_SIDE', adam_side)                       # the k0 grid's optimizer step on a second stream
        tr = joint_train.JointTrainer(model, net, cfg, rk, n_train_images=17)
        hist = [float(tr.step(*batch, global_step=1 + i)['total']) for i in range(3)]
        assert model.k0.grad_route.idle and model.density.grad_route.idle              # every seed was consumed (or folded in by finish_grad_seed)
        assert (model.k0._k4_pending is not None) == adam_side                         # the last step's update may still be running ...
        sd = model.state_dict()                                                         # ... every reader waits for it: state_dict,
        if adam_side:                                                                   # (the event stays until the next update: a reader on ANOTHER stream waits too)
            assert torch.cuda.current_stream().cuda_stream in model.k0._k4_pending_seen
            osd = tr.optimizer.state_dict()                                             # the optimizer's own checkpoint copy waits as well
            assert any(torch.is_tensor(v.get('exp_avg')) for v in osd['state'].values())
        with torch.no_grad():                                                           # the fused marcher
            img = model(*batch[:3], **{k: v for k, v in rk.items() if k != 'rand_bkgd'})['rgb_marched'].clone()
        res.append((hist, {k: v.detach().clone() for k, v in sd.items() if v.is_floating_point()}, [p.detach().clone() for p in net.parameters()], img))
    h0, m0, s0, i0 = res[0]
    for h1, m1, s1, i1 in res[1:]:
        assert np.allclose(h1, h0, rtol=1e-6, atol=0), (h1, h0)
        for k in m1:
            _close(m1[k], m0[k].cpu(), k, rel=1e-5, abs_=1e-8)
        for a, b in zip(s1, s0):
            _close(a, b.cpu(), 'decoder parameter', rel=1e-5, abs_=1e-8)
        _close(i1, i0.cpu(), 'render after the steps', rel=1e-5, abs_=1e-7)
    # a backward pass that never reaches the grid: the seed becomes the gradient
    z, model, net, rk, cfg, batch = _load_joint()
    g = model.k0
    g.total_variation_add_grad(0.3, 0.3, 0.1, 'seed')
    assert g.grid.grad is None and not g.grad_route.idle                            # (a seed is parked)
    g.finish_grad_seed()
    want = torch.zeros_like(g.grid)
    from nerf4k_amd.lib import grid as k4grid
    k4grid.total_variation_add_grad(g.grid, want, 0.3, 0.3, 0.1, True)
    assert g.grad_route.idle and torch.equal(g.grid.grad, want)


def test_iterations_without_tv_update_k0_from_the_scatter_image(monkeypatch):
    """After tv_before (run_sr.py:1005-1011: no total variation; 290,000 of fern_lg_joint_l1's 300,000 iterations) JointTrainer.step leaves k0's gradient in
    the scratch image of the lookups' backward and MaskedAdam updates the touched voxels from there (the 'sparse' route of DenseGrid.grad_route, MaskedAdam._sparse_step):
    four steps each way from the same state -- step 1 with dense TV (dense gradient both ways), steps 2-4 without -- same losses, parameters, moments and
    step counts (scatter atomics reorder sums: 1e-5 relative); `.grad` of k0 stays None in the in-place form; an iteration that raises drops its sums."""
    from nerf4k_amd.lib import masked_adam
    from nerf4k_amd.lib import grid as k4grid
    monkeypatch.setattr(masked_adam, '_MULTI_BELOW', 1000)
    res = []
    for sparse_on in (False, True):
        z, model, net, rk, cfg, batch = _load_joint()
        cfg = joint_train.JointCfg(dict(cfg, tv_before=2, tv_dense_before=2))
        monkeypatch.setattr(joint_train, '_SPARSE_GRID_GRAD', sparse_on)
        monkeypatch.setattr(joint_train, '_SPLIT_GRID_STEP', False)       # (step 1, the dense-TV iteration: the one-pass step -- the split form has its own test)
        tr = joint_train.JointTrainer(model, net, cfg, rk, n_train_images=17)
        assert [o is model.k0 for o in tr._sparse_grid_owners()] == [True]
        hist = []
        for i in range(4):
            hist.append(float(tr.step(*batch, global_step=1 + i)['total']))
            assert (model.k0.grid.grad is None) == (sparse_on and i >= 1), i
            assert model.k0.grad_route.idle and not model.k0.grad_route.pending
            assert model.density.grid.grad is not None
        st = tr.optimizer.state[model.k0.grid]
        assert st['step'] == 4
        sd = {k: v.detach().clone() for k, v in model.state_dict().items() if v.is_floating_point()}
        res.append((hist, sd, st['exp_avg'].clone(), st['exp_avg_sq'].clone()))
        ws = k4grid._GSB_WS[model.k0.grid.device].ws
        assert int(ws.count_nonzero()) == 0                               # the image is all zero between iterations
    (h0, m0, a0, b0), (h1, m1, a1, b1) = res
    assert np.allclose(h1, h0, rtol=1e-6, atol=0), (h1, h0)
    for k in m1:
        _close(m1[k], m0[k].cpu(), k, rel=1e-5, abs_=1e-8)
    _close(a1, a0.cpu(), 'exp_avg', rel=1e-5, abs_=1e-9)
    _close(b1, b0.cpu(), 'exp_avg_sq', rel=1e-5, abs_=1e-12)
    assert torch.equal(a1 == 0, a0 == 0)                                  # the same voxels ever touched
    # an iteration that raises after its backward: the pending sums do not reach the next one
    before = model.k0.grid.detach().clone()
    with monkeypatch.context() as mp:
        mp.setattr(joint_train, 'exchange_gradients', lambda *a, **k: (_ for _ in ()).throw(RuntimeError('skip this batch')))
        with pytest.raises(RuntimeError, match='skip this batch'):
            tr.step(*batch, global_step=9)
    assert model.k0.grad_route.idle and not model.k0.grad_route.pending and model.k0.grid.device not in k4grid._GSB_WS
    assert torch.equal(model.k0.grid.detach(), before)
    # ... and a pending gradient met by a step that cannot take the in-place form is swept into the dense tensor
    route = model.k0.grad_route
    route.arm('sparse')
    with torch.enable_grad():
        rr, rgb_sr, ls = tr.forward(*batch, global_step=9)
        tr.optimizer.zero_grad(set_to_none=True)
        ls['total'].backward()
    assert route.pending and model.k0.grid.grad is None
    route.sweep()
    assert model.k0.grid.grad is not None and int(model.k0.grid.grad.count_nonzero()) > 0 and not route.pending
    route.abort()
    assert route.idle
    assert torch.equal(model.k0.grid.detach(), before)


@pytest.mark.parametrize('nhwc', [False, True])
@pytest.mark.parametrize('terms_on', [(True, True, True), (False, False, False), (True, False, True)])
def test_fused_joint_loss_terms_equal_the_op_sequence(nhwc, terms_on, monkeypatch):
    """JointTrainer.losses with the elementwise terms as ONE autograd node (train_ops.JointSmallLosses: k4_joint_losses_fwd / _bwd) against the same method on
    the tensor-library op sequence of run_sr.py:877-995 (checked against the oracle's restatement in tests/test_joint_cpu.py): every term, the total and the
    gradients w.r.t. rgb_feature, rgb_sr, alphainv_last, raw_rgb and weights (the distortion term's) -- values 2e-6 relative (fp64 sums against the library's
    fp32 trees), gradients 1e-6 of their scale; decoder result as NCHW and as the NHWC view the training tape hands out; transmittances on and beyond the clamp."""
    ent_on, dist_on, per_on = terms_on
    g = torch.Generator().manual_seed(31 + int(nhwc) + 2 * int(ent_on))
    pr, pc, n_pts = 7, 9, 333
    n = pr * pc
    base = {'rgb_feature': torch.rand([n, 3], generator=g), 'alphainv_last': torch.rand([n], generator=g),
            'weights': torch.rand([n_pts], generator=g) * 0.1, 'raw_rgb': torch.rand([n_pts, 3], generator=g),
            'ray_id': torch.sort(torch.randint(0, n, [n_pts], generator=g)).values, 's': torch.sort(torch.rand([n_pts], generator=g)).values, 'n_max': 12}
    base['alphainv_last'][:5] = torch.tensor([0.0, 1.0, 1e-9, 1e-6, 1 - 1e-6])
    base['rgb_feature'][3] = 0.25                                           # exact ties: sign(0) = 0
    sr0 = torch.rand([1, 3, 4 * pr, 4 * pc], generator=g) * 1.4 - 0.2      # beyond [0, 1]: the PSNR clamps
    target, target_4x = torch.rand([n, 3], generator=g).cuda(), torch.rand([16 * n, 3], generator=g).cuda()
    target[3] = 0.25
    cfg = joint_train.JointCfg.fern_lg_joint_l1(weight_entropy_last=0.001 if ent_on else 0, weight_distortion=0.01 if dist_on else 0, weight_rgbper=0.01 if per_on else 0)
    tr = joint_train.JointTrainer.__new__(joint_train.JointTrainer)
    tr.cfg, tr.sr_ratio = cfg, 4
    res = []
    for fused in (False, True):
        monkeypatch.setattr(joint_train, '_FUSED_LOSSES', fused)
        rr = {k: (v.cuda().requires_grad_(True) if torch.is_tensor(v) and v.is_floating_point() and k != 's' else (v.cuda() if torch.is_tensor(v) else v)) for k, v in base.items()}
        leaf = (sr0.permute(0, 2, 3, 1).contiguous().cuda() if nhwc else sr0.cuda()).requires_grad_(True)
        rgb_sr = leaf.permute(0, 3, 1, 2) if nhwc else leaf
        with torch.enable_grad():
            out = tr.losses(rr, rgb_sr, target, target_4x, pr, pc, n)
            out['total'].backward()
        res.append(({k: float(v) for k, v in out.items()}, [rr[k].grad for k in ('rgb_feature', 'alphainv_last', 'raw_rgb', 'weights')] + [leaf.grad]))
    (v0, g0), (v1, g1) = res
    assert set(v0) == set(v1) == {'photo', 'l1', 'psnr_sr', 'total'} | ({'entropy_last'} if ent_on else set()) | ({'distortion'} if dist_on else set()) | ({'rgbper'} if per_on else set())
    for k in v0:
        assert abs(v1[k] - v0[k]) <= 2e-6 * abs(v0[k]) + 1e-9, (k, v1[k], v0[k])
    for name, a, b in zip(('rgb_feature', 'alphainv_last', 'raw_rgb', 'weights', 'rgb_sr'), g1, g0):
        assert (a is None) == (b is None), name
        if b is not None:
            assert a.shape == b.shape
            _close(a, b.cpu(), name, rel=1e-6, abs_=1e-12)
    assert g0[4] is not None and g0[0] is not None and (g0[1] is not None) == ent_on and (g0[2] is not None) == per_on and (g0[3] is not None) == dist_on


def test_fused_joint_loss_terms_without_any_sample(monkeypatch):
    """A patch whose rays pick up no sample (empty space): the per-sample terms are zero, their gradients empty, in both forms."""
    g = torch.Generator().manual_seed(5)
    pr, pc = 4, 6
    n = pr * pc
    target, target_4x = torch.rand([n, 3], generator=g).cuda(), torch.rand([16 * n, 3], generator=g).cuda()
    cfg = joint_train.JointCfg.fern_lg_joint_l1()
    tr = joint_train.JointTrainer.__new__(joint_train.JointTrainer)
    tr.cfg, tr.sr_ratio = cfg, 4
    res = []
    for fused in (False, True):
        monkeypatch.setattr(joint_train, '_FUSED_LOSSES', fused)
        rr = {'rgb_feature': torch.rand([n, 3], generator=torch.Generator().manual_seed(6)).cuda().requires_grad_(True),
              'alphainv_last': torch.ones([n]).cuda().requires_grad_(True), 'weights': torch.zeros([0]).cuda().requires_grad_(True),
              'raw_rgb': torch.zeros([0, 3]).cuda().requires_grad_(True), 'ray_id': torch.zeros([0], dtype=torch.int64).cuda(), 's': torch.zeros([0]).cuda(), 'n_max': 12}
        sr = torch.rand([1, 3, 4 * pr, 4 * pc], generator=torch.Generator().manual_seed(7)).cuda().requires_grad_(True)
        with torch.enable_grad():
            out = tr.losses(rr, sr, target, target_4x, pr, pc, n)
            out['total'].backward()
        res.append(({k: float(v) for k, v in out.items()}, rr['rgb_feature'].grad, sr.grad, rr['alphainv_last'].grad))
    (v0, *g0), (v1, *g1) = res
    assert v0['rgbper'] == 0.0 and v1['rgbper'] == 0.0 and v0['distortion'] == 0.0 and v1['distortion'] == 0.0
    for k in v0:
        assert abs(v1[k] - v0[k]) <= 2e-6 * abs(v0[k]) + 1e-9, (k, v1[k], v0[k])
    for a, b in zip(g1, g0):
        assert (a is None) == (b is None)
        if b is not None:
            _close(a, b.cpu(), 'grad', rel=1e-6, abs_=1e-12)


def test_rgbnet_layer_by_layer_path_and_rejected_shapes():
    """the layer-by-layer path (`rgbnet_sigmoid_layers`: stacks outside k4_rgbnet_fwd's shapes, inference only) against the
    module itself in fp64, including a depth-4 stack, odd widths and an input count that is not a multiple of 4 -- and the shapes that ARE
    rejected, on the GPU under no_grad (so that it is the shape, not the device or autograd, that raises)."""
    from torch import nn
    torch.manual_seed(3)
    x = torch.randn([1000, 39], device='cuda')
    add = torch.randn([1000, 3], device='cuda')
    for net, xin, ad in ((dmpigo._mlp(39, 128, 4, 3), x, None),                                     # two hidden->hidden layers (depth 4)
                         (nn.Sequential(nn.Linear(15, 48), nn.ReLU(), nn.Linear(48, 3)), x[:, :15].contiguous(), add),                  # width 48
                         (nn.Sequential(nn.Linear(13, 40), nn.ReLU(), nn.Linear(40, 24), nn.ReLU(), nn.Linear(24, 3)), x[:, :13].contiguous(), None)):  # cin % 4 != 0, uneven widths
        net = net.cuda()
        assert not train_ops.rgbnet_supported(net)
        with torch.no_grad():
            got = train_ops.rgbnet_sigmoid_layers(net, xin, ad)
            want = torch.sigmoid(net.double()(xin.double()) + (0 if ad is None else ad.double()))
        assert got.shape == (1000, 3) and float((got.double() - want).abs().max()) <= 2e-6
        net.float()
        with torch.enable_grad(), pytest.raises(N.K4Error):                                           # these shapes do not train
            train_ops.rgbnet_sigmoid_layers(net, xin, ad)
    rejected = [nn.Sequential(nn.Linear(15, 48), nn.Tanh(), nn.Linear(48, 3)),                        # another activation
                nn.Sequential(nn.Linear(15, 48, bias=False), nn.ReLU(), nn.Linear(48, 3)),            # a bias-free Linear
                nn.Sequential(nn.Linear(15, 160), nn.ReLU(), nn.Linear(160, 3)),                      # wider than 128
                nn.Sequential(nn.Linear(15, 48), nn.ReLU(), nn.Linear(48, 4))]                        # not 3 outputs
    with torch.no_grad():
        for net in rejected:
            with pytest.raises(N.K4Error):
                train_ops.rgbnet_sigmoid_layers(net.cuda(), x[:, :15].contiguous())


@pytest.mark.parametrize('P,V,C', [(0, 0, 9), (2, 3, 12), (1, 0, 4)])
def test_fused_rgbnet_input_equals_the_reference_op_sequence(P, V, C):
    """train_ops.RgbnetInputMPI (k4_rgbnet_input_mpi: the colour MLP's input of DirectMPIGO's training forward in one launch) against the reference's op
    sequence (lib/dmpigo.py:360-374: normalised flipped position, frequency embeddings of position and view direction, gather by ray, concatenation):
    identical bits -- without frequencies (the LLFF configuration) and with them -- and the same gradient for the voxel features."""
    from nerf4k_amd.lib import train_ops
    g = torch.Generator().manual_seed(P * 7 + V * 3 + C)
    n, nr = 5000, 300
    vox = torch.randn([n, C], generator=g).cuda().requires_grad_(True)
    pts = (torch.rand([n, 3], generator=g) * 2 - 1).cuda()
    vd = torch.nn.functional.normalize(torch.randn([nr, 3], generator=g), dim=-1).cuda()
    rid = torch.randint(0, nr, [n], generator=g).sort().values.cuda()
    lo, hi = torch.tensor([-1.0, -1.1, -0.9]).cuda(), torch.tensor([1.2, 1.0, 1.1]).cuda()
    pf, vf = torch.FloatTensor([2 ** i for i in range(P)]).cuda(), torch.FloatTensor([2 ** i for i in range(V)]).cuda()
    x = train_ops.rgbnet_input_mpi(vox, pts, vd, rid, lo, hi, pf, vf)
    assert x is not None and x.shape == (n, C + 3 + 6 * P + 3 + 6 * V)
    gx = torch.randn(x.shape, generator=g).cuda()
    x.backward(gx)
    got_g = vox.grad.clone()
    vox2 = vox.detach().clone().requires_grad_(True)
    pe_spa = ((pts - lo) / (hi - lo)).flip((-1,)) * 2 - 1
    ve = (vd.unsqueeze(-1) * vf).flatten(-2)
    ve = torch.cat([vd, ve.sin(), ve.cos()], -1)[rid]
    pe = (pe_spa.unsqueeze(-1) * pf).flatten(-2)
    pe = torch.cat([pe_spa, pe.sin(), pe.cos()], -1)
    want = torch.cat([vox2, pe, ve], -1)
    want.backward(gx)
    assert torch.equal(x.detach(), want.detach()), float((x.detach() - want.detach()).abs().max())
    assert torch.equal(got_g, vox2.grad)


def test_split_grid_step_of_the_dense_tv_iterations_equals_the_one_pass_step(monkeypatch):
    """JointTrainer.step with a dense TV term written ahead: k0's optimizer step in two exact parts (MaskedAdam.early_step right after the forward pass for every voxel
    the lookups' backward cannot touch, the touched ones after the backward pass from the scatter's scratch image) against the one-pass step after the backward pass.
    Three iterations each way from the same state: same losses, same parameters / moments to the scatter atomics' rounding; the split form was really taken (the
    grid's gradient never exists, its flags are all zero again), and the sparse-TV iteration after tv_dense_before takes the one-pass route in both."""
    from nerf4k_amd.lib import masked_adam
    monkeypatch.setattr(masked_adam, '_MULTI_BELOW', 1000)
    res = []
    for split in (False, True):
        z, model, net, rk, cfg, batch = _load_joint()
        cfg = joint_train.JointCfg(dict(cfg, tv_before=100, tv_dense_before=3))          # steps 1, 2 dense; step 3 sparse
        monkeypatch.setattr(joint_train, '_SPLIT_GRID_STEP', split)
        tr = joint_train.JointTrainer(model, net, cfg, rk, n_train_images=17)
        taken = []
        early = masked_adam.MaskedAdam.early_step

        def spy(self, owner, seed, ev, _early=early, _taken=taken):
            ok = _early(self, owner, seed, ev)
            _taken.append(ok)
            return ok
        monkeypatch.setattr(masked_adam.MaskedAdam, 'early_step', spy)
        hist = []
        for i in range(3):
            hist.append(float(tr.step(*batch, global_step=1 + i)['total']))
            assert model.k0.grad_route.idle and not model.k0.grad_route.pending
            if split and i < 2:
                assert model.k0.grid.grad is None and int(model.k0.grad_route.flags.count_nonzero()) == 0
        monkeypatch.setattr(masked_adam.MaskedAdam, 'early_step', early)
        assert taken == ([True, True] if split else [])
        sd = model.state_dict()
        tr.optimizer.state_dict()                                                       # (waits for the grid's pending update)
        st = [tr.optimizer.state[p] for _, p in model.named_parameters() if p in tr.optimizer.state]      # (the split form creates k0's state earlier: keyed by parameter)
        moments = [v[k].detach().clone() for v in st for k in ('exp_avg', 'exp_avg_sq')]
        steps = [int(v['step']) for v in st]
        res.append((hist, {k: v.detach().clone() for k, v in sd.items() if v.is_floating_point()}, moments, steps))
    (h0, m0, a0, s0), (h1, m1, a1, s1) = res
    assert np.allclose(h1, h0, rtol=1e-6, atol=0), (h1, h0)
    assert s0 == s1 and len(a0) == len(a1)
    for k in m1:
        _close(m1[k], m0[k].cpu(), k, rel=1e-5, abs_=1e-8)
    for a, b in zip(a1, a0):
        _close(a, b.cpu(), 'optimizer moment', rel=1e-5, abs_=1e-9)


def _k0_sums_pending(tr, model, batch):
    """Forward + backward of one patch with k0 on the 'sparse' route: its gradient stays in the scratch image."""
    model.k0.grad_route.arm('sparse')
    with torch.enable_grad():
        rr, rgb_sr, ls = tr.forward(*batch, global_step=9)
        tr.optimizer.zero_grad(set_to_none=True)
        tr.optimizer_sr.zero_grad(set_to_none=True)
        ls['total'].backward()
    assert model.k0.grad_route.pending and model.k0.grid.grad is None


def test_scratch_image_with_pending_sums_is_handed_to_its_holder_only(monkeypatch):
    """While the scratch image holds a grid's pending gradient sums, a lookup backward for anybody else -- a grid of the same shape (it would sweep the foreign sums
    into its own gradient) or of another shape (it would free them) -- raises K4Error, and the sums are intact: swept afterwards they are the dense gradient of a
    run without the intruder (same non-zero voxels, values to the scatter atomics' 1e-5 relative)."""
    from nerf4k_amd.lib import masked_adam, grid as k4grid
    monkeypatch.setattr(masked_adam, '_MULTI_BELOW', 1000)
    grads = []
    for intruder in (False, True):
        z, model, net, rk, cfg, batch = _load_joint()
        tr = joint_train.JointTrainer(model, net, cfg, rk, n_train_images=17)
        _k0_sums_pending(tr, model, batch)
        if intruder:
            _, C_, X, Y, Z = model.k0.grid.shape
            dev = model.k0.grid.device
            pts = model.k0.xyz_min + (model.k0.xyz_max - model.k0.xyz_min) * torch.rand([50, 3], device=dev)
            for shape in ((C_, X, Y, Z), (C_, X + 1, Y, Z)):
                gg = torch.zeros([1, *shape], device=dev)
                with pytest.raises(N.K4Error, match='pending gradient'):
                    k4grid.grid_sample_3d_backward(torch.ones([50, C_], device=dev), *shape, pts, model.k0.xyz_min, model.k0.xyz_max, gg)
                assert int(gg.count_nonzero()) == 0
                other = k4grid.DenseGrid(C_, list(shape[1:]), model.k0.xyz_min, model.k0.xyz_max).to(dev)
                with torch.enable_grad(), pytest.raises(N.K4Error, match='pending gradient'):
                    other(pts).sum().backward()
            assert model.k0.grad_route.pending
        model.k0.grad_route.sweep()
        model.k0.grad_route.abort()
        assert model.k0.grad_route.idle and int(k4grid._GSB_WS[model.k0.grid.device].ws.count_nonzero()) == 0
        grads.append(model.k0.grid.grad.detach().clone())
    assert int(grads[0].count_nonzero()) > 0 and torch.equal(grads[0] != 0, grads[1] != 0)
    _close(grads[1], grads[0].cpu(), 'k0 gradient after the refused intruders', rel=1e-5, abs_=0)


def test_iteration_given_up_after_the_first_part_of_a_split_step_is_completed_from_the_seed(monkeypatch):
    """A dense-TV iteration whose k0 step was split (MaskedAdam.early_step) and that raises afterwards: GridGrad.abort completes the step from the seed alone, so k0,
    its moments and its step count are EXACTLY those of a one-pass masked_adam_upd with the TV term as the whole gradient (Adam is elementwise; the two-part step
    equals the one-pass step bit for bit, tests/test_optim_gpu.py); nothing of the iteration is left (route idle, flags and scratch image all zero or gone) and the
    next iteration runs.  An iteration that raises BEFORE the first part leaves k0, its moments and its step count untouched."""
    from nerf4k_amd.lib import masked_adam, grid as k4grid
    monkeypatch.setattr(masked_adam, '_MULTI_BELOW', 1000)
    z, model, net, rk, cfg, batch = _load_joint()
    cfg = joint_train.JointCfg(dict(cfg, tv_before=100, tv_dense_before=100))
    tr = joint_train.JointTrainer(model, net, cfg, rk, n_train_images=17)
    tr.step(*batch, global_step=1)                                                  # (creates k0's optimizer state)
    k0, route = model.k0.grid, model.k0.grad_route
    st = tr.optimizer.state[k0]
    pg = next(g for g in tr.optimizer.param_groups if any(p is k0 for p in g['params']))

    def snapshot():
        tr.optimizer.state_dict()                                                   # (waits for the grid's pending update)
        torch.cuda.synchronize()
        return [t.detach().clone() for t in (k0, st['exp_avg'], st['exp_avg_sq'])], int(st['step'])
    # before the first part: the model's forward raises
    before, step0 = snapshot()
    with monkeypatch.context() as mp:
        mp.setattr(type(model), 'forward', lambda *a, **k: (_ for _ in ()).throw(RuntimeError('no forward')))
        with pytest.raises(RuntimeError, match='no forward'):
            tr.step(*batch, global_step=2)
    after, step1 = snapshot()
    assert step1 == step0 and all(torch.equal(a, b) for a, b in zip(after, before)) and route.idle and not route.pending
    # after it: the exchange raises.  Expected: the one-pass step of the pre-iteration tensors with the TV term alone
    want = [t.clone() for t in before]
    k0.grad = torch.empty_like(k0)
    model.k0_total_variation_add_grad(cfg.weight_tv_k0 / 17, 'write')
    tv, k0.grad = k0.grad, None
    masked_adam.masked_adam_upd(*want[:1], tv, *want[1:], step0 + 1, *pg['betas'], pg['lr'], pg['eps'])
    taken = []
    early = masked_adam.MaskedAdam.early_step
    with monkeypatch.context() as mp:
        mp.setattr(masked_adam.MaskedAdam, 'early_step', lambda self, *a: taken.append(early(self, *a)) or taken[-1])
        mp.setattr(joint_train, 'exchange_gradients', lambda *a, **k: (_ for _ in ()).throw(RuntimeError('skip this batch')))
        with pytest.raises(RuntimeError, match='skip this batch'):
            tr.step(*batch, global_step=2)
    assert taken == [True]
    got, step2 = snapshot()
    assert step2 == step0 + 1 and route.idle and not route.pending
    for a, b, name in zip(got, want, ('k0', 'exp_avg', 'exp_avg_sq')):
        assert torch.equal(a, b), (name, float((a - b).abs().max()))
    img = k4grid._GSB_WS.get(k0.device)
    assert img is None or (img.holder is None and int(img.ws.count_nonzero()) == 0)
    assert route.flags is None or int(route.flags.count_nonzero()) == 0
    # ... and the next iteration is a normal one
    assert np.isfinite(float(tr.step(*batch, global_step=3)['total']))
    assert snapshot()[1] == step0 + 2 and route.idle
