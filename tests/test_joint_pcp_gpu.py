"""The joint iteration with the perceptual and style terms (4k-nerf_amd/joint_train.py with ``cri_perceptual``; run_sr.py:670-678, 929-957) on the small
synthetic MPI scene of tests/test_joint_gan_gpu.py: the full "+gan" preset with the discriminator, the same without the adversarial term, the two
terms' values and place in ``total``, and their gradient against the same step with that gradient added by hand."""
import contextlib
import io

import pytest
import torch

import nerf4k_amd  # noqa: F401
from nerf4k_amd import joint_train, scene
from nerf4k_amd.lib import dvgo, sr_esrnet, sr_loss, sr_unetdisc, utils

pytestmark = pytest.mark.gpu

TOL = 1e-5            # the cap of the stage bound of tests/test_sr_loss_gpu.py
P = 16                # patch side; the loss network and the discriminator see 64 x 64
LW = {'conv1_2': 0, 'conv2_2': 0, 'conv3_4': 1, 'conv4_4': 1, 'conv5_4': 1}


def _cri(pw=0.5, sw=0.2):
    return sr_loss.PerceptualLoss(LW, perceptual_weight=pw, style_weight=sw).load_vgg_state_dict(sr_loss.seeded_vgg19_state_dict(7)).to('cuda')


def _setup(cri=None, with_d=True, **over):
    dev = torch.device('cuda', 0)
    ck = scene.make_llff_checkpoint(seed=5, num_voxels=48 * 48 * 32, mpi_depth=32)
    H, W = 48, 64
    K = scene.LLFF_K.copy()
    K[:2] *= W / scene.LLFF_HW[1]
    ro, rd, vd = dvgo.get_rays_of_a_view(H, W, K, torch.from_numpy(scene.llff_spiral_poses()[3]).to(dev), True, False, False, False)
    model = utils.model_from_checkpoint_dict(ck).to(dev).train()
    torch.manual_seed(21)
    net = sr_esrnet.SFTNet(3, scale=4, num_feat=64, num_block=1, num_grow_ch=32, num_cond=1).to(dev).train()
    torch.manual_seed(22)
    net_d = sr_unetdisc.UNetDiscriminatorSN(3, num_feat=16, skip_connection=True).to(dev).train() if with_d else None
    cfg = joint_train.JointCfg.fern_lg_joint_l1_gan(**over)
    with contextlib.redirect_stdout(io.StringIO()):
        tr = joint_train.JointTrainer(model, net, cfg, dict(ck['render_kwargs'], render_depth=True), n_train_images=4, net_d=net_d, cri_perceptual=cri)
    g = torch.Generator().manual_seed(6)
    r0, c0 = 7, 11
    rays = [x[r0:r0 + P, c0:c0 + P].reshape(-1, 3).contiguous() for x in (ro, rd, vd)]
    batch = rays + [torch.rand([P * P, 3], generator=g).to(dev), torch.rand([16 * P * P, 3], generator=g).to(dev), P, P]
    return tr, model, net, batch


class _AddGrad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, g):
        ctx.save_for_backward(g)
        return x.view_as(x)

    @staticmethod
    def backward(ctx, go):
        return go + ctx.saved_tensors[0], None


def _step(tr, model, net, batch, extra_grad=None):
    """One step; returns (losses, the decoder output, `total` as losses() left it, every gradient at the moment the marcher's optimizer steps)."""
    seen = {}
    dec = tr._decoder

    def decoder(x, cond):
        y = dec(x, cond)
        seen['rgb_sr'] = y.detach().clone()
        return y if extra_grad is None else _AddGrad.apply(y, extra_grad)
    tr._decoder = decoder
    losses = tr.losses

    def spy_losses(*a):
        out = losses(*a)
        seen['total0'] = out['total'].detach().clone()
        return out
    tr.losses = spy_losses
    step_g = tr.optimizer.step

    def spy():
        seen['grads'] = {'model.' + k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
        seen['grads'].update({'net_sr.' + k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None})
        return step_g()
    tr.optimizer.step = spy
    torch.manual_seed(100)
    ls = tr.step(*batch, global_step=1)
    torch.cuda.synchronize()
    return ls, seen['rgb_sr'], seen['total0'], seen['grads']


@pytest.fixture
def dense_grid_grads(monkeypatch):
    # the grids' gradients as dense `.grad` tensors at the optimizer step, so that the test can read them (the routes are A/B attributes of the module)
    monkeypatch.setattr(joint_train, '_TV_SEED', False)
    monkeypatch.setattr(joint_train, '_SPLIT_GRID_STEP', False)
    monkeypatch.setattr(joint_train, '_SPARSE_GRID_GRAD', False)


@pytest.mark.parametrize('weight_gan', [0.05, 0.0])
def test_joint_step_with_the_perceptual_and_style_terms(weight_gan, dense_grid_grads):
    cri = _cri()
    tr, model, net, batch = _setup(cri, weight_gan=weight_gan)
    assert tr.cri_perceptual is cri and (tr.net_d is not None) == (weight_gan > 0)
    ls, rgb_sr, total0, grads = _step(tr, model, net, batch)
    want = {'photo', 'l1', 'psnr_sr', 'entropy_last', 'distortion', 'rgbper', 'pcp', 'style', 'total'} | ({'g', 'd_real', 'd_fake'} if weight_gan > 0 else set())
    assert set(ls) == want, sorted(ls)
    # the two terms are the module's, on the step's own decoder output
    rgb_hr = batch[4].reshape(4 * P, 4 * P, 3).movedim(-1, 0).unsqueeze(0)
    xi = rgb_sr.clone().requires_grad_(True)
    pcp, style = cri(xi, rgb_hr)
    assert torch.equal(ls['pcp'], pcp.detach()) and torch.equal(ls['style'], style.detach())
    assert 0.05 < float(pcp) < 2.0 and 1e-5 < float(style) < 1e-1, (float(pcp), float(style))
    # `total` is the reference's sum in its order: ... + l1, + pcp, + style, + g (run_sr.py:929, 936, 937, 954)
    total = (total0 + ls['pcp']) + ls['style']
    if weight_gan > 0:
        total = total + ls['g']
    assert torch.equal(ls['total'], total)
    print(f'joint + pcp (weight_gan={weight_gan}):', {k: round(float(v), 6) for k, v in ls.items()})
    # the gradients: the same step without the two terms, their gradient to rgb_sr added by hand
    (pcp + style).backward()
    tr2, model2, net2, batch2 = _setup(None, weight_gan=weight_gan, weight_pcp=0, weight_style=0)
    ls2, rgb_sr2, _, grads2 = _step(tr2, model2, net2, batch2, extra_grad=xi.grad)
    assert torch.equal(rgb_sr, rgb_sr2) and 'pcp' not in ls2
    assert set(grads) == set(grads2) and any(k.startswith('model.k0') for k in grads) and any(k.startswith('model.density') for k in grads)
    worst = ('', 0.0)
    for k in grads:
        e = float((grads[k] - grads2[k]).abs().max() / grads2[k].abs().max().clamp_min(1e-30))
        worst = max(worst, (k, e), key=lambda t: t[1])
        assert e <= TOL, (k, e)
    print('largest gradient deviation from the step with the gradient added by hand:', worst)
    # ... and the terms do reach the decoder: without them its gradient is a different one
    tr3, model3, net3, batch3 = _setup(None, weight_gan=weight_gan, weight_pcp=0, weight_style=0)
    _, _, _, grads3 = _step(tr3, model3, net3, batch3)
    # the baseline beside the figure above: the step without any module, run twice -- what the existing kernels' own run-to-run summation order gives
    tr4, model4, net4, batch4 = _setup(None, weight_gan=weight_gan, weight_pcp=0, weight_style=0)
    _, _, _, grads4 = _step(tr4, model4, net4, batch4)
    base = max(((k, float((grads3[k] - grads4[k]).abs().max() / grads4[k].abs().max().clamp_min(1e-30))) for k in grads3), key=lambda t: t[1])
    print('the same step without any module, two identical runs, largest gradient deviation:', base)
    assert base[1] <= TOL, base
    k = 'net_sr.conv_last.weight'
    assert float((grads[k] - grads3[k]).abs().max()) > 1e-2 * float(grads3[k].abs().max())


def test_without_the_terms_a_module_handed_in_changes_nothing():
    """The returned terms are compared bit for bit, as tests/test_joint_gan_gpu.py does for the discriminator.  The decoder's parameter gradients are not bit-stable
    from run to run even without any module, so the third run (no module again) shows what two identical runs give, printed and held to the same tolerance."""
    outs = []
    for cri in (_cri(), None, None):
        tr, model, net, batch = _setup(cri, weight_pcp=0, weight_style=0)
        assert tr.cri_perceptual is None
        torch.manual_seed(100)
        ls = tr.step(*batch, global_step=1)
        torch.cuda.synchronize()
        outs.append(({k: v.clone() for k, v in ls.items()}, net.conv_last.weight.grad.detach().clone()))
    assert set(outs[0][0]) == set(outs[1][0]) and 'pcp' not in outs[0][0] and 'style' not in outs[0][0]
    for k in outs[0][0]:
        assert torch.equal(outs[0][0][k], outs[1][0][k]), k
        assert torch.equal(outs[1][0][k], outs[2][0][k]), k
    scale = float(outs[1][1].abs().max())
    with_module, baseline = float((outs[0][1] - outs[1][1]).abs().max()) / scale, float((outs[2][1] - outs[1][1]).abs().max()) / scale
    print(f'conv_last.weight.grad: module handed in vs none {with_module:.3e}; none vs none {baseline:.3e}')
    assert with_module <= TOL and baseline <= TOL
