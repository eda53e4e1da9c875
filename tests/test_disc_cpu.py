"""U-Net SN discriminator and GAN loss, CPU side (4k-nerf_amd/lib/sr_unetdisc.py, tensor-library path) against tests/golden/disc_nf8.npz,
which tests/gen_disc_golden.py wrote from the reference's own class; the JointTrainer's handling of ``net_d``; the data-parallel exchange of
the discriminator's gradients (gloo, two ranks)."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn.functional as F

import nerf4k_amd  # noqa: F401
from nerf4k_amd import joint_train
from nerf4k_amd.lib import sr_unetdisc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'disc_nf8.npz')

# largest error of any tensor relative to that tensor's largest magnitude, tensor-library path vs the golden, measured on the build machine:
#   with one thread, as the generator ran: 0.0 on every tensor (the two classes issue the same operations);
#   with the library's default thread count (what this test runs with): 1.99e-6 on the 64x64 input (gradient of conv6.weight_orig, a sum over
#   4096 pixels split differently among the threads), 3.4e-7 on the 40x24 input.
# Asserted: 4x the larger figure.  The reference's own fp32 run differs from its fp64 run by 2.5e-7 .. 2.1e-6 on these shapes.
BOUND = 4 * 1.99e-6
assert BOUND <= 1e-5


def _z():
    return np.load(GOLDEN, allow_pickle=False)


def _sd(z):
    return {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith('sd/')}


def _rel(got, want):
    want = torch.as_tensor(want).double()
    return float((torch.as_tensor(got).double() - want).abs().max() / want.abs().max().clamp_min(1e-30))


def test_state_dict_keys_shapes_and_strict_loading_both_ways():
    z = _z()
    sd = _sd(z)
    net = sr_unetdisc.UNetDiscriminatorSN(3, num_feat=8)
    own = net.state_dict()
    assert len(own) == 28 and set(own) == set(sd)
    for k in sd:
        assert own[k].shape == sd[k].shape and own[k].dtype == sd[k].dtype, k
    want = {'conv0.weight', 'conv0.bias', 'conv9.weight', 'conv9.bias'} | {f'conv{i}.{s}' for i in range(1, 9) for s in ('weight_orig', 'weight_u', 'weight_v')}
    assert set(own) == want
    net.load_state_dict(sd, strict=True)
    # ... and a spectral_norm-wrapped torch module with the reference's layer list takes ours, strictly
    conv, sn = torch.nn.Conv2d, torch.nn.utils.spectral_norm
    other = torch.nn.Module()
    other.conv0 = conv(3, 8, 3, 1, 1)
    for i, (a, b, k, s) in enumerate([(8, 16, 4, 2), (16, 32, 4, 2), (32, 64, 4, 2), (64, 32, 3, 1), (32, 16, 3, 1), (16, 8, 3, 1), (8, 8, 3, 1), (8, 8, 3, 1)], 1):
        setattr(other, f'conv{i}', sn(conv(a, b, k, s, 1, bias=False)))
    other.conv9 = conv(8, 1, 3, 1, 1)
    other.load_state_dict(net.state_dict(), strict=True)
    assert sum(p.numel() for p in net.parameters()) == 68649
    # fresh modules are initialised like the wrapped ones: unit u, v
    fresh = sr_unetdisc.UNetDiscriminatorSN(3, num_feat=8)
    assert abs(float(fresh.conv3.weight_u.norm()) - 1) < 1e-6 and abs(float(fresh.conv3.weight_v.norm()) - 1) < 1e-6


@pytest.mark.parametrize('tag', ['a', 'b'])
def test_tensor_library_path_matches_the_reference(tag):
    """Measured here: worst tensor 1.99e-6 (input a) / 3.4e-7 (input b) of its largest magnitude; see BOUND."""
    z = _z()
    net = sr_unetdisc.UNetDiscriminatorSN(3, num_feat=8)
    net.load_state_dict(_sd(z))
    net.train()
    x = torch.from_numpy(z[f'x_{tag}']).requires_grad_(True)
    logits = net(x)
    F.softplus(-logits).mean().backward()
    errs = {'logits': _rel(logits.detach(), z[f'{tag}/logits']), 'gx': _rel(x.grad, z[f'{tag}/gx'])}
    for i in range(1, 9):
        m = getattr(net, f'conv{i}')
        errs[f'u{i}'] = _rel(m.weight_u, z[f'{tag}/u/conv{i}'])
        errs[f'v{i}'] = _rel(m.weight_v, z[f'{tag}/v/conv{i}'])
    for k, p in net.named_parameters():
        errs['g/' + k] = _rel(p.grad, z[f'{tag}/g/{k}'])
    net.load_state_dict(_sd(z))
    net.eval()
    with torch.no_grad():
        e1 = net(x.detach())
        e2 = net(x.detach())
    errs['eval'] = _rel(e1, z[f'{tag}/eval'])
    assert torch.equal(e1, e2) and torch.equal(net.conv1.weight_u, torch.from_numpy(z['sd/conv1.weight_u']))      # eval leaves u alone
    # the joint loop's three calls: frozen on the fake image, then real, then fake -- u advances every time
    net.load_state_dict(_sd(z))
    net.train()
    for p in net.parameters():
        p.requires_grad = False
    net(x.detach())
    for p in net.parameters():
        p.requires_grad = True
    net(torch.from_numpy(z[f'x2_{tag}']))
    net(x.detach())
    for i in range(1, 9):
        errs[f'u3/{i}'] = _rel(getattr(net, f'conv{i}').weight_u, z[f'{tag}/u3/conv{i}'])
    worst = max(errs, key=errs.get)
    print(f'disc cpu {tag}: worst relative error {errs[worst]:.3e} at {worst}')
    assert errs[worst] <= BOUND, (worst, errs[worst])


def test_gan_loss_is_bce_with_logits():
    g = torch.Generator().manual_seed(3)
    x = torch.randn([1, 1, 16, 24], generator=g) * 4
    x.view(-1)[:4] = torch.tensor([80., -80., 0., 1e-8])
    for w in (1.0, 0.05):
        cri = sr_unetdisc.GANLoss('vanilla', loss_weight=w)
        for real in (True, False):
            target = torch.ones_like(x) if real else torch.zeros_like(x)
            want = F.binary_cross_entropy_with_logits(x, target)
            want_soft = F.softplus(-x if real else x).mean()
            assert torch.isfinite(want) and abs(float(want - want_soft)) <= 1e-6 * float(want)
            assert torch.equal(cri(x, real, is_disc=True), want)                       # the discriminator's terms: never weighted
            assert torch.allclose(cri(x, real, is_disc=False), want * w, rtol=1e-7, atol=0)
            xi = x.clone().requires_grad_(True)
            cri(xi, real, is_disc=False).backward()
            sig = torch.sigmoid(-x if real else x) * (-1 if real else 1) * w / x.numel()
            assert float((xi.grad - sig).abs().max()) <= 1e-6 * float(sig.abs().max())      # (fp32 sigmoid: relative to the largest entry)
    with pytest.raises(NotImplementedError):
        sr_unetdisc.GANLoss('lsgan')


def _small_pair():
    from nerf4k_amd import scene
    from nerf4k_amd.lib import sr_esrnet, utils
    ck = scene.make_llff_checkpoint(seed=5, num_voxels=24 * 24 * 16, mpi_depth=16)
    model = utils.model_from_checkpoint_dict(ck)
    torch.manual_seed(1)
    return model, sr_esrnet.SFTNet(3, scale=4, num_feat=64, num_block=1, num_grow_ch=32, num_cond=1)


def test_joint_trainer_and_the_discriminator():
    cfg = joint_train.JointCfg.fern_lg_joint_l1_gan()
    assert (cfg.weight_pcp, cfg.weight_gan, cfg.weight_style) == (0.5, 0.05, 0.2) and cfg.lrate_srnet == 2e-4
    net_d = sr_unetdisc.UNetDiscriminatorSN(3, num_feat=8)
    with pytest.raises(NotImplementedError):                     # the preset as the configuration file states it: perceptual terms raise
        joint_train.JointTrainer(None, None, cfg, {}, 1, net_d=net_d)
    with pytest.raises(NotImplementedError):
        joint_train.JointTrainer(None, None, joint_train.JointCfg.fern_lg_joint_l1(weight_pcp=0.5), {}, 1)
    with pytest.raises(NotImplementedError):
        joint_train.JointTrainer(None, None, joint_train.JointCfg.fern_lg_joint_l1(weight_style=0.2), {}, 1, net_d=net_d)
    cfg = joint_train.JointCfg.fern_lg_joint_l1_gan(weight_pcp=0, weight_style=0)
    with pytest.raises(NotImplementedError):                     # the adversarial term without a discriminator
        joint_train.JointTrainer(None, None, cfg, {}, 1)
    model, net_sr = _small_pair()
    tr = joint_train.JointTrainer(model, net_sr, cfg, {}, 1, net_d=net_d)
    assert tr.net_d is net_d and tr.optimizer_d is not None and tr.cri_gan.loss_weight == 0.05
    pg = tr.optimizer_d.param_groups
    assert len(pg) == 1 and pg[0]['lr'] == cfg.lrate_srnet and pg[0]['skip_zero_grad'] is False
    assert {id(p) for p in pg[0]['params']} == {id(p) for p in net_d.parameters()}
    # without the term a discriminator handed in is ignored
    tr0 = joint_train.JointTrainer(model, net_sr, joint_train.JointCfg.fern_lg_joint_l1(), {}, 1, net_d=net_d)
    assert tr0.net_d is None and tr0.optimizer_d is None


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dp_worker(rank, world, port, q):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        torch.set_num_threads(1)
        torch.manual_seed(0)                                      # identical replicas
        net_d = sr_unetdisc.UNetDiscriminatorSN(3, num_feat=8)
        cfg = joint_train.JointCfg.fern_lg_joint_l1_gan(weight_pcp=0, weight_style=0)
        tr = joint_train.JointTrainer(*_small_pair(), cfg, {}, 1, net_d=net_d)
        tr.optimizer_d.step = lambda: None                        # keep the parameters: the test reads the exchanged gradients
        g = torch.Generator().manual_seed(10 + rank)              # each rank its own patch
        rgb_sr = torch.rand([1, 3, 16, 16], generator=g)
        target_4x = torch.rand([256, 3], generator=g)
        local = sr_unetdisc.UNetDiscriminatorSN(3, num_feat=8)
        local.load_state_dict(net_d.state_dict())
        out = tr._discriminator_step(rgb_sr, target_4x, 4, 4)
        # the same two backward passes on a copy, without exchange
        cri = sr_unetdisc.GANLoss('vanilla', loss_weight=0.05)
        cri(local(target_4x.reshape(16, 16, 3).movedim(-1, 0).unsqueeze(0)), True, is_disc=True).backward()
        cri(local(rgb_sr), False, is_disc=True).backward()
        q.put((rank, torch.cat([p.grad.reshape(-1) for p in net_d.parameters()]).numpy(),
               torch.cat([p.grad.reshape(-1) for p in local.parameters()]).numpy(), float(out['d_real']), float(out['d_fake'])))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_discriminator_gradients_are_averaged_across_ranks():
    world = 2
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = {}
    for _ in range(world):
        r, ex, loc, d_real, d_fake = q.get(timeout=240)
        got[r] = (ex, loc, d_real, d_fake)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert np.array_equal(got[0][0], got[1][0])                                 # replicas hold the same gradient
    assert not np.array_equal(got[0][1], got[1][1])                             # ... although their patches differ
    want = (got[0][1].astype(np.float64) + got[1][1]) / 2
    np.testing.assert_allclose(got[0][0], want, rtol=0, atol=1e-7 * np.abs(want).max() + 1e-12)
    assert all(np.isfinite(v) and v > 0 for r in got for v in got[r][2:])
