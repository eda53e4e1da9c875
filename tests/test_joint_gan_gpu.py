"""The joint iteration with the adversarial term (4k-nerf_amd/joint_train.py with ``net_d``; run_sr.py:916-957, 1016-1061) on a small synthetic
MPI scene: the discriminator on the HIP path against the same iterations with it on the tensor-library path, and the bookkeeping of the
reference loop (frozen parameters in the generator phase, three power iterations per step, the third optimizer and its learning rate)."""
import contextlib
import io

import pytest
import torch
import torch.nn.functional as F

import nerf4k_amd  # noqa: F401
from nerf4k_amd import joint_train, scene
from nerf4k_amd.lib import dvgo, sr_esrnet, sr_unetdisc, utils

pytestmark = pytest.mark.gpu

TOL = 2e-5            # the bound of tests/test_disc_gpu.py::test_module_matches_the_tensor_library_path_in_fp64
P = 16                # patch side; the discriminator sees 64 x 64


def _setup(weight_gan, with_d=True, nf=16):
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
    net_d = sr_unetdisc.UNetDiscriminatorSN(3, num_feat=nf, skip_connection=True).to(dev).train() if with_d else None
    cfg = joint_train.JointCfg.fern_lg_joint_l1_gan(weight_pcp=0, weight_style=0, weight_gan=weight_gan)
    with contextlib.redirect_stdout(io.StringIO()):
        tr = joint_train.JointTrainer(model, net, cfg, dict(ck['render_kwargs'], render_depth=True), n_train_images=4, net_d=net_d)
    g = torch.Generator().manual_seed(6)
    batches = []
    for i in range(2):
        r0, c0 = 7 + 9 * i, 11 + 17 * i
        rays = [x[r0:r0 + P, c0:c0 + P].reshape(-1, 3).contiguous() for x in (ro, rd, vd)]
        batches.append(rays + [torch.rand([P * P, 3], generator=g).to(dev), torch.rand([16 * P * P, 3], generator=g).to(dev), P, P])
    return tr, net, net_d, batches


def _two_steps(tr, net, batches, probe=None):
    out = []
    for i, b in enumerate(batches):
        if probe is not None and i == 0:
            probe()
        torch.manual_seed(100 + i)
        ls = tr.step(*b, global_step=1 + i)
        out.append(({k: float(v) for k, v in ls.items()}, net.conv_last.weight.grad.detach().clone()))
    torch.cuda.synchronize()
    return out


def _relerr(a, b):
    return abs(a - b) / max(abs(b), 1e-30)


def test_joint_step_with_the_discriminator_on_both_paths(monkeypatch):
    tr, net, net_d, batches = _setup(0.05)
    sd0 = {k: v.clone() for k, v in net_d.state_dict().items()}
    seen = {}
    step_g = tr.optimizer.step

    def spy():                                          # the marcher's optimizer steps right after the generator phase's backward pass
        if 'frozen' not in seen:
            seen['frozen'] = all(p.grad is None and not p.requires_grad for p in net_d.parameters())
            seen['u_after_g'] = net_d.conv1.weight_u.clone()
        return step_g()
    tr.optimizer.step = spy
    u_mid = {}
    step_d = tr.optimizer_d.step

    def spy_d():
        if not u_mid:
            u_mid.update({i: (getattr(net_d, f'conv{i}').weight_u.clone(), getattr(net_d, f'conv{i}').weight_v.clone()) for i in range(1, 9)})
        return step_d()
    tr.optimizer_d.step = spy_d
    hip = _two_steps(tr, net, batches)
    assert seen['frozen'], 'the discriminator got a parameter gradient in the generator phase'
    assert all(p.requires_grad and p.grad is not None for p in net_d.parameters())
    moved = [k for k, p in net_d.named_parameters() if not torch.equal(p.detach(), sd0[k])]
    assert len(moved) == 12, moved
    # exactly three power iterations in the first step (the weights are those of sd0 until optimizer_d.step)
    for i in range(1, 9):
        w = sd0[f'conv{i}.weight_orig'].double().cpu()
        wm = w.reshape(w.shape[0], -1)
        u, v = sd0[f'conv{i}.weight_u'].double().cpu(), sd0[f'conv{i}.weight_v'].double().cpu()
        trail = []
        for _ in range(4):
            v = F.normalize(wm.t() @ u, dim=0, eps=1e-12)
            u = F.normalize(wm @ v, dim=0, eps=1e-12)
            trail.append(u)
        err = [float((u_mid[i][0].double().cpu() - t).abs().max() / t.abs().max()) for t in trail]
        assert err[2] <= TOL, (i, err)
        if i <= 3:                                      # (the deep layers' iteration has visibly not converged after two steps)
            assert err[1] > TOL or err[3] > TOL or err[2] < min(err[1], err[3]), (i, err)
    factor = 0.1 ** (1 / (tr.cfg.lrate_decay * 1000))
    assert abs(tr.optimizer_d.param_groups[0]['lr'] - tr.cfg.lrate_srnet * factor ** 2) <= 1e-12
    assert abs(tr.optimizer_sr.param_groups[0]['lr'] - tr.cfg.lrate_srnet * factor ** 2) <= 1e-12
    # the same two iterations with the discriminator on the tensor-library path
    monkeypatch.setattr(sr_unetdisc, '_K4', False)
    tr2, net2, net_d2, batches2 = _setup(0.05)
    lib = _two_steps(tr2, net2, batches2)
    for it, ((a, ga), (b, gb)) in enumerate(zip(hip, lib)):
        assert set(a) == set(b) and {'g', 'd_real', 'd_fake', 'total'} <= set(a)
        errs = {k: _relerr(a[k], b[k]) for k in ('g', 'd_real', 'd_fake', 'total')}
        errs['conv_last.weight.grad'] = float((ga - gb).abs().max() / gb.abs().max())
        print(f'joint + gan, iteration {it}:', {k: f'{e:.2e}' for k, e in errs.items()}, {k: round(a[k], 6) for k in ('g', 'd_real', 'd_fake', 'total')})
        assert max(errs.values()) <= TOL, (it, errs)
        assert a['g'] > 0 and abs(a['g'] - 0.05 * 0.6931) < 0.05 * 0.3          # weighted: a near-chance discriminator gives weight_gan * ln 2


def test_without_the_term_a_discriminator_changes_nothing():
    outs = []
    for with_d in (True, False):
        tr, net, net_d, batches = _setup(0.0, with_d=with_d)
        assert tr.net_d is None and tr.optimizer_d is None
        torch.manual_seed(100)
        ls = tr.step(*batches[0], global_step=1)
        torch.cuda.synchronize()
        outs.append({k: v.clone() for k, v in ls.items()})
        if with_d:
            assert all(p.grad is None for p in net_d.parameters())
    assert set(outs[0]) == set(outs[1]) and 'g' not in outs[0]
    for k in outs[0]:
        assert torch.equal(outs[0][k], outs[1][k]), k
