"""Training with factored grids on the GPU: one MaskedAdam step of every factor parameter against oracle/optim.py, and one JointTrainer iteration with a
factored k0 (the DenseGrid-only gradient routes stay off)."""
import contextlib
import io
import os

import numpy as np
import pytest
import torch

import nerf4k_amd  # noqa: F401
from nerf4k_amd import joint_train, scene
from nerf4k_amd.lib import dvgo, dmpigo, grid as kgrid, sr_esrnet
from nerf4k_amd.lib.masked_adam import MaskedAdam
from oracle import optim as O
from helpers import GOLDEN

pytestmark = pytest.mark.gpu


def test_masked_adam_steps_every_factor_parameter_as_the_oracle():
    """The 4-D factors and the 2-D f_vec on MaskedAdam's ordinary path, masked (zero-gradient entries untouched).  Tolerances of tests/test_optim_gpu.py
    (the oracle emulates FMA through float64: rtol 2e-6, atol 1e-7 on moments, 2e-7 on parameters)."""
    torch.manual_seed(4)
    g = kgrid.TensoRFGrid(9, [7, 5, 9], [0, 0, 0], [1, 1, 1], {'n_comp': 5, 'n_comp_xy': 3}).cuda()
    gen = torch.Generator().manual_seed(5)
    before, grads = {}, {}
    for k, p in g.named_parameters():
        gr = torch.randn(p.shape, generator=gen)
        gr[torch.rand(p.shape, generator=gen) < 0.4] = 0
        before[k], grads[k] = p.detach().cpu().numpy().copy(), gr.numpy().copy()
        p.grad = gr.cuda()
    assert set(before) == {'xy_plane', 'xz_plane', 'yz_plane', 'x_vec', 'y_vec', 'z_vec', 'f_vec'}
    opt = MaskedAdam([{'params': list(g.parameters()), 'lr': 0.1, 'skip_zero_grad': True}])
    opt.step()
    torch.cuda.synchronize()
    for k, p in g.named_parameters():
        z = np.zeros_like(before[k])
        wp, wm, wv = O.adam_upd(before[k], grads[k], z, z, 1, 0.9, 0.99, 0.1, 1e-8, masked=True)
        st = opt.state[p]
        np.testing.assert_allclose(st['exp_avg'].cpu().numpy(), wm, rtol=2e-6, atol=1e-7, err_msg=k)
        np.testing.assert_allclose(st['exp_avg_sq'].cpu().numpy(), wv, rtol=2e-6, atol=1e-7, err_msg=k)
        np.testing.assert_allclose(p.detach().cpu().numpy(), wp, rtol=2e-6, atol=2e-7, err_msg=k)
        untouched = grads[k] == 0
        assert untouched.any() and np.array_equal(p.detach().cpu().numpy()[untouched], before[k][untouched]), k


P = 16


def test_joint_iteration_with_a_factored_k0():
    """The smallest configuration of the joint tests (tests/test_joint_gan_gpu.py: 48 x 48 x 32 MPI scene, 16 x 16 patch, one-block SFTNet) with k0 a TensoRFGrid.
    The loss is finite, no grid takes the sparse / split / side-stream routes, and after an iteration without total variation the factor gradients are those of
    the same forward and backward run outside the trainer.  Both are the same fp32 computation up to the order of the float-atomic sums; the bound is the
    measured one of the march goldens carried over by scale: 4 x the largest err32 / max|gradient| over the k0 factor gradients of tensorf_march_mpi.npz,
    times this tensor's largest magnitude."""
    z = np.load(os.path.join(GOLDEN, 'tensorf_march_mpi.npz'), allow_pickle=False)
    rel = 4 * max(float(z['grad/err32/' + k[len('grad/'):]]) / float(np.abs(z[k]).max()) for k in z.files if k.startswith('grad/k0.'))
    dev = torch.device('cuda', 0)
    ck = scene.make_llff_checkpoint(seed=5, num_voxels=48 * 48 * 32, mpi_depth=32)
    kw = dict(ck['model_kwargs'], k0_type='TensoRFGrid', k0_config={'n_comp': 8})
    torch.manual_seed(3)
    model = dmpigo.DirectMPIGO(**kw)
    missing = model.load_state_dict({k: v for k, v in ck['model_state_dict'].items() if k != 'k0.grid'}, strict=False)
    assert set(missing.missing_keys) == {'k0.' + k for k in ('xy_plane', 'xz_plane', 'yz_plane', 'x_vec', 'y_vec', 'z_vec', 'f_vec')}
    model = model.to(dev).train()
    H, W = 48, 64
    K = scene.LLFF_K.copy()
    K[:2] *= W / scene.LLFF_HW[1]
    ro, rd, vd = dvgo.get_rays_of_a_view(H, W, K, torch.from_numpy(scene.llff_spiral_poses()[3]).to(dev), True, False, False, False)
    torch.manual_seed(21)
    net = sr_esrnet.SFTNet(3, scale=4, num_feat=64, num_block=1, num_grow_ch=32, num_cond=1).to(dev).train()
    cfg = joint_train.JointCfg.fern_lg_joint_l1()
    with contextlib.redirect_stdout(io.StringIO()):
        tr = joint_train.JointTrainer(model, net, cfg, dict(ck['render_kwargs'], render_depth=True), n_train_images=4)
    assert tr._sparse_grid_owners() == [] and tr.optimizer._side == []
    gen = torch.Generator().manual_seed(6)
    rays = [x[7:7 + P, 11:11 + P].reshape(-1, 3).contiguous() for x in (ro, rd, vd)]
    batch = rays + [torch.rand([P * P, 3], generator=gen).to(dev), torch.rand([16 * P * P, 3], generator=gen).to(dev), P, P]
    step = cfg.tv_before + 1                                            # no total variation: .grad after the step is the backward pass's alone
    factors = {k: p for k, p in model.k0.named_parameters()}
    torch.manual_seed(100)
    with torch.enable_grad():
        _, _, ls = tr.forward(*batch, step)
        tr.optimizer.zero_grad(set_to_none=True)
        tr.optimizer_sr.zero_grad(set_to_none=True)
        ls['total'].backward()
    outside = {k: p.grad.detach().clone() for k, p in factors.items()}
    assert all(float(v.abs().max()) > 0 for v in outside.values())
    torch.manual_seed(100)
    losses = tr.step(*batch, global_step=step)
    torch.cuda.synchronize()
    assert all(np.isfinite(float(v)) for v in losses.values())
    assert tr._sparse_grid_owners() == []
    for k, p in factors.items():
        err, scale = float((p.grad - outside[k]).abs().max()), float(outside[k].abs().max())
        print(f'k0.{k}: trainer vs outside {err:.3e} <= {rel * scale:.3e} ({rel:.2e} of {scale:.3e})')
        assert err <= rel * scale, (k, err, rel * scale)
    # an iteration with the dense total variation term runs too (the seeded route is DenseGrid-only: the term is added after the backward pass)
    losses = tr.step(*batch, global_step=1)
    assert all(np.isfinite(float(v)) for v in losses.values())
