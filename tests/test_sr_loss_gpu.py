"""The perceptual / style terms on the GPU (4k-nerf_amd/lib/sr_loss.py on csrc/k4_vgg.hip) against tests/vgg_oracle.py in fp64 on the same fp32 inputs.

The bound of a comparison is the largest error divided by the largest magnitude of the fp64 result, and it is MEASURED here: what torch fp32 on the CPU
shows against fp64 on the same inputs, times 4 (a different summation order over reductions up to 4608 long), and never above 1e-5, the bar of
tests/test_disc_gpu.py.  Every figure is printed in front of its assertion.

The end-to-end gradient cannot be compared that tightly: the two terms are piecewise smooth, and wherever a pre-activation, a pool gap or a feature / Gram
difference is within rounding of zero, two correct evaluations take different pieces (torch fp32 against torch fp64 on the CPU: 5e-7 relative L2 without a
flipped decision, 6e-4 .. 3.5e-3 with one).  So the product records its decisions (``sr_loss._KEEP_RECORD``), the checker evaluates the gradient WITH them
(``grad_with_record``) -- that comparison is tight -- and the record itself is checked against the checker's own decisions: every disagreement must sit
within 1e-5 of its tensor's largest magnitude from the kink, and there may be at most 10x as many (floor 16) as torch fp32 on the CPU shows.
The plain gradient against fp64 autograd is a backstop at the level of that kink noise."""
import functools

import pytest
import torch
import torch.nn.functional as F

import nerf4k_amd  # noqa: F401
from nerf4k_amd.lib import sr_loss
import vgg_oracle as VO

pytestmark = pytest.mark.gpu

SIZES = [(64, 64), (96, 160), (128, 128), (256, 256)]
LW = {'conv1_2': 0, 'conv2_2': 0, 'conv3_4': 1, 'conv4_4': 1, 'conv5_4': 1}           # run_sr.py:671-677
PW, SW = 0.5, 0.2                                                                       # configs/llff/fern_lg_joint_l1+gan.py
CAP = 1e-5
DEV = 'cuda'


@functools.lru_cache(None)
def _sd():
    return sr_loss.seeded_vgg19_state_dict(7)


def _rel(got, want):
    want = torch.as_tensor(want).double().cpu()
    return float((torch.as_tensor(got).double().cpu() - want).abs().max() / want.abs().max().clamp_min(1e-300))


def _check(what, got, cpu32, want64):
    """got: the product; cpu32: torch fp32 on the CPU; want64: fp64 -- all on the same fp32 inputs."""
    e_cpu, e = _rel(cpu32, want64), _rel(got, want64)
    bound = min(4 * e_cpu, CAP)
    print(f'{what}: product {e:.3e}  torch fp32 CPU {e_cpu:.3e}  bound {bound:.3e}')
    assert e <= bound, (what, e, e_cpu, bound)


def _nchw(t):          # [B, H, W, C] -> [B, C, H, W]
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _layer_cases(H, W):
    """(name, cin, cout, h, w, pool follows) of every 3x3 layer behind conv1_1, one per distinct (cin, cout, size)."""
    out, seen = [], set()
    h, w = H, W
    for i, n in enumerate(VO.NAMES[:35]):
        if n.startswith('pool'):
            h, w = h // 2, w // 2
        if n.startswith('conv') and n != 'conv1_1':
            cout, cin = sr_loss.CONV_SHAPES[n]
            pool = VO.NAMES[i + 2].startswith('pool') if i + 2 < 35 else False
            if (cin, cout, h, w) not in seen or pool:
                seen.add((cin, cout, h, w))
                out.append((n, cin, cout, h, w, pool))
    return out


def _wb(name):
    i = VO.NAMES.index(name)
    return _sd()[f'features.{i}.weight'], _sd()[f'features.{i}.bias']


@pytest.mark.parametrize('H,W', SIZES)
def test_convolution_forward_with_tap_and_pool(H, W):
    g = torch.Generator().manual_seed(H * 1000 + W)
    for name, cin, cout, h, w, pool in _layer_cases(H, W):
        wt, b = _wb(name)
        x = torch.relu(torch.randn([2, cin, h, w], generator=g))                           # what a layer of the stack sees: a batch of two post-ReLU images
        want = F.conv2d(x.double(), wt.double(), b.double(), 1, 1)
        cpu = F.conv2d(x, wt, b, 1, 1)
        op = sr_loss.pack_weight(wt.to(DEV), sr_loss.FWD)
        y, pre, yp = sr_loss.conv3x3(_nhwc(x).to(DEV), op, b.to(DEV), cout, relu=True, keep_relu=True, keep_pre=True, pool=pool)
        _check(f'{name} {cin}->{cout} {h}x{w} pre-ReLU', _nchw(pre), cpu, want)
        _check(f'{name} {cin}->{cout} {h}x{w} post-ReLU', _nchw(y), torch.relu(cpu), torch.relu(want))
        assert torch.equal(y, torch.relu(pre))
        if pool:                                                                             # the pooled image is the pool of the full image that was written
            assert torch.equal(_nchw(yp), F.max_pool2d(_nchw(y), 2, 2)), name
        y2, pre2, _ = sr_loss.conv3x3(_nhwc(x).to(DEV), op, b.to(DEV), cout, relu=True, keep_relu=False, keep_pre=True)
        assert y2 is None and torch.equal(pre2, pre)
    # conv1_1: planar input, normalisation in the load (zero padding of the NORMALISED image)
    wt, b = _wb('conv1_1')
    x = torch.rand([2, 3, H, W], generator=g)
    mean, std = torch.tensor(sr_loss.MEAN), torch.tensor(sr_loss.STD)
    want = F.conv2d((x.double() - mean.double().view(1, 3, 1, 1)) / std.double().view(1, 3, 1, 1), wt.double(), b.double(), 1, 1)
    cpu = F.conv2d((x - mean.view(1, 3, 1, 1)) / std.view(1, 3, 1, 1), wt, b, 1, 1)
    xd = x.to(DEV)
    y, pre = sr_loss.conv1_1(xd[0].contiguous(), xd[1].contiguous(), mean.to(DEV), std.to(DEV), wt.to(DEV), b.to(DEV), keep_relu=True, keep_pre=True)
    _check(f'conv1_1 {H}x{W} pre-ReLU', _nchw(pre), cpu, want)
    _check(f'conv1_1 {H}x{W} post-ReLU', _nchw(y), torch.relu(cpu), torch.relu(want))


@pytest.mark.parametrize('H,W', SIZES)
def test_input_gradient_with_the_mask_supplied_to_both_sides(H, W):
    g = torch.Generator().manual_seed(H * 1000 + W + 1)
    for name, cin, cout, h, w, _ in _layer_cases(H, W):
        wt, _b = _wb(name)
        gy = torch.randn([1, cout, h, w], generator=g)
        act = torch.relu(torch.randn([1, cin, h, w], generator=g))                          # the saved activation of the producing layer
        add = torch.randn([1, cin, h, w], generator=g)
        mask = act > 0
        want = F.conv_transpose2d(gy.double(), wt.double(), None, 1, 1) * mask + add.double()
        cpu = F.conv_transpose2d(gy, wt, None, 1, 1) * mask + add
        op = sr_loss.pack_weight(wt.to(DEV), sr_loss.DGRAD)
        got = sr_loss.conv3x3_dgrad(_nhwc(gy).to(DEV), op, cin, mask=_nhwc(act).to(DEV), add=_nhwc(add).to(DEV))
        _check(f'd {name} {cout}->{cin} {h}x{w} masked + seed', _nchw(got), cpu, want)
        got = sr_loss.conv3x3_dgrad(_nhwc(gy).to(DEV), op, cin)
        _check(f'd {name} {cout}->{cin} {h}x{w} plain', _nchw(got), F.conv_transpose2d(gy, wt, None, 1, 1), F.conv_transpose2d(gy.double(), wt.double(), None, 1, 1))
    wt, _b = _wb('conv1_1')
    std = torch.tensor(sr_loss.STD)
    gy = torch.randn([1, 64, H, W], generator=g)
    want = F.conv_transpose2d(gy.double(), wt.double(), None, 1, 1) / std.double().view(1, 3, 1, 1)
    cpu = F.conv_transpose2d(gy, wt, None, 1, 1) / std.view(1, 3, 1, 1)
    got = sr_loss.conv1_1_bwd(_nhwc(gy)[0].to(DEV), wt.to(DEV), std.to(DEV))
    _check(f'd conv1_1 {H}x{W} planar, 1/std', got.unsqueeze(0), cpu, want)


@pytest.mark.parametrize('H,W', SIZES)
def test_pool_routing(H, W):
    g = torch.Generator().manual_seed(H * 1000 + W + 2)
    for C, h, w in ((64, H, W), (128, H // 2, W // 2), (256, H // 4, W // 4), (512, H // 8, W // 8)):
        n = C * h * w
        act = ((torch.randperm(n, generator=g).float() + 1) / n).reshape(1, C, h, w)          # tie-free, positive
        gp = torch.randn([1, C, h // 2, w // 2], generator=g)
        a = act.clone().requires_grad_(True)
        F.max_pool2d(a, 2, 2).backward(gp)
        got = sr_loss.pool_bwd(_nhwc(act)[0].to(DEV), _nhwc(gp)[0].to(DEV))
        assert torch.equal(_nchw(got.unsqueeze(0)).cpu(), a.grad), (C, h, w)
        # the ReLU mask and the seed: zeros (and negatives under relu_mask) take no gradient, the seed is added everywhere
        act2 = act - 0.5
        add = torch.randn([1, C, h, w], generator=g)
        a = act2.clone().requires_grad_(True)
        F.max_pool2d(torch.relu(a), 2, 2).backward(gp)
        got = sr_loss.pool_bwd(_nhwc(torch.relu(act2))[0].to(DEV), _nhwc(gp)[0].to(DEV), add=_nhwc(add)[0].to(DEV))
        assert torch.equal(_nchw(got.unsqueeze(0)).cpu(), a.grad * (act2 > 0) + add), (C, h, w)
        # relu_mask=False: the plain pool gradient, negative maxima included
        a = act2.clone().requires_grad_(True)
        F.max_pool2d(a, 2, 2).backward(gp)
        got = sr_loss.pool_bwd(_nhwc(act2)[0].to(DEV), _nhwc(gp)[0].to(DEV), relu_mask=False)
        assert torch.equal(_nchw(got.unsqueeze(0)).cpu(), a.grad), (C, h, w)
        assert bool(((a.grad != 0) & (act2 < 0)).any())
    # ties: the first maximum in (dy, dx) order takes the gradient
    act = torch.ones([4, 4, 4], device=DEV)
    act[0, 1] = 2.0                                                                            # window (0, 0): candidate 1 is the only maximum
    act[2, 2:4] = 3.0                                                                          # window (1, 1): candidates 0 and 1 tie
    gp = torch.arange(1, 17, dtype=torch.float32, device=DEV).reshape(2, 2, 4)
    got = sr_loss.pool_bwd(act, gp)
    want = torch.zeros_like(act)
    want[0, 0], want[0, 2], want[2, 0], want[2, 2] = gp[0, 0], gp[0, 1], gp[1, 0], gp[1, 1]
    want[0, 0], want[0, 1] = 0, gp[0, 0]
    assert torch.equal(got, want)


@pytest.mark.parametrize('H,W', SIZES)
def test_gram_and_l1_heads(H, W):
    g = torch.Generator().manual_seed(H * 1000 + W + 3)
    for C, h, w in ((256, H // 4, W // 4), (512, H // 8, W // 8), (512, H // 16, W // 16)):
        P = h * w
        f = torch.randn([2, P, C], generator=g)
        f[1] = f[0] + 0.1 * torch.randn([P, C], generator=g)
        fd = f.double()
        want = fd.transpose(1, 2).bmm(fd) / (C * P)
        cpu = f.transpose(1, 2).bmm(f) / (C * P)
        G = sr_loss.gram(f.to(DEV))
        _check(f'gram C={C} P={P}', G, cpu, want)
        # L1 of the two Gram matrices and of the two feature images, scale = 0.25
        for what, a, b in (('gram', G[0].cpu(), G[1].cpu()), ('feature', f[0], f[1])):
            got = sr_loss.l1_fwd(a.to(DEV), b.to(DEV), 0.25)
            assert got.dtype == torch.float64
            # (the module rounds the sum of the layers' terms to fp32 once; the same rounding here)
            _check(f'L1 {what} C={C} P={P}', got.float(), (a - b).abs().mean() * 0.25, (a.double() - b.double()).abs().mean() * 0.25)
        go = torch.tensor([0.75])
        add = torch.randn([P, C], generator=g)
        sgn = torch.sign(f[0] - f[1])
        got = sr_loss.l1_bwd(f[0].to(DEV), f[1].to(DEV), 0.25, go.to(DEV), add=add.to(DEV))
        _check(f'd L1 C={C} P={P}', got, sgn * (go * 0.25 / (P * C)) + add, sgn.double() * (0.75 * 0.25 / (P * C)) + add.double())
        assert torch.equal(sr_loss.l1_bwd(f[0].to(DEV), f[1].to(DEV), 0.25).cpu() != 0, sgn != 0)
        # the Gram term's gradient with the product's own signs: (2 / (C P)) S_sym f, S = go * scale / C^2 * sign(Gx - Gg)
        s = torch.sign(G[0] - G[1]).cpu()
        k = 0.75 * 0.25 / (C * C) / (C * P)
        want = fd[0] @ ((s + s.t()).double() * k)
        cpu = f[0] @ ((s + s.t()) * k)
        got = sr_loss.gram_bwd(f[0].reshape(h, w, C).to(DEV), G, 0.25, go.to(DEV))
        _check(f'd gram C={C} P={P}', got.reshape(P, C), cpu, want)
        got2 = sr_loss.gram_bwd(f[0].reshape(h, w, C).to(DEV), G, 0.25, go.to(DEV), add=add.reshape(h, w, C).to(DEV))
        _check(f'd gram + seed C={C} P={P}', got2.reshape(P, C), cpu + add, want + add.double())


# ---- the whole module -------------------------------------------------------------------------------------------------------------

def _images(H, W, seed):
    g = torch.Generator().manual_seed(seed)
    gt = torch.rand([1, 3, H, W], generator=g)
    return gt + 0.1 * torch.randn([1, 3, H, W], generator=g), gt


def _module(lw=LW, pw=PW, sw=SW):
    return sr_loss.PerceptualLoss(lw, perceptual_weight=pw, style_weight=sw).load_vgg_state_dict(_sd()).to(DEV)


def _run(cri, x, gt):
    xi = x.to(DEV).requires_grad_(True)
    p, s = cri(xi, gt.to(DEV))
    total = sum(t for t in (p, s) if t is not None)
    total.backward()
    return p, s, xi.grad


@functools.lru_cache(None)
def _whole(H, W):
    """Everything the whole-module tests of one size compare, computed once."""
    was = sr_loss._KEEP_RECORD
    sr_loss._KEEP_RECORD = True
    try:
        x, gt = _images(H, W, 100 * H + W)
        cri = _module()
        p, s, grad = _run(cri, x, gt)
        rec = {k: {n: v.cpu() for n, v in d.items()} for k, d in cri.k4_record.items()}
        ext = sr_loss.VGGFeatureExtractor(['conv3_4', 'conv4_4', 'conv5_4']).load_vgg_state_dict(_sd()).to(DEV)
        feats = {n: v.cpu() for n, v in ext(x.to(DEV)).items()}
    finally:
        sr_loss._KEEP_RECORD = was
    out = dict(x=x, gt=gt, p=float(p), s=float(s), grad=grad.cpu(), rec=rec, feats=feats)
    p64, p32 = VO.params_from_torchvision(_sd()), VO.params_from_torchvision(_sd(), torch.float32)
    with torch.no_grad():
        out['loss64'] = [float(t) for t in VO.losses(x.double(), gt.double(), p64, LW, PW, SW)]
        out['loss32'] = [float(t) for t in VO.losses(x, gt, p32, LW, PW, SW)]
        out['feats64'] = {n: VO.run_stack(x.double(), p64, 'conv5_4')['out'][n] for n in feats}
        out['feats32'] = {n: VO.run_stack(x, p32, 'conv5_4')['out'][n] for n in feats}
    out['dec64'], out['mar64'] = VO.decisions(x.double(), gt.double(), p64, LW)
    out['dec32'], _ = VO.decisions(x, gt, p32, LW)
    out['grad_rec64'] = VO.grad_with_record(x.double(), gt.double(), p64, rec, LW, PW, SW)
    out['grad_rec32'] = VO.grad_with_record(x, gt, p32, rec, LW, PW, SW)
    out['grad64'] = VO.grad_autograd(x.double(), gt.double(), p64, LW, PW, SW)
    e_ref = []
    for k in range(3):                                                                       # torch fp32 against torch fp64: the reference's own kink noise at this size
        xs, gs = (x, gt) if k == 0 else _images(H, W, 100 * H + W + k)
        a = out['grad64'] if k == 0 else VO.grad_autograd(xs.double(), gs.double(), p64, LW, PW, SW)
        b = VO.grad_autograd(xs, gs, p32, LW, PW, SW)
        e_ref.append(float((b.double() - a).norm() / a.norm()))
    out['e_ref'] = e_ref
    return out


@pytest.mark.parametrize('H,W', SIZES)
def test_module_features_and_losses(H, W):
    R = _whole(H, W)
    for n, f in R['feats'].items():
        _check(f'{H}x{W} feature {n}', f, R['feats32'][n], R['feats64'][n])
    for what, got, c32, w64 in (('percep', R['p'], R['loss32'][0], R['loss64'][0]), ('style', R['s'], R['loss32'][1], R['loss64'][1])):
        e, e_cpu = abs(got - w64) / abs(w64), abs(c32 - w64) / abs(w64)
        bound = min(4 * e_cpu, CAP)
        print(f'{H}x{W} {what}: {got:.8g}  fp64 {w64:.10g}  product {e:.3e}  torch fp32 CPU {e_cpu:.3e}  bound {bound:.3e}')
        assert e <= bound, (what, e, e_cpu, bound)
    assert 0.3 < R['p'] < 1.0 and 1e-4 < R['s'] < 1e-2


@pytest.mark.parametrize('H,W', SIZES)
def test_module_gradient_with_its_own_record(H, W):
    R = _whole(H, W)
    _check(f'{H}x{W} gradient, the product\'s decisions', R['grad'], R['grad_rec32'], R['grad_rec64'])


@pytest.mark.parametrize('H,W', SIZES)
def test_module_record_against_the_checkers_decisions(H, W):
    R = _whole(H, W)
    rec, d64, d32, mar = R['rec'], R['dec64'], R['dec32'], R['mar64']
    assert {k: set(v) for k, v in rec.items()} == {k: set(v) for k, v in d64.items()}
    worst = []
    for kind in ('relu_mask', 'pool_choice', 'feat_sign', 'gram_sign'):
        for n in d64[kind]:
            got, want, cpu, m = rec[kind][n], d64[kind][n], d32[kind][n], mar[kind][n]
            got = got.reshape(want.shape)
            assert got.dtype == want.dtype, (kind, n, got.dtype)
            bad = got != want
            if kind == 'pool_choice':                                                        # the gap between the two candidates chosen
                q = (m.gather(-1, got.long().unsqueeze(-1)) - m.gather(-1, want.long().unsqueeze(-1))).squeeze(-1).abs()
            else:
                q = m.abs()
            dist = float(q[bad].max() / m.abs().max()) if bad.any() else 0.0
            n_bad, n_cpu = int(bad.sum()), int((cpu.reshape(want.shape) != want).sum())
            allowed = max(10 * n_cpu, 16)
            worst.append((kind, n, n_bad, n_cpu, dist))
            print(f'{H}x{W} {kind}[{n}]: {n_bad} of {bad.numel()} differ from fp64 (torch fp32 CPU: {n_cpu}; allowed {allowed}); farthest from its kink {dist:.3e}')
            assert dist <= 1e-5, (kind, n, dist)
            assert n_bad <= allowed, (kind, n, n_bad, n_cpu)


@pytest.mark.parametrize('H,W', SIZES)
def test_module_plain_gradient_backstop(H, W):
    R = _whole(H, W)
    e = float((R['grad'].double() - R['grad64']).norm() / R['grad64'].norm())
    bound = max(4 * max(R['e_ref']), 1e-5)
    print(f'{H}x{W} plain gradient: relative L2 {e:.3e}; torch fp32 vs fp64 over three images {[f"{v:.3e}" for v in R["e_ref"]]}; bound {bound:.3e}')
    assert e <= bound


# ---- repeatability and interface --------------------------------------------------------------------------------------------------

def test_two_runs_are_bitwise_identical():
    x, gt = _images(64, 64, 1)
    cri = _module()
    a, b = _run(cri, x, gt), _run(cri, x, gt)
    c = _run(_module(), x, gt)
    for u, v in ((a, b), (a, c)):
        assert torch.equal(u[0], v[0]) and torch.equal(u[1], v[1]) and torch.equal(u[2], v[2])
    assert a[0].dtype == torch.float32 and a[0].dim() == 0 and float(a[2].abs().max()) > 0


def test_swapped_arguments_give_the_same_losses():
    x, gt = _images(64, 64, 2)
    cri = _module()
    with torch.no_grad():
        p, s = cri(x.to(DEV), gt.to(DEV))
        p2, s2 = cri(gt.to(DEV), x.to(DEV))
    assert torch.equal(p, p2) and torch.equal(s, s2)


def test_zero_weight_layers_change_nothing_and_zero_style_weight_is_none():
    x, gt = _images(64, 64, 3)
    a = _run(_module(), x, gt)
    b = _run(_module({'conv3_4': 1, 'conv4_4': 1, 'conv5_4': 1}), x, gt)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    p, s, g = _run(_module(sw=0.0), x, gt)
    assert s is None and torch.equal(p, a[0])
    p2, s2, g2 = _run(_module(pw=0.0), x, gt)
    assert p2 is None and torch.equal(s2, a[1])
    assert float((g + g2 - a[2]).abs().max()) <= 1e-5 * float(a[2].abs().max())             # the two terms' gradients add up
    # layer weights scale their term
    p3, _, _ = _run(_module({'conv3_4': 2.0}, sw=0.0), x, gt)
    p4, _, _ = _run(_module({'conv3_4': 1.0}, sw=0.0), x, gt)
    assert abs(float(p3) - 2 * float(p4)) <= 1e-6 * float(p3)


def test_gt_gradient_is_ignored_and_a_non_contiguous_input_gets_its_gradient():
    x, gt = _images(64, 96, 4)
    cri = _module()
    want = _run(cri, x, gt)
    base = x.permute(0, 2, 3, 1).contiguous().to(DEV).requires_grad_(True)                   # [1, H, W, 3]: the image below is a non-contiguous view
    xi = base.permute(0, 3, 1, 2)
    assert not xi.is_contiguous()
    gi = gt.to(DEV).requires_grad_(True)
    p, s = cri(xi, gi)
    (p + s).backward()
    assert gi.grad is None
    assert torch.equal(p, want[0]) and torch.equal(s, want[1])
    assert torch.equal(base.grad.permute(0, 3, 1, 2), want[2])
    # scaled upstream gradients reach the seeds on the device
    xj = x.to(DEV).requires_grad_(True)
    p, s = cri(xj, gt.to(DEV))
    (3.0 * p + 0.5 * s).backward()
    p_only = _run(_module(sw=0.0), x, gt)[2]
    s_only = _run(_module(pw=0.0), x, gt)[2]
    ref = 3.0 * p_only + 0.5 * s_only
    assert float((xj.grad - ref).abs().max()) <= 1e-5 * float(ref.abs().max())


def test_extractor_returns_the_requested_layers_and_unloaded_weights_raise():
    from nerf4k_amd import _native as N
    x, _ = _images(64, 64, 5)
    names = ['conv1_2', 'relu2_1', 'pool2', 'conv3_4']
    ext = sr_loss.VGGFeatureExtractor(names).load_vgg_state_dict(_sd()).to(DEV)
    out = ext(x.to(DEV))
    assert list(out) == names
    want = VO.run_stack(x.double(), VO.params_from_torchvision(_sd()), 'conv3_4')['out']
    for n in names:
        assert out[n].shape == want[n].shape
        assert _rel(out[n], want[n]) <= CAP, n
    with pytest.raises(N.K4Error, match='load_vgg_state_dict'):
        sr_loss.PerceptualLoss(LW).to(DEV)(x.to(DEV), x.to(DEV))
    with pytest.raises(N.K4Error):
        ext(torch.rand(1, 3, 40, 64, device=DEV))                                             # H not a multiple of 16
