"""LPIPS-VGG on the GPU (4k-nerf_amd/lib/lpips.py on csrc/k4_vgg.hip + csrc/k4_lpips.hip) against tests/lpips_oracle.py in fp64 on the same fp32 inputs,
with seeded weights.

Bounds.  A tensor follows tests/test_sr_loss_gpu.py::_check: the largest error over the largest magnitude of the fp64 result, at most min(4 * e_cpu, 1e-5),
e_cpu being what torch fp32 on the CPU shows against fp64 on the same inputs.  A scalar (a tap's value, the total) is held to its relative error, with
e_cpu the LARGEST relative error of torch fp32 on the CPU over all the pairs of that size (one pair's fp32 error varies from 5e-9 to 1.5e-7 by chance),
a floor of 2^-23 (the value is rounded to fp32 once) and the cap of 1e-5.  Every figure is printed in front of its assertion.

With the seeded head weights (U(0, 2 / C): a tap is about |n_0 - n_1|^2 / C) a near pair scores about 1e-3 and an independent pair about 1e-2.
Full-size frames (756 x 1008, 3024 x 4032) are exercised by tools/lpips_time.py, not here."""
import functools
import hashlib
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import nerf4k_amd  # noqa: F401
from nerf4k_amd import _native as N, render, scene
from nerf4k_amd.lib import lpips, sr_loss, utils
import lpips_oracle as LO

pytestmark = pytest.mark.gpu

DEV = 'cuda'
CAP, FLOOR = 1e-5, 2.0 ** -23
SENTINEL, GUARD = -12345.0, 4096
SEED = 11


@functools.lru_cache(None)
def _sd():
    return lpips.seeded_lpips_state_dict(SEED)


@functools.lru_cache(None)
def _module():
    return lpips.LPIPS(net='vgg', verbose=False).load_lpips_state_dict(_sd()).to(DEV)


@pytest.fixture(autouse=True)
def _clear_registered_weights():
    yield
    utils.load_lpips_weights(None)


def _rel(got, want):
    want = torch.as_tensor(want).double().cpu()
    return float((torch.as_tensor(got).double().cpu() - want).abs().max() / want.abs().max().clamp_min(1e-300))


def _check(what, got, cpu32, want64):
    e_cpu, e = _rel(cpu32, want64), _rel(got, want64)
    bound = min(4 * e_cpu, CAP)
    print(f'{what}: product {e:.3e}  torch fp32 CPU {e_cpu:.3e}  bound {bound:.3e}')
    assert e <= bound, (what, e, e_cpu, bound)


def _scalar_bound(cpu32, want64):
    """cpu32, want64: all the values of one quantity over the pairs of one size."""
    e_cpu = float(((cpu32.double() - want64).abs() / want64.abs().clamp_min(1e-300))[want64 != 0].max())
    return max(FLOOR, min(4 * e_cpu, CAP)), e_cpu


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _guarded(shape):
    """(whole buffer, the view handed to the kernel): GUARD sentinel floats on both sides."""
    n = int(np.prod(shape))
    buf = torch.full([GUARD + n + GUARD], SENTINEL, dtype=torch.float32, device=DEV)
    return buf, buf[GUARD:GUARD + n].view(shape)


def _guards_untouched(buf):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())


def _conv3x3_guarded(x, op, bias, cout, pool):
    B, H, W, cin = x.shape
    by, y = _guarded([B, H, W, cout])
    bp, yp = _guarded([B, H // 2, W // 2, cout]) if pool else (None, None)
    N.check(N.lib().k4_vgg_conv3x3(N.f32(x), cin, H, W, B, N.ptr(op), 3, N.f32(bias), N.f32(y), None, None if yp is None else N.f32(yp), cout, sr_loss.FWD, 1,
                                   None, None, N.stream()), 'k4_vgg_conv3x3')
    torch.cuda.synchronize()
    assert _guards_untouched(by) and (bp is None or _guards_untouched(bp)), 'a store left its buffer'
    assert not bool((y == SENTINEL).any()) and (yp is None or not bool((yp == SENTINEL).any())), 'an element was not written'
    return y, yp


# ---- 1. single layers on ragged sizes ---------------------------------------------------------------------------------------------
LAYER_CASES = [('net.slice1.2', 64, 37, 51), ('net.slice1.2', 64, 5, 1009), ('net.slice1.2', 64, 757, 9), ('net.slice2.7', 128, 18, 25),
               ('net.slice3.12', 256, 9, 12), ('net.slice4.19', 512, 4, 6), ('net.slice4.19', 512, 2, 3), ('net.slice4.19', 512, 1, 1)]


@pytest.mark.parametrize('key,C,H,W', LAYER_CASES)
def test_ragged_layer_with_and_without_pool(key, C, H, W):
    g = torch.Generator().manual_seed(H * 10007 + W)
    wt, b = _sd()[key + '.weight'], _sd()[key + '.bias']
    x = torch.relu(torch.randn([2, C, H, W], generator=g))
    want = torch.relu(F.conv2d(x.double(), wt.double(), b.double(), 1, 1))
    cpu = torch.relu(F.conv2d(x, wt, b, 1, 1))
    op = sr_loss.pack_weight(wt.to(DEV), sr_loss.FWD)
    xd, bd = _nhwc(x).to(DEV), b.to(DEV)
    y, _ = _conv3x3_guarded(xd, op, bd, C, pool=False)
    _check(f'{C}->{C} {H}x{W} post-ReLU', _nchw(y), cpu, want)
    if H < 2 or W < 2:                                  # no 2x2 window exists (torch refuses the shape too): refused, nothing is written
        band = torch.full([64], SENTINEL, dtype=torch.float32, device=DEV)
        rc = N.lib().k4_vgg_conv3x3(N.f32(xd), C, H, W, 2, N.ptr(op), 3, N.f32(bd), N.f32(torch.empty_like(y)), None, N.f32(band), C, sr_loss.FWD, 1, None, None, N.stream())
        torch.cuda.synchronize()
        assert rc == N.K4_ERR_UNSUPPORTED and bool((band == SENTINEL).all())
        return
    y2, yp = _conv3x3_guarded(xd, op, bd, C, pool=True)
    assert torch.equal(y2, y)
    assert tuple(yp.shape) == (2, H // 2, W // 2, C)
    assert torch.equal(_nchw(yp), F.max_pool2d(_nchw(y), 2, 2)), 'the pooled image is not the floor-mode pool of the image that was written'
    # the wrapper's own allocation (what the module uses) gives the same bits
    y3, _, yp3 = sr_loss.conv3x3(xd, op, bd, C, relu=True, keep_relu=True, pool=True)
    assert torch.equal(y3, y) and torch.equal(yp3, yp)


@pytest.mark.parametrize('H,W', [(37, 51), (17, 23)])
def test_ragged_conv1_1(H, W):
    g = torch.Generator().manual_seed(H * 10007 + W + 1)
    sd = _sd()
    wt, b = sd['net.slice1.0.weight'], sd['net.slice1.0.bias']
    shift, scale = sd['scaling_layer.shift'].reshape(3), sd['scaling_layer.scale'].reshape(3)
    x = torch.rand([2, 3, H, W], generator=g) * 2 - 1
    want = torch.relu(F.conv2d((x.double() - shift.double().view(1, 3, 1, 1)) / scale.double().view(1, 3, 1, 1), wt.double(), b.double(), 1, 1))
    cpu = torch.relu(F.conv2d((x - shift.view(1, 3, 1, 1)) / scale.view(1, 3, 1, 1), wt, b, 1, 1))
    xd, shift_d, scale_d, wd, bd = x.to(DEV), shift.to(DEV), scale.to(DEV), wt.to(DEV), b.to(DEV)          # (named: a temporary's block would be handed out again)
    buf, y = _guarded([2, H, W, 64])
    N.check(N.lib().k4_vgg_conv1_1(N.f32(xd[0]), N.f32(xd[1]), H, W, N.f32(shift_d), N.f32(scale_d), N.f32(wd), N.f32(bd), 64, N.f32(y), None, N.stream()),
            'k4_vgg_conv1_1')
    torch.cuda.synchronize()
    assert _guards_untouched(buf) and not bool((y == SENTINEL).any())
    _check(f'conv1_1 {H}x{W} post-ReLU', _nchw(y), cpu, want)


# ---- 2. the head alone ------------------------------------------------------------------------------------------------------------
def _head_inputs(C, n_pix, g):
    """Feature pairs [2, n_pix, C] that cover: all-zero in both images, in one image only, one channel only non-zero."""
    out = []
    base = torch.relu(torch.randn([2, n_pix, C], generator=g))
    if n_pix >= 6:
        f = base.clone()
        f[:, 0] = 0
        f[0, 1] = 0
        f[1, 2] = 0
        f[:, 3] = 0
        f[0, 3, 5], f[1, 3, C - 1] = 1.5, 0.25
        f[:, 4] = 0
        f[0, 4, 7], f[1, 4, 7] = 2.0, 3.0                # same direction: the normalised features are equal, the pixel adds an exact zero
        out.append(f)
        out.append(base)
    else:
        z = torch.zeros_like(base)
        one0, one1 = z.clone(), z.clone()
        one0[0, :, 3], one1[0, :, 3], one1[1, :, C - 2] = 0.75, 0.75, 4.0
        out += [base, z, torch.stack([z[0], base[1]]), torch.stack([base[0], z[1]]), one0, one1]
    return out


@pytest.mark.parametrize('C', [64, 512])
@pytest.mark.parametrize('n_pix', [1, 6, 1000])
def test_head_alone(C, n_pix):
    g = torch.Generator().manual_seed(C * 31 + n_pix)
    w = torch.rand([C], generator=g) * (2.0 / C)
    fs = _head_inputs(C, n_pix, g) + _head_inputs(C, n_pix, g)
    want = torch.stack([LO.head(f[0:1].double().permute(0, 2, 1).unsqueeze(-1), f[1:2].double().permute(0, 2, 1).unsqueeze(-1), w.double())[0] for f in fs])
    cpu = torch.stack([LO.head(f[0:1].permute(0, 2, 1).unsqueeze(-1), f[1:2].permute(0, 2, 1).unsqueeze(-1), w)[0] for f in fs])
    bound, e_cpu = _scalar_bound(cpu, want)
    taps = torch.full([len(fs) + 2], float(SENTINEL), dtype=torch.float64, device=DEV)
    for k, f in enumerate(fs):
        lpips.head(f.to(DEV), w.to(DEV), taps, 1 + k)
    got = taps.cpu()
    assert got[0] == SENTINEL and got[-1] == SENTINEL
    got = got[1:-1]
    for k in range(len(fs)):
        if want[k] == 0:
            print(f'head C={C} n_pix={n_pix} case {k}: value {float(got[k])!r}, expected an exact zero')
            assert got[k] == 0
        else:
            e = abs(float(got[k]) - float(want[k])) / abs(float(want[k]))
            print(f'head C={C} n_pix={n_pix} case {k}: value {float(want[k]):.6e}  product {e:.3e}  torch fp32 CPU (largest) {e_cpu:.3e}  bound {bound:.3e}')
            assert e <= bound
    assert torch.isfinite(got).all()
    # total: added in fp64, each value rounded once
    n = min(5, len(fs))
    out = lpips.total(taps[1:1 + n].contiguous()).cpu()
    acc = 0.0
    for v in got[:n].tolist():
        acc += v
    assert out.shape == (1 + n,) and out[0] == torch.tensor(acc, dtype=torch.float64).float() and torch.equal(out[1:], got[:n].float())


# ---- 3. the module ----------------------------------------------------------------------------------------------------------------
SIZES = [(16, 16), (17, 23), (37, 51), (64, 96)]


def _pairs(H, W):
    g = torch.Generator().manual_seed(H * 1000 + W)
    a = torch.rand([6, 3, H, W], generator=g)
    near = (a[:3] + 0.1 * torch.randn([3, 3, H, W], generator=g)).clamp(0, 1)
    return a, torch.cat([near, torch.rand([3, 3, H, W], generator=g)])


@functools.lru_cache(None)
def _reference(H, W):
    """normalize -> (inputs a, b; fp64 and fp32 results of the checker): computed once per size."""
    a, b = _pairs(H, W)
    out = {}
    for normalize in (True, False):
        x0, x1 = (a, b) if normalize else (2 * a - 1, 2 * b - 1)
        out[normalize] = (x0, x1, LO.evaluate(_sd(), x0, x1, normalize, torch.float64), LO.evaluate(_sd(), x0, x1, normalize, torch.float32))
    return out


@pytest.mark.parametrize('H,W', SIZES)
def test_module_against_the_checker(H, W):
    ref = _reference(H, W)
    m = _module()
    # the bound of a quantity: over all the pairs of this size (both input ranges)
    want_t = [torch.cat([ref[nz][2]['taps'][k] for nz in (True, False)]) for k in range(5)] + [torch.cat([ref[nz][2]['total'] for nz in (True, False)])]
    cpu_t = [torch.cat([ref[nz][3]['taps'][k] for nz in (True, False)]) for k in range(5)] + [torch.cat([ref[nz][3]['total'] for nz in (True, False)])]
    bounds = [_scalar_bound(c, w) for c, w in zip(cpu_t, want_t)]
    worst = [0.0] * 6
    for normalize in (True, False):
        x0, x1, want, _ = ref[normalize]
        for p in range(6):
            a, b = x0[p].to(DEV), x1[p].to(DEV)
            val, per = m(a, b, retPerLayer=True, normalize=normalize)
            assert val.shape == (1, 1, 1, 1) and val.dtype == torch.float32 and len(per) == 5 and all(t.shape == (1, 1, 1, 1) for t in per)
            plain = m(a.unsqueeze(0), b.unsqueeze(0), normalize=normalize)
            assert torch.equal(plain, val)
            got = [float(t) for t in per] + [float(val)]
            ws = [float(want['taps'][k][p]) for k in range(5)] + [float(want['total'][p])]
            for q in range(6):
                e = abs(got[q] - ws[q]) / abs(ws[q])
                worst[q] = max(worst[q], e)
                print(f'{H}x{W} normalize={normalize} pair {p} {"tap %d" % q if q < 5 else "total"}: value {ws[q]:.6e}  product {e:.3e}  '
                      f'torch fp32 CPU (largest of the size) {bounds[q][1]:.3e}  bound {bounds[q][0]:.3e}')
    for q in range(6):
        assert worst[q] <= bounds[q][0], (q, worst[q], bounds[q])


# ---- 4. properties ----------------------------------------------------------------------------------------------------------------
def test_properties():
    m = _module()
    g = torch.Generator().manual_seed(5)
    H, W = 37, 51
    a, b = torch.rand([3, H, W], generator=g).to(DEV), torch.rand([3, H, W], generator=g).to(DEV)
    v1, p1 = m(a, b, retPerLayer=True, normalize=True)
    v2, p2 = m(a, b, retPerLayer=True, normalize=True)
    assert torch.equal(v1, v2) and all(torch.equal(x, y) for x, y in zip(p1, p2)), 'two calls differ'
    v3, p3 = m(b, a, retPerLayer=True, normalize=True)
    assert torch.equal(v1, v3) and all(torch.equal(x, y) for x, y in zip(p1, p3)), 'lpips(a, b) != lpips(b, a)'
    v0, p0 = m(a, a, retPerLayer=True, normalize=True)
    assert float(v0) == 0.0 and all(float(x) == 0.0 for x in p0)
    assert float(v1) > 0


def test_frame_lpips_layouts_clamp_and_rgb_lpips():
    utils.load_lpips_weights(_sd())
    g = torch.Generator().manual_seed(6)
    H, W = 33, 47
    pred = torch.rand([H, W, 3], generator=g) * 1.4 - 0.2                  # leaves [0, 1]: the clamp matters
    gt = torch.rand([H, W, 3], generator=g)
    pd, gd = pred.to(DEV), gt.to(DEV)
    v = utils.frame_lpips(pd, gd)
    assert v.shape == () and v.is_cuda and v.dtype == torch.float32
    planar = utils.frame_lpips(pd.permute(2, 0, 1).contiguous(), gd.permute(2, 0, 1).contiguous())
    four = utils.frame_lpips(pd.permute(2, 0, 1).contiguous().unsqueeze(0), gd)
    view = utils.frame_lpips(pd.permute(2, 0, 1).unsqueeze(0), gd)            # the decoder's [1,3,H,W] view of an NHWC result
    assert torch.equal(v, planar) and torch.equal(v, four) and torch.equal(v, view)
    c = utils.frame_lpips(pd, gd, clamp_pred=True)
    assert torch.equal(c, utils.frame_lpips(pd.clamp(0, 1), gd)) and not torch.equal(c, v)
    host = utils.rgb_lpips(gt.numpy(), pred.clamp(0, 1).numpy(), 'vgg', DEV)
    assert isinstance(host, float) and host == float(c)
    want = float(_module()(gd.permute(2, 0, 1).contiguous(), pd.clamp(0, 1).permute(2, 0, 1).contiguous(), normalize=True))
    assert host == want
    utils.load_lpips_weights(None)
    with pytest.raises(NotImplementedError, match='load_lpips_weights'):
        utils.frame_lpips(pd, gd)


@pytest.mark.parametrize('H,W', [(15, 40), (40, 15)])
def test_small_frames_are_refused(H, W):
    a = torch.rand([3, H, W], device=DEV)
    with pytest.raises(N.K4Error, match='K4_ERR_UNSUPPORTED'):
        _module()(a, a)
    assert N.lib().k4_lpips_check_frame(16, 16) == 0 and N.lib().k4_lpips_check_frame(H, W) == N.K4_ERR_UNSUPPORTED
    assert N.lib().k4_lpips_check_frame(8192, 8192) == N.K4_ERR_UNSUPPORTED          # 2 * H * W > 2^26: refused, never wrapped


def test_other_inputs_are_refused():
    m = _module()
    a = torch.rand([3, 32, 32], device=DEV)
    for bad in (a.double(), a.half(), a[:2], a.unsqueeze(0).repeat(2, 1, 1, 1), a.cpu()):
        with pytest.raises(N.K4Error):
            m(bad, bad)
    with pytest.raises(N.K4Error):
        m(a, a[:, :16])
    with pytest.raises(N.K4Error):
        lpips.LPIPS(net='vgg', verbose=False).to(DEV)(a, a)                  # never loaded
    x = a.clone().requires_grad_(True)
    assert not m(x, a).requires_grad                                         # an evaluation metric: no gradient is recorded


# ---- 5. render_viewpoints ---------------------------------------------------------------------------------------------------------
def test_render_viewpoints_eval_lpips_vgg(capsys):
    ck = scene.make_llff_checkpoint(seed=11, num_voxels=48 * 48 * 32, mpi_depth=32)
    H, W = 44, 60
    K = scene.LLFF_K.copy()
    K[:2] *= W / scene.LLFF_HW[1]
    model = utils.model_from_checkpoint_dict(ck).cuda().eval()
    poses = scene.llff_spiral_poses()[[2, 9]]
    rk = dict(ck['render_kwargs'], bg=1.5, render_depth=True)            # bg > 1: marched colours leave [0, 1], the clamp matters
    HW, Ks = np.array([[H, W], [H, W]]), np.stack([K, K])
    plain = render.render_viewpoints(model, poses, HW, Ks, True, rk)
    rng = np.random.default_rng(3)
    gt = [np.clip(f + 0.05 * rng.standard_normal(f.shape).astype(np.float32), 0, 1).astype(np.float32) for f in plain[0]]
    base = render.render_viewpoints(model, poses, HW, Ks, True, rk, gt_imgs=gt)
    with pytest.raises(NotImplementedError, match='lpips'):
        render.render_viewpoints(model, poses, HW, Ks, True, rk, gt_imgs=gt, eval_lpips_vgg=True)
    utils.load_lpips_weights(_sd())
    capsys.readouterr()
    got = render.render_viewpoints(model, poses, HW, Ks, True, rk, gt_imgs=gt, eval_lpips_vgg=True, eval_ssim=True)
    out = capsys.readouterr().out
    for x, y in zip(got, base):
        if isinstance(x, list):
            assert len(x) == len(y) and all(np.array_equal(np.asarray(u.cpu() if torch.is_tensor(u) else u), np.asarray(v.cpu() if torch.is_tensor(v) else v))
                                            for u, v in zip(x, y))
        else:
            assert np.array_equal(x, y)
    m = re.search(r'^Testing lpips \(vgg\) (\S+) \(avg\)$', out, re.M)
    assert m and re.search(r'^Testing ssim (\S+) \(avg\)$', out, re.M), out
    want = np.mean([float(utils.frame_lpips(torch.from_numpy(got[0][i]).to(DEV), torch.from_numpy(gt[i]).to(DEV))) for i in range(2)])
    print('render_viewpoints lpips (vgg)', float(m.group(1)), 'frame_lpips over the returned frames', want)
    assert float(m.group(1)) == want and want > 0
    # no ground truth: nothing is scored and nothing printed (run_sr.py:143)
    capsys.readouterr()
    render.render_viewpoints(model, poses[:1], HW[:1], Ks[:1], True, rk, eval_lpips_vgg=True)
    assert 'lpips' not in capsys.readouterr().out.replace('init_lpips', '')


# ---- 6. what the perceptual loss uses is unchanged --------------------------------------------------------------------------------
# sha256 of (y, y_pre, y_pool) of sr_loss.conv3x3 with tap and pool, computed by regression_hashes() on the commit in front of the ragged sizes
PARENT_HASHES = {
    '64->64 64x64': 'e114ed8e35b519aa9ea14c2912a89ebdcac2f7847e4ee789a44c5df6d5d1405b',
    '128->128 32x32': '3145e3f61049bd08610034e0400ee4db49f30c1bd50563fed73d36c7f07418b9',
    '256->256 16x16': '1e4e3c2202cb576b18f0ce9f1153a4ee9a395c2b0dff71428539e76adf8be99d',
    '512->512 8x8': '700ce398a70f00c00e9a433e20aa650dc2a703de2ffe47d178a532266e76ab5f',
    '512->512 4x4': '0f5da9a46ea72cf9c12779ac5802294a3852947dda2186d489f8436e94ef9ded',
    '64->64 96x160': 'ea0b2566f9f83746803ffeadc7dbfa8d90261485bcba3dd71a7208b080af00d3',
    '128->128 48x80': 'f2fb0f212c6a3205742a0e5180cc88af4aff893e45b7d7657c361d9026a42e36',
    '256->256 24x40': 'd096bf7649219d6fdf52bbed6a2c52a6f71b8327f431e64ec66d8a3082eefef4',
    '512->512 12x20': '469d501bfb6c80b1e2d9ec7b70c66c4e1f2bbc21987e2359b784caf2a31dad68',
    '512->512 6x10': 'fec6f805f81f2a62e5853cd2ee724b6620fd3280df0b9ae9d35f6b4a48741b76',
}


def regression_hashes():
    sd = sr_loss.seeded_vgg19_state_dict(7)
    out = {}
    for H, W in ((64, 64), (96, 160)):
        g = torch.Generator().manual_seed(H * 1000 + W + 9)
        for idx, C, d in ((2, 64, 1), (7, 128, 2), (12, 256, 4), (21, 512, 8), (30, 512, 16)):
            h, w = H // d, W // d
            wt, b = sd[f'features.{idx}.weight'], sd[f'features.{idx}.bias']
            x = torch.relu(torch.randn([2, h, w, C], generator=g)).to(DEV)
            y, pre, yp = sr_loss.conv3x3(x, sr_loss.pack_weight(wt.to(DEV), sr_loss.FWD), b.to(DEV), C, relu=True, keep_relu=True, keep_pre=True, pool=True)
            hsh = hashlib.sha256()
            for t in (y, pre, yp):
                hsh.update(t.cpu().numpy().tobytes())
            out[f'{C}->{C} {h}x{w}'] = hsh.hexdigest()
    return out


def test_even_sizes_keep_their_bits():
    got = regression_hashes()
    assert len(PARENT_HASHES) == 10
    for k, v in got.items():
        print(k, v, 'recorded', PARENT_HASHES.get(k))
    assert got == PARENT_HASHES
