"""CPU-side checks of LPIPS-VGG (4k-nerf_amd/lib/lpips.py, lib/utils.py rgb_lpips / frame_lpips; the kernels: tests/test_lpips_gpu.py): the checker the
GPU tests lean on (tests/lpips_oracle.py) against an independently built nn.Sequential VGG16 + NetLinLayer modules written the way the `lpips` package
writes them, the module tree and its keys, the loaders and their errors, and that there is no CPU path and nothing is fetched."""
import inspect

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import nerf4k_amd  # noqa: F401
from nerf4k_amd import _native as N, render
from nerf4k_amd.lib import lpips, utils
import lpips_oracle as LO

SEED = 11
CFG16 = [64, 64, 'M', 128, 128, 'M', 256, 256, 256, 'M', 512, 512, 512, 'M', 512, 512, 512, 'M']


@pytest.fixture(scope='module')
def sd():
    return lpips.seeded_lpips_state_dict(SEED)


@pytest.fixture(autouse=True)
def _clear_registered_weights():
    yield
    utils.load_lpips_weights(None)


# ---- the package's way of writing it, built independently of lib/lpips.py and of the checker ----------------------------------------
def _vgg16_features():
    layers, cin = [], 3
    for v in CFG16:
        if v == 'M':
            layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
        else:
            layers += [nn.Conv2d(cin, v, kernel_size=3, padding=1), nn.ReLU(inplace=False)]
            cin = v
    return nn.Sequential(*layers)


class _NetLinLayer(nn.Module):
    def __init__(self, chn_in, chn_out=1, use_dropout=True):
        super().__init__()
        layers = [nn.Dropout()] if use_dropout else []
        layers += [nn.Conv2d(chn_in, chn_out, 1, stride=1, padding=0, bias=False)]
        self.model = nn.Sequential(*layers)

    def forward(self, x):
        return self.model(x)


def _normalize_tensor(in_feat, eps=1e-10):
    norm_factor = torch.sqrt(torch.sum(in_feat ** 2, dim=1, keepdim=True))
    return in_feat / (norm_factor + eps)


def _spatial_average(in_tens, keepdim=True):
    return in_tens.mean([2, 3], keepdim=keepdim)


class _PackageStyle(nn.Module):
    def __init__(self):
        super().__init__()
        feats = _vgg16_features()
        cuts = (0, 4, 9, 16, 23, 30)
        self.slices = nn.ModuleList([nn.Sequential(*[feats[i] for i in range(cuts[k], cuts[k + 1])]) for k in range(5)])
        self.features = feats
        self.register_buffer('shift', torch.Tensor([-.030, -.088, -.188])[None, :, None, None])
        self.register_buffer('scale', torch.Tensor([.458, .448, .450])[None, :, None, None])
        self.lins = nn.ModuleList([_NetLinLayer(c) for c in (64, 128, 256, 512, 512)])

    def forward(self, in0, in1, normalize=False):
        if normalize:
            in0, in1 = 2 * in0 - 1, 2 * in1 - 1
        h0, h1 = (in0 - self.shift) / self.scale, (in1 - self.shift) / self.scale
        res = []
        for k in range(5):
            h0, h1 = self.slices[k](h0), self.slices[k](h1)
            diff = (_normalize_tensor(h0) - _normalize_tensor(h1)) ** 2
            res.append(_spatial_average(self.lins[k](diff), keepdim=True))
        val = res[0]
        for k in range(1, 5):
            val = val + res[k]
        return val, res


def _torchvision_sd(sd):
    tv = {}
    for s, i, _, _ in lpips.conv_layers():
        for part in ('weight', 'bias'):
            tv[f'features.{i}.{part}'] = sd[f'net.slice{s}.{i}.{part}']
    return tv


def _lin_sd(sd, prefix):
    return {(f'lin{k}' if prefix == 'lin' else f'lins.{k}') + '.model.1.weight': sd[f'lin{k}.model.1.weight'] for k in range(5)}


def test_checker_against_the_package_style_modules(sd):
    ref = _PackageStyle().double().eval()
    ref.features.load_state_dict({k[len('features.'):]: v.double() for k, v in _torchvision_sd(sd).items()})
    ref.lins.load_state_dict({k[len('lins.'):]: v.double() for k, v in _lin_sd(sd, 'lins').items()})
    g = torch.Generator().manual_seed(3)
    for H, W in ((16, 16), (37, 51)):
        a = torch.rand([2, 3, H, W], generator=g)
        b = torch.stack([(a[0] + 0.1 * torch.randn([3, H, W], generator=g)).clamp(0, 1), torch.rand([3, H, W], generator=g)])
        for normalize in (False, True):
            got = LO.evaluate(sd, a, b, normalize, torch.float64)
            for p in range(2):
                with torch.no_grad():
                    val, res = ref(a[p:p + 1].double(), b[p:p + 1].double(), normalize=normalize)
                assert val.shape == (1, 1, 1, 1)
                errs = [abs(float(got['taps'][k][p]) - float(res[k])) / abs(float(res[k])) for k in range(5)]
                e = abs(float(got['total'][p]) - float(val)) / abs(float(val))
                print(f'{H}x{W} normalize={normalize} pair {p}: value {float(val):.6f}, checker against package style: total {e:.2e} taps {max(errs):.2e}  bound 1e-12')
                assert e <= 1e-12 and max(errs) <= 1e-12
            # the folded normalisation the kernel applies in its load is the same image (fp64: to rounding)
            fold = LO.evaluate(sd, a, b, normalize, torch.float64, folded=True)
            e = float(((fold['total'] - got['total']).abs() / got['total'].abs()).max())
            x_err = float((LO.scale_input_folded(sd, a, normalize, torch.float64) - LO.scale_input(sd, a, normalize, torch.float64)).abs().max())
            print(f'{H}x{W} normalize={normalize}: folded mean / std against 2x - 1 and the scaling layer: image {x_err:.2e} value {e:.2e}  bounds 1e-14, 1e-11')
            assert x_err <= 1e-14 and e <= 1e-11


def test_normalize_is_the_normalisation_of_sr_loss():
    from nerf4k_amd.lib import sr_loss
    shift, scale = torch.tensor(lpips.SHIFT, dtype=torch.float64), torch.tensor(lpips.SCALE, dtype=torch.float64)
    assert torch.allclose((1 + shift) / 2, torch.tensor(sr_loss.MEAN, dtype=torch.float64), rtol=0, atol=1e-12)
    assert torch.allclose(scale / 2, torch.tensor(sr_loss.STD, dtype=torch.float64), rtol=0, atol=1e-12)


def test_state_dict_keys_and_shapes(sd):
    m = lpips.LPIPS(net='vgg')
    own = m.state_dict()
    want = {}
    cin = 3
    for s, idx in enumerate(((0, 2), (5, 7), (10, 12, 14), (17, 19, 21), (24, 26, 28)), 1):
        for i in idx:
            cout = (64, 128, 256, 512, 512)[s - 1]
            want[f'net.slice{s}.{i}.weight'], want[f'net.slice{s}.{i}.bias'] = (cout, cin, 3, 3), (cout,)
            cin = cout
    for k, c in enumerate((64, 128, 256, 512, 512)):
        want[f'lin{k}.model.1.weight'] = (1, c, 1, 1)
    want['scaling_layer.shift'] = want['scaling_layer.scale'] = (1, 3, 1, 1)
    assert {k: tuple(v.shape) for k, v in own.items()} == want
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    assert own['scaling_layer.shift'].flatten().tolist() == pytest.approx([-.030, -.088, -.188], abs=1e-7)
    assert own['scaling_layer.scale'].flatten().tolist() == pytest.approx([.458, .448, .450], abs=1e-7)
    assert not any(p.requires_grad for p in m.parameters()) and not m.training
    for k in range(5):
        assert float(sd[f'lin{k}.model.1.weight'].min()) >= 0 and float(sd[f'lin{k}.model.1.weight'].max()) <= 2.0 / want[f'lin{k}.model.1.weight'][1]


def test_load_from_own_keys_torchvision_keys_and_either_lin_form(sd):
    def same(m):
        return all(torch.equal(v, sd[k]) for k, v in m.state_dict().items())
    assert same(lpips.LPIPS(net='vgg').load_lpips_state_dict(sd))
    m = lpips.LPIPS(net='vgg')
    m.load_state_dict(sd)
    assert same(m) and m._loaded
    tv = _torchvision_sd(sd)
    assert same(lpips.LPIPS(net='vgg').load_lpips_state_dict(tv, _lin_sd(sd, 'lin')))
    assert same(lpips.LPIPS(net='vgg').load_lpips_state_dict(tv, _lin_sd(sd, 'lins')))
    assert same(lpips.LPIPS(net='vgg').load_lpips_state_dict({**tv, **_lin_sd(sd, 'lins')}))
    with pytest.raises(KeyError):
        lpips.LPIPS(net='vgg').load_lpips_state_dict(tv)                                     # no heads
    with pytest.raises(KeyError):
        lpips.LPIPS(net='vgg').load_lpips_state_dict({k: v for k, v in sd.items() if k != 'net.slice3.12.bias'})
    with pytest.raises(KeyError):
        lpips.LPIPS(net='vgg').load_lpips_state_dict(_lin_sd(sd, 'lin'))                     # no backbone
    bad = dict(sd)
    bad['lin2.model.1.weight'] = torch.zeros(1, 128, 1, 1)
    with pytest.raises(ValueError):
        lpips.LPIPS(net='vgg').load_lpips_state_dict(bad)
    bad = dict(tv)
    bad['features.5.weight'] = torch.zeros(128, 64, 1, 1)
    with pytest.raises(ValueError):
        lpips.LPIPS(net='vgg').load_lpips_state_dict(bad, _lin_sd(sd, 'lin'))
    m = lpips.LPIPS(net='vgg')                                                               # a failed load leaves the module unloaded
    with pytest.raises(ValueError):
        m.load_lpips_state_dict(bad, _lin_sd(sd, 'lin'))
    assert not m._loaded


def test_constructor_signature_and_rejections():
    sig = inspect.signature(lpips.LPIPS.__init__)
    assert list(sig.parameters)[1:] == ['pretrained', 'net', 'version', 'lpips', 'spatial', 'pnet_rand', 'pnet_tune', 'use_dropout', 'model_path',
                                        'eval_mode', 'verbose']
    assert [p.default for p in list(sig.parameters.values())[1:]] == [True, 'alex', '0.1', True, False, False, False, True, None, True, True]
    assert list(inspect.signature(lpips.LPIPS.forward).parameters)[1:] == ['in0', 'in1', 'retPerLayer', 'normalize']
    for kw in ({}, {'net': 'alex'}, {'net': 'squeeze'}, {'net': 'vgg', 'version': '0.0'}, {'net': 'vgg', 'lpips': False}, {'net': 'vgg', 'spatial': True},
               {'net': 'vgg', 'pnet_tune': True}):
        with pytest.raises(NotImplementedError):
            lpips.LPIPS(**kw)
    lpips.LPIPS(net='vgg', pretrained=True, model_path='/nonexistent/vgg.pth', verbose=False)          # accepted and ignored: nothing is read


def test_no_cpu_path_and_unloaded_module_raises(sd):
    m = lpips.LPIPS(net='vgg').load_lpips_state_dict(sd)
    a = torch.rand(3, 32, 32)
    with pytest.raises(N.K4Error):
        m(a, a)
    with pytest.raises(N.K4Error):
        m(a.unsqueeze(0), a.unsqueeze(0), normalize=True)
    with pytest.raises(N.K4Error):                      # holders do not evaluate anything
        m.net.slice1(a.unsqueeze(0))
    with pytest.raises(N.K4Error):
        m.lin0(torch.zeros(1, 64, 4, 4))
    with pytest.raises(N.K4Error):
        getattr(m.net.slice1, '0')(a.unsqueeze(0))
    with pytest.raises(N.K4Error):
        utils.frame_lpips(torch.rand(32, 32, 3), torch.rand(32, 32, 3))
    with pytest.raises(N.K4Error):                      # never loaded: raises at the first forward, whatever the device
        lpips.LPIPS(net='vgg').k4_operands(torch.device('cpu'))


def test_rgb_lpips_and_render_viewpoints_raise_without_weights_and_alex_always(sd, tmp_path):
    a = np.zeros((32, 32, 3), np.float32)
    assert not utils.lpips_weights_registered()
    with pytest.raises(NotImplementedError, match='lpips'):
        utils.rgb_lpips(a, a, 'alex', 'cpu')
    with pytest.raises(NotImplementedError, match='load_lpips_weights') as e:
        utils.rgb_lpips(a, a, 'vgg', 'cpu')
    assert 'lpips' in str(e.value)
    for kw in ({'eval_lpips_vgg': True}, {'eval_lpips_alex': True}):
        with pytest.raises(NotImplementedError, match='lpips'):
            render.render_viewpoints(None, [], [], [], True, {}, **kw)
    # registered: every accepted form; vgg no longer raises on entry (no frames: the empty return), alex still does
    path = tmp_path / 'lpips_vgg.pth'
    torch.save(sd, str(path))
    for obj in (sd, (_torchvision_sd(sd), _lin_sd(sd, 'lins')), str(path)):
        utils.load_lpips_weights(obj)
        assert utils.lpips_weights_registered() and not utils.__LPIPS__
        out = render.render_viewpoints(None, [], [], [], True, {}, eval_lpips_vgg=True)
        assert len(out) == 6 and len(out[0]) == 0
        with pytest.raises(NotImplementedError, match='lpips'):
            render.render_viewpoints(None, [], [], [], True, {}, eval_lpips_alex=True)
        with pytest.raises(NotImplementedError, match='lpips'):
            utils.rgb_lpips(a, a, 'alex', 'cpu')
        with pytest.raises(N.K4Error):                  # registered, but there is no CPU path
            utils.rgb_lpips(a, a, 'vgg', 'cpu')
        utils.load_lpips_weights(None)
        assert not utils.lpips_weights_registered() and not utils.__LPIPS__
        with pytest.raises(NotImplementedError, match='lpips'):
            render.render_viewpoints(None, [], [], [], True, {}, eval_lpips_vgg=True)
    with pytest.raises(KeyError):
        utils.load_lpips_weights(_torchvision_sd(sd))
    assert not utils.lpips_weights_registered()


def test_signatures_are_the_reference_signatures():
    assert list(inspect.signature(utils.init_lpips).parameters) == ['net_name', 'device']
    assert list(inspect.signature(utils.rgb_lpips).parameters) == ['np_gt', 'np_im', 'net_name', 'device']
    assert list(inspect.signature(utils.frame_lpips).parameters) == ['pred', 'gt', 'clamp_pred']
    assert isinstance(utils.__LPIPS__, dict)
