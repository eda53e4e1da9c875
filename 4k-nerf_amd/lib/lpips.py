"""LPIPS-VGG frame scoring: ``lpips.LPIPS(net='vgg', version='0.1')`` as the reference's lib/utils.py:137-149 uses it
(run_sr.py:1135-1138, run.py:141, run_sr.py:151), on the VGG kernels of csrc/k4_vgg.hip and the head of csrc/k4_lpips.hip.

The `lpips` package is not part of the reference tree.  What is restated here comes from its published 0.1 source and was not available to compare
against ("Unpinned against its upstream"): a torchvision ``vgg16().features`` cut after relu1_2, relu2_2, relu3_3, relu4_3 and relu5_3;
the scaling layer ``(x - shift) / scale``; per tap ``normalize_tensor`` (``f / (sqrt(sum_c f^2) + 1e-10)``), the squared difference, a bias-free
1x1 convolution to one channel (``NetLinLayer``; its dropout is the identity in eval mode) and the spatial mean; the sum of the five taps.

There is ONE execution path: the kernels, on CUDA float32 frames.  CPU tensors raise ``K4Error``; argument values outside
``net='vgg' / version='0.1' / lpips=True / spatial=False / pnet_tune=False`` raise ``NotImplementedError``.  The constructor never reads a file
and never fetches: ``pretrained`` and ``model_path`` are accepted and IGNORED, the caller loads the weights with ``load_lpips_state_dict`` (or
the module's own keys with ``load_state_dict``), and a module that was never loaded raises ``K4Error`` at its first forward.  The module is an
evaluation metric: it records no gradient.
"""
import torch
import torch.nn as nn

from .. import _native as N
from . import sr_loss

# torchvision.models.vgg16().features: (index of the convolution, cout, cin) per slice; a 2x2 stride-2 max pool (floor mode) opens slices 2..5
_SLICES = (((0, 64, 3), (2, 64, 64)),
           ((5, 128, 64), (7, 128, 128)),
           ((10, 256, 128), (12, 256, 256), (14, 256, 256)),
           ((17, 512, 256), (19, 512, 512), (21, 512, 512)),
           ((24, 512, 512), (26, 512, 512), (28, 512, 512)))
CHNS = (64, 128, 256, 512, 512)
SHIFT, SCALE = (-.030, -.088, -.188), (.458, .448, .450)


def conv_layers():
    """[(slice number 1..5, features index, cout, cin)] in layer order."""
    return [(s, i, cout, cin) for s, layers in enumerate(_SLICES, 1) for i, cout, cin in layers]


def seeded_lpips_state_dict(seed):
    """The module's own keys with seeded values, for tests and tools: the backbone as ``sr_loss.seeded_vgg19_state_dict`` draws it (weights
    N(0, 2 / (9 cin)), biases U(-0.1, 0.1), one ``torch.Generator`` in layer order), then the head weights, non-negative, U(0, 2 / C)."""
    g = torch.Generator().manual_seed(int(seed))
    sd = {}
    for s, i, cout, cin in conv_layers():
        sd[f'net.slice{s}.{i}.weight'] = torch.randn([cout, cin, 3, 3], generator=g) * (2.0 / (9 * cin)) ** 0.5
        sd[f'net.slice{s}.{i}.bias'] = torch.rand([cout], generator=g) * 0.2 - 0.1
    for k, c in enumerate(CHNS):
        sd[f'lin{k}.model.1.weight'] = torch.rand([1, c, 1, 1], generator=g) * (2.0 / c)
    sd['scaling_layer.shift'] = torch.tensor(SHIFT).view(1, 3, 1, 1)
    sd['scaling_layer.scale'] = torch.tensor(SCALE).view(1, 3, 1, 1)
    return sd


def head(f, w, taps, slot):
    """k4_lpips_head: f [2, h, w, C] (or [2, n_pix, C]) and w [C] -> taps[slot] (fp64, on the device)."""
    L = N.lib()
    C = f.shape[-1]
    n_pix = f.numel() // (2 * C)
    nb = L.k4_lpips_workspace_bytes(n_pix)
    if nb < 0:
        raise N.K4Error(f'k4_lpips_head: unsupported shape {tuple(f.shape)}')
    ws = torch.empty([nb // 8], dtype=torch.float64, device=f.device)
    N.check(L.k4_lpips_head(N.f32(f), n_pix, C, N.f32(w), N.ptr(ws), N.ptr(taps), slot, N.stream()), 'k4_lpips_head')


def total(taps):
    """k4_lpips_total: taps [n] fp64 -> fp32 [1 + n]: the sum (added in fp64), then each tap."""
    out = torch.empty([1 + taps.numel()], dtype=torch.float32, device=taps.device)
    N.check(N.lib().k4_lpips_total(N.ptr(taps), taps.numel(), N.f32(out), N.stream()), 'k4_lpips_total')
    return out


class _Holder(nn.Module):
    """A parameter holder (as ``sr_loss._Layer``): the kernels evaluate the network."""

    def forward(self, *a, **k):
        raise N.K4Error('a layer of LPIPS is a parameter holder: call the LPIPS module')


class _Conv(_Holder):
    def __init__(self, cout, cin, k, bias):
        super().__init__()
        self.weight = nn.Parameter(torch.zeros(cout, cin, k, k), requires_grad=False)
        if bias:
            self.bias = nn.Parameter(torch.zeros(cout), requires_grad=False)


class _Slice(_Holder):
    def __init__(self, layers):
        super().__init__()
        for i, cout, cin in layers:
            self.add_module(str(i), _Conv(cout, cin, 3, True))


class _Net(_Holder):
    def __init__(self):
        super().__init__()
        for s, layers in enumerate(_SLICES, 1):
            self.add_module(f'slice{s}', _Slice(layers))


class _Lin(_Holder):
    """``NetLinLayer``: ``model = Sequential(Dropout, Conv2d(C, 1, 1, bias=False))`` -- the key is ``model.1.weight``."""

    def __init__(self, c):
        super().__init__()
        self.model = _Holder()
        self.model.add_module('1', _Conv(1, c, 1, False))


class _Scaling(_Holder):
    def __init__(self):
        super().__init__()
        self.register_buffer('shift', torch.tensor(SHIFT).view(1, 3, 1, 1))
        self.register_buffer('scale', torch.tensor(SCALE).view(1, 3, 1, 1))


class LPIPS(nn.Module):
    """``lpips.LPIPS`` with the package's constructor; ``forward(in0, in1, retPerLayer=False, normalize=False)`` -> ``[1, 1, 1, 1]``.
    ``pretrained`` and ``model_path`` are accepted and ignored: nothing is read or fetched (``load_lpips_state_dict``)."""

    def __init__(self, pretrained=True, net='alex', version='0.1', lpips=True, spatial=False, pnet_rand=False, pnet_tune=False, use_dropout=True,
                 model_path=None, eval_mode=True, verbose=True):
        super().__init__()
        if net != 'vgg':
            raise NotImplementedError(f"LPIPS: net={net!r} is not provided (only net='vgg': the alex and squeeze backbones need convolutions and pools "
                                      f'that csrc/k4_vgg.hip does not have, and no training logic of the reference depends on them)')
        for arg, val, want, why in (('version', version, '0.1', 'lib/utils.py:142 asks for it'), ('lpips', lpips, True, 'the linear layers are the metric'),
                                    ('spatial', spatial, False, 'the head reduces over the pixels on the device'),
                                    ('pnet_tune', pnet_tune, False, 'the module records no gradient')):
            if val != want:
                raise NotImplementedError(f'LPIPS: {arg}={val!r} is not provided (only {arg}={want!r}: {why})')
        self.pnet_type, self.version, self.lpips, self.spatial, self.pnet_rand, self.pnet_tune = net, version, lpips, spatial, pnet_rand, pnet_tune
        self.chns, self.L = list(CHNS), len(CHNS)
        self.scaling_layer = _Scaling()
        self.net = _Net()
        for k, c in enumerate(CHNS):
            self.add_module(f'lin{k}', _Lin(c))
        self._loaded, self._packed = False, None
        self.register_load_state_dict_post_hook(LPIPS._after_load)
        if eval_mode:
            self.eval()

    @staticmethod
    def _after_load(module, incompatible):
        if not any(k.startswith('net.') or k.startswith('lin') for k in incompatible.missing_keys):
            module._loaded, module._packed = True, None

    def _params(self):
        convs = [(getattr(getattr(self.net, f'slice{s}'), str(i)), f'net.slice{s}.{i}', i) for s, i, _, _ in conv_layers()]
        lins = [getattr(getattr(self, f'lin{k}').model, '1') for k in range(self.L)]
        return convs, lins

    def load_lpips_state_dict(self, sd, lin_sd=None):
        """Copy the weights from the module's own keys, or the backbone from a torchvision ``vgg16`` state dict (``features.<i>.weight`` / ``.bias``)
        and the heads from ``lin<k>.model.1.weight`` or ``lins.<k>.model.1.weight`` of either dict (the package's weights/v0.1/vgg.pth holds only those).
        A missing layer raises ``KeyError``, a wrong shape ``ValueError``."""
        convs, lins = self._params()
        both = (sd,) if lin_sd is None else (sd, lin_sd)
        plan = []
        for m, own, i in convs:
            for part in ('weight', 'bias'):
                keys = (f'{own}.{part}', f'features.{i}.{part}')
                src = next((sd[k] for k in keys if k in sd), None)
                if src is None:
                    raise KeyError(f'load_lpips_state_dict: no {keys[0]} / {keys[1]} in the state dict')
                plan.append((f'{own}.{part}', getattr(m, part), src))
        for k, m in enumerate(lins):
            keys = (f'lin{k}.model.1.weight', f'lins.{k}.model.1.weight')
            src = next((d[key] for d in both for key in keys if key in d), None)
            if src is None:
                raise KeyError(f'load_lpips_state_dict: no {keys[0]} / {keys[1]} in the state dict(s)')
            plan.append((keys[0], m.weight, src))
        for name, dst, src in plan:
            if tuple(src.shape) != tuple(dst.shape):
                raise ValueError(f'load_lpips_state_dict: {name} has shape {tuple(src.shape)}, expected {tuple(dst.shape)}')
        with torch.no_grad():
            for _, dst, src in plan:
                dst.copy_(src)
            for name in ('shift', 'scale'):
                if f'scaling_layer.{name}' in sd:
                    getattr(self.scaling_layer, name).copy_(sd[f'scaling_layer.{name}'].reshape(1, 3, 1, 1))
        self._loaded, self._packed = True, None
        return self

    def k4_operands(self, device):
        """The packed operands on `device`, built once per weight load (the weights are constant)."""
        if not self._loaded:
            raise N.K4Error('LPIPS: the weights were never loaded (load_lpips_state_dict(...); the constructor reads and fetches nothing)')
        convs, lins = self._params()
        sl = self.scaling_layer
        tensors = [m.weight for m, _, _ in convs] + [m.weight for m in lins] + [sl.shift, sl.scale]
        key = (str(device), tuple((t.data_ptr(), t._version) for t in tensors))
        if self._packed is None or self._packed['key'] != key:
            for t in tensors + [m.bias for m, _, _ in convs]:
                if not (t.is_cuda and t.device == device and t.dtype == torch.float32 and t.is_contiguous()):
                    raise N.K4Error(f'LPIPS: parameters must be contiguous CUDA float32 tensors on the frames\' device {device} (no CPU path exists)')
            ops = [{'w': m.weight.detach(), 'b': m.bias.detach(), 'fwd': None if i == 0 else sr_loss.pack_weight(m.weight.detach(), sr_loss.FWD)} for m, _, i in convs]
            shift, scale = sl.shift.detach().reshape(3), sl.scale.detach().reshape(3)
            # normalize=True is 2x - 1 in front of the scaling layer: ((2x - 1) - shift) / scale == (x - (1 + shift) / 2) / (scale / 2)
            self._packed = {'key': key, 'ops': ops, 'lin': [m.weight.detach().reshape(-1).contiguous() for m in lins],
                            'norm': {False: (shift.contiguous(), scale.contiguous()), True: (((1 + shift) / 2).contiguous(), (scale / 2).contiguous())}}
        return self._packed

    @staticmethod
    def _image(x, what):
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise N.K4Error(f'{what}: tensor must be on the GPU (no CPU path exists for LPIPS)')
        if x.dim() == 4 and x.shape[0] == 1:
            x = x[0]
        if x.dtype != torch.float32 or x.dim() != 3 or x.shape[0] != 3:
            raise N.K4Error(f'{what}: expected one planar float32 image [3, H, W] or [1, 3, H, W], got {x.dtype} {tuple(x.shape)}')
        return x.detach().contiguous()

    @torch.no_grad()
    def forward(self, in0, in1, retPerLayer=False, normalize=False):
        x0, x1 = self._image(in0, 'LPIPS(in0)'), self._image(in1, 'LPIPS(in1)')
        if x0.shape != x1.shape:
            raise N.K4Error(f'LPIPS: in0 {tuple(x0.shape)} and in1 {tuple(x1.shape)} differ in shape')
        if x0.device != x1.device:
            raise N.K4Error(f'LPIPS: the images are on different devices: {x0.device}, {x1.device}')
        H, W = int(x0.shape[1]), int(x0.shape[2])
        with torch.cuda.device(x0.device):
            P = self.k4_operands(x0.device)
            N.check(N.lib().k4_lpips_check_frame(H, W), f'LPIPS on a {H}x{W} frame (H and W must be at least 16)')
            mean, std = P['norm'][bool(normalize)]
            ops, layer = P['ops'], 0
            taps = torch.empty([self.L], dtype=torch.float64, device=x0.device)
            cur = None
            for s, layers in enumerate(_SLICES):
                for j, (_, cout, _) in enumerate(layers):
                    op = ops[layer]
                    layer += 1
                    last = j == len(layers) - 1
                    if op['fwd'] is None:
                        cur, _ = sr_loss.conv1_1(x0, x1, mean, std, op['w'], op['b'], keep_relu=True, keep_pre=False)
                    else:                                           # the level's last layer writes the next level's input beside the tapped image
                        y, _, yp = sr_loss.conv3x3(cur, op['fwd'], op['b'], cout, relu=True, keep_relu=True, keep_pre=False, pool=last and s + 1 < self.L)
                        cur = y
                head(cur, P['lin'][s], taps, s)
                cur = yp                                            # the level's activations are released here
            out = total(taps)
        val = out[0].reshape(1, 1, 1, 1)
        if retPerLayer:
            return val, [out[1 + k].reshape(1, 1, 1, 1) for k in range(self.L)]
        return val
