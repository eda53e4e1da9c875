"""The perceptual and style terms of the "+gan" joint recipes: a frozen VGG19 feature extractor and the L1 / Gram losses on its features.

Restates ``basicsr.losses.PerceptualLoss`` and ``basicsr.archs.vgg_arch.VGGFeatureExtractor``, which the reference's run_sr.py:18 imports and
run_sr.py:670-678, 934-945 uses.  basicsr is not part of the reference tree; the loss formulas are the ones the reference's own
lib/sr_loss.py:123-188 repeats (``NNFMLoss.forward`` :134-161: ``sum_k criterion(f_k(x), f_k(gt)) * w_k`` times the term's weight;
``_gram_mat`` :175-188: ``f f^T / (c h w)``).  The layer naming, the normalisation constants, the taps in front of the ReLU and the 2x2
stride-2 max pooling come from the published basicsr 1.4 source and were not available to compare against.

There is ONE execution path: the kernels of csrc/k4_vgg.hip on CUDA fp32 tensors.  CPU tensors raise ``K4Error``; argument values outside
``vgg19 / criterion='l1' / range_norm=False / requires_grad=False / pooling kept`` raise ``NotImplementedError``.  The constructor never
fetches weights: the caller loads a torchvision ``vgg19`` state dict with ``load_vgg_state_dict`` (or the module's own keys with
``load_state_dict``), and a module that was never loaded raises at its first forward.

Module attributes (A/B, tests): ``_KEEP_RECORD`` -- ``PerceptualLoss.k4_record`` receives the decisions of the last forward (ReLU masks,
pool choices, signs of the feature and Gram differences) for tests/vgg_oracle.grad_with_record.
"""
import torch
import torch.nn as nn

from .. import _native as N

_KEEP_RECORD = False

# torchvision.models.vgg19().features: widths per block, 'M' = MaxPool2d(2, 2)
_BLOCKS = ((64, 64), (128, 128), (256, 256, 256, 256), (512, 512, 512, 512), (512, 512, 512, 512))
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
FWD, DGRAD = 0, 1


def vgg19_layer_names():
    """``conv1_1, relu1_1, conv1_2, relu1_2, pool1, conv2_1, ...`` in the order of torchvision's ``vgg19().features`` (37 entries)."""
    names = []
    for b, widths in enumerate(_BLOCKS, 1):
        for j in range(1, len(widths) + 1):
            names += [f'conv{b}_{j}', f'relu{b}_{j}']
        names.append(f'pool{b}')
    return names


NAMES = vgg19_layer_names()


def _conv_shapes():
    out, cin = {}, 3
    for b, widths in enumerate(_BLOCKS, 1):
        for j, c in enumerate(widths, 1):
            out[f'conv{b}_{j}'] = (c, cin)
            cin = c
    return out


CONV_SHAPES = _conv_shapes()          # name -> (cout, cin)


def seeded_vgg19_state_dict(seed):
    """A torchvision-keyed ``vgg19`` state dict (``features.<i>.weight`` / ``.bias``) of seeded values for tests and tools: weights N(0, 2 / (9 cin)),
    biases U(-0.1, 0.1), drawn from one ``torch.Generator`` in layer order."""
    g = torch.Generator().manual_seed(int(seed))
    sd = {}
    for i, name in enumerate(NAMES):
        if name.startswith('conv'):
            cout, cin = CONV_SHAPES[name]
            sd[f'features.{i}.weight'] = torch.randn([cout, cin, 3, 3], generator=g) * (2.0 / (9 * cin)) ** 0.5
            sd[f'features.{i}.bias'] = torch.rand([cout], generator=g) * 0.2 - 0.1
    return sd


# ---- the entry points of csrc/k4_vgg.hip ------------------------------------------------------------------------------------------

def pack_weight(w, form):
    """k4_vgg_pack_weight: w [cout, cin, k, k] -> the packed operand (FWD) or the input-gradient operand (DGRAD)."""
    L = N.lib()
    cout, cin, k, _ = w.shape
    outs, ins = (cout, cin) if form == FWD else (cin, cout)
    nb = L.k4_vgg_weight_bytes(outs, ins, k)
    if nb < 0:
        raise N.K4Error(f'k4_vgg_pack_weight: unsupported shape {tuple(w.shape)}')
    out = torch.empty([nb // 2], dtype=torch.int16, device=w.device)
    N.check(L.k4_vgg_pack_weight(N.f32(w), cout, cin, k, form, N.ptr(out), N.stream()), 'k4_vgg_pack_weight')
    return out


def conv3x3(x, w_split, bias, cout, relu=True, keep_relu=True, keep_pre=False, pool=False, ksize=3):
    """k4_vgg_conv3x3 forward on x [B, H, W, cin]: (y or None, y_pre or None, y_pool or None)."""
    B, H, W, cin = x.shape
    dev = x.device
    y = torch.empty([B, H, W, cout], dtype=torch.float32, device=dev) if keep_relu else None
    pre = torch.empty([B, H, W, cout], dtype=torch.float32, device=dev) if keep_pre else None
    yp = torch.empty([B, H // 2, W // 2, cout], dtype=torch.float32, device=dev) if pool else None
    N.check(N.lib().k4_vgg_conv3x3(N.f32(x), cin, H, W, B, N.ptr(w_split), ksize, None if bias is None else N.f32(bias),
                                   None if y is None else N.f32(y), None if pre is None else N.f32(pre), None if yp is None else N.f32(yp),
                                   cout, FWD, 1 if relu else 0, None, None, N.stream()), 'k4_vgg_conv3x3')
    return y, pre, yp


def conv3x3_dgrad(gy, w_split, cin, mask=None, add=None, ksize=3):
    """k4_vgg_conv3x3 input gradient: gy [B, H, W, cout] -> [B, H, W, cin], masked by ``mask > 0`` and with ``add`` added."""
    B, H, W, cout = gy.shape
    gx = torch.empty([B, H, W, cin], dtype=torch.float32, device=gy.device)
    N.check(N.lib().k4_vgg_conv3x3(N.f32(gy), cout, H, W, B, N.ptr(w_split), ksize, None, N.f32(gx), None, None, cin, DGRAD, 0,
                                   None if mask is None else N.f32(mask), None if add is None else N.f32(add), N.stream()), 'k4_vgg_conv3x3')
    return gx


def conv1_1(x0, x1, mean, std, w, b, keep_relu=True, keep_pre=False):
    """k4_vgg_conv1_1 on planar images x0, x1 (or None) [3, H, W]: (y or None, y_pre or None), [n, H, W, cout]."""
    _, H, W = x0.shape
    n, cout = (1 if x1 is None else 2), w.shape[0]
    y = torch.empty([n, H, W, cout], dtype=torch.float32, device=x0.device) if keep_relu else None
    pre = torch.empty([n, H, W, cout], dtype=torch.float32, device=x0.device) if keep_pre else None
    N.check(N.lib().k4_vgg_conv1_1(N.f32(x0), None if x1 is None else N.f32(x1), H, W, N.f32(mean), N.f32(std), N.f32(w), N.f32(b), cout,
                                   None if y is None else N.f32(y), None if pre is None else N.f32(pre), N.stream()), 'k4_vgg_conv1_1')
    return y, pre


def conv1_1_bwd(g, w, std):
    """k4_vgg_conv1_1_bwd: g [H, W, cout] -> the planar image gradient [3, H, W], 1 / std included."""
    H, W, cout = g.shape
    gx = torch.empty([3, H, W], dtype=torch.float32, device=g.device)
    N.check(N.lib().k4_vgg_conv1_1_bwd(N.f32(g), H, W, cout, N.f32(w), N.f32(std), N.f32(gx), N.stream()), 'k4_vgg_conv1_1_bwd')
    return gx


def pool_bwd(act, gp, add=None, relu_mask=True):
    """k4_vgg_pool_bwd: act [H, W, C], gp [H/2, W/2, C] -> [H, W, C]."""
    H, W, C = act.shape
    out = torch.empty_like(act)
    N.check(N.lib().k4_vgg_pool_bwd(N.f32(act), N.f32(gp), None if add is None else N.f32(add), H, W, C, 1 if relu_mask else 0, N.f32(out), N.stream()),
            'k4_vgg_pool_bwd')
    return out


def l1_fwd(a, b, scale=1.0):
    """scale * mean|a - b| as a float64 tensor [1] (fixed-order fp64 sums on the device)."""
    L = N.lib()
    n = a.numel()
    ws = torch.empty([L.k4_vgg_l1_workspace_bytes(n) // 8], dtype=torch.float64, device=a.device)
    out = torch.empty([1], dtype=torch.float64, device=a.device)
    N.check(L.k4_vgg_l1_fwd(N.f32(a), N.f32(b), n, float(scale), N.ptr(ws), N.ptr(out), N.stream()), 'k4_vgg_l1_fwd')
    return out


def l1_bwd(a, b, scale=1.0, grad_loss=None, add=None):
    ga = torch.empty_like(a)
    N.check(N.lib().k4_vgg_l1_bwd(N.f32(a), N.f32(b), a.numel(), float(scale), None if grad_loss is None else N.f32(grad_loss),
                                  None if add is None else N.f32(add), N.f32(ga), N.stream()), 'k4_vgg_l1_bwd')
    return ga


def gram(f):
    """k4_vgg_gram: f [2, P, C] -> [2, C, C], ``f^T f / (C P)`` of each image."""
    L = N.lib()
    _, P, C = f.shape
    nb = L.k4_vgg_gram_workspace_bytes(P, C)
    if nb < 0:
        raise N.K4Error(f'k4_vgg_gram: unsupported shape {tuple(f.shape)}')
    ws = torch.empty([nb // 4], dtype=torch.float32, device=f.device)
    G = torch.empty([2, C, C], dtype=torch.float32, device=f.device)
    N.check(L.k4_vgg_gram(N.f32(f), P, C, N.f32(ws), nb, N.f32(G), N.stream()), 'k4_vgg_gram')
    return G


def gram_bwd(fx, G, scale=1.0, grad_loss=None, add=None):
    """d(scale * mean|G[0] - G[1]|) / d fx for fx [H, W, C] (+ add): the operand from k4_vgg_gram_bwd_pack, then a one-tap k4_vgg_conv3x3."""
    L = N.lib()
    H, W, C = fx.shape
    M = torch.empty([L.k4_vgg_weight_bytes(C, C, 1) // 2], dtype=torch.int16, device=fx.device)
    N.check(L.k4_vgg_gram_bwd_pack(N.f32(G), H * W, C, float(scale), None if grad_loss is None else N.f32(grad_loss), N.ptr(M), N.stream()), 'k4_vgg_gram_bwd_pack')
    return conv3x3_dgrad(fx.reshape(1, H, W, C), M, C, add=None if add is None else add.reshape(1, H, W, C), ksize=1).reshape(H, W, C)


# ---- the modules ------------------------------------------------------------------------------------------------------------------

class _Layer(nn.Module):
    """One entry of ``vgg_net``: a convolution's frozen ``weight`` / ``bias`` (nn.Conv2d(cin, cout, 3, 1, 1)), or a parameter-free ReLU / pool.
    A holder: csrc/k4_vgg.hip evaluates the stack."""

    def __init__(self, name):
        super().__init__()
        if name in CONV_SHAPES:
            cout, cin = CONV_SHAPES[name]
            self.weight = nn.Parameter(torch.zeros(cout, cin, 3, 3), requires_grad=False)
            self.bias = nn.Parameter(torch.zeros(cout), requires_grad=False)

    def forward(self, *a, **k):
        raise N.K4Error('a layer of VGGFeatureExtractor is a parameter holder: call the extractor')


class VGGFeatureExtractor(nn.Module):
    """``basicsr.archs.vgg_arch.VGGFeatureExtractor``: torchvision's ``vgg19().features`` truncated after the deepest requested layer;
    ``forward(x)`` -> ``{name: tensor [1, C, h, w]}``; a tapped ``convK_J`` is the convolution's output in front of its ReLU."""

    def __init__(self, layer_name_list, vgg_type='vgg19', use_input_norm=True, range_norm=False, requires_grad=False, remove_pooling=False, pooling_stride=2):
        super().__init__()
        for arg, val, want in (('vgg_type', vgg_type, 'vgg19'), ('range_norm', range_norm, False), ('requires_grad', requires_grad, False),
                               ('remove_pooling', remove_pooling, False), ('pooling_stride', pooling_stride, 2)):
            if val != want:
                raise NotImplementedError(f'VGGFeatureExtractor: {arg}={val!r} is not provided (only {arg}={want!r}: configs/llff/fern_lg_joint_l1+gan.py)')
        self.layer_name_list = list(layer_name_list)
        for n in self.layer_name_list:
            if n not in NAMES:
                raise ValueError(f'VGGFeatureExtractor: {n!r} is not a layer of vgg19')
        if not self.layer_name_list:
            raise ValueError('VGGFeatureExtractor: empty layer_name_list')
        self.use_input_norm, self.range_norm = use_input_norm, range_norm
        self.names = NAMES[:max(NAMES.index(n) for n in self.layer_name_list) + 1]
        self.vgg_net = nn.Module()
        for n in self.names:
            self.vgg_net.add_module(n, _Layer(n))
        if use_input_norm:
            self.register_buffer('mean', torch.tensor(MEAN).view(1, 3, 1, 1))
            self.register_buffer('std', torch.tensor(STD).view(1, 3, 1, 1))
        self._loaded = False
        self._packed = None
        self.register_load_state_dict_post_hook(VGGFeatureExtractor._after_load)

    @staticmethod
    def _after_load(module, incompatible):
        if not any('vgg_net.' in k for k in incompatible.missing_keys):
            module._loaded, module._packed = True, None

    def conv_names(self):
        return [n for n in self.names if n in CONV_SHAPES]

    def load_vgg_state_dict(self, sd):
        """Copy the convolution weights from a torchvision ``vgg19`` state dict (``features.<i>.weight`` / ``.bias``; classifier keys ignored) or from the
        extractor's own keys (``vgg_net.<name>.weight``, with or without a ``vgg.`` prefix).  Every layer of this extractor must be present."""
        with torch.no_grad():
            for n in self.conv_names():
                i = NAMES.index(n)
                for part in ('weight', 'bias'):
                    src = None
                    for key in (f'features.{i}.{part}', f'vgg_net.{n}.{part}', f'vgg.vgg_net.{n}.{part}'):
                        if key in sd:
                            src = sd[key]
                            break
                    if src is None:
                        raise KeyError(f'load_vgg_state_dict: no features.{i}.{part} / vgg_net.{n}.{part} in the state dict')
                    dst = getattr(getattr(self.vgg_net, n), part)
                    if tuple(src.shape) != tuple(dst.shape):
                        raise ValueError(f'load_vgg_state_dict: {n}.{part} has shape {tuple(src.shape)}, expected {tuple(dst.shape)}')
                    dst.copy_(src)
        self._loaded, self._packed = True, None
        return self

    def k4_operands(self, device, need_dgrad):
        """The packed operands of the stack on `device`, built once per weight load (the weights are constant)."""
        if not self._loaded:
            raise N.K4Error('VGGFeatureExtractor: the VGG19 weights were never loaded (load_vgg_state_dict(torchvision vgg19 state dict); the constructor fetches nothing)')
        params = [getattr(self.vgg_net, n) for n in self.conv_names()]
        key = (str(device), tuple((m.weight.data_ptr(), m.weight._version) for m in params))
        if self._packed is None or self._packed['key'] != key:
            for m in params:
                if not (m.weight.is_cuda and m.weight.dtype == torch.float32 and m.weight.is_contiguous() and m.bias.is_contiguous()):
                    raise N.K4Error('VGGFeatureExtractor: parameters must be contiguous CUDA float32 tensors (no CPU path exists)')
            ops = {}
            for n, m in zip(self.conv_names(), params):
                ops[n] = {'w': m.weight.detach(), 'b': m.bias.detach(), 'fwd': None if n == 'conv1_1' else pack_weight(m.weight.detach(), FWD), 'bwd': None}
            if self.use_input_norm:
                mean, std = self.mean.reshape(3).contiguous(), self.std.reshape(3).contiguous()
            else:
                mean, std = torch.zeros(3, device=device), torch.ones(3, device=device)
            self._packed = {'key': key, 'ops': ops, 'mean': mean, 'std': std}
        if need_dgrad:
            for n, op in self._packed['ops'].items():
                if op['bwd'] is None and n != 'conv1_1':
                    op['bwd'] = pack_weight(op['w'], DGRAD)
        return self._packed

    def _check_image(self, x, what):
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise N.K4Error(f'{what}: tensor must be on the GPU (no CPU path exists for the VGG19 feature losses)')
        if x.dtype != torch.float32 or x.dim() != 4 or x.shape[0] != 1 or x.shape[1] != 3:
            raise N.K4Error(f'{what}: expected one float32 image [1, 3, H, W], got {x.dtype} {tuple(x.shape)}')
        if x.shape[2] % 16 != 0 or x.shape[3] % 16 != 0 or x.shape[2] <= 0 or x.shape[3] <= 0:
            raise N.K4Error(f'{what}: H and W must be multiples of 16, got {tuple(x.shape[2:])}')

    def k4_run(self, x0, x1, names, taps, keep):
        """The stack `names` on planar images x0, x1 (None: one image) [3, H, W].  taps: names whose tensor is returned; keep: also return every
        post-ReLU activation (the backward pass reads masks and pool choices from them).  Returns (feats {name: [n, h, w, C]}, acts {conv name: [n, h, w, C]})."""
        P = self.k4_operands(x0.device, False)
        ops = P['ops']
        feats, acts = {}, {}
        last = len(names) - 1
        cur = None
        for i, n in enumerate(names):
            if n not in CONV_SHAPES:
                continue
            cout, cin = CONV_SHAPES[n]
            rn, pn = 'relu' + n[4:], (names[i + 2] if i + 2 <= last and names[i + 2].startswith('pool') else None)
            want_relu = i < last                                    # anything after the convolution reads its ReLU
            want_pre = n in taps
            if n == 'conv1_1':
                y, pre = conv1_1(x0, x1, P['mean'], P['std'], ops[n]['w'], ops[n]['b'], keep_relu=want_relu, keep_pre=want_pre)
                yp = None
                if pn is not None:                                  # (vgg19 has no pool behind conv1_1)
                    raise N.K4Error('unexpected layer order')
            else:
                y, pre, yp = conv3x3(cur, ops[n]['fwd'], ops[n]['b'], cout, relu=True, keep_relu=want_relu, keep_pre=want_pre, pool=pn is not None)
            if want_pre:
                feats[n] = pre
            if rn in taps:
                feats[rn] = y
            if pn is not None and pn in taps:
                feats[pn] = yp
            if keep and y is not None:
                acts[n] = y
            cur = yp if pn is not None else y
        return feats, acts

    def forward(self, x):
        self._check_image(x, 'VGGFeatureExtractor')
        if torch.is_grad_enabled() and x.requires_grad:
            raise N.K4Error('VGGFeatureExtractor.forward does not record a gradient: the losses and their input gradient are PerceptualLoss')
        if self.range_norm:
            raise NotImplementedError('range_norm')
        x0 = x.detach().contiguous().reshape(3, x.shape[2], x.shape[3])
        feats, _ = self.k4_run(x0, None, self.names, set(self.layer_name_list), False)
        return {n: feats[n].permute(0, 3, 1, 2) for n in self.layer_name_list}


class _K4Perceptual(torch.autograd.Function):
    """Both terms and their gradient to ``x`` as one node: forward = the stack on (x, gt) as a batch of two + the loss heads; backward = the
    seeds of the tapped layers followed back through the input gradient of every layer."""

    @staticmethod
    def forward(ctx, x, gt, mod):
        vgg = mod.vgg
        H, W = x.shape[2], x.shape[3]
        need = ctx.needs_input_grad[0]
        x0 = x.detach().contiguous().reshape(3, H, W)
        g0 = gt.detach().contiguous().reshape(3, H, W)
        taps = mod.k4_taps()                                         # [(name, w_k)] with w_k != 0, in layer order
        names = NAMES[:NAMES.index(taps[-1][0]) + 1] if taps else []
        pw, sw = float(mod.perceptual_weight), float(mod.style_weight)
        feats, acts = vgg.k4_run(x0, g0, names, {n for n, _ in taps}, need or _KEEP_RECORD) if taps else ({}, {})
        dev = x.device
        percep = torch.zeros([1], dtype=torch.float64, device=dev)
        style = torch.zeros([1], dtype=torch.float64, device=dev)
        grams = {}
        for n, wk in taps:                                           # lib/sr_loss.py:140-145, 152-159: sum of criterion * w_k, then the term's weight
            f = feats[n]
            if pw > 0:
                percep = percep + l1_fwd(f[0], f[1], wk)
            if sw > 0:
                grams[n] = gram(f.reshape(2, -1, f.shape[3]))
                style = style + l1_fwd(grams[n][0], grams[n][1], wk)
        percep, style = (percep * pw).float().reshape(()), (style * sw).float().reshape(())
        if _KEEP_RECORD:
            mod.k4_record = _record(names, feats, acts, grams, taps)
        if need:
            ctx.k4 = dict(mod=mod, names=names, taps=taps, feats=feats, acts=acts, grams=grams, hw=(H, W))
        return percep, style

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_p, g_s):
        S = ctx.k4
        mod, names, taps, feats, acts, grams = S['mod'], S['names'], dict(S['taps']), S['feats'], S['acts'], S['grams']
        H, W = S['hw']
        ctx.k4 = None
        if not names:
            return torch.zeros([1, 3, H, W], dtype=torch.float32, device=g_p.device), None, None
        vgg = mod.vgg
        P = vgg.k4_operands(g_p.device, True)
        ops = P['ops']
        pw, sw = float(mod.perceptual_weight), float(mod.style_weight)
        go_p = g_p.detach().float().reshape(1).contiguous()
        go_s = g_s.detach().float().reshape(1).contiguous()

        def seed(n):                                                 # d(percep + style) / d f_n(x), or None
            if n not in taps:
                return None
            f, wk = feats[n], taps[n]
            s = None
            if sw > 0:
                s = gram_bwd(f[0], grams[n], sw * wk, go_s)
            if pw > 0:
                s = l1_bwd(f[0], f[1], pw * wk, go_p, add=s)
            return s
        convs = [n for n in names if n in CONV_SHAPES]
        g = seed(convs[-1])                                          # gradient at the convolution's output, in front of its ReLU
        for k in range(len(convs) - 1, 0, -1):
            n, below = convs[k], convs[k - 1]
            cin = CONV_SHAPES[n][1]
            pooled = names[names.index(n) - 1].startswith('pool')
            act = acts[below][0]
            if pooled:
                gp = conv3x3_dgrad(g.unsqueeze(0) if g.dim() == 3 else g, ops[n]['bwd'], cin)
                g = pool_bwd(act, gp[0], add=seed(below), relu_mask=True)
            else:
                sd = seed(below)
                g = conv3x3_dgrad(g.unsqueeze(0) if g.dim() == 3 else g, ops[n]['bwd'], cin, mask=act.unsqueeze(0), add=None if sd is None else sd.unsqueeze(0))[0]
        gx = conv1_1_bwd(g if g.dim() == 3 else g[0], ops['conv1_1']['w'], P['std'])
        return gx.reshape(1, 3, H, W), None, None


def _record(names, feats, acts, grams, taps):
    """The decisions of a forward pass, from the buffers it saved (tests/vgg_oracle.grad_with_record evaluates the gradient with them)."""
    rec = {'relu_mask': {}, 'pool_choice': {}, 'feat_sign': {}, 'gram_sign': {}}
    for n, a in acts.items():
        rec['relu_mask'][n] = (a[0] > 0).permute(2, 0, 1).unsqueeze(0)
        i = names.index(n)
        if i + 2 < len(names) and names[i + 2].startswith('pool'):
            v = a[0]
            cand = [v[dy::2, dx::2] for dy in (0, 1) for dx in (0, 1)]
            best, idx = cand[0], torch.zeros_like(cand[0], dtype=torch.uint8)
            for k in (1, 2, 3):
                take = cand[k] > best
                best, idx = torch.where(take, cand[k], best), torch.where(take, torch.full_like(idx, k), idx)
            rec['pool_choice'][names[i + 2]] = idx.permute(2, 0, 1).unsqueeze(0)
    for n, _ in taps:
        f = feats[n]
        rec['feat_sign'][n] = torch.sign(f[0] - f[1]).to(torch.int8).permute(2, 0, 1).unsqueeze(0)
        if n in grams:
            rec['gram_sign'][n] = torch.sign(grams[n][0] - grams[n][1]).to(torch.int8)
    return rec


class PerceptualLoss(nn.Module):
    """``basicsr.losses.PerceptualLoss``: ``forward(x, gt) -> (percep, style)``,

        percep = perceptual_weight * sum_k w_k * mean|f_k(x) - f_k(gt)|,   style = style_weight * sum_k w_k * mean|G(f_k(x)) - G(f_k(gt))|,
        G(f) = f f^T / (c h w)                                            (lib/sr_loss.py:134-161, 175-188 restate the same expressions)

    a term whose weight is not > 0 is None; ``gt`` is detached; a layer with ``w_k == 0`` adds an exact zero and is not evaluated."""

    def __init__(self, layer_weights, vgg_type='vgg19', use_input_norm=True, range_norm=False, perceptual_weight=1.0, style_weight=0., criterion='l1'):
        super().__init__()
        if criterion != 'l1':
            raise NotImplementedError(f"PerceptualLoss: criterion={criterion!r} is not provided (only criterion='l1': run_sr.py:678)")
        self.perceptual_weight, self.style_weight = perceptual_weight, style_weight
        self.layer_weights = dict(layer_weights)
        for n, w in self.layer_weights.items():
            if w != 0 and n not in CONV_SHAPES:
                raise NotImplementedError(f'PerceptualLoss: a weighted tap on {n!r} is not provided (only convK_J layers: run_sr.py:671-677)')
            if w < 0:
                raise NotImplementedError(f'PerceptualLoss: negative layer weight for {n!r}')
        self.vgg = VGGFeatureExtractor(list(self.layer_weights.keys()), vgg_type=vgg_type, use_input_norm=use_input_norm, range_norm=range_norm)
        self.criterion_type = criterion
        self.k4_record = None

    def load_vgg_state_dict(self, sd):
        self.vgg.load_vgg_state_dict(sd)
        return self

    def k4_taps(self):
        return sorted(((n, float(w)) for n, w in self.layer_weights.items() if w != 0), key=lambda t: NAMES.index(t[0]))

    def forward(self, x, gt):
        self.vgg._check_image(x, 'PerceptualLoss(x)')
        self.vgg._check_image(gt, 'PerceptualLoss(gt)')
        if x.shape != gt.shape:
            raise N.K4Error(f'PerceptualLoss: x {tuple(x.shape)} and gt {tuple(gt.shape)} differ in shape')
        self.vgg.k4_operands(x.device, False)                        # (raises on weights that were never loaded, whatever the weights of the terms)
        percep, style = _K4Perceptual.apply(x, gt.detach(), self)
        return (percep if self.perceptual_weight > 0 else None), (style if self.style_weight > 0 else None)
