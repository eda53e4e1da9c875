"""U-Net discriminator with spectral normalisation and the vanilla GAN loss of the "+gan" joint recipes.

Restates ``UNetDiscriminatorSN`` of the reference's lib/sr_unetdisc.py:7-62 (constructor :10-29, forward :31-62) behind the same
constructor and the same 28 ``state_dict`` keys (``conv0.weight/bias``, ``conv{1..8}.weight_orig/weight_u/weight_v``,
``conv9.weight/bias`` -- the keys of ``torch.nn.utils.spectral_norm``, which wraps conv1-8 upstream), so a discriminator checkpoint
loads both ways, strictly.  ``UNetDiscriminatorSN_pose`` / ``_viewdir`` (:65-) need the StyleGAN epilogue and are not provided.

Two execution paths:
  * the tensor-library path (``F.conv2d`` / ``F.interpolate``): any device, any dtype; what the CPU tests pin to the reference;
  * the HIP path (csrc/k4_disc.hip + the decoder's 3x3 kernels), default for one CUDA fp32 image whose sides are multiples of 8 and
    ``num_feat`` in {16, 32, 48, 64}: the whole forward + backward is ONE autograd node on NHWC buffers.  Spectral norm (power
    iteration, sigma, the scaled weight in packed operand form) is one native call per layer; the 4x4 stride-2 layers, their input and
    weight gradients, the x2 bilinear resampling and the loss run on the kernels of k4_disc.hip; the 3x3 layers on
    k4_conv2d_nhwc_bf16x6 / k4_conv2d_wgrad_bf16x6.  Everything else takes the tensor-library path silently.
``_K4 = False`` forces the tensor-library path (A/B, tests).

``GANLoss`` restates ``basicsr.losses.GANLoss(gan_type='vanilla')`` from its published definition (basicsr is not a dependency of this
package and was not available to compare against): ``BCEWithLogitsLoss`` against an all-ones ("real") or all-zeros ("fake") target,
``loss_weight`` applied to the generator's term only (``is_disc=False``).  The tests pin it to ``F.binary_cross_entropy_with_logits``.
"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _native as N

_K4 = True          # False: tensor-library path on every input (A/B, tests)
SLOPE = 0.2
SN_EPS = 1e-12


class _PlainConv(nn.Module):
    """The parameters of nn.Conv2d(cin, cout, 3, 1, 1) with bias (conv0, conv9): ``weight`` / ``bias``, nn.Conv2d's default initialisation.
    A holder: the two execution paths of UNetDiscriminatorSN evaluate it."""

    def __init__(self, cin, cout):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(cout, cin, 3, 3))
        self.bias = nn.Parameter(torch.empty(cout))
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        bound = 1.0 / math.sqrt(cin * 9)
        nn.init.uniform_(self.bias, -bound, bound)


class _SNConv(nn.Module):
    """A bias-free convolution whose weight is ``weight_orig / sigma`` (torch.nn.utils.spectral_norm, one power iteration per training-mode
    call, in place and without gradient; ``weight_u`` / ``weight_v`` are buffers).  The iteration runs in training mode whatever the
    parameter's ``requires_grad`` says: the joint loop advances u, v three times per iteration."""

    def __init__(self, cin, cout, ksize, stride):
        super().__init__()
        self.ksize, self.stride = ksize, stride
        self.weight_orig = nn.Parameter(torch.empty(cout, cin, ksize, ksize))
        nn.init.kaiming_uniform_(self.weight_orig, a=math.sqrt(5))
        self.register_buffer('weight_u', F.normalize(torch.randn(cout), dim=0, eps=SN_EPS))
        self.register_buffer('weight_v', F.normalize(torch.randn(cin * ksize * ksize), dim=0, eps=SN_EPS))

    def normalized_weight(self):
        w = self.weight_orig
        wm = w.reshape(w.shape[0], -1)
        u, v = self.weight_u, self.weight_v
        if self.training:
            with torch.no_grad():
                v = F.normalize(torch.mv(wm.t(), u), dim=0, eps=SN_EPS, out=v)
                u = F.normalize(torch.mv(wm, v), dim=0, eps=SN_EPS, out=u)
            u, v = u.clone(), v.clone()             # the buffers change in place on the next call; backward needs these values
        sigma = torch.dot(u, torch.mv(wm, v))
        return w / sigma


def _up2(x):
    return F.interpolate(x, scale_factor=2, mode='bilinear', align_corners=False)


class UNetDiscriminatorSN(nn.Module):
    """[N, num_in_ch, H, W] -> [N, 1, H//8*8, W//8*8] logits."""

    def __init__(self, num_in_ch, num_feat=64, skip_connection=True):
        super().__init__()
        nf = num_feat
        self.num_in_ch, self.num_feat, self.skip_connection = num_in_ch, num_feat, skip_connection
        self.conv0 = _PlainConv(num_in_ch, nf)
        self.conv1 = _SNConv(nf, nf * 2, 4, 2)          # encoder: three 4x4 stride-2 layers
        self.conv2 = _SNConv(nf * 2, nf * 4, 4, 2)
        self.conv3 = _SNConv(nf * 4, nf * 8, 4, 2)
        self.conv4 = _SNConv(nf * 8, nf * 4, 3, 1)      # decoder: x2 bilinear, 3x3, skip
        self.conv5 = _SNConv(nf * 4, nf * 2, 3, 1)
        self.conv6 = _SNConv(nf * 2, nf, 3, 1)
        self.conv7 = _SNConv(nf, nf, 3, 1)
        self.conv8 = _SNConv(nf, nf, 3, 1)
        self.conv9 = _PlainConv(nf, 1)

    def sn_layers(self):
        return [getattr(self, f'conv{i}') for i in range(1, 9)]

    def k4_eligible(self, x):
        return (_K4 and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.shape[0] == 1 and x.shape[1] == self.num_in_ch
                and self.num_in_ch <= 3 and x.shape[2] % 8 == 0 and x.shape[3] % 8 == 0 and x.shape[2] >= 8 and x.shape[3] >= 8
                and self.num_feat % 16 == 0 and self.num_feat <= 64
                and all(p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() for p in self.parameters())
                and all(b.is_cuda and b.dtype == torch.float32 and b.is_contiguous() for b in self.buffers()))

    def forward(self, x):
        if self.k4_eligible(x):
            return _K4Disc.apply(x, self, *self.parameters())
        return tensor_library_forward(self, x)


def tensor_library_forward(net, x):
    """lib/sr_unetdisc.py:31-62 on tensor-library operations (any device): the pin of the CPU tests and the HIP path's A/B partner."""
    H, W = x.shape[2] // 8 * 8, x.shape[3] // 8 * 8
    x = F.interpolate(x, size=(H, W), mode='bilinear', align_corners=False)       # the identity for sides that are multiples of 8

    def plain(m, t):
        return F.conv2d(t, m.weight, m.bias, 1, 1)

    def sn(m, t):
        return F.leaky_relu(F.conv2d(t, m.normalized_weight(), None, m.stride, 1), SLOPE)
    x0 = F.leaky_relu(plain(net.conv0, x), SLOPE)
    x1 = sn(net.conv1, x0)
    x2 = sn(net.conv2, x1)
    x3 = sn(net.conv3, x2)
    x4 = sn(net.conv4, _up2(x3))
    if net.skip_connection:
        x4 = x4 + x2
    x5 = sn(net.conv5, _up2(x4))
    if net.skip_connection:
        x5 = x5 + x1
    x6 = sn(net.conv6, _up2(x5))
    if net.skip_connection:
        x6 = x6 + x0
    return plain(net.conv9, sn(net.conv8, sn(net.conv7, x6)))


# ---- HIP path ---------------------------------------------------------------------------------------------------------------------

def sn_prepare(weight_orig, u, v, train, bwd_form=None):
    """k4_sn_prepare on one layer: (sigma [1], forward operand, input-gradient operand or None); u, v advance in place when ``train``."""
    L = N.lib()
    cout, cin, k, _ = weight_orig.shape
    dev = weight_orig.device
    sigma = torch.empty([1], dtype=torch.float32, device=dev)
    ws = torch.empty([L.k4_sn_workspace_floats(cout, cin, k)], dtype=torch.float32, device=dev)
    wf = torch.empty([L.k4_disc_weight_bytes(cout, cin, k) // 2], dtype=torch.int16, device=dev)
    wb = None if bwd_form is None else torch.empty([L.k4_disc_weight_bytes(cin, cout, k) // 2], dtype=torch.int16, device=dev)
    N.check(L.k4_sn_prepare(N.f32(weight_orig), N.f32(u), N.f32(v), cout, cin, k, 1 if train else 0, SN_EPS, N.f32(sigma), N.f32(ws),
                            N.ptr(wf), N.ptr(wb), bwd_form or 0, N.stream()), 'k4_sn_prepare')
    return sigma, wf, wb


def sn_project_grad(g, weight_orig, u, v, sigma):
    L = N.lib()
    cout = weight_orig.shape[0]
    K = weight_orig.numel() // cout
    ws = torch.empty([L.k4_sn_workspace_floats(cout, K, 1)], dtype=torch.float32, device=g.device)
    out = torch.empty_like(weight_orig)
    N.check(L.k4_sn_project_grad(N.f32(g), N.f32(weight_orig), N.f32(u), N.f32(v), N.f32(sigma), cout, K, N.f32(ws), N.f32(out), N.stream()),
            'k4_sn_project_grad')
    return out


def conv_s2(x, H, W, cin, w_split, cout, mode, lrelu=False):
    """k4_disc_conv_s2 on a contiguous NHWC image x [H, W, cin]; returns the new image."""
    shape = {0: (H // 2, W // 2), 1: (2 * H, 2 * W), 2: (H, W)}[mode]
    y = torch.empty([shape[0], shape[1], cout], dtype=torch.float32, device=x.device)
    N.check(N.lib().k4_disc_conv_s2(N.f32(x), cin, cin, H, W, N.ptr(w_split), N.f32(y), cout, cout, mode, 1 if lrelu else 0, SLOPE, N.stream()),
            'k4_disc_conv_s2')
    return y


def wgrad_s2(x, H, W, cin, gy, cout):
    L = N.lib()
    nb = L.k4_disc_wgrad_workspace_bytes(cin, cout, H, W)
    if nb < 0:
        raise N.K4Error('k4_disc_wgrad_s2: unsupported shape')
    ws = torch.empty([nb // 4], dtype=torch.float32, device=x.device)
    dw = torch.empty([cout, cin, 4, 4], dtype=torch.float32, device=x.device)
    N.check(L.k4_disc_wgrad_s2(N.f32(x), cin, cin, H, W, N.f32(gy), cout, cout, N.f32(dw), N.f32(ws), nb, N.stream()), 'k4_disc_wgrad_s2')
    return dw


def bilinear2x(x, add=None):
    H, W, C = x.shape
    y = torch.empty([2 * H, 2 * W, C], dtype=torch.float32, device=x.device)
    N.check(N.lib().k4_bilinear2x_nhwc(N.f32(x), None if add is None else N.f32(add), H, W, C, N.f32(y), N.stream()), 'k4_bilinear2x_nhwc')
    return y


def bilinear2x_bwd(gy):
    H2, W2, C = gy.shape
    gx = torch.empty([H2 // 2, W2 // 2, C], dtype=torch.float32, device=gy.device)
    N.check(N.lib().k4_bilinear2x_bwd_nhwc(N.f32(gy), H2 // 2, W2 // 2, C, N.f32(gx), N.stream()), 'k4_bilinear2x_bwd_nhwc')
    return gx


class _Op3:
    """A packed operand of k4_conv2d_nhwc_bf16x6 filled by k4_sn_prepare (the fields SFTNet._conv reads)."""
    mode, flags_extra, k = 'bf16x6', 0, 3

    def __init__(self, w, cin, nout, zeros):
        self.w, self.cin, self.b = w, cin, zeros[:(nout + 31) // 32 * 32]


def _lrelu_bwd(g, y):
    n_pix, c = y.shape[0] * y.shape[1], y.shape[2]
    N.check(N.lib().k4_lrelu_bwd(N.f32(g), c, N.f32(y), c, n_pix, c, SLOPE, N.f32(g), c, N.stream()), 'k4_lrelu_bwd')
    return g


def _add_(a, b):
    N.check(N.lib().k4_add_f32(N.f32(a), N.f32(b), N.f32(a), a.numel(), N.stream()), 'k4_add_f32')
    return a


class _K4Disc(torch.autograd.Function):
    """The discriminator's forward and backward as one node.  Inputs: the image, the module, its parameters in ``parameters()`` order
    (conv0.weight, conv0.bias, conv1..8.weight_orig, conv9.weight, conv9.bias)."""

    @staticmethod
    def forward(ctx, x, net, *params):
        from .sr_esrnet import SFTNet, _Packed, EPI_LRELU, CONV_SMALL
        conv3 = SFTNet._conv
        nf, train = net.num_feat, net.training
        _, cin0, H, W = x.shape
        dev = x.device
        need_w = any(ctx.needs_input_grad[2:])
        need_x = ctx.needs_input_grad[0]
        need = need_w or need_x
        w0, b0, w9, b9 = params[0], params[1], params[10], params[11]
        sn = net.sn_layers()
        zeros = torch.zeros([256], dtype=torch.float32, device=dev)
        ops = []
        for i, m in enumerate(sn):                                   # one native call per layer: power iteration, sigma, both operands
            if not need:
                form = None
            elif m.ksize == 4 or m.weight_orig.shape[1] > 256:       # (conv4 at num_feat=64: 512 dgrad outputs, k4_disc_conv_s2's 3x3 form)
                form = 4
            else:
                form = 1
            ops.append(sn_prepare(m.weight_orig.detach(), m.weight_u, m.weight_v, train, form) + (form,))
        net.k4_sigma = [op[0] for op in ops]                         # the last call's sigma per layer (tests, diagnosis)
        xh = x.detach().permute(0, 2, 3, 1).reshape(H, W, cin0).contiguous()

        def c3(i, t, h, w, act=True):                                # SN 3x3 layer i on image t [h, w, cin]
            m = sn[i - 1]
            cout, cin = m.weight_orig.shape[:2]
            y = torch.empty([h, w, cout], dtype=torch.float32, device=dev)
            conv3(_Op3(ops[i - 1][1], cin, cout, zeros), t, 0, cin, y, 0, cout, cout, h, w, flags=(EPI_LRELU if act else 0) | CONV_SMALL)
            return y
        x0 = torch.empty([H, W, nf], dtype=torch.float32, device=dev)
        conv3(_Packed.native(w0.detach(), b0.detach()), xh, 0, cin0, x0, 0, nf, nf, H, W, flags=EPI_LRELU | CONV_SMALL)
        x1 = conv_s2(x0, H, W, nf, ops[0][1], 2 * nf, 0, True)
        x2 = conv_s2(x1, H // 2, W // 2, 2 * nf, ops[1][1], 4 * nf, 0, True)
        x3 = conv_s2(x2, H // 4, W // 4, 4 * nf, ops[2][1], 8 * nf, 0, True)
        skip = net.skip_connection
        u3 = bilinear2x(x3)
        x4 = c3(4, u3, H // 4, W // 4)
        u4 = bilinear2x(x4, x2 if skip else None)
        x5 = c3(5, u4, H // 2, W // 2)
        u5 = bilinear2x(x5, x1 if skip else None)
        x6 = c3(6, u5, H, W)
        s6 = _add_(x6.clone(), x0) if skip else x6
        x7 = c3(7, s6, H, W)
        x8 = c3(8, x7, H, W)
        out = torch.empty([H, W, 1], dtype=torch.float32, device=dev)
        conv3(_Packed.native(w9.detach(), b9.detach()), x8, 0, nf, out, 0, 1, 1, H, W, flags=CONV_SMALL)
        if need:
            uv = [(m.weight_u.clone(), m.weight_v.clone()) for m in sn] if need_w else None
            ctx.k4 = dict(net=net, acts=(xh, x0, x1, x2, x3, u3, x4, u4, x5, u5, x6, s6, x7, x8), ops=ops, uv=uv, zeros=zeros, hw=(H, W), cin0=cin0)
            ctx.save_for_backward(*params)
        return out.reshape(1, 1, H, W)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        from .sr_esrnet import SFTNet, _Packed, CONV_SMALL
        from .sr_train import _wgrad
        conv3 = SFTNet._conv
        S = ctx.k4
        net, ops, uv, zeros = S['net'], S['ops'], S['uv'], S['zeros']
        xh, x0, x1, x2, x3, u3, x4, u4, x5, u5, x6, s6, x7, x8 = S['acts']
        params = ctx.saved_tensors
        H, W = S['hw']
        nf, cin0, skip = net.num_feat, S['cin0'], net.skip_connection
        dev = g.device
        sn = net.sn_layers()
        need_p = [ctx.needs_input_grad[2 + i] for i in range(12)]
        grads = [None] * 12
        g = g.contiguous().float().reshape(H, W, 1)

        def dgrad3(i, gy, h, w):                                     # input gradient of SN 3x3 layer i
            cout, cin = sn[i - 1].weight_orig.shape[:2]
            sigma, wf, wb, form = ops[i - 1]
            if form == 4:
                return conv_s2(gy, h, w, cout, wb, cin, 2)
            gx = torch.empty([h, w, cin], dtype=torch.float32, device=dev)
            conv3(_Op3(wb, cout, cin, zeros), gy, 0, cout, gx, 0, cin, cin, h, w, flags=CONV_SMALL)
            return gx

        def wg3(i, xin, gy, h, w):                                   # weight gradient of SN 3x3 layer i, through the division by sigma
            if not need_p[1 + i]:
                return
            m = sn[i - 1]
            cout, cin = m.weight_orig.shape[:2]
            raw, _ = _wgrad(xin, 0, cin, cin, gy, 0, cout, cout, 3, h, w, m.weight_orig.shape, False)
            grads[1 + i] = sn_project_grad(raw, params[1 + i], uv[i - 1][0], uv[i - 1][1], ops[i - 1][0])

        def wg4(i, xin, gy, h, w):                                   # ... of a 4x4 stride-2 layer (xin [h, w, cin], gy [h/2, w/2, cout])
            if not need_p[1 + i]:
                return
            m = sn[i - 1]
            cout, cin = m.weight_orig.shape[:2]
            raw = wgrad_s2(xin, h, w, cin, gy, cout)
            grads[1 + i] = sn_project_grad(raw, params[1 + i], uv[i - 1][0], uv[i - 1][1], ops[i - 1][0])
        # conv9 (plain, with bias)
        w9 = params[10]
        if need_p[10] or need_p[11]:
            gw, gb = _wgrad(x8, 0, nf, nf, g, 0, 1, 1, 3, H, W, w9.shape, True)
            grads[10], grads[11] = (gw if need_p[10] else None), (gb if need_p[11] else None)
        g8 = torch.empty([H, W, nf], dtype=torch.float32, device=dev)
        pk = _Packed.native(w9.detach(), None, dgrad=True)
        conv3(pk, g, 0, 1, g8, 0, nf, nf, H, W, flags=CONV_SMALL)
        _lrelu_bwd(g8, x8)
        wg3(8, x7, g8, H, W)
        g7 = _lrelu_bwd(dgrad3(8, g8, H, W), x7)
        wg3(7, s6, g7, H, W)
        gs6 = dgrad3(7, g7, H, W)
        g6 = _lrelu_bwd(gs6.clone(), x6) if skip else _lrelu_bwd(gs6, x6)
        wg3(6, u5, g6, H, W)
        gs5 = bilinear2x_bwd(dgrad3(6, g6, H, W))                    # gradient of x5 (+ x1)
        g5 = _lrelu_bwd(gs5.clone(), x5) if skip else _lrelu_bwd(gs5, x5)
        wg3(5, u4, g5, H // 2, W // 2)
        gs4 = bilinear2x_bwd(dgrad3(5, g5, H // 2, W // 2))          # gradient of x4 (+ x2)
        g4 = _lrelu_bwd(gs4.clone(), x4) if skip else _lrelu_bwd(gs4, x4)
        wg3(4, u3, g4, H // 4, W // 4)
        g3 = _lrelu_bwd(bilinear2x_bwd(dgrad3(4, g4, H // 4, W // 4)), x3)
        wg4(3, x2, g3, H // 4, W // 4)
        g2 = conv_s2(g3, H // 8, W // 8, 8 * nf, ops[2][2], 4 * nf, 1)
        if skip:
            _add_(g2, gs4)
        _lrelu_bwd(g2, x2)
        wg4(2, x1, g2, H // 2, W // 2)
        g1 = conv_s2(g2, H // 4, W // 4, 4 * nf, ops[1][2], 2 * nf, 1)
        if skip:
            _add_(g1, gs5)
        _lrelu_bwd(g1, x1)
        wg4(1, x0, g1, H, W)
        g0 = conv_s2(g1, H // 2, W // 2, 2 * nf, ops[0][2], nf, 1)
        if skip:
            _add_(g0, gs6)
        _lrelu_bwd(g0, x0)
        w0 = params[0]
        if need_p[0] or need_p[1]:
            gw, gb = _wgrad(xh, 0, cin0, cin0, g0, 0, nf, nf, 3, H, W, w0.shape, True)
            grads[0], grads[1] = (gw if need_p[0] else None), (gb if need_p[1] else None)
        gx = None
        if ctx.needs_input_grad[0]:
            pk = _Packed.native(w0.detach(), None, dgrad=True)
            gxh = torch.empty([H, W, cin0], dtype=torch.float32, device=dev)
            conv3(pk, g0, 0, nf, gxh, 0, cin0, cin0, H, W, flags=CONV_SMALL)
            gx = gxh.permute(2, 0, 1).unsqueeze(0).contiguous()
        ctx.k4 = None
        return (gx, None) + tuple(grads)


# ---- the adversarial loss ---------------------------------------------------------------------------------------------------------

class _K4GanLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, real, scale):
        x = x.contiguous()
        loss = torch.empty([1], dtype=torch.float32, device=x.device)
        N.check(N.lib().k4_gan_loss_fwd(N.f32(x), x.numel(), 1 if real else 0, scale, N.f32(loss), N.stream()), 'k4_gan_loss_fwd')
        ctx.save_for_backward(x)
        ctx.real, ctx.scale = real, scale
        return loss.reshape(())

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, go):
        x, = ctx.saved_tensors
        gx = torch.empty_like(x)
        go = go.contiguous().float().reshape(1)
        N.check(N.lib().k4_gan_loss_bwd(N.f32(x), x.numel(), 1 if ctx.real else 0, ctx.scale, N.f32(go), N.f32(gx), N.stream()), 'k4_gan_loss_bwd')
        return gx, None, None


class GANLoss(nn.Module):
    """``GANLoss('vanilla', loss_weight=w)(logits, target_is_real, is_disc=False)``: mean(softplus(-x)) for a real target, mean(softplus(x)) for a
    fake one; multiplied by ``loss_weight`` unless ``is_disc`` (see the module docstring for where this definition comes from)."""

    def __init__(self, gan_type='vanilla', real_label_val=1.0, fake_label_val=0.0, loss_weight=1.0):
        super().__init__()
        if gan_type != 'vanilla' or real_label_val != 1.0 or fake_label_val != 0.0:
            raise NotImplementedError("only gan_type='vanilla' with labels 1 / 0 (configs/llff/fern_lg_joint_l1+gan.py)")
        self.loss_weight = loss_weight

    def forward(self, logits, target_is_real, is_disc=False):
        scale = 1.0 if is_disc else float(self.loss_weight)
        return vanilla_gan_loss(logits, bool(target_is_real), scale)


def vanilla_gan_loss(logits, target_is_real, scale=1.0):
    """scale * BCEWithLogitsLoss(logits, all ones | all zeros): k4_gan_loss_fwd / _bwd on CUDA fp32 logits, the tensor library elsewhere."""
    if _K4 and logits.is_cuda and logits.dtype == torch.float32:
        return _K4GanLoss.apply(logits, target_is_real, scale)
    target = torch.ones_like(logits) if target_is_real else torch.zeros_like(logits)
    return F.binary_cross_entropy_with_logits(logits, target) * scale
