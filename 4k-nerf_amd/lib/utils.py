"""Checkpoint helpers with the reference's formats (/root/reference/lib/utils.py:50-66).

DVGO/MPI checkpoints: ``{'global_step', 'model_kwargs', 'model_state_dict', 'optimizer_state_dict'}``
(run_sr.py:1173-1178).  Only what the render / training-step path needs is restated.  Frame evaluation: ``rgb_ssim`` with the
reference's signature (lib/utils.py:88-134) and ``frame_metrics`` (MSE, PSNR and SSIM of a frame pair in one pass) run on the device
(csrc/k4_metric.hip).  LPIPS: ``init_lpips`` / ``rgb_lpips`` with the reference's signatures (lib/utils.py:137-149) and ``frame_lpips`` for device
frames run lib/lpips.LPIPS (VGG only) on csrc/k4_vgg.hip and csrc/k4_lpips.hip.  Nothing is fetched: the caller registers the weights with
``load_lpips_weights`` first, and an unregistered metric raises ``NotImplementedError``.
"""
import numpy as np
import torch
import torch.nn as nn

from .masked_adam import MaskedAdam

to8b = lambda x: (255 * np.clip(x, 0, 1)).astype(np.uint8)     # lib/utils.py:19
mse2psnr = lambda x: -10. * torch.log10(x)


def to8b_device(x):
    """to8b for a device tensor: uint8 tensor of the same shape, packed on the GPU (k4_to8b) -- a 4K frame leaves the device
    as 36.6 MB instead of 146 MB of fp32."""
    from .. import _native as N
    xc = x.detach().float().contiguous()
    out = torch.empty(xc.shape, dtype=torch.uint8, device=xc.device)
    N.check(N.lib().k4_to8b(N.f32(xc), xc.numel(), N.ptr(out), N.stream()), 'k4_to8b')
    return out


def window_to_planes(hr, oy, ox, th, tw, dst):
    """dst[c, y, x] = hr[0, c, oy + y, ox + x] for a decoded window `hr` ([1, C, H, W] VIEW of the decoder's NHWC result) and a destination `dst` [C, th, tw]
    whose rows are contiguous (a tile of the frame, a slice of a gather buffer reshaped): one pass of k4_nhwc_window_to_planar instead of a channel-stride
    gather by slice assignment.  Falls back to the slice assignment for any other layout (CPU tensors of the gloo tests, other dtypes)."""
    C, H, W = int(hr.shape[1]), int(hr.shape[2]), int(hr.shape[3])
    ok = (hr.is_cuda and dst.is_cuda and hr.dtype == torch.float32 and dst.dtype == torch.float32 and C <= 4 and hr.shape[0] == 1
          and hr.stride(1) == 1 and hr.stride(3) == C and hr.stride(2) == W * C and dst.dim() == 3 and tuple(dst.shape) == (C, th, tw)
          and dst.stride(2) == 1 and th > 0 and tw > 0)
    if not ok:
        dst.copy_(hr[0, :, oy:oy + th, ox:ox + tw])
        return
    from .. import _native as N
    N.check(N.lib().k4_nhwc_window_to_planar(N.C.c_void_p(hr.data_ptr()), W, C, int(oy), int(ox), int(th), int(tw), N.C.c_void_p(dst.data_ptr()),
                                             int(dst.stride(0)), int(dst.stride(1)), N.stream()), 'k4_nhwc_window_to_planar')


def create_optimizer_or_freeze_model(model, cfg_train, global_step):
    """lib/utils.py:21-48: one param group per `lrate_<name>` entry of cfg_train whose attribute exists on the model;
    lr decays by 0.1 every `lrate_decay` k-steps; lr == 0 freezes the parameter.  cfg_train: attribute-style mapping
    (mmcv ConfigDict upstream; anything with .keys() and getattr works)."""
    decay = 0.1 ** (global_step / (cfg_train.lrate_decay * 1000))
    names = [key[len('lrate_'):] for key in cfg_train.keys() if key.startswith('lrate_')]
    param_group = []
    for name in names:
        target = getattr(model, name, None)
        if target is None:
            if hasattr(model, name):
                print(f'create_optimizer_or_freeze_model: param {name} not exist')
            continue
        lr = getattr(cfg_train, 'lrate_' + name) * decay
        if lr <= 0:
            print(f'create_optimizer_or_freeze_model: param {name} freeze')
            target.requires_grad = False        # (a plain attribute on an nn.Module, exactly as upstream)
            continue
        print(f'create_optimizer_or_freeze_model: param {name} lr {lr}')
        param_group.append({'params': target.parameters() if isinstance(target, nn.Module) else target,
                            'lr': lr, 'kname': name,
                            'skip_zero_grad': name in cfg_train.skip_zero_grad_fields})
    return MaskedAdam(param_group)


def load_checkpoint(model, optimizer, ckpt_path, no_reload_optimizer):
    ckpt = torch.load(ckpt_path, map_location='cpu', weights_only=False)
    start = ckpt['global_step']
    model.load_state_dict(ckpt['model_state_dict'])
    if not no_reload_optimizer:
        optimizer.load_state_dict(ckpt['optimizer_state_dict'])
    return model, optimizer, start


def load_model(model_class, ckpt_path):
    ckpt = torch.load(ckpt_path, map_location='cpu', weights_only=False)
    model = model_class(**ckpt['model_kwargs'])
    model.load_state_dict(ckpt['model_state_dict'])
    return model


def model_from_checkpoint_dict(ckpt):
    """Same as load_model for an in-memory checkpoint dict (synthetic scenes)."""
    from . import dvgo, dmpigo, dcvgo, dbvgo, dvqgo
    cls = {'DirectMPIGO': dmpigo.DirectMPIGO, 'DirectVoxGO': dvgo.DirectVoxGO,
           'DirectContractedVoxGO': dcvgo.DirectContractedVoxGO, 'DirectBiVoxGO': dbvgo.DirectBiVoxGO, 'DirectQVGO': dvqgo.DirectQVGO}[ckpt['model_class']]
    model = cls(**ckpt['model_kwargs'])
    model.load_state_dict(ckpt['model_state_dict'])
    return model


# ---- frame evaluation (csrc/k4_metric.hip) ---------------------------------------------------------------------------
def ssim_taps(filter_size, filter_sigma):
    """The 1D Gaussian of lib/utils.py:100-104 as float64, by the reference's own numpy expression (bit for bit: the device sums are
    held to 1e-10 of the reference's map).  Symmetric for odd and even sizes."""
    half = filter_size // 2
    shift = (2 * half - filter_size + 1) / 2
    taps = np.exp(-0.5 * ((np.arange(filter_size) - half + shift) / filter_sigma)**2)
    taps /= np.sum(taps)
    return taps


def _metric_image(img, what, channel_last=False):
    """-> (device fp32 tensor, H, W, pixel stride, channel stride) of a frame given channel-last [H,W,3] or planar [3,H,W] / [1,3,H,W]
    (any view of either whose rows are dense, e.g. the decoder's [1,3,H,W] view of an NHWC result).  channel_last: the frame came as a numpy
    array, which is [H,W,3] by the reference's contract; a [3,H,3] TENSOR could be either layout and is refused."""
    from .. import _native as N
    if not isinstance(img, torch.Tensor):
        raise N.K4Error(f'{what}: expected a numpy array or a torch tensor, got {type(img).__name__}')
    if img.dtype != torch.float32:          # float64 frames would silently change the reference's fp32 rounding of img**2
        raise N.K4Error(f'{what}: expected float32, got {img.dtype}')
    if not img.is_cuda:
        raise N.K4Error(f'{what}: tensor must be on the GPU (no CPU path exists for the frame metrics)')
    planar = None
    if img.dim() == 4 and img.shape[0] == 1 and img.shape[1] == 3:          # the four-dimensional form is planar only
        img, planar = img[0], True
    if img.dim() != 3:
        raise N.K4Error(f'{what}: expected [H,W,3], [3,H,W] or [1,3,H,W], got {tuple(img.shape)}')
    if planar is None:
        if img.shape[-1] == 3 and img.shape[0] == 3 and not channel_last:
            raise N.K4Error(f'{what}: a {tuple(img.shape)} tensor is both [H,W,3] and [3,H,W]; pass the planar frame as [1,3,H,W] '
                            f'or the channel-last one as a numpy array')
        planar = img.shape[-1] != 3
    if not planar:                          # channel-last, as the reference asserts (lib/utils.py:95-96)
        H, W = int(img.shape[0]), int(img.shape[1])
        sy, sx, sc = img.stride()
    elif img.shape[0] == 3:
        H, W = int(img.shape[1]), int(img.shape[2])
        sc, sy, sx = img.stride()
    else:
        raise N.K4Error(f'{what}: expected [H,W,3], [3,H,W] or [1,3,H,W], got {tuple(img.shape)}')
    if sx < 1 or sc < 1 or (H > 1 and sy != W * sx):
        raise N.K4Error(f'{what}: rows must be dense (strides {tuple(img.stride())} of shape {tuple(img.shape)})')
    return img, H, W, int(sx), int(sc)


def _frame_metric_sums(img0, img1, clamp0, clamp1, max_val, filter_size, filter_sigma, k1, k2, want_map, channel_last=(False, False)):
    """One k4_frame_metrics call -> (sums [2] fp64 device tensor: sum of the SSIM map, sum of squared differences; the map or None; H, W)."""
    from .. import _native as N
    a, H, W, ps0, cs0 = _metric_image(img0, 'img0', channel_last[0])
    b, H1, W1, ps1, cs1 = _metric_image(img1, 'img1', channel_last[1])
    if (H, W) != (H1, W1):
        raise N.K4Error(f'frames differ in size: {H}x{W} against {H1}x{W1}')
    if a.device != b.device:
        raise N.K4Error(f'frames are on different devices: {a.device}, {b.device}')
    n = int(filter_size)
    if n < 1 or n > 31:
        raise N.K4Error(f'filter_size {filter_size} outside [1, 31]')
    if H < n or W < n:
        raise N.K4Error(f'a {H}x{W} frame is smaller than the {n}-tap filter')
    taps = np.ascontiguousarray(ssim_taps(n, filter_sigma), dtype=np.float64)
    c1, c2 = float((k1 * max_val)**2), float((k2 * max_val)**2)             # lib/utils.py:128-129
    lib = N.lib()
    with torch.cuda.device(a.device):
        ws = torch.empty(int(lib.k4_frame_metrics_workspace_bytes(H, W, n)), dtype=torch.uint8, device=a.device)
        sums = torch.empty(2, dtype=torch.float64, device=a.device)
        ssim_map = torch.empty(H - n + 1, W - n + 1, 3, dtype=torch.float64, device=a.device) if want_map else None
        N.check(lib.k4_frame_metrics(N.C.c_void_p(a.data_ptr()), ps0, cs0, int(bool(clamp0)), N.C.c_void_p(b.data_ptr()), ps1, cs1, int(bool(clamp1)),
                                     H, W, taps.ctypes.data_as(N.C.POINTER(N.C.c_double)), n, c1, c2,
                                     N.ptr(ssim_map), N.ptr(ws), N.ptr(sums), N.stream()), 'k4_frame_metrics')
    return sums, ssim_map, H, W


def _to_device_frame(x, device=None):
    """numpy float32 [H,W,3] -> device tensor (uploaded); tensors pass through."""
    if isinstance(x, np.ndarray):
        from .. import _native as N
        if x.dtype != np.float32:
            raise N.K4Error(f'expected a float32 frame, got {x.dtype}')
        if x.ndim != 3 or x.shape[-1] != 3:
            raise N.K4Error(f'expected a [H,W,3] array, got {x.shape}')
        return torch.from_numpy(np.ascontiguousarray(x)).to(device if device is not None else 'cuda')
    return x


def rgb_ssim(img0, img1, max_val, filter_size=11, filter_sigma=1.5, k1=0.01, k2=0.03, return_map=False):
    """lib/utils.py:88-134 on the device.  numpy float32 [H,W,3] frames are uploaded and the result is numpy (np.float64, or the float64 map):
    drop-in for run_sr.py:147,1134.  Device float32 tensors (channel-last [H,W,3] or planar [3,H,W] / [1,3,H,W]) give device float64 tensors
    without a host synchronisation.  Any other dtype, a size mismatch or a frame smaller than the filter raises."""
    as_numpy = isinstance(img0, np.ndarray) and isinstance(img1, np.ndarray)
    dev = next((x.device for x in (img0, img1) if isinstance(x, torch.Tensor) and x.is_cuda), None)
    a, b = _to_device_frame(img0, dev), _to_device_frame(img1, dev)
    sums, ssim_map, H, W = _frame_metric_sums(a, b, False, False, max_val, filter_size, filter_sigma, k1, k2, return_map,
                                              (isinstance(img0, np.ndarray), isinstance(img1, np.ndarray)))
    if return_map:
        return ssim_map.cpu().numpy() if as_numpy else ssim_map
    ssim = sums[0] / float((H - filter_size + 1) * (W - filter_size + 1) * 3)
    return np.float64(ssim.item()) if as_numpy else ssim


def frame_metrics(pred, gt, max_val=1.0, clamp_pred=False, return_map=False):
    """{'mse', 'psnr', 'ssim'[, 'ssim_map']} of a frame pair as device float64 tensors from ONE pass over the two frames (what a validation
    loop computes on the decoder's output, run_sr.py:1131-1134: clamp_pred=True clamps `pred` to [0, 1] in the load).  mse = mean (pred - gt)^2,
    psnr = 20 log10(max_val) - 10 log10(mse) (run_sr.py:1133 with max_val = 1), ssim = rgb_ssim(pred, gt, max_val) with the default filter."""
    dev = next((x.device for x in (pred, gt) if isinstance(x, torch.Tensor) and x.is_cuda), None)
    a, b = _to_device_frame(pred, dev), _to_device_frame(gt, dev)
    sums, ssim_map, H, W = _frame_metric_sums(a, b, clamp_pred, False, max_val, 11, 1.5, 0.01, 0.03, return_map,
                                              (isinstance(pred, np.ndarray), isinstance(gt, np.ndarray)))
    mse = sums[1] / float(H * W * 3)
    out = {'mse': mse, 'psnr': 20. * float(np.log10(max_val)) - 10. * torch.log10(mse), 'ssim': sums[0] / float((H - 10) * (W - 10) * 3)}
    if return_map:
        out['ssim_map'] = ssim_map
    return out


# ---- LPIPS (lib/lpips.py on csrc/k4_vgg.hip + csrc/k4_lpips.hip) ------------------------------------------------------
__LPIPS__ = {}                  # net_name -> module, as lib/utils.py:137
_LPIPS_WEIGHTS = None           # (state dict, lin state dict or None) registered by load_lpips_weights


def load_lpips_weights(obj):
    """Register the LPIPS-VGG weights for this process: a state dict with the keys of lib/lpips.LPIPS, a ``(torchvision vgg16 state dict, lin state
    dict)`` pair (``lin<k>.model.1.weight`` or ``lins.<k>.model.1.weight``: the `lpips` package's weights/v0.1/vgg.pth), a path to a ``torch.save``d one
    of those, or ``None`` to clear.  Nothing is fetched.  Missing layers raise ``KeyError`` and wrong shapes ``ValueError`` here, not at the first frame."""
    global _LPIPS_WEIGHTS
    __LPIPS__.clear()
    if obj is None:
        _LPIPS_WEIGHTS = None
        return
    if not isinstance(obj, (dict, tuple, list)):
        obj = torch.load(obj, map_location='cpu', weights_only=True)
    sd, lin = (obj[0], obj[1]) if isinstance(obj, (tuple, list)) else (obj, None)
    from . import lpips
    lpips.LPIPS(net='vgg', version='0.1', verbose=False).load_lpips_state_dict(sd, lin)
    _LPIPS_WEIGHTS = (sd, lin)


def lpips_weights_registered():
    return _LPIPS_WEIGHTS is not None


LPIPS_ALEX_MISSING = ("LPIPS (alex) is not provided: the `lpips` package's AlexNet backbone needs kernels this package does not have "
                      "(only net_name='vgg', eval_lpips_vgg)")
LPIPS_WEIGHTS_MISSING = ("LPIPS (vgg) needs the `lpips` package's weights, which are never fetched: register them first with "
                         'lib.utils.load_lpips_weights(state dict | (vgg16 state dict, lin state dict) | path)')


def init_lpips(net_name, device):
    """lib/utils.py:138-142: the module is built from the weights registered with ``load_lpips_weights``."""
    assert net_name in ['alex', 'vgg']
    if net_name == 'alex':
        raise NotImplementedError(LPIPS_ALEX_MISSING)
    if _LPIPS_WEIGHTS is None:
        raise NotImplementedError(LPIPS_WEIGHTS_MISSING)
    from . import lpips
    print(f'init_lpips: lpips_{net_name}')
    return lpips.LPIPS(net=net_name, version='0.1', verbose=False).load_lpips_state_dict(*_LPIPS_WEIGHTS).eval().to(device)


def rgb_lpips(np_gt, np_im, net_name, device):
    """lib/utils.py:144-149: numpy [H,W,3] frames in [0, 1] -> Python float (one host synchronisation, the reference's ``.item()``)."""
    if net_name not in __LPIPS__:
        __LPIPS__[net_name] = init_lpips(net_name, device)
    gt = torch.from_numpy(np_gt).permute([2, 0, 1]).contiguous().to(device)
    im = torch.from_numpy(np_im).permute([2, 0, 1]).contiguous().to(device)
    return __LPIPS__[net_name](gt, im, normalize=True).item()


def frame_lpips(pred, gt, clamp_pred=False):
    """The device form of ``rgb_lpips(gt, pred, 'vgg', device)``: frames are device float32 tensors, channel-last [H,W,3] (the marcher's) or planar
    [3,H,W] / [1,3,H,W] (the decoder's), in [0, 1]; clamp_pred clamps `pred` first (run_sr.py:1131).  Returns a device float32 scalar without a
    host synchronisation."""
    def planar(img, what):
        v, H, W, _, _ = _metric_image(img, what)
        if tuple(v.shape) == (H, W, 3) and not (img.dim() == 4):
            v = v.permute(2, 0, 1)
        return v.contiguous()
    a, b = planar(pred, 'pred'), planar(gt, 'gt')
    if clamp_pred:
        a = a.clamp(0, 1)
    if 'vgg' not in __LPIPS__:
        __LPIPS__['vgg'] = init_lpips('vgg', a.device)
    return __LPIPS__['vgg'](b, a, normalize=True).reshape(())
