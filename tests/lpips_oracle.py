"""Checker for 4k-nerf_amd/lib/lpips.py: LPIPS-VGG 0.1 as a plain functional restatement in a chosen dtype, on the CPU.

    evaluate(sd, in0, in1, normalize, dtype) -> {'total': [B], 'taps': [5][B], 'feats': [5] of ([B, C, h, w], [B, C, h, w])}

`sd` has the module's own keys (lpips.seeded_lpips_state_dict); in0, in1 are [B, 3, H, W] batches of image pairs (the pairs are independent: a batch
only shares the convolution calls).  tests/test_lpips_cpu.py holds this against an independently built nn.Sequential VGG16 + NetLinLayer modules."""
import torch
import torch.nn.functional as F

SLICES = ((0, 2), (5, 7), (10, 12, 14), (17, 19, 21), (24, 26, 28))
CHNS = (64, 128, 256, 512, 512)
EPS = 1e-10


def features(sd, x, dtype):
    """x [B, 3, H, W], already scaled -> the five tapped post-ReLU images."""
    out = []
    for s, idx in enumerate(SLICES, 1):
        if s > 1:
            x = F.max_pool2d(x, 2, 2)
        for i in idx:
            x = torch.relu(F.conv2d(x, sd[f'net.slice{s}.{i}.weight'].to(dtype), sd[f'net.slice{s}.{i}.bias'].to(dtype), 1, 1))
        out.append(x)
    return out


def head(f0, f1, w):
    """f0, f1 [B, C, h, w], w [C] -> [B]: the tap's value per pair."""
    n0 = f0 / (torch.sqrt((f0 * f0).sum(1, keepdim=True)) + EPS)
    n1 = f1 / (torch.sqrt((f1 * f1).sum(1, keepdim=True)) + EPS)
    d = (n0 - n1) ** 2
    return (d * w.reshape(1, -1, 1, 1)).sum(1).mean((1, 2))


def scale_input(sd, x, normalize, dtype):
    shift, scale = sd['scaling_layer.shift'].to(dtype).reshape(1, 3, 1, 1), sd['scaling_layer.scale'].to(dtype).reshape(1, 3, 1, 1)
    x = x.to(dtype)
    if normalize:
        x = 2 * x - 1
    return (x - shift) / scale


def scale_input_folded(sd, x, normalize, dtype):
    """The form the product hands to k4_vgg_conv1_1: (x - mean) / std with 2x - 1 folded into mean = (1 + shift) / 2, std = scale / 2."""
    shift, scale = sd['scaling_layer.shift'].to(dtype).reshape(1, 3, 1, 1), sd['scaling_layer.scale'].to(dtype).reshape(1, 3, 1, 1)
    mean, std = ((1 + shift) / 2, scale / 2) if normalize else (shift, scale)
    return (x.to(dtype) - mean) / std


def evaluate(sd, in0, in1, normalize=False, dtype=torch.float64, folded=False):
    B = in0.shape[0]
    sc = scale_input_folded if folded else scale_input
    with torch.no_grad():
        fs = features(sd, torch.cat([sc(sd, in0, normalize, dtype), sc(sd, in1, normalize, dtype)]), dtype)
        feats = [(f[:B], f[B:]) for f in fs]
        taps = [head(f0, f1, sd[f'lin{k}.model.1.weight'].to(dtype).reshape(-1)) for k, (f0, f1) in enumerate(feats)]
        total = taps[0]
        for t in taps[1:]:
            total = total + t
    return {'total': total, 'taps': taps, 'feats': feats}
