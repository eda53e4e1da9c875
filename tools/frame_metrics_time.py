"""ms per frame evaluation (lib/utils.frame_metrics: SSIM + squared differences of a frame pair in one k4_frame_metrics call) against the same
formula written in torch-ROCm fp64 tensor operations (F.conv2d with the tap table), ALTERNATED call by call in one process.  GPU box.

    python tools/frame_metrics_time.py [--calls 200] [--budget-s 60] [--no-host] [--only NAME] [--hip-only]

Frames: 1008x756 channel-last, 4032x3024 channel-last and planar, seeded synthetic.  Every figure is the time between two device events around
one call, after a warm-up of both arms.  Where one tensor-library call takes so long that `--calls` pairs would not fit `--budget-s` seconds per
frame size, fewer pairs are run and the count is printed.  The host formula (scipy.signal.convolve2d, as the reference's rgb_ssim) is timed once per
size where scipy imports.  Floors: the two frames' bytes over the HBM bandwidth, and 110 fp64 FMAs per map entry (n = 11: five moments, two passes of
11 taps) over the fp64 vector rate.  Prints one JSON line per frame size."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.nn.functional as F
import nerf4k_amd  # noqa: F401,E402
from nerf4k_amd.lib import utils  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--calls', type=int, default=200)
ap.add_argument('--budget-s', type=float, default=60.0, help='seconds of alternated calls per frame size')
ap.add_argument('--no-host', action='store_true')
ap.add_argument('--only', default=None)
ap.add_argument('--hip-only', action='store_true', help='the HIP arm alone (for a kernel trace of its own)')
args = ap.parse_args()
dev = torch.device('cuda', 0)
HBM_BYTES_PER_S = 6.29e12           # measured float4 copy on an MI355X (8.0e12 is the specification)
FP64_FMA_PER_S = 78.6e12 / 2        # MI355X fp64 vector peak, 78.6 TFLOP/s
N, SIGMA = 11, 1.5
HOST_S = {}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def stats(v):
    v = sorted(v)
    return {'median_ms': round(statistics.median(v), 4), 'p10_ms': round(v[len(v) // 10], 4), 'p90_ms': round(v[len(v) * 9 // 10], 4), 'n': len(v)}


def torch_formula(a, b, taps):
    """The reference's formula on planar [3,H,W] fp32 device frames in fp64 tensor operations -> (ssim mean, mse), device scalars."""
    kv, kh = taps.reshape(1, 1, -1, 1), taps.reshape(1, 1, 1, -1)
    z = torch.stack([a, b, a * a, b * b, a * b]).double().reshape(15, 1, a.shape[1], a.shape[2])       # fp32 products, then fp64
    m = F.conv2d(F.conv2d(z, kv), kh).reshape(5, 3, z.shape[2] - N + 1, z.shape[3] - N + 1)
    mu0, mu1 = m[0], m[1]
    mu00, mu11, mu01 = mu0 * mu0, mu1 * mu1, mu0 * mu1
    s00, s11, s01 = (m[2] - mu00).clamp_min(0), (m[3] - mu11).clamp_min(0), m[4] - mu01
    s01 = torch.sign(s01) * torch.minimum(torch.sqrt(s00 * s11), s01.abs())
    c1, c2 = 0.01**2, 0.03**2
    q = ((2 * mu01 + c1) * (2 * s01 + c2)) / ((mu00 + mu11 + c1) * (s00 + s11 + c2))
    d = a - b
    return q.mean(), (d * d).double().mean()


def host_formula_seconds(a, b):
    try:
        import scipy.signal
    except ImportError:
        return None
    taps = utils.ssim_taps(N, SIGMA)

    def blur(z):
        return np.stack([scipy.signal.convolve2d(scipy.signal.convolve2d(z[..., i], taps[:, None], mode='valid'), taps[None, :], mode='valid')
                         for i in range(3)], -1)
    t0 = time.perf_counter()
    for z in (a, b, a**2, b**2, a * b):
        blur(z)
    return time.perf_counter() - t0


for name, (H, W), planar in (('1008x756 channel-last', (756, 1008), False), ('4032x3024 channel-last', (3024, 4032), False),
                             ('4032x3024 planar', (3024, 4032), True)):
    if args.only and args.only not in name:
        continue
    g = torch.Generator(device='cpu').manual_seed(H + W)
    a_cl = torch.rand(H, W, 3, generator=g)
    b_cl = (a_cl + 0.05 * torch.randn(H, W, 3, generator=g)).clamp(0, 1)
    a_pl, b_pl = a_cl.permute(2, 0, 1).contiguous().to(dev), b_cl.permute(2, 0, 1).contiguous().to(dev)
    a, b = (a_pl, b_pl) if planar else (a_cl.to(dev), b_cl.to(dev))
    taps = torch.from_numpy(utils.ssim_taps(N, SIGMA)).to(dev)

    def hip():
        return utils.frame_metrics(a, b)

    def lib():
        return torch_formula(a_pl, b_pl, taps)

    for _ in range(3):
        hip()
    torch.cuda.synchronize()
    res = {'frame': name, 'H': H, 'W': W}
    try:
        if args.hip_only:
            raise RuntimeError('not run (--hip-only)')
        first, _ = timed(lib)
        t1, got_lib = timed(lib)
    except RuntimeError as e:           # e.g. no fp64 convolution in the tensor library's backend
        t1, got_lib = None, None
        res['torch_fp64_error'] = str(e).splitlines()[0][:200]
    t_hip, got = timed(hip)
    pairs = args.calls if t1 is None else max(5, min(args.calls, int(args.budget_s * 1e3 / (t1 + t_hip))))
    hip_ms, lib_ms = [], []
    for _ in range(pairs):
        hip_ms.append(timed(hip)[0])
        if t1 is not None:
            lib_ms.append(timed(lib)[0])
    res['hip'] = stats(hip_ms)
    if t1 is not None:
        res['torch_fp64'] = stats(lib_ms)
        res['torch_minus_hip'] = stats([l - h for h, l in zip(hip_ms, lib_ms)])
        res['ssim_hip_minus_torch'] = float(got['ssim'] - got_lib[0])
        res['mse_hip_over_torch_minus_1'] = float(got['mse'] / got_lib[1] - 1)
    floor_hbm = 2 * H * W * 3 * 4 / HBM_BYTES_PER_S * 1e3
    floor_fma = 110 * (H - N + 1) * (W - N + 1) * 3 / FP64_FMA_PER_S * 1e3
    res['floor_hbm_ms'], res['floor_fp64_fma_ms'] = round(floor_hbm, 4), round(floor_fma, 4)
    res['binding_floor'] = 'fp64 FMA' if floor_fma > floor_hbm else 'HBM'
    res['hip_over_floor'] = round(res['hip']['median_ms'] / max(floor_hbm, floor_fma), 2)
    if not args.no_host:                # once per size
        if (H, W) not in HOST_S:
            s = host_formula_seconds(a_cl.numpy(), b_cl.numpy())
            HOST_S[(H, W)] = 'scipy does not import here' if s is None else round(s, 2)
        res['host_scipy_s'] = HOST_S[(H, W)]
    print(json.dumps(res), flush=True)
