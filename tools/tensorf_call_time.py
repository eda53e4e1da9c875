"""ms per TensoRFGrid lookup, forward and backward (lib/grid.TensoRFGrid: k4_tensorf_sample / k4_tensorf_sample_backward), against the reference's own
expression (lib/grid.py:241-256: six F.grid_sample, three products, a cat and a mm) run as torch-ROCm eager operations on the same GPU -- the product
has no such path; it is the stand-in for the reference on this GPU.  The two are ALTERNATED call by call in one process.  GPU box.

    python tools/tensorf_call_time.py [--calls 200] [--points 200000] [--n-comp 48] [--channels 12] [--world 160]

Points: consecutive samples along random rays through 1.05 x the box (a training batch's order), seeded.  Every figure is the time between two device
events around one call (forward: the lookup; backward: autograd's backward of sum(out * grad_out), gradient buffers included), after a warm-up of
both arms.  Prints the shape, the agreement of the two arms and one JSON line."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
import nerf4k_amd  # noqa: F401,E402
from nerf4k_amd.lib import grid as kgrid  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--calls', type=int, default=200)
ap.add_argument('--points', type=int, default=200000)
ap.add_argument('--n-comp', type=int, default=48)
ap.add_argument('--channels', type=int, default=12)
ap.add_argument('--world', type=int, default=160)
ap.add_argument('--warmup', type=int, default=5)
args = ap.parse_args()
dev = torch.device('cuda', 0)
torch.manual_seed(0)
W = args.world
g = kgrid.TensoRFGrid(args.channels, [W, W, W], [-1., -1., -1.], [1., 1., 1.], {'n_comp': args.n_comp}).to(dev)
per_ray = 200
n_rays = (args.points + per_ray - 1) // per_ray
o = (torch.rand([n_rays, 1, 3], device=dev) * 2 - 1) * 1.05
d = torch.nn.functional.normalize(torch.randn([n_rays, 1, 3], device=dev), dim=-1)
t = torch.linspace(-0.6, 0.6, per_ray, device=dev)[None, :, None]
pts = (o * 0.4 + d * t).reshape(-1, 3)[:args.points].contiguous()
go = torch.randn([pts.shape[0], args.channels], device=dev)


def reference_expression(xyz):
    """lib/grid.py:178-196, 241-268 as written upstream, on this module's parameters."""
    xyz = xyz.reshape(1, 1, -1, 3)
    ind = (xyz - g.xyz_min) / (g.xyz_max - g.xyz_min) * 2 - 1
    ind = torch.cat([ind, torch.zeros_like(ind[..., [0]])], dim=-1)
    gs = lambda p, idx: F.grid_sample(p, ind[:, :, :, idx], mode='bilinear', align_corners=True).flatten(0, 2).T
    xy, xz, yz = gs(g.xy_plane, [1, 0]), gs(g.xz_plane, [2, 0]), gs(g.yz_plane, [2, 1])
    x, y, z = gs(g.x_vec, [3, 0]), gs(g.y_vec, [3, 1]), gs(g.z_vec, [3, 2])
    if g.channels > 1:
        return torch.mm(torch.cat([xy * z, xz * y, yz * x], dim=-1), g.f_vec)
    return ((xy * z).sum(-1) + (xz * y).sum(-1) + (yz * x).sum(-1))[:, None]


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), r


def one(arm):
    for p in g.parameters():
        p.grad = None
    fwd, out = timed(lambda: (g(pts) if arm == 'hip' else reference_expression(pts)).reshape(pts.shape[0], -1))
    bwd, _ = timed(lambda: out.backward(go))
    return fwd, bwd, out.detach(), [p.grad.detach().clone() for p in g.parameters()]


for _ in range(args.warmup):
    hip, ref = one('hip'), one('ref')
scale = float(ref[2].abs().max())
print(f'shape: {pts.shape[0]} points, n_comp {args.n_comp}, C = {args.channels}, world {W}^3; factors {sum(p.numel() for p in g.parameters()) * 4 / 2**20:.1f} MiB')
print(f'agreement: output max |hip - eager| = {float((hip[2] - ref[2]).abs().max()):.3e} at scale {scale:.3e}; gradients '
      + ', '.join(f'{float((a - b).abs().max()):.2e}/{float(b.abs().max()):.2e}' for a, b in zip(hip[3], ref[3])))
T = {'hip': ([], []), 'ref': ([], [])}
for _ in range(args.calls):
    for arm in ('hip', 'ref'):
        f, b = one(arm)[:2]
        T[arm][0].append(f)
        T[arm][1].append(b)


def stats(v):
    q = statistics.quantiles(v, n=10)
    return {'median': round(statistics.median(v), 4), 'p10': round(q[0], 4), 'p90': round(q[-1], 4)}


res = {'points': pts.shape[0], 'n_comp': args.n_comp, 'channels': args.channels, 'world': W, 'calls': args.calls}
for i, what in enumerate(('forward', 'backward')):
    res[what] = {'hip_ms': stats(T['hip'][i]), 'eager_ms': stats(T['ref'][i]),
                 'paired_eager_minus_hip_ms': stats([r - h for h, r in zip(T['hip'][i], T['ref'][i])])}
print(json.dumps(res))
