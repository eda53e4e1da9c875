"""One full coarse-stage iteration of the direct-colour DirectVoxGO (zero_grad, render + loss + backward, MaskedAdam.step): the fused step
(train_ops.dvgo_direct_render_loss: k4_direct_train_fwd / _bwd) against the staged path (model(..., k4_staged=True) under autograd plus the eager
loss lines of run_sr.py:523-546), the parent commit's code and therefore the yardstick.
Model: scene.make_lego_checkpoint(rgbnet_dim=0, num_voxels=1024000, fast_color_thres=1e-7, alpha_init=1e-6); 8192 rays per iteration drawn from 800x800
scene.lego_pose views (a fresh batch per iteration, the same batches for both paths).  Two states: the seeded blob scene, and the same scene with
density.grid zeroed -- the recipe's first iterations, where every in-mask sample is shaded.  Each path steps its own copy of the model with its own
optimizer (learning rate 1e-6: the state stays what it was); the two are ALTERNATED iteration by iteration in one process after a warm-up; wall time
between device synchronisations.  Reported: medians, the paired difference staged - fused with p10 / p90, host synchronisations per iteration
(torch's sync debug mode) and kernel launches per iteration (torch.profiler), both counted on one iteration outside the timed ones, and the
backward's atomic bytes per iteration (128 B per shaded sample; the 32 B of a sample only the weight filter drops are left out: a lower bound).
    python tools/direct_train_time.py [--iters 200] [--rays 8192] [--views 4] [--voxels 1024000] [--out FILE.md]"""
import argparse
import copy
import os
import sys
import time
import warnings
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.nn.functional as F
import nerf4k_amd  # noqa: F401
from nerf4k_amd import scene
from nerf4k_amd.lib import utils, dvgo, train_ops

ap = argparse.ArgumentParser()
ap.add_argument('--iters', type=int, default=200)
ap.add_argument('--rays', type=int, default=8192)
ap.add_argument('--views', type=int, default=4)
ap.add_argument('--hw', type=int, default=800)
ap.add_argument('--voxels', type=int, default=1024000)
ap.add_argument('--out', default=None)
args = ap.parse_args()
dev = torch.device('cuda', 0)
WEIGHTS = dict(weight_main=1.0, weight_entropy_last=0.01, weight_rgbper=0.1)             # configs/default.py, coarse stage
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def pct(v):
    v = np.asarray(v)
    return f'{np.median(v):.3f} ms (p10 {np.percentile(v, 10):.3f}, p90 {np.percentile(v, 90):.3f})'


class Cfg(dict):
    __getattr__ = dict.__getitem__


def eager_loss(out, target, n_rays, weight_main, weight_entropy_last, weight_rgbper):
    loss = weight_main * F.mse_loss(out['rgb_marched'], target)
    pout = out['alphainv_last'].clamp(1e-6, 1 - 1e-6)
    loss = loss + weight_entropy_last * -(pout * torch.log(pout) + (1 - pout) * torch.log(1 - pout)).mean()
    rgbper = (out['raw_rgb'] - target[out['ray_id']]).pow(2).sum(-1)
    return loss + weight_rgbper * (rgbper * out['weights'].detach()).sum() / n_rays


def fused_iter(model, opt, ro, rd, tgt, rk):
    opt.zero_grad(set_to_none=True)
    out = train_ops.dvgo_direct_render_loss(model, ro, rd, tgt, **rk, **WEIGHTS)
    out['total'].backward()
    opt.step()
    return out


def staged_iter(model, opt, ro, rd, tgt, rk):
    opt.zero_grad(set_to_none=True)
    out = model(ro, rd, rd, k4_staged=True, **rk)
    eager_loss(out, tgt, len(ro), **WEIGHTS).backward()
    opt.step()
    return out


def timed(fn, *a):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(*a)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def count_syncs(fn, *a):
    try:
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode(1)
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter('always')
            fn(*a)
        return sum('synchroniz' in str(x.message) for x in w)
    except Exception as e:                                # noqa: BLE001
        return f'not measured ({type(e).__name__})'
    finally:
        torch.cuda.set_sync_debug_mode(0)


def count_launches(fn, *a):
    try:
        from torch.profiler import profile, ProfilerActivity
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn(*a)
            torch.cuda.synchronize()
        ev = [e for e in prof.events() if str(e.device_type).endswith('CUDA')]
        kernels = [e for e in ev if not e.name.lower().startswith(('memcpy', 'memset'))]
        return f'{len(kernels)} kernels + {len(ev) - len(kernels)} memset / memcpy' if ev else 'not measured (the profiler recorded no device event)'
    except Exception as e:                                # noqa: BLE001
        return f'not measured ({type(e).__name__})'


ck = scene.make_lego_checkpoint(rgbnet_dim=0, num_voxels=args.voxels, fast_color_thres=1e-7, alpha_init=1e-6)
rk = {k: ck['render_kwargs'][k] for k in ('near', 'far', 'bg', 'stepsize')}
H = W = args.hw
K = scene.lego_K(H, W)
ros, rds = [], []
for v in range(args.views):
    ro, rd, _ = dvgo.get_rays_of_a_view(H, W, K, torch.Tensor(scene.lego_pose(theta_deg=360. * v / args.views)), False, inverse_y=False, flip_x=False, flip_y=False)
    ros.append(ro.reshape(-1, 3).to(dev))
    rds.append(rd.reshape(-1, 3).to(dev))
ro_all, rd_all = torch.cat(ros), torch.cat(rds)
g = torch.Generator().manual_seed(11)
warm = 5
batches = [torch.randint(len(ro_all), [args.rays], generator=g).to(dev) for _ in range(args.iters + warm + 2)]
tgt_all = torch.rand([len(ro_all), 3], generator=g).to(dev)
say(f'DirectVoxGO rgbnet_dim=0, {args.voxels} voxels, fast_color_thres 1e-7, alpha_init 1e-6, stepsize {rk["stepsize"]}; {args.rays} rays per iteration from '
    f'{args.views} views of {W}x{H}; {args.iters} alternated iterations per path after {warm} warm-up iterations; wall time between device synchronisations')

for state in ('seeded blob scene', 'density.grid zeroed (every in-mask sample shaded)'):
    base = utils.model_from_checkpoint_dict(ck).to(dev)
    if state.startswith('density'):
        with torch.no_grad():
            base.density.grid.zero_()
    models = {'fused': base, 'staged': copy.deepcopy(base)}
    fns = {'fused': fused_iter, 'staged': staged_iter}
    opts = {k: utils.create_optimizer_or_freeze_model(m, Cfg(lrate_decay=20, lrate_density=1e-6, lrate_k0=1e-6, skip_zero_grad_fields=['density', 'k0']), 0)
            for k, m in models.items()}
    for k, m in models.items():
        opts[k].set_pervoxel_lr(torch.ones_like(m.density.grid))
    ms = {'fused': [], 'staged': []}
    with torch.enable_grad():
        for i in range(warm + args.iters):
            b = batches[i]
            ro, rd, tgt = ro_all[b], rd_all[b], tgt_all[b]
            for k in ('fused', 'staged'):
                t = timed(fns[k], models[k], opts[k], ro, rd, tgt, rk)
                if i >= warm:
                    ms[k].append(t)
        b = batches[-1]
        ro, rd, tgt = ro_all[b], rd_all[b], tgt_all[b]
        syncs = {k: count_syncs(fns[k], models[k], opts[k], ro, rd, tgt, rk) for k in fns}
        b = batches[-2]
        ro, rd, tgt = ro_all[b], rd_all[b], tgt_all[b]
        launches = {k: count_launches(fns[k], models[k], opts[k], ro, rd, tgt, rk) for k in fns}
        out = fused_iter(models['fused'], opts['fused'], ro, rd, tgt, rk)
    shaded = int(out['n_shaded'].sum())
    f, s = np.asarray(ms['fused']), np.asarray(ms['staged'])
    say(f'state: {state}')
    say(f'  shaded samples per iteration {shaded:,} ({shaded / args.rays:.0f} per ray): atomic bytes of the fused backward {shaded * 128 / 1e6:.1f} MB '
        f'(32 float adds = 128 B per shaded sample; a lower bound: the 8 adds = 32 B of an alpha-passing sample the weight filter drops are not counted)')
    say(f'  fused : {pct(f)}; host synchronisations {syncs["fused"]}; launches {launches["fused"]}')
    say(f'  staged: {pct(s)}; host synchronisations {syncs["staged"]}; launches {launches["staged"]}')
    say(f'  paired difference staged - fused: {pct(s - f)}; staged / fused = {np.median(s) / np.median(f):.2f}x (ratio of medians)')
    d = float((models['fused'].density.grid.detach() - models['staged'].density.grid.detach()).abs().max())
    say(f'  after {warm + args.iters + 3} steps at lr 1e-6 the two copies differ by at most {d:.2e} in density.grid')
if args.out:
    with open(args.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')
