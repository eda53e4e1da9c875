"""DirectBiVoxGO (lib/dbvgo.py) render time: an 800x800 frame of a seeded two-grid scene (default 160^3, stepsize 0.5), timed with HIP events:
the fused inference call (k4_march_bivox_fwd, one launch for the whole frame, no workspace) against the staged path in chunks of 8192 rays as the
reference's render loop evaluates it (run_sr.py:121-124).  The two are timed INTERLEAVED (fused, staged, fused, staged, ...) so that clock and
cache state drift hits both alike; medians over the repetitions.  Prints frame times, Mrays/s, the eight sample counters and the largest
fused - staged difference, for the default rgbnet (width 128, both passes) and, with --all, for width 64, a background without MLP and the
coarse colour grids, which shows how much of the fused call is the per-lane fp32 rgbnet.
    python tools/dbvgo_call_time.py [--voxels 160] [--chunk 8192] [--reps 5] [--all] [--out FILE.md]"""
import argparse
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import nerf4k_amd  # noqa: F401
from nerf4k_amd import scene
from nerf4k_amd.lib import utils, dvgo

ap = argparse.ArgumentParser()
ap.add_argument('--voxels', type=int, default=160)
ap.add_argument('--chunk', type=int, default=8192)
ap.add_argument('--reps', type=int, default=5)
ap.add_argument('--H', type=int, default=800)
ap.add_argument('--W', type=int, default=800)
ap.add_argument('--all', action='store_true')
ap.add_argument('--out', default=None)
args = ap.parse_args()
dev = torch.device('cuda', 0)
H, W = args.H, args.W
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def run(tag, **cfg):
    ck = scene.make_bivox_checkpoint(num_voxels=args.voxels ** 3, **cfg)
    model = utils.model_from_checkpoint_dict(ck).to(dev).eval()
    rk = ck['render_kwargs']
    pose = torch.from_numpy(scene.unbounded_poses()[1]).to(dev)
    with torch.no_grad():
        ro, rd, vd = [x.reshape(-1, 3).contiguous() for x in dvgo.get_rays_of_a_view(H, W, scene.unbounded_K(H, W), pose, False, False, False, False)]
        n_rays = ro.shape[0]

        def fused():
            return model(ro, rd, vd, **rk)

        def staged():
            return [model(ro[s:s + args.chunk], rd[s:s + args.chunk], vd[s:s + args.chunk], k4_staged=True, **rk) for s in range(0, n_rays, args.chunk)]

        def once(fn):
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            r = fn()
            b.record()
            torch.cuda.synchronize()
            return a.elapsed_time(b), r
        ms_f, ms_s = [], []
        for i in range(args.reps + 1):                  # the first round warms caches and plans
            tf, out_f = once(fused)
            ts, out_s = once(staged)
            if i:
                ms_f.append(tf)
                ms_s.append(ts)
        cnt = torch.zeros(8, dtype=torch.int64, device=dev)
        model(ro, rd, vd, k4_counters=cnt, **rk)
        c = cnt.cpu().tolist()
        n_staged = sum(o['ray_id'].shape[0] for o in out_s)
        d_rgb = float((out_f['rgb_marched'] - torch.cat([o['rgb_marched'] for o in out_s])).abs().max())
        d_dep = float((out_f['depth'] - torch.cat([o['depth'] for o in out_s])).abs().max())
        T = out_f['alphainv_last']
        mean_T = float((T[:n_rays] * T[n_rays:]).mean())
    f, s = float(np.median(ms_f)), float(np.median(ms_s))
    say(f'{tag}: DirectBiVoxGO {args.voxels}^3, {W}x{H} ({n_rays} rays), N_outer {model._n_outer(rk["stepsize"])[1]}, mean T_fg*T_bg {mean_T:.3f}')
    say(f'  fused (1 launch, workspace 0 bytes): median {f:.2f} ms per frame ({min(ms_f):.2f} .. {max(ms_f):.2f}, {args.reps} runs) = {n_rays / f / 1e3:.1f} Mrays/s')
    say(f'  staged ({args.chunk}-ray chunks): median {s:.1f} ms per frame ({min(ms_s):.1f} .. {max(ms_s):.1f}) = {n_rays / s / 1e3:.2f} Mrays/s; '
        f'fused is {s / f:.2f}x')
    say(f'  counters fg: in-bbox {c[0]}, mask-pass {c[1]}, alpha-pass {c[2]}, shaded {c[3]}; bg: sampled {c[4]}, mask-pass {c[5]}, alpha-pass {c[6]}, '
        f'shaded {c[7]} (staged shaded {n_staged})')
    say(f'  max |fused - staged|: rgb {d_rgb:.2e}, depth {d_dep:.2e}')


run('width 128, depth 3, 12 channels', rgbnet_dim=12, rgbnet_width=128)
if args.all:
    run('width 64, depth 3, 12 channels', rgbnet_dim=12, rgbnet_width=64)
    run('width 128 foreground, background without MLP', rgbnet_dim=12, rgbnet_width=128, bg_use_mlp=False)
    run('coarse (no rgbnet)', rgbnet_dim=0)
if args.out:
    with open(args.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')
