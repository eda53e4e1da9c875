"""DirectQVGO (lib/dvqgo.py) call times on a seeded codebook scene, from HIP events:
  (a) the one-launch frame (k4_march_vq_fwd) at 1008x756, per call;
  (b) the codeword lookup (VQGrid.forward, eval mode) on the frame's shaded points against the reference's expressions as eager tensor-library
      operations on device tensors (the restatement of tests/vq_oracle.py), both in the 8192-ray chunks run.py's loop would hand them -- the
      expression's one-hot tensor does not fit for a whole frame.  The two are ALTERNATED call by call (one call = the whole frame's chunks) and the
      paired difference is reported with p10 / p90, as profiles/joint_gan_step_time.md does.
    python tools/dvqgo_call_time.py [--voxels 192 192 128] [--clusters 64] [--dim 6] [--width 32] [--pe 2] [--reps 20] [--out FILE.md]"""
import argparse
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import numpy as np
import torch
import nerf4k_amd  # noqa: F401
from nerf4k_amd import scene
from nerf4k_amd.lib import utils, dvgo
import vq_oracle as vo

ap = argparse.ArgumentParser()
ap.add_argument('--voxels', type=int, nargs=3, default=[192, 192, 128])
ap.add_argument('--clusters', type=int, default=64)
ap.add_argument('--dim', type=int, default=6)
ap.add_argument('--width', type=int, default=32)
ap.add_argument('--pe', type=int, default=2)
ap.add_argument('--chunk', type=int, default=8192)
ap.add_argument('--reps', type=int, default=20)
ap.add_argument('--H', type=int, default=756)
ap.add_argument('--W', type=int, default=1008)
ap.add_argument('--out', default=None)
args = ap.parse_args()
dev = torch.device('cuda', 0)
H, W = args.H, args.W
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def once(fn):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), r


def stats(v):
    return f'{np.median(v):.3f} (p10 {np.percentile(v, 10):.3f}, p90 {np.percentile(v, 90):.3f}, {np.min(v):.3f} .. {np.max(v):.3f})'


X, Y, Z = args.voxels
ck = scene.make_vq_checkpoint(num_voxels=X * Y * Z, mpi_depth=Z, n_cluster=args.clusters, rgbnet_dim=args.dim, rgbnet_width=args.width, spatial_pe=args.pe)
model = utils.model_from_checkpoint_dict(ck).to(dev).eval()
rk = ck['render_kwargs']
K = scene.LLFF_K.copy()
K[:2] *= W / scene.LLFF_HW[1]
pose = torch.from_numpy(scene.llff_spiral_poses()[4]).to(dev)
with torch.no_grad():
    ro, rd, vd = [x.reshape(-1, 3).contiguous() for x in dvgo.get_rays_of_a_view(H, W, K, pose, True, False, False, False)]
    n_rays = ro.shape[0]
    # the frame's shaded points per 8192-ray chunk: what the staged path hands the codebook
    pes = []
    hook = model.k0.register_forward_hook(lambda m, a, o: pes.append(a[0].contiguous()))
    staged = [model(ro[s:s + args.chunk], rd[s:s + args.chunk], vd[s:s + args.chunk], k4_staged=True, **rk) for s in range(0, n_rays, args.chunk)]
    hook.remove()
    n_pts = sum(p.shape[0] for p in pes)
    say(f'DirectQVGO {X}x{Y}x{Z}, {W}x{H} ({n_rays} rays), {n_pts} shaded points in {len(pes)} chunks of {args.chunk} rays; codebook {args.clusters} x {args.dim}, '
        f'{3 + 6 * args.pe} embedded inputs, rgbnet width {args.width}')
    # (a) the one-launch frame
    ms = [once(lambda: model(ro, rd, vd, k4_fused=True, **rk))[0] for _ in range(args.reps + 1)][1:]
    out = model(ro, rd, vd, k4_fused=True, **rk)
    d = float((out['rgb_marched'] - torch.cat([o['rgb_marched'] for o in staged])).abs().max())
    say(f'(a) one launch (k4_march_vq_fwd): {stats(ms)} ms per frame over {args.reps} calls = {n_rays / np.median(ms) / 1e3:.1f} Mrays/s; '
        f'max |one launch - staged| rgb {d:.2e}')
    ms_st = [once(lambda: [model(ro[s:s + args.chunk], rd[s:s + args.chunk], vd[s:s + args.chunk], k4_staged=True, **rk) for s in range(0, n_rays, args.chunk)])[0]
             for _ in range(3)][1:]
    say(f'    the staged path in {args.chunk}-ray chunks (host-paced: one read-back per chunk): {np.median(ms_st):.1f} ms per frame')
    # (b) the lookup: HIP against the eager expressions, alternated
    st = {k: v.to(dev) for k, v in vo.vq_state(model.k0.state_dict()).items()}
    hip = lambda: [model.k0(p)[0] for p in pes]
    eager = lambda: [vo.vq_forward(st, p)[0] for p in pes]
    same = all(torch.equal(model.k0(p)[2], vo.vq_forward(st, p)[2]) for p in pes)
    t_h, t_e = [], []
    for i in range(args.reps + 1):
        a, _ = once(hip)
        b, _ = once(eager)
        if i:
            t_h.append(a)
            t_e.append(b)
    diff = np.asarray(t_e) - np.asarray(t_h)
    say(f'(b) codeword lookup of the frame\'s points ({len(pes)} calls per frame), {args.reps} alternated frames, ms per frame:')
    say(f'    VQGrid.forward (k4_vq_project_fwd + k4_vq_assign): {stats(t_h)}')
    say(f'    eager tensor-library expressions:                  {stats(t_e)}')
    say(f'    paired difference eager - HIP:                     {stats(diff)}; same indices on every point: {same}')
if args.out:
    with open(args.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')
