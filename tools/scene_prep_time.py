"""Scene preparation at the chair recipe's coarse-stage shape: the fused routes (DirectVoxGO.k4_voxel_count_views, k4_maskout_near_cam_vox) against the
staged methods (voxel_count_views, maskout_near_cam_vox), in one process and ALTERNATED (fused, staged, fused, staged, ...) after a warm-up round.
Scene: scene.make_lego_checkpoint(num_voxels=1024000), 100 views of 800x800 from scene.lego_pose / scene.lego_K with the checkpoint's near / far /
stepsize, downrate 1; the near mask with the 100 camera centres.  The ray tables are built once on the device, outside the timed region (both routes read
them).  The staged count is timed on --staged-views views (default 4: 256 chunks of 10,000 rays) and SCALED to all views -- its cost per view does not
depend on the other views; the fused count is timed on all of them.  Wall time between device synchronisations; median (min .. max) of --reps rounds.
Also: that fused and staged counts agree on the staged views, and the number of atomics an unskipped walk would issue per view (8 per sample that
touches the grid, counted from the ray geometry) next to the fused time per view.
    python tools/scene_prep_time.py [--views 100] [--staged-views 4] [--reps 5] [--H 800] [--W 800] [--num-voxels 1024000] [--out FILE.md]"""
import argparse
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import nerf4k_amd  # noqa: F401
from nerf4k_amd import scene
from nerf4k_amd.lib import utils, dvgo, render_utils_cuda as ruc

ap = argparse.ArgumentParser()
ap.add_argument('--views', type=int, default=100)
ap.add_argument('--staged-views', type=int, default=4)
ap.add_argument('--reps', type=int, default=5)
ap.add_argument('--H', type=int, default=800)
ap.add_argument('--W', type=int, default=800)
ap.add_argument('--num-voxels', type=int, default=1024000)
ap.add_argument('--out', default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit('scene_prep_time: needs the GPU (a CPU timing says nothing about it)')
dev = torch.device('cuda', 0)
H, W, NV, SV = args.H, args.W, args.views, min(args.staged_views, args.views)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def stat(v):
    v = np.asarray(v)
    return f'{np.median(v):.1f} ms ({v.min():.1f} .. {v.max():.1f})'


def once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


ck = scene.make_lego_checkpoint(num_voxels=args.num_voxels)
model = utils.model_from_checkpoint_dict(ck).to(dev).eval()
rk = ck['render_kwargs']
K = scene.lego_K(H, W)
poses = torch.stack([torch.as_tensor(scene.lego_pose(theta_deg=360. * i / NV, phi_deg=-15. - 30. * (i % 3))[:3, :4], dtype=torch.float32) for i in range(NV)]).to(dev)
ro, rd = (torch.empty([NV, H, W, 3], device=dev) for _ in range(2))
with torch.no_grad():
    for v in range(NV):
        ro[v], rd[v], _ = dvgo.get_rays_of_a_view(H, W, K, poses[v], False, rk['inverse_y'], rk['flip_x'], rk['flip_y'])
kw = dict(near=rk['near'], far=rk['far'], stepsize=rk['stepsize'], downrate=1)

ms_f, ms_s = [], []
for i in range(args.reps + 1):                          # the first round warms the allocator and the code objects
    tf, cnt_f = once(lambda: model.k4_voxel_count_views(ro, rd, [1] * NV, **kw))
    ts, cnt_s = once(lambda: model.voxel_count_views(ro[:SV], rd[:SV], [1] * SV, **kw))
    if i:
        ms_f.append(tf)
        ms_s.append(ts)
cnt_f_sv = model.k4_voxel_count_views(ro[:SV], rd[:SV], [1] * SV, **kw)
differ = int((cnt_f_sv != cnt_s).sum())
f, s = np.asarray(ms_f), np.asarray(ms_s) * (NV / SV)

# what an unskipped walk would issue: 8 atomics per sample inside the box (the box samples are all but a cell's width of those that touch the grid)
sd = float(rk['stepsize'] * model.voxel_size)
with torch.no_grad():
    o, d = ro[0].reshape(-1, 3), rd[0].reshape(-1, 3)
    t_min, t_max = ruc.infer_t_minmax(o, d, model.xyz_min, model.xyz_max, rk['near'], 1e9)
    box_samples = int(ruc.infer_n_samples(d, t_min, t_max, sd)[t_max > t_min].sum())
n_samples = int(np.linalg.norm(np.array(model.world_size.cpu()) + 1) / rk['stepsize']) + 1

cams = poses[:, :3, 3].contiguous()
grid0 = model.density.grid.detach().clone()
ms_nf, ms_ns = [], []
for i in range(args.reps + 1):
    with torch.no_grad():
        model.density.grid.copy_(grid0)
    tf, _ = once(lambda: model.k4_maskout_near_cam_vox(cams, rk['near']))
    near_f = model.density.grid.detach().clone()
    with torch.no_grad():
        model.density.grid.copy_(grid0)
    ts, _ = once(lambda: model.maskout_near_cam_vox(cams, rk['near']))
    if i:
        ms_nf.append(tf)
        ms_ns.append(ts)
near_same = bool(torch.equal(near_f, model.density.grid.detach()))

say(f'DirectVoxGO {model.world_size.tolist()} ({args.num_voxels} voxels), {NV} views of {W}x{H} = {NV * H * W} rays, stepsize {rk["stepsize"]} '
    f'({n_samples} samples per ray at most), downrate 1; {args.reps} alternated rounds after one warm-up round, wall time between device synchronisations')
say(f'  view count, fused  (2 launches per view, {NV} views): {stat(f)} = {np.median(f) / NV:.2f} ms per view')
say(f'  view count, staged ({SV} views timed = {SV * ((H * W + 9999) // 10000)} chunks of 10,000 rays, SCALED x{NV / SV:g} to {NV} views): {stat(s)} = '
    f'{np.median(s) / NV:.1f} ms per view')
say(f'  staged / fused = {np.median(s) / np.median(f):.1f}x (ratio of medians); counts of the {SV} staged views: {differ} of {cnt_s.numel()} voxels differ '
    f'(a voxel whose sum lies within fp32 rounding of 1 is decided by the atomic order in the staged method)')
say(f'  an unskipped walk would issue ~{8 * box_samples / 1e9:.2f} G atomics per view ({box_samples / (H * W):.0f} box samples per ray x 8 corners, view 0) = '
    f'{8 * box_samples * 8 / 1e9:.1f} GB of added bytes; the fused walk takes {np.median(f) / NV:.2f} ms per view with the finalise pass')
say(f'  near mask, {NV} cameras: fused (1 launch) {stat(ms_nf)}; staged ([X, Y, Z, 100, 3] tables) {stat(ms_ns)}; staged / fused = '
    f'{np.median(ms_ns) / np.median(ms_nf):.1f}x; grids equal: {near_same}')
if args.out:
    with open(args.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')
