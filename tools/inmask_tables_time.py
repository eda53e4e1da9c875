"""The hit masks of the 'patch_inmask' / 'in_maskcache' ray samplers: the one-launch hit test (DirectVoxGO.k4_hit_coarse_geo, all views in one call)
against the staged path in 64-row chunks exactly as dvgo.get_training_rays_in_maskcache_sampling issues it (hit_coarse_geo per chunk: sample list,
mask lookup, boolean indexing, scatter).  Scene: the default scene.make_lego_checkpoint() (160^3, stepsize 0.5), 8 views of 800x800 from
scene.lego_pose / scene.lego_K, the checkpoint's render_kwargs; the ray tables are built once, outside the timed region (both paths read them).
Wall time with a device synchronisation on both sides, the two ALTERNATED (fused, staged, fused, staged, ...) after a warm-up round; median and
p10 / p90 of each and of the paired difference staged - fused.  Also: the hit fraction, that the two masks are equal, the per-tile count launch, and
the bytes the staged path writes per view (from the sample count: 12 B point + 1 B out-of-box flag + 8 B ray id + 8 B step id per sample).
    python tools/inmask_tables_time.py [--views 8] [--reps 10] [--H 800] [--W 800] [--voxels 160] [--out FILE.md]"""
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
ap.add_argument('--views', type=int, default=8)
ap.add_argument('--reps', type=int, default=10)
ap.add_argument('--H', type=int, default=800)
ap.add_argument('--W', type=int, default=800)
ap.add_argument('--voxels', type=int, default=160)
ap.add_argument('--out', default=None)
args = ap.parse_args()
assert args.reps >= 10, 'at least 10 repetitions'
dev = torch.device('cuda', 0)
H, W, NV = args.H, args.W, args.views
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def pct(v):
    v = np.asarray(v)
    return f'{np.median(v):.2f} ms (p10 {np.percentile(v, 10):.2f}, p90 {np.percentile(v, 90):.2f})'


ck = scene.make_lego_checkpoint(num_voxels=args.voxels ** 3)
model = utils.model_from_checkpoint_dict(ck).to(dev).eval()
rk = ck['render_kwargs']
K = scene.lego_K(H, W)
poses = torch.stack([torch.as_tensor(scene.lego_pose(theta_deg=360. * i / NV)[:3, :4], dtype=torch.float32) for i in range(NV)]).to(dev)
imgs = torch.zeros([NV, H, W, 3], device=dev)
with torch.no_grad():
    _, ro, rd, _, _ = dvgo.get_training_rays(imgs, poses, np.array([[H, W]] * NV), np.stack([K] * NV), False, rk['inverse_y'], rk['flip_x'], rk['flip_y'])

    def fused():
        return model.k4_hit_coarse_geo(rays_o=ro, rays_d=rd, **rk)

    def staged():
        return torch.stack([torch.cat([model.hit_coarse_geo(rays_o=ro[v, i:i + 64], rays_d=rd[v, i:i + 64], **rk) for i in range(0, H, 64)], 0)
                            for v in range(NV)])

    def once(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    ms_f, ms_s, ms_c = [], [], []
    for i in range(args.reps + 1):                      # the first round warms the allocator and the code objects
        tf, hit_f = once(fused)
        ts, hit_s = once(staged)
        tc, counts = once(lambda: dvgo.patch_hit_counts(hit_f, 64))
        if i:
            ms_f.append(tf)
            ms_s.append(ts)
            ms_c.append(tc)
    same = bool(torch.equal(hit_f, hit_s))
    frac = float(hit_f.float().mean())
    # what the staged path writes: per sample 12 + 1 + 8 + 8 bytes (point, out-of-box flag, int64 ray id, int64 step id)
    sd = float(rk['stepsize'] * model.voxel_size)
    n_samples = []
    for v in range(NV):
        o, d = ro[v].reshape(-1, 3), rd[v].reshape(-1, 3)
        t_min, t_max = ruc.infer_t_minmax(o, d, model.xyz_min, model.xyz_max, rk['near'], 1e9)
        n_samples.append(int(ruc.infer_n_samples(d, t_min, t_max, sd).sum()))
    kept = int((counts > 2048).sum())
f, s = np.asarray(ms_f), np.asarray(ms_s)
n_rays = NV * H * W
say(f'DirectVoxGO {args.voxels}^3 (mask cache {list(model.mask_cache.mask.shape)}), {NV} views of {W}x{H} = {n_rays} rays, stepsize {rk["stepsize"]}, '
    f'{args.reps} alternated repetitions after one warm-up round, wall time between device synchronisations')
say(f'  fused  (1 launch, one lane per ray): {pct(f)} = {n_rays / np.median(f) / 1e3:.1f} Mrays/s')
say(f'  staged ({NV * ((H + 63) // 64)} calls of 64 rows): {pct(s)} = {n_rays / np.median(s) / 1e3:.1f} Mrays/s')
say(f'  paired difference staged - fused: {pct(s - f)}; staged / fused = {np.median(s) / np.median(f):.1f}x (ratio of medians)')
say(f'  per-tile counts of all views (1 launch, {counts.shape[1]} entries per view): {pct(ms_c)}; tiles with more than 2048 hits: {kept} of {counts.numel()}')
say(f'  masks equal: {same}; hit fraction {frac:.3f}')
say(f'  samples per view {int(np.mean(n_samples)):,} (mean of {NV}; {np.mean(n_samples) / (H * W):.0f} per ray): the staged path writes '
    f'{np.mean(n_samples) * 29 / 1e9:.2f} GB of per-sample values per view ({sum(n_samples) * 29 / 1e9:.1f} GB for {NV} views); the fused call writes '
    f'{H * W} bytes per view')
if args.out:
    with open(args.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')
