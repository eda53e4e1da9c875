"""DirectContractedVoxGO (lib/dcvgo.py) render time: a 1008x756 frame of a seeded unbounded scene (default 320^3, stepsize 0.5: 1,068 steps
per ray), timed with HIP events: the fused inference call (k4_march_contracted_fwd, one launch for the whole frame, no workspace) and the
staged path in chunks of 8192 rays as the reference's render loop evaluates it (run_sr.py:121-124).  Prints median frame times, Mrays/s,
the fused sample counters and the largest fused - staged difference; the staged chunk's table size is an estimate, not a measurement.
    python tools/dcvgo_call_time.py [--voxels 320] [--chunk 8192] [--reps 3]"""
import argparse
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import nerf4k_amd  # noqa: F401
from nerf4k_amd import scene
from nerf4k_amd.lib import utils, dvgo, dcvgo

ap = argparse.ArgumentParser()
ap.add_argument('--voxels', type=int, default=320)
ap.add_argument('--chunk', type=int, default=8192)
ap.add_argument('--reps', type=int, default=3)
ap.add_argument('--H', type=int, default=756)
ap.add_argument('--W', type=int, default=1008)
args = ap.parse_args()
dev = torch.device('cuda', 0)
ck = scene.make_unbounded_checkpoint(num_voxels=args.voxels ** 3)
model = utils.model_from_checkpoint_dict(ck).to(dev).eval()
rk = ck['render_kwargs']
H, W = args.H, args.W
pose = torch.from_numpy(scene.unbounded_poses()[1]).to(dev)
with torch.no_grad():
    ro, rd, vd = [x.reshape(-1, 3).contiguous() for x in dvgo.get_rays_of_a_view(H, W, scene.unbounded_K(H, W), pose, False, False, False, False)]
    n_rays = ro.shape[0]

    def timed(fn):
        ms = []
        for i in range(args.reps + 1):
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            r = fn()
            b.record()
            torch.cuda.synchronize()
            if i >= 1:
                ms.append(a.elapsed_time(b))
        return float(np.median(ms)), r, f'{min(ms):.2f} .. {max(ms):.2f}, {len(ms)} runs'

    # fused: ONE call for the whole frame (k4_march_contracted_fwd, no workspace)
    fused_ms, out_f, fused_span = timed(lambda: model(ro, rd, vd, **rk))
    cnt = torch.zeros(8, dtype=torch.int64, device=dev)
    model(ro, rd, vd, k4_counters=cnt, **rk)
    c = cnt.cpu().tolist()

    # staged: the reference's op sequence in chunks of 8192 rays (run_sr.py:121-124)
    def staged():
        n = 0
        for s in range(0, n_rays, args.chunk):
            n += model(ro[s:s + args.chunk], rd[s:s + args.chunk], vd[s:s + args.chunk], k4_staged=True, **rk)['ray_id'].shape[0]
        return n
    staged_ms, n_staged, _ = timed(staged)
    n_max = len(model._step_table(rk['stepsize'], dev))
    agree = float((out_f['rgb_marched'] - torch.cat([model(ro[s:s + args.chunk], rd[s:s + args.chunk], vd[s:s + args.chunk], k4_staged=True, **rk)['rgb_marched']
                                                     for s in range(0, n_rays, args.chunk)])).abs().max())
table_est = args.chunk * n_max * (3 * 4 * 3 + 4 + 1 + 1)     # ESTIMATE (not measured): the staged chunk's [chunk][n_max] point / difference / dist / mask tables
print(f'DirectContractedVoxGO {args.voxels}^3, {W}x{H}, {n_max} steps per ray ({n_rays * n_max} per frame)')
print(f'  fused (1 launch, workspace 0 bytes): median {fused_ms:.2f} ms per frame ({fused_span}) = {n_rays / fused_ms / 1e3:.1f} Mrays/s')
print(f'  staged ({args.chunk}-ray chunks): median {staged_ms:.1f} ms per frame = {n_rays / staged_ms / 1e3:.2f} Mrays/s; '
      f'its per-chunk step tables ~{table_est / 1e9:.2f} GB (estimate)')
print(f'  sample counters (fused): inner|cumdist {c[0]}, mask-pass {c[1]}, alpha-pass {c[2]}, shaded {c[3]} (staged shaded {n_staged}); '
      f'max |fused - staged| rgb {agree:.2e}')
