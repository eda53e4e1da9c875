"""sha1 of the fused marcher's outputs (rgb, depth, alphainv) on one named case, under the CURRENT environment: the library reads K4_DEBUG once
while it loads, so the geometry kernel's FAST instantiation and its general path (K4_DEBUG=16384) are compared across processes
(tests/test_geom_fast_gpu.py).      python tools/geom_hash.py <case>
Cases: bench (the bench scene, 1008 x 756), small (bench.py --small's scene), linear (ray list, length not a multiple of 64), windows (a row band
and a tile window with ragged 8 x 8 tiles), threshold (every voxel's density at the alpha == fast_color_thres bound: the live-mask tests'
scene, 40 planes, so interval = 256 / 40 and the general path) and threshold256 (the same construction on 256 planes: interval 1, FAST), opaque (the opaque-wall scene:
the depth split is chosen, both runs take the general path), halfstep (stepsize 0.5: interval != 1, the general path)."""
import hashlib, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import nerf4k_amd  # noqa: F401
from nerf4k_amd import scene
from nerf4k_amd.lib import utils, dvgo
dev = torch.device('cuda', 0)
case = sys.argv[1] if len(sys.argv) > 1 else 'bench'
h = hashlib.sha1()


def rays_of(H, W, frame):
    K = scene.LLFF_K.copy()
    K[:2] *= W / scene.LLFF_HW[1]
    v = dvgo.get_rays_of_a_view(H, W, K, torch.from_numpy(scene.llff_spiral_poses()[frame]).to(dev), True, False, False, False)
    return [x.reshape(-1, 3).contiguous() for x in v]


def march(model, rays, img_w, rk):
    out = model(*rays, k4_img_w=img_w, **rk)
    torch.cuda.synchronize()
    for k in ('rgb_marched', 'depth', 'alphainv_last'):
        h.update(out[k].cpu().numpy().tobytes())
    return out


with torch.no_grad():
    cfg = {'bench': {}, 'small': dict(num_voxels=96 * 96 * 64, mpi_depth=64),
           'linear': {}, 'windows': {},            # the bench scene again: 256 samples (all four depth quarters at work) and a single launch
           'threshold': dict(seed=61, num_voxels=48 * 48 * 40, mpi_depth=40),
           'threshold256': dict(seed=61, num_voxels=48 * 48 * 256, mpi_depth=256),      # 256 planes: interval == 1, the shape FAST takes
           'opaque': dict(seed=781, opaque=True),
           'halfstep': dict(seed=34, num_voxels=56 * 56 * 64, mpi_depth=64, stepsize=0.5)}[case]
    ck = scene.make_llff_checkpoint(**cfg)
    model = utils.model_from_checkpoint_dict(ck).to(dev).eval()
    rk = dict(ck['render_kwargs'], render_depth=True)
    if case.startswith('threshold'):
        # tests/test_march_gpu.py::test_live_mask_adversarial_density_at_the_threshold: every voxel within 1e-6 .. 1e-2 of the density at which
        # alpha == fast_color_thres (or of a level 1.0 below it), all-ones MaskGrid
        thres = float(model.fast_color_thres)
        interval = float(rk['stepsize'] * model.voxel_size_ratio)
        sig = float(np.log(np.power(1.0 - thres, -1.0 / interval) - 1.0))
        g = torch.Generator().manual_seed(9)
        d = model.density.grid
        noise = torch.randn(d.shape, generator=g) * torch.pow(10.0, torch.randint(-6, -1, d.shape, generator=g).float())
        blk = (torch.rand([1, 1] + [(n + 3) // 4 for n in d.shape[2:]], generator=g) < 0.5).float()
        for ax in (2, 3, 4):
            blk = blk.repeat_interleave(4, dim=ax)
        noise = noise - blk[:, :, :d.shape[2], :d.shape[3], :d.shape[4]]
        zi = torch.linspace(0, model.act_shift.grid.numel() - 1, d.shape[-1]).round().long()
        base = sig - model.act_shift.grid.reshape(-1)[zi].cpu()
        d.copy_((base.view(1, 1, 1, 1, -1) + noise).to(d.device))
        model.mask_cache.mask.fill_(True)
        from torch.autograd.graph import increment_version
        increment_version(model.mask_cache.mask)
    seen = 0.0
    if case in ('bench', 'small', 'opaque'):
        H, W = scene.LLFF_HW if case != 'opaque' else (378, 504)
        for f in (3, 11):
            seen += float((1 - march(model, rays_of(H, W, f), W, rk)['alphainv_last']).sum())
    elif case == 'linear':
        H, W = 378, 504
        rays = rays_of(H, W, 2)
        for n in (H * W - 37, 64 * 100 + 1, 63):                       # none a multiple of 64
            seen += float((1 - march(model, [r[:n].contiguous() for r in rays], 0, rk)['alphainv_last']).sum())
    elif case == 'windows':
        H, W = 378, 504
        rays = rays_of(H, W, 2)
        ar = lambda a, b: torch.arange(a, b, device=dev)
        band = (ar(100, 161)[:, None] * W + ar(0, W)[None, :]).reshape(-1)             # 61 rows: the last tile row holds 5
        win = (ar(50, 239)[:, None] * W + ar(37, 226)[None, :]).reshape(-1)            # 189 x 189: ragged on both axes
        seen += float((1 - march(model, [r[band].contiguous() for r in rays], W, rk)['alphainv_last']).sum())
        seen += float((1 - march(model, [r[win].contiguous() for r in rays], 189, rk)['alphainv_last']).sum())
    else:
        H, W = (60, 80) if case.startswith('threshold') else (90, 120)
        seen += float((1 - march(model, rays_of(H, W, 3 if case.startswith('threshold') else 7), W, rk)['alphainv_last']).sum())
    assert seen > 0, 'nothing was composited'
    split = int(model._k4_cache().get('dsplit', 0))
    interval = float(rk['stepsize'] * model.voxel_size_ratio)
print('GEOM_HASH', case, h.hexdigest(), f'interval={interval:g}', f'depth_split={split}')
