"""sha1 of the fused marcher's outputs (rgb, depth, alphainv) on cases aimed at the TAIL of the geometry kernel -- the transmittance scan and the
hand-over of the w > thres survivors to the shading kernel -- under the CURRENT environment (the library reads K4_DEBUG once while it loads):
the FAST instantiation scans and appends survivors in one pass (record order: quarter, rank within the ray, ray slot), the general one
(K4_DEBUG=16384) writes the weights back and compacts in a second pass (quarter, ray, depth).  tests/test_geom_tail_gpu.py runs this tool once
per setting and wants equal hashes.      python tools/geom_tail_hash.py <case> [<case> ...]
Every case meets the FAST predicate (256 planes, stepsize 1, one launch, occupancy summary) on a 48 x 48 x 256 grid:
  full    all-ones mask, alpha ~ 2e-3 on every sample: every in-box sample passes alpha and every weight stays above fast_color_thres, so a
          bundle of in-box rays carries 64 x 256 survivors -- every quarter filled to capacity (tests/test_geom_tail_gpu.py checks the 256 shaded
          samples per ray with the CPU oracle on the 16 x 16 pixels FULL_BLOCK of the frame)
  stop    the opaque-wall scene with the depth split switched off: rays stop mid-depth (predicated loads, early exit)
  ragged  the blob scene: an image with ragged 8 x 8 tiles on both axes, ray lists whose length is no multiple of 64 (one shorter than 64)
  empty   the blob scene with one half of the volume emptied: bundles without a record, whose outputs the geometry kernel writes itself
  reuse   frames A, B, A, A, a larger C, A through ONE workspace slot: every A equal to the first (no stale record is read)"""
import hashlib, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import nerf4k_amd  # noqa: F401
from nerf4k_amd import scene
from nerf4k_amd.lib import utils, dvgo, dmpigo

dev = torch.device('cuda', 0)
GRID = dict(num_voxels=48 * 48 * 256, mpi_depth=256)
KEYS = ('rgb_marched', 'depth', 'alphainv_last')
FULL_FRAME = (60, 80, 3)                                    # case full: H, W, pose
FULL_BLOCK = (16, 32, 32, 48)                               # ... and the rows / columns of one workgroup (four 8 x 8 bundles) in its middle


def rays_of(H, W, frame):
    K = scene.LLFF_K.copy()
    K[:2] *= W / scene.LLFF_HW[1]
    v = dvgo.get_rays_of_a_view(H, W, K, torch.from_numpy(scene.llff_spiral_poses()[frame]).to(dev), True, False, False, False)
    return [x.reshape(-1, 3).contiguous() for x in v]


def model_of(ck):
    model = utils.model_from_checkpoint_dict(ck).to(dev).eval()
    return model, dict(ck['render_kwargs'], render_depth=True)


def march(model, rays, img_w, rk, h):
    out = model(*rays, k4_img_w=img_w, **rk)
    torch.cuda.synchronize()
    out = {k: out[k].clone() for k in KEYS}
    for k in KEYS:
        h.update(out[k].cpu().numpy().tobytes())
    return out


def full_checkpoint():
    """Per plane z the density that makes sigma + act_shift[z] the logit of alpha = 2e-3 (the construction of geom_hash.py's threshold cases, aimed
    above the threshold instead of at it), a +-1e-3 ripple so that no two samples carry the same weight, all-ones MaskGrid."""
    ck = scene.make_llff_checkpoint(seed=61, **GRID)
    sd = ck['model_state_dict']
    d = sd['density.grid']
    act = sd['act_shift.grid'].reshape(-1)
    assert act.numel() == d.shape[-1]
    sig = float(np.log(2e-3 / (1.0 - 2e-3)))                # interval 1: alpha = e / (1 + e)
    g = torch.Generator().manual_seed(9)
    d.copy_((sig - act).view(1, 1, 1, 1, -1) + (torch.rand(d.shape, generator=g) - 0.5) * 2e-3)
    sd['mask_cache.mask'].fill_(True)
    return ck


def case_full(h):
    ck = full_checkpoint()
    model, rk = model_of(ck)
    march(model, rays_of(*FULL_FRAME), FULL_FRAME[1], rk, h)
    return model


def case_stop(h):
    ck = scene.make_llff_checkpoint(seed=781, opaque=True, **GRID)
    model, rk = model_of(ck)
    H, W = 60, 80
    nstop = 0
    for f in (3, 11):
        out = march(model, rays_of(H, W, f), W, rk, h)
        nstop += int((out['alphainv_last'] < 1e-3).sum())
    assert nstop > 0, 'no ray reached the T < 1e-3 stop'
    return model


def case_ragged(h):
    model, rk = model_of(scene.make_llff_checkpoint(**GRID))
    seen = 0.0
    seen += float((1 - march(model, rays_of(36, 20, 3), 20, rk, h)['alphainv_last']).sum())          # 2.5 x 4.5 tiles
    rays = rays_of(60, 80, 7)
    for n in (64 * 5 + 17, 64 * 40 - 1, 37):                 # linear ray lists: none a multiple of 64, one shorter than a bundle
        seen += float((1 - march(model, [r[1000:1000 + n].contiguous() for r in rays], 0, rk, h)['alphainv_last']).sum())
    assert seen > 0, 'nothing was composited'
    return model


def case_empty(h):
    ck = scene.make_llff_checkpoint(**GRID)
    d = ck['model_state_dict']['density.grid']
    d[:, :, :d.shape[2] // 2] = -30.0                         # x < mid: alpha == 0 to fp32, no sample passes
    model, rk = model_of(ck)
    H, W = 64, 80
    out = march(model, rays_of(H, W, 3), W, rk, h)
    ainv = out['alphainv_last'].view(H // 8, 8, W // 8, 8)
    none = (ainv == 1.0).all(dim=3).all(dim=1)                # 8 x 8 tiles (= bundles) in which no ray met an alpha-passing sample
    some = (ainv < 1.0).any(dim=3).any(dim=1)
    assert int(none.sum()) > 0 and int(some.sum()) > 0, (int(none.sum()), int(some.sum()))
    rgb = out['rgb_marched'].view(H // 8, 8, W // 8, 8, 3)
    dep = out['depth'].view(H // 8, 8, W // 8, 8)
    bg = float(rk['bg'])
    for ty, tx in none.nonzero().tolist():                    # rgb = alphainv_last * bg, depth 0: written by the geometry kernel
        assert bool((rgb[ty, :, tx] == bg).all()) and bool((dep[ty, :, tx] == 0).all()), (ty, tx)
    return model


def case_reuse(h):
    model, rk = model_of(scene.make_llff_checkpoint(**GRID))
    a, b, c = rays_of(60, 80, 3), rays_of(60, 80, 11), rays_of(72, 96, 5)
    first = march(model, a, 80, rk, h)
    march(model, b, 80, rk, h)
    again = [march(model, a, 80, rk, h), march(model, a, 80, rk, h)]
    march(model, c, 96, rk, h)                                # a larger frame: other bundle count, other slices
    again.append(march(model, a, 80, rk, h))
    assert float((1 - first['alphainv_last']).sum()) > 0
    for i, o in enumerate(again):
        for k in KEYS:
            assert torch.equal(first[k], o[k]), (i, k)
    return model


CASES = {'full': case_full, 'stop': case_stop, 'ragged': case_ragged, 'empty': case_empty, 'reuse': case_reuse}
if __name__ == '__main__':
    dmpigo.DEPTH_SPLIT = False                              # one geometry launch whatever the scene: the FAST predicate
    with torch.no_grad():
        for case in (sys.argv[1:] or list(CASES)):
            h = hashlib.sha1()
            model = CASES[case](h)
            split = int(model._k4_cache().get('dsplit', 0))
            interval = float(1.0 * model.voxel_size_ratio)
            assert split == 0 and interval == 1.0, (split, interval)
            print('GEOM_TAIL_HASH', case, h.hexdigest(), f'interval={interval:g}', f'depth_split={split}', flush=True)
