"""sha1 of the fused marcher's outputs (rgb, depth, alphainv) on cases aimed at the DEAL of the geometry kernel's FAST instantiation -- group G of
ray slot r goes to wave (G + (r >> 4)) & 3, a depth quarter's records lie in four per-wave segments (4k-nerf_amd/csrc/k4_geom_deal.h) -- under the
CURRENT environment (the library reads K4_DEBUG once while it loads; K4_DEBUG=16384 forces the general instantiation, which keeps one depth
quarter per wave).  tests/test_geom_deal_gpu.py runs this tool once per setting and wants equal hashes.
      python tools/geom_deal_hash.py <case> [<case> ...]
Every case meets the FAST predicate (at most 256 planes, interval 1, one launch, occupancy summary) on a 48 x 48 x N grid and asserts its premise:
  sheet16   N = 256, density above the alpha threshold only in planes 96..111 = group 6: with quarters one wave's whole load, with the deal four
            segments of depth quarter 1 and three empty quarters.  Premise: every shaded step lies in [96, 112) (asserted here on the grid's alphas,
            by the test on the CPU oracle's step list).
  straddle  N = 256, a slab of alpha ~ 0.4 over planes 56..72 in front of the blob scene: it crosses a quarter and two group boundaries, rays stop
            inside a segment and the later quarters are never read.  Premise: some rays end with T < 1e-3, some do not.
  n250      250 planes: the last group has 10 samples; the blob scene has content at every depth.
  n40       40 planes: groups 0..2 only -- for each 16-ray subset of a bundle one wave has no group at all.
  ragged    N = 256, image width and height no multiple of 8, ray lists no multiple of 64 (one shorter than a bundle); content at every depth.
A scene with N != 256 planes gets voxel_size_ratio = 1 on the model (the reference ties it to 256 / N): the FAST predicate wants interval == 1,
and both instantiations are given the same value."""
import hashlib, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.nn.functional as F
import nerf4k_amd  # noqa: F401
from nerf4k_amd import scene
from nerf4k_amd.lib import utils, dvgo, dmpigo

KEYS = ('rgb_marched', 'depth', 'alphainv_last')
SHEET = (96, 112)                                           # case sheet16: planes with content
SHEET_FRAME = (60, 80, 3)                                   # ... and its frame: H, W, pose
SLAB = (56, 73)


def grid_of(n):
    return dict(num_voxels=48 * 48 * n, mpi_depth=n)


def rays_of(H, W, frame, dev):
    K = scene.LLFF_K.copy()
    K[:2] *= W / scene.LLFF_HW[1]
    v = dvgo.get_rays_of_a_view(H, W, K, torch.from_numpy(scene.llff_spiral_poses()[frame]).to(dev), True, False, False, False)
    return [x.reshape(-1, 3).contiguous() for x in v]


def remask(ck, margin=5.5):
    """The occupancy mask of scene.make_llff_checkpoint, derived again from an edited density grid."""
    sd, kw = ck['model_state_dict'], ck['model_kwargs']
    loose = scene._raw2alpha(sd['density.grid'] + margin + sd['act_shift.grid'], 0, kw['voxel_size_ratio'])
    sd['mask_cache.mask'] = (F.max_pool3d(loose, kernel_size=3, padding=1, stride=1)[0, 0] > kw['fast_color_thres'])
    assert list(sd['mask_cache.mask'].shape) == list(kw['mask_cache_world_size'])


def sheet_checkpoint():
    ck = scene.make_llff_checkpoint(seed=23, n_blobs=64, **grid_of(256))
    d = ck['model_state_dict']['density.grid']
    d[..., :SHEET[0]] = -30.0                               # alpha == 0 to fp32 outside the sheet
    d[..., SHEET[1]:] = -30.0
    d[..., SHEET[0]:SHEET[1]] += 9.0                        # the blobs' flanks above the threshold too: most rays meet records
    remask(ck)
    return ck


def straddle_checkpoint():
    ck = scene.make_llff_checkpoint(seed=29, **grid_of(256))
    sd = ck['model_state_dict']
    d, act = sd['density.grid'], sd['act_shift.grid'].reshape(-1)
    g = torch.Generator().manual_seed(5)
    sig = float(np.log(0.4 / 0.6))                          # interval 1: alpha = e / (1 + e); 0.6^14 < 1e-3 -- the stop falls inside the slab
    z = slice(SLAB[0], SLAB[1])
    d[..., z] = (sig - act[z]).view(1, 1, 1, 1, -1) + (torch.rand(d[..., z].shape, generator=g) - 0.5) * 1.5
    remask(ck)
    return ck


def model_of(ck, dev):
    model = utils.model_from_checkpoint_dict(ck).to(dev).eval()
    model.voxel_size_ratio = 1.0 * float(ck['model_kwargs']['voxel_size_ratio']) if int(ck['model_kwargs']['mpi_depth']) == 256 else 1.0
    return model, dict(ck['render_kwargs'], render_depth=True)


def march(model, rays, img_w, rk, h):
    out = model(*rays, k4_img_w=img_w, **rk)
    torch.cuda.synchronize()
    out = {k: out[k].clone() for k in KEYS}
    for k in KEYS:
        h.update(out[k].cpu().numpy().tobytes())
    return out


def case_sheet16(h, dev):
    ck = sheet_checkpoint()
    sd, kw = ck['model_state_dict'], ck['model_kwargs']
    # premise, on the grid: no density point outside planes [96, 112) reaches the alpha threshold, points inside do.  Sample k of an LLFF ray
    # lies on plane k, so every shaded step lies in [96, 112): tests/test_geom_deal_gpu.py asserts that on the CPU oracle's step list
    a = scene._raw2alpha(sd['density.grid'] + sd['act_shift.grid'], 0, kw['voxel_size_ratio'])[0, 0]
    thres = float(kw['fast_color_thres'])
    assert float(a[..., :SHEET[0]].max()) <= thres and float(a[..., SHEET[1]:].max()) <= thres and float(a[..., SHEET[0]:SHEET[1]].max()) > thres
    H, W, pose = SHEET_FRAME
    model, rk = model_of(ck, dev)
    out = march(model, rays_of(H, W, pose, dev), W, rk, h)
    assert int((out['alphainv_last'] < 1).sum()) > 64 * 16, 'the sheet met too few rays'
    return model


def case_straddle(h, dev):
    model, rk = model_of(straddle_checkpoint(), dev)
    H, W = 60, 80
    nstop = nopen = 0
    for f in (3, 11):
        ainv = march(model, rays_of(H, W, f, dev), W, rk, h)['alphainv_last']
        nstop += int((ainv < 1e-3).sum()); nopen += int((ainv >= 1e-3).sum())
    assert nstop > 0 and nopen > 0, (nstop, nopen)
    return model


def case_planes(n):
    def run(h, dev):
        model, rk = model_of(scene.make_llff_checkpoint(**grid_of(n)), dev)
        seen = float((1 - march(model, rays_of(60, 80, 3, dev), 80, rk, h)['alphainv_last']).sum())
        seen += float((1 - march(model, [r[:64 * 9 + 5].contiguous() for r in rays_of(60, 80, 7, dev)], 0, rk, h)['alphainv_last']).sum())
        assert seen > 0, 'nothing was composited'
        assert int(model.mpi_depth) == n
        return model
    return run


def case_ragged(h, dev):
    model, rk = model_of(scene.make_llff_checkpoint(**grid_of(256)), dev)
    seen = float((1 - march(model, rays_of(36, 20, 3, dev), 20, rk, h)['alphainv_last']).sum())                 # 2.5 x 4.5 tiles
    rays = rays_of(60, 80, 7, dev)
    for n in (64 * 5 + 17, 64 * 40 - 1, 37):                 # linear ray lists: none a multiple of 64, one shorter than a bundle
        seen += float((1 - march(model, [r[1000:1000 + n].contiguous() for r in rays], 0, rk, h)['alphainv_last']).sum())
    assert seen > 0, 'nothing was composited'
    return model


CASES = {'sheet16': case_sheet16, 'straddle': case_straddle, 'n250': case_planes(250), 'n40': case_planes(40), 'ragged': case_ragged}
if __name__ == '__main__':
    dmpigo.DEPTH_SPLIT = False                              # one geometry launch whatever the scene: the FAST predicate
    dev = torch.device('cuda', 0)
    with torch.no_grad():
        for case in (sys.argv[1:] or list(CASES)):
            h = hashlib.sha1()
            model = CASES[case](h, dev)
            split = int(model._k4_cache().get('dsplit', 0))
            interval = float(1.0 * model.voxel_size_ratio)
            assert split == 0 and interval == 1.0 and int(model.mpi_depth) <= 256, (split, interval, int(model.mpi_depth))
            print('GEOM_DEAL_HASH', case, h.hexdigest(), f'interval={interval:g}', f'depth_split={split}', f'planes={int(model.mpi_depth)}', flush=True)
