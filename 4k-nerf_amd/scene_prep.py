"""Scene preparation: the steps of the reference's ``run_sr.py`` between loading a scene and the first training iteration, each on one HIP launch
(csrc/k4_prep.hip) instead of per-view / per-chunk tensor loops.

  compute_bbox_by_cam_frustrm   run_sr.py:222-268   the coarse stage's box from the training cameras' frusta
  compute_bbox_by_coarse_geo    run_sr.py:271-291   the fine stage's box from the coarse model's density
  per_voxel_init                run_sr.py:441-448   per-voxel learning rates and the view-count mask (DirectVoxGO.k4_voxel_count_views)

(The near-camera mask, run_sr.py:366, is ``DirectVoxGO.k4_maskout_near_cam_vox``.)  The kernels are the product: without a GPU every function raises
``K4Error``.
"""
import numpy as np
import torch

from . import _native as N
from .lib import render_utils_cuda, utils


def _device_of(*tensors):
    for t in tensors:
        if torch.is_tensor(t) and t.is_cuda:
            return t.device
    if not torch.cuda.is_available():
        raise N.K4Error('scene preparation runs on the GPU (no CPU path exists for this op)')
    return torch.device('cuda', torch.cuda.current_device())


def _as_f32(x, dev):
    t = x.detach().float() if torch.is_tensor(x) else torch.as_tensor(np.asarray(x), dtype=torch.float32)
    return t.to(dev)


@torch.no_grad()
def compute_bbox_by_cam_frustrm(HW, Ks, poses, i_train, near, far, *, ndc, inverse_y, flip_x, flip_y,
                                unbounded_inward=False, unbounded_inner_r=1.0, near_clip=None):
    """The box of the training cameras' frusta, one launch over all views (k4_frustum_bounds; views may differ in size and intrinsics).
    Bounded, ndc: the points rays_o + rays_d * {near, far}; bounded, not ndc: rays_o + viewdirs * {near, far}; ``unbounded_inward``: the tightest cube
    around rays_o + rays_d * near_clip, its radius scaled by ``unbounded_inner_r``.  The rays are those of ``dvgo.get_rays_of_a_view`` on a device
    pose.  -> (xyz_min, xyz_max), CPU float tensors as the reference returns them."""
    dev = _device_of(poses)
    idx = [int(i) for i in np.asarray(i_train).reshape(-1)]
    if not idx:
        raise ValueError('compute_bbox_by_cam_frustrm: no training view')
    hw = np.asarray([[int(HW[i][0]), int(HW[i][1])] for i in idx], dtype=np.int32)
    # -1./(W/(2.*focal)): Python double arithmetic on the fp32 focal the ray kernel's entry point receives (k4_get_rays_of_a_view)
    focal = [float(np.float32(float(Ks[i][0][0]))) for i in idx]
    scale = np.asarray([[-1. / (w / (2. * f)), -1. / (h / (2. * f))] for (h, w), f in zip(hw.tolist(), focal)], dtype=np.float32)
    K_dev = torch.stack([_as_f32(Ks[i], dev).reshape(3, 3) for i in idx]).contiguous()
    c2w = torch.stack([_as_f32(poses[i], dev)[:3, :4] for i in idx]).contiguous()
    if unbounded_inward:
        if near_clip is None:
            raise ValueError('compute_bbox_by_cam_frustrm: unbounded_inward needs near_clip')
        use_viewdirs, ts = False, [near_clip]
    else:
        use_viewdirs, ts = not ndc, [near, far]
    per_view = render_utils_cuda.frustum_bounds(torch.from_numpy(hw).to(dev), K_dev, c2w, torch.from_numpy(scale).to(dev),
                                                int((hw[:, 0].astype(np.int64) * hw[:, 1]).max()), ndc, inverse_y, flip_x, flip_y, use_viewdirs, ts).cpu()
    xyz_min, xyz_max = per_view[:, :3].amin(0), per_view[:, 3:].amax(0)
    if unbounded_inward:                                   # the tightest cube that covers the camera centres (run_sr.py:250-253)
        center = (xyz_min + xyz_max) * 0.5
        radius = (center - xyz_min).max() * unbounded_inner_r
        xyz_min, xyz_max = center - radius, center + radius
    return xyz_min, xyz_max


@torch.no_grad()
def coarse_geo_bounds(model, thres):
    """The box of the grid nodes whose activated density exceeds ``thres``: one launch over the dense density grid (k4_coarse_geo_bounds: alpha from
    the NODE values themselves, integer min / max of the passing indices per axis, exact), then the reference's node coordinates
    xyz_min * (1 - interp) + xyz_max * interp at the six indices.  -> (xyz_min, xyz_max) on the model's device; ValueError when no node passes."""
    dense = model.density.get_dense_grid().detach()
    X, Y, Z = (int(v) for v in dense.shape[2:])
    interval = model.voxel_size_ratio
    ijk = render_utils_cuda.coarse_geo_bounds(dense.reshape(X, Y, Z).float().contiguous(), float(model.act_shift), float(interval), thres).tolist()
    if ijk[3] < 0:
        raise ValueError(f'coarse_geo_bounds: no grid node has alpha > {thres}')
    lo, hi = [], []
    for a, n in enumerate((X, Y, Z)):
        interp = torch.linspace(0, 1, n, device=dense.device)
        axis = model.xyz_min[a] * (1 - interp) + model.xyz_max[a] * interp
        lo.append(axis[ijk[a]])
        hi.append(axis[ijk[3 + a]])
    return torch.stack(lo), torch.stack(hi)


@torch.no_grad()
def compute_bbox_by_coarse_geo(model_class, model_path, thres):
    """run_sr.py:271-291: load the coarse checkpoint, -> ``coarse_geo_bounds`` of it."""
    dev = _device_of()
    model = utils.load_model(model_class, model_path).to(dev)
    return coarse_geo_bounds(model, thres)


def per_voxel_init(model, optimizer, rays_o_tr, rays_d_tr, imsz, near, far, stepsize, downrate, irregular_shape):
    """run_sr.py:441-448 on the fused count: per-voxel learning rates from the view counts, and the mask cache cleared where at most two views
    see a voxel.  -> the count [1, 1, X, Y, Z]."""
    cnt = model.k4_voxel_count_views(rays_o_tr=rays_o_tr, rays_d_tr=rays_d_tr, imsz=imsz, near=near, far=far, stepsize=stepsize,
                                     downrate=downrate, irregular_shape=irregular_shape)
    optimizer.set_pervoxel_lr(cnt)
    with torch.no_grad():
        model.mask_cache.mask[cnt.squeeze() <= 2] = False
    return cnt
