"""float64 numpy oracle of the scene-preparation steps (nerf4k_amd.scene_prep, DirectVoxGO.k4_voxel_count_views) and the seeded scenes the CPU and GPU
tests share.  The formulas restate lib/dvgo.py:235-268 and run_sr.py:271-291 of the reference; nothing here touches the GPU or the library.

View count.  Per view, per ray:  vec = d == 0 ? 1e-6 : d;  t_min = clamp(max_c min((max_c - o_c) / vec_c, (min_c - o_c) / vec_c), near, 1e9);
t_i = t_min + stepsize * voxel_size * i / |d|, i < n_samples = int(|world_size + 1| / stepsize) + 1;  p_i = o + d t_i.  Every sample adds its eight
trilinear weights (align_corners, ZERO padding: corners off the grid are dropped, the others still count) to the voxels; a view counts for a voxel
when its sum exceeds 1.  ``count_sums`` returns the sums so a test can leave out the voxels whose sum is too close to 1 to be decided in fp32."""
import json
import os

import numpy as np

BAND = 1e-3              # |sum - 1| <= BAND: not compared (fp32 sums deviate from float64 by ~1e-5 at these shapes)
MAX_EXCLUDED = 0.01      # at most this share of a grid may fall in the band, per scene (asserted on the oracle alone)


def n_samples_of(world_size, stepsize):
    return int(np.linalg.norm(np.asarray(world_size) + 1) / stepsize) + 1


def split_views(rays, imsz, downrate, irregular_shape):
    """rays_tr.split(imsz), then the piece itself (irregular) or piece[::downrate, ::downrate].flatten(0, -2): numpy arrays [n_i, 3]."""
    pieces = np.split(rays, np.cumsum(imsz)[:-1], axis=0)
    if irregular_shape:
        return [p.reshape(-1, 3) for p in pieces]
    return [p[::downrate, ::downrate].reshape(-1, 3) for p in pieces]


def view_sums(o, d, xyz_min, xyz_max, world_size, near, stepsize, voxel_size):
    """One view's per-voxel weight sums, float64 [X, Y, Z]."""
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    lo, hi = np.asarray(xyz_min, np.float64), np.asarray(xyz_max, np.float64)
    size = np.asarray(world_size, np.int64)
    vec = np.where(d == 0, 1e-6, d)
    t_min = np.clip(np.minimum((hi - o) / vec, (lo - o) / vec).max(-1), near, 1e9)
    step = float(stepsize) * float(voxel_size) * np.arange(n_samples_of(world_size, stepsize), dtype=np.float64)
    t = t_min[:, None] + step[None] / np.linalg.norm(d, axis=-1, keepdims=True)
    p = o[:, None] + d[:, None] * t[..., None]
    u = ((p - lo) / (hi - lo)).reshape(-1, 3) * (size - 1)
    i0 = np.floor(u).astype(np.int64)
    f = u - i0
    sums = np.zeros(int(size.prod()))
    for c in range(8):
        off = np.array([(c >> 2) & 1, (c >> 1) & 1, c & 1])
        idx = i0 + off
        w = np.where(off == 1, f, 1 - f).prod(-1)
        ok = ((idx >= 0) & (idx < size)).all(-1)
        np.add.at(sums, ((idx[ok, 0] * size[1] + idx[ok, 1]) * size[2] + idx[ok, 2]), w[ok])
    return sums.reshape(tuple(size))


def count_sums(rays_o_tr, rays_d_tr, imsz, xyz_min, xyz_max, world_size, near, stepsize, voxel_size, downrate=1, irregular_shape=False):
    """-> float64 [n_views, X, Y, Z]"""
    vo = split_views(np.asarray(rays_o_tr), imsz, downrate, irregular_shape)
    vd = split_views(np.asarray(rays_d_tr), imsz, downrate, irregular_shape)
    return np.stack([view_sums(a, b, xyz_min, xyz_max, world_size, near, stepsize, voxel_size) for a, b in zip(vo, vd)])


def count_and_band(sums):
    """-> (count float32 [1, 1, X, Y, Z], compared bool [X, Y, Z]: no view's sum within BAND of 1)"""
    return (sums > 1).sum(0).astype(np.float32)[None, None], (np.abs(sums - 1) > BAND).all(0)


def raw2alpha(density, shift, interval):
    return 1 - np.power(1 + np.exp(np.asarray(density, np.float64) + shift), -interval)


# ---------------------------------------------------------------- seeded scenes
def dvgo_kwargs(extent_cells, cell=0.2):
    """Coarse DirectVoxGO kwargs whose world_size is floor(extent_cells): a box of extent_cells * cell centred on the origin."""
    ext = np.asarray(extent_cells, np.float64) * cell
    return dict(xyz_min=(-ext / 2).astype(np.float32), xyz_max=(ext / 2).astype(np.float32), num_voxels=float(np.prod(extent_cells)),
                num_voxels_base=float(np.prod(extent_cells)), alpha_init=1e-2, fast_color_thres=1e-4)


def _look_at_rays(rng, n, H, W, radius, jitter, focal):
    """n pinhole views [n, H, W, 3] on a sphere of `radius`, looking at a jittered point near the origin."""
    ro, rd = np.zeros([n, H, W, 3], np.float32), np.zeros([n, H, W, 3], np.float32)
    for v in range(n):
        c = rng.normal(size=3)
        c = c / np.linalg.norm(c) * radius
        fwd = rng.uniform(-jitter, jitter, 3) - c
        fwd /= np.linalg.norm(fwd)
        right = np.cross(fwd, [0.1, 0.2, 1.0])
        right /= np.linalg.norm(right)
        up = np.cross(right, fwd)
        j, i = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing='ij')
        d = fwd + ((i - W / 2) / focal)[..., None] * right + ((j - H / 2) / focal)[..., None] * up
        ro[v], rd[v] = c, d
    return ro, rd


def count_case(name):
    """A seeded view-count scene: dict(extent_cells, rays_o, rays_d, imsz, near, stepsize, downrate, irregular_shape).  Each exercises what its name says;
    test_scene_prep_cpu.py asserts for every one that at most MAX_EXCLUDED of the grid falls in the band."""
    if name == 'noncubic_3views_20x20':                      # stepsize 0.5, a non-cubic world, the camera outside
        rng = np.random.default_rng(11)
        ro, rd = _look_at_rays(rng, 3, 20, 20, radius=3.0, jitter=0.3, focal=22.0)
        return dict(extent_cells=(9.5, 14.5, 11.5), rays_o=ro, rays_d=rd, imsz=[1, 1, 1], near=0.2, stepsize=0.5, downrate=1, irregular_shape=False)
    if name == 'cubic_24x17_downrate2':                      # the literal slice on [1, H, W, 3] pieces, stepsize 1.0, rays that miss the box
        rng = np.random.default_rng(12)
        ro, rd = _look_at_rays(rng, 3, 24, 17, radius=3.5, jitter=1.5, focal=12.0)
        return dict(extent_cells=(12.5, 12.5, 12.5), rays_o=ro, rays_d=rd, imsz=[1, 1, 1], near=0.2, stepsize=1.0, downrate=2, irregular_shape=False)
    if name == 'irregular_unequal_views_inside_camera':      # unequal imsz, exactly-zero direction components, a camera inside the box (t_min = near)
        rng = np.random.default_rng(13)
        a = _look_at_rays(rng, 1, 20, 20, radius=3.0, jitter=0.2, focal=20.0)
        b = _look_at_rays(rng, 1, 24, 17, radius=0.4, jitter=0.1, focal=9.0)          # inside the 1.9 x 2.9 x 2.3 box
        c = _look_at_rays(rng, 1, 13, 11, radius=2.5, jitter=0.2, focal=10.0)
        ro = np.concatenate([x[0].reshape(-1, 3) for x in (a, b, c)])
        rd = np.concatenate([x[1].reshape(-1, 3) for x in (a, b, c)])
        axis = np.zeros([60, 3], np.float32)                                          # axis-parallel rays through the box: two zero components each
        axis[:, 0] = 1.0
        axis_o = np.stack([np.full(60, -3.0), rng.uniform(-1.2, 1.2, 60), rng.uniform(-1.0, 1.0, 60)], -1).astype(np.float32)
        rd[5::7][:40, 1] = 0.0                                                        # and single zero components among ordinary rays
        ro, rd = np.concatenate([ro, axis_o]), np.concatenate([rd, axis])
        return dict(extent_cells=(9.5, 14.5, 11.5), rays_o=ro, rays_d=rd, imsz=[400, 408, 143 + 60], near=0.05, stepsize=0.5, downrate=1,
                    irregular_shape=True)
    if name == 'no_wrap_64x64_identical':                    # thousands of equal contributions on a few voxels of a 4^3 grid
        o = np.tile(np.array([[-2.0, 0.07, -0.11]], np.float32), (2 * 64 * 64, 1)).reshape(2, 64, 64, 3)
        d = np.tile(np.array([[1.0, 0.02, 0.03]], np.float32), (2 * 64 * 64, 1)).reshape(2, 64, 64, 3)
        return dict(extent_cells=(4.5, 4.5, 4.5), rays_o=o, rays_d=d, imsz=[1, 1], near=0.2, stepsize=0.5, downrate=1, irregular_shape=False)
    raise KeyError(name)


COUNT_CASES = ('noncubic_3views_20x20', 'cubic_24x17_downrate2', 'irregular_unequal_views_inside_camera', 'no_wrap_64x64_identical')


def world_of(kw):
    """world_size and voxel_size of DirectVoxGO._set_grid_resolution for these kwargs, in the fp32 the model uses."""
    import torch
    lo, hi = torch.Tensor(kw['xyz_min']), torch.Tensor(kw['xyz_max'])
    voxel_size = ((hi - lo).prod() / kw['num_voxels']).pow(1 / 3)
    return ((hi - lo) / voxel_size).long().tolist(), float(voxel_size)


def oracle_of_case(case):
    kw = dvgo_kwargs(case['extent_cells'])
    world, voxel_size = world_of(kw)
    sums = count_sums(case['rays_o'], case['rays_d'], case['imsz'], kw['xyz_min'], kw['xyz_max'], world, case['near'], case['stepsize'], voxel_size,
                      case['downrate'], case['irregular_shape'])
    return kw, world, sums


def golden_occ():
    """tests/golden/occ_dvgo.npz: (checkpoint dict, render kwargs, the npz)"""
    import torch
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'occ_dvgo.npz'))
    kw = json.loads(str(z['model_kwargs_json']))
    for k in ('xyz_min', 'xyz_max'):
        kw[k] = np.asarray(kw[k], dtype=np.float32)
    ck = {'model_class': str(z['model_class']), 'model_kwargs': kw,
          'model_state_dict': {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith('sd/')}}
    return ck, json.loads(str(z['render_kwargs_json'])), z


# ---------------------------------------------------------------- coarse-geometry scenes: (extent_cells, seed, thres)
GEO_CASES = {'cubic_12': ((12.5, 12.5, 12.5), 21, 1e-3), 'noncubic_9x14x11': ((9.5, 14.5, 11.5), 22, 1e-3)}


def geo_density(world, seed):
    """A blob of raised density well inside an [X, Y, Z] grid over a low floor, float32."""
    rng = np.random.default_rng(seed)
    ax = [np.linspace(-1, 1, n) for n in world]
    X, Y, Z = np.meshgrid(*ax, indexing='ij')
    c = rng.uniform(-0.25, 0.25, 3)
    s = rng.uniform(0.25, 0.4, 3)
    field = 14.0 * np.exp(-0.5 * (((X - c[0]) / s[0]) ** 2 + ((Y - c[1]) / s[1]) ** 2 + ((Z - c[2]) / s[2]) ** 2)) - 8.0
    return (field + rng.normal(scale=0.3, size=field.shape)).astype(np.float32)


def geo_oracle(density, act_shift, interval, thres):
    """-> (six indices or None, smallest relative distance of any node's float64 alpha to thres)"""
    alpha = raw2alpha(density, float(act_shift), float(interval))
    idx = np.argwhere(alpha > thres)
    margin = float(np.abs(alpha / thres - 1).min())
    return (None if len(idx) == 0 else idx.min(0).tolist() + idx.max(0).tolist()), margin
