"""DirectBiVoxGO with the reference's interface (/root/reference/lib/dbvgo.py), on the gfx950 kernels.

The two-grid model for unbounded scenes: a foreground DirectVoxGO inside the unit cube of the normalised scene and a second grid sampled
along an inverse-sphere background parameterisation (``render_utils_cuda.sample_bg_pts_on_rays``).  Kept from the reference contract:
constructor kwargs and defaults, registered buffers and ``state_dict`` keys (``scene_center``, ``scene_radius``, ``xyz_min`` / ``xyz_max``
= -/+1, ``act_shift``, ``viewfreq``, ``density.{0,1}.*``, ``k0.{0,1}.*``, ``mask_cache.{0,1}.*``, ``rgbnet.{0,1}.*``),
``sample_ray`` -> ``(ray_pts, ray_id, step_id, ray_pts_outer)`` and ``forward(rays_o, rays_d, viewdirs, global_step=None, **render_kwargs)``.
``get_kwargs()`` returns the reference's keys and, unlike upstream, ``bg_preserve`` and ``bg_use_mlp``.

``forward`` under autograd or with ``render_kwargs['k4_staged']=True`` is the reference's op sequence (lib/dbvgo.py:310-397) with every
per-sample stage on a HIP op and returns every key of lib/dbvgo.py:360-395 plus ``rgb_feature`` (the same tensor as ``rgb_marched``).
Inference (``torch.no_grad``, rgbnets of width 32 / 64 / 128 and depth 2 / 3, or none) is ONE launch of k4_march_bivox_fwd with the same
stages and arithmetic, returning ``rgb_marched`` (= ``rgb_feature``), ``alphainv_last`` (``cat([fg, bg])``, 2N) and ``depth``.
With ``rgbnet_dim <= 0`` upstream builds ``self.rgbnet = None`` and then indexes it in ``forward``; here both passes take the
``rgbnet=None`` branch of ``_forward`` (sigmoid(k0)).  There is no CPU path: CPU tensors raise ``K4Error``.
"""
import numpy as np
import torch
import torch.nn as nn

from .. import _native as N
from . import grid
from .dvgo import Raw2Alpha, Alphas2Weights      # noqa: F401  (names the reference's module exports)
from .dvgo import _VoxGOCommon, _take, _rgbnet_stack, create_full_step_id, segment_sum, render_utils_cuda


def segment_max(src, index, out):
    """torch_scatter.segment_coo(src, index, out=out, reduce='max') (lib/dbvgo.py:382-391): the tensor library's scatter_reduce_(amax) on the
    device, in place on ``out`` (a few thousand elements under no_grad)."""
    return out.scatter_reduce_(0, index, src, reduce='amax', include_self=True)


'''Model'''
class DirectBiVoxGO(nn.Module, _VoxGOCommon):
    def __init__(self, xyz_min, xyz_max,
                 num_voxels=0, num_voxels_base=0,
                 alpha_init=None,
                 mask_cache_world_size=None,
                 fast_color_thres=0, bg_preserve=0.5,
                 density_type='DenseGrid', k0_type='DenseGrid',
                 density_config={}, k0_config={},
                 rgbnet_dim=0, bg_use_mlp=True,
                 rgbnet_depth=3, rgbnet_width=128,
                 viewbase_pe=4,
                 **kwargs):
        super(DirectBiVoxGO, self).__init__()
        xyz_min = torch.Tensor(np.asarray(xyz_min, dtype=np.float32))
        xyz_max = torch.Tensor(np.asarray(xyz_max, dtype=np.float32))
        self.register_buffer('scene_center', (xyz_min + xyz_max) * 0.5)
        self.register_buffer('scene_radius', (xyz_max - xyz_min) * 0.5)
        self.register_buffer('xyz_min', torch.Tensor([-1, -1, -1]))
        self.register_buffer('xyz_max', torch.Tensor([1, 1, 1]))
        self.fast_color_thres = fast_color_thres
        self.bg_preserve = bg_preserve
        self.bg_use_mlp = bg_use_mlp

        # base grid resolution (lib/dbvgo.py:41-43): host float32 arithmetic, as the reference evaluates it at construction
        self.num_voxels_base = num_voxels_base
        self.voxel_size_base = ((self.xyz_max - self.xyz_min).prod() / self.num_voxels_base).pow(1 / 3)

        self.alpha_init = alpha_init
        self.register_buffer('act_shift', torch.FloatTensor([np.log(1 / (1 - alpha_init) - 1)]))

        self._set_grid_resolution(num_voxels)

        def new_grid(type_, channels, config):
            return grid.create_grid(type_, channels=channels, world_size=self.world_size,
                                    xyz_min=self.xyz_min, xyz_max=self.xyz_max, config=config)

        self.density_type = density_type
        self.density_config = density_config
        self.density = nn.ModuleList([new_grid(density_type, 1, self.density_config) for _ in range(2)])

        self.rgbnet_kwargs = {
            'rgbnet_dim': rgbnet_dim,
            'rgbnet_depth': rgbnet_depth, 'rgbnet_width': rgbnet_width,
            'viewbase_pe': viewbase_pe,
        }
        self.k0_type = k0_type
        self.k0_config = k0_config
        if rgbnet_dim <= 0:
            # colour voxel grids (coarse stage, lib/dbvgo.py:72-82)
            self.k0_dim = 3
            self.k0 = nn.ModuleList([new_grid(k0_type, self.k0_dim, self.k0_config) for _ in range(2)])
            self.rgbnet = None
        else:
            # feature voxel grids + shallow MLPs (fine stage, lib/dbvgo.py:83-114): features [k0, viewdirs, sin, cos]
            self.k0_dim = rgbnet_dim
            self.k0 = nn.ModuleList([new_grid(k0_type, self.k0_dim, self.k0_config) for _ in range(2)])
            self.register_buffer('viewfreq', torch.FloatTensor([(2 ** i) for i in range(viewbase_pe)]))
            dim0 = (3 + 3 * viewbase_pe * 2)
            dim0 += self.k0_dim
            self.rgbnet = nn.ModuleList([_rgbnet_stack(dim0, rgbnet_width, rgbnet_depth) for _ in range(2)])
            if not bg_use_mlp:
                self.k0[1] = new_grid(k0_type, 3, self.k0_config)
                self.rgbnet[1] = None

        # occupancy grids (lib/dbvgo.py:118-128)
        if mask_cache_world_size is None:
            mask_cache_world_size = self.world_size
        mask = torch.ones(list(mask_cache_world_size), dtype=torch.bool)
        self.mask_cache = nn.ModuleList([
            grid.MaskGrid(path=None, mask=mask.clone(), xyz_min=self.xyz_min, xyz_max=self.xyz_max)      # a tensor each: upstream registers ONE in
            for _ in range(2)                                                                               # both, and a strict load on the CPU
        ])                                                                                                  # leaves both with the background's mask

    def _set_grid_resolution(self, num_voxels):
        """lib/dbvgo.py:130-139: float32 torch arithmetic on the host, truncated by .long() -- evaluated on host copies of the bbox so that a
        model living on the GPU grows to the same world_size the reference computes."""
        lo, hi = self.xyz_min.detach().cpu(), self.xyz_max.detach().cpu()
        self.num_voxels = num_voxels
        self.voxel_size = ((hi - lo).prod() / num_voxels).pow(1 / 3)
        self.world_size = ((hi - lo) / self.voxel_size).long()
        self.voxel_size_ratio = self.voxel_size / self.voxel_size_base.cpu()

    def get_kwargs(self):
        return {
            'xyz_min': self.xyz_min.cpu().numpy(),
            'xyz_max': self.xyz_max.cpu().numpy(),
            'num_voxels': self.num_voxels,
            'num_voxels_base': self.num_voxels_base,
            'alpha_init': self.alpha_init,
            'voxel_size_ratio': self.voxel_size_ratio,
            'mask_cache_world_size': list(self.mask_cache[0].mask.shape),
            'fast_color_thres': self.fast_color_thres,
            'bg_preserve': self.bg_preserve,           # (upstream drops these two: a reload renders with 0.5 and cannot load a
            'bg_use_mlp': self.bg_use_mlp,             #  bg_use_mlp=False state_dict -- INTEGRATION.md)
            'density_type': self.density_type,
            'k0_type': self.k0_type,
            'density_config': self.density_config,
            'k0_config': self.k0_config,
            **self.rgbnet_kwargs,
        }

    def _rgbnet_of(self, i):
        return None if self.rgbnet is None else self.rgbnet[i]

    # ------------------------------------------------------------------ resolution / occupancy maintenance (training loop)
    @torch.no_grad()
    def scale_volume_grid(self, num_voxels):
        """Progressive growing (lib/dbvgo.py:158-187): resample both density / k0 pairs (k4_resample_trilinear); while the grid is <= 256^3 each
        occupancy is REPLACED by max-pooled alpha > fast_color_thres (k4_alpha_maxpool3_gt) -- not ANDed with the old mask, unlike dcvgo."""
        self._set_grid_resolution(num_voxels)
        for g in list(self.density) + list(self.k0):
            g.scale_volume_grid(self.world_size)
        if int(np.prod(self.world_size.tolist())) <= 256 ** 3:
            dev = self.xyz_min.device
            self.mask_cache = nn.ModuleList([
                grid.MaskGrid(path=None,
                              mask=grid.occupancy_from_alpha(self.activate_density(self.density[i].get_dense_grid())[0, 0], self.fast_color_thres),
                              xyz_min=self.xyz_min, xyz_max=self.xyz_max).to(dev)
                for i in range(2)
            ])

    # ------------------------------------------------------------------ sampling
    def _n_outer(self, stepsize):
        """lib/dbvgo.py:234,242: with the reference's host float32 ``stepdist.item()``."""
        stepdist = stepsize * self.voxel_size
        return stepdist, int(np.sqrt(3) / stepdist.item() * (1 - self.bg_preserve)) + 1

    def sample_ray(self, ori_rays_o, ori_rays_d, stepsize, is_train=False, **render_kwargs):
        '''Sample query points on rays (lib/dbvgo.py:217-245), sorted near to far.
        -> ray_pts [M, 3], ray_id [M], step_id [M] of the foreground samples inside the unit cube, ray_pts_outer [N, N_outer, 3].'''
        if not ori_rays_o.is_cuda:
            raise N.K4Error('sample_ray: rays must be on the GPU (no CPU path)')
        rays_o = ((ori_rays_o - self.scene_center) / self.scene_radius).contiguous()
        rays_d = (ori_rays_d / ori_rays_d.norm(dim=-1, keepdim=True)).contiguous()
        # sample query points in inter scene
        near = 0
        far = 2 * np.sqrt(3)
        stepdist, N_outer = self._n_outer(stepsize)
        ray_pts, mask_outbbox, ray_id, step_id, N_steps, t_min, t_max = render_utils_cuda.sample_pts_on_rays(
            rays_o, rays_d, self.xyz_min, self.xyz_max, near, far, stepdist)
        ray_pts, ray_id, step_id = _take(~mask_outbbox, ray_pts, ray_id, step_id)
        # sample query points in outer scene
        ray_pts_outer = render_utils_cuda.sample_bg_pts_on_rays(rays_o, rays_d, t_max, self.bg_preserve, N_outer)
        return ray_pts, ray_id, step_id, ray_pts_outer

    # ------------------------------------------------------------------ forward
    def _forward(self, ray_pts, viewdirs, interval, N_,
                 mask_grid, density_grid, k0_grid, rgbnet=None,
                 ray_id=None, step_id=None, prev_alphainv_last=None):
        """One pass of the staged path (lib/dbvgo.py:247-308) on the staged kernels."""
        # preprocess for bg queries
        if ray_id is None:
            # ray_pts is [N, M, 3] in bg query
            assert len(ray_pts.shape) == 3
            ray_id, step_id = create_full_step_id(ray_pts.shape[:2], device=ray_pts.device)
            ray_pts = ray_pts.reshape(-1, 3)

        # skip ray which is already occluded by fg
        if prev_alphainv_last is not None:
            rows = (prev_alphainv_last > self.fast_color_thres).nonzero().squeeze(1)
            ray_id = ray_id.view(N_, -1).index_select(0, rows).reshape(-1)
            step_id = step_id.view(N_, -1).index_select(0, rows).reshape(-1)
            ray_pts = ray_pts.view(N_, -1, 3).index_select(0, rows).reshape(-1, 3)

        # skip known free space, alpha and weights below the threshold (lib/dbvgo.py:270-292); then the colour (lib/dbvgo.py:294-304)
        ray_pts, ray_id, (step_id,), alpha, weights, alphainv_last, _ = self._k4_filter_samples(
            ray_pts, ray_id, (step_id,), interval, N_, mask_grid, density_grid)
        rgb = self._k4_shade(k0_grid(ray_pts), viewdirs, ray_id, rgbnet)

        return dict(
            rgb=rgb, alpha=alpha, weights=weights, alphainv_last=alphainv_last,
            ray_id=ray_id, step_id=step_id)

    def forward(self, rays_o, rays_d, viewdirs, global_step=None, **render_kwargs):
        '''Volume rendering
        @rays_o:   [N, 3] the starting point of the N shooting rays.
        @rays_d:   [N, 3] the shooting direction of the N rays.
        @viewdirs: [N, 3] viewing direction to compute positional embedding for MLP.
        '''
        rays_o, rays_d, viewdirs = self._k4_check_rays(rays_o, rays_d, viewdirs)
        self._k4_params_ready()
        if render_kwargs.get('k4_staged', False) or torch.is_grad_enabled() or not self._k4_fusable():
            return self._forward_staged(rays_o, rays_d, viewdirs, global_step=global_step, **render_kwargs)
        return self._forward_fused(rays_o, rays_d, viewdirs, **render_kwargs)

    def _forward_staged(self, rays_o, rays_d, viewdirs, stepsize, bg=0, global_step=None, render_depth=False, **_ignored):
        """The reference's op sequence (lib/dbvgo.py:318-397) on the staged gfx950 kernels."""
        ret_dict = {}
        Nr = len(rays_o)

        # sample points on rays
        ray_pts, ray_id, step_id, ray_pts_outer = self.sample_ray(
            ori_rays_o=rays_o, ori_rays_d=rays_d, stepsize=stepsize, is_train=global_step is not None)
        interval = stepsize * self.voxel_size_ratio

        # query for foreground
        fg = self._forward(
            ray_pts=ray_pts, viewdirs=viewdirs,
            interval=interval, N_=Nr,
            mask_grid=self.mask_cache[0],
            density_grid=self.density[0],
            k0_grid=self.k0[0],
            rgbnet=self._rgbnet_of(0),
            ray_id=ray_id, step_id=step_id)

        # query for background
        bgq = self._forward(
            ray_pts=ray_pts_outer, viewdirs=viewdirs,
            interval=interval, N_=Nr,
            mask_grid=self.mask_cache[1],
            density_grid=self.density[1],
            k0_grid=self.k0[1],
            rgbnet=self._rgbnet_of(1),
            prev_alphainv_last=fg['alphainv_last'])

        # Ray marching
        rgb_marched_fg = segment_sum(fg['weights'].unsqueeze(-1) * fg['rgb'], fg['ray_id'], Nr)
        rgb_marched_bg = segment_sum(bgq['weights'].unsqueeze(-1) * bgq['rgb'], bgq['ray_id'], Nr)
        rgb_marched = rgb_marched_fg + \
            fg['alphainv_last'].unsqueeze(-1) * rgb_marched_bg + \
            (fg['alphainv_last'] * bgq['alphainv_last']).unsqueeze(-1) * bg
        ret_dict.update({
            'rgb_marched': rgb_marched,
            'rgb_feature': rgb_marched,           # alias, as DirectVoxGO returns it (lib/dvgo.py:424-427)
            'alphainv_last': torch.cat([fg['alphainv_last'], bgq['alphainv_last']]),
            'weights': torch.cat([fg['weights'], bgq['weights']]),
            'raw_alpha': torch.cat([fg['alpha'], bgq['alpha']]),
            'raw_rgb': torch.cat([fg['rgb'], bgq['rgb']]),
            'ray_id': torch.cat([fg['ray_id'], bgq['ray_id']]),
        })

        if render_depth:
            with torch.no_grad():
                depth_fg = segment_sum(fg['weights'] * fg['step_id'], fg['ray_id'], Nr)
                depth_bg = segment_sum(bgq['weights'] * bgq['step_id'], bgq['ray_id'], Nr)
                depth_fg_last = segment_max(fg['step_id'].float(), fg['ray_id'], torch.zeros([Nr], device=rays_o.device))
                depth_bg_last = segment_max(bgq['step_id'].float(), bgq['ray_id'], depth_fg_last.clone())
                depth = depth_fg + \
                    fg['alphainv_last'] * (1 + depth_fg_last + depth_bg) + \
                    fg['alphainv_last'] * bgq['alphainv_last'] * (2 + depth_fg_last + depth_bg_last)
            ret_dict.update({'depth': depth})

        return ret_dict

    def _forward_fused(self, rays_o, rays_d, viewdirs, stepsize, bg=0, render_depth=False, k4_counters=None, **_ignored):
        """Inference in one launch (k4_march_bivox_fwd): both passes of a ray with the staged path's stages and arithmetic, nothing per sample in
        memory.  Returns alphainv_last (cat([fg, bg]), 2N), rgb_marched (= rgb_feature) and, with render_depth, depth."""
        Nr = rays_o.shape[0]
        dev = rays_o.device
        rgb, depth, ainv, ret = self._k4_ray_outputs(Nr, dev, render_depth, n_ainv=2)
        if Nr == 0:
            return ret

        def build():
            d = N.BivoxDesc()
            stepdist, n_outer = self._n_outer(stepsize)
            d.scene_center = N.vec3(self.scene_center)
            d.scene_radius = N.vec3(self.scene_radius)
            d.stepdist, d.far, d.bg_preserve, d.n_outer = float(stepdist), float(2 * np.sqrt(3)), float(self.bg_preserve), n_outer
            d.act_shift = self._k4_host_scalar('act_shift', self.act_shift)
            d.interval = float(stepsize * self.voxel_size_ratio)                                    # lib/dbvgo.py:324
            d.fast_color_thres = float(self.fast_color_thres)
            d.xyz_min, d.xyz_max = self.xyz_min.data_ptr(), self.xyz_max.data_ptr()
            keep = []
            if self.rgbnet is not None:
                d.viewfreq, d.n_pe = self.viewfreq.data_ptr(), int(self.viewfreq.numel())
            for i in range(2):
                dens = self._k4_dense(self.density[i]).detach().contiguous()
                k0 = self._k4_dense(self.k0[i]).detach().contiguous()
                mc = self.mask_cache[i]
                mask = mc.mask.contiguous()
                keep += [dens, k0, mask]
                d.density[i], d.k0[i], d.k0_ch[i] = dens.data_ptr(), k0.data_ptr(), int(k0.shape[1])
                d.mask[i], d.xyz2ijk_scale[i], d.xyz2ijk_shift[i] = mask.data_ptr(), mc.xyz2ijk_scale.data_ptr(), mc.xyz2ijk_shift.data_ptr()
                for a in range(3):
                    d.dims[i][a] = int(dens.shape[2 + a])
                    d.mask_dims[i][a] = int(mask.shape[a])
                net = self._rgbnet_of(i)
                if net is None:
                    d.width[i] = 0
                    continue
                ws, (d.dim0[i], d.width[i], d.n_hidden[i]) = self._k4_rgbnet_into(net, d, i)
                keep += ws
            return d, keep
        d = self._k4_plan('dbvgo', (float(stepsize), float(self.fast_color_thres), float(self.bg_preserve), float(self.voxel_size),
                                    float(self.voxel_size_ratio)) + tuple(
            (t.data_ptr(), t._version) for t in (self.scene_center, self.scene_radius)), build)
        d.rays_o, d.rays_d, d.viewdirs, d.n_rays = rays_o.data_ptr(), rays_d.data_ptr(), viewdirs.data_ptr(), Nr
        d.bg = float(bg)
        d.rgb, d.depth = rgb.data_ptr(), depth.data_ptr()
        d.alphainv_fg, d.alphainv_bg = ainv.data_ptr(), ainv.data_ptr() + 4 * Nr
        d.counters = self._k4_counters_ptr(k4_counters, 8)
        rc = N.lib().k4_march_bivox_fwd(N.C.byref(d), N.stream())
        if rc == N.K4_ERR_UNSUPPORTED:              # a shape outside the fused kernel: the staged ops
            return self._forward_staged(rays_o, rays_d, viewdirs, stepsize=stepsize, bg=bg, render_depth=render_depth)
        N.check(rc, 'k4_march_bivox_fwd')
        return ret
