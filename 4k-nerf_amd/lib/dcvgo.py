"""DirectContractedVoxGO with the reference's interface (/root/reference/lib/dcvgo.py), on the gfx950 staged kernels.

The contracted-space DVGO of ``run.py`` / ``run_sr.py`` for unbounded, inward-facing 360-degree captures (``cfg.data.unbounded_inward``).
Kept verbatim from the reference contract: constructor kwargs, ``get_kwargs()`` (which, as upstream, omits ``bg_len``: a reload uses
0.2), registered buffers and ``state_dict`` keys (``scene_center``, ``scene_radius``, ``xyz_min`` / ``xyz_max`` = -/+(1 + bg_len),
``act_shift``, ``density.*``, ``k0.*``, ``viewfreq``, ``rgbnet.*``, ``mask_cache.*``), ``sample_ray`` -> ``(ray_pts, inner_mask, t)``,
``forward(rays_o, rays_d, viewdirs, global_step=None, is_train=False, **render_kwargs)`` and the module-level names
``ub360_utils_cuda``, ``DistortionLoss``, ``distortion_loss``.

``forward`` is the reference's op sequence (lib/dcvgo.py:255-383) with every per-sample stage on a HIP op: the contraction of the sample
table (device tensor expressions, the reference's own), ``cumdist_thres`` (k4_cumdist_thres), compaction, ``mask_cache``
(k4_maskcache_lookup), density / k0 lookups (k4_grid_sample_3d and its backward), ``Raw2Alpha``, ``Alphas2Weights``, the colour MLP
(k4_rgbnet_fwd / _bwd) and the ``segment_coo`` sums (k4_segment_sum).  It returns every key of lib/dcvgo.py:358-380 and, as the
reference's DirectVoxGO does (lib/dvgo.py:424-427), ``rgb_feature`` -- the same tensor as ``rgb_marched``.  That is the path of autograd
and of ``render_kwargs['k4_staged']=True``.  Inference (``torch.no_grad``, an rgbnet of width 32 / 64 / 128 and depth 2 / 3, or the coarse
k0 colour grid) is ONE launch of k4_march_contracted_fwd with the same stages and arithmetic, returning ``alphainv_last``, ``rgb_marched``
(= ``rgb_feature``) and ``depth``.
There is no CPU path: CPU tensors raise ``K4Error``.
"""
import numpy as np
import torch
import torch.nn as nn

from .. import _native as N
from . import grid
from .dvgo import Raw2Alpha, Alphas2Weights      # noqa: F401  (names the reference's module exports)
from .dvgo import _VoxGOCommon, _take, _rgbnet_stack, create_full_step_id, segment_sum
from . import train_ops


class _Ub360Utils:
    """Drop-in for the reference's JIT-built ``ub360_utils_cuda`` (lib/cuda/ub360_utils.cpp): the one entry point it defines."""

    @staticmethod
    def cumdist_thres(dist, thres):
        """mask[r, i] = the running sum of dist[r, :i+1] since the last reset exceeds ``thres`` (and resets); bool [n_rays, n_pts]."""
        if not dist.is_cuda:
            raise N.K4Error('cumdist_thres: tensor must be on the GPU (no CPU path exists for this op)')
        d = dist.detach().float().contiguous()
        if d.dim() != 2:
            raise ValueError('cumdist_thres: dist must be [n_rays, n_pts]')
        mask = torch.empty(d.shape, dtype=torch.bool, device=d.device)
        N.check(N.lib().k4_cumdist_thres(N.f32(d), d.shape[0], d.shape[1], float(thres), N.ptr(mask), N.stream()), 'k4_cumdist_thres')
        return mask


ub360_utils_cuda = _Ub360Utils()


'''Model'''
class DirectContractedVoxGO(nn.Module, _VoxGOCommon):
    def __init__(self, xyz_min, xyz_max,
                 num_voxels=0, num_voxels_base=0,
                 alpha_init=None,
                 mask_cache_world_size=None,
                 fast_color_thres=0, bg_len=0.2,
                 contracted_norm='inf',
                 density_type='DenseGrid', k0_type='DenseGrid',
                 density_config={}, k0_config={},
                 rgbnet_dim=0,
                 rgbnet_depth=3, rgbnet_width=128,
                 viewbase_pe=4,
                 **kwargs):
        super(DirectContractedVoxGO, self).__init__()
        # xyz_min/max are the boundary that separates fg and bg scene (lib/dcvgo.py:42-49; the reference's cube assertion is vacuous)
        xyz_min = torch.Tensor(np.asarray(xyz_min, dtype=np.float32))
        xyz_max = torch.Tensor(np.asarray(xyz_max, dtype=np.float32))
        self.register_buffer('scene_center', (xyz_min + xyz_max) * 0.5)
        self.register_buffer('scene_radius', (xyz_max - xyz_min) * 0.5)
        self.register_buffer('xyz_min', torch.Tensor([-1, -1, -1]) - bg_len)
        self.register_buffer('xyz_max', torch.Tensor([1, 1, 1]) + bg_len)
        if isinstance(fast_color_thres, dict):
            self._fast_color_thres = fast_color_thres
            self.fast_color_thres = fast_color_thres[0]
        else:
            self._fast_color_thres = None
            self.fast_color_thres = fast_color_thres
        self.bg_len = bg_len
        self.contracted_norm = contracted_norm
        if contracted_norm not in ('inf', 'l2'):
            raise NotImplementedError(f'contracted_norm={contracted_norm!r}')

        # base grid resolution (lib/dcvgo.py:60-62): host float32 arithmetic, as the reference evaluates it at construction
        self.num_voxels_base = num_voxels_base
        self.voxel_size_base = ((self.xyz_max - self.xyz_min).prod() / self.num_voxels_base).pow(1 / 3)
        self._set_grid_resolution(num_voxels)

        self.alpha_init = alpha_init
        self.register_buffer('act_shift', torch.FloatTensor([np.log(1 / (1 - alpha_init) - 1)]))

        self.density_type = density_type
        self.density_config = density_config
        self.density = grid.create_grid(
            density_type, channels=1, world_size=self.world_size,
            xyz_min=self.xyz_min, xyz_max=self.xyz_max, config=self.density_config)

        self.rgbnet_kwargs = {
            'rgbnet_dim': rgbnet_dim,
            'rgbnet_depth': rgbnet_depth, 'rgbnet_width': rgbnet_width,
            'viewbase_pe': viewbase_pe,
        }
        self.k0_type = k0_type
        self.k0_config = k0_config
        if rgbnet_dim <= 0:
            # colour voxel grid (coarse stage, lib/dcvgo.py:87-94)
            self.k0_dim = 3
            self.k0 = grid.create_grid(
                k0_type, channels=self.k0_dim, world_size=self.world_size,
                xyz_min=self.xyz_min, xyz_max=self.xyz_max, config=self.k0_config)
            self.rgbnet = None
        else:
            # feature voxel grid + shallow MLP (fine stage, lib/dcvgo.py:95-114): direct, features [k0, viewdirs, sin, cos]
            self.k0_dim = rgbnet_dim
            self.k0 = grid.create_grid(
                k0_type, channels=self.k0_dim, world_size=self.world_size,
                xyz_min=self.xyz_min, xyz_max=self.xyz_max, config=self.k0_config)
            self.register_buffer('viewfreq', torch.FloatTensor([(2 ** i) for i in range(viewbase_pe)]))
            dim0 = (3 + 3 * viewbase_pe * 2)
            dim0 += self.k0_dim
            self.rgbnet = _rgbnet_stack(dim0, rgbnet_width, rgbnet_depth)

        # occupancy grid (lib/dcvgo.py:116-123)
        if mask_cache_world_size is None:
            mask_cache_world_size = self.world_size
        mask = torch.ones(list(mask_cache_world_size), dtype=torch.bool)
        self.mask_cache = grid.MaskGrid(path=None, mask=mask, xyz_min=self.xyz_min, xyz_max=self.xyz_max)

    def _set_grid_resolution(self, num_voxels):
        """lib/dcvgo.py:125-131: float32 torch arithmetic on the host, truncated by .long() -- evaluated on host copies of the bbox so that a
        model living on the GPU grows to the same world_size the reference computes."""
        lo, hi = self.xyz_min.detach().cpu(), self.xyz_max.detach().cpu()
        self.num_voxels = num_voxels
        self.voxel_size = ((hi - lo).prod() / num_voxels).pow(1 / 3)
        self.world_size = ((hi - lo) / self.voxel_size).long()
        self.world_len = self.world_size[0].item()
        self.voxel_size_ratio = self.voxel_size / self.voxel_size_base.cpu()

    def get_kwargs(self):
        return {
            'xyz_min': self.xyz_min.cpu().numpy(),
            'xyz_max': self.xyz_max.cpu().numpy(),
            'num_voxels': self.num_voxels,
            'num_voxels_base': self.num_voxels_base,
            'alpha_init': self.alpha_init,
            'voxel_size_ratio': self.voxel_size_ratio,
            'mask_cache_world_size': list(self.mask_cache.mask.shape),
            'fast_color_thres': self.fast_color_thres,
            'contracted_norm': self.contracted_norm,
            'density_type': self.density_type,
            'k0_type': self.k0_type,
            'density_config': self.density_config,
            'k0_config': self.k0_config,
            **self.rgbnet_kwargs,
        }

    # ------------------------------------------------------------------ resolution / occupancy maintenance (training loop)
    @torch.no_grad()
    def scale_volume_grid(self, num_voxels):
        """Progressive growing (lib/dcvgo.py:156-178): resample density / k0 (k4_resample_trilinear); while the grid is <= 256^3 the
        occupancy becomes old mask at the new nodes AND max-pooled alpha > fast_color_thres (k4_alpha_maxpool3_gt)."""
        self._set_grid_resolution(num_voxels)
        self.density.scale_volume_grid(self.world_size)
        self.k0.scale_volume_grid(self.world_size)
        self._k4_regrow_mask_cache()

    def update_occupancy_cache_lt_nviews(self, rays_o_tr, rays_d_tr, imsz, render_kwargs, maskout_lt_nviews):
        """lib/dcvgo.py:194-211: keep the voxels that at least ``maskout_lt_nviews`` training views sample (gradient of an all-ones grid > 1)."""
        count = torch.zeros_like(self.density.get_dense_grid()).long()
        device = count.device
        for rays_o_, rays_d_ in zip(rays_o_tr.split(imsz), rays_d_tr.split(imsz)):
            ones = grid.DenseGrid(1, self.world_size, self.xyz_min, self.xyz_max).to(device)
            for rays_o, rays_d in zip(rays_o_.split(8192), rays_d_.split(8192)):
                ray_pts, inner_mask, t = self.sample_ray(
                    ori_rays_o=rays_o.to(device), ori_rays_d=rays_d.to(device), **render_kwargs)
                with torch.enable_grad():
                    ones(ray_pts).sum().backward()
            with torch.no_grad():
                count.data += (ones.grid.grad > 1)
        with torch.no_grad():
            self.mask_cache.mask &= (count >= maskout_lt_nviews)[0, 0]

    # ------------------------------------------------------------------ sampling
    def _step_table(self, stepsize, device):
        """t of every step (lib/dcvgo.py:239-247) built on the host with the reference's own expressions, cached per (stepsize, world_len, bg_len)."""
        c = self._k4_cache()
        key = ('t_tab', float(stepsize), int(self.world_len), float(self.bg_len), str(device))
        if c.get('t_key') != key:
            N_inner = int(2 / (2 + 2 * self.bg_len) * self.world_len / stepsize) + 1
            N_outer = N_inner
            b_inner = torch.linspace(0, 2, N_inner + 1)
            b_outer = 2 / torch.linspace(1, 1 / 128, N_outer + 1)
            t = torch.cat([
                (b_inner[1:] + b_inner[:-1]) * 0.5,
                (b_outer[1:] + b_outer[:-1]) * 0.5,
            ])
            s = 1 - (1 + t).reciprocal()                   # lib/dcvgo.py:357 per step
            c['t_key'], c['t_tab'], c['s_tab'] = key, t.to(device), s.to(device)
        return c['t_tab']

    def _step_tables(self, stepsize, device):
        """(t_tab, s_tab) of the fused kernel: the step table and s = 1 - 1/(1+t) per step, built once per plan on the host."""
        t = self._step_table(stepsize, device)
        return t, self._k4_cache()['s_tab']

    def sample_ray(self, ori_rays_o, ori_rays_d, stepsize, is_train=False, **render_kwargs):
        '''Sample query points on rays (lib/dcvgo.py:213-253), sorted near to far, in the contracted space.
        -> ray_pts [N, n_max, 3], inner_mask [N, n_max] (norm <= 1), t [n_max].'''
        if not ori_rays_o.is_cuda:
            raise N.K4Error('sample_ray: rays must be on the GPU (no CPU path)')
        rays_o = (ori_rays_o - self.scene_center) / self.scene_radius
        rays_d = ori_rays_d / ori_rays_d.norm(dim=-1, keepdim=True)
        t = self._step_table(stepsize, rays_o.device)
        ray_pts = rays_o[:, None, :] + rays_d[:, None, :] * t[None, :, None]
        if self.contracted_norm == 'inf':
            norm = ray_pts.abs().amax(dim=-1, keepdim=True)
        else:
            norm = ray_pts.norm(dim=-1, keepdim=True)
        inner_mask = (norm <= 1)
        ray_pts = torch.where(
            inner_mask,
            ray_pts,
            ray_pts / norm * ((1 + self.bg_len) - norm.reciprocal() * self.bg_len)      # `bg_len/norm` as torch evaluates it (Tensor.__rdiv__)
        )
        return ray_pts, inner_mask.squeeze(-1), t

    # ------------------------------------------------------------------ forward
    def forward(self, rays_o, rays_d, viewdirs, global_step=None, is_train=False, **render_kwargs):
        '''Volume rendering
        @rays_o:   [N, 3] the starting point of the N shooting rays.
        @rays_d:   [N, 3] the shooting direction of the N rays.
        @viewdirs: [N, 3] viewing direction to compute positional embedding for MLP.
        '''
        rays_o, rays_d, viewdirs = self._k4_check_rays(rays_o, rays_d, viewdirs)
        if isinstance(self._fast_color_thres, dict) and global_step in self._fast_color_thres:
            self.fast_color_thres = self._fast_color_thres[global_step]
        self._k4_params_ready()
        if render_kwargs.get('k4_staged', False) or torch.is_grad_enabled() or not self._k4_fusable():
            return self._forward_staged(rays_o, rays_d, viewdirs, global_step=global_step, is_train=is_train, **render_kwargs)
        return self._forward_fused(rays_o, rays_d, viewdirs, **render_kwargs)

    def _forward_fused(self, rays_o, rays_d, viewdirs, stepsize, bg=0, render_depth=False, k4_counters=None, **_ignored):
        """Inference in one launch (k4_march_contracted_fwd): the same stages and arithmetic as the staged path, nothing per sample in memory.
        Returns alphainv_last, rgb_marched (= rgb_feature) and, with render_depth, depth."""
        Nr = rays_o.shape[0]
        dev = rays_o.device
        rgb, depth, ainv, ret = self._k4_ray_outputs(Nr, dev, render_depth)
        if Nr == 0:
            return ret

        def build():
            t_tab, s_tab = self._step_tables(stepsize, dev)
            d = N.ContractedDesc()
            d.t_tab, d.s_tab, d.n_max = t_tab.data_ptr(), s_tab.data_ptr(), int(t_tab.numel())
            d.scene_center = N.vec3(self.scene_center)
            d.scene_radius = N.vec3(self.scene_radius)
            d.bg_len = float(self.bg_len)
            d.dist_thres = float((2 + 2 * self.bg_len) / self.world_len * stepsize * 0.95)        # lib/dcvgo.py:300
            d.norm_l2 = int(self.contracted_norm == 'l2')
            dens, k0 = self._k4_dense(self.density).detach().contiguous(), self._k4_dense(self.k0).detach().contiguous()
            mc = self.mask_cache
            mask = mc.mask.contiguous()
            d.density, d.k0, d.k0_ch = dens.data_ptr(), k0.data_ptr(), int(k0.shape[1])
            d.dims = (N.C.c_int32 * 3)(*[int(v) for v in dens.shape[2:]])
            d.xyz_min, d.xyz_max = self.xyz_min.data_ptr(), self.xyz_max.data_ptr()
            d.mask, d.mask_dims = mask.data_ptr(), (N.C.c_int32 * 3)(*[int(v) for v in mask.shape])
            d.xyz2ijk_scale, d.xyz2ijk_shift = mc.xyz2ijk_scale.data_ptr(), mc.xyz2ijk_shift.data_ptr()
            d.act_shift = self._k4_host_scalar('act_shift', self.act_shift)
            d.interval = float(stepsize * self.voxel_size_ratio)                                    # lib/dcvgo.py:280
            d.fast_color_thres = float(self.fast_color_thres)
            keep = [t_tab, s_tab, dens, k0, mask]
            if self.rgbnet is None:
                d.width = 0
            else:
                ws, (d.dim0, d.width, d.n_hidden) = self._k4_rgbnet_into(self.rgbnet, d)
                keep += ws
                d.viewfreq, d.n_pe = self.viewfreq.data_ptr(), int(self.viewfreq.numel())
            return d, keep
        d = self._k4_plan('dcvgo', (float(stepsize), float(self.fast_color_thres), float(self.bg_len), int(self.world_len),
                                    self.contracted_norm, float(self.voxel_size_ratio)) + tuple(
            (t.data_ptr(), t._version) for t in (self.scene_center, self.scene_radius)), build)
        d.rays_o, d.rays_d, d.viewdirs, d.n_rays = rays_o.data_ptr(), rays_d.data_ptr(), viewdirs.data_ptr(), Nr
        d.bg = float(bg)
        d.rgb, d.depth, d.alphainv_last = rgb.data_ptr(), depth.data_ptr(), ainv.data_ptr()
        d.counters = self._k4_counters_ptr(k4_counters, 4)
        N.check(N.lib().k4_march_contracted_fwd(N.C.byref(d), N.stream()), 'k4_march_contracted_fwd')
        return ret

    def _forward_staged(self, rays_o, rays_d, viewdirs, stepsize, bg=0, global_step=None, is_train=False, render_depth=False,
                        rand_bkgd=False, **_ignored):
        """The reference's op sequence (lib/dcvgo.py:266-383) on the staged gfx950 kernels."""
        ret_dict = {}
        Nr = len(rays_o)
        dev = rays_o.device

        # sample points on rays
        ray_pts, inner_mask, t = self.sample_ray(ori_rays_o=rays_o, ori_rays_d=rays_d, stepsize=stepsize, is_train=global_step is not None)
        n_max = len(t)
        interval = stepsize * self.voxel_size_ratio
        ray_id, step_id = create_full_step_id(ray_pts.shape[:2], device=dev)

        # skip oversampled points outside scene bbox
        mask = inner_mask.clone()
        dist_thres = (2 + 2 * self.bg_len) / self.world_len * stepsize * 0.95
        dist = (ray_pts[:, 1:] - ray_pts[:, :-1]).norm(dim=-1)
        mask[:, 1:] |= ub360_utils_cuda.cumdist_thres(dist, dist_thres)
        keep = mask.flatten()
        ray_pts, inner_mask, t, ray_id, step_id = _take(
            keep, ray_pts.reshape(-1, 3), inner_mask.flatten(), t[None].expand(Nr, n_max).flatten(), ray_id, step_id)

        # skip known free space, alpha and weights below the threshold (lib/dcvgo.py:306-328); then the colour (lib/dcvgo.py:330-341)
        ray_pts, ray_id, (inner_mask, t, step_id), alpha, weights, alphainv_last, density = self._k4_filter_samples(
            ray_pts, ray_id, (inner_mask, t, step_id), interval, Nr, self.mask_cache, self.density, keep_density=True)
        rgb = self._k4_shade(self.k0(ray_pts), viewdirs, ray_id, self.rgbnet)

        # Ray marching
        rgb_marched = segment_sum(weights.unsqueeze(-1) * rgb, ray_id, Nr)
        if rand_bkgd and is_train:
            rgb_marched += (alphainv_last.unsqueeze(-1) * torch.rand_like(rgb_marched))
        else:
            rgb_marched += (alphainv_last.unsqueeze(-1) * bg)
        im = inner_mask.nonzero().squeeze(1)
        wsum_mid = segment_sum(weights.index_select(0, im), ray_id.index_select(0, im), Nr)
        s = 1 - (1 + t).reciprocal()  # [0, inf] => [0, 1]      (`1/(1+t)` as torch evaluates it)
        ret_dict.update({
            'alphainv_last': alphainv_last,
            'weights': weights,
            'wsum_mid': wsum_mid,
            'rgb_marched': rgb_marched,
            'rgb_feature': rgb_marched,           # alias, as DirectVoxGO returns it (lib/dvgo.py:424-427)
            'raw_density': density,
            'raw_alpha': alpha,
            'raw_rgb': rgb,
            'ray_id': ray_id,
            'step_id': step_id,
            'n_max': n_max,
            't': t,
            's': s,
        })
        if render_depth:
            with torch.no_grad():
                ret_dict['depth'] = segment_sum(weights * s, ray_id, Nr)
        return ret_dict


class DistortionLoss:
    """lib/dcvgo.py:385-408 on k4_distortion_loss (the per-ray form of torch_efficient_distloss.flatten_eff_distloss, lib/train_ops.py):
        loss = sum_i [ interval/3 w_i^2 + 2 w_i (s_i P_i - Q_i) ] / (max(ray_id) + 1),  interval = 1 / n_max,
    P / Q the exclusive prefix sums of w / w*s along each ray; differentiable w.r.t. ``w``.  The reference's own forward calls
    ``ub360_utils_cuda.segment_cumsum``, which its native extension never defines (lib/cuda/ub360_utils.cpp exports cumdist_thres only),
    so the class cannot run there.  This one computes the formula that call was written for; there is no ``segment_cumsum`` entry point."""

    @staticmethod
    def apply(w, s, n_max, ray_id):
        return train_ops.flatten_eff_distloss(w, s, 1 / n_max, ray_id)


distortion_loss = DistortionLoss.apply
