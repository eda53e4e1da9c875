"""DirectQVGO: DirectMPIGO's geometry with a vector-quantised colour feature (/root/reference/lib/dvqgo.py).

Constructor kwargs and defaults, buffers, ``state_dict`` key names (``density.grid``, ``act_shift.grid``, ``k0.embed``, ``k0.cluster_size``,
``k0.embed_avg``, ``k0.project_layer.{0,2}.*``, ``rgbnet.*``, ``viewfreq``, ``posfreq``, ``mask_cache.*``) and
``forward(rays_o, rays_d, viewdirs, global_step=None, **render_kwargs) -> dict`` are the reference's (lib/dvqgo.py:19-142,279-408).  A shaded sample's
feature is not a trilinear lookup: its positional embedding goes through ``k0`` (lib/grid.VQGrid: two-layer projection, nearest of ``n_cluster``
codewords), and the rgbnet sees ``[vq_emb, pe_emb, viewdirs_emb]`` (lib/dvqgo.py:366).  Everything else -- sampling, occupancy, density, compositing,
the maintenance methods -- is DirectMPIGO's code.  Inference (no_grad, eval mode) is ONE launch (``k4_march_vq_fwd``: rgbnet width 32 / 64 / 128, depth 2 / 3) where that was measured to pay
(``_k4_one_launch_pays``; ``k4_fused=True`` asks for it at any covered shape);
autograd, ``k4_staged=True`` and training mode (which moves the codebook) run the reference's op sequence on the staged gfx950 kernels.  No CPU path.

What upstream cannot run raises here with the reason: ``mode_type`` 'TRANS' / 'adain' / 'adain_vq' (modules the reference never defines),
``viewbase_pe != 0`` (project_layer's input width counts a view embedding its input does not have, lib/dvqgo.py:82-86), ``rgbnet_dim <= 0`` (forward reads
``posfreq`` and calls a DenseGrid with an embedding), ``k0_total_variation_add_grad`` (VQGrid has no such method).  Unlike upstream, ``get_kwargs()`` also
returns ``n_cluster``: without it a checkpoint cannot be reloaded.
"""

import torch

from .. import _native as N
from . import grid
from . import train_ops
from .dmpigo import DirectMPIGO


'''Model'''
class DirectQVGO(DirectMPIGO):
    def __init__(self, xyz_min, xyz_max,
                 num_voxels=0, mpi_depth=0,
                 mask_cache_path=None, mask_cache_thres=1e-3, mask_cache_world_size=None,
                 fast_color_thres=0,
                 density_type='DenseGrid', k0_type='DenseGrid',
                 density_config={}, k0_config={},
                 rgbnet_dim=0,
                 rgbnet_depth=3, rgbnet_width=128,
                 viewbase_pe=0,
                 spatial_pe=0,
                 **kwargs):
        if rgbnet_dim <= 0:
            raise NotImplementedError(f'rgbnet_dim={rgbnet_dim}: upstream cannot run DirectQVGO without an rgbnet -- forward reads posfreq, which only exists '
                                      'with one, and calls a DenseGrid with an embedding (lib/dvqgo.py:70-77,322-327)')
        if viewbase_pe != 0:
            raise NotImplementedError(f'viewbase_pe={viewbase_pe}: upstream cannot run it -- project_layer is built for pe_dim - 3 inputs, which counts the view '
                                      'embedding, and receives the positional embedding alone (lib/dvqgo.py:82-86,327)')
        if kwargs.get('mode_type') in ('TRANS', 'adain', 'adain_vq'):
            raise NotImplementedError(f"mode_type={kwargs['mode_type']!r} needs modules the reference never defines (lib/dvqgo.py:111-118)")
        if k0_type != 'VQGrid':
            raise NotImplementedError(f'k0_type={k0_type!r}: DirectQVGO hands its feature grid a codebook size and an input width, which only VQGrid takes '
                                      '(lib/dvqgo.py:85-88)')
        super().__init__(xyz_min, xyz_max, num_voxels=num_voxels, mpi_depth=mpi_depth, mask_cache_path=mask_cache_path, mask_cache_thres=mask_cache_thres,
                         mask_cache_world_size=mask_cache_world_size, fast_color_thres=fast_color_thres, density_type=density_type, k0_type=k0_type,
                         density_config=density_config, k0_config=k0_config, rgbnet_dim=rgbnet_dim, rgbnet_depth=rgbnet_depth, rgbnet_width=rgbnet_width,
                         viewbase_pe=viewbase_pe, spatial_pe=spatial_pe, **kwargs)
        if isinstance(self.density, grid.DenseGrid):
            self.density.ordered_grad = True      # with the kernels of csrc/k4_vq.hip: the same state and inputs give the same gradients, bit for bit

    def _new_k0(self, kwargs):
        # lib/dvqgo.py:82-88: input_dim = pe_dim - 3 = 3 + 6 spatial_pe with viewbase_pe == 0; world_size is the number of codewords
        self.n_cluster = int(kwargs['n_cluster'])
        return grid.create_grid(self.k0_type, input_dim=3 + 6 * self.rgbnet_kwargs['spatial_pe'], channels=self.k0_dim, world_size=self.n_cluster,
                                xyz_min=self.xyz_min, xyz_max=self.xyz_max, config=self.k0_config)

    def get_kwargs(self):
        kw = super().get_kwargs()
        del kw['dim_rend']                    # not among upstream's keys (lib/dvqgo.py:156-174)
        kw['n_cluster'] = self.n_cluster      # ... and this one is missing there: upstream cannot rebuild the model from its own checkpoint
        return kw

    def _scale_k0(self):
        pass                                  # lib/dvqgo.py:183-184: the codebook has no resolution

    def k0_total_variation_add_grad(self, weight, dense_mode):
        raise NotImplementedError('k0_total_variation_add_grad: upstream calls VQGrid.total_variation_add_grad, which does not exist (lib/dvqgo.py:240-243); '
                                  'a codebook has no neighbouring voxels to smooth')

    def _k4_fusable_uncached(self):
        return self._k4_net_fusable(self.rgbnet) and isinstance(self.density, grid.DenseGrid)

    def _k4_one_launch_pays(self):
        """Measured (profiles/dvqgo_call_time.md): at width 32, 6 channels, 64 codewords the one launch renders a 1008x756 frame in 15.7 ms against 40.5 ms
        for the staged path in 8192-ray chunks; at width 128 / 12 channels / 300 codewords and at width 64 / 32 channels / 2500 codewords it is 9x and
        12x SLOWER (one wave per SIMD, a per-lane scan of the whole codebook).  Until a shape in between is measured only the winning one's class takes
        the one launch by itself; ``k4_fused=True`` in the render kwargs asks for it at any shape it covers (tests)."""
        width = [m for m in self.rgbnet.modules() if isinstance(m, torch.nn.Linear)][0].out_features
        return width == 32 and self.k0.dim <= 8 and self.k0.dim * self.k0.n_embed <= 512

    def k4_warm(self, stepsize=None):
        self.k0.prepared_codebook()           # the one load-time product of the one-launch path

    def _k0_features(self, ray_pts):
        """lib/dvqgo.py:322-327: the positional embedding of the shaded samples (k4_rgbnet_input_mpi without feature channels and view frequencies: the
        embedding's own arithmetic) through the codebook."""
        n = ray_pts.shape[0]
        nothing = ray_pts.new_empty([n, 0])
        ray0 = torch.zeros([n], dtype=torch.int64, device=ray_pts.device)
        pe = train_ops.RgbnetInputMPI.apply(nothing, ray_pts, self.xyz_min.new_zeros([1, 3]), ray0, self.xyz_min, self.xyz_max, self.posfreq, self.viewfreq)
        vq_emb, _, _ = self.k0(pe[:, :3 + 6 * len(self.posfreq)])
        return vq_emb

    def forward(self, rays_o, rays_d, viewdirs, global_step=None, **render_kwargs):
        '''Volume rendering (lib/dvqgo.py:279-408)
        @rays_o:   [N, 3] the starting point of the N shooting rays.
        @rays_d:   [N, 3] the shooting direction of the N rays.
        @viewdirs: [N, 3] viewing direction to compute positional embedding for MLP.
        '''
        rays_o, rays_d, viewdirs = self._k4_check_rays(rays_o, rays_d, viewdirs)
        if not self.k0.embed.is_cuda:
            raise N.K4Error('DirectQVGO.forward: the model must be on the GPU (no CPU path)')
        # training mode moves the codebook from per-sample sums: it takes the op sequence, as autograd and k4_staged=True do
        staged = render_kwargs.get('k4_staged', False) or torch.is_grad_enabled() or self.training or not self._k4_fusable()
        staged = staged or not (render_kwargs.get('k4_fused', False) or self._k4_one_launch_pays())
        staged = staged or int((self.mpi_depth - 1) / render_kwargs['stepsize']) + 1 < 2        # (one sample per ray: the sampler's 0 / 0 is the op sequence's)
        if staged:
            return self._forward_staged(rays_o, rays_d, viewdirs, global_step=global_step, **render_kwargs)
        self._k4_params_ready()
        return self._forward_vq_fused(rays_o, rays_d, viewdirs, **render_kwargs)

    def _forward_vq_fused(self, rays_o, rays_d, viewdirs, near, far, stepsize, bg, render_depth=False, **_ignored):
        """Inference in ONE launch (k4_march_vq_fwd): rgb_marched (= rgb_feature), alphainv_last and, on request, depth."""
        assert near == 0 and far == 1                                     # lib/dvqgo.py:262
        Nr, dev = rays_o.shape[0], rays_o.device
        rgb, depth, ainv, ret = self._k4_ray_outputs(Nr, dev, render_depth)
        N_samples = int((self.mpi_depth - 1) / stepsize) + 1              # lib/dvqgo.py:265
        mc, k0, dens, act = self.mask_cache, self.k0, self.density.grid, self.act_shift.grid
        keep = [rays_o, rays_d, viewdirs, dens.detach().contiguous(), act.detach().contiguous(), mc.mask.contiguous(), k0.prepared_codebook()]
        keep += [t.detach().float().contiguous() for t in (self.xyz_min, self.xyz_max, mc.xyz2ijk_scale, mc.xyz2ijk_shift, self.posfreq,
                                                           k0.project_layer[0].weight, k0.project_layer[0].bias, k0.project_layer[2].weight,
                                                           k0.project_layer[2].bias)]
        p = [t.data_ptr() or None for t in keep]
        d = N.VqDesc()
        ws, (d.dim0, d.width, d.n_hidden) = self._k4_rgbnet_into(self.rgbnet, d)
        keep += ws
        d.rays_o, d.rays_d, d.viewdirs, d.density, d.act_shift, d.mask, d.codebook = p[:7]
        d.xyz_min, d.xyz_max, d.xyz2ijk_scale, d.xyz2ijk_shift, d.posfreq, d.pw1, d.pb1, d.pw2, d.pb2 = p[7:16]
        d.n_rays, d.n_samples = Nr, N_samples
        d.dims = (N.C.c_int32 * 3)(*[int(v) for v in dens.shape[2:]])
        d.act_depth = int(act.numel())
        d.mask_dims = (N.C.c_int32 * 3)(*[int(v) for v in mc.mask.shape])
        d.interval, d.fast_color_thres, d.bg = float(stepsize * self.voxel_size_ratio), float(self.fast_color_thres), float(bg)
        d.n_pe, d.dim, d.n_embed = int(self.posfreq.numel()), k0.dim, k0.n_embed
        d.rgb, d.depth, d.alphainv_last = rgb.data_ptr() or None, depth.data_ptr() or None, ainv.data_ptr() or None
        if any(not t.is_cuda for t in keep):
            raise N.K4Error('DirectQVGO.forward: every tensor of the model must be on the GPU (no CPU path)')
        N.check(N.lib().k4_march_vq_fwd(N.C.byref(d), N.stream()), 'k4_march_vq_fwd')
        ret['n_max'] = N_samples
        return ret
