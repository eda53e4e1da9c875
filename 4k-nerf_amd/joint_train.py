"""Joint training step of the marcher and the VC-Decoder (BASELINE configs[4]; SURVEY.md 3.4, 8e "Training", 8f ranks 1-3).

Restates ONE iteration of the reference's joint loop (/root/reference/run_sr.py:801-1061, configuration
configs/llff/fern_lg_joint_l1.py) on this package's HIP training graph:

    patch of rays -> DirectMPIGO / DirectVoxGO forward (staged HIP ops under autograd, colour MLP on k4_rgbnet_*)
                  -> SFTNet(rgb_feature, depth)   (lib/sr_train.py: every convolution forward / dgrad / wgrad on MFMA kernels)
                  -> L1(LR) + L1(HR) + background entropy + distortion (k4_distortion_loss) + per-point rgb
                  -> backward -> [data parallel: gradient exchange] -> total-variation add-grad -> MaskedAdam x 2 -> lr decay

The adversarial term of the "+gan" recipes (run_sr.py:678-690, 916-957, 1016-1049) runs when a discriminator is handed in (``net_d``,
lib/sr_unetdisc.UNetDiscriminatorSN): its generator loss joins ``total``, and after the two optimizer steps the discriminator takes its own
step on the real patch and the detached decoder output.  The perceptual / style terms (weight_pcp, weight_style; run_sr.py:670-678, 934-945) run when
a loss module is handed in (``cri_perceptual``, lib/sr_loss.PerceptualLoss with the VGG19 weights loaded by the caller): they join ``total`` after the
high-resolution L1 term and in front of the adversarial one.  The network is frozen, so nothing of it is exchanged between data-parallel ranks.

Data parallelism (one 64x64 patch per rank, run_sr.py:829-835): the decoder's 15.8 MB of gradients, the rgbnet and every other
small tensor travel in ONE flat all-reduce (lib/sr_train.allreduce_gradients); the voxel grids do not -- `k0.grid` is 1.36 GB
dense while a patch touches well under 1 % of it -- they use ``sparse_grad_allreduce``: every rank compacts the voxels its
backward touched to (int32 index, values) lists, ONE all-gather of the padded lists moves them, and every rank adds all
lists into its dense gradient in RANK order, so the replicas hold bit-identical gradients (and MaskedAdam's "skip voxels
with zero gradient" sees the union of the touched voxels).  Pure torch.distributed plumbing: RCCL on the GPUs, gloo in the
CPU tests.  In the iterations without total variation (after tv_before) k0 has no dense gradient to begin with: the lookups'
backward stops after its scatter, and the same message is built from the scatter's scratch image -- k4_scatter_image_list
(the flagged voxels in ascending order, one byte read per voxel), k4_scatter_image_take (their sums into the message, the
image cleared) -- and after the same all-gather every rank's list is added back into the image in rank order
(k4_scatter_image_add), where MaskedAdam steps the union of the touched voxels in place (lib/grid.GridGrad.exchange;
``_SPARSE_IMAGE_EXCHANGE = False`` is the A/B switch).  The iterations with total variation exchange dense gradients as before.
"""
import torch
import torch.distributed as dist
import torch.nn.functional as F

from . import _native as N
from .lib import grid as G, sr_train, sr_unetdisc, train_ops, utils
from .lib.masked_adam import MaskedAdam

_ADAM_SIDE = True   # False: the k0 grid's optimizer step on the current stream (A/B, tests)
_TV_SEED = True     # False: dense total variation added after the backward pass, as run_sr.py orders it (A/B, tests)
_FUSED_LOSSES = True     # False: the elementwise loss terms as tensor-library ops (A/B, tests; CPU tensors always)
_SPLIT_GRID_STEP = True      # False: k0's optimizer step of an iteration with a dense TV term in one pass after the backward pass (A/B, tests)
_SPARSE_GRID_GRAD = True     # False: k0's gradient as a dense tensor in the iterations without TV too (A/B, tests)
_SPARSE_IMAGE_EXCHANGE = True    # False: ... whenever a gradient exchange runs (data parallelism), which then lists the touched voxels of the dense tensor (A/B, tests)

SPARSE_MIN_NUMEL = 1 << 20          # tensors at least this large are exchanged as (index, value) lists


def _world(group):
    return dist.get_world_size(group) if dist.is_available() and dist.is_initialized() else 1


def _exchange_runs(group):
    """Does a gradient exchange run this iteration?  In a job of several ranks -- and in the one-rank RCCL smoke test (_native.FORCE_COLLECTIVES).  THE predicate: the
    seeded routes that keep a grid's gradient out of a dense ``.grad`` (JointTrainer.step) are taken only when it says no (the 'sparse' route has an exchange of its
    own: _SPARSE_IMAGE_EXCHANGE), and every exchange runs only when it says yes."""
    return sr_train.collectives_run(_world(group))


def touched_voxels(g, cap=None):
    """Sorted int32 indices of the columns of g [C, V] with a non-zero entry.  On the GPU: one pass of k4_touched_voxels over the gradient
    (no [C, V] boolean temporary -- 340 MB next to the 1.36 GB k0 gradient -- and one host synchronisation, for the count)."""
    C, V = g.shape
    if not g.is_cuda:
        return (g != 0).any(0).nonzero().flatten().to(torch.int32)
    assert g.is_contiguous() and g.dtype == torch.float32
    cap = max(1024, V // 16) if cap is None else cap
    counter = torch.empty([1], dtype=torch.int64, device=g.device)
    while True:
        idx = torch.empty([cap], dtype=torch.int32, device=g.device)
        N.check(N.lib().k4_touched_voxels(N.f32(g), C, V, N.ptr(idx), cap, N.ptr(counter), N.stream()), 'k4_touched_voxels')
        n = int(counter)
        if n <= cap:
            return idx[:n].sort().values
        cap = n


def sparse_grad_allreduce(params, group=None, average=True):
    """Sum (average) the gradients of voxel-grid parameters [1, C, X, Y, Z] over the ranks by exchanging only touched voxels.
    A voxel is touched when any of its C channels has a non-zero gradient.  Returns a dict of exchange statistics."""
    world = _world(group)
    stats = {'world': world, 'bytes_gathered': 0, 'touched': []}
    params = [p for p in params if p.requires_grad]
    if not _exchange_runs(group):
        return stats
    for p in params:
        nbytes, touched = _list_exchange(p, group, world, average)
        stats['bytes_gathered'] += nbytes
        stats['touched'].append(touched)
    return stats


def _list_exchange(p, group, world, average=True):
    """One dense grid gradient through the (index, value) lists: -> (bytes gathered, (the ranks' counts, voxels))."""
    C = p.shape[1] if p.dim() == 5 else 1
    if p.grad is None:
        p.grad = torch.zeros_like(p)
    g = p.grad.view(C, -1)
    V = g.shape[1]
    assert V < 2 ** 31
    idx = touched_voxels(g)
    n = torch.tensor([idx.numel()], dtype=torch.int64, device=g.device)
    counts = [torch.zeros_like(n) for _ in range(world)]
    dist.all_gather(counts, n, group=group)
    counts = [int(c) for c in counts]
    cap = max(max(counts), 1)
    # one message per rank: [cap] int32 indices followed by the bits of the [C][cap] fp32 values (integer buffers: plain byte moves)
    send = torch.zeros([(C + 1) * cap], dtype=torch.int32, device=g.device)
    send[:idx.numel()] = idx
    send[cap:].view(torch.float32).view(C, cap)[:, :idx.numel()] = g[:, idx.long()]
    recv = torch.empty([world * (C + 1) * cap], dtype=torch.int32, device=g.device)
    dist.all_gather_into_tensor(recv, send, group=group)
    g[:, idx.long()] = 0                                     # own contribution comes back with the others, in rank order
    scale = 1.0 / world if average else 1.0
    for r in range(world):
        msg = recv[r * (C + 1) * cap:(r + 1) * (C + 1) * cap]
        ri = msg[:counts[r]].long()
        g.index_add_(1, ri, msg[cap:].view(torch.float32).view(C, cap)[:, :counts[r]] * scale)
    return recv.numel() * 4, (counts, V)


def _image_exchange_grids(model):
    """The grids whose gradient of this iteration travels from the scatter's scratch image: those JointTrainer.step armed 'sparse' -- a function of the
    configuration and global_step alone, hence the same on every rank (what a rank's backward did or did not leave behind must not decide which collectives
    it enters: they would stop matching and the job would hang)."""
    out = []
    for m in model.modules():
        route = m.__dict__.get('_k4_route')
        if route is not None and route.route == 'sparse':
            out.append(m)
    return out


def exchange_gradients(model, net_sr, group=None):
    """Data-parallel gradient exchange of the joint step: a grid armed 'sparse' from its scratch image (lib/grid.GridGrad.exchange: no dense gradient on either
    side of it), the other big grids as lists from their dense gradients, everything else in one dense bucket."""
    if not _exchange_runs(group):
        return {'world': 1}
    world = _world(group)
    image = {'image_bytes_gathered': 0, 'image_touched': []}
    taken = set()
    for owner in _image_exchange_grids(model):
        one = owner.grad_route.exchange(group)
        if one is None:
            # this rank's gradient is a dense tensor after all (no scratch image, a `.grad` from elsewhere): the same two collectives, the same
            # message, built from and merged into that tensor
            nbytes, touched = _list_exchange(owner.grid, group, world)
            one = {'bytes_gathered': nbytes, 'touched': touched}
        image['image_bytes_gathered'] += one['bytes_gathered']
        image['image_touched'].append(one['touched'])
        taken.add(id(owner.grid))
    # (a grid exchanged above is in neither list: sparse_grad_allreduce would give it a dense zero `.grad`)
    everything = [p for p in list(model.parameters()) + list(net_sr.parameters()) if p.requires_grad and id(p) not in taken]
    big = [p for p in everything if p.numel() >= SPARSE_MIN_NUMEL and p.dim() == 5]
    big_ids = {id(p) for p in big}
    small = [p for p in everything if id(p) not in big_ids]
    stats = sparse_grad_allreduce(big, group=group)
    stats.update(image)
    stats['bytes_dense'] = sr_train.allreduce_gradients(small, group=group)
    return stats


class JointCfg(dict):
    """Attribute-style view of the `fine_train` section (mmcv ConfigDict upstream)."""
    __getattr__ = dict.__getitem__

    @classmethod
    def fern_lg_joint_l1(cls, **over):
        """configs/llff/fern_lg_joint_l1.py on top of llff_default_lg.py and default.py (the values the joint loop reads)."""
        cfg = dict(N_iters=300000, N_rand=4096, N_patch=64, ray_sampler='patch_mimg',
                   lrate_density=1e-1, lrate_k0=1e-1, lrate_rgbnet=1e-3, lrate_srnet=2e-4, lrate_decay=300,
                   skip_zero_grad_fields=['density', 'k0'],
                   weight_main=1.0, weight_entropy_last=0.001, weight_nearclip=0, weight_distortion=0.01, weight_rgbper=0.01,
                   weight_pcp=0, weight_gan=0, weight_style=0,
                   tv_every=1, tv_after=0, tv_before=10000, tv_dense_before=10000, weight_tv_density=1e-5, weight_tv_k0=1e-6)
        cfg.update(over)
        return cls(cfg)

    @classmethod
    def fern_lg_joint_l1_gan(cls, **over):
        """configs/llff/fern_lg_joint_l1+gan.py: fern_lg_joint_l1 with weight_pcp=0.5, weight_gan=0.05, weight_style=0.2.  The preset carries the
        perceptual / style weights as the configuration file states them; JointTrainer needs ``cri_perceptual`` for them (the caller loads the VGG19
        weights: lib/sr_loss.PerceptualLoss), so a caller who wants the adversarial term alone passes ``weight_pcp=0, weight_style=0``."""
        cfg = dict(weight_pcp=0.5, weight_gan=0.05, weight_style=0.2)
        cfg.update(over)
        return cls.fern_lg_joint_l1(**cfg)

    @classmethod
    def chair_1x_joint_l1_gan(cls, **over):
        """configs/syn/1x_chair_joint_l1+gan.py on top of default.py (NOT syn_default.py: no TV terms, no distortion term, N_rand=8192): the synthetic
        recipe at sr_ratio 1, patches from the 'patch_inmask' sampler (lib/dvgo.get_training_rays_in_maskcache_sampling_sr).  As with
        ``fern_lg_joint_l1_gan`` the perceptual / style weights need ``cri_perceptual`` and the adversarial weight needs ``net_d``."""
        cfg = dict(N_iters=300000, N_rand=8192, N_patch=64, ray_sampler='patch_inmask',
                   lrate_density=1e-1, lrate_k0=1e-1, lrate_rgbnet=1e-3, lrate_srnet=2e-4, lrate_decay=300,
                   skip_zero_grad_fields=['density', 'k0'],
                   weight_main=1.0, weight_entropy_last=0.001, weight_nearclip=0, weight_distortion=0, weight_rgbper=0.01,
                   weight_pcp=0.5, weight_gan=0.05, weight_style=0.2,
                   tv_every=1, tv_after=0, tv_before=0, tv_dense_before=0, weight_tv_density=0.0, weight_tv_k0=0.0)
        cfg.update(over)
        return cls(cfg)


class JointTrainer:
    """Optimizers + one-iteration method of the joint loop.  ``render_kwargs`` as run_sr.py:690-702 builds them
    (``render_depth=True``; ``rand_bkgd`` for LLFF); ``n_train_images`` = len(rays_o_tr), the TV weights' divisor (:1008-1011)."""

    def __init__(self, model, net_sr, cfg_train, render_kwargs, n_train_images, sr_ratio=4, num_cond=1, dim_rend=3, group=None, near_clip=None, net_d=None,
                 cri_perceptual=None):
        weight_style = cfg_train.get('weight_style', 0)
        if (cfg_train.weight_pcp > 0 or weight_style > 0) and cri_perceptual is None:
            raise NotImplementedError('weight_pcp / weight_style > 0 need the loss module: JointTrainer(..., cri_perceptual=sr_loss.PerceptualLoss(layer_weights, '
                                      'perceptual_weight=weight_pcp, style_weight=weight_style)) with the VGG19 weights loaded by the caller '
                                      '(load_vgg_state_dict; run_sr.py:670-678)')
        if weight_style > 0 and not cfg_train.weight_pcp > 0:
            raise NotImplementedError('weight_style > 0 with weight_pcp == 0: run_sr.py:934 evaluates both terms under `weight_pcp > 0` only and would drop the '
                                      'style term silently; set weight_style=0 or weight_pcp > 0')
        if cfg_train.weight_pcp > 0 and (cri_perceptual.perceptual_weight != cfg_train.weight_pcp or cri_perceptual.style_weight != weight_style):
            raise ValueError(f'cri_perceptual carries perceptual_weight={cri_perceptual.perceptual_weight}, style_weight={cri_perceptual.style_weight}; the '
                             f'configuration states weight_pcp={cfg_train.weight_pcp}, weight_style={weight_style} (run_sr.py:678)')
        if cfg_train.weight_gan > 0 and net_d is None:
            raise NotImplementedError('weight_gan > 0 needs a discriminator: JointTrainer(..., net_d=sr_unetdisc.UNetDiscriminatorSN(3, 64)) (run_sr.py:679-690)')
        if num_cond != 1 or dim_rend != 3:
            raise NotImplementedError('joint step: num_cond=1 (depth condition), dim_rend=3 as configs/llff/fern_lg_joint_l1.py')
        self.model, self.net_sr, self.cfg, self.group = model, net_sr, cfg_train, group
        self.render_kwargs = dict(render_kwargs)
        self.n_train_images, self.sr_ratio = n_train_images, sr_ratio
        self.near_clip = near_clip                  # data_dict['near_clip'] (run_sr.py:971): the weight_nearclip term's distance, world units
        self.optimizer = utils.create_optimizer_or_freeze_model(model, cfg_train, global_step=0)                  # run_sr.py:640
        self._side_stream_updates()
        self.optimizer_sr = MaskedAdam([{'params': net_sr.parameters(), 'lr': cfg_train.lrate_srnet, 'kname': 'srnet',
                                         'skip_zero_grad': False}])                                               # run_sr.py:665-667
        self.last_exchange = None
        self._after_march = None
        # the adversarial term (run_sr.py:679-690); with weight_gan == 0 a discriminator handed in is ignored: the step is the one without it
        self.net_d = net_d if cfg_train.weight_gan > 0 else None
        # the perceptual / style terms (run_sr.py:670-678); with weight_pcp == 0 a module handed in is ignored
        self.cri_perceptual = cri_perceptual if cfg_train.weight_pcp > 0 else None
        self.optimizer_d = self.cri_gan = None
        if self.net_d is not None:
            self.cri_gan = sr_unetdisc.GANLoss(gan_type='vanilla', loss_weight=cfg_train.weight_gan)
            self.optimizer_d = MaskedAdam([{'params': net_d.parameters(), 'lr': cfg_train.lrate_srnet, 'kname': 'd', 'skip_zero_grad': False}])

    def rebuild_optimizer(self, global_step=0):
        """Re-create the marcher's optimizer after ``model.scale_volume_grid`` replaced the grid parameters (run_sr.py:812-818 does the
        same after every progressive-growing step): the old MaskedAdam would keep stepping the dead tensors."""
        self.optimizer = utils.create_optimizer_or_freeze_model(self.model, self.cfg, global_step=global_step)
        self._side_stream_updates()
        return self.optimizer

    def _dense_tv_ahead(self, global_step):
        """Write the dense TV term ahead of the backward pass?  Only while TV is dense, and only in a single-process job: under data parallelism (a group of
        its own OR the default process group -- ``self.group`` is None for both that and no job at all) the exchange between backward and TV sends the
        touched voxels, which a dense seed would make all of them (3.6 GB per rank instead of a few MB)."""
        return _TV_SEED and not _exchange_runs(self.group) and global_step < self.cfg.tv_dense_before

    def _sparse_grid_owners(self):
        """The grids whose gradient may stay in the scatter's scratch image this iteration: multi-channel DenseGrids stepped by MaskedAdam on the side stream
        (the optimizer looks for pending sums there) in a param group that skips zero gradients, without a per-voxel learning rate."""
        opt = self.optimizer
        if not isinstance(opt, MaskedAdam):
            return []
        out = []
        for owner in opt._side:
            g = owner.grid
            if g.is_cuda and g.dim() == 5 and g.shape[1] > 1 and g.requires_grad and not (opt.per_lr is not None and opt.per_lr.shape == g.shape) \
                    and any(pg.get('skip_zero_grad') and any(p is g for p in pg['params']) for pg in opt.param_groups):
                out.append(owner)
        return out

    def _side_stream_updates(self):
        """The feature grid's optimizer step (1.9 ms of HBM time on the LLFF scene) on a second stream: the next iteration's sample selection
        reads the density grid only and no longer queues behind it; DenseGrid makes every reader of k0 wait (lib/grid.DenseGrid.params_ready)."""
        k0 = getattr(self.model, 'k0', None)
        if _ADAM_SIDE and isinstance(self.optimizer, MaskedAdam) and hasattr(k0, 'note_pending_update') and k0.grid.is_cuda:
            self.optimizer.update_on_side_stream(k0.grid, k0)

    def losses(self, rr, rgb_sr, target, target_4x, pr, pc, n_rays):
        """run_sr.py:877-995: the scalar terms of one iteration (dict of tensors; 'total' is what is back-propagated)."""
        cfg, s = self.cfg, self.sr_ratio
        if _FUSED_LOSSES and rgb_sr.is_cuda and rgb_sr.dtype == torch.float32 and rr['rgb_feature'].dtype == torch.float32 and cfg.weight_nearclip <= 0 \
                and tuple(rgb_sr.shape) == (1, 3, s * pr, s * pc):
            # the elementwise terms as ONE autograd node (two launches forward, one backward: lib/train_ops.JointSmallLosses) instead of ~40 tensor-library launches
            ent, per = cfg.weight_entropy_last > 0, cfg.weight_rgbper > 0
            small, terms = train_ops.joint_small_losses(rr['rgb_feature'], rgb_sr, rr['alphainv_last'] if ent else None, rr['raw_rgb'] if per else None,
                                                        target, target_4x.detach().reshape(-1, 3), rr['weights'] if per else None, rr['ray_id'] if per else None,
                                                        cfg.weight_main, cfg.weight_entropy_last if ent else 0.0, cfg.weight_rgbper if per else 0.0)
            out = {'photo': terms[0], 'l1': terms[1], 'psnr_sr': terms[2]}
            if ent:
                out['entropy_last'] = terms[3]
            if cfg.weight_distortion > 0:
                out['distortion'] = cfg.weight_distortion * train_ops.flatten_eff_distloss(rr['weights'], rr['s'], 1 / rr['n_max'], rr['ray_id'],
                                                                                            n_rays=rr['alphainv_last'].shape[0])
            if per:
                out['rgbper'] = terms[4]
            out['total'] = small + out['distortion'] if cfg.weight_distortion > 0 else small
            return out
        out = {'photo': cfg.weight_main * F.l1_loss(rr['rgb_feature'], target)}
        rgb_hr = target_4x.detach().reshape(s * pr, s * pc, 3).movedim(-1, 0).unsqueeze(0)
        out['l1'] = F.l1_loss(rgb_sr, rgb_hr)
        out['psnr_sr'] = -10.0 * torch.log10((rgb_sr.detach().clamp(0, 1) - rgb_hr).pow(2).mean())
        if cfg.weight_entropy_last > 0:
            p = rr['alphainv_last'].clamp(1e-6, 1 - 1e-6)
            out['entropy_last'] = -(p * torch.log(p) + (1 - p) * torch.log(1 - p)).mean() * cfg.weight_entropy_last
        if cfg.weight_nearclip > 0:
            # run_sr.py:970-976: push down the density of the samples closer than near_clip (t in units of the scene radius)
            if 't' not in rr or 'raw_density' not in rr:
                raise ValueError(f"weight_nearclip > 0 needs the 't' / 'raw_density' keys of the forward dict, which {type(self.model).__name__} "
                                 "does not return (DirectContractedVoxGO does)")
            if self.near_clip is None:
                raise ValueError("weight_nearclip > 0 needs JointTrainer(near_clip=data_dict['near_clip'])")
            near_thres = self.near_clip / self.model.scene_radius[0].item()
            density = rr['raw_density'][rr['t'] < near_thres]
            if len(density):
                out['nearclip'] = cfg.weight_nearclip * (density - density.detach()).sum()
        if cfg.weight_distortion > 0:
            out['distortion'] = cfg.weight_distortion * train_ops.flatten_eff_distloss(rr['weights'], rr['s'], 1 / rr['n_max'], rr['ray_id'],
                                                                                        n_rays=rr['alphainv_last'].shape[0])
        if cfg.weight_rgbper > 0:
            per = (rr['raw_rgb'] - target[rr['ray_id']]).pow(2).sum(-1)
            out['rgbper'] = cfg.weight_rgbper * (per * rr['weights'].detach()).sum() / n_rays
        out['total'] = sum(v for k, v in out.items() if k != 'psnr_sr')
        return out

    def forward(self, rays_o, rays_d, viewdirs, target, target_4x, pr, pc, global_step):
        rr = self.model(rays_o, rays_d, viewdirs, global_step=global_step, is_train=True, **self.render_kwargs)
        if self._after_march is not None:                        # (step: the first part of a split grid step, as early as the lookups' points are known)
            self._after_march()
        rgb_cache = rr['rgb_feature'].reshape(1, pr, pc, -1).movedim(-1, 1)
        cond = rr['depth'].reshape(1, pr, pc, 1).movedim(-1, 1)                          # num_cond == 1 (run_sr.py:894-897)
        rgb_sr = self._decoder(rgb_cache, cond)                                          # run_sr.py:918
        ls = self.losses(rr, rgb_sr, target, target_4x, pr, pc, len(rays_o))
        if self.cri_perceptual is not None:                      # run_sr.py:934-937: after the L1 terms, in front of the adversarial one
            s = self.sr_ratio
            rgb_hr = target_4x.detach().reshape(s * pr, s * pc, 3).movedim(-1, 0).unsqueeze(0)
            ls['pcp'], style = self.cri_perceptual(rgb_sr, rgb_hr)
            ls['total'] = ls['total'] + ls['pcp']
            if style is not None:
                ls['style'] = style
                ls['total'] = ls['total'] + style
        if self.net_d is not None:                               # generator phase (run_sr.py:920-922, 946-957): D frozen, one more summand of `total`
            for p in self.net_d.parameters():
                p.requires_grad = False
            ls['g'] = self.cri_gan(self.net_d(rgb_sr), True, is_disc=False)
            ls['total'] = ls['total'] + ls['g']
        return rr, rgb_sr, ls

    def _discriminator_step(self, rgb_sr, target_4x, pr, pc):
        """run_sr.py:1019-1049: the discriminator's own iteration on the real patch and the detached decoder output."""
        net_d, s = self.net_d, self.sr_ratio
        for p in net_d.parameters():
            p.requires_grad = True
        self.optimizer_d.zero_grad()
        rgb_hr = target_4x.detach().reshape(s * pr, s * pc, 3).movedim(-1, 0).unsqueeze(0).contiguous()
        with torch.enable_grad():
            d_real = self.cri_gan(net_d(rgb_hr), True, is_disc=True)
            d_real.backward()
            d_fake = self.cri_gan(net_d(rgb_sr.detach().clone()), False, is_disc=True)
            d_fake.backward()
        if _exchange_runs(self.group):
            sr_train.allreduce_gradients(list(net_d.parameters()), group=self.group)
        self.optimizer_d.step()
        return {'d_real': d_real.detach(), 'd_fake': d_fake.detach()}

    def _decoder(self, x, cond):                                # (a method of its own: tools/joint_phase_events.py marks the phase around it)
        return self.net_sr(x, cond)

    def step(self, rays_o, rays_d, viewdirs, target, target_4x, pr, pc, global_step):
        """One iteration (run_sr.py:869-1014,1052-1061).  Returns the dict of loss tensors (detached)."""
        cfg = self.cfg
        tv_now = cfg.tv_after < global_step < cfg.tv_before and global_step % cfg.tv_every == 0                 # run_sr.py:1005-1011
        # Where each grid's gradient goes this iteration (lib/grid.GridGrad; a grid that is not armed takes the reference's form: a dense `.grad` from zeros).
        # 'dense' + seed: DENSE total variation does not look at the gradient, so its term is written ahead of the backward pass (side stream) into the buffer the
        #   lookups' backward accumulates into -- the same sum with a third of the memory traffic, and none of it at the end of the iteration where the next iteration's
        #   sample selection waits.
        # 'split' + seed: ... and a grid MaskedAdam can step from the scratch image is stepped in two exact parts: every voxel the scatter cannot touch right after the
        #   marcher's forward pass (beside the decoder's passes), the touched ones after the backward pass -- the dense pass over k0 (1.8 ms) no longer sits between
        #   this iteration's backward pass and the next iteration's lookup.
        # 'sparse': without TV (after tv_before: 290,000 of fern_lg_joint_l1's 300,000 iterations) the lookups' backward is the only contribution to k0's gradient and
        #   MaskedAdam skips voxels without one: the backward stops after its scatter and the optimizer updates the touched voxels from there -- no dense 1.36 GB gradient.
        # The two seeded routes only when no gradient exchange runs: it reads the dense gradient and sends the TOUCHED voxels, which a dense seed would make all of them.
        # 'sparse' under an exchange too (_SPARSE_IMAGE_EXCHANGE): the scratch image already is the exchange's message -- a flag byte per touched voxel, its sums as C
        #   consecutive floats -- so exchange_gradients sends the lists from there and merges the ranks' lists back into it in rank order (GridGrad.exchange), and
        #   the in-place step runs over the union.  The arming depends on the configuration and global_step only: every rank takes the same collectives.
        seed_tv = tv_now and self._dense_tv_ahead(global_step)
        armed, seeded = [], []

        def arm(grid, route):
            armed.append(grid)
            grid.grad_route.arm(route)
        try:
            if seed_tv:
                owners = self._sparse_grid_owners() if _SPLIT_GRID_STEP else []
                for weight, grid, fn in ((cfg.weight_tv_density, getattr(self.model, 'density', None), self.model.density_total_variation_add_grad),
                                         (cfg.weight_tv_k0, getattr(self.model, 'k0', None), self.model.k0_total_variation_add_grad)):
                    if weight > 0 and hasattr(grid, 'grad_route') and grid.grid.requires_grad:
                        arm(grid, 'split' if grid in owners else 'dense')
                        fn(weight / self.n_train_images, 'seed')
                        seeded.append(grid)
            elif _SPARSE_GRID_GRAD and not tv_now and (not _exchange_runs(self.group) or _SPARSE_IMAGE_EXCHANGE):
                for grid in self._sparse_grid_owners():
                    arm(grid, 'sparse')
            split = [g for g in seeded if g in owners] if seed_tv else []
            with torch.enable_grad():
                if split:
                    # (zero_grad makes the current stream wait for a grid's pending update: in front of the first part, not behind it; its place relative to the
                    # forward pass changes nothing -- run_sr.py:961-962 clears the gradients between the loss terms and the backward pass (:1003))
                    self.optimizer.zero_grad(set_to_none=True)
                    self.optimizer_sr.zero_grad(set_to_none=True)
                    # between the marcher's forward pass and the decoder's the lookups' points are known: the first part of the split step
                    self._after_march = lambda: [g.grad_route.first_part(self.optimizer) for g in split]
                rr, rgb_sr, ls = self.forward(rays_o, rays_d, viewdirs, target, target_4x, pr, pc, global_step)
                self._after_march = None
                if hasattr(self.model, '_k4_params_ready'):
                    self.model._k4_params_ready()                # (a forward that never read k0: its pending update still precedes what follows)
                if not split:
                    self.optimizer.zero_grad(set_to_none=True)
                    self.optimizer_sr.zero_grad(set_to_none=True)
                ls['total'].backward()
            for grid in armed:
                grid.grad_route.close()
            self.last_exchange = exchange_gradients(self.model, self.net_sr, self.group)
            if tv_now:
                if cfg.weight_tv_density > 0 and getattr(self.model, 'density', None) not in seeded:
                    self.model.density_total_variation_add_grad(cfg.weight_tv_density / self.n_train_images, global_step < cfg.tv_dense_before)
                if cfg.weight_tv_k0 > 0 and getattr(self.model, 'k0', None) not in seeded:
                    self.model.k0_total_variation_add_grad(cfg.weight_tv_k0 / self.n_train_images, global_step < cfg.tv_dense_before)
            self.optimizer.step()
        finally:
            # The one clean-up.  After a finished iteration this only disarms.  After one that raised (e.g. an out-of-memory batch the caller skips) nothing of it
            # reaches a later one: parked seeds and pending sums are dropped, a split step whose first part ran is completed from the seed (GridGrad.abort)
            self._after_march = None
            for grid in armed:
                grid.grad_route.abort()
        self.optimizer_sr.step()
        if self.net_d is not None:
            ls.update(self._discriminator_step(rgb_sr, target_4x, pr, pc))
        factor = 0.1 ** (1 / (cfg.lrate_decay * 1000))                                                           # run_sr.py:1052-1061
        for opt in (self.optimizer, self.optimizer_sr) + ((self.optimizer_d,) if self.optimizer_d is not None else ()):
            for pg in opt.param_groups:
                pg['lr'] = pg['lr'] * factor
        return {k: v.detach() for k, v in ls.items()}
