"""Voxel grids with the reference's interface (/root/reference/lib/grid.py).

``DenseGrid`` (lib/grid.py:108-151) and ``MaskGrid`` (lib/grid.py:274-307) keep constructor
arguments, parameter / buffer names (``grid``, ``xyz_min``, ``xyz_max``, ``mask``, ``xyz2ijk_scale``,
``xyz2ijk_shift``) and forward semantics; the lookups run on the gfx950 kernels of lib4k_hip.so.
``TensoRFGrid`` (lib/grid.py:157-268): the vector-matrix factored grid, its lookup / backward / dense expansion / total variation on the
kernels of csrc/k4_tensorf.hip.  ``VQGrid`` (lib/grid.py:38-103): a codebook of feature vectors behind a two-layer projection of the embedded position, the
nearest codeword found and the codebook's moving average updated on the kernels of csrc/k4_vq.hip.
"""

import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _native as N
from . import render_utils_cuda


def _grid_sample_fwd(grid, pts, xyz_min, xyz_max):
    C_ = grid.shape[1]
    out = torch.empty([pts.shape[0], C_], dtype=torch.float32, device=pts.device)
    N.check(N.lib().k4_grid_sample_3d(N.f32(grid), C_, grid.shape[2], grid.shape[3], grid.shape[4],
                                      N.f32(pts), N.f32(xyz_min), N.f32(xyz_max),
                                      pts.shape[0], N.f32(out), N.stream()), 'grid_sample_3d')
    return out


class GridSample3D(torch.autograd.Function):
    """DenseGrid lookup with a HIP backward: d/d(grid) by fp32 atomic scatter-add (what grid_sampler_3d_backward does for
    lib/grid.py:124 in the reference's training step).  No gradient w.r.t. the sample points (they come from rays)."""

    @staticmethod
    def forward(ctx, grid, pts, xyz_min, xyz_max, owner=None):
        ctx.save_for_backward(pts, xyz_min, xyz_max)
        ctx.grid_shape = tuple(grid.shape)
        ctx.owner = owner                                  # the DenseGrid: its gradient route (GridGrad) says where this backward leaves the gradient
        return _grid_sample_fwd(grid.detach().contiguous(), pts, xyz_min, xyz_max)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        pts, xyz_min, xyz_max = ctx.saved_tensors
        go = grad_out.float().contiguous()
        if ctx.owner is not None:
            return ctx.owner.grad_route.backward(go, ctx.grid_shape, pts, xyz_min, xyz_max), None, None, None, None
        gg = torch.zeros(ctx.grid_shape, dtype=torch.float32, device=go.device)
        grid_sample_3d_backward(go, *ctx.grid_shape[1:], pts, xyz_min, xyz_max, gg)
        return gg, None, None, None, None


class _ScratchImage:
    """One device's workspace of k4_grid_sample_3d_backward_cl ([voxel][C] fp32 sums + a flag byte per voxel: as large as the gradient).  It is all-zero
    while `holder` is None.  From the first scatter that leaves sums in it until they are consumed (in-place optimizer step, sweep) or discarded, `holder`
    is the GridGrad they belong to, and ``_scratch_image`` hands the image to nobody else."""
    __slots__ = ('shape', 'ws', 'event', 'holder')

    def __init__(self, shape, ws):
        self.shape, self.ws, self.event, self.holder = shape, ws, None, None

    def run(self, launch, stream=None):
        """ONE buffer per device: `stream` (default: the current one) waits for the image's last use, `launch()` is issued, and its completion is the new
        last use (-> that event).  A launch that raises drops the image -- it may hold half-written sums; the next use allocates a cleared one."""
        st = stream if stream is not None else torch.cuda.current_stream(self.ws.device)
        if self.event is not None:
            st.wait_event(self.event)
        self.ws.record_stream(st)
        try:
            launch()
        except Exception:
            self.drop()
            raise
        self.event = torch.cuda.Event()
        self.event.record(st)
        return self.event

    def drop(self):
        self.holder = None
        if _GSB_WS.get(self.ws.device) is self:
            del _GSB_WS[self.ws.device]


_GSB_WS = {}          # device -> _ScratchImage; one grid shape per device


def release_grid_sample_workspace(device=None):
    """Free the cached scratch image(s) of the channel-last grid_sample_3d backward (as large as the gradient: 1.4 GB for the LLFF k0)."""
    for d in list(_GSB_WS) if device is None else [torch.device(device)]:
        _GSB_WS.pop(d, None)


GSB_CHANNEL_LAST = True


def _who(route):
    return 'a call without an owning grid' if route is None else f'DenseGrid({route.owner.extra_repr()}) at {id(route.owner):#x}'


def _scratch_image(device, C_, X, Y, Z, taker=None):
    """The device's scratch image for this grid shape, allocated (cleared) when missing or of another shape, or None (one channel, switched off, out of
    memory).  `taker`: the GridGrad that asks (None: an ownerless dense call).  While the image holds a grid's pending sums only that grid gets it:
    anybody else would sweep them into a gradient of its own (same shape) or free them (another shape)."""
    nbytes = int(N.lib().k4_grid_sample_3d_backward_workspace_bytes(C_, X, Y, Z)) if GSB_CHANNEL_LAST else -1
    if nbytes <= 0:
        return None
    img = _GSB_WS.get(device)
    if img is not None and img.holder is not None and img.holder is not taker:
        raise N.K4Error(f'grid_sample_3d backward for {_who(taker)}: the scratch image holds the pending gradient of {_who(img.holder)} '
                        '(step or sweep that grid first)')
    if img is None or img.shape != (C_, X, Y, Z):
        _GSB_WS.pop(device, None)
        try:
            img = _GSB_WS[device] = _ScratchImage((C_, X, Y, Z), torch.zeros([nbytes // 4], dtype=torch.int32, device=device))
        except torch.OutOfMemoryError:
            return None
    return img


def grid_sample_3d_backward(go, C_, X, Y, Z, pts, xyz_min, xyz_max, gg, taker=None):
    """gg [1|-, C, X, Y, Z] += d(trilinear lookup)/d(grid) for grad_out `go` [n, C] at `pts` [n, 3].  More than one channel: through the
    channel-last scratch image (k4_grid_sample_3d_backward_cl; the workspace, as large as the gradient, is allocated and cleared once
    per device and grid shape and kept -- GSB_CHANNEL_LAST = False (module attribute: bench A/B) or an allocation failure selects the channel-major atomic scatter).
    The image must be all-zero on entry (K4Error while it holds another grid's pending sums) and is left all-zero by the sweep."""
    L = N.lib()
    n = pts.shape[0]
    if taker is not None and getattr(taker.owner, 'ordered_grad', False) and C_ == 1:
        # a fixed summation order instead of the atomic scatter (DenseGrid.ordered_grad; lib/dvqgo.py): the samples' terms sorted by voxel, stably
        vox = torch.empty([n * 8 + 1], dtype=torch.int64, device=go.device)
        term = torch.empty([n * 8 + 1], dtype=torch.float32, device=go.device)
        N.check(L.k4_grid_sample_3d_backward_terms(N.f32(go), X, Y, Z, N.f32(pts), N.f32(xyz_min), N.f32(xyz_max), n, N.ptr(vox), N.f32(term), N.stream()),
                'k4_grid_sample_3d_backward_terms')
        key, order = torch.sort(vox[:n * 8], stable=True)
        N.check(L.k4_sorted_segment_add(N.ptr(key), N.f32(term[:n * 8].index_select(0, order)), n * 8, X * Y * Z, N.f32(gg), N.stream()), 'k4_sorted_segment_add')
        return
    img = _scratch_image(go.device, C_, X, Y, Z, taker) if n > 0 else None
    if img is not None:
        img.run(lambda: N.check(L.k4_grid_sample_3d_backward_cl(N.f32(go), C_, X, Y, Z, N.f32(pts), N.f32(xyz_min), N.f32(xyz_max), n, N.f32(gg), N.ptr(img.ws),
                                                                 N.stream()), 'grid_sample_3d_backward_cl'))
    else:
        N.check(L.k4_grid_sample_3d_backward(N.f32(go), C_, X, Y, Z, N.f32(pts), N.f32(xyz_min), N.f32(xyz_max), n, N.f32(gg), N.stream()),
                'grid_sample_3d_backward')


def total_variation_add_grad(param, grad, wx, wy, wz, dense_mode):
    """total_variation_cuda.total_variation_add_grad (lib/cuda/total_variation.cpp:16-20): grad += TV gradient of param,
    in place.  param, grad: [1, C, X, Y, Z] contiguous fp32 device tensors (CHECK_INPUT upstream)."""
    if param.dim() != 5 or grad.shape != param.shape:
        raise ValueError('total_variation_add_grad: param/grad must be [1,C,X,Y,Z] of equal shape')
    for t in (param, grad):
        if not t.is_cuda or not t.is_contiguous() or t.dtype != torch.float32:
            raise ValueError('total_variation_add_grad: tensors must be contiguous fp32 device tensors')
    N.check(N.lib().k4_total_variation_add_grad(N.ptr(param), N.ptr(grad), float(wx), float(wy), float(wz),
                                                param.size(2), param.size(3), param.size(4), param.numel(),
                                                2 if dense_mode == 'write' else 1 if dense_mode else 0, N.stream()),
            'k4_total_variation_add_grad')


def _tv_stream(device):
    """The stream the dense TV term is written on ahead of the backward pass: verified to run beside the current stream and the package's other side
    streams (_native.overlapping_stream)."""
    return N.overlapping_stream(device, 'dense total variation')


def _vec3(v):
    """float32 CPU copy of a bbox corner given as list / numpy / tensor on any device (the reference's torch.Tensor(v) needs its
    global CUDA default tensor type for device inputs)."""
    if torch.is_tensor(v):
        return v.detach().float().cpu().clone()
    return torch.Tensor(v)


class GridGrad:
    """Where one DenseGrid's gradient of the current training iteration is, and how it reaches the optimizer (``DenseGrid.grad_route``; the trainer arms it per
    iteration, lib/masked_adam.MaskedAdam consumes it; nobody else touches the fields).

        idle --arm('dense' | 'sparse' | 'split')--> armed            (a seed -- the dense TV term written ahead, park_seed -- may be parked in any state)
        armed 'split' --lookup under autograd--> corners flagged      (k4_grid_flag_corners: the voxels the backward will touch)
        armed 'split' --first_part(optimizer)--> early                (every unflagged voxel stepped from the seed; lookups under autograd now raise)
        backward:  'sparse' without a seed, or early: the scatter's sums stay in the device's scratch image, which this object then holds;
                   otherwise a dense gradient (zeros or the seed, + scatter + sweep) is returned to autograd
        close():   a seed no backward consumed becomes (or is added to) ``.grad``
        exchange(): data parallelism, route 'sparse': the image's sums are replaced by the ranks' averaged sums over the union of their voxels (in place)
        optimizer: image() + consumed() around its in-place step / sweep() into a dense ``.grad``
        abort():   from any state back to idle; nothing of this iteration reaches the next one
    """

    def __init__(self, owner):
        self.owner = owner
        self.route = None           # None: idle (a backward then takes the dense form)
        self.seed = None            # (buffer, event of its completion)
        self.early = None           # first part of a split step done: (optimizer, seed buffer, step count, (beta1, beta2, lr, eps))
        self.sums = False           # this iteration's scatter sums are in the scratch image
        self.flags = None           # split route: uint8 [X*Y*Z], all-zero between iterations and reused across them
        self.flagged = False        # ... a lookup of this iteration wrote into them

    idle = property(lambda self: self.route is None and self.seed is None and self.early is None and not self.sums)
    pending = property(lambda self: self.sums or self.early is not None)         # the optimizer has an in-place step (or a sweep) to do

    def arm(self, route):
        if self.route is not None:
            raise N.K4Error(f'GridGrad.arm({route!r}): still armed ({self.route!r}) -- the previous iteration was neither finished nor aborted')
        if route not in ('dense', 'sparse', 'split'):
            raise ValueError(f'GridGrad.arm: unknown route {route!r}')
        if route == 'split':
            g = self.owner.grid
            if self.flags is None or self.flags.numel() != g[0, 0].numel() or self.flags.device != g.device:
                self.flags = torch.zeros([g[0, 0].numel()], dtype=torch.uint8, device=g.device)
        self.route = route

    def lookup_flags(self):
        """DenseGrid.forward under autograd: the flags this lookup's corners go into, or None."""
        if self.route != 'split':
            return None
        if self.early is not None:
            raise N.K4Error('DenseGrid.forward: a lookup under autograd after the first part of the split optimizer step')
        self.flagged = True
        return self.flags

    def first_part(self, optimizer):
        """Between the marcher's forward pass and the decoder's: ``optimizer.early_step`` steps every voxel no lookup flagged; refused -> the one-pass step."""
        if self.route == 'split' and (self.seed is None or not optimizer.early_step(self.owner, *self.seed)):
            self.route, self.flags, self.flagged = 'dense', None, False

    def first_part_done(self, optimizer, seed, step, hyper):
        """(MaskedAdam.early_step) the seed is consumed; the second part runs even if no backward pass reaches the grid (its flagged voxels: seed alone)."""
        self.early, self.seed = (optimizer, seed, step, hyper), None

    def split_flags(self):
        """(MaskedAdam.early_step) the flags of a grid armed 'split' whose first part has not run, else None."""
        return self.flags if self.route == 'split' and self.early is None else None

    def split_part(self):
        """(MaskedAdam) after the first part of a split step: (flags, seed, step count, hyper-parameters) for the second, else None."""
        return (self.flags,) + self.early[1:] if self.early is not None else None

    # ---- the dense TV term BEFORE the backward pass (no reference counterpart; joint_train.JointTrainer.step) ----
    # The reference adds the term after backward (run_sr.py:1005-1011): zero-fill the gradient (4 B / voxel), scatter, then read grad + param
    # and write grad (12 B) -- on the 339 M-float LLFF k0 that is 1.1 ms at the END of the iteration, where the next iteration's sample
    # selection (a device-to-host read) waits for it.  Dense mode does not look at the gradient, so the term can be WRITTEN into a fresh
    # buffer first (8 B / voxel, on a side stream under the iteration's host-paced phases) and the lookup's backward accumulates into
    # that buffer instead of into zeros: grad = term + scatter, the same sum.
    def park_seed(self, wx, wy, wz):
        owner = self.owner
        cur = torch.cuda.current_stream(owner.grid.device)
        seed = torch.empty_like(owner.grid.data, memory_format=torch.contiguous_format)
        side = _tv_stream(owner.grid.device)
        side.wait_stream(cur)                              # the optimizer step that produced these parameter values (and the allocation point)
        owner.params_ready(side, clear=False)              # ... also when that step runs on a stream of its own (the current stream still has to wait)
        with torch.cuda.stream(side):
            total_variation_add_grad(owner.grid.data, seed, wx, wy, wz, 'write')
            ev = torch.cuda.Event()
            ev.record(side)
        self.seed = (seed, ev)

    def take_seed(self, shape, device):
        hit, self.seed = self.seed, None
        if hit is None:
            return None
        seed, ev = hit
        torch.cuda.current_stream(device).wait_event(ev)
        if tuple(seed.shape) != tuple(shape) or seed.device != device:        # the grid was replaced in between (scale_volume_grid)
            raise N.K4Error('total_variation_seed_grad: the grid changed shape between the seed and the backward pass')
        return seed

    def close(self):
        """After the backward pass: a seed no lookup consumed becomes (or is added to) the gradient."""
        if self.seed is not None:
            g = self.owner.grid
            seed = self.take_seed(g.shape, g.device)
            g.grad = seed if g.grad is None else g.grad.add_(seed)

    def backward(self, go, shape, pts, xyz_min, xyz_max):
        """GridSample3D.backward: -> the dense gradient, or None with the sums left in the scratch image for MaskedAdam (k4_masked_adam_upd_sparse_cl[_seeded])."""
        _, C_, X, Y, Z = shape
        if self.early is not None or (self.route == 'sparse' and self.seed is None):
            img = _scratch_image(go.device, C_, X, Y, Z, self)
            if img is not None:
                img.holder, n = self, pts.shape[0]
                if n > 0:
                    img.run(lambda: N.check(N.lib().k4_grid_sample_3d_backward_cl_scatter(N.f32(go), C_, X, Y, Z, N.f32(pts), N.f32(xyz_min), N.f32(xyz_max), n,
                                                                                           N.ptr(img.ws), N.stream()), 'grid_sample_3d_backward_cl_scatter'))
                self.sums = True
                return None
            if self.early is not None:
                raise N.K4Error('GridSample3D.backward: the scratch image of a grid whose step was split is gone')
        gg = self.take_seed(shape, go.device)
        if gg is None:
            gg = torch.zeros(shape, dtype=torch.float32, device=go.device)
        grid_sample_3d_backward(go, C_, X, Y, Z, pts, xyz_min, xyz_max, gg, self)
        return gg

    def image(self, cleared=False):
        """(MaskedAdam) the scratch image its in-place step reads: this iteration's sums, or -- `cleared`, or a split step no backward reached -- all zero."""
        g = self.owner.grid
        img = _GSB_WS.get(g.device)
        if self.sums and (img is None or img.holder is not self or img.shape != tuple(g.shape[1:])):
            self.sums = False
            img = None
        elif not self.sums:
            img = _scratch_image(g.device, *g.shape[1:], self)
        elif cleared:
            img.run(img.ws.zero_)
        if img is None:
            raise N.K4Error('the scratch image of the pending grid gradient is gone')
        return img

    def consumed(self):
        """(MaskedAdam) the in-place step was launched: image and flags are all-zero behind it."""
        img = _GSB_WS.get(self.owner.grid.device)
        if img is not None and img.holder is self:
            img.holder = None
        self.sums, self.early, self.flagged = False, None, False

    def sweep(self):
        """Move the sums a scatter-only backward left in the scratch image into ``.grad`` (created when missing): the dense gradient after all."""
        g = self.owner.grid
        img = self.image()
        if g.grad is None:
            g.grad = torch.zeros_like(g, memory_format=torch.contiguous_format)
        _, C_, X, Y, Z = g.shape
        img.run(lambda: N.check(N.lib().k4_grid_sample_3d_backward_cl_sweep(C_, X, Y, Z, N.ptr(img.ws), N.f32(g.grad), N.stream()), 'grid_sample_3d_backward_cl_sweep'))
        img.holder, self.sums = None, False

    def exchange(self, group=None, average=True):
        """Data-parallel exchange of a gradient that stayed in the scratch image (route 'sparse' under joint_train.exchange_gradients), on the current stream:
        the flagged voxels are listed in ascending order (k4_scatter_image_list; the host reads their number -- the one synchronisation the dense form has too),
        the ranks' counts are all-gathered, the list's sums are taken out of the image into the message of joint_train.sparse_grad_allreduce ([cap] int32 indices |
        bits of the [C][cap] fp32 values; k4_scatter_image_take leaves the image all-zero), ONE all_gather_into_tensor moves the padded messages, and every rank's
        list is added back in rank order (k4_scatter_image_add, scale 1 / world): the image then holds bit-identical averaged sums on every replica, its flags mark
        the union of the ranks' voxels, and MaskedAdam._sparse_step runs as in a single-process job -- `.grad` stays None.  A rank whose backward never reached the
        grid sends an empty list and receives like the others.  -> statistics, or None when this rank's gradient is a dense tensor after all (no scratch image,
        a `.grad` from elsewhere: pending sums are swept into it): the caller then runs the SAME two collectives with the message built from that tensor."""
        import torch.distributed as dist
        g = self.owner.grid
        _, C_, X, Y, Z = g.shape
        if g.grad is not None:
            if self.sums:
                self.sweep()
            return None
        if self.sums:
            img = self.image()
        else:
            img = _scratch_image(g.device, C_, X, Y, Z, self)
            if img is None:
                return None
        L, dev, V = N.lib(), g.device, X * Y * Z
        world = dist.get_world_size(group)
        n = 0
        if self.sums:
            counter = torch.empty([1], dtype=torch.int64, device=dev)
            room = max(1024, V // 16)
            while True:
                idx = torch.empty([room], dtype=torch.int32, device=dev)
                img.run(lambda: N.check(L.k4_scatter_image_list(N.ptr(img.ws), C_, X, Y, Z, N.ptr(idx), room, N.ptr(counter), N.stream()), 'k4_scatter_image_list'))
                n = int(counter)
                if n <= room:
                    break
                room = n
        mine = torch.tensor([n], dtype=torch.int64, device=dev)
        counts = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(counts, mine, group=group)
        counts = [int(c) for c in counts]
        cap = max(max(counts), 1)
        words = (C_ + 1) * cap
        send = torch.zeros([words], dtype=torch.int32, device=dev)
        if n > 0:
            send[:n] = idx[:n]
            img.run(lambda: N.check(L.k4_scatter_image_take(N.ptr(img.ws), C_, X, Y, Z, N.ptr(send), n, cap, N.ptr(send[cap:]), N.stream()), 'k4_scatter_image_take'))
        recv = torch.empty([world * words], dtype=torch.int32, device=dev)
        dist.all_gather_into_tensor(recv, send, group=group)
        scale = 1.0 / world if average else 1.0

        def add():
            for r in range(world):
                msg = recv[r * words:(r + 1) * words]
                N.check(L.k4_scatter_image_add(N.ptr(img.ws), C_, X, Y, Z, N.ptr(msg), N.ptr(msg[cap:]), counts[r], cap, scale, N.stream()), 'k4_scatter_image_add')
        img.holder = self
        img.run(add)
        self.sums = True
        return {'bytes_gathered': recv.numel() * 4, 'touched': (counts, V)}

    def abort(self):
        """Back to idle.  After a finished iteration that only disarms.  After one the caller gave up on: the seed is forgotten (it holds a TV term of parameters a later
        iteration no longer has), pending sums are dropped with their image, written flags with their buffer -- and a split step whose first part ran is COMPLETED from
        the seed alone (its flagged voxels against a cleared image, the step count advanced): every voxel stepped once, a TV-only iteration for this grid."""
        try:
            if self.early is not None:
                self.early[0].finish_split_step(self.owner, seed_only=True)
        finally:
            if self.sums:
                img = _GSB_WS.get(self.owner.grid.device)
                if img is not None and img.holder is self:
                    img.drop()
            if self.flagged:
                self.flags = None
            self.route = self.seed = self.early = None
            self.sums = self.flagged = False


def create_grid(type, **kwargs):
    if type == 'DenseGrid':
        return DenseGrid(**kwargs)
    if type == 'TensoRFGrid':
        return TensoRFGrid(**kwargs)
    if type == 'VQGrid':
        if 'input_dim' not in kwargs:
            # a model that looks its grids up at positions (density_type / k0_type of DirectVoxGO, DirectMPIGO, ...) asking for a codebook: upstream
            # fails there too, on the missing constructor argument
            raise NotImplementedError('VQGrid takes an embedded input of input_dim values and a codebook size as world_size (lib/grid.py:39): it is '
                                      "DirectQVGO's k0 (lib/dvqgo.py:85-88), not a voxel grid of the other models")
        return VQGrid(**kwargs)
    raise NotImplementedError(f'{type}: DenseGrid, TensoRFGrid and VQGrid are provided (lib/grid.py:27-35)')


class DenseGrid(nn.Module):
    def __init__(self, channels, world_size, xyz_min, xyz_max, **kwargs):
        super().__init__()
        self.channels, self.world_size = channels, world_size
        for name, val in (('xyz_min', xyz_min), ('xyz_max', xyz_max)):
            self.register_buffer(name, _vec3(val))
        self.grid = nn.Parameter(torch.zeros([1, channels, *[int(v) for v in world_size]]))          # [1, C, X, Y, Z], Z fastest

    def forward(self, xyz):
        """Trilinear lookup == F.grid_sample(bilinear, align_corners=True, zero pad) of lib/grid.py:117-128: HIP kernel
        k4_grid_sample_3d; under autograd its backward is k4_grid_sample_3d_backward (gradient w.r.t. the grid)."""
        shape = xyz.shape[:-1]
        pts = xyz.reshape(-1, 3).contiguous()
        self.params_ready()
        if torch.is_grad_enabled() and self.grid.requires_grad:
            flags = self.grad_route.lookup_flags() if pts.shape[0] > 0 else None
            if flags is not None:                              # (a split optimizer step, JointTrainer.step: the voxels this lookup's backward will touch)
                _, _, X, Y, Z = self.grid.shape
                N.check(N.lib().k4_grid_flag_corners(X, Y, Z, N.f32(pts), N.f32(self.xyz_min), N.f32(self.xyz_max), pts.shape[0], N.ptr(flags), N.stream()),
                        'k4_grid_flag_corners')
            out = GridSample3D.apply(self.grid, pts.detach(), self.xyz_min, self.xyz_max, self)
        else:
            out = _grid_sample_fwd(self.grid.detach(), pts, self.xyz_min, self.xyz_max)
        out = out.reshape(*shape, self.channels)
        if self.channels == 1:
            out = out.squeeze(-1)
        return out

    def scale_volume_grid(self, new_world_size):
        """Trilinear resample to a new resolution (progressive growing, lib/grid.py:130-135): F.interpolate(trilinear,
        align_corners=True) on the HIP kernel k4_resample_trilinear.  The new tensor replaces the parameter, as upstream."""
        size = tuple(int(v) for v in new_world_size)
        self.params_ready()
        old = self.grid.data
        if self.channels == 0:
            data = torch.zeros([1, 0, *size], device=old.device)
        else:
            if not old.is_cuda:
                # deliberately no F.interpolate fallback: nothing in this package computes on the CPU (move the model to the GPU first)
                raise N.K4Error('scale_volume_grid: the grid must be on the GPU -- call model.to(device) before growing it (no CPU path)')
            src = old.float().contiguous()
            data = torch.empty([1, self.channels, *size], dtype=torch.float32, device=old.device)
            N.check(N.lib().k4_resample_trilinear(N.f32(src), self.channels, src.shape[2], src.shape[3], src.shape[4],
                                                  N.f32(data), size[0], size[1], size[2], N.stream()), 'k4_resample_trilinear')
        # a NEW parameter, as upstream: optimizers holding the old tensor must be re-created (run_sr.py:818; JointTrainer.rebuild_optimizer)
        self.grid = nn.Parameter(data)
        self.world_size = new_world_size

    def total_variation_add_grad(self, wx, wy, wz, dense_mode):
        '''Add gradients by total variation loss in-place (lib/grid.py:137-140).  dense_mode == 'seed' (no reference counterpart): the
        dense term ahead of the backward pass, see total_variation_seed_grad.'''
        if isinstance(dense_mode, str) and dense_mode == 'seed':
            return self.total_variation_seed_grad(wx, wy, wz)
        self.params_ready()
        total_variation_add_grad(self.grid, self.grid.grad, wx, wy, wz, dense_mode)

    @property
    def grad_route(self):
        """The grid's GridGrad: where this iteration's gradient is and how it reaches the optimizer.  Created on first use; neither copied nor saved."""
        r = self.__dict__.get('_k4_route')
        if r is None:
            r = self.__dict__['_k4_route'] = GridGrad(self)
        return r

    # ---- an optimizer step of the grid running on a second stream (lib/masked_adam.MaskedAdam.update_on_side_stream) ----
    _k4_pending = None

    def note_pending_update(self, event):
        self._k4_pending = event
        self._k4_pending_seen = set()                     # streams that already wait for it

    def params_ready(self, stream=None, clear=True):
        """Everything queued on `stream` (default: the current one) after this call sees the finished parameter update.  Called by every
        reader of the parameter in this package (lookups, total variation, resampling, the fused marchers' descriptors, state_dict)."""
        ev = self._k4_pending
        if ev is not None:
            # the event stays until the NEXT update replaces it: a reader on another stream later on must wait too (a cleared event made only
            # the first waiting stream safe); a stream waits once
            st = stream if stream is not None else torch.cuda.current_stream(self.grid.device)
            seen = self.__dict__.setdefault('_k4_pending_seen', set())
            if st.cuda_stream not in seen:
                st.wait_event(ev)
                seen.add(st.cuda_stream)

    def _save_to_state_dict(self, destination, prefix, keep_vars):
        self.params_ready()
        return super()._save_to_state_dict(destination, prefix, keep_vars)

    def _apply(self, fn, *args, **kwargs):                 # .to() / .cpu() / .cuda() / .float(): copies of the parameter on the current stream
        self.params_ready()
        return super()._apply(fn, *args, **kwargs)

    def __deepcopy__(self, memo):                          # copy.deepcopy(model) clones the parameter on the current stream
        self.params_ready()
        cls = self.__class__
        new = cls.__new__(cls)
        memo[id(self)] = new
        import copy
        for k, v in self.__dict__.items():
            if k in ('_k4_route', '_k4_pending', '_k4_pending_seen'):
                continue
            new.__dict__[k] = copy.deepcopy(v, memo)
        return new

    def total_variation_seed_grad(self, wx, wy, wz):
        """Start computing the dense TV term of the CURRENT parameter values into a new buffer (side stream).  The next backward pass
        through this grid accumulates into it; ``finish_grad_seed`` after the backward pass covers a pass that never reached the grid."""
        self.grad_route.park_seed(wx, wy, wz)

    def _take_grad_seed(self, shape, device):
        return self.grad_route.take_seed(shape, device)

    def finish_grad_seed(self):
        """After the backward pass: a seed no lookup consumed becomes (or is added to) the gradient."""
        self.grad_route.close()

    # True: the one-channel gradient of a lookup is summed in a fixed order (sorted terms, no atomics) so that a training step repeats bit for bit;
    # slower than the atomic scatter.  Set by models that promise it (lib/dvqgo.py); other channel counts and the optimizer's sparse routes are as ever.
    ordered_grad = False

    def get_dense_grid(self):
        self.params_ready()
        return self.grid

    @torch.no_grad()
    def __isub__(self, val):
        self.grid.data -= val
        torch.autograd.graph.increment_version(self.grid)      # `.data` edits bypass the version counter the repack caches key on
        return self

    def extra_repr(self):
        ws = self.world_size.tolist() if torch.is_tensor(self.world_size) else list(self.world_size)
        return f'channels={self.channels}, world_size={ws}'



_TENSORF_FACTORS = ('xy_plane', 'xz_plane', 'yz_plane', 'x_vec', 'y_vec', 'z_vec')


def _tensorf_args(factors, f_vec, channels, world):
    """The factor pointers and sizes every k4_tensorf_* entry point takes (include/k4nerf.h), from contiguous fp32 device tensors in checkpoint layout."""
    xy, xz, yz = factors[:3]
    X, Y, Z = world
    shapes = ((1, xy.shape[1], X, Y), (1, xz.shape[1], X, Z), (1, xz.shape[1], Y, Z), (1, xz.shape[1], X, 1), (1, xz.shape[1], Y, 1), (1, xy.shape[1], Z, 1))
    for name, t, want in zip(_TENSORF_FACTORS, factors, shapes):
        if tuple(t.shape) != want:
            raise N.K4Error(f'TensoRFGrid: {name} is {tuple(t.shape)}, expected {want}')
    if channels > 1 and tuple(f_vec.shape) != (xy.shape[1] + 2 * xz.shape[1], channels):
        raise N.K4Error(f'TensoRFGrid: f_vec is {tuple(f_vec.shape)}, expected {(xy.shape[1] + 2 * xz.shape[1], channels)}')
    return [N.f32(t) for t in factors] + [N.f32(f_vec) if channels > 1 else None, channels, xz.shape[1], xy.shape[1], X, Y, Z]


def _tensorf_fwd(factors, f_vec, channels, world, pts, xyz_min, xyz_max):
    out = torch.empty([pts.shape[0], channels], dtype=torch.float32, device=pts.device)
    N.check(N.lib().k4_tensorf_sample(*_tensorf_args(factors, f_vec, channels, world), N.f32(pts), N.f32(xyz_min), N.f32(xyz_max), pts.shape[0],
                                      N.f32(out), N.stream()), 'k4_tensorf_sample')
    return out


class TensoRFSample(torch.autograd.Function):
    """TensoRFGrid lookup with a HIP backward (k4_tensorf_sample_backward): gradients of the six factors and f_vec, the interpolated values recomputed from the
    points; none w.r.t. the points (they come from rays).  Float-atomic sums: not bitwise reproducible from run to run."""

    @staticmethod
    def forward(ctx, pts, xyz_min, xyz_max, channels, world, f_vec, *factors):
        factors = [f.detach().contiguous() for f in factors]
        f_vec = f_vec.detach().contiguous() if channels > 1 else None
        ctx.save_for_backward(pts, xyz_min, xyz_max, *factors, *([f_vec] if channels > 1 else []))
        ctx.channels, ctx.world = channels, world
        return _tensorf_fwd(factors, f_vec, channels, world, pts, xyz_min, xyz_max)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        pts, xyz_min, xyz_max, *rest = ctx.saved_tensors
        factors, f_vec = rest[:6], rest[6] if ctx.channels > 1 else None
        go = grad_out.float().contiguous()
        grads = [torch.zeros_like(f) for f in factors]
        g_f = torch.zeros_like(f_vec) if f_vec is not None else None
        N.check(N.lib().k4_tensorf_sample_backward(N.f32(go), *_tensorf_args(factors, f_vec, ctx.channels, ctx.world), N.f32(pts), N.f32(xyz_min), N.f32(xyz_max),
                                                   pts.shape[0], *[N.f32(g) for g in grads], N.f32(g_f) if g_f is not None else None, N.stream()),
                'k4_tensorf_sample_backward')
        return (None, None, None, None, None, g_f, *grads)


class TensoRFGrid(nn.Module):
    """Vector-matrix factored grid (TensoRF, arXiv:2203.09517; lib/grid.py:157-268): constructor, parameter / buffer names, initial distributions and
    semantics of the reference; lookup, backward, dense expansion and total variation on csrc/k4_tensorf.hip, resize on k4_resample_trilinear."""

    def __init__(self, channels, world_size, xyz_min, xyz_max, config):
        super().__init__()
        self.channels, self.world_size, self.config = channels, world_size, config
        for name, val in (('xyz_min', xyz_min), ('xyz_max', xyz_max)):
            self.register_buffer(name, _vec3(val))
        X, Y, Z = [int(v) for v in world_size]
        R = config['n_comp']
        Rxy = config.get('n_comp_xy', R)
        self.xy_plane = nn.Parameter(torch.randn([1, Rxy, X, Y]) * 0.1)
        self.xz_plane = nn.Parameter(torch.randn([1, R, X, Z]) * 0.1)
        self.yz_plane = nn.Parameter(torch.randn([1, R, Y, Z]) * 0.1)
        self.x_vec = nn.Parameter(torch.randn([1, R, X, 1]) * 0.1)
        self.y_vec = nn.Parameter(torch.randn([1, R, Y, 1]) * 0.1)
        self.z_vec = nn.Parameter(torch.randn([1, Rxy, Z, 1]) * 0.1)
        if self.channels > 1:
            self.f_vec = nn.Parameter(torch.ones([R + R + Rxy, channels]))
            nn.init.kaiming_uniform_(self.f_vec, a=math.sqrt(5))

    def factors(self):
        return [getattr(self, name) for name in _TENSORF_FACTORS]

    def _world(self):
        return (self.xy_plane.shape[2], self.xy_plane.shape[3], self.xz_plane.shape[3])

    def _device_factors(self, what):
        fs = [f.detach().contiguous() for f in self.factors()]
        fv = self.f_vec.detach().contiguous() if self.channels > 1 else None
        if not fs[0].is_cuda:
            raise N.K4Error(f'TensoRFGrid.{what}: the grid must be on the GPU (no CPU path)')
        return fs, fv

    def forward(self, xyz):
        """The six bilinear lookups, their products and the f_vec product of lib/grid.py:178-196, 241-268 in one kernel (k4_tensorf_sample); under autograd
        the backward is k4_tensorf_sample_backward."""
        shape = xyz.shape[:-1]
        pts = xyz.reshape(-1, 3).contiguous()
        if not pts.is_cuda or not self.xy_plane.is_cuda:
            raise N.K4Error('TensoRFGrid.forward: points and grid must be on the GPU (no CPU path)')
        params = self.factors() + ([self.f_vec] if self.channels > 1 else [])
        if torch.is_grad_enabled() and any(p.requires_grad for p in params):
            out = TensoRFSample.apply(pts.detach(), self.xyz_min, self.xyz_max, self.channels, self._world(),
                                      self.f_vec if self.channels > 1 else None, *self.factors())
        else:
            fs, fv = self._device_factors('forward')
            out = _tensorf_fwd(fs, fv, self.channels, self._world(), pts, self.xyz_min, self.xyz_max)
        return out.reshape(*shape, self.channels) if self.channels > 1 else out.reshape(*shape)

    def scale_volume_grid(self, new_world_size):
        """F.interpolate(bilinear, align_corners=True) of each factor (lib/grid.py:198-207) on k4_resample_trilinear with size-1 trailing axes: there the
        kernel's z weights are exactly (1, 0), which leaves torch's bilinear expression.  New parameters, as upstream."""
        if self.channels == 0:
            return
        X, Y, Z = [int(v) for v in new_world_size]
        fs, _ = self._device_factors('scale_volume_grid')
        for name, src, (a, b) in zip(_TENSORF_FACTORS, fs, ((X, Y), (X, Z), (Y, Z), (X, 1), (Y, 1), (Z, 1))):
            data = torch.empty([1, src.shape[1], a, b], dtype=torch.float32, device=src.device)
            N.check(N.lib().k4_resample_trilinear(N.f32(src), src.shape[1], src.shape[2], src.shape[3], 1, N.f32(data), a, b, 1, N.stream()), 'k4_resample_trilinear')
            setattr(self, name, nn.Parameter(data))
        self.world_size = new_world_size

    def total_variation_add_grad(self, wx, wy, wz, dense_mode=None):
        """lib/grid.py:209-221 without autograd: the smooth-L1 (beta 1, summed) total variation of the six factors, weighted per axis, / 6, added to ``.grad``
        (created when missing).  f_vec gets nothing; `dense_mode` is ignored, as upstream."""
        fs, _ = self._device_factors('total_variation_add_grad')
        for p, src, (wa, wb) in zip(self.factors(), fs, ((wx, wy), (wx, wz), (wy, wz), (wx, 0.), (wy, 0.), (wz, 0.))):
            if p.grad is None:
                p.grad = torch.zeros_like(p, memory_format=torch.contiguous_format)
            N.check(N.lib().k4_tensorf_tv_add_grad(N.f32(src), N.f32(p.grad), src.shape[1], src.shape[2], src.shape[3], float(wa), float(wb), N.stream()),
                    'k4_tensorf_tv_add_grad')

    @torch.no_grad()
    def get_dense_grid(self):
        """[1, C, X, Y, Z] = sum_r plane_r (x) vec_r (times f_vec) of lib/grid.py:223-236 (k4_tensorf_dense)."""
        fs, fv = self._device_factors('get_dense_grid')
        X, Y, Z = self._world()
        out = torch.empty([1, self.channels, X, Y, Z], dtype=torch.float32, device=fs[0].device)
        N.check(N.lib().k4_tensorf_dense(*_tensorf_args(fs, fv, self.channels, (X, Y, Z)), N.f32(out), N.stream()), 'k4_tensorf_dense')
        return out

    def factor_key(self):
        """(data_ptr, version) of every factor parameter: what a cached dense expansion is keyed on."""
        return tuple((p.data_ptr(), p._version) for p in self.factors() + ([self.f_vec] if self.channels > 1 else []))

    def extra_repr(self):
        ws = self.world_size.tolist() if torch.is_tensor(self.world_size) else list(self.world_size)
        return f'channels={self.channels}, world_size={ws}, n_comp={self.config["n_comp"]}'


class VQProject(torch.autograd.Function):
    """v = W2 relu(W1 x + b1) + b2 of VQGrid.project_layer (lib/grid.py:54-58,64) on k4_vq_project_fwd; the backward (k4_vq_project_bwd) sums the four
    parameter gradients in a fixed order and hands the input its gradient only when the input requires one."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2):
        x = x.detach().contiguous()
        ws = [t.detach().contiguous() for t in (w1, b1, w2, b2)]
        n, in_dim = x.shape
        dim = ws[0].shape[0]
        need = any(ctx.needs_input_grad)
        h = torch.empty([n, dim], dtype=torch.float32, device=x.device) if need else None
        v = torch.empty([n, dim], dtype=torch.float32, device=x.device)
        N.check(N.lib().k4_vq_project_fwd(N.f32(x), n, in_dim, dim, *[N.f32(t) for t in ws], None if h is None else N.f32(h), N.f32(v), N.stream()),
                'k4_vq_project_fwd')
        if need:
            ctx.save_for_backward(x, h, ws[0], ws[2])
        return v

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_v):
        x, h, w1, w2 = ctx.saved_tensors
        n, in_dim = x.shape
        dim = w1.shape[0]
        g = grad_v.float().contiguous()
        gx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        gw1, gb1, gw2, gb2 = torch.empty_like(w1), w1.new_empty([dim]), torch.empty_like(w2), w2.new_empty([dim])
        L = N.lib()
        wsb = int(L.k4_vq_project_bwd_workspace_bytes(n, in_dim, dim))
        work = torch.empty([max(wsb, 4) // 4], dtype=torch.float32, device=x.device)
        N.check(L.k4_vq_project_bwd(N.f32(x), N.f32(h), N.f32(g), n, in_dim, dim, N.f32(w1), N.f32(w2), None if gx is None else N.f32(gx),
                                    N.f32(gw1), N.f32(gb1), N.f32(gw2), N.f32(gb2), N.f32(work), wsb, N.stream()), 'k4_vq_project_bwd')
        return gx, gw1, gb1, gw2, gb2


class VQAssign(torch.autograd.Function):
    """(quantize, diff, embed_ind) of lib/grid.py:67-100 for the projected vectors v [n, dim]: the nearest codeword by k4_vq_assign and, with `train`, one
    moving-average update of the owner's three buffers after the features were taken from the old codebook.  Straight-through: quantize's gradient is
    v's; diff = mean((e - v)^2) adds 2 (v - e) / numel of its own; the buffers get none."""

    @staticmethod
    def forward(ctx, v, owner, train):
        v = v.detach().contiguous()
        n, dim = v.shape
        dev = v.device
        L = N.lib()
        ne = owner.n_embed
        ind = torch.empty([n], dtype=torch.int64, device=dev)
        q = torch.empty([n, dim], dtype=torch.float32, device=dev)
        diff = torch.empty([], dtype=torch.float32, device=dev)
        wsb = int(L.k4_vq_assign_workspace_bytes(n, dim, ne, int(train)))
        work = torch.empty([wsb // 8], dtype=torch.float64, device=dev)
        N.check(L.k4_vq_assign(N.f32(v), n, dim, N.f32(owner.prepared_codebook()), ne, N.ptr(ind), N.f32(q), N.f32(diff), int(train), N.ptr(work), wsb,
                               N.stream()), 'k4_vq_assign')
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(v, q)
        if train:
            owner._ema_update(work, n)
        ctx.mark_non_differentiable(ind)
        ctx.set_materialize_grads(False)
        return q, diff, ind

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_q, g_diff, _g_ind):
        v, q = ctx.saved_tensors
        g = g_q
        if g_diff is not None:
            # q = v + (e - v) = e up to the last bit
            d = (v - q) * (g_diff * (2.0 / max(v.numel(), 1)))
            g = d if g is None else g + d
        return g, None, None


class VQGrid(nn.Module):
    """Vector-quantised feature field (lib/grid.py:38-103): constructor, buffer / parameter names and semantics of the reference.  ``world_size`` is the
    number of codewords.  ``forward(ind_norm)`` projects the embedded position (Linear, ReLU, Linear), finds the nearest of the ``n_embed`` codewords and
    returns ``(v + (e - v), mean((e - v)^2), index)``; with the module in training mode -- whatever the autograd mode, as upstream -- the codebook then
    moves by one exponential-moving-average step.  Everything runs on csrc/k4_vq.hip; there is no CPU path."""

    def __init__(self, input_dim, channels, world_size, xyz_min, xyz_max, decay=0.99, eps=1e-5, **kwargs):
        super().__init__()
        self.dim, self.n_embed, self.decay, self.eps = int(channels), int(world_size), decay, eps
        for name, val in (('xyz_min', xyz_min), ('xyz_max', xyz_max)):
            self.register_buffer(name, _vec3(val))
        embed = torch.randn(self.dim, self.n_embed)
        self.register_buffer('embed', embed)
        self.register_buffer('cluster_size', torch.zeros(self.n_embed))
        self.register_buffer('embed_avg', embed.clone())
        self.project_layer = nn.Sequential(nn.Linear(input_dim, self.dim), nn.ReLU(), nn.Linear(self.dim, self.dim))
        if not (1 <= input_dim <= 63 and 1 <= self.dim <= 32 and self.n_embed >= 1):
            raise NotImplementedError(f'VQGrid(input_dim={input_dim}, channels={channels}, world_size={world_size}): the kernels of csrc/k4_vq.hip cover '
                                      '1..63 inputs, 1..32 channels and at least one codeword')

    def _flat(self, ind_norm, what):
        if not ind_norm.is_cuda or not self.embed.is_cuda:
            raise N.K4Error(f'VQGrid.{what}: input and module must be on the GPU (no CPU path)')
        return ind_norm.reshape(-1, ind_norm.shape[-1]).float()

    def project(self, ind_norm):
        """``project_layer(ind_norm)`` (lib/grid.py:64) -> [..., dim]."""
        l1, l2 = self.project_layer[0], self.project_layer[2]
        v = VQProject.apply(self._flat(ind_norm, 'project'), l1.weight, l1.bias, l2.weight, l2.bias)
        return v.reshape(*ind_norm.shape[:-1], self.dim)

    def prepared_codebook(self):
        """The codebook as k4_vq_assign reads it (codewords contiguous, |e|^2 behind each), cached per version of ``embed``."""
        e = self.embed
        key = (e.data_ptr(), e._version, str(e.device))
        hit = self.__dict__.get('_k4_prepared')
        if hit is None or hit[0] != key:
            src = e.detach().float().contiguous()
            out = torch.empty([int(N.lib().k4_vq_codebook_floats(self.dim, self.n_embed))], dtype=torch.float32, device=e.device)
            N.check(N.lib().k4_vq_prepare_codebook(N.f32(src), self.dim, self.n_embed, N.f32(out), N.stream()), 'k4_vq_prepare_codebook')
            hit = self.__dict__['_k4_prepared'] = (key, out)
        return hit[1]

    def _ema_update(self, work, n):
        """lib/grid.py:80-93 from the counts and sums k4_vq_assign left in `work`: the three buffers in place, their versions bumped (a kernel's store
        does not bump them), so the prepared codebook re-keys."""
        bufs = (self.cluster_size, self.embed_avg, self.embed)
        if any(b.dtype != torch.float32 or not b.is_contiguous() for b in bufs):
            raise N.K4Error('VQGrid: the codebook buffers must be contiguous fp32 tensors')
        N.check(N.lib().k4_vq_update_codebook(N.ptr(work), n, self.dim, self.n_embed, float(self.decay), float(1 - self.decay), float(self.eps),
                                              float(self.n_embed * self.eps), *[N.f32(b) for b in bufs], N.stream()), 'k4_vq_update_codebook')
        for b in bufs:
            torch.autograd.graph.increment_version(b)

    def forward(self, ind_norm):
        shape = ind_norm.shape[:-1]
        v = self.project(ind_norm).reshape(-1, self.dim)
        quantize, diff, embed_ind = VQAssign.apply(v, self, bool(self.training))
        return quantize.reshape(*shape, self.dim), diff, embed_ind.reshape(*shape)

    def embed_code(self, embed_id):
        """lib/grid.py:102-103: the codewords of the given indices, [..., dim]."""
        if not embed_id.is_cuda or not self.embed.is_cuda:
            raise N.K4Error('VQGrid.embed_code: indices and module must be on the GPU (no CPU path)')
        return self.embed.t().index_select(0, embed_id.reshape(-1)).reshape(*embed_id.shape, self.dim)

    def __deepcopy__(self, memo):
        import copy
        new = self.__class__.__new__(self.__class__)
        memo[id(self)] = new
        for k, val in self.__dict__.items():
            if k != '_k4_prepared':
                new.__dict__[k] = copy.deepcopy(val, memo)
        return new

    def extra_repr(self):
        return f'channels={self.dim}, n_embed={self.n_embed}, decay={self.decay}'


def _mask_from_coarse_checkpoint(path, thres):
    """Occupancy of a coarse-stage DVGO checkpoint (lib/grid.py:277-284): alpha of the 3x3x3 max-pooled density >= thres."""
    st = torch.load(path, map_location='cpu', weights_only=False)
    sd, kw = st['model_state_dict'], st['model_kwargs']
    pooled = F.max_pool3d(sd['density.grid'], kernel_size=3, padding=1, stride=1)
    alpha = 1 - torch.exp(-F.softplus(pooled + sd['act_shift']) * kw['voxel_size_ratio'])
    return (alpha >= thres)[0, 0], kw['xyz_min'], kw['xyz_max']


def occupancy_from_alpha(alpha, thres):
    """(F.max_pool3d(alpha[None,None], kernel_size=3, padding=1, stride=1)[0,0] > thres) for an [X,Y,Z] fp32 device tensor, on
    the HIP kernel k4_alpha_maxpool3_gt -> bool tensor [X,Y,Z]."""
    a = alpha.detach().float().contiguous()
    if a.dim() != 3 or not a.is_cuda:
        raise N.K4Error('occupancy_from_alpha: [X,Y,Z] device tensor expected')
    out = torch.empty(a.shape, dtype=torch.bool, device=a.device)
    N.check(N.lib().k4_alpha_maxpool3_gt(N.f32(a), a.shape[0], a.shape[1], a.shape[2], float(thres), N.ptr(out), N.stream()),
            'k4_alpha_maxpool3_gt')
    return out


def grid_nodes(xyz_min, xyz_max, shape):
    """World positions of the nodes of an [X,Y,Z] grid spanning the bbox (the meshgrid of linspaces of lib/dmpigo.py:199-203)."""
    return torch.stack(torch.meshgrid(*grid_axes(xyz_min, xyz_max, shape), indexing='ij'), -1)


def grid_axes(xyz_min, xyz_max, shape):
    """The three 1-D node coordinate axes ``grid_nodes`` is the meshgrid of."""
    dev = xyz_min.device
    return [torch.linspace(float(xyz_min[i]), float(xyz_max[i]), int(shape[i]), device=dev) for i in range(3)]


class MaskGrid(nn.Module):
    """Boolean occupancy grid + the affine map world -> voxel index (buffers `mask`, `xyz2ijk_scale`, `xyz2ijk_shift`)."""

    def __init__(self, path=None, mask_cache_thres=None, mask=None, xyz_min=None, xyz_max=None):
        super().__init__()
        if path is not None:
            self.mask_cache_thres = mask_cache_thres
            mask, xyz_min, xyz_max = _mask_from_coarse_checkpoint(path, mask_cache_thres)
        lo, hi = _vec3(xyz_min), _vec3(xyz_max)
        self.register_buffer('mask', mask.bool())
        scale = (torch.Tensor(list(mask.shape)) - 1) / (hi - lo)
        self.register_buffer('xyz2ijk_scale', scale)
        self.register_buffer('xyz2ijk_shift', -lo * scale)

    @torch.no_grad()
    def forward(self, xyz):
        """Skip known free space: nearest-voxel lookup with C round() (lib/grid.py:295-304) on k4_maskcache_lookup."""
        pts = xyz.reshape(-1, 3).contiguous()
        hit = render_utils_cuda.maskcache_lookup(self.mask, pts, self.xyz2ijk_scale, self.xyz2ijk_shift)
        return hit.reshape(xyz.shape[:-1])

    def extra_repr(self):
        return f'mask.shape={list(self.mask.shape)}'
