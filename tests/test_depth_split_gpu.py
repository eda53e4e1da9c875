"""The fused MPI marcher's two-launch geometry stage (k4_grid_desc.depth_split: k4_geom3_kernel with slab = 1, then slab = 2 on the rays the
first launch's transmittance scan left alive) against the single launch, which it must equal to the BIT -- a ray's records reach the scan in
depth order either way, through the same fmaf chain, and the shading kernel's per-ray sums are fixed point -- and against the CPU oracle.
Then the load-time statistic that proposes a split (k4_mpi_depth_split_stats) against its fp64 restatement (tests/depth_split_oracle.py).

The switches are in-process: dmpigo.DEPTH_SPLIT = False is the single launch, a forced split k is DirectMPIGO._k4_depth_split patched to return
k under a plan-cache key of its own (DEPTH_SPLIT_MIN_GAIN nudged by k, as tools/march_split_time.py does).  After every march the split is read
back from the cached plan's k4_grid_desc: k for a split run, 0 for a base run -- single launch against single launch would prove nothing.

Shapes (grid ~48 x 48 x mpi_depth, frame 40 x 56: the width is no multiple of 8, the bundles are ragged):
  n128   128 planes, stepsize 1               split 64: the smallest there is
  n256   256 planes, stepsize 1 (interval 1)  splits 64, 128, 192; the base run takes the FAST geometry instantiation: split against FAST
  n130   130 planes, stepsize 1               split 128: the back slab holds 2 samples, span1 = 16, almost every group empty
  n199   100 planes, stepsize 0.5 (199)       splits 64, 192: ragged back slab, the powf form of raw2alpha (interval 1.28)
  n319   160 planes, stepsize 0.5 (319)       split 256: span0 = 64, samples beyond the K4_TKTAB table
Scenes (each aims at one rule of the slab arithmetic):
  opaque   scene.make_llff_checkpoint(opaque=True): a slanted wall over planes 0.29 .. 0.51 of the depth -- in front of, across or behind the split
  blob     six translucent blobs and the translucent sheet: survivors on both sides, the back launch appends behind the front launch's
  sheet    blob + a FLAT opaque sheet (+22 over three planes, x < 0.8 X) whose first plane is sample k - 1, k or k + 1: the crossing sample of the
           T < 1e-3 stop is the last of the front slab, the first of the back slab, the one behind it; far in front / far behind: every covered ray
           dead in the back launch / none stopped in front
  behind   translucent content only behind every split: the front launch leaves counts = 0 and must not finalise the outputs
  front    translucent content only in front of every split: the back launch finds no record, keeps counts and must not overwrite rgb
  empty    no content: rgb = alphainv * bg (bg = 1), depth = 0, written by the back launch
Outputs cannot show whether the back launch really skips a stopped ray (the scan drops such a ray's records anyway):
test_back_launch_takes_no_sample_of_a_stopped_ray compares the marcher's workspace bytes instead.

Each of these breaks of k4_geom3_kernel was tried once against this file: run0 dropped from the back launch's run pointer (31 tests fail: every
case with survivors on both sides), the back launch's cnt started at 0 (55), `alive` always true together with the scan's stored-T stop ignored (52);
`alive` always true alone changes no output and fails the workspace test only.
"""
import functools

import numpy as np
import pytest
import torch

import nerf4k_amd  # noqa: F401
from nerf4k_amd import scene, _native as N
from nerf4k_amd.lib import utils, dmpigo
from oracle import marcher
import depth_split_oracle as DSO
from test_march_gpu import _cmp

pytestmark = pytest.mark.gpu

KEYS = ('rgb_marched', 'depth', 'alphainv_last')
H, W, POSE = 40, 56, 7
SHAPES = {'n128': (128, 1.0), 'n256': (256, 1.0), 'n130': (130, 1.0), 'n199': (100, 0.5), 'n319': (160, 0.5)}
N_SAMPLES = {s: int((d - 1) / st) + 1 for s, (d, st) in SHAPES.items()}
assert N_SAMPLES == {'n128': 128, 'n256': 256, 'n130': 130, 'n199': 199, 'n319': 319}


@pytest.fixture(autouse=True)
def _inference_mode():
    with torch.no_grad():
        yield


# ---------------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------------
def _slab(sd, z0, z1):
    """Translucent content on planes [z0, z1), x < 0.7 X: density + act_shift = -3 +- 1.3 (alpha 0.01 .. 0.2 per sample; -0.5 +- 1.3 where only a few
    planes hold it, so that a ray still loses half its transmittance), everything else empty."""
    d, act = sd['density.grid'], sd['act_shift.grid'].reshape(-1)
    X, Y, Z = d.shape[2:]
    d.fill_(-30.0)
    x, y, z = torch.arange(X).float()[:, None, None], torch.arange(Y).float()[None, :, None], torch.arange(z0, z1).float()[None, None, :]
    raw = (-3.0 if z1 - z0 >= 8 else -0.5) + torch.sin(0.45 * x + 0.3 * z) * torch.cos(0.6 * y) + 0.3 * torch.sin(1.7 * z + 0.2 * y)
    d[0, 0, :int(0.7 * X), :, z0:z1] = (raw - act[z0:z1])[:int(0.7 * X)]
    sd['mask_cache.mask'].fill_(True)                         # (the live mask the render path derives from the density drops the empty part)


@functools.lru_cache(maxsize=4)
def _checkpoint(kind, shape, arg=None, frame=(H, W)):
    """-> (checkpoint, rays [ro, rd, vd] on the CPU, flattened).  `arg`: sheet -- the plane of its first layer; behind / front -- the planes
    [arg, arg + 40) / [arg - 40, arg) that hold the content."""
    D, stepsize = SHAPES[shape]
    kw = dict(num_voxels=48 * 48 * D, mpi_depth=D, stepsize=stepsize)
    if kind == 'opaque':
        ck = scene.make_llff_checkpoint(seed=781, opaque=True, **kw)
    else:
        ck = scene.make_llff_checkpoint(seed=779, n_blobs=6, **kw)
    sd = ck['model_state_dict']
    Z = sd['density.grid'].shape[-1]
    assert Z == D and sd['mask_cache.mask'].shape == sd['density.grid'].shape[2:]
    if kind == 'sheet':
        xs = int(0.8 * sd['density.grid'].shape[2])
        sd['density.grid'][0, 0, :xs, :, arg:arg + 3] = 22.0
        sd['mask_cache.mask'][:xs, :, max(arg - 1, 0):arg + 4] = True
    elif kind == 'behind':
        _slab(sd, arg, min(arg + 40, Z))
    elif kind == 'front':
        _slab(sd, max(arg - 40, 0), arg)
    elif kind == 'empty':
        sd['density.grid'].fill_(-30.0)
    else:
        assert kind in ('opaque', 'blob'), kind
    if kind in ('behind', 'front', 'empty'):
        ck['render_kwargs'] = dict(ck['render_kwargs'], bg=1)
    h, w = frame
    K = scene.LLFF_K.copy()
    K[:2] *= w / scene.LLFF_HW[1]
    rays = [x.reshape(-1, 3).contiguous() for x in marcher.get_rays_of_a_view(h, w, K, scene.llff_spiral_poses()[POSE], ndc=True)]
    return ck, rays


# ---------------------------------------------------------------------------------------------------------------------
# marches
# ---------------------------------------------------------------------------------------------------------------------
def _march(model, rays, rk, split, img_w, k4_out=None, real_rule=False):
    """One march with the geometry stage as `split` says (0: single launch; k: forced split; real_rule: DEPTH_SPLIT on, the model's own choice)
    -> (clones of the three outputs, the depth_split of the plan the march ran on)."""
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(dmpigo, 'DEPTH_SPLIT', bool(split) or real_rule)
        if split and not real_rule:
            mp.setattr(dmpigo.DirectMPIGO, '_k4_depth_split', lambda self, gd, n, itv: split)
            mp.setattr(dmpigo, 'DEPTH_SPLIT_MIN_GAIN', 0.05 + split * 1e-6)           # a plan key of its own: no cached plan of another split is reused
        out = model(*rays, k4_img_w=img_w, **(rk if k4_out is None else dict(rk, k4_out=k4_out)))
        torch.cuda.synchronize()
    plan = model._k4_cache()[('plan', 'mpi')]
    return {k: out[k].clone() for k in KEYS}, int(plan[1][1].depth_split)


@functools.lru_cache(maxsize=4)
def _loaded(kind, shape, arg=None, frame=(H, W)):
    """-> dict: the scene on the GPU and its single-launch frame (image layout), made once per scene."""
    ck, rays = _checkpoint(kind, shape, arg, frame)
    model = utils.model_from_checkpoint_dict(ck).cuda().eval()
    rk = dict(ck['render_kwargs'], render_depth=True)
    drays = [r.cuda() for r in rays]
    with torch.no_grad():
        base, split = _march(model, drays, rk, 0, frame[1])
    assert split == 0
    return dict(ck=ck, model=model, rk=rk, rays=drays, cpu_rays=rays, base=base, n=N_SAMPLES[shape])


def _assert_equal(got, want, what):
    for k in KEYS:
        if not torch.equal(got[k], want[k]):
            d = (got[k].double() - want[k].double()).abs()
            d = torch.nan_to_num(d, nan=float('inf'))
            rays = d.reshape(d.shape[0], -1).amax(1)
            raise AssertionError(f'{what}: {k} differs on {int((rays > 0).sum())} of {rays.numel()} rays, max |diff| {float(rays.max()):.3e}, '
                                 f'first rays {(rays > 0).nonzero().flatten()[:8].tolist()}')


def _assert_not_trivial(kind, base, bg):
    """The base frame is what the scene says: coloured rays and background rays, or nothing but background."""
    ainv, rgb, depth = base['alphainv_last'], base['rgb_marched'], base['depth']
    assert torch.isfinite(rgb).all() and torch.isfinite(depth).all() and torch.isfinite(ainv).all()
    untouched = ainv == 1.0
    if kind == 'empty':
        assert bool(untouched.all()) and bool((rgb == bg).all()) and bool((depth == 0).all())
        return
    hit = ainv < 0.5
    assert int(hit.sum()) > 0.15 * ainv.numel(), int(hit.sum())
    assert float(rgb[hit].std()) > 0.01 and float(depth[hit].std()) > 1e-3           # colours and depths vary over the covered rays
    if kind in ('opaque', 'sheet'):
        assert int((ainv < 1e-3).sum()) > 0.5 * ainv.numel()                           # rays that reach the stop
    else:
        assert int((ainv >= 1e-3).sum()) > 0.5 * ainv.numel()                          # rays the back launch still marches
    if kind in ('behind', 'front'):                                                    # (content on x < 0.7 X only; the other scenes fill the frame)
        assert int(untouched.sum()) > 0.05 * ainv.numel(), int(untouched.sum())
    assert bool((rgb[untouched] == bg).all()) and bool((depth[untouched] == 0).all())


# ---------------------------------------------------------------------------------------------------------------------
# a. bit identity
# ---------------------------------------------------------------------------------------------------------------------
def _cases():
    c = []
    c += [('opaque', 'n128', None, 64), ('blob', 'n128', None, 64), ('sheet', 'n128', 64, 64), ('empty', 'n128', None, 64)]
    for k in (64, 128, 192):
        c += [('sheet', 'n256', k + off, k) for off in (-1, 0, 1)]
    c += [('behind', 'n256', 200, k) for k in (64, 128, 192)]
    c += [('front', 'n256', 56, k) for k in (64, 128, 192)]
    c += [('opaque', 'n256', None, k) for k in (64, 128, 192)]                      # wall over samples 74 .. 131: behind 64, across 128, in front of 192
    c += [('blob', 'n256', None, k) for k in (64, 128, 192)]
    c += [('sheet', 'n256', 30, 128), ('sheet', 'n256', 220, 128)]                  # flat wall far in front of / entirely behind the split
    c += [('blob', 'n130', None, 128), ('opaque', 'n130', None, 128), ('sheet', 'n130', 128, 128), ('behind', 'n130', 128, 128)]
    c += [('blob', 'n199', None, 64), ('blob', 'n199', None, 192), ('opaque', 'n199', None, 64), ('opaque', 'n199', None, 192),
          ('sheet', 'n199', 96, 192), ('empty', 'n199', None, 192)]                 # (plane 96 = sample 192)
    c += [('blob', 'n319', None, 256), ('opaque', 'n319', None, 256), ('sheet', 'n319', 140, 256), ('behind', 'n319', 130, 256)]
    return c


@pytest.mark.parametrize('kind,shape,arg,k', _cases(), ids=lambda v: str(v))
def test_split_is_bit_identical(kind, shape, arg, k):
    S = _loaded(kind, shape, arg)
    assert 0 < k < S['n'] and k % 64 == 0
    _assert_not_trivial(kind, S['base'], float(S['rk']['bg']))
    got, split = _march(S['model'], S['rays'], S['rk'], k, W)
    assert split == k
    _assert_equal(got, S['base'], f'{kind} {shape} arg={arg} split {k}')
    if kind == 'sheet' and shape in ('n128', 'n256') and abs(arg - k) <= 1:
        # the premise (stepsize 1: sample = plane): rays that stop with ALL their weight on sample `arg`, depth = (arg + 0.5) / n -- nothing in front
        # of the sheet, the crossing sample is the sheet's first plane.  (Fewer at 192, where the scene's own translucent sheet lies in front.)
        b = S['base']
        at = (b['alphainv_last'] < 1e-3) & ((b['depth'] - (arg + 0.5) / S['n']).abs() < 0.25 / S['n'])
        assert int(at.sum()) > 0.05 * at.numel(), int(at.sum())


# ---------------------------------------------------------------------------------------------------------------------
# b. ray layouts
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['opaque', 'blob'])
@pytest.mark.parametrize('layout', ['linear_1297', 'linear_37', 'image'])
def test_split_ray_layouts(kind, layout):
    """A linear ray list whose length is no multiple of 64, one shorter than a bundle, and the image layout: each against its own single launch."""
    S = _loaded(kind, 'n256')
    n = {'linear_1297': 64 * 20 + 17, 'linear_37': 37, 'image': H * W}[layout]
    first = 0 if layout == 'image' else 611
    rays = [r[first:first + n].contiguous() for r in S['rays']]
    img_w = W if layout == 'image' else 0
    base, s0 = _march(S['model'], rays, S['rk'], 0, img_w)
    got, s1 = _march(S['model'], rays, S['rk'], 128, img_w)
    assert (s0, s1) == (0, 128)
    assert int((base['alphainv_last'] < 0.5).sum()) > 0
    _assert_equal(got, base, f'{kind} {layout}')


# ---------------------------------------------------------------------------------------------------------------------
# c. out_alphainv as the state between the launches
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind,arg', [('opaque', None), ('blob', None), ('behind', 200)])
@pytest.mark.parametrize('fill', [float('nan'), 0.0])
def test_split_defines_every_rays_transmittance(kind, arg, fill):
    """The back launch reads each ray's T from out_alphainv: the front launch must have written it for EVERY ray (also where it found nothing),
    whatever the caller's buffer held -- NaN (never below 1e-3: every ray alive, T poisoned) or 0 (every ray dead)."""
    S = _loaded(kind, 'n256', arg)
    nr = H * W
    bufs = (torch.full([nr, 3], fill, device='cuda'), torch.full([nr], fill, device='cuda'), torch.full([nr], fill, device='cuda'))
    first, s1 = _march(S['model'], S['rays'], S['rk'], 128, W, k4_out=bufs)
    assert s1 == 128
    _assert_equal(first, S['base'], f'{kind} into buffers of {fill}')
    again, _ = _march(S['model'], S['rays'], S['rk'], 128, W, k4_out=bufs)          # now the buffers hold the previous frame
    _assert_equal(again, first, f'{kind} second run into the same buffers')
    assert torch.equal(bufs[2], first['alphainv_last'])


def test_back_launch_takes_no_sample_of_a_stopped_ray():
    """What the split is for, and what no output can show (the scan drops a stopped ray's records anyway): the back launch records NOTHING for a ray
    the front launch stopped.  Scene A: blobs throughout the depth behind a flat opaque sheet at plane 30 over the whole grid; scene B: A with the
    planes from 136 on emptied (the split is 128: no sample of the front slab reads them).  On the rays that stop in A, the marcher's workspace --
    raw records, survivors, counts, shading queue -- must come out the same bytes for A and for B: whatever lies behind the split is never looked at."""
    import copy
    a = scene.make_llff_checkpoint(seed=779, n_blobs=24, num_voxels=48 * 48 * 256, mpi_depth=256)
    sd = a['model_state_dict']
    sd['density.grid'][..., 30:33] = 22.0
    sd['mask_cache.mask'][..., 29:34] = True
    b = copy.deepcopy(a)
    b['model_state_dict']['density.grid'][..., 136:] = -30.0
    behind = DSO.stats(sd['density.grid'][0, 0, :, :, 136:].numpy(), sd['act_shift.grid'].reshape(-1)[136:].numpy(), 1.0, a['model_kwargs']['fast_color_thres'])
    assert behind['voxels'] > 1000, behind['voxels']                     # A does hold alpha-passing voxels back there
    rays = [r.cuda() for r in _checkpoint('blob', 'n256')[1]]
    rk = dict(a['render_kwargs'], render_depth=True)
    out, ws = {}, {}
    for name, ck in (('a', a), ('b', b)):
        model = utils.model_from_checkpoint_dict(ck).cuda().eval()
        frame, _ = _march(model, rays, rk, 0, W)                         # (both models: the same workspace allocation)
        if name == 'a':
            stopped = (frame['alphainv_last'] < 1e-3).nonzero().flatten()
            assert 0.8 * H * W < stopped.numel()
            sub = [r[stopped].contiguous() for r in rays]
        _march(model, sub, rk, 128, 0)                                    # (allocates the workspace)
        for run in (name, name + '_again'):
            model._k4_cache()[('workspace', 0)].fill_(0xA5)
            out[run], split = _march(model, sub, rk, 128, 0)
            assert split == 128
            ws[run] = model._k4_cache()[('workspace', 0)].clone()
    assert bool((out['a']['alphainv_last'] < 1e-3).all())
    assert torch.equal(ws['a'], ws['a_again']) and torch.equal(ws['b'], ws['b_again'])          # the premise: a march leaves the same bytes every time
    assert ws['a'].shape == ws['b'].shape
    diff = int((ws['a'] != ws['b']).sum())
    assert diff == 0, f'{diff} workspace bytes depend on the density behind the split although every ray stopped in front of it'
    _assert_equal(out['a'], out['b'], 'scenes A and B on the stopped rays')


# ---------------------------------------------------------------------------------------------------------------------
# d. the CPU oracle
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind,shape,arg,k', [('opaque', 'n256', None, 128), ('blob', 'n256', None, 128), ('sheet', 'n256', 128, 128),
                                              ('opaque', 'n199', None, 64)], ids=lambda v: str(v))
def test_split_frame_vs_oracle(kind, shape, arg, k):
    """The split frame against oracle.marcher with the bars of test_mpi_frame_vs_oracle (>= 100 dB per frame, 99.9 % of rays within 2e-5, every
    ray within 2e-3), on that test's 90 x 120 frame: the per-ray bounds allow a sample whose alpha or weight sits at the threshold to flip, and the
    frame bar was set where one such ray in 10800 costs 0.1 dB, not the 5 dB it costs in 2240."""
    frame = (90, 120)
    S = _loaded(kind, shape, arg, frame)
    got, split = _march(S['model'], S['rays'], S['rk'], k, frame[1])
    assert split == k
    ck = S['ck']
    want = marcher.forward('DirectMPIGO', ck['model_kwargs'], ck['model_state_dict'], *S['cpu_rays'], **ck['render_kwargs'])
    for key, name in zip(KEYS, ('rgb', 'depth', 'alphainv')):
        d = (got[key].cpu() - want[key]).abs()
        print(kind, shape, k, name, 'max', float(d.max()), 'within 2e-5', float((d.reshape(d.shape[0], -1).amax(1) <= 2e-5).float().mean()))
    _cmp(got['rgb_marched'], want['rgb_marched'], 'rgb', min_psnr=100.0)
    _cmp(got['depth'], want['depth'], 'depth', min_psnr=100.0)
    _cmp(got['alphainv_last'], want['alphainv_last'], 'alphainv', min_psnr=100.0)
    _assert_equal(got, S['base'], f'{kind} {shape} split {k} on the 90 x 120 frame')


# ---------------------------------------------------------------------------------------------------------------------
# e. the split the load-time statistic proposes
# ---------------------------------------------------------------------------------------------------------------------
def _own_choice(ck):
    model = utils.model_from_checkpoint_dict(ck).cuda().eval()
    rk = dict(ck['render_kwargs'], render_depth=True)
    K = scene.LLFF_K.copy()
    K[:2] *= W / scene.LLFF_HW[1]
    rays = [x.reshape(-1, 3).contiguous().cuda() for x in marcher.get_rays_of_a_view(H, W, K, scene.llff_spiral_poses()[POSE], ndc=True)]
    base, s0 = _march(model, rays, rk, 0, W)
    got, s1 = _march(model, rays, rk, 0, W, real_rule=True)
    assert s0 == 0 and s1 == int(model._k4_cache()['dsplit'])
    assert int((base['alphainv_last'] < 0.5).sum()) > 0.15 * H * W
    _assert_equal(got, base, f'proposed split {s1}')
    return s1, model._k4_cache()['dsplit_stats']


def test_opaque_scene_proposes_a_split_and_renders_the_same():
    """The 128-plane opaque-wall scene: every occupied column stops a ray and a large share of the voxels lies behind the wall."""
    split, st = _own_choice(scene.make_llff_checkpoint(seed=781, num_voxels=96 * 96 * 128, mpi_depth=128, opaque=True))
    print('statistic', [round(v, 4) for v in st], '-> split', split)
    assert split > 0 and split % 64 == 0 and split < 128
    assert st[0] >= dmpigo.DEPTH_SPLIT_MIN_OPAQUE and st[4] >= dmpigo.DEPTH_SPLIT_MIN_GAIN


def test_translucent_scene_renders_the_same_whatever_is_proposed():
    split, st = _own_choice(scene.make_llff_checkpoint(seed=779, num_voxels=48 * 48 * 256, mpi_depth=256, n_blobs=6))
    print('statistic', [round(v, 4) for v in st], '-> split', split)
    assert split == dmpigo.depth_split_of(st, 256, dmpigo.DEPTH_SPLIT_MIN_GAIN, dmpigo.DEPTH_SPLIT_MIN_OPAQUE)


# ---------------------------------------------------------------------------------------------------------------------
# f. descriptor validation
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,bad', [('n256', 32), ('n256', -64), ('n256', 256), ('n256', 320), ('n128', 128), ('n130', 192), ('n199', 100)])
def test_bad_split_is_refused_on_the_host(shape, bad):
    """Not a multiple of 64, negative, n_samples itself, beyond n_samples: K4_ERR_BAD_ARG before anything is launched -- the outputs keep the
    caller's bytes."""
    S = _loaded('blob', shape)
    assert bad < 0 or bad % 64 != 0 or bad >= S['n']
    nr = H * W
    bufs = (torch.full([nr, 3], 7.0, device='cuda'), torch.full([nr], 7.0, device='cuda'), torch.full([nr], 7.0, device='cuda'))
    with pytest.raises(N.K4Error, match='K4_ERR_BAD_ARG'):
        _march(S['model'], S['rays'], S['rk'], bad, W, k4_out=bufs)
    torch.cuda.synchronize()
    assert all(bool((b == 7.0).all()) for b in bufs)
    got, split = _march(S['model'], S['rays'], S['rk'], 64, W)                        # the model is none the worse for it
    assert split == 64
    _assert_equal(got, S['base'], 'after a refused call')


# ---------------------------------------------------------------------------------------------------------------------
# the load-time statistic
# ---------------------------------------------------------------------------------------------------------------------
def _kernel_stats(d, act, interval, thres):
    dens = torch.from_numpy(np.ascontiguousarray(d)).cuda()
    a = torch.from_numpy(act).cuda()
    gd = N.GridDesc()
    gd.density, gd.act_shift, gd.act_depth = dens.data_ptr(), a.data_ptr(), int(a.numel())
    gd.dims = (N.C.c_int32 * 3)(*[int(v) for v in dens.shape])
    out = torch.full([16], float('nan'), device='cuda')                               # (the entry point zeroes its accumulators itself)
    N.check(N.lib().k4_mpi_depth_split_stats(N.C.byref(gd), float(interval), float(thres), N.f32(out), N.stream()), 'k4_mpi_depth_split_stats')
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize('name', [c[0] for c in DSO.STATS_CASES])
def test_depth_split_stats_vs_fp64(name):
    """out16[0:8] == the fp32 quotients of the reference's integer counts, exactly: the kernel's sums are integers below 2^24 and the inputs keep
    every alpha and every running T clear of the two thresholds (asserted here on the reference; tests/test_depth_split_cpu.py)."""
    d, act, interval, thres = DSO.stats_case(name)
    ref = DSO.stats(d, act, interval, thres)
    assert ref['alpha_margin'] > 1e-3 and ref['T_margin'] > 1e-3
    want = DSO.expected(ref)
    got = _kernel_stats(d, act, interval, thres)
    print(name, 'kernel', got[:10].tolist(), 'reference', want.tolist())
    assert np.array_equal(got[:8], want), (got[:8].tolist(), want.tolist())
    if ref['columns'] == 0:
        assert not got.any()                                                            # all sixteen zero, no 0 / 0
    else:
        assert got[8] == np.float32(ref['voxels']) and got[9] == np.float32(ref['columns'])


def test_statistic_is_recomputed_when_the_density_changes():
    """The statistic's cache is keyed on the density tensor's version: an in-place edit (the wall and everything behind it removed) must be seen by
    the next call -- statistic, split and frame are those of a model loaded from the edited grid."""
    ck = scene.make_llff_checkpoint(seed=781, num_voxels=48 * 48 * 128, mpi_depth=128, opaque=True)
    rays = [r.cuda() for r in _checkpoint('blob', 'n128')[1]]
    rk = dict(ck['render_kwargs'], render_depth=True)
    model = utils.model_from_checkpoint_dict(ck).cuda().eval()
    _, s_before = _march(model, rays, rk, 0, W, real_rule=True)
    st_before = list(model._k4_cache()['dsplit_stats'])
    assert s_before == 64 and st_before[0] > 0.9
    version = model.density.grid._version
    model.density.grid[..., 30:] = -30.0
    assert model.density.grid._version > version
    got, s_after = _march(model, rays, rk, 0, W, real_rule=True)
    st_after = list(model._k4_cache()['dsplit_stats'])
    ck['model_state_dict']['density.grid'][..., 30:] = -30.0
    fresh = utils.model_from_checkpoint_dict(ck).cuda().eval()
    want, s_fresh = _march(fresh, rays, rk, 0, W, real_rule=True)
    print('before', s_before, [round(v, 4) for v in st_before], 'after', s_after, [round(v, 4) for v in st_after])
    assert st_after != st_before and st_after == list(fresh._k4_cache()['dsplit_stats'])
    assert s_after == s_fresh == 0 and st_after[0] < dmpigo.DEPTH_SPLIT_MIN_OPAQUE
    _assert_equal(got, want, 'after the edit')
