"""Generate ``tests/golden/tensorf_grid.npz`` and ``tests/golden/tensorf_march_{dvgo,mpi}.npz`` from the REFERENCE's own ``lib/grid.py`` /
``lib/dvgo.py`` / ``lib/dmpigo.py`` (TensoRFGrid, lib/grid.py:157-268).  TEST INFRASTRUCTURE ONLY.
Usage (build container, where the reference tree exists):  PYTHONDONTWRITEBYTECODE=1 python tests/gen_tensorf_golden.py

Tolerances are MEASURED: every case is evaluated twice, by the reference class in fp32 and by the same class ``.double()``.  The fp64 values are stored
as the expectation (``<key>``) and, per key, ``err32/<key>`` = max |fp32 reference - fp64 reference|.  Tests hold the HIP result to 4 * err32 per key
(another summation order over components and points, FMA contraction: the error family of the fp32 reference itself).  The rank-48 case stores its
expectations rounded to fp32 (file size) with ``rnd/<key>`` = the largest rounding distance, which the tests SUBTRACT from the tolerance.

March goldens: the native ops the reference calls (point sampling, Raw2Alpha, Alphas2Weights: oracle/native_cpu.py) compute in fp32 in both runs, so both
runs see the same sample points; grids, rgbnet and the ray sums run in fp64 in the second.  A seed is accepted only when both runs select identical samples
and no candidate's alpha or weight lies within 100 x the density lookup's err32 of fast_color_thres (recorded as ``margin/*``).
"""
import contextlib
import copy
import io
import json
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, HERE]

from oracle import ref_import, marcher         # noqa: E402
import nerf4k_amd                              # noqa: E402,F401
from nerf4k_amd import scene                   # noqa: E402

GOLDEN = os.path.join(HERE, 'golden')
FACTORS = ('xy_plane', 'xz_plane', 'yz_plane', 'x_vec', 'y_vec', 'z_vec')
TV_W = (0.3, 0.2, 0.1)
NEW_WORLD = [9, 8, 11]


def _save(name, arrs):
    path = os.path.join(GOLDEN, name + '.npz')
    np.savez_compressed(path, **arrs)
    print(f'{name}: {os.path.getsize(path) / 1024:.1f} KiB')
    assert os.path.getsize(path) < 1000 * 1024


def _quant(t, step):
    """Round to multiples of `step` (a power of two): exactly representable, and the file compresses."""
    return (t / step).round() * step


class Rec:
    """Collects expectation (fp64), err32 and, for fp32-stored cases, the rounding distance."""

    def __init__(self, arrs, prefix, store32=False):
        self.arrs, self.prefix, self.store32 = arrs, prefix, store32

    def put(self, key, v32, v64):
        v32, v64 = v32.detach().double().numpy(), v64.detach().double().numpy()
        err = float(np.abs(v32 - v64).max()) if v64.size else 0.0
        self.arrs[f'{self.prefix}/err32/{key}'] = np.array(err)
        if self.store32:
            st = v64.astype(np.float32)
            self.arrs[f'{self.prefix}/rnd/{key}'] = np.array(float(np.abs(st.astype(np.float64) - v64).max()) if v64.size else 0.0)
            self.arrs[f'{self.prefix}/{key}'] = st
        else:
            self.arrs[f'{self.prefix}/{key}'] = v64
        print(f'  {self.prefix}/{key}: err32 = {err:.3e}  (scale {float(np.abs(v64).max()) if v64.size else 0.0:.3e})')


def _both(g32, fn):
    """fn(grid) evaluated on the fp32 module and on a ``.double()`` copy -> (result32, result64); fn gets (module, dtype)."""
    g64 = copy.deepcopy(g32).double()
    return fn(g32, torch.float32), fn(g64, torch.float64)


def _lookup_and_grads(g, dt, pts, go):
    for p in g.parameters():
        p.grad = None
    out = g(pts.to(dt))
    out.backward(go.to(dt).reshape(out.shape))
    return [out.detach()] + [p.grad.detach().clone() for _, p in g.named_parameters()]


def grid_case(ref, arrs, name, channels, world, config, n_pts, seed, full=True, store32=False):
    print(name)
    gen = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    lo, hi = [-1.0, -0.5, 0.25], [1.5, 0.75, 2.0]
    g = ref.grid.TensoRFGrid(channels, torch.tensor(world), lo, hi, config)
    if store32:
        with torch.no_grad():
            for p in g.parameters():
                p.copy_(_quant(p, 2.0 ** -9))
    rec = Rec(arrs, name, store32)
    arrs[f'{name}/keys'] = np.array(json.dumps(list(g.state_dict().keys())))
    arrs[f'{name}/config'] = np.array(json.dumps(config))
    arrs[f'{name}/channels'] = np.array(channels)
    arrs[f'{name}/world'] = np.array(world)
    for k, v in g.state_dict().items():
        arrs[f'{name}/sd/{k}'] = v.numpy().copy()
    lo_t, hi_t = torch.tensor(lo), torch.tensor(hi)
    cen, half = (lo_t + hi_t) / 2, (hi_t - lo_t) / 2
    # over 1.3 x the box, plus the exact corners, mixed-face points and the centre
    pts = cen + half * 1.3 * (torch.rand([n_pts, 3], generator=gen) * 2 - 1)
    special = [lo_t, hi_t, cen, torch.stack([lo_t[0], hi_t[1], cen[2]]), torch.stack([hi_t[0], cen[1], lo_t[2]]), torch.stack([cen[0], lo_t[1], hi_t[2]]),
               torch.stack([lo_t[0], lo_t[1], hi_t[2]]), torch.stack([hi_t[0], lo_t[1], lo_t[2]])]
    pts[:len(special)] = torch.stack(special)
    sets = {'': pts}
    if full:
        # every point inside ONE cell: the same four plane corners and the same vector entries take every contribution
        vox = (hi_t - lo_t) / (torch.tensor(world).float() - 1)
        sets['cell_'] = lo_t + vox * (torch.tensor([2., 1., 5.]) + 0.02 + 0.96 * torch.rand([333, 3], generator=gen))
    names = [k for k, _ in g.named_parameters()]
    for tag, p in sets.items():
        go = _quant(torch.randn([p.shape[0], channels], generator=gen), 2.0 ** -6)
        arrs[f'{name}/{tag}pts'] = p.numpy().copy()
        arrs[f'{name}/{tag}go'] = go.numpy().copy()
        r32, r64 = _both(g, lambda m, dt: _lookup_and_grads(m, dt, p, go))
        rec.put(f'{tag}out', r32[0].reshape(p.shape[0], channels), r64[0].reshape(p.shape[0], channels))
        for k, a, b in zip(names, r32[1:], r64[1:]):
            rec.put(f'{tag}grad/{k}', a, b)
    if not full:
        return
    d32, d64 = _both(g, lambda m, dt: m.get_dense_grid().detach())
    rec.put('dense', d32, d64)
    # total variation on factors scaled so that differences land on both sides of |d| = 1
    gt = copy.deepcopy(g)
    with torch.no_grad():
        for k in FACTORS:
            getattr(gt, k).mul_(8.0)
    for k in FACTORS:
        arrs[f'{name}/tvsd/{k}'] = getattr(gt, k).detach().numpy().copy()
    big = max(float((getattr(gt, k)[:, :, 1:] - getattr(gt, k)[:, :, :-1]).abs().max()) for k in FACTORS)
    small = min(float((getattr(gt, k)[:, :, 1:] - getattr(gt, k)[:, :, :-1]).abs().min()) for k in FACTORS)
    assert big > 1 and small < 1

    def tv(m, dt):
        for p in m.parameters():
            p.grad = None
        m.total_variation_add_grad(*TV_W, True)
        return [getattr(m, k).grad.detach().clone() for k in FACTORS]
    t32, t64 = _both(gt, tv)
    for k, a, b in zip(FACTORS, t32, t64):
        rec.put(f'tv/{k}', a, b)

    def resize(m, dt):
        m.scale_volume_grid(NEW_WORLD)
        return [getattr(m, k).detach().clone() for k in FACTORS]
    s32, s64 = _both(g, resize)
    for k, a, b in zip(FACTORS, s32, s64):
        rec.put(f'scaled/{k}', a, b)


def gen_grid(ref):
    arrs = {}
    grid_case(ref, arrs, 'c1', 1, [7, 5, 9], {'n_comp': 5, 'n_comp_xy': 3}, 1037, seed=11)
    grid_case(ref, arrs, 'c9', 9, [7, 5, 9], {'n_comp': 5, 'n_comp_xy': 3}, 1037, seed=12)
    grid_case(ref, arrs, 'r48', 12, [20, 17, 33], {'n_comp': 48}, 4096, seed=13, full=False, store32=True)
    _save('tensorf_grid', arrs)


# ---------------------------------------------------------------------------------------------------------------- march goldens
def _kwargs_json(kw):
    return json.dumps({k: (v.tolist() if isinstance(v, np.ndarray) or torch.is_tensor(v) else v) for k, v in kw.items()})


def _np(v):
    v = v.detach().cpu()
    return (v.int() if v.dtype == torch.int64 else v).numpy()


def _ref_model(ref, cls, kw, seed):
    torch.manual_seed(seed)
    with contextlib.redirect_stdout(io.StringIO()):
        m = getattr(ref.dvgo if cls == 'DirectVoxGO' else ref.dmpigo, cls)(**kw)
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        # a scene instead of the initial noise: densities on both sides of the activation's knee, colours of order one
        def smooth(t):                                # [1,2,1]/4 along the two spatial axes, twice: a field whose lookup error stays near one ulp
            for _ in range(2):
                for d in (2, 3):
                    if t.shape[d] > 2:
                        t = torch.cat([t.narrow(d, 0, 1), (t.narrow(d, 0, t.shape[d] - 2) + 2 * t.narrow(d, 1, t.shape[d] - 2) + t.narrow(d, 2, t.shape[d] - 2)) / 4,
                                       t.narrow(d, t.shape[d] - 1, 1)], d)
            return t
        for k in FACTORS:
            getattr(m.density, k).copy_(smooth(torch.randn(getattr(m.density, k).shape, generator=gen)) * (2.6 if 'plane' in k else 2.4))
            getattr(m.k0, k).copy_(smooth(torch.randn(getattr(m.k0, k).shape, generator=gen)) * 1.5)
        std = float(m.density.get_dense_grid().std())   # raw densities of order one: the fp32 lookup's error scales with them
        for k in FACTORS[:3]:
            getattr(m.density, k).mul_(1.5 / std)
        # an occupancy that excludes half the box (few candidates: see the selection condition), so that the mask decides something
        mask = torch.ones_like(m.mask_cache.mask)
        mask[:, :, : mask.shape[2] // 2] = False
        m.mask_cache.mask.copy_(mask)
    return m


def _alpha2weight_any_dtype(alpha, ray_id, n_rays):
    """oracle/native_cpu.alpha2weight (render_utils_kernel.cu:591-603) with the running transmittance in alpha's dtype: the fp64 run's scan."""
    from oracle import native_cpu as nat
    n_rays = int(n_rays)
    weight, T = torch.zeros_like(alpha), torch.ones_like(alpha)
    i_start, i_end = nat._segments(ray_id, n_rays)
    if alpha.numel() == 0:
        return weight, T, torch.ones([n_rays], dtype=alpha.dtype), i_start, i_end
    seg_len = i_end - i_start
    Tc = torch.ones([n_rays], dtype=alpha.dtype)
    alive = seg_len > 0
    new_end = i_end.clone()
    for s in range(int(seg_len.max())):
        act = alive & (s < seg_len)
        idx = (i_start + s)[act]
        a = alpha[idx]
        T[idx] = Tc[act]
        weight[idx] = Tc[act] * a
        Tn = Tc[act] * (1. - a)
        Tc[act] = Tn
        stop = Tn < 1e-3
        rid = torch.nonzero(act).flatten()
        new_end[rid[stop]] = idx[stop] + 1
        alive[rid[stop]] = False
    return weight, T, Tc.clone(), i_start, new_end


def _run(mod, model, rays, rk, dt, train, dvgo_mod=None):
    """-> (outputs, gradients of rgb_marched.sum() w.r.t. the factor parameters | None, the selection candidates' (alpha, weight) margins)."""
    ro, rd, vd = (r.to(dt) for r in rays)
    seen = {}
    import types
    # record the candidates of the two threshold filters: alpha before mask2, weights before mask3
    act = model.activate_density

    def spy_act(density, interval=None):
        a = act(density, interval)
        seen['alpha'] = a.detach().double()
        return a
    model.activate_density = spy_act
    a2w = mod.Alphas2Weights

    class Spy:
        @staticmethod
        def apply(alpha, ray_id, n):
            w, last = a2w.apply(alpha, ray_id, n)
            seen['weight'] = w.detach().double()
            return w, last
    mod.Alphas2Weights = Spy
    nat = mod.render_utils_cuda
    if dt == torch.float64:
        import types
        def in_fp32(fn):                              # samplers and mask lookups: the fp32 run's own arithmetic, so both runs see the same points
            def call(*a):
                r = fn(*[x.float() if torch.is_tensor(x) and x.dtype == torch.float64 else x for x in a])
                return tuple(x.double() if torch.is_tensor(x) and x.dtype == torch.float32 else x for x in r) if isinstance(r, tuple) else \
                    (r.double() if torch.is_tensor(r) and r.dtype == torch.float32 else r)
            return call
        keep = ('raw2alpha', 'raw2alpha_backward', 'raw2alpha_nonuni', 'raw2alpha_nonuni_backward', 'alpha2weight_backward')
        mod.render_utils_cuda = types.SimpleNamespace(**{k: (getattr(nat, k) if k in keep else in_fp32(getattr(nat, k)))
                                                         for k in dir(nat) if not k.startswith('_') and callable(getattr(nat, k)) and not isinstance(getattr(nat, k), type)})
        mod.render_utils_cuda.alpha2weight = _alpha2weight_any_dtype
        if dvgo_mod is not None:                      # (lib/dmpigo.py takes Raw2Alpha / Alphas2Weights from lib/dvgo.py)
            dvgo_mod.render_utils_cuda = mod.render_utils_cuda
    torch.set_default_dtype(dt)                       # (the reference allocates its ray sums with torch.zeros of the default dtype)
    try:
        if train:
            for p in model.parameters():
                p.grad = None
            out = model(ro, rd, vd, global_step=0, **rk)
            out['rgb_marched'].sum().backward()
            grads = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None and any(f in k for f in FACTORS + ('f_vec',))}
        else:
            with torch.no_grad():
                out = model(ro, rd, vd, **rk)
            grads = None
    finally:
        mod.Alphas2Weights = a2w
        mod.render_utils_cuda = nat
        if dvgo_mod is not None:
            dvgo_mod.render_utils_cuda = nat
        torch.set_default_dtype(torch.float32)
        del model.activate_density
    thres = float(model.fast_color_thres)
    margin = min(float((seen['alpha'] - thres).abs().min()), float((seen['weight'] - thres).abs().min()))
    return {k: v.detach() for k, v in out.items() if torch.is_tensor(v)}, grads, margin


def march_case(ref, name, cls, kw, rk, rays):
    print(name)
    mod = ref.dvgo if cls == 'DirectVoxGO' else ref.dmpigo
    for seed in range(100, 400):
        m32 = _ref_model(ref, cls, kw, seed)
        m64 = copy.deepcopy(m32).double()
        # the density lookup's own err32 at the candidates (all in-box sample points)
        with torch.no_grad():
            probe = (m32.xyz_min + (m32.xyz_max - m32.xyz_min) * torch.rand([4096, 3], generator=torch.Generator().manual_seed(seed)))
            derr = float((m32.density(probe).double() - m64.density(probe.double())).abs().max())
        runs = {}
        ok = True
        for train in (False, True):
            o32, g32, mg32 = _run(mod, m32, rays, rk, torch.float32, train, ref.dvgo)
            o64, g64, mg64 = _run(mod, m64, rays, rk, torch.float64, train, ref.dvgo)
            same = o32['ray_id'].shape == o64['ray_id'].shape and bool((o32['ray_id'] == o64['ray_id']).all()) and \
                bool((o32['s'].double() - o64['s'].double()).abs().max() == 0 if 's' in o32 else True)
            margin = min(mg32, mg64)
            if os.environ.get('GEN_VERBOSE'):
                print(f'  seed {seed} train {train}: same {same} margin {margin:.3e} derr {derr:.3e} samples {o32["ray_id"].numel()} / {o64["ray_id"].numel()}')
            if not same or margin <= 100 * derr or o32['ray_id'].numel() < 2 * rays[0].shape[0]:
                ok = False
                break
            runs[train] = (o32, g32, o64, g64, margin)
        if ok:
            break
    assert ok, 'no seed met the selection condition'
    print(f'  seed {seed}: density err32 {derr:.3e}, selection margins eval {runs[False][4]:.3e} train {runs[True][4]:.3e}, samples {runs[False][0]["ray_id"].numel()}')
    arrs = {'model_class': np.array(cls), 'model_kwargs_json': np.array(_kwargs_json(m32.get_kwargs())), 'render_kwargs_json': np.array(json.dumps(rk)),
            'seed': np.array(seed), 'density_err32': np.array(derr), 'margin/eval': np.array(runs[False][4]), 'margin/train': np.array(runs[True][4])}
    for k, v in m32.state_dict().items():
        arrs['sd/' + k] = _np(v)
    for k, v in zip(('rays_o', 'rays_d', 'viewdirs'), rays):
        arrs['in/' + k] = _np(v)
    for train, tag in ((False, 'out'), (True, 'train')):
        o32, g32, o64, g64, _ = runs[train]
        rec = Rec(arrs, tag)
        for k in o64:
            if o64[k].dtype in (torch.int64, torch.int32, torch.bool):
                arrs[f'{tag}/{k}'] = _np(o64[k])
            else:
                rec.put(k, o32[k], o64[k])
        if g64 is not None:
            rec = Rec(arrs, 'grad')
            for k in g64:
                rec.put(k, g32[k], g64[k])
    _save(name, arrs)


def gen_march(ref, which=('dvgo', 'mpi')):
    tf = {'n_comp': 4}
    # DirectVoxGO: non-cubic box, an rgbnet the fused path accepts
    ck = scene.make_lego_checkpoint(seed=5, num_voxels=20 ** 3, rgbnet_dim=6, rgbnet_width=64, rgbnet_depth=3, viewbase_pe=2)
    kw = dict(ck['model_kwargs'], xyz_min=np.array([-1.5, -1.2, -1.0], dtype=np.float32), xyz_max=np.array([1.4, 1.3, 1.2], dtype=np.float32),
              density_type='TensoRFGrid', k0_type='TensoRFGrid', density_config=tf, k0_config=tf, mask_cache_world_size=[18, 17, 15], fast_color_thres=0.05, alpha_init=0.5)
    H, W = 20, 24
    ro, rd, vd = marcher.get_rays_of_a_view(H, W, scene.lego_K(H, W), torch.Tensor(scene.lego_pose()), ndc=False)
    sel = torch.randperm(H * W, generator=torch.Generator().manual_seed(1))[:200].sort().values
    rays = [x.reshape(-1, 3)[sel].contiguous() for x in (ro, rd, vd)]
    if 'dvgo' in which:
        march_case(ref, 'tensorf_march_dvgo', 'DirectVoxGO', kw, dict(ck['render_kwargs'], stepsize=2.0), rays)
    # DirectMPIGO
    ck = scene.make_llff_checkpoint(seed=6, num_voxels=24 * 24 * 16, mpi_depth=16, rgbnet_dim=6, rgbnet_width=64, rgbnet_depth=3, viewbase_pe=2)
    kw = dict(ck['model_kwargs'], density_type='TensoRFGrid', k0_type='TensoRFGrid', density_config=tf, k0_config=tf, fast_color_thres=0.05)
    K = scene.LLFF_K.copy()
    K[:2] *= W / scene.LLFF_HW[1]
    ro, rd, vd = marcher.get_rays_of_a_view(H, W, K, torch.Tensor(scene.llff_spiral_poses()[3]), ndc=True)
    rays = [x.reshape(-1, 3)[sel].contiguous() for x in (ro, rd, vd)]
    if 'mpi' in which:
        march_case(ref, 'tensorf_march_mpi', 'DirectMPIGO', kw, dict(ck['render_kwargs'], stepsize=2.0), rays)


if __name__ == '__main__':
    ref = ref_import.load_reference()
    what = sys.argv[1:] or ['grid', 'march']
    if 'grid' in what:
        gen_grid(ref)
    if 'march' in what:
        gen_march(ref)
    for w in ('dvgo', 'mpi'):
        if 'march_' + w in what:
            gen_march(ref, (w,))
