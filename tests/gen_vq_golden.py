"""Generate ``tests/golden/{vq_grid,march_dvqgo_*,grad_dvqgo}.npz`` from the REFERENCE's own ``lib/grid.py`` (VQGrid) and ``lib/dvqgo.py``.
TEST INFRASTRUCTURE ONLY.  Usage (build container, where the reference tree exists):  PYTHONDONTWRITEBYTECODE=1 python tests/gen_vq_golden.py

The reference modules are imported unmodified on the CPU through the stubs of ``oracle/ref_import.py`` (the JIT ``load`` of render_utils_cuda ->
oracle/native_cpu.py), by an import of this file's own because ``ref_import.load_reference`` does not import ``lib.dvqgo``.

Conditions on the inputs, asserted here, so that a differing index on the GPU is a defect and no test has to exclude samples:
  * ties: every vector that reaches a codebook has a gap between its best and second-best ``dist`` above ``tau = 1e-5 * max|dist|`` of the case (about 40
    times the rounding bound ``(dim + 2) * 2^-24 * max|dist|`` of an fp32 dot product at dim <= 12).  A model case or a training sequence whose seed fails
    moves to the next seed; the bare-grid fixtures draw more points than they need and keep the first ``n`` that pass;
  * sample lists: the reference and the fp32 restatement (tests/vq_oracle.py, on the marcher pieces of oracle/ -- the source-rounded native kernels of
    oracle/native_cpu.py, which the reference's own modules run on here as well) give identical ``ray_id`` / ``step_id`` lists.
The moving-average sums depend on the summation order: per training call the fixture stores the spread between the reference's fp32 buffers and the
same update carried out in fp64 (``spread/...``); the tests allow 4 times that.
"""
import contextlib
import copy
import importlib
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
import vq_oracle as vo                         # noqa: E402

GOLDEN = os.path.join(HERE, 'golden')
TAU_REL = 1e-5


def load_reference():
    cpp_ext, real_load = ref_import._install_stubs()
    saved_path = list(sys.path)
    saved_lib = {k: v for k, v in sys.modules.items() if k == 'lib' or k.startswith('lib.')}
    for k in saved_lib:
        del sys.modules[k]
    sys.path.insert(0, ref_import.REFERENCE_ROOT)
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            dvqgo = importlib.import_module('lib.dvqgo')
            rgrid = importlib.import_module('lib.grid')
    finally:
        cpp_ext.load = real_load
        sys.path[:] = saved_path
        for k in [k for k in sys.modules if k == 'lib' or k.startswith('lib.')]:
            del sys.modules[k]
        sys.modules.update(saved_lib)
    return dvqgo, rgrid


def _np(v):
    if torch.is_tensor(v):
        v = v.detach().cpu()
        if v.dtype == torch.int64:
            v = v.int()
        return v.numpy()
    return np.asarray(v)


def _kwargs_json(kw):
    return json.dumps({k: (v.tolist() if isinstance(v, np.ndarray) or torch.is_tensor(v) else v) for k, v in kw.items()})


def _save(name, arrs):
    path = os.path.join(GOLDEN, name + '.npz')
    np.savez_compressed(path, **arrs)
    print(f'{name}: {os.path.getsize(path) / 1024:.1f} KiB')
    assert os.path.getsize(path) < 1000 * 1024


def _gaps(st, v):
    """(gap between the best and the second-best dist per vector, tau of the case)."""
    dist = vo.vq_dist(st, v.reshape(-1, v.shape[-1]))
    tau = TAU_REL * float(dist.abs().max()) if dist.numel() else 0.0
    if dist.shape[1] < 2:
        return torch.full([dist.shape[0]], float('inf')), tau
    top = (-dist).topk(2, dim=1).values
    return top[:, 0] - top[:, 1], tau


def _f16(t):
    """Values an fp16 holds exactly (stored as fp16: half the bytes)."""
    return t.half().float()


# ------------------------------------------------------------------------------------------------------------------ the bare grid
GRID_CASES = {          # name: (in_dim, dim, n_embed, n_points, train)
    'base': (15, 6, 64, 1000, True),
    'one': (3, 1, 1, 65, True),
    'odd': (27, 12, 1000, 4097, False),
    'chunked': (15, 32, 2500, 300, False),
}


def _ref_grid(rgrid, in_dim, dim, n_embed, g):
    vq = rgrid.VQGrid(input_dim=in_dim, channels=dim, world_size=n_embed, xyz_min=[-1, -1, -1], xyz_max=[1, 1, 1])
    with torch.no_grad():
        vq.embed.copy_(_f16(torch.randn([dim, n_embed], generator=g)))
        vq.cluster_size.copy_(torch.rand([n_embed], generator=g) * 10 + 1)
        vq.embed_avg.copy_(vq.embed * vq.cluster_size)
        for l in (vq.project_layer[0], vq.project_layer[2]):
            w, b = scene._linear_init(g, l.out_features, l.in_features)
            l.weight.copy_(w * 4.0)
            l.bias.copy_(b)
    return vq


def _train_calls(vq, x):
    """Two training calls on x and one on an empty input -> per call the outputs, the buffers and their spread against an fp64 update; None on a tie."""
    vq = copy.deepcopy(vq).train()
    vq64 = copy.deepcopy(vq).double()
    calls = []
    for xi in (x, x, x[:0]):
        st = vo.vq_state(vq.state_dict())
        with torch.no_grad():
            gap, tau = _gaps(st, vo.vq_project(st, xi))
            if xi.numel() and not bool((gap > tau).all()):
                return None
            q, diff, ind = vq(xi)
            q64, _, ind64 = vq64(xi.double())
        assert torch.equal(ind, ind64)
        # the restatement in training mode gives the reference's values
        q2, d2, i2 = vo.vq_forward(st, xi, training=True)
        assert torch.equal(i2, ind) and torch.equal(q2, q) and (torch.equal(d2, diff) or xi.numel() == 0)
        bufs = {k: getattr(vq, k).clone() for k in ('cluster_size', 'embed_avg', 'embed')}
        for k in bufs:
            assert torch.equal(st[k], bufs[k]), k
        spread = {k: float((bufs[k].double() - getattr(vq64, k)).abs().max()) for k in bufs}
        calls.append(dict(q=q, diff=diff, ind=ind, bufs=bufs, spread=spread))
    return calls


def gen_grid(rgrid):
    arrs = {}
    for ci, (name, (in_dim, dim, n_embed, n, train)) in enumerate(GRID_CASES.items()):
        for seed in range(500 + ci, 500 + ci + 2000, 50):
            g = torch.Generator().manual_seed(seed)
            vq = _ref_grid(rgrid, in_dim, dim, n_embed, g).eval()
            st = vo.vq_state(vq.state_dict())
            cand = _f16(torch.rand([2 * n + 64, in_dim], generator=g) * 2 - 1)
            gap, tau = _gaps(st, vo.vq_project(st, cand))
            keep = (gap > tau).nonzero().squeeze(1)
            assert keep.numel() >= n, (name, int(keep.numel()))
            print(f'{name}: seed {seed}, {int((gap <= tau).sum())} of {cand.shape[0]} candidate points within tau = {tau:.3e} dropped, '
                  f'smallest kept gap {float(gap[keep[:n]].min()):.3e}')
            x = cand[keep[:n]].contiguous()
            calls = _train_calls(vq, x) if train else []
            if calls is not None:
                break
            print(f'{name}: seed {seed} holds a tie in its second training call, next seed')
        else:
            raise SystemExit(f'{name}: no seed without ties')
        with torch.no_grad():
            q, diff, ind = vq(x)
            v = vq.project_layer(x)
        aux = {}
        q2, d2, i2 = vo.vq_forward(st, x, aux=aux)
        assert torch.equal(i2, ind) and torch.equal(q2, q) and torch.equal(d2, diff) and torch.equal(aux['v'], v)
        assert torch.equal(q, v + (vq.embed.t()[ind] - v))
        p = name + '/'
        arrs[p + 'shape'] = np.array([in_dim, dim, n_embed, n])
        arrs[p + 'x'] = _np(x.half())
        for k, t in vq.state_dict().items():
            if k in ('xyz_min', 'xyz_max') or (k == 'embed_avg' and not train):
                continue
            arrs[p + 'sd/' + k] = _np(t.half()) if k == 'embed' else _np(t)
        arrs[p + 'v'], arrs[p + 'ind'], arrs[p + 'diff'] = _np(v), _np(ind).astype(np.int16), _np(diff)
        arrs[p + 'used_codes'] = np.array(int(ind.unique().numel()))
        for i, c in enumerate(calls):
            t = f'{p}train{i + 1}/'
            arrs[t + 'ind'], arrs[t + 'diff'] = _np(c['ind']).astype(np.int16), _np(c['diff'])
            for k in c['bufs']:
                arrs[t + k], arrs[t + 'spread/' + k] = _np(c['bufs'][k]), np.array(c['spread'][k])
            print(f'{name}: training call {i + 1}: spread ' + ', '.join(f'{k} {v:.2e}' for k, v in c['spread'].items()))
        print(f'{name}: {int(arrs[p + "used_codes"])} of {n_embed} codes used')
    _save('vq_grid', arrs)


# ------------------------------------------------------------------------------------------------------------------ the model
def _rays(n_view, seed):
    """n_view rays of an LLFF view plus 7 made by hand in NDC: three that miss the box altogether, four that leave it part of the way."""
    H, W = 24, 32
    K = scene.LLFF_K.copy()
    K[:2] *= W / scene.LLFF_HW[1]
    ro, rd, vd = marcher.get_rays_of_a_view(H, W, K, scene.llff_spiral_poses()[3], ndc=True)
    sel = torch.randperm(H * W, generator=torch.Generator().manual_seed(seed))[:n_view].sort().values
    ro, rd, vd = ro.reshape(-1, 3)[sel], rd.reshape(-1, 3)[sel], vd.reshape(-1, 3)[sel]
    eo = torch.tensor([[2.0, 0.3, -1], [-1.9, -1.8, -1], [0.2, 1.7, -1], [1.1, 0.2, -1], [-0.9, 0.7, -1], [0.4, -0.8, -1], [-1.25, -1.05, -1]])
    ed = torch.tensor([[0.1, 0.0, 2], [0.0, 0.1, 2], [0.05, 0.3, 2], [0.6, 0.1, 2], [-0.9, 0.2, 2], [0.3, -0.7, 2], [0.3, 0.25, 2]])
    ro, rd = torch.cat([ro, eo]).contiguous(), torch.cat([rd, ed]).contiguous()
    vd = torch.cat([vd, ed / ed.norm(dim=-1, keepdim=True)]).contiguous()
    return [ro, rd, vd]


def _ref_model(ref, ck):
    with contextlib.redirect_stdout(io.StringIO()):
        model = ref.DirectQVGO(**ck['model_kwargs'])
    model.load_state_dict(ck['model_state_dict'])
    return model


def _common(ck, rk):
    arrs = {'model_class': np.array(ck['model_class']), 'model_kwargs_json': np.array(_kwargs_json(ck['model_kwargs'])),
            'render_kwargs_json': np.array(json.dumps(rk))}
    for k, v in ck['model_state_dict'].items():
        arrs['sd/' + k] = _np(v)
    return arrs


MARCH_CASES = {
    'march_dvqgo_base': dict(seed=91, num_voxels=24 * 24 * 16, mpi_depth=16, stepsize=1.0, rgbnet_dim=6, n_cluster=64, rgbnet_width=32, rgbnet_depth=3,
                             spatial_pe=2),
    'march_dvqgo_half': dict(seed=92, num_voxels=24 * 24 * 16, mpi_depth=16, stepsize=0.5, rgbnet_dim=6, n_cluster=64, rgbnet_width=32, rgbnet_depth=3,
                             spatial_pe=2),
    # 80 samples per ray: two 64-lane chunks; an opaque wall at 0.4 of the depth range, so the T < 1e-3 stop falls mid-ray
    'march_dvqgo_deep_opaque': dict(seed=93, num_voxels=20 * 20 * 80, mpi_depth=80, stepsize=1.0, rgbnet_dim=6, n_cluster=64, rgbnet_width=32,
                                    rgbnet_depth=3, spatial_pe=2, opaque=True),
    'march_dvqgo_w64_d2': dict(seed=94, num_voxels=24 * 24 * 16, mpi_depth=16, stepsize=1.0, rgbnet_dim=9, n_cluster=300, rgbnet_width=64,
                               rgbnet_depth=2, spatial_pe=0),
}


def _checked_forward(ref, ck, rk, rays, train=False):
    """The reference's forward (eval), the restatement's, and the two conditions -> (reference model, its dict, the restatement's aux) or None."""
    model = _ref_model(ref, ck).eval()
    with torch.no_grad():
        out = model(*rays, **rk)
    aux = {}
    mine = vo.forward(ck['model_kwargs'], ck['model_state_dict'], *rays, aux=aux, **rk)
    if not torch.equal(mine['ray_id'], out['ray_id']) or not torch.equal(mine['s'], out['s']):
        return None
    gap, tau = _gaps(vo.vq_state(ck['model_state_dict'], 'k0.'), aux['v'])
    if not bool((gap > tau).all()):
        return None
    for k in out:                                   # the restatement computes the reference's values
        if torch.is_tensor(out[k]):
            assert torch.allclose(mine[k].float(), out[k].float(), rtol=0, atol=1e-6), (k, float((mine[k] - out[k]).abs().max()))
    return model, out, aux


def gen_march(ref):
    for i, (name, cfg) in enumerate(MARCH_CASES.items()):
        for seed in range(cfg['seed'], cfg['seed'] + 2000, 100):
            ck = scene.make_vq_checkpoint(**dict(cfg, seed=seed))
            rk = dict(ck['render_kwargs'], bg=(1 if i % 2 == 0 else 0))
            rays = _rays(60, seed)
            hit = _checked_forward(ref, ck, rk, rays)
            if hit is not None:
                break
            print(f'{name}: seed {seed} holds a tie, next seed')
        else:
            raise SystemExit(f'{name}: no seed without ties')
        _, out, aux = hit
        arrs = _common(ck, rk)
        for k, v in zip(('rays_o', 'rays_d', 'viewdirs'), rays):
            arrs['in/' + k] = _np(v)
        for k, v in out.items():
            arrs['out/' + k] = _np(v)
        arrs['aux/step_id'], arrs['aux/embed_ind'] = _np(aux['step_id']), _np(aux['embed_ind'])
        per_ray = torch.bincount(out['ray_id'], minlength=len(rays[0]))
        print(f'{name}: seed {seed}, {len(rays[0])} rays, {int(out["ray_id"].numel())} shaded samples (most on a ray: {int(per_ray.max())}, rays without: '
              f'{int((per_ray == 0).sum())}), {int(aux["embed_ind"].unique().numel())} codes used, mean alphainv_last {float(out["alphainv_last"].mean()):.3f}, '
              f'last shaded step {int(aux["step_id"].max())} of {out["n_max"]}')
        _save(name, arrs)


def gen_grad(ref):
    cfg = dict(num_voxels=24 * 24 * 16, mpi_depth=16, stepsize=1.0, rgbnet_dim=6, n_cluster=64, rgbnet_width=32, rgbnet_depth=3, spatial_pe=2)
    for seed in range(95, 2095, 100):
        ck = scene.make_vq_checkpoint(**dict(cfg, seed=seed))
        rk = dict(ck['render_kwargs'], bg=1)
        rays = _rays(60, seed)
        hit = _checked_forward(ref, ck, rk, rays)
        if hit is not None:
            break
    else:
        raise SystemExit('grad_dvqgo: no seed without ties')
    model = hit[0]
    out = model(*rays, global_step=0, **rk)
    g = torch.Generator().manual_seed(7)
    cot = {k: torch.randn(out[k].shape, generator=g) for k in ('rgb_marched', 'alphainv_last', 'weights', 'raw_rgb')}
    loss = sum((out[k] * cot[k]).sum() for k in cot)
    loss.backward()
    arrs = _common(ck, rk)
    for k, v in zip(('rays_o', 'rays_d', 'viewdirs'), rays):
        arrs['in/' + k] = _np(v)
    for k, v in cot.items():
        arrs['cot/' + k] = _np(v)
    arrs['loss'] = np.array(float(loss))
    arrs['out/ray_id'] = _np(out['ray_id'])
    for k, p in model.named_parameters():
        if p.grad is not None:
            arrs['grad/' + k] = _np(p.grad)
    assert {'density.grid', 'k0.project_layer.0.weight', 'k0.project_layer.2.bias', 'rgbnet.0.weight'} <= {k[5:] for k in arrs if k.startswith('grad/')}
    print(f'grad_dvqgo: seed {seed}, loss {float(loss):.6f}, ' + ', '.join(f'{k[5:]} {float(np.abs(v).max()):.2e}' for k, v in arrs.items() if k.startswith('grad/')))
    _save('grad_dvqgo', arrs)


if __name__ == '__main__':
    if not ref_import.available():
        raise SystemExit('the reference tree is not present: nothing to generate')
    torch.manual_seed(0)
    ref_dvqgo, ref_grid = load_reference()
    gen_grid(ref_grid)
    gen_march(ref_dvqgo)
    gen_grad(ref_dvqgo)
