"""Generate ``tests/golden/grad_dvgo_direct.npz`` from the REFERENCE's own ``lib/dvgo.py``.  TEST INFRASTRUCTURE ONLY.
Usage (build container, where the reference tree exists):  PYTHONDONTWRITEBYTECODE=1 python tests/gen_direct_train_golden.py

The reference module is imported unmodified on the CPU through the stubs of ``oracle/ref_import.py``.  ``DirectVoxGO(rgbnet_dim=0)`` on a 12^3
seeded scene renders 20 x 20 rays under autograd; the loss lines of run_sr.py:523-547 (photo, last-transmittance entropy, per-sample colour)
give the terms and the gradients of ``density.grid`` and ``k0.grid``.  Besides them the file holds the sample lists the oracle of
tests/direct_train_oracle.py evaluates on: the shaded list (ray_id / step_id) and the alpha-passing list with the weight filter's decisions.

Condition on the inputs (asserted here): the reference, the fp32 restatement and the fp64 restatement (direct_train_oracle.sample_list) keep
the same lists, so no sample sits within rounding of a decision and a mismatch on the GPU is a defect, not a tie.  A seed that fails the
condition moves to the next seed.
"""
import contextlib
import io
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, HERE]

from oracle import ref_import                  # noqa: E402
import nerf4k_amd                              # noqa: E402,F401
from nerf4k_amd import scene                   # noqa: E402
import direct_train_oracle as dto              # noqa: E402

GOLDEN = os.path.join(HERE, 'golden')
WEIGHTS = dict(weight_main=1.0, weight_entropy_last=0.01, weight_rgbper=0.1)          # configs/default.py, coarse stage
HW = 20


def _np(v):
    v = v.detach().cpu()
    return (v.int() if v.dtype == torch.int64 else v).numpy()


def _kwargs_json(kw):
    return json.dumps({k: (v.tolist() if isinstance(v, np.ndarray) or torch.is_tensor(v) else v) for k, v in kw.items()})


def _reference_lists(ref, model, rays_o, rays_d, rk):
    """The reference's own stages (lib/dvgo.py:338-369) strung by hand, to read the lists forward does not return."""
    with torch.no_grad():
        ray_pts, ray_id, step_id, _, _ = model.sample_ray(rays_o=rays_o, rays_d=rays_d, **rk)
        m1 = model.mask_cache(ray_pts)
        ray_pts, ray_id, step_id = ray_pts[m1], ray_id[m1], step_id[m1]
        alpha = model.activate_density(model.density(ray_pts), rk['stepsize'] * model.voxel_size_ratio)
        m2 = alpha > model.fast_color_thres
        ray_id, step_id, alpha = ray_id[m2], step_id[m2], alpha[m2]
        weights, _ = ref.dvgo.Alphas2Weights.apply(alpha, ray_id, len(rays_o))
        shaded = weights > model.fast_color_thres
        live = weights > 0            # in front of and including the stop (alpha > thres > 0 there); the reference leaves weight 0 behind it
    return {'ray_id': ray_id[shaded], 'step_id': step_id[shaded], 'a_ray_id': ray_id[live], 'a_step_id': step_id[live], 'shaded': shaded[live]}


def _case(ref, seed):
    ck = scene.make_lego_checkpoint(seed=seed, num_voxels=12 ** 3, rgbnet_dim=0)
    rk = {k: ck['render_kwargs'][k] for k in ('near', 'far', 'bg', 'stepsize')}
    ro, rd, vd = ref.dvgo.get_rays_of_a_view(HW, HW, scene.lego_K(HW, HW), torch.Tensor(scene.lego_pose()), False,
                                             inverse_y=False, flip_x=False, flip_y=False)
    rays = [x.flatten(0, -2).contiguous() for x in (ro, rd, vd)]
    with contextlib.redirect_stdout(io.StringIO()):
        model = ref.dvgo.DirectVoxGO(**ck['model_kwargs'])
    model.load_state_dict(ck['model_state_dict'])
    target = torch.rand([rays[0].shape[0], 3], generator=torch.Generator().manual_seed(seed + 1))

    out = model(*rays, global_step=0, **rk)
    # run_sr.py:523-547
    loss = WEIGHTS['weight_main'] * F.mse_loss(out['rgb_marched'], target)
    photo = loss.detach().clone()
    pout = out['alphainv_last'].clamp(1e-6, 1 - 1e-6)
    entropy = WEIGHTS['weight_entropy_last'] * -(pout * torch.log(pout) + (1 - pout) * torch.log(1 - pout)).mean()
    loss = loss + entropy
    rgbper = (out['raw_rgb'] - target[out['ray_id']]).pow(2).sum(-1)
    rgbper = WEIGHTS['weight_rgbper'] * (rgbper * out['weights'].detach()).sum() / len(rays[0])
    loss = loss + rgbper
    loss.backward()

    lists = _reference_lists(ref, model, rays[0], rays[1], rk)
    assert torch.equal(lists['ray_id'], out['ray_id'])
    stepdist = float(rk['stepsize'] * model.voxel_size)
    interval = float(rk['stepsize'] * model.voxel_size_ratio)
    for dtype in (torch.float32, torch.float64):
        got = dto.sample_list(ck['model_state_dict'], model.fast_color_thres, rays[0], rays[1], rk['near'], stepdist, interval, dtype)
        if not all(torch.equal(got[k], lists[k]) for k in lists):
            return None
    arrs = {'model_class': np.array(ck['model_class']), 'model_kwargs_json': np.array(_kwargs_json(ck['model_kwargs'])),
            'render_kwargs_json': np.array(json.dumps(rk)), 'weights_json': np.array(json.dumps(WEIGHTS)), 'target': _np(target),
            'stepdist': np.array(stepdist), 'interval': np.array(interval)}
    for k, v in ck['model_state_dict'].items():
        arrs['sd/' + k] = _np(v)
    for k, v in zip(('rays_o', 'rays_d', 'viewdirs'), rays):
        arrs['in/' + k] = _np(v)
    for k, v in (('total', loss), ('photo', photo), ('entropy', entropy), ('rgbper', rgbper)):
        arrs['term/' + k] = np.array(float(v))
    arrs['out/rgb_marched'], arrs['out/alphainv_last'] = _np(out['rgb_marched']), _np(out['alphainv_last'])
    for k, v in lists.items():
        arrs['list/' + k] = _np(v)
    arrs['grad/density.grid'], arrs['grad/k0.grid'] = _np(model.density.grid.grad), _np(model.k0.grid.grad)
    print(f'grad_dvgo_direct: seed {seed}, {len(lists["ray_id"])} shaded of {len(lists["a_ray_id"])} alpha-passing samples, '
          f'longest ray {int(torch.bincount(lists["a_ray_id"]).max())}, total {float(loss):.6f}')
    return arrs


if __name__ == '__main__':
    if not ref_import.available():
        raise SystemExit('the reference tree is not present: nothing to generate')
    torch.manual_seed(0)
    ref = ref_import.load_reference()
    for seed in range(31, 1031, 100):
        arrs = _case(ref, seed)
        if arrs is not None:
            break
        print(f'grad_dvgo_direct: seed {seed} holds a tie between the restatements, next seed')
    else:
        raise SystemExit('grad_dvgo_direct: no seed without ties')
    path = os.path.join(GOLDEN, 'grad_dvgo_direct.npz')
    np.savez_compressed(path, **arrs)
    print(f'grad_dvgo_direct: {os.path.getsize(path) / 1024:.1f} KiB')
    assert os.path.getsize(path) < 200 * 1024
