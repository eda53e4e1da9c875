"""The tail of the geometry kernel's FAST instantiation -- transmittance scan and survivor append in ONE pass, survivors in the order
quarter / rank within the ray / ray slot, written to the quarter in front of the four raw runs -- against the general instantiation, whose tail
is the two-pass form (weights written back, then compacted in place: quarter / ray / depth).  K4_DEBUG=16384 forces the general path and is read
while the library loads, so each side is ONE child process (tools/geom_tail_hash.py, all cases in it) that prints one sha1 per case over rgb,
depth and alphainv of every march.  The shading kernel's per-ray sums are exact integer adds and a sample's MLP column does not depend on its lane
or batch: the hashes must be EQUAL.

Cases (48 x 48 x 256 grid, 256 planes at stepsize 1, one launch, occupancy summary: the FAST predicate; the tool asserts interval == 1 and
depth_split == 0 for each): full = every quarter of a bundle filled to capacity, 64 x 256 survivors (the largest write index the layout allows;
test_full_case_fills_every_quarter checks the 256 shaded samples per ray with the CPU oracle); stop = rays that reach T < 1e-3 mid-depth (the tool asserts some do);
ragged = ragged tiles and ray lists that are no multiple of 64; empty = bundles without a record (the tool asserts there are some and that
their outputs are alphainv * bg and 0); reuse = A, B, A, A, larger C, A in one workspace slot, every A torch.equal to the first (in the tool)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ['full', 'stop', 'ragged', 'empty', 'reuse']
CHILD_TIMEOUT_S = 300          # one child = five small scenes built on the host + a few dozen millisecond marches


def _hashes(debug):
    env = dict(os.environ, K4_DEBUG=str(debug))
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'geom_tail_hash.py')] + CASES, env=env, capture_output=True, text=True,
                         timeout=CHILD_TIMEOUT_S)
    assert out.returncode == 0, out.stdout[-1000:] + out.stderr[-3000:]
    lines = {l.split()[1]: l for l in out.stdout.splitlines() if l.startswith('GEOM_TAIL_HASH')}
    assert sorted(lines) == sorted(CASES), out.stdout[-2000:]
    return lines


@pytest.fixture(scope='module')
def both_paths():
    return {'general': _hashes(16384), 'fast': _hashes(0)}


@pytest.mark.parametrize('case', CASES)
def test_one_pass_tail_bit_identical(both_paths, case):
    general, fast = both_paths['general'][case], both_paths['fast'][case]
    print(general)
    print(fast)
    assert fast == general
    assert general.endswith('interval=1 depth_split=0'), general      # what the host predicate needs for FAST (launch_march)


def test_full_case_fills_every_quarter():
    """The premise of case `full`, from the CPU oracle: in the 16 x 16 pixels of one workgroup every ray has 255 or 256 of its 256 samples shaded
    and at least one 8 x 8 bundle has 256 on all 64 rays -- 64 x 64 survivors per quarter, the slice's capacity, so the append reaches the last
    record in front of each raw run.  Weights stay above fast_color_thres by a margin (T ends near 0.6, alpha ~ 2e-3: w >= 1.2e-3 against 7.8e-4)
    and the fused marcher's alphainv agrees with the oracle's on those rays."""
    import torch
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    sys.path.insert(0, ROOT)
    import geom_tail_hash as T
    from oracle import marcher
    with torch.no_grad():
        ck = T.full_checkpoint()
        H, W, pose = T.FULL_FRAME
        y0, y1, x0, x1 = T.FULL_BLOCK
        rays = T.rays_of(H, W, pose)
        blk = (torch.arange(y0, y1)[:, None] * W + torch.arange(x0, x1)[None, :]).reshape(-1).to(rays[0].device)
        sub = [r[blk].contiguous() for r in rays]
        ref = marcher.mpi_forward(ck['model_kwargs'], ck['model_state_dict'], *[r.cpu() for r in sub], **ck['render_kwargs'])
        per_ray = torch.bincount(ref['ray_id'], minlength=blk.numel()).view((y1 - y0) // 8, 8, (x1 - x0) // 8, 8)
        print('shaded samples per ray: min', int(per_ray.min()), 'max', int(per_ray.max()), 'per bundle min', per_ray.amin(dim=(1, 3)).tolist())
        assert int(per_ray.max()) == 256 and int(per_ray.min()) >= 255
        assert int((per_ray == 256).all(dim=3).all(dim=1).sum()) >= 1
        thres = float(ck['model_kwargs']['fast_color_thres'])
        print('smallest weight', float(ref['weights'].min()), 'threshold', thres)
        assert float(ref['weights'].min()) > 1.1e-3 > thres
        assert 0.55 < float(ref['alphainv_last'].min()) and float(ref['alphainv_last'].max()) < 0.65
        model, rk = T.model_of(ck)
        out = model(*sub, k4_img_w=0, **rk)
        # 256 factors (1 - alpha) of ~0.998 each: fp32 rounding and libm / ocml exp differences stay below 256 * 2^-23 * a few
        assert float((out['alphainv_last'].cpu() - ref['alphainv_last']).abs().max()) < 1e-4
