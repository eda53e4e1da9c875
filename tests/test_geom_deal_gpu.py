"""The deal of the geometry kernel's FAST instantiation -- group G of ray slot r goes to wave (G + (r >> 4)) & 3, a depth quarter's raw records lie
in four per-wave segments, the tail walks a ray's four pieces in depth order (4k-nerf_amd/csrc/k4_geom_deal.h) -- against the general
instantiation, which keeps one depth quarter per wave.  K4_DEBUG=16384 forces the general path and is read while the library loads, so each side
is ONE child process (tools/geom_deal_hash.py, all cases in it) that prints one sha1 per case over rgb, depth and alphainv of every march.  Per
ray the scan sees the same alphas in the same depth order and the shading kernel's per-ray sums are exact integer adds: the hashes must be EQUAL.

Cases (48 x 48 x N grid; the tool asserts interval == 1, depth_split == 0 and each case's premise): sheet16 = content in planes 96..111 only, one
group: four segments of one quarter, three empty quarters; straddle = a slab over planes 56..72 that stops rays inside a segment; n250 = a last
group of 10 samples; n40 = groups 0..2 only, so one wave per 16-ray subset has no group; ragged = ragged tiles and ray lists that are no multiple
of 64.  sheet16 is also compared with the CPU oracle at the tolerance of tests/test_march_gpu.py's golden frames (5e-6 absolute)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ['sheet16', 'straddle', 'n250', 'n40', 'ragged']
CHILD_TIMEOUT_S = 300          # one child = five small scenes built on the host + a dozen millisecond marches


def _hashes(debug):
    env = dict(os.environ, K4_DEBUG=str(debug))
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'geom_deal_hash.py')] + CASES, env=env, capture_output=True, text=True,
                         timeout=CHILD_TIMEOUT_S)
    assert out.returncode == 0, out.stdout[-1000:] + out.stderr[-3000:]
    lines = {l.split()[1]: l for l in out.stdout.splitlines() if l.startswith('GEOM_DEAL_HASH')}
    assert sorted(lines) == sorted(CASES), out.stdout[-2000:]
    return lines


@pytest.fixture(scope='module')
def both_paths():
    return {'general': _hashes(16384), 'fast': _hashes(0)}


@pytest.mark.parametrize('case', CASES)
def test_deal_bit_identical(both_paths, case):
    general, fast = both_paths['general'][case], both_paths['fast'][case]
    print(general)
    print(fast)
    assert fast == general
    assert ' interval=1 depth_split=0 ' in general, general           # what the host predicate needs for FAST (launch_march)


def test_sheet16_against_cpu_oracle():
    """sheet16 on the CPU oracle: its premise (every shaded step in planes 96..111) and the fused frame at the golden frames' tolerance."""
    import torch
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    sys.path.insert(0, ROOT)
    import geom_deal_hash as T
    from oracle import marcher
    with torch.no_grad():
        ck = T.sheet_checkpoint()
        H, W, pose = T.SHEET_FRAME
        dev = torch.device('cuda', 0)
        ref = marcher.mpi_forward(ck['model_kwargs'], ck['model_state_dict'], *T.rays_of(H, W, pose, torch.device('cpu')), **dict(ck['render_kwargs'], render_depth=True))
        step = torch.round(ref['s'] * ref['n_max'] - 0.5).long()       # the case's premise: every shaded step lies in the sheet's 16 planes
        print('shaded samples', step.numel(), 'steps', int(step.min()), '..', int(step.max()))
        assert step.numel() > 64 * 64 and int(step.min()) >= T.SHEET[0] and int(step.max()) < T.SHEET[1]
        model, rk = T.model_of(ck, dev)
        out = model(*T.rays_of(H, W, pose, dev), k4_img_w=W, **rk)
        for k in T.KEYS:
            d = float((out[k].cpu() - ref[k]).abs().max())
            print(k, 'max abs difference', d)
            assert d <= 5e-6, (k, d)
