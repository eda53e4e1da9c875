"""The geometry kernel's FAST instantiation (k4_geom3_kernel<MPI, false, .., true>: the LLFF configuration fixed at compile time -- interval 1,
threshold on, one launch, occupancy summary, step positions from the table, no ablation bits) against its general path.  K4_DEBUG=16384 forces
the general path and is read while the library loads, so each side runs in its own process (tools/geom_hash.py) and prints one sha1 over rgb,
depth and alphainv of every march of the case.  The FAST path only drops code its conditions make dead: the hashes must be EQUAL.

Cases: the bench scene at full size and at bench.py --small's size; on the bench scene again (256 samples, single launch) a linear ray list
whose length is not a multiple of 64, and a row band and a tile window with ragged 8 x 8 tiles; the adversarial scene of the live-mask tests (every voxel at the alpha == threshold bound; 40 planes, interval 6.4: general path on both sides) and the same construction on 256 planes (FAST); the opaque-wall
scene, where the depth split is chosen and both runs take the general path; stepsize 0.5, where interval != 1 does."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT_S = 420          # per child: scene construction on the host dominates (the full-size scenes take tens of seconds), the marches are milliseconds


def _hash(case, debug):
    env = dict(os.environ, K4_DEBUG=str(debug))
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'geom_hash.py'), case], env=env, capture_output=True, text=True,
                         timeout=CHILD_TIMEOUT_S)
    assert out.returncode == 0, out.stderr[-2000:]
    return [l for l in out.stdout.splitlines() if l.startswith('GEOM_HASH')][-1]


@pytest.mark.parametrize('case', ['bench', 'small', 'linear', 'windows', 'threshold', 'threshold256', 'opaque', 'halfstep'])
def test_fast_geometry_path_bit_identical(case):
    general = _hash(case, 16384)
    fast = _hash(case, 0)
    print(general)
    print(fast)
    assert fast == general
    split = int(general.rsplit('depth_split=', 1)[1])
    interval = float(general.rsplit('interval=', 1)[1].split()[0])
    # what the host predicate sees (launch_march): FAST needs interval == 1 (256 planes at stepsize 1) and a single launch.  bench, linear,
    # windows and threshold256 must be such shapes -- the comparison is then FAST against general (the kernel names per case are in
    # profiles/geom_fast_path.md); small (64 planes), threshold (40 planes) and halfstep have interval != 1 and opaque is split: both runs
    # take the general path and must still agree.
    if case in ('bench', 'linear', 'windows', 'threshold256'):
        assert interval == 1.0 and split == 0, (interval, split)
    elif case == 'opaque':
        assert split > 0
    else:
        assert interval != 1.0, interval
