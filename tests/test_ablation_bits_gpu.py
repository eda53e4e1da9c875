"""The product library cannot be made to compute a wrong frame from its environment: the ablation bits of K4_DEBUG / K4_SR_DEBUG (profiling
switches with WRONG results) exist only in a -DK4_ABLATE build (4k-nerf_amd/csrc/k4_env.h); the default build ignores them, says so once on
stderr while it loads, and still honours the exact selectors that share the two variables.  The library reads its environment at load, so each
side is a child process (tools/geom_hash.py, tools/sr_hash.py) that prints one sha1 per case.

Marcher: the adversarial-threshold scene at 60 x 80 rays on 40 planes (general geometry path) and on 256 planes (FAST), both shaded through the
rgbnet -- the smallest cases that reach both geometry instantiations.  K4_DEBUG=12979 is every ablation bit; 29363 adds the exact selector 16384.
Decoder: SFTNet x4, one block, 32 x 40 input with a condition image, in the f16x3p (p16 kernels) and bf16x6 (3x3 kernel) arithmetics.
K4_SR_DEBUG=991 is every ablation bit.  That these bits do change the hashes at these sizes where they are compiled in is recorded in
profiles/ablate_build.md (parent library, -DK4_ABLATE library)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT_S = 240          # per child: imports and the scene construction on the host dominate, the kernels are milliseconds
MARCH_ABLATE = 1 | 2 | 16 | 32 | 128 | 512 | 4096 | 8192           # 12979
SR_ABLATE = 1 | 2 | 4 | 8 | 16 | 64 | 128 | 256 | 512              # 991


def _child(tool, args, prefix, **env):
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', tool)] + args, env=dict(os.environ, **{k: str(v) for k, v in env.items()}),
                         capture_output=True, text=True, timeout=CHILD_TIMEOUT_S)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith(prefix)]
    assert lines, out.stdout[-2000:]
    return lines, out.stderr


def _ignored(stderr):
    return [l for l in stderr.splitlines() if 'ignored' in l and 'no ablations' in l]


@pytest.mark.parametrize('case', ['threshold', 'threshold256'])
@pytest.mark.parametrize('selector', [0, 16384])
def test_marcher_ignores_ablation_bits(case, selector):
    assert MARCH_ABLATE == 12979 and MARCH_ABLATE + 16384 == 29363
    ablated, err_a = _child('geom_hash.py', [case], 'GEOM_HASH', K4_DEBUG=MARCH_ABLATE | selector, K4_SR_DEBUG=0)
    clean, err_c = _child('geom_hash.py', [case], 'GEOM_HASH', K4_DEBUG=selector, K4_SR_DEBUG=0)
    print(ablated[-1])
    print(clean[-1])
    assert ablated[-1] == clean[-1]
    assert len(_ignored(err_a)) == 1 and str(MARCH_ABLATE) in _ignored(err_a)[0], err_a[-2000:]
    assert not _ignored(err_c), err_c[-2000:]


def test_decoder_ignores_ablation_bits():
    assert SR_ABLATE == 991
    ablated, err_a = _child('sr_hash.py', [], 'SR_HASH', K4_SR_DEBUG=SR_ABLATE, K4_DEBUG=0)
    clean, err_c = _child('sr_hash.py', [], 'SR_HASH', K4_SR_DEBUG=0, K4_DEBUG=0)
    print('\n'.join(ablated + clean))
    assert [l.split()[1] for l in clean] == ['f16x3p', 'bf16x6']
    assert ablated == clean
    assert len(_ignored(err_a)) == 1 and str(SR_ABLATE) in _ignored(err_a)[0], err_a[-2000:]
    assert not _ignored(err_c), err_c[-2000:]
