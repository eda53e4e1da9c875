"""The split of K4_DEBUG / K4_SR_DEBUG into exact selectors and ablation masks (4k-nerf_amd/csrc/k4_env.h), checked on the host by
tests/env_split_check.cpp for every single bit 0..15 of both variables and for all-ones: the product build (no -DK4_ABLATE) keeps both ablation
masks at 0 whatever it is given, an ablation build keeps exactly the wrong-result bits, and both honour every exact selector.  The header
includes nothing from HIP: the plain host compiler builds it, with the address and undefined-behaviour sanitizers where it has them; no GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compiler():
    for c in (os.environ.get('CXX'), 'g++', 'c++', 'clang++'):
        if c and shutil.which(c):
            return shutil.which(c)
    return None


@pytest.mark.parametrize('ablate', [False, True], ids=['product', 'ablation'])
def test_env_split(tmp_path, ablate):
    cxx = _compiler()
    if cxx is None:
        pytest.skip('no host C++ compiler')
    src = os.path.join(ROOT, 'tests', 'env_split_check.cpp')
    base = [cxx, '-std=c++17', '-O1', '-g', '-Wall', '-Werror', '-I' + os.path.join(ROOT, '4k-nerf_amd', 'csrc'), src] + (['-DK4_ABLATE'] if ablate else [])
    exe = str(tmp_path / 'env_split_check')
    built = subprocess.run(base + ['-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-o', exe], capture_output=True, text=True)
    if built.returncode != 0:                                   # a compiler without the sanitizer runtimes: the plain program checks the same
        built = subprocess.run(base + ['-o', exe], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-3000:]
    # the program's own environment carries every bit: the header's load-time initialiser runs in it too and must not disturb the pure function
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=dict(os.environ, K4_DEBUG='65535', K4_SR_DEBUG='65535'))
    print(run.stdout[-2000:], run.stderr[-500:])
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert ('env split ok (%s build)' % ('ablation' if ablate else 'product')) in run.stdout
    # the load-time line: the product build names what it ignored, an ablation build has nothing to ignore
    assert ('ignored' in run.stderr) == (not ablate), run.stderr
    if not ablate:
        assert 'K4_DEBUG & 12979' in run.stderr and 'K4_SR_DEBUG & 991' in run.stderr and 'no ablations' in run.stderr
