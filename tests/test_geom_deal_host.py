"""The index arithmetic of the geometry kernel's group deal (4k-nerf_amd/csrc/k4_geom_deal.h: wave of (ray, group), group of (wave, ray, slot),
segment base, depth order of a ray's four segments), checked on the host for every sample count 1..256 by tests/geom_deal_check.cpp: bijection,
segment capacity, depth-ascending tail order and the append bound of the kernel's hazard argument.  Built with the host compiler, with the
address and undefined-behaviour sanitizers where the compiler has them; no GPU."""
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


def test_deal_index_arithmetic(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip('no host C++ compiler')
    src = os.path.join(ROOT, 'tests', 'geom_deal_check.cpp')
    base = [cxx, '-std=c++17', '-O1', '-g', '-Wall', '-Werror', '-I' + os.path.join(ROOT, '4k-nerf_amd', 'csrc'), src]
    exe = str(tmp_path / 'geom_deal_check')
    built = subprocess.run(base + ['-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-o', exe], capture_output=True, text=True)
    if built.returncode != 0:                                   # a compiler without the sanitizer runtimes: the plain program checks the same
        built = subprocess.run(base + ['-o', exe], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(run.stdout[-2000:])
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert 'sample counts 1..256 ok' in run.stdout
