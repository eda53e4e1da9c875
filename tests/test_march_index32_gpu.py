"""The cheaper instruction forms of the geometry kernel's FAST instantiation -- every array addressed as a uniform base + a 32-bit byte offset, the
tail's prefix scans and the prologue's maximum through DPP (4k-nerf_amd/csrc/k4_march.hip: K4_IDX_OFF32, K4_IDX_DPP) -- against the general
instantiations, which keep the 64-bit addresses and the __shfl_up scans.
K4_DEBUG=17408 (16384 | 1024) forces the general path of both kernels and is read while the library loads, so each side is ONE child process
(tools/march_index32_hash.py, all cases in it) that prints one sha1 per case over rgb, depth and alphainv.  The indices, the loaded values and the
order of a ray's records are the same on both sides: the hashes must be EQUAL.  The cases and the premise each asserts on the CPU are described in
the tool: big24 (voxel, mask and byte offsets above 2^24 / 2^26), scanlanes (record counts per ray slot set by construction: 0, 1 on the DPP row
and half-wave boundaries, the 8-bit field's maximum, full segments), boxcert (rays that cross the box inside a group, run exactly on a face, lie
outside, carry an infinite / a NaN direction component).  scanlanes is also compared with the CPU oracle at the tolerance of
tests/test_geom_deal_gpu.py (5e-6 absolute), where the oracle's own step list must show the constructed counts.

The host predicate of the 32-bit forms (csrc/k4_index32.h, exported as k4_march_index32_ok) is checked without a GPU at and one past each limit."""
import ctypes
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ['big24', 'scanlanes', 'boxcert']
CHILD_TIMEOUT_S = 300          # one child = a 17 M voxel scene and two small ones built on the host + three millisecond marches


def _hashes(debug):
    env = dict(os.environ, K4_DEBUG=str(debug))
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'march_index32_hash.py')] + CASES, env=env, capture_output=True, text=True,
                         timeout=CHILD_TIMEOUT_S)
    assert out.returncode == 0, out.stdout[-1000:] + out.stderr[-3000:]
    lines = {l.split()[1]: l for l in out.stdout.splitlines() if l.startswith('MARCH_INDEX32_HASH')}
    assert sorted(lines) == sorted(CASES), out.stdout[-2000:]
    return lines


@pytest.fixture(scope='module')
def both_paths():
    return {'general': _hashes(16384 | 1024), 'fast': _hashes(0)}


@pytest.mark.gpu
@pytest.mark.parametrize('case', CASES)
def test_index32_bit_identical(both_paths, case):
    general, fast = both_paths['general'][case], both_paths['fast'][case]
    print(general)
    print(fast)
    assert fast == general
    assert ' interval=1 depth_split=0 ' in general, general           # what the host predicate needs for FAST (launch_march)


@pytest.mark.gpu
def test_scanlanes_against_cpu_oracle():
    """scanlanes on the CPU oracle: its premise (the shaded steps per ray slot are the constructed ones) and the fused frame at 5e-6."""
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    sys.path.insert(0, ROOT)
    import march_index32_hash as T
    from oracle import marcher
    with torch.no_grad():
        ck = T.scan_checkpoint()
        rays = T.scan_rays(ck)
        ref = marcher.mpi_forward(ck['model_kwargs'], ck['model_state_dict'], *rays, **dict(ck['render_kwargs'], render_depth=True))
        step = torch.round(ref['s'] * ref['n_max'] - 0.5).long()
        got = np.zeros((64, 256), dtype=bool)
        for ray, k in zip(ref['ray_id'].tolist(), step.tolist()):
            got[T.slot_of_pixel(ray // 8, ray % 8), k] = True
        want = T.counts_of()
        print('shaded samples', int(got.sum()), 'constructed', int(want.sum()))
        assert (got == want).all(), np.argwhere(got != want)[:10]
        q1 = want[:, 64:128].sum(1)
        assert all(q1[r] == 1 for r in T.ONE_REC) and q1[5] == 16 and q1[40] == 64 and int((q1 == 0).sum()) == 64 - len(T.ONE_REC) - 2
        assert want[:, :64].all() and want[40, 64:128].reshape(4, 16).sum(1).tolist() == [16] * 4
        dev = torch.device('cuda', 0)
        model, rk = T.G.model_of(ck, dev)
        out = model(*[r.to(dev) for r in rays], k4_img_w=8, **rk)
        for k in T.KEYS:
            d = float((out[k].cpu() - ref[k]).abs().max())
            print(k, 'max abs difference', d)
            assert d <= 5e-6, (k, d)


def _predicate():
    from nerf4k_amd import _native
    lib = ctypes.CDLL(_native.LIB_PATH)
    fn = lib.k4_march_index32_ok
    fn.argtypes = [ctypes.c_int64] * 8
    fn.restype = ctypes.c_int
    return fn


def test_index32_predicate_limits():
    """k4_march_index32_ok(X, Y, Z, MX, MY, MZ, occ_bytes, slice_bytes) at and one past each limit; everything else far inside."""
    sys.path.insert(0, ROOT)
    ok = _predicate()
    b24, b32 = 1 << 24, 1 << 32
    llff = (417, 353, 256)
    assert ok(*llff, *llff, 53 * 45 * 8 * 32, 5 * 16 * 256 * 8) == 1                      # the LLFF grid, its summary and its slice
    # X*Y < 2^24 (Z = 1 keeps the byte limit out of the way)
    assert ok(4096, 4095, 1, 1, 1, 1, 0, 0) == 1 and ok(4096, 4096, 1, 1, 1, 1, 0, 0) == 0
    assert ok(b24 - 1, 1, 1, 1, 1, 1, 0, 0) == 1 and ok(b24, 1, 1, 1, 1, 1, 0, 0) == 0
    # Z < 2^24
    assert ok(1, 1, b24 - 1, 1, 1, 1, 0, 0) == 1 and ok(1, 1, b24, 1, 1, 1, 0, 0) == 0
    # MX*MY < 2^24, MZ < 2^24
    assert ok(1, 1, 1, 4096, 4095, 1, 0, 0) == 1 and ok(1, 1, 1, 4096, 4096, 1, 0, 0) == 0
    assert ok(1, 1, 1, 1, 1, b24 - 1, 0, 0) == 1 and ok(1, 1, 1, 1, 1, b24, 0, 0) == 0
    # X*Y*Z*4 < 2^32: 2^30 voxels is one past; 2^30 - 1024 is inside
    assert ok(1024, 1024, 1023, 1, 1, 1, 0, 0) == 1 and ok(1024, 1024, 1024, 1, 1, 1, 0, 0) == 0
    assert ok(1, 1, (1 << 30) - 1, 1, 1, 1, 0, 0) == 0                                   # (Z itself is past 2^24 first)
    # MX*MY*MZ < 2^32
    assert ok(1, 1, 1, 4096, 4095, 256, 0, 0) == 1 and ok(1, 1, 1, 4096, 4095, 257, 0, 0) == 0
    assert 4096 * 4095 * 256 < b32 <= 4096 * 4095 * 257
    assert ok(1, 1, 1, 65535, 1, 65537, 0, 0) == 1 and ok(1, 1, 1, 65536, 1, 65536, 0, 0) == 0      # 2^32 - 1 and 2^32 mask voxels
    # the summary's tables and a bundle's slice, in bytes
    assert ok(1, 1, 1, 1, 1, 1, b32 - 1, 0) == 1 and ok(1, 1, 1, 1, 1, 1, b32, 0) == 0
    assert ok(1, 1, 1, 1, 1, 1, 0, b32 - 1) == 1 and ok(1, 1, 1, 1, 1, 1, 0, b32) == 0
    # nonsense never passes
    assert ok(0, 1, 1, 1, 1, 1, 0, 0) == 0 and ok(1, 1, 1, 1, 1, 1, -1, 0) == 0
