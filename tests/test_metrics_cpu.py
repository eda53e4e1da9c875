"""CPU-side checks of the frame metrics (lib/utils.py rgb_ssim / frame_metrics; the kernel itself: tests/test_metrics_gpu.py): the plain-numpy
oracle the GPU tests lean on reproduces the reference's own maps (tests/golden/ssim_ref.npz, written by tests/gen_ssim_golden.py from the
reference's rgb_ssim), the host tap table is the reference's bit for bit, and there is no CPU path."""
import os

import numpy as np
import pytest
import torch

import nerf4k_amd  # noqa: F401
from nerf4k_amd import _native as N, render
from nerf4k_amd.lib import utils
from helpers import GOLDEN
import ssim_oracle

CASES = ['one', 'ragged', 'rand', 'wide', 'same', 'const_pair', 'anticorr', 'smooth_noise', 'nan', 'taps5', 'taps8']


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(GOLDEN, 'ssim_ref.npz'))


@pytest.mark.parametrize('name', CASES)
def test_oracle_meets_the_reference_map(golden, name):
    a, b, n = golden[f'{name}/img0'], golden[f'{name}/img1'], int(golden[f'{name}/filter_size'])
    want = golden[f'{name}/map']
    got = ssim_oracle.ssim_map(a, b, 1, filter_size=n)
    assert got.dtype == np.float64 and got.shape == want.shape == (a.shape[0] - n + 1, a.shape[1] - n + 1, 3)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    err = float(np.abs(got[ok] - want[ok]).max())
    print(name, 'max |oracle map - reference map| =', err)
    assert err <= 1e-12
    if ok.all():
        assert abs(ssim_oracle.ssim(a, b, 1, filter_size=n) - float(golden[f'{name}/ssim'])) <= 1e-12
        with np.errstate(divide='ignore'):
            p, want_p = ssim_oracle.psnr(a, b), float(golden[f'{name}/psnr'])
        assert p == want_p or abs(p - want_p) <= 1e-4          # the reference's value is a float32 pairwise mean; `same`: inf on both sides
    else:
        assert name == 'nan' and np.isnan(golden[f'{name}/ssim']) and np.isnan(golden[f'{name}/psnr'])
        assert int(np.isnan(want).sum()) == 121 and np.isnan(want[4:15, 10:21, 1]).all()


def test_golden_cases_are_what_they_claim(golden):
    assert np.array_equal(golden['same/map'], np.ones_like(golden['same/map']))
    assert float(golden['anticorr/ssim']) < 0
    assert tuple(golden['one/map'].shape) == (1, 1, 3)


@pytest.mark.parametrize('n', [1, 4, 5, 8, 11])
def test_host_tap_table_is_the_reference_table(golden, n):
    """Against the table the reference's own rgb_ssim handed to its convolution (lib/utils.py:100-104, recorded by tests/gen_ssim_golden.py)."""
    want = golden[f'taps/{n}']
    got = utils.ssim_taps(n, 1.5)
    assert want.dtype == np.float64 and want.shape == (n,)
    assert got.dtype == np.float64 and np.array_equal(got, want)
    assert np.array_equal(got, got[::-1])           # symmetric, odd and even: correlation equals convolution
    assert np.array_equal(ssim_oracle.taps_of(n, 1.5), want)


def test_no_cpu_path_and_no_other_dtype():
    a = torch.rand(16, 16, 3)
    with pytest.raises(N.K4Error):
        utils.rgb_ssim(a, a, 1)
    with pytest.raises(N.K4Error):
        utils.frame_metrics(a, a)
    with pytest.raises(N.K4Error):                  # float64 frames would change the reference's fp32 rounding of the squares
        utils.rgb_ssim(a.double(), a.double(), 1)
    with pytest.raises(N.K4Error):
        utils.rgb_ssim(np.zeros((16, 16, 3)), np.zeros((16, 16, 3)), 1)
    with pytest.raises(N.K4Error):
        utils.rgb_ssim(np.zeros((16, 16, 4), np.float32), np.zeros((16, 16, 4), np.float32), 1)


def test_lpips_still_raises():
    for kw in ({'eval_lpips_vgg': True}, {'eval_lpips_alex': True}):
        with pytest.raises(NotImplementedError, match='lpips'):
            render.render_viewpoints(None, [], [], [], True, {}, **kw)


def test_signature_is_the_reference_signature():
    import inspect
    sig = inspect.signature(utils.rgb_ssim)
    assert list(sig.parameters) == ['img0', 'img1', 'max_val', 'filter_size', 'filter_sigma', 'k1', 'k2', 'return_map']
    assert [p.default for p in sig.parameters.values()][3:] == [11, 1.5, 0.01, 0.03, False]
    assert list(inspect.signature(utils.frame_metrics).parameters) == ['pred', 'gt', 'max_val', 'clamp_pred', 'return_map']
