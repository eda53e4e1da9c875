"""Frame evaluation on the device (csrc/k4_metric.hip through lib/utils.py rgb_ssim / frame_metrics and render_viewpoints(eval_ssim=True)) against the
reference's own maps (tests/golden/ssim_ref.npz: lib/utils.py:88-134 of the reference, run on the CPU) and against tests/ssim_oracle.py, which
tests/test_metrics_cpu.py holds to 1e-12 of those maps.

Tolerances, stated as the contract.  The reference's map is a float64 sum of float32 values with float32 products; a reordered float64 sum is <= 5e-13
away from it, float64 products 2e-8 .. 2e-7, a float32 accumulation 5e-7 .. 2e-4 ("Frame evaluation").  The device map and mean are
held to 1e-10 absolute: 200 times a reordering, 200 times below the nearest wrong arithmetic.  PSNR: 1e-4 dB against the reference's float32 pairwise mean
(3.5e-6 dB away from a float64 sum at 1008x756), 1e-9 dB against the float64 sum of the same float32 squares.  Two layouts of one image, a map-less
call and a repeated call give identical bits.
"""
import os
import re

import numpy as np
import pytest
import torch

import nerf4k_amd  # noqa: F401
from nerf4k_amd import _native as N, scene, render
from nerf4k_amd.lib import utils
from helpers import GOLDEN
import ssim_oracle

pytestmark = pytest.mark.gpu

TOL = 1e-10
CASES = ['one', 'ragged', 'rand', 'wide', 'same', 'const_pair', 'anticorr', 'smooth_noise', 'nan', 'taps5', 'taps8']


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(GOLDEN, 'ssim_ref.npz'))


def _planar(t):
    return t.permute(2, 0, 1).contiguous()


def _seeded_pair(h, w, seed):
    rng = np.random.default_rng(seed)
    a = rng.random((h, w, 3), dtype=np.float32)
    b = np.clip(a + 0.1 * rng.standard_normal((h, w, 3)).astype(np.float32), 0, 1).astype(np.float32)
    return a, b


_SEAM = {}


def _seam_case(h, w):
    """(a, b, oracle map, oracle squared-difference sum), computed once per shape and left unchanged."""
    if (h, w) not in _SEAM:
        a, b = _seeded_pair(h, w, 1000 * h + w)
        _SEAM[(h, w)] = (a, b, ssim_oracle.ssim_map(a, b, 1), ssim_oracle.sq_diff_sum(a, b))
    return _SEAM[(h, w)]


@pytest.mark.parametrize('name', CASES)
def test_golden_cases(golden, name):
    a, b, n = golden[f'{name}/img0'], golden[f'{name}/img1'], int(golden[f'{name}/filter_size'])
    want = golden[f'{name}/map']
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    got_t = utils.rgb_ssim(ta, tb, 1, filter_size=n, return_map=True)
    mean_t = utils.rgb_ssim(ta, tb, 1, filter_size=n)
    assert got_t.is_cuda and got_t.dtype == torch.float64 and mean_t.is_cuda and mean_t.dtype == torch.float64 and mean_t.dim() == 0
    got, mean = got_t.cpu().numpy(), float(mean_t)
    assert got.shape == want.shape
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    err = float(np.abs(got[~nan] - want[~nan]).max())
    print(name, 'max |map - reference map| =', err, ' mean', mean, 'reference', float(golden[f'{name}/ssim']))
    assert err <= TOL
    if name == 'nan':
        where = np.zeros_like(nan)
        where[4:15, 10:21, 1] = True                       # the 11 x 11 windows that hold (14, 20) of channel 1, and nothing else
        assert int(nan.sum()) == 121 and np.array_equal(np.isnan(got), where) and np.isnan(mean)
    else:
        assert abs(mean - float(golden[f'{name}/ssim'])) <= TOL
    if name == 'same':
        assert np.array_equal(got, np.ones_like(got)) and mean == 1.0
    # channel-last and planar copies of the same images (and the [1,3,H,W] form, and a mix) give the same bits
    for pa, pb in ((_planar(ta), _planar(tb)), (_planar(ta).unsqueeze(0), _planar(tb).unsqueeze(0)), (_planar(ta), tb)):
        assert np.array_equal(utils.rgb_ssim(pa, pb, 1, filter_size=n, return_map=True).cpu().numpy(), got, equal_nan=True)
        assert np.array_equal(utils.rgb_ssim(pa, pb, 1, filter_size=n).cpu().numpy(), mean_t.cpu().numpy(), equal_nan=True)
    # numpy in, numpy out: drop-in for run_sr.py:147,1134
    s = utils.rgb_ssim(a, b, max_val=1, filter_size=n)
    m = utils.rgb_ssim(a, b, max_val=1, filter_size=n, return_map=True)
    assert isinstance(s, np.float64) and isinstance(m, np.ndarray) and m.dtype == np.float64
    assert np.array_equal(m, got, equal_nan=True) and np.array_equal(s, np.float64(mean), equal_nan=True)


@pytest.mark.parametrize('h,w', [(150, 211), (300, 23), (23, 300)])
def test_tile_seams(h, w):
    a, b, want, _ = _seam_case(h, w)
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    with_map = utils.frame_metrics(ta, tb, return_map=True)
    without = utils.frame_metrics(ta, tb)
    got = with_map['ssim_map'].cpu().numpy()
    err = float(np.abs(got - want).max())
    print(f'{h}x{w}: max |map - oracle map| = {err}, mean {float(with_map["ssim"])} oracle {np.mean(want)}')
    assert got.shape == want.shape and err <= TOL
    assert abs(float(with_map['ssim']) - float(np.mean(want))) <= TOL
    assert 'ssim_map' not in without
    for k in ('ssim', 'mse', 'psnr'):
        assert torch.equal(with_map[k], without[k]), k                 # the same sums, bit for bit, whether the map is written or not


def test_mixed_layouts_and_clamp():
    h, w = 61, 47
    rng = np.random.default_rng(5)
    raw = (rng.random((h, w, 3), dtype=np.float32) * np.float32(1.5) - np.float32(0.2)).astype(np.float32)      # [-0.2, 1.3]
    assert raw.min() < 0 and raw.max() > 1
    gt = rng.random((h, w, 3), dtype=np.float32)
    pred = torch.from_numpy(raw).cuda().permute(2, 0, 1).unsqueeze(0).contiguous()          # planar [1,3,H,W], as the decoder's frames
    tg = torch.from_numpy(gt).cuda()
    got = utils.frame_metrics(pred, tg, clamp_pred=True, return_map=True)
    want = utils.frame_metrics(pred.clamp(0, 1), tg, return_map=True)
    ref = utils.frame_metrics(torch.from_numpy(np.clip(raw, 0, 1)).cuda(), tg, return_map=True)
    for k in ('mse', 'psnr', 'ssim', 'ssim_map'):
        assert torch.equal(got[k], want[k]) and torch.equal(got[k], ref[k]), k
    unclamped = utils.frame_metrics(pred, tg)
    assert not torch.equal(unclamped['mse'], got['mse'])
    assert abs(float(got['ssim']) - ssim_oracle.ssim(np.clip(raw, 0, 1), gt, 1)) <= TOL
    # the decoder's [1,3,H,W] VIEW of a channel-last result is taken as it is
    view = torch.from_numpy(raw).cuda().unsqueeze(0).permute(0, 3, 1, 2)
    assert not view.is_contiguous()
    got_v = utils.frame_metrics(view, tg, clamp_pred=True)
    assert torch.equal(got_v['ssim'], got['ssim']) and torch.equal(got_v['mse'], got['mse'])


@pytest.mark.parametrize('name', CASES)
def test_psnr(golden, name):
    a, b = golden[f'{name}/img0'], golden[f'{name}/img1']
    got = utils.frame_metrics(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda())
    p, want32 = float(got['psnr']), float(golden[f'{name}/psnr'])
    if name == 'nan':
        assert np.isnan(p) and np.isnan(want32)
        return
    with np.errstate(divide='ignore'):
        want64 = ssim_oracle.psnr(a, b)
    print(name, 'psnr', p, 'reference (float32 mean)', want32, 'oracle (float64 sum)', want64)
    assert p == want32 or abs(p - want32) <= 1e-4                       # (`same`: inf on both sides)
    assert p == want64 or abs(p - want64) <= 1e-9
    assert float(got['mse']) == 0.0 or abs(float(got['mse']) / (ssim_oracle.sq_diff_sum(a, b) / a.size) - 1) <= 1e-13


def test_large_filters_past_64k_of_lds():
    """filter_size 28..31 need more than 64 KiB of dynamic LDS (10,240 + 2,048 n bytes).  A smaller one of them is scored FIRST in the process that
    runs this file, then the largest: the limit raised for the first must cover the second.  120 columns are more than one strip wide at both sizes
    (360 - 3 (n - 1) outputs against strips of 256 - 3 (n - 1)); 31 taps use the whole 256-wide LDS row (166 + 90)."""
    a, b = _seeded_pair(60, 120, 2831)
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    for n in (28, 31, 29):
        got = utils.rgb_ssim(ta, tb, 1, filter_size=n, return_map=True).cpu().numpy()
        mean = float(utils.rgb_ssim(_planar(ta), tb, 1, filter_size=n))
        want = ssim_oracle.ssim_map(a, b, 1, filter_size=n)
        err = float(np.abs(got - want).max())
        print(f'filter_size {n}: max |map - oracle map| = {err}, mean {mean} oracle {np.mean(want)}')
        assert got.shape == want.shape == (61 - n, 121 - n, 3) and err <= TOL and abs(mean - float(np.mean(want))) <= TOL


def test_determinism():
    a, b, _, _ = _seam_case(150, 211)
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    one, two = utils.frame_metrics(ta, tb), utils.frame_metrics(ta, tb)
    assert torch.equal(one['ssim'], two['ssim']) and torch.equal(one['mse'], two['mse'])


def test_errors():
    a = torch.rand(10, 40, 3, device='cuda')
    with pytest.raises(N.K4Error, match='smaller'):
        utils.rgb_ssim(a, a, 1)
    with pytest.raises(N.K4Error):
        utils.rgb_ssim(a, torch.rand(10, 41, 3, device='cuda'), 1, filter_size=5)
    with pytest.raises(N.K4Error):
        utils.rgb_ssim(a.double(), a.double(), 1, filter_size=5)
    with pytest.raises(N.K4Error):
        utils.rgb_ssim(a, a, 1, filter_size=32)
    lib = N.lib()
    assert lib.k4_frame_metrics_workspace_bytes(10, 40, 11) == -1 and lib.k4_frame_metrics_workspace_bytes(11, 11, 11) == 16
    taps = (N.C.c_double * 11)(*utils.ssim_taps(11, 1.5))
    sums, ws = torch.zeros(2, dtype=torch.float64, device='cuda'), torch.zeros(64, dtype=torch.uint8, device='cuda')
    rc = lib.k4_frame_metrics(N.f32(a), 3, 1, 0, N.f32(a), 3, 1, 0, 10, 40, taps, 11, 1e-4, 9e-4, None, N.ptr(ws), N.ptr(sums), N.stream())
    assert rc == N.K4_ERR_UNSUPPORTED
    rc = lib.k4_frame_metrics(N.f32(a), 3, 1, 0, N.f32(a), 3, 1, 0, 40000, 40000, taps, 11, 1e-4, 9e-4, None, N.ptr(ws), N.ptr(sums), N.stream())
    assert rc == N.K4_ERR_UNSUPPORTED                                   # beyond 2^31 elements: refused before anything is launched
    one = (N.C.c_double * 1)(1.0)
    W = (2**31 - 100) // 3                                              # H W 3 < 2^31, but the last strip's threads would count past 2^31
    rc = lib.k4_frame_metrics(N.f32(a), 3, 1, 0, N.f32(a), 3, 1, 0, 1, W, one, 1, 1e-4, 9e-4, None, N.ptr(ws), N.ptr(sums), N.stream())
    assert rc == N.K4_ERR_UNSUPPORTED and lib.k4_frame_metrics_workspace_bytes(1, W, 1) == -1
    # a [3,H,3] tensor could be either layout: refused; the four-dimensional form and a numpy array are not ambiguous
    amb = torch.rand(3, 8, 3, device='cuda')
    with pytest.raises(N.K4Error, match='both'):
        utils.rgb_ssim(amb, amb, 1, filter_size=3)
    as_planar = utils.rgb_ssim(amb.unsqueeze(0), amb.unsqueeze(0) * 0.5, 1, filter_size=3, return_map=True)
    assert tuple(as_planar.shape) == (6, 1, 3)
    want = ssim_oracle.ssim_map(amb.permute(1, 2, 0).contiguous().cpu().numpy(), (amb * 0.5).permute(1, 2, 0).contiguous().cpu().numpy(), 1, filter_size=3)
    assert float(np.abs(as_planar.cpu().numpy() - want).max()) <= TOL
    assert utils.rgb_ssim(amb.cpu().numpy(), amb.cpu().numpy(), 1, filter_size=3, return_map=True).shape == (1, 6, 3)


def test_render_viewpoints_eval_ssim(capsys):
    """run_sr.py:143-155 on the small synthetic LLFF scene of tests/test_e2e_gpu.py: the flag changes nothing that is returned, and the printed mean is
    the SSIM of the returned (clamped) frames against the ground truth."""
    ck = scene.make_llff_checkpoint(seed=11, num_voxels=48 * 48 * 32, mpi_depth=32)
    H, W = 44, 60
    K = scene.LLFF_K.copy()
    K[:2] *= W / scene.LLFF_HW[1]
    model = utils.model_from_checkpoint_dict(ck).cuda().eval()
    poses = scene.llff_spiral_poses()[[2, 9]]
    rk = dict(ck['render_kwargs'], bg=1.5, render_depth=True)            # bg > 1: marched colours leave [0, 1], the clamp matters
    HW, Ks = np.array([[H, W], [H, W]]), np.stack([K, K])
    plain = render.render_viewpoints(model, poses, HW, Ks, True, rk)
    rng = np.random.default_rng(3)
    gt = [np.clip(f + 0.05 * rng.standard_normal(f.shape).astype(np.float32), 0, 1).astype(np.float32) for f in plain[0]]
    base = render.render_viewpoints(model, poses, HW, Ks, True, rk, gt_imgs=gt)
    capsys.readouterr()
    got = render.render_viewpoints(model, poses, HW, Ks, True, rk, gt_imgs=gt, eval_ssim=True)
    out = capsys.readouterr().out
    for x, y in zip(got, base):
        if isinstance(x, list):
            assert len(x) == len(y) and all(np.array_equal(np.asarray(u.cpu() if torch.is_tensor(u) else u), np.asarray(v.cpu() if torch.is_tensor(v) else v))
                                            for u, v in zip(x, y))
        else:
            assert np.array_equal(x, y)
    m = re.search(r'^Testing ssim (\S+) \(avg\)$', out, re.M)
    assert m, out
    want = np.mean([ssim_oracle.ssim(got[0][i], gt[i], 1) for i in range(2)])
    print('render_viewpoints ssim', float(m.group(1)), 'oracle', want)
    assert abs(float(m.group(1)) - want) <= TOL
    # no ground truth, or a reduced render: nothing is scored and nothing printed (run_sr.py:143)
    render.render_viewpoints(model, poses[:1], HW[:1], Ks[:1], True, rk, eval_ssim=True)
    assert 'Testing ssim' not in capsys.readouterr().out


def test_full_frame():
    """One 756 x 1008 frame (the LLFF render size): 37 x 14 workgroups; the mean only."""
    a, b = _seeded_pair(756, 1008, 77)
    got = utils.frame_metrics(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda())
    want = ssim_oracle.ssim(a, b, 1)
    print('756x1008 mean ssim', float(got['ssim']), 'oracle', want, 'psnr', float(got['psnr']), 'oracle', ssim_oracle.psnr(a, b))
    assert abs(float(got['ssim']) - want) <= TOL
    assert abs(float(got['psnr']) - ssim_oracle.psnr(a, b)) <= 1e-9
