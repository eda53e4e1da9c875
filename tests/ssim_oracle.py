"""The frame metrics in plain numpy (no scipy: a GPU box may not have it): what the device results are compared with on shapes that have no
golden file.  tests/test_metrics_cpu.py holds this restatement to 1e-12 of the reference's own ``rgb_ssim`` maps (tests/golden/ssim_ref.npz).

Arithmetic as the reference (lib/utils.py:88-134): float32 images filtered with a float64 tap table, so every filtered moment is a float64 sum;
``img0**2``, ``img1**2`` and ``img0 * img1`` are float32 products, rounded before they are filtered.  The vertical pass comes first and a pass adds its taps from the last
sample of the window to the first, the order of a direct convolution's inner loop: in that order the golden maps are met exactly, in any other to ~1e-12
(the variances of a smooth image are differences of nearly equal sums).
"""
import numpy as np


def taps_of(filter_size, filter_sigma):
    half = filter_size // 2
    shift = (2 * half - filter_size + 1) / 2
    t = np.exp(-0.5 * ((np.arange(filter_size) - half + shift) / filter_sigma)**2)
    return t / np.sum(t)


def _blur_valid(z, taps):
    """'valid' separable filter of a float32 [H,W,3] image with a float64 table -> float64 [H-n+1, W-n+1, 3]."""
    assert z.dtype == np.float32
    n = len(taps)
    H, W = z.shape[:2]
    v = np.zeros((H - n + 1, W, z.shape[2]), np.float64)
    for k in range(n - 1, -1, -1):
        v += taps[k] * z[k:k + H - n + 1].astype(np.float64)
    h = np.zeros((H - n + 1, W - n + 1, z.shape[2]), np.float64)
    for k in range(n - 1, -1, -1):
        h += taps[k] * v[:, k:k + W - n + 1]
    return h


def ssim_map(img0, img1, max_val, filter_size=11, filter_sigma=1.5, k1=0.01, k2=0.03):
    assert img0.dtype == np.float32 and img1.dtype == np.float32 and img0.shape == img1.shape and img0.shape[-1] == 3
    taps = taps_of(filter_size, filter_sigma)
    mu0, mu1 = _blur_valid(img0, taps), _blur_valid(img1, taps)
    mu00, mu11, mu01 = mu0 * mu0, mu1 * mu1, mu0 * mu1
    with np.errstate(invalid='ignore'):
        s00 = np.maximum(0., _blur_valid(img0 * img0, taps) - mu00)
        s11 = np.maximum(0., _blur_valid(img1 * img1, taps) - mu11)
        s01 = _blur_valid(img0 * img1, taps) - mu01
        s01 = np.sign(s01) * np.minimum(np.sqrt(s00 * s11), np.abs(s01))
    c1, c2 = (k1 * max_val)**2, (k2 * max_val)**2
    return ((2 * mu01 + c1) * (2 * s01 + c2)) / ((mu00 + mu11 + c1) * (s00 + s11 + c2))


def ssim(img0, img1, max_val, **kw):
    return np.mean(ssim_map(img0, img1, max_val, **kw))


def sq_diff_sum(img0, img1):
    """float64 sum of the float32 squared differences (the reference's np.mean(np.square(a - b)) is a float32 pairwise mean of the same terms)."""
    d = img0 - img1
    return float(np.sum((d * d).astype(np.float64)))


def psnr(img0, img1):
    return -10. * np.log10(sq_diff_sum(img0, img1) / img0.size)
