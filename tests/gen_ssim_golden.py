"""Writes tests/golden/ssim_ref.npz from the reference's own ``rgb_ssim`` (lib/utils.py of the reference tree, imported in place, unmodified) and the
PSNR expression of run_sr.py:144.  Runs on the CPU of the build machine only (it needs scipy, as the reference does); the tests read the .npz.

``lib/utils.py`` imports cv2, ``torch_utils.misc`` and ``.masked_adam`` at module level; empty stub modules stand in (``rgb_ssim`` uses none of them).

Per case <name>:
    <name>/img0, <name>/img1      float32 [H,W,3] on 8-bit levels k / 255 (``const_pair``: float32 0.3 and 0.7; ``nan``: one NaN in img0)
    <name>/filter_size            int
    <name>/map                    the reference's float64 SSIM map (max_val = 1)
    <name>/ssim                   its mean, as the reference returns it
    <name>/psnr                   -10 log10(np.mean(np.square(img0 - img1))): the reference's float32 value
and, for filter sizes 1, 4, 5, 8 and 11 (sigma 1.5):
    taps/<n>                      the float64 table the reference's rgb_ssim itself hands to scipy.signal.convolve2d (recorded from inside a call)
"""
import importlib.util
import os
import sys
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import ref_import  # noqa: E402

REF = ref_import.REFERENCE_ROOT
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ssim_ref.npz')


def reference_utils():
    lib = types.ModuleType('lib')
    lib.__path__ = [os.path.join(REF, 'lib')]
    stubs = {'lib': lib, 'cv2': types.ModuleType('cv2'), 'torch_utils': types.ModuleType('torch_utils'),
             'torch_utils.misc': types.ModuleType('torch_utils.misc'), 'lib.masked_adam': types.ModuleType('lib.masked_adam')}
    stubs['cv2'].COLORMAP_JET = 2
    stubs['torch_utils'].misc = stubs['torch_utils.misc']
    stubs['lib.masked_adam'].MaskedAdam = object
    saved = {k: sys.modules.get(k) for k in stubs}
    sys.modules.update(stubs)
    sys.dont_write_bytecode = True
    try:
        spec = importlib.util.spec_from_file_location('lib.utils', os.path.join(REF, 'lib', 'utils.py'))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return mod


def levels(rng, h, w):
    return (rng.integers(0, 256, size=(h, w, 3)).astype(np.float32) / np.float32(255)).astype(np.float32)


def quantise(x):
    return (np.round(np.clip(x, 0, 1) * 255).astype(np.float32) / np.float32(255)).astype(np.float32)


def cases():
    rng = np.random.default_rng(20261018)
    out = {}
    for name, (h, w) in (('one', (11, 11)), ('ragged', (12, 37)), ('rand', (75, 70)), ('wide', (43, 140))):
        out[name] = (levels(rng, h, w), levels(rng, h, w), 11)
    a = levels(rng, 40, 52)
    out['same'] = (a, a.copy(), 11)
    out['const_pair'] = (np.full((30, 33, 3), 0.3, np.float32), np.full((30, 33, 3), 0.7, np.float32), 11)
    ramp = np.broadcast_to((np.arange(64, dtype=np.float64) / 63)[None, :, None], (48, 64, 3))
    out['anticorr'] = (quantise(ramp), quantise(1 - ramp), 11)
    yy, xx = np.meshgrid(np.arange(64) / 63, np.arange(80) / 79, indexing='ij')
    smooth = np.stack([0.5 + 0.3 * np.sin(2.1 * xx + c) * np.cos(1.7 * yy) for c in range(3)], -1)
    out['smooth_noise'] = (quantise(smooth), quantise(smooth + rng.integers(-1, 2, size=smooth.shape) / 255), 11)
    a, b = levels(rng, 30, 41), levels(rng, 30, 41)
    a[14, 20, 1] = np.nan
    out['nan'] = (a, b, 11)
    out['taps5'] = (levels(rng, 30, 41), levels(rng, 30, 41), 5)
    out['taps8'] = (levels(rng, 30, 41), levels(rng, 30, 41), 8)
    return out


def reference_taps(ref, n):
    """The table rgb_ssim builds for `filter_size` n, taken from the first argument pair it passes to scipy.signal.convolve2d (a column vector)."""
    seen = []
    real = ref.scipy.signal.convolve2d

    def recording(z, f, **kw):
        seen.append(np.array(f, copy=True))
        return real(z, f, **kw)
    ref.scipy.signal.convolve2d = recording
    try:
        ref.rgb_ssim(np.zeros((n, n, 3), np.float32), np.zeros((n, n, 3), np.float32), max_val=1, filter_size=n)
    finally:
        ref.scipy.signal.convolve2d = real
    col = seen[0]
    assert col.dtype == np.float64 and col.shape == (n, 1) and all(np.array_equal(f.reshape(-1), col[:, 0]) for f in seen)
    return col[:, 0].copy()


def main():
    if not ref_import.available():
        raise SystemExit('the reference tree is not present: nothing to generate')
    ref = reference_utils()
    out = {f'taps/{n}': reference_taps(ref, n) for n in (1, 4, 5, 8, 11)}
    for name, (a, b, n) in cases().items():
        with np.errstate(invalid='ignore'):
            m = ref.rgb_ssim(a, b, max_val=1, filter_size=n, return_map=True)
            s = ref.rgb_ssim(a, b, max_val=1, filter_size=n)
            p = -10. * np.log10(np.mean(np.square(a - b)))                  # run_sr.py:144
        assert m.dtype == np.float64 and m.shape == (a.shape[0] - n + 1, a.shape[1] - n + 1, 3)
        out[f'{name}/img0'], out[f'{name}/img1'], out[f'{name}/filter_size'] = a, b, np.int64(n)
        out[f'{name}/map'], out[f'{name}/ssim'], out[f'{name}/psnr'] = m, np.float64(s), np.asarray(p)
        print(name, a.shape, n, 'ssim', s, 'psnr', p, p.dtype if hasattr(p, 'dtype') else type(p))
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), 'bytes', len(out), 'arrays')


if __name__ == '__main__':
    main()
