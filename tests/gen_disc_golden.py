"""Writes tests/golden/disc_nf8.npz from the reference's own ``UNetDiscriminatorSN`` (lib/sr_unetdisc.py of the reference tree, imported in place,
unmodified).  Runs on the CPU of the build machine only; the tests read the .npz.

``lib/sr_unetdisc.py`` imports ``DiscriminatorEpilogue`` from ``lib.utils``, which needs cv2: a stub ``lib.utils`` module with that one name stands
in (``UNetDiscriminatorSN`` itself does not use it).

Contents (num_feat=8, 68,649 parameters; inputs 64x64 and 40x24, uniform 8-bit levels in [0, 1); parameters rounded to bf16 values so that the file stays small):
    sd/<key>                       the seeded state_dict (before any call)
    x_<tag>                        the input
    <tag>/logits                   training-mode logits of the first call from that state
    <tag>/u/<layer>, <tag>/v/..    weight_u / weight_v after that call
    <tag>/gx, <tag>/g/<param>      gradient of mean(softplus(-logits)) w.r.t. the input and every parameter
    <tag>/eval                     eval-mode logits from the initial state
    <tag>/u3/<layer>               weight_u after the joint loop's three calls (parameters frozen on a fake image, real image, fake image)
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import ref_import  # noqa: E402

REF = ref_import.REFERENCE_ROOT
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'disc_nf8.npz')


def reference_class():
    lib = types.ModuleType('lib')
    lib.__path__ = [os.path.join(REF, 'lib')]
    utils = types.ModuleType('lib.utils')
    utils.DiscriminatorEpilogue = type('DiscriminatorEpilogue', (torch.nn.Module,), {})
    saved = {k: sys.modules.get(k) for k in ('lib', 'lib.utils')}
    sys.modules['lib'], sys.modules['lib.utils'] = lib, utils
    try:
        spec = importlib.util.spec_from_file_location('lib.sr_unetdisc', os.path.join(REF, 'lib', 'sr_unetdisc.py'))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return mod.UNetDiscriminatorSN


def main():
    if not ref_import.available():
        raise SystemExit('the reference tree is not present: nothing to generate')
    torch.set_num_threads(1)
    Ref = reference_class()
    torch.manual_seed(20261016)
    net = Ref(3, num_feat=8)
    with torch.no_grad():
        for p in net.parameters():              # parameters on the bf16 grid, images on the 8-bit grid: exact fp32 values that compress well
            p.copy_(p.bfloat16().float())
    sd0 = {k: v.clone() for k, v in net.state_dict().items()}
    out = {f'sd/{k}': v.numpy() for k, v in sd0.items()}
    g = torch.Generator().manual_seed(7)
    for tag, (h, w) in (('a', (64, 64)), ('b', (40, 24))):
        x = torch.floor(torch.rand([1, 3, h, w], generator=g) * 256) / 256
        x2 = torch.floor(torch.rand([1, 3, h, w], generator=g) * 256) / 256          # the "real" image of the three-call sequence
        out[f'x_{tag}'], out[f'x2_{tag}'] = x.numpy(), x2.numpy()
        net.load_state_dict(sd0)
        net.train()
        xi = x.clone().requires_grad_(True)
        logits = net(xi)
        F.softplus(-logits).mean().backward()
        out[f'{tag}/logits'] = logits.detach().numpy()
        out[f'{tag}/gx'] = xi.grad.numpy()
        for k, v in net.state_dict().items():
            if k.endswith('weight_u'):
                out[f'{tag}/u/{k[:-9]}'] = v.numpy().copy()
            if k.endswith('weight_v'):
                out[f'{tag}/v/{k[:-9]}'] = v.numpy().copy()
        for k, p in net.named_parameters():
            out[f'{tag}/g/{k}'] = p.grad.numpy().copy()
            p.grad = None
        net.load_state_dict(sd0)
        net.eval()
        with torch.no_grad():
            out[f'{tag}/eval'] = net(x).numpy()
        net.load_state_dict(sd0)
        net.train()
        for p in net.parameters():
            p.requires_grad = False
        net(x)
        for p in net.parameters():
            p.requires_grad = True
        net(x2)
        net(x.detach())
        for k, v in net.state_dict().items():
            if k.endswith('weight_u'):
                out[f'{tag}/u3/{k[:-9]}'] = v.numpy().copy()
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), 'bytes', len(out), 'arrays')


if __name__ == '__main__':
    main()
