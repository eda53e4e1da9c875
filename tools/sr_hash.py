"""sha1 of the VC-Decoder's output (SFTNet x4, one block, with a condition image) on a 32 x 40 input -- ragged against every tile size of the
convolution kernels -- under the CURRENT environment: the library reads K4_SR_DEBUG once while it loads, so runs that differ in it are compared
across processes (tests/test_ablation_bits_gpu.py).  One line per decoder arithmetic: K4_SR_MODE=f16x3p (the p16 kernels of k4_sr_p16.hip) and
bf16x6 (the 3x3 kernel of k4_sr.hip).      python tools/sr_hash.py [H W]"""
import hashlib, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import nerf4k_amd  # noqa: F401
from nerf4k_amd.lib import sr_esrnet
H, W = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (32, 40)
g = torch.Generator().manual_seed(23)
x = torch.rand([1, 3, H, W], generator=g).cuda()
cond = torch.rand([1, 1, H, W], generator=g).cuda()
for mode in ('f16x3p', 'bf16x6'):
    os.environ['K4_SR_MODE'] = mode                       # read by SFTNet.__init__
    torch.manual_seed(7)                                  # the same weights for both modes
    net = sr_esrnet.SFTNet(3, scale=4, num_feat=64, num_block=1, num_grow_ch=32, num_cond=1).cuda().eval()
    assert net.k4_mode == mode
    with torch.no_grad():
        hr = net(x, cond)
    torch.cuda.synchronize()
    assert hr.shape == (1, 3, 4 * H, 4 * W)
    print('SR_HASH', mode, hashlib.sha1(hr.cpu().numpy().tobytes()).hexdigest(), f'{H}x{W}', f'max|hr|={float(hr.abs().max()):.6g}')
