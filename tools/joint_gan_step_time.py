"""ms per joint training iteration (configs[4]: 64x64 patch, 5-block SFTNet) without and with the adversarial term, the discriminator
(num_feat=64 on the 256x256 decoder output) on the HIP path and on the tensor-library path, ALTERNATED iteration by iteration in one
process; plus the discriminator alone and its 4x4 stride-2 kernels one by one.  GPU box.

    python tools/joint_gan_step_time.py [--iters 200] [--step0 0] [--kernels]

Every figure is the time between two device events around synchronised work (the iteration is synchronised before the first event and
the second event is waited for), after a warm-up of every variant.  Prints one JSON line per section."""
import argparse
import contextlib
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import nerf4k_amd  # noqa: F401,E402
from nerf4k_amd import scene, joint_train  # noqa: E402
from nerf4k_amd.lib import dvgo, sr_esrnet, sr_unetdisc, utils  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--iters', type=int, default=200)
ap.add_argument('--step0', type=int, default=0, help='0: the dense-TV iterations; >= 10000: the iterations after tv_before')
ap.add_argument('--kernels', action='store_true', help='also time the discriminator alone and the 4x4 stride-2 kernels')
args = ap.parse_args()
dev = torch.device('cuda', 0)


def timed(fn):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(v):
    v = sorted(v)
    return {'median_ms': round(statistics.median(v), 3), 'p10_ms': round(v[len(v) // 10], 3), 'p90_ms': round(v[len(v) * 9 // 10], 3), 'n': len(v)}


ck = scene.make_llff_checkpoint()
H, W = scene.LLFF_HW
ro, rd, vd = dvgo.get_rays_of_a_view(H, W, scene.LLFF_K, torch.from_numpy(scene.llff_spiral_poses()[0]).to(dev), True, False, False, False)
model = utils.model_from_checkpoint_dict(ck).to(dev).train()
torch.manual_seed(778)
net = sr_esrnet.SFTNet(3, scale=4, num_feat=64, num_block=5, num_grow_ch=32, num_cond=1).to(dev).train()
net_d = sr_unetdisc.UNetDiscriminatorSN(3, num_feat=64, skip_connection=True).to(dev).train()
cfg = joint_train.JointCfg.fern_lg_joint_l1_gan(weight_pcp=0, weight_style=0)
with contextlib.redirect_stdout(sys.stderr):
    tr = joint_train.JointTrainer(model, net, cfg, dict(ck['render_kwargs'], render_depth=True, rand_bkgd=True), n_train_images=17, net_d=net_d)
g = torch.Generator(device=dev).manual_seed(5)


def batch(i):
    r0, c0 = (37 * i) % (H - 64), (101 * i) % (W - 64)
    rays = [x[r0:r0 + 64, c0:c0 + 64].reshape(-1, 3).contiguous() for x in (ro, rd, vd)]
    return rays + [torch.rand([4096, 3], device=dev, generator=g), torch.rand([65536, 3], device=dev, generator=g), 64, 64]


# the three variants of ONE trainer: without the term (what JointTrainer does when weight_gan == 0: net_d is None), D on the HIP path, D on the library
VARIANTS = {'no_gan': (None, True), 'gan_hip': (net_d, True), 'gan_library': (net_d, False)}
times = {k: [] for k in VARIANTS}
step = [args.step0]


def one(name):
    tr.net_d, sr_unetdisc._K4 = VARIANTS[name]
    step[0] += 1
    b = batch(step[0])
    return timed(lambda: tr.step(*b, global_step=step[0]))


for _ in range(5):                       # warm-up of every variant (allocator, launch tapes, MIOpen's kernel selection)
    for name in VARIANTS:
        one(name)
for _ in range(args.iters):
    for name in VARIANTS:
        times[name].append(one(name))
tr.net_d, sr_unetdisc._K4 = net_d, True
out = {k: stats(v) for k, v in times.items()}
pairs = [a - b for a, b in zip(times['gan_library'], times['gan_hip'])]
out['library_minus_hip_ms'] = stats(pairs)
out['step0'] = args.step0
print(json.dumps({'joint_iteration': out}))

if args.kernels:
    x = torch.rand([1, 3, 256, 256], device=dev)
    cri = sr_unetdisc.GANLoss('vanilla', loss_weight=0.05)

    def d_pass(train_d):
        for p in net_d.parameters():
            p.requires_grad = train_d
            p.grad = None
        xi = x.clone().requires_grad_(not train_d)
        cri(net_d(xi), True, is_disc=train_d).backward()
    res = {}
    for train_d in (False, True):
        t = {True: [], False: []}
        for i in range(10 + 100):
            for k4 in (True, False):
                sr_unetdisc._K4 = k4
                ms = timed(lambda: d_pass(train_d))
                if i >= 10:
                    t[k4].append(ms)
        res['discriminator_step' if train_d else 'generator_pass'] = {'hip': stats(t[True]), 'library': stats(t[False])}
    sr_unetdisc._K4 = True
    print(json.dumps({'discriminator_forward_backward_256x256_nf64': res}))
    # the 4x4 stride-2 layers alone: 50 launches between two events; FLOP = 2 * pixels_out * cout * cin * 16 per pass
    layers = {}
    for name, cin, cout, hw in (('conv1', 64, 128, 256), ('conv2', 128, 256, 128), ('conv3', 256, 512, 64)):
        xin = torch.randn([hw, hw, cin], device=dev)
        gy = torch.randn([hw // 2, hw // 2, cout], device=dev)
        w = torch.randn([cout, cin, 4, 4], device=dev) / (cin * 16) ** 0.5
        u = torch.nn.functional.normalize(torch.randn([cout], device=dev), dim=0)
        v = torch.nn.functional.normalize(torch.randn([cin * 16], device=dev), dim=0)
        _, wf, wb = sr_unetdisc.sn_prepare(w, u, v, False, 4)
        xt, wt = xin.permute(2, 0, 1).unsqueeze(0).contiguous().requires_grad_(True), w.clone().requires_grad_(True)
        gyt = gy.permute(2, 0, 1).unsqueeze(0).contiguous()
        flop = 2.0 * (hw // 2) ** 2 * cout * cin * 16
        row = {'gflop_per_pass': round(flop / 1e9, 2)}
        fns = {'forward': lambda: sr_unetdisc.conv_s2(xin, hw, hw, cin, wf, cout, 0, True),
               'dgrad': lambda: sr_unetdisc.conv_s2(gy, hw // 2, hw // 2, cout, wb, cin, 1),
               'wgrad': lambda: sr_unetdisc.wgrad_s2(xin, hw, hw, cin, gy, cout),
               'library_forward': lambda: torch.nn.functional.conv2d(xt.detach(), wt.detach(), None, 2, 1),
               'library_dgrad': lambda: torch.autograd.grad(torch.nn.functional.conv2d(xt, wt.detach(), None, 2, 1), xt, gyt),
               'library_wgrad': lambda: torch.autograd.grad(torch.nn.functional.conv2d(xt.detach(), wt, None, 2, 1), wt, gyt)}
        for k, fn in fns.items():
            for _ in range(5):
                fn()
            ms = timed(lambda: [fn() for _ in range(50)]) / 50
            row[k] = {'ms': round(ms, 4)}
            if not k.startswith('library'):
                row[k]['useful_tflops'] = round(flop / ms / 1e9, 1)
                row[k]['mfma_tflops_6_products'] = round(6 * flop / ms / 1e9, 1)
            elif k != 'library_forward':
                row[k]['note'] = 'includes the forward convolution of the autograd graph'
        layers[name] = row
    print(json.dumps({'conv4x4_stride2_layers': layers}))
