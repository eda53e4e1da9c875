"""ms per joint training iteration (configs[4]: 64x64 patch, 5-block SFTNet, the "+gan" recipe with its discriminator) without and with the
perceptual / style terms, ALTERNATED iteration by iteration in one process; the loss module's forward + backward alone at 256x256 against
the same network built from torch-ROCm eager operations in fp32; and the 3x3 kernels layer group by layer group.  GPU box.

    python tools/joint_pcp_step_time.py [--iters 200] [--step0 0] [--layers] [--module-only]

Every figure is the time between two device events around synchronised work, after a warm-up of every variant.  The VGG19 weights are the
seeded ones of lib/sr_loss.seeded_vgg19_state_dict (the time does not depend on their values).  Prints one JSON line per section."""
import argparse
import contextlib
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn as nn
import nerf4k_amd  # noqa: F401,E402
from nerf4k_amd import scene, joint_train  # noqa: E402
from nerf4k_amd.lib import dvgo, sr_esrnet, sr_loss, sr_unetdisc, utils  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--iters', type=int, default=200)
ap.add_argument('--step0', type=int, default=0, help='0: the dense-TV iterations; >= 10000: the iterations after tv_before')
ap.add_argument('--layers', action='store_true', help='also time the 3x3 kernels per layer group')
ap.add_argument('--module-only', action='store_true', help='skip the joint iteration')
args = ap.parse_args()
dev = torch.device('cuda', 0)
LW = {'conv1_2': 0, 'conv2_2': 0, 'conv3_4': 1, 'conv4_4': 1, 'conv5_4': 1}       # run_sr.py:671-677


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


sd = sr_loss.seeded_vgg19_state_dict(7)
cri = sr_loss.PerceptualLoss(LW, perceptual_weight=0.5, style_weight=0.2).load_vgg_state_dict(sd).to(dev)

if not args.module_only:
    ck = scene.make_llff_checkpoint()
    H, W = scene.LLFF_HW
    ro, rd, vd = dvgo.get_rays_of_a_view(H, W, scene.LLFF_K, torch.from_numpy(scene.llff_spiral_poses()[0]).to(dev), True, False, False, False)
    model = utils.model_from_checkpoint_dict(ck).to(dev).train()
    torch.manual_seed(778)
    net = sr_esrnet.SFTNet(3, scale=4, num_feat=64, num_block=5, num_grow_ch=32, num_cond=1).to(dev).train()
    net_d = sr_unetdisc.UNetDiscriminatorSN(3, num_feat=64, skip_connection=True).to(dev).train()
    cfg = joint_train.JointCfg.fern_lg_joint_l1_gan()
    with contextlib.redirect_stdout(sys.stderr):
        tr = joint_train.JointTrainer(model, net, cfg, dict(ck['render_kwargs'], render_depth=True, rand_bkgd=True), n_train_images=17, net_d=net_d,
                                      cri_perceptual=cri)
    g = torch.Generator(device=dev).manual_seed(5)

    def batch(i):
        r0, c0 = (37 * i) % (H - 64), (101 * i) % (W - 64)
        rays = [x[r0:r0 + 64, c0:c0 + 64].reshape(-1, 3).contiguous() for x in (ro, rd, vd)]
        return rays + [torch.rand([4096, 3], device=dev, generator=g), torch.rand([65536, 3], device=dev, generator=g), 64, 64]

    # two variants of ONE trainer: without the terms (what JointTrainer does when weight_pcp == 0: cri_perceptual is None) and with them
    VARIANTS = {'gan': None, 'gan_pcp_style': cri}
    times = {k: [] for k in VARIANTS}
    step = [args.step0]

    def one(name):
        tr.cri_perceptual = VARIANTS[name]
        step[0] += 1
        b = batch(step[0])
        return timed(lambda: tr.step(*b, global_step=step[0]))

    for _ in range(5):
        for name in VARIANTS:
            one(name)
    for _ in range(args.iters):
        for name in VARIANTS:
            times[name].append(one(name))
    out = {k: stats(v) for k, v in times.items()}
    out['with_minus_without_ms'] = stats([a - b for a, b in zip(times['gan_pcp_style'], times['gan'])])
    out['step0'] = args.step0
    print(json.dumps({'joint_iteration': out}), flush=True)


# ---- the module alone against the tensor library ----------------------------------------------------------------------------------
class EagerPerceptual(nn.Module):
    """The same network and losses from torch-ROCm eager operations, fp32 (the tensor-library partner of the comparison; not part of the package)."""

    def __init__(self, sd, lw, pw, sw):
        super().__init__()
        layers, cin = [], 3
        for n in sr_loss.NAMES[:sr_loss.NAMES.index('conv5_4') + 1]:
            if n.startswith('conv'):
                cout = sr_loss.CONV_SHAPES[n][0]
                layers.append(nn.Conv2d(cin, cout, 3, 1, 1))
                cin = cout
            elif n.startswith('relu'):
                layers.append(nn.ReLU(inplace=False))
            else:
                layers.append(nn.MaxPool2d(2, 2))
        self.net = nn.Sequential(*layers)
        self.net.load_state_dict({k[len('features.'):]: v for k, v in sd.items()})
        for p in self.net.parameters():
            p.requires_grad = False
        self.register_buffer('mean', torch.tensor(sr_loss.MEAN).view(1, 3, 1, 1))
        self.register_buffer('std', torch.tensor(sr_loss.STD).view(1, 3, 1, 1))
        self.taps = {sr_loss.NAMES.index(n): w for n, w in lw.items() if w != 0}
        self.pw, self.sw = pw, sw

    def feats(self, x):
        x = (x - self.mean) / self.std
        out = {}
        for i, m in enumerate(self.net):
            x = m(x)
            if i in self.taps:
                out[i] = x
        return out

    @staticmethod
    def gram(f):
        n, c, h, w = f.size()
        f = f.view(n, c, w * h)
        return f.bmm(f.transpose(1, 2)) / (c * h * w)

    def forward(self, x, gt):
        fx, fg = self.feats(x), self.feats(gt.detach())
        p = sum(torch.nn.functional.l1_loss(fx[i], fg[i]) * w for i, w in self.taps.items()) * self.pw
        s = sum(torch.nn.functional.l1_loss(self.gram(fx[i]), self.gram(fg[i])) * w for i, w in self.taps.items()) * self.sw
        return p, s


eager = EagerPerceptual(sd, LW, 0.5, 0.2).to(dev)
gen = torch.Generator(device=dev).manual_seed(9)
gt = torch.rand([1, 3, 256, 256], device=dev, generator=gen)
x = gt + 0.1 * torch.randn([1, 3, 256, 256], device=dev, generator=gen)


def module_pass(mod):
    xi = x.clone().requires_grad_(True)
    p, s = mod(xi, gt)
    (p + s).backward()
    return p, s, xi.grad


ph, sh, gh = module_pass(cri)
pe, se, ge = module_pass(eager)
agree = {'percep_hip': float(ph), 'percep_library': float(pe), 'style_hip': float(sh), 'style_library': float(se),
         'grad_rel_l2': float((gh - ge).norm() / ge.norm())}
t = {'hip': [], 'library': []}
for i in range(10 + args.iters):
    for name, mod in (('hip', cri), ('library', eager)):
        ms = timed(lambda: module_pass(mod))
        if i >= 10:
            t[name].append(ms)
res = {'hip': stats(t['hip']), 'library': stats(t['library']), 'library_minus_hip_ms': stats([a - b for a, b in zip(t['library'], t['hip'])]), 'agreement': agree,
       'useful_gflop': round(3 * 2 * 25.07, 1)}
print(json.dumps({'perceptual_style_forward_backward_256x256': res}), flush=True)

if args.layers:
    # the 3x3 kernels alone: 20 launches between two events; FLOP = 2 * images * pixels * cout * cin * 9
    rows = {}
    for name, cin, cout, hw in (('conv1_2', 64, 64, 256), ('conv2_1', 64, 128, 128), ('conv2_2', 128, 128, 128), ('conv3_1', 128, 256, 64), ('conv3_x', 256, 256, 64),
                                ('conv4_1', 256, 512, 32), ('conv4_x', 512, 512, 32), ('conv5_x', 512, 512, 16)):
        w = torch.randn([cout, cin, 3, 3], device=dev) / (9 * cin) ** 0.5
        b = torch.zeros([cout], device=dev)
        wf, wb = sr_loss.pack_weight(w, sr_loss.FWD), sr_loss.pack_weight(w, sr_loss.DGRAD)
        xin = torch.relu(torch.randn([2, hw, hw, cin], device=dev))
        gy = torch.randn([1, hw, hw, cout], device=dev)
        xt = xin.permute(0, 3, 1, 2).contiguous()
        flop2 = 2.0 * 2 * hw * hw * cout * cin * 9
        fns = {'forward_2_images': (lambda: sr_loss.conv3x3(xin, wf, b, cout), flop2),
               'dgrad_1_image': (lambda: sr_loss.conv3x3_dgrad(gy, wb, cin, mask=xin[:1]), flop2 / 2),
               'library_forward_2_images': (lambda: torch.nn.functional.conv2d(xt, w, b, 1, 1), flop2)}
        row = {}
        for k, (fn, flop) in fns.items():
            for _ in range(3):
                fn()
            ms = timed(lambda: [fn() for _ in range(20)]) / 20
            row[k] = {'us': round(ms * 1e3, 1), 'useful_tflops': round(flop / ms / 1e9, 1)}
        rows[f'{name} {cin}->{cout} {hw}x{hw}'] = row
    print(json.dumps({'conv3x3_layers': rows}), flush=True)
