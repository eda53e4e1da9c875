"""ms per LPIPS-VGG score of a frame pair (lib/utils.frame_lpips: lib/lpips.LPIPS on csrc/k4_vgg.hip + csrc/k4_lpips.hip) against the same network written
in torch-ROCm eager fp32 operations (F.conv2d / F.max_pool2d and the package's normalize_tensor / spatial_average expressions), ALTERNATED call by call
in one process, on seeded weights.  GPU box.

    python tools/lpips_time.py [--pairs 200] [--budget-s 120] [--only 756x1008] [--out profiles/lpips_time.md] [--index profiles/INDEX.md]

Frames: 756 x 1008 and 3024 x 4032, planar, seeded synthetic (a frame and a noisy copy of it).  Every figure is the time between two device events around
one call, after a warm-up of both arms.  Where `--pairs` pairs would not fit `--budget-s` seconds per frame size, fewer pairs are run and the count is
written.  Per layer: the HIP launch alone on the activations of that level (device events, median of `--layer-calls`), its useful FLOP (2 * 9 * cin * cout per
output pixel, both images) over that time.  Peak working set: torch's peak allocated bytes over one call, above what was allocated in front of it.
Writes the markdown report to --out, one line to --index (when it is not there yet), and prints one JSON line per frame size."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
import nerf4k_amd  # noqa: F401,E402
from nerf4k_amd.lib import lpips, sr_loss, utils  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--pairs', type=int, default=200)
ap.add_argument('--budget-s', type=float, default=120.0, help='seconds of alternated calls per frame size')
ap.add_argument('--layer-calls', type=int, default=10)
ap.add_argument('--only', default=None)
ap.add_argument('--out', default=os.path.join('profiles', 'lpips_time.md'))
ap.add_argument('--index', default=os.path.join('profiles', 'INDEX.md'))
args = ap.parse_args()
dev = torch.device('cuda', 0)
SEED = 11
sd = lpips.seeded_lpips_state_dict(SEED)
utils.load_lpips_weights(sd)
sd_dev = {k: v.to(dev) for k, v in sd.items()}
LAYERS = lpips.conv_layers()


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def stats(v):
    v = sorted(v)
    return {'median_ms': round(statistics.median(v), 4), 'p10_ms': round(v[len(v) // 10], 4), 'p90_ms': round(v[len(v) * 9 // 10], 4), 'n': len(v)}


def fmt(s):
    return f"{s['median_ms']:.3f} ({s['p10_ms']:.3f} .. {s['p90_ms']:.3f})"


@torch.no_grad()
def eager(gt, pred):
    """lpips.LPIPS(net='vgg')(gt, pred, normalize=True) in eager fp32 tensor operations, both images as a batch of two -> device scalar."""
    x = torch.stack([gt, pred]) * 2 - 1
    x = (x - sd_dev['scaling_layer.shift']) / sd_dev['scaling_layer.scale']
    val, s_prev = None, 0
    for s, i, _, _ in LAYERS:
        if s != s_prev and s > 1:
            x = F.max_pool2d(x, 2, 2)
        x = F.relu(F.conv2d(x, sd_dev[f'net.slice{s}.{i}.weight'], sd_dev[f'net.slice{s}.{i}.bias'], 1, 1))
        s_prev = s
        if i in (2, 7, 14, 21, 28):                      # the slice's last layer: its head
            n = x / (torch.sqrt(torch.sum(x ** 2, dim=1, keepdim=True)) + 1e-10)
            d = (n[0:1] - n[1:2]) ** 2
            t = F.conv2d(d, sd_dev[f'lin{s - 1}.model.1.weight']).mean([2, 3])
            val = t if val is None else val + t
    return val.reshape(())


def layer_times(H, W):
    """[(name, cin, cout, h, w, median ms of the HIP launch, useful TFLOP/s)] on seeded activations of each level's size."""
    m = utils.__LPIPS__['vgg']
    P = m.k4_operands(dev)
    rows, h, w, g = [], H, W, torch.Generator().manual_seed(1)
    mean, std = P['norm'][True]
    for k, (s, i, cout, cin) in enumerate(LAYERS):
        last = i in (2, 7, 14, 21)
        op = P['ops'][k]
        if i == 0:
            x0, x1 = torch.rand([3, h, w], generator=g).to(dev), torch.rand([3, h, w], generator=g).to(dev)
            fn = lambda: sr_loss.conv1_1(x0, x1, mean, std, op['w'], op['b'])          # noqa: E731
        else:
            x = torch.relu(torch.randn([2, h, w, cin], device=dev))
            fn = lambda: sr_loss.conv3x3(x, op['fwd'], op['b'], cout, relu=True, keep_relu=True, pool=last)          # noqa: E731
        fn()
        ms = statistics.median(timed(fn)[0] for _ in range(args.layer_calls))
        flop = 2.0 * 9 * cin * cout * h * w * 2
        rows.append((f'slice{s}.{i}' + (' + pool' if last else ''), cin, cout, h, w, ms, flop / (ms * 1e-3) / 1e12))
        x = x0 = x1 = None
        if last:
            h, w = h // 2, w // 2
    # the five heads on their levels
    h, w = H, W
    for k, c in enumerate(lpips.CHNS):
        f = torch.relu(torch.randn([2, h, w, c], device=dev))
        taps = torch.empty([5], dtype=torch.float64, device=dev)
        fn = lambda: lpips.head(f, P['lin'][k], taps, k)          # noqa: E731
        fn()
        ms = statistics.median(timed(fn)[0] for _ in range(args.layer_calls))
        rows.append((f'head {k}', c, 1, h, w, ms, None))
        f = None
        h, w = h // 2, w // 2
    return rows


results, report = [], []
for H, W in ((756, 1008), (3024, 4032)):
    name = f'{H}x{W}'
    if args.only and args.only != name:
        continue
    g = torch.Generator().manual_seed(H + W)
    gt_cpu = torch.rand(3, H, W, generator=g)
    pred = (gt_cpu + 0.05 * torch.randn(3, H, W, generator=g)).clamp(0, 1).to(dev)
    gt = gt_cpu.to(dev)

    def hip():
        return utils.frame_lpips(pred, gt)

    def lib():
        return eager(gt, pred)

    for _ in range(2):
        hip()
        lib()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    t_hip, got = timed(hip)
    peak_hip = torch.cuda.max_memory_allocated(dev) - base
    torch.cuda.reset_peak_memory_stats(dev)
    t_lib, got_lib = timed(lib)
    peak_lib = torch.cuda.max_memory_allocated(dev) - base
    same_bits = bool(torch.equal(hip(), got))
    pairs = max(5, min(args.pairs, int(args.budget_s * 1e3 / (t_hip + t_lib))))
    hip_ms, lib_ms = [], []
    for _ in range(pairs):
        hip_ms.append(timed(hip)[0])
        lib_ms.append(timed(lib)[0])
    res = {'frame': name, 'H': H, 'W': W, 'pairs': pairs, 'hip': stats(hip_ms), 'torch_eager_fp32': stats(lib_ms),
           'torch_minus_hip': stats([b - a for a, b in zip(hip_ms, lib_ms)]), 'value_hip': float(got), 'value_torch': float(got_lib),
           'hip_over_torch_minus_1': float(got.double() / got_lib.double() - 1), 'two_calls_same_bits': same_bits,
           'peak_bytes_hip': int(peak_hip), 'peak_bytes_torch': int(peak_lib)}
    rows = layer_times(H, W)
    res['layers'] = [{'layer': r[0], 'cin': r[1], 'cout': r[2], 'h': r[3], 'w': r[4], 'ms': round(r[5], 4), 'tflops': None if r[6] is None else round(r[6], 1)} for r in rows]
    print(json.dumps(res), flush=True)
    results.append(res)
    slower = res['hip']['median_ms'] > res['torch_eager_fp32']['median_ms']
    report += [f'## {name}', '',
               f'{pairs} alternated pairs.  One call, ms: median (p10 .. p90).', '',
               '| HIP call (`frame_lpips`) | torch-ROCm eager fp32 | paired difference torch − HIP | value HIP | value torch | HIP / torch − 1 | two HIP calls give the same bits | peak working set HIP | peak working set torch |',
               '|---|---|---|---|---|---|---|---|---|',
               f"| {fmt(res['hip'])} | {fmt(res['torch_eager_fp32'])} | {fmt(res['torch_minus_hip'])} | {res['value_hip']:.9g} | {res['value_torch']:.9g} | "
               f"{res['hip_over_torch_minus_1']:.2e} | {'yes' if same_bits else 'NO'} | {peak_hip / 2**30:.2f} GiB | {peak_lib / 2**30:.2f} GiB |", '',
               ('**The HIP path is SLOWER than the eager formulation at this size.**' if slower else 'The HIP path is faster than the eager formulation at this size.'), '',
               f'Per launch (median of {args.layer_calls}, seeded activations of the level\'s size, both images; useful FLOP = 2 * 9 * cin * cout per output pixel):', '',
               '| launch | cin | cout | h x w | ms | useful TFLOP/s |', '|---|---|---|---|---|---|']
    report += [f'| {r[0]} | {r[1]} | {r[2]} | {r[3]} x {r[4]} | {r[5]:.3f} | {"" if r[6] is None else "%.1f" % r[6]} |' for r in rows]
    report += ['', f'Sum of the launches: {sum(r[5] for r in rows):.3f} ms.', '']
    gt = pred = None
    torch.cuda.empty_cache()

head = ['# LPIPS-VGG frame scoring (`frame_lpips`: `csrc/k4_vgg.hip` + `csrc/k4_lpips.hip`): times', '',
        f'One MI355X, one process.  Command: `python tools/lpips_time.py --pairs {args.pairs} --budget-s {args.budget_s:g}`.  Device events around one call,',
        'both arms warmed up; the HIP call `lib/utils.frame_lpips` and the same network in torch-ROCm eager fp32 operations (`F.conv2d`, `F.max_pool2d`, the package\'s',
        f'`normalize_tensor` / `spatial_average` expressions, both frames as a batch of two) alternated call by call; seeded weights (`seeded_lpips_state_dict({SEED})`), seeded synthetic frames',
        '(a frame and a copy with 0.05 sigma noise).  The matrix products of the HIP path are the exact 3-term bf16 split (six matrix instructions per fp32-equivalent product);',
        'no speed figure is a merge condition.', '']
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, 'w') as fh:
    fh.write('\n'.join(head + report))
line = ('`lpips_time.md`: LPIPS-VGG scoring of a frame pair (`lib/utils.frame_lpips`) on an MI355X at 756 x 1008 and 3024 x 4032 against the same network in eager torch-ROCm fp32 '
        'operations, alternated, HIP events: call times (median, p10 / p90, paired difference), per-launch useful TFLOP/s, peak working set, the difference of the two values, '
        'and whether two calls give the same bits (`tools/lpips_time.py`).')
have = open(args.index).read() if os.path.exists(args.index) else ''
if '`lpips_time.md`' not in have:
    with open(args.index, 'a') as fh:
        fh.write(('\n' if have and not have.endswith('\n\n') else '') + '## LPIPS\n\n' + line + '\n')
