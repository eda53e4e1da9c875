"""Share of the 16-sample groups the geometry kernel's probe (stage P) keeps on the bench scene, emulated in torch with the kernel's box rule
(per-axis index interval of the end samples, clamped; <= 2 x 2 cells of 8 x 8 voxels and <= 32 planes, wider boxes kept unseen; cell-level
occupancy of the live mask): the shipped form (two end samples per group) and the five-boundary-sample form of
profiles/geom_fast_probe5_minw6.patch (group j spans samples [ka + 16 j, ka + 16 (j + 1)], the last one clipped to the quarter).  torch does not
fuse a*b+c, so an index can differ from the kernel's in the last place at a rounding boundary: a statistic, not a bit-exact replay.  GPU box."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
import nerf4k_amd  # noqa: F401
from nerf4k_amd import scene
from nerf4k_amd.lib import utils, dvgo
dev = torch.device('cuda', 0)
with torch.no_grad():
    ck = scene.make_llff_checkpoint()
    model = utils.model_from_checkpoint_dict(ck).to(dev).eval()
    rk = ck['render_kwargs']
    interval = float(rk['stepsize'] * model.voxel_size_ratio)
    model._k4_grid(act_shift_grid=model.act_shift.grid, live=(0.0, interval))
    live = model._k4_cache()['live'][0].bool()
    MX, MY, MZ = live.shape[-3:]
    live = live.reshape(MX, MY, MZ)
    mc = model.mask_cache
    ms, mt = mc.xyz2ijk_scale.float().to(dev), mc.xyz2ijk_shift.float().to(dev)
    # cell-level occupancy [cx][cy][z] and its prefix sum along z
    pad = F.pad(live.permute(2, 0, 1).float()[None], (0, (-MY) % 8, 0, (-MX) % 8))
    cell = F.max_pool2d(pad, 8)[0].permute(1, 2, 0)                       # [CX][CY][MZ]
    CX, CY = cell.shape[:2]
    cz = F.pad(cell.cumsum(2), (1, 0)).contiguous()                       # [CX][CY][MZ+1]
    H, W = scene.LLFF_HW
    N = int((model.mpi_depth - 1) / rk['stepsize']) + 1
    assert N == 256
    tk = torch.arange(N, device=dev, dtype=torch.float32) / float(N - 1)

    def idx_of(o, d, k):                                                  # [R, G] sample index -> 3 x [R, G] mask indices, C round()
        t = tk[k]
        out = []
        for a in range(3):
            v = (d[:, a:a + 1] * t + o[:, a:a + 1]) * ms[a] + mt[a]
            out.append((torch.sign(v) * torch.floor(v.abs() + 0.5)).long())
        return out

    def kept(ia, ib):
        lo = [torch.minimum(a, b).clamp_min(0) for a, b in zip(ia, ib)]
        hi = [torch.minimum(torch.maximum(a, b), torch.full_like(a, n - 1)) for a, b, n in zip(ia, ib, (MX, MY, MZ))]
        empty = (lo[0] > hi[0]) | (lo[1] > hi[1]) | (lo[2] > hi[2])
        cx0, cy0 = lo[0] >> 3, lo[1] >> 3
        sx, sy = (hi[0] >> 3) - cx0, (hi[1] >> 3) - cy0
        wide = (sx > 1) | (sy > 1) | (hi[2] - lo[2] >= 32)
        z0, z1 = lo[2].clamp(0, MZ - 1), hi[2].clamp(0, MZ - 1)
        any_ = torch.zeros_like(empty)
        for ax in (0, 1):
            for ay in (0, 1):
                use = (sx >= ax) & (sy >= ay)
                cx, cy = (cx0 + ax).clamp(0, CX - 1), (cy0 + ay).clamp(0, CY - 1)
                base = (cx * CY + cy) * (MZ + 1)
                flat = cz.reshape(-1)
                any_ |= use & ((flat[base + z1 + 1] - flat[base + torch.minimum(z0, z1)]) > 0)
        return ~empty & (wide | any_)

    tot = k2 = k5 = 0
    for f in (3, 11):
        ro, rd, _ = [x.reshape(-1, 3).contiguous() for x in dvgo.get_rays_of_a_view(H, W, scene.LLFF_K, torch.from_numpy(scene.llff_spiral_poses()[f]).to(dev), True, False, False, False)]
        for s in range(0, ro.shape[0], 1 << 17):
            o, d = ro[s:s + (1 << 17)], rd[s:s + (1 << 17)]
            g = torch.arange(16, device=dev)
            ka, kb = (16 * g)[None].expand(o.shape[0], 16), (16 * g + 15)[None].expand(o.shape[0], 16)
            k2 += int(kept(idx_of(o, d, ka), idx_of(o, d, kb)).sum())
            kb5 = torch.minimum(ka + 16, (ka // 64) * 64 + 63)
            k5 += int(kept(idx_of(o, d, ka), idx_of(o, d, kb5)).sum())
            tot += o.shape[0] * 16
print(f'PROBE_SHARE bench scene, frames 3 and 11, {tot} groups: two end samples keep {k2} = {100 * k2 / tot:.2f} %; five boundary samples keep {k5} = {100 * k5 / tot:.2f} %')
