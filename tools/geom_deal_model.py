"""Host-only model of how a bundle's work falls on the four waves of a geometry workgroup (k4_geom3_kernel, FAST instantiation): a replay of
stage P (which 16-sample groups are kept) and stage A (which samples pass the live mask) on the bench scene, frame 3 of the spiral, every third
8 x 8 tile in x and y.  Needs no GPU.      python tools/geom_deal_model.py [tile stride, default 3]

It compares three deals of the (ray, group) pairs: depth QUARTERS (group G to wave G >> 2: the general instantiation), a plain INTERLEAVE
(G & 3) and the DEAL of k4_geom_deal.h ((G + (r >> 4)) & 3), and prints per workgroup the mean wave and the heaviest wave of each.

It is a statistic, not a bit-exact replay:
  * the LIVE MASK IS APPROXIMATED in torch as mask_cache AND (a 3 x 3 x 3 neighbourhood of the voxel holds a density-grid point whose alpha is
    above fast_color_thres) -- the kernel's live mask is built by k4_build_live_mask from cell maxima;
  * a group counts as kept when one of its 16 samples falls into an 8 x 8 (x, y) cell and z plane with a live voxel; the kernel tests the box
    spanned by the group's two end samples against the same summary, which keeps a few groups more."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
import nerf4k_amd  # noqa: F401
from nerf4k_amd import scene
from nerf4k_amd.lib import dvgo

GRP, CELL = 16, 8


def main():
    stride = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    torch.manual_seed(0)
    ck = scene.make_llff_checkpoint()
    sd, kw = ck['model_state_dict'], ck['model_kwargs']
    n = int(kw['mpi_depth'])
    thres = float(kw['fast_color_thres'])
    alpha = scene._raw2alpha(sd['density.grid'] + sd['act_shift.grid'], 0, kw['voxel_size_ratio'])
    mask = sd['mask_cache.mask']
    assert list(mask.shape) == list(alpha.shape[2:]), 'the model takes the mask on the density grid'
    live = mask & (F.max_pool3d(alpha, kernel_size=3, padding=1, stride=1)[0, 0] > thres)
    X, Y, Z = live.shape
    cells = F.max_pool3d(live[None, None].float(), kernel_size=(CELL, CELL, 1), stride=(CELL, CELL, 1), ceil_mode=True)[0, 0] > 0
    scale, shift = sd['mask_cache.xyz2ijk_scale'].float(), sd['mask_cache.xyz2ijk_shift'].float()
    xyz_min, xyz_max = sd['xyz_min'].float(), sd['xyz_max'].float()

    H, W = scene.LLFF_HW
    ro, rd, _ = dvgo.get_rays_of_a_view(H, W, scene.LLFF_K, torch.from_numpy(scene.llff_spiral_poses()[3]), True, False, False, False)
    ty, tx = torch.arange(0, (H + 7) // 8, stride), torch.arange(0, (W + 7) // 8, stride)
    n_frame = 4 * ((H + 15) // 16) * ((W + 15) // 16)                  # bundles of the frame: workgroup tiles of 16 x 16 pixels, four bundles each
    # ray slots of a bundle: 8 rows of 8 pixels (the serpentine order inside a row does not change a slot's 16-ray subset r >> 4 = row >> 1)
    py = (ty[:, None, None, None] * 8 + torch.arange(8)[None, None, :, None]).expand(len(ty), len(tx), 8, 8)
    px = (tx[None, :, None, None] * 8 + torch.arange(8)[None, None, None, :]).expand(len(ty), len(tx), 8, 8)
    ok = (px < W) & (py < H)
    px, py = px.clamp(max=W - 1), py.clamp(max=H - 1)
    o, d = ro[py, px], rd[py, px]                                        # [ty, tx, 8, 8, 3]
    nb = len(ty) * len(tx)
    o, d, ok = o.reshape(nb, 64, 1, 3), d.reshape(nb, 64, 1, 3), ok.reshape(nb, 64, 1)
    t = (torch.arange(n, dtype=torch.float32) / (n - 1)).view(1, 1, n, 1)
    kept = torch.zeros(nb, 64, n // GRP, dtype=torch.bool)
    nlive = torch.zeros(nb, 64, n // GRP)
    for b0 in range(0, nb, 128):                                         # in slabs of bundles: [128, 64, 256, 3] points at a time
        s = slice(b0, b0 + 128)
        p = o[s] + d[s] * t
        inb = ((p >= xyz_min) & (p <= xyz_max)).all(-1) & ok[s]
        q = p * scale + shift
        ijk = torch.where(q >= 0, torch.floor(q + 0.5), torch.ceil(q - 0.5)).long()      # C round(): half away from zero
        inb &= ((ijk >= 0) & (ijk < torch.tensor([X, Y, Z]))).all(-1)
        i, j, k = [ijk[..., a].clamp(0, m - 1) for a, m in enumerate((X, Y, Z))]
        lv = live[i, j, k] & inb
        cl = cells[i // CELL, j // CELL, k] & inb
        kept[s] = cl.view(-1, 64, n // GRP, GRP).any(-1)
        nlive[s] = (lv & kept[s].repeat_interleave(GRP, dim=-1)).view(-1, 64, n // GRP, GRP).sum(-1).float()

    G = torch.arange(n // GRP).view(1, 1, -1)
    skew = (torch.arange(64) >> 4).view(1, 64, 1)
    deals = {'quarters (today)': (G >> 2).expand(nb, 64, -1), 'plain interleave': (G & 3).expand(nb, 64, -1), 'proposed deal': ((G + skew) & 3).expand(nb, 64, -1)}
    print(f'bench scene, frame 3, one 8 x 8 tile in {stride} in x and y: {nb} of {n_frame} bundles.  THE LIVE MASK IS APPROXIMATED (see the tool\'s header): a statistic, not a replay.')
    print(f'kept groups {100 * kept.float().mean():.1f} % of all; live-mask-passing samples, scaled to the frame: {nlive.sum() * n_frame / nb / 1e6:.2f} M')
    rows = {'stage-A items (4 entries x 16 samples)': [], 'stage-A byte-fetch round trips (4 items each)': [], 'live-mask-passing samples (stage B input)': []}
    cols = []
    for name, wave in deals.items():
        ent = torch.stack([(kept & (wave == w)).sum((1, 2)).float() for w in range(4)], 1)          # [nb, 4] entries per wave
        lv = torch.stack([(nlive * (wave == w)).sum((1, 2)) for w in range(4)], 1)
        per = {'stage-A items (4 entries x 16 samples)': ent / 4, 'stage-A byte-fetch round trips (4 items each)': torch.ceil(ent / 16),
               'live-mask-passing samples (stage B input)': lv}
        if not cols:
            cols.append('mean wave')
            for r in rows:
                rows[r].append(float(per[r].mean()))
        cols.append('heaviest wave, ' + name)
        for r in rows:
            rows[r].append(float(per[r].max(1).values.mean()))
    print('| per workgroup | ' + ' | '.join(cols) + ' |')
    print('|---' * (len(cols) + 1) + '|')
    for r, v in rows.items():
        print(f'| {r} | ' + ' | '.join(f'{x:.2f}' if x < 100 else f'{x:.0f}' for x in v) + ' |')


if __name__ == '__main__':
    with torch.no_grad():
        main()
