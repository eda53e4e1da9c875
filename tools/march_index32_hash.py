"""sha1 of the fused marcher's outputs (rgb, depth, alphainv) on cases aimed at the 32-bit addressing, the DPP scans and the box test of the
geometry kernel's FAST instantiation (4k-nerf_amd/csrc/k4_march.hip: K4_IDX_OFF32, K4_IDX_DPP), under the CURRENT environment: the
library reads K4_DEBUG once while it loads, K4_DEBUG=17408 (16384 | 1024) forces the general instantiation of both kernels.
tests/test_march_index32_gpu.py runs this tool once per setting and wants equal hashes.
      python tools/march_index32_hash.py <case> [<case> ...]
Every case meets the FAST predicate (256 planes, interval 1, one launch, occupancy summary) and asserts its premise on the CPU before it marches:
  big24     a 282 x 238 x 256 grid (17.2 M voxels > 2^24, x and y no powers of two), content only in the x slabs from 274 on, and a 32 x 32 window of
            rays that runs through the slabs 276..281: every voxel and mask index a sample of the window forms is above 2^24, every density byte
            offset above 2^26 (asserted).  A 24-bit product or a wrapped 32-bit offset reads another voxel and changes the hash.
  scanlanes ONE bundle (an 8 x 8 tile) of rays along z through voxel centres of a 48 x 48 x 256 grid, the density set column by column so that the
            alpha-passing records per ray slot and depth quarter are known (counts_of): quarter 0 full on every ray (four full segments of 1024
            records), quarter 1 with exactly one record on slots 15, 16, 31, 32, 47, 48, 63 (the DPP row and half-wave boundaries), a full group (the
            8-bit field's maximum, 16) on slot 5, all 64 samples on slot 40 and none elsewhere, quarter 2 with a seeded 0..64 per slot, quarter 3
            with one record on slots 0 and 63.
  boxcert   a 16 x 16 view of the blob scene whose rows are: a camera's own rays; rays that leave / enter the box in the middle of a 16-sample
            group; rays that run exactly on xyz_min.x / xyz_max.y; rays entirely outside; one ray with an infinite and one with a NaN direction
            component.  These are the rays a per-group box certificate has to get right; the one that was tried is not in the tree (it measured
            slower: profiles/march_index32_boxcert_slower.patch) and this case is what a next attempt is held to."""
import hashlib, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import nerf4k_amd  # noqa: F401
from nerf4k_amd import scene
from nerf4k_amd.lib import dmpigo
import geom_deal_hash as G          # the scene helpers of the deal's cases (same directory)

KEYS = G.KEYS
BIG = (282, 238, 256)                                       # big24: the grid make_llff_checkpoint derives from BIG_VOXELS
BIG_VOXELS = 17_238_000
BIG_X0 = 274                                                # ... first x slab with content
SCAN_ALPHA = 0.002                                          # scanlanes: alpha of an "on" voxel (2.5 x the threshold; 64 of them leave T = 0.88)
ONE_REC = (15, 16, 31, 32, 47, 48, 63)


def _unit(d):
    return d / d.norm(dim=-1, keepdim=True)


# ---- big24 ---------------------------------------------------------------------------------------------------------------------------
def big_checkpoint():
    ck = scene.make_llff_checkpoint(seed=31, num_voxels=BIG_VOXELS, mpi_depth=256, n_blobs=8)
    d = ck['model_state_dict']['density.grid']
    assert tuple(d.shape[2:]) == BIG, d.shape
    d[:, :, :BIG_X0] = -30.0                                # alpha == 0 to fp32 in front of the last slabs
    d[:, :, BIG_X0:] += 9.0                                 # ... and the blobs' flanks above the threshold inside them
    G.remask(ck)
    return ck


def big_rays():
    """32 x 32 rays along z, inside x slabs 276..281 (x >= 1.262 for every sample), fanned a little so that they are not voxel aligned."""
    col = torch.arange(32, dtype=torch.float32).view(1, 32).expand(32, 32)
    row = torch.arange(32, dtype=torch.float32).view(32, 1).expand(32, 32)
    o = torch.stack([1.264 + col * (0.034 / 31), -1.0 + row * (2.0 / 31), torch.full((32, 32), -1.0)], -1)
    d = torch.stack([(col - 15.5) * 1e-4, (row - 15.5) * 3e-3, torch.full((32, 32), 2.0)], -1)
    return [o.reshape(-1, 3).contiguous(), d.reshape(-1, 3).contiguous(), _unit(d).reshape(-1, 3).contiguous()]


def big_premise(ck, rays):
    """Every in-box sample of the window: its density voxel (floor corner) and its mask voxel have a linear index above 2^24."""
    sd = ck['model_state_dict']
    lo, hi = sd['xyz_min'].double(), sd['xyz_max'].double()
    X, Y, Z = BIG
    t = (torch.arange(256, dtype=torch.float64) / 255).view(1, 256, 1)
    p = rays[0].double().view(-1, 1, 3) + rays[1].double().view(-1, 1, 3) * t
    inbox = ((p >= lo) & (p <= hi)).all(-1)
    u = (p - lo) / (hi - lo) * torch.tensor([X - 1, Y - 1, Z - 1], dtype=torch.float64)
    v = u.floor().long()
    vox = ((v[..., 0] * Y + v[..., 1]) * Z + v[..., 2])[inbox]
    m = u.round().long()
    mvox = ((m[..., 0] * Y + m[..., 1]) * Z + m[..., 2])[inbox]
    assert list(sd['mask_cache.mask'].shape) == list(BIG)
    assert int(inbox.sum()) > 1000 * 128 and int(vox.min()) > 2 ** 24 and int(mvox.min()) > 2 ** 24 and int(vox.min()) * 4 > 2 ** 26, \
        (int(inbox.sum()), int(vox.min()), int(mvox.min()))
    return int(vox.min())


def case_big24(h, dev):
    ck = big_checkpoint()
    rays = big_rays()
    lowest = big_premise(ck, rays)
    model, rk = G.model_of(ck, dev)
    out = G.march(model, [r.to(dev) for r in rays], 32, rk, h)
    seen = float((1 - out['alphainv_last']).sum())
    assert seen > 1.0, 'nothing was composited in the last slabs'
    return model, f'lowest_voxel_index={lowest}'


# ---- scanlanes -----------------------------------------------------------------------------------------------------------------------
def counts_of():
    """on[slot][plane]: the alpha-passing samples of the bundle by construction."""
    on = np.zeros((64, 256), dtype=bool)
    on[:, 0:64] = True                                      # quarter 0: every sample of every ray -- four full segments
    for r in ONE_REC:
        on[r, 64 + (r * 7) % 64] = True                     # quarter 1: one record, in a group (= a wave) that moves with the slot
    on[5, 80:96] = True                                     # ... one whole group: the 8-bit field's maximum
    on[40, 64:128] = True                                   # ... one ray with all four fields at the maximum
    g = np.random.default_rng(9)
    for r in range(64):                                     # quarter 2: 0..64 records, any planes
        n = int(g.integers(0, 65)) if r % 5 else 0
        on[r, 128 + g.permutation(64)[:n]] = True
    on[0, 200] = True; on[63, 255] = True                   # quarter 3: one record on the first and on the last slot
    return on


def slot_of_pixel(py, px):
    return py * 8 + (7 - px if py & 1 else px)              # the serpentine ray order inside a tile (k4_march.hip: ray_index)


def scan_checkpoint():
    ck = scene.make_llff_checkpoint(seed=37, **G.grid_of(256))
    sd, kw = ck['model_state_dict'], ck['model_kwargs']
    d, act = sd['density.grid'], sd['act_shift.grid'].reshape(-1)
    assert float(kw['voxel_size_ratio']) == 1.0 and SCAN_ALPHA > 2 * float(kw['fast_color_thres'])
    d.fill_(-30.0)
    sig = float(np.log(SCAN_ALPHA / (1 - SCAN_ALPHA)))      # interval 1: alpha = e / (1 + e)
    on = torch.from_numpy(counts_of())
    for r in range(64):
        xi, yi = 4 + 5 * (r % 8), 4 + 5 * (r // 8)          # the slot's voxel column and its 8 neighbours carry the same values
        col = torch.where(on[r], sig - act, torch.full_like(act, -30.0))
        d[0, 0, xi - 1:xi + 2, yi - 1:yi + 2, :] = col.view(1, 1, -1)
    G.remask(ck)
    return ck


def scan_rays(ck):
    sd = ck['model_state_dict']
    lo, hi = sd['xyz_min'], sd['xyz_max']
    X, Y = ck['model_state_dict']['density.grid'].shape[2:4]
    o = torch.zeros(8, 8, 3)
    for py in range(8):
        for px in range(8):
            r = slot_of_pixel(py, px)
            xi, yi = 4 + 5 * (r % 8), 4 + 5 * (r // 8)
            o[py, px] = torch.tensor([float(lo[0]) + xi * float(hi[0] - lo[0]) / (X - 1), float(lo[1]) + yi * float(hi[1] - lo[1]) / (Y - 1), -1.0])
    d = torch.tensor([0.0, 0.0, 2.0]).expand(64, 3).contiguous()
    return [o.reshape(-1, 3).contiguous(), d, _unit(d).contiguous()]


def case_scanlanes(h, dev):
    ck = scan_checkpoint()
    model, rk = G.model_of(ck, dev)
    out = G.march(model, [r.to(dev) for r in scan_rays(ck)], 8, rk, h)
    # T after every "on" sample of a ray, in closed form: the rays' alphainv must follow the constructed counts
    n_on = torch.from_numpy(counts_of().sum(1)).double()
    want = torch.zeros(64, dtype=torch.float64)
    for py in range(8):
        for px in range(8):
            want[py * 8 + px] = (1 - SCAN_ALPHA) ** float(n_on[slot_of_pixel(py, px)])
    err = float((out['alphainv_last'].cpu().double() - want).abs().max())
    assert err < 2e-4, f'alphainv does not follow the constructed record counts: {err}'
    return model, f'records={int(n_on.sum())}'


# ---- boxcert -------------------------------------------------------------------------------------------------------------------------
def box_rays(ck):
    sd = ck['model_state_dict']
    lo, hi = sd['xyz_min'], sd['xyz_max']
    o, d, v = [x.reshape(16, 16, 3).cpu().clone() for x in G.rays_of(16, 16, 3, torch.device('cpu'))]
    m = torch.arange(1, 17, dtype=torch.float32)
    tc = (16 * m + 8) / 255                                 # the crossing falls on sample 16 m + 8: the middle of group m
    for row, (ox, sgn) in ((4, (1.0, 1.0)), (5, (-1.6, 1.0)), (10, (-1.0, -1.0))):      # leave through x_max / enter through x_min / leave through x_min
        o[row, :, 0] = ox; d[row, :, 0] = sgn * 0.3 / tc
    o[6, :, 0] = lo[0]; d[6, :, 0] = 0.0                   # every sample exactly on xyz_min.x
    o[7, :, 1] = hi[1]; d[7, :, 1] = 0.0                   # ... on xyz_max.y
    o[8, :, 0] = 2.0; d[8, :, 0] = 0.0                     # entirely outside
    d[9, 0, 0] = float('inf'); d[9, 1, 1] = float('nan')
    v = torch.where(torch.isfinite(d).all(-1, keepdim=True), _unit(torch.where(torch.isfinite(d), d, torch.zeros_like(d))), torch.tensor([0.0, 0.0, 1.0]))
    return [x.reshape(-1, 3).contiguous() for x in (o, d, v)]


def box_premise(ck, rays):
    sd = ck['model_state_dict']
    lo, hi = sd['xyz_min'], sd['xyz_max']
    t = (torch.arange(256, dtype=torch.float32) / 255).view(1, 256, 1)
    p = torch.addcmul(rays[0].view(-1, 1, 3), rays[1].view(-1, 1, 3), t)
    inbox = ~((lo > p) | (hi < p)).any(-1)                  # stage A's closed-box expression (NaN passes)
    inbox = inbox.view(16, 16, 256)
    px = p.view(16, 16, 256, 3)[..., 0]
    inx = ~((lo[0] > px) | (hi[0] < px))
    flips = (inx[..., 1:] != inx[..., :-1])
    for row in (4, 5, 10):                                  # the x test of these rays first flips at a sample that is no multiple of 16
        k = flips[row, :15].float().argmax(-1) + 1
        assert bool((flips[row, :15].sum(-1) >= 1).all()) and bool((k % 16 != 0).all()), (row, k)
    assert bool(inbox[6].all()) and bool(inbox[7].all()) and not bool(inbox[8].any())
    assert bool((p.view(16, 16, 256, 3)[6, :, :, 0] == lo[0]).all()) and bool((p.view(16, 16, 256, 3)[7, :, :, 1] == hi[1]).all())
    assert not bool(torch.isfinite(rays[1].view(16, 16, 3)[9, :2]).all(-1).any())


def case_boxcert(h, dev):
    ck = scene.make_llff_checkpoint(**G.grid_of(256))
    rays = box_rays(ck)
    box_premise(ck, rays)
    model, rk = G.model_of(ck, dev)
    out = G.march(model, [r.to(dev) for r in rays], 16, rk, h)
    ainv = out['alphainv_last'].cpu().view(16, 16)
    assert bool((ainv[8] == 1).all()), 'a ray outside the box met a sample'
    assert float((1 - ainv[:8]).sum()) > 1.0, 'nothing was composited'
    return model, 'rows=camera,leave,enter,on_min,on_max,outside,inf_nan'


CASES = {'big24': case_big24, 'scanlanes': case_scanlanes, 'boxcert': case_boxcert}
if __name__ == '__main__':
    dmpigo.DEPTH_SPLIT = False                              # one geometry launch whatever the scene: the FAST predicate
    dev = torch.device('cuda', 0)
    with torch.no_grad():
        for case in (sys.argv[1:] or list(CASES)):
            h = hashlib.sha1()
            model, note = CASES[case](h, dev)
            split = int(model._k4_cache().get('dsplit', 0))
            interval = float(1.0 * model.voxel_size_ratio)
            assert split == 0 and interval == 1.0 and int(model.mpi_depth) == 256, (split, interval, int(model.mpi_depth))
            print('MARCH_INDEX32_HASH', case, h.hexdigest(), f'interval={interval:g}', f'depth_split={split}', note, flush=True)
            del model
            torch.cuda.empty_cache()
