"""The 'patch_inmask' ray sampler on the GPU: the one-launch hit test (k4_hit_coarse_geo) gives the bits of the staged ``hit_coarse_geo``, the per-tile
counts (k4_patch_hit_counts) are the sums of the mask over ``patch_gen``'s index arrays, and ``get_training_rays_in_maskcache_sampling_sr`` keeps the
tiles and draws the sequence the reference's own function does (tests/golden/patch_inmask.npz, made by tests/gen_patch_inmask_golden.py).

Tolerances: everything is compared exactly (``torch.equal`` / integer equality) except the per-tile counts against the golden's: the golden is the CPU
oracle's, which may differ from the GPU sampler on a ray whose sample sits on a cell boundary (tests/test_march_gpu.py allows 4 such rays in 6,720); the
golden was chosen with no count within 32 of the 2048 bar, so counts within 32 leave the selection exact."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import nerf4k_amd  # noqa: F401
from nerf4k_amd import scene
from nerf4k_amd.lib import utils, dvgo as D, grid as kgrid
from helpers import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def G():
    z = np.load(os.path.join(GOLDEN, 'patch_inmask.npz'), allow_pickle=False)
    return {k: z[k] for k in z.files}


def _bump(t):
    torch.autograd.graph.increment_version(t)


@pytest.fixture(scope='module')
def S(G):
    """The golden's scene on the device: model (mask cache carved as the generator did), render kwargs, the three views' inputs, and -- computed once, left
    unchanged -- the staged hit masks of the three views."""
    ck = scene.make_lego_checkpoint(seed=int(G['seed']), num_voxels=36 ** 3)
    model = utils.model_from_checkpoint_dict(ck).cuda().eval()
    model.mask_cache.mask[:int(G['carve_x'])] = False
    _bump(model.mask_cache.mask)
    H, W = (int(v) for v in G['hw'])
    K = scene.lego_K(H, W)
    n = len(G['thetas'])
    poses = torch.stack([torch.as_tensor(scene.lego_pose(theta_deg=float(t))[:3, :4], dtype=torch.float32) for t in G['thetas']]).cuda()
    imgs = torch.rand([n, H, W, 3], generator=torch.Generator().manual_seed(5)).cuda()
    rk = dict(ck['render_kwargs'])
    args = (imgs, poses, np.array([[H, W]] * n), np.stack([K] * n), False, rk['inverse_y'], rk['flip_x'], rk['flip_y'])
    _, ro, rd, vd, _ = D.get_training_rays(*args)
    staged = torch.stack([model.hit_coarse_geo(rays_o=ro[i], rays_d=rd[i], **rk) for i in range(n)])
    return dict(ck=ck, model=model, rk=rk, args=args, H=H, W=W, n=n, ro=ro, rd=rd, vd=vd, imgs=imgs, staged=staged)


def _with_mask_of(S, shape, seed=0):
    """A model of the golden's scene whose mask cache has another resolution than the density grid: the scene's mask resampled (nearest), one x half cleared."""
    model = utils.model_from_checkpoint_dict(S['ck']).cuda().eval()
    src = model.mask_cache.mask.float()[None, None]
    m = F.interpolate(src, size=tuple(shape), mode='nearest')[0, 0] > 0.5
    m[: shape[0] // 2] = False
    model.mask_cache = kgrid.MaskGrid(path=None, mask=m.cpu(), xyz_min=model.xyz_min.cpu(), xyz_max=model.xyz_max.cpu()).cuda()
    assert list(model.mask_cache.mask.shape) == list(shape)
    return model


def test_hit_equals_staged_on_the_golden_views(S, G):
    model, rk = S['model'], S['rk']
    hit = model.k4_hit_coarse_geo(rays_o=S['ro'], rays_d=S['rd'], **rk)            # all views in one call
    assert hit.dtype == torch.bool and hit.shape == (S['n'], S['H'], S['W'])
    assert torch.equal(hit, S['staged'])
    frac = float(hit.float().mean())
    assert 0.2 < frac < 0.8, frac                                                  # a real mix of hits and misses
    want = np.unpackbits(G['hit_bits'])[:hit.numel()].reshape(hit.shape).astype(bool)
    differ = int((hit.cpu().numpy() != want).sum())
    print(f'hit fraction {frac:.3f}; rays that differ from the CPU oracle: {differ} of {hit.numel()}')
    for i in range(S['n']):                                                        # and view by view, as a caller with one view issues it
        assert torch.equal(model.k4_hit_coarse_geo(rays_o=S['ro'][i], rays_d=S['rd'][i], **rk), S['staged'][i])


def test_hit_on_a_noncontiguous_view_with_a_ragged_ray_count(S):
    model, rk = S['model'], S['rk']
    H, W = 37, 106
    ro, rd, _ = D.get_rays_of_a_view(H, W, scene.lego_K(H, W), torch.as_tensor(scene.lego_pose(theta_deg=75.)[:3, :4]).cuda(), False,
                                     rk['inverse_y'], rk['flip_x'], rk['flip_y'])
    ro, rd = ro[:, ::2], rd[:, ::2]                                                # [37, 53, 3]: 1961 rays, no multiple of 64, strided
    assert ro.shape == (37, 53, 3) and not ro.is_contiguous() and not rd.is_contiguous()
    hit = model.k4_hit_coarse_geo(rays_o=ro, rays_d=rd, **rk)
    want = model.hit_coarse_geo(rays_o=ro, rays_d=rd, **rk)
    assert hit.shape == (37, 53) and hit.dtype == torch.bool and torch.equal(hit, want)
    assert 0 < int(hit.sum()) < hit.numel()


@pytest.mark.parametrize('mask_size', [[33, 29, 23], [77, 71, 90]])
@pytest.mark.parametrize('stepsize', [0.5, 1.0])
def test_hit_with_a_mask_coarser_and_finer_than_the_density_grid(S, mask_size, stepsize):
    model = _with_mask_of(S, mask_size)
    rk = dict(S['rk'], stepsize=stepsize)
    ro, rd = S['ro'][1, 20:150:1, 7:200], S['rd'][1, 20:150, 7:200]               # 130 x 193 rays of the second view
    hit = model.k4_hit_coarse_geo(rays_o=ro, rays_d=rd, **rk)
    want = model.hit_coarse_geo(rays_o=ro, rays_d=rd, **rk)
    assert torch.equal(hit, want)
    assert 0 < int(hit.sum()) < hit.numel()


def _hand_made_rays(model):
    mn, mx = model.xyz_min.cpu(), model.xyz_max.cpu()
    c, h = (mn + mx) / 2, (mx - mn) / 2
    o, d = [], []

    def ray(origin, direction):
        o.append(torch.as_tensor(origin, dtype=torch.float32))
        d.append(torch.as_tensor(direction, dtype=torch.float32))

    # zero direction components (the 1e-6 substitution): one and two
    ray(c + h * torch.tensor([-2.5, 0.1, 0.2]), [1., 0., 0.3])
    ray(c + h * torch.tensor([-2.5, 0.1, 0.2]), [1., 0., 0.])
    ray(c + h * torch.tensor([0.3, 2.5, -0.4]), [0., -2., 0.])
    ray(c + h * torch.tensor([0.3, -0.2, 2.2]), [0., 0.5, -1.])
    # origin inside the box
    ray(c + h * torch.tensor([0.1, 0.2, -0.3]), [0.3, -0.5, 0.8])
    ray(c + h * torch.tensor([-0.6, 0.7, 0.5]), [1., -1., -0.7])
    ray(c + h * torch.tensor([0.9, 0.9, 0.9]), [0., 0., -1.])
    # misses the box
    ray(c + h * torch.tensor([-2.5, 2.0, 0.]), [1., 0., 0.])
    ray(c + h * torch.tensor([-2.5, 0., 0.]), [-1., 0.2, 0.1])
    ray(c + h * torch.tensor([3., 3., 3.]), [1., -0.1, 0.4])
    # grazes a face / runs along an edge / aims at a corner
    ray(torch.stack([c[0] - 2.5 * h[0], mx[1], c[2] + 0.2 * h[2]]), [1., 0., 0.])
    ray(torch.stack([c[0] - 2.5 * h[0], mn[1], c[2]]), [2., 0., 0.1])
    ray(torch.stack([c[0] - 2.5 * h[0], mx[1], mx[2]]), [1., 0., 0.])
    ray(torch.stack([c[0] + 0.3 * h[0], c[1] - 2.0 * h[1], mn[2]]), [0., 1., 0.])
    ray(c + h * torch.tensor([-3., -3., -3.]), [1., 1., 1.])
    ray(c + h * torch.tensor([-3., -1.0, 0.3]), [1., 1e-7, 0.])
    ray(c + h * torch.tensor([-3., 0., 2.0]), [2., 0., -1.])                         # meets the edge x = min, z = max from outside
    # a few through the middle, long and short directions
    ray(c + h * torch.tensor([-2.5, 0.05, -0.1]), [5., 0.2, 0.3])
    ray(c + h * torch.tensor([2.5, -0.3, 0.4]), [-0.01, 0.001, -0.002])
    return torch.stack(o).cuda(), torch.stack(d).cuda()


@pytest.mark.parametrize('mask_kind', ['scene', 'all_false', 'all_true'])
def test_hit_on_hand_made_rays(S, mask_kind):
    model = utils.model_from_checkpoint_dict(S['ck']).cuda().eval()
    m = model.mask_cache.mask
    if mask_kind != 'scene':
        m.fill_(mask_kind == 'all_true')
        _bump(m)
    ro, rd = _hand_made_rays(model)
    assert ro.shape[0] % 64 != 0
    for near in (S['rk']['near'], 0.0, 0.2):
        rk = dict(S['rk'], near=near)
        hit = model.k4_hit_coarse_geo(rays_o=ro, rays_d=rd, **rk)
        want = model.hit_coarse_geo(rays_o=ro, rays_d=rd, **rk)
        assert torch.equal(hit, want), (mask_kind, near, hit.tolist(), want.tolist())
        if mask_kind == 'all_false':
            assert not bool(hit.any())
        if mask_kind == 'all_true' and near == 0.0:
            h = hit.tolist()
            assert h[0] and h[1] and h[2] and h[4] and h[5] and h[6] and h[17]         # through the box / from inside it
            assert not (h[7] or h[8] or h[9])                                          # past the box


def test_hit_on_zero_rays(S):
    model, rk = S['model'], S['rk']
    e = torch.empty([0, 3], device='cuda')
    hit = model.k4_hit_coarse_geo(rays_o=e, rays_d=e, **rk)
    assert hit.shape == (0,) and hit.dtype == torch.bool and hit.is_cuda
    e = torch.empty([0, 5, 3], device='cuda')
    assert model.k4_hit_coarse_geo(rays_o=e, rays_d=e, **rk).shape == (0, 5)


def _want_counts(hit, bs):
    """Sums of the mask over patch_gen's index arrays (host, exact integers)."""
    h = hit.cpu().numpy().astype(bool)
    arr = D.patch_gen(h.shape[-2:], None, bs, 1)
    return np.array([[int(v[a[..., 0], a[..., 1]].sum()) for a in arr] for v in h.reshape((-1,) + h.shape[-2:])], dtype=np.int32)


@pytest.mark.parametrize('H,W,bs', [(200, 264, 64), (128, 192, 64), (40, 56, 16), (40, 56, 64)])
def test_patch_hit_counts_are_the_sums_over_patch_gen(H, W, bs):
    g = torch.Generator().manual_seed(H * 1000 + W + bs)
    hit = (torch.rand([H, W], generator=g) < 0.45).cuda()
    P = (H // bs) * (W // bs) + H // bs + W // bs + 1
    got = D.patch_hit_counts(hit, bs)
    assert got.dtype == torch.int32 and got.shape == (P,) and got.is_cuda
    want = _want_counts(hit, bs)[0]
    assert np.array_equal(got.cpu().numpy(), want)
    assert int(got.sum()) == int(hit.sum())                                           # the entries partition the view
    if (H, W, bs) == (128, 192, 64):                                                  # divisible: the empty entries are 0 and keep their place
        assert got[6:].tolist() == [0] * 6 and bool((got[:6] > 0).all())
    if (H, W, bs) == (40, 56, 64):                                                    # no full tile: the corner is the view
        assert got.tolist() == [int(hit.sum())]
    assert torch.equal(D.patch_hit_counts(hit.to(torch.uint8) * 3, bs), got)          # uint8: non-zero counts as a hit
    assert torch.equal(D.patch_hit_counts(torch.ones_like(hit), bs).cpu(),
                       torch.from_numpy(_want_counts(torch.ones_like(hit), bs)[0]))


def test_patch_hit_counts_of_a_batch_equal_the_single_image_calls():
    g = torch.Generator().manual_seed(11)
    hit = (torch.rand([3, 200, 264], generator=g) < torch.tensor([0.1, 0.5, 0.9])[:, None, None]).cuda()
    got = D.patch_hit_counts(hit, 64)
    assert got.shape == (3, 20) and got.dtype == torch.int32
    for i in range(3):
        assert torch.equal(got[i], D.patch_hit_counts(hit[i], 64))
    assert np.array_equal(got.cpu().numpy(), _want_counts(hit, 64))
    wide = torch.zeros([3, 200, 300], dtype=torch.bool, device='cuda')
    wide[:, :, 10:274] = hit
    assert torch.equal(D.patch_hit_counts(wide[:, :, 10:274], 64), got)               # a non-contiguous window
    assert D.patch_hit_counts(hit[:0], 64).shape == (0, 20)


def test_inmask_tables_selection_and_draws_on_the_golden_scene(S, G):
    model, rk, n, H, W = S['model'], S['rk'], S['n'], S['H'], S['W']
    before = np.random.get_state()
    rgb, ro, rd, vd, imsz, gen = D.get_training_rays_in_maskcache_sampling_sr(*S['args'], model, rk, None)
    after = np.random.get_state()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]   # nothing drawn before the first next()
    # the tables are get_training_rays'
    assert torch.equal(rgb, S['imgs']) and torch.equal(ro, S['ro']) and torch.equal(rd, S['rd']) and torch.equal(vd, S['vd'])
    assert ro.shape == (n, H, W, 3)
    assert [int(v) for v in imsz] == S['staged'].sum((1, 2)).tolist()
    # per-tile counts against the CPU oracle's, within the margin the golden was chosen for
    counts = D.patch_hit_counts(model.k4_hit_coarse_geo(rays_o=ro, rays_d=rd, **rk), 64).cpu().numpy()
    diff = np.abs(counts.astype(np.int64) - G['counts'])
    print('largest per-tile count difference from the CPU oracle:', int(diff.max()))
    assert counts.shape == G['counts'].shape and int(diff.max()) <= 32
    patch_all, index_all = D.select_inmask_patches(counts, (H, W), 64, 2048)
    assert np.array_equal(index_all, G['index_all']) and len(patch_all) == len(G['kept_origin'])
    for p, o, s in zip(patch_all, G['kept_origin'], G['kept_shape']):
        assert p.shape == (s[0], s[1], 2) and p[0, 0].tolist() == o.tolist() and p[-1, -1].tolist() == [o[0] + s[0] - 1, o[1] + s[1] - 1]
    # the returned generator holds that selection: it draws the reference's sequence
    np.random.seed(int(G['draws_seed']))
    for want in G['draws']:
        image, rows, cols, rows4, cols4, (pr, pc) = next(gen)
        assert (int(image), int(rows[0]), int(cols[0]), pr, pc) == tuple(int(v) for v in want)
        assert rows4 == rows and cols4 == cols
        r0, c0 = int(rows[0]), int(cols[0])
        for table in (ro, rd, vd, rgb):                                               # a draw indexes a pr x pc window of its view
            patch = table[image, rows, cols].reshape(pr, pc, 3)
            assert torch.equal(patch, table[int(image), r0:r0 + pr, c0:c0 + pc])


def test_inmask_tables_keep_tiles_of_unequal_shape_and_say_when_none_qualifies(S):
    """The golden views in tiles of side 72 (2 x 3 full tiles, a 56-row band, a 48-column band): with the bar just under the fullest remainder entry that
    entry qualifies beside full tiles (upstream's np.stack would fail).  With a bar no tile can pass (4096 of 4096 rays) the function raises ValueError."""
    model, rk = S['model'], S['rk']
    imgs, poses, HW, Ks = S['args'][:4]
    args = (imgs, poses, HW, Ks) + S['args'][4:]
    with pytest.raises(ValueError, match='no 64x64 tile'):
        D.get_training_rays_in_maskcache_sampling_sr(*args, model, rk, None, min_hits=4096)
    counts = D.patch_hit_counts(S['staged'], 72).cpu().numpy()                        # side 72: 2 x 3 full tiles, a 56-row band, a 48-column band
    bar = int(np.sort(counts[:, 6:].reshape(-1))[-1]) - 1                             # low enough for the fullest remainder entry
    out = D.get_training_rays_in_maskcache_sampling_sr(*args, model, rk, None, patch_rays=72 * 8, sz_patch=8, min_hits=bar)
    patch_all, index_all = D.select_inmask_patches(counts, (S['H'], S['W']), 72, bar)
    shapes = {p.shape[:2] for p in patch_all}
    assert len(shapes) > 1 and (72, 72) in shapes, shapes
    np.random.seed(5)
    seen = set()
    for _ in range(len(patch_all)):
        image, rows, cols, _, _, (pr, pc) = next(out[5])
        seen.add((int(image), int(rows[0]), int(cols[0]), pr, pc))
    assert seen == {(int(b), int(p[0, 0, 0]), int(p[0, 0, 1]), p.shape[0], p.shape[1]) for p, b in zip(patch_all, index_all)}
