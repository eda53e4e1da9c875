"""Host side of the 'patch_inmask' ray sampler (lib/dvgo.py:683-819 upstream) against tests/golden/patch_inmask.npz, which
tests/gen_patch_inmask_golden.py made with the reference's own functions: the three generators draw the reference's sequences from the global
numpy generator, the selection from the per-tile counts is the reference's, the recipe's preset and the ABI number.  Nothing here needs a GPU."""
import os
import re

import numpy as np
import pytest

import nerf4k_amd  # noqa: F401
from nerf4k_amd import _native as N
from nerf4k_amd.joint_train import JointCfg
from nerf4k_amd.lib import dvgo as D
from helpers import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def G():
    z = np.load(os.path.join(GOLDEN, 'patch_inmask.npz'), allow_pickle=False)
    return {k: z[k] for k in z.files}


def _window(r0, c0, pr, pc):
    rr, cc = np.meshgrid(np.arange(r0, r0 + pr), np.arange(c0, c0 + pc), indexing='ij')
    return rr.reshape(-1), cc.reshape(-1)


def _kept_tiles(G):
    return [np.stack(np.meshgrid(np.arange(o[0], o[0] + s[0]), np.arange(o[1], o[1] + s[1]), indexing='ij'), -1)
            for o, s in zip(G['kept_origin'], G['kept_shape'])]


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def test_inmask_generator_draws_the_reference_sequence(G):
    tiles = _kept_tiles(G)
    np.random.seed(int(G['draws_seed']))
    before = np.random.get_state()
    gen = D.inmask_patch_indices_generator(tiles, G['index_all'])
    assert _same_state(before, np.random.get_state())            # creating it draws nothing: the first permutation belongs to the first next()
    assert len(G['draws']) == 2 * len(tiles) + 3                  # two whole permutations and the start of a third
    for want in G['draws']:
        image, rows, cols, rows4, cols4, (pr, pc) = next(gen)
        assert (int(image), int(rows[0]), int(cols[0]), pr, pc) == tuple(int(v) for v in want)
        wr, wc = _window(want[1], want[2], pr, pc)
        assert isinstance(rows, list) and np.array_equal(rows, wr) and np.array_equal(cols, wc)
        assert np.array_equal(rows4, wr) and np.array_equal(cols4, wc)      # sr_ratio 1: the "4x" lists are the plain ones
    assert not _same_state(before, np.random.get_state())


@pytest.mark.parametrize('key,imsz', [('simg', (200, 264)), ('simg_div', (128, 192))])
def test_simg_generator_draws_the_reference_sequence(G, key, imsz):
    np.random.seed(int(G[key + '_seed']))
    before = np.random.get_state()
    gen = D.simg_patch_indices_generator(imsz, 4096)
    assert _same_state(before, np.random.get_state())
    want_all = G[key + '_draws']
    n_entries = (imsz[0] // 64) * (imsz[1] // 64) + imsz[0] // 64 + imsz[1] // 64 + 1
    assert len(want_all) > n_entries                              # across two permutations
    assert ((want_all[:, 0] == 0).any()) == (key == 'simg_div')   # the divisible size: empty remainder entries take part in the permutation
    for want in want_all:
        y = next(gen)
        assert isinstance(y, list) and len(y) == 2
        rows, cols = y
        n = int(want[0])
        assert len(rows) == len(cols) == n
        if n:
            assert (rows[0], cols[0], rows[-1], cols[-1]) == tuple(want[1:])
            wr, wc = _window(want[1], want[2], want[3] - want[1] + 1, want[4] - want[2] + 1)
            assert np.array_equal(rows, wr) and np.array_equal(cols, wc)


def test_batch_images_generator_matches_the_reference(G):
    before = np.random.get_state()
    gen = D.batch_images_generator(3, 1000, 300)
    for start, stop, image, last in G['batch_images']:
        r, n_im, flag = next(gen)
        assert isinstance(r, range) and (r.start, r.stop, r.step) == (start, stop, 1) and n_im == image and flag is bool(last)
    assert _same_state(before, np.random.get_state())            # no random numbers
    # a range of exactly BS that reaches the end of the image is the last one; N images wrap
    gen = D.batch_images_generator(2, 6, 3)
    assert [(list(r), i, f) for r, i, f in (next(gen) for _ in range(5))] == [
        ([0, 1, 2], 0, False), ([3, 4, 5], 0, True), ([0, 1, 2], 1, False), ([3, 4, 5], 1, True), ([0, 1, 2], 0, False)]


def test_selection_from_the_golden_counts(G):
    H, W = (int(v) for v in G['hw'])
    patch_all, index_all = D.select_inmask_patches(G['counts'], (H, W), 64, int(G['min_hits']))
    assert index_all.dtype == np.int64 and np.array_equal(index_all, G['index_all'])
    assert len(patch_all) == len(G['kept_origin'])
    for got, want in zip(patch_all, _kept_tiles(G)):
        assert got.dtype == np.int64 and np.array_equal(got, want)
    # the conditions the golden was chosen under hold for the stored counts
    full = G['counts'][:, :(H // 64) * (W // 64)]
    assert (full > 2048).sum() >= 4 and (full <= 2048).sum() >= 4 and ((full <= 2048) & (full > 0)).any()
    assert (np.abs(G['counts'].astype(np.int64) - 2048) > 32).all()
    # the counts partition a view
    hit = np.unpackbits(G['hit_bits'])[:3 * H * W].reshape(3, H, W)
    assert np.array_equal(G['counts'].sum(1), hit.sum((1, 2))) and np.array_equal(G['imsz'], hit.sum((1, 2)))
    for b in range(3):
        for p, a in enumerate(D.patch_gen((H, W), None, 4096, 64)):
            assert G['counts'][b, p] == hit[b][a[..., 0], a[..., 1]].sum()


def test_selection_keeps_tiles_of_unequal_shape_and_the_generator_serves_them():
    """Where upstream's np.stack fails: a 40 x 56 view in tiles of side 16 (patch_rays=256, sz_patch=16) with min_hits=100 -- the 8-row bottom band of a
    column band holds 128 rays and qualifies beside the 16 x 16 tiles."""
    H, W, bs = 40, 56, 16
    P = (H // bs) * (W // bs) + H // bs + W // bs + 1
    counts = np.zeros([2, P], dtype=np.int32)
    arr = D.patch_gen((H, W), None, 256, 16)
    assert len(arr) == P
    bottom0 = (H // bs) * (W // bs) + H // bs                     # the first bottom-edge entry: rows 32..39, cols 0..15
    counts[0, 1], counts[0, bottom0], counts[1, 0], counts[1, P - 1] = 200, 128, 101, 64
    patch_all, index_all = D.select_inmask_patches(counts, (H, W), bs, min_hits=100)
    assert index_all.tolist() == [0, 0, 1]
    assert [p.shape for p in patch_all] == [(16, 16, 2), (8, 16, 2), (16, 16, 2)]
    assert patch_all[1][0, 0].tolist() == [32, 0] and patch_all[0][0, 0].tolist() == [16, 0]
    np.random.seed(3)
    gen = D.inmask_patch_indices_generator(patch_all, index_all)
    seen = set()
    for _ in range(3):
        image, rows, cols, _, _, (pr, pc) = next(gen)
        assert len(rows) == len(cols) == pr * pc
        seen.add((int(image), pr, pc, int(rows[0]), int(cols[0])))
    assert seen == {(0, 16, 16, 16, 0), (0, 8, 16, 32, 0), (1, 16, 16, 0, 0)}
    # nothing above the bar: the list is empty (the table builder turns that into ValueError, tests/test_patch_inmask_gpu.py)
    patch_all, index_all = D.select_inmask_patches(counts, (H, W), bs, min_hits=200)
    assert patch_all == [] and index_all.shape == (0,)


def test_no_qualifying_tile_raises_value_error(monkeypatch):
    """The table builder with its device steps replaced by host stand-ins: the selection and its error path need no GPU."""
    import torch
    H, W = 40, 56

    class Model:
        def k4_hit_coarse_geo(self, rays_o, rays_d, **kw):
            hit = torch.zeros(rays_o.shape[:-1], dtype=torch.bool)
            hit[:, :16, :16] = True
            hit[0, 32:, :16] = True
            return hit

    def rays_of(hw, K, c2w, *a):
        return tuple(torch.zeros([hw[0], hw[1], 3]) for _ in range(3))

    def counts_of(hit, bs):
        arr = D.patch_gen(hit.shape[1:], None, bs, 1)
        return torch.tensor([[int(h[a[..., 0], a[..., 1]].sum()) for a in arr] for h in hit], dtype=torch.int32)

    monkeypatch.setattr(D, '_rays_of', rays_of)
    monkeypatch.setattr(D, 'patch_hit_counts', counts_of)
    imgs = torch.rand([2, H, W, 3])
    args = (imgs, torch.zeros([2, 3, 4]), np.array([[H, W]] * 2), np.zeros([2, 3, 3]), False, False, False, False, Model(), {}, None)
    with pytest.raises(ValueError, match='no 16x16 tile'):
        D.get_training_rays_in_maskcache_sampling_sr(*args, patch_rays=256, sz_patch=16, min_hits=256)
    rgb, ro, rd, vd, imsz, gen = D.get_training_rays_in_maskcache_sampling_sr(*args, patch_rays=256, sz_patch=16, min_hits=100)
    assert torch.equal(rgb, imgs) and ro.shape == (2, H, W, 3) and imsz == [256 + 128, 256]
    shapes = sorted(tuple(next(gen)[5]) for _ in range(3))
    assert shapes == [(8, 16), (16, 16), (16, 16)]                 # tiles of unequal shape are kept
    with pytest.raises(AssertionError, match='one size'):
        D.get_training_rays_in_maskcache_sampling_sr(*(args[:2] + (np.array([[H, W], [H, W + 1]]),) + args[3:]))


def test_chair_1x_preset_carries_the_recipe_values():
    cfg = JointCfg.chair_1x_joint_l1_gan()
    want = dict(N_iters=300000, N_rand=8192, N_patch=64, ray_sampler='patch_inmask',
                lrate_density=1e-1, lrate_k0=1e-1, lrate_rgbnet=1e-3, lrate_srnet=2e-4, lrate_decay=300,
                skip_zero_grad_fields=['density', 'k0'],
                weight_main=1.0, weight_entropy_last=0.001, weight_nearclip=0, weight_distortion=0, weight_rgbper=0.01,
                weight_pcp=0.5, weight_gan=0.05, weight_style=0.2,
                tv_every=1, tv_after=0, tv_before=0, tv_dense_before=0, weight_tv_density=0.0, weight_tv_k0=0.0)
    assert dict(cfg) == want
    assert cfg.ray_sampler == 'patch_inmask' and cfg.weight_gan == 0.05
    assert JointCfg.chair_1x_joint_l1_gan(weight_gan=0, N_rand=4096).N_rand == 4096
    assert set(want) == set(JointCfg.fern_lg_joint_l1())          # the keys the joint loop reads


def test_abi_24_in_header_loader_and_documents():
    hdr = open(os.path.join(ROOT, 'include', 'k4nerf.h')).read()
    assert int(re.search(r'#define\s+K4_ABI_VERSION\s+(\d+)', hdr).group(1)) == N.K4_ABI_VERSION == 24
    for doc in ('INTEGRATION.md', 'DESIGN.md'):
        quoted = [int(x) for x in re.findall(r'ABI version (\d+)', open(os.path.join(ROOT, doc)).read())]
        assert quoted and set(quoted) == {24}, (doc, quoted)
    for name in ('k4_hit_coarse_geo', 'k4_patch_hit_counts', 'k4_patch_hit_entries'):
        assert re.search(r'\b' + name + r'\s*\(', hdr), name
        assert name in N._SIGS or name in N._EXTRA_SIGS, name
        assert hasattr(N.lib(), name), name
    L = N.lib()
    assert L.k4_patch_hit_entries(200, 264, 64) == 20 and L.k4_patch_hit_entries(128, 192, 64) == 12 and L.k4_patch_hit_entries(40, 56, 64) == 1
    assert L.k4_patch_hit_entries(800, 800, 64) == 169 and L.k4_patch_hit_entries(0, 8, 8) < 0 and L.k4_patch_hit_entries(8, 8, 0) < 0
