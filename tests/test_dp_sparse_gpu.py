"""The three kernels behind the data-parallel exchange of a gradient that stayed in the scatter's scratch image (csrc/k4_opt.hip: k4_scatter_image_list /
_take / _add), in-process and without a process group, on hand-built images: scratch[nvox][C] fp32 sums followed by one flag byte per voxel at byte offset
nvox*C*4 of a 16-byte aligned workspace -- an offset that is a multiple of 4 only, so the cases put the flag array 0, 4, 8 and 12 bytes past a 16-byte boundary.
Everything here is exact: index lists equal `flags.nonzero()`, values are compared as bits, sums against fp32 arithmetic done in rank order on the CPU."""
import numpy as np
import pytest
import torch

import nerf4k_amd  # noqa: F401
from nerf4k_amd import _native as N

pytestmark = pytest.mark.gpu

# the list kernels' constants (csrc/k4_opt.hip): a workgroup of K4_IMG_LIST_THREADS threads counts K4_IMG_LIST_SPAN consecutive flag bytes, one workgroup of as many
# threads scans the per-workgroup counts
K4_IMG_LIST_THREADS = 256
K4_IMG_LIST_SPAN = K4_IMG_LIST_THREADS * 16


def _workspace(C, nvox, flags, sums=None):
    """The image as the scatter leaves it, from CPU tensors: flags uint8 [nvox], sums fp32 [nvox, C] (None: zeros)."""
    nbytes = int(N.lib().k4_grid_sample_3d_backward_workspace_bytes(C, 1, 1, nvox))
    assert nbytes >= nvox * C * 4 + nvox and nbytes % 4 == 0
    ws = torch.zeros([nbytes // 4], dtype=torch.int32, device='cuda')
    assert ws.data_ptr() % 16 == 0
    if sums is not None:
        ws[:nvox * C] = sums.contiguous().view(-1).view(torch.int32).cuda()
    ws.view(torch.uint8)[nvox * C * 4:nvox * C * 4 + nvox] = flags.cuda()
    return ws


def _flags_of(ws, C, nvox):
    return ws.view(torch.uint8)[nvox * C * 4:nvox * C * 4 + nvox].cpu()


def _sums_of(ws, C, nvox):
    return ws[:nvox * C].cpu().view(torch.float32).view(nvox, C)


def _list(ws, C, nvox, cap):
    idx = torch.full([max(cap, 1)], -7, dtype=torch.int32, device='cuda')
    counter = torch.full([1], -1, dtype=torch.int64, device='cuda')
    N.check(N.lib().k4_scatter_image_list(N.ptr(ws), C, 1, 1, nvox, N.ptr(idx), cap, N.ptr(counter), N.stream()), 'k4_scatter_image_list')
    return idx.cpu(), int(counter)


def _random_flags(nvox, density, seed):
    g = torch.Generator().manual_seed(seed)
    if density == 0:
        return torch.zeros([nvox], dtype=torch.uint8)
    if density == 1.0:
        return torch.ones([nvox], dtype=torch.uint8)
    hit = torch.rand([nvox], generator=g) < density
    # (the scatter writes 1; any non-zero byte counts as a flag)
    return torch.where(hit, torch.where(torch.rand([nvox], generator=g) < 0.5, 1, 128), 0).to(torch.uint8)


LIST_CASES = [(2, nvox, d) for nvox in (1, 255, 4095, 4096, 4097, 100003) for d in (0, 0.01, 1.0)] + \
             [(3, 513, 0.01), (3, 513, 1.0), (9, 70001, 0.01), (9, 70001, 1.0), (5, 4099, 0.3),
              # more per-workgroup counts than the scan's one workgroup has threads: every scanning thread owns a slice of several counts
              (2, K4_IMG_LIST_SPAN * (4 * K4_IMG_LIST_THREADS + 1) + 37, 0.01)]


def test_the_cases_cover_every_alignment_of_the_flag_array_and_a_scan_of_slices():
    assert {(nvox * C * 4) % 16 for C, nvox, _ in LIST_CASES} == {0, 4, 8, 12}
    assert max(-(-nvox // K4_IMG_LIST_SPAN) for _, nvox, _ in LIST_CASES) > K4_IMG_LIST_THREADS


@pytest.mark.parametrize('C,nvox,density', LIST_CASES)
def test_list_is_the_ascending_list_of_flagged_voxels(C, nvox, density):
    flags = _random_flags(nvox, density, seed=nvox % 1000 + C)
    # sums that would read as flags if a wide load strayed below the flag array (its first aligned 16 bytes start inside the sums)
    sums = torch.full([nvox, C], 1.5)
    ws = _workspace(C, nvox, flags, sums)
    before = ws.clone()
    want = flags.nonzero().flatten().to(torch.int32)
    cap = max(int(want.numel()), 1) + 3
    idx, n = _list(ws, C, nvox, cap)
    assert n == want.numel()
    assert torch.equal(idx[:n], want)                                    # ascending, exact
    assert bool((idx[n:] == -7).all())                                   # nothing written behind the list
    assert torch.equal(ws, before)                                       # the workspace is unchanged


@pytest.mark.parametrize('C,nvox', [(2, 4097), (3, 513)])
def test_list_overflow_reports_the_full_count_and_writes_cap_indices(C, nvox):
    flags = _random_flags(nvox, 0.3, seed=5)
    ws = _workspace(C, nvox, flags)
    want = flags.nonzero().flatten().to(torch.int32)
    assert want.numel() > 7
    idx = torch.full([16], -7, dtype=torch.int32, device='cuda')
    counter = torch.full([1], -1, dtype=torch.int64, device='cuda')
    N.check(N.lib().k4_scatter_image_list(N.ptr(ws), C, 1, 1, nvox, N.ptr(idx), 7, N.ptr(counter), N.stream()), 'k4_scatter_image_list')
    assert int(counter) == want.numel()
    assert torch.equal(idx.cpu()[:7], want[:7]) and bool((idx.cpu()[7:] == -7).all())
    # cap = 0: the count alone
    _, n = _list(ws, C, nvox, 0)
    assert n == want.numel()


def _hand_built_image(C, nvox, seed):
    """Flagged voxels (the first and the last one among them) with random sums; some flagged voxels whose sums are all zero, some -0.0; unflagged voxels hold
    zeros, as in the scatter's image."""
    g = torch.Generator().manual_seed(seed)
    flags = torch.zeros([nvox], dtype=torch.uint8)
    picked = torch.randperm(nvox, generator=g)[:max(nvox // 9, 6)]
    flags[picked] = 1
    flags[0] = flags[nvox - 1] = 1
    touched = flags.nonzero().flatten()
    sums = torch.zeros([nvox, C])
    sums[touched] = torch.randn([touched.numel(), C], generator=g)
    sums[touched[1]] = 0.0                                               # flagged, all sums zero (two contributions that cancelled, a zero output gradient)
    sums[touched[2]] = -0.0
    sums[touched[3], 0] = -0.0
    sums[touched[-1], C - 1] = 0.0
    return flags, sums, touched.to(torch.int32)


@pytest.mark.parametrize('C,nvox', [(3, 513), (12, 1000), (2, 4097)])
def test_take_moves_the_listed_sums_into_the_message_and_clears_the_image(C, nvox):
    flags, sums, touched = _hand_built_image(C, nvox, seed=C + nvox)
    ws = _workspace(C, nvox, flags, sums)
    n = int(touched.numel())
    cap = n + 5
    values = torch.zeros([C * cap], dtype=torch.int32, device='cuda')
    N.check(N.lib().k4_scatter_image_take(N.ptr(ws), C, 1, 1, nvox, N.ptr(touched.cuda()), n, cap, N.ptr(values), N.stream()), 'k4_scatter_image_take')
    got = values.cpu().view(C, cap)
    want = sums[touched.long()].t().contiguous().view(torch.int32)       # [C][n], as bits: -0.0 travels as -0.0
    assert torch.equal(got[:, :n], want)
    assert int(got[:, n:].count_nonzero()) == 0                          # the padding stays zero
    assert int(ws.count_nonzero()) == 0                                  # sums (the -0.0 bit patterns too) and flags cleared


def test_take_of_a_part_of_the_list_leaves_the_rest():
    C, nvox = 4, 777
    flags, sums, touched = _hand_built_image(C, nvox, seed=3)
    ws = _workspace(C, nvox, flags, sums)
    part = touched[::2].contiguous()
    values = torch.zeros([C * int(part.numel())], dtype=torch.int32, device='cuda')
    N.check(N.lib().k4_scatter_image_take(N.ptr(ws), C, 1, 1, nvox, N.ptr(part.cuda()), part.numel(), part.numel(), N.ptr(values), N.stream()), 'k4_scatter_image_take')
    rest = touched[1::2].long()
    want_flags = torch.zeros_like(flags)
    want_flags[rest] = 1
    want_sums = torch.zeros_like(sums)
    want_sums[rest] = sums[rest]
    assert torch.equal(_flags_of(ws, C, nvox), want_flags)
    assert torch.equal(_sums_of(ws, C, nvox).view(torch.int32), want_sums.view(torch.int32))


def test_add_merges_the_ranks_lists_in_rank_order_without_fusing():
    """Three synthetic ranks with overlapping voxel sets, scale 1/3: ((0 + v0*s) + v1*s) + v2*s in fp32, every product rounded before its sum -- one fused
    multiply-add anywhere gives other bits for some of the ~4000 sums here."""
    C, nvox, world = 4, 1000, 3
    g = torch.Generator().manual_seed(17)
    lists = []
    for r in range(world):
        idx = torch.randperm(nvox, generator=g)[:300 + 50 * r].sort().values.to(torch.int32)
        vals = torch.randn([C, idx.numel()], generator=g) * (10.0 ** r)
        lists.append((idx, vals))
    assert len(set(lists[0][0].tolist()) & set(lists[1][0].tolist()) & set(lists[2][0].tolist())) > 0
    # an index outside [0, nvox) changes nothing
    lists[1] = (torch.cat([torch.tensor([-1], dtype=torch.int32), lists[1][0], torch.tensor([nvox], dtype=torch.int32)]),
                torch.cat([torch.full([C, 1], 7.0), lists[1][1], torch.full([C, 1], 9.0)], 1))
    cap = max(int(i.numel()) for i, _ in lists) + 3
    scale = np.float32(1.0 / 3.0)
    ws = _workspace(C, nvox, torch.zeros([nvox], dtype=torch.uint8))
    want = np.zeros([nvox, C], dtype=np.float32)
    want_flags = torch.zeros([nvox], dtype=torch.uint8)
    for idx, vals in lists:
        n = int(idx.numel())
        msg = torch.zeros([(C + 1) * cap], dtype=torch.int32)
        msg[:n] = idx
        msg[cap:].view(torch.float32).view(C, cap)[:, :n] = vals
        dev = msg.cuda()
        N.check(N.lib().k4_scatter_image_add(N.ptr(ws), C, 1, 1, nvox, N.ptr(dev), N.ptr(dev[cap:]), n, cap, float(scale), N.stream()), 'k4_scatter_image_add')
        ok = (idx >= 0) & (idx < nvox)
        rows = idx[ok].long().numpy()
        prod = (vals.numpy()[:, ok.numpy()] * scale).astype(np.float32)  # rounded on its own
        want[rows] = (want[rows] + prod.T).astype(np.float32)
        want_flags[idx[ok].long()] = 1
    torch.cuda.synchronize()
    assert torch.equal(_sums_of(ws, C, nvox).view(torch.int32), torch.from_numpy(want).view(torch.int32))
    assert torch.equal(_flags_of(ws, C, nvox), want_flags)
    nbytes = ws.numel() * 4
    assert int(ws.view(torch.uint8)[nvox * C * 4 + nvox:nbytes].count_nonzero()) == 0           # the padding behind the flags


@pytest.mark.parametrize('C,nvox', [(3, 513), (9, 4101)])
def test_list_take_add_round_trip_reproduces_the_image(C, nvox):
    flags, sums, touched = _hand_built_image(C, nvox, seed=nvox)
    ws = _workspace(C, nvox, flags, sums)
    cap = int(touched.numel()) + 2
    idx, n = _list(ws, C, nvox, cap)
    assert n == touched.numel() and torch.equal(idx[:n], touched)
    msg = torch.zeros([(C + 1) * cap], dtype=torch.int32, device='cuda')
    msg[:n] = idx[:n].cuda()
    N.check(N.lib().k4_scatter_image_take(N.ptr(ws), C, 1, 1, nvox, N.ptr(msg), n, cap, N.ptr(msg[cap:]), N.stream()), 'k4_scatter_image_take')
    assert int(ws.count_nonzero()) == 0
    N.check(N.lib().k4_scatter_image_add(N.ptr(ws), C, 1, 1, nvox, N.ptr(msg), N.ptr(msg[cap:]), n, cap, 1.0, N.stream()), 'k4_scatter_image_add')
    assert torch.equal(_flags_of(ws, C, nvox), flags)
    assert bool((_sums_of(ws, C, nvox) == sums).all())                   # (0 + -0.0 * 1 = +0.0: equal as values)
