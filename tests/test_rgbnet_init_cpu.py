"""The seeded initial weights of every voxel-grid model's rgbnet, without a GPU: each class constructed under ``torch.manual_seed(s)`` against a
Linear-ReLU stack this file spells out in that class's construction order, bit for bit, and the rgbnet's state-dict key names.

Where the stack sits in the RNG stream: a DenseGrid is ``torch.zeros`` and a MaskGrid ``torch.ones``, so with dense grids the constructors draw
nothing before their rgbnet -- the stack built right after the same ``manual_seed`` is at the same point of the stream.  DirectVoxGO,
DirectContractedVoxGO and DirectBiVoxGO (its two stacks one after the other, the background's drawn even when ``bg_use_mlp=False`` drops it)
construct the layers in written order; DirectMPIGO constructs the hidden layers before the first one (bench.py's scene is built under a seed)."""
import pytest
import torch
import torch.nn as nn

import nerf4k_amd  # noqa: F401
from nerf4k_amd.lib import dbvgo, dcvgo, dmpigo, dvgo

WIDTH, K0_DIM, PE = 32, 6, 4
BOX = dict(xyz_min=[-1., -1., -1.], xyz_max=[1., 1., 1.], num_voxels=8 ** 3)
VOX = dict(BOX, num_voxels_base=8 ** 3, alpha_init=1e-2, rgbnet_dim=K0_DIM, rgbnet_width=WIDTH, viewbase_pe=PE)
DIM0 = 3 + 3 * PE * 2 + K0_DIM                     # [k0, viewdirs, sin, cos]


def _in_order(dim0, depth):
    net = nn.Sequential(
        nn.Linear(dim0, WIDTH), nn.ReLU(inplace=True),
        *[nn.Sequential(nn.Linear(WIDTH, WIDTH), nn.ReLU(inplace=True)) for _ in range(depth - 2)],
        nn.Linear(WIDTH, 3),
    )
    nn.init.constant_(net[-1].bias, 0)
    return net


def _hidden_first(dim0, depth):
    hidden = [nn.Sequential(nn.Linear(WIDTH, WIDTH), nn.ReLU(inplace=True)) for _ in range(depth - 2)]
    net = nn.Sequential(nn.Linear(dim0, WIDTH), nn.ReLU(inplace=True), *hidden, nn.Linear(WIDTH, 3))
    nn.init.constant_(net[-1].bias, 0)
    return net


# name -> (constructor, the stacks in the parent's order under the same seed, the prefixes of their state-dict keys)
CASES = {
    'dvgo_direct': (lambda d: dvgo.DirectVoxGO(rgbnet_direct=True, rgbnet_depth=d, **VOX),
                    lambda d: [_in_order(DIM0, d)], ['rgbnet.']),
    'dvgo_diffuse': (lambda d: dvgo.DirectVoxGO(rgbnet_direct=False, rgbnet_depth=d, **VOX),
                     lambda d: [_in_order(DIM0 - 3, d)], ['rgbnet.']),
    'dcvgo': (lambda d: dcvgo.DirectContractedVoxGO(rgbnet_depth=d, **VOX),
              lambda d: [_in_order(DIM0, d)], ['rgbnet.']),
    'dbvgo_bg_mlp': (lambda d: dbvgo.DirectBiVoxGO(bg_use_mlp=True, rgbnet_depth=d, **VOX),
                     lambda d: [_in_order(DIM0, d), _in_order(DIM0, d)], ['rgbnet.0.', 'rgbnet.1.']),
    'dbvgo_bg_grid': (lambda d: dbvgo.DirectBiVoxGO(bg_use_mlp=False, rgbnet_depth=d, **VOX),
                      lambda d: [_in_order(DIM0, d), _in_order(DIM0, d)][:1], ['rgbnet.0.']),
    'dmpigo': (lambda d: dmpigo.DirectMPIGO(mpi_depth=8, rgbnet_dim=K0_DIM, rgbnet_width=WIDTH, rgbnet_depth=d, viewbase_pe=PE, spatial_pe=2,
                                            act_type='relu', mode_type='mlp', **BOX),
               lambda d: [_hidden_first(DIM0 + 3 + 3 * 2 * 2, d)], ['rgbnet.']),
}


@pytest.mark.parametrize('depth', [2, 3, 4])
@pytest.mark.parametrize('name', list(CASES))
def test_seeded_rgbnet_is_the_written_out_stack(name, depth):
    make, stacks, prefixes = CASES[name]
    seed = 1000 + 10 * depth + list(CASES).index(name)
    torch.manual_seed(seed)
    model = make(depth)
    torch.manual_seed(seed)
    want = {}
    for prefix, net in zip(prefixes, stacks(depth)):
        want.update({prefix + k: v for k, v in net.state_dict().items()})
    got = {k: v for k, v in model.state_dict().items() if k.startswith('rgbnet.')}
    layers = ['0'] + [f'{2 + j}.0' for j in range(depth - 2)] + [str(depth)]
    assert set(got) == {p + layer + end for p in prefixes for layer in layers for end in ('.weight', '.bias')}
    assert set(got) == set(want)
    for k in got:
        assert got[k].shape == want[k].shape and torch.equal(got[k], want[k]), (name, depth, k)
    last = prefixes[0] + str(depth)
    assert not got[last + '.bias'].any() and got[last + '.weight'].any() and got[prefixes[0] + '0.bias'].any()
