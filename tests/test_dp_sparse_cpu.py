"""Host-side facts of the scratch-image exchange (no GPU): its three entry points are declared in include/k4nerf.h, bound in _native.py and exported by the
library under ABI version 24; its A/B switch is a module attribute, not an environment variable; the step's gate and the exchange's choice of grids depend on
nothing rank-local."""
import glob
import os
import re

import torch

import nerf4k_amd  # noqa: F401
from nerf4k_amd import _native as N, joint_train
from nerf4k_amd.lib import grid as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('k4_scatter_image_list', 'k4_scatter_image_take', 'k4_scatter_image_add')


def test_the_three_entry_points_are_declared_bound_and_exported_under_abi_24():
    header = open(os.path.join(ROOT, 'include', 'k4nerf.h')).read()
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    for s in SYMBOLS:
        assert re.search(r'\bint\s+%s\s*\(' % s, code), f'{s} is not declared in include/k4nerf.h'
        assert s in N._EXTRA_SIGS, f'{s} is not bound in _native.py'
        assert hasattr(N.lib(), s)
    # (arguments as declared: workspace, C, X, Y, Z, then the list / message pointers and sizes, the stream last)
    assert len(N._EXTRA_SIGS['k4_scatter_image_list'][0]) == 9
    assert len(N._EXTRA_SIGS['k4_scatter_image_take'][0]) == 10
    assert len(N._EXTRA_SIGS['k4_scatter_image_add'][0]) == 11
    assert re.search(r'#define\s+K4_ABI_VERSION\s+24\b', header)
    assert N.K4_ABI_VERSION == 24 and N.lib().k4_abi_version() == 24


def test_the_switch_is_a_module_attribute_and_no_environment_variable_was_added():
    assert joint_train._SPARSE_IMAGE_EXCHANGE is True
    names = set()
    for f in glob.glob(os.path.join(ROOT, '4k-nerf_amd', '**', '*.py'), recursive=True):
        names |= set(re.findall(r"environ(?:\.get)?[\(\[]\s*'(K4_[A-Z0-9_]+)'", open(f).read()))
    for f in glob.glob(os.path.join(ROOT, '4k-nerf_amd', 'csrc', '*')):
        names |= set(re.findall(r'env_int\("(K4_[A-Z0-9_]+)"', open(f).read())) | set(re.findall(r'getenv\("(K4_[A-Z0-9_]+)"', open(f).read()))
    assert len(names) == 12, sorted(names)                      # as before the exchange was added
    for f in ('joint_train.py', os.path.join('lib', 'grid.py'), os.path.join('csrc', 'k4_opt.hip')):
        assert not re.search(r'environ|getenv|env_int', open(os.path.join(ROOT, '4k-nerf_amd', f)).read()), f


def test_the_exchange_picks_its_grids_by_their_arming_alone():
    """Which collectives a rank enters follows from what JointTrainer.step armed (configuration and global_step), never from what its backward left behind."""
    model = torch.nn.Module()
    model.k0 = G.DenseGrid(4, [3, 4, 5], [0, 0, 0], [1, 1, 1])
    model.density = G.DenseGrid(1, [3, 4, 5], [0, 0, 0], [1, 1, 1])
    assert joint_train._image_exchange_grids(model) == []                 # no route object yet, and none is created by asking
    assert '_k4_route' not in model.k0.__dict__
    model.k0.grad_route.arm('sparse')
    model.density.grad_route.arm('dense')
    assert joint_train._image_exchange_grids(model) == [model.k0]        # armed, no backward yet: no sums, no gradient -- chosen all the same
    assert not model.k0.grad_route.sums and model.k0.grid.grad is None
    model.k0.grad_route.abort()
    assert joint_train._image_exchange_grids(model) == []
    # without a process group (and without the one-rank smoke test's switch) nothing is exchanged
    assert joint_train.exchange_gradients(model, torch.nn.Linear(2, 2)) == {'world': 1}
