"""JointTrainer.step keeps k0's gradient in the scatter's scratch image while a gradient exchange runs (joint_train._SPARSE_IMAGE_EXCHANGE; lib/grid.GridGrad.exchange):
tools/dp_sparse_route_check.py in ONE subprocess (a world-size-1 `nccl` process group that must not leak into the other tests), its JSON line taken apart here.

Whole runs are compared at the tolerances tests/test_train_ops_gpu.py::test_iterations_without_tv_update_k0_from_the_scatter_image grants the scatter's atomic
reordering (losses 1e-6, parameters and moments 1e-5 relative): two runs of the SAME form differ by that much.  Bit-for-bit equality is therefore asserted where
the inputs are identical: one scatter image handed to both forms of the exchange + step, and one dense gradient (the scratch image withheld from the backward)
handed to the exchange under the armed route and to the one without it."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def result():
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0')
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'dp_sparse_route_check.py')], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    line = [l for l in out.stdout.splitlines() if l.startswith('DP_SPARSE_ROUTE ')][-1]
    res = json.loads(line[len('DP_SPARSE_ROUTE '):])
    print(json.dumps(res))
    assert res['ok'] and res['backend'] == 'nccl' and res['world_size'] == 1
    return res


@pytest.mark.gpu
def test_k0_has_no_dense_gradient_in_the_iterations_without_tv_under_an_exchange(result):
    ii = result['forms']['ii']
    assert ii['k0_grad'] == [True, False, False, False]          # step 1 (dense TV): the dense gradient; steps 2-4: `.grad` stays None
    assert all(ii['density_grad'])                               # one channel: no scratch image, the dense list exchange as ever
    assert all(ii['idle']) and all(ii['image_zero'])             # the route is idle and the image all-zero between iterations
    assert ii['k0_step'] == 4
    assert ii['image_bytes'][0] == 0 and all(b > 0 for b in ii['image_bytes'][1:])
    for touched in ii['image_touched'][1:]:
        (counts, nvox), = touched
        assert len(counts) == 1 and 0 < counts[0] < nvox
    # the A/B switch off: today's path
    iii = result['forms']['iii']
    assert iii['k0_grad'] == [True] * 4 and iii['image_bytes'] == [0] * 4 and iii['k0_step'] == 4
    # no exchange: the single-process routes (step 1: the split step, steps 2-4: the scratch image) -- never a dense gradient
    assert result['forms']['i']['k0_grad'] == [False] * 4 and result['forms']['i']['image_bytes'] == [0] * 4


@pytest.mark.gpu
@pytest.mark.parametrize('pair', ['ii_vs_i', 'ii_vs_iii', 'iv_vs_iii'])
def test_the_image_route_trains_like_the_other_forms(result, pair):
    cmp = result['against'][pair]
    assert cmp['loss_rel_err'] <= 1e-6, cmp
    assert cmp['tensor_rel_err'] <= 1e-5, cmp
    assert cmp['same_voxels_touched'], cmp


@pytest.mark.gpu
def test_both_forms_of_the_exchange_give_the_same_bits_from_one_scatter_image(result):
    one = result['one_image']
    assert one['changed'] and one['touched'][0] > 0
    assert one['equal'] == [True, True, True], one               # k0, exp_avg, exp_avg_sq
    assert one['image_zero_after']


@pytest.mark.gpu
def test_a_rank_with_a_dense_gradient_sends_the_same_message(result):
    iv = result['forms']['iv']
    assert iv['k0_grad'] == [True] * 4                           # the scratch image withheld from the backward: dense after all
    assert all(b > 0 for b in iv['image_bytes'][1:]) and iv['k0_step'] == 4 and all(iv['idle'])
    one = result['one_dense_gradient']
    assert one['grad_dense'] and one['message_bytes'] > 0 and one['changed']
    assert one['equal'] == [True, True, True], one
