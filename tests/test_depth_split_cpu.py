"""The host side of the two-launch depth split, without a GPU: the selection rule (lib/dmpigo.depth_split_of) and the fp64 restatement of
k4_mpi_depth_split_stats that tests/test_depth_split_gpu.py holds the kernel to (tests/depth_split_oracle.py) -- a hand-worked grid, and the
condition under which that comparison is exact, on every input the GPU test uses."""
import numpy as np
import pytest

import nerf4k_amd  # noqa: F401
from nerf4k_amd.lib import dmpigo
import depth_split_oracle as DSO

GAIN, OPAQUE = 0.05, 0.5
# k -> depth eighth min(7, 8 k // n) whose statistic decides about k, written out per sample count
BIN_OF_K = {128: {64: 4}, 199: {64: 2, 128: 5, 192: 7}, 256: {64: 2, 128: 4, 192: 6}, 319: {64: 1, 128: 3, 192: 4, 256: 6}}


def _stats(opaque=1.0, **bins):
    st = [0.0] * 8
    st[0] = opaque
    for b, v in bins.items():
        st[int(b[1:])] = v
    return st


def test_defaults_are_the_measured_thresholds():
    assert dmpigo.DEPTH_SPLIT is True and dmpigo.DEPTH_SPLIT_MIN_GAIN == GAIN and dmpigo.DEPTH_SPLIT_MIN_OPAQUE == OPAQUE


@pytest.mark.parametrize('n', [2, 33, 63, 64])
def test_no_multiple_of_64_below_n_samples(n):
    assert dmpigo.depth_split_of([1.0] * 8, n, GAIN, OPAQUE) == 0


def test_65_samples_split_at_64_on_the_last_eighth():
    assert dmpigo.depth_split_of(_stats(b7=0.4), 65, GAIN, OPAQUE) == 64
    assert dmpigo.depth_split_of(_stats(b6=0.4), 65, GAIN, OPAQUE) == 0


@pytest.mark.parametrize('n', sorted(BIN_OF_K))
def test_bin_mapping(n):
    table = BIN_OF_K[n]
    assert sorted(table) == list(range(64, n, 64))
    for k, b in table.items():
        assert b == min(7, 8 * k // n) and b >= 1
        assert dmpigo.depth_split_of(_stats(**{f'b{b}': 0.4}), n, GAIN, OPAQUE) == k, (n, k, b)
    for b in set(range(1, 8)) - set(table.values()):                    # an eighth no candidate reads proposes nothing
        assert dmpigo.depth_split_of(_stats(**{f'b{b}': 0.9}), n, GAIN, OPAQUE) == 0, (n, b)


def test_first_eighth_never_counts():
    """n = 1000: k = 64 maps to eighth 0, whose slot holds the opaque share, not a gain."""
    assert dmpigo.depth_split_of(_stats(opaque=1.0), 1000, GAIN, OPAQUE) == 0
    assert dmpigo.depth_split_of(_stats(opaque=1.0, b1=0.3), 1000, GAIN, OPAQUE) == 128          # 128 and 192 both read eighth 1: the smaller


def test_gain_threshold_vetoes():
    assert dmpigo.depth_split_of(_stats(b4=0.0499), 256, GAIN, OPAQUE) == 0
    assert dmpigo.depth_split_of(_stats(b4=0.05), 256, GAIN, OPAQUE) == 128                         # at the threshold: split
    assert dmpigo.depth_split_of(_stats(b4=0.05), 256, 0.051, OPAQUE) == 0
    assert dmpigo.depth_split_of(_stats(), 256, 0.0, 0.0) == 0                                      # no gain anywhere: nothing to choose


def test_opaque_share_threshold_vetoes():
    assert dmpigo.depth_split_of(_stats(opaque=0.499, b4=0.9), 256, GAIN, OPAQUE) == 0
    assert dmpigo.depth_split_of(_stats(opaque=0.5, b4=0.9), 256, GAIN, OPAQUE) == 128
    assert dmpigo.depth_split_of(_stats(opaque=0.16, b4=0.9), 256, GAIN, OPAQUE) == 0              # the bench scene's share
    assert dmpigo.depth_split_of(_stats(opaque=0.16, b4=0.9), 256, GAIN, 0.1) == 128


def test_largest_gain_wins_and_ties_keep_the_smallest_k():
    assert dmpigo.depth_split_of(_stats(b2=0.3, b4=0.3, b6=0.3), 256, GAIN, OPAQUE) == 64
    assert dmpigo.depth_split_of(_stats(b2=0.3, b4=0.31, b6=0.31), 256, GAIN, OPAQUE) == 128
    assert dmpigo.depth_split_of(_stats(b2=0.3, b4=0.2, b6=0.31), 256, GAIN, OPAQUE) == 192
    assert dmpigo.depth_split_of(_stats(b1=0.9, b3=0.9, b5=0.9, b7=0.9, b6=0.1), 256, GAIN, OPAQUE) == 192      # eighths nobody reads do not compete


def test_result_is_zero_or_a_multiple_of_64_below_n_samples():
    rng = np.random.default_rng(5)
    seen = set()
    for n in list(range(2, 700, 7)) + [64, 65, 128, 129, 199, 256, 319, 512, 513]:
        for _ in range(6):
            st = rng.random(8).tolist()
            k = dmpigo.depth_split_of(st, n, float(rng.random() * 0.5), float(rng.random() * 0.8))
            assert isinstance(k, int) and k % 64 == 0 and 0 <= k < max(n, 1), (n, k)
            seen.add(k)
    assert {0, 64, 128, 192, 256} <= seen


# ---------------------------------------------------------------------------------------------------------------------
# the statistic's fp64 restatement
# ---------------------------------------------------------------------------------------------------------------------
def test_oracle_on_a_hand_worked_grid():
    """Z = 8 (one plane per eighth), interval 1, act_shift 0, thres 0.01.  Density +20 is alpha = 1 (a stop), 0 is alpha = 1/2 (ten of them
    stop: 2^-10 < 1e-3), -20 is empty.
      column A: opaque plane 2, half-alpha planes 5, 6        -> stops, zs = 3; voxels 3
      column B: half-alpha planes 1, 7                        -> never stops;   voxels 2
      column C: empty                                         -> not counted
      column D: half-alpha planes 0..7 (T = 2^-8: no stop)    -> never stops;   voxels 8
    13 voxels in 3 columns, 1 stops.  Column A alone has zs <= b for b = 3..7: voxels at or behind b: 2, 2, 2, 1, 0."""
    d = np.full((4, 8), -20.0)
    d[0, 2] = 20.0
    d[0, 5:7] = 0.0
    d[1, [1, 7]] = 0.0
    d[3, :] = 0.0
    s = DSO.stats(d, np.zeros(8), 1.0, 0.01)
    assert s['zs'].tolist() == [3, 8, 8, 8] and s['columns'] == 3 and s['voxels'] == 13
    assert s['num'].tolist() == [1, 0, 0, 2, 2, 2, 1, 0]
    want = np.array([1 / 3, 0, 0, 2 / 13, 2 / 13, 2 / 13, 1 / 13, 0], dtype=np.float32)
    assert np.array_equal(DSO.expected(s), want)


def test_oracle_nearest_act_plane():
    assert [DSO.act_plane(z, 9, 5) for z in range(9)] == [0, 1, 1, 2, 2, 3, 3, 4, 4]               # z / 2 + 1/2, halves upward
    assert [DSO.act_plane(z, 8, 8) for z in range(8)] == list(range(8))
    assert DSO.act_plane(99, 100, 40) == 39 and DSO.act_plane(0, 100, 40) == 0 and DSO.act_plane(0, 1, 4) == 0


@pytest.mark.parametrize('name', [c[0] for c in DSO.STATS_CASES])
def test_stats_inputs_keep_clear_of_both_thresholds(name):
    """What makes the GPU comparison exact: on the fp64 reference no alpha lies within 1e-3 (relative) of the threshold and no running T within
    1e-3 of the 1e-3 stop -- fp32 evaluation (exp / pow to an ulp or two, up to 256 roundings of the T chain: < 1e-4 relative) decides alike."""
    d, act, interval, thres = DSO.stats_case(name)
    s = DSO.stats(d, act, interval, thres)
    print(name, 'alpha margin', s['alpha_margin'], 'T margin', s['T_margin'], 'columns', s['columns'], 'voxels', s['voxels'], s['num'].tolist())
    assert s['alpha_margin'] > 1e-3 and s['T_margin'] > 1e-3
    kind = next(c[4] for c in DSO.STATS_CASES if c[0] == name)
    if kind == 'empty':
        assert s['columns'] == 0 and not DSO.expected(s).any()
    elif kind == 'stop0':
        assert (s['zs'] == 1).all() and s['num'][0] == s['columns'] == d.shape[0] * d.shape[1] and s['num'][1] > 0
    else:
        assert s['columns'] > 0 and s['voxels'] > 0
        if d.shape[0] * d.shape[1] > 1:                                 # the case is not trivial: stopped and unstopped columns, gains that differ
            assert 0 < s['num'][0] < s['columns'] and len(set(s['num'][1:].tolist())) > 2
