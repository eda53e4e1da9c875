"""fp64 restatement of k4_mpi_depth_split_stats (include/k4nerf.h) and of the inputs its tests use.  Test infrastructure only.

Per (x, y) column of an MPI density grid [X, Y, Z], planes z ascending:
  alpha[z] = raw2alpha(density[z] + act_shift[plane of z], 0, interval) = 1 - (1 + exp(.))^-interval
  T        = running product of (1 - alpha); the column STOPS at the first plane where T < 1e-3, zs = that plane + 1 (Z: it never stops)
  cnt[e]   = planes with alpha > thres in depth eighth e = min(7, 8 z // Z)
A column with no alpha-passing plane does not count at all.  Over the others:
  out[0] = (columns that stop) / (columns)
  out[b] = (alpha-passing voxels in eighths b..7 of the columns with zs <= b * Z // 8) / (alpha-passing voxels), b = 1..7
The kernel's sums are integer-valued floats (exact below 2^24) and each output is ONE fp32 quotient of two of them, so `expected()` is
what it must return to the bit -- provided no alpha sits at `thres` and no running T at 1e-3 closer than fp32 rounding can move them:
`stats()` reports both margins and the tests assert them on their inputs."""
import numpy as np


def act_plane(z, Z, D):
    """Plane of the act_shift grid [D] that density plane z of Z reads: itself when D == Z, else the nearest (align_corners) --
    floor(z (D - 1) / max(Z - 1, 1) + 1/2) in integers."""
    if D == Z:
        return z
    den = max(Z - 1, 1)
    return min(D - 1, (2 * z * (D - 1) + den) // (2 * den))


def stats(density, act_shift, interval, thres):
    """density [X, Y, Z] (or [n, Z]) and act_shift [D], any float type -> dict of the integer counts and the two margins."""
    d = np.asarray(density, dtype=np.float64)
    Z = d.shape[-1]
    d = d.reshape(-1, Z)
    act = np.asarray(act_shift, dtype=np.float64).reshape(-1)
    D = act.shape[0]
    n = d.shape[0]
    T = np.ones(n)
    zs = np.full(n, Z, dtype=np.int64)
    cnt = np.zeros((n, 8), dtype=np.int64)
    alpha_margin, T_margin = np.full(n, np.inf), np.full(n, np.inf)     # per column
    for z in range(Z):
        e = np.exp(d[:, z] + act[act_plane(z, Z, D)])
        a = 1.0 - np.power(1.0 + e, -float(interval))
        alpha_margin = np.minimum(alpha_margin, np.abs(a / thres - 1.0))
        cnt[:, min(7, z * 8 // Z)] += a > thres
        run = zs == Z                                       # the scan goes on until the stop; the crossing plane is its last
        T = np.where(run, T * (1.0 - a), T)
        T_margin = np.where(run, np.minimum(T_margin, np.abs(T / 1e-3 - 1.0)), T_margin)
        zs = np.where(run & (T < 1e-3), z + 1, zs)
    tot = cnt.sum(1)
    occ = tot > 0
    behind = np.cumsum(cnt[:, ::-1], axis=1)[:, ::-1]      # behind[:, b] = voxels in eighths b..7
    num = np.zeros(8, dtype=np.int64)
    num[0] = int((occ & (zs < Z)).sum())
    for b in range(1, 8):
        num[b] = int(behind[occ & (zs <= b * Z // 8), b].sum())
    return {'num': num, 'voxels': int(tot[occ].sum()), 'columns': int(occ.sum()), 'zs': zs, 'cnt': cnt,
            'alpha_margin': float(alpha_margin.min()), 'T_margin': float(T_margin.min()), 'margin_per_column': np.minimum(alpha_margin, T_margin)}


def expected(s):
    """out16[0:8] of the kernel from the counts of `stats`: single fp32 quotients of exact integers (0 where nothing is occupied)."""
    assert max(int(s['num'].max()), s['voxels'], s['columns']) < 2 ** 24
    out = np.zeros(8, dtype=np.float32)
    if s['columns'] > 0:
        out[0] = np.float32(s['num'][0]) / np.float32(s['columns'])
        for b in range(1, 8):
            out[b] = np.float32(s['num'][b]) / np.float32(s['voxels'])
    return out


def make_columns(n, Z, seed, kind='mixed'):
    """density [n, Z] float32 of the tests: background -10, occupied voxels +2 .. +22, opaque sheets of +22 (three planes).
    kind 'mixed': a third of the columns empty, a third with scattered occupied voxels (translucent or not, as the draw falls),
    a third with a sheet at a random plane behind a few scattered voxels; 'empty': background only; 'stop0': a sheet from plane 0 in
    every column and scattered voxels behind it."""
    rng = np.random.default_rng(seed)
    d = np.full((n, Z), -10.0, dtype=np.float32)
    if kind == 'empty':
        return d
    scatter = rng.random((n, Z)) < (min(0.25, 3.0 / Z) if kind == 'mixed' else 0.3)       # mixed: about three voxels per column, so that not every column stops
    vals = rng.choice(np.array([2.0, 3.0, 4.0, 6.0, 9.0, 14.0, 22.0], dtype=np.float32), size=(n, Z), p=[.3, .25, .2, .1, .05, .05, .05])
    vals = (vals + rng.uniform(0.0, 0.5, size=(n, Z))).astype(np.float32)
    d[scatter] = vals[scatter]
    if kind == 'stop0':
        d[:, :min(3, Z)] = 22.0
        return d
    role = np.arange(n) % 3 if n >= 3 else np.full(n, 2)
    rng.shuffle(role)
    d[role == 0] = -10.0
    for c in np.nonzero(role == 2)[0]:
        z0 = int(rng.integers(0, Z))
        d[c, z0:z0 + 3] = 22.0
    return d


def mpi_act_shift(D, ratio):
    """DirectMPIGO's per-plane density bias (lib/dmpigo.py:48-58) in fp64 -> float32 [D]."""
    g = np.full([D], 1.0 / D - 1e-6)
    keep = [1 - g[0]] + [(1 - g[:i + 1].sum()) / (1 - g[:i].sum()) for i in range(1, D)]
    return np.array([np.log(p ** (-1.0 / ratio) - 1.0) for p in keep], dtype=np.float32)


# (name, (X, Y), Z, act_depth, kind): every Z with every column count (1 thread, one short of / one past a 64-thread block, 36 blocks); Z = 9 and
# 100 are no multiples of 8 (uneven z * 8 // Z eighths); the grids without an occupied voxel and with every column stopped by plane 0; one
# act_depth != Z (nearest-plane branch)
STATS_CASES = [(f'z{Z}_n{X * Y}', (X, Y), Z, Z, 'mixed') for Z in (8, 9, 64, 100, 256) for (X, Y) in ((1, 1), (7, 9), (5, 13), (48, 48))]
STATS_CASES += [('empty', (5, 13), 64, 64, 'empty'), ('stop0', (5, 13), 64, 64, 'stop0'), ('stop0_z9', (7, 9), 9, 9, 'stop0'),
                ('act40_z100', (5, 13), 100, 40, 'mixed'), ('act5_z9', (7, 9), 9, 5, 'mixed')]


def stats_case(name):
    """-> (density [X, Y, Z] float32, act_shift [D] float32, interval, thres) of a STATS_CASES entry: the model's own interval and threshold
    for a grid of Z planes at stepsize 1 (256 / Z, 1 / (5 Z): configs/llff/llff_default_lg.py)."""
    _, (X, Y), Z, D, kind = next(c for c in STATS_CASES if c[0] == name)
    seed = 1000 + sum(ord(ch) for ch in name)
    d = make_columns(X * Y, Z, seed, kind)
    act, interval, thres = mpi_act_shift(D, 256.0 / D), float(np.float32(256.0 / Z)), float(np.float32(1.0 / (5 * Z)))
    for _ in range(8):          # a column whose reference comes near one of the two thresholds gets its occupied voxels nudged until none does
        near = stats(d, act, interval, thres)['margin_per_column'] < 5e-3
        if not near.any():
            break
        d[near] = np.where(d[near] > 0, d[near] + np.float32(0.37), d[near])
    return d.reshape(X, Y, Z), act, interval, thres
