"""fp64 restatement of the reference's TensoRFGrid (lib/grid.py:157-268): lookup, its gradients, total variation, dense expansion, resize.
TEST INFRASTRUCTURE ONLY.  Corner and weight arithmetic is written out here (no ``F.grid_sample`` / ``F.interpolate`` / autograd): bilinear,
``align_corners=True``, zero padding per lookup; a vector's size-1 axis resolves to index 0 with weight 1.  Held to the reference-made goldens by
tests/test_tensorf_cpu.py."""
import torch

FACTORS = ('xy_plane', 'xz_plane', 'yz_plane', 'x_vec', 'y_vec', 'z_vec')
# group -> (plane, its two axes, vector, its axis): f_vec rows in this order
GROUPS = (('xy_plane', 0, 1, 'z_vec', 2), ('xz_plane', 0, 2, 'y_vec', 1), ('yz_plane', 1, 2, 'x_vec', 0))


def _axes(sd, pts):
    """Per axis: (i0, i1, w0, w1) with out-of-range nodes at index 0 / weight 0."""
    X, Y = sd['xy_plane'].shape[2:]
    Z = sd['xz_plane'].shape[3]
    lo, hi = sd['xyz_min'].double(), sd['xyz_max'].double()
    out = []
    for a, size in enumerate((X, Y, Z)):
        u = ((pts[:, a].double() - lo[a]) / (hi[a] - lo[a]) * 2 - 1 + 1) / 2 * (size - 1)
        f = torch.floor(u)
        i0, i1 = f.long(), f.long() + 1
        ok0, ok1 = (i0 >= 0) & (i0 < size), (i1 >= 0) & (i1 < size)
        out.append((torch.where(ok0, i0, 0), torch.where(ok1, i1, 0), torch.where(ok0, f + 1 - u, 0.), torch.where(ok1, u - f, 0.)))
    return out


def _interp(sd, pts):
    """-> per group (plane values [n, R], vector values [n, R], plane corner terms, vector node terms) in fp64."""
    ax = _axes(sd, pts)
    res = []
    for pk, a, b, vk, v in GROUPS:
        P, V = sd[pk].double()[0], sd[vk].double()[0, :, :, 0]          # [R, A, B], [R, L]
        (a0, a1, wa0, wa1), (b0, b1, wb0, wb1), (v0, v1, wv0, wv1) = ax[a], ax[b], ax[v]
        corners = [(a0, b0, wa0 * wb0), (a0, b1, wa0 * wb1), (a1, b0, wa1 * wb0), (a1, b1, wa1 * wb1)]
        nodes = [(v0, wv0), (v1, wv1)]
        pv = sum(P[:, i, j].T * w[:, None] for i, j, w in corners)
        vv = sum(V[:, i].T * w[:, None] for i, w in nodes)
        res.append((pv, vv, corners, nodes))
    return res


def lookup(sd, pts):
    """[n, C] (C == 1 without f_vec)."""
    feat = torch.cat([pv * vv for pv, vv, _, _ in _interp(sd, pts)], 1)
    return feat @ sd['f_vec'].double() if 'f_vec' in sd else feat.sum(1, keepdim=True)


def gradients(sd, pts, go):
    """d sum(out * go) / d every parameter, by the chain rule written out."""
    go = go.double()
    grads = {}
    parts = _interp(sd, pts)
    if 'f_vec' in sd:
        fv = sd['f_vec'].double()
        feat = torch.cat([pv * vv for pv, vv, _, _ in parts], 1)
        grads['f_vec'] = feat.T @ go
        gfeat = go @ fv.T                                                 # [n, rows]
    row = 0
    for (pk, a, b, vk, v), (pv, vv, corners, nodes) in zip(GROUPS, parts):
        R = pv.shape[1]
        g = gfeat[:, row:row + R] if 'f_vec' in sd else go.expand(-1, R)
        row += R
        gp = torch.zeros_like(sd[pk].double())
        for i, j, w in corners:
            gp[0].index_put_((torch.arange(R)[None, :].expand(len(w), R), i[:, None].expand(-1, R), j[:, None].expand(-1, R)), (g * vv) * w[:, None], accumulate=True)
        gv = torch.zeros_like(sd[vk].double())
        for i, w in nodes:
            gv[0, :, :, 0].index_put_((torch.arange(R)[None, :].expand(len(w), R), i[:, None].expand(-1, R)), (g * pv) * w[:, None], accumulate=True)
        grads[pk], grads[vk] = gp, gv
    return grads


def dense(sd):
    xy, xz, yz = (sd[k].double()[0] for k in FACTORS[:3])
    xv, yv, zv = (sd[k].double()[0, :, :, 0] for k in FACTORS[3:])
    feat = torch.cat([xy[:, :, :, None] * zv[:, None, None, :], xz[:, :, None, :] * yv[:, None, :, None], yz[:, None, :, :] * xv[:, :, None, None]])
    if 'f_vec' in sd:
        return torch.tensordot(sd['f_vec'].double().T, feat, dims=1)[None]
    return feat.sum(0)[None, None]


def tv_grad(sd, wx, wy, wz):
    """Gradient of the total variation term (smooth-L1, beta 1, summed; / 6) w.r.t. the six factors."""
    w = {'xy_plane': (wx, wy), 'xz_plane': (wx, wz), 'yz_plane': (wy, wz), 'x_vec': (wx, 0.), 'y_vec': (wy, 0.), 'z_vec': (wz, 0.)}
    out = {}
    for k in FACTORS:
        p = sd[k].double()
        g = torch.zeros_like(p)
        for dim, wk in zip((2, 3), w[k]):
            if p.shape[dim] < 2:
                continue
            d = p.narrow(dim, 1, p.shape[dim] - 1) - p.narrow(dim, 0, p.shape[dim] - 1)
            dd = torch.where(d.abs() < 1, d, torch.sign(d)) * wk
            g.narrow(dim, 1, p.shape[dim] - 1).add_(dd)
            g.narrow(dim, 0, p.shape[dim] - 1).sub_(dd)
        out[k] = g / 6
    return out


def _resize1(p, dim, new):
    old = p.shape[dim]
    if new == 1 and old == 1:
        return p
    scale = (old - 1) / (new - 1) if new > 1 else 0.
    src = torch.arange(new, dtype=torch.float64) * scale
    i0 = src.floor().long().clamp(max=old - 1)
    i1 = (i0 + 1).clamp(max=old - 1)
    lam = src - i0
    shape = [1] * p.dim()
    shape[dim] = new
    return p.index_select(dim, i0) * (1 - lam).reshape(shape) + p.index_select(dim, i1) * lam.reshape(shape)


def resize(sd, new_world):
    X, Y, Z = new_world
    sizes = {'xy_plane': (X, Y), 'xz_plane': (X, Z), 'yz_plane': (Y, Z), 'x_vec': (X, 1), 'y_vec': (Y, 1), 'z_vec': (Z, 1)}
    return {k: _resize1(_resize1(sd[k].double(), 2, sizes[k][0]), 3, sizes[k][1]) for k in FACTORS}


# ---------------------------------------------------------------------------------------------------------------- golden access
def load_grid_case(name):
    """One case of tests/golden/tensorf_grid.npz -> dict: 'sd', 'tvsd' (state dicts), 'config', 'channels', 'world', 'keys', and the flat arrays
    ('pts', 'go', 'out', 'grad/<param>', 'cell_*', 'dense', 'tv/<factor>', 'scaled/<factor>') with ``tol(key)``."""
    import json
    import os
    import numpy as np
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'tensorf_grid.npz'), allow_pickle=False)
    pre = name + '/'
    c = {'sd': {}, 'tvsd': {}, 'arr': {}, 'err32': {}, 'rnd': {}}
    for k in z.files:
        if not k.startswith(pre):
            continue
        r = k[len(pre):]
        for sec in ('sd', 'tvsd', 'err32', 'rnd'):
            if r.startswith(sec + '/'):
                c[sec][r[len(sec) + 1:]] = torch.from_numpy(z[k]) if sec in ('sd', 'tvsd') else float(z[k])
                break
        else:
            c['arr'][r] = z[k]
    c['config'], c['keys'] = json.loads(str(c['arr'].pop('config'))), json.loads(str(c['arr'].pop('keys')))
    c['channels'], c['world'] = int(c['arr'].pop('channels')), [int(v) for v in c['arr'].pop('world')]
    return c


def tol(case, key):
    """4 x the fp32 reference's own distance from the fp64 expectation, less the rounding of an expectation stored in fp32."""
    return 4 * case['err32'][key] - case['rnd'].get(key, 0.0)


def check(case, key, got, what=''):
    """Print the figure, then hold `got` to the golden `key` within tol."""
    want = torch.from_numpy(case['arr'][key]).double()
    got = got.detach().cpu().double().reshape(want.shape)
    err = float((got - want).abs().max()) if want.numel() else 0.0
    t = tol(case, key)
    print(f'{what}{key}: max |got - fp64 reference| = {err:.3e}, tolerance 4 x err32 = {t:.3e}')
    assert err <= t, (what, key, err, t)
