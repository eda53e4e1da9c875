"""Checker of the perceptual / style terms (4k-nerf_amd/lib/sr_loss.py).  TEST INFRASTRUCTURE ONLY: pure torch on the CPU, fp64 by default.

The VGG19 stack up to a requested layer, the two loss terms as lib/sr_loss.py:134-161, 175-188 of the reference states them

    percep = perceptual_weight * sum_k w_k * mean|f_k(x) - f_k(gt)|,   style = style_weight * sum_k w_k * mean|G(f_k(x)) - G(f_k(gt))|,   G(f) = f f^T / (c h w)

and ``grad_with_record``: the gradient to ``x`` evaluated with a GIVEN set of decisions -- ReLU masks, pool choices, signs of the feature
differences, signs of the Gram differences -- instead of the checker's own.  The two terms are piecewise smooth in ``x``; two correct
evaluations in different arithmetic land on different pieces wherever a pre-activation, a pool gap or a difference is within rounding of
zero, and the gradients of neighbouring pieces differ by far more than rounding.  With the decisions fixed, the gradient is a smooth
function of the inputs and can be compared tightly.
"""
import torch
import torch.nn.functional as F

BLOCKS = ((64, 64), (128, 128), (256, 256, 256, 256), (512, 512, 512, 512), (512, 512, 512, 512))
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def layer_names():
    out = []
    for b, ws in enumerate(BLOCKS, 1):
        for j in range(1, len(ws) + 1):
            out += [f'conv{b}_{j}', f'relu{b}_{j}']
        out.append(f'pool{b}')
    return out


NAMES = layer_names()


def params_from_torchvision(sd, dtype=torch.float64):
    """{conv name: (weight, bias)} from ``features.<i>.weight`` / ``.bias`` keys."""
    return {n: (sd[f'features.{i}.weight'].to(dtype), sd[f'features.{i}.bias'].to(dtype)) for i, n in enumerate(NAMES) if n.startswith('conv') and f'features.{i}.weight' in sd}


def _windows(x):
    """[1, C, H, W] -> [1, C, H/2, W/2, 4], candidate k = dy * 2 + dx."""
    return torch.stack([x[..., dy::2, dx::2] for dy in (0, 1) for dx in (0, 1)], -1)


def first_max(cands):
    """Index of the FIRST maximum along the last axis in candidate order (aten max_pool2d replaces its maximum on `>` only)."""
    best, idx = cands[..., 0], torch.zeros(cands.shape[:-1], dtype=torch.uint8)
    for k in range(1, cands.shape[-1]):
        take = cands[..., k] > best
        best, idx = torch.where(take, cands[..., k], best), torch.where(take, torch.full_like(idx, k), idx)
    return idx


def run_stack(x, params, upto, record=None, use_input_norm=True):
    """The stack up to layer `upto` on x [1, 3, H, W].  record None: the checker's own decisions (max(v, 0), max pool); else ReLU = v * relu_mask[conv name],
    pool = the candidate pool_choice[pool name] names.  Returns {'out': {every layer name: tensor}, 'cands': {pool name: windows of its input}}."""
    dt = x.dtype
    if use_input_norm:
        x = (x - torch.tensor(MEAN).to(dt).view(1, 3, 1, 1)) / torch.tensor(STD).to(dt).view(1, 3, 1, 1)          # the fp32 buffers of the module, widened
    out, cands = {}, {}
    for n in NAMES[:NAMES.index(upto) + 1]:
        if n.startswith('conv'):
            w, b = params[n]
            x = F.conv2d(x, w.to(dt), b.to(dt), 1, 1)
        elif n.startswith('relu'):
            x = torch.relu(x) if record is None else x * record['relu_mask']['conv' + n[4:]].to(dt)
        else:
            c = _windows(x)
            cands[n] = c
            x = c.max(-1).values if record is None else c.gather(-1, record['pool_choice'][n].long().unsqueeze(-1)).squeeze(-1)
        out[n] = x
    return {'out': out, 'cands': cands}


def gram(f):
    """lib/sr_loss.py:184-187."""
    n, c, h, w = f.size()
    features = f.view(n, c, w * h)
    return features.bmm(features.transpose(1, 2)) / (c * h * w)


def _taps(layer_weights):
    return sorted(((n, float(w)) for n, w in layer_weights.items() if w != 0), key=lambda t: NAMES.index(t[0]))


def losses(x, gt, params, layer_weights, perceptual_weight, style_weight, record=None, use_input_norm=True, detail=False):
    """(percep, style) -- tensors; a term whose weight is not > 0 is None.  With `record`: every decision taken from it (the x image's masks and choices;
    |d| = sign * d for the feature and Gram differences).  detail: also the traces of both images and the Gram matrices."""
    taps = _taps(layer_weights)
    upto = taps[-1][0]
    tx = run_stack(x, params, upto, record, use_input_norm)
    tg = run_stack(gt.detach(), params, upto, None, use_input_norm)
    percep = x.new_zeros(()) if perceptual_weight > 0 else None
    style = x.new_zeros(()) if style_weight > 0 else None
    grams = {}
    for n, wk in taps:
        fx, fg = tx['out'][n], tg['out'][n]
        if percep is not None:
            d = fx - fg
            percep = percep + (d.abs().mean() if record is None else (record['feat_sign'][n].to(x.dtype) * d).mean()) * wk
        if style is not None:
            gx, gg = gram(fx), gram(fg)
            grams[n] = (gx, gg)
            d = gx - gg
            style = style + (d.abs().mean() if record is None else (record['gram_sign'][n].to(x.dtype).view_as(d) * d).mean()) * wk
    if percep is not None:
        percep = percep * perceptual_weight
    if style is not None:
        style = style * style_weight
    if detail:
        return percep, style, {'x': tx, 'gt': tg, 'grams': grams}
    return percep, style


def decisions(x, gt, params, layer_weights, style=True, use_input_norm=True):
    """The checker's own decisions in the layout of ``PerceptualLoss.k4_record``, and the quantities whose sign or order they are:
    (record, margins) with margins = {'relu_mask': {conv: pre-activation}, 'pool_choice': {pool: windows [.., 4]}, 'feat_sign': {k: f(x) - f(gt)}, 'gram_sign': {k: G(x) - G(gt)}}."""
    taps = _taps(layer_weights)
    with torch.no_grad():
        tx = run_stack(x, params, taps[-1][0], None, use_input_norm)
        tg = run_stack(gt, params, taps[-1][0], None, use_input_norm)
    rec = {'relu_mask': {}, 'pool_choice': {}, 'feat_sign': {}, 'gram_sign': {}}
    mar = {'relu_mask': {}, 'pool_choice': {}, 'feat_sign': {}, 'gram_sign': {}}
    for n, v in tx['out'].items():
        if n.startswith('relu'):
            pre = tx['out']['conv' + n[4:]]
            rec['relu_mask']['conv' + n[4:]], mar['relu_mask']['conv' + n[4:]] = pre > 0, pre
        elif n.startswith('pool'):
            rec['pool_choice'][n], mar['pool_choice'][n] = first_max(tx['cands'][n]), tx['cands'][n]
    for n, _ in taps:
        d = tx['out'][n] - tg['out'][n]
        rec['feat_sign'][n], mar['feat_sign'][n] = torch.sign(d).to(torch.int8), d
        if style:
            dg = (gram(tx['out'][n]) - gram(tg['out'][n]))[0]
            rec['gram_sign'][n], mar['gram_sign'][n] = torch.sign(dg).to(torch.int8), dg
    return rec, mar


def grad_autograd(x, gt, params, layer_weights, perceptual_weight, style_weight, use_input_norm=True):
    """d(percep + style) / dx by autograd through the plain formulas."""
    xi = x.detach().clone().requires_grad_(True)
    p, s = losses(xi, gt, params, layer_weights, perceptual_weight, style_weight, None, use_input_norm)
    total = sum(t for t in (p, s) if t is not None)
    return torch.autograd.grad(total, xi)[0]


def grad_with_record(x, gt, params, record, layer_weights=None, perceptual_weight=1.0, style_weight=0.0, use_input_norm=True):
    """d(percep + style) / dx on the piece of the function that `record` names: ReLU = multiplication by the recorded mask, pool = the recorded candidate,
    |d| = recorded sign * d.  Fed the checker's own decisions it is the plain gradient."""
    record = {k: {n: torch.as_tensor(v).cpu() for n, v in d.items()} for k, d in record.items()}
    xi = x.detach().clone().requires_grad_(True)
    p, s = losses(xi, gt, params, layer_weights, perceptual_weight, style_weight, record, use_input_norm)
    total = sum(t for t in (p, s) if t is not None)
    return torch.autograd.grad(total, xi)[0]
