"""CPU restatement, in fp32 torch, of the reference's ``VQGrid.forward`` (lib/grid.py:60-103, eval and training mode) and ``DirectQVGO.forward``
(lib/dvqgo.py:279-408).  TEST INFRASTRUCTURE ONLY.  The marcher pieces (NDC sampler, mask lookup, trilinear gather, raw2alpha, alpha2weight, positional
embedding, MLP, segment sum) are those of oracle/marcher.py / oracle/native_cpu.py; ``tests/test_vq_cpu.py`` pins this file against goldens made by the
reference's own classes (tests/gen_vq_golden.py).  The expressions work on tensors of any device (tools/dvqgo_call_time.py times them on the GPU).
"""
import torch
import torch.nn.functional as F


def vq_state(sd, prefix=''):
    """The seven tensors of a VQGrid from a state dict (keys as lib/grid.py:46-58 registers them), as copies."""
    keys = ('embed', 'cluster_size', 'embed_avg', 'project_layer.0.weight', 'project_layer.0.bias', 'project_layer.2.weight', 'project_layer.2.bias')
    return {k: sd[prefix + k].float().clone() for k in keys}


def vq_project(st, x):
    h = F.relu(F.linear(x, st['project_layer.0.weight'], st['project_layer.0.bias']))
    return F.linear(h, st['project_layer.2.weight'], st['project_layer.2.bias'])


def vq_dist(st, flatten):
    embed = st['embed']
    return flatten.pow(2).sum(1, keepdim=True) - 2 * flatten @ embed + embed.pow(2).sum(0, keepdim=True)


def vq_forward(st, x, training=False, decay=0.99, eps=1e-5, aux=None):
    """-> (quantize, diff, embed_ind).  training: ``st``'s three buffers are replaced by their values after the update (new tensors; the features come
    from the old codebook).  aux: a dict that receives 'v' and, in training mode, the per-code counts and sums."""
    embed = st['embed']
    dim, n_embed = embed.shape
    vq_input = vq_project(st, x)
    flatten = vq_input.reshape(-1, dim)
    _, embed_ind = (-vq_dist(st, flatten)).max(1)
    quantize = F.embedding(embed_ind.view(*vq_input.shape[:-1]), embed.transpose(0, 1))
    if aux is not None:
        aux['v'] = vq_input
    if training:
        onehot = F.one_hot(embed_ind, n_embed).type(flatten.dtype)
        onehot_sum = onehot.sum(0)
        embed_sum = flatten.transpose(0, 1) @ onehot
        cluster_size = (st['cluster_size'] * decay).add(onehot_sum, alpha=1 - decay)
        embed_avg = (st['embed_avg'] * decay).add(embed_sum, alpha=1 - decay)
        n = cluster_size.sum()
        norm = (cluster_size + eps) / (n + n_embed * eps) * n
        st['cluster_size'], st['embed_avg'], st['embed'] = cluster_size, embed_avg, embed_avg / norm.unsqueeze(0)
        if aux is not None:
            aux['count'], aux['sum'] = onehot_sum, embed_sum
    diff = (quantize.detach() - vq_input).pow(2).mean()
    quantize = vq_input + (quantize - vq_input).detach()
    return quantize, diff, embed_ind.view(*vq_input.shape[:-1])


def forward(model_kwargs, sd, rays_o, rays_d, viewdirs, near=0, far=1, stepsize=1.0, bg=0, render_depth=False, aux=None, **_ignored):
    """DirectQVGO.forward in eval mode -> the reference's dict (+ 'rgb_feature', as the package returns it).  aux: receives 'step_id', the embedded
    positions 'pe_emb', the projected vectors 'v' and the chosen codes 'embed_ind' of the shaded samples."""
    from oracle import marcher, native_cpu as nat                    # (here: the codebook expressions above serve tools/ without the oracle package)
    assert near == 0 and far == 1                                    # lib/dvqgo.py:262
    rays_o, rays_d, viewdirs = rays_o.float().contiguous(), rays_d.float().contiguous(), viewdirs.float()
    N = rays_o.shape[0]
    xyz_min, xyz_max = sd['xyz_min'].float(), sd['xyz_max'].float()
    mpi_depth = int(model_kwargs['mpi_depth'])
    thres = float(model_kwargs.get('fast_color_thres', 0))
    N_samples = int((mpi_depth - 1) / stepsize) + 1                  # lib/dvqgo.py:265
    interval = stepsize * (256. / mpi_depth)                         # lib/dvqgo.py:293,152
    pts, mask_outbbox = nat.sample_ndc_pts_on_rays(rays_o, rays_d, xyz_min, xyz_max, N_samples)
    mask_inbbox = ~mask_outbbox
    ray_pts = pts.view(-1, 3)[mask_inbbox.view(-1)]
    ray_id = torch.arange(N).view(-1, 1).expand_as(mask_inbbox)[mask_inbbox]
    step_id = torch.arange(N_samples).view(1, -1).expand_as(mask_inbbox)[mask_inbbox]
    mask1 = marcher.mask_grid(sd['mask_cache.mask'], ray_pts, sd['mask_cache.xyz2ijk_scale'].float(), sd['mask_cache.xyz2ijk_shift'].float())
    ray_pts, ray_id, step_id = ray_pts[mask1], ray_id[mask1], step_id[mask1]
    density = marcher.dense_grid(sd['density.grid'].float(), ray_pts, xyz_min, xyz_max) \
        + marcher.dense_grid(sd['act_shift.grid'].float(), ray_pts, xyz_min, xyz_max)
    _, alpha = nat.raw2alpha(density.flatten(), 0, interval)
    if thres > 0:
        mask2 = alpha > thres
        ray_pts, ray_id, step_id, alpha = ray_pts[mask2], ray_id[mask2], step_id[mask2], alpha[mask2]
    weights, _, alphainv_last, _, _ = nat.alpha2weight(alpha, ray_id, N)
    if thres > 0:
        mask3 = weights > thres
        ray_pts, ray_id, step_id, alpha, weights = ray_pts[mask3], ray_id[mask3], step_id[mask3], alpha[mask3], weights[mask3]
    # colour (lib/dvqgo.py:322-368)
    pe_spa = ((ray_pts - xyz_min) / (xyz_max - xyz_min)).flip((-1,)) * 2 - 1
    pe_emb = marcher._pe(pe_spa, sd['posfreq'].float())
    sub = {} if aux is not None else None
    vq_emb, _, embed_ind = vq_forward(vq_state(sd, 'k0.'), pe_emb, aux=sub)
    viewdirs_emb = marcher._pe(viewdirs, sd['viewfreq'].float())[ray_id]
    rgb = torch.sigmoid(marcher._mlp(marcher._rgbnet_layers(sd), torch.cat([vq_emb, pe_emb, viewdirs_emb], -1)))
    rgb_marched = marcher._segment_sum(weights.unsqueeze(-1) * rgb, ray_id, N)
    rgb_marched += alphainv_last.unsqueeze(-1) * bg
    s = (step_id + 0.5) / N_samples
    ret = {'alphainv_last': alphainv_last, 'weights': weights, 'rgb_marched': rgb_marched, 'rgb_feature': rgb_marched, 'raw_alpha': alpha,
           'raw_rgb': rgb, 'ray_id': ray_id, 'n_max': N_samples, 's': s}
    if render_depth:
        ret['depth'] = marcher._segment_sum(weights * s, ray_id, N)
    if aux is not None:
        aux.update(step_id=step_id, pe_emb=pe_emb, v=sub['v'], embed_ind=embed_ind)
    return ret
