"""The 'sparse' grid route under a gradient exchange, on ONE GPU: a world-size-1 `nccl` process group with _native.FORCE_COLLECTIVES, so that
JointTrainer.step runs the production collectives of joint_train.exchange_gradients.  Four steps (step 1 with dense total variation, steps 2-4 without) from
the same state in four forms:
  (i)   no exchange                                     -- k0 stepped from the scatter's scratch image, as in a single-process job
  (ii)  exchange, image route on                        -- the lists are sent from the image and merged back into it (lib/grid.GridGrad.exchange)
  (iii) exchange, joint_train._SPARSE_IMAGE_EXCHANGE off -- the dense gradient, sparse_grad_allreduce, the dense masked step
  (iv)  as (ii) with the scratch image withheld from the lookups' backward: this rank's gradient is a dense tensor, the same message still travels
and two comparisons from IDENTICAL inputs, where the forms must agree bit for bit (the scatter's atomics reorder sums between runs, so whole runs agree
to 1e-5 only): one scatter image handed to the image route + in-place step and to sweep + sparse_grad_allreduce + dense masked step; one dense gradient
handed to the exchange of (iv) and to that of (iii).  Prints one JSON line; tests/test_dp_sparse_route_gpu.py runs it in a subprocess."""
import json, os, socket, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import torch.distributed as dist


def main():
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    s = socket.socket(); s.bind(('127.0.0.1', 0)); port = s.getsockname()[1]; s.close()
    dist.init_process_group('nccl', init_method=f'tcp://127.0.0.1:{port}', world_size=1, rank=0, device_id=dev)
    import nerf4k_amd  # noqa: F401
    from nerf4k_amd import _native as N, scene, joint_train
    from nerf4k_amd.lib import dvgo, grid as G, masked_adam, sr_esrnet, utils
    masked_adam._MULTI_BELOW = 1000                              # the small scene's k0 takes the large-tensor path (side stream) like the 1.36 GB one
    joint_train.SPARSE_MIN_NUMEL = 4096                          # ... and the list exchange
    ck = scene.make_llff_checkpoint(seed=11, num_voxels=48 * 48 * 32, mpi_depth=32)
    H, W = 44, 60
    K = scene.LLFF_K.copy()
    K[:2] *= W / scene.LLFF_HW[1]
    pose = scene.llff_spiral_poses()[3]
    with torch.no_grad():
        rays = dvgo.get_rays_of_a_view(H, W, K, torch.from_numpy(pose).to(dev), True, False, False, False)
    gb = torch.Generator(device=dev).manual_seed(9)
    batch = [x[8:24, 20:36].reshape(-1, 3).contiguous() for x in rays] + [torch.rand([256, 3], device=dev, generator=gb),
                                                                         torch.rand([4096, 3], device=dev, generator=gb), 16, 16]
    cfg = joint_train.JointCfg.fern_lg_joint_l1(tv_before=2, tv_dense_before=2)

    def fresh():
        m = utils.model_from_checkpoint_dict(ck).to(dev).train()
        torch.manual_seed(31)
        n2 = sr_esrnet.SFTNet(3, scale=4, num_feat=64, num_block=2, num_grow_ch=32, num_cond=1).to(dev).train()
        return m, n2, joint_train.JointTrainer(m, n2, cfg, dict(ck['render_kwargs'], render_depth=True), n_train_images=17)

    route_backward = G.GridGrad.backward

    def backward_without_image(self, *a):
        keep = G._scratch_image
        G._scratch_image = lambda *b, **k: None
        try:
            return route_backward(self, *a)
        finally:
            G._scratch_image = keep

    def image_all_zero():
        img = G._GSB_WS.get(dev)
        return img is None or int(img.ws.count_nonzero()) == 0

    forms = {}
    for name, force, image_route, withheld in (('i', False, True, False), ('ii', True, True, False), ('iii', True, False, False), ('iv', True, True, True)):
        N.FORCE_COLLECTIVES, joint_train._SPARSE_IMAGE_EXCHANGE = force, image_route
        G.GridGrad.backward = backward_without_image if withheld else route_backward
        G.release_grid_sample_workspace()
        m, n2, tr = fresh()
        assert [o is m.k0 for o in tr._sparse_grid_owners()] == [True]
        rec = {'loss': [], 'k0_grad': [], 'density_grad': [], 'idle': [], 'image_zero': [], 'image_bytes': [], 'image_touched': []}
        for i in range(4):
            rec['loss'].append(float(tr.step(*batch, global_step=1 + i)['total']))
            rec['k0_grad'].append(m.k0.grid.grad is not None)
            rec['density_grad'].append(m.density.grid.grad is not None)
            rec['idle'].append(bool(m.k0.grad_route.idle and not m.k0.grad_route.pending))
            m.k0.params_ready()
            torch.cuda.synchronize()
            rec['image_zero'].append(image_all_zero())
            ex = tr.last_exchange or {}
            rec['image_bytes'].append(int(ex.get('image_bytes_gathered', 0)))
            rec['image_touched'].append([[c, v] for c, v in ex.get('image_touched', [])])
        st = tr.optimizer.state[m.k0.grid]
        rec['k0_step'] = int(st['step'])
        tensors = {k: v.detach().clone() for k, v in m.state_dict().items() if v.is_floating_point()}
        tensors.update({f'decoder/{j}': p.detach().clone() for j, p in enumerate(n2.parameters())})
        tensors['k0/exp_avg'], tensors['k0/exp_avg_sq'] = st['exp_avg'].clone(), st['exp_avg_sq'].clone()
        forms[name] = (rec, tensors, (m, n2, tr))
    G.GridGrad.backward = route_backward

    def rel_err(a, b):
        """max |a - b| over max |b|, per tensor: the largest over the tensors, with its name"""
        worst = (0.0, '')
        for k in b:
            if b[k].numel():
                e = float((a[k] - b[k]).abs().max()) / max(float(b[k].abs().max()), 1e-30)
                worst = max(worst, (e, k))
        return worst

    out = {'backend': dist.get_backend(), 'world_size': dist.get_world_size(), 'forms': {k: v[0] for k, v in forms.items()}, 'against': {}}
    for a, b in (('ii', 'i'), ('ii', 'iii'), ('iv', 'iii')):
        (ra, ta, _), (rb, tb, _) = forms[a], forms[b]
        e, worst = rel_err(ta, tb)
        out['against'][f'{a}_vs_{b}'] = {
            'loss_rel_err': max(abs(x - y) / abs(y) for x, y in zip(ra['loss'], rb['loss'])), 'tensor_rel_err': e, 'worst_tensor': worst,
            'same_voxels_touched': bool(torch.equal(ta['k0/exp_avg'] == 0, tb['k0/exp_avg'] == 0))}

    # ---- from ONE scatter image: image route + in-place step against sweep + sparse_grad_allreduce + dense masked step
    N.FORCE_COLLECTIVES, joint_train._SPARSE_IMAGE_EXCHANGE = True, True
    G.release_grid_sample_workspace()
    m, n2, tr = forms['ii'][2]
    k0, route, opt = m.k0, m.k0.grad_route, tr.optimizer
    group = next(g for g in opt.param_groups if any(p is k0.grid for p in g['params']))
    hyper = (float(group['betas'][0]), float(group['betas'][1]), float(group['lr']), float(group['eps']))
    state = opt.state[k0.grid]

    def snapshot():
        k0.params_ready()
        torch.cuda.synchronize()
        return k0.grid.detach().clone(), state['exp_avg'].clone(), state['exp_avg_sq'].clone()

    def restore(snap, step):
        k0.params_ready()
        torch.cuda.synchronize()
        with torch.no_grad():
            k0.grid.copy_(snap[0]); state['exp_avg'].copy_(snap[1]); state['exp_avg_sq'].copy_(snap[2])
        state['step'] = step

    start, step0 = snapshot(), int(state['step'])
    route.arm('sparse')
    with torch.enable_grad():
        rr, rgb_sr, ls = tr.forward(*batch, global_step=9)
        opt.zero_grad(set_to_none=True)
        tr.optimizer_sr.zero_grad(set_to_none=True)
        ls['total'].backward()
    assert route.pending and k0.grid.grad is None
    img = G._GSB_WS[dev]
    torch.cuda.synchronize()
    sums = img.ws.clone()
    assert int(sums.count_nonzero()) > 0
    stats = route.exchange(None)
    assert stats is not None and stats['bytes_gathered'] > 0 and k0.grid.grad is None
    opt._sparse_step(k0.grid, k0, True, *hyper)
    route.abort()
    new = snapshot()
    zero_after = image_all_zero()
    restore(start, step0)
    img = G._scratch_image(dev, *k0.grid.shape[1:], route)
    img.ws.copy_(sums)
    img.holder, route.sums = route, True
    route.arm('sparse')
    route.sweep()
    assert k0.grid.grad is not None and not route.pending
    joint_train.sparse_grad_allreduce([k0.grid])
    state['step'] = step0 + 1
    masked_adam.masked_adam_upd(k0.grid, k0.grid.grad, state['exp_avg'], state['exp_avg_sq'], step0 + 1, *hyper)
    route.abort()
    old = snapshot()
    out['one_image'] = {'equal': [bool(torch.equal(a, b)) for a, b in zip(new, old)], 'changed': not torch.equal(new[0], start[0]), 'image_zero_after': zero_after,
                        'touched': stats['touched'][0]}

    # ---- from ONE dense gradient (the scratch image withheld from the backward): the exchange under the armed route against the one of (iii)
    restore(start, step0)
    k0.grid.grad = None
    G.GridGrad.backward = backward_without_image
    route.arm('sparse')
    with torch.enable_grad():
        rr, rgb_sr, ls = tr.forward(*batch, global_step=9)
        opt.zero_grad(set_to_none=True)
        tr.optimizer_sr.zero_grad(set_to_none=True)
        ls['total'].backward()
    G.GridGrad.backward = route_backward
    assert k0.grid.grad is not None and not route.pending
    dense = k0.grid.grad.clone()
    others = {id(p): p.grad.clone() for p in list(m.parameters()) + list(n2.parameters()) if p.grad is not None}
    ex = joint_train.exchange_gradients(m, n2, None)
    sent = int(ex['image_bytes_gathered'])
    still_dense = k0.grid.grad is not None
    state['step'] = step0 + 1
    masked_adam.masked_adam_upd(k0.grid, k0.grid.grad, state['exp_avg'], state['exp_avg_sq'], step0 + 1, *hyper)
    route.abort()
    new = snapshot()
    restore(start, step0)
    for p in list(m.parameters()) + list(n2.parameters()):
        if id(p) in others:
            p.grad = others[id(p)].clone()
    k0.grid.grad = dense.clone()
    joint_train._SPARSE_IMAGE_EXCHANGE = False                   # (not armed: the exchange of (iii))
    ex = joint_train.exchange_gradients(m, n2, None)
    assert ex['image_bytes_gathered'] == 0 and ex['bytes_gathered'] > 0
    state['step'] = step0 + 1
    masked_adam.masked_adam_upd(k0.grid, k0.grid.grad, state['exp_avg'], state['exp_avg_sq'], step0 + 1, *hyper)
    old = snapshot()
    out['one_dense_gradient'] = {'equal': [bool(torch.equal(a, b)) for a, b in zip(new, old)], 'changed': not torch.equal(new[0], start[0]),
                                 'message_bytes': sent, 'grad_dense': still_dense}
    joint_train._SPARSE_IMAGE_EXCHANGE = True
    N.FORCE_COLLECTIVES = False
    dist.barrier()
    dist.destroy_process_group()
    out['ok'] = True
    print('DP_SPARSE_ROUTE ' + json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
