"""The data-parallel joint iteration (BASELINE configs[4], N > 1) on ONE GPU: `python tools/joint_dp_smoke.py` starts two ranks on cuda:0 over gloo (a process
group with a timeout; every rank a fresh process under a time limit) and times the iterations WITHOUT total variation (global_step >= tv_before: 290,000 of
fern_lg_joint_l1's 300,000) at the configuration's full sizes, with k0's gradient exchanged from the scatter's scratch image (joint_train._SPARSE_IMAGE_EXCHANGE,
'on') and from a dense tensor ('off'), in alternating blocks, 200 iterations each.  With the route on k0 never has a dense `.grad`; at the end the replicas'
k0, exp_avg and exp_avg_sq are equal (one gathered checksum).  Every rank prints one JSON line `JOINT_DP {...}`.  A measurement tool, not a test; what a 1-GPU box
can say about the N > 1 leg, which it cannot run over RCCL.

    python tools/joint_dp_smoke.py                    two ranks, route on / off alternated
    python tools/joint_dp_smoke.py --route off        the dense exchange alone (also what a tree without the image route can run)
    python tools/joint_dp_smoke.py --world 1          the one-rank iteration of the same box: the yardstick from below
"""
import argparse, datetime, json, os, socket, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCK = 20                     # iterations per timed block; the modes alternate block by block


def launch(args):
    s = socket.socket(); s.bind(('127.0.0.1', 0)); port = s.getsockname()[1]; s.close()
    procs = []
    for r in range(args.world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(args.world), MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__), '--route', args.route, '--iters', str(args.iters), '--world', str(args.world), '--phases', str(args.phases)],
                                      env=env))
    deadline = time.time() + args.limit
    rc = 0
    for p in procs:
        try:
            rc |= p.wait(timeout=max(1.0, deadline - time.time()))
        except subprocess.TimeoutExpired:
            rc = 124
            break
    for p in procs:                                          # a rank that outlived the limit (or its peer's failure) does not stay behind
        if p.poll() is None:
            p.kill()
            p.wait()
    return rc


def worker(args):
    import numpy as np, torch, torch.distributed as dist
    sys.path.insert(0, ROOT)
    rank, world = int(os.environ['RANK']), int(os.environ['WORLD_SIZE'])
    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    if world > 1:
        dist.init_process_group('gloo', timeout=datetime.timedelta(seconds=120))
    import nerf4k_amd  # noqa: F401
    from nerf4k_amd import scene, joint_train
    from nerf4k_amd.lib import dvgo, sr_esrnet, utils
    import contextlib
    ck = scene.make_llff_checkpoint()
    (H, W), K = scene.LLFF_HW, scene.LLFF_K
    with torch.no_grad():
        ro, rd, vd = (x.reshape(H, W, 3) for x in dvgo.get_rays_of_a_view(H, W, K, torch.from_numpy(scene.llff_spiral_poses()[0]).to(dev), True, False, False, False))
    model = utils.model_from_checkpoint_dict(ck).to(dev).train()
    torch.manual_seed(778)
    net = sr_esrnet.SFTNet(3, scale=4, num_feat=64, num_block=5, num_grow_ch=32, num_cond=1).to(dev).train()
    cfg = joint_train.JointCfg.fern_lg_joint_l1()
    with contextlib.redirect_stdout(sys.stderr):
        tr = joint_train.JointTrainer(model, net, cfg, dict(ck['render_kwargs'], render_depth=True, rand_bkgd=True), n_train_images=17)
    pr = pc = cfg.N_rand // cfg.N_patch
    gen = torch.Generator(device=dev).manual_seed(5)

    def batch(i):
        i = i * world + rank                                 # every rank its own patch
        r0, c0 = (37 * i) % (H - pr), (101 * i) % (W - pc)
        rays = [x[r0:r0 + pr, c0:c0 + pc].reshape(-1, 3).contiguous() for x in (ro, rd, vd)]
        return rays + [torch.rand([pr * pc, 3], device=dev, generator=gen), torch.rand([16 * pr * pc, 3], device=dev, generator=gen), pr, pc]

    def set_route(on):
        if args.route != 'off':                              # ('off' never touches the switch)
            joint_train._SPARSE_IMAGE_EXCHANGE = on
    modes = ['off'] if args.route == 'off' or world == 1 else ['on', 'off']
    it, late0 = 0, int(cfg.tv_before) + 10
    for i in range(3):                                       # warm-up with dense total variation: packing, optimizer state, allocator
        tr.step(*batch(it), global_step=1 + it)
        it += 1
    for mode in modes:                                       # ... and of both forms of the late iteration
        set_route(mode == 'on')
        for i in range(3):
            tr.step(*batch(it), global_step=late0 + it)
            it += 1
    torch.cuda.synchronize()
    blocks, dense_grad_seen = {m: [] for m in modes}, {m: 0 for m in modes}
    last = {}
    for b in range(max(1, args.iters // BLOCK)):
        for mode in modes:
            set_route(mode == 'on')
            if world > 1:
                dist.barrier()
            torch.cuda.synchronize()
            t = time.perf_counter()
            for i in range(BLOCK):
                tr.step(*batch(it), global_step=late0 + it)
                dense_grad_seen[mode] += model.k0.grid.grad is not None
                it += 1
            torch.cuda.synchronize()
            blocks[mode].append((time.perf_counter() - t) / BLOCK * 1e3)
            last[mode] = tr.last_exchange or {}
    n_iter = {m: len(v) * BLOCK for m, v in blocks.items()}
    if world > 1:
        if 'on' in modes:
            assert dense_grad_seen['on'] == 0, 'k0 had a dense .grad in an iteration of the image route'
        assert dense_grad_seen['off'] == n_iter['off'], 'the dense exchange leaves k0 a dense .grad in every iteration'
    # what the iteration consists of, per mode: a few more iterations with the exchange and its parts bracketed by device synchronisations (which removes the
    # overlap between streams and ranks the timed blocks have: a decomposition of the SYNCHRONISED iteration, reported beside its total)
    phases = {}
    if args.phases > 0:
        from nerf4k_amd.lib import grid as G, sr_train
        spent = {}

        def timed(name, fn):
            def call(*a, **k):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                try:
                    return fn(*a, **k)
                finally:
                    torch.cuda.synchronize()
                    spent[name] = spent.get(name, 0.0) + (time.perf_counter() - t0) * 1e3
            return call
        keep = [(joint_train, 'exchange_gradients'), (joint_train, 'sparse_grad_allreduce'), (sr_train, 'allreduce_gradients')]
        keep += [(G.GridGrad, 'exchange')] if hasattr(G.GridGrad, 'exchange') else []
        saved = [(o, n, getattr(o, n)) for o, n in keep]
        names = {'exchange_gradients': 'exchange_total', 'sparse_grad_allreduce': 'lists_of_dense_gradients', 'allreduce_gradients': 'dense_bucket_allreduce',
                 'exchange': 'k0_lists_from_the_image'}
        try:
            for o, n, fn in saved:
                setattr(o, n, timed(names[n], fn))
            for mode in modes:
                set_route(mode == 'on')
                spent.clear()
                for i in range(args.phases):
                    if world > 1:
                        dist.barrier()
                    step = timed('iteration_synchronised', tr.step)
                    step(*batch(it), global_step=late0 + it)
                    it += 1
                phases[mode] = {k: round(v / args.phases, 3) for k, v in sorted(spent.items())}
        finally:
            for o, n, fn in saved:
                setattr(o, n, fn)
    # the replicas after all of it: ONE gathered checksum over k0 and its moments (the bits, summed as integers: exact, order-free)
    model.k0.params_ready()
    torch.cuda.synchronize()
    st = tr.optimizer.state[model.k0.grid]
    check = torch.stack([t.detach().contiguous().view(torch.int32).sum(dtype=torch.int64) for t in (model.k0.grid, st['exp_avg'], st['exp_avg_sq'])]).cpu()
    sums = [check]
    if world > 1:
        sums = [torch.zeros_like(check) for _ in range(world)]
        dist.all_gather(sums, check)
        assert all(torch.equal(s, sums[0]) for s in sums), f'the replicas differ: {[s.tolist() for s in sums]}'

    def stats(ex):
        return {'image_bytes_gathered': int(ex.get('image_bytes_gathered', 0)), 'image_touched': [list(c) for c, _ in ex.get('image_touched', [])],
                'list_bytes_gathered': int(ex.get('bytes_gathered', 0)), 'list_touched': [list(c) for c, _ in ex.get('touched', [])],
                'dense_bucket_bytes': int(ex.get('bytes_dense', 0))}
    out = {'rank': rank, 'world': world, 'device': torch.cuda.get_device_name(0), 'image_route_available': hasattr(joint_train, '_SPARSE_IMAGE_EXCHANGE'),
           'iterations': n_iter, 'block': BLOCK,
           'ms_per_iteration': {m: round(float(np.median(v)), 3) for m, v in blocks.items()},
           'ms_blocks': {m: [round(x, 3) for x in v] for m, v in blocks.items()},
           'synchronised_ms': phases, 'k0_dense_grad_iterations': dense_grad_seen, 'exchange': {m: stats(ex) for m, ex in last.items()},
           'replica_checksums_equal': True, 'checksum': check.tolist(), 'k0_step': int(st['step'])}
    print('JOINT_DP ' + json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == '__main__':
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--world', type=int, default=2)
    ap.add_argument('--route', choices=['both', 'off'], default='both')
    ap.add_argument('--iters', type=int, default=200, help='timed iterations per mode')
    ap.add_argument('--phases', type=int, default=20, help='further iterations per mode with the exchange and its parts bracketed by synchronisations (0: none)')
    ap.add_argument('--limit', type=float, default=420.0, help='seconds after which the ranks are ended')
    a = ap.parse_args()
    if 'RANK' in os.environ:
        worker(a)
    else:
        sys.exit(launch(a))
