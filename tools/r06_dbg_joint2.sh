O=gpurun_out/r06_dbg; mkdir -p $O
cat > /tmp/dbg2.py <<'PY'
import os, sys, json, torch
sys.path.insert(0, os.getcwd())
import bench
import nerf4k_amd
from nerf4k_amd import scene
from nerf4k_amd.lib import dvgo, sr_train
dev = torch.device('cuda', 0)
n_pre = int(os.environ.get('PRE_STREAMS', '0'))
pre = [torch.cuda.Stream() for _ in range(n_pre)]
for s in pre:
    with torch.cuda.stream(s):
        torch.zeros([1024], device=dev).add_(1)
torch.cuda.synchronize()
ck = scene.make_llff_checkpoint()
(H, W), K = scene.LLFF_HW, scene.LLFF_K
poses = scene.llff_spiral_poses()
with torch.no_grad():
    rays = [x.reshape(-1, 3).contiguous() for x in dvgo.get_rays_of_a_view(H, W, K, torch.from_numpy(poses[0]).to(dev), True, False, False, False)]
out = bench.joint_train_step(ck, rays, H, W, dev)
print(os.environ.get('PRE_STREAMS'), os.environ.get('SIDE_PRIO'), json.dumps({k: out[k] for k in ('ms_per_iteration', 'ms_per_iteration_per_block_graph')}))
PY
for v in "PRE_STREAMS=0 SIDE_PRIO=1" "PRE_STREAMS=6 SIDE_PRIO=1" "PRE_STREAMS=6 SIDE_PRIO=0" "PRE_STREAMS=12 SIDE_PRIO=1" "PRE_STREAMS=12 SIDE_PRIO=0"; do
  env $v python /tmp/dbg2.py 2>/dev/null | tail -1
done
