"""The perceptual / style terms, CPU side: the public interface of 4k-nerf_amd/lib/sr_loss.py (constructor, state_dict keys, weight loading, what raises),
the checker tests/vgg_oracle.py against independently written forms of the same formulas, and JointTrainer's handling of ``cri_perceptual``."""
import inspect

import pytest
import torch
import torch.nn as nn

import nerf4k_amd  # noqa: F401
from nerf4k_amd import _native as N, joint_train
from nerf4k_amd.lib import sr_loss
import vgg_oracle as VO

LW = {'conv1_2': 0, 'conv2_2': 0, 'conv3_4': 1, 'conv4_4': 1, 'conv5_4': 1}           # run_sr.py:671-677
WIDTHS = [64, 64, 'M', 128, 128, 'M', 256, 256, 256, 256, 'M', 512, 512, 512, 512, 'M', 512, 512, 512, 512, 'M']     # torchvision vgg19 ('E')


def test_constructor_defaults_and_layer_names():
    sig = inspect.signature(sr_loss.VGGFeatureExtractor.__init__)
    assert [(k, p.default) for k, p in list(sig.parameters.items())[2:]] == [
        ('vgg_type', 'vgg19'), ('use_input_norm', True), ('range_norm', False), ('requires_grad', False), ('remove_pooling', False), ('pooling_stride', 2)]
    sig = inspect.signature(sr_loss.PerceptualLoss.__init__)
    assert [(k, p.default) for k, p in list(sig.parameters.items())[2:]] == [
        ('vgg_type', 'vgg19'), ('use_input_norm', True), ('range_norm', False), ('perceptual_weight', 1.0), ('style_weight', 0.), ('criterion', 'l1')]
    names = sr_loss.vgg19_layer_names()
    assert len(names) == 37 and names[:5] == ['conv1_1', 'relu1_1', 'conv1_2', 'relu1_2', 'pool1'] and names[-3:] == ['conv5_4', 'relu5_4', 'pool5']
    # the i-th name is the i-th module of torchvision's vgg19().features
    kinds = []
    for w in WIDTHS:
        kinds += ['pool'] if w == 'M' else ['conv', 'relu']
    assert [n[:4] for n in names] == kinds and names == VO.NAMES
    cri = sr_loss.PerceptualLoss(LW, perceptual_weight=0.5, style_weight=0.2)
    assert cri.perceptual_weight == 0.5 and cri.style_weight == 0.2 and cri.layer_weights == LW
    assert cri.k4_taps() == [('conv3_4', 1.0), ('conv4_4', 1.0), ('conv5_4', 1.0)]        # w_k == 0 layers are not evaluated


def test_state_dict_keys():
    ext = sr_loss.VGGFeatureExtractor(['conv3_4'])
    convs = [n for n in VO.NAMES[:VO.NAMES.index('conv3_4') + 1] if n.startswith('conv')]
    assert len(convs) == 8
    want = {f'vgg_net.{n}.{p}' for n in convs for p in ('weight', 'bias')} | {'mean', 'std'}
    assert set(ext.state_dict()) == want
    assert ext.mean.shape == (1, 3, 1, 1) and ext.std.shape == (1, 3, 1, 1)
    assert torch.equal(ext.mean.flatten(), torch.tensor([0.485, 0.456, 0.406])) and torch.equal(ext.std.flatten(), torch.tensor([0.229, 0.224, 0.225]))
    assert all(not p.requires_grad for p in ext.parameters())
    assert ext.vgg_net.conv3_1.weight.shape == (256, 128, 3, 3) and ext.vgg_net.conv1_1.weight.shape == (64, 3, 3, 3)
    assert set(sr_loss.VGGFeatureExtractor(['relu1_1'], use_input_norm=False).state_dict()) == {'vgg_net.conv1_1.weight', 'vgg_net.conv1_1.bias'}
    cri = sr_loss.PerceptualLoss(LW)
    own = set(cri.state_dict())
    assert len(own) == 34 and own == {f'vgg.vgg_net.{n}.{p}' for n in VO.NAMES if n.startswith('conv') for p in ('weight', 'bias')} | {'vgg.mean', 'vgg.std'}


def test_loading_from_both_key_formats():
    sd = sr_loss.seeded_vgg19_state_dict(7)
    assert len(sd) == 32 and sd['features.0.weight'].shape == (64, 3, 3, 3) and sd['features.34.weight'].shape == (512, 512, 3, 3)
    assert all(torch.equal(a, b) for a, b in zip(sd.values(), sr_loss.seeded_vgg19_state_dict(7).values()))
    assert not torch.equal(sd['features.0.weight'], sr_loss.seeded_vgg19_state_dict(8)['features.0.weight'])
    w = sd['features.28.weight']
    assert abs(float(w.std()) - (2 / (9 * 512)) ** 0.5) < 0.02 * (2 / (9 * 512)) ** 0.5 and float(sd['features.28.bias'].abs().max()) <= 0.1
    a = sr_loss.PerceptualLoss(LW).load_vgg_state_dict(dict(sd, **{'classifier.0.weight': torch.zeros(3)}))
    b = sr_loss.PerceptualLoss(LW).load_vgg_state_dict(a.state_dict())             # the module's own keys
    c = sr_loss.PerceptualLoss(LW)
    c.load_state_dict(a.state_dict(), strict=True)                                  # ... and plain load_state_dict
    e = sr_loss.VGGFeatureExtractor(list(LW)).load_vgg_state_dict(a.vgg.state_dict())
    for i, n in enumerate(VO.NAMES):
        if n.startswith('conv'):
            for m in (a.vgg, b.vgg, c.vgg, e):
                assert torch.equal(getattr(m.vgg_net, n).weight, sd[f'features.{i}.weight']) and torch.equal(getattr(m.vgg_net, n).bias, sd[f'features.{i}.bias'])
    assert a.vgg._loaded and b.vgg._loaded and c.vgg._loaded and e._loaded
    with pytest.raises(KeyError):
        sr_loss.PerceptualLoss(LW).load_vgg_state_dict({k: v for k, v in sd.items() if k != 'features.30.bias'})


def test_what_raises():
    x = torch.rand(1, 3, 32, 32)
    cri = sr_loss.PerceptualLoss(LW, perceptual_weight=0.5, style_weight=0.2)
    with pytest.raises(N.K4Error):                               # CPU tensors: there is no tensor-library path
        cri(x, x)
    with pytest.raises(N.K4Error):
        sr_loss.VGGFeatureExtractor(['conv1_2'])(x)
    for kw in (dict(vgg_type='vgg16'), dict(range_norm=True), dict(requires_grad=True), dict(remove_pooling=True), dict(pooling_stride=1)):
        with pytest.raises(NotImplementedError, match=next(iter(kw))):
            sr_loss.VGGFeatureExtractor(['conv1_2'], **kw)
    for kw in (dict(vgg_type='vgg16'), dict(range_norm=True), dict(criterion='l2'), dict(criterion='fro')):
        with pytest.raises(NotImplementedError, match=next(iter(kw))):
            sr_loss.PerceptualLoss(LW, **kw)
    # never-loaded weights: K4Error naming the loader, from the operand builder every forward goes through (no GPU needed to see it)
    with pytest.raises(N.K4Error, match='load_vgg_state_dict'):
        cri.vgg.k4_operands(torch.device('cpu'), False)
    # no tensor-library evaluation inside the package's forward methods (tests/test_abi.py holds the static rule)
    src = inspect.getsource(sr_loss)
    assert 'torch.nn.functional' not in src and 'F.conv2d' not in src and 'max_pool2d(' not in src


def _sequential(sd, upto):
    """torchvision's vgg19().features written out (nn.Sequential of Conv2d / ReLU / MaxPool2d), fp64, with the seeded weights."""
    layers, cin = [], 3
    for w in WIDTHS:
        if w == 'M':
            layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
        else:
            layers += [nn.Conv2d(cin, w, kernel_size=3, padding=1), nn.ReLU(inplace=False)]
            cin = w
    net = nn.Sequential(*layers[:upto + 1]).double()
    net.load_state_dict({k[len('features.'):]: v.double() for k, v in sd.items() if int(k.split('.')[1]) <= upto})
    return net


def _case(seed, H, W):
    g = torch.Generator().manual_seed(seed)
    gt = torch.rand([1, 3, H, W], generator=g, dtype=torch.float64)
    return gt + 0.1 * torch.randn([1, 3, H, W], generator=g, dtype=torch.float64), gt


def test_checker_against_a_sequential_stack_and_the_gram_formula():
    sd = sr_loss.seeded_vgg19_state_dict(7)
    params = VO.params_from_torchvision(sd)
    x, gt = _case(3, 32, 48)
    net = _sequential(sd, 34)
    mean, std = torch.tensor(VO.MEAN).double().view(1, 3, 1, 1), torch.tensor(VO.STD).double().view(1, 3, 1, 1)
    feats = {}
    with torch.no_grad():
        for img, t in (('x', x), ('gt', gt)):
            h = (t - mean) / std
            for i, m in enumerate(net):
                h = m(h)
                feats[img, VO.NAMES[i]] = h
    tr = VO.run_stack(x, params, 'conv5_4')
    for n in VO.NAMES[:35]:
        a, b = tr['out'][n], feats['x', n]
        assert a.shape == b.shape and float((a - b).abs().max()) <= 1e-12 * float(b.abs().max()), n
    # the two terms, restated: lib/sr_loss.py:134-161 and the Gram matrix of :175-188
    def gram_restated(t):
        n, c, h, w = t.size()
        f = t.view(n, c, w * h)
        return f.bmm(f.transpose(1, 2)) / (c * h * w)
    pcp = sum(torch.nn.L1Loss()(feats['x', k], feats['gt', k]) * w for k, w in LW.items()) * 0.5
    sty = sum(torch.nn.L1Loss()(gram_restated(feats['x', k]), gram_restated(feats['gt', k])) * w for k, w in LW.items()) * 0.2
    p, s = VO.losses(x, gt, params, LW, 0.5, 0.2)
    assert abs(float(p - pcp)) <= 1e-12 * float(pcp) and abs(float(s - sty)) <= 1e-12 * float(sty)
    assert 0.3 < float(p) < 1.0 and 1e-4 < float(s) < 1e-2                            # neither term is degenerate on seeded weights
    assert VO.losses(x, gt, params, LW, 0.5, 0.0)[1] is None and VO.losses(x, gt, params, LW, 0.0, 0.2)[0] is None
    # first_max: ties keep the first candidate in (dy, dx) order
    c = torch.tensor([[1., 1., 0., 1.], [0., 2., 2., 1.], [0., 0., 0., 0.], [1., 2., 3., 3.]])
    assert VO.first_max(c).tolist() == [0, 1, 0, 2]


def test_grad_with_record_fed_the_checkers_own_decisions_is_autograd():
    sd = sr_loss.seeded_vgg19_state_dict(7)
    params = VO.params_from_torchvision(sd)
    x, gt = _case(4, 32, 32)
    want = VO.grad_autograd(x, gt, params, LW, 0.5, 0.2)
    rec, mar = VO.decisions(x, gt, params, LW)
    assert set(rec) == {'relu_mask', 'pool_choice', 'feat_sign', 'gram_sign'}
    assert set(rec['pool_choice']) == {'pool1', 'pool2', 'pool3', 'pool4'} and len(rec['relu_mask']) == 15 and set(rec['gram_sign']) == {'conv3_4', 'conv4_4', 'conv5_4'}
    assert rec['relu_mask']['conv1_1'].dtype == torch.bool and rec['pool_choice']['pool1'].dtype == torch.uint8 and rec['gram_sign']['conv3_4'].shape == (256, 256)
    got = VO.grad_with_record(x, gt, params, rec, LW, 0.5, 0.2)
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert float(want.abs().max()) > 0
    # ... and a changed decision changes it: the record is used
    rec2 = {k: dict(v) for k, v in rec.items()}
    rec2['relu_mask']['conv5_3'] = ~rec['relu_mask']['conv5_3']
    other = VO.grad_with_record(x, gt, params, rec2, LW, 0.5, 0.2)
    assert float((other - want).abs().max()) > 1e-3 * float(want.abs().max())
    # each term alone
    for pw, sw in ((0.5, 0.0), (0.0, 0.2)):
        a, b = VO.grad_autograd(x, gt, params, LW, pw, sw), VO.grad_with_record(x, gt, params, rec, LW, pw, sw)
        assert float((a - b).abs().max()) <= 1e-12 * float(a.abs().max())


def _small_pair():
    from nerf4k_amd import scene
    from nerf4k_amd.lib import sr_esrnet, utils
    ck = scene.make_llff_checkpoint(seed=5, num_voxels=24 * 24 * 16, mpi_depth=16)
    model = utils.model_from_checkpoint_dict(ck)
    torch.manual_seed(1)
    return model, sr_esrnet.SFTNet(3, scale=4, num_feat=64, num_block=1, num_grow_ch=32, num_cond=1)


def test_joint_trainer_and_the_perceptual_module():
    from nerf4k_amd.lib import sr_unetdisc
    cfg = joint_train.JointCfg.fern_lg_joint_l1_gan()
    net_d = sr_unetdisc.UNetDiscriminatorSN(3, num_feat=8)
    cri = sr_loss.PerceptualLoss(LW, perceptual_weight=0.5, style_weight=0.2)
    with pytest.raises(NotImplementedError, match='cri_perceptual.*load'):          # names the argument and says who loads the weights
        joint_train.JointTrainer(None, None, cfg, {}, 1, net_d=net_d)
    with pytest.raises(NotImplementedError, match='cri_perceptual'):
        joint_train.JointTrainer(None, None, joint_train.JointCfg.fern_lg_joint_l1(weight_style=0.2), {}, 1)
    with pytest.raises(NotImplementedError, match='weight_style'):                  # the reference would drop the style term silently
        joint_train.JointTrainer(None, None, joint_train.JointCfg.fern_lg_joint_l1(weight_style=0.2), {}, 1, cri_perceptual=cri)
    for bad in (sr_loss.PerceptualLoss(LW, perceptual_weight=1.0, style_weight=0.2), sr_loss.PerceptualLoss(LW, perceptual_weight=0.5, style_weight=0.0)):
        with pytest.raises(ValueError, match='weight'):
            joint_train.JointTrainer(None, None, cfg, {}, 1, net_d=net_d, cri_perceptual=bad)
    model, net_sr = _small_pair()
    tr = joint_train.JointTrainer(model, net_sr, cfg, {}, 1, net_d=net_d, cri_perceptual=cri)
    assert tr.cri_perceptual is cri and tr.net_d is net_d
    assert all(not any(p is q for q in cri.parameters()) for opt in (tr.optimizer, tr.optimizer_sr, tr.optimizer_d) for pg in opt.param_groups for p in pg['params'])
    tr = joint_train.JointTrainer(model, net_sr, joint_train.JointCfg.fern_lg_joint_l1(weight_pcp=0.5), {}, 1,
                                  cri_perceptual=sr_loss.PerceptualLoss(LW, perceptual_weight=0.5))
    assert tr.cri_perceptual is not None and tr.net_d is None
    # with weight_pcp == 0 a module handed in is ignored, whatever its weights
    tr0 = joint_train.JointTrainer(model, net_sr, joint_train.JointCfg.fern_lg_joint_l1(), {}, 1, cri_perceptual=cri)
    assert tr0.cri_perceptual is None
