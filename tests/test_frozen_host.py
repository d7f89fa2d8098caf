"""CPU: the bookkeeping of grounding_model.freeze_batchnorm (module state, requires_grad, state_dict) and the driver's --freeze-bn flags.
What the frozen layers compute is tests/test_frozen_gpu.py."""
import pytest
import torch

from util import new_product, ref_shapes

_BN = torch.nn.modules.batchnorm._BatchNorm


def _bns(m):
    inside = {id(x) for x in m.visumodel.modules() if isinstance(x, _BN)}
    every = [x for x in m.modules() if isinstance(x, _BN)]
    return [x for x in every if id(x) in inside], [x for x in every if id(x) not in inside]


def test_freeze_batchnorm_bookkeeping():
    m = new_product(256)
    keys = list(m.state_dict().keys())
    assert len(keys) == 597 and set(keys) == set(ref_shapes(256))
    backbone, head = _bns(m)
    assert len(backbone) > 70 and len(head) == 22            # 3 + 3 + 9 + 3 ConvBatchNormReLU blocks, mapping_lang's two, the two location ones
    drop = [x for x in m.modules() if isinstance(x, torch.nn.Dropout)]
    assert m.freeze_batchnorm("backbone") is m
    for step in (m.train, m.eval, m.train):
        step()
        assert not any(x.training for x in backbone)
        assert all(x.training == m.training for x in head) and all(x.training == m.training for x in drop)
    assert m.visumodel.training and m.training               # train mode stays train mode: only the BatchNorm flags differ
    m.visumodel.train()                                      # ... also when the backbone is switched on its own
    assert not any(x.training for x in backbone)
    m.freeze_batchnorm("all")
    m.eval(); m.train()
    assert not any(x.training for x in backbone + head) and all(x.training for x in drop)
    assert all(p.requires_grad for x in backbone + head for p in (x.weight, x.bias))
    # train_affine=False: the in-scope gamma / beta stop training; what the caller had switched off himself stays off afterwards
    head[0].bias.requires_grad_(False)
    m.freeze_batchnorm("backbone", train_affine=False)
    assert not any(p.requires_grad for x in backbone for p in (x.weight, x.bias))
    assert all(p.requires_grad for x in head for p in (x.weight, x.bias) if p is not head[0].bias)
    assert all(x.training for x in head) and not any(x.training for x in backbone)
    m.freeze_batchnorm("all", train_affine=False)
    assert not any(p.requires_grad for x in backbone + head for p in (x.weight, x.bias))
    m.freeze_batchnorm(None)
    assert all(p.requires_grad for x in backbone + head for p in (x.weight, x.bias) if p is not head[0].bias)
    assert not head[0].bias.requires_grad
    assert all(x.training for x in backbone + head)
    m.eval()
    assert not any(x.training for x in backbone + head)
    m.train()
    assert all(x.training for x in backbone + head)
    assert list(m.state_dict().keys()) == keys                # nobody's state_dict was touched
    with pytest.raises(ValueError):
        m.freeze_batchnorm("head")
    with pytest.raises(ValueError):
        m.freeze_batchnorm(True)


def test_freeze_bn_arguments_parse():
    from dcnet_amd.train import arg_parser, freeze_bn_args
    ap = arg_parser()
    assert freeze_bn_args(ap.parse_args([])) is None
    assert freeze_bn_args(ap.parse_args(["--freeze-bn", "none", "--freeze-bn-stats-only"])) is None
    assert freeze_bn_args(ap.parse_args(["--freeze-bn", "backbone"])) == dict(scope="backbone", train_affine=False)
    assert freeze_bn_args(ap.parse_args(["--freeze-bn", "all", "--freeze-bn-stats-only"])) == dict(scope="all", train_affine=True)
    with pytest.raises(SystemExit):
        ap.parse_args(["--freeze-bn", "head"])
