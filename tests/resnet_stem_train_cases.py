"""
Shared by the stem training tests (tests/test_resnet_stem_train.py, tests/test_gpu_resnet_stem_train.py), the fixture
recipe (muzero-general_amd/tools/make_resnet_stem_train_golden.py) and the bench (tools/train_bench.py --family stem): the
case table of residual networks WITH a downsample stem ("resnet": DownSample, "CNN": DownsampleCNN), inputs and weights
rebuilt from seeds, the residual network with either stem restated in plain torch.nn under the reference's state_dict
keys, and the gates -- those of resnet_train_cases, bound to this module's tables.
"""
import collections
import functools
import hashlib
import json
import math
import os
import sys

import numpy
import torch

import resnet_train_cases as base
import trainer_loss_cases
from mzx import configs

LOGIT_GATE = base.LOGIT_GATE
LOSS_KEYS = base.LOSS_KEYS

# The smallest shapes at which each mechanism of the stems can still go wrong; the hidden board is ceil(H/16) x ceil(W/16).
CASES = [
    # C // 2 = 1 channel; boards 5x7 -> 3x4 -> 2x2 -> 1x1 -> 1x1: a pool window that is all padding but its centre, BatchNorm
    # over 2 values.  No dynamics: its gradients are exact zeros and its statistics keep their bits
    dict(name="sa_b2_k1", stem="resnet", B=2, steps=1, obs=(2, 5, 7), stacked=0, C=2, blocks=1, red=(2, 2, 2), rew=[4], val=[4],
         pol=[4], A=4, S=2, per=False, alpha=1.0, vlw=1.0, seed=41),
    # odd C (C // 2 = 2); odd and even boards alternate: 19 -> 10 -> 5 -> 3 -> 2 and 33 -> 17 -> 9 -> 5 -> 3; stride-2 right and
    # bottom edges; 510 stem positions: a ragged M tile and one weight-gradient chunk
    dict(name="sb_b3_k3", stem="resnet", B=3, steps=3, obs=(3, 19, 33), stacked=0, C=5, blocks=1, red=(2, 2, 2), rew=[4], val=[4],
         pol=[4], A=9, S=2, per=False, alpha=0.5, vlw=1.0, seed=42),
    # 5 input planes, a second ragged N tile (18 > 16), 800 stem positions: two weight-gradient chunks
    dict(name="sc_b5_k2_stacked", stem="resnet", B=5, steps=2, obs=(1, 16, 40), stacked=2, C=18, blocks=1, red=(2, 2, 2), rew=[4],
         val=[4], pol=[4], A=5, S=2, per=True, alpha=0.6, vlw=0.25, seed=43, sgd=dict(lr=0.05, momentum=0.9, weight_decay=1e-4)),
    # 4 x 4 stride-4 kernel, mid = 3 channels; boards 9x11 -> 4x5 -> 4x5 -> 1x2 -> adaptive 2x3 (out > in)
    dict(name="ca_b2_k2", stem="CNN", B=2, steps=2, obs=(2, 32, 40), stacked=0, C=4, blocks=1, red=(2, 2, 2), rew=[4], val=[4],
         pol=[4], A=6, S=2, per=False, alpha=0.5, vlw=1.0, seed=44),
    # 7 input planes, 6 x 6 stride-4 kernel, mid = 8; boards 12x14 -> 5x6 -> 5x6 -> 2x2 -> adaptive 3x4 (overlapping windows)
    dict(name="cb_b3_k3_stacked", stem="CNN", B=3, steps=3, obs=(3, 48, 56), stacked=1, C=9, blocks=1, red=(2, 2, 2), rew=[4],
         val=[4], pol=[4], A=7, S=2, per=True, alpha=0.5, vlw=0.25, seed=45),
]
BY_NAME = {c["name"]: c for c in CASES}

input_channels = base.input_channels
is_statistic = base.is_statistic
load = base.load


def config_of(case, **kw):
    kw.setdefault("train_downsample", True)
    return base.config_of(case, downsample=case["stem"], **kw)


def case_of_config(config, B, steps, seed=60, name=None):
    """A case (seeded weights and batch) for a shipped configuration with a stem, e.g. ``configs.breakout()``."""
    return dict(base.case_of_config(config, B, steps, seed, name), stem=config.downsample)


def hidden_board(case):
    return math.ceil(case["obs"][1] / 16), math.ceil(case["obs"][2] / 16)


def is_bypassed(key):
    """representation_network.module.conv / .bn: in the state_dict, never applied behind a stem."""
    return key.startswith(("representation_network.module.conv.", "representation_network.module.bn."))


# ---------------------------------------------------------------------------------------------------------------------
# The two stems and the representation network in plain torch.nn, under the reference's state_dict keys.

class _DownSample(torch.nn.Module):
    def __init__(self, cin, C):
        super().__init__()
        self.conv1 = torch.nn.Conv2d(cin, C // 2, kernel_size=3, stride=2, padding=1, bias=False)
        self.resblocks1 = torch.nn.ModuleList([base._Block(C // 2) for _ in range(2)])
        self.conv2 = torch.nn.Conv2d(C // 2, C, kernel_size=3, stride=2, padding=1, bias=False)
        self.resblocks2 = torch.nn.ModuleList([base._Block(C) for _ in range(3)])
        self.pooling1 = torch.nn.AvgPool2d(kernel_size=3, stride=2, padding=1)
        self.resblocks3 = torch.nn.ModuleList([base._Block(C) for _ in range(3)])
        self.pooling2 = torch.nn.AvgPool2d(kernel_size=3, stride=2, padding=1)

    def forward(self, x):
        x = self.conv1(x)
        for block in self.resblocks1:
            x = block(x)
        x = self.conv2(x)
        for block in self.resblocks2:
            x = block(x)
        x = self.pooling1(x)
        for block in self.resblocks3:
            x = block(x)
        return self.pooling2(x)


class _DownsampleCNN(torch.nn.Module):
    def __init__(self, cin, C, board):
        super().__init__()
        mid = (cin + C) // 2
        self.features = torch.nn.Sequential(
            torch.nn.Conv2d(cin, mid, kernel_size=board[0] * 2, stride=4, padding=2), torch.nn.ReLU(),
            torch.nn.MaxPool2d(kernel_size=3, stride=2),
            torch.nn.Conv2d(mid, C, kernel_size=5, padding=2), torch.nn.ReLU(),
            torch.nn.MaxPool2d(kernel_size=3, stride=2))
        self.avgpool = torch.nn.AdaptiveAvgPool2d(board)

    def forward(self, x):
        return self.avgpool(self.features(x))


class _StemTower(torch.nn.Module):
    def __init__(self, case):
        super().__init__()
        cin, C = input_channels(case), case["C"]
        self.downsample_net = _DownSample(cin, C) if case["stem"] == "resnet" else _DownsampleCNN(cin, C, hidden_board(case))
        self.conv, self.bn = base._conv3(cin, C), torch.nn.BatchNorm2d(C)       # bypassed, but in the state_dict
        self.resblocks = torch.nn.ModuleList([base._Block(C) for _ in range(case["blocks"])])

    def forward(self, x):
        x = self.downsample_net(x)
        for block in self.resblocks:
            x = block(x)
        return x


class StemNetwork(base.ResNetwork):
    def __init__(self, case):
        h, w = hidden_board(case)
        super().__init__(dict(case, obs=(case["obs"][0], h, w)))      # the dynamics and prediction networks on the hidden board
        self.representation_network = base._Replicated(_StemTower(case))


def tensor_shapes(case):
    return collections.OrderedDict((k, tuple(v.shape)) for k, v in StemNetwork(case).state_dict().items()
                                   if not k.endswith("num_batches_tracked"))


def split(case, joined):
    out, at = collections.OrderedDict(), 0
    for key, shape in tensor_shapes(case).items():
        n = int(numpy.prod(shape))
        out[key] = joined[at:at + n].reshape(shape)
        at += n
    assert at == joined.size
    return out


def weights(case):
    """The state_dict of the case (float32 numpy arrays), from its seed: the rule of resnet_train_cases.weights."""
    rs = numpy.random.RandomState(case["seed"] + 1000)
    out = collections.OrderedDict()
    for key, shape in tensor_shapes(case).items():
        draw = rs.uniform(-1, 1, size=shape).astype(numpy.float32)
        if len(shape) >= 2:
            out[key] = draw * numpy.float32(base.WEIGHT_SCALE / numpy.sqrt(numpy.prod(shape[1:])))
        elif key.endswith(".running_var"):
            out[key] = numpy.float32(1.0) + draw * numpy.float32(0.5)
        elif key.endswith(".running_mean"):
            out[key] = draw * numpy.float32(0.3)
        elif ".bn" in key and key.endswith(".weight"):
            out[key] = numpy.float32(1.0) + draw * numpy.float32(0.4)
        else:
            out[key] = draw * numpy.float32(0.3)
    return out


batch = base.batch      # (the observation keeps the case's full board)


def digest(case):
    h = hashlib.sha1()
    for a in list(weights(case).values()) + [x for x in batch(case) if x is not None]:
        h.update(numpy.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def torch_step(case, dtype, device="cpu"):
    """resnet_train_cases.torch_step on the network with its stem."""
    model = load(StemNetwork(case), weights(case)).to(dtype).to(device).train()
    config = config_of(case)
    observation, action, tv, tr, tp, weight, scale = batch(case)
    t = lambda a: torch.tensor(a).to(dtype).to(device)
    observation, tv, tr, tp, scale = t(observation), t(tv), t(tr), t(tp), t(scale)
    weight = t(weight) if case["per"] else None
    action = torch.tensor(action).long().to(device).unsqueeze(-1)
    value, reward, policy, hidden = model.initial_inference(observation)
    values, rewards, policies = [value], [reward], [policy]
    for i in range(1, action.shape[1]):
        value, reward, policy, hidden = model.recurrent_inference(hidden, action[:, i].to(dtype))
        hidden.register_hook(lambda grad: grad * 0.5)
        values.append(value), rewards.append(reward), policies.append(policy)
    loss, vl, rl, pl, priorities = trainer_loss_cases.torch_loss_head(values, rewards, policies, tv, tr, tp, weight, scale, config)
    loss.backward()
    out = dict(loss=loss.item(), value_loss=vl.mean().item(), reward_loss=rl.mean().item(), policy_loss=pl.mean().item(),
               value_logits=torch.stack(values).detach().cpu().numpy(), reward_logits=torch.stack(rewards).detach().cpu().numpy(),
               policy_logits=torch.stack(policies).detach().cpu().numpy(),
               pred=numpy.stack([trainer_loss_cases.torch_support_to_scalar(v.detach(), case["S"]).cpu().numpy().squeeze(-1)
                                 for v in values], 1))
    for key, p in model.named_parameters():
        out["grad/" + key] = numpy.zeros(tuple(p.shape)) if p.grad is None else p.grad.detach().cpu().numpy().copy()
    for key, b in model.named_buffers():
        if is_statistic(key):
            out["stat/" + key] = b.detach().cpu().numpy().copy()
    return out


# ---------------------------------------------------------------------------------------------------------------------
# Running a case through the native path (any backend).

def golden(golden_dir):
    return numpy.load(os.path.join(golden_dir, "resnet_stem_train.npz"))


def golden_keys(gold):
    return json.loads(str(gold["keys"]))


def network(be, case, **kw):
    from mzx import models
    net = models.MuZeroNetwork(config_of(case, **kw), _backend=be)
    net.set_weights({k: torch.from_numpy(v) for k, v in weights(case).items()})
    return net


# The floor of the per-tensor gate is resnet_train_cases.PARAM_GRAD_ERROR_FLOOR (1e-6).  MEASURED on the serial build
# (tests/test_resnet_stem_train.py prints, per case, the largest error on a tensor that needs the floor): the largest is
# 2.747e-7 (sc_b5_k2_stacked, representation_network.module.resblocks.0.bn2.weight).  Twice that, 5.5e-7, stays below 1e-6, so
# the parent's floor holds here unchanged.
PARAM_GRAD_ERROR_FLOOR = base.PARAM_GRAD_ERROR_FLOOR
tensor_gate = base.tensor_gate


def tracked_after(key, case, updates):
    """``num_batches_tracked`` of a BatchNorm after ``updates`` steps."""
    return 0 if is_bypassed(key) else base.tracked_after(key, case, updates)


# the groups of BatchNorms whose ``num_batches_tracked`` check_sgd has to meet
TRACKED = {"stem", "bypassed", "representation_network", "dynamics_network", "prediction_network"}

# The gates: resnet_train_cases' own, on this module's tables.  Beyond what they hold a plain network to, the tables make
# them assert exact-zero gradients and untouched statistic bits for the bypassed tensors, no counted application of the
# bypassed BatchNorm, and ``num_batches_tracked`` of the stem's BatchNorms (``tracked_after``, every group of ``TRACKED``).
THIS = sys.modules[__name__]
run_native = functools.partial(base.run_native, tables=THIS)
check_against = functools.partial(base.check_against, tables=THIS)
check_case = functools.partial(base.check_case, tables=THIS)
check_live = functools.partial(base.check_live, tables=THIS)
sgd_reference = functools.partial(base.sgd_reference, tables=THIS)
check_sgd = functools.partial(base.check_sgd, tables=THIS)
