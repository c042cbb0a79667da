"""
Shared by the stem training tests (tests/test_resnet_stem_train.py, tests/test_gpu_resnet_stem_train.py), the fixture
recipe (muzero-general_amd/tools/make_resnet_stem_train_golden.py) and the bench (tools/resnet_stem_train_bench.py): the
case table of residual networks WITH a downsample stem ("resnet": DownSample, "CNN": DownsampleCNN), inputs and weights
rebuilt from seeds, the residual network with either stem restated in plain torch.nn under the reference's state_dict
keys, and the gates -- the rules of resnet_train_cases, whose helpers run here on this module's tables.
"""
import collections
import hashlib
import json
import math
import os

import numpy
import torch

import fc_train_cases
import resnet_train_cases as base
import trainer_loss_cases
from mzx import configs

LOGIT_GATE = fc_train_cases.LOGIT_GATE
LOSS_KEYS = fc_train_cases.LOSS_KEYS
LOSS_ERROR_FLOOR = trainer_loss_cases.LOSS_ERROR_FLOOR
DECODED_SCALAR_GATE = trainer_loss_cases.DECODED_SCALAR_GATE

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
# Running a case through the native path (any backend) and the gates.

def golden(golden_dir):
    return numpy.load(os.path.join(golden_dir, "resnet_stem_train.npz"))


def golden_keys(gold):
    return json.loads(str(gold["keys"]))


def network(be, case, **kw):
    from mzx import models
    net = models.MuZeroNetwork(config_of(case, **kw), _backend=be)
    net.set_weights({k: torch.from_numpy(v) for k, v in weights(case).items()})
    return net


def run_native(be, case, net=None):
    """resnet_train_cases.run_native on this module's tables: ``grad_flat`` pre-filled with NaN."""
    from mzx import trainer
    net = net if net is not None else network(be, case)
    param = next(net.parameters())
    param.grad = torch.full_like(net.flat_weights(), float("nan"))
    logits, stats = {}, {}
    packed = trainer.train_resnet_gradients(net, batch(case), config_of(case), logits=logits, stats=stats)
    host = packed.cpu().numpy()
    out = dict(loss=host[0], value_loss=host[1], reward_loss=host[2], policy_loss=host[3],
               priorities=host[4:].reshape(case["B"], case["steps"]).copy(),
               value_logits=logits["value"].cpu().numpy(), reward_logits=logits["reward"].cpu().numpy(),
               policy_logits=logits["policy"].cpu().numpy(), grad_flat=param.grad.cpu().numpy().copy(),
               running=stats["running"].cpu().numpy().copy())
    at = 0
    for key, off, numel, shape in net._tensors:
        out["grad/" + key] = out["grad_flat"][off:off + numel].reshape(shape)
        if is_statistic(key):
            out["stat/" + key] = out["running"][at:at + numel]
            at += numel
    assert at == out["running"].size
    assert stats["applications"]["representation_network.module.bn."] == 0
    return out


# The floor of the per-tensor gate is resnet_train_cases.PARAM_GRAD_ERROR_FLOOR (1e-6).  MEASURED on the serial build
# (tests/test_resnet_stem_train.py prints, per case, the largest error on a tensor that needs the floor): the largest is
# 2.747e-7 (sc_b5_k2_stacked, representation_network.module.resblocks.0.bn2.weight).  Twice that, 5.5e-7, stays below 1e-6, so
# the parent's floor holds here unchanged.
PARAM_GRAD_ERROR_FLOOR = base.PARAM_GRAD_ERROR_FLOOR


def tensor_gate(ref_error):
    return max(4 * ref_error, PARAM_GRAD_ERROR_FLOOR)


def check_against(case, got, want32_logits, ref64, ref_errors, f32_losses, f32_pred, be, report=print):
    """The gates of resnet_train_cases.check_against over this module's tensors."""
    name = case["name"]
    failures = []
    for head in ("value", "reward", "policy"):
        ours, ref = got[f"{head}_logits"], want32_logits[head]
        assert ours.shape == ref.shape, (head, ours.shape, ref.shape)
        finite = numpy.isfinite(ref)
        assert numpy.array_equal(ours[~finite], ref[~finite]), head
        err = float(numpy.max(numpy.abs(ours[finite].astype(numpy.float64) - ref[finite]))) if finite.any() else 0.0
        report(f"{name} {head} logits: error {err:.3e} against the reference float32, gate {LOGIT_GATE:.1e}")
        if not err <= LOGIT_GATE:
            failures.append(head)
    for key in LOSS_KEYS:
        mine, ref = abs(float(got[key]) - float(ref64[key])), abs(float(f32_losses[key]) - float(ref64[key]))
        gate = max(4 * ref, LOSS_ERROR_FLOOR)
        report(f"{name} {key}: error {mine:.3e}, reference float32 error {ref:.3e}, gate {gate:.3e}")
        if not mine <= gate:
            failures.append(key)
    logits = torch.from_numpy(got["value_logits"]).to(be.device).reshape(-1, 2 * case["S"] + 1)
    pred = be.empty((logits.shape[0],), torch.float32)
    be.lib.check(be.lib.mzx_support_to_scalar(be.ptr(logits), logits.shape[0], case["S"], be.ptr(pred), be.stream()))
    pred = pred.cpu().numpy().reshape(case["steps"], case["B"]).T.copy()
    want = numpy.abs(pred - batch(case)[2]) ** case["alpha"]
    assert want.dtype == numpy.float32
    ulps = trainer_loss_cases.ulp_distance(want, got["priorities"])
    report(f"{name} priorities: max ulp distance {ulps.max()} (alpha {case['alpha']})")
    assert ulps.max() <= (0 if case["alpha"] == 1.0 else 1)
    gap = numpy.abs(pred.astype(numpy.float64) - f32_pred)
    report(f"{name} decoded value against the reference: {gap.max():.3e} (values up to {numpy.abs(pred).max():.2f})")
    assert gap.max() <= DECODED_SCALAR_GATE
    assert not numpy.isnan(got["grad_flat"]).any(), "d_grad_flat was not fully overwritten"
    state = weights(case)
    worst = (0.0, None)
    for key in tensor_shapes(case):
        if is_statistic(key):
            assert numpy.array_equal(got["grad/" + key], numpy.zeros_like(got["grad/" + key])), key      # exact zeros
            kind, mine64 = "stat", got["stat/" + key]
        else:
            kind, mine64 = "grad", got["grad/" + key]
        if is_bypassed(key):        # never applied: exact-zero gradients, the statistics keep their bits
            assert numpy.array_equal(got["grad/" + key], numpy.zeros_like(got["grad/" + key])), key
            if is_statistic(key):
                assert numpy.array_equal(got["stat/" + key].view(numpy.int32), state[key].reshape(-1).view(numpy.int32)), key
        ref = float(ref_errors[f"{kind}/{key}"])
        gate = tensor_gate(ref)
        mine = float(numpy.max(numpy.abs(mine64.astype(numpy.float64).reshape(-1) - numpy.asarray(ref64[f"{kind}/{key}"]).reshape(-1))))
        report(f"{name} {kind} {key}: error {mine:.3e}, reference float32 error {ref:.3e}, gate {gate:.3e}")
        if 4 * ref < PARAM_GRAD_ERROR_FLOOR and mine > worst[0]:
            worst = (mine, key)
        if not mine <= gate:
            failures.append(key)
    report(f"{name} largest error on a tensor that needs the floor: {worst[0]:.3e} ({worst[1]})")
    assert not failures, failures


def check_case(be, case, gold, report=print):
    """Every gate of one fixture case; returns (network, outputs).  Figures are printed before they are asserted."""
    name = case["name"]
    assert digest(case) == str(gold[f"{name}/digest"]), "this machine rebuilt other input bits than the fixture's"
    net = network(be, case)
    got = run_native(be, case, net)
    keys = list(tensor_shapes(case))
    ref64 = {k: gold[f"{name}/f64_{k}"] for k in LOSS_KEYS}
    ref_errors = {}
    tensors = split(case, gold[f"{name}/f64_tensors"])
    for key, error in zip(keys, gold[f"{name}/f32_errors"]):
        kind = "stat" if is_statistic(key) else "grad"
        ref64[f"{kind}/{key}"] = tensors[key]
        ref_errors[f"{kind}/{key}"] = error
    check_against(case, got, {h: gold[f"{name}/f32_{h}_logits"] for h in ("value", "reward", "policy")}, ref64, ref_errors,
                  {k: gold[f"{name}/f32_{k}"] for k in LOSS_KEYS}, gold[f"{name}/f32_pred"], be, report)
    if case["steps"] == 1:      # no dynamics: exact zeros, statistics unchanged bit for bit
        state = weights(case)
        for key in keys:
            if key.startswith("dynamics_"):
                assert numpy.array_equal(got["grad/" + key], numpy.zeros_like(got["grad/" + key])), key
                if is_statistic(key):
                    assert numpy.array_equal(got["stat/" + key].view(numpy.int32), state[key].view(numpy.int32)), key
    again = run_native(be, case, net)
    for key, value in got.items():
        a, b = numpy.ascontiguousarray(value, numpy.float32), numpy.ascontiguousarray(again[key], numpy.float32)
        assert numpy.array_equal(a.view(numpy.int32), b.view(numpy.int32)), key
    return net, got


def check_live(be, case, report=print):
    """The gates of ``check_case`` against the torch restatement run here in binary64 and float32 (shapes the fixture does
    not carry)."""
    ref64, ref32 = torch_step(case, torch.float64), torch_step(case, torch.float32)
    errors = {k: float(numpy.max(numpy.abs(ref32[k].astype(numpy.float64) - ref64[k]))) for k in ref64 if k[:5] in ("grad/", "stat/")}
    net = network(be, case)
    got = run_native(be, case, net)
    check_against(case, got, {h: ref32[f"{h}_logits"] for h in ("value", "reward", "policy")}, ref64, errors,
                  {k: ref32[k] for k in LOSS_KEYS}, ref32["pred"], be, report)
    return net, got


def sgd_reference(gold, case):
    delta, initial = split(case, gold[f"{case['name']}/f64_sgd_delta"]), weights(case)
    return {key: initial[key].astype(numpy.float64) + delta[key].astype(numpy.float64) for key in initial}


def tracked_after(key, case, updates):
    """``num_batches_tracked`` of a BatchNorm after ``updates`` steps."""
    if is_bypassed(key):
        return 0
    per_step = 1 if key.startswith("representation") else case["steps"] - 1 if key.startswith("dynamics") else case["steps"]
    return updates * per_step


def check_sgd(be, case, gold, report=print):
    """resnet_train_cases.check_sgd: two ``update_weights`` steps with SGD-momentum and weight decay against the reference's
    weights AND buffers after two steps, the same gates; ``num_batches_tracked`` rises for the stem's BatchNorms and stays 0
    for the bypassed one."""
    from mzx import trainer
    name, hp = case["name"], case["sgd"]
    net = network(be, case)
    optimizer = torch.optim.SGD(net.parameters(), lr=hp["lr"], momentum=hp["momentum"], weight_decay=hp["weight_decay"])
    for _ in range(2):
        out = trainer.update_weights(net, optimizer, batch(case), config_of(case))
        assert isinstance(out[0], numpy.ndarray) and out[0].dtype == numpy.float32 and out[0].shape == (case["B"], case["steps"])
        assert all(type(v) is float for v in out[1:])
    failures = []
    state, want = net.get_weights(), sgd_reference(gold, case)
    for key, error in zip(tensor_shapes(case), gold[f"{name}/f32_errors"]):
        gate_of = tensor_gate(float(error))
        gate = 2 * gate_of if is_statistic(key) else 2 * hp["lr"] * (1 + hp["momentum"]) * gate_of
        err = float(numpy.max(numpy.abs(state[key].numpy().astype(numpy.float64) - want[key])))
        report(f"{name} after two SGD steps {key}: error {err:.3e}, gate {gate:.3e}")
        if not err <= gate:
            failures.append(key)
    seen = set()
    for key, value in state.items():
        if key.endswith("num_batches_tracked"):
            assert int(value) == tracked_after(key, case, 2), (key, int(value))
            seen.add("stem" if ".downsample_net." in key else "bypassed" if is_bypassed(key) else key.split(".")[0])
    assert seen == {"stem", "bypassed", "representation_network", "dynamics_network", "prediction_network"}, seen
    assert not failures, failures
    return net, optimizer
