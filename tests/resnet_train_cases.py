"""
Shared by the residual training tests (tests/test_resnet_train.py, tests/test_gpu_resnet_train.py), the fixture recipe
(muzero-general_amd/tools/make_resnet_train_golden.py) and the bench (tools/train_bench.py --family resnet): the case
table, the inputs and weights rebuilt from seeds (numpy.random.RandomState, float32 only), the gates, and the residual MuZero
network restated with plain torch.nn modules under the reference's state_dict keys (training mode: BatchNorm on batch
statistics).
"""
import collections
import functools
import hashlib
import json
import os
import sys

import numpy
import torch

import fc_train_cases
import train_cases_common as common
import trainer_loss_cases
from mzx import configs

# The smallest shapes that can still break each mechanism (B samples, steps = unroll steps + 1, board h x w).
CASES = [
    # no dynamics: its gradients are exactly 0.0, its running statistics keep their bits
    dict(name="a_b2_k1", B=2, steps=1, obs=(2, 2, 2), stacked=0, C=2, blocks=1, red=(2, 2, 2), rew=[], val=[], pol=[], A=4,
         S=1, per=False, alpha=1.0, vlw=1.0, seed=31),
    # the dynamics convolution is 6 -> 5, channels below one MFMA tile, 27 positions: a ragged M tile
    dict(name="b_b3_k3", B=3, steps=3, obs=(3, 3, 3), stacked=0, C=5, blocks=1, red=(2, 2, 2), rew=[4], val=[4], pol=[4], A=9,
         S=2, per=False, alpha=0.5, vlw=1.0, seed=32),
    # non-square board, a second ragged N tile, odd head widths, stacked planes, PER, two blocks
    dict(name="c_b5_k4_stacked", B=5, steps=4, obs=(1, 2, 5), stacked=2, C=20, blocks=2, red=(1, 2, 3), rew=[], val=[5, 4], pol=[3],
         A=5, S=10, per=True, alpha=0.6, vlw=0.25, seed=33, sgd=dict(lr=0.05, momentum=0.9, weight_decay=1e-4)),
    # 2940 positions per application: several workgroups, several chunks of the weight-gradient reduction
    dict(name="d_b70_k3", B=70, steps=3, obs=(3, 6, 7), stacked=0, C=20, blocks=1, red=(2, 2, 2), rew=[8], val=[8], pol=[8], A=7,
         S=3, per=True, alpha=0.5, vlw=0.25, seed=34),
    # case b with one channel of the last bn2 of the representation and dynamics networks at gamma = 0, beta = -100: that
    # channel is 0 over the whole board, the `scale += 1e-5` branch runs with arg-min == arg-max
    dict(name="e_b3_k3_dead", B=3, steps=3, obs=(3, 3, 3), stacked=0, C=5, blocks=1, red=(2, 2, 2), rew=[4], val=[4], pol=[4], A=9,
         S=2, per=False, alpha=0.5, vlw=1.0, seed=32, dead_channel=3),
]
# Shapes the fixture does not carry, held live to the restatement in binary64 (check_live).
LIVE_CASES = [
    # case b with one channel of the state between 0 and a few 1e-6 (the tiny_range recipe): 0 < range < 1e-5, the
    # `scale += 1e-5` branch with arg-min != arg-max.  Nothing else has such a range -- planes are constant (range exactly
    # 0) or of order 1 -- so a threshold of 1e-7 in place of 1e-5 passes every other case
    dict(name="f_b3_k3_tiny_range", B=3, steps=3, obs=(3, 3, 3), stacked=0, C=5, blocks=1, red=(2, 2, 2), rew=[4], val=[4], pol=[4],
         A=9, S=2, per=False, alpha=0.5, vlw=1.0, seed=32, tiny_channel=1),
]
BY_NAME = {c["name"]: c for c in CASES + LIVE_CASES}


def config_of(case, **kw):
    base = dict(observation_shape=case["obs"], stacked_observations=case["stacked"], action_space=list(range(case["A"])),
                players=[0], network="resnet", downsample=False, blocks=case["blocks"], channels=case["C"],
                reduced_channels_reward=case["red"][0], reduced_channels_value=case["red"][1],
                reduced_channels_policy=case["red"][2], resnet_fc_reward_layers=list(case["rew"]),
                resnet_fc_value_layers=list(case["val"]), resnet_fc_policy_layers=list(case["pol"]),
                support_size=case["S"], PER=case["per"], PER_alpha=case["alpha"], value_loss_weight=case["vlw"],
                num_unroll_steps=case["steps"] - 1, batch_size=case["B"], encoding_size=8, fc_representation_layers=[],
                fc_dynamics_layers=[], fc_reward_layers=[], fc_value_layers=[], fc_policy_layers=[])
    base.update(kw)
    return configs.HotPathConfig(**base)


def case_of_config(config, B, steps, seed=50, name=None):
    """A case (seeded weights and batch) for a shipped configuration, e.g. ``configs.connect4()``."""
    return dict(name=name or "config", B=B, steps=steps, obs=tuple(config.observation_shape), stacked=config.stacked_observations,
                C=config.channels, blocks=config.blocks,
                red=(config.reduced_channels_reward, config.reduced_channels_value, config.reduced_channels_policy),
                rew=list(config.resnet_fc_reward_layers), val=list(config.resnet_fc_value_layers),
                pol=list(config.resnet_fc_policy_layers), A=len(config.action_space), S=config.support_size, per=True,
                alpha=0.5, vlw=0.25, seed=seed)


input_channels = common.input_channels


# ---------------------------------------------------------------------------------------------------------------------
# The residual network in plain torch.nn (any dtype / device), parameters and buffers under the reference's state_dict
# keys: what the live test holds against the reference, what the device tests run in binary64 for shapes the fixture is
# too small to carry, and what the bench times as the path before the native one.

_Replicated = fc_train_cases._Replicated


def _conv3(cin, cout):
    return torch.nn.Conv2d(cin, cout, kernel_size=3, stride=1, padding=1, bias=False)


_mlp = common._mlp


class _Block(torch.nn.Module):
    def __init__(self, C):
        super().__init__()
        self.conv1, self.bn1 = _conv3(C, C), torch.nn.BatchNorm2d(C)
        self.conv2, self.bn2 = _conv3(C, C), torch.nn.BatchNorm2d(C)

    def forward(self, x):
        out = torch.relu(self.bn1(self.conv1(x)))
        return torch.relu(self.bn2(self.conv2(out)) + x)


class _Tower(torch.nn.Module):
    def __init__(self, cin, C, blocks):
        super().__init__()
        self.conv, self.bn = _conv3(cin, C), torch.nn.BatchNorm2d(C)
        self.resblocks = torch.nn.ModuleList([_Block(C) for _ in range(blocks)])

    def forward(self, x):
        x = torch.relu(self.bn(self.conv(x)))
        for block in self.resblocks:
            x = block(x)
        return x


class _Dynamics(_Tower):
    def __init__(self, C, blocks, reduced, layers, F, hw):
        super().__init__(C + 1, C, blocks)
        self.conv1x1_reward = torch.nn.Conv2d(C, reduced, 1)
        self.fc = _mlp([reduced * hw] + layers + [F])

    def forward(self, x):
        state = super().forward(x)
        return state, self.fc(self.conv1x1_reward(state).flatten(1))


class _Prediction(torch.nn.Module):
    def __init__(self, C, blocks, red_value, red_policy, value_layers, policy_layers, F, A, hw):
        super().__init__()
        self.resblocks = torch.nn.ModuleList([_Block(C) for _ in range(blocks)])
        self.conv1x1_value, self.conv1x1_policy = torch.nn.Conv2d(C, red_value, 1), torch.nn.Conv2d(C, red_policy, 1)
        self.fc_value = _mlp([red_value * hw] + value_layers + [F])
        self.fc_policy = _mlp([red_policy * hw] + policy_layers + [A])

    def forward(self, x):
        for block in self.resblocks:
            x = block(x)
        return self.fc_policy(self.conv1x1_policy(x).flatten(1)), self.fc_value(self.conv1x1_value(x).flatten(1))


_unit_range = functools.partial(common._unit_range, dim=2)      # per channel, over its board


class ResNetwork(torch.nn.Module):
    def __init__(self, case):
        super().__init__()
        C, A, F = case["C"], case["A"], 2 * case["S"] + 1
        hw = case["obs"][1] * case["obs"][2]
        self.A, self.F = A, F
        self.representation_network = _Replicated(_Tower(input_channels(case), C, case["blocks"]))
        self.dynamics_network = _Replicated(_Dynamics(C, case["blocks"], case["red"][0], list(case["rew"]), F, hw))
        self.prediction_network = _Replicated(_Prediction(C, case["blocks"], case["red"][1], case["red"][2], list(case["val"]),
                                                          list(case["pol"]), F, A, hw))

    def initial_inference(self, observation):
        state = _unit_range(self.representation_network(observation))
        policy, value = self.prediction_network(state)
        reward = torch.full((observation.shape[0], self.F), float("-inf"), device=observation.device, dtype=value.dtype)
        reward[:, self.F // 2] = 0.0
        return value, reward, policy, state

    def recurrent_inference(self, state, action):
        plane = torch.ones((state.shape[0], 1, state.shape[2], state.shape[3]), device=state.device, dtype=state.dtype)
        plane = action.reshape(-1, 1)[:, :, None, None] * plane / self.A
        raw, reward = self.dynamics_network(torch.cat((state, plane), dim=1))
        state = _unit_range(raw)
        policy, value = self.prediction_network(state)
        return value, reward, policy, state


def tensor_shapes(case):
    """OrderedDict key -> shape of every float tensor of the reference's state_dict, in its order (parameters and the
    running statistics; ``num_batches_tracked`` is left out)."""
    return collections.OrderedDict((k, tuple(v.shape)) for k, v in ResNetwork(case).state_dict().items()
                                   if not k.endswith("num_batches_tracked"))


is_statistic = common.is_statistic


def split(case, joined):
    """key -> array: a fixture vector that joins every tensor of the state_dict, flattened, in its order."""
    out, at = collections.OrderedDict(), 0
    for key, shape in tensor_shapes(case).items():
        n = int(numpy.prod(shape))
        out[key] = joined[at:at + n].reshape(shape)
        at += n
    assert at == joined.size
    return out


WEIGHT_SCALE = 1.0      # of the convolution / Linear weights (times 1 / sqrt(fan-in))


def weights(case):
    """The state_dict of the case (float32 numpy arrays), from its seed."""
    rs = numpy.random.RandomState(case["seed"] + 1000)
    out = collections.OrderedDict()
    for key, shape in tensor_shapes(case).items():
        draw = rs.uniform(-1, 1, size=shape).astype(numpy.float32)
        if len(shape) >= 2:
            out[key] = draw * numpy.float32(WEIGHT_SCALE / numpy.sqrt(numpy.prod(shape[1:])))
        elif key.endswith(".running_var"):
            out[key] = numpy.float32(1.0) + draw * numpy.float32(0.5)
        elif key.endswith(".running_mean"):
            out[key] = draw * numpy.float32(0.3)
        elif ".bn" in key and key.endswith(".weight"):
            out[key] = numpy.float32(1.0) + draw * numpy.float32(0.4)
        else:
            out[key] = draw * numpy.float32(0.3)
    if "dead_channel" in case:
        last = case["blocks"] - 1
        for net in ("representation_network", "dynamics_network"):
            out[f"{net}.module.resblocks.{last}.bn2.weight"][case["dead_channel"]] = 0.0
            out[f"{net}.module.resblocks.{last}.bn2.bias"][case["dead_channel"]] = -100.0
    if "tiny_channel" in case:
        tiny_range(out, case["blocks"], case["tiny_channel"])
    return out


def amplified(case):
    """The tensors whose gradient the tiny_range recipe amplifies by 1 / 1e-5 (train_cases_common.AMPLIFIED_ULPS)."""
    if "tiny_channel" not in case:
        return ()
    return tuple(f"{net}.module.resblocks.0.bn2.{leaf}" for net in ("representation_network", "dynamics_network")
                 for leaf in ("weight", "bias"))


def tiny_range(state, blocks, channel):
    """The ``tiny_range`` recipe on a state_dict (numpy arrays or tensors, in place): the first BatchNorm of the
    representation and dynamics towers gets gamma 0, beta -1 on ``channel`` (0 behind the ReLU, so the blocks' residual adds
    nothing), the last bn2 gamma 1e-6, beta 0: the channel of the state is relu(1e-6 x a normalised plane), 0 to a few 1e-6,
    anchored at 0: 0 < range < 1e-5, the `scale += 1e-5` branch with arg-min != arg-max, which nothing else reaches.  One
    block per tower (an earlier block's bn2 would put order-1 values into the channel).  The gradients of that bn2 are
    amplified by 1 / 1e-5: see ``amplified``."""
    assert blocks == 1
    for net in ("representation_network", "dynamics_network"):
        state[f"{net}.module.bn.weight"][channel] = 0.0
        state[f"{net}.module.bn.bias"][channel] = -1.0
        state[f"{net}.module.resblocks.0.bn2.weight"][channel] = 1e-6
        state[f"{net}.module.resblocks.0.bn2.bias"][channel] = 0.0
    return state


batch = common.batch


def digest(case):
    h = hashlib.sha1()
    for a in list(weights(case).values()) + [x for x in batch(case) if x is not None]:
        h.update(numpy.ascontiguousarray(a).tobytes())
    return h.hexdigest()


load = functools.partial(common.load, strict=False)


def torch_step(case, dtype, device="cpu", steps_of_sgd=0):
    """One training step of the restatement in ``dtype`` (training mode) -> dict: the step-major logits, losses, decoded
    values, ``grad/<key>`` per parameter and ``stat/<key>`` per running statistic after the step.  What the device tests
    hold the shapes against that the fixture does not carry (binary64 on the CPU)."""
    model = load(ResNetwork(case), weights(case)).to(dtype).to(device).train()
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
# Running a case through the native path (any backend) and the gates.  run_native, check_against, check_case, check_live
# and check_sgd exist once, here; their last argument ``tables`` is the module whose case tables they run on (``network``,
# ``batch``, ``config_of``, ``weights``, ``tensor_shapes``, ``split``, ``digest``, ``torch_step``, ``is_bypassed``,
# ``tracked_after``, ``TRACKED``): this module, or resnet_stem_train_cases, which binds them to itself under the same names.

THIS = sys.modules[__name__]


def golden(golden_dir):
    return numpy.load(os.path.join(golden_dir, "resnet_train.npz"))


def golden_keys(gold):
    return json.loads(str(gold["keys"]))


def network(be, case):
    from mzx import models
    net = models.MuZeroNetwork(config_of(case), _backend=be)
    net.set_weights({k: torch.from_numpy(v) for k, v in weights(case).items()})
    return net


def is_bypassed(key):
    """A tensor of the state_dict that no application reads (none here; behind a stem, the tower's first convolution)."""
    return False


def tracked_after(key, case, updates):
    """``num_batches_tracked`` of a BatchNorm after ``updates`` steps."""
    per_step = 1 if key.startswith("representation") else case["steps"] - 1 if key.startswith("dynamics") else case["steps"]
    return updates * per_step


# the groups of BatchNorms whose ``num_batches_tracked`` check_sgd has to meet
TRACKED = {"representation_network", "dynamics_network", "prediction_network"}


def run_native(be, case, net=None, tables=THIS):
    """mzx_train_resnet_step of a case through mzx.trainer.train_resnet_gradients -> dict of host arrays: losses,
    priorities, logits, grad/<key> per tensor and stat/<key> per running statistic after the step.  The gradient buffer
    is pre-filled with NaN: the call has to overwrite all of it."""
    from mzx import trainer
    net = net if net is not None else tables.network(be, case)
    stats = {}
    out = common.run_native(net, case, lambda logits: trainer.train_resnet_gradients(
        net, tables.batch(case), tables.config_of(case), logits=logits, stats=stats))
    out["running"] = stats["running"].cpu().numpy().copy()
    at = 0
    for key, off, numel, shape in net._tensors:
        if is_statistic(key):      # the packed statistics: [running_mean | running_var] per BatchNorm, in state_dict order
            out["stat/" + key] = out["running"][at:at + numel]
            at += numel
    assert at == out["running"].size
    for key, *_ in net._tensors:      # a bypassed BatchNorm counts no application
        if key.endswith(".running_var") and tables.is_bypassed(key):
            assert stats["applications"][key[:-len("running_var")]] == 0, key
    return out


LOGIT_GATE = fc_train_cases.LOGIT_GATE
LOSS_KEYS = fc_train_cases.LOSS_KEYS
# Parameter gradients and post-step running statistics, the yardstick of fc_train_cases: per tensor, max |ours - binary64
# reference| <= 4 x the error of the reference's own float32 result on that tensor, or a floor where that error happens to
# be small.  BatchNorm's 1 / sigma amplifies rounding, and the weight-gradient sums run over up to 8820 positions, so the
# floor is larger than the fully connected one.  It is MEASURED on the serial build (tests/test_resnet_train.py prints
# every figure, and per case the largest error on a tensor that needs the floor): the largest is 3.737e-7
# (b_b3_k3, representation_network.module.resblocks.0.conv2.weight; the reference's float32 error on it is below a quarter
# of the floor), times two, rounded up.
PARAM_GRAD_ERROR_FLOOR = 1.0e-6


def tensor_gate(ref_error):
    return max(4 * ref_error, PARAM_GRAD_ERROR_FLOOR)


def check_against(case, got, want32_logits, ref64, ref_errors, f32_losses, f32_pred, be, report=print, tables=THIS):
    """The gates of one case (train_cases_common.check_against) with this module's floor and head gate."""
    common.check_against(case, got, want32_logits, ref64, ref_errors, f32_losses, f32_pred, be, report, tables,
                         floor=PARAM_GRAD_ERROR_FLOOR, logit_gate=LOGIT_GATE)


def check_case(be, case, gold, report=print, tables=THIS):
    """Every gate of one fixture case; returns (network, outputs).  Figures are printed before they are asserted."""
    name = case["name"]
    assert tables.digest(case) == str(gold[f"{name}/digest"]), "this machine rebuilt other input bits than the fixture's"
    net = tables.network(be, case)
    got = run_native(be, case, net, tables)
    keys = list(tables.tensor_shapes(case))
    ref64 = {k: gold[f"{name}/f64_{k}"] for k in LOSS_KEYS}
    ref_errors = {}
    tensors = tables.split(case, gold[f"{name}/f64_tensors"])
    for key, error in zip(keys, gold[f"{name}/f32_errors"]):
        kind = "stat" if is_statistic(key) else "grad"
        ref64[f"{kind}/{key}"] = tensors[key]
        ref_errors[f"{kind}/{key}"] = error
    check_against(case, got, {h: gold[f"{name}/f32_{h}_logits"] for h in ("value", "reward", "policy")}, ref64, ref_errors,
                  {k: gold[f"{name}/f32_{k}"] for k in LOSS_KEYS}, gold[f"{name}/f32_pred"], be, report, tables)
    if case["steps"] == 1:      # no dynamics: exact zeros, statistics unchanged bit for bit
        state = tables.weights(case)
        for key in keys:
            if key.startswith("dynamics_"):
                assert numpy.array_equal(got["grad/" + key], numpy.zeros_like(got["grad/" + key])), key
                if is_statistic(key):
                    assert numpy.array_equal(got["stat/" + key].view(numpy.int32), state[key].view(numpy.int32)), key
    again = run_native(be, case, net, tables)
    for key, value in got.items():
        a, b = numpy.ascontiguousarray(value, numpy.float32), numpy.ascontiguousarray(again[key], numpy.float32)
        assert numpy.array_equal(a.view(numpy.int32), b.view(numpy.int32)), key
    return net, got


def check_live(be, case, report=print, tables=THIS):
    """The gates of ``check_case`` against the torch restatement run here in binary64 and float32 (shapes the fixture does
    not carry)."""
    ref64, ref32 = tables.torch_step(case, torch.float64), tables.torch_step(case, torch.float32)
    errors = {k: float(numpy.max(numpy.abs(ref32[k].astype(numpy.float64) - ref64[k]))) for k in ref64 if k[:5] in ("grad/", "stat/")}
    net = tables.network(be, case)
    got = run_native(be, case, net, tables)
    check_against(case, got, {h: ref32[f"{h}_logits"] for h in ("value", "reward", "policy")}, ref64, errors,
                  {k: ref32[k] for k in LOSS_KEYS}, ref32["pred"], be, report, tables)
    return net, got


def sgd_reference(gold, case, tables=THIS):
    """key -> the reference's binary64 tensor after two SGD steps: the fixture stores its distance from the initial float32
    value."""
    delta, initial = tables.split(case, gold[f"{case['name']}/f64_sgd_delta"]), tables.weights(case)
    return {key: initial[key].astype(numpy.float64) + delta[key].astype(numpy.float64) for key in initial}


def check_sgd(be, case, gold, report=print, tables=THIS):
    """Two ``update_weights`` steps with SGD-momentum and weight decay on the flat parameter against the reference's weights
    AND buffers after two steps.  Parameters: within lr x (1 + momentum) x the gradient gate (the second step's gradient is
    taken at weights that differ by the first step's error: x 2); running statistics: within twice their gate -- an
    optimizer's decay of them (the last step alone moves a variance near 1 by lr x (1 + momentum) x 1e-4, about 1e-5)
    would not pass.  ``num_batches_tracked`` rises by each network's applications (a stem's BatchNorms with the
    representation network, a bypassed one not at all), and every group of ``tables.TRACKED`` has to be met."""
    from mzx import trainer
    name, hp = case["name"], case["sgd"]
    net = tables.network(be, case)
    optimizer = torch.optim.SGD(net.parameters(), lr=hp["lr"], momentum=hp["momentum"], weight_decay=hp["weight_decay"])
    for _ in range(2):
        out = trainer.update_weights(net, optimizer, tables.batch(case), tables.config_of(case))
        assert isinstance(out[0], numpy.ndarray) and out[0].dtype == numpy.float32 and out[0].shape == (case["B"], case["steps"])
        assert all(type(v) is float for v in out[1:])
    failures = []
    state, want = net.get_weights(), sgd_reference(gold, case, tables)
    for key, error in zip(tables.tensor_shapes(case), gold[f"{name}/f32_errors"]):
        base = tensor_gate(float(error))
        gate = 2 * base if is_statistic(key) else 2 * hp["lr"] * (1 + hp["momentum"]) * base
        err = float(numpy.max(numpy.abs(state[key].numpy().astype(numpy.float64) - want[key])))
        report(f"{name} after two SGD steps {key}: error {err:.3e}, gate {gate:.3e}")
        if not err <= gate:
            failures.append(key)
    seen = set()
    for key, value in state.items():
        if key.endswith("num_batches_tracked"):
            assert int(value) == tables.tracked_after(key, case, 2), (key, int(value))
            seen.add("stem" if ".downsample_net." in key else "bypassed" if tables.is_bypassed(key) else key.split(".")[0])
    assert seen == tables.TRACKED, seen
    assert not failures, failures
    return net, optimizer


adam_reference_step = common.adam_reference_step
