"""
Shared by the fully connected training tests (tests/test_fc_train.py, tests/test_gpu_fc_train.py), the fixture recipe
(muzero-general_amd/tools/make_fc_train_golden.py) and the bench (tools/train_bench.py --family fc): the case table, the
inputs rebuilt from seeds (numpy.random.RandomState, float32 only, so every machine builds the same bits), the gates, and
the fully connected MuZero network restated with plain torch.nn modules under the reference's state_dict keys.  What the
residual case modules need as well lives in train_cases_common.
"""
import collections
import functools
import hashlib
import json
import os

import numpy
import torch

import train_cases_common as common
import trainer_loss_cases
from mzx import configs

# The smallest shapes that can still break each mechanism (B samples, steps = unroll steps + 1).
CASES = [
    # no dynamics: the gradients of the dynamics and reward networks are exactly 0.0
    dict(name="b1_k1_nolayers", B=1, steps=1, obs=(1, 1, 4), stacked=0, enc=3, rep=[], dyn=[], rew=[], val=[], pol=[], A=2,
         S=1, per=False, alpha=1.0, vlw=1.0, seed=21),
    # one state element: every state takes the `scale += 1e-5` branch with arg-min == arg-max
    dict(name="b3_k3_enc1", B=3, steps=3, obs=(1, 1, 4), stacked=0, enc=1, rep=[5], dyn=[5], rew=[5], val=[5], pol=[5], A=3,
         S=2, per=False, alpha=0.5, vlw=1.0, seed=22),
    # multi-layer MLPs, empty lists, odd widths, stacked planes in the input size
    dict(name="b5_k4_stacked", B=5, steps=4, obs=(1, 2, 3), stacked=2, enc=7, rep=[6, 5], dyn=[9], rew=[], val=[4, 4], pol=[3],
         A=9, S=10, per=True, alpha=0.6, vlw=0.25, seed=23, sgd=dict(lr=0.05, momentum=0.9, weight_decay=1e-4)),
    # CartPole's network: more than one workgroup, a ragged last workgroup, rows beyond one pass of the gradient sums
    dict(name="b130_k11_cartpole", B=130, steps=11, obs=(1, 1, 4), stacked=0, enc=8, rep=[], dyn=[16], rew=[16], val=[16],
         pol=[16], A=2, S=10, per=True, alpha=0.5, vlw=0.25, seed=24),
    # the widest rows the kernels take: support size 41 is the last one inside the 160 KiB LDS budget at this width
    # (WIDE_UNSUPPORTED_S = 42 is refused)
    dict(name="b2_k2_wide", B=2, steps=2, obs=(1, 1, 8), stacked=0, enc=64, rep=[64], dyn=[64], rew=[64], val=[64], pol=[64],
         A=18, S=41, per=False, alpha=1.0, vlw=1.0, seed=25),
]
WIDE_UNSUPPORTED_S = 42
# Shapes the fixture does not carry, held live to the restatement below in binary64 (check_live).
LIVE_CASES = [
    # wider than a wavefront everywhere: 72 inputs, an encoding of 70, 73 dynamics inputs with the action one-hot and hidden
    # layers of 72 take the second `j += 64` pass of every row loop, not the logits alone.  72 is the width that stays inside
    # the 160 KiB LDS budget: 37 530 floats of padded weights + 4 x 360 per wave of 40 960; hidden layers of 100 need 52 006
    # floats for the weights alone and are refused (OVER64_UNSUPPORTED_WIDTH, tests/test_fc_train.py)
    dict(name="b3_k3_over64", B=3, steps=3, obs=(1, 1, 72), stacked=0, enc=70, rep=[72], dyn=[72], rew=[72], val=[72],
         pol=[72], A=3, S=2, per=False, alpha=0.5, vlw=1.0, seed=26),
]
OVER64_UNSUPPORTED_WIDTH = 100
LIVE_CASES.append(
    # every state has 0 < range < 1e-5 (the tiny_range recipe): the `scale += 1e-5` branch with arg-min != arg-max.  Nothing
    # else has such a range, so a threshold of 1e-7 in place of 1e-5 passes every other case
    dict(name="b3_k3_tiny_range", B=3, steps=3, obs=(1, 1, 4), stacked=0, enc=6, rep=[5], dyn=[5], rew=[5], val=[5], pol=[5], A=3,
         S=2, per=False, alpha=0.5, vlw=1.0, seed=27, tiny_range=True))
BY_NAME = {c["name"]: c for c in CASES + LIVE_CASES}


def config_of(case, **kw):
    """A config with the attributes the network factories and the trainer read."""
    base = dict(observation_shape=case["obs"], stacked_observations=case["stacked"], action_space=list(range(case["A"])),
                players=[0], network="fullyconnected", encoding_size=case["enc"], support_size=case["S"],
                fc_representation_layers=list(case["rep"]), fc_dynamics_layers=list(case["dyn"]),
                fc_reward_layers=list(case["rew"]), fc_value_layers=list(case["val"]), fc_policy_layers=list(case["pol"]),
                PER=case["per"], PER_alpha=case["alpha"], value_loss_weight=case["vlw"], num_unroll_steps=case["steps"] - 1,
                batch_size=case["B"])
    base.update(kw)
    return configs.HotPathConfig(**base)


def input_size(case):
    c, h, w = case["obs"]
    return c * h * w * (case["stacked"] + 1) + case["stacked"] * h * w


def tensor_shapes(case):
    """OrderedDict key -> shape: the reference's state_dict of this configuration, in its order."""
    E, A, F = case["enc"], case["A"], 2 * case["S"] + 1
    out = collections.OrderedDict()
    for name, sizes in (("representation_network", [input_size(case)] + case["rep"] + [E]),
                        ("dynamics_encoded_state_network", [E + A] + case["dyn"] + [E]),
                        ("dynamics_reward_network", [E] + case["rew"] + [F]),
                        ("prediction_policy_network", [E] + case["pol"] + [A]),
                        ("prediction_value_network", [E] + case["val"] + [F])):
        for i in range(len(sizes) - 1):
            out[f"{name}.module.{2 * i}.weight"] = (sizes[i + 1], sizes[i])
            out[f"{name}.module.{2 * i}.bias"] = (sizes[i + 1],)
    return out


def weights(case):
    """The state_dict of the case (float32 numpy arrays), from its seed."""
    rs = numpy.random.RandomState(case["seed"] + 1000)
    out = collections.OrderedDict()
    for key, shape in tensor_shapes(case).items():
        if key.endswith("weight"):
            bound = numpy.float32(1.5 / numpy.sqrt(shape[1]))
            out[key] = (rs.uniform(-1, 1, size=shape).astype(numpy.float32) * bound)
        else:
            out[key] = (rs.uniform(-1, 1, size=shape).astype(numpy.float32) * numpy.float32(0.5))
    if case.get("tiny_range"):
        tiny_range(out, len(case["rep"]), len(case["dyn"]))
    return out


def amplified(case):
    """The tensors whose gradient the tiny_range recipe amplifies by 1 / 1e-5 (train_cases_common.AMPLIFIED_ULPS)."""
    if not case.get("tiny_range"):
        return ()
    return tuple(f"{name}.module.{2 * n}.{leaf}" for name, n in (("representation_network", len(case["rep"])),
                                                                 ("dynamics_encoded_state_network", len(case["dyn"])))
                 for leaf in ("weight", "bias"))


def tiny_range(state, rep_layers, dyn_layers):
    """The ``tiny_range`` recipe on a state_dict (numpy arrays or tensors, in place): the last layer of the representation
    and dynamics networks gets weight x 1e-7 and bias 0, so every state is about 1e-7 to 3e-6, anchored at 0: 0 < range <
    1e-5, the `scale += 1e-5` branch with arg-min != arg-max, which nothing else reaches (synthetic and trained states have
    ranges of order 1 or exactly 0).  The gradients of those two layers are amplified by 1 / 1e-5: see ``amplified``."""
    for name, n in (("representation_network", rep_layers), ("dynamics_encoded_state_network", dyn_layers)):
        state[f"{name}.module.{2 * n}.weight"] *= 1e-7
        state[f"{name}.module.{2 * n}.bias"] *= 0
    return state


batch = common.batch


def digest(case):
    h = hashlib.sha1()
    for a in list(weights(case).values()) + [x for x in batch(case) if x is not None]:
        h.update(numpy.ascontiguousarray(a).tobytes())
    return h.hexdigest()


# ---------------------------------------------------------------------------------------------------------------------
# The fully connected network in plain torch.nn (any dtype / device), parameters under the reference's state_dict keys:
# what the live test holds against the reference and what the bench times as the path before the native one.

class _Replicated(torch.nn.Module):
    """Gives a sub-network the ``.module.`` infix DataParallel puts into the keys."""

    def __init__(self, module):
        super().__init__()
        self.module = module

    def forward(self, x):
        return self.module(x)


def _mlp(sizes):
    return _Replicated(common._mlp(sizes))


_unit_range = functools.partial(common._unit_range, dim=1)


class FcNetwork(torch.nn.Module):
    def __init__(self, case):
        super().__init__()
        E, A, F = case["enc"], case["A"], 2 * case["S"] + 1
        self.A, self.F = A, F
        self.representation_network = _mlp([input_size(case)] + case["rep"] + [E])
        self.dynamics_encoded_state_network = _mlp([E + A] + case["dyn"] + [E])
        self.dynamics_reward_network = _mlp([E] + case["rew"] + [F])
        self.prediction_policy_network = _mlp([E] + case["pol"] + [A])
        self.prediction_value_network = _mlp([E] + case["val"] + [F])

    def initial_inference(self, observation):
        state = _unit_range(self.representation_network(observation.view(observation.shape[0], -1)))
        policy = self.prediction_policy_network(state)
        value = self.prediction_value_network(state)
        reward = torch.full((observation.shape[0], self.F), float("-inf"), device=observation.device)   # log of a one-hot
        reward[:, self.F // 2] = 0.0
        return value, reward, policy, state

    def recurrent_inference(self, state, action):
        one_hot = torch.nn.functional.one_hot(action.long().reshape(-1), self.A).to(torch.float32)
        raw = self.dynamics_encoded_state_network(torch.cat((state, one_hot), dim=1))
        reward = self.dynamics_reward_network(raw)
        state = _unit_range(raw)
        policy = self.prediction_policy_network(state)
        value = self.prediction_value_network(state)
        return value, reward, policy, state


load = common.load


# ---------------------------------------------------------------------------------------------------------------------
# Running a case through the native path (any backend: the serial test double on host tensors, the product library on
# the device) and the gates both test files apply.

def golden(golden_dir):
    return numpy.load(os.path.join(golden_dir, "fc_train.npz"))


def golden_keys(gold):
    return json.loads(str(gold["keys"]))


def network(be, case):
    from mzx import models
    net = models.MuZeroNetwork(config_of(case), _backend=be)
    net.set_weights({k: torch.from_numpy(v) for k, v in weights(case).items()})
    return net


def run_native(be, case, net=None):
    """mzx_train_fc_step of a case through mzx.trainer.train_fc_gradients -> the dict of ``common.run_native``."""
    from mzx import trainer
    net = net if net is not None else network(be, case)
    return common.run_native(net, case, lambda logits: trainer.train_fc_gradients(net, batch(case), config_of(case), logits=logits))


def is_bypassed(key):
    return False


def torch_step(case, dtype, device="cpu"):
    """One training step of the restatement in ``dtype`` -> dict: the step-major logits, losses, decoded values and
    ``grad/<key>`` per parameter (the layout of resnet_train_cases.torch_step)."""
    model = load(FcNetwork(case), weights(case)).to(dtype).to(device)
    observation, action, tv, tr, tp, weight, scale = batch(case)
    t = lambda a: torch.tensor(a).to(dtype).to(device)
    observation, tv, tr, tp, scale = t(observation), t(tv), t(tr), t(tp), t(scale)
    weight = t(weight) if case["per"] else None
    action = torch.tensor(action).long().to(device)
    value, reward, policy, hidden = model.initial_inference(observation)
    reward = reward.to(dtype)
    values, rewards, policies = [value], [reward], [policy]
    for i in range(1, action.shape[1]):
        one_hot = torch.nn.functional.one_hot(action[:, i], model.A).to(dtype)
        raw = model.dynamics_encoded_state_network(torch.cat((hidden, one_hot), dim=1))
        reward = model.dynamics_reward_network(raw)
        hidden = _unit_range(raw)
        policy, value = model.prediction_policy_network(hidden), model.prediction_value_network(hidden)
        hidden.register_hook(lambda grad: grad * 0.5)
        values.append(value), rewards.append(reward), policies.append(policy)
    loss, vl, rl, pl, _ = trainer_loss_cases.torch_loss_head(values, rewards, policies, tv, tr, tp, weight, scale, config_of(case))
    loss.backward()
    out = dict(loss=loss.item(), value_loss=vl.mean().item(), reward_loss=rl.mean().item(), policy_loss=pl.mean().item(),
               value_logits=torch.stack(values).detach().cpu().numpy(), reward_logits=torch.stack(rewards).detach().cpu().numpy(),
               policy_logits=torch.stack(policies).detach().cpu().numpy(),
               pred=numpy.stack([trainer_loss_cases.torch_support_to_scalar(v.detach(), case["S"]).cpu().numpy().squeeze(-1)
                                 for v in values], 1))
    for key, p in model.named_parameters():
        out["grad/" + key] = numpy.zeros(tuple(p.shape)) if p.grad is None else p.grad.detach().cpu().numpy().copy()
    return out


def check_live(be, case, report=print):
    """The gates of ``check_case`` against the torch restatement run here in binary64 and float32 (shapes the fixture does
    not carry), in the shape of resnet_train_cases.check_live; train_cases_common.check_against applies them with this module's floor."""
    import sys
    ref64, ref32 = torch_step(case, torch.float64), torch_step(case, torch.float32)
    errors = {k: float(numpy.max(numpy.abs(ref32[k].astype(numpy.float64) - ref64[k]))) for k in ref64 if k.startswith("grad/")}
    net = network(be, case)
    got = run_native(be, case, net)
    common.check_against(case, got, {h: ref32[f"{h}_logits"] for h in ("value", "reward", "policy")}, ref64, errors,
                         {k: ref32[k] for k in LOSS_KEYS}, ref32["pred"], be, report, sys.modules[__name__],
                         floor=PARAM_GRAD_ERROR_FLOOR, logit_gate=LOGIT_GATE)
    again = run_native(be, case, net)
    for key, value in got.items():
        a, b = numpy.ascontiguousarray(value, numpy.float32), numpy.ascontiguousarray(again[key], numpy.float32)
        assert numpy.array_equal(a.view(numpy.int32), b.view(numpy.int32)), key
    return net, got


LOGIT_GATE = 1e-4           # the heads, against the reference's float32 results
LOSS_KEYS = ("loss", "value_loss", "reward_loss", "policy_loss")
# Parameter gradients, the yardstick of trainer_loss_cases: per tensor, max |ours - binary64 reference| <= 4 x the error of
# the reference's own float32 gradient of that tensor, or a floor where that error happens to be small (a gradient is a sum
# over up to 1430 rows here; torch's blocked sums land closer to binary64 than a plain running sum on some tensors).  The
# floor is MEASURED on the serial build (tests/test_fc_train.py prints every figure): the largest error there on a tensor
# that needs the floor is 4.7e-7 (b130_k11_cartpole, dynamics_encoded_state_network.module.2.weight; the reference's
# float32 error on it is 5.0e-8), times two, rounded.
PARAM_GRAD_ERROR_FLOOR = 1.0e-6


def grad_gate(gold, case, key):
    name = case["name"]
    ref64 = gold[f"{name}/f64_grad/{key}"]
    ref = float(numpy.max(numpy.abs(gold[f"{name}/f32_grad/{key}"].astype(numpy.float64) - ref64)))
    return max(4 * ref, PARAM_GRAD_ERROR_FLOOR), ref


def check_case(be, case, gold, report=print):
    """Every gate of one case; returns (network, outputs).  Figures are printed before they are asserted."""
    name = case["name"]
    assert digest(case) == str(gold[f"{name}/digest"]), "this machine rebuilt other input bits than the fixture's"
    net = network(be, case)
    got = run_native(be, case, net)
    failures = []
    # logits: the project's head gate against the reference's float32 (the reward rows of step 0 are 0 / -inf: equal)
    for head in ("value", "reward", "policy"):
        ours, ref = got[f"{head}_logits"], gold[f"{name}/f32_{head}_logits"]
        assert ours.shape == ref.shape, (head, ours.shape, ref.shape)
        finite = numpy.isfinite(ref)
        assert numpy.array_equal(ours[~finite], ref[~finite]), head
        err = float(numpy.max(numpy.abs(ours[finite].astype(numpy.float64) - ref[finite]))) if finite.any() else 0.0
        report(f"{name} {head} logits: error {err:.3e} against the reference float32, gate {LOGIT_GATE:.1e}")
        if not err <= LOGIT_GATE:
            failures.append(head)
    # losses: the gates of trainer_loss_cases.check_case
    for key in LOSS_KEYS:
        ref64 = float(gold[f"{name}/f64_{key}"])
        mine, ref = abs(float(got[key]) - ref64), abs(float(gold[f"{name}/f32_{key}"]) - ref64)
        gate = max(4 * ref, trainer_loss_cases.LOSS_ERROR_FLOOR)
        report(f"{name} {key}: error {mine:.3e}, reference float32 error {ref:.3e}, gate {gate:.3e}")
        if not mine <= gate:
            failures.append(key)
    # priorities: the prediction has the bits of mzx_support_to_scalar of OUR value logits; the power is numpy's
    logits = torch.from_numpy(got["value_logits"]).to(be.device).reshape(-1, 2 * case["S"] + 1)
    pred = be.empty((logits.shape[0],), torch.float32)
    be.lib.check(be.lib.mzx_support_to_scalar(be.ptr(logits), logits.shape[0], case["S"], be.ptr(pred), be.stream()))
    pred = pred.cpu().numpy().reshape(case["steps"], case["B"]).T.copy()
    target_value = batch(case)[2]
    want = numpy.abs(pred - target_value) ** case["alpha"]
    assert want.dtype == numpy.float32
    ulps = trainer_loss_cases.ulp_distance(want, got["priorities"])
    report(f"{name} priorities: max ulp distance {ulps.max()} (alpha {case['alpha']})")
    assert ulps.max() <= (0 if case["alpha"] == 1.0 else 1)
    gap = numpy.abs(pred.astype(numpy.float64) - gold[f"{name}/f32_pred"])
    report(f"{name} decoded value against the reference: {gap.max():.3e} (values up to {numpy.abs(pred).max():.2f})")
    assert gap.max() <= trainer_loss_cases.DECODED_SCALAR_GATE
    # parameter gradients, per tensor
    assert not numpy.isnan(got["grad_flat"]).any(), "d_grad_flat was not fully overwritten"
    for key in tensor_shapes(case):
        gate, ref = grad_gate(gold, case, key)
        mine = float(numpy.max(numpy.abs(got["grad/" + key].astype(numpy.float64) - gold[f"{name}/f64_grad/{key}"])))
        report(f"{name} grad {key}: error {mine:.3e}, reference float32 error {ref:.3e}, gate {gate:.3e}")
        if not mine <= gate:
            failures.append(key)
    assert not failures, failures
    if case["steps"] == 1:      # no dynamics: exact zeros
        for key in tensor_shapes(case):
            if key.startswith("dynamics_"):
                assert numpy.array_equal(got["grad/" + key], numpy.zeros_like(got["grad/" + key])), key
    # a second call: identical bits in every output
    again = run_native(be, case, net)
    for key, value in got.items():
        a, b = numpy.ascontiguousarray(value, numpy.float32), numpy.ascontiguousarray(again[key], numpy.float32)
        assert numpy.array_equal(a.view(numpy.int32), b.view(numpy.int32)), key
    return net, got


def check_sgd(be, case, gold, report=print):
    """Two ``update_weights`` steps with SGD-momentum on the flat parameter against the reference's weights after two
    steps: within lr x (1 + momentum) x the gradient gate of the tensor."""
    from mzx import trainer
    name, hp = case["name"], case["sgd"]
    net = network(be, case)
    optimizer = torch.optim.SGD(net.parameters(), lr=hp["lr"], momentum=hp["momentum"], weight_decay=hp["weight_decay"])
    for _ in range(2):
        out = trainer.update_weights(net, optimizer, batch(case), config_of(case))
        assert isinstance(out[0], numpy.ndarray) and out[0].dtype == numpy.float32 and out[0].shape == (case["B"], case["steps"])
        assert all(type(v) is float for v in out[1:])
    failures = []
    state = net.get_weights()
    for key in tensor_shapes(case):
        gate = hp["lr"] * (1 + hp["momentum"]) * grad_gate(gold, case, key)[0]
        err = float(numpy.max(numpy.abs(state[key].numpy().astype(numpy.float64) - gold[f"{name}/f64_sgd/{key}"])))
        report(f"{name} after two SGD steps {key}: error {err:.3e}, gate {gate:.3e}")
        if not err <= gate:
            failures.append(key)
    assert not failures, failures
    return net, optimizer


def adam_reference_step(net, grad_flat, flat_before, **hp):
    """torch Adam applied PER TENSOR to the flat gradient split by mzx_net_tensor_info -> the flat weights after."""
    return torch.cat([p.reshape(-1) for p in common.adam_reference_step(net, grad_flat, flat_before, **hp).values()])
