"""
Writes tests/golden/trainer_loss.npz: what the UNMODIFIED reference computes between the network's logits and
loss.backward() (trainer.py:161-258) for the cases of tests/trainer_loss_cases.py.

    python muzero-general_amd/tools/make_trainer_loss_golden.py

Needs the reference checkout (oracle.ref_shim; `import trainer` works under the shim's ray stub).  Per case `<name>/...`:
  digest            sha1 of the input arrays (the inputs themselves are rebuilt from seeds by trainer_loss_cases.inputs)
  f32_*             float32: Trainer.update_weights ITSELF, called unbound on a stand-in `self` whose model hands out the
                    case's logits as leaf tensors (so autograd leaves d loss / d logit on them) and whose optimizer does
                    nothing: loss, value_loss, reward_loss, policy_loss (the returned log numbers), priorities, and
                    grad_value / grad_reward / grad_policy [steps, B, width]; f32_pred is models.support_to_scalar of
                    the value logits.  f32_support_value / f32_support_reward are models.scalar_to_support of the
                    targets with torch.sqrt correctly rounded (trainer_loss_cases.ieee_sqrt says why): the rows the
                    tests compare bit for bit.
                    (The case without an unroll step goes through the loop below in float32: update_weights needs one.)
  f64_*             the same quantities in binary64: Trainer.loss_function, models.scalar_to_support and
                    models.support_to_scalar driven by the loop below under torch.set_default_dtype(torch.float64)
                    (update_weights itself casts to float32; scalar_to_support allocates in the default dtype).
The gradient scales of a case are constant over the unroll steps of a sample, as ReplayBuffer.get_batch produces them
(replay_buffer.py:103-111); the reference's hook closures read the scale column of the LAST step for every step, which
is the same number then.
Only data goes into the file.
"""
import hashlib
import os
import sys
import types

import numpy
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "tests"), ROOT, os.path.join(ROOT, "muzero-general_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
import trainer_loss_cases as cases  # noqa: E402
from oracle import ref_shim  # noqa: E402


def digest(x):
    h = hashlib.sha1()
    for key in sorted(x):
        if x[key] is not None:
            h.update(numpy.ascontiguousarray(x[key]).tobytes())
    return h.hexdigest()


class LeafModel:
    """initial_inference / recurrent_inference that hand out prepared per-step logits."""

    def __init__(self, values, rewards, policies):
        self.steps = list(zip(values, rewards, policies))
        self.at = 0

    def parameters(self):
        return iter([torch.zeros(1)])

    def _next(self):
        v, r, p = self.steps[self.at]
        self.at += 1
        return v, r, p, torch.zeros(1, requires_grad=True)

    def initial_inference(self, observation):
        return self._next()

    def recurrent_inference(self, hidden_state, action):
        return self._next()


class NoOptimizer:
    def zero_grad(self):
        pass

    def step(self):
        pass


def leaves(array, dtype):
    return [torch.tensor(a, dtype=dtype, requires_grad=True) for a in array]


def support_rows(ref_models, case, x):
    """models.scalar_to_support of the targets in float32, with a correctly rounded square root (cases.ieee_sqrt)."""
    with cases.ieee_sqrt():
        return dict(support_value=ref_models.scalar_to_support(torch.tensor(x["target_value"]), case["S"]).numpy(),
                    support_reward=ref_models.scalar_to_support(torch.tensor(x["target_reward"]), case["S"]).numpy())


def reference_f32(ref_trainer, ref_models, case, x):
    if case["steps"] == 1:       # update_weights itself needs an unroll step (its reward loss stays the integer 0)
        out = reference_loop(ref_trainer, ref_models, case, x, torch.float32)
        out.update(support_rows(ref_models, case, x))
        return {k: (numpy.float32(v) if numpy.ndim(v) == 0 else v.astype(numpy.float32)) for k, v in out.items()}
    v, r, p = (leaves(x[k], torch.float32) for k in ("value", "reward", "policy"))
    cfg = types.SimpleNamespace(support_size=case["S"], PER=case["per"], PER_alpha=case["alpha"], value_loss_weight=case["vlw"])
    me = types.SimpleNamespace(model=LeafModel(v, r, p), optimizer=NoOptimizer(), config=cfg, training_step=0,
                               loss_function=ref_trainer.Trainer.loss_function)
    B, steps = case["B"], case["steps"]
    batch = (numpy.zeros((B, 1), numpy.float32), numpy.zeros((B, steps), numpy.int64), x["target_value"], x["target_reward"],
             x["target_policy"], x["weight"], x["gradient_scale"])
    priorities, loss, value_loss, reward_loss, policy_loss = ref_trainer.Trainer.update_weights(me, batch)
    grad = lambda leaf_list, like: numpy.stack([numpy.zeros_like(like[i]) if t.grad is None else t.grad.numpy()
                                                for i, t in enumerate(leaf_list)])
    pred = numpy.stack([ref_models.support_to_scalar(t.detach(), case["S"]).numpy().squeeze(-1) for t in v], 1)
    return dict(loss=numpy.float32(loss), value_loss=numpy.float32(value_loss), reward_loss=numpy.float32(reward_loss),
                policy_loss=numpy.float32(policy_loss), priorities=priorities.astype(numpy.float32),
                grad_value=grad(v, x["value"]), grad_reward=grad(r, x["reward"]), grad_policy=grad(p, x["policy"]),
                pred=pred.astype(numpy.float32), **support_rows(ref_models, case, x))


def reference_loop(ref_trainer, ref_models, case, x, f64=torch.float64):
    """Trainer.loss_function, models.scalar_to_support and models.support_to_scalar in the dtype ``f64``."""
    torch.set_default_dtype(f64)
    try:
        v, r, p = (leaves(x[k], f64) for k in ("value", "reward", "policy"))
        S, steps = case["S"], case["steps"]
        tv_scalar = torch.tensor(x["target_value"], dtype=f64)
        tv = ref_models.scalar_to_support(tv_scalar, S)
        tr = ref_models.scalar_to_support(torch.tensor(x["target_reward"], dtype=f64), S)
        tp = torch.tensor(x["target_policy"], dtype=f64)
        scale = torch.tensor(x["gradient_scale"], dtype=f64)
        value_loss = reward_loss = policy_loss = 0
        kind = numpy.float64 if f64 == torch.float64 else numpy.float32
        priorities, pred = numpy.zeros((case["B"], steps), kind), numpy.zeros((case["B"], steps), kind)
        for i in range(steps):
            vl, rl, pl = ref_trainer.Trainer.loss_function(v[i], r[i], p[i], tv[:, i], tr[:, i], tp[:, i])
            if i > 0:
                for term in (vl, rl, pl):
                    term.register_hook(lambda grad, i=i: grad / scale[:, i])
                reward_loss = reward_loss + rl
            value_loss = value_loss + vl
            policy_loss = policy_loss + pl
            pred[:, i] = ref_models.support_to_scalar(v[i].detach(), S).numpy().squeeze(-1)
            priorities[:, i] = numpy.abs(pred[:, i] - tv_scalar[:, i].numpy()) ** case["alpha"]
        if not torch.is_tensor(reward_loss):
            reward_loss = torch.zeros_like(value_loss)
        loss = value_loss * case["vlw"] + reward_loss + policy_loss
        if case["per"]:
            loss = loss * torch.tensor(x["weight"], dtype=f64)
        loss = loss.mean()
        loss.backward()
        grad = lambda leaf_list, like: numpy.stack([numpy.zeros(like[i].shape) if t.grad is None else t.grad.numpy()
                                                    for i, t in enumerate(leaf_list)])
        return dict(loss=loss.item(), value_loss=value_loss.mean().item(), reward_loss=reward_loss.mean().item(),
                    policy_loss=policy_loss.mean().item(), priorities=priorities, pred=pred,
                    grad_value=grad(v, x["value"]), grad_reward=grad(r, x["reward"]), grad_policy=grad(p, x["policy"]))
    finally:
        torch.set_default_dtype(torch.float32)


def main():
    ref_models, _ = ref_shim.load()
    import trainer as ref_trainer  # the reference's trainer.py, under the shim's ray stub

    out = {}
    for case in cases.CASES:
        x = cases.inputs(case)
        out[f"{case['name']}/digest"] = numpy.array(digest(x))
        for tag, fn in (("f32", reference_f32), ("f64", reference_loop)):
            for key, value in fn(ref_trainer, ref_models, case, x).items():
                out[f"{case['name']}/{tag}_{key}"] = numpy.asarray(value)
        assert all(numpy.isfinite(v).all() for k, v in out.items() if k.startswith(case["name"]) and v.dtype.kind == "f"), case
    path = os.path.join(ROOT, "tests", "golden", "trainer_loss.npz")
    numpy.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
