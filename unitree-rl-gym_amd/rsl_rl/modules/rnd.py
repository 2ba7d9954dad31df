"""Random network distillation (rsl_rl 2.x `RandomNetworkDistillation`).

A `predictor` MLP is trained to match a frozen, randomly initialised `target` MLP on the states
the policy visits; the prediction error ||target(s) - predictor(s)||_2, times a scheduled weight,
is paid to the policy as an exploration bonus.

`parse_cfg` is the one reader of `algorithm.rnd_cfg` (rsl_rl's key names and our `state` key);
`weight_at` the one statement of the weight schedules.  The counter of a schedule is the number
of env steps taken, iteration x T + t.
"""
import torch
import torch.nn as nn

from .actor_critic import mlp

RND_KEYS = ("weight", "weight_schedule", "learning_rate", "num_outputs", "predictor_hidden_dims",
            "target_hidden_dims", "reward_normalization", "state_normalization", "state", "seed")
SCHEDULE_KEYS = {"constant": (), "step": ("final_step", "final_value"),
                 "linear": ("initial_step", "final_step", "final_value")}
STATES = ("critic", "policy")


def parse_cfg(cfg):
    """The checked rnd_cfg with its defaults filled in, or None when RND is off (absent, None, or
    weight 0 with no schedule).  Unknown keys and the two normalisers raise ValueError."""
    if cfg is None:
        return None
    cfg = dict(cfg)
    unknown = sorted(set(cfg) - set(RND_KEYS))
    if unknown:
        raise ValueError(f"rnd_cfg: unknown keys {unknown} (known: {list(RND_KEYS)})")
    sched = cfg.get("weight_schedule")
    if sched is not None:
        sched = dict(sched)
        mode = sched.get("mode")
        if mode not in SCHEDULE_KEYS:
            raise ValueError(f"rnd_cfg.weight_schedule: unknown mode {mode!r} (known: {list(SCHEDULE_KEYS)})")
        want = set(SCHEDULE_KEYS[mode]) | {"mode"}
        if set(sched) != want:
            raise ValueError(f"rnd_cfg.weight_schedule: mode {mode!r} takes exactly the keys {sorted(want)}")
        if mode == "linear" and not sched["final_step"] > sched["initial_step"]:
            raise ValueError("rnd_cfg.weight_schedule: linear needs final_step > initial_step")
    weight = float(cfg.get("weight", 0.0))
    if weight == 0.0 and sched is None:
        return None
    if cfg.get("reward_normalization", False):
        raise ValueError("rnd_cfg.reward_normalization is not supported: its running statistics are sequential in "
                         "the env step, and the bonus is computed once per rollout")
    if cfg.get("state_normalization", False):
        raise ValueError("rnd_cfg.state_normalization is not supported: its running statistics are sequential in "
                         "the env step (the runner's empirical_normalization already normalises the stored rows)")
    state = cfg.get("state", "critic")
    if state not in STATES:
        raise ValueError(f"rnd_cfg.state: {state!r} (known: {list(STATES)})")
    return dict(weight=weight, weight_schedule=sched, learning_rate=float(cfg.get("learning_rate", 1e-3)),
                num_outputs=int(cfg.get("num_outputs", 16)),
                predictor_hidden_dims=list(cfg.get("predictor_hidden_dims", [256, 128, 64])),
                target_hidden_dims=list(cfg.get("target_hidden_dims", [256, 128, 64])),
                reward_normalization=False, state_normalization=False, state=state, seed=int(cfg.get("seed", 0)))


def weight_at(initial_weight, schedule, step):
    """The bonus weight at env-step counter `step` (rsl_rl's constant / step / linear schedules)."""
    w0 = float(initial_weight)
    if schedule is None or schedule["mode"] == "constant":
        return w0
    if schedule["mode"] == "step":
        return float(schedule["final_value"]) if step >= schedule["final_step"] else w0
    s0, s1, w1 = schedule["initial_step"], schedule["final_step"], float(schedule["final_value"])
    if step <= s0:
        return w0
    if step >= s1:
        return w1
    return w0 + (w1 - w0) * (step - s0) / (s1 - s0)


class RandomNetworkDistillation(nn.Module):
    def __init__(self, num_states, cfg, device="cpu"):
        """cfg: a parse_cfg result (or the raw dict, which is parsed; it must switch RND on)."""
        super().__init__()
        if "reward_normalization" not in cfg or "seed" not in cfg or "state" not in cfg:
            cfg = parse_cfg(cfg)
        if cfg is None:
            raise ValueError("RandomNetworkDistillation: the rnd_cfg switches RND off")
        self.cfg = cfg
        self.num_states, self.num_outputs = int(num_states), cfg["num_outputs"]
        self.initial_weight, self.weight_schedule = cfg["weight"], cfg["weight_schedule"]
        self.update_counter = 0  # env steps taken
        # under a forked RNG: switching RND on does not move the global stream the policy's
        # initialisation and the mini-batch permutations draw from
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(cfg["seed"])
            self.predictor = mlp(self.num_states, cfg["predictor_hidden_dims"], self.num_outputs, nn.ELU())
            self.target = mlp(self.num_states, cfg["target_hidden_dims"], self.num_outputs, nn.ELU())
        for p in self.target.parameters():
            p.requires_grad = False
        self.target.eval()
        self.to(device)

    def weight_at(self, step):
        return weight_at(self.initial_weight, self.weight_schedule, step)

    @property
    def weight(self):
        return self.weight_at(self.update_counter)

    def error(self, rnd_state):
        """||target(s) - predictor(s)||_2 per row, nothing tracked."""
        with torch.no_grad():
            d = self.target(rnd_state) - self.predictor(rnd_state)
            return torch.sqrt((d * d).sum(dim=1))

    def get_intrinsic_reward(self, rnd_state):
        """rsl_rl's per-step statement: the weighted error per row; advances the step counter."""
        r = self.error(rnd_state) * self.weight
        self.update_counter += 1
        return r

    def train(self, mode=True):
        self.predictor.train(mode)  # the target stays in eval mode
        return self

    def forward(self, *args, **kwargs):
        raise NotImplementedError
