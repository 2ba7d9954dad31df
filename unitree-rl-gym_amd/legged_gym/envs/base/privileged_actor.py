"""PrivilegedActorRobot: LeggedRobot whose VecEnv surface presents the privileged row as THE
observation (env cfg `privileged_as_observations`): the teacher tasks of the
teacher-student recipe.  The native step is untouched: it still builds the noisy policy row and
the privileged row; only what the runner sees changes, so PPO, the captured rollout, play.py and
the export work as for any task with one observation row (actor and critic share the clean row)."""
from .legged_robot import LeggedRobot


def presented_widths(cfg):
    """(num_obs, num_privileged_obs) as the env of cfg presents them to a runner."""
    e = cfg.env
    if getattr(e, "privileged_as_observations", False):
        if e.num_privileged_obs is None:
            raise ValueError("env.privileged_as_observations needs a privileged row (env.num_privileged_obs)")
        return e.num_privileged_obs, None
    return e.num_observations, e.num_privileged_obs


class PrivilegedActorRobot(LeggedRobot):
    def __init__(self, cfg, sim_params, physics_engine, sim_device, headless):
        super().__init__(cfg, sim_params, physics_engine, sim_device, headless)
        self.privileged_as_observations = bool(getattr(cfg.env, "privileged_as_observations", False))
        if self.privileged_as_observations:
            # (after construction: the buffers and the native step keep the inner widths)
            self.num_policy_obs = self.num_obs
            self.num_obs, self.num_privileged_obs = presented_widths(cfg)

    def get_observations(self):
        return self.privileged_obs_buf if self.privileged_as_observations else self.obs_buf

    def get_privileged_observations(self):
        return None if self.privileged_as_observations else self.privileged_obs_buf

    def step(self, actions):
        obs, priv, rew, reset, extras = super().step(actions)
        if self.privileged_as_observations:
            return priv, None, rew, reset, extras
        return obs, priv, rew, reset, extras
