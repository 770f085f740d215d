"""DeviceNavEnv: 2-D robot navigation stepped and observed on the GPU (csrc/navenv.hip).

The reference's robot_nav task talks to a ROS simulator (img_env) that is not part of its tree.  A DeviceNavEnv stands where it stood:
a differential-drive robot, static circular obstacles and walking pedestrians in a round arena, and the three observation components
NavPreNet1D reads -- laser [1, 960], vector [5], pedestrian map [3, 48, 48], fp32 -- written by one launch per step for all N envs.
The rules are integer-only (tests/nav_env_ref.py is the rule book), so a trajectory is reproducible bit for bit from (seed, global env
index, populations, actions)."""
import torch

from ddrl4nav_amd import ops
from ddrl4nav_amd.env.device_env_base import DeviceEnvBase

NAV_ENV_NAME = "DeviceNav-v0"


def truncations_per_rollout(horizon, max_steps):
    """ceil(horizon / max_steps): an episode lasts max_steps steps at the most, so no env truncates more often in `horizon` steps."""
    horizon, max_steps = int(horizon), int(max_steps)
    if horizon < 1 or max_steps < 1:
        raise ValueError("horizon and max_steps must be at least 1, got %d and %d" % (horizon, max_steps))
    return -(-horizon // max_steps)


class NavArenaEnv(DeviceEnvBase):
    """What DeviceNavEnv and FleetNavEnv (env/fleet_nav_env.py) share: the arena's populations and max_steps with their checks, the
    observation, info and terminal-observation tensors (a row per robot), where a call renders to, the pedestrian model, and the knobs
    of a config_env."""
    state_shapes = [tuple(s) for s in ops.NAV_ENV_SHAPES]

    def __init__(self, n_states, rows_per_state, device, seed, n_obstacles, n_peds, max_steps, index0, emit_info, emit_final_obs,
                 ped_model="walk"):
        """After the subclass's own checks.  emit_final_obs implies emit_info.  ped_model: "walk" or "avoid" (DESIGN.md section 6.16)."""
        self.n_obstacles, self.n_peds, self.max_steps = int(n_obstacles), int(n_peds), int(max_steps)
        if not isinstance(ped_model, str) or ped_model not in ops.NAV_PED_MODELS:
            raise ValueError("ped_model must be one of %r, got %r" % (ops.NAV_PED_MODELS, ped_model))
        self.ped_model = ped_model
        if not 0 <= self.n_obstacles <= 10:
            raise ValueError("n_obstacles must be in 0..10, got %d" % self.n_obstacles)
        if not 0 <= self.n_peds <= 5:
            raise ValueError("n_peds must be in 0..5, got %d" % self.n_peds)
        if self.max_steps < 1:
            raise ValueError("max_steps must be at least 1, got %d" % self.max_steps)
        super().__init__(n_states, device, seed, index0, rows_per_state)
        self.obs = [torch.empty((self.N,) + shape, dtype=torch.float32, device=self.device) for shape in self.state_shapes]
        self.emit_final_obs = bool(emit_final_obs)
        self.emit_info = bool(emit_info) or self.emit_final_obs
        self.info = torch.zeros(self.N, dtype=torch.int32, device=self.device) if self.emit_info else None
        self.final_obs = [torch.zeros_like(o) for o in self.obs] if self.emit_final_obs else None

    def _arena_kw(self):
        return dict(seed=self.seed, n_obstacles=self.n_obstacles, n_peds=self.n_peds)

    def _obs_out(self, obs_out):
        return self.obs if obs_out is None else list(obs_out)

    def _final_out(self, final_out):
        """Where a step renders the terminal observations: the env's own tensors or the caller's; None for an env without them."""
        if final_out is not None and not self.emit_final_obs:
            raise ValueError("final_out needs an env built with emit_final_obs=True")
        return self.final_obs if final_out is None else list(final_out)

    def truncations_per_rollout(self, horizon):
        """The most truncations one row can have in `horizon` steps, ceil(horizon / max_steps): the pool depth with which a
        StateRollout(bootstrap_truncated=...) drops none."""
        return truncations_per_rollout(horizon, self.max_steps)

    def load_state_dict(self, sd):
        """A state_dict saved before there was a choice of pedestrian model is one of "walk"."""
        super().load_state_dict(sd if "ped_model" in sd else dict(sd, ped_model="walk"))


def arena_config_kw(config_env):
    """The optional knobs of a config_env both nav envs read: env_seed, env_obstacles, env_peds, env_max_steps, env_info (emit_info),
    env_final_obs (emit_final_obs), env_ped_model ("walk", the default, or "avoid")."""
    return dict(seed=int(config_env.get("env_seed", 0)), n_obstacles=int(config_env.get("env_obstacles", 10)),
                n_peds=int(config_env.get("env_peds", 5)), max_steps=int(config_env.get("env_max_steps", 500)),
                emit_info=bool(config_env.get("env_info", False)), emit_final_obs=bool(config_env.get("env_final_obs", False)),
                ped_model=config_env.get("env_ped_model", "walk"))


class DeviceNavEnv(NavArenaEnv):
    _PARAMS = ("n_envs", "seed", "n_obstacles", "n_peds", "max_steps", "env0", "ped_model")
    _state_ints = staticmethod(ops.nav_env_state_ints)

    def __init__(self, n_envs, device=None, seed=0, n_obstacles=10, n_peds=5, max_steps=500, env0=0, emit_info=False,
                 emit_final_obs=False, ped_model="walk"):
        """n_obstacles 0..10 static circles, n_peds 0..5 pedestrians; an episode ends at a collision, at the goal or after max_steps
        steps (a truncation counts as a done).  env0: the global index of local env 0, as for DeviceEnv.  emit_info: every step also
        fills ``info`` (int32 [N]: why the step ended or did not, ops.nav_info_fields; agent.NavStatus accumulates it); the trajectory is
        the same either way.  emit_final_obs (implies emit_info): a step that truncates an env's episode also
        renders the observation that episode ended in into row i of ``final_obs`` ([laser, vector, image], [N, ...] each; the rows of
        the other envs keep what they held), for a rollout that bootstraps truncated episodes.  ped_model:
        "walk", pedestrians that walk straight ahead and turn at walls and obstacles only, or "avoid", pedestrians that also give way to
        each other and to the robot; anything else is a ValueError.  With "walk" the env calls the operators it has always called."""
        super().__init__(n_envs, 1, device, seed, n_obstacles, n_peds, max_steps, env0, emit_info, emit_final_obs, ped_model)

    def reset(self, mask=None, obs_out=None):
        """A new first episode for every env, or for those with a non-zero entry in mask (uint8 [N] on the device); returns the
        observation [laser, vector, image] (the env's own tensors, or obs_out: contiguous fp32 device tensors of those shapes, laser and
        image 16-byte aligned -- the rows of a StateRollout's pools are).  A masked-out env's rows are not written."""
        return ops.nav_env_reset(self.state, self._obs_out(obs_out), env0=self.env0, mask=mask, **self._arena_kw())

    def step(self, actions, obs_out=None, final_out=None):
        """actions fp32 [N, 2] on the device (what a Gaussian actor's act() returns) -> ([laser, vector, image], reward fp32 [N], done
        uint8 [N]): device tensors the env owns, valid until the next step (obs_out: render there instead).  A finished env has already
        begun its next episode: the observation is that episode's first and done is the reset flag.  With emit_info, ``info`` describes the
        step just played (the finished episode's last, not the new one's first).  With emit_final_obs the truncated envs' rows of
        ``final_obs`` (final_out: of those tensors instead) receive the observation their episode ended in.  Asynchronous."""
        final = self._final_out(final_out)
        args = (self.state, actions, self._obs_out(obs_out), self.reward, self.done)
        kw = dict(env0=self.env0, max_steps=self.max_steps, **self._arena_kw())
        if self.ped_model != "walk":
            return ops.nav_env_step_model(*args, self.info, final, ped_model=self.ped_model, **kw)
        if self.emit_final_obs:
            return ops.nav_env_step_final(*args, self.info, final, **kw)[:3]
        if self.emit_info:
            return ops.nav_env_step_info(*args, self.info, **kw)[:3]
        return ops.nav_env_step(*args, **kw)


def make_device_nav_env(config_env, device=None, env0=0):
    """The DeviceNavEnv of a config_env dict: env_name "DeviceNav-v0", env_num, and the optional knobs of arena_config_kw."""
    if config_env.get("env_name") != NAV_ENV_NAME:
        raise ValueError("env_name must be %r, got %r" % (NAV_ENV_NAME, config_env.get("env_name")))
    if "env_num" not in config_env:
        raise ValueError("config_env needs env_num")
    return DeviceNavEnv(int(config_env["env_num"]), device=device, env0=env0, **arena_config_kw(config_env))
