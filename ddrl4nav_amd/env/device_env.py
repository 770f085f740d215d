"""DeviceEnv: Pong and Catch stepped and rendered on the GPU (csrc/denv.hip).

The reference's env package wraps gym and a ROS simulator on the host; neither exists here, and at the acting rates of this path a host
emulator would need dozens of cores per GPU.  A DeviceEnv turns the device actions act() returns into the next frame, reward and done
without leaving the GPU: one launch per step for all N envs.  The rules are integer-only (tests/device_env_ref.py is the rule book), so
a trajectory is reproducible bit for bit from (game, seed, global env index, actions)."""
import torch

from ddrl4nav_amd import ops
from ddrl4nav_amd.env.device_env_base import DeviceEnvBase
from ddrl4nav_amd.env.device_nav_env import NAV_ENV_NAME, make_device_nav_env
from ddrl4nav_amd.env.fleet_nav_env import FLEET_ENV_NAME, make_fleet_nav_env

ENV_NAMES = {"DevicePong-v0": "pong", "DeviceCatch-v0": "catch"}


class DeviceEnv(DeviceEnvBase):
    _PARAMS = ("game", "n_envs", "seed", "n_actions", "points", "max_steps", "env0")
    _state_ints = staticmethod(ops.env_state_ints)

    def __init__(self, game, n_envs, device=None, seed=0, n_actions=6, points=21, max_steps=10000, env0=0):
        """game: "pong" or "catch".  env0: the global index of local env 0 -- a rank that owns dist.shard_envs' range [a, b) builds
        DeviceEnv(game, b - a, env0=a) and plays exactly the games envs a..b-1 of a single process would.  Pong ends at `points` points
        of either side, every game at `max_steps` steps (a truncation counts as a done)."""
        if game not in ops.ENV_GAMES:
            raise ValueError("game must be one of %s, got %r" % (sorted(ops.ENV_GAMES), game))
        self.game, self.n_actions, self.points, self.max_steps = game, int(n_actions), int(points), int(max_steps)
        if not 2 <= self.n_actions <= 18:
            raise ValueError("n_actions must be in 2..18, got %d" % self.n_actions)
        if self.points < 1 or self.max_steps < 1:
            raise ValueError("points and max_steps must be at least 1, got %d and %d" % (self.points, self.max_steps))
        super().__init__(n_envs, device, seed, env0)
        self.frame = torch.empty((self.N, 84, 84), dtype=torch.uint8, device=self.device)

    def _frame_out(self, frame_out):
        return self.frame if frame_out is None else frame_out

    def reset(self, mask=None, frame_out=None):
        """A new first episode for every env, or for those with a non-zero entry in mask (uint8 [N] on the device); returns the frame
        uint8 [N, 84, 84] (the env's own, or frame_out: any 16-byte-aligned contiguous uint8 [N, 84, 84] device tensor).  A masked-out
        env's rows of the frame are not written."""
        return ops.env_reset(self.game, self.state, self._frame_out(frame_out), env0=self.env0, seed=self.seed, mask=mask)

    def step(self, actions, frame_out=None):
        """actions fp32 [N] on the device (what act() returns) -> (frame uint8 [N, 84, 84], reward fp32 [N], done uint8 [N]): device
        tensors the env owns, valid until the next step (frame_out: render there instead).  A finished env has already begun its next
        episode: the frame is that episode's first and done is the reset flag the frame pools expect.  Asynchronous."""
        return ops.env_step(self.game, self.state, actions, self._frame_out(frame_out), self.reward, self.done, env0=self.env0,
                            n_actions=self.n_actions, points=self.points, max_steps=self.max_steps, seed=self.seed)


def make_device_env(config_env, device=None, env0=0):
    """The DeviceEnv of a config_env dict: env_name "DevicePong-v0" / "DeviceCatch-v0", env_num, and the optional knobs env_seed,
    discrete_actions (its length is n_actions), env_points, env_max_steps; or the DeviceNavEnv of env_name "DeviceNav-v0" with env_num,
    env_seed, env_obstacles, env_peds, env_max_steps (env/device_nav_env.py); or the FleetNavEnv of env_name "DeviceNavFleet-v0", where
    env_num counts the worlds and agent_num_per_env (required) the robots of each, with the same knobs (env/fleet_nav_env.py)."""
    name = config_env.get("env_name")
    if name == NAV_ENV_NAME:
        return make_device_nav_env(config_env, device=device, env0=env0)
    if name == FLEET_ENV_NAME:
        return make_fleet_nav_env(config_env, device=device, env0=env0)
    if name not in ENV_NAMES:
        raise ValueError("env_name must be one of %s, got %r" % (sorted(ENV_NAMES) + [NAV_ENV_NAME, FLEET_ENV_NAME], name))
    if "env_num" not in config_env:
        raise ValueError("config_env needs env_num")
    actions = config_env.get("discrete_actions")
    return DeviceEnv(ENV_NAMES[name], int(config_env["env_num"]), device=device, seed=int(config_env.get("env_seed", 0)),
                     n_actions=len(actions) if actions is not None else 6, points=int(config_env.get("env_points", 21)),
                     max_steps=int(config_env.get("env_max_steps", 10000)), env0=env0)
