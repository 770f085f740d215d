"""FleetNavEnv: several robots per arena, stepped and observed on the GPU (csrc/fleetenv.hip).

The reference's agent runs ``agent_num_per_env`` robots in every env, all_num = agent_num_per_env * batch_num_per_env rows per step, in
[batch, agent] order.  A FleetNavEnv is DeviceNavEnv's arena with R = 1..4 robots in it: they see each other in their lidar and in their
dynamic-agent map and collide with each other (info collision kind 3, the reference's coll_robot_num).  A ROW is one robot -- row
i * R + r is robot r of world i -- and everything downstream of the env (StateRollout, GenericPPO, NavStatus, device_loop) works on rows:
``N`` is the number of rows.  One launch per step for all worlds; the rules are integer-only (tests/fleet_env_ref.py is the rule book)."""
from ddrl4nav_amd import ops
from ddrl4nav_amd.env.device_nav_env import NavArenaEnv, arena_config_kw

FLEET_ENV_NAME = "DeviceNavFleet-v0"


class FleetNavEnv(NavArenaEnv):
    _PARAMS = ("n_worlds", "n_robots", "seed", "n_obstacles", "n_peds", "max_steps", "world0", "ped_model")
    _state_ints = staticmethod(ops.fleet_env_state_ints)

    def __init__(self, n_worlds, n_robots, device=None, seed=0, n_obstacles=10, n_peds=5, max_steps=500, world0=0, emit_info=False,
                 emit_final_obs=False, ped_model="walk"):
        """n_worlds arenas of n_robots 1..4 robots, n_obstacles 0..10 static circles and n_peds 0..5 pedestrians each.  A robot's episode
        ends at a collision (wall, obstacle, pedestrian, another robot), at its goal or after max_steps steps; it alone respawns, the
        world stays.  world0: the global index of local world 0, as DeviceNavEnv's env0.  emit_info: every step also fills ``info``
        (int32 [N], ops.nav_info_fields; agent.NavStatus accumulates it, one status row per robot); the trajectory is the same either
        way.  emit_final_obs (implies emit_info): a step that truncates a robot's episode also renders what that
        robot saw at its end -- every robot where it is after all moves and before any respawn -- into its row of ``final_obs``
        ([laser, vector, image], [N, ...] each; the other rows keep what they held).  ped_model: "walk" or "avoid", as DeviceNavEnv's;
        under "avoid" the pedestrians give way to each other and to every robot."""
        self.n_worlds, self.n_robots, self.world0 = int(n_worlds), int(n_robots), int(world0)
        if self.n_worlds < 1:
            raise ValueError("n_worlds must be at least 1, got %d" % self.n_worlds)
        if self.world0 < 0 or self.world0 + self.n_worlds > 2 ** 32:
            raise ValueError("global world indices world0 .. world0 + n_worlds - 1 must fit 32 bits")
        if not 1 <= self.n_robots <= ops.FLEET_ENV_MAX_ROBOTS:
            raise ValueError("n_robots must be in 1..%d, got %d" % (ops.FLEET_ENV_MAX_ROBOTS, self.n_robots))
        if self.n_worlds * self.n_robots >= 2 ** 31:
            raise ValueError("n_worlds * n_robots must fit int32")
        super().__init__(self.n_worlds, self.n_robots, device, seed, n_obstacles, n_peds, max_steps, self.world0, emit_info,
                         emit_final_obs, ped_model)                      # N = the rows: what device_loop compares with a rollout's N

    def reset(self, mask=None, obs_out=None):
        """A new world for every world, or for those with a non-zero entry in mask (uint8 [n_worlds] on the device: one byte per WORLD);
        returns the observation [laser, vector, image] of all N rows (the env's own tensors, or obs_out: contiguous fp32 device tensors of
        those shapes, laser and image 16-byte aligned).  The rows of a masked-out world are not written."""
        return ops.fleet_env_reset(self.state, self.n_robots, self._obs_out(obs_out), world0=self.world0, mask=mask, **self._arena_kw())

    def step(self, actions, obs_out=None, final_out=None):
        """actions fp32 [N, 2] on the device -> ([laser, vector, image], reward fp32 [N], done uint8 [N]): device tensors the env owns,
        valid until the next step (obs_out: render there instead).  A finished robot has already begun its next episode: its observation
        is that episode's first and done is its reset flag.  With emit_info, ``info`` describes the step just played.  With
        emit_final_obs the truncated rows of ``final_obs`` (final_out: of those tensors instead) receive the observation their episode
        ended in.  Asynchronous."""
        final = self._final_out(final_out)
        args = (self.state, self.n_robots, actions, self._obs_out(obs_out), self.reward, self.done, self.info)
        kw = dict(world0=self.world0, max_steps=self.max_steps, **self._arena_kw())
        if self.ped_model != "walk":
            return ops.fleet_env_step_model(*args, final, ped_model=self.ped_model, **kw)
        if self.emit_final_obs:
            return ops.fleet_env_step_final(*args, final, **kw)
        return ops.fleet_env_step(*args, **kw)


def make_fleet_nav_env(config_env, device=None, env0=0):
    """The FleetNavEnv of a config_env dict: env_name "DeviceNavFleet-v0", env_num (the worlds), agent_num_per_env (the robots of a
    world; required), and the optional knobs of arena_config_kw.  env0: world0."""
    if config_env.get("env_name") != FLEET_ENV_NAME:
        raise ValueError("env_name must be %r, got %r" % (FLEET_ENV_NAME, config_env.get("env_name")))
    for key in ("env_num", "agent_num_per_env"):
        if key not in config_env:
            raise ValueError("config_env needs %s" % key)
    return FleetNavEnv(int(config_env["env_num"]), int(config_env["agent_num_per_env"]), device=device, world0=env0,
                       **arena_config_kw(config_env))
