"""The closed loop on one GPU: a DeviceRollout / PlaneRollout driven by a DeviceEnv (env/device_env.py), or a StateRollout driven by a
DeviceNavEnv (env/device_nav_env.py) or a FleetNavEnv (env/fleet_nav_env.py; collect_states / train_states), then net.learn on its
batch.

Every tensor that moves between acting, the env and the pools is a device tensor and every call is asynchronous on the current stream:
a rollout adds no host synchronisation to what act(), record() and the puts do already (none, for device arguments).  On a PlaneRollout
the env renders straight into the pool row the frame belongs to (PlaneRollout.new_frame_row), so the put copies nothing; on a
StateRollout it renders into StateRollout.state_rows.

There is one loop (_collect) and one generator (_train).  A frame rollout and a state rollout differ in where the env renders, how a
slot is put and how the (T + 1)-th step is drawn: _frame_io / _state_io say that, as five values."""


def _frame_io(ro, env, keep_step):
    """(render, put, put_own, bootstrap, info) of a DeviceRollout / PlaneRollout on a DeviceEnv.  render(t): where the env renders slot t
    -- the plane pool's own row, or None (the env's buffer, which the put copies)."""
    row = ro.new_frame_row if hasattr(ro, "new_frame_row") else (lambda t: None)
    return (lambda t: {"frame_out": row(t)}, ro.put_new_frames, lambda t: ro.put_new_frames(t, env.frame), ro.bootstrap, {})


def _state_io(ro, env, keep_step):
    """The same of a StateRollout on a DeviceNavEnv: the env renders into the pool rows, so the put copies nothing."""
    tracks = getattr(ro, "nav_status", None) is not None
    boots = getattr(ro, "S", 0) > 0
    if tracks and getattr(env, "info", None) is None:
        raise ValueError("the rollout tracks the navigation status but the env was built without emit_info")
    if boots and getattr(env, "final_obs", None) is None:
        raise ValueError("the rollout bootstraps truncated episodes but the env was built without emit_final_obs")
    if boots and keep_step:
        raise ValueError("keep_step is not supported with bootstrap_truncated: the terminal observation of row T would have to move "
                         "between rollouts")
    info = {"info": env.info} if tracks or boots else {}
    if boots:
        info["final_obs"] = env.final_obs
    return (lambda t: {"obs_out": ro.state_rows(t)}, lambda t, obs, reset=None: ro.put_states_in_place(t),
            lambda t: ro.put_states(t, env.obs), lambda: ro.bootstrap(sample=keep_step), info)


def _collect(ro, env, keep_step, reset, io):
    if env.N != ro.N:
        raise ValueError("the env has %d envs, the rollout %d" % (env.N, ro.N))
    render, put, put_own, bootstrap, info = io(ro, env, keep_step)
    T = ro.T
    if reset is None:
        reset = ro.rollouts == 0 and ro.t0 == 0
    if reset:
        if ro.t0 != 0:
            raise ValueError("a rollout that carried a whole step over cannot restart its env")
        put(0, env.reset(**render(0)), reset=True)
    elif ro.t0 == 1:
        # the kept step's action was played at the end of the previous rollout: the env's own buffer is the observation of slot 1
        put_own(1)
    for t in range(ro.t0, T):
        obs, reward, done = env.step(ro.act(t), **render(t + 1))
        ro.record(t, reward, done, **info)
        put(t + 1, obs)
    action = bootstrap()
    if keep_step:
        _, reward, done = env.step(action)
        ro.record(T, reward, done, **info)
    ro.finish()


def _train(collect_one, net, env, ro, updates, keep_step):
    for _ in range(int(updates)):
        collect_one(ro, env, keep_step=keep_step)
        losses = None
        for item in net.learn(ro.batch()):
            losses = item[0]
        yield losses, (ro.returns.mean_return() if ro.returns is not None else None)
        ro.carry_over(keep_step=keep_step)


def collect(ro, env, keep_step=False, reset=None):
    """One rollout of `ro` on `env`: act(t) -> env.step -> record(t, reward, done) -> put_new_frames(t + 1, frame) for t = t0 .. T - 1,
    then bootstrap() and finish().

    reset (None: True for ro's first rollout, ro.rollouts == 0 with nothing carried over): the env is reset and its first frame put as
    slot 0.  Otherwise slot 0 is what carry_over() left there.
    keep_step: the caller will close this rollout with carry_over(keep_step=True) -- the bootstrap action is then sent to the env as
    well and its reward and done recorded in row T; the frame it produced stays in env.frame and becomes slot 1 of the next rollout,
    which starts at ro.t0 == 1 with the kept action already played."""
    _collect(ro, env, keep_step, reset, _frame_io)


def train(net, env, ro, updates, keep_step=False):
    """A generator over `updates` PPO updates: collect(ro, env), net.learn(ro.batch()), carry_over(keep_step).  Yields, per update,
    (the last loss dict of net.learn, ro.returns.mean_return() -- None without track_returns)."""
    return _train(collect, net, env, ro, updates, keep_step)


def collect_states(ro, env, keep_step=False, reset=None):
    """collect() for a StateRollout `ro` and an env whose observation is a list of fp32 components (DeviceNavEnv; or a FleetNavEnv, whose
    rows are robots: build the rollout with n_envs = env.N = n_worlds * n_robots): act(t) ->
    env.step(obs_out=ro.state_rows(t + 1)) -> record(t, reward, done) -> put_states_in_place(t + 1) for t = t0 .. T - 1, then
    bootstrap() and finish().  The env renders into the pool rows, so no observation is copied.

    reset (None: True for ro's first rollout, ro.rollouts == 0 with nothing carried over): the env is reset into slot 0.  Otherwise
    slot 0 is what carry_over() left there.
    keep_step: as for collect() -- bootstrap(sample=True) draws the (T + 1)-th action, the env plays it into its own tensors and its
    reward and done are recorded in row T; the next rollout starts at ro.t0 == 1 and copies that observation into slot 1.

    A rollout built with track_nav_status=True also records env.info, the info words of every step: the env must have been built with
    emit_info=True (ValueError otherwise).  A rollout built with bootstrap_truncated=S also records env.info and env.final_obs, the
    terminal observations of truncated episodes: the env must have been built with emit_final_obs=True, and keep_step is refused
    (ValueError either way)."""
    _collect(ro, env, keep_step, reset, _state_io)


def train_states(net, env, ro, updates, keep_step=False):
    """train() for a StateRollout: collect_states(ro, env), net.learn(ro.batch()), carry_over(keep_step).  Yields, per update, (the last
    loss dict of net.learn, ro.returns.mean_return() -- None without track_returns).  The navigation status of a tracking rollout is read
    from ro.nav_status (summary() is its one device-to-host copy; on a FleetNavEnv other_robot_collision_rate() is one more)."""
    return _train(collect_states, net, env, ro, updates, keep_step)
